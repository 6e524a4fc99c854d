"""Working package init (the reference's evals/models/__init__.py:1-7 re-exports names that
no longer exist and raises ImportError; hydra only needs the sub-modules to be importable)."""
from . import probes  # noqa: F401
from .beit_v2 import BEiTV2  # noqa: F401
from .clip import CLIP  # noqa: F401
from .convnext import ConvNext  # noqa: F401
from .croco import CROCO  # noqa: F401
from .crocov2 import CROCOV2  # noqa: F401
from .dino import DINO  # noqa: F401
from .ibot import iBOT  # noqa: F401
from .mae import MAE  # noqa: F401
from .mocov3 import MoCoV3  # noqa: F401
from .pixel_metrics import PSNR, SSIM  # noqa: F401
from .sam import SAM  # noqa: F401
from .siglip import SigLIP  # noqa: F401
from . import ssl_resnet50 as _ssl  # noqa: E402

_ssl.register(__name__)  # evals.models.{barlowtwins, byol, ..., swav}: one table, fourteen importable sub-modules
