"""Input side of the hot path: batch-dict contract + loader construction of the reference
(evals/datasets/builder.py:39-67, nyu.py:245-251).  Real dataset decoders (NYU .mat, the Hugging Face Taskonomy reader, NAVI) are out of scope; Taskonomy's per-sample transforms and its dataset wrapper are in transforms.py / taskonomy.py."""
from .builder import build_loader  # noqa: F401
from .synthetic import SyntheticNYU, SyntheticNYURaw  # noqa: F401
