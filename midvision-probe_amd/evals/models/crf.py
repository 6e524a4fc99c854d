"""evals/models/crf.py of the reference, on the HIP path: ``densecrf(image, mask)`` with the reference's name and signature.  The CRF
is the model pydensecrf is configured with there (include/mvp_hip.h, "Dense CRF"), its message passing evaluated exactly on the device
(mvp/densecrf.py) instead of approximately on a permutohedral lattice (MaskCut deviations)."""
import numpy as np
import torch

from mvp import densecrf as _crf
from mvp import functional as MF
from mvp import lib

MAX_ITER = _crf.MAX_ITER
POS_W, POS_XY_STD = _crf.POS_W, _crf.POS_XY_STD
Bi_W, Bi_XY_STD, Bi_RGB_STD = _crf.BI_W, _crf.BI_XY_STD, _crf.BI_RGB_STD


def densecrf(image, mask):
    """image [H, W, 3] uint8 array, mask [h, w] array of 0 / 1 -> MAP [H, W] float32 array.  The two logit planes (1 - mask, mask) are
    resized bilinearly to H x W when the sizes differ, as the reference does (bilinear weights sum to one, so the background plane is one
    minus the resized foreground plane).  Tensors are taken too, but only device tensors: there is no CPU path."""
    for name, t in (("image", image), ("mask", mask)):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise lib.MvpError(f"densecrf: {name} is a CPU tensor; the HIP path takes arrays or device tensors (there is no CPU fallback)")
    if not torch.cuda.is_available():
        raise lib.MvpError("densecrf: no HIP device (there is no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image)).to(dev)
    m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev)
    if img.dim() != 3 or img.shape[-1] != 3 or img.dtype != torch.uint8 or m.dim() != 2:
        raise ValueError(f"densecrf: image must be [H, W, 3] uint8 and mask [h, w], got {tuple(img.shape)} {img.dtype} and {tuple(m.shape)}")
    H, W = img.shape[:2]
    plane = m.float().view(1, 1, *m.shape)
    if tuple(m.shape) != (H, W):
        plane = MF.interpolate(plane, size=(H, W), mode="bilinear")
    buf = _crf.mean_field(img.view(1, H, W, 3), plane.contiguous(), None, MAX_ITER)
    return buf.map.view(H, W).float().cpu().numpy()
