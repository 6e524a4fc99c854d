"""Sequential reference of the training augmentation (mvp/augment.py, csrc/augment.hip), for the tests: every stage materialises its
image exactly as the reference's host pipeline does (get_nyu_transforms, evals/datasets/utils.py:160-218, nyu.py:227-239) — ColorJitter on
the full image with torchvision's float-tensor formulas, then flip, rotate and resized crop one after the other, each nearest-neighbour,
then Normalize.  Everything is evaluated in ``dtype``: float64 is the reference, float32 is the "fp32 torch restatement of the same
formulas" whose own error against float64 sets the kernel tests' tolerance.  Parameters come from mvp.augment.unpack_params."""
import torch

from mvp import augment

TIE_MARGIN = 1e-3  # pixels: a source coordinate this close to a rounding tie may legitimately round either way in fp32


def to_unit(image: torch.Tensor, dtype) -> torch.Tensor:
    """uint8 [H, W, 3] or float [3, H, W] -> [3, H, W] in [0, 1]."""
    if image.dtype == torch.uint8:
        return image.permute(2, 0, 1).to(dtype) / 255
    return image.to(dtype)


def _grey(img):
    return 0.2989 * img[0] + 0.587 * img[1] + 0.114 * img[2]


def _blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0, 1)


def _rgb2hsv(img):
    r, g, b = img.unbind(0)
    maxc, minc = img.max(0).values, img.min(0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc))


def _hsv2rgb(img):
    h, s, v = img.unbind(0)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * f)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    mask = i.unsqueeze(0) == torch.arange(6).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v))
    a2 = torch.stack((t, v, v, q, p, p))
    a3 = torch.stack((p, p, t, v, v, q))
    a4 = torch.stack((a1, a2, a3))
    return torch.einsum("ijk,xijk->xjk", mask.to(img.dtype), a4)


def jitter(img: torch.Tensor, e) -> torch.Tensor:
    """torchvision ColorJitter's four operations on a float [3, H, W] image in [0, 1], in the entry's order."""
    if not e["jitter"]:
        return img
    for op in e["order"]:
        if op == 0:
            img = (e["brightness"] * img).clamp(0, 1)
        elif op == 1:
            img = _blend(img, _grey(img).mean(), e["contrast"])
        elif op == 2:
            img = _blend(img, _grey(img).unsqueeze(0), e["saturation"])
        else:
            hsv = _rgb2hsv(img)
            hsv = torch.stack((torch.remainder(hsv[0] + e["hue"], 1.0), hsv[1], hsv[2]))
            img = _hsv2rgb(hsv)
    return img


def contrast_mean(img: torch.Tensor, e) -> float:
    """The mean grey value the contrast operation of entry ``e`` uses on the float [3, H, W] image (the operations before it applied)."""
    for op in e["order"]:
        if op == 1:
            return float(_grey(img).mean())
        img = jitter(img, dict(e, jitter=True, order=(op,)))
    raise AssertionError("no contrast operation")


def _reflect101(i, n):
    period = 2 * (n - 1)
    m = torch.remainder(i, period)
    return torch.where(m > n - 1, period - m, m)


def rotate(planes: torch.Tensor, cos: float, sin: float):
    """Nearest-neighbour rotation of [C, H, W] about ((W-1)/2, (H-1)/2), fp64 inverse map, reflect-101 border ->
    (rotated planes, [H, W] bool: the source coordinate is within TIE_MARGIN of a rounding tie in x or y)."""
    C, H, W = planes.shape
    y = torch.arange(H, dtype=torch.float64).view(H, 1).expand(H, W)
    x = torch.arange(W, dtype=torch.float64).view(1, W).expand(H, W)
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    u, v = x - cx, y - cy
    fx = cx + cos * u - sin * v + 0.5
    fy = cy + sin * u + cos * v + 0.5
    tie = ((fx - torch.round(fx)).abs() < TIE_MARGIN) | ((fy - torch.round(fy)).abs() < TIE_MARGIN)
    sx = _reflect101(torch.floor(fx).to(torch.int64), W)
    sy = _reflect101(torch.floor(fy).to(torch.int64), H)
    return planes[:, sy, sx], tie


def crop_resize(planes: torch.Tensor, box, out_hw) -> torch.Tensor:
    """Crop [C, H, W] to the box and resize it to out_hw, nearest without half-pixel offset (OpenCV INTER_NEAREST)."""
    x0, y0, cw, ch = box
    Ho, Wo = out_hw
    crop = planes[:, y0:y0 + ch, x0:x0 + cw]
    sy = (torch.arange(Ho) * ch) // Ho
    sx = (torch.arange(Wo) * cw) // Wo
    return crop[:, sy][:, :, sx]


def geometry(planes: torch.Tensor, e, out_hw):
    """flip -> rotate -> resized crop of [C, H, W], one stage after the other -> (planes [C, Ho, Wo], tie mask [Ho, Wo])."""
    H, W = planes.shape[-2:]
    tie = torch.zeros(H, W, dtype=torch.bool)
    if e["flip"]:
        planes = planes.flip(-1)
    if e["rotate"]:
        planes, tie = rotate(planes, e["cos"], e["sin"])
    planes = crop_resize(planes, e["box"], out_hw)
    tie = crop_resize(tie.unsqueeze(0), e["box"], out_hw)[0]
    return planes, tie


def apply(image, depth, snorm, params, out_hw, image_mean, dtype=torch.float64):
    """The whole stage on host tensors: image uint8 [B, H, W, 3] or float [B, 3, H, W], depth [B, 1, H, W], snorm [B, 3, H, W] or None ->
    (image [B, 3, Ho, Wo] in ``dtype``, depth, snorm (their own dtype), tie mask [B, Ho, Wo])."""
    mean, std = augment.mean_std(image_mean)
    mean, std = torch.tensor(mean, dtype=dtype).view(3, 1, 1), torch.tensor(std, dtype=dtype).view(3, 1, 1)
    imgs, deps, sns, ties = [], [], [], []
    for b, e in enumerate(augment.unpack_params(params)):
        img = jitter(to_unit(image[b], dtype), e)
        img, tie = geometry(img, e, out_hw)
        imgs.append((img - mean) / std)
        deps.append(geometry(depth[b], e, out_hw)[0])
        if snorm is not None:
            sns.append(geometry(snorm[b], e, out_hw)[0])
        ties.append(tie)
    return torch.stack(imgs), torch.stack(deps), (torch.stack(sns) if snorm is not None else None), torch.stack(ties)


def source_index(params, H, W, out_hw):
    """([B, Ho, Wo] int64 linear source index yy * W + xx of the sequential pipeline, tie mask): the pipeline run on an index plane."""
    idx = torch.arange(H * W, dtype=torch.int64).view(1, H, W)
    out, ties = [], []
    for e in augment.unpack_params(params):
        g, tie = geometry(idx, e, out_hw)
        out.append(g[0])
        ties.append(tie)
    return torch.stack(out), torch.stack(ties)
