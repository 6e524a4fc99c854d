"""fp64 restatement of the objectness probe's tail, written from the formulas (numpy only, no torch.nn):

  bn_act_fwd / bn_act_bwd   nn.BatchNorm2d (eps 1e-5, momentum 0.1, biased variance to normalise, unbiased into running_var) + sigmoid,
                            or plain tanh / identity, and the backward of each
  bce / bce_grad            nn.BCELoss (mean) with torch's -100 clamp of both log terms, and (p - t) / max(p (1 - p), 1e-12) / N
  counts / metrics          TP FP FN TN of pred > threshold, and the reference's mask metrics on them

The kernels (tests/test_gpu_objectness_kernels.py) and the reference's recorded fp32 results (tests/test_objectness_cpu.py) are both
held to this."""
import numpy as np


def sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def bn_act_fwd(x, gamma=None, beta=None, running_mean=None, running_var=None, act="sigmoid", training=True, n=None, eps=1e-5, momentum=0.1):
    """x [B, C, H, W] -> dict(y, mean, rstd, xhat, running_mean, running_var): the running statistics AFTER the call (unchanged in eval
    mode).  ``n``: the count of the unbiased correction (default: B*H*W)."""
    x = np.asarray(x, dtype=np.float64)
    if act == "tanh":
        return dict(y=np.tanh(x))
    if act == "none":
        return dict(y=x.copy())
    B, C, H, W = x.shape
    P = B * H * W
    n = P if n is None else n
    rm = None if running_mean is None else np.asarray(running_mean, dtype=np.float64)
    rv = None if running_var is None else np.asarray(running_var, dtype=np.float64)
    if training:
        mean = x.mean(axis=(0, 2, 3))
        var = ((x - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
        if rm is not None:
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    else:
        mean, var = rm, rv
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean[None, :, None, None]) * rstd[None, :, None, None]
    z = xhat * np.asarray(gamma, dtype=np.float64)[None, :, None, None] + np.asarray(beta, dtype=np.float64)[None, :, None, None]
    return dict(y=sigmoid(z), mean=mean, rstd=rstd, xhat=xhat, running_mean=rm, running_var=rv)


def bn_act_bwd(x, grad_y, gamma=None, beta=None, running_mean=None, running_var=None, act="sigmoid", training=True, eps=1e-5):
    """-> dict(grad_x [B, C, H, W], grad_gamma, grad_beta)."""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(grad_y, dtype=np.float64)
    if act == "tanh":
        return dict(grad_x=gy * (1.0 - np.tanh(x) ** 2))
    if act == "none":
        return dict(grad_x=gy.copy())
    f = bn_act_fwd(x, gamma, beta, running_mean, running_var, act, training, eps=eps)
    y, xhat, rstd = f["y"], f["xhat"], f["rstd"]
    gz = gy * y * (1.0 - y)
    db = gz.sum(axis=(0, 2, 3))
    dg = (gz * xhat).sum(axis=(0, 2, 3))
    P = x.shape[0] * x.shape[2] * x.shape[3]
    a = (np.asarray(gamma, dtype=np.float64) * rstd)[None, :, None, None]
    if training:
        gx = a * (gz - db[None, :, None, None] / P - xhat * dg[None, :, None, None] / P)
    else:
        gx = a * gz
    return dict(grad_x=gx, grad_gamma=dg, grad_beta=db)


def bce(p, t):
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    with np.errstate(divide="ignore"):
        lp = np.maximum(np.log(p), -100.0)
        lq = np.maximum(np.log1p(-p), -100.0)
    return float(np.mean(-(t * lp + (1.0 - t) * lq)))


def bce_grad(p, t):
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    return (p - t) / np.maximum(p * (1.0 - p), 1e-12) / p.size


def counts(pred, gt, threshold=0.5):
    """pred, gt [G, n] -> int64 [G, 4] = TP, FP, FN, TN with pred > threshold strictly."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    pos = pred > threshold
    return np.stack([(pos & (gt == 1)).sum(-1), (pos & (gt == 0)).sum(-1), (~pos & (gt == 1)).sum(-1), (~pos & (gt == 0)).sum(-1)], axis=-1).astype(np.int64)


def metrics(tp, fp, fn, tn, beta=0.3, threshold=0.5):
    """train_generic_objectness.py:56-183 on the four counts, in Python floats."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    precision = tp / (tp + fp + 1e-6)
    recall = tp / (tp + fn + 1e-6)
    f = (1 + beta**2) * (precision * recall) / (beta**2 * precision + recall + 1e-6)
    iou = tp / (tp + fp + fn + 1e-6)
    return {"Precision": precision, "Recall": recall, "F-measure": f, "IoU": iou, "Accuracy": (tp + tn) / (tp + fp + fn + tn),
            "CorLoc": 1 if iou >= threshold else 0}
