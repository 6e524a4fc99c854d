"""The four MaskCut launches (csrc/maskcut.hip), each against the fp64 oracle of tests/maskcut_ref.py on the same inputs.

Fixtures (maskcut_ref.FIXTURES; features = prototype[label] + noise + a smooth ramp, seeded):
  5x7    C 24   N = 35: not a multiple of 32 or of the wave, one partial word per row
  9x13   C 40   h != w, two passes (painting, the rejection rule's inputs), gap lambda_2 - lambda_3 = 0.13
  16x16  C 64   N a multiple of 32
  32x32  C 64   N = 1024, the LDS limit; two passes; the smallest gap of the converging fixtures (~0.06)
  30x30  C 768  the evaluation's own shape, once
  8x8    C 32   cleanly separated components, lambda_2 ~ lambda_3 (gap ~ 2e-5): the fallback case

Contracts.
  affinity   max |A - A64| <= AFF_TOL = 4 * max(measured, 2.4e-5); measured on an MI355X over these fixtures: 1.43e-6 (AFF_MEASURED,
             at C = 768; 2.4e-7 to 3.9e-7 at C <= 64: the fp32 fma chain of the fp32-input MFMA), so AFF_TOL = 9.6e-5.
  tau        within AFF_TOL of the oracle's.
  bits       equal to the oracle's except where |A64 - tau| <= 2 AFF_TOL (skipped; at most 0.1 % of an image's entries).
  d          exact on rows without a skipped entry.
  fiedler    reported lambda / residual = the fp64 re-derivation from the written v (1e-10); converged within the cap on every
             fixture but 8x8; bipartition equal to the oracle's on every cell with |v_i - mean| > 4 (R_TOL / gap) max |v| (at most 2 %
             skipped); |lambda - oracle| <= R_TOL^2 / gap + 1e-6.
  partition  masks, painting, union and seed exact."""
import functools

import numpy as np
import pytest
import torch

import maskcut_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AFF_MEASURED = 1.43e-6
AFF_TOL = 4 * max(AFF_MEASURED, 2.4e-5)
NAMES = list(ref.FIXTURES)


@functools.lru_cache(maxsize=None)
def oracle(name):
    f, lab, h, w, P = ref.fixture(name)
    return f, h, w, P, ref.maskcut(f, h, w, P)


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def device_affinity(feats, painted, active):
    """feats [B, C, N] fp32, painted [B, N] 0 / 1, active [B] -> (A, sums, tau, bits, deg, rounds) on the host; the outputs of inactive
    images keep their sentinels."""
    from mvp import ops

    B, C, N = feats.shape
    NW = (N + 31) // 32
    A = torch.full((B, N, N), -7.0, dtype=torch.float32, device=DEV)
    sums = torch.full((B, 2), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(max(1, ops.ncut_workspace_bytes(B, N) // 8), dtype=torch.float64, device=DEV)
    act = dev(active, torch.uint8)
    ops.ncut_affinity(dev(feats, torch.float32), A, sums, ws, B, C, N, painted=dev(painted, torch.uint8), active=act)
    tau = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    bits = torch.full((B, N, NW), -7, dtype=torch.int32, device=DEV)
    deg = torch.full((B, N), -7.0, dtype=torch.float64, device=DEV)
    rounds = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ops.ncut_threshold(A, sums, tau, bits, deg, B, N, 64, rounds=rounds, active=act)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (A, sums, tau, bits, deg, rounds))


@pytest.mark.parametrize("name", NAMES)
def test_affinity_and_threshold(name):
    """Batch of three: the fixture as it is, the fixture with the first pass's mask painted out, and an inactive image."""
    f, h, w, P, out = oracle(name)
    N = h * w
    painted1 = out["passes"][0]["mask"].reshape(-1).astype(np.uint8)
    feats = np.stack([f, f, f])
    painted = np.stack([np.zeros(N, np.uint8), painted1, np.zeros(N, np.uint8)])
    A, sums, tau, bits, deg, rounds = device_affinity(feats, painted, [1, 1, 0])
    assert (A[2] == -7.0).all() and (sums[2] == -7.0).all() and tau[2] == -7.0 and (bits[2] == -7).all() and (deg[2] == -7.0).all()
    for b in range(2):
        A64 = ref.affinity(f, painted[b])
        err = float(np.abs(A[b].astype(np.float64) - A64).max())
        t64, r64 = ref.lloyd_tau(A64)
        B64, d64 = ref.threshold(A64, t64)
        near = np.abs(A64 - t64) <= 2 * AFF_TOL
        got = ref.unpack_bits(bits[b], N)
        print(f"{name}[{b}]: max|A - A64| = {err:.3e}  |tau - tau64| = {abs(tau[b] - t64):.3e}  rounds {rounds[b]} / {r64}  "
              f"skipped {int(near.sum())} of {near.size}  sum err {abs(sums[b, 0] - A64.sum()):.3e}")
        assert err <= AFF_TOL
        assert np.array_equal(A[b], A[b].T)  # the fma chains of (i, j) and (j, i) are the same
        assert abs(sums[b, 0] - A[b].astype(np.float64).sum()) <= 1e-9 * N * N
        assert abs(sums[b, 1] - (A[b].astype(np.float64) ** 2).sum()) <= 1e-9 * N * N
        assert abs(tau[b] - t64) <= AFF_TOL
        assert near.mean() <= 1e-3
        assert np.array_equal(got[~near], B64[~near])
        pad = ref.unpack_bits(bits[b], ((N + 31) // 32) * 32)[:, N:]
        assert not pad.any()  # the bits beyond column N - 1
        cnt = got.sum(axis=1)
        assert np.array_equal(deg[b], cnt + 1e-5 * (N - cnt))  # from its own integer counts, exactly
        clean = ~near.any(axis=1)
        assert np.array_equal(deg[b][clean], d64[clean])


def device_fiedler(Bs, ds, active=None, max_iters=1000):
    from mvp import maskcut, ops

    n = len(Bs)
    N = Bs[0].shape[0]
    bits = dev(np.stack([ref.pack_bits(B).view(np.int32) for B in Bs]), torch.int32)  # (the same 32 bits)
    deg = dev(np.stack(ds), torch.float64)
    v = torch.full((n, N), -7.0, dtype=torch.float32, device=DEV)
    lam = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    res = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    iters = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    conv = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    act = None if active is None else dev(active, torch.uint8)
    ops.ncut_fiedler(bits, deg, v, lam, res, iters, conv, n, N, max_iters, maskcut.R_TOL, maskcut.MIX_TOL, active=act)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (v, lam, res, iters, conv))


@pytest.mark.parametrize("name", NAMES)
def test_fiedler(name):
    """One image per pass of the fixture (bits and degrees from the oracle) plus an inactive copy."""
    from mvp import maskcut

    f, h, w, P, out = oracle(name)
    passes = out["passes"]
    Bs = [ps["B"] for ps in passes] + [passes[0]["B"]]
    ds = [ps["d"] for ps in passes] + [passes[0]["d"]]
    v, lam, res, iters, conv = device_fiedler(Bs, ds, active=[1] * len(passes) + [0])
    assert (v[-1] == -7.0).all() and lam[-1] == -7.0 and iters[-1] == -7 and conv[-1] == 9
    for k, ps in enumerate(passes):
        lam_re, res_re = ref.residual(ps["B"], ps["d"], v[k])
        gap = ps["gap"]
        vo = ps["v"]
        margin = 4 * (maskcut.R_TOL / gap) * np.abs(vo).max()
        keep = np.abs(vo - vo.mean()) > margin
        same = ref.bipartition(v[k]) == ref.bipartition(vo)
        print(f"{name} pass {k}: iters {iters[k]} converged {conv[k]} residual {res[k]:.3e} (re-derived {res_re:.3e}) lambda {lam[k]:.9f} "
              f"(oracle {ps['lam']:.9f}) gap {gap:.3e} skipped {int((~keep).sum())} of {keep.size} differing {int((~same & keep).sum())}")
        assert abs(res[k] - res_re) <= 1e-10 and abs(lam[k] - lam_re) <= 1e-10
        k_lead = int(np.argmax(np.abs(v[k])))
        assert v[k][k_lead] > 0  # the sign convention
        assert abs(np.linalg.norm(np.sqrt(ps["d"]) * v[k]) - 1.0) <= 1e-5
        if name == "8x8":
            continue  # lambda_2 ~ lambda_3: the device may converge or not (tests/test_gpu_maskcut.py holds the final masks)
        assert conv[k] == 1 and 0 < iters[k] < 1000
        assert res[k] <= maskcut.R_TOL
        assert (~keep).mean() <= 0.02
        assert same[keep].all()
        assert abs(lam[k] - ps["lam"]) <= maskcut.R_TOL ** 2 / gap + 1e-6


def test_fiedler_cap_reports_not_converged():
    """Two rounds cannot reach the tolerance: the byte is clear, the outputs are still the re-derivable ones."""
    f, h, w, P, out = oracle("9x13")
    ps = out["passes"][0]
    v, lam, res, iters, conv = device_fiedler([ps["B"]], [ps["d"]], max_iters=2)
    lam_re, res_re = ref.residual(ps["B"], ps["d"], v[0])
    assert conv[0] == 0 and iters[0] == 2
    assert abs(res[0] - res_re) <= 1e-10 and abs(lam[0] - lam_re) <= 1e-10


def device_partition(vs, h, w, painted, prev, use_prev, active=None):
    from mvp import ops

    n, N = len(vs), h * w
    v = dev(np.stack(vs), torch.float32)
    mask = dev(np.stack(prev), torch.uint8) if prev is not None else torch.zeros(n, N, dtype=torch.uint8, device=DEV)
    pt = dev(np.stack(painted), torch.uint8)
    un = torch.full((n, N), 9, dtype=torch.uint8, device=DEV)
    seed = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    act = None if active is None else dev(active, torch.uint8)
    ops.ncut_partition(v, mask, pt, un, seed, n, h, w, prev_mask=mask if use_prev else None, use_prev=use_prev, active=act)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (mask, pt, un, seed))


def check_partition(vs, h, w, painted, prev, use_prev):
    N = h * w
    vs = [np.asarray(v, dtype=np.float32) for v in vs]
    mask, pt, un, seed = device_partition(vs, h, w, painted, prev, use_prev)
    outs = []
    for k, v in enumerate(vs):
        o = ref.partition(v.astype(np.float64), h, w, painted[k], prev[k] if prev is not None else None, use_prev)
        assert np.array_equal(mask[k].reshape(h, w).astype(bool), o["mask"]), k
        assert np.array_equal(pt[k].reshape(h, w).astype(bool), o["painted"]), k
        assert np.array_equal(un[k].reshape(h, w).astype(bool), o["union"]), k
        assert seed[k] == o["seed"], k
        outs.append(o)
    return outs


@pytest.mark.parametrize("name", NAMES)
def test_partition_on_the_oracle_eigenvectors(name):
    f, h, w, P, out = oracle(name)
    N = h * w
    painted = np.zeros(N, np.uint8)
    prev = np.zeros(N, np.uint8)
    for k, ps in enumerate(out["passes"]):
        o = check_partition([ps["v"]], h, w, [painted], [prev], use_prev=k >= 1)[0]
        assert np.array_equal(o["mask"], ps["mask"])  # (fp32 rounding of v moves no cell across the mean)
        painted, prev = o["painted"].reshape(-1).astype(np.uint8), o["mask"].reshape(-1).astype(np.uint8)


def blob(h, w, y0, y1, x0, x1, hi=1.0, lo=-0.2):
    """v with a plateau (the peak at its first cell) on a negative background; distinct values, so no arg-extremum ties"""
    v = np.full((h, w), lo) - 1e-3 * np.arange(h * w).reshape(h, w) / (h * w)
    v[y0:y1, x0:x1] = hi - 1e-3 * np.arange((y1 - y0) * (x1 - x0)).reshape(y1 - y0, x1 - x0) / (h * w)
    return v.reshape(-1)


def test_partition_line_grids():
    for h, w in ((1, 37), (37, 1)):
        v = blob(h, w, 0, h, 0, w, hi=-0.2)  # background everywhere ...
        v[10:20] = 1.0 - 1e-3 * np.arange(10)  # ... with one run
        v[25:28] = 0.9
        o = check_partition([v], h, w, [np.zeros(h * w, np.uint8)], None, False)[0]
        assert o["mask"].sum() == 10 and o["nc"] == 0
        v2 = -v  # both ends foreground: each is counted twice (four corner reads on two cells) -> reversed
        o = check_partition([v2], h, w, [np.zeros(h * w, np.uint8)], None, False)[0]
        assert o["nc"] == 4 and o["reverse"] and o["mask"].sum() == 10


def test_partition_three_foreground_corners_reverse():
    h, w = 7, 9
    v = blob(h, w, 2, 5, 3, 6, hi=-1.0, lo=0.3)  # the background is the high side and holds all four corners
    v.reshape(h, w)[h - 1, w - 1] = -0.9      # ... but one
    o = check_partition([v], h, w, [np.zeros(h * w, np.uint8)], None, False)[0]
    assert o["nc"] == 3 and o["reverse"] and o["mask"].sum() == 9 and o["seed"] == 4 * w + 5  # the plateau falls towards its last cell


def test_partition_rejections_and_hole():
    h, w = 16, 16
    N = h * w
    z = np.zeros(N, np.uint8)
    big = blob(h, w, 4, 10, 4, 10)
    prev_same = ref.partition(big, h, w, z)["mask"].reshape(-1).astype(np.uint8)
    prev_far = np.zeros((h, w), np.uint8)
    prev_far[12:15, 12:15] = 1
    two = blob(h, w, 5, 6, 5, 7)     # 2 cells of 256 = 0.0078 <= 0.01: rejected for area
    three = blob(h, w, 5, 6, 5, 8)   # 3 cells = 0.0117: kept
    ring = blob(h, w, 3, 9, 3, 9)
    ring.reshape(h, w)[5:7, 5:7] = -0.2  # an enclosed hole
    vs = [big, big, two, three, ring]
    prevs = [prev_same, prev_far.reshape(-1), prev_far.reshape(-1), prev_far.reshape(-1), prev_far.reshape(-1)]
    painted = [prev_same, prev_far.reshape(-1), z, z, z]
    outs = check_partition(vs, h, w, painted, prevs, use_prev=True)
    assert outs[0]["mask"].sum() == 0      # IoU 1 with the previous mask
    assert outs[1]["mask"].sum() == 36     # IoU 0
    assert outs[2]["mask"].sum() == 0 and outs[3]["mask"].sum() == 3
    assert outs[4]["mask"].sum() == 32 and outs[4]["union"].sum() == 36 and outs[4]["painted"].sum() == 32
    # the same five as a first pass: nothing is rejected, and an inactive image keeps its buffers
    mask, pt, un, seed = device_partition([np.asarray(v, np.float32) for v in vs], h, w, [z] * 5, None, False, active=[1, 1, 1, 1, 0])
    assert mask[0].sum() == 36 and mask[2].sum() == 2 and (un[4] == 9).all() and seed[4] == -7 and mask[4].sum() == 0
