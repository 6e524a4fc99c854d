"""The kernel choice of mvp_gemm_bias_act_res as the library reports it — mvp_gemm_route, a host-only query (no GPU needed) — and as
ops.gemm_tile labels it, held to a literal table.  The plain-GEMM rows are what the Python copy of the rule returned before ABI 8; the
cases that copy got wrong (K % 64 != 0, EXT epilogues, convolutions, interleaved operands, MVP_TILES_NO_PP) are read off csrc/gemm.hip.
A row changes only with a measurement behind it: the tile choice decides the speed of every GEMM."""
import ctypes as C

import pytest

from mvp import lib, ops

BF16, X3, F2 = lib.PREC_BF16, lib.PREC_BF16X3, lib.PREC_F16X2
POLICIES = (0, lib.TILES_SHARED, lib.TILES_NO_PP, lib.TILES_SHARED | lib.TILES_NO_PP)

# ViT-B/16 blocks (C 768, hidden 3072) at M = 16, 64 and 110 images of 197 rows; DINOv2-L/14 blocks (C 1024, hidden 4096) at 16 and 64
# images of 257 rows; the probe head.
PLAIN = {
    # (M, N, K): {precision: (ALONE, SHARED, ALONE | NO_PP, SHARED | NO_PP)}
    (3152, 2304, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('128, 128, 64, 3, 1', 'pp 256, 256, 32, 3', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (3152, 768, 768): {BF16: ('64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2'),
                          X3: ('64, 64, 64, 3, 1', '128, 128, 64, 3, 1', '64, 64, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('64, 64, 64, 2, 1', '64, 64, 64, 2, 1', '64, 64, 64, 2, 1', '64, 64, 64, 2, 1')},
    (3152, 3072, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('64, 128, 64, 3, 1', 'pp 256, 256, 32, 3', '64, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (3152, 768, 3072): {BF16: ('64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2'),
                          X3: ('64, 64, 64, 3, 1', '128, 128, 64, 3, 1', '64, 64, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('64, 64, 64, 2, 1', '64, 64, 64, 2, 1', '64, 64, 64, 2, 1', '64, 64, 64, 2, 1')},
    (12608, 2304, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (12608, 768, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('128, 64, 64, 3, 1', 'pp 256, 256, 32, 3', '128, 64, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 64, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 64, 64, 2, 1', '128, 64, 64, 2, 1')},
    (12608, 3072, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('128, 128, 64, 3, 1', 'pp 256, 256, 32, 3', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (12608, 768, 3072): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '128, 64, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 64, 64, 2, 1', '128, 64, 64, 2, 1')},
    (21670, 2304, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (21670, 768, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '128, 64, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 64, 64, 2, 1', '128, 64, 64, 2, 1')},
    (21670, 3072, 768): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (21670, 768, 3072): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '128, 64, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 64, 64, 2, 1', '128, 64, 64, 2, 1')},
    (4112, 3072, 1024): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('64, 128, 64, 3, 1', 'pp 256, 256, 32, 3', '64, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (4112, 1024, 1024): {BF16: ('64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2'),
                          X3: ('128, 128, 64, 3, 1', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (4112, 4096, 1024): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('64, 128, 64, 3, 1', 'pp 256, 256, 32, 3', '64, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (4112, 1024, 4096): {BF16: ('64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2'),
                          X3: ('128, 128, 64, 3, 1', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (16448, 3072, 1024): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('128, 128, 64, 3, 1', 'pp 256, 256, 32, 3', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (16448, 1024, 1024): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('64, 128, 64, 3, 1', 'pp 256, 256, 32, 3', '64, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('128, 128, 64, 2, 1', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (16448, 4096, 1024): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '128, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (16448, 1024, 4096): {BF16: ('128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2', '128, 128, 64, 1, 2'),
                          X3: ('pp 256, 256, 32, 3', 'pp 256, 256, 32, 3', '64, 128, 64, 3, 1', '128, 128, 64, 3, 1'),
                          F2: ('pp 256, 256, 32, 2', 'pp 256, 256, 32, 2', '128, 128, 64, 2, 1', '128, 128, 64, 2, 1')},
    (3136, 256, 3072): {BF16: ('64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2', '64, 64, 64, 1, 2'),
                          X3: ('64, 64, 64, 3, 2', '64, 64, 64, 3, 2', '64, 64, 64, 3, 2', '64, 64, 64, 3, 2'),
                          F2: ('64, 64, 64, 2, 1', '64, 64, 64, 2, 1', '64, 64, 64, 2, 1', '64, 64, 64, 2, 1')},
}


def _args(M, N, K, precision=X3, splitk=1, tile_policy=0, **kw):
    """A GEMM's arguments with stand-in operand pointers (the route and the argument checks only test them for NULL)."""
    a = lib.GemmArgs(a_hi=16, a_lo=16, w_hi=16, w_lo=16, out_f32=16, out_hi=16, out_lo=16, M=M, N=N, K=K, lda=K, ldw=K, ldr=N, ldo=N,
                     ldob=N, precision=precision, splitk=splitk, tile_policy=tile_policy)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_route_struct_matches_the_compiled_header():
    assert lib.load().mvp_sizeof(b"mvp_gemm_route_t") == C.sizeof(lib.GemmRoute) == 8 * 4
    assert lib.SYMBOLS["mvp_gemm_route"] is None and hasattr(lib.load(), "mvp_gemm_route")


def _route(a):
    r = lib.GemmRoute()
    rc = lib.load().mvp_gemm_route(C.byref(a), C.byref(r))
    return rc, (r.family, r.bm, r.bn, r.bk, r.split, r.nstage, r.nw, r.wnw)


@pytest.mark.parametrize("shape", list(PLAIN))
def test_plain_gemm_routes(shape):
    M, N, K = shape
    for pr, labels in PLAIN[shape].items():
        for pol, want in zip(POLICIES, labels):
            assert ops.gemm_tile(M, N, K, pr, 1, pol) == want, (shape, pr, pol)
            rc, r = _route(_args(M, N, K, pr, 1, pol))
            assert rc == 0 and (r[0] == lib.ROUTE_PP) == want.startswith("pp "), (shape, pr, pol, r)


def test_splitk_routes():
    for pol in (0, lib.TILES_SHARED):
        assert ops.gemm_tile(3136, 256, 3072, X3, 4, pol) == "128, 64, 64, 3, 1, splitk"
        assert ops.gemm_tile(3136, 256, 3072, BF16, 4, pol) == "128, 64, 64, 1, 2, splitk"
    assert ops.gemm_tile(3152, 2304, 768, X3, 2) == "128, 128, 64, 3, 1, splitk"
    assert _route(_args(3136, 256, 3072, X3, 4)) == (0, (lib.ROUTE_SPLITK, 128, 64, 64, 3, 1, 4, 2))


def test_routes_the_python_copy_got_wrong():
    # K % 64 != 0: the BK = 32 two-stage tile (DINOv2's bf16x3 patch embedding, K = 3 * 14 * 14 padded to 608; the ResNet stem, K = 160)
    assert ops.gemm_tile(4096, 768, 608, X3) == "128, 64, 32, 3, 2"
    assert ops.gemm_tile(200704, 64, 160, X3) == "128, 64, 32, 3, 2"
    assert _route(_args(4096, 768, 608)) == (0, (lib.ROUTE_TILE, 128, 64, 32, 3, 2, 4, 2))
    # an EXT epilogue (here an output mask) never runs on the large-M kernel
    assert ops.gemm_tile(21670, 3072, 768, X3) == "pp 256, 256, 32, 3"
    assert _route(_args(21670, 3072, 768, out_mask=16, ldm=3072)) == (0, (lib.ROUTE_TILE, 128, 128, 64, 3, 1, 8, 2))
    # an interleaved A operand: only the large-M kernel reads it, whatever the shape
    assert _route(_args(300, 512, 96, pair_layout=lib.PAIR_A_ILV32, lda=192, a_lo=None)) == (0, (lib.ROUTE_PP, 256, 256, 32, 3, 0, 0, 0))
    assert ops._route_label(3152, 768, 768, X3, 1, 0, a_ilv=True) == "pp 256, 256, 32, 3"
    assert ops._route_label(300, 512, 96, F2, 1, 0, a_ilv=True) == "pp 256, 256, 32, 2"


@pytest.mark.parametrize("rows,family", [(256, lib.ROUTE_PP), (255, lib.ROUTE_CONV)])
def test_conv_routes_on_each_side_of_512_large_tiles(rows, family):
    """3x3 convolution, 256 -> 256 channels, two images: 2 * rows * 256 output pixels = 512 (rows = 256) or 510 tiles of 256 x 256."""
    H, W, Cc = rows, 256, 256
    a = _args(2 * H * W, 256, 9 * Cc, lda=Cc, conv=1, cH=H, cW=W, cC=Cc, cHo=H, cWo=W, ckh=3, ckw=3, cstride=1, cpad=1, zero_page=16)
    want = (lib.ROUTE_PP, 256, 256, 32, 3, 0, 0, 0) if family == lib.ROUTE_PP else (lib.ROUTE_CONV, 128, 128, 64, 3, 1, 8, 2)
    assert _route(a) == (0, want)
    a.tile_policy = lib.TILES_NO_PP
    assert _route(a) == (0, (lib.ROUTE_CONV, 128, 128, 64, 3, 1, 8, 2))


def test_refused_arguments():
    so = lib.load()
    # splitk < 0 (what selected the removed k-balanced kernel): refused by the query, the dispatcher and mvp_gemm_pp, before any launch
    a = _args(21670, 3072, 768, splitk=-1)
    assert _route(a)[0] == -1
    assert so.mvp_gemm_bias_act_res(C.byref(a), None) == -1
    assert so.mvp_gemm_pp(C.byref(a), None) == -1
    # the two-product mode has no K % 64 != 0 tile
    assert _route(_args(4096, 768, 608, F2))[0] == -1
    with pytest.raises(lib.MvpError):
        ops.gemm_tile(4096, 768, 608, F2)
    # K % 32 != 0 anywhere, and no output
    assert _route(_args(4096, 768, 600))[0] == -1
    assert _route(_args(4096, 768, 768, out_f32=None, out_hi=None, out_lo=None))[0] == -1
    assert so.mvp_gemm_route(C.byref(_args(64, 64, 64)), None) == -1
