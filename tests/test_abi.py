"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/mvp_hip.h declares; mvp/lib.py's structs, signatures and constants are the header's, field by field
(tests/abi_header.py reads it); argument validation returns error codes (no compute, no GPU)."""
import ctypes
import functools
import os
import re

import pytest

import abi_header
from conftest import REPO
from mvp import lib


def _declared():
    src = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(mvp_\w+)\s*\(", src, flags=re.M)))


def test_header_symbols_are_exported_and_bound():
    from mvp import lib

    declared = _declared()
    assert len(declared) >= 20
    assert set(declared) == set(lib.SYMBOLS) == set(_header()[1]), set(declared) ^ set(lib.SYMBOLS)
    so = lib.load()
    for name in declared:
        assert hasattr(so, name), name


def test_info_reports_abi_8_and_strerror():
    from mvp import lib

    inf = lib.info()
    assert inf.abi_version == 8
    assert lib.load().mvp_strerror(-1).decode().startswith("invalid argument")


def test_bad_arguments_return_einval():
    """Host-side shape checks run before any launch, so they are testable without a GPU."""
    from mvp import lib

    so = lib.load()
    a = lib.GemmArgs()  # all NULL / zero
    assert so.mvp_gemm_bias_act_res(ctypes.byref(a), None) == -1
    a = lib.GemmArgs(a_hi=16, w_hi=16, out_f32=16, M=4, N=4, K=48, lda=48, ldw=48, precision=1)
    assert so.mvp_gemm_bias_act_res(ctypes.byref(a), None) == -1  # K % 64 != 0
    b = lib.AttentionArgs(qkv_hi=16, out_hi=16, B=1, N=4, H=1, ld_qkv=100, ld_out=64, precision=1)
    assert so.mvp_attention_fwd(ctypes.byref(b), None) == -1  # ld_qkv < 3*H*64
    c = lib.LayerNormArgs(x=16, gamma=16, beta=16, out_hi=16, M=1, C=4098)
    assert so.mvp_layernorm_fwd(ctypes.byref(c), None) == -1
    assert so.mvp_bn_tokens_workspace_bytes(3152, 768) == (394 * 768 * 3 + 2 * 768) * 4  # 8-row slabs
    assert so.mvp_colsum_workspace_bytes(3136, 256) == 49 * 256 * 4


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from mvp import lib

    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(lib.MvpError, match="no CPU fallback"):
        lib.load()


@functools.lru_cache(None)
def _header():
    """(structs, prototypes, defines) of include/mvp_hip.h, as ctypes types (tests/abi_header.py)."""
    return abi_header.parse(lib.STRUCTS)


def test_every_header_struct_has_one_mirror():
    assert set(_header()[0]) == set(lib.STRUCTS), set(_header()[0]) ^ set(lib.STRUCTS)


@pytest.mark.parametrize("cname", sorted(lib.STRUCTS))
def test_mirror_fields_match_the_header(cname):
    """Name, order and ctypes type of every field: two neighbours of one size swapped in a mirror, or a float bound as an int, keep
    sizeof and hand the kernel wrong arguments (mvp/ops.py builds most structs positionally)."""
    assert lib.STRUCTS[cname]._fields_ == _header()[0][cname], cname


def test_ctypes_structs_match_the_compiled_header():
    """Every ctypes mirror in mvp/lib.py has the size the C compiler gave the struct of include/mvp_hip.h (mvp_sizeof); an entry
    missing from info.hip's MVP_SZ list answers -1."""
    so = lib.load()
    for cname in _header()[0]:
        assert so.mvp_sizeof(cname.encode()) == ctypes.sizeof(lib.STRUCTS[cname]), (cname, so.mvp_sizeof(cname.encode()))
    assert so.mvp_sizeof(b"nope") == -1


@pytest.mark.parametrize("name", sorted(lib.SYMBOLS))
def test_bound_signature_matches_the_header(name):
    """restype and argtypes of every loaded function are the header's prototype; for `int f(const T*, void* stream)` that is
    SYMBOLS[f] is STRUCTS[T]."""
    fn = getattr(lib.load(), name)
    assert (fn.restype, list(fn.argtypes)) == _header()[1][name], name


# the constants mvp/lib.py copies from the header: lib.<X> is MVP_<X>, the GEMM route families excepted
CONSTANTS = ("PREC_BF16 PREC_BF16X3 PREC_F16X2 ACT_NONE ACT_GELU ACT_RELU ACT_QUICK_GELU ACT_GELU_TANH RESIZE_NEAREST RESIZE_BILINEAR "
             "RESIZE_BICUBIC PAIR_SEPARATE PAIR_A_ILV32 PAIR_W_ILV32 BN_ACT_NONE BN_ACT_SIGMOID BN_ACT_TANH BN_ACT_WORKSPACE_BYTES "
             "BCE_WORKSPACE_BYTES BN_RUNNING_MAX TILES_SHARED TILES_NO_PP TILES_NO_UNI ROUTE_PP ROUTE_TILE ROUTE_SPLITK ROUTE_CONV "
             "ATT_V_BF16_PAIR ATT_V_F16 ATT_V_F16_QK_F16").split()


def _header_name(x):
    return "MVP_GEMM_" + x if x.startswith("ROUTE_") else "MVP_" + x


def test_the_expected_constants_are_the_ones_lib_defines():
    defines = _header()[2]
    found = {x for x, v in vars(lib).items() if x.isupper() and isinstance(v, int) and _header_name(x) in defines}
    assert len(CONSTANTS) == 30 and found == set(CONSTANTS), found ^ set(CONSTANTS)


@pytest.mark.parametrize("x", CONSTANTS)
def test_constant_equals_the_header_define(x):
    assert getattr(lib, x) == _header()[2][_header_name(x)], x


def test_integration_md_binding_matches_the_header():
    """INTEGRATION.md §3 shows the ctypes struct a maintainer would copy.  Execute exactly that snippet's class definition and hold its
    size to the compiled header (mvp_sizeof) and its field names / order to mvp/lib.py's mirror: a field added to mvp_gemm_args without
    updating the document fails here (boundary doc drift)."""
    import ctypes as C

    from mvp import lib

    md = open(os.path.join(REPO, "INTEGRATION.md")).read()
    m = re.search(r"class GemmArgs\(C\.Structure\):.*?\n(    _fields_ = .*?\])\s*\n\s*#", md, flags=re.S)
    assert m, "INTEGRATION.md: the GemmArgs binding snippet was not found"
    ns = {"C": C, "_vp": C.c_void_p, "_i": C.c_int}
    exec("class GemmArgs(C.Structure):\n" + m.group(1), ns)
    doc = ns["GemmArgs"]
    assert [f[0] for f in doc._fields_] == [f[0] for f in lib.GemmArgs._fields_]
    assert C.sizeof(doc) == lib.load().mvp_sizeof(b"mvp_gemm_args") == C.sizeof(lib.GemmArgs)
