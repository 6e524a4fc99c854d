"""CPU side of the f16x2 range guard: the record's restatement on hand-made bit patterns, the policy table of
mvp.backbone.range_guard_action, and the C ABI of mvp_f16_range_scan (header text, export, argument checks — no launch)."""
import ctypes
import os
import warnings

import pytest
import torch

from conftest import REPO
from f16_scan_ref import ilv32, scan_record
from mvp import backbone as bb
from mvp import lib


def _bits(*words):
    return torch.tensor([w - 0x10000 if w >= 0x8000 else w for w in words], dtype=torch.int16)


def test_restatement_on_bit_patterns():
    assert scan_record(_bits(0x7BFE, 0x0000, 0x3C00)) == [0x7BFE, 0, 0, 3]  # 65472: the largest value below saturation
    assert float(_bits(0x7BFE).view(torch.float16)[0]) == 65472.0
    assert scan_record(_bits(0x7BFF)) == [0x7BFF, 1, 0, 1]
    assert scan_record(_bits(0xFBFF, 0x7BFF, 0x0001)) == [0x7BFF, 2, 0, 3]  # the sign is dropped
    assert scan_record(_bits(0x7C00)) == [0x7C00, 0, 1, 1]  # +inf
    assert scan_record(_bits(0xFC00, 0x7E00, 0x7BFF)) == [0x7E00, 1, 2, 3]  # -inf, a quiet NaN, one saturated
    assert scan_record(_bits(0xFFFF)) == [0x7FFF, 0, 1, 1]
    assert scan_record(_bits(0x8000, 0x0000)) == [0, 0, 0, 2]  # -0, +0


def test_restatement_accumulates_and_takes_any_16_bit_dtype():
    a, b = _bits(0x7BFF, 0x0400), _bits(0x7C01, 0x7BFF, 0x7BFF)
    assert scan_record(b, accumulate=scan_record(a)) == [0x7C01, 3, 1, 5]
    assert scan_record(a.view(torch.bfloat16)) == scan_record(a.view(torch.float16)) == scan_record(a)
    assert scan_record(_bits(1), accumulate=[5, 0, 0, (1 << 32) - 1]) == [5, 0, 0, 0]  # n_scanned wraps
    hi, lo = torch.arange(128, dtype=torch.int16).view(2, 64), -torch.arange(128, dtype=torch.int16).view(2, 64)
    t = ilv32(hi, lo)
    assert t.shape == (2, 128) and torch.equal(t[:, :32], hi[:, :32]) and torch.equal(t[:, 32:64], lo[:, :32]) and torch.equal(t[:, 64:96], hi[:, 32:])


POLICY = [
    # (MVP_F16_GUARD, range_guard=, weights from a file, world) -> action
    ((None, None, False, 1), "off"),       # auto, seeded random init or weights=: nothing existing changes
    ((None, None, False, 8), "off"),
    ((None, None, True, 1), "fallback"),   # auto, a checkpoint file, one rank
    ((None, None, True, 2), "raise"),      # auto, a checkpoint file, several ranks: never different arithmetic per rank
    (("auto", None, True, 2), "raise"),
    (("auto", None, False, 1), "off"),
    (("", None, True, 1), "fallback"),     # an empty variable is an unset one
    (("off", None, True, 1), "off"),
    (("warn", None, False, 1), "warn"),    # forced on whatever the source
    (("raise", None, False, 1), "raise"),
    (("fallback", None, False, 4), "fallback"),
    (("off", "fallback", False, 1), "fallback"),  # the keyword wins over the environment
    (("raise", "off", True, 2), "off"),
    (("warn", "auto", True, 1), "fallback"),
    (("warn", "auto", True, 3), "raise"),
    (("warn", "auto", False, 1), "off"),
    ((None, "WARN", True, 1), "warn"),
]


@pytest.mark.parametrize("args, action", POLICY)
def test_policy_table(args, action):
    assert bb.range_guard_action(*args) == action


def test_policy_rejects_unknown_modes():
    with pytest.raises(ValueError, match="off, auto, warn, raise, fallback"):
        bb.range_guard_action("sometimes", None, False, 1)
    with pytest.raises(ValueError):
        bb.range_guard_action(None, "on", True, 1)


def test_wrapper_reads_keyword_environment_and_file_flag(monkeypatch, tmp_path):
    from evals.models.dino import DINO

    sd = bb.random_vit_state_dict(embed_dim=128, depth=4, patch=16, img=64, seed=3)
    monkeypatch.delenv("MVP_F16_GUARD", raising=False)
    m = DINO(weights=sd)
    assert not m.weights_from_file and m.range_guard_action() == "off" and m.f16_range_report() is None
    monkeypatch.setenv("MVP_F16_GUARD", "warn")
    assert m.range_guard_action() == "warn"
    assert DINO(weights=sd, range_guard="raise").range_guard_action() == "raise"
    with pytest.raises(ValueError):
        DINO(weights=sd, range_guard="maybe")
    monkeypatch.delenv("MVP_F16_GUARD")
    # a checkpoint file under MVP_CKPT_DIR: the loader sets the flag, 'auto' arms the guard (no forward runs on the CPU)
    full = bb.random_vit_state_dict(embed_dim=128, depth=4, patch=16, img=64, seed=3)
    torch.save(full, tmp_path / "dino_vitb16.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (no "using seeded random init" warning: the file was found)
        f = DINO()
    assert f.weights_from_file and f.range_guard_action() == "fallback"
    monkeypatch.setenv("MVP_F16_GUARD", "off")
    assert f.range_guard_action() == "off"


def test_header_and_export():
    src = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    assert "struct mvp_f16_scan_args {" in src
    assert "Added within 8: mvp_f16_range_scan" in src
    assert "#define MVP_ABI_VERSION 8" in src
    so = lib.load()
    assert hasattr(so, "mvp_f16_range_scan")
    assert lib.SYMBOLS["mvp_f16_range_scan"] is lib.STRUCTS["mvp_f16_scan_args"]
    assert so.mvp_sizeof(b"mvp_f16_scan_args") == ctypes.sizeof(lib.F16ScanArgs)


BAD_ARGS = [
    dict(hi=0), dict(record=0), dict(rows=0), dict(cols=0), dict(cols=12), dict(col0=4), dict(col0=-8), dict(ld=36), dict(hi=24), dict(record=18),
    dict(layout=2), dict(cols=48), dict(col0=8, cols=40),  # a window that ends beyond ld = 40
    dict(layout=1, col0=32, cols=32, ld=64), dict(layout=1, cols=64, ld=88),  # interleaved: the second hi block starts at word 64
    dict(rows=1 << 30, cols=32),  # rows * cols / 8 >= 2^31
]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_arguments_return_einval(bad):
    """Host-side checks run before any launch (the pointers are never dereferenced)."""
    kw = dict(hi=4096, record=8192, rows=3, col0=0, cols=32, ld=40, layout=0)
    kw.update(bad)
    assert lib.load().mvp_f16_range_scan(ctypes.byref(lib.F16ScanArgs(**kw)), None) == -1
