"""CPU checks of the DINOv2 backbones (ViT-B/14, B/14 with registers, L/14): the choice files, hub-layout checkpoints, the wrapper's
refusals and taps, the fp64 restatement (tests/dinov2_ref.py) against the transformers-built goldens, and the ABI 7 additions
(mvp_gemm_scaled, mvp_patch_gather_ld, mvp_prefix_rows) as declared, exported, bound and sized."""
import hashlib
import json
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch
import yaml

from conftest import PKG, REPO, load_golden, rel_l2

# SHA-256 of the reference's configs/backbone/<name>.yaml as parsed (canonical JSON, sorted keys), as in test_configs_cpu.py
REF_DIGESTS = {
    "dinov2_b14": "896049008d568ea4c57a35f3ee89aa64527d8fc546d4d8c3810eea25243404ca",
    "dinov2_b14_reg": "9d581a246711a7261d07bd4c47025261edd6fd31c46d3f6f3cdc5dd1c6807c6a",
    "dinov2_l14": "835b948475987a8b937a339f80831d1afda19b0ad66607f428d662a8ad71fe34",
}


def _dino(**kw):
    from evals.models.dino import DINO

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "no local checkpoint: seeded random init"
        return DINO(**kw)


@pytest.mark.parametrize("name", sorted(REF_DIGESTS))
def test_choice_files_match_reference_and_compose(name):
    from mvp import config

    node = yaml.safe_load(open(os.path.join(config.CONFIG_DIR, "backbone", name + ".yaml")))
    assert hashlib.sha256(json.dumps(node, sort_keys=True).encode()).hexdigest() == REF_DIGESTS[name], node
    for entry in ("depth_training", "spair_correspondence"):
        cfg = config.compose(entry, [f"backbone={name}"])
        assert cfg["backbone"]["dino_name"] == "dinov2" and cfg["backbone"]["output"] == "dense-cls"
    model = config.instantiate(node, return_multilayer=True)
    assert model.patch_size == 14 and model.output == "dense-cls"


def test_taps_prefix_and_pos_modes():
    b = _dino(dino_name="dinov2", model_name="vitb14", output="dense-cls", return_multilayer=True)
    r = _dino(dino_name="dinov2", model_name="vitb14_reg", return_multilayer=True)
    big = _dino(dino_name="dinov2", model_name="vitl14", output="dense-cls", return_multilayer=True)
    assert b.multilayers == r.multilayers == [2, 5, 8, 11] and big.multilayers == [5, 11, 17, 23]
    assert (b.n_prefix, r.n_prefix, big.n_prefix) == (1, 5, 1)
    assert (b.pos_embed_mode, r.pos_embed_mode) == ("dino", "dinov2_reg")
    assert b.feat_dim == [1536] * 4 and big.feat_dim == [2048] * 4
    assert big.vit.embed_dim == 1024 and big.heads == 16 and big.vit.pos_embed.shape == (1, 1370, 1024)
    single = _dino(dino_name="dinov2", model_name="vitl14")
    assert single.multilayers == [23]


def test_refusals():
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        _dino(dino_name="dinov2", model_name="vitg14")
    with pytest.raises(NotImplementedError, match="return_kqv"):
        _dino(dino_name="dinov2", model_name="vitb14", return_kqv=True)
    with pytest.raises(NotImplementedError):
        _dino(dino_name="dinov2", model_name="vitb16")


def test_hub_layout_checkpoint_with_chunked_blocks(tmp_path, monkeypatch):
    """torch.hub layout under MVP_CKPT_DIR with the hub's file name: chunked ``blocks.<chunk>.<i>.`` keys are flattened, mask_token and
    the final norm are dropped, register tokens and LayerScale gammas kept."""
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(128, 4, 4, seed=9)
    chunked = {}
    for k, v in sd.items():
        m = re.match(r"blocks\.(\d+)\.(.*)", k)
        chunked[f"blocks.{int(m.group(1)) // 2}.{m.group(1)}.{m.group(2)}" if m else k] = v
    torch.save(chunked, tmp_path / "dinov2_vitb14_reg4_pretrain.pth")
    monkeypatch.setenv("MVP_CKPT_DIR", str(tmp_path))
    m = _dino(dino_name="dinov2", model_name="vitb14_reg", return_multilayer=True)
    got = m.vit.state_dict()
    assert "mask_token" not in got and not any(k.startswith("norm.") for k in got)
    assert m.vit.depth == 4 and m.n_prefix == 5 and m.multilayers == [0, 1, 2, 3]
    for k, v in bb.dinov2_hub_to_engine(sd).items():
        assert torch.equal(got[k], v), k
    assert torch.equal(got["blocks.3.ls2.gamma"], sd["blocks.3.ls2.gamma"])


def test_random_generator_statistics():
    from mvp import backbone as bb

    sd = bb.random_dinov2_state_dict(768, 12, 4, seed=0)
    assert sd["pos_embed"].shape == (1, 37 * 37 + 1, 768) and sd["register_tokens"].shape == (1, 4, 768)
    g = torch.cat([sd[f"blocks.{i}.ls{j}.gamma"] for i in range(12) for j in (1, 2)])
    assert 1e-6 <= g.min().item() and g.max().item() <= 1.0 and g.min().item() < 1e-5


@pytest.mark.parametrize("R", [0, 4])
def test_oracle_matches_goldens(R):
    """tests/dinov2_ref.py against transformers' Dinov2Model / Dinov2WithRegistersModel with the reference wrapper's glue
    (tests/golden/make_goldens_dinov2.py), tiny model, ragged image size."""
    import sys

    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import dinov2_ref
    import make_goldens_dinov2 as mg
    from mvp import backbone as bb

    g = load_golden("dinov2_tiny.npz")
    sd = bb.random_dinov2_state_dict(mg.TINY["C"], mg.TINY["depth"], R, seed=mg.tiny_seed(R))
    np.testing.assert_allclose(mg.checksums(sd), g[f"r{R}_checksums"], rtol=1e-9)
    assert np.array_equal(mg.tiny_images().numpy(), g["images"])
    outs = dinov2_ref.dense_features(bb.dinov2_hub_to_engine(sd), torch.from_numpy(g["images"]).double(), [0, 1, 2, 3])
    for j, o in enumerate(outs):
        assert rel_l2(o.numpy(), g[f"r{R}_tap{j}"]) < 1e-6, j


def test_new_exports_declared_bound_and_sized():
    from mvp import lib

    hdr = open(os.path.join(REPO, "include", "mvp_hip.h")).read()
    so = lib.load()
    for name, st in (("mvp_gemm_scaled", lib.GemmScaledArgs), ("mvp_patch_gather_ld", lib.PatchGatherLdArgs), ("mvp_prefix_rows", lib.PrefixRowsArgs)):
        assert re.search(rf"^int {name}\(", hdr, flags=re.M), name
        assert lib.SYMBOLS[name] is st and hasattr(so, name)
    for cname in ("mvp_gemm_scaled_args", "mvp_patch_gather_ld_args", "mvp_prefix_rows_args"):
        assert so.mvp_sizeof(cname.encode()) == __import__("ctypes").sizeof(lib.STRUCTS[cname]), cname
    assert so.mvp_sizeof(b"mvp_gemm_scaled_args") == so.mvp_sizeof(b"mvp_gemm_args") + 8
    integ = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in ("mvp_gemm_scaled", "mvp_patch_gather_ld", "mvp_prefix_rows"):
        assert name in integ, name


def test_new_exports_validate_arguments():
    import ctypes as C

    from mvp import lib

    so = lib.load()
    g = lib.GemmArgs(a_hi=16, a_lo=16, w_hi=16, w_lo=16, out_f32=16, M=64, N=64, K=64, lda=64, ldw=64, ldo=64, precision=3)
    assert so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(g, None)), None) == -1  # no scale
    g.splitk = 2
    assert so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(g, 256)), None) == -1  # split-K takes no scale
    g.splitk, g.conv = 0, 1
    assert so.mvp_gemm_scaled(C.byref(lib.GemmScaledArgs(g, 256)), None) == -1
    pg = lib.PatchGatherArgs(16, 16, 16, 1, 3, 28, 28, 14, 2, 2, 0, 0)
    assert so.mvp_patch_gather_ld(C.byref(lib.PatchGatherLdArgs(pg, 584)), None) == -1  # ldk < C*P*P
    assert so.mvp_patch_gather_ld(C.byref(lib.PatchGatherLdArgs(pg, 610)), None) == -1  # ldk % 4
    assert so.mvp_prefix_rows(C.byref(lib.PrefixRowsArgs(16, 16, None, 16, 1, 10, 64, 4)), None) == -1  # R > 0 without registers
    assert so.mvp_prefix_rows(C.byref(lib.PrefixRowsArgs(16, 16, 16, 16, 1, 4, 64, 4)), None) == -1  # N < 1 + R


def test_new_code_objects_have_no_private_segment():
    """Every kernel of the two GEMM objects — the large-M kernel and the tile kernels, their LayerScale instantiations among them —
    keeps every value in registers (no scratch)."""
    import shutil
    import tempfile

    so = os.path.join(PKG, "csrc", "libmvp_hip.so")
    tool = lambda n: shutil.which(n) or os.path.join("/opt/rocm/llvm/bin", n)  # noqa: E731
    objs = [os.path.join(PKG, "csrc", "build", f) for f in ("gemm_pp.o", "gemm.o")]
    with tempfile.TemporaryDirectory() as td:
        seen = scaled = 0
        for o in objs:  # the device code object: the object's offload bundle (.hip_fatbin), unbundled for gfx950
            fb, co = os.path.join(td, "fatbin"), os.path.join(td, os.path.basename(o) + ".co")
            subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", o, os.path.join(td, "host.o")], check=True)
            subprocess.run([tool("clang-offload-bundler"), "--type=o", f"--input={fb}", f"--output={co}", "--unbundle",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
            readelf = tool("llvm-readelf")
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split(".name:")[1:]:
                name = block.split("\n", 1)[0].strip()
                m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
                assert m and int(m.group(1)) == 0, (name, m and m.group(1))
                seen += 1
                scaled += "mvp_gemm_kscaled" in name
        assert seen >= 64 and scaled >= 8, (seen, scaled)
    assert os.path.exists(so)


def _full_cases():
    import sys

    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_goldens_dinov2 as mg

    return [(key, shape) for key, (_, _, shapes) in mg.FULL.items() for shape in shapes]


@pytest.mark.parametrize("key,shape", _full_cases())
def test_oracle_matches_full_size_sampled_goldens(key, shape):
    """The fp64 restatement at full size — B/14 and B/14-reg at 224^2 and 480 x 640 (pos-embed 37 x 37 resampled to 16 x 16 and 34 x 45),
    L/14 at 224^2 — against the sampled outputs of transformers' models (tests/golden/make_goldens_dinov2.py)."""
    import sys

    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import dinov2_ref
    import make_goldens_dinov2 as mg
    from mvp import backbone as bb

    g = load_golden("dinov2_full_sampled.npz")
    model_name, seed, _ = mg.FULL[key]
    C, depth, R = bb.DINOV2_ARCH[model_name]
    sd = bb.random_dinov2_state_dict(C, depth, R, seed=seed)
    np.testing.assert_allclose(mg.checksums(sd), g[f"{key}_checksums"], rtol=1e-9)
    B, H, W = shape
    layers = bb.multilayer_indices(depth)
    outs = dinov2_ref.dense_features(bb.dinov2_hub_to_engine(sd), mg.full_images(B, H, W).double(), layers)
    for j, o in enumerate(outs):
        tag = f"{key}_{B}x{H}x{W}_tap{j}"
        assert tuple(o.shape) == tuple(g[tag + "_shape"]), tag
        got = o.numpy().reshape(-1)[mg.sample_index(o.numel())]
        assert rel_l2(got, g[tag]) < 1e-6, tag
