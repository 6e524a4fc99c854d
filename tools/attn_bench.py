#!/usr/bin/env python3
"""Attention microbenchmark + ablation (diagnostic).  Builds ablated copies of attention.hip under
gpurun_out/ and times the hot-path shape with HIP events, interleaved rounds in one process.
ablate: 0 full, 1 no softmax VALU, 2 no PV MFMAs, 3 no S MFMAs, 4 no K/V staging, 5 no tiles (prologue+epilogue).
--relpos: instead, mvp_attention_relpos_fwd (SAM's decomposed relative-position bias) against mvp_attention_fwd, plus mvp_relpos_terms and
the two row gathers of a windowed block (relpos_ab).
--bias: instead, the shipped library's mvp_attention_bias_fwd (a dense fp32 [H, N, ld] logit bias) against mvp_attention_fwd on the same
operands, alternating, at N = 197 and 577 (env N="197 577"), B from env B (default 110), H = 12, every bf16x3 operand form."""
import ctypes as C, os, subprocess, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "midvision-probe_amd"))
import torch
from mvp import lib, ops

CS = os.path.join(REPO, "midvision-probe_amd", "csrc")
OUT = os.path.join(REPO, "tools", "micro")  # built in the build container, travels with the tree
os.makedirs(OUT, exist_ok=True)


def build(ablate, extra="", src=None, tag=""):
    so = os.path.join(OUT, f"libattn_ab{ablate}{tag}.so")
    src = src or f"{CS}/attention.hip"
    so = so.replace(".so", extra.replace(" ", "").replace("-D", "_").replace("=", "") + ".so")
    # the product's flags (csrc/Makefile print-cxxflags: no packed fp32, no SLP vectoriser), so that what is timed is what ships
    fl = subprocess.run(["make", "-s", "-C", CS, "print-cxxflags"], capture_output=True, text=True, check=True).stdout.strip().replace("-I../../include", f"-I{REPO}/include")
    cmd = f"set -o pipefail; /opt/rocm/bin/hipcc {fl} -w -shared -I{CS} -DMVP_ATT_ABLATE={ablate} {extra} {src} -o {so} 2>&1 | {{ grep -v 'recognized feature' || true; }}"
    if not os.path.exists(so):  # (reused when already built in the build container)
        subprocess.run(["bash", "-c", cmd], check=True)
    l = C.CDLL(so)
    l.mvp_attention_fwd.argtypes = [C.POINTER(lib.AttentionArgs), C.c_void_p]
    l.mvp_attention_fwd.restype = C.c_int
    return l


def bias_ab():
    """Biased against unbiased attention: same build, same buffers, three alternations of 20 launches each; min and median per variant."""
    import statistics
    dev = torch.device("cuda")
    B = int(os.environ.get("B", 110)); H = 12
    so = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for N in (int(n) for n in os.environ.get("N", "197 577").split()):
        ld = 64 * ((N + 63) // 64)
        bias = torch.randn(H, N, ld, device=dev)
        qkv = ops.split_bf16(torch.randn(B * N, 3 * H * 64, device=dev) * 0.5, 3)
        out = ops.empty_pair((B * N, H * 64), 3, dev)
        for vf, form in ((2, "bf16x3_vf16_qk16"), (1, "bf16x3_vf16"), (0, "bf16x3")):
            att = lib.AttentionArgs(qkv[0].data_ptr(), qkv[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, N, H, 3 * H * 64, H * 64, 0.125, 3, 0, vf, 0)
            ab = lib.AttentionBiasArgs(att, bias.data_ptr(), N * ld, ld)
            calls = {"plain": lambda: so.mvp_attention_fwd(C.byref(att), st), "bias": lambda: so.mvp_attention_bias_fwd(C.byref(ab), st)}
            res = {}
            for rnd in range(3):
                for vn, fn in calls.items():
                    for _ in range(3):
                        assert fn() == 0
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn()
                    e1.record(); torch.cuda.synchronize()
                    res.setdefault(vn, []).append(e0.elapsed_time(e1) / 20 * 1e3)
            mp, mb = statistics.median(res["plain"]), statistics.median(res["bias"])
            print(f"B={B} N={N} H={H} {form}: plain {mp:7.1f} us (rounds {' '.join(f'{x:.1f}' for x in res['plain'])})  "
                  f"bias {mb:7.1f} us (rounds {' '.join(f'{x:.1f}' for x in res['bias'])})  bias / plain = {mb / mp:.3f}  "
                  f"bias array {H * N * ld * 4 / 1e6:.2f} MB", flush=True)


def relpos_ab():
    """mvp_attention_relpos_fwd against mvp_attention_fwd at the same (B', N, H) (N = K * K keys on a K x K grid), the cost of
    mvp_relpos_terms and of the two row gathers of a windowed block: three alternations of 20 launches each, median per variant.
    Environment: B (images, default 4), N (default "196 4096"; N = 196 runs B' = 25 B windows, the 1024^2 geometry), H (default 12)."""
    import statistics
    dev = torch.device("cuda")
    B = int(os.environ.get("B", 4)); H = int(os.environ.get("H", 12)); Cw = H * 64
    so = lib.load()
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 20 * 1e3

    for N in (int(n) for n in os.environ.get("N", "196 4096").split()):
        K = int(round(N ** 0.5))
        assert K * K == N
        Bp = 25 * B if N == 196 else B
        M, ld = Bp * N, -(-2 * K // 4) * 4
        qf = torch.randn(M, 3 * Cw, device=dev) * 0.5
        rh, rw = torch.randn(K, K, 64, device=dev) * 0.1, torch.randn(K, K, 64, device=dev) * 0.1
        rel = torch.empty(Bp * H, N, ld, device=dev)
        qkv, out = ops.empty_pair((M, 3 * Cw), 3, dev), ops.empty_pair((M, Cw), 3, dev)
        res = {}
        for vf, form in ((2, "bf16x3_vf16_qk16"), (1, "bf16x3_vf16"), (0, "bf16x3")):
            terms = lambda: ops.relpos_terms(qf, qkv, rel, rh, rw, M, N, H, 3, v_f16=vf > 0, qk_f16=vf == 2)
            terms()
            att = lib.AttentionArgs(qkv[0].data_ptr(), qkv[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), Bp, N, H, 3 * Cw, Cw, 0.125, 3, 0, vf, 0)
            ar = lib.AttentionRelposArgs(att, rel.data_ptr(), N * ld, ld, K, K)
            calls = {"plain": lambda: so.mvp_attention_fwd(C.byref(att), st), "relpos": lambda: so.mvp_attention_relpos_fwd(C.byref(ar), st), "terms": terms}
            res = {k: [] for k in calls}
            for rnd in range(3):
                for vn, fn in calls.items():
                    res[vn].append(timed(fn))
            mp, mr, mt = (statistics.median(res[k]) for k in ("plain", "relpos", "terms"))
            print(f"B'={Bp} N={N} ({K}x{K}) H={H} {form}: plain {mp:8.1f} us  relpos {mr:8.1f} us  relpos / plain = {mr / mp:.3f}  "
                  f"relpos_terms {mt:7.1f} us  rel {Bp * H * N * ld * 4 / 1e6:.1f} MB", flush=True)
        if N == 196:  # the two gathers of a windowed block at 1024^2: 64 x 64 grid, 25 windows of 14 x 14 per image
            from mvp import vit
            part, unpart = (t.to(dev) for t in vit.sam_window_index(B, 64, 64, 14))
            xn, xw = ops.empty_pair((B * 4096, Cw), 3, dev), ops.empty_pair((M, Cw), 3, dev)
            gp = statistics.median(timed(lambda: ops.gather_rows(xn, xw, part, B * 4096, Cw)) for _ in range(3))
            gu = statistics.median(timed(lambda: ops.gather_rows(xw, xn, unpart, M, Cw)) for _ in range(3))
            print(f"B={B} 64x64 grid, w=14: gather into windows {gp:.1f} us, gather back {gu:.1f} us", flush=True)


def main():
    if "--bias" in sys.argv:
        return bias_ab()
    if "--relpos" in sys.argv:
        return relpos_ab()
    names = {0: "full", 1: "no_softmax", 2: "no_pv", 3: "no_s", 4: "no_stage", 5: "no_tiles"}
    variants = {names[a]: build(a) for a in names}
    prev = os.path.join(REPO, "tools", "micro", "attention_prev.hip")
    if "--ab" in sys.argv and os.path.exists(prev):  # A/B against a saved earlier version of the kernel
        variants = {"full": build(0), "prev": build(0, src=prev, tag="_prev")}
        for n in os.environ.get("SGB", "").split():  # the interleave ratio of the streaming kernel's S(t+1) / softmax(t) block
            variants[f"sgb{n}"] = build(0, extra=f"-DMVP_ATT_SGB={n}")
    if "--prio" in sys.argv:  # s_setprio around the MFMA clusters x stagger of waves 4-7 (MVP_ATT_PRIO / MVP_ATT_STAGGER)
        variants = {"base": build(0)}
        for pr, stg in ((1, 0), (0, 12), (0, 25), (1, 12), (1, 25), (1, 40)):
            variants[f"prio{pr}_stag{stg}"] = build(0, extra=f"-DMVP_ATT_PRIO={pr} -DMVP_ATT_STAGGER={stg}")
    # (tried in round 3 and dropped: delaying waves 4-7 of the resident kernel by 8 .. 48 x 64 cycles so that SIMD partners run out of
    # phase — 77.8 us -> 77.6 .. 80.4 at B = 96, 16.7 -> 16.8 .. 17.1 at B = 16: nothing)
    dev = torch.device("cuda")
    B = int(os.environ.get("B", 16)); H = 12
    for N in (197, 785, 1201):
        for prec in (3, 1):
            qkv = ops.split_bf16(torch.randn(B * N, 3 * H * 64, device=dev), 3)
            out = ops.empty_pair((B * N, H * 64), 3, dev)
            args = lib.AttentionArgs()
            vals = dict(qkv_hi=qkv[0].data_ptr(), qkv_lo=qkv[1].data_ptr(), out_hi=out[0].data_ptr(), out_lo=out[1].data_ptr(),
                        B=B, N=N, H=H, ld_qkv=3 * H * 64, ld_out=H * 64, scale=0.125, precision=prec)
            for k, v in vals.items():
                setattr(args, k, v)
            st = torch.cuda.current_stream().cuda_stream
            res = {}
            for rnd in range(3):
                for vn, l in variants.items():
                    for _ in range(3):
                        rc = l.mvp_attention_fwd(C.byref(args), st)
                        assert rc == 0, rc
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        l.mvp_attention_fwd(C.byref(args), st)
                    e1.record(); torch.cuda.synchronize()
                    res.setdefault(vn, []).append(e0.elapsed_time(e1) / 20 * 1e3)
            print(f"N={N} prec={prec}: " + "  ".join(f"{vn}={min(v):6.1f}us" for vn, v in res.items()), flush=True)


if __name__ == "__main__":
    main()
