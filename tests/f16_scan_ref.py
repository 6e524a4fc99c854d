"""The record of mvp_f16_range_scan restated with torch integer ops on the CPU (tests/test_f16_guard_cpu.py,
tests/test_gpu_f16_scan_kernel.py): no float is ever made of the bits."""
import torch

SAT_BITS, INF_BITS = 0x7BFF, 0x7C00  # |v| = 65504 (where the producers saturate), +inf


def scan_record(hi: torch.Tensor, accumulate=None):
    """[max_bits, n_sat, n_nonfinite, n_scanned mod 2^32] of the 16-bit words ``hi`` (any shape; bf16 / fp16 / int16 typed), as four
    Python ints; ``accumulate``: an earlier record the new one is folded into (max, add, add, add mod 2^32)."""
    mag = hi.contiguous().view(torch.int16).to(torch.int32) & 0x7FFF
    rec = [int(mag.max()) if mag.numel() else 0, int((mag == SAT_BITS).sum()), int((mag >= INF_BITS).sum()), mag.numel() % (1 << 32)]
    if accumulate is not None:
        rec = [max(rec[0], accumulate[0])] + [(a + b) % (1 << 32) for a, b in zip(rec[1:], accumulate[1:])]
    return rec


def ilv32(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    """[R, K] hi and lo words -> ONE [R, 2K] array, hi | lo interleaved per 32 columns (MVP_PAIR_A_ILV32); K % 32 == 0."""
    R, K = hi.shape
    return torch.stack((hi.view(R, K // 32, 32), lo.view(R, K // 32, 32)), dim=2).reshape(R, 2 * K).contiguous()
