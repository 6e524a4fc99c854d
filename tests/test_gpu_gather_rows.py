"""mvp_gather_rows — out[r] = idx[r] >= 0 ? in[idx[r]] : 0 — against torch.index_select plus zero rows, bit for bit: both pair forms
(separate hi / lo, interleaved), widths 128 and 384, SAM's window tables (5 x 7 / w 3 with B = 2, 16 x 16 / w 14), an all-pad table, an
identity table, and the un-partition applied after the partition.  Outputs are prefilled with a sentinel pattern."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(rows, cols, dev, salt):
    i = torch.arange(rows * cols, device=dev, dtype=torch.int64)
    return ((i * 40503 + salt) % 65536 - 32768).to(torch.int16).view(rows, cols).view(torch.bfloat16)


def _want(src, idx):
    out = src.view(torch.int16)[idx.clamp(min=0).long()].clone()
    out[idx < 0] = 0
    return out


def _gather(src, idx, cols, form, dev):
    """-> list of (got, source) int16 arrays, one per array of the pair form."""
    from mvp import ops

    rows_in, rows = src[0].shape[0], idx.numel()
    if form == "ilv":
        a, b = ops.IlvPair(rows_in, cols, dev), ops.IlvPair(rows, cols, dev)
        a.t.copy_(_bits(rows_in, 2 * cols, dev, 5))
        b.t.copy_(_bits(rows, 2 * cols, dev, 6))
        ops.gather_rows(a, b, idx, rows_in, cols)
        torch.cuda.synchronize()
        return [(b.t.view(torch.int16), a.t)]
    dst = (_bits(rows, cols, dev, 7), _bits(rows, cols, dev, 8))
    ops.gather_rows(src, dst, idx, rows_in, cols)
    torch.cuda.synchronize()
    return [(dst[0].view(torch.int16), src[0]), (dst[1].view(torch.int16), src[1])]


@pytest.mark.parametrize("form", ["separate", "ilv"])
@pytest.mark.parametrize("cols", [128, 384])
@pytest.mark.parametrize("grid", [(2, 5, 7, 3), (1, 16, 16, 14)])
def test_window_tables_bit_for_bit(dev, form, cols, grid):
    from mvp import vit

    B, gh, gw, w = grid
    part, unpart = (t.to(dev) for t in vit.sam_window_index(B, gh, gw, w))
    M = B * gh * gw
    src = (_bits(M, cols, dev, 1), _bits(M, cols, dev, 2))
    for got, s in _gather(src, part, cols, form, dev):
        assert torch.equal(got, _want(s, part))
        assert int((got[part < 0] != 0).sum()) == 0 and int((part < 0).sum()) > 0
    if form == "separate":  # the inverse after the forward returns the input
        from mvp import ops

        mid = (torch.empty(part.numel(), cols, dtype=torch.bfloat16, device=dev), torch.empty(part.numel(), cols, dtype=torch.bfloat16, device=dev))
        back = (_bits(M, cols, dev, 3), _bits(M, cols, dev, 4))
        ops.gather_rows(src, mid, part, M, cols)
        ops.gather_rows(mid, back, unpart, part.numel(), cols)
        torch.cuda.synchronize()
        assert torch.equal(back[0].view(torch.int16), src[0].view(torch.int16)) and torch.equal(back[1].view(torch.int16), src[1].view(torch.int16))


@pytest.mark.parametrize("form", ["separate", "ilv"])
def test_all_pad_identity_and_out_of_range(dev, form):
    cols, M = 128, 37
    src = (_bits(M, cols, dev, 11), _bits(M, cols, dev, 12))
    allpad = torch.full((50,), -1, dtype=torch.int32, device=dev)
    for got, _ in _gather(src, allpad, cols, form, dev):
        assert int((got != 0).sum()) == 0
    ident = torch.arange(M, dtype=torch.int32, device=dev)
    for got, s in _gather(src, ident, cols, form, dev):
        assert torch.equal(got, s.view(torch.int16))
    beyond = torch.tensor([0, M - 1, M, 1 << 30, -5], dtype=torch.int32, device=dev)  # an index >= rows_in is a zero row, never a read
    for got, s in _gather(src, beyond, cols, form, dev):
        assert torch.equal(got[:2], s.view(torch.int16)[[0, M - 1]]) and int((got[2:] != 0).sum()) == 0


def test_single_array_and_strided_rows(dev):
    """lo = None on both sides; rows as column slices of wider arrays: the columns outside stay as they were."""
    from mvp import ops

    cols, M = 128, 20
    wide_in, wide_out = _bits(M, 256, dev, 21), _bits(30, 192, dev, 22)
    keep = wide_out.clone()
    idx = torch.randint(-1, M, (30,), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(dev)
    ops.gather_rows((wide_in[:, 64:192], None), (wide_out[:, 32:160], None), idx, M, cols, ld_in=256, ld_out=192)
    torch.cuda.synchronize()
    keep.view(torch.int16)[:, 32:160] = _want(wide_in[:, 64:192].contiguous(), idx)
    assert torch.equal(wide_out.view(torch.int16), keep.view(torch.int16))
