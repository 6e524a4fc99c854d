"""Host logic of a ViT forward that needs no GPU: which buffers an engine keeps alive (mvp/buffers.py: one shape resident per kind, two
pipeline namespaces, one carry store per stream, what a captured graph's snapshot holds) and the span arithmetic of
``ViTEngine.forward_taps`` (mvp.vit.plan_taps).  The store takes its allocations as callables, so plain dicts stand for device buffers."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "midvision-probe_amd"))

from mvp import lib, pipeline  # noqa: E402
from mvp.buffers import EngineBuffers  # noqa: E402
from mvp.vit import plan_taps  # noqa: E402

A, B = (16, 14, 14), (16, 30, 40)  # two resolutions: 224^2 and 480x640 at patch 16
TAPS = (4,)
LAYERS = ((2, 5, 8, 11), False)


_SERIAL = itertools.count()


def new(headroom=0):
    return lambda: {"headroom": headroom, "serial": next(_SERIAL)}  # (distinct stand-ins compare unequal)


def never():
    raise AssertionError("the store allocated for buffers it should still hold")


def holds(snapshot, buf) -> bool:
    return any(b is buf for b in snapshot)


def forward(st, shape, G=1, stream=None, headroom=0):
    """The requests of one forward, in forward_taps' order: workspace, carry store (span forwards), packings, output maps."""
    ws = st.workspace(shape, headroom, new(headroom))
    carry = st.carry(stream, shape + TAPS, new()) if stream is not None else None
    return ws, carry, st.packings(shape + TAPS, G, new()), st.outputs(shape + LAYERS, G, new())


def test_one_resolution_resident_per_kind_on_every_slot():
    st = EngineBuffers()
    ws, _, packs, outs = forward(st, A)
    assert st.workspace(A, 0, never) is ws and st.packings(A + TAPS, 1, never) is packs and st.outputs(A + LAYERS, 1, never) is outs
    snap = st.snapshot(0)
    assert all(holds(snap, b) for b in (ws, packs, outs)) and len(snap) == 3
    ws_b = st.workspace(B, 0, new())
    now = st.snapshot(0)
    assert holds(now, ws_b) and not holds(now, ws)            # the other resolution's workspace went ...
    assert holds(now, packs) and holds(now, outs)             # ... each kind by its own shape: these go when THEIR shape changes
    st.packings(B + TAPS, 1, new()), st.outputs(B + LAYERS, 1, new())
    assert not holds(st.snapshot(0), packs) and not holds(st.snapshot(0), outs) and len(st.snapshot(0)) == 3
    assert all(holds(snap, b) for b in (ws, packs, outs))     # a snapshot taken earlier (a captured graph's) still holds its buffers
    assert st.workspace(A, 0, new()) is not ws                # back to the first resolution: allocated anew
    assert st.outputs(A + ((2, 5), False), 1, new()) and len(st.snapshot(0)) == 3   # other layers / want_cls: another shape of outputs
    # "on every slot": two slots of one pipeline hold A; slot 0 meets B, and slot 1's A buffers go too
    st = EngineBuffers()
    with pipeline._slot((1, 0)):
        forward(st, A)
    with pipeline._slot((1, 1)):
        held = forward(st, A)
    with pipeline._slot((1, 0)):
        forward(st, B)
    assert st.snapshot((1, 1)) == [] and len(st.snapshot((1, 0))) == 3 and not any(holds(st.snapshot((1, 0)), b) for b in held)
    with pipeline._slot((1, 1)):                               # slots of one shape live side by side
        forward(st, B)
    assert len(st.snapshot((1, 1))) == 3 and len(st.snapshot((1, 0))) == 3 and st.snapshot(0) == []


def test_two_most_recently_used_namespaces_survive():
    st = EngineBuffers()
    plain = forward(st, A)                                     # slot 0 (no pipeline) belongs to no namespace: never evicted by one
    sets = {}
    for ns in (1, 2, 3):
        with pipeline._slot((ns, 0)):
            sets[ns] = forward(st, A, G=6, stream=ns)
    assert st.snapshot((1, 0)) == [sets[2][1], sets[3][1]]                    # nothing of namespace 1 is left, its carry store included
    for ns in (2, 3):
        snap = st.snapshot((ns, 0))
        assert all(holds(snap, b) for b in sets[ns]) and len(snap) == 3 + 2
    assert all(holds(st.snapshot(0), b) for b in plain if b is not None)
    # least recently USED, not oldest: 2 is touched again before 4 arrives, so 3 goes
    with pipeline._slot((2, 0)):
        assert forward(st, A, G=6, stream=2)[0] is sets[2][0]
    with pipeline._slot((4, 0)):
        forward(st, A, G=6, stream=4)
    assert holds(st.snapshot((2, 0)), sets[2][0]) and not any(holds(st.snapshot((3, 0)), b) for b in sets[3])


def test_headroom_increase_replaces_the_workspace_only():
    st = EngineBuffers()
    with pipeline._slot((1, 1)):
        other = st.workspace(A, 0, new(0))
    with pipeline._slot((1, 0)):
        ws0 = st.workspace(A, 0, new(0))
        packs = st.packings(A + TAPS, 6, new())
        before = st.snapshot((1, 0))
        ws16 = st.workspace(A, 16, new(16))                    # a span forward needs head-room in front of x
        assert ws16 is not ws0 and ws16["headroom"] == 16
        assert st.workspace(A, 0, never) is ws16 and st.workspace(A, 16, never) is ws16   # enough head-room serves a smaller request
        after = st.snapshot((1, 0))
    assert holds(before, ws0) and not holds(after, ws0) and holds(after, ws16) and holds(after, packs)
    assert holds(st.snapshot((1, 1)), other)                   # same shape, other slot: untouched


def test_two_group_sizes_of_one_shape_stay():
    st = EngineBuffers()
    with pipeline._slot((1, 0)):
        p6, o6 = st.packings(A + TAPS, 6, new()), st.outputs(A + LAYERS, 6, new())
        p7, o7 = st.packings(A + TAPS, 7, new()), st.outputs(A + LAYERS, 7, new())   # a span pipeline completes 6 or 7 batches per forward
        assert p7 is not p6 and o7 is not o6
        assert st.packings(A + TAPS, 6, never) is p6 and st.outputs(A + LAYERS, 6, never) is o6
        assert st.packings(A + TAPS, 7, never) is p7 and st.outputs(A + LAYERS, 7, never) is o7
        st.packings(A + (2,), 6, new())                        # another tap count is another shape: both G go
        snap = st.snapshot((1, 0))
    assert not holds(snap, p6) and not holds(snap, p7) and holds(snap, o6) and holds(snap, o7)


def test_a_stream_that_changes_shape_drops_its_carry_store():
    st = EngineBuffers()
    for ns in (5, 6):
        with pipeline._slot((ns, 0)):
            st.workspace(A, 16, new(16))
    c5, c6 = st.carry(5, A + TAPS, new()), st.carry(6, A + TAPS, new())
    assert st.carry(5, A + TAPS, never) is c5 and st.carry(6, A + TAPS, never) is c6
    c5b = st.carry(5, B + TAPS, new())
    snap = st.snapshot((5, 0))
    assert not holds(snap, c5) and holds(snap, c5b) and holds(snap, c6)    # one store per stream; the other stream keeps its own
    assert holds(st.snapshot("any slot"), c6)                               # carry stores are part of every slot's snapshot


def test_snapshot_is_a_list_of_its_own():
    st = EngineBuffers()
    ws = st.workspace(A, 0, new())
    snap = st.snapshot(0)
    st.workspace(B, 0, new())
    assert snap == [ws] and snap is not st.snapshot(0)


def test_plan_taps_span_arithmetic():
    assert plan_taps(96, 6) == (6, 16, 0, 0) and plan_taps(16, 1) == (1, 16, 0, 0)
    assert plan_taps(110, pipeline.Span(16, 0)) == (6, 16, 0, 14)
    assert plan_taps(110, pipeline.Span(16, 14, 3)) == (7, 16, 14, 12)
    for B_ in (1, 4, 16, 64):
        for carry in range(B_):
            for Bt in range(1, 3 * B_ + 2):
                if carry + Bt < B_:
                    continue
                G, b, c, tail = plan_taps(Bt, pipeline.Span(B_, carry))
                assert (b, c) == (B_, carry) and G >= 1 and 0 <= tail < B_ and carry + Bt == G * B_ + tail
    # consecutive spans of a stream: each one's tail is the next one's carry (pipeline.span_patterns)
    carry = 0
    for slot, expect in pipeline.span_patterns(110, 16):
        assert carry == expect
        carry = plan_taps(110, pipeline.Span(16, carry))[3]
    assert carry == 0


def test_plan_taps_errors():
    with pytest.raises(lib.MvpError, match=r"^grouped forward: 96 images do not split into 7 equal batches$"):
        plan_taps(96, 7)
    with pytest.raises(lib.MvpError, match=r"^grouped forward: 96 images do not split into 0 equal batches$"):
        plan_taps(96, 0)
    with pytest.raises(lib.MvpError, match=r"^span forward: carry 16 outside \[0, 16\)$"):
        plan_taps(110, pipeline.Span(16, 16))
    with pytest.raises(lib.MvpError, match=r"^span forward: carry -1 outside \[0, 16\)$"):
        plan_taps(110, pipeline.Span(16, -1))
    with pytest.raises(lib.MvpError, match=r"^span forward: 3 \+ 5 images complete no batch of 16$"):
        plan_taps(5, pipeline.Span(16, 3))
