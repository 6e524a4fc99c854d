"""What a ViTEngine keeps alive between forwards, and the one place that decides when it goes.

A frozen forward reuses its buffers: activation workspaces, token-major feature packings, the output maps of pipelined forwards, the
carry store of a span's cut batch.  Each set belongs to a slot — ``pipeline.current_slot()``: 0 outside a pipeline, (pipeline namespace,
slot index) inside: every FeaturePipeline owns its buffer sets, so two pipelines over one backbone (a training loop suspended with
forwards in flight, a validation pass) never write each other's.  The rules, each written once below:
  * one shape resident per kind (``_get``): asking for a shape the engine does not hold drops that kind's buffers of every OTHER shape,
    on every slot; variants of the held shape stay (the G of a packing or an output set: a span pipeline cycles through two);
  * the two most recently used namespaces keep their sets (``_touch``): a loop that builds a new pipeline per epoch would otherwise
    pile them up (a captured graph holds on to its own slot's buffers whatever happens here: ``snapshot``);
  * one carry store per image stream (``carry``).
No device calls here: allocations come in as callables, so the rules run on plain objects (tests/test_vit_buffers_cpu.py).
"""
from . import pipeline


class EngineBuffers:
    def __init__(self):
        self._held = {}  # kind -> (shape, {(variant, slot): buffers}): all entries of a kind have ONE shape
        self._namespaces = []  # pipeline namespaces, least recently used first
        self._carry = {}  # image stream -> (shape, store)

    def _touch(self, slot) -> None:
        ns = slot[0] if isinstance(slot, tuple) else None
        if ns is None or self._namespaces[-1:] == [ns]:
            return
        if ns in self._namespaces:
            self._namespaces.remove(ns)
        self._namespaces.append(ns)
        dead, self._namespaces = self._namespaces[:-2], self._namespaces[-2:]
        for kind, (shape, entries) in self._held.items():
            self._held[kind] = (shape, {(v, s): buf for (v, s), buf in entries.items() if not (isinstance(s, tuple) and s[0] in dead)})

    def _get(self, kind: str, shape: tuple, variant, alloc, stale=None):
        slot = pipeline.current_slot()
        self._touch(slot)
        held_shape, entries = self._held.get(kind, (None, {}))
        buf = entries.get((variant, slot)) if held_shape == shape else None
        if buf is None or (stale is not None and stale(buf)):
            buf = alloc()
            if held_shape != shape:
                entries = {}  # keep one resolution resident: the sets of the other shape go, on every slot
            entries[(variant, slot)] = buf
            self._held[kind] = (shape, entries)
        return buf

    def workspace(self, shape: tuple, headroom: int, alloc) -> dict:
        """The activation workspace of forwards over ``shape`` = (images, gh, gw); one with less ``headroom`` than asked is replaced.
        (Scratch that depends on more than the shape lives INSIDE the dict, ``("bn_ws", G)``, and goes with it.)"""
        return self._get("workspace", shape, None, alloc, stale=lambda ws: ws["headroom"] < headroom)

    def packings(self, shape: tuple, G: int, alloc) -> list:
        """The G feature packings of a forward whose batches have ``shape`` = (B, gh, gw, taps)."""
        return self._get("packings", shape, G, alloc)

    def outputs(self, shape: tuple, G: int, alloc) -> dict:
        """The output maps of a pipelined forward over G batches of ``shape`` = (B, gh, gw, layers, want_cls)."""
        return self._get("outputs", shape, G, alloc)

    def carry(self, stream, shape: tuple, alloc):
        """The carry store of image stream ``stream`` (= its pipeline's namespace) for batches of ``shape`` = (B, gh, gw, taps)."""
        held = self._carry.get(stream)
        if held is None or held[0] != shape:
            self._carry.pop(stream, None)  # the stream changed shape: its old store has no reader left (captured graphs keep theirs alive)
            for s in [s for s in self._carry if s not in self._namespaces]:
                del self._carry[s]  # (streams of pipelines whose buffer sets were dropped too: _touch)
            held = self._carry[stream] = (shape, alloc())
        return held[1]

    def snapshot(self, slot) -> list:
        """The buffer objects held for ``slot`` right now, plus every carry store: a list of its own, which keeps them alive after
        the rules above have dropped or replaced them here (ViTEngine.slot_state)."""
        return ([buf for _, entries in self._held.values() for (_, s), buf in entries.items() if s == slot]
                + [store for _, store in self._carry.values()])
