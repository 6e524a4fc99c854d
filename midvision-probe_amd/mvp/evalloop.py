"""What the sharded evaluation loops share (mvp/spair.py, mvp/corr3d.py, mvp/percept.py).  The contract of such a loop:

* rank r takes items r, r + W, ... of the dataset (``shard``); the items are independent of each other;
* no collective is in flight while the loop runs, so its forwards may replay hipGraphs at any world size (``graph_policy``);
* nothing in the loop syncs the host: inputs go through pinned staging (``PinnedRing``), the forwards are kept in flight
  (``features``), the per-item results stay on the device and are fetched after the last forward has been issued;
* one exchange at the end (``gather_parts``), after which every rank holds the result of the whole dataset, in dataset order
  (``in_index_order``), as the reference's single loop produces it."""
from __future__ import annotations

import os
from typing import Iterable, Iterator, List, Tuple

import torch

from .pipeline import pipelined_features


def shard(n: int, rank: int, world: int) -> List[int]:
    """Rank r takes items r, r + W, ... of n: every item once, nothing padded (DistributedSampler would repeat samples, and a
    repeated item changes the counts).  The per-item results are gathered at the end."""
    return list(range(rank, n, world))


def graph_policy(world: int):
    """``graphs`` of ``FeaturePipeline`` for a loop with no collective in flight: True at world > 1, else None (the pipeline's default)."""
    # Jobs with more than one rank launch their forwards eagerly by default (mvp/pipeline.py: a lazy graph capture is a device-wide sync
    # that must not land beside a pending all-reduce).  These loops have NO collective in flight — the one exchange is the gather
    # after them — so they keep hipGraph replay at any world size (eager launches: 48-80 pairs/s against 115-148 at 800^2 in the
    # SPair loop, profiles/r04_fullsize_configs.txt); MVP_PIPELINE_GRAPHS still wins when set.
    return True if (world > 1 and os.environ.get("MVP_PIPELINE_GRAPHS") is None) else None


def features(model, items: Iterable, world: int) -> Iterator[Tuple[object, torch.Tensor]]:
    """Yield ``(item, features)`` for every item of ``items`` (dicts with the input under "image"), the forwards kept in flight by
    mvp.pipeline under ``graph_policy(world)``.  The maps of a multi-layer output are concatenated on dim 1; a single tensor is handed
    on as it is, a view of the slot's buffer that later forwards overwrite: ``.clone()`` it to keep it beyond the next item."""
    for item, feats in pipelined_features(model, items, graphs=graph_policy(world)):
        yield item, (torch.cat(list(feats), dim=1) if isinstance(feats, (list, tuple)) else feats)


def gather_parts(local, world: int) -> list:
    """The loop's one exchange: every rank's ``local`` (host-side, picklable), by rank.  A single process never touches
    torch.distributed."""
    if world == 1:
        return [local]
    import torch.distributed as dist

    parts = [None] * world
    dist.all_gather_object(parts, local)
    return parts


def in_index_order(parts) -> list:
    """The rows of all parts, ordered by each row's leading index: dataset order, as the reference's single loop."""
    return sorted((row for part in parts for row in part), key=lambda row: row[0])


class PinnedRing:
    """Host -> device staging through a few reused pinned buffers: the copy engine moves them asynchronously, where a pageable
    ``.to(device)`` blocks the host until the copy has run (and with it the whole look-ahead of the pipeline)."""

    def __init__(self, slots: int):
        self.slots, self.k = [dict() for _ in range(max(2, slots))], 0

    def to_device(self, parts, dev, dtype=torch.float32) -> torch.Tensor:
        """torch.stack(parts) on the device."""
        slot = self.slots[self.k % len(self.slots)]
        self.k += 1
        shape = (len(parts),) + tuple(parts[0].shape)
        ev = slot.get("event")
        if ev is not None:
            ev.synchronize()  # the copy that last read this pinned buffer has finished (normally long ago)
        buf = slot.get("buf")
        if buf is None or tuple(buf.shape) != shape or buf.dtype != dtype:
            buf = slot["buf"] = torch.empty(shape, dtype=dtype).pin_memory()
        torch.stack([p.to(dtype) for p in parts], out=buf)
        out = torch.empty(shape, dtype=dtype, device=dev)
        out.copy_(buf, non_blocking=True)
        slot["event"] = torch.cuda.Event()
        slot["event"].record()
        return out
