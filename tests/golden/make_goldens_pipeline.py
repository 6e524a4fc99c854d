"""Records tests/golden/pipeline_policy.json: the two host policies of mvp/pipeline.py, as the code this script is run against decides them.

    python tests/golden/make_goldens_pipeline.py

"plans": the shape FeaturePipeline settles on (depth, chains, group, span, span_batch, number of streams, graphs) for every combination
of constructor arguments, batch shape and backbone ability in PLAN_AXES, for the default-argument rows under each environment variable
in ENV_CASES, and along REBINDS.  "feeds": how pipelined_features cuts a stream of batches into forwards (FEED_CASES), against a stand-in
pipeline that only records what is submitted and in which order the batches come back.

Everything goes through calls that exist on both sides of a change to that file (FeaturePipeline, resolve_group, rebind,
pipelined_features), needs no device (torch.cuda.Stream and torch.cuda.is_available are replaced while recording), and is
deterministic: the file it writes must not change when the policies are only restructured.  tests/test_pipeline_policy_cpu.py imports
the cases and the stand-ins from here."""
import collections
import contextlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "midvision-probe_amd"))

from mvp import pipeline  # noqa: E402

OUT = os.path.join(HERE, "pipeline_policy.json")
ENV = ("MVP_INFLIGHT", "MVP_PIPELINE_GROUP", "MVP_PIPELINE_SPAN", "MVP_PIPELINE_STREAMS", "MVP_PIPELINE_GRAPHS", "MVP_FORCE_DEVICE")

# the product of these, in this order (the fixture stores one result row per combination, in itertools.product order)
PLAN_AXES = collections.OrderedDict(
    shape=[(16, 3, 224, 224), (64, 3, 224, 224), (16, 3, 480, 640), (4, 3, 64, 80)],
    depth=[None, 1, 2, 3, 4],
    group=[None, 1, 3],
    span=[None, 0, 7, 10],
    streams=[None, 1, 2],
    ungrouped_depth=[None, 1],
    grouping=[True, False],
)
# the rows with nothing asked for (group None is what pipelined_features and bench.py pass, 1 the constructor's own default), under each of these
ENV_CASES = [("MVP_INFLIGHT", "3"), ("MVP_PIPELINE_GROUP", "4"), ("MVP_PIPELINE_SPAN", "0"), ("MVP_PIPELINE_SPAN", "96"),
             ("MVP_PIPELINE_STREAMS", "2"), ("MVP_FORCE_DEVICE", "0")]
ENV_AXES = collections.OrderedDict(shape=PLAN_AXES["shape"], group=[None, 1], ungrouped_depth=[None, 1], grouping=[True, False])
# resolve at the first shape, rebind to the second, rebind back
REBINDS = [dict(ungrouped_depth=None), dict(ungrouped_depth=1)]
REBIND_SHAPES = [(16, 3, 224, 224), (16, 3, 480, 640), (16, 3, 224, 224)]


class StubEngine:
    C = 768
    n_prefix = 1


class StubModel:
    """What the plan asks a backbone: ViT-B/16-like, grouping switchable."""
    patch_size, n_prefix, supports_pipelining, graph_safe, training = 16, 1, True, True, False

    def __init__(self, grouping=True):
        self.grouping = grouping

    def supports_grouping(self):
        return self.grouping

    def engine(self):
        return StubEngine()


@contextlib.contextmanager
def no_device(env=()):
    """No stream is created, no device is looked for, 256 CUs, and only ``env`` of the pipeline's environment variables set."""
    saved = (torch.cuda.Stream, torch.cuda.is_available, pipeline._cu_count, {k: os.environ.pop(k, None) for k in ENV})
    torch.cuda.Stream, torch.cuda.is_available, pipeline._cu_count = object, (lambda: False), (lambda: 256)
    os.environ.update(dict(env))
    try:
        yield
    finally:
        torch.cuda.Stream, torch.cuda.is_available, pipeline._cu_count = saved[:3]
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved[3].items() if v is not None})


def state(pipe):
    return [pipe.depth, pipe.chains, pipe.group, pipe.span, pipe.span_batch, len(pipe.streams), int(pipe.graphs)]


def plan_row(shape, grouping, **kwargs):
    pipe = pipeline.FeaturePipeline(StubModel(grouping), **kwargs)
    pipe.resolve_group(torch.empty(shape))
    return state(pipe)


def rows(axes):
    for combo in itertools.product(*axes.values()):
        yield dict(zip(axes, combo))


def record_plans():
    with no_device():
        product = [plan_row(**kw) for kw in rows(PLAN_AXES)]
    env = {}
    for name, value in ENV_CASES:
        with no_device({name: value}):
            env[f"{name}={value}"] = [plan_row(depth=None, **kw) for kw in rows(ENV_AXES)]
    rebinds = []
    with no_device():
        for kw in REBINDS:
            pipe = pipeline.FeaturePipeline(StubModel(), depth=None, group=None, **kw)
            seq = [state(pipe)]  # (as the constructor leaves it)
            pipe.resolve_group(torch.empty(REBIND_SHAPES[0]))
            seq.append(state(pipe))
            for shape in REBIND_SHAPES[1:]:
                pipe.rebind(torch.empty(shape))
                seq.append(state(pipe) + [list(pipe._resolved_for[0])])
            rebinds.append(seq)
    return dict(columns="depth chains group span span_batch streams graphs".split(), product=product, env=env, rebinds=rebinds)


# ---------------------------------------------------------------------------------------------------------------- feeds
class RecordingPipe:
    """What pipelined_features reads of a pipeline; records every submission, hands each batch back with the index of the submission
    that ran it."""

    def __init__(self, depth, group, span, span_batch):
        self.depth, self.group, self.span, self.span_batch = depth, group, span, span_batch
        self.chains = 1 if (span or group > 1) else min(depth, 3)
        self._open, self._queue, self._resolved_for, self._lent = collections.deque(), collections.deque(), None, False
        self.submissions, self.drained = [], 0

    def __len__(self):
        return len(self._queue)

    def free_slots(self):
        return self.depth - len(self._open)

    def resolve_group(self, images):
        if self._resolved_for is None:
            self._resolved_for = (tuple(images.shape), images.dtype)
        return self.group

    def _submitted(self, what, nb):
        assert self.free_slots() > 0 and nb >= 1
        self._queue.extend([len(self.submissions)] * nb)
        self._open.append(nb)
        self.submissions.append(what)

    def submit_group(self, batches):
        self._submitted(["group", [int(b.shape[0]) for b in batches], [int(b.flatten()[0]) for b in batches]], len(batches))

    def submit_span(self, pieces, batch, carry):
        T = sum(int(p.shape[0]) for p in pieces)
        self._submitted(["span", [int(p.shape[0]) for p in pieces], [int(p.flatten()[0]) for p in pieces], int(batch), int(carry)], (carry + T) // batch)

    def next(self):
        self._open[0] -= 1
        if self._open[0] == 0:
            self._open.popleft()
        return self._queue.popleft()

    def drain(self):
        self.drained += 1
        self._queue.clear()
        self._open.clear()


class Loader(list):
    """A list of batches that counts how many were pulled from it."""
    pulled = 0

    def __iter__(self):
        for b in list.__iter__(self):
            self.pulled += 1
            yield b


class LaggedLoader(Loader):
    consumer_lag = 0  # (what mvp.prefetch.DevicePrefetcher offers)


# name: (batch sizes, depth, group, span, span_batch, then options)
FEED_CASES = collections.OrderedDict([
    ("spans_10_of_4", dict(sizes=[4] * 9, depth=2, group=3, span=10, B=4)),
    ("spans_ragged_last_batch", dict(sizes=[4] * 8 + [3], depth=2, group=3, span=10, B=4)),
    ("spans_7_of_4", dict(sizes=[4] * 11, depth=2, group=2, span=7, B=4)),
    ("groups_of_2_three_slots", dict(sizes=[4] * 5, depth=3, group=2, span=0, B=4)),
    ("groups_ragged_batch_inside", dict(sizes=[4, 4, 2, 4, 4], depth=2, group=3, span=0, B=4)),
    ("inline", dict(sizes=[4] * 3, depth=1, group=1, span=0, B=4)),
    ("spans_fifth_batch_taller", dict(sizes=[4] * 8, depth=2, group=3, span=10, B=4, taller=4)),
    ("spans_closed_after_three", dict(sizes=[4] * 9, depth=2, group=3, span=10, B=4, close_after=3)),
    ("spans_consumer_lag", dict(sizes=[4] * 9, depth=2, group=3, span=10, B=4, lagged=True)),
])


def feed_inputs(sizes, depth, group, span, B, taller=None, lagged=False, **_):
    """(stand-in pipeline, batches): batch i is the pair (images [n, 3, 8, 8] filled with i, i)."""
    batches = (LaggedLoader if lagged else Loader)(
        (torch.full((n, 3, 10 if i == taller else 8, 8), float(i)), i) for i, n in enumerate(sizes))
    return RecordingPipe(depth, group, span, B if span else 0), batches


def feed_row(name):
    case = FEED_CASES[name]
    pipe, batches = feed_inputs(**case)
    gen = pipeline.pipelined_features(None, batches, pipe=pipe)
    yielded = []
    for (_, i), sub in gen:
        yielded.append([i, sub])
        if len(yielded) == case.get("close_after"):
            break
    pulled = batches.pulled
    gen.close()
    out = dict(submissions=pipe.submissions, yielded=yielded, drained=pipe.drained)
    if "close_after" in case:
        out["pulled_when_closed"], out["pulled_after_close"] = pulled, batches.pulled
    if case.get("lagged"):
        out["consumer_lag"] = batches.consumer_lag
    return out


def record_feeds():
    with no_device():
        return {name: feed_row(name) for name in FEED_CASES}


def record():
    return dict(plans=record_plans(), feeds=record_feeds())


def dumps(rec) -> str:
    """One line per plan row group and per feed case: small, and a change shows up as a readable diff."""
    lines = ["{", ' "plans": {', '  "columns": ' + json.dumps(rec["plans"]["columns"]) + ",", '  "product": [']
    prod = rec["plans"]["product"]
    per = len(PLAN_AXES["ungrouped_depth"]) * len(PLAN_AXES["grouping"])
    chunks = [prod[i:i + per] for i in range(0, len(prod), per)]
    lines += ["   " + json.dumps(c)[1:-1] + ("," if i + 1 < len(chunks) else "") for i, c in enumerate(chunks)]
    lines += ["  ],", '  "env": {']
    lines += ["   " + json.dumps(k) + ": " + json.dumps(v) + ("," if i + 1 < len(rec["plans"]["env"]) else "") for i, (k, v) in enumerate(rec["plans"]["env"].items())]
    lines += ["  },", '  "rebinds": ' + json.dumps(rec["plans"]["rebinds"]), " },", ' "feeds": {']
    lines += ["  " + json.dumps(k) + ": " + json.dumps(v) + ("," if i + 1 < len(rec["feeds"]) else "") for i, (k, v) in enumerate(rec["feeds"].items())]
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    rec = record()
    text = dumps(rec)
    assert json.loads(text) == json.loads(json.dumps(rec))
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}: {len(text)} bytes")
