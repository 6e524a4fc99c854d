"""The two host policies of mvp/pipeline.py, held to tests/golden/pipeline_policy.json (recorded by tests/golden/make_goldens_pipeline.py
from the code BEFORE the policies were gathered into ``_plan`` and ``_Feeder``): which shape a pipeline takes for a request, a backbone
and a batch shape, and how a stream of batches is cut into forwards.  No device: the recorder's stand-ins replace the streams."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_goldens_pipeline as rec  # noqa: E402  (puts midvision-probe_amd on the path)
from mvp import pipeline  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(rec.OUT) as f:
        return json.load(f)


def _row(golden, **want):
    """The recorded row of the product for one combination of PLAN_AXES (axes not named: None / grouping on)."""
    kw = dict(dict(depth=None, group=None, span=None, streams=None, ungrouped_depth=None, grouping=True), **want)
    return golden["plans"]["product"][[tuple(r.values()) for r in rec.rows(rec.PLAN_AXES)].index(tuple(kw[a] for a in rec.PLAN_AXES))]


def test_the_fixture_holds_what_was_read_off_the_code_before(golden):
    """Guards against a recorder that is wired wrong: values read off the earlier code by hand."""
    assert golden["plans"]["columns"] == ["depth", "chains", "group", "span", "span_batch", "streams", "graphs"]
    assert len(golden["plans"]["product"]) == 4 * 5 * 3 * 4 * 3 * 2 * 2
    assert _row(golden, shape=(16, 3, 224, 224))[:6] == [2, 1, 7, 110, 16, 1]
    assert _row(golden, shape=(16, 3, 480, 640))[:6] == [4, 3, 1, 0, 0, 3]
    assert _row(golden, shape=(16, 3, 480, 640), ungrouped_depth=1)[:6] == [1, 1, 1, 0, 0, 0]
    assert _row(golden, shape=(64, 3, 224, 224))[2:4] == [2, 104]
    assert _row(golden, shape=(16, 3, 224, 224), depth=4)[:4] == [4, 1, 6, 0]
    small = _row(golden, shape=(4, 3, 64, 80), depth=2, span=7, streams=2)
    assert (small[1], small[3]) == (2, 0)
    assert golden["plans"]["rebinds"][0][2][:6] == [4, 3, 1, 0, 0, 3]
    assert [s[:-1] for s in golden["feeds"]["spans_10_of_4"]["submissions"]] == [
        ["span", [4, 4, 2], [0, 1, 2], 4], ["span", [2, 4, 4], [2, 3, 4], 4], ["span", [4, 4, 2], [5, 6, 7], 4], ["span", [2, 4], [7, 8], 4]]
    assert [s[-1] for s in golden["feeds"]["spans_10_of_4"]["submissions"]] == [0, 2, 0, 2]
    closed = golden["feeds"]["spans_closed_after_three"]
    assert closed["drained"] == 1 and closed["pulled_after_close"] == closed["pulled_when_closed"]


def test_every_recorded_plan_and_rebind_is_reproduced(golden):
    """Through the public calls the recorder used: FeaturePipeline(...), resolve_group, rebind."""
    now = rec.record_plans()
    assert now["rebinds"] == golden["plans"]["rebinds"]
    assert now["env"] == golden["plans"]["env"]
    wrong = [(kw, got, want) for kw, got, want in zip(rec.rows(rec.PLAN_AXES), now["product"], golden["plans"]["product"]) if got != want]
    assert not wrong, f"{len(wrong)} plans differ, the first: {wrong[0]}"


def _direct(kw):
    kw = dict(kw)
    shape, model = kw.pop("shape"), rec.StubModel(kw.pop("grouping"))
    return list(pipeline._plan(pipeline._Request(**kw), model, shape))


def test_the_plan_function_alone_gives_the_recorded_numbers(golden):
    with rec.no_device():
        wrong = [(kw, got, want[:5]) for kw, want in zip(rec.rows(rec.PLAN_AXES), golden["plans"]["product"]) if (got := _direct(kw)) != want[:5]]
    assert not wrong, f"{len(wrong)} plans differ, the first: {wrong[0]}"
    for name, value in rec.ENV_CASES:
        with rec.no_device({name: value}):
            got = [_direct(dict(kw, depth=None, span=None, streams=None)) for kw in rec.rows(rec.ENV_AXES)]
        assert got == [r[:5] for r in golden["plans"]["env"][f"{name}={value}"]], name
    with rec.no_device():
        for kw, seq in zip(rec.REBINDS, golden["plans"]["rebinds"]):
            req = pipeline._Request(None, None, None, None, kw["ungrouped_depth"])
            assert list(pipeline._plan(req, rec.StubModel())) == seq[0][:5]  # before a batch shape is known
            assert [list(pipeline._plan(req, rec.StubModel(), s)) for s in rec.REBIND_SHAPES] == [r[:5] for r in seq[1:]]


@pytest.mark.parametrize("name", list(rec.FEED_CASES))
def test_pipelined_features_cuts_the_stream_as_recorded(golden, name):
    with rec.no_device():
        assert json.loads(json.dumps(rec.feed_row(name))) == golden["feeds"][name]


@pytest.mark.parametrize("name", list(rec.FEED_CASES))
def test_the_feeder_alone_yields_the_recorded_submissions(golden, name):
    """The feeder driven without a pipeline behind it: the forwards do not depend on when they are submitted.  (The case the consumer
    closes early recorded only the forwards submitted until then.)"""
    pipe, batches = rec.feed_inputs(**rec.FEED_CASES[name])
    feeder, got = pipeline._Feeder(pipe, batches), []
    with rec.no_device():
        while (fwd := feeder.next_forward()) is not None:
            done, images, span = fwd
            what = [int(x.shape[0]) for x in images], [int(x.flatten()[0]) for x in images]
            got.append(["group", *what] if span is None else ["span", *what, *span])
            # the batches a forward completes: all of a group; of a span all but a last piece that stops inside its batch
            assert len(done) == (len(images) if span is None else (span[1] + sum(what[0])) // span[0])
            assert [i for _, i in done] == what[1][:len(done)]
    want = golden["feeds"][name]["submissions"]
    assert got[:len(want)] == want and (len(got) == len(want) or "close_after" in rec.FEED_CASES[name])
    assert batches.pulled == len(batches)
