"""Host logic of mvp/evalloop.py, the loop the sharded evaluations share: the sharding rule and its two older names, the graph-replay
policy, the feature generator over a stub model (the pattern of tests/test_pipeline_cpu.py), the end-of-loop exchange in a single
process and the re-ordering of gathered rows.  No device, no native library."""
import pytest
import torch


def test_shard_partitions_the_range():
    from mvp import evalloop

    for n in range(8):
        for world in range(1, 5):
            shards = [evalloop.shard(n, r, world) for r in range(world)]
            assert all(isinstance(s, list) for s in shards)
            assert sorted(i for s in shards for i in s) == list(range(n)), (n, world)  # every item once
            assert all(s == list(range(r, n, world)) for r, s in enumerate(shards)), (n, world)  # rank r: r, r + W, ...
            assert max(len(s) for s in shards) - min(len(s) for s in shards) <= 1


def test_the_older_names_are_the_same_function():
    from mvp import evalloop, percept, spair

    assert spair.shard_pairs is percept.shard_batches is evalloop.shard
    assert percept.PinnedRing is evalloop.PinnedRing and not hasattr(spair, "_PinnedRing")  # one staging ring, public, in one place


def test_graph_policy(monkeypatch):
    from mvp import evalloop

    monkeypatch.delenv("MVP_PIPELINE_GRAPHS", raising=False)
    assert evalloop.graph_policy(1) is None
    assert evalloop.graph_policy(2) is True and evalloop.graph_policy(8) is True
    for value in ("0", "1"):  # set: the pipeline reads the variable itself
        monkeypatch.setenv("MVP_PIPELINE_GRAPHS", value)
        assert evalloop.graph_policy(1) is None and evalloop.graph_policy(2) is None


class _Stub(torch.nn.Module):
    """Returns tensors it keeps, so that a test can tell a handed-on object from a copy."""

    def __init__(self, multilayer):
        super().__init__()
        self.multilayer, self.outputs = multilayer, []

    def forward(self, x):
        out = [x * 2.0, x * 3.0, x * 4.0] if self.multilayer else x * 2.0
        self.outputs.append(out)
        return out


def _items(n):
    for i in range(n):
        yield {"image": torch.full((2, 3, 1, 2), float(i)), "meta": i}


@pytest.mark.parametrize("world", [1, 2])
def test_features_hands_a_tensor_on_and_concatenates_a_list(world, monkeypatch):
    from mvp import evalloop, pipeline

    monkeypatch.delenv("MVP_PIPELINE_GRAPHS", raising=False)
    monkeypatch.setattr(pipeline, "_extract", lambda model, images: model(images))  # (extract_features detaches: a new tensor object)
    single = _Stub(multilayer=False)
    got = list(evalloop.features(single, _items(5), world))
    assert [item["meta"] for item, _ in got] == [0, 1, 2, 3, 4]  # item order
    assert len(single.outputs) == 5 and all(f is out for (_, f), out in zip(got, single.outputs))  # the same object: no copy
    assert all(torch.equal(f.cpu(), item["image"] * 2.0) for item, f in got)  # (.cpu(): with a device present the pipeline moves the images there)

    multi = _Stub(multilayer=True)
    got = list(evalloop.features(multi, _items(4), world))
    assert [item["meta"] for item, _ in got] == [0, 1, 2, 3]
    for (item, f), out in zip(got, multi.outputs):
        assert f.shape == (2, 9, 1, 2) and torch.equal(f, torch.cat(out, dim=1))
        assert torch.equal(f[:, 3:6].cpu(), item["image"] * 3.0)


def test_features_through_extract_features_shares_the_output_storage():
    """Unpatched: mvp.train.extract_features detaches the output, which is a view of the same memory, not a copy."""
    from mvp import evalloop

    single = _Stub(multilayer=False)
    got = list(evalloop.features(single, _items(3), 1))
    assert all(f.data_ptr() == out.data_ptr() and not f.requires_grad for (_, f), out in zip(got, single.outputs))


def test_gather_parts_in_a_single_process_never_touches_torch_distributed():
    import torch.distributed as dist

    from mvp import evalloop

    assert not (dist.is_available() and dist.is_initialized())
    local = [(0, torch.arange(3)), (1, torch.arange(2))]
    parts = evalloop.gather_parts(local, 1)
    assert len(parts) == 1 and parts[0] is local
    shard_result = ([(0, [{"id": 0}])], [1, 2, 3, 4], ["an error"])  # what percept.predict_batch exchanges: not a list of rows
    assert evalloop.gather_parts(shard_result, 1) == [shard_result]
    assert evalloop.gather_parts([], 1) == [[]]
    with pytest.raises((RuntimeError, ValueError)):  # more than one rank needs an initialised process group
        evalloop.gather_parts(local, 2)


def test_in_index_order_restores_dataset_order():
    from mvp import evalloop

    n, world = 7, 3
    parts = [[(i, f"row {i}", float(i) / 2) for i in evalloop.shard(n, r, world)] for r in range(world)]
    assert [row[0] for row in parts[1]] == [1, 4]  # interleaved over the ranks
    assert evalloop.in_index_order(parts) == [(i, f"row {i}", float(i) / 2) for i in range(n)]
    # more ranks than rows: ranks 2 and 3 hold nothing
    parts = [[(i, "x") for i in evalloop.shard(2, r, 4)] for r in range(4)]
    assert parts[2] == [] and parts[3] == []
    assert evalloop.in_index_order(parts) == [(0, "x"), (1, "x")]
    # NAVI's rows: batches of pairs are sharded, the pair index leads each row
    batches = [[0, 1, 2], [3, 4, 5], [6]]
    parts = [[(i, r) for b in evalloop.shard(len(batches), r, 2) for i in batches[b]] for r in range(2)]
    assert [row[0] for row in parts[0]] == [0, 1, 2, 6]
    assert evalloop.in_index_order(parts) == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1), (5, 1), (6, 0)]
    assert evalloop.in_index_order([]) == [] and evalloop.in_index_order([[]]) == []
