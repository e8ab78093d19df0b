"""`EdgePipeline` (ams_amd/edge_pipeline.py) without a GPU: the ticket bookkeeping over an engine stand-in that logs its calls and tags
every per-frame array with the frame's first pixel.  What is under test is which frame's results a ticket gets and the ORDER of the engine
calls: the engine has one output block, so a pass is fetched before the next one is launched.  Also the flat-arena helpers of weights.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ams_amd import confidence as Cf, weights as Wt
from ams_amd.edge_pipeline import EdgePipeline
from ams_amd.semantic_network import pass_metrics

H, W, K = 2, 4, 3


class _Rows:
    """a pass's statistics rows 'on the device': the copy to the host is logged"""

    def __init__(self, rows, log):
        self.rows, self.log = rows, log

    def cpu(self):
        self.log.append(("rows_to_host", self.rows[:, Cf.OFF_SUM_ALL].tolist()))
        return torch.from_numpy(self.rows)


class _Engine:
    def __init__(self):
        self.log = []

    def predict_frames(self, frames, labels, mode, u8=False):
        assert u8 and mode == "mode" and len(frames) == len(labels)
        self.tags = [int(f[0, 0, 0]) for f in frames]
        assert [int(l[0, 0]) for l in labels] == self.tags, "a frame travels with its own labels"
        self.inputs = (frames, labels)
        self.log.append(("predict_frames", list(self.tags)))
        return np.stack([np.full((H, W), t, np.uint8) for t in self.tags]), None, None

    def last_inputs(self):
        return self.inputs

    def fetch_frames(self):
        self.log.append(("fetch_frames", list(self.tags)))
        return (np.stack([np.full((H, W), t, np.int32) for t in self.tags]), np.stack([_conf(t) for t in self.tags]),
                np.stack([_loss(t) for t in self.tags]))

    def confidence(self, teacher):
        assert teacher is self.inputs[1]
        self.log.append(("confidence", list(self.tags)))
        rows = np.zeros((len(self.tags), Cf.STATS_LEN), dtype=np.int64)
        rows[:, Cf.OFF_SUM_ALL] = self.tags
        return np.stack([np.full((H, W), 100 + t, np.uint8) for t in self.tags]), None, _Rows(rows, self.log)

    def calls(self, name):
        return [entry for entry in self.log if entry[0] == name]


def _conf(t):
    return np.arange(K * K, dtype=np.int64).reshape(K, K) * t + np.eye(K, dtype=np.int64)


def _loss(t):
    return np.array([3.0 * t, 2.0])


def _frame(t):
    return np.full((1, H, W, 3), t, np.uint8), np.full((1, H, W), t, np.uint8)


def _pipeline(depth=3):
    eng = _Engine()

    def render(frames, student, teacher, views):
        assert int(frames[0, 0, 0, 0]) == int(student[0, 0, 0]) == int(teacher[0, 0, 0]) and len(frames) == 1
        eng.log.append(("render", int(frames[0, 0, 0, 0]), tuple(views)))
        return {v: (v, int(student[0, 0, 0])) for v in views}

    return EdgePipeline(eng, "mode", depth, lambda: SimpleNamespace(render=render), pass_metrics, K), eng


def _is_result_of(result, t):
    labels, *metrics = result
    assert len(result) == 5 and labels.shape == (1, H, W) and labels.dtype == np.int32 and (labels == t).all()
    for got, want in zip(metrics, pass_metrics(_conf(t), _loss(t))):
        assert type(got) is type(want) and np.array_equal(got, want, equal_nan=True)
    assert metrics[3] == np.float32(1.5 * t)


def test_depth_frames_make_one_pass_in_ticket_order():
    pipe, eng = _pipeline(3)
    tickets = [pipe.submit(*_frame(t)) for t in (7, 5, 9)]
    assert tickets == [1, 2, 3] and eng.log == [("predict_frames", [7, 5, 9])]          # launched, nothing fetched yet
    for ticket, t in ((3, 9), (1, 7), (2, 5)):                                          # any order: each its own
        _is_result_of(pipe.collect(ticket), t)
    assert eng.log == [("predict_frames", [7, 5, 9]), ("fetch_frames", [7, 5, 9])]      # one copy for the whole pass
    with pytest.raises(AssertionError, match="unknown ticket"):
        pipe.collect(1)                                                                 # handed over already
    with pytest.raises(AssertionError, match="unknown ticket"):
        pipe.collect(17)


def test_collecting_a_queued_ticket_launches_the_partial_pass():
    pipe, eng = _pipeline(3)
    a, b = pipe.submit(*_frame(4)), pipe.submit(*_frame(6))
    assert eng.log == []
    _is_result_of(pipe.collect(b), 6)
    assert eng.log == [("predict_frames", [4, 6]), ("fetch_frames", [4, 6])]
    _is_result_of(pipe.collect(a), 4)
    assert len(eng.log) == 2
    # ... and so does taking its views or its confidence
    c = pipe.submit(*_frame(8), render=("cross_mask",))
    assert pipe.take_rendered(c) == {"cross_mask": ("cross_mask", 8)}
    d = pipe.submit(*_frame(2), confidence=True)
    assert pipe.take_confidence(d).stats[0].sum_all == 2
    assert [e[1] for e in eng.calls("predict_frames")] == [[4, 6], [8], [2]]


def test_a_second_launch_fetches_the_pending_pass_first():
    pipe, eng = _pipeline(2)
    first = [pipe.submit(*_frame(t)) for t in (1, 2)]
    second = [pipe.submit(*_frame(t)) for t in (3, 4)]
    assert eng.log == [("predict_frames", [1, 2]), ("fetch_frames", [1, 2]), ("predict_frames", [3, 4])]
    for ticket, t in zip(first + second, (1, 2, 3, 4)):
        _is_result_of(pipe.collect(ticket), t)
    assert eng.log[3:] == [("fetch_frames", [3, 4])]


def test_drain_keeps_the_pending_tickets_collectable():
    pipe, eng = _pipeline(2)
    tickets = [pipe.submit(*_frame(t)) for t in (5, 6)]
    pipe.drain()                                   # what a synchronous call does before it writes the output block
    pipe.drain()                                   # nothing pending any more: no second fetch
    assert eng.log == [("predict_frames", [5, 6]), ("fetch_frames", [5, 6])]
    eng.tags = [99]                                # the synchronous call's own pass
    _is_result_of(pipe.collect(tickets[1]), 6)
    _is_result_of(pipe.collect(tickets[0]), 5)
    assert len(eng.log) == 2


def test_views_and_confidence_only_where_asked_and_once():
    pipe, eng = _pipeline(3)
    plain = pipe.submit(*_frame(1))
    both = pipe.submit(*_frame(2), render=("colour_student", "cross_mask"), confidence=True)
    sure = pipe.submit(*_frame(3), confidence=True)
    # behind the pass: the views of the one ticket that asked, then ONE confidence launch for the pass
    assert eng.log == [("predict_frames", [1, 2, 3]), ("render", 2, ("colour_student", "cross_mask")), ("confidence", [1, 2, 3])]
    assert pipe.take_rendered(both) == {"colour_student": ("colour_student", 2), "cross_mask": ("cross_mask", 2)}
    for ticket, t in ((sure, 3), (both, 2)):
        conf = pipe.take_confidence(ticket)
        assert conf.map.shape == (1, H, W) and (conf.map == 100 + t).all()
        assert len(conf.stats) == 1 and conf.stats[0].sum_all == t and conf.stats[0].n_classes == K
    assert eng.calls("rows_to_host") == [("rows_to_host", [1, 2, 3])]                    # the pass's rows, once for all its tickets
    assert not eng.calls("fetch_frames")                                                # taking needs no fetch
    for take, ticket, message in ((pipe.take_rendered, both, "no views were requested"), (pipe.take_confidence, both, "no confidence was requested"),
                                  (pipe.take_rendered, plain, "no views were requested"), (pipe.take_confidence, plain, "no confidence was requested"),
                                  (pipe.take_rendered, sure, "no views were requested"), (pipe.take_confidence, 17, "no confidence was requested")):
        with pytest.raises(AssertionError, match=message):
            take(ticket)
    for ticket, t in ((plain, 1), (both, 2), (sure, 3)):                                 # before or after collect
        _is_result_of(pipe.collect(ticket), t)


def test_flush_leaves_nothing_queued_or_pending():
    pipe, eng = _pipeline(3)
    tickets = [pipe.submit(*_frame(t)) for t in (1, 2, 3, 4)]          # a pass on the GPU and one frame queued
    pipe.flush()
    assert eng.log == [("predict_frames", [1, 2, 3]), ("fetch_frames", [1, 2, 3]), ("predict_frames", [4]), ("fetch_frames", [4])]
    assert not pipe._queued and not pipe._pending
    pipe.flush()
    assert len(eng.log) == 4
    for ticket, t in zip(tickets, (1, 2, 3, 4)):
        _is_result_of(pipe.collect(ticket), t)
    assert len(eng.log) == 4
    kept = pipe.submit(*_frame(5), render=("cross_mask",), confidence=True)
    pipe.flush()
    pipe.clear()
    with pytest.raises(AssertionError, match="no views were requested"):
        pipe.take_rendered(kept)


def test_torch_frames_are_concatenated_as_tensors():
    pipe, eng = _pipeline(2)
    for t in (3, 4):
        pipe.submit(*(torch.from_numpy(x) for x in _frame(t)))
    assert isinstance(eng.inputs[0], torch.Tensor) and tuple(eng.inputs[0].shape) == (2, H, W, 3) and eng.tags == [3, 4]


# ---------------------------------------------------------------------------------------------------- flat arenas
def test_split_flat_and_fill_flat_round_trip():
    var = lambda name, shape, offset, trainable: SimpleNamespace(name=name, shape=shape, size=int(np.prod(shape)), offset=offset, trainable=trainable)  # noqa: E731
    trainable = [var("a/weights:0", (2, 3), 0, True), var("a/gamma:0", (3,), 6, True), var("b/weights:0", (1, 1, 2, 2), 9, True)]
    stats = [var("a/moving_mean:0", (3,), 0, False), var("a/moving_variance:0", (3,), 3, False)]
    order = ["a/weights:0", "a/gamma:0", "a/moving_mean:0", "a/moving_variance:0", "b/weights:0"]
    spec = SimpleNamespace(trainable=trainable, stats=stats, n_trainable=13, n_stats=6, by_name={v.name: v for v in trainable + stats},
                           all_variable_names=lambda: order)
    rng = np.random.default_rng(0)
    values = {v.name: rng.standard_normal(v.shape).astype(np.float32) for v in trainable + stats}
    flat_t, flat_s = np.full(13, np.nan, np.float32), np.full(6, np.nan, np.float32)
    Wt.fill_flat(flat_t, trainable, values)
    Wt.fill_flat(flat_s, stats, values)
    assert np.array_equal(flat_t, Wt.pack_trainable(spec, values)) and np.array_equal(flat_s, Wt.pack_stats(spec, values))
    unpacked = Wt.unpack(spec, flat_t, flat_s)
    assert list(unpacked) == order
    for v, part in list(zip(trainable, Wt.split_flat(flat_t, trainable))) + list(zip(stats, Wt.split_flat(flat_s, stats))):
        assert part.shape == v.shape and np.array_equal(part, values[v.name]) and np.array_equal(part, unpacked[v.name])
        assert np.shares_memory(part, flat_t if v.trainable else flat_s) and not np.shares_memory(unpacked[v.name], part)      # views; unpack copies
    # any shape of the right size, cast to the arena's dtype; a subset of the variables leaves the rest alone
    mask = np.zeros(13, dtype=np.uint8)
    Wt.fill_flat(mask, trainable[1:], {"a/gamma:0": np.array([True, False, True]), "b/weights:0": np.ones(4, dtype=bool)})
    assert mask.tolist() == [0] * 6 + [1, 0, 1] + [1] * 4
    with pytest.raises(KeyError):
        Wt.fill_flat(mask, trainable, {"a/gamma:0": np.ones(3)})
    with pytest.raises(ValueError):
        Wt.pack_trainable(spec, dict(values, **{"a/gamma:0": np.ones((1, 3), np.float32)}))
