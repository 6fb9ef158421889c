"""InFlight (blocks/block_base.py): the calls and staged copies a streaming block keeps in flight, with fake spans and a
backend whose copies land late.  No ring, no GPU."""
import weakref

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd.blocks.block_base import InFlight
from caltech_bifrost_dsp_amd.ndarray import XArray

UNIT = 48


class _Span:
    """An output span: `.data` (nbytes, byte_slice, numpy) and a close() that records when it came and what the span held."""

    def __init__(self, name, events, nbytes=UNIT):
        self.name, self.events = name, events
        self.data = XArray(shape=(nbytes,), dtype=np.uint8, space="system")
        self.closed = 0
        self.seen = None

    def close(self):
        self.closed += 1
        self.seen = self.data.numpy().copy()
        self.events.append(("close", self.name))


class _Backend:
    """Tickets that are waited for, a stream that is synced, and an enqueue-only copy (tests/test_blocks_round4_cpu.py
    _AsyncCopyBackend): one stamp per copy, copy_done false until the copy is completed -- by copy_wait or by land()."""
    space_in = "system"

    def __init__(self, sync_raises=False):
        self.events = []
        self.copies = []
        self.blocked = []               # stamps that copy_wait had to wait for
        self.nsync = 0
        self.sync_raises = sync_raises

    def wait(self, ticket):
        self.events.append(("wait", ticket))

    def sync(self):
        self.nsync += 1
        self.events.append(("sync",))
        if self.sync_raises:
            raise RuntimeError("the stream is gone")

    def copy_async(self, dst, src):
        assert dst.nbytes == src.nbytes
        stamp = {"id": len(self.copies), "dst": dst, "src": src, "done": False, "waited": 0}
        self.copies.append(stamp)
        self.events.append(("copy", stamp["id"]))
        return stamp

    def land(self, stamp):
        if not stamp["done"]:
            stamp["dst"].numpy()[...] = stamp["src"].numpy()        # (the copy lands only now)
            stamp["done"] = True

    def copy_done(self, stamp):
        return stamp["done"]

    def copy_wait(self, stamp):
        stamp["waited"] += 1
        self.events.append(("copy_wait", stamp["id"]))
        if not stamp["done"]:
            self.blocked.append(stamp["id"])
        self.land(stamp)

    def outstanding(self):
        return [c["id"] for c in self.copies if not c["done"]]


def _inflight(be, **kw):
    return InFlight(be.wait, be.sync, be, **kw)


def _staged_call(fl, be, ticket, name, keep, meta=None):
    """One call whose kernel wrote a stage: the stage holds `ticket` in every byte."""
    stage = fl.take_stage(UNIT)
    stage.numpy()[...] = ticket
    sp = _Span(name, be.events)
    fl.push(ticket, sp, object(), stage, meta)
    fl.retire(keep)
    return sp, stage


def _closes(be):
    return [e[1] for e in be.events if e[0] == "close"]


def test_direct_and_staged_spans_finish_once_in_push_order_with_their_data():
    """Direct (D) and staged (S) calls interleaved, two kept in flight, copies that land only when waited for: every span is
    closed exactly once, in push order, and a staged span holds its stage's bytes when it is closed."""
    be = _Backend()
    spans = []
    with _inflight(be) as fl:
        for t, kind in enumerate("DSSDSDDSSSD", 1):
            if kind == "S":
                sp, _ = _staged_call(fl, be, t, "s%d" % t, 2)
            else:
                sp = _Span("s%d" % t, be.events)
                fl.push(t, sp, object())                            # (the three-argument form)
                fl.retire(2)
            spans.append((kind, t, sp))
        fl.retire(0)
    assert _closes(be) == ["s%d" % t for _, t, _ in spans]
    assert [e[1] for e in be.events if e[0] == "wait"] == [t for _, t, _ in spans]
    for kind, t, sp in spans:
        assert sp.closed == 1
        if kind == "S":
            assert np.all(sp.seen == t), (t, sp.seen)
    assert be.nsync == 0 and not be.outstanding() and all(c["waited"] == 1 for c in be.copies)


def test_staged_span_is_not_finished_before_its_copy_has_landed():
    be = _Backend()
    with _inflight(be) as fl:
        sp, _ = _staged_call(fl, be, 7, "a", 0 + 1)                 # still in flight: nothing enqueued
        assert not be.copies and sp.closed == 0
        fl.push(8, None, object())
        fl.retire(1)                                                # a's ticket is done: its copy is enqueued, and may stay
        assert len(be.copies) == 1 and not be.copies[0]["done"] and sp.closed == 0 and np.all(sp.data.numpy() == 0)
        fl.retire(1)                                                # (nothing new: a copy that is not done is left alone)
        assert sp.closed == 0 and not be.blocked
        be.land(be.copies[0])
        fl.retire(1)
        assert sp.closed == 1 and np.all(sp.seen == 7) and not be.blocked
        fl.retire(0)
    assert sp.closed == 1


def test_finish_gets_the_meta_pushed_with_the_span():
    be, got = _Backend(), []
    with _inflight(be, finish=lambda sp, meta: got.append((sp.name, meta))) as fl:
        a = _Span("a", be.events)
        fl.push(1, a, object(), None, ("direct", 1))
        _staged_call(fl, be, 2, "b", 4, meta=("staged", 2))
        three = [_Span(n, be.events) for n in "cde"]
        stage = fl.take_stage(3 * UNIT)
        fl.push(3, three, object(), stage, "three")
        fl.retire(0)
    assert got == [("a", ("direct", 1)), ("b", ("staged", 2)), ("c", "three"), ("d", "three"), ("e", "three")]
    assert not _closes(be)                                          # (finish replaces the default close)


def test_call_without_output_only_holds_its_input_until_its_ticket_is_done():
    class Held:
        pass
    be = _Backend()
    with _inflight(be) as fl:
        held = Held()
        alive = weakref.ref(held)
        fl.push(5, None, held)
        del held
        fl.retire(1)
        assert alive() is not None and ("wait", 5) not in be.events
        fl.retire(0)
        assert alive() is None
    assert be.events == [("wait", 5)]


def test_three_spans_from_one_stage_three_copies_stage_back_after_the_third():
    be = _Backend()
    with _inflight(be, outstanding=8) as fl:
        stage = fl.take_stage(4 * UNIT)                             # (room for four, three completed)
        stage.numpy()[...] = np.repeat(np.arange(1, 5, dtype=np.uint8), UNIT)
        spans = [_Span(n, be.events) for n in "abc"]
        fl.push(1, spans, object(), stage)
        fl.push(2, None, object())
        fl.retire(1)
        assert len(be.copies) == 3 and not _closes(be)
        for k, c in enumerate(be.copies):
            assert c["src"].nbytes == UNIT and c["src"].ptr == stage.ptr + k * UNIT and c["dst"] is spans[k].data
        be.land(be.copies[0])
        be.land(be.copies[1])
        fl.retire(1)
        assert _closes(be) == ["a", "b"]
        other = fl.take_stage(4 * UNIT)
        assert other is not stage                                   # (the third copy still reads it)
        be.land(be.copies[2])
        fl.retire(1)
        assert _closes(be) == ["a", "b", "c"]
        assert fl.take_stage(4 * UNIT) is stage
        fl.retire(0)
    for k, sp in enumerate(spans):
        assert sp.closed == 1 and np.all(sp.seen == k + 1)
    assert not be.blocked


@pytest.mark.parametrize("keep,allowed", [(1, 2), (3, 2), (4, lambda: 6), (2, 0)])
def test_retire_keeps_at_most_the_allowed_copies_and_the_pool_stays_small(keep, allowed):
    """Copies that never complete by themselves: a retire that keeps calls waits for those beyond the allowance only, oldest
    first, and leaves the allowance running; no more stages exist than keep + allowance + 1; retire(0) leaves nothing."""
    n_allowed = allowed() if callable(allowed) else allowed
    be = _Backend()
    stages, spans = [], []
    with _inflight(be, outstanding=allowed) as fl:
        for t in range(1, 41):
            sp, stage = _staged_call(fl, be, t, "s%d" % t, keep)
            spans.append(sp)
            if not any(stage is s for s in stages):
                stages.append(stage)
            assert len(be.outstanding()) == min(n_allowed, max(0, t - keep))
        assert len(stages) <= keep + n_allowed + 1
        assert be.blocked == list(range(40 - keep - n_allowed))      # (each waited for only when it was beyond the allowance)
        assert _closes(be) == ["s%d" % t for t in range(1, 41 - keep - n_allowed)]
        fl.retire(0)
        assert not be.outstanding() and len(be.copies) == 40
    assert _closes(be) == ["s%d" % t for t in range(1, 41)] and all(sp.closed == 1 for sp in spans)
    assert be.nsync == 0


def test_stage_of_the_wrong_size_is_replaced():
    be = _Backend()
    with _inflight(be) as fl:
        _, first = _staged_call(fl, be, 1, "a", 0)
        assert first.nbytes == UNIT and first.space == "system" and first.dtype == np.uint8
        bigger = fl.take_stage(2 * UNIT)                            # (the pooled one does not fit: a new one, the old one dropped)
        assert bigger is not first and bigger.nbytes == 2 * UNIT
        fl.push(2, _Span("b", be.events, 2 * UNIT), object(), bigger)
        fl.retire(0)
        assert fl.take_stage(2 * UNIT) is bigger
        assert fl.take_stage(2 * UNIT) is not bigger                # (the pool is empty)


@pytest.mark.parametrize("sync_raises", [False, True])
def test_leaving_on_an_exception_waits_and_drops_everything_uncommitted(sync_raises):
    be = _Backend(sync_raises=sync_raises)
    spans = []
    with pytest.raises(KeyError, match="the block's own"):
        with _inflight(be, outstanding=3) as fl:
            for t in range(1, 7):
                spans.append(_staged_call(fl, be, t, "s%d" % t, 2)[0])
            spans.append(_Span("direct", be.events))
            fl.push(7, spans[-1], object())
            assert len(be.outstanding()) == 3 and _closes(be) == ["s1"]
            n = len(be.events)
            raise KeyError("the block's own")
    assert be.nsync == 1
    if sync_raises:
        assert be.events[n:] == [("sync",)]
    else:
        assert be.events[n:] == [("sync",)] + [("copy_wait", i) for i in (1, 2, 3)] and not be.outstanding()
    assert [sp.closed for sp in spans] == [1, 0, 0, 0, 0, 0, 0]     # (nothing more was finished or closed)
    n = len(be.events)
    fl.retire(0)                                                    # (and nothing is left to finish)
    assert be.events[n:] == []


def test_leaving_with_nothing_in_flight_does_not_touch_the_stream():
    be = _Backend()
    with _inflight(be) as fl:
        _staged_call(fl, be, 1, "a", 0)
    assert be.nsync == 0 and _closes(be) == ["a"]


@pytest.mark.parametrize("staged", [False, True])
def test_a_finish_that_raises_leaves_the_queue_consistent(staged):
    be, got = _Backend(), []

    def finish(sp, meta):
        got.append(sp.name)
        if sp.name == "b" and got.count("b") == 1:
            raise ValueError("on_candidates failed")
        sp.close()

    with _inflight(be, finish=finish) as fl:
        spans = []
        for t, name in enumerate("abcd", 1):
            sp = _Span(name, be.events)
            spans.append(sp)
            stage = fl.take_stage(UNIT) if staged else None
            fl.push(t, sp, object(), stage)
        with pytest.raises(ValueError, match="on_candidates failed"):
            fl.retire(0)
        assert got == ["a", "b"]
        fl.retire(0)
        assert got == ["a", "b", "c", "d"]                          # (b was popped: it is not finished again)
        if staged:
            assert fl.take_stage(UNIT) is not None and len(be.copies) == 4 and not be.outstanding()
    assert [sp.closed for sp in spans] == [1, 0, 1, 1] and be.nsync == 0
