"""SpanLoop and Block.take_commands (blocks/block_base.py): the one loop of the span-in, span-out streaming blocks, with fake
spans, a fake input sequence and output ring, and the recording backend of tests/test_inflight_cpu.py.  No ring, no GPU."""
import json
import logging
import types
import weakref

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd.blocks.block_base import RESTART, SKIP, Block, InFlight, SpanLoop
from tests.test_inflight_cpu import UNIT, _Backend, _Span

LOG = logging.getLogger("span-loop-test")
G, NT, SEQ0, DEPTH = 32, 10, 1000, 2            # bytes and samples of an input gulp, the input sequence's first sample, STREAM_DEPTH


class _Ticketed(_Backend):
    def __init__(self):
        super().__init__()
        self.ticket = 0
        self.on_wait = None

    def mark(self):
        self.ticket += 1
        self.events.append(("mark", self.ticket))
        return self.ticket

    def wait(self, ticket):
        if self.on_wait is not None:
            self.on_wait(ticket)
        super().wait(ticket)


class _OutSpan(_Span):
    """An output span that also gives the view the synchronous copy writes through; `bad`: that copy raises."""
    bad = False

    def data_view(self, dtype):
        self.events.append(("view", self.name))
        if self.bad:
            raise IOError("the copy failed")
        return self.data.view(dtype)


class _OutSeq:
    def __init__(self, ring, index, time_tag, header):
        self.ring, self.index, self.time_tag, self.header, self.spans = ring, index, time_tag, json.loads(header), []

    def reserve(self, nbytes):
        assert nbytes == UNIT and self.ring.open is self
        sp = _OutSpan("q%d.%d" % (self.index, len(self.spans)), self.ring.events, nbytes)
        sp.bad = sp.name in self.ring.bad
        self.spans.append(sp)
        self.ring.events.append(("reserve", sp.name))
        return sp

    def end(self):
        assert self.ring.open is self
        self.ring.open = None
        self.ring.events.append(("end", self.index))


class _OutRing:
    def __init__(self, events, bad=()):
        self.events, self.bad, self.seqs, self.open = events, bad, [], None

    def begin_sequence(self, time_tag, header):
        assert self.open is None
        self.open = _OutSeq(self, len(self.seqs), time_tag, header)
        self.seqs.append(self.open)
        self.events.append(("begin", self.open.index))
        return self.open


class _Data:
    """What an input span holds: nothing but a number, and it can be weakly referenced."""

    def __init__(self, tag):
        self.tag = tag


class _InSeq:
    """An input sequence whose spans are made as they are read and kept by nobody: (gulp index or None, bytes skipped, size)."""

    def __init__(self, spans):
        self.spans, self.refs = spans, []

    def read(self, n):
        assert n == G
        for k, (index, skipped, size) in enumerate(self.spans):
            data = _Data(k + 1)
            self.refs.append(weakref.ref(data))
            sp = types.SimpleNamespace(size=size, data=data, skipped=skipped)
            if index is not None:
                sp.offset = index * G
            del data
            yield sp


def _at(*indices):
    return _InSeq([(k, 0, G) for k in indices])


class _Blk(Block):
    STREAM_DEPTH = DEPTH

    def __init__(self, be):
        super().__init__(LOG, None, None, True, -1)
        self._bf = be
        self.perf = []
        self.perf_proclog = types.SimpleNamespace(update=self.perf.append)
        self.update_stats({'ngap': 0, 'n': 0})


class _Rig:
    """A block, its backend, InFlight, output ring and SpanLoop; run() is one input sequence with a body that `writes' the input's
    number to where target() says -- for the calls in `outputs` (default: all) -- and records the call."""

    def __init__(self, streaming, staged=False, finish=None, bad=(), **kw):
        self.be = _Ticketed()
        self.events = self.be.events
        self.blk = _Blk(self.be)
        self.ring = _OutRing(self.events, bad)
        self.fl = InFlight(self.be.wait, self.be.sync, self.be, finish=finish, mark=self.be.mark)
        self.loop = SpanLoop(self.blk, "WHO", self.fl, self.ring, streaming, staged, **kw)
        self.targets, self.times, self.depth = [], [], []

    def body(self, t, held, out, outputs=None, fail_at=None):
        self.depth.append(len(self.fl._calls))
        self.times.append(t)
        n = len(self.times)
        if outputs is None or n in outputs:
            tgt = out.target(("meta", t))
            tgt.numpy()[...] = held.tag
            self.targets.append(tgt)
        if n == fail_at:
            raise KeyError("the run failed")
        self.events.append(("run", n))
        return {'n': self.blk.stats['n'] + 1}

    def run(self, iseq, header=None, before=None, on_gap=None, **kw):
        with self.fl:
            self.loop.run(iseq, SEQ0, G, NT, UNIT, header or (lambda t: {'seq0': t}), lambda t, held, out: self.body(t, held, out, **kw),
                          before=before, on_gap=on_gap)

    def names(self, kind):
        return [e[1] for e in self.events if e[0] == kind]

    def spans(self):
        return [sp for q in self.ring.seqs for sp in q.spans]


def test_gap_runs_the_hook_retires_then_ends_and_the_new_sequence_starts_at_the_first_span_after_it(caplog):
    rig = _Rig(streaming=True, gap_note=": the history starts again")
    with caplog.at_level(logging.WARNING, logger=LOG.name):
        rig.run(_at(0, 1, 3, 4), on_gap=lambda: rig.events.append(("gap", None)))
    ev = rig.events
    gap, end0, begin1 = ev.index(("gap", None)), ev.index(("end", 0)), ev.index(("begin", 1))
    # the hook, then the calls in flight are waited for and their spans finished, then the old sequence ends, then the new one begins
    assert gap < ev.index(("wait", 1)) < ev.index(("close", "q0.0")) < ev.index(("wait", 2)) < ev.index(("close", "q0.1")) < end0 < begin1
    assert begin1 < ev.index(("run", 3))
    assert [(q.time_tag, q.header['seq0'], len(q.spans)) for q in rig.ring.seqs] == [(SEQ0, SEQ0, 2), (SEQ0 + 3 * NT, SEQ0 + 3 * NT, 2)]
    assert rig.times == [SEQ0 + k * NT for k in (0, 1, 3, 4)]
    assert rig.blk.stats['ngap'] == 1 and rig.blk.stats['n'] == 4 and rig.blk.stats['last_end_sample'] == SEQ0 + 5 * NT
    assert rig.blk.stats['curr_sample'] == SEQ0 + 4 * NT
    assert [r.getMessage() for r in caplog.records] == ["WHO >> samples [%d, %d) were not read: the history starts again" % (SEQ0 + 2 * NT, SEQ0 + 3 * NT)]
    assert rig.names("end") == [0, 1] and [sp.closed for sp in rig.spans()] == [1, 1, 1, 1] and len(rig.blk.perf) == 4


def test_gaps_are_not_counted_when_the_block_does_not():
    rig = _Rig(streaming=True, count_gaps=False)
    rig.run(_at(0, 2))
    assert rig.blk.stats['ngap'] == 0 and rig.names("begin") == [0, 1]


def test_restart_from_the_pending_hook_header_evaluated_after_it_and_no_op_without_a_sequence():
    rig = _Rig(streaming=True)
    state = {'ref': -1}

    def before(t):
        rig.events.append(("before", t))
        if t in (SEQ0, SEQ0 + 2 * NT):
            state['ref'] = t                # (what the header of the sequence begun now must show)
            return RESTART

    rig.run(_at(0, 1, 2, 3), header=lambda t: {'seq0': t, 'ref': state['ref']}, before=before)
    ev = rig.events
    assert ev[0] == ("before", SEQ0) and ev[1] == ("begin", 0)          # (nothing was open: nothing retired, nothing ended)
    assert [(q.time_tag, q.header) for q in rig.ring.seqs] == [(SEQ0, {'seq0': SEQ0, 'ref': SEQ0}),
                                                               (SEQ0 + 2 * NT, {'seq0': SEQ0 + 2 * NT, 'ref': SEQ0 + 2 * NT})]
    # the restart: retire(0), then end, then the lazy begin
    assert ev.index(("before", SEQ0 + 2 * NT)) < ev.index(("close", "q0.1")) < ev.index(("end", 0)) < ev.index(("begin", 1)) < ev.index(("run", 3))
    assert [len(q.spans) for q in rig.ring.seqs] == [2, 2] and rig.blk.stats['ngap'] == 0


def test_a_run_that_raises_closes_its_span_once_finishes_the_earlier_ones_in_order_and_ends_the_sequence():
    rig = _Rig(streaming=True)
    with pytest.raises(KeyError, match="the run failed"):
        rig.run(_at(0, 1, 2, 3), fail_at=3)
    assert [sp.name for sp in rig.spans()] == ["q0.0", "q0.1", "q0.2"] and [sp.closed for sp in rig.spans()] == [1, 1, 1]
    closes = rig.names("close")
    assert closes.index("q0.0") < closes.index("q0.1")
    assert rig.events[-1] == ("end", 0) and rig.names("end") == [0]
    assert rig.names("wait") == [1, 2] and rig.be.nsync == 0            # (everything was retired: InFlight had nothing to drop)
    assert rig.blk.stats['n'] == 2 and rig.blk.stats['last_end_sample'] == SEQ0 + 2 * NT and len(rig.blk.perf) == 2


def test_streaming_keeps_at_most_stream_depth_calls_and_each_input_until_its_ticket_is_waited_for():
    rig = _Rig(streaming=True)
    iseq = _at(*range(7))
    alive_at_wait = []
    rig.be.on_wait = lambda ticket: alive_at_wait.append((ticket, iseq.refs[ticket - 1]() is not None))
    seen = []

    def before(t):
        k = (t - SEQ0) // NT
        seen.append((k, [r() is not None for r in iseq.refs]))

    rig.run(iseq, before=before)
    assert rig.depth == [min(k, DEPTH) for k in range(7)]              # (what is in flight when the next call is made)
    assert alive_at_wait == [(t, True) for t in range(1, 8)]
    for k, alive in seen:
        # before call k: the inputs of the DEPTH calls in flight and this span's own are alive, the earlier ones are gone
        assert alive == [j >= k - DEPTH for j in range(k + 1)], (k, alive)
    assert all(r() is None for r in iseq.refs)
    assert rig.names("close") == ["q0.%d" % k for k in range(7)] and rig.names("wait") == list(range(1, 8))
    assert all(tgt is sp.data for tgt, sp in zip(rig.targets, rig.spans()))     # (direct: the kernel writes the span itself)
    assert all(np.all(sp.seen == k + 1) for k, sp in enumerate(rig.spans()))


def test_staged_the_kernel_writes_the_stage_and_the_span_is_finished_after_its_copy():
    rig = _Rig(streaming=True, staged=True)
    rig.run(_at(*range(9)))
    spans, ev = rig.spans(), rig.events
    assert len(spans) == 9 and len(rig.be.copies) == 9
    for k, (sp, tgt, copy) in enumerate(zip(spans, rig.targets, rig.be.copies)):
        assert tgt is not sp.data and tgt.nbytes == UNIT and copy["src"] is tgt and copy["dst"] is sp.data
        assert ev.index(("wait", k + 1)) < ev.index(("copy", k)) < ev.index(("copy_wait", k)) < ev.index(("close", sp.name))
        assert sp.closed == 1 and np.all(sp.seen == k + 1)
    assert len({id(t) for t in rig.targets}) < 9                        # (stages went back to the pool and were taken again)
    assert any(rig.fl.take_stage(UNIT) is t for t in rig.targets)
    assert rig.names("end") == [0] and ev.index(("close", "q0.8")) < ev.index(("end", 0))


def test_synchronous_path_syncs_then_copies_then_finishes_with_the_meta_of_the_call():
    got = []

    def finish(sp, meta):
        rig.events.append(("finish", sp.name))
        got.append((sp.name, meta, sp.data.numpy().copy()))
        sp.close()

    rig = _Rig(streaming=False, finish=finish)
    rig.run(_at(0, 1, 2))
    per_call = [e for e in rig.events if e[0] in ("run", "sync", "view", "finish")]
    assert per_call == [x for k in range(3) for x in (("run", k + 1), ("sync",), ("view", "q0.%d" % k), ("finish", "q0.%d" % k))]
    assert [(n, m) for n, m, _ in got] == [("q0.%d" % k, ("meta", SEQ0 + k * NT)) for k in range(3)]
    assert all(np.all(d == k + 1) for k, (_, _, d) in enumerate(got))          # (the copy had landed when finish saw the span)
    assert all(t is rig.targets[0] and t.nbytes == UNIT and t.dtype == np.uint8 for t in rig.targets)      # one scratch buffer
    assert all(t is not sp.data for t, sp in zip(rig.targets, rig.spans()))
    assert not rig.names("mark") and not rig.names("wait") and [sp.closed for sp in rig.spans()] == [1, 1, 1]


def test_synchronous_path_closes_the_span_when_the_copy_raises():
    got = []
    rig = _Rig(streaming=False, finish=lambda sp, meta: (got.append(sp.name), sp.close()), bad=("q0.1",))
    with pytest.raises(IOError, match="the copy failed"):
        rig.run(_at(0, 1, 2))
    assert got == ["q0.0"] and [(sp.name, sp.closed) for sp in rig.spans()] == [("q0.0", 1), ("q0.1", 1)]
    assert rig.events[-1] == ("end", 0)


@pytest.mark.parametrize("streaming", [True, False])
def test_a_call_without_an_output_span_reserves_nothing_and_holds_its_input_until_its_ticket(streaming):
    rig = _Rig(streaming=streaming)
    iseq = _at(*range(6))
    alive_at_wait = []
    rig.be.on_wait = lambda ticket: alive_at_wait.append((ticket, iseq.refs[ticket - 1]() is not None))
    rig.run(iseq, outputs=(3, 6))
    assert rig.names("reserve") == ["q0.0", "q0.1"] and rig.names("close") == ["q0.0", "q0.1"]
    assert [int(sp.seen[0]) for sp in rig.spans()] == [3, 6] and rig.names("run") == list(range(1, 7))
    if streaming:
        assert alive_at_wait == [(t, True) for t in range(1, 7)] and rig.depth == [0, 1, 2, 2, 2, 2]
        ev = rig.events
        assert ev.index(("wait", 3)) < ev.index(("close", "q0.0")) < ev.index(("wait", 4)) < ev.index(("wait", 6)) < ev.index(("close", "q0.1"))
    else:
        assert rig.be.nsync == 6                                        # (every call is waited for, with a span or without)
    assert all(r() is None for r in iseq.refs) and rig.blk.stats['n'] == 6 and len(rig.blk.perf) == 6


def test_a_skip_after_the_hooks_begins_no_sequence_and_reserves_nothing():
    rig = _Rig(streaming=True)
    rig.run(_at(0, 1, 2, 3), before=lambda t: SKIP if t < SEQ0 + 2 * NT else None)
    assert rig.events[0] == ("begin", 0) and rig.names("reserve") == ["q0.0", "q0.1"]
    assert [(q.time_tag, q.header['seq0']) for q in rig.ring.seqs] == [(SEQ0 + 2 * NT, SEQ0 + 2 * NT)]
    assert rig.times == [SEQ0 + 2 * NT, SEQ0 + 3 * NT] and len(rig.blk.perf) == 2 and rig.blk.stats['ngap'] == 0

    rig = _Rig(streaming=True)
    rig.run(_at(0, 1), before=lambda t: SKIP)
    assert rig.events == [] and rig.ring.seqs == [] and rig.blk.stats['curr_sample'] == SEQ0 + NT


def test_a_short_final_span_is_ignored():
    rig = _Rig(streaming=True)
    rig.run(_InSeq([(0, 0, G), (1, 0, G), (2, 0, G - 1)]))
    assert rig.times == [SEQ0, SEQ0 + NT] and rig.names("reserve") == ["q0.0", "q0.1"] and rig.blk.stats['curr_sample'] == SEQ0 + NT
    assert rig.names("end") == [0] and rig.blk.stats['ngap'] == 0


def test_times_follow_the_offset_or_the_bytes_skipped():
    """Both branches of gulp_time: spans that say where they are in the sequence (`offset`), and spans that only say how many
    bytes the reader skipped right before them (`skipped`)."""
    rig = _Rig(streaming=False)
    rig.run(_at(0, 1, 4, 5))
    assert rig.times == [SEQ0 + k * NT for k in (0, 1, 4, 5)] and [q.time_tag for q in rig.ring.seqs] == [SEQ0, SEQ0 + 4 * NT]
    assert rig.blk.stats['ngap'] == 1 and rig.blk.stats['last_end_sample'] == SEQ0 + 6 * NT

    rig = _Rig(streaming=False)
    rig.run(_InSeq([(None, 0, G), (None, 3 * G, G)]))
    assert rig.times == [SEQ0, SEQ0 + 3 * NT] and [q.time_tag for q in rig.ring.seqs] == [SEQ0, SEQ0 + 3 * NT]
    assert rig.blk.stats['ngap'] == 1 and rig.blk.stats['last_end_sample'] == SEQ0 + 4 * NT


def test_take_commands_takes_a_command_once():
    """A command for `a` is taken; the caller then sets `a` itself (a set_*()); a later command for `b` alone must not bring the
    old `a` back over that."""
    blk = Block(LOG, None, None, True, -1)
    blk.define_command_key('a', type=list)
    blk.define_command_key('b', type=int)

    def command(**kw):
        blk.process_command_strings(json.dumps({'id': '1', 'cmd': 'update', 'val': {'kwargs': kw}}))
        assert blk.update_pending

    current = {}
    command(a=[1, 2])
    current.update(blk.take_commands(('a', 'b')))
    assert current == {'a': [1, 2]} and not blk.update_pending
    current['a'] = [3, 4]                                               # (set_a([3, 4]))
    command(b=7)
    taken = blk.take_commands(('a', 'b'))
    assert taken == {'b': 7}
    current.update(taken)
    assert current == {'a': [3, 4], 'b': 7}
    assert blk.command_vals == {'a': None, 'b': None} and blk._pending_command_vals == {'a': None, 'b': None}
    assert blk.take_commands(('a', 'b')) == {}
    command(a=[5], b=8)
    assert blk.take_commands(('b',)) == {'b': 8} and blk.command_vals['a'] == [5]       # (a key that was not asked for stays)
