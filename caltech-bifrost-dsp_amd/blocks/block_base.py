"""Block: the base class of the hot-path blocks, with the reference's public surface
(pipeline/lwa352_pipeline/blocks/block_base.py:95-387): command keys with type/condition
checks, the pending -> active command hand-off under a control lock, JSON command parsing
(etcd callback shape), stats and proclogs.  etcd is optional (`etcd_client=None`), commands
can be injected with process_command_strings() exactly as the reference's tests do
(block_base.py:194-214)."""
import collections
import json
import socket
import time
from threading import Lock

import numpy as np

from ..ndarray import XArray
from ..proclog import ProcLog, cpu_affinity

COMMAND_OK = 0
COMMAND_NOT_RECOGNIZED = -1
COMMAND_WRONG_TYPE = -2
COMMAND_INVALID = -3


class _Event:
    def __init__(self, value):
        self.value = value


class _WatchResponse:
    def __init__(self, cmds):
        self.events = [_Event(c) for c in cmds]


def declare_streams(ring, *classes):
    """Tell an in-repo ring which of the library's streams touch its spans (ring.py declare_streams; a bifrost ring has no
    such method: nothing to do)."""
    f = getattr(ring, 'declare_streams', None)
    if f is not None:
        f(*classes)


def spans_outlive_release(iring, oring):
    """Both rings keep a span's memory alive while it is referenced (in-repo rings): a block may keep several gulps in flight
    and let go of each gulp's spans when ITS kernels have completed.  A bifrost ring: wait for the kernels after every gulp."""
    return getattr(iring, 'span_memory_outlives_release', False) and getattr(oring, 'span_memory_outlives_release', False)


class InFlight(object):
    """The calls of a streaming block whose kernels may still run, oldest first, and the copies of their outputs that may:
    everything that keeps span memory from going back to a ring under a running kernel or copy.

    `wait(ticket)` / `sync()` / `mark()` are the backend's ticket wait, stream sync and ticket for what has been enqueued so far
    (`mark`: kept for SpanLoop, which pushes it).  A call is pushed with the ticket that follows its
    kernels, its output span(s) (none: only the input is held) and the input it reads.  Its kernel wrote either the span itself,
    or a `stage` from take_stage(): a device buffer that the copy stream (`backend`: copy_async / copy_done / copy_wait,
    space_in) moves into the span(s) once the ticket is done -- a kernel that stores into a pinned-host span holds its stream
    for the length of the transfer.  A span is handed to `finish(ospan, meta)` (default: close it) when its kernel and its copy
    have completed, always in the order pushed.  `outstanding` (a number, or a callable that gives it): the copies a retire
    that keeps calls may leave running.

    Used as a context manager: a block that leaves with calls or copies in flight (an exception) waits for the stream and the
    copies before it drops their spans, uncommitted -- released under a running kernel, their memory would go back to the
    ring, to be handed out again or freed."""

    def __init__(self, wait, sync, backend=None, finish=None, outstanding=2, mark=None):
        self._wait, self._sync, self._bf, self._outstanding = wait, sync, backend, outstanding
        self.mark = mark
        self._finish = finish if finish is not None else lambda ospan, meta: ospan.close()
        self._calls = collections.deque()       # (ticket, output spans, input kept alive, stage or None, meta)
        self._copies = collections.deque()      # (stamp, output span, stage to give back after this copy or None, meta)
        self._stages = []

    def take_stage(self, nbytes):
        """A device buffer of `nbytes` for a kernel to write: a pooled one, or a new one when there is none of that size."""
        stage = self._stages.pop() if self._stages else None
        if stage is None or stage.nbytes != nbytes:
            stage = XArray(shape=(nbytes,), dtype=np.uint8, space=self._bf.space_in)
        return stage

    def push(self, ticket, ospans, held, stage=None, meta=None):
        if ospans is None:
            ospans = ()
        elif not isinstance(ospans, (list, tuple)):
            ospans = (ospans,)
        self._calls.append((ticket, ospans, held, stage, meta))

    def _finish_copies(self, keep):
        """Complete the oldest copies: those beyond the newest `keep`, and those that are done."""
        while self._copies and (len(self._copies) > keep or self._bf.copy_done(self._copies[0][0])):
            stamp, ospan, stage, meta = self._copies.popleft()
            self._bf.copy_wait(stamp)           # (returns at once when it is done)
            if stage is not None:
                self._stages.append(stage)
            self._finish(ospan, meta)

    def retire(self, keep):
        """Wait for all but the newest `keep` calls; finish their output spans, or start the copies that fill them."""
        while len(self._calls) > keep:
            ticket, ospans, _, stage, meta = self._calls.popleft()
            self._wait(ticket)
            for k, ospan in enumerate(ospans):
                if stage is None:
                    self._finish_copies(0)      # (spans are committed in order: the copies of earlier calls first)
                    self._finish(ospan, meta)
                    continue
                dst = ospan.data
                piece = stage if stage.nbytes == dst.nbytes else stage.byte_slice(k * dst.nbytes, dst.nbytes)
                self._copies.append((self._bf.copy_async(dst, piece), ospan, stage if k == len(ospans) - 1 else None, meta))
        if self._copies:
            self._finish_copies((self._outstanding() if callable(self._outstanding) else self._outstanding) if keep else 0)

    def finish_now(self, ospan, dev, meta=None):
        """The synchronous path, for rings whose spans do not outlive release: wait for the stream, copy the bytes the kernel
        wrote into the scratch buffer `dev` to the span and finish it (no span: only the wait)."""
        self._sync()
        if ospan is None:
            return
        try:
            ospan.data_view(np.uint8).reshape(-1)[...] = dev
        except BaseException:
            ospan.close()
            raise
        self._finish(ospan, meta)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._calls or self._copies:
            try:
                self._sync()
                for copy in self._copies:
                    self._bf.copy_wait(copy[0])
            except Exception:
                pass
            self._calls.clear()
            self._copies.clear()


def gulp_time(ispan, seq0, igulp_size, ntime_gulp, prev):
    """The first sample of the gulp in `ispan` from its place in the sequence (`offset`, bytes from the sequence's start), or
    after the gulps the reader skipped (`skipped` bytes right before it), or else `prev`."""
    offset = getattr(ispan, 'offset', None)
    if offset is not None:
        return seq0 + (offset // igulp_size) * ntime_gulp
    if getattr(ispan, 'skipped', 0):
        return prev + (ispan.skipped // igulp_size) * ntime_gulp
    return prev


RESTART, SKIP = 'restart', 'skip'               # what SpanLoop's `before` hook may answer


class SpanLoop(object):
    """The loop of a block that reads one span and writes at most one: which span is closed uncommitted on an error, what is
    waited for before an output sequence ends, and what keeps an input alive under a running kernel.

    Made once in main(): `block` gives the log, the stats, the perf log, STREAM_DEPTH and the backend's space; `who` heads the
    log lines and `gap_note` ends the one about a gap; `inflight` is the block's InFlight (with `mark`), `oring` the output
    ring being written.  `streaming`: the rings' spans outlive release, so calls are pushed and up to STREAM_DEPTH stay in
    flight; else every call is waited for and its output copied from the loop's device scratch buffer.  `staged`: the kernel
    writes a stage of the InFlight, not the span.  `count_gaps`: a gap bumps stats['ngap'].

    run() is one input sequence.  Per whole span (a short final one is ignored), with t its first sample:
      a gap (t is not where the span before ended): on_gap(), the log line, the output sequence ends;
      before(t) loads what is pending and may answer RESTART (the output sequence ends here) or SKIP (the span is dropped);
      the output sequence is begun if there is none, at time tag t + tag_offset with header(t + tag_offset) (tag_offset, in
      samples, is for a block whose first committed span is a later input span than the one that begins the sequence);
      body(t, held, loop) enqueues the kernels on the input `held`.  It writes where loop.target(meta) says -- which reserves
      the output span -- or nowhere, and returns the stats it changes; 'last_end_sample' is added.
    The call is then pushed with its ticket, or waited for and finished.  An output sequence ends only after retire(0)."""

    def __init__(self, block, who, inflight, oring, streaming, staged=False, gap_note="", count_gaps=True):
        self.block, self.who, self.inflight, self.oring = block, who, inflight, oring
        self.streaming, self.staged, self.gap_note, self.count_gaps = streaming, staged, gap_note, count_gaps
        self._oseq = self._ospan = self._stage = self._meta = self._dev = None

    def target(self, meta=None):
        """Reserve this call's output span and give what its kernel writes: a stage, the span itself, or the scratch buffer.
        `meta` goes to the InFlight's finish with the span."""
        self._meta = meta
        self._ospan = self._oseq.reserve(self._ogulp_size)
        if self.staged:
            self._stage = self.inflight.take_stage(self._ogulp_size)
            return self._stage
        return self._ospan.data if self.streaming else self._dev

    def _end_sequence(self):
        if self._oseq is not None:
            self.inflight.retire(0)             # every call in flight is complete (and every output span committed) first
            oseq, self._oseq = self._oseq, None
            oseq.end()

    def run(self, iseq, seq0, igulp_size, ntime_gulp, ogulp_size, header, body, before=None, on_gap=None, tag_offset=0):
        block, inflight = self.block, self.inflight
        self._ogulp_size, self._oseq = ogulp_size, None
        if not self.streaming and (self._dev is None or self._dev.nbytes != ogulp_size):
            self._dev = XArray(shape=(ogulp_size,), dtype=np.uint8, space=block._bf.space_in)
        this_gulp_time = expected = seq0
        try:
            prev_time = time.time()
            for ispan in iseq.read(igulp_size):
                if ispan.size < igulp_size:
                    continue                    # a short final span is skipped (as the reference's gulp_nframe reader does)
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, ntime_gulp, this_gulp_time)
                if this_gulp_time != expected:
                    # spans this reader never saw: the output goes on in a sequence of its own, so that a span's time follows
                    # from its place
                    if on_gap is not None:
                        on_gap()
                    if self.count_gaps:
                        block.update_stats({'ngap': block.stats['ngap'] + 1})
                    block.log.warning("%s >> samples [%d, %d) were not read%s" % (self.who, expected, this_gulp_time, self.gap_note))
                    self._end_sequence()
                expected = this_gulp_time + ntime_gulp
                block.update_stats({'curr_sample': this_gulp_time})
                action = before(this_gulp_time) if before is not None else None
                if action == SKIP:
                    continue
                if action == RESTART:
                    self._end_sequence()
                held = ispan.data
                if self._oseq is None:
                    self._oseq = self.oring.begin_sequence(time_tag=this_gulp_time + tag_offset, header=json.dumps(header(this_gulp_time + tag_offset)))
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                self._ospan = self._stage = self._meta = None
                try:
                    stats = body(this_gulp_time, held, self) or {}
                    stats['last_end_sample'] = this_gulp_time + ntime_gulp
                    block.update_stats(stats)
                    osp, self._ospan = self._ospan, None
                    if self.streaming:
                        inflight.push(inflight.mark(), osp, held, self._stage, self._meta)
                        inflight.retire(block.STREAM_DEPTH)
                    else:
                        inflight.finish_now(osp, self._dev, self._meta)
                finally:
                    if self._ospan is not None:
                        self._ospan.close()     # (reserved, but not handed over)
                        self._ospan = None
                curr_time = time.time()
                process_time = curr_time - prev_time
                prev_time = curr_time
                block.perf_proclog.update({'acquire_time': acquire_time, 'reserve_time': 0.0, 'process_time': process_time})
        finally:
            inflight.retire(0)                  # (with or without an output sequence: the input spans are let go of)
            self._end_sequence()


def split_frames(parts, row, nupchan, who):
    """Samples in the first of a gulp's two parts (`row` bytes each), which must be whole frames of `nupchan` samples."""
    ntime0 = parts[0].nbytes // row
    if ntime0 % nupchan:
        raise RuntimeError("%s: a gulp split after %d samples is not whole frames of %d" % (who, ntime0, nupchan))
    return ntime0


class Block(object):
    pipeline_id = 0
    _instance_count = -1

    @classmethod
    def set_id(cls, x):
        cls.pipeline_id = x

    @classmethod
    def _get_instance_id(cls):
        # per-subclass zero-based counter (block_base.py:80-91)
        cls._instance_count += 1
        return cls._instance_count

    def __init__(self, log, iring, oring, guarantee, core, etcd_client=None,
                 command_keyroot='/cmd/corr', monitor_keyroot='/mon/corr',
                 response_keyroot='/resp/corr', name=None):
        self.log = log
        self.iring, self.oring = iring, oring
        self.guarantee, self.core = guarantee, core
        self.instance_id = self._get_instance_id()
        self.name = name or type(self).__name__
        self.stats = {}
        self.log.info("Pipeline %d: Initializing block: %s (instance %d)" % (self.pipeline_id, self.name, self.instance_id))
        cls = type(self).__name__
        self.bind_proclog = ProcLog(cls + "/bind")
        self.in_proclog = ProcLog(cls + "/in")
        self.out_proclog = ProcLog(cls + "/out")
        self.size_proclog = ProcLog(cls + "/size")
        self.sequence_proclog = ProcLog(cls + "/sequence0")
        self.perf_proclog = ProcLog(cls + "/perf")
        self.stats_proclog = ProcLog(cls + "/stats")
        if self.iring is not None:
            self.in_proclog.update({'nring': 1, 'ring0': self.iring.name})
        if self.oring is not None:
            self.out_proclog.update({'nring': 1, 'ring0': self.oring.name})

        self.etcd_client = etcd_client
        keyfmt = '{root}/x/{host}/pipeline/{pid}/{block}/{id}'
        ids = dict(host=socket.gethostname(), pid=self.pipeline_id, block=self.name, id=self.instance_id)
        self.command_key = keyfmt.format(root=command_keyroot, **ids)
        self.monitor_key = keyfmt.format(root=monitor_keyroot, **ids)
        self.response_key = keyfmt.format(root=response_keyroot, **ids)
        self._etcd_watch_id = None
        self._control_lock = Lock()
        if self.etcd_client:
            self.log.info("Adding watch callback to %s" % self.command_key)
            self._etcd_watch_id = self.etcd_client.add_watch_prefix_callback(self.command_key, self._etcd_callback)
        self.update_pending = False
        self.command_vals = {}
        self._pending_command_vals = {}
        self._command_types = {}
        self._command_conditions = {}
        self._etcd_sets_pending = True

    def bind(self):
        """The first lines of a GPU block's main(): this thread on the block's core, the block's device current, both logged."""
        cpu_affinity.set_core(self.core)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.bind_proclog.update({'ncore': 1, 'core0': cpu_affinity.get_core(), 'ngpu': 1, 'gpu0': self._bf.get_device()})

    def _call(self, name, *args):
        """A call of the block's backend that returns a status: anything but success raises."""
        rv = getattr(self._bf, name)(*args)
        if rv != self._bf.BF_STATUS_SUCCESS:
            raise RuntimeError("%s returned %d: %s" % (name, rv, self._bf.last_error()))

    # ------------------------------------------------------------------ command keys
    def define_command_key(self, name, type=None, condition=None, initial_val=None):
        if initial_val:
            if type:
                assert isinstance(initial_val, type), "%s: key %s: Initial value type check fail!" % (self.name, name)
            if condition:
                assert condition(initial_val), "%s: key %s: Intial value failed condition check! (%s)" % (self.name, name, condition)
        self.command_vals[name] = initial_val
        self._pending_command_vals[name] = initial_val
        self._command_types[name] = type
        self._command_conditions[name] = condition

    def process_command_strings(self, cmds):
        """Process command JSON string(s) as if they had arrived over etcd."""
        if not isinstance(cmds, list):
            cmds = [cmds]
        self._etcd_callback(_WatchResponse(cmds))

    def _parse_event(self, event):
        """-> (seq_id, kwargs) or (seq_id, None) after having sent the error response."""
        v = json.loads(event.value)
        seq_id = v.get('id', None)
        if seq_id is None:
            self._send_command_response("0", False, "Missing ID field")
            return None, None
        if v.get('cmd', None) != "update":
            self._send_command_response("0", False, "Invalid command")
            return None, None
        val = v.get("val", None)
        if not isinstance(val, dict):
            self._send_command_response(seq_id, False, "`val` field should be a dictionary")
            return seq_id, None
        kwargs = val.get("kwargs", None)
        if not isinstance(kwargs, dict):
            self._send_command_response(seq_id, False, "`val[kwargs]` field should be a dictionary")
            return seq_id, None
        return seq_id, kwargs

    def _etcd_callback(self, watchresponse):
        cpu_affinity.set_core(self.core)
        with self._control_lock:
            for event in watchresponse.events:
                seq_id, kwargs = self._parse_event(event)
                if kwargs is None:
                    continue
                try:
                    proc_ok = self._process_commands(kwargs, set_pending_flag=self._etcd_sets_pending)
                except Exception:
                    proc_ok = COMMAND_INVALID
                self.update_stats({'last_cmd_response': proc_ok})
                self._send_command_response(seq_id, proc_ok == COMMAND_OK, str(proc_ok))

    def _send_command_response(self, seq_id, processed_ok, response):
        resp = {'id': seq_id, 'val': {'status': 'normal' if processed_ok else 'error',
                                      'response': response, 'timestamp': time.time()}}
        self.last_response = resp
        if self.etcd_client:
            try:
                self.etcd_client.put(self.response_key, json.dumps(resp))
            except Exception:
                self.log.error("Error trying to send ETCD command response")
                raise
        else:
            self.log.info("No ETCD interface: Command response: %s" % (resp,))

    def _process_commands(self, command_dict, set_pending_flag=True):
        for key, val in command_dict.items():
            if key not in self.command_vals:
                self.log.error("%s: Command key %s not recognized" % (self.name, key))
                return COMMAND_NOT_RECOGNIZED
            if self._command_types[key] and not isinstance(val, self._command_types[key]):
                self.log.error("%s: Command key %s had wrong type (had %s, expected %s)" %
                               (self.name, key, type(val), self._command_types[key]))
                return COMMAND_WRONG_TYPE
            if self._command_conditions[key] and not self._command_conditions[key](val):
                self.log.error("%s: Command key %s failed requirements" % (self.name, key))
                return COMMAND_INVALID
            self._pending_command_vals[key] = val
            self.stats['new_' + key] = val
        if set_pending_flag:
            self.update_pending = True
        self.stats['update_pending'] = True
        self.stats['last_cmd_time'] = time.time()
        return COMMAND_OK

    def update_command_vals(self):
        with self._control_lock:
            self.command_vals.update(self._pending_command_vals)
            self.update_pending = False
            self.stats['update_pending'] = False
            self.stats['last_cmd_proc_time'] = time.time()
        self.update_stats(self.command_vals)

    def take_commands(self, keys):
        """update_command_vals(), then {key: value} of the `keys` a command has set.  A command is taken once: left in place, a
        later command for another key would bring it back over a set_*() made since."""
        self.update_command_vals()
        taken = {}
        with self._control_lock:
            for k in keys:
                cmd = self.command_vals.get(k)
                if cmd is not None:
                    taken[k] = cmd
                    self.command_vals[k] = None
                    if self._pending_command_vals.get(k) is cmd:
                        self._pending_command_vals[k] = None
        return taken

    def acquire_control_lock(self):
        self._control_lock.acquire()

    def release_control_lock(self):
        self._control_lock.release()

    def update_stats(self, new_stats={}):
        self.stats.update(new_stats)
        self.stats_proclog.update(self.stats)
