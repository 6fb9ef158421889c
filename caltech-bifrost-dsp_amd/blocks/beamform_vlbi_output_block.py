"""BeamformVlbiOutput: voltage beams -> one "ibeam" UDP packet per time sample, the packets built on the device.

Drop-in counterpart of pipeline/lwa352_pipeline/blocks/beamform_vlbi_output_block.py (constructor :188-206, main :208-290).
The reference copies the selected beams to the host for every gulp, transposes them with numpy and hands bursts of 32 samples
to bifrost's `UDPTransmit('ibeam1_<nchan>')` (:258-275).  Here one HIP kernel on the beamformer's stream
(xengBeamformPacketizeVoltages, csrc/beam_vlbi_kernels.h) selects, transposes and writes the headers into a device packet
buffer; the host copies the finished packets to pinned memory and sends them.

Input: the Beamform output span, cf32 [nchan][nbeam * npol][ntime_gulp] (the reference's gulp size, :225).  Packet t of a gulp
carries sample t of the beams [0, (2 // npol) * nbeam_send): pairs of single-pol beams are one dual-pol "beam" (:206, 263).

Packet (the 15-byte packed `struct ibeam` of the reference docstring, :141-149; multi-byte fields big-endian, as
BeamformOutput builds the pbeam header): u8 server (= pipeline_idx, one-based as the docstring says; the reference hands
bifrost `pipeline_idx - 1` as the source, :270), gbe (1), nchan, nbeam (= nbeam_send),
nserver (= system_nchan // nchan); u16 chan0; u64 seq (the sample number); then the payload cf32 [nchan][beams] in native byte
order.  The layout is UNPINNED: the same docstring speaks of a "32 byte header" (:137) and a uint32 chan0 (:174), and the
writer that defines the format (bifrost's `ibeam` packet writer) is an empty submodule in the reference tree -- this block
follows the struct.

Where packets live: slot t of a gulp's packet buffer is `pkt_stride` bytes (16 + payload, rounded up to 16); the packet is
bytes [1, 16 + payload) of its slot, sent as one contiguous slice.  `dest_ip` "0.0.0.0" skips the gulp (no kernel, no copy)
unless a `sink(packet_bytes)` callable is given (tests); `dest_ip` / `dest_port` changes re-target (:236-254).  Sending is
throttled as the reference does: bursts of `_npacket_burst` packets, then a sleep of burst_bits / _max_bps less the time the
burst took (:262-275), through the `_clock` / `_sleep` attributes.

Gulps in flight (in-repo rings, whose span memory outlives its release): gulp k's kernel is enqueued, then gulp k-1's packets
(copied already) are sent while it runs, then gulp k's packets go to pinned memory on the copy stream -- two gulps in flight,
the staged pattern of BeamformSumBeams.  A bifrost ring: kernel, wait, copy, send, per gulp.
"""
import collections
import json
import socket
import time

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray
from ..proclog import cpu_affinity
from .block_base import Block, declare_streams, gulp_time

HEADER_BYTES = 16           # header at bytes [1, 16) of a slot, payload from byte 16 (16-byte aligned)


class BeamformVlbiOutput(Block):
    def __init__(self, log, iring,
                 guarantee=True, core=-1, etcd_client=None, dest_port=10000,
                 ntime_gulp=480, pipeline_idx=1, nbeam_send=1, gpu=-1, backend=None, sink=None):
        super(BeamformVlbiOutput, self).__init__(log, iring, None, guarantee, core, etcd_client=etcd_client)
        cpu_affinity.set_core(self.core)
        self._bf = backend if backend is not None else default_backend()
        self.gpu = gpu
        self.sink = sink
        self.sock = None
        self.define_command_key('dest_ip', type=str, initial_val='0.0.0.0')
        self.define_command_key('dest_port', type=int, initial_val=dest_port)
        self.update_command_vals()
        self.dest_ip = self.command_vals['dest_ip']
        self.dest_port = self.command_vals['dest_port']
        self.ntime_gulp = ntime_gulp
        self._npacket_burst = 32        # packets between throttle sleeps
        self._max_bps = 0.6 * 1e9
        self._clock = time.time         # (tests replace these two)
        self._sleep = time.sleep
        self.pipeline_idx = pipeline_idx
        self.nbeam_send = nbeam_send
        self.npol = 2                   # single-pol upstream beams are sent in pairs, as dual-pol beams
        declare_streams(iring, 'beam')  # (the packetiser runs on the beamformer's stream)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)

    def _update_destination(self):
        """:236-254: re-target only when something has changed."""
        self.update_command_vals()
        if not (self.dest_ip == self.command_vals['dest_ip'] and self.dest_port == self.command_vals['dest_port']):
            self.dest_ip = self.command_vals['dest_ip']
            self.dest_port = self.command_vals['dest_port']
            self.log.info("VLBI OUTPUT >> Updating destination to %s:%s" % (self.dest_ip, self.dest_port))
            if self.sock is not None:
                self.sock.close()
                self.sock = None
            if self.dest_ip != '0.0.0.0':
                self.sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
                self.sock.connect((self.dest_ip, self.dest_port))
        self.update_stats({'dest_ip': self.dest_ip, 'dest_port': self.dest_port, 'update_pending': self.update_pending,
                           'last_update_time': time.time()})

    def _send(self, host, npkt, pkt_stride, pkt_bytes, burst_bits):
        """Packets of one gulp from the host copy of its packet buffer, throttled per burst (:262-275)."""
        mv = memoryview(host.numpy()).cast('B')
        sock, sink = self.sock, self.sink
        try:
            toff = 0
            while toff < npkt:
                t0 = self._clock()
                for t in range(toff, min(toff + self._npacket_burst, npkt)):
                    pkt = mv[t * pkt_stride + 1:t * pkt_stride + 1 + pkt_bytes]
                    if sink is not None:
                        sink(bytes(pkt))
                    if sock is not None:
                        sock.send(pkt)
                toff += self._npacket_burst
                delay = burst_bits / self._max_bps - (self._clock() - t0)
                if delay > 0:
                    self._sleep(delay)
        except OSError as e:
            self.log.error("VLBI OUTPUT >> Sending error: %s" % str(e))

    def main(self):
        self.bind()
        # Streaming (in-repo rings): a gulp's input is kept until ITS kernel is done, its packets go to pinned memory on the copy
        # stream, and they are sent while the next gulp's kernel runs.  A bifrost ring: the synchronous form.
        streaming = (getattr(self.iring, 'span_memory_outlives_release', False) and hasattr(self._bf, 'beam_mark')
                     and hasattr(self._bf, 'copy_async'))
        self._streaming = streaming
        self._free = []                 # (device packet buffer, host packet buffer) pairs of the current size
        inflight = collections.deque()  # (ticket or copy stamp, is_copy, input kept alive, buffers, send arguments, gulp time)
        try:
            self._main_loop(streaming, inflight)
        finally:
            # (as InFlight does, block_base.py: nothing a kernel or copy in flight still touches is let go before the stream is idle)
            if inflight:
                try:
                    self._bf.beam_sync()
                    for stamp, is_copy, _, _, _, _ in inflight:
                        if is_copy:
                            self._bf.copy_wait(stamp)
                except Exception:
                    pass
                inflight.clear()
            if self.sock is not None:
                self.sock.close()
                self.sock = None

    def _buffers(self, nbytes):
        if self._free and self._free[-1][0].nbytes == nbytes:
            return self._free.pop()
        self._free = []
        host_space = 'system' if self._bf.space_in == 'system' else 'cuda_host'
        return (XArray(shape=(nbytes,), dtype=np.uint8, space=self._bf.space_in), XArray(shape=(nbytes,), dtype=np.uint8, space=host_space))

    def _finish(self, inflight, keep):
        """Send the gulps in flight beyond the newest `keep`: a gulp whose kernel is done has its packets copied first."""
        while len(inflight) > keep:
            stamp, is_copy, _, bufs, args, gulp_time = inflight.popleft()
            if not is_copy:
                self._bf.beam_wait(stamp)
                stamp = self._bf.copy_async(bufs[1], bufs[0])
            self._bf.copy_wait(stamp)
            self._send(bufs[1], *args)
            self._free.append(bufs)
            self.update_stats({'last_end_sample': gulp_time})

    def _main_loop(self, streaming, inflight):
        prev_time = time.time()
        for iseq in self.iring.read(guarantee=self.guarantee):
            self.update_pending = True
            ihdr = json.loads(iseq.header.tostring())
            self.sequence_proclog.update(ihdr)
            seq0 = ihdr['seq0']
            nchan, nbeam, nbit, npol = ihdr['nchan'], ihdr['nbeam'], ihdr['nbit'], ihdr['npol']
            system_nchan, chan0 = ihdr['system_nchan'], ihdr['chan0']
            if nbit != 32 or not ihdr.get('complex', False):
                raise ValueError("VLBI OUTPUT: input must be complex 32-bit floats (nbit=%d, complex=%s)" % (nbit, ihdr.get('complex')))
            if npol not in (1, 2) or system_nchan % nchan:
                raise ValueError("VLBI OUTPUT: npol %d / system_nchan %d of %d channels not supported" % (npol, system_nchan, nchan))
            nrow = nbeam * npol                                 # cf32 rows per channel (:225)
            nsel = (self.npol // npol) * self.nbeam_send        # rows sent (:263)
            if nsel > nrow:
                raise ValueError("VLBI OUTPUT: %d beams to send, %d in the input" % (nsel, nrow))
            igulp_size = self.ntime_gulp * nrow * nchan * 8
            pkt_bytes = HEADER_BYTES - 1 + nchan * nsel * 8
            pkt_stride = -(-(HEADER_BYTES + nchan * nsel * 8) // 16) * 16
            burst_bits = self._npacket_burst * nchan * nsel * 2 * 32
            hdr_args = (self.pipeline_idx, 1, self.nbeam_send, system_nchan // nchan, chan0)
            this_gulp_time = seq0
            for ispan in iseq.read(igulp_size):
                if ispan.size < igulp_size:
                    continue                                    # ignore final gulp
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, self.ntime_gulp, this_gulp_time)
                if self.update_pending:
                    self._update_destination()
                self.update_stats({'curr_sample': this_gulp_time})
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                reserve_time = 0.0
                if self.command_vals['dest_ip'] != '0.0.0.0' or self.sink is not None:
                    bufs = self._buffers(self.ntime_gulp * pkt_stride)
                    curr_time = time.time()
                    reserve_time = curr_time - prev_time
                    prev_time = curr_time
                    data = ispan.data
                    server, gbe, nbeam_hdr, nserver, c0 = hdr_args
                    rv = self._bf.beam_packetize_voltages(data, bufs[0], nchan, nrow, self.ntime_gulp, 0, nsel, pkt_stride,
                                                          server, gbe, nbeam_hdr, nserver, c0, this_gulp_time)
                    if rv != self._bf.BF_STATUS_SUCCESS:
                        self._free.append(bufs)
                        raise RuntimeError("xengBeamformPacketizeVoltages returned %d: %s" % (rv, self._bf.last_error()))
                    args = (self.ntime_gulp, pkt_stride, pkt_bytes, burst_bits)
                    if streaming:
                        inflight.append((self._bf.beam_mark(), False, data, bufs, args, this_gulp_time))
                        self._finish(inflight, 1)       # send the previous gulp while this one's kernel runs ...
                        stamp, _, _, _, _, _ = inflight[0]
                        self._bf.beam_wait(stamp)       # ... then this one's packets go to pinned memory (input let go)
                        inflight[0] = (self._bf.copy_async(bufs[1], bufs[0]), True, None, bufs, args, this_gulp_time)
                    else:
                        self._bf.beam_sync()
                        bufs[1][...] = bufs[0]          # (synchronous copy)
                        self._send(bufs[1], *args)
                        self._free.append(bufs)
                        self.update_stats({'last_end_sample': this_gulp_time})
                    del data
                else:
                    self._finish(inflight, 0)
                    self.update_stats({'last_end_sample': this_gulp_time})
                curr_time = time.time()
                process_time = curr_time - prev_time
                prev_time = curr_time
                self.perf_proclog.update({'acquire_time': acquire_time, 'reserve_time': reserve_time, 'process_time': process_time})
                this_gulp_time += self.ntime_gulp
            self._finish(inflight, 0)               # the sequence ends: every gulp in flight is sent
