"""TbfSource: triggered voltage dumps (.tbf files) -> gulps in a ring.  Host-only; no GPU work.

Reads the file format that the reference documents in pipeline/lwa352_pipeline/blocks/triggered_dump_block.py:121-150: a
little-endian u32 `hsize`, a little-endian u32 `hblock_size`, `hsize` bytes of JSON header (the dumped sequence's header plus
`seq`, the sample number of the file's first sample), and from byte `hblock_size` to the end the data as the input ring held
it, [time][chan][stand][pol] 4+4 bit.  It plays the role of the reference's TrigBufSourceBlock (lwa352-upchan-bf.py:94).

The files are read in the order given (a dump's `.0`, `.1`, ...).  Consecutive files whose `seq` values are contiguous
continue one output sequence, gulps running across file boundaries; a gap (or a different header shape) starts a new
sequence, whose header is the file's header with `seq0` = its `seq`.  A trailing partial gulp of a sequence is dropped.
Copy moves the gulps to a device ring.
"""
import json
import os
import struct

import numpy as np

from ..proclog import cpu_affinity
from .block_base import Block


def read_tbf_header(fh):
    """(header dict, byte offset of the data) of an open .tbf file (triggered_dump_block.py:143-148)."""
    hsize, hblock_size = struct.unpack('<II', fh.read(8))
    header = json.loads(fh.read(hsize))
    return header, hblock_size


class TbfSource(Block):
    def __init__(self, log, oring, filenames, ntime_gulp, core=-1):
        super(TbfSource, self).__init__(log, None, oring, True, core, etcd_client=None)
        self.filenames = list(filenames)
        self.ntime_gulp = ntime_gulp
        self.size_proclog.update({'nseq_per_gulp': ntime_gulp})

    @staticmethod
    def _bytes_per_time(hdr):
        return hdr['nchan'] * hdr['nstand'] * hdr['npol']        # one byte per 4+4-bit sample

    def _files(self):
        """(header, data offset, data bytes, path) per file, in order."""
        for path in self.filenames:
            with open(path, 'rb') as fh:
                hdr, off = read_tbf_header(fh)
            nbytes = os.path.getsize(path) - off
            yield hdr, off, nbytes, path

    def main(self):
        cpu_affinity.set_core(self.core)
        self.bind_proclog.update({'ncore': 1, 'core0': cpu_affinity.get_core()})
        # group the files into sequences: contiguous seq, same shape
        seqs = []
        for hdr, off, nbytes, path in self._files():
            bpt = self._bytes_per_time(hdr)
            ntime = nbytes // bpt
            last = seqs[-1] if seqs else None
            if (last is not None and hdr['seq'] == last['next'] and bpt == last['bpt']):
                last['files'].append((path, off, ntime * bpt))
                last['next'] += ntime
            else:
                seqs.append({'hdr': hdr, 'bpt': bpt, 'files': [(path, off, ntime * bpt)], 'next': hdr['seq'] + ntime})
        if not seqs:
            return
        gulp = max(s['bpt'] for s in seqs) * self.ntime_gulp
        self.oring.resize(gulp, total_span=4 * gulp)
        with self.oring.begin_writing() as oring:
            for s in seqs:
                ohdr = dict(s['hdr'])
                ohdr['seq0'] = ohdr['seq']
                igulp = s['bpt'] * self.ntime_gulp
                self.sequence_proclog.update(ohdr)
                with oring.begin_sequence(time_tag=ohdr['seq0'], header=json.dumps(ohdr), nringlet=1) as oseq:
                    carry = b''
                    for path, off, nbytes in s['files']:
                        with open(path, 'rb') as fh:
                            fh.seek(off)
                            left = nbytes
                            while left > 0:
                                chunk = fh.read(min(left, max(igulp - len(carry), 1 << 20)))
                                if not chunk:
                                    break
                                left -= len(chunk)
                                carry += chunk
                                while len(carry) >= igulp:
                                    with oseq.reserve(igulp) as sp:
                                        sp.data[...] = np.frombuffer(carry[:igulp], dtype=np.uint8)
                                    carry = carry[igulp:]
                    # (a trailing partial gulp is dropped)
