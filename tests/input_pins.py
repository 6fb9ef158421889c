"""Pins for the "never written" contract of include/xeng.h: remember the exact bytes uploaded to a device buffer and compare
them with a download after the engine's Sync.

The comparison is on uint8 -- never on floats: a NaN whose payload changed and a -0.0 that became +0.0 are writes.  On a mismatch
the message names the buffer, the count of differing bytes, the first byte offset and the expected and found values there; the
offset maps back to (sample, channel, input) of the buffer's layout, which is how the kernel at fault is found.

A buffer is anything with download(dtype, count, offset) (ffi.DeviceBuffer, or a stand-in on the CPU: tests/test_input_pins_cpu.py)
or a `Guarded` of tests/test_guard_bands_gpu.py, whose guard bands are then checked in the same breath."""
import numpy as np


def as_bytes(arr):
    """the exact bytes of an array (or bytes-like) as a flat uint8 copy"""
    if isinstance(arr, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    return np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()


def assert_same_bytes(name, expected, found):
    """expected, found: arrays of any dtype; equal means byte for byte"""
    e, f = as_bytes(expected), as_bytes(found)
    assert e.size == f.size, "%s: %d bytes downloaded where %d were uploaded" % (name, f.size, e.size)
    bad = np.flatnonzero(e != f)
    if bad.size:
        o = int(bad[0])
        raise AssertionError("%s: input was WRITTEN: %d of %d bytes differ, first at byte offset %d (expected 0x%02x, found 0x%02x)"
                             % (name, bad.size, e.size, o, e[o], f[o]))


class Pin:
    """the bytes that `buf` held at [offset, offset + len) when it was uploaded; check() downloads them again"""

    def __init__(self, name, buf, data, offset=0):
        self.name, self.buf, self.offset = name, buf, int(offset)
        self.want = as_bytes(data)

    def found(self):
        if hasattr(self.buf, "payload"):                     # a Guarded: bands first, then the payload between them
            self.buf.check(self.name)
            return self.buf.payload(np.uint8)[self.offset:self.offset + self.want.size]
        return self.buf.download(np.uint8, self.want.size, self.offset)

    def check(self):
        assert_same_bytes(self.name, self.want, self.found())


def upload(name, buf, data, offset=0):
    """upload `data` into an ffi.DeviceBuffer and pin it"""
    buf.upload(as_bytes(data), offset)
    return Pin(name, buf, data, offset)


def guarded(ffi, name, data):
    """a fresh input of the test's own between two guard bands (tests/test_guard_bands_gpu.Guarded), uploaded and pinned;
    returns (Guarded, Pin)"""
    from tests.test_guard_bands_gpu import Guarded
    raw = as_bytes(data)
    g = Guarded(ffi, raw.size)
    ffi.call("xengMemcpy", g.ptr, raw.ctypes.data, raw.nbytes)
    return g, Pin(name, g, raw)


class Pins:
    """the pins of one test: add as you upload, check_all() after the Sync"""

    def __init__(self):
        self.pins = []

    def add(self, name, buf, data, offset=0):
        self.pins.append(Pin(name, buf, data, offset))
        return buf

    def upload(self, name, buf, data, offset=0):
        self.pins.append(upload(name, buf, data, offset))
        return buf

    def guarded(self, ffi, name, data):
        g, p = guarded(ffi, name, data)
        self.pins.append(p)
        return g

    def check_all(self):
        assert self.pins, "nothing was pinned"
        for p in self.pins:
            p.check()


class Recorder:
    """Pins every upload made through a buffer class while `recording` is in force: the engine's own test helpers (the `.din` and
    friends they own) upload their inputs as they always do, and each buffer is held to its uploaded bytes
      - before the next upload overwrites them (the helpers sync before they hand a result back, so the call that read them is over),
      - before the buffer is freed, and
      - when the recording ends, for every buffer still alive.
    A buffer that the engine is meant to write (an accumulator whose start value was uploaded) is taken out with release()."""

    def __init__(self):
        self.live = {}                   # id(buf) -> (buf, name, {offset: bytes})
        self.nchecked = 0                # uploads that were compared after use
        self.names = []
        self.failures = []               # messages of checks that failed inside a free()

    def _name(self, buf, depth):
        import os
        import sys
        f = sys._getframe(depth)
        owner = f.f_locals.get("self")
        attr = [k for k, v in vars(owner).items() if v is buf] if owner is not None and hasattr(owner, "__dict__") else []
        local = [k for k, v in f.f_locals.items() if v is buf]
        what = "%s.%s" % (type(owner).__name__, attr[0]) if attr else (local[0] if local else "buffer")
        return "%s of %d bytes (uploaded at %s:%d)" % (what, buf.nbytes, os.path.basename(f.f_code.co_filename), f.f_lineno)

    def uploaded(self, buf, data, offset, depth=2):
        raw = as_bytes(data)
        _, _, parts = self.live.get(id(buf), (None, None, {}))
        parts = {o: b for o, b in parts.items() if o + b.size <= offset or o >= offset + raw.size}      # (what this upload replaces)
        parts[int(offset)] = raw
        name = self._name(buf, depth + 1)
        self.live[id(buf)] = (buf, name, parts)
        self.names.append(name)

    def check(self, buf):
        if id(buf) not in self.live or not buf.ptr:
            return
        _, name, parts = self.live[id(buf)]
        for offset, want in sorted(parts.items()):
            assert_same_bytes("%s at +%d" % (name, offset) if offset else name, want, buf.download(np.uint8, want.size, offset))
            self.nchecked += 1

    def release(self, buf):
        self.live.pop(id(buf), None)

    def check_all(self):
        for buf, _, _ in list(self.live.values()):
            self.check(buf)


class recording:
    """with recording(ffi.DeviceBuffer) as rec: ... -- see Recorder"""

    def __init__(self, cls):
        self.cls, self.rec = cls, Recorder()

    def __enter__(self):
        cls, rec = self.cls, self.rec
        self.saved = (cls.upload, cls.free)
        upload0, free0 = self.saved

        def upload(buf, arr, offset=0):
            rec.check(buf)
            out = upload0(buf, arr, offset)
            rec.uploaded(buf, arr, offset)
            return out

        def free(buf):
            try:
                rec.check(buf)
            except AssertionError as e:         # (a free from __del__ swallows exceptions: kept, and raised when the recording ends)
                rec.failures.append(str(e))
                raise
            finally:
                rec.release(buf)
                free0(buf)

        cls.upload, cls.free = upload, free
        return rec

    def __exit__(self, etype, exc, tb):
        self.cls.upload, self.cls.free = self.saved
        if etype is None:
            self.rec.check_all()
            assert not self.rec.failures, self.rec.failures[0]
        return False
