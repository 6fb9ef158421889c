"""The byte comparison behind the input pins (tests/input_pins.py), on a stand-in buffer: no GPU."""
import numpy as np
import pytest

from tests import input_pins


class FakeBuffer:
    """what ffi.DeviceBuffer offers the pins: upload(arr, offset) and download(dtype, count, offset) over host bytes"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.mem = np.full(nbytes, 0xEE, dtype=np.uint8)

    def upload(self, arr, offset=0):
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert offset + raw.size <= self.nbytes
        self.mem[offset:offset + raw.size] = raw
        return self

    def download(self, dtype, count=None, offset=0):
        dtype = np.dtype(dtype)
        if count is None:
            count = (self.nbytes - offset) // dtype.itemsize
        return self.mem[offset:offset + count * dtype.itemsize].copy().view(dtype)


class FakeGuarded:
    """what tests/test_guard_bands_gpu.Guarded offers the pins: check(what) and payload(dtype)"""

    def __init__(self, data):
        self.mem = input_pins.as_bytes(data)
        self.checked = []

    def check(self, what):
        self.checked.append(what)

    def payload(self, dtype):
        return self.mem.copy().view(dtype)


def _pinned(data, offset=0, slack=0):
    buf = FakeBuffer(offset + np.asarray(data).nbytes + slack)
    return buf, input_pins.upload("the input", buf, data, offset)


def test_untouched_bytes_pass():
    data = np.random.default_rng(0).integers(0, 256, 4099, dtype=np.uint8)
    buf, pin = _pinned(data, offset=64, slack=32)
    pin.check()
    buf.mem[63] ^= 1                                    # outside the pinned bytes: not this pin's business
    buf.mem[64 + data.size] ^= 1
    pin.check()


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bit", [0, 7])
def test_one_flipped_bit_at_either_end_is_named(where, bit):
    data = np.random.default_rng(1).integers(0, 256, 1000, dtype=np.uint8)
    buf, pin = _pinned(data, offset=16)
    o = 0 if where == "first" else data.size - 1
    buf.mem[16 + o] ^= 1 << bit
    with pytest.raises(AssertionError) as e:
        pin.check()
    msg = str(e.value)
    assert "the input" in msg and "1 of 1000 bytes differ" in msg
    assert "first at byte offset %d " % o in msg
    assert "expected 0x%02x, found 0x%02x" % (data[o], data[o] ^ (1 << bit)) in msg


def test_the_message_counts_every_byte_and_names_the_first():
    data = np.arange(4096, dtype=np.uint8)
    buf, pin = _pinned(data)
    for o in (777, 1500, 4000):
        buf.mem[o] = (int(buf.mem[o]) + 3) & 0xFF
    with pytest.raises(AssertionError) as e:
        pin.check()
    msg = str(e.value)
    assert "3 of 4096 bytes differ" in msg and "first at byte offset 777 " in msg
    assert "expected 0x%02x, found 0x%02x" % (777 & 0xFF, (777 + 3) & 0xFF) in msg


def test_a_nan_whose_payload_changed_counts():
    data = np.random.default_rng(2).standard_normal(64).astype(np.float32)
    data[5] = np.nan
    buf, pin = _pinned(data)
    pin.check()                                          # (NaN != NaN as floats; as bytes it is itself)
    words = buf.mem.view(np.uint32)
    assert words[5] == 0x7FC00000
    words[5] = 0x7FC00001                                # still a quiet NaN, another payload
    got = buf.download(np.float32)
    assert np.isnan(got[5]) and np.array_equal(np.isnan(got), np.isnan(data))
    with pytest.raises(AssertionError) as e:
        pin.check()
    assert "1 of 256 bytes differ" in str(e.value) and "first at byte offset 20 " in str(e.value)
    assert "expected 0x00, found 0x01" in str(e.value)


def test_negative_zero_against_positive_zero_counts():
    data = np.zeros(8, dtype=np.float32)
    data[3] = -0.0
    buf, pin = _pinned(data)
    pin.check()
    buf.upload(np.zeros(1, dtype=np.float32), 12)        # +0.0 over -0.0: equal as floats
    assert np.array_equal(buf.download(np.float32), data)
    with pytest.raises(AssertionError) as e:
        pin.check()
    assert "1 of 32 bytes differ" in str(e.value) and "first at byte offset 15 " in str(e.value)
    assert "expected 0x80, found 0x00" in str(e.value)


def test_complex_and_int_inputs_are_pinned_by_their_bytes():
    w = (np.arange(6) + 1j * np.arange(6)).astype(np.complex64)
    buf, pin = _pinned(w)
    pin.check()
    buf.mem[4 * 8 + 4] ^= 0x10                           # imaginary part of element 4
    with pytest.raises(AssertionError) as e:
        pin.check()
    assert "first at byte offset 36 " in str(e.value)


def test_a_guarded_buffer_has_its_bands_checked_in_the_same_breath():
    data = np.arange(100, dtype=np.uint8)
    g = FakeGuarded(data)
    pin = input_pins.Pin("guarded input", g, data)
    pin.check()
    assert g.checked == ["guarded input"]
    g.mem[99] ^= 0x80
    with pytest.raises(AssertionError) as e:
        pin.check()
    assert "guarded input" in str(e.value) and "first at byte offset 99 " in str(e.value)


def test_a_short_download_is_a_failure_not_a_pass():
    with pytest.raises(AssertionError):
        input_pins.assert_same_bytes("x", np.zeros(8, np.uint8), np.zeros(7, np.uint8))


def test_pins_collects_and_checks_all():
    pins = input_pins.Pins()
    with pytest.raises(AssertionError):
        pins.check_all()                                 # a test that pinned nothing has checked nothing
    a, b = FakeBuffer(16), FakeBuffer(16)
    pins.upload("a", a, np.arange(16, dtype=np.uint8))
    b.upload(np.arange(4, dtype=np.float32))
    pins.add("b", b, np.arange(4, dtype=np.float32))
    pins.check_all()
    b.mem[0] = 9
    with pytest.raises(AssertionError) as e:
        pins.check_all()
    assert str(e.value).startswith("b:")


class Helper:
    """an engine test helper in miniature: owns its input buffer, uploads per call, frees at close"""

    def __init__(self):
        self.din = FakeBuffer(64)
        self.din.ptr = 1
        self.freed = False

    def run(self, x, write_at=None):
        self.din.upload(x)
        if write_at is not None:                         # "the kernel" writes into its input
            self.din.mem[write_at] ^= 0x01

    def close(self):
        self.din.free()


def _fake_free(self):
    self.ptr = None


def test_recording_pins_every_upload_of_a_helper(monkeypatch):
    monkeypatch.setattr(FakeBuffer, "free", _fake_free, raising=False)
    x = np.arange(16, dtype=np.float32)
    with input_pins.recording(FakeBuffer) as rec:
        h = Helper()
        for k in range(3):
            h.run(x + k)
        h.close()
    assert rec.nchecked == 3 and h.din.ptr is None
    assert all(n.startswith("Helper.din of 64 bytes (uploaded at test_input_pins_cpu.py:") for n in rec.names)
    assert FakeBuffer.free is _fake_free                # (the hooks are gone)


@pytest.mark.parametrize("call,how", [(0, "next upload"), (2, "free"), (2, "end")])
def test_recording_catches_a_write_before_the_next_upload_the_free_and_at_the_end(monkeypatch, call, how):
    monkeypatch.setattr(FakeBuffer, "free", _fake_free, raising=False)
    x = np.arange(16, dtype=np.float32)
    with pytest.raises(AssertionError) as e:
        with input_pins.recording(FakeBuffer):
            h = Helper()
            for k in range(3):
                h.run(x + k, write_at=37 if k == call else None)
            if how == "free":
                h.close()
    assert "Helper.din" in str(e.value) and "first at byte offset 37 " in str(e.value)


def test_recording_keeps_partial_uploads_apart_and_lets_outputs_go(monkeypatch):
    monkeypatch.setattr(FakeBuffer, "free", _fake_free, raising=False)
    with input_pins.recording(FakeBuffer) as rec:
        buf = FakeBuffer(32)
        buf.ptr = 1
        buf.upload(np.full(8, 1, np.uint8), 0)
        buf.upload(np.full(8, 2, np.uint8), 16)
        buf.mem[10] = 0xFF                               # between the two uploads: nobody's input
        acc = FakeBuffer(8)
        acc.ptr = 1
        acc.upload(np.zeros(8, np.uint8))
        acc.mem[:] = 7                                   # an accumulator is written by design
        rec.release(acc)
    assert rec.nchecked == 3                             # (the first part once before the second upload, both at the end)
    with pytest.raises(AssertionError) as e:
        with input_pins.recording(FakeBuffer):
            buf = FakeBuffer(32)
            buf.ptr = 1
            buf.upload(np.full(8, 1, np.uint8), 0)
            buf.upload(np.full(8, 2, np.uint8), 16)
            buf.mem[17] = 0xFF
    assert "at +16" in str(e.value) and "first at byte offset 1 " in str(e.value)


def test_recording_keeps_a_failure_that_a_destructor_swallowed(monkeypatch):
    monkeypatch.setattr(FakeBuffer, "free", _fake_free, raising=False)
    with pytest.raises(AssertionError) as e:
        with input_pins.recording(FakeBuffer):
            h = Helper()
            h.run(np.arange(16, dtype=np.float32), write_at=5)
            try:                                         # (what ffi.DeviceBuffer.__del__ does around free())
                h.close()
            except Exception:
                pass
    assert "Helper.din" in str(e.value) and "first at byte offset 5 " in str(e.value)
    assert h.din.ptr is None                             # (freed all the same)
