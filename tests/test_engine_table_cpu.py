"""ffi.ENGINES, the table of the engines on the beamformer's stream, row by row: the symbols each row stands for are declared in
include/xeng.h, exported by the library and bound with the right handle; HipBackend has the methods made from the row; and, on a
machine without a GPU, the entry points shared by every engine keep the status contract of beam_context_* (csrc/xeng_util.hip):
a null result pointer is INVALID_ARGUMENT before the context is looked at, a missing context INVALID_STATE with the engine's name
in the message, Destroy of nothing succeeds."""
import ctypes
import os
import re

import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.backend import HipBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
IDS = [row[0] for row in ffi.ENGINES]


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xeng.h")).read(), flags=re.S)
    return set(re.findall(r"\b(xeng[A-Z]\w*)\s*\(", src))


DECLARED = _declared()


def test_the_table_lists_each_engine_once():
    assert len(ffi.ENGINES) == 19
    assert len(set(IDS)) == 19 and len({row[1] for row in ffi.ENGINES}) == 19
    assert sum(1 for row in ffi.ENGINES if row[2]) == 15
    assert "Beamform" not in IDS                                    # (a native binding of its own: beam_mark / beam_wait / beam_sync)
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))


@pytest.mark.parametrize("cname,prefix,guards", ffi.ENGINES, ids=IDS)
def test_symbols_and_methods_of_a_row(cname, prefix, guards):
    L = ctypes.CDLL(ffi.LIB_PATH)
    protos = {"Mark": [ctypes.POINTER(ctypes.c_ulonglong)], "Wait": [ctypes.c_ulonglong], "TicketDone": [ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_int)],
              "Sync": [], "Destroy": []}
    if guards:
        protos["CheckGuards"] = [ctypes.POINTER(ctypes.c_int)]
    for what, args in protos.items():
        name = "xeng%s%s" % (cname, what)
        assert hasattr(L, name), "libxeng.so does not export %s" % name
        assert name in DECLARED, "include/xeng.h does not declare %s" % name
        assert ffi.SYMBOLS[name] == args, name
        assert (name in ffi.ENQUEUE_ONLY) == (what in ("Mark", "TicketDone")), name
    assert ("xeng%sCheckGuards" % cname in DECLARED) == guards
    for m in ("mark", "wait", "ticket_done", "sync"):
        f = getattr(HipBackend, "%s_%s" % (prefix, m))
        assert callable(f) and f.__doc__ and f.__name__ == "%s_%s" % (prefix, m)
        assert "%s_%s" % (prefix, m) in vars(HipBackend)            # (an attribute of the class, not a lookup hook)
    assert hasattr(HipBackend, prefix + "_guards_intact") == guards
    if guards:
        assert callable(getattr(HipBackend, prefix + "_guards_intact")) and getattr(HipBackend, prefix + "_guards_intact").__doc__


@pytest.mark.parametrize("cname,prefix,guards", ffi.ENGINES, ids=IDS)
def test_status_contract_of_a_row_without_a_gpu(cname, prefix, guards):
    n = ctypes.c_int(-1)
    if ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    x = "xeng" + cname
    t, d = ctypes.c_ulonglong(), ctypes.c_int()
    null = [(x + "Mark", (None,)), (x + "TicketDone", (1, None))]
    missing = [(x + "Mark", (ctypes.byref(t),)), (x + "Wait", (1,)), (x + "TicketDone", (1, ctypes.byref(d))), (x + "Sync", ())]
    if guards:
        null.append((x + "CheckGuards", (None,)))
        missing.append((x + "CheckGuards", (ctypes.byref(d),)))
    for name, args in null:
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, name
        assert (": %s%s: null " % (cname, name[len(x):])) in str(ei.value), str(ei.value)
    for name, args in missing:
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
        assert (": %s: not initialized" % cname) in str(ei.value), str(ei.value)
    assert getattr(ffi.lib(), x + "Destroy")() == 0
