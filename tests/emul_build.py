"""Builds an emulation driver (tests/<engine>_emul/driver.cpp) twice from the same source, each a program of its own with the
sanitizer's runtime inside the program: once with -fsanitize=address,undefined (a word outside a buffer, an undefined operation)
and once with -fsanitize=thread (two threads of a work-group touching a word with no barrier between them).  Nothing is loaded
into Python under a sanitizer and no environment variable is set for a run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc")
BUILDS = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}


def build_both(workdir, emul, include_dirs):
    """{"asan": exe, "tsan": exe} of <emul>/driver.cpp; include_dirs come before <emul> (for <hip/hip_runtime.h>)."""
    exes = {}
    for name, flags in BUILDS.items():
        exe = os.path.join(str(workdir), "driver_" + name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing", "-pthread"] + flags + ["-Wno-unknown-pragmas"]
        for d in list(include_dirs) + [emul]:
            cmd += ["-I", str(d)]
        subprocess.check_call(cmd + [os.path.join(emul, "driver.cpp"), "-o", exe])
        exes[name] = exe
    return exes


def run(exe, *args):
    """The driver's stdout; a sanitizer report or a difference from the expectation is a non-zero status and fails here."""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "%s ended with status %d:\n%s" % (os.path.basename(exe), r.returncode, r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout
