"""legged_mpc_control_amd/build.py: what makes the library stale."""
import glob
import os

from conftest import ROOT

from legged_mpc_control_amd import build as B


def test_any_csrc_or_public_header_newer_than_the_library_makes_it_stale():
    """build_native's dependencies are listed from csrc/*.h and include/lmpc/*: a header newer than liblmpc.so makes
    _stale(LIB, ...) true, whichever header it is (a hand-kept list once missed one and left a stale library).  The
    header's times are moved past the library's and put back; nothing is rebuilt."""
    deps = B._library_deps()
    headers = sorted(glob.glob(os.path.join(B.CSRC, "*.h"))) + sorted(glob.glob(os.path.join(ROOT, "include", "lmpc", "*")))
    assert len(headers) > 20 and set(headers) <= set(deps)
    assert {os.path.join(B.CSRC, s) for s in B.SOURCES} <= set(deps)
    lib_time = os.path.getmtime(B.LIB)
    saved = {h: os.stat(h) for h in headers}
    try:
        for h in headers:
            os.utime(h, ns=(saved[h].st_atime_ns, int((lib_time - 10) * 1e9)))
        older = [d for d in deps if os.path.getmtime(d) < lib_time]
        assert set(headers) <= set(older) and not B._stale(B.LIB, older)
        for h in headers:
            os.utime(h, ns=(saved[h].st_atime_ns, int((lib_time + 10) * 1e9)))
            assert B._stale(B.LIB, older), h
            os.utime(h, ns=(saved[h].st_atime_ns, int((lib_time - 10) * 1e9)))
    finally:
        for h, st in saved.items():
            os.utime(h, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert all(os.stat(h).st_mtime_ns == st.st_mtime_ns for h, st in saved.items())
