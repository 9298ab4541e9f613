"""csrc/lmpc_order.h on the host: the cross-stream ordering of a context's buffers (lmpc_capi.cpp, hoqp_capi.cpp) and the
grown device buffer, over an Api that logs its calls in place of HIP's."""
import subprocess


def test_order_host_check_under_sanitizers():
    """tests/cpp/order_host_check.cpp asserts the exact call sequence of every ordering case (one stream: no call at
    all; a stream change: one record, one wait; the host's waits; a failing record; a failed allocation); built by the
    host compiler with -fsanitize=address,undefined and run directly (nothing loaded into Python is instrumented)."""
    from legged_mpc_control_amd import build as B

    exe = B.build_cpp_order_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "order_host_check ok" in r.stdout and "runtime error" not in r.stderr
