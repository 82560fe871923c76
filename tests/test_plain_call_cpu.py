"""PlainCall's error-return rule and ctx_resolve, without a device (tests/plain_call_host/main.cpp): ctx.hip's host side compiled
into a stand-alone program whose HIP entry points are stubs that count and fail on request.  Nothing is loaded into this process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "plain_call_host", "main.cpp")
HIPCC = "/opt/rocm/bin/hipcc"


def test_plain_call_waits_on_error_returns_only_and_under_the_lock(tmp_path):
    exe = str(tmp_path / "plain_call_host")
    # the host side alone, and no HIP runtime in the link: every hip* symbol is the program's own
    r = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "hip", "--offload-host-only", "-no-hip-rt", SRC, "-o", exe, "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "plain_call_host ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
