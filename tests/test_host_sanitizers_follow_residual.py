"""AddressSanitizer + UBSan over the host half of ph_follow_residual, the way tests/test_host_sanitizers_follow.py does
it for ph_follow: period_hip.hip compiled host-only with -fsanitize=address,undefined, linked against
tests/hipstub/hip_stub.cpp (host memory in place of the HIP runtime; kernels do not run) and the stand-alone driver
tests/hipstub/host_driver_follow_residual.cpp (its own main): every refusal, pcap == 0 with NULL periods and counts, the
staging of host arrays with exact-size vectors, and the size arithmetic with f0 * hop and Wb * N beyond 2^31.  Nothing is
loaded into python."""
import os
import subprocess

import pytest

from test_host_sanitizers import CLANG, HIPCC, SAN, STUB, host_objects  # noqa: F401  (the fixture builds the objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER, OK_LINE = "host_driver_follow_residual", "host sanitizer driver follow_residual ok"


@pytest.mark.skipif(not os.path.exists(HIPCC) or not os.path.exists(CLANG), reason="ROCm clang not available")
def test_follow_residual_entry_point_under_asan_ubsan(host_objects):  # noqa: F811
    tmp, objects = host_objects
    exe = str(tmp / DRIVER)
    cmd = [CLANG, *SAN, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(STUB, DRIVER + ".cpp"), *objects,
           "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert OK_LINE in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
