"""AddressSanitizer + UBSan over the HOST half of ph_ramanujan_select: period_hip.hip compiled host-only with
-fsanitize=address,undefined and linked against tests/hipstub/hip_stub.cpp (host memory in place of the HIP runtime;
kernels do not run) and the stand-alone driver tests/hipstub/host_driver_ram_select.cpp (its own main) -- built and run
exactly as tests/test_host_sanitizers.py builds its drivers.  The driver goes through every refusal, the staging with
and without reference levels, pcap = 2^20 and the size arithmetic with W * (q_hi + 1) * 8 beyond 2^31.  Nothing is
loaded into python."""
import os
import subprocess

import pytest

from test_host_sanitizers import CLANG, HIPCC, ROOT, SAN, STUB, host_objects  # noqa: F401  (the module's fixture)

DRIVER, DONE = "host_driver_ram_select", "host sanitizer driver ram_select ok"


@pytest.mark.skipif(not os.path.exists(HIPCC) or not os.path.exists(CLANG), reason="ROCm clang not available")
def test_ram_select_host_half_under_asan_ubsan(host_objects):  # noqa: F811
    tmp, objects = host_objects
    exe = str(tmp / DRIVER)
    # plain clang++ link: no HIP runtime library on the line, the stub provides the symbols
    cmd = [CLANG, *SAN, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(STUB, DRIVER + ".cpp"), *objects,
           "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert DONE in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
