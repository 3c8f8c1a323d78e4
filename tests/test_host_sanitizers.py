"""AddressSanitizer + UBSan over the HOST half of libperiod_hip.so: period_hip.hip is compiled
host-only with -fsanitize=address,undefined -- once for the module -- and linked against tests/hipstub/hip_stub.cpp (host
memory in place of the HIP runtime; kernels do not run) and each of the stand-alone drivers under tests/hipstub/ (their
own main, the shared pieces in driver_common.h): host_driver.cpp goes through every entry point of the C ABI, the others
through one entry point's refusals, staging and size arithmetic each.  Nothing is loaded into python.
Round 1's advisor found an out-of-bounds read in a table check this way by hand; this keeps looking."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
STUB = os.path.join(ROOT, "tests", "hipstub")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17"]
# driver source -> the line it prints when every call returned what was expected
DRIVERS = {
    "host_driver": "host sanitizer driver ok",
    "host_driver_frames": "host sanitizer driver frames ok",
    "host_driver_get_periods": "host sanitizer driver get_periods ok",
    "host_driver_greedy_win": "host sanitizer driver greedy_win ok",
    "host_driver_tracks": "host sanitizer driver tracks ok",
    "host_driver_periodic": "host sanitizer driver periodic ok",
    "host_driver_ram_select": "host sanitizer driver ram_select ok",
    "host_driver_plans": "host sanitizer driver plans ok",
}


@pytest.fixture(scope="module")
def host_objects(tmp_path_factory):
    """The library's host half and the runtime stub as sanitized objects, and the link flags that go with them."""
    tmp = tmp_path_factory.mktemp("host_sanitizers")
    src = os.path.join(ROOT, "pyperiod_amd", "csrc", "period_hip.hip")
    obj, stub = str(tmp / "period_host.o"), str(tmp / "hip_stub.o")
    subprocess.run([HIPCC, "--cuda-host-only", *SAN, "-Wno-unused-function", "-c", src, "-o", obj], check=True, cwd=ROOT,
                   timeout=900)
    subprocess.run([CLANG, *SAN, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", os.path.join(STUB, "hip_stub.cpp"),
                    "-o", stub], check=True, cwd=ROOT, timeout=900)
    # the fat binary symbol the host object refers to (device code is not built here)
    nm = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout
    fat = [ln.split()[-1] for ln in nm.splitlines() if "__hip_fatbin" in ln]
    return tmp, [stub, obj] + [f"-Wl,--defsym,{s}=0" for s in fat]


@pytest.mark.skipif(not os.path.exists(HIPCC) or not os.path.exists(CLANG), reason="ROCm clang not available")
@pytest.mark.parametrize("driver", list(DRIVERS), ids=[d.replace("host_driver_", "") for d in DRIVERS])
def test_host_half_under_asan_ubsan(host_objects, driver):
    tmp, objects = host_objects
    exe = str(tmp / driver)
    # plain clang++ link: no HIP runtime library on the line, the stub provides the symbols
    cmd = [CLANG, *SAN, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(STUB, driver + ".cpp"), *objects,
           "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert DRIVERS[driver] in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
