"""The owner of a Context's device allocations (csrc/device_memory.h) as a host program: tests/cpp/device_memory_check.cpp includes the header,
supplies the five HIP entry points it uses on top of malloc / free / memcpy (the n-th hipMalloc or hipMemcpy can be made to fail) and walks upload of an
empty vector, alloc / free, mark / rollback after a failed allocation and after a failed copy, grow, release twice and destruction with blocks held.
Built with AddressSanitizer and UBSan and run with leak detection on: a double free, a use after free or a block left behind fails the test.
A stand-alone program with its own main: the sanitizer runtime is linked into it (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def _gcc_file(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True, check=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_device_memory_owner_under_asan_and_ubsan(tmp_path):
    if not _gcc_file("libasan.so"):
        pytest.skip("no libasan in this toolchain")
    exe = str(tmp_path / "device_memory_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-isystem", ROCM_INCLUDE, "-I", os.path.join(ROOT, "mkhe-kklss_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "device_memory_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    assert out.stdout.strip().endswith("device memory owner ok")
    assert out.stderr.strip() == "", out.stderr[-3000:]          # (the program writes there only when a check fails; so do the sanitizers)
