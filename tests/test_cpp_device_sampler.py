"""The C++ mirror of the device sampler (include/mkhe.hpp: mkrlwe::small_cdt, DeviceSampler, the seeded overloads of Encryptor) compiles without
warnings under the flags of test_cpp_mirror.py and links against the C ABI; its small_cdt(3.2) is the Python mirror's (no GPU: no engine call is
made).  Both tables are float64 arithmetic on erfc: they may differ where two libm differ in the last place, 2^11 at the top of the table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def test_cpp_device_sampler_mirror_compiles_links_and_builds_the_table(tmp_path):
    from mkhe_kklss_amd import mkrlwe
    exe = str(tmp_path / "device_sampler_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "device_sampler_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("device sampler mirror links"), out.stdout[-300:] + out.stderr[-300:]
    table = [int(l) for l in out.stdout.split()[:38]]
    want = mkrlwe.small_cdt(3.2)
    assert len(want) == 38 and all(a < b for a, b in zip(table, table[1:]))
    assert all(abs(a - b) <= 1 << 14 for a, b in zip(table, want))
