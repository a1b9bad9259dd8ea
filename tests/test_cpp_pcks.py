"""The C++ mirror of the collective key switch to a recipient's public key (include/mkhe.hpp: mkrlwe / mkckks / mkbfv PublicKeySwitcher on
mkrlwe::PublicKeySwitchShare) compiles without warnings under the flags of test_cpp_bfv_refresh.py and links against the C ABI (no GPU: no engine
call is made)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def test_cpp_pcks_mirror_compiles_and_links(tmp_path):
    exe = str(tmp_path / "pcks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pcks_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("pcks mirror links"), out.stdout[-300:] + out.stderr[-300:]
    assert "118272.0" in out.stdout                             # NoiseBound(3, 10, 1024) = 3 (2^9 + 2 * 1024 * 19)
