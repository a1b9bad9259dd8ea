"""The C++ mirror of the threshold secret keys (include/mkhe.hpp: mkrlwe::SecretKeyShare, Thresholdizer, Combiner and Decryptor::FoldShares, through
the mkrlwe, mkckks and mkbfv Decryptors) compiles without warnings under the flags of test_cpp_pcks.py and links against the C ABI (no GPU: no
engine call is made)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def test_cpp_threshold_mirror_compiles_and_links(tmp_path):
    exe = str(tmp_path / "threshold_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "threshold_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("threshold mirror links"), out.stdout[-300:] + out.stderr[-300:]
    assert "1536.0" in out.stdout                               # FloodBound(2 - 1 + 2, 10) = 3 * 2^9
