"""The C++ mirror of the noise measures (include/mkhe.hpp: mkrlwe::NoiseValue, mkrlwe::Decryptor::NoiseNormBatch / NoiseNorm, mkckks::Decryptor,
mkbfv::Decryptor) compiles without warnings under the flags of test_cpp_pcks.py and links against the C ABI (no GPU: no engine call is made
beyond the refusal of a null context; the host arithmetic of NoiseValue is checked by the program itself)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def test_cpp_noise_mirror_compiles_and_links(tmp_path):
    exe = str(tmp_path / "noise_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "noise_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("noise mirror links"), out.stdout[-300:] + out.stderr[-300:]
    Q = 0x3fffffffd60001 * 0x3fffffff6d0001 * 0x3fffffff550001
    assert "%d %d\n" % (Q.bit_length() - 1, round(((Q - 1) // 2) / 1e40)) in out.stdout       # Bits() and Value() of (Q - 1) / 2
