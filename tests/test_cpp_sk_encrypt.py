"""The C++ mirror of secret-key encryption with a seeded c1 (include/mkhe.hpp: mkrlwe / mkckks / mkbfv SecretKeyEncryptor and SeededCiphertext)
compiles without warnings under the flags of test_cpp_pcks.py and links against the C ABI (no GPU: no engine call is made)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def test_cpp_sk_encrypt_mirror_compiles_and_links(tmp_path):
    exe = str(tmp_path / "sk_encrypt_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sk_encrypt_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("sk encrypt mirror links"), out.stdout[-300:] + out.stderr[-300:]
    assert "7340032 3670056" in out.stdout                      # a fresh PN15QP880 ciphertext on the wire: both polynomials, or c0 + seed + nonce
