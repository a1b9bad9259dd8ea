"""The C++ mirror of the device CKKS encoder with sparse packing (include/mkhe.hpp: mkckks::Encoder(params, logSlots)) compiles without warnings
under the flags of test_cpp_encoder.py and links against the C ABI (no GPU: nothing is called)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def test_cpp_sparse_encoder_mirror_compiles_and_links(tmp_path):
    exe = str(tmp_path / "sparse_encoder_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sparse_encoder_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "sparse encoder mirror links" in out.stdout
