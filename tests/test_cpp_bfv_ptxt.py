"""The C++ mirror of the BFV plaintext operands (include/mkhe.hpp: mkbfv::Encoder::EncodeMul, mkbfv::Evaluator::MulPtxtNew / AddPtxtNew /
SubPtxtNew) compiles without warnings under the flags of test_cpp_bfv_encoder.py and links against the C ABI (no GPU: nothing is called)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def test_cpp_bfv_ptxt_mirror_compiles_and_links(tmp_path):
    exe = str(tmp_path / "bfv_ptxt_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bfv_ptxt_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "bfv ptxt mirror links" in out.stdout
