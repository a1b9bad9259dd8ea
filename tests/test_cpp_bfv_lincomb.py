"""The C++ mirror of mkhe_bfv_ct_lincomb (include/mkhe.hpp: mkbfv::Evaluator::LinCombs) compiles without warnings under the flags of
test_cpp_bfv_mulrelin_sum.py and links against the C ABI (no GPU: nothing is called); on a GPU the same program checks the wrapper against the C
call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def _build(tmp_path, sanitize):
    """sanitize: UBSan for the link check, which touches no GPU; the program that runs on the GPU is built without any sanitizer"""
    exe = str(tmp_path / "bfv_lincomb_check")
    flags = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bfv_lincomb_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined"])
    return exe


def test_cpp_bfv_lincomb_mirror_compiles_and_links(tmp_path):
    out = subprocess.run([_build(tmp_path, sanitize=True)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "bfv lincomb mirror links" in out.stdout


@pytest.mark.gpu
def test_cpp_bfv_lincomb_wrapper_equals_the_c_call(tmp_path):
    out = subprocess.run([_build(tmp_path, sanitize=False), "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bfv lincomb mirror ok" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
