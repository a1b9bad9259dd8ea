"""The C++ mirror of the BFV plaintext linear transform (include/mkhe.hpp: mkbfv::LinearTransform, mkbfv::Evaluator::HoistedForm / RotateHoistedNew /
LinearTransformNew over mkhe_bfv_ct_ptxt_dot) compiles without warnings under the flags of test_cpp_bfv_ptxt.py and links against the C ABI (no GPU:
nothing is called); on a GPU the same program checks the wrappers against the single calls, bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def _build(tmp_path, sanitize):
    """sanitize: UBSan for the link check, which touches no GPU; the program that runs on the GPU is built without any sanitizer"""
    exe = str(tmp_path / "bfv_lintrans_check")
    flags = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bfv_lintrans_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined"])
    return exe


def test_cpp_bfv_lintrans_mirror_compiles_and_links(tmp_path):
    out = subprocess.run([_build(tmp_path, sanitize=True)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "bfv lintrans mirror links" in out.stdout


@pytest.mark.gpu
def test_cpp_bfv_lintrans_wrappers_equal_the_single_calls(tmp_path):
    out = subprocess.run([_build(tmp_path, sanitize=False), "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bfv lintrans mirror ok" in out.stdout, out.stdout[-1500:] + out.stderr[-500:]
