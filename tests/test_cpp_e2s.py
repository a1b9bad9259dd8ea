"""The C++ mirror of "encryption to shares" and the BFV slot map (include/mkhe.hpp: mkrlwe / mkckks / mkbfv ShareConverter, SecretShare,
mkbfv::SlotMap, the map methods of mkbfv::Refresher): one C++17 program, tests/cpp/e2s_check.cpp, compiled without warnings under the flags of
test_cpp_mirror.py and linked against the C ABI.  Without a GPU it makes no engine call; on one (-m gpu) it runs the identity-map equality against
mkbfv::Refresher, one permuted refresh and the CKKS identity R~ + sum of the secret shares == Decrypt."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mkhe-kklss_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "e2s_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "e2s_check.cpp"), "-o", exe,
                           "-L", LIB, "-lmkhe_hip", "-Wl,-rpath," + LIB, "-Wl,--allow-shlib-undefined", "-pthread"])
    return exe


def test_cpp_e2s_mirror_compiles_and_links(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("e2s mirror links"), out.stdout[-300:] + out.stderr[-300:]


@pytest.mark.gpu
def test_cpp_e2s_mirror_runs(tmp_path):
    out = subprocess.run([build(tmp_path), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("e2s mirror runs"), out.stdout[-600:] + out.stderr[-600:]
