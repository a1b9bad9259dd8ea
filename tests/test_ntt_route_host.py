"""The route of an NTT launch (csrc/ntt_route.h: which kernels, in which order, on which slots, under which timing class) on both sides of every
size threshold of the dispatch, printed by a standalone host program (tests/cpp/ntt_route_check.cpp: g++ alone, sanitizers on, no library)
and compared with the literal below.  One modulus per launch unless the row says otherwise, so that the limb count is the class's count.

Where the expected text comes from: the rows `fwd 2^N limbs=C` and `inv 2^N limbs=C` are the kernels, grids and order that the library
launched for mkhe_ntt of C polynomials under one modulus BEFORE the dispatch was gathered into ntt_route.h (kernel trace of the parent commit;
tests/test_gpu_ntt_routes.py runs the same shapes against the oracle; the big-modulus row: modulus 0 of the same run).  DERIVED BY HAND from
the earlier code, not traced: the `decompose` rows, the prestaged rows (N = 2^16 behind decomp_spread_kernel), the 65536-limb and nouter caps, the no_h16 contexts, the merged inverse launches counted by vi_jobs, and the `thresholds at 1` rows (MKHE_NTT16_MIN =
MKHE_NTT14_MIN = MKHE_NTT16_INV_MIN = 1, what tests/test_gpu_forced_paths.py sets).  DESIGN.md section 4.1a shows the same table."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
fwd 2^13 limbs=128: [small fwd: split_fwd(2^13 split=0 jobs=128 src->dst) fwd_reg(2^12 split=1 jobs=256 in-place)]
fwd 2^13 limbs=129: [small fwd: fwd_reg(2^13 split=0 jobs=129 src->dst)]
fwd 2^14 limbs=63: [small fwd: pass8_fwd(2^14 split=0 jobs=63 src->dst) fwd_lds(2^11 split=1 depth=3 jobs=504 in-place)]
fwd 2^14 limbs=64: [small fwd: pass4_fwd(2^14 split=0 jobs=64 src->dst) fwd_lds(2^12 split=1 depth=2 jobs=256 in-place)]
fwd 2^14 limbs=127: [small fwd: pass4_fwd(2^14 split=0 jobs=127 src->dst) fwd_lds(2^12 split=1 depth=2 jobs=508 in-place)]
fwd 2^14 limbs=128: [big16+small16 h16_fwd: h14_fwd(2^14 split=0 jobs=128 src->dst)]
fwd 2^14 limbs=129: [big16+small16 h16_fwd: h14_fwd(2^14 split=0 jobs=129 src->dst)]
fwd 2^15 limbs=127: [small fwd: pass8_fwd(2^15 split=0 jobs=127 src->dst) fwd_lds(2^12 split=1 depth=3 jobs=1016 in-place)]
fwd 2^15 limbs=128: [big16+small16 h16_fwd: h16_fwd(2^15 split=0 jobs=128 src->dst)]
fwd 2^15 limbs=511: [big16+small16 h16_fwd: h16_fwd(2^15 split=0 jobs=511 src->dst)]
fwd 2^15 limbs=512: pick{h32|h16} [big16+small16+u h32_fwd: h32_fwd(2^15 split=0 jobs=512 src->dst)] [big16+small16 h16_fwd: h16_fwd(2^15 split=0 jobs=512 src->dst)]
fwd 2^16 limbs=63: [small fwd: split_fwd(2^16 split=0 jobs=63 src->dst) fwd_reg(2^15 split=1 jobs=126 in-place)]
fwd 2^16 limbs=64: [small fwd: pass4_fwd(2^16 split=0 jobs=64 src->dst) h14_split(2^14 split=2 jobs=256 in-place)]
fwd 2^15 limbs=127 big-modulus class: [big fwd_bigq: pass8_fwd(2^15 split=0 jobs=127 src->dst) fwd_lds(2^12 split=1 depth=3 jobs=1016 in-place)]
fwd 2^16 limbs=63 prestaged=1: [small fwd: fwd_reg(2^15 split=1 jobs=126 in-place)]
  prestaged launch on the H16 sub-transform kernel: no
fwd 2^16 limbs=63 prestaged=1 out of place: throws mkhe: internal: out-of-place prestaged launch outside the H16 path
fwd 2^16 limbs=63 prestaged=2: throws mkhe: internal: radix-4 prestaged launch outside the H16 path
fwd 2^16 limbs=64 prestaged=1: [small fwd: h16_split(2^15 split=1 jobs=128 in-place)]
  prestaged launch on the H16 sub-transform kernel: yes
fwd 2^16 limbs=64 prestaged=1 out of place: [small fwd: h16_split(2^15 split=1 jobs=128 src->dst)]
fwd 2^16 limbs=64 prestaged=2: [small h14_split: h14_split(2^14 split=2 jobs=256 in-place)]
decompose 2^15 16 slots x 56: pick{h32|h16} [big16+small16+u h32_decomp: h32_fwd<dec>(2^15 split=0 jobs=896 src->dst)] [big16+small16 h16_decomp: h16_fwd<dec>(2^15 split=0 jobs=896 src->dst)]
decompose 2^14 8 slots x 24: [big16+small16 h16_decomp: h14_fwd<dec>(2^14 split=0 jobs=192 src->dst)]
fwd 2^15 1 slot x 65535: pick{h32|h16} [big16+small16+u h32_fwd: h32_fwd(2^15 split=0 jobs=65535 src->dst)] [big16+small16 h16_fwd: h16_fwd(2^15 split=0 jobs=65535 src->dst)]
fwd 2^15 1 slot x 65536 (nouter cap): [small fwd: fwd_reg(2^15 split=0 jobs=65536 src->dst)]
fwd 2^15 2 slots x 32768 (limb cap): [small fwd: fwd_reg(2^15 split=0 jobs=65536 src->dst)]
fwd 2^14 2 slots x 32768 (limb cap): [small fwd: fwd_reg(2^14 split=0 jobs=65536 src->dst)]
fwd 2^16 2 slots x 32768 (limb cap): [small fwd: split_fwd(2^16 split=0 jobs=65536 src->dst) fwd_reg(2^15 split=1 jobs=131072 in-place)]
decompose 2^15 no_h16 1 big + 3 small slots x 128: [big decomp_bigq side: pass8_fwd<dec>(2^15 split=0 jobs=128 src->dst) fwd_lds(2^12 split=1 depth=3 jobs=1024 in-place)] [small decomp: fwd_reg<dec>(2^15 split=0 jobs=384 src->dst)]
decompose 2^15 no_h16 1 big + 3 small slots x 129: [big+small decomp_mixed: fwd_mixed<dec>(2^15 split=0 jobs=516 src->dst)]
decompose 2^15 no_h16 4 small slots x 129: [small decomp: fwd_reg<dec>(2^15 split=0 jobs=516 src->dst)]
fwd 2^16 limbs=64 no_h16: [small fwd: split_fwd(2^16 split=0 jobs=64 src->dst) fwd_reg(2^15 split=1 jobs=128 in-place)]
inv 2^13 limbs=128: [all inv: inv_reg(2^12 split=1 jobs=256 src->dst) split_inv(2^13 split=1 jobs=128 in-place)]
inv 2^13 limbs=129: [all inv: inv_reg(2^13 split=0 jobs=129 src->dst)]
inv 2^14 limbs=63: [all inv: inv_lds(2^11 split=0 depth=3 jobs=504 src->dst) pass8_inv(2^14 split=1 jobs=63 in-place)]
inv 2^14 limbs=64: [all inv: inv_lds(2^12 split=0 depth=2 jobs=256 src->dst) pass4_inv(2^14 split=1 jobs=64 in-place)]
inv 2^14 limbs=128: [all inv: inv_lds(2^12 split=0 depth=2 jobs=512 src->dst) pass4_inv(2^14 split=1 jobs=128 in-place)]
inv 2^14 limbs=129: [all inv: h14_inv(2^14 split=0 jobs=129 src->dst)]
inv 2^15 limbs=127: [all inv: inv_lds(2^12 split=0 depth=3 jobs=1016 src->dst) pass8_inv(2^15 split=1 jobs=127 in-place)]
inv 2^15 limbs=128: [all inv: h14_inv(2^14 split=1 jobs=256 src->dst) split_inv(2^15 split=0 jobs=128 in-place)]
inv 2^16 limbs=63: [all inv: inv_reg(2^15 split=1 jobs=126 src->dst) split_inv(2^16 split=1 jobs=63 in-place)]
inv 2^16 limbs=64: [all inv: h14_inv(2^14 split=2 jobs=256 src->dst) pass4_inv(2^16 split=0 jobs=64 in-place)]
inv 2^14 merged 8 slots x 20, 128 jobs: [all inv: inv_lds(2^12 split=0 depth=2 jobs=640 src->dst) pass4_inv(2^14 split=1 jobs=160 in-place)]
inv 2^14 merged 8 slots x 20, 129 jobs: [all inv: h14_inv(2^14 split=0 jobs=160 src->dst)]
inv 2^14 2 slots x 32768 (limb cap): [all inv: inv_reg(2^14 split=0 jobs=65536 src->dst)]
inv 2^15 limbs=128 no_h16: [all inv: inv_lds(2^12 split=0 depth=3 jobs=1024 src->dst) pass8_inv(2^15 split=1 jobs=128 in-place)]
thresholds at 1: fwd 2^14 limbs=1: [big16+small16 h16_fwd: h14_fwd(2^14 split=0 jobs=1 src->dst)]
thresholds at 1: inv 2^14 limbs=1: [all inv: inv_lds(2^11 split=0 depth=3 jobs=8 src->dst) pass8_inv(2^14 split=1 jobs=1 in-place)]
thresholds at 1: fwd 2^15 limbs=1: [big16+small16 h16_fwd: h16_fwd(2^15 split=0 jobs=1 src->dst)]
thresholds at 1: inv 2^15 limbs=1: [all inv: h14_inv(2^14 split=1 jobs=2 src->dst) split_inv(2^15 split=0 jobs=1 in-place)]
thresholds at 1: fwd 2^16 limbs=1: [small fwd: pass4_fwd(2^16 split=0 jobs=1 src->dst) h14_split(2^14 split=2 jobs=4 in-place)]
thresholds at 1: inv 2^16 limbs=1: [all inv: h14_inv(2^14 split=2 jobs=4 src->dst) pass4_inv(2^16 split=0 jobs=1 in-place)]
"""


def _routes(tmp_path):
    exe = str(tmp_path / "ntt_route_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "mkhe-kklss_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "ntt_route_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    return out.stdout


def test_route_of_every_threshold(tmp_path):
    got = _routes(tmp_path).splitlines()
    want = EXPECTED.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_design_md_shows_the_same_table(tmp_path):
    """DESIGN.md section 4.1a (shape -> steps) is this program's output, line for line"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        doc = f.read()
    for line in _routes(tmp_path).splitlines():
        assert line.rstrip() in doc, line


def test_route_header_stands_alone():
    """ntt_route.h includes no HIP header and reads no environment: the decision is a function of its two arguments"""
    with open(os.path.join(ROOT, "mkhe-kklss_amd", "csrc", "ntt_route.h")) as f:
        src = f.read()
    assert re.findall(r"#include\s+(\S+)", src) == ["<stdexcept>"] and "getenv" not in src and "MKHE_AB_INT" not in src
