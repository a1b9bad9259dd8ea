"""small_sample_kernel on the ISA hipcc makes for gfx950 (no GPU): integer ALU work out of registers -- no scratch, no LDS, no spill, eight waves
per SIMD -- whose only memory instructions are its stores: key, nonce and table come from the kernel arguments through scalar loads, and the table
scan is a run of 64-bit unsigned compares with no vector branch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_small_sample_kernel_resources_and_memory_instructions():
    src = os.path.join(ROOT, "mkhe-kklss_amd", "csrc", "encdec_kernels.hip")
    r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only",
                        src, "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-1500:]
    name = [n for n in re.findall(r"^(\S*small_sample_kernel\S*):", r.stdout, re.M)]
    assert len(name) == 1, name
    body = r.stdout.split(name[0] + ":", 1)[1].split("s_endpgm", 1)[0]
    code = [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith((";", ".", "//")) and not l.strip().endswith(":")]
    ops = [l.split()[0] for l in code]
    memory = sorted({o for o in ops if o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_"))})
    assert memory == ["global_store_dwordx4"], memory
    assert any(o.startswith("s_load_dwordx2") for o in ops)                                       # the table, one threshold at a time
    assert sum(o.startswith(("v_cmp_le_u64", "v_cmp_ge_u64")) for o in ops) >= 8                  # r >= T on all 64 bits, eight coefficients
    # behind the bounds check at the entry (the only place where lanes differ) every branch is scalar: on the kind, on the loop counters
    assert [o for o in ops if o.startswith("s_cbranch_exec")] == ["s_cbranch_execz"], [o for o in ops if o.startswith("s_cbranch")]
    meta = [b for b in r.stdout.split("- .agpr_count:")[1:] if "small_sample_kernel" in b]
    assert len(meta) == 1
    val = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, meta[0]).group(1))
    print("small_sample_kernel: %d VGPRs, %d SGPRs" % (val("vgpr_count"), val("sgpr_count")))
    assert val("vgpr_count") <= 64 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0
    assert val("private_segment_fixed_size") == 0 and val("group_segment_fixed_size") == 0
