"""small_sample_kernel on the ISA hipcc makes for gfx950 (no GPU): integer ALU work out of registers -- no scratch, no LDS, no spill, eight waves
per SIMD -- whose only memory instructions are its stores: key, nonce and table come from the kernel arguments through scalar loads, and the table
scan is a run of 64-bit unsigned compares with no vector branch."""
import os

import pytest

from isa_static import HIPCC, compile_asm, resources
from isa_static import ops as kernel_ops


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_small_sample_kernel_resources_and_memory_instructions():
    asm = compile_asm("encdec_kernels.hip")
    ops = kernel_ops(asm, "small_sample_kernel")
    memory = sorted({o for o in ops if o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_"))})
    assert memory == ["global_store_dwordx4"], memory
    assert any(o.startswith("s_load_dwordx2") for o in ops)                                       # the table, one threshold at a time
    assert sum(o.startswith(("v_cmp_le_u64", "v_cmp_ge_u64")) for o in ops) >= 8                  # r >= T on all 64 bits, eight coefficients
    # behind the bounds check at the entry (the only place where lanes differ) every branch is scalar: on the kind, on the loop counters
    assert [o for o in ops if o.startswith("s_cbranch_exec")] == ["s_cbranch_execz"], [o for o in ops if o.startswith("s_cbranch")]
    val = resources(asm, "small_sample_kernel")
    print("small_sample_kernel: %d VGPRs, %d SGPRs" % (val["vgpr_count"], val["sgpr_count"]))
    assert val["vgpr_count"] <= 64 and val["vgpr_spill_count"] == 0 and val["sgpr_spill_count"] == 0
    assert val["private_segment_fixed_size"] == 0 and val["group_segment_fixed_size"] == 0
