"""The two kernels of distributed decryption on the ISA hipcc makes for gfx950 (no GPU): share_finish_kernel forms its flooding sample in
registers and share_merge_kernel streams, so neither may spill, use scratch or touch LDS; the finish kernel fits eight waves per SIMD.  The
register counts are printed (DESIGN.md 4.5i quotes them)."""
import os

import pytest

from isa_static import HIPCC, compile_asm, ops, resources


@pytest.fixture(scope="module")
def asm():
    return compile_asm("decshare_kernels.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel,vgprs", [("share_finish_kernel", 64), ("share_merge_kernel", 64)])
def test_no_spill_no_scratch_no_lds(asm, kernel, vgprs):
    res = resources(asm, kernel)
    print("%s: %d VGPRs, %d SGPRs" % (kernel, res["vgpr_count"], res["sgpr_count"]))
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0
    assert res["private_segment_fixed_size"] == 0 and res["group_segment_fixed_size"] == 0
    assert res["vgpr_count"] <= vgprs                           # eight waves per SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_memory_instructions_are_16_byte_global_accesses(asm):
    """key, nonce and the per-modulus constants come through scalar loads; what the lanes of share_finish_kernel touch in memory are the limbs,
    16 bytes at a time.  share_merge_kernel reads through pointers of a table (flat loads, and 8-byte loads of a staged table's entries)."""
    memory = lambda k: sorted({o for o in ops(asm, k) if o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_"))})
    assert memory("share_finish_kernel") == ["global_load_dwordx4", "global_store_dwordx4"], memory("share_finish_kernel")
    assert memory("share_merge_kernel") == ["flat_load_dwordx2", "flat_load_dwordx4", "global_store_dwordx4"], memory("share_merge_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_flood_is_reduced_without_a_lane_dependent_branch(asm):
    """behind the bounds check at the entry every branch of share_finish_kernel is scalar (on flood_bits, on the limb loop): the sign of a
    sample is folded in by selects"""
    o = ops(asm, "share_finish_kernel")
    assert [x for x in o if x.startswith("s_cbranch_exec")] == ["s_cbranch_execz"], [x for x in o if x.startswith("s_cbranch")]
    assert any(x.startswith("v_cndmask") for x in o)
