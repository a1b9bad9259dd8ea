"""The kernel of mkhe_ct_mod_raise on the ISA hipcc makes for gfx950 (no GPU): no spill, no scratch, no LDS, no barrier, no atomic; every load and
store of coefficients is a 16-byte one (the row access of ed_access.h).  The register counts are printed."""
import os

import pytest

from isa_static import HIPCC, compile_asm, ops, resources

KERNEL = "mod_raise_kernel"


@pytest.fixture(scope="module")
def asm():
    return compile_asm("modraise_kernels.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_no_spill_no_scratch_no_lds(asm):
    res = resources(asm, KERNEL)
    print("%s: %d VGPRs, %d SGPRs" % (KERNEL, res["vgpr_count"], res["sgpr_count"]))
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0
    assert res["private_segment_fixed_size"] == 0 and res["group_segment_fixed_size"] == 0
    assert res["vgpr_count"] <= 128                             # four waves per SIMD at least


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_streams_with_16_byte_accesses_only(asm):
    o = ops(asm, KERNEL)
    assert not [x for x in o if "atomic" in x or x.startswith("ds_") or x == "s_barrier"]
    vector = [x for x in o if x.startswith(("global_load", "global_store", "flat_load", "flat_store", "buffer_load", "buffer_store"))]
    assert vector and set(vector) <= {"global_load_dwordx4", "global_store_dwordx4"}, sorted(set(vector))
    assert vector.count("global_load_dwordx4") == 4             # the row of 8 coefficients is read once
