"""The three kernels of the threshold secret keys on the ISA hipcc makes for gfx950 (no GPU): threshold_share_kernel keeps 8 THR_G accumulators and
the coefficient polynomials in registers, the other two stream, so none may spill, use scratch or touch LDS.  The register counts are printed
(DESIGN.md 4.5s quotes them): the share kernel at THR_G = 4 sits in the 129 .. 168 VGPR step (three waves per SIMD), the streaming kernels fit
eight waves per SIMD."""
import os

import pytest

from isa_static import HIPCC, compile_asm, resources


@pytest.fixture(scope="module")
def asm():
    return compile_asm("threshold_kernels.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel,vgprs", [("threshold_share_kernel", 168), ("threshold_scale_kernel", 64), ("limbs_sum_kernel", 64)])
def test_no_spill_no_scratch_no_lds(asm, kernel, vgprs):
    res = resources(asm, kernel)
    print("%s: %d VGPRs, %d SGPRs" % (kernel, res["vgpr_count"], res["sgpr_count"]))
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0
    assert res["private_segment_fixed_size"] == 0 and res["group_segment_fixed_size"] == 0
    assert res["vgpr_count"] <= vgprs
