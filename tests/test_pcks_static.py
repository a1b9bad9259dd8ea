"""The three kernels of the collective key switch to a recipient's public key on the ISA hipcc makes for gfx950 (no GPU): pcks_mac_kernel and
pcks_merge_kernel stream, pcks_finish_kernel forms the flood and e1 in registers, so none may spill, use scratch or touch LDS; each fits eight
waves per SIMD (at most 64 VGPRs: the occupancy step the printed counts fall under).  The register counts are printed (DESIGN.md 4.5m quotes
them)."""
import os

import pytest

from isa_static import HIPCC, compile_asm, resources


@pytest.fixture(scope="module")
def asm():
    return compile_asm("pcks_kernels.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel,vgprs", [("pcks_mac_kernel", 64), ("pcks_finish_kernel", 64), ("pcks_merge_kernel", 64)])
def test_no_spill_no_scratch_no_lds(asm, kernel, vgprs):
    res = resources(asm, kernel)
    print("%s: %d VGPRs, %d SGPRs" % (kernel, res["vgpr_count"], res["sgpr_count"]))
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0
    assert res["private_segment_fixed_size"] == 0 and res["group_segment_fixed_size"] == 0
    assert res["vgpr_count"] <= vgprs                           # eight waves per SIMD
