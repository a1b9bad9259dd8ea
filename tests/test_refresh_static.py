"""The four kernels of the two collective refreshes on the ISA hipcc makes for gfx950 (no GPU).  The finish kernels form a mask (and, for MK-BFV,
a flood) in registers and are the widest of the protocol kernels: four waves per SIMD (at most 128 VGPRs), as DESIGN.md 4.5k and 4.5l state.  The
merge kernels own one coefficient through every modulus out of a digit scratch in memory: eight waves per SIMD (at most 64 VGPRs).  None may spill,
use scratch or touch LDS.  The register counts are printed (DESIGN.md quotes them)."""
import os

import pytest

from isa_static import HIPCC, compile_asm, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("src,kernel,vgprs", [("refresh_kernels.hip", "refresh_finish_kernel", 128), ("refresh_kernels.hip", "refresh_merge_kernel", 64),
                                              ("bfv_refresh_kernels.hip", "bfv_refresh_finish_kernel", 128),
                                              ("bfv_refresh_kernels.hip", "bfv_refresh_merge_kernel", 64)])
def test_no_spill_no_scratch_no_lds(src, kernel, vgprs):
    res = resources(compile_asm(src), kernel)
    print("%s: %d VGPRs, %d SGPRs" % (kernel, res["vgpr_count"], res["sgpr_count"]))
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0
    assert res["private_segment_fixed_size"] == 0 and res["group_segment_fixed_size"] == 0
    assert res["vgpr_count"] <= vgprs                           # 64: eight waves per SIMD; 128: four
