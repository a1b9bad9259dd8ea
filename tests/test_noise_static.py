"""The two kernels of mkhe_noise_norm on the ISA hipcc makes for gfx950 (no GPU): neither spills or uses scratch, each holds the 64 bytes of LDS of
its block maximum and nothing else, neither contains an atomic, and both fit eight waves per SIMD.  The register counts are printed (DESIGN.md
quotes them)."""
import os

import pytest

from isa_static import HIPCC, compile_asm, ops, resources

KERNELS = ["noise_centre_kernel", "noise_reduce_kernel"]


@pytest.fixture(scope="module")
def asm():
    return compile_asm("noise_kernels.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spill_no_scratch_64_bytes_of_lds(asm, kernel):
    res = resources(asm, kernel)
    print("%s: %d VGPRs, %d SGPRs" % (kernel, res["vgpr_count"], res["sgpr_count"]))
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0
    assert res["private_segment_fixed_size"] == 0 and res["group_segment_fixed_size"] == 64
    assert res["vgpr_count"] <= 64                              # eight waves per SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel", KERNELS)
def test_no_atomics_and_the_selection_goes_through_lds(asm, kernel):
    o = ops(asm, kernel)
    assert not [x for x in o if "atomic" in x], [x for x in o if "atomic" in x]
    assert "s_barrier" in o and any(x.startswith("ds_") for x in o)
