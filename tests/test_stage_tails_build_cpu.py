"""Resource budget of the translation stage's tail launch (`opt_tail_kernel_trans`, csrc/refine.h), checked without a GPU like the
generic forms' (tests/test_tail_build_cpu.py: the same assembly listing of the product flags).

The only heavy code of that launch is the collision sampler, which needs 95 vector registers in `opt_sample_loss_kernel`: the kernel
stays a full allocation step under the generic forms' 128 (at most 96), free of scratch and of spilled registers, and with less than
half of their static LDS (no `LbsBwdShared` records, no dynamic LDS)."""
import shutil

import pytest

import codeobj

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

VGPR_BOUND = 96             # the allocation step under 128 that still holds the sampler's 95 (the build reaches 88)
GENERIC_STATIC_LDS = 55840  # the three generic forms (csrc/refine.h)


def test_translation_tail_uses_no_scratch_and_stays_under_96_registers():
    name, m = codeobj.kernel("_Z21opt_tail_kernel_trans")
    print(f"[build] {name}: {m['vgpr_count']} VGPRs, {m['vgpr_spill_count']} spilled, {m['sgpr_spill_count']} SGPRs spilled, "
          f"{m['private_segment_fixed_size']} B scratch, {m['group_segment_fixed_size']} B static LDS")
    assert m["vgpr_spill_count"] == 0, m
    assert m["sgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= VGPR_BOUND, m
    assert m["group_segment_fixed_size"] < GENERIC_STATIC_LDS, m
