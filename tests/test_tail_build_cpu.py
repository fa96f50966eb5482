"""Resource budget of the fused tail launch (`opt_tail_kernel`, csrc/refine.h), checked without a GPU (hipcc cross-compiles gfx950 here).

The tail closes every iteration of the refinement loop: one workgroup of 512 threads per sample, two workgroups per CU.  Its cost is
the length of the dependent chain inside a workgroup, so a register spilled to scratch is a memory round trip on that chain -- and a
spilling `sdf_prep_kernel` once made the launch behind it fault (tests/test_build_cpu.py).  All three instantiations stay free of
scratch, inside the 128 vector registers that two workgroups per CU leave a thread, and inside the 80 KB of LDS that two workgroups
share at MANO's 248 weight segments.  The test reads the AMDGPU metadata records of the product build only."""
import shutil

import pytest

import codeobj

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

NSEG = 248                  # single-joint segments of MANO's skinning weights (four bones per vertex)
LDS_TWO_PER_CU = 81920      # half of a CU's 160 KB


def opt_tail_dynamic_lds(nseg):
    """csrc/refine.h: [2][nseg][12] floats of the LBS backward's per-segment partial sums."""
    return 2 * nseg * 12 * 4


def test_tail_kernel_forms_use_no_scratch_and_fit_two_per_cu():
    seen = codeobj.matching("_Z15opt_tail_kernelILb")
    assert len(seen) == 3, sorted(seen)
    for name, m in sorted(seen.items()):
        lds = m["group_segment_fixed_size"] + opt_tail_dynamic_lds(NSEG)
        print(f"[build] {name[:40]}: {m['vgpr_count']} VGPRs, {m['vgpr_spill_count']} spilled, {m['sgpr_spill_count']} SGPRs spilled, "
              f"{m['private_segment_fixed_size']} B scratch, {lds} B LDS at nseg = {NSEG}")
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["sgpr_spill_count"] == 0, (name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
        assert lds <= LDS_TWO_PER_CU, (name, m, lds)
