"""Resource budget of the LDS form of the pose-gradient GEMM (`lbs_bwd2_lds_kernel`, csrc/mano_lbs.h), checked without a GPU (hipcc
cross-compiles gfx950 here).

The kernel's schedule rests on whole SIMDs: a workgroup is a multiple of four waves (one per SIMD of a CU), and three workgroups are
resident per CU, so that all 600 - 700 workgroups of a launch of the refinement loop are resident at once and no SIMD carries more than
three units.  That holds while the static LDS of a workgroup is at most a third of a CU's 160 KB and nothing goes to scratch (a spilled
register is a memory round trip between two MFMAs).  The test reads the AMDGPU metadata record of the product build only."""
import shutil

import pytest

import codeobj

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

RESIDENT_PER_CU = 3                 # the kernel's comment: three workgroups per CU
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512                # one wave of each resident workgroup per SIMD


def test_pose_gradient_kernel_uses_no_scratch_and_fits_three_per_cu():
    name, m = codeobj.kernel("_Z19lbs_bwd2_lds_kernel")
    print(f"[build] {name}: {m['vgpr_count']} VGPRs ({m['agpr_count']} of them accumulation registers), {m['vgpr_spill_count']} spilled, "
          f"{m['sgpr_spill_count']} SGPRs spilled, {m['private_segment_fixed_size']} B scratch, {m['group_segment_fixed_size']} B LDS, "
          f"{m['max_flat_workgroup_size']} threads")
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0, m
    assert m["sgpr_spill_count"] == 0, m
    assert m["max_flat_workgroup_size"] % 256 == 0, m
    assert RESIDENT_PER_CU * m["group_segment_fixed_size"] <= LDS_PER_CU, m
    # one wave per SIMD and workgroup: the waves of three workgroups share a SIMD's register file
    assert RESIDENT_PER_CU * (m["max_flat_workgroup_size"] // 256) * m["vgpr_count"] <= VGPRS_PER_SIMD, m
