"""The collision prep kernel with its face table in LDS still fits its budgets -- read from the cross-compiled code object, no GPU needed.

`sdf_prep_kernel` keeps the packed face table of the hand's side (1600 words) in the LDS array whose first 1024 words are `cur`.  The
512-thread forms run four workgroups per CU: at most 64 vector registers, and at most 40 960 B of static LDS (a CU has 160 KB).  A
form of this kernel that spills has faulted the launch behind it before (tests/test_build_cpu.py), so no scratch and no spilled
register, vector or scalar.  The 1024-thread form runs two workgroups per CU: no scratch, LDS within half a CU's.

The DMA that fills the table is tracked by the issuing wave's vmcnt only: in the built code every form waits `s_waitcnt vmcnt(0)`
directly in front of the workgroup barrier that precedes the pair loop."""
import shutil

import pytest

import codeobj

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

LDS_PER_CU = 163840
FORMS = {"dense-512": "_Z15sdf_prep_kernelILb1ELi512E", "sparse-512": "_Z15sdf_prep_kernelILb0ELi512E", "sparse-1024": "_Z15sdf_prep_kernelILb0ELi1024E"}


@pytest.mark.parametrize("form", ["dense-512", "sparse-512"])
def test_512_thread_forms_fit_four_workgroups_per_cu(form):
    name, r = codeobj.kernel(FORMS[form])
    print(f"[build] {name[:48]}: {r['vgpr_count']} VGPRs ({r['vgpr_spill_count']} spilled), {r['sgpr_count']} SGPRs ({r['sgpr_spill_count']} spilled), "
          f"{r['private_segment_fixed_size']} B scratch, {r['group_segment_fixed_size']} B LDS")
    assert r["vgpr_count"] <= 64, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["group_segment_fixed_size"] <= 40960 and 4 * r["group_segment_fixed_size"] <= LDS_PER_CU, r


def test_1024_thread_form_fits_two_workgroups_per_cu():
    name, r = codeobj.kernel(FORMS["sparse-1024"])
    print(f"[build] {name[:48]}: {r['vgpr_count']} VGPRs ({r['vgpr_spill_count']} spilled), {r['private_segment_fixed_size']} B scratch, "
          f"{r['group_segment_fixed_size']} B LDS")
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert 2 * r["group_segment_fixed_size"] <= LDS_PER_CU, r


@pytest.mark.parametrize("form", sorted(FORMS))
def test_face_table_dma_is_waited_for_at_the_barrier_before_the_pair_loop(form):
    """The pair loop is the kernel's only LDS XOR (`atomicXor(&parity[col], hits)`); the barrier in front of it is the one that
    publishes the queued pairs."""
    name, _ = codeobj.kernel(FORMS[form])
    body = codeobj.body(name)
    dma = [i for i, l in enumerate(body) if "global_load_lds_dwordx4" in l]
    assert dma, "no LDS-DMA load in the kernel: the face table is not staged"
    xor = [i for i, l in enumerate(body) if "ds_xor_b32" in l]
    assert len(xor) == 1, "the pair loop was expected to be the kernel's only LDS XOR"
    barrier = max(i for i, l in enumerate(body) if "s_barrier" in l and i < xor[0])
    assert barrier > dma[-1]
    assert any("s_waitcnt" in l and "vmcnt(0)" in l for l in body[barrier - 8:barrier]), body[barrier - 8:barrier + 1]
