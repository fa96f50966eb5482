"""Resource budget of the LDS form of the pose-gradient GEMM (`lbs_bwd2_lds_kernel`, csrc/mano_lbs.h), checked without a GPU (hipcc
cross-compiles gfx950 here).

The kernel's schedule rests on whole SIMDs: a workgroup is a multiple of four waves (one per SIMD of a CU), and three workgroups are
resident per CU, so that all 600 - 700 workgroups of a launch of the refinement loop are resident at once and no SIMD carries more than
three units.  That holds while the static LDS of a workgroup is at most a third of a CU's 160 KB and nothing goes to scratch (a spilled
register is a memory round trip between two MFMAs).  The test reads the AMDGPU metadata record of the product build only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ihmr_amd", "csrc")
# the product flags (ihmr_amd/hip.py: HIPCC_FLAGS) as a device-only assembly listing
BASE = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only", "-S"]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

RESIDENT_PER_CU = 3                 # the kernel's comment: three workgroups per CU
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512                # one wave of each resident workgroup per SIMD


def test_pose_gradient_kernel_uses_no_scratch_and_fits_three_per_cu(tmp_path):
    out = tmp_path / "ihmr.s"
    r = subprocess.run(BASE + ["-o", str(out), "ihmr_hip.hip"], cwd=SRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    text = out.read_text()
    # one YAML record per kernel, keys sorted: a record is cut at its first and last key
    recs = re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, flags=re.S)
    assert recs, "no kernel metadata records in the assembly"
    seen = {}
    for body in recs:
        name = re.search(r"\.name:\s+(\S+)", body).group(1)
        if not name.startswith("_Z19lbs_bwd2_lds_kernel"):
            continue
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", body).group(1))
        seen[name] = {k: get(k) for k in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                          "group_segment_fixed_size", "max_flat_workgroup_size")}
    assert len(seen) == 1, sorted(seen)
    (name, m), = seen.items()
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
