"""Build hygiene of the HIP library, checked without a GPU (hipcc cross-compiles gfx950 here).

* every instrumentation / experiment macro threaded through the product kernels still compiles (round 5 review: five macros, nothing
  checked them);
* the collision kernels of the refinement loop do not spill to scratch.  Round 6: `sdf_prep_kernel<false, 512>` at its 64-register budget
  spilled seven registers to scratch after a change, and the refinement then died with a GPU memory fault in the NEXT launch
  (`sdf_dist_kernel`, fed garbage) whenever more than 128 hands were in flight -- only behind the fused tail launch, never in the
  three-launch checker path.  The kernel was brought back under its budget (the candidate-list words are requested where they are
  used); this test keeps it there."""
import os
import re
import shutil
import subprocess

import pytest

import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ihmr_amd", "csrc")
BASE = ["hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

MACROS = ["-DSDF_STAMPS=1", "-DSDF_STAMPS=2", "-DTAIL_STAMPS", "-DCONV_STAMPS", "-DIHMR_TIMELINE", "-DSDF_SPIN=1", "-DSDF_HANDLOG", "-DSDF_QMASK_CHECK",
          "-DIHMR_TUNING_BUILD", "-DCONV_NO_XCD_MAP", "-DCONV_DUMMY_VALU=32", "-DSDF_PREP_MIN_WAVES=4", "-DSDF_REFUSED_BITS=0",
          "-DSDF_STAMPS=1 -DTAIL_STAMPS -DCONV_STAMPS -DIHMR_TIMELINE -DSDF_HANDLOG -DSDF_QMASK_CHECK -DIHMR_TUNING_BUILD"]


@pytest.mark.parametrize("macro", MACROS)
def test_instrumentation_macros_compile(macro):
    """`hipcc -fsyntax-only` (device pass: templates instantiated, no code generation) of the whole library with the macro defined."""
    r = subprocess.run(BASE + ["-fsyntax-only"] + macro.split() + ["ihmr_hip.hip"], cwd=SRC, capture_output=True, text=True, timeout=600)
    errs = [l for l in r.stderr.splitlines() if "error" in l]
    assert r.returncode == 0 and not errs, (macro, r.stderr[-3000:])


def test_loop_collision_kernels_do_not_spill():
    """Device assembly of the product build: the kernels the refinement loop launches at its register budgets -- both forms of
    sdf_prep_kernel (64 registers) and sdf_dist_kernel (128) -- use no scratch at all (`.private_segment_fixed_size` 0, no spilled
    vector register)."""
    seen = {name: (r["vgpr_count"], r["vgpr_spill_count"], r["private_segment_fixed_size"])
            for name, r in codeobj.records().items() if re.match(r"_Z15sdf_(prep|dist)_kernelILb0", name)}
    assert len(seen) >= 3, list(seen)
    # the staging wait of sdf_list_item (SDF_STAGE_CLOSE_KEEP1: `s_waitcnt vmcnt(1)` + barrier) is correct only while the wave's YOUNGEST
    # vector-memory operation at that point is the map-word prefetch -- a plain load issued after the table's LDS-DMA pieces -- and not
    # a DMA piece, a spill reload or a store (advisor, round 5): in the built code the nearest memory instruction before every such
    # wait must be that 8-byte global load
    body = codeobj.body("_Z15sdf_dist_kernelILb0EEv12SdfWorkspace")
    waits = [i for i, l in enumerate(body) if "s_waitcnt vmcnt(1)" in l and any("s_barrier" in x for x in body[i + 1:i + 6])]
    assert waits, "no vmcnt(1) staging wait found in sdf_dist_kernel"
    for i in waits:
        prev = next(l for l in reversed(body[:i]) if re.search(r"\b(global_|scratch_|buffer_|flat_)(load|store|atomic)", l))
        assert "global_load_dwordx2" in prev and "lds" not in prev, prev
    for name, (vgpr, spill, scratch) in seen.items():
        print(f"[build] {name[:60]}: {vgpr} VGPRs, {spill} spilled, {scratch} B scratch")
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        assert vgpr <= (64 if "prep" in name else 128), (name, vgpr)
