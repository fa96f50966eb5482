"""Resource budget of the translation stage's tail launch (`opt_tail_kernel_trans`, csrc/refine.h), checked without a GPU like the
generic forms' (tests/test_tail_build_cpu.py: the same assembly listing of the product flags).

The only heavy code of that launch is the collision sampler, which needs 95 vector registers in `opt_sample_loss_kernel`: the kernel
stays a full allocation step under the generic forms' 128 (at most 96), free of scratch and of spilled registers, and with less than
half of their static LDS (no `LbsBwdShared` records, no dynamic LDS)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ihmr_amd", "csrc")
BASE = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only", "-S"]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

VGPR_BOUND = 96             # the allocation step under 128 that still holds the sampler's 95 (the build reaches 88)
GENERIC_STATIC_LDS = 55840  # the three generic forms (csrc/refine.h)


def test_translation_tail_uses_no_scratch_and_stays_under_96_registers(tmp_path):
    out = tmp_path / "ihmr.s"
    r = subprocess.run(BASE + ["-o", str(out), "ihmr_hip.hip"], cwd=SRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", out.read_text(), flags=re.S)
    assert recs, "no kernel metadata records in the assembly"
    seen = {}
    for body in recs:
        name = re.search(r"\.name:\s+(\S+)", body).group(1)
        if name.startswith("_Z21opt_tail_kernel_trans"):
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", body).group(1))
            seen[name] = {k: get(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                              "group_segment_fixed_size")}
    assert len(seen) == 1, sorted(seen)
    (name, m), = seen.items()
    print(f"[build] {name}: {m['vgpr_count']} VGPRs, {m['vgpr_spill_count']} spilled, {m['sgpr_spill_count']} SGPRs spilled, "
          f"{m['private_segment_fixed_size']} B scratch, {m['group_segment_fixed_size']} B static LDS")
    assert m["vgpr_spill_count"] == 0, m
    assert m["sgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= VGPR_BOUND, m
    assert m["group_segment_fixed_size"] < GENERIC_STATIC_LDS, m
