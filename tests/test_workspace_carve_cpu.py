"""The size queries cover the carves -- checked on the host, without a GPU.

`ihmr_opt_workspace_bytes(B)` / `ihmr_sdf_workspace_bytes(B)` (csrc/refine.h `opt_ws_bytes`, csrc/mano_lbs.h `lbs_ws_bytes`,
csrc/sdf_collision.h `sdf_ws_bytes` / `sdf_list_bytes`) and the carves that cut about forty regions out of a workspace of that size
(`opt_carve`, `lbs_carve`, `sdf_carve`) are separate pieces of arithmetic: eleven regions are rounded up per region, three alignment
pads depend on the ABSOLUTE address of the base, and bare `+ 8192` / `+ 1024` / `+ 256` terms of the size functions pay for both.
tests/workspace_carve_driver.cpp calls the product's own functions on a base pointer that is never dereferenced and prints every region's
offset; here each region's SIZE comes from the element counts of the struct comments (`lbs_regions`, `opt_regions`, `sdf_regions` below -- not from the carve), and

  * regions ascend, and each starts at or after the end of the previous one;
  * the end of the last region lies at or below the size query (for the loop's workspace: below `opt_ws_bytes(B)`, and the collision part
    below `sdf_ws_bytes(2B, true)` from `sdf_ws`; for the stand-alone entry points: below `sdf_ws_bytes(2B)`, with the face copies of
    `faces_to_workspace` behind it inside `ihmr_sdf_workspace_bytes(B)`);
  * float4 / uint2 / unsigned long long regions have their natural alignment, every region the alignment of its element;
  * what the code aligns to 256 is 256-aligned: the `take()` regions relative to the base, the three padded regions of the list part
    absolutely;

at B = 1 .. 16384 (SDF_MAX_HANDS / 2) and at bases 0, 16 and 240 bytes past a 256-aligned address.  All three bases pass: the carves
tolerate every base that is a multiple of 16 -- what the float4 regions need and every device allocator gives -- so a 256-aligned base
is NOT a requirement of these workspaces.

Sensitivity (run on a scratch copy of the headers, never in the tree; `build_driver(include_dir=...)`): with `sdf_list_bytes`'s `+ 1024`
removed the candidate lists end 16 bytes past `sdf_ws_bytes(2B, true)` at base + 240 of B = 1, 2, 8, 33 and 65 (and the restated
`sdf_ws_bytes` disagrees with the product's at every case); with `opt_ws_bytes`'s `+ 8192` removed they end 16 bytes past
`opt_ws_bytes(B)` at B = 1, base + 240.  Both pass at the 256-aligned base: the base offsets are what makes the check bite."""
import os
import shutil
import subprocess
from collections import OrderedDict

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")

# include/ihmr_hip.h, csrc/ihmr_common.h, csrc/mano_lbs.h, csrc/sdf_collision.h
NV, NV3, NFP, NVOX, NCOL, NV4 = 778, 2334, 1600, 32768, 1024, 784
SK_STRIDE, LBS_KG = 784, 25
SDF_LCAP_V, SDF_LCAP_L, SDF_NCTR, SDF_MAX_HANDS = 1024, 192, 64, 32768
LARGEST_HAND_RECORD = SDF_LCAP_V * SDF_LCAP_L * 2      # one hand's candidate lists: the guard width of tests/guarded.py

BATCHES = (1, 2, 3, 8, 9, 33, 64, 65, 512, SDF_MAX_HANDS // 2)
BASE_OFFSETS = (0, 16, 240)


def xcd_cap(H):
    return H * (NVOX + 64)


# region -> (bytes, element alignment), in carve order, from the struct comments (LbsWork, OptWork, SdfWorkspace); H = 2B hands
def lbs_regions(N):
    return OrderedDict([("lbs.skel", (N * SK_STRIDE * 4, 4)), ("lbs.v_posed", (N * NV3 * 4, 4)), ("lbs.dvp", (N * NV3 * 4, 4)),
                        ("lbs.chain", (N * 192 * 4, 4)), ("lbs.dpf_part", (LBS_KG * N * 136 * 4, 4)), ("lbs.pose_off", (N * NV3 * 4, 4))])


def opt_regions(B):
    r = lbs_regions(2 * B)
    r.update([("g_verts", (2 * B * NV * 3 * 4, 4)), ("joints_raw", (B * 42 * 3 * 4, 4)), ("g_joints", (B * 42 * 3 * 4, 4)),
              ("g_trans_direct", (B * 3 * 4, 4)), ("g_orient", (2 * B * 3 * 4, 4)), ("g_pose", (2 * B * 45 * 4, 4)),
              ("g_shape", (2 * B * 10 * 4, 4)), ("g_trans", (B * 3 * 4, 4)), ("g_cam", (B * 3 * 4, 4)), ("kept_left", (B * NV * 3 * 4, 4))])
    return r


def sdf_regions(H, lists):
    r = OrderedDict([("box", (H * 4 * 4, 4)), ("sph", (H * NFP * 16, 16)), ("vn4", (H * NV4 * 16, 16)), ("nrm", (H * NFP * 4, 4)),
                     ("phi", (H * NVOX * 4, 4)), ("inside_bits", (H * NCOL * 4, 4)), ("stats", (16 * 8, 8)), ("inside_count", (SDF_NCTR * 4, 4)),
                     ("inside_list", (xcd_cap(H) * 4, 4)), ("qcell", (H * NV * 4, 4))])
    if lists:
        r.update([("vn_ref", (H * NV3 * 4, 4)), ("hmode", (H * 4, 4)), ("run_start", (H * 4, 4)), ("hdisp", (H * 4, 4)), ("lnext", (H * 4, 4)),
                  ("lbits", (H * NCOL * 4, 4)), ("rbits", (H * NCOL * 4, 4)), ("known", (H * NCOL * 4, 4)), ("inside_k", (H * NCOL * 4, 4)),
                  ("inside_list_a", (xcd_cap(H) * 4, 4)), ("lmap", (H * NVOX * 8, 8)), ("lists", (H * SDF_LCAP_V * SDF_LCAP_L * 2, 2))])
    return r


ALIGNED_256_ABSOLUTE = ("vn_ref", "lbits", "lists")        # sdf_carve pads the ADDRESS before these


def _up256(n):
    return (n + 255) & ~255


def sdf_ws_bytes(H, lists=False):
    """csrc/sdf_collision.h: sdf_ws_bytes / sdf_list_bytes, restated (compared with the product's own at every case below)."""
    n = 0
    if lists:
        n += H * (NV3 * 4 + 16 + 4 * NCOL * 4 + NVOX * 8 + SDF_LCAP_V * SDF_LCAP_L * 2) + xcd_cap(H) * 4 + 1024
    n += H * 16 + H * NFP * 16 + H * NFP * 4 + H * NV4 * 16 + H * NVOX * 4 + H * NCOL * 4 + xcd_cap(H) * 4
    n += 128 + SDF_NCTR * 4 + 256
    n += _up256(H * NV * 4)
    return _up256(n)


FACE_COPIES_BYTES = 2 * NFP * 4 * 4           # csrc/ihmr_hip.hip faces_to_workspace: per hand 3 SoA rows + 1 packed row of NFP words


def sdf_public_workspace_bytes(B):
    """csrc/ihmr_hip.hip: ihmr_sdf_workspace_bytes(B) = sdf_ws_bytes(2B) + 2 * NFP * 4 * 4 + 256, restated (tests/test_gpu_guarded_refinement.py
    compares it with the library's answer)."""
    return sdf_ws_bytes(2 * B) + FACE_COPIES_BYTES + 256


def build_driver(out_dir, include_dir=None):
    """The driver, host side only: hipcc with the include path of the product headers (`include_dir`: a scratch copy of csrc/)."""
    exe = os.path.join(str(out_dir), "workspace_carve_driver")
    empty = os.path.join(str(out_dir), "no_device_code.bin")
    open(empty, "wb").close()                  # the host pass embeds this in place of the device code object nobody launches
    csrc = include_dir or os.path.join(ROOT, "ihmr_amd", "csrc")
    cmd = ["hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", f"-I{csrc}", "--cuda-host-only",
           "-Xclang", "-fcuda-include-gpubinary", "-Xclang", empty, os.path.join(ROOT, "tests", "workspace_carve_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def carve(exe, B, base_offset):
    """sizes (name -> bytes) and tables (carve -> OrderedDict region -> offset from the base) as the driver prints them."""
    r = subprocess.run([exe, str(B), str(base_offset)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes, tables = {}, {"opt": OrderedDict(), "sdf": OrderedDict()}
    for line in r.stdout.splitlines():
        a, b, c = line.split()
        if a == "size":
            sizes[b] = int(c)
        else:
            assert b not in tables[a], line
            tables[a][b] = int(c)
    return sizes, tables


def check_case(sizes, tables, B, base_offset):
    """Every assertion of this module on one (B, base offset); returns the loop workspace's rows (region, offset, bytes) for the summary."""
    H = 2 * B
    what = f"B = {B}, base + {base_offset}"
    assert sizes["sdf_ws_bytes"] == sdf_ws_bytes(H) and sizes["sdf_ws_bytes_lists"] == sdf_ws_bytes(H, True), what
    assert sizes["sdf_xcd_cap"] == sizes["opt.xcd_cap"] == sizes["sdf.xcd_cap"] == xcd_cap(H), what

    def walk(offsets, regions, start, label):
        assert list(offsets) == list(regions), (what, label, list(offsets))
        end, rows = start, []
        for name, (nbytes, align) in regions.items():
            off = offsets[name]
            assert off >= end, f"{what}: {label} {name} at {off} starts before the end of the previous region ({end})"
            assert (base_offset + off) % align == 0, f"{what}: {label} {name} at base + {off} is not {align}-byte aligned"
            rows.append((name, off, nbytes))
            end = off + nbytes
        return end, rows

    # ---- the loop's workspace: LbsWork + OptWork, then the collision workspace with its lists behind sdf_ws
    opt = tables["opt"]
    sdf_ws = opt["sdf_ws"]
    head = OrderedDict((k, opt[k]) for k in opt_regions(B))
    end, rows = walk(head, opt_regions(B), 0, "opt_carve")
    assert sdf_ws >= end, what
    for name in list(head) + ["sdf_ws"]:
        assert opt[name] % 256 == 0, f"{what}: opt_carve {name} is not a multiple of 256 from the base"
    first_opt = opt["g_verts"]
    assert opt["lbs.pose_off"] + opt_regions(B)["lbs.pose_off"][0] <= first_opt <= sizes["lbs_ws_bytes"], f"{what}: lbs_carve ends past lbs_ws_bytes"
    tail = OrderedDict((k, opt[k]) for k in sdf_regions(H, True))
    end, more = walk(tail, sdf_regions(H, True), sdf_ws, "sdf_carve(lists)")
    rows += [("sdf_ws", sdf_ws, 0)] + more
    for name in ALIGNED_256_ABSOLUTE:
        assert (base_offset + opt[name]) % 256 == 0, f"{what}: {name} is not 256-aligned"
    assert end - sdf_ws <= sizes["sdf_ws_bytes_lists"], f"{what}: lists end {end - sdf_ws - sizes['sdf_ws_bytes_lists']} bytes past sdf_ws_bytes(2B, true)"
    assert end <= sizes["opt_ws_bytes"], f"{what}: lists end {end - sizes['opt_ws_bytes']} bytes past opt_ws_bytes(B)"

    # ---- the stand-alone collision entry points: sdf_carve(base, 2B), the face copies behind sdf_ws_bytes(2B)
    end_sdf, _ = walk(tables["sdf"], sdf_regions(H, False), 0, "sdf_carve")
    assert end_sdf <= sizes["sdf_ws_bytes"], f"{what}: qcell ends past sdf_ws_bytes(2B)"
    assert (base_offset + sizes["sdf_ws_bytes"]) % 4 == 0
    assert sizes["sdf_ws_bytes"] + FACE_COPIES_BYTES <= sdf_public_workspace_bytes(B), what
    return rows, dict(opt=sizes["opt_ws_bytes"] - end, sdf_lists=sizes["sdf_ws_bytes_lists"] - (end - sdf_ws), sdf=sizes["sdf_ws_bytes"] - end_sdf)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("carve"))


@pytest.mark.parametrize("base_offset", BASE_OFFSETS)
@pytest.mark.parametrize("B", BATCHES)
def test_size_queries_cover_the_carves(driver, B, base_offset):
    sizes, tables = carve(driver, B, base_offset)
    rows, slack = check_case(sizes, tables, B, base_offset)
    if B == 3:
        print(f"[carve] B = 3, base + {base_offset}: opt_ws_bytes {sizes['opt_ws_bytes']}, slack under opt_ws_bytes {slack['opt']}, under "
              f"sdf_ws_bytes(2B, true) {slack['sdf_lists']}, under sdf_ws_bytes(2B) {slack['sdf']}")
        for name, off, nbytes in rows:
            print(f"[carve]   {name:16s} {off:9d} {nbytes:9d}")


def test_the_largest_region_of_one_hand_is_its_candidate_lists():
    """tests/guarded.py sizes the workspace guards by it: an overrun by one hand's record of ANY region lands inside a guard."""
    per_hand = [n for n, _ in sdf_regions(1, True).values()] + [n for n, _ in lbs_regions(1).values()]
    assert max(per_hand) == LARGEST_HAND_RECORD == 393216
    from guarded import WORKSPACE_GUARD
    assert WORKSPACE_GUARD >= LARGEST_HAND_RECORD


def test_guard_check_reports_a_flipped_byte_on_host_memory():
    """tests/guarded.py on host tensors (no GPU): intact after construction and after writing the whole payload; one flipped guard byte
    on either side is reported at its payload-relative offset."""
    import torch
    from guarded import GUARD_BYTE, Guarded
    g = Guarded(1000, guard=512, fill=0x00, device="cpu")
    assert g.data_ptr % 256 == 0 and g.payload_bytes().numel() == 1000 and int(g.payload_bytes().max()) == 0
    g.view(torch.float32, (10, 25)).fill_(float("nan"))
    assert g.guards_intact() is None
    for off in (1000, 1000 + 511, -1, 1003):
        g.raw[g.lo + off] ^= 0x01
        assert g.guards_intact() == off, off
        g.raw[g.lo + off] = GUARD_BYTE
        assert g.guards_intact() is None


def test_the_driver_refuses_what_the_entry_points_refuse(driver):
    for bad in (0, SDF_MAX_HANDS // 2 + 1):
        assert subprocess.run([driver, str(bad), "0"], capture_output=True).returncode == 2
