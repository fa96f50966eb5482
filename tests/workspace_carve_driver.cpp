// Host driver of tests/test_workspace_carve_cpu.py: the workspace carves of the refinement loop and of the collision entry points
// (csrc/mano_lbs.h lbs_carve, csrc/refine.h opt_carve, csrc/sdf_collision.h sdf_carve) and their size queries, evaluated by the very
// functions the library calls, on a base pointer that is never dereferenced.  Compiled for the host only; calls no HIP runtime function.
//
//   workspace_carve_driver B base_offset
//
// prints `size <name> <bytes>` lines and `<carve> <region> <offset from the carve's base>` lines, regions in carve order:
//   opt   opt_carve(base, B) with its LbsWork and, behind `sdf_ws`, sdf_carve(w.sdf_ws, 2B, true) -- offsets from `base`
//   sdf   sdf_carve(base, 2B, false), the carve of the stand-alone collision entry points -- offsets from `base`
// where base = a 256-aligned address + base_offset.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ihmr_common.h"
#include "mano_lbs.h"
#include "sdf_collision.h"
#include "mlp_infer.h"
#include "refine.h"

static const char* g_base;
static void region(const char* carve, const char* name, const void* p) {
    printf("%s %s %lld\n", carve, name, (long long)((const char*)p - g_base));
}

static void sdf_regions(const char* carve, const SdfWorkspace& s, bool lists) {
    region(carve, "box", s.box);
    region(carve, "sph", s.sph);
    region(carve, "vn4", s.vn4);
    region(carve, "nrm", s.nrm);
    region(carve, "phi", s.phi);
    region(carve, "inside_bits", s.inside_bits);
    region(carve, "stats", s.stats);
    region(carve, "inside_count", s.inside_count);
    region(carve, "inside_list", s.inside_list);
    region(carve, "qcell", s.qcell);
    printf("size %s.xcd_cap %d\n", carve, s.xcd_cap);
    if (!lists) return;
    region(carve, "vn_ref", s.vn_ref);
    region(carve, "hmode", s.hmode);
    region(carve, "run_start", s.run_start);
    region(carve, "hdisp", s.hdisp);
    region(carve, "lnext", s.lnext);
    region(carve, "lbits", s.lbits);
    region(carve, "rbits", s.rbits);
    region(carve, "known", s.known);
    region(carve, "inside_k", s.inside_k);
    region(carve, "inside_list_a", s.inside_list_a);
    region(carve, "lmap", s.lmap);
    region(carve, "lists", s.lists);
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s B base_offset\n", argv[0]); return 2; }
    const int B = atoi(argv[1]);
    const long off = atol(argv[2]);
    if (B <= 0 || 2 * B > SDF_MAX_HANDS || off < 0 || off >= 256) { fprintf(stderr, "B or base_offset out of range\n"); return 2; }
    g_base = (const char*)(uintptr_t)((1ull << 40) + (unsigned long long)off);   // 256-aligned + off; an address only
    printf("size opt_ws_bytes %zu\n", opt_ws_bytes(B));
    printf("size lbs_ws_bytes %zu\n", lbs_ws_bytes(2 * B));
    printf("size sdf_ws_bytes_lists %zu\n", sdf_ws_bytes(2 * B, true));
    printf("size sdf_ws_bytes %zu\n", sdf_ws_bytes(2 * B, false));
    printf("size sdf_list_bytes %zu\n", sdf_list_bytes(2 * B));
    printf("size sdf_xcd_cap %zu\n", sdf_xcd_cap(2 * B));

    const OptWork w = opt_carve((void*)g_base, B);
    region("opt", "lbs.skel", w.lbs.skel);
    region("opt", "lbs.v_posed", w.lbs.v_posed);
    region("opt", "lbs.dvp", w.lbs.dvp);
    region("opt", "lbs.chain", w.lbs.chain);
    region("opt", "lbs.dpf_part", w.lbs.dpf_part);
    region("opt", "lbs.pose_off", w.lbs.pose_off);
    region("opt", "g_verts", w.g_verts);
    region("opt", "joints_raw", w.joints_raw);
    region("opt", "g_joints", w.g_joints);
    region("opt", "g_trans_direct", w.g_trans_direct);
    region("opt", "g_orient", w.g_orient);
    region("opt", "g_pose", w.g_pose);
    region("opt", "g_shape", w.g_shape);
    region("opt", "g_trans", w.g_trans);
    region("opt", "g_cam", w.g_cam);
    region("opt", "kept_left", w.kept_left);
    region("opt", "sdf_ws", w.sdf_ws);
    sdf_regions("opt", sdf_carve(w.sdf_ws, 2 * B, true), true);

    sdf_regions("sdf", sdf_carve((void*)g_base, 2 * B, false), false);
    return 0;
}
