"""``ihmr_mano_update_shapedirs`` and the refusals of ``ihmr_mano_create`` through the C ABI.  The tables themselves are checked on the
host (tests/test_mano_tables_cpu.py); here: a layer created with one ``shapedirs`` and updated to a second is, bit for bit, the layer
created with the second -- one-hand forward and backward, and the two-hand forward -- and an asset the table builder refuses leaves
the handle null."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3


def _second_shapedirs(asset):
    rng = np.random.default_rng(23)
    return (asset["shapedirs"] + 1e-3 * rng.standard_normal(asset["shapedirs"].shape)).astype(np.float32)


@pytest.fixture(scope="module")
def handles(mano_arrays):
    """A: created with the first shapedirs, updated to the second; B: created with the second; first: still holds the first."""
    from ihmr_amd import hip
    assert torch.cuda.is_available()
    right, _ = mano_arrays
    sd2 = _second_shapedirs(right)
    h = {"A": hip.ManoHandle(right), "B": hip.ManoHandle(dict(right, shapedirs=sd2)), "first": hip.ManoHandle(right)}
    h["A"].update_shapedirs(sd2)
    return h


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _lbs(handle, seed=31):
    """ihmr_mano_lbs_fwd + ihmr_mano_lbs_bwd (need_mask 7) of N seeded hands with non-zero betas: verts, joints, the three gradients."""
    from ihmr_amd import hip
    L, g = hip.lib(), torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    orient, pose, betas, gv, gj = r(N, 3, scale=0.8), r(N, 45, scale=0.3), r(N, 10, scale=0.8), r(N, 778, 3), r(N, 16, 3)
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = dict(verts=z(N, 778, 3), joints=z(N, 16, 3), d_orient=z(N, 3), d_pose=z(N, 45), d_betas=z(N, 10))
    ws = torch.empty(L.ihmr_mano_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    hip.check(L.ihmr_mano_lbs_fwd(handle.handle, hip.ptr(orient), hip.ptr(pose), hip.ptr(betas), N, hip.ptr(out["verts"]), hip.ptr(out["joints"]),
                                  hip.ptr(ws), hip.stream_ptr()), "ihmr_mano_lbs_fwd")
    hip.check(L.ihmr_mano_lbs_bwd(handle.handle, N, hip.ptr(ws), hip.ptr(gv), hip.ptr(gj), hip.ptr(out["d_orient"]), hip.ptr(out["d_pose"]),
                                  hip.ptr(out["d_betas"]), 7, hip.stream_ptr()), "ihmr_mano_lbs_bwd")
    torch.cuda.synchronize()
    return {k: _bits(v) for k, v in out.items()}


def test_updated_layer_is_the_layer_created_with_the_second_shapedirs(handles):
    a, b, first = (_lbs(handles[k]) for k in ("A", "B", "first"))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the update took effect: the shape basis moves the mesh, the regressed joints and the shape gradient
    for k in ("verts", "joints", "d_betas"):
        assert not np.array_equal(a[k], first[k]), k


def _two_hand_verts(handle, B=2, seed=37):
    """ihmr_opt_forward_verts at B samples on buffers laid out as OptimizeModel allocates them: verts (2, B, 778, 3)."""
    from ihmr_amd import hip
    L, g = hip.lib(), torch.Generator().manual_seed(seed)
    z = lambda *s: torch.zeros(*s, device="cuda")
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    buf = dict(cam=z(B, 3), trans=r(B, 3, scale=0.05), orient=r(2, B, 3, scale=0.8), pose=r(2, B, 45, scale=0.3), shape=r(2, B, 10, scale=0.8),
               init_joints_2d=z(B, 42, 3), init_joints_3d=z(B, 42, 4), init_hand_trans_j=z(B, 4),
               gt_joints_2d=z(B, 42, 3), gt_joints_3d=z(B, 42, 4), gt_hand_trans=z(B, 4), hand_type_array=z(B, 2),
               verts=z(2, B, 778, 3), joints_3d=z(B, 42, 3), joints_2d=z(B, 42, 2), loss_batch=z(8, B),
               coll_per_vert=z(B, 1556), coll_origin_scale=z(B, 1556), snap_params=z(1, B, hip.OPT_NPARAM), snap_loss=z(1, 3, B),
               selected=torch.zeros(B, device="cuda", dtype=torch.int32), adam_m=z(B, hip.OPT_NPARAM), adam_v=z(B, hip.OPT_NPARAM),
               workspace=torch.zeros(L.ihmr_opt_workspace_bytes(B), device="cuda", dtype=torch.uint8))
    io = hip.OptIO(**{k: v.data_ptr() for k, v in buf.items()}, norm_batch=B)
    hip.check(L.ihmr_opt_forward_verts(handle.handle, C.byref(io), B, hip.stream_ptr()), "ihmr_opt_forward_verts")
    torch.cuda.synchronize()
    return _bits(buf["verts"])


def test_updated_layer_on_the_two_hand_path(handles):
    a, b, first = (_two_hand_verts(handles[k]) for k in ("A", "B", "first"))
    assert a.any() and np.array_equal(a, b) and not np.array_equal(a, first)


@pytest.mark.parametrize("what", ["parents", "faces"])
def test_create_refuses_and_leaves_the_handle_null(mano_arrays, what):
    """parents[5] = 5 (a joint that is its own parent) and a face id of 778: ihmr_mano_create returns non-zero before anything is
    uploaded or launched, and the caller's handle stays null."""
    from ihmr_amd import hip
    right, _ = mano_arrays
    a = dict(right)
    if what == "parents":
        a["parents"] = np.array(right["parents"], np.int32)
        a["parents"][5] = 5
    else:
        a["faces"] = np.array(right["faces"], np.int32)
        a["faces"][700, 1] = 778
    keep = {k: np.ascontiguousarray(a[k], np.int32 if k in ("parents", "faces") else np.float32) for k, _ in hip.ManoArrays._fields_ if k != "tip_ids"}
    keep["tip_ids"] = np.asarray((744, 320, 443, 554, 671), np.int32)
    arrays, handle = hip.ManoArrays(**{k: v.ctypes.data for k, v in keep.items()}), C.c_void_p()
    assert hip.lib().ihmr_mano_create(C.byref(arrays), C.byref(handle)) != 0 and not handle.value
    with pytest.raises(RuntimeError, match="ihmr_mano_create"):
        hip.ManoHandle(a)
