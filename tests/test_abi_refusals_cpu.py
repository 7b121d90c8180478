"""CPU (no GPU): calls that libenslam_hip.so refuses -- or takes as a no-op -- BEFORE any HIP call, and the exact code each
returns (include/enslam_hip.h: 0, ENSLAM_EINVAL -1, ENSLAM_EUNSUPPORTED -3).  The codes were read off csrc/capi.hip; the table
pins what the members of an entry-point family share and the few places where they differ, including which code a call with
two faults returns (the order of the checks).

No row reaches a kernel launch: a row is refused by the argument checks, or its job is empty (zero rays, nothing to convert,
nothing to unpack), which the launchers return from before they touch the device.  Pointers the host code only passes on are
addresses of a small host buffer; the library never reads through them.

Rules a family does not have are absent from its rows: the samplers take any n_lin + n_surf the launcher accepts and an empty
marking scene (only NULL switches marking off), the compositing backward takes every sample count from 1 to 64 without a work
list, and enslam_step_finish takes no rays at all."""
import ctypes

import pytest

OK, EINVAL, EUNSUPPORTED = 0, -1, -3

_HOST = ctypes.create_string_buffer(256)
P = ctypes.addressof(_HOST)                      # a non-NULL pointer the host code never dereferences
BOUND = (ctypes.c_double * 6)(0.0, 1.0, 0.0, 1.0, 0.0, 1.0)


def _arr(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _scene(L, dims=(2, 2, 2), big=False):
    """A scene whose four grids and decoders are all present (dims None: the zero-initialised, empty scene)."""
    sc = L.Scene()
    if dims is None:
        return sc
    for i in range(6):
        sc.bound[i] = sc.coarse_bound[i] = float(i % 2)
    for k in range(4):
        sc.grids[k].data, sc.packed[k] = P, P
        sc.grids[k].D, sc.grids[k].H, sc.grids[k].W = dims
    if big:                                      # 2^29 voxels: one more than a saved cell record can index
        sc.grids[1].D, sc.grids[1].H, sc.grids[1].W = 1024, 1024, 512
    return sc


def _resolve(L, lib, v):
    """Table values that need the binding: scenes, parameter structs, the tracker's ray limit."""
    if v == "scene":
        return ctypes.byref(_scene(L))
    if v == "scene_empty":
        return ctypes.byref(_scene(L, None))
    if v == "scene_big":
        return ctypes.byref(_scene(L, big=True))
    if v == "params_null":
        return ctypes.pointer(L.MlpParams())     # every tensor pointer NULL
    if v == "tail_max+1":
        return lib.enslam_tracker_tail_max_rays() + 1
    return v


# ---- base calls: name -> ordered (argument, value) pairs of a call that passes every check up to the launch ------------------
_CONV = [("n_conv", 0), ("src", None), ("dst", None), ("n_voxels", None), ("need", None)]
_DEC = [("n_dec", 0), ("kinds", None), ("packed_grads", None)]
_RAYS = [("stage", 3), ("n_rays", 4), ("n_samples", 48), ("rays_o", P), ("rays_d", P), ("z_vals", P), ("scene", "scene"),
         ("dgrid_ws", P), ("g_rays_o", P), ("g_rays_d", P), ("work_list", None), ("work_count", None)]
_FWD = [("stage", 3), ("n_rays", 4), ("n_samples", 48), ("rays_o", P), ("rays_d", P), ("z_vals", P), ("scene", "scene"),
        ("depth", P), ("var", P), ("rgb", P), ("raw_out", P), ("act_ws", None), ("act_light", 0)]
_LIST = [("d_raw_unit", None), ("work_list", None), ("work_count", None)]
_SAMPLE = [("n_rays", 4), ("n_lin", 32), ("n_surf", 16), ("rays_o", P), ("rays_d", P), ("gt_depth", P), ("bound_host", BOUND),
           ("t_lin", P), ("t_surf", P), ("lindisp", 0), ("t_rand", None), ("scratch", P), ("depth_max_given", 0), ("z_vals", P),
           ("mark_stage", 3), ("mark_scene", None), ("mark_flags", None)]
_MARK_G = [("mark_block_voxels", 64), ("mark_flags64", None)]
_COMP = [("n_rays", 4), ("n_samples", 48), ("raw", P), ("z_vals", P), ("depth", P)]
_GRADS = [("g_depth", P), ("g_var", None), ("g_rgb", None)]
_ST = [("stream", None)]

BASE = {
    "enslam_step_finish": _CONV + _DEC + [("grads", None)] + _ST,
    "enslam_step_finish_rays": _CONV + _DEC + [("grads", None)] + _RAYS + _ST,
    "enslam_step_finish_rays_prev": _CONV + [("prev", None)] + _DEC + [("grads", None)] + _RAYS + _ST,
    "enslam_step_finish_partials": _CONV + [("prev", None)] + _DEC + [("grad_partials", None), ("grads", None)] + _RAYS + _ST,
    "enslam_step_finish_native": _CONV + [("prev", None)] + _DEC + [("grad_partials", None), ("grads", None)] + _RAYS +
    [("move_need", None), ("move_prev", None), ("n_move", 0)] + _ST,
    "enslam_render_fwd": _FWD + _ST,
    "enslam_render_loss_fwd": _FWD + [("gt_depth", P), ("gt_color", None), ("w_color", 0.2), ("loss", P)] + _LIST + _ST,
    "enslam_render_tracker_loss_fwd": _FWD + [("gt_depth", P), ("gt_color", None), ("w_color", 0.2), ("inside", None),
                                              ("handle_dynamic", 0), ("tmp_scratch", P), ("loss", P)] + _LIST + _ST,
    "enslam_sample_rays": _SAMPLE + _ST,
    "enslam_sample_rays_g": _SAMPLE + _MARK_G + _ST,
    "enslam_sample_prepare": _SAMPLE + _MARK_G + [("n_dec", 0), ("kinds", None), ("params", None), ("packed", None), ("n_zero", 0),
                                                  ("zero_dst", None), ("zero_voxels", None), ("zero_need", None), ("flat", None),
                                                  ("n_flat", 0)] + _ST,
    "enslam_composite_bwd": _COMP + _GRADS + [("d_raw", P)] + _ST,
    "enslam_composite_bwd_list": _COMP + _GRADS + [("d_raw", P), ("work_list", None), ("work_count", None)] + _ST,
    "enslam_composite_loss_bwd": _COMP + [("rgb", None), ("gt_depth", P), ("gt_color", None), ("w_color", 0.2), ("g_loss", P),
                                          ("d_raw", P), ("work_list", None), ("work_count", None)] + _ST,
    "enslam_pack_mlp_multi": [("n", 1), ("kinds", _i32(1)), ("params", "params_null"), ("packed", _arr(P))] + _ST,
    "enslam_unpack_mlp_grads_multi": [("n", 1), ("kinds", _i32(1)), ("packed_grads", _arr(P)), ("grads", "params_null")] + _ST,
    "enslam_step_prepare": [("n_dec", 0), ("kinds", None), ("params", None), ("packed", None)] + _CONV +
    [("valid", None), ("n_zero", 0), ("zero_dst", None), ("zero_voxels", None), ("zero_need", None), ("flat", None), ("n_flat", 0)] + _ST,
}

FINISH_RAYS = ("enslam_step_finish_rays", "enslam_step_finish_rays_prev", "enslam_step_finish_partials", "enslam_step_finish_native")
FINISH_PREV = FINISH_RAYS[1:]
FWD_ALL = ("enslam_render_fwd", "enslam_render_loss_fwd", "enslam_render_tracker_loss_fwd")
FWD_LOSS = FWD_ALL[1:]
SAMPLERS = ("enslam_sample_rays", "enslam_sample_rays_g", "enslam_sample_prepare")
SAMPLERS_G = SAMPLERS[1:]
COMP_ALL = ("enslam_composite_bwd", "enslam_composite_bwd_list", "enslam_composite_loss_bwd")
COMP_LIST = COMP_ALL[1:]

ROWS = []                                        # (entry, overrides, expected code, label)


def rows(entries, expected, label, **over):
    for e in ((entries,) if isinstance(entries, str) else entries):
        ROWS.append((e, over, expected, label))


def finish_rows(expected, label, **over):
    """A row about the roles all five finish members share: the four that take rays get none (no ray role)."""
    rows("enslam_step_finish", expected, label, **over)
    rows(FINISH_RAYS, expected, label, n_rays=0, **over)


# ---- the finish launch ----------------------------------------------------------------------------------------------
rows(FINISH_RAYS, EINVAL, "negative ray count", n_rays=-1)
for s in (40, 80):
    rows(FINISH_RAYS, EUNSUPPORTED, f"{s} samples", n_samples=s)
rows(FINISH_RAYS, EINVAL, "empty scene", scene="scene_empty")
rows(FINISH_RAYS, EINVAL, "NULL scene", scene=None)
rows(FINISH_RAYS, EINVAL, "unknown stage", stage=4)
for a in ("rays_o", "rays_d", "z_vals", "g_rays_o", "g_rays_d"):
    rows(FINISH_RAYS, EINVAL, f"{a} NULL", **{a: None})
rows(FINISH_RAYS, EINVAL, "work list without count", work_list=P)
rows(FINISH_RAYS, EINVAL, "count without work list", work_count=P)
rows(FINISH_RAYS, OK, "zero rays: plain finish, nothing to do", n_rays=0, rays_o=None, rays_d=None, z_vals=None, scene=None,
     dgrid_ws=None, g_rays_o=None, g_rays_d=None)
rows(FINISH_RAYS, OK, "coarse stage: plain finish, nothing to do", stage=0, scene=None)
rows("enslam_step_finish", OK, "nothing to do")
# the NULL hand-off: an error for the two narrow members, "no ray role" for the two wide ones
rows(FINISH_RAYS[:2], EINVAL, "NULL dgrid_ws with rays at the colour stage", dgrid_ws=None)
rows(FINISH_RAYS[2:], OK, "NULL dgrid_ws: no ray role, nothing to do", dgrid_ws=None)
rows(FINISH_RAYS[:2], EUNSUPPORTED, "NULL dgrid_ws and 40 samples: the sample count is looked at first", dgrid_ws=None, n_samples=40)
rows(FINISH_RAYS[2:], OK, "NULL dgrid_ws and 40 samples: no ray role, nothing looked at", dgrid_ws=None, n_samples=40, scene=None)
# prev
rows(FINISH_PREV, EINVAL, "prev with NULL need", n_conv=1, prev=_arr(P), src=_arr(P), dst=_arr(P), n_voxels=_i64(64))
rows(FINISH_PREV, EINVAL, "prev with need[0] NULL", n_conv=1, prev=_arr(P), need=_arr(None), src=_arr(P), dst=_arr(P),
     n_voxels=_i64(64))
rows(FINISH_PREV, EINVAL, "prev[0] NULL", n_conv=1, prev=_arr(None), need=_arr(P), src=_arr(P), dst=_arr(P), n_voxels=_i64(64))
rows(FINISH_PREV, EINVAL, "prev with n_conv out of range", n_conv=5, prev=_arr(P), need=_arr(P))
rows(FINISH_PREV, EINVAL, "prev fault and 40 samples: prev is looked at first", n_conv=1, prev=_arr(P), n_samples=40)
rows(FINISH_PREV, EINVAL, "prev fault and zero rays: prev is looked at first", n_conv=1, prev=_arr(P), n_rays=0)
# move
rows("enslam_step_finish_native", EINVAL, "n_move > 0 with NULL move pointers", n_move=2)
rows("enslam_step_finish_native", EINVAL, "n_move > 0 with NULL move_prev", n_move=2, move_need=P)
rows("enslam_step_finish_native", EINVAL, "negative n_move", n_move=-1)
rows("enslam_step_finish_native", EINVAL, "n_move fault and 40 samples: n_move is looked at first", n_move=2, n_samples=40)
rows("enslam_step_finish_native", EINVAL, "n_move fault and zero rays", n_move=2, n_rays=0)
# order of the checks
rows(FINISH_RAYS, EUNSUPPORTED, "40 samples and empty scene", n_samples=40, scene="scene_empty")
rows(FINISH_RAYS, EUNSUPPORTED, "40 samples and NULL rays_o", n_samples=40, rays_o=None)
rows(FINISH_RAYS, EINVAL, "negative ray count and 40 samples", n_rays=-1, n_samples=40)
rows(FINISH_RAYS, OK, "zero rays, 40 samples, empty scene: the shortcut comes first", n_rays=0, n_samples=40, scene="scene_empty")
rows(FINISH_RAYS, EUNSUPPORTED, "40 samples and n_dec out of range: the ray role is checked first", n_samples=40, n_dec=5)
rows(FINISH_RAYS, EINVAL, "empty scene and n_dec out of range", scene="scene_empty", n_dec=5)
# the conversion / unpack roles every member shares
finish_rows(EINVAL, "n_dec out of range", n_dec=5)
finish_rows(EINVAL, "negative n_conv", n_conv=-1)
finish_rows(EINVAL, "n_conv without need", n_conv=1, src=_arr(P), dst=_arr(P), n_voxels=_i64(64))
finish_rows(EINVAL, "n_conv with need[0] NULL", n_conv=1, src=_arr(P), dst=_arr(P), n_voxels=_i64(64), need=_arr(None))
finish_rows(EINVAL, "n_conv without dst", n_conv=1, src=_arr(P), n_voxels=_i64(64), need=_arr(P))
finish_rows(EINVAL, "n_conv with src[0] NULL", n_conv=1, src=_arr(None), dst=_arr(P), n_voxels=_i64(64), need=_arr(P))
finish_rows(EINVAL, "negative voxel count", n_conv=1, src=_arr(P), dst=_arr(P), n_voxels=_i64(-1), need=_arr(P))
finish_rows(EINVAL, "n_dec without kinds", n_dec=1, packed_grads=_arr(P), grads="params_null")
finish_rows(EINVAL, "n_dec without grads", n_dec=1, kinds=_i32(1), packed_grads=_arr(P))
finish_rows(EINVAL, "packed_grads[0] NULL", n_dec=1, kinds=_i32(1), packed_grads=_arr(None), grads="params_null")
finish_rows(EINVAL, "unknown decoder kind", n_dec=1, kinds=_i32(7), packed_grads=_arr(P), grads="params_null")
finish_rows(OK, "a decoder whose gradient tensors are all NULL: nothing to unpack", n_dec=1, kinds=_i32(1), packed_grads=_arr(P),
            grads="params_null")

# ---- the rendering forward -------------------------------------------------------------------------------------------
rows(FWD_ALL, EINVAL, "negative ray count", n_rays=-1)
rows(FWD_ALL, OK, "zero rays", n_rays=0, rays_o=None, rays_d=None, z_vals=None, scene=None, depth=None, var=None, rgb=None, raw_out=None)
for s in (40, 80):
    rows(FWD_ALL, EUNSUPPORTED, f"{s} samples", n_samples=s)
rows(FWD_ALL, EINVAL, "empty scene", scene="scene_empty")
rows(FWD_ALL, EINVAL, "NULL scene", scene=None)
rows(FWD_ALL, EINVAL, "unknown stage", stage=4)
for a in ("rays_o", "rays_d", "z_vals", "depth", "var", "rgb"):
    rows(FWD_ALL, EINVAL, f"{a} NULL", **{a: None})
for a in ("raw_out", "gt_depth", "loss"):
    rows(FWD_LOSS, EINVAL, f"{a} NULL with a loss", **{a: None})
rows("enslam_render_tracker_loss_fwd", EINVAL, "tmp_scratch NULL", tmp_scratch=None)
rows(FWD_ALL, EUNSUPPORTED, "a workspace with a grid of 2^29 voxels", scene="scene_big", act_ws=P)
rows(FWD_LOSS, EINVAL, "work list without count", d_raw_unit=P, work_list=P)
rows(FWD_LOSS, EINVAL, "count without work list", d_raw_unit=P, work_count=P)
rows(FWD_LOSS, EINVAL, "work list with NULL d_raw_unit", work_list=P, work_count=P)
rows("enslam_render_tracker_loss_fwd", EUNSUPPORTED, "the tracker's loss at the coarse stage", stage=0)
rows("enslam_render_tracker_loss_fwd", EUNSUPPORTED, "one ray more than the tracker's tail takes", n_rays="tail_max+1")
rows("enslam_render_loss_fwd", EINVAL, "the mapper's loss at the coarse stage with a work list that lacks its count", stage=0,
     d_raw_unit=P, work_list=P)
# order of the checks
rows(FWD_ALL, EUNSUPPORTED, "40 samples and empty scene", n_samples=40, scene="scene_empty")
rows(FWD_ALL, EUNSUPPORTED, "40 samples and NULL rays_o", n_samples=40, rays_o=None)
rows(FWD_ALL, EINVAL, "negative ray count and 40 samples", n_rays=-1, n_samples=40)
rows(FWD_ALL, OK, "zero rays, 40 samples, empty scene", n_rays=0, n_samples=40, scene="scene_empty")
rows(FWD_ALL, EINVAL, "NULL depth and a grid of 2^29 voxels: pointers first", scene="scene_big", act_ws=P, depth=None)
rows(FWD_LOSS, EUNSUPPORTED, "a grid of 2^29 voxels and a list without count: voxel count first", scene="scene_big", act_ws=P,
     d_raw_unit=P, work_list=P)
rows("enslam_render_tracker_loss_fwd", EUNSUPPORTED, "coarse stage and empty scene", stage=0, scene="scene_empty")
rows("enslam_render_tracker_loss_fwd", EUNSUPPORTED, "too many rays and NULL loss", n_rays="tail_max+1", loss=None)
rows("enslam_render_tracker_loss_fwd", EINVAL, "negative ray count at the coarse stage", stage=0, n_rays=-1)
rows("enslam_render_tracker_loss_fwd", OK, "zero rays at the coarse stage", stage=0, n_rays=0)

# ---- the sampler -----------------------------------------------------------------------------------------------------
rows(SAMPLERS, EINVAL, "negative ray count", n_rays=-1)
rows(SAMPLERS, EINVAL, "no linear samples", n_lin=0)
rows(SAMPLERS, EINVAL, "negative n_surf", n_surf=-1)
for a in ("rays_o", "rays_d", "bound_host", "t_lin", "z_vals"):
    rows(SAMPLERS, EINVAL, f"{a} NULL", **{a: None})
rows(SAMPLERS, EINVAL, "gt_depth without scratch", scratch=None)
rows(SAMPLERS, EINVAL, "gt_depth and n_surf > 0 without t_surf", t_surf=None)
rows(SAMPLERS, EINVAL, "marking with an unknown stage", mark_scene="scene", mark_flags=_arr(P, P, P, P), mark_stage=4)
rows(SAMPLERS, EINVAL, "marking with a negative stage", mark_scene="scene_empty", mark_flags=_arr(P, P, P, P), mark_stage=-1)
rows(SAMPLERS_G, EINVAL, "48 voxels per flag", mark_block_voxels=48)
rows(SAMPLERS_G, EINVAL, "48 voxels per flag with zero rays", mark_block_voxels=48, n_rays=0)
rows(SAMPLERS_G, EINVAL, "no voxels per flag", mark_block_voxels=0)
# zero rays: enslam_sample_rays(_g) is done before it looks at a pointer; enslam_sample_prepare has prepare roles and goes on
rows(SAMPLERS[:2], OK, "zero rays, every pointer NULL", n_rays=0, rays_o=None, rays_d=None, gt_depth=None, bound_host=None, t_lin=None,
     t_surf=None, scratch=None, z_vals=None)
rows(SAMPLERS[:2], OK, "zero rays, marking with an unknown stage", n_rays=0, mark_scene="scene", mark_flags=_arr(P, P, P, P), mark_stage=4)
rows("enslam_sample_prepare", EINVAL, "zero rays without bound_host", n_rays=0, bound_host=None)
rows("enslam_sample_prepare", EINVAL, "zero rays, marking with an unknown stage", n_rays=0, mark_scene="scene",
     mark_flags=_arr(P, P, P, P), mark_stage=4)
rows("enslam_sample_prepare", OK, "zero rays and no prepare role: nothing to do", n_rays=0, rays_o=None, rays_d=None, gt_depth=None,
     t_lin=None, t_surf=None, scratch=None, z_vals=None)
# the prepare roles of enslam_sample_prepare
rows("enslam_sample_prepare", EINVAL, "n_dec out of range", n_dec=4)
rows("enslam_sample_prepare", EINVAL, "n_zero out of range", n_zero=5)
rows("enslam_sample_prepare", EINVAL, "negative n_flat", n_flat=-1)
rows("enslam_sample_prepare", EINVAL, "n_flat without flat", n_flat=8)
rows("enslam_sample_prepare", EINVAL, "n_dec without kinds", n_dec=1, params="params_null", packed=_arr(P))
rows("enslam_sample_prepare", EINVAL, "packed[0] NULL", n_dec=1, kinds=_i32(1), params="params_null", packed=_arr(None))
rows("enslam_sample_prepare", EINVAL, "a decoder with NULL parameter tensors", n_dec=1, kinds=_i32(1), params="params_null", packed=_arr(P))
rows("enslam_sample_prepare", EINVAL, "unknown decoder kind", n_dec=1, kinds=_i32(7), params="params_null", packed=_arr(P))
rows("enslam_sample_prepare", EINVAL, "n_zero without zero_dst", n_zero=1, zero_voxels=_i64(64))

# ---- the compositing backward ---------------------------------------------------------------------------------------
rows(COMP_ALL, EINVAL, "negative ray count", n_rays=-1)
rows(COMP_ALL, EINVAL, "no samples", n_samples=0)
for s in (65, 80):
    rows(COMP_ALL, EINVAL, f"{s} samples", n_samples=s)
rows(COMP_ALL, OK, "zero rays", n_rays=0, raw=None, z_vals=None, depth=None, d_raw=None)
rows(COMP_ALL, EINVAL, "zero rays and 80 samples: the range is looked at first", n_rays=0, n_samples=80)
for a in ("raw", "z_vals", "depth", "d_raw"):
    rows(COMP_ALL, EINVAL, f"{a} NULL", **{a: None})
rows("enslam_composite_loss_bwd", EINVAL, "gt_depth NULL", gt_depth=None)
rows("enslam_composite_loss_bwd", EINVAL, "g_loss NULL", g_loss=None)
rows("enslam_composite_loss_bwd", EINVAL, "gt_color without rgb", gt_color=P)
rows(COMP_LIST, EINVAL, "work list without count", work_list=P)
rows(COMP_LIST, EINVAL, "count without work list", work_count=P)
rows(COMP_LIST, EINVAL, "40 samples with a work list: whole tiles only", n_samples=40, work_list=P, work_count=P)

# ---- the pack / unpack loops ---------------------------------------------------------------------------------------
rows("enslam_pack_mlp_multi", OK, "no decoder", n=0, kinds=None, params=None, packed=None)
rows("enslam_pack_mlp_multi", EINVAL, "four decoders", n=4)
rows("enslam_pack_mlp_multi", EINVAL, "negative count", n=-1)
rows("enslam_pack_mlp_multi", EINVAL, "kinds NULL", kinds=None)
rows("enslam_pack_mlp_multi", EINVAL, "packed[0] NULL", packed=_arr(None))
rows("enslam_pack_mlp_multi", EINVAL, "a decoder with NULL parameter tensors")
rows("enslam_pack_mlp_multi", EINVAL, "unknown decoder kind", kinds=_i32(7))
rows("enslam_unpack_mlp_grads_multi", OK, "no decoder", n=0, kinds=None, packed_grads=None, grads=None)
rows("enslam_unpack_mlp_grads_multi", EINVAL, "five decoders", n=5)
rows("enslam_unpack_mlp_grads_multi", EINVAL, "grads NULL", grads=None)
rows("enslam_unpack_mlp_grads_multi", EINVAL, "packed_grads[0] NULL", packed_grads=_arr(None))
rows("enslam_unpack_mlp_grads_multi", EINVAL, "unknown decoder kind", kinds=_i32(7))
rows("enslam_unpack_mlp_grads_multi", OK, "gradient tensors all NULL: nothing to unpack")
rows("enslam_step_prepare", OK, "nothing to do")
rows("enslam_step_prepare", EINVAL, "four decoders", n_dec=4)
rows("enslam_step_prepare", EINVAL, "n_dec without kinds", n_dec=1, params="params_null", packed=_arr(P))
rows("enslam_step_prepare", EINVAL, "packed[0] NULL", n_dec=1, kinds=_i32(1), params="params_null", packed=_arr(None))
rows("enslam_step_prepare", EINVAL, "a decoder with NULL parameter tensors", n_dec=1, kinds=_i32(1), params="params_null", packed=_arr(P))
rows("enslam_step_prepare", EINVAL, "n_conv without need", n_conv=1, src=_arr(P), dst=_arr(P), n_voxels=_i64(64))


@pytest.fixture(scope="module")
def binding():
    import __graft_entry__ as G
    G.build()
    import evennicer_slam_amd as E
    return E._lib, E._lib.lib()


def test_the_table_covers_every_member():
    listed = {e for e, _, _, _ in ROWS}
    assert listed == set(BASE)
    for e, over, _, label in ROWS:
        assert set(over) <= {a for a, _ in BASE[e]}, (e, label)
    assert len({(e, label) for e, _, _, label in ROWS}) == len(ROWS)           # labels tell the rows of an entry apart


@pytest.mark.parametrize("entry", sorted(BASE))
def test_refusals_and_no_ops_return_the_documented_code(binding, entry):
    L, lib = binding
    assert [a for a, _ in BASE[entry]][-1] == "stream" and len(BASE[entry]) == len(L._SIGS[entry][1])
    wrong = []
    for e, over, expected, label in ROWS:
        if e != entry:
            continue
        args = [_resolve(L, lib, over.get(a, v)) for a, v in BASE[entry]]
        got = getattr(lib, entry)(*args)
        if got != expected:
            wrong.append((label, got, expected))
    assert not wrong, wrong
