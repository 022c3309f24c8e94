"""ctypes binding of libdx.so (include/dx.h).

The library is built in-tree (`dexterity_amd/libdx.so`, see `build.py`).  There is
deliberately no fallback: if the HIP library is missing or cannot reach a GPU,
every entry point raises.
"""

from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DX_LIB") or os.path.join(_HERE, "libdx.so")  # DX_LIB: A/B-test a variant build

# dx_field
QPOS, QVEL, CTRL, QACC_WARMSTART, QACC, TIME = 0, 1, 2, 3, 4, 5
SITE_XPOS, SITE_VEL, XPOS, XQUAT, NCON, GROUND_CONTACT, NITER, NCAND, STEP_COST = 6, 7, 8, 9, 10, 11, 12, 13, 14
SENSOR_TORQUE, DIVERGED = 15, 16
CFRC_EXT, PAD_FORCE = 17, 18  # contact force sensing (dx_contact_enable / dx_contact_set_pads)
MAX_PADS = 64
INT_FIELDS = (NCON, GROUND_CONTACT, NITER, NCAND, STEP_COST, DIVERGED)
HEALTH_WORDS, NCON_HIST = 16, 65
HEALTH = ("contact_overflow", "candidate_overflow", "jacobian_dof_overflow", "row_overflow", "diverged",
          "ncon_max", "contact_deferred", "mid_tier_gave_up", "deferred_behind_launch")

EXPORTS = (
    "dx_model_load", "dx_model_free", "dx_model_sizes", "dx_model_lds_bytes", "dx_field_width",
    "dx_batch_create", "dx_batch_destroy", "dx_batch_nenv", "dx_reset",
    "dx_set_field", "dx_get_field", "dx_field_ptr", "dx_set_xfrc", "dx_set_ground_geom",
    "dx_set_watch", "dx_step", "dx_forward", "dx_stream", "dx_sync",
    "dx_debug_enable", "dx_debug_get", "dx_last_error", "dx_abi_version",
    "dx_env_create", "dx_env_destroy", "dx_env_batch", "dx_env_obs_dim", "dx_env_reset",
    "dx_env_step", "dx_env_output", "dx_env_action_buffer", "dx_env_sample_actions",
    "dx_env_pack_outputs", "dx_timing_enable", "dx_timing_read", "dx_stage_timing", "dx_stage_read",
    "dx_debug_poison_lds", "dx_hull_support", "dx_model_layout", "dx_env_goal_dim",
    "dx_jac_site", "dx_ik_solve", "dx_jac_object", "dx_dls_map",
    "dx_comm_unique_id", "dx_comm_init", "dx_comm_destroy", "dx_comm_rank", "dx_comm_size",
    "dx_allgather_obs", "dx_comm_allreduce_max", "dx_comm_barrier", "dx_sensor_enable",
    "dx_env_set_time_limit", "dx_set_outputs", "dx_env_create_shard",
    "dx_health", "dx_health_clear", "dx_ncon_histogram", "dx_env_set_goal_time_limit",
    "dx_env_step_random", "dx_env_save", "dx_env_load", "dx_env_state_field", "dx_env_step_host",
    "dx_build_key", "dx_env_set_action_filter", "dx_env_action_noise_draw",
    "dx_env_set_hand_observables", "dx_env_hand_obs_dim",
    "dx_env_set_obs_pipeline", "dx_env_obs_pipe_dims", "dx_env_obs_noise_draw",
    "dx_contact_enable", "dx_contact_set_pads", "dx_contact_npad",
    "dx_env_set_contact_forces", "dx_env_contact_force_dim", "dx_env_contact_force_bodies",
    "dx_set_xfrc_env", "dx_get_xfrc_env", "dx_xfrc_ptr", "dx_env_set_perturbation", "dx_env_perturb_draw",
    "dx_model_hull_planes", "dx_render_set_cameras", "dx_render", "dx_render_output", "dx_render_get",
    "dx_render_stats", "dx_ray", "dx_env_set_cameras",
    "dx_render_set_shading", "dx_env_set_shading", "dx_render_stats2",
)
COMM_ID_BYTES = 128
STAGES = ("kinematics", "crb", "broadphase", "midphase", "narrowphase", "constraints", "velocity",
          "smooth_solve", "newton_eval", "newton_grad", "newton_hessian", "newton_chol", "newton_linesearch",
          "qfrc_constraint", "euler", "observe", "io", "matvec", "np_mpr", "jacvec")
COUNTERS = {20: "plane_box", 21: "plane_convex", 22: "capsule", 23: "mpr", 24: "mpr_support", 25: "mpr_hit",
            26: "mpr_maxit", 27: "newton_iter", 28: "linesearch_iter", 29: "solves", 30: "nefc",
            31: "np_trips", 32: "broad_keep", 33: "mid_pairs", 34: "mid_keep", 35: "queue_wait"}
NSTAGE = 48
# the narrowphase trip's parts (DX_NP_MARKS builds only)
NP_STAGES = {36: "np_loop", 37: "np_fresh", 38: "np_supload", 39: "np_supred", 40: "np_portal"}
OUT_OBS, OUT_REWARD, OUT_DISCOUNT, OUT_STEP_TYPE, OUT_GOAL, OUT_SUCCESSES, OUT_GOAL_FAILURES, OUT_GOAL_QPOS = range(8)
OUT_PREV_ACTION = 8
ACT_NOISE, ACT_SMOOTH, ACT_PREVIOUS = 1, 2, 4  # dx_action_filter.flags
OUT_HAND_OBS = 9
# dx_hand_obs.mask, in the order of the row's blocks within a hand
HOBS_JOINT_POSITIONS, HOBS_TIP_ORIENTATIONS, HOBS_TIP_ANGULAR_VELOCITIES, HOBS_TIP_POSITIONS_EGO = 1, 2, 4, 8
OUT_OBS_BUFFER = 10
OUT_CONTACT_FORCE = 11
OUT_PERTURB = 12
PERTURB_MAX_BODIES = 4
OUT_DEPTH, OUT_SEGMENTATION = 13, 14
RENDER_DEPTH, RENDER_SEGMENTATION, RENDER_NO_CULL = 1, 2, 4  # dx_render_set_cameras flags / dx_render_output
RENDER_MAX_CAMERAS, RENDER_MAX_SIDE = 8, 512
OUT_RGB = 15
RENDER_RGB = 8
RENDER_MAX_LIGHTS, RENDER_MAX_FACE_GEOMS = 4, 8
# dx_obs_pipeline.padding / .aggregator, by composer's names
OBS_PAD = {"zero": 0, "initial_value": 1}
OBS_AGG = {None: 0, "min": 1, "max": 2, "mean": 3, "median": 4, "sum": 5}
OBS_INTERVAL_MAX, OBS_DELAY_MAX, OBS_BUFFER_MAX = 64, 64, 16  # control steps, control steps, slots
TASK_REORIENT, TASK_REACH, TASK_HANDOVER = 0, 1, 2
OBJ_BODY, OBJ_GEOM, OBJ_SITE = 1, 5, 6  # dx_obj_type (MuJoCo's mjtObj values)
REACH_NPARAMS_HEAD = 26

_lib = None


class DxError(RuntimeError):
    pass


class IkOptions(ctypes.Structure):
    """struct dx_ik_options (include/dx.h)."""

    _fields_ = [
        ("linear_tol", ctypes.c_float),
        ("regularization", ctypes.c_float),
        ("gain", ctypes.c_float),
        ("progress_threshold", ctypes.c_float),
        ("max_steps", ctypes.c_int32),
        ("early_stop", ctypes.c_int32),
        ("num_attempts", ctypes.c_int32),
        ("stop_on_first", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
    ]


class ActionFilter(ctypes.Structure):
    """struct dx_action_filter (include/dx.h)."""

    _fields_ = [
        ("flags", ctypes.c_int32),
        ("noise_scale", ctypes.c_float),
        ("smooth_alpha", ctypes.c_double),
        ("noise_seed", ctypes.c_uint64),
    ]


class HandObs(ctypes.Structure):
    """struct dx_hand_obs (include/dx.h)."""

    _fields_ = [
        ("mask", ctypes.c_int32),
        ("nhands", ctypes.c_int32),
        ("root_body", ctypes.c_int32 * 2),
    ]


class ObsPipeline(ctypes.Structure):
    """struct dx_obs_pipeline (include/dx.h)."""

    _fields_ = [
        ("update_interval", ctypes.c_int32),
        ("delay", ctypes.c_int32),
        ("buffer_size", ctypes.c_int32),
        ("aggregator", ctypes.c_int32),
        ("padding", ctypes.c_int32),
        ("noise", ctypes.c_int32),
        ("noise_seed", ctypes.c_uint64),
        ("noise_sigma", ctypes.c_void_p),
        ("nsigma", ctypes.c_int32),
    ]


class Perturbation(ctypes.Structure):
    """struct dx_perturbation (include/dx.h)."""

    _fields_ = [
        ("nbody", ctypes.c_int32),
        ("bodies", ctypes.c_int32 * 4),
        ("probability", ctypes.c_double),
        ("force_min", ctypes.c_double),
        ("force_max", ctypes.c_double),
        ("torque_min", ctypes.c_double),
        ("torque_max", ctypes.c_double),
        ("duration", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
    ]


class Camera(ctypes.Structure):
    """struct dx_camera (include/dx.h)."""

    _fields_ = [
        ("pos", ctypes.c_float * 3),
        ("xyaxes", ctypes.c_float * 6),
        ("fovy", ctypes.c_float),
        ("near_", ctypes.c_float),
        ("far_", ctypes.c_float),
        ("body", ctypes.c_int32),
    ]


class Light(ctypes.Structure):
    """struct dx_light (include/dx.h)."""

    _fields_ = [
        ("pos", ctypes.c_float * 3),
        ("dir", ctypes.c_float * 3),
        ("diffuse", ctypes.c_float * 3),
        ("directional", ctypes.c_int32),
        ("castshadow", ctypes.c_int32),
    ]


class Shading(ctypes.Structure):
    """struct dx_shading (include/dx.h)."""

    _fields_ = [
        ("ambient", ctypes.c_float * 3),
        ("background", ctypes.c_float * 3),
        ("headlight", ctypes.c_float * 3),
        ("checker_rgb", ctypes.c_float * 6),
        ("checker_cell", ctypes.c_float),
    ]


def shading_args(geom_rgb, face_geom, face_rgb, lights, shading):
    """The arguments of dx_render_set_shading / dx_env_set_shading behind the handle, from
    what cameras.validate_shading returns (None: that part's default), and the objects that
    must stay alive over the call."""
    nface = 0 if face_geom is None else len(face_geom)
    fg = None if face_geom is None else (ctypes.c_int32 * max(nface, 1))(*[int(g) for g in face_geom])
    larr = None
    if lights is not None:
        larr = (Light * max(len(lights), 1))()
        for c, l in zip(larr, lights):
            c.pos[:] = [float(v) for v in l.pos]
            c.dir[:] = [float(v) for v in l.dir]
            c.diffuse[:] = [float(v) for v in l.diffuse]
            c.directional, c.castshadow = int(bool(l.directional)), int(bool(l.castshadow))
    sh = None
    if shading is not None:
        sh = Shading()
        sh.ambient[:] = [float(v) for v in shading.ambient]
        sh.background[:] = [float(v) for v in shading.background]
        sh.headlight[:] = [float(v) for v in shading.headlight]
        sh.checker_rgb[:] = [float(v) for row in shading.checker_rgb for v in row]
        sh.checker_cell = float(shading.checker_cell)
    keep = (geom_rgb, face_rgb, fg, larr, sh)
    args = (None if geom_rgb is None else geom_rgb.ctypes.data, fg,
            None if face_rgb is None or not nface else face_rgb.ctypes.data, nface,
            larr, 0 if lights is None else len(lights), None if sh is None else ctypes.byref(sh))
    return args, keep


def load(path: str = LIB_PATH):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise DxError(
            f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')"
        )
    L = ctypes.CDLL(path)
    if not hasattr(L, "dx_build_key"):
        raise DxError(f"{path} has no dx_build_key: it is not a libdx.so of these sources, rebuild it "
                      "(python -c 'import __graft_entry__ as g; g.build()')")
    L.dx_build_key.restype = ctypes.c_char_p
    if path == os.path.join(_HERE, "libdx.so") and os.path.isdir(os.path.join(_HERE, "csrc")):
        # the in-tree library must have been built from the sources beside it (a GPU box
        # runs the library that travelled with the tree, without rebuilding)
        from dexterity_amd import build as _build

        want, have = _build.source_key(), L.dx_build_key().decode()
        if want != have:
            raise DxError(f"{path} was built from other sources (key {have}, sources {want}): rebuild it "
                          "(python -c 'import __graft_entry__ as g; g.build()')")
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    L.dx_model_load.restype = vp
    L.dx_model_load.argtypes = [ctypes.c_char_p, sz]
    L.dx_model_free.argtypes = [vp]
    L.dx_model_sizes.argtypes = [vp, ctypes.POINTER(i32)]
    L.dx_model_lds_bytes.argtypes = [vp]
    L.dx_field_width.argtypes = [vp, ctypes.c_int]
    L.dx_model_layout.argtypes = [vp, ctypes.POINTER(i32), i32]
    L.dx_hull_support.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i32)]
    L.dx_batch_create.restype = vp
    L.dx_batch_create.argtypes = [vp, i32, i32]
    L.dx_batch_destroy.argtypes = [vp]
    L.dx_batch_nenv.argtypes = [vp]
    L.dx_reset.argtypes = [vp, i32, i32]
    L.dx_set_field.argtypes = [vp, ctypes.c_int, vp, i32, i32]
    L.dx_get_field.argtypes = [vp, ctypes.c_int, vp, i32, i32]
    L.dx_field_ptr.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp)]
    L.dx_set_xfrc.argtypes = [vp, vp, i32]
    L.dx_set_ground_geom.argtypes = [vp, i32]
    L.dx_set_watch.argtypes = [vp, i32, i32]
    L.dx_step.argtypes = [vp, i32]
    L.dx_forward.argtypes = [vp]
    L.dx_stream.restype = vp
    L.dx_stream.argtypes = [vp]
    L.dx_sync.argtypes = [vp]
    L.dx_debug_enable.argtypes = [vp, ctypes.c_int]
    L.dx_sensor_enable.argtypes = [vp, ctypes.c_int]
    L.dx_set_outputs.argtypes = [vp, ctypes.c_int]
    L.dx_debug_get.argtypes = [vp, ctypes.c_char_p, vp, sz]
    L.dx_last_error.restype = ctypes.c_char_p
    L.dx_abi_version.restype = ctypes.c_int
    L.dx_env_create.restype = vp
    L.dx_env_create.argtypes = [vp, i32, i32, i32, ctypes.c_uint64, vp, i32]
    L.dx_health.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), i32]
    L.dx_health_clear.argtypes = [vp]
    L.dx_ncon_histogram.argtypes = [vp, ctypes.c_int]
    L.dx_env_create_shard.restype = vp
    L.dx_env_create_shard.argtypes = [vp, i32, i32, i32, ctypes.c_uint64, ctypes.c_int64, vp, i32]
    L.dx_env_destroy.argtypes = [vp]
    L.dx_env_batch.restype = vp
    L.dx_env_batch.argtypes = [vp]
    L.dx_env_obs_dim.argtypes = [vp]
    L.dx_env_goal_dim.argtypes = [vp]
    L.dx_env_reset.argtypes = [vp]
    L.dx_env_step.argtypes = [vp, vp]
    L.dx_env_set_time_limit.argtypes = [vp, ctypes.c_double]
    L.dx_env_set_goal_time_limit.argtypes = [vp, ctypes.c_double]
    L.dx_env_output.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp)]
    L.dx_env_action_buffer.argtypes = [vp, ctypes.POINTER(vp)]
    L.dx_env_sample_actions.argtypes = [vp, ctypes.c_uint64, i32]
    L.dx_env_step_random.argtypes = [vp, ctypes.c_uint64, i32]
    L.dx_env_save.argtypes = [vp, vp, sz]
    L.dx_env_load.argtypes = [vp, vp, sz]
    L.dx_env_state_field.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz),
                                     ctypes.POINTER(sz)]
    L.dx_env_pack_outputs.argtypes = [vp, vp]
    if hasattr(L, "dx_env_step_host"):  # (round 6; an older variant library for A/B lacks it)
        L.dx_env_step_host.argtypes = [vp, vp, vp]
    if hasattr(L, "dx_env_set_action_filter"):  # (an older variant library for A/B lacks the action pipeline)
        L.dx_env_set_action_filter.argtypes = [vp, ctypes.POINTER(ActionFilter)]
        L.dx_env_action_noise_draw.argtypes = [vp, i32, vp]
    if hasattr(L, "dx_env_set_hand_observables"):  # (an older variant library for A/B lacks the hand observables)
        L.dx_env_set_hand_observables.argtypes = [vp, ctypes.POINTER(HandObs)]
        L.dx_env_hand_obs_dim.argtypes = [vp]
    if hasattr(L, "dx_env_set_obs_pipeline"):  # (an older variant library for A/B lacks the observation pipeline)
        L.dx_env_set_obs_pipeline.argtypes = [vp, ctypes.POINTER(ObsPipeline)]
        L.dx_env_obs_pipe_dims.argtypes = [vp, ctypes.POINTER(i32)]
        L.dx_env_obs_noise_draw.argtypes = [vp, i32, vp]
    if hasattr(L, "dx_contact_enable"):  # (an older variant library for A/B lacks contact force sensing)
        L.dx_contact_enable.argtypes = [vp, ctypes.c_int]
        L.dx_contact_set_pads.argtypes = [vp, vp, i32]
        L.dx_contact_npad.argtypes = [vp]
        L.dx_env_set_contact_forces.argtypes = [vp, ctypes.c_int]
        L.dx_env_contact_force_dim.argtypes = [vp]
        L.dx_env_contact_force_bodies.argtypes = [vp, ctypes.POINTER(i32), i32]
    if hasattr(L, "dx_set_xfrc_env"):  # (an older variant library for A/B lacks per-env wrenches and the pushes)
        L.dx_set_xfrc_env.argtypes = [vp, vp, i32, i32]
        L.dx_get_xfrc_env.argtypes = [vp, vp, i32, i32]
        L.dx_xfrc_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i32)]
        L.dx_env_set_perturbation.argtypes = [vp, ctypes.POINTER(Perturbation)]
        L.dx_env_perturb_draw.argtypes = [vp, i32, vp]
    if hasattr(L, "dx_render_set_cameras"):  # (an older variant library for A/B lacks the cameras)
        L.dx_model_hull_planes.argtypes = [vp, i32, vp, i32]
        L.dx_render_set_cameras.argtypes = [vp, vp, i32, i32, i32, i32]
        L.dx_render.argtypes = [vp]
        L.dx_render_output.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp)]
        L.dx_render_get.argtypes = [vp, ctypes.c_int, vp, i32, i32]
        L.dx_render_stats.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        L.dx_ray.argtypes = [vp, vp, vp, i32, vp, vp]
        L.dx_env_set_cameras.argtypes = [vp, vp, i32, i32, i32, i32]
    if hasattr(L, "dx_render_set_shading"):  # (an older variant library for A/B lacks the shaded RGB)
        L.dx_render_set_shading.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp]
        L.dx_env_set_shading.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp]
        L.dx_render_stats2.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.dx_timing_enable.argtypes = [vp, ctypes.c_int]
    L.dx_timing_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i32)]
    L.dx_stage_timing.argtypes = [vp, ctypes.c_int]
    L.dx_stage_read.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), i32]
    L.dx_debug_poison_lds.argtypes = [i32]
    L.dx_jac_site.argtypes = [vp, vp, i32, vp, vp]
    L.dx_ik_solve.argtypes = [vp, ctypes.POINTER(IkOptions), vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "dx_dls_map"):  # (an older variant library for A/B lacks the velocity mapper)
        L.dx_jac_object.argtypes = [vp, vp, vp, i32, vp, vp]
        L.dx_dls_map.argtypes = [vp, vp, vp, i32, ctypes.c_float, vp, vp, vp]
    L.dx_comm_unique_id.argtypes = [vp]
    L.dx_comm_init.restype = vp
    L.dx_comm_init.argtypes = [ctypes.c_char_p, i32, i32, i32]
    L.dx_comm_destroy.argtypes = [vp]
    L.dx_comm_rank.argtypes = [vp]
    L.dx_comm_size.argtypes = [vp]
    L.dx_allgather_obs.argtypes = [vp, vp, vp]
    L.dx_comm_allreduce_max.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.dx_comm_barrier.argtypes = [vp]
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        raise DxError(f"libdx error {rc}: {load().dx_last_error().decode()}")
    return rc
