"""ctypes bindings of ``librocket_hip.so`` (C-ABI declared in ``include/rocket_hip.h``).

There is no CPU fallback: if the HIP library is missing, every entry point of the
package raises.  ``torch`` is imported first so that the process has ONE HIP
runtime (torch's bundled ``libamdhip64.so`` carries the same soname,
``libamdhip64.so.7``, as the one ``librocket_hip.so`` links against; the dynamic
loader reuses the already-loaded copy).
"""
import ctypes
import os
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RR_LIB_PATH") or os.path.join(HERE, "librocket_hip.so")  # override: diagnostics only
HEADER = os.path.join(os.path.dirname(HERE), "include", "rocket_hip.h")

ABI_VERSION = 14

RR_OK, RR_EINVAL, RR_EHIP, RR_ENOMEM = 0, -1, -2, -3
RR_MODEL_3DOF, RR_MODEL_6DOF = 3, 6
RR_INT_RK4, RR_INT_EULER, RR_INT_DOPRI5 = 0, 1, 2
RR_FLAG_AUTO_RESET = 0x1
RR_FLAG_EPISODE_STATS = 0x2
RR_FLAG_REWARD_ANNEALING = 0x4
RR_FLAG_ACTION_SOA = 0x8
RR_FLAG_SCIPY_H0_CLAMP = 0x10
RR_FLAG_HOST_STATE = 0x20
RR_MAX_STATE = 14
RR_POLICY_FP32, RR_POLICY_BF16, RR_POLICY_FP16X3 = 0, 1, 2
RR_EVAL_EVENT, RR_EVAL_BOUNDS, RR_EVAL_TRUNCATED, RR_EVAL_NONFINITE, RR_EVAL_LANDED = 0x01, 0x02, 0x04, 0x08, 0x10

_d3 = ctypes.c_double * 3
_f14 = ctypes.c_float * RR_MAX_STATE
_d14 = ctypes.c_double * RR_MAX_STATE


class RrParams(ctypes.Structure):
    """Mirror of ``rr_params`` (include/rocket_hip.h)."""

    _fields_ = [
        ("model", ctypes.c_int32),
        ("integrator", ctypes.c_int32),
        ("max_episode_steps", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("dt", ctypes.c_double),
        ("ic_low", _f14),
        ("ic_high", _f14),
        ("normalizer", _d14),
        ("bounds_low", _d3),
        ("bounds_high", _d3),
        ("max_gimbal", ctypes.c_double),
        ("max_thrust", ctypes.c_double),
        ("alfa", ctypes.c_double),
        ("beta", ctypes.c_double),
        ("eta", ctypes.c_double),
        ("gamma", ctypes.c_double),
        ("delta", ctypes.c_double),
        ("kappa", ctypes.c_double),
        ("xi", ctypes.c_double),
        ("waypoint", ctypes.c_double),
        ("landing_radius", ctypes.c_double),
        ("max_velocity", ctypes.c_double),
        ("att_limit", _d3),
        ("land_att_limit", _d3),
        ("omega_lim", _d3),
    ]


class RrBuffers(ctypes.Structure):
    """Mirror of ``rr_buffers``."""

    _fields_ = [
        ("state", ctypes.c_void_p),
        ("v0", ctypes.c_void_p),
        ("elapsed", ctypes.c_void_p),
        ("ep_return", ctypes.c_void_p),
        ("done_bits", ctypes.c_void_p),
        ("terminal_obs", ctypes.c_void_p),
        ("terminal_return", ctypes.c_void_p),
        ("terminal_len", ctypes.c_void_p),
    ]


class RrEvalOut(ctypes.Structure):
    """Mirror of ``rr_eval_out`` (device pointers; any but ``episodes`` may be NULL)."""

    _fields_ = [
        ("episodes", ctypes.c_void_p),
        ("ep_return", ctypes.c_void_p),
        ("ep_length", ctypes.c_void_p),
        ("flags", ctypes.c_void_p),
        ("used_mass", ctypes.c_void_p),
        ("final_state", ctypes.c_void_p),
    ]


class RrRolloutStats(ctypes.Structure):
    """Mirror of ``rr_rollout_stats`` (device pointers; ``accum`` may be NULL)."""

    _fields_ = [
        ("partials", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("accum", ctypes.c_void_p),
    ]


# the slots of a statistics block (rocket_hip.h RR_RSTAT_*): 16 x 8 bytes
(RR_RSTAT_EPISODES, RR_RSTAT_LEN_SUM, RR_RSTAT_LANDED, RR_RSTAT_END_EVENT, RR_RSTAT_END_BOUNDS, RR_RSTAT_END_TRUNCATED,
 RR_RSTAT_END_NONFINITE, RR_RSTAT_RET_SUM, RR_RSTAT_RET_SQ, RR_RSTAT_RET_MIN, RR_RSTAT_RET_MAX, RR_RSTAT_Y_SUM,
 RR_RSTAT_Y_SQ, RR_RSTAT_D_SUM, RR_RSTAT_D_SQ, RR_RSTAT_SAMPLES, RR_RSTAT_SLOTS) = range(17)
RR_RSTAT_INT_SLOTS = (0, 1, 2, 3, 4, 5, 6, 15)


class RrPpoOptions(ctypes.Structure):
    """Mirror of ``rr_ppo_options`` (host record of rr_ppo_update_opts; 0 switches an option off)."""

    _fields_ = [
        ("clip_range_vf", ctypes.c_float),
        ("target_kl", ctypes.c_float),
        ("normalize_advantage", ctypes.c_int32),
        ("train_stats", ctypes.c_int32),
    ]


# rr_ppo_update / rr_ppo_update_opts flags and the slots of the latter's control block (rocket_hip.h
# RR_PPO_CTL_*): 16 floats
RR_PPO_CHAINED, RR_PPO_EPOCH_START = 0x1, 0x2
(RR_PPO_CTL_STOP, RR_PPO_CTL_DECIDE, RR_PPO_CTL_STEPS, RR_PPO_CTL_EVALS, RR_PPO_CTL_EPOCHS, RR_PPO_CTL_SUM_POLICY,
 RR_PPO_CTL_SUM_VALUE, RR_PPO_CTL_SUM_ENTROPY, RR_PPO_CTL_SUM_CLIP, RR_PPO_CTL_KL_SUM, RR_PPO_CTL_KL_COUNT,
 RR_PPO_CTL_KL_LAST) = range(12)
RR_PPO_CTL_SLOTS = 16
# rr_bc_update's flag and the slots of its statistics block (rocket_hip.h RR_BC_STAT_*): 8 floats
RR_BC_CHAINED = 0x1
(RR_BC_STAT_NEGLOGP, RR_BC_STAT_ENTROPY, RR_BC_STAT_ENT_LOSS, RR_BC_STAT_PROB_TRUE_ACT, RR_BC_STAT_L2_NORM,
 RR_BC_STAT_L2_LOSS, RR_BC_STAT_LOSS) = range(7)
RR_BC_STAT_SLOTS = 8
# rr_a2c_update's optimizers and the slots of its statistics block (rocket_hip.h RR_A2C_*): 8 floats
RR_A2C_RMSPROP, RR_A2C_RMSPROP_TF, RR_A2C_ADAM = range(3)
(RR_A2C_STAT_POLICY_LOSS, RR_A2C_STAT_VALUE_LOSS, RR_A2C_STAT_ENTROPY, RR_A2C_STAT_LOSS,
 RR_A2C_STAT_LOG_PROB) = range(5)
RR_A2C_STAT_SLOTS = 8


class RrEvalTrace(ctypes.Structure):
    """Mirror of ``rr_eval_trace`` (device pointers; ``action`` / ``terms`` may be NULL)."""

    _fields_ = [
        ("slot", ctypes.c_void_p),
        ("n_slots", ctypes.c_int32),
        ("steps", ctypes.c_int32),
        ("state", ctypes.c_void_p),
        ("action", ctypes.c_void_p),
        ("terms", ctypes.c_void_p),
        ("length", ctypes.c_void_p),
    ]


# symbol -> (restype, argtypes); the test suite checks this against include/rocket_hip.h
_P = ctypes.c_void_p
SIGNATURES = {
    "rr_abi_version": (ctypes.c_int, []),
    "rr_last_error": (ctypes.c_char_p, []),
    "rr_create": (ctypes.c_int, [ctypes.POINTER(_P), ctypes.POINTER(RrParams), ctypes.c_int64, ctypes.c_int64,
                                 ctypes.c_int]),
    "rr_destroy": (ctypes.c_int, [_P]),
    "rr_num_envs": (ctypes.c_int64, [_P]),
    "rr_state_dim": (ctypes.c_int, [_P]),
    "rr_action_dim": (ctypes.c_int, [_P]),
    "rr_seed": (ctypes.c_int, [_P, ctypes.c_uint64, _P]),
    "rr_reset": (ctypes.c_int, [_P, _P, _P, _P]),
    "rr_step": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "rr_step_rows": (ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    "rr_step_repeat": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, _P]),
    "rr_set_state": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "rr_get_state": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "rr_set_state64": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "rr_get_state64": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "rr_counter_bits": (ctypes.c_int, [_P]),
    "rr_get_aux": (ctypes.c_int, [_P, _P, _P, _P]),
    "rr_set_aux": (ctypes.c_int, [_P, _P, _P, _P]),
    "rr_get_buffers": (ctypes.c_int, [_P, ctypes.POINTER(RrBuffers)]),
    "rr_host_alloc": (ctypes.c_int, [ctypes.POINTER(_P), ctypes.c_int64]),
    "rr_host_free": (ctypes.c_int, [_P]),
    "rr_fetch_done": (ctypes.c_int64, [_P, ctypes.c_int64, _P, _P, _P, _P, _P]),
    "rr_copy_terminal": (ctypes.c_int, [_P, _P, _P, _P, _P]),
    "rr_gather_rows": (ctypes.c_int64, [_P, _P, _P, _P, _P, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P]),
    "rr_policy_layout": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "rr_policy_pack": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    "rr_policy_act": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, _P,
                                     ctypes.c_uint64, _P, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P,
                                     ctypes.c_float, _P, _P, _P, _P]),
    "rr_policy_bootstrap": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P, _P, _P,
                                           ctypes.c_float, _P, _P, _P, _P]),
    "rr_rollout_step": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_uint64, _P, ctypes.c_int, ctypes.c_float,
                                       _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rr_rollout_collect": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_uint64, _P, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_double] + [_P] * 17),
    "rr_rollout_stats_rows": (ctypes.c_int64, [ctypes.c_int64]),
    "rr_rollout_collect_stats": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_uint64, _P, ctypes.c_int,
                                                ctypes.c_double, ctypes.c_double] + [_P] * 16 +
                                 [ctypes.POINTER(RrRolloutStats), _P]),
    "rr_policy_evaluate": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                          ctypes.POINTER(RrEvalOut), _P, _P]),
    "rr_policy_evaluate_trace": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                ctypes.POINTER(RrEvalOut), ctypes.POINTER(RrEvalTrace), _P, _P]),
    "rr_policy_evaluate_exact": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                ctypes.POINTER(RrEvalOut), _P, _P]),
    "rr_policy_evaluate_exact_trace": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                      ctypes.POINTER(RrEvalOut), ctypes.POINTER(RrEvalTrace), _P, _P]),
    "rr_gae": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, ctypes.c_double, ctypes.c_double, _P,
                              _P, _P]),
    "rr_clip_adam_workspace_size": (ctypes.c_int, [ctypes.c_int64, _P]),
    "rr_clip_adam": (ctypes.c_int, [ctypes.c_int, _P, _P, _P, _P, _P, _P, ctypes.c_float, _P, ctypes.c_double,
                                    ctypes.c_double, ctypes.c_float, _P, ctypes.c_int64, _P]),
    "rr_ppo_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_ppo_grad": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_int64,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P, ctypes.c_int64, _P]),
    "rr_ppo_update_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_ppo_update": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 11 + [ctypes.c_int64, _P, ctypes.c_int64,
                                     ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P,
                                     ctypes.c_double, ctypes.c_double, ctypes.c_float, _P, ctypes.c_uint32, _P,
                                     ctypes.c_int64, _P]),
    "rr_ppo_update_opts_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_ppo_update_opts": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 12 +
                           [ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                            ctypes.c_float, _P, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                            ctypes.POINTER(RrPpoOptions), _P, _P, ctypes.c_uint32, _P, ctypes.c_int64, _P]),
    "rr_bc_update_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_bc_update": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 8 +
                     [ctypes.c_int64, ctypes.c_float, ctypes.c_float, _P, ctypes.c_double, ctypes.c_double,
                      ctypes.c_float, _P, ctypes.c_uint32, _P, ctypes.c_int64, _P]),
    "rr_a2c_update_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_a2c_update": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 10 +
                      [ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, _P,
                       ctypes.c_double, ctypes.c_double, ctypes.c_float, _P, _P, ctypes.c_int64, _P]),
    "rr_a2c_update_discrete_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_a2c_update_discrete": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 10 +
                               [ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                ctypes.c_int, _P, ctypes.c_double, ctypes.c_double, ctypes.c_float, _P, _P,
                                ctypes.c_int64, _P]),
    "rr_policy_layout_discrete": (ctypes.c_int, [ctypes.c_int, _P]),
    "rr_policy_pack_discrete": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    "rr_policy_act_discrete": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int64,
                                              ctypes.c_int64, _P, ctypes.c_uint64, _P, ctypes.c_int, _P, _P, _P, _P,
                                              _P, _P, _P, _P, ctypes.c_float, _P, _P, _P, _P]),
    "rr_ppo_update_discrete_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_ppo_update_discrete": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 11 +
                               [ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                ctypes.c_float, _P, ctypes.c_double, ctypes.c_double, ctypes.c_float, _P,
                                ctypes.c_uint32, _P, ctypes.c_int64, _P]),
    "rr_ppo_update_discrete_opts_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_ppo_update_discrete_opts": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 12 +
                                    [ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_float, ctypes.c_float,
                                     ctypes.c_float, ctypes.c_float, _P, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_float, ctypes.POINTER(RrPpoOptions), _P, _P, ctypes.c_uint32, _P,
                                     ctypes.c_int64, _P]),
    "rr_bc_update_discrete_workspace_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P]),
    "rr_bc_update_discrete": (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + [_P] * 8 +
                              [ctypes.c_int64, ctypes.c_float, ctypes.c_float, _P, ctypes.c_double, ctypes.c_double,
                               ctypes.c_float, _P, ctypes.c_uint32, _P, ctypes.c_int64, _P]),
    # the Gaussian calls' arguments with (n_choices, table) after params
    "rr_rollout_step_discrete": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_uint64, _P,
                                                ctypes.c_int, ctypes.c_float] + [_P] * 12),
    "rr_rollout_collect_discrete": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_uint64, _P,
                                                   ctypes.c_int, ctypes.c_double, ctypes.c_double] + [_P] * 17),
    "rr_policy_evaluate_discrete": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int64, ctypes.POINTER(RrEvalOut), _P, _P]),
    # rr_rollout_collect_stats's / rr_policy_evaluate_trace's arguments with (n_choices, table) after params;
    # the latter with the choice plane after the trace
    "rr_rollout_collect_discrete_stats": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_uint64, _P,
                                                         ctypes.c_int, ctypes.c_double, ctypes.c_double] + [_P] * 16 +
                                          [ctypes.POINTER(RrRolloutStats), _P]),
    "rr_policy_evaluate_discrete_trace": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int64, ctypes.POINTER(RrEvalOut),
                                                         ctypes.POINTER(RrEvalTrace), _P, _P, _P]),
    # rr_policy_evaluate_discrete's arguments, for an RR_INT_DOPRI5 handle
    "rr_policy_evaluate_exact_discrete": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int64, ctypes.POINTER(RrEvalOut), _P, _P]),
    # rr_policy_evaluate_trace's / rr_policy_evaluate_discrete_trace's arguments with (seed, iter) after the
    # precision; the trace may be None (the plain call)
    "rr_policy_evaluate_sampled": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_uint64, _P, ctypes.c_int,
                                                  ctypes.c_int64, ctypes.POINTER(RrEvalOut),
                                                  ctypes.POINTER(RrEvalTrace), _P, _P]),
    "rr_policy_evaluate_discrete_sampled": (ctypes.c_int, [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_uint64, _P,
                                                           ctypes.c_int, ctypes.c_int64, ctypes.POINTER(RrEvalOut),
                                                           ctypes.POINTER(RrEvalTrace), _P, _P, _P]),
}

_LIB = None


class RocketHipError(RuntimeError):
    pass


def load(require_torch=True):
    """Load librocket_hip.so (raises if it has not been built: no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if require_torch:
        import torch  # noqa: F401  (one HIP runtime per process, see module doc)
    if not os.path.exists(LIB_PATH):
        raise RocketHipError(
            "librocket_hip.so is not built (expected at %s). Build it with "
            "`python -m rl_rocket_amd.build` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    override = bool(os.environ.get("RR_LIB_PATH"))
    missing = []
    for name, (res, args) in SIGNATURES.items():
        if override and not hasattr(lib, name):
            missing.append(name)  # an older diagnostic build (tools/ab_kernel.py) may lack newer entry points
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    abi = lib.rr_abi_version()
    if abi != ABI_VERSION:
        if not override:
            raise RocketHipError("librocket_hip.so ABI %d != expected %d" % (abi, ABI_VERSION))
        # diagnostic builds may be older: say so now rather than as a wrong counter decoding later
        warnings.warn("RR_LIB_PATH=%s has ABI %d, this package expects %d%s" % (
            LIB_PATH, abi, ABI_VERSION, (" (missing: %s)" % ", ".join(missing)) if missing else ""),
            RuntimeWarning, stacklevel=2)
    for name in missing:  # a call of a missing entry point raises a clear error at the call site
        setattr(lib, name, _missing(name))
    _LIB = lib
    return lib


def _missing(name):
    def call(*a, **k):
        raise RocketHipError("%s is not exported by the RR_LIB_PATH library %s (ABI mismatch)" % (name, LIB_PATH))
    return call


def check(rc, what="rocket_hip"):
    if rc < 0:
        msg = load().rr_last_error()
        raise RocketHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))
    return rc
