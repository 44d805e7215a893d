"""ctypes binding of libdartmpc.so (the C ABI declared in include/dart_mpc.h).

The product path has exactly one implementation: the HIP kernel in this
library.  There is no CPU fallback -- if the library or a GPU is missing,
every solve raises ``DartMPCError``.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import subprocess
import threading
import weakref

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(os.path.dirname(PKG_DIR), "csrc")
# DART_MPC_LIB: file name of an alternative in-tree build.  The product path loads only a library built from the
# sources beside it (build_id below): the product library itself, or a diagnostic build of the same sources
# (phase stamps, restoration trace).  A/B timing of two different builds (tools/ab_lib.sh) must say so with
# DART_MPC_AB=1, which only the A/B tools set.
LIB_NAME = os.path.basename(os.environ.get("DART_MPC_LIB", "libdartmpc.so"))
LIB_PATH = os.path.join(PKG_DIR, LIB_NAME)

SOLVED, ACCEPTABLE, INFEASIBLE, MAXITER, LS_FAIL, INERTIA_FAIL, MAXTIME = 0, 1, 2, -1, -2, -3, -4
STATUS_NAMES = {SOLVED: "Solve_Succeeded", ACCEPTABLE: "Solved_To_Acceptable_Level", INFEASIBLE: "Infeasible_Problem_Detected",
                MAXITER: "Maximum_Iterations_Exceeded", LS_FAIL: "Restoration_Failed",
                INERTIA_FAIL: "Error_In_Step_Computation", MAXTIME: "Maximum_CpuTime_Exceeded"}

# exported symbols of include/dart_mpc.h (tests check every one is present)
EXPORTS = ("dart_mpc_config_default", "dart_mpc_create", "dart_mpc_solve_batch", "dart_mpc_solve_batch_dev",
           "dart_mpc_sync", "dart_mpc_last_error", "dart_mpc_destroy", "dart_mpc_nw", "dart_mpc_abi_version",
           "dart_rmpc_solve_batch", "dart_rmpc_solve_batch_dev", "dart_rmpc_nw",
           "dart_rls_update_batch", "dart_rls_update_batch_dev",
           "dart_lmpc_solve_batch", "dart_lmpc_solve_batch_dev", "dart_lmpc_nw",
           "dart_lmpc_policy_config_default", "dart_lmpc_policy_step", "dart_lmpc_policy_step_dev",
           "dart_lmpc_policy_solve_batch", "dart_lmpc_policy_solve_batch_dev",
           "dart_arm_config_default", "dart_arm_snapshot_len", "dart_arm_param_len", "dart_arm_solve_batch",
           "dart_arm_solve_batch_dev", "dart_set_device", "dart_mpc_serve_start", "dart_mpc_serve_stop",
           "dart_mpc_serve_running", "dart_mpc_bind", "dart_mpc_solve_bound", "dart_mpc_build_id",
           "dart_mpc_build_flavor",
           "dart_plant_config_default", "dart_rmpc_loop_config_default", "dart_rmpc_loop_step_dev",
           "dart_pmpc_loop_step_dev", "dart_rmpc_rollout_dev", "dart_pmpc_rollout_dev", "dart_rmpc_rollout",
           "dart_pmpc_rollout", "dart_lmpc_loop_step_dev", "dart_lmpc_rollout_dev", "dart_lmpc_rollout",
           "dart_lmpc_reward_config_default", "dart_lmpc_experience_step_dev", "dart_lmpc_collect_dev",
           "dart_lmpc_collect", "dart_lmpc_gae_dev", "dart_lmpc_gae",
           "dart_lmpc_ppo_config_default", "dart_lmpc_ppo_workspace_bytes", "dart_lmpc_ppo_update_dev",
           "dart_lmpc_ppo_update", "dart_lmpc_ppo_prepare_dev", "dart_lmpc_ppo_grad_dev", "dart_lmpc_ppo_apply_dev",
           "dart_lmpc_critic_value_dev", "dart_lmpc_critic_value",
           "dart_lmpc_philox_dev", "dart_lmpc_noise_dev", "dart_lmpc_noise", "dart_lmpc_perms_dev", "dart_lmpc_perms",
           "dart_lmpc_mean_param_update_dev", "dart_lmpc_mean_param_update", "dart_lmpc_train_config_default",
           "dart_lmpc_train_workspace_bytes", "dart_lmpc_train_dev", "dart_lmpc_train",
           "dart_lmpc_choice_dev", "dart_lmpc_choice", "dart_lmpc_perms_stream_dev", "dart_lmpc_global_rows",
           "dart_lmpc_global_fill_after", "dart_lmpc_global_workspace_bytes", "dart_lmpc_global_append_dev",
           "dart_lmpc_global_append", "dart_lmpc_gae_seq_dev", "dart_lmpc_gae_seq", "dart_lmpc_train_global_dev",
           "dart_lmpc_train_global",
           "dart_lmpc_train_pop_workspace_bytes", "dart_lmpc_train_pop_dev", "dart_lmpc_train_pop",
           "dart_lmpc_global_pop_workspace_bytes", "dart_lmpc_choice_pop_dev", "dart_lmpc_global_append_pop_dev",
           "dart_lmpc_gae_seq_pop_dev", "dart_lmpc_train_pop_global_dev", "dart_lmpc_train_pop_global",
           "dart_pmpc_lm_loop_step_dev", "dart_pmpc_lm_rollout_dev", "dart_pmpc_lm_rollout",
           "dart_rmpc_lm_loop_step_dev", "dart_rmpc_lm_rollout_dev", "dart_rmpc_lm_rollout",
           "dart_lmpc_eval_loop_step_dev", "dart_lmpc_eval_dev", "dart_lmpc_eval", "dart_lmpc_eval_scores_dev",
           "dart_lmpc_eval_scores",
           "dart_lmpc_train_pop_hyper_dev", "dart_lmpc_train_pop_hyper", "dart_lmpc_pbt_config_default",
           "dart_lmpc_pbt_step_dev", "dart_lmpc_pbt_step",
           "dart_arm_dyn_config_default", "dart_arm_model_len", "dart_arm_state_len", "dart_arm_dynamics_batch_dev",
           "dart_arm_dynamics_batch", "dart_arm_control_batch_dev", "dart_arm_control_batch",
           "dart_dual_arm_control_dev", "dart_dual_arm_control", "dart_dual_arm_work_len",
           "dart_dual_arm_rollout_dev", "dart_dual_arm_rollout",
           "dart_stack_config_default", "dart_stack_work_len", "dart_tray_from_arms_dev", "dart_tray_from_arms",
           "dart_pmpc_stack_loop_step_dev", "dart_pmpc_stack_lm_loop_step_dev", "dart_pmpc_stack_rollout_dev",
           "dart_pmpc_stack_lm_rollout_dev", "dart_pmpc_stack_rollout", "dart_pmpc_stack_lm_rollout",
           "dart_rmpc_stack_loop_step_dev", "dart_rmpc_stack_lm_loop_step_dev", "dart_rmpc_stack_rollout_dev",
           "dart_rmpc_stack_lm_rollout_dev", "dart_rmpc_stack_rollout", "dart_rmpc_stack_lm_rollout")
VARIANT_PMPC, VARIANT_RMPC, VARIANT_LMPC = 0, 1, 2
ABI_VERSION = 8


class DartMPCError(RuntimeError):
    pass


class Config(ctypes.Structure):
    """Mirror of ``struct dart_mpc_config``."""
    _fields_ = [("variant", ctypes.c_int32), ("N", ctypes.c_int32), ("Ts", ctypes.c_double),
                ("tol", ctypes.c_double), ("max_iter", ctypes.c_int32), ("B_max", ctypes.c_int32),
                ("gravity", ctypes.c_double), ("acceptable_tol", ctypes.c_double),
                ("acceptable_iter", ctypes.c_int32), ("max_soc", ctypes.c_int32), ("pmpc_path", ctypes.c_int32),
                ("restoration", ctypes.c_int32), ("constr_mult_init_max", ctypes.c_double),
                ("max_cpu_time", ctypes.c_double)]


class PlantConfig(ctypes.Structure):
    """Mirror of ``struct dart_plant_config`` (the tray plant of the closed-loop rollouts)."""
    _fields_ = [("tau", ctypes.c_double), ("mu_c", ctypes.c_double), ("v_c", ctypes.c_double)]


class RmpcLoopConfig(ctypes.Structure):
    """Mirror of ``struct dart_rmpc_loop_config`` (governor, staged reference, RLS, episode tolerance)."""
    _fields_ = [("dr_max", ctypes.c_double), ("alpha_rg", ctypes.c_double), ("step_fraction", ctypes.c_double),
                ("rls_lambda", ctypes.c_double), ("pos_tol", ctypes.c_double)]


class RewardConfig(ctypes.Structure):
    """Mirror of ``struct dart_lmpc_reward_config`` (reward, done and record settings of the experience collection)."""
    _fields_ = [("sigma_pos", ctypes.c_double), ("sigma_vel", ctypes.c_double), ("w_pos", ctypes.c_double),
                ("w_vel", ctypes.c_double), ("w_change", ctypes.c_double), ("w_d_ctrl", ctypes.c_double),
                ("success_tol", ctypes.c_double), ("success_bonus", ctypes.c_double), ("oob_penalty", ctypes.c_double),
                ("tray_limit", ctypes.c_double * 2), ("max_per_dim_rms", ctypes.c_double),
                ("time_penalty_rate", ctypes.c_double), ("max_episode_steps", ctypes.c_int32),
                ("record_every", ctypes.c_int32), ("done_sticky", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PpoConfig(ctypes.Structure):
    """Mirror of ``struct dart_lmpc_ppo_config`` (the hyper-parameters of the PPO update on the device)."""
    _fields_ = [("clip_eps", ctypes.c_double), ("vf_coef", ctypes.c_double), ("ent_coef", ctypes.c_double),
                ("max_grad_norm", ctypes.c_double), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("adam_eps", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("log_std_min", ctypes.c_double), ("log_std_max", ctypes.c_double), ("epochs", ctypes.c_int32),
                ("mini_batch_size", ctypes.c_int32)]


HYPER_COLS = 9                  # DART_LMPC_HYPER_COLS: columns of a population's hyper-parameter table
# the table's columns: the first nine doubles of dart_lmpc_ppo_config in the struct's order
HYPER_FIELDS = tuple(f[0] for f in PpoConfig._fields_[:HYPER_COLS])


class PbtConfig(ctypes.Structure):
    """Mirror of ``struct dart_lmpc_pbt_config`` (the exploit/explore step of population-based training)."""
    _fields_ = [("seed", ctypes.c_uint64), ("generation", ctypes.c_int32), ("n_replace", ctypes.c_int32),
                ("higher_is_better", ctypes.c_int32), ("explore_mask", ctypes.c_uint32),
                ("factor_down", ctypes.c_double), ("factor_up", ctypes.c_double),
                ("lo", ctypes.c_double * HYPER_COLS), ("hi", ctypes.c_double * HYPER_COLS)]


class TrainConfig(ctypes.Structure):
    """Mirror of ``struct dart_lmpc_train_config`` (seed, iteration range and GAE settings of the training entry)."""
    _fields_ = [("seed", ctypes.c_uint64), ("iterations", ctypes.c_int32), ("it0", ctypes.c_int32),
                ("steps", ctypes.c_int32), ("mean_update", ctypes.c_int32), ("track_best", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("gamma", ctypes.c_double), ("lam", ctypes.c_double)]


class GlobalBuffer(ctypes.Structure):
    """Mirror of ``struct dart_lmpc_global_buffer`` (the global buffer of the training loop's second update)."""
    _fields_ = [("obs", ctypes.c_void_p), ("action", ctypes.c_void_p), ("logp", ctypes.c_void_p),
                ("value", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p),
                ("capacity", ctypes.c_int32), ("fill", ctypes.c_int32), ("global_log", ctypes.c_void_p),
                ("workspace", ctypes.c_void_p)]


class StackConfig(ctypes.Structure):
    """Mirror of ``struct dart_stack_config`` (the PMPC loop through the dual-arm layer)."""
    _fields_ = [("couple", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7)]


STACK_RIDE, STACK_ACHIEVED = 0, 1               # dart_stack_config.couple
STACK_COMMAND, STACK_COUPLE = 0, 1              # phase of a stack loop-step launch
STACK_METRIC_SLOTS = ("tilt_deviation", "max_tilt_deviation", "max_yaw", "max_grasp_gap", "max_disagreement_angle",
                      "max_tray_pos_error", "held_steps", "steps")
# pointer arguments of the stack entries in the argument order of include/dart_mpc.h ("lm": the LMPC plant's entries)
STACK_STEP_ARGS = {False: ("target", "prm", "tray_pos", "grasp", "snap", "ee_quat", "x", "tilt", "metrics", "stack_metrics",
                           "x0", "tray_cmd", "u0", "f", "status", "iters"),
                   True: ("target", "plant_pvec", "pz_vz", "tray_pos", "grasp", "snap", "ee_quat", "x", "tilt", "metrics",
                          "stack_metrics", "x0", "tray_cmd", "u0", "f", "status", "iters")}
STACK_ROLLOUT_ARGS = {False: ("target", "prm", "x", "tilt", "metrics", "grasp", "models", "plant_models", "arm_prm", "q", "qd",
                              "qdd_prev", "arm_metrics", "work", "tray_pos", "stack_metrics"),
                      True: ("target", "prm", "plant_pvec", "pz_vz", "x", "tilt", "metrics", "grasp", "models", "plant_models",
                             "arm_prm", "q", "qd", "qdd_prev", "arm_metrics", "work", "tray_pos", "stack_metrics")}
STACK_LOGS = (("tilt", 2, np.float64), ("tray", 7, np.float64))
ARM_LOOP_LOGS = ("q", "qd", "tau", "ee_pos", "loss", "status")         # [rows, 2 E, .]; status int32
# the RMPC loop through the dual-arm layer (dart_rmpc_stack_*): pointer arguments in the argument order of
# include/dart_mpc.h, and its stack log group (the command, its quaternion, the achieved tilt and pose)
_RMPC_STACK_STEP = ("tray_pos", "grasp", "snap", "ee_quat", "x", "tilt", "prev", "u_prev", "r_v", "theta", "done", "nlog",
                    "metrics", "stack_metrics", "x0", "Rref", "phi", "y", "tray_cmd", "u0", "f", "status", "iters")
_RMPC_STACK_ROLLOUT = ("x", "tilt", "prev", "u_prev", "r_v", "theta", "P", "w", "done", "nlog", "metrics", "grasp", "models",
                       "plant_models", "arm_prm", "q", "qd", "qdd_prev", "arm_metrics", "work", "tray_pos", "stack_metrics")
RMPC_STACK_STEP_ARGS = {False: ("target", "prm", "mu") + _RMPC_STACK_STEP,
                        True: ("target", "prm", "plant_pvec") + _RMPC_STACK_STEP}
RMPC_STACK_ROLLOUT_ARGS = {False: ("target", "prm", "mu") + _RMPC_STACK_ROLLOUT,
                           True: ("target", "prm", "plant_pvec") + _RMPC_STACK_ROLLOUT}
RMPC_STACK_LOGS = (("U_cmd", 2, np.float64), ("quat_tray", 4, np.float64), ("tilt", 2, np.float64), ("tray", 7, np.float64))


# Arrays of the closed-loop rollouts in the argument order of include/dart_mpc.h: (name, row width, dtype);
# width 0 = one scalar per instance, "nw" = the solver's w.  State arrays are [B, width], logs [rows, B, width].
RMPC_LOOP_STATE = (("x", 6, np.float64), ("tilt", 2, np.float64), ("prev", 4, np.float64), ("u_prev", 2, np.float64),
                   ("r_v", 4, np.float64), ("theta", 14, np.float64), ("P", 98, np.float64), ("w", "nw", np.float64),
                   ("done", 0, np.int32), ("nlog", 0, np.int32))
RMPC_LOOP_IO = (("x0", 4, np.float64), ("Rref", "nref", np.float64), ("phi", 7, np.float64), ("y", 2, np.float64),
                ("u0", 2, np.float64), ("f", 0, np.float64), ("status", 0, np.int32), ("iters", 0, np.int32))
RMPC_LOOP_LOGS = (("pos_err", 2, np.float64), ("pos_err_norm", 0, np.float64), ("u_cmd", 2, np.float64),
                  ("timestep", 0, np.float64), ("x", 4, np.float64), ("theta", 14, np.float64), ("r_v", 4, np.float64),
                  ("f", 0, np.float64), ("status", 0, np.int32), ("iters", 0, np.int32))
PMPC_LOOP_STATE = (("x", 6, np.float64), ("tilt", 2, np.float64))
PMPC_LOOP_IO = (("x0", 6, np.float64), ("u0", 2, np.float64), ("f", 0, np.float64), ("status", 0, np.int32),
                ("iters", 0, np.int32))
PMPC_LOOP_LOGS = (("X", 6, np.float64), ("U_cmd", 2, np.float64), ("quat_tray", 4, np.float64), ("loss", 0, np.float64),
                  ("status", 0, np.int32), ("iters", 0, np.int32))
LMPC_LOOP_STATE = (("x", 8, np.float64), ("tilt", 2, np.float64), ("u_prev", 2, np.float64), ("w", "nw", np.float64),
                   ("obs_mean", 52, np.float64), ("obs_M2", 52, np.float64), ("obs_count", 0, np.int32),
                   ("history", 520, np.float32), ("timestep", 0, np.int32), ("model_params", 34, np.float64))
LMPC_LOOP_IO = (("state", 8, np.float64), ("u0", 2, np.float64), ("f", 0, np.float64), ("status", 0, np.int32),
                ("iters", 0, np.int32))
LMPC_LOOP_LOGS = (("X", 8, np.float64), ("U_cmd", 2, np.float64), ("pos_error", 0, np.float64), ("pvec", 34, np.float64),
                  ("loss", 0, np.float64), ("status", 0, np.int32), ("iters", 0, np.int32))
# cross-plant loops (dart_pmpc_lm_* / dart_rmpc_lm_*): PMPC / RMPC on the LMPC plant, x [B, 8], with streaming metrics
# [B, 8] (METRIC_SLOTS) and the rotation log; the solve's per-step arrays are PMPC_LOOP_IO / RMPC_LOOP_IO
PMPC_LM_LOOP_STATE = (("x", 8, np.float64), ("tilt", 2, np.float64), ("metrics", 8, np.float64))
PMPC_LM_LOOP_LOGS = PMPC_LOOP_LOGS + (("rot", 4, np.float64),)
RMPC_LM_LOOP_STATE = (("x", 8, np.float64),) + RMPC_LOOP_STATE[1:] + (("metrics", 8, np.float64),)
RMPC_LM_LOOP_LOGS = RMPC_LOOP_LOGS + (("rot", 4, np.float64),)
METRIC_SLOTS = ("steady_state_error", "convergence_step", "control_effort", "max_error", "status_nonzero", "iters",
                "max_rotation", "steps")
# LMPC evaluation (dart_lmpc_eval*): the rollout's state plus the streaming metrics [P B, 8] (METRIC_SLOTS), P learners
# of B instances stacked learner-major; the scores [P, 8] reduce a learner's metrics over its instances
LMPC_EVAL_STATE = LMPC_LOOP_STATE + (("metrics", 8, np.float64),)
SCORE_SLOTS = ("mean_steady_state_error", "converged_fraction", "mean_convergence_step", "mean_control_effort",
               "max_error", "status_nonzero", "iters_per_solve", "max_rotation")
# experience collection (dart_lmpc_collect): the collection state [B, width], the reset pool [reset_rows, B, width],
# the per-step logs [rows, B] and the records [rec_rows, B, width]
LMPC_COLLECT_STATE = (("prev_cmd", 2, np.float64), ("control_seen", 2, np.float64), ("ep_step", 0, np.int32),
                      ("ep_return", 0, np.float64), ("time_penalty", 0, np.float64), ("episodes", 0, np.int32),
                      ("last_return", 0, np.float64), ("last_steps", 0, np.int32), ("nrec", 0, np.int32),
                      ("sticky", 0, np.int32))
LMPC_COLLECT_POOL = (("reset_x", 8, np.float64), ("reset_target", 8, np.float64), ("reset_pvec", 34, np.float64))
LMPC_COLLECT_LOGS = (("reward", 0, np.float64), ("done", 0, np.int32), ("value", 0, np.float32), ("logp", 0, np.float32))
LMPC_COLLECT_REC = (("rec_obs", 520, np.float32), ("rec_action", 34, np.float32), ("rec_logp", 0, np.float32),
                    ("rec_value", 0, np.float32), ("rec_reward", 0, np.float64), ("rec_done", 0, np.float32))
DONE_OOB, DONE_MAX_STEPS = 1, 2                 # bits of the done log
CRITIC_NWEIGHTS = 520 * 64 + 64 + 64 * 64 + 64 + 64 + 1
ACTOR_NWEIGHTS = 520 * 64 + 64 + 64 * 64 + 64 + 64 * 34 + 34 + 34
PPO_NPARAMS = ACTOR_NWEIGHTS + CRITIC_NWEIGHTS  # 77317: the actor, then the critic, in the packed order
LOG_INT_FILL = int(np.iinfo(np.int32).min)      # prefill of the int32 logs (the float logs are prefilled with NaN)

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lib = None


def build(verbose: bool = False) -> str:
    """Compile libdartmpc.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-j6", "-C", CSRC_DIR], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise DartMPCError("building libdartmpc.so failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


def source_build_id() -> str:
    """SHA-1 (first 16 hex digits) of the library's sources as the Makefile computes it: the SRC then HDR files."""
    import hashlib
    import re
    mk = open(os.path.join(CSRC_DIR, "Makefile")).read()
    files = []
    for var in ("SRC", "HDR"):
        m = re.search(r"^%s := (.*)$" % var, mk, re.M)
        files += m.group(1).split()
    h = hashlib.sha1()
    for f in files:
        with open(os.path.join(CSRC_DIR, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _check_build(L):
    """Refuse a library that was not built from the sources beside it (unless an A/B run says otherwise)."""
    if not hasattr(L, "dart_mpc_build_id"):
        if os.environ.get("DART_MPC_AB") == "1":
            return
        raise DartMPCError(f"{LIB_PATH} predates the build identity: rebuild it (make -C {CSRC_DIR})")
    L.dart_mpc_build_id.restype = ctypes.c_char_p
    L.dart_mpc_build_flavor.restype = ctypes.c_char_p
    got, want = L.dart_mpc_build_id().decode(), source_build_id()
    flavor = L.dart_mpc_build_flavor().decode()
    if os.path.basename(LIB_PATH) == "libdartmpc.so" and flavor:
        raise DartMPCError(f"{LIB_PATH} is a diagnostic ({flavor}) build, not the product library")
    if got != want and os.environ.get("DART_MPC_AB") != "1":
        raise DartMPCError(f"{LIB_PATH} was built from other sources (build id {got}, sources {want}): "
                           f"stale build, run __graft_entry__.build() or `make -C {CSRC_DIR}`")


def lib():
    """Load the library (no compute).  Raises if it is missing or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DartMPCError(f"{LIB_PATH} not built: run __graft_entry__.build() or `make -C {CSRC_DIR}`")
    # One HIP runtime per process: libamdhip64.so.7 is the SONAME of both the system ROCm runtime and
    # the one torch bundles, and the first one loaded serves both.  torch only works on its own, so
    # load torch first when it is installed (it is the device-memory / stream plumbing of the
    # package); our library then binds to the same runtime.
    # (DART_MPC_NO_TORCH=1: a process that never uses torch -- a controller worker -- skips it)
    if os.environ.get("DART_MPC_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:     # pragma: no cover - the C ABI works without torch
            pass
    L = ctypes.CDLL(LIB_PATH)
    L.dart_mpc_config_default.argtypes = [ctypes.POINTER(Config)]
    L.dart_mpc_config_default.restype = None
    L.dart_mpc_create.argtypes = [ctypes.POINTER(Config), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.dart_mpc_create.restype = ctypes.c_int
    sig = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.dart_mpc_solve_batch.argtypes = sig
    L.dart_mpc_solve_batch.restype = ctypes.c_int
    L.dart_mpc_solve_batch_dev.argtypes = sig
    L.dart_mpc_solve_batch_dev.restype = ctypes.c_int
    L.dart_mpc_sync.argtypes = [ctypes.c_void_p]
    L.dart_mpc_sync.restype = ctypes.c_int
    L.dart_mpc_last_error.argtypes = [ctypes.c_void_p]
    L.dart_mpc_last_error.restype = ctypes.c_char_p
    L.dart_mpc_destroy.argtypes = [ctypes.c_void_p]
    L.dart_mpc_destroy.restype = None
    L.dart_mpc_nw.argtypes = [ctypes.c_int]
    L.dart_mpc_nw.restype = ctypes.c_int
    L.dart_mpc_abi_version.argtypes = []
    L.dart_mpc_abi_version.restype = ctypes.c_int
    rsig = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_double] + [ctypes.c_void_p] * 9
    L.dart_rmpc_solve_batch.argtypes = rsig
    L.dart_rmpc_solve_batch.restype = ctypes.c_int
    L.dart_rmpc_solve_batch_dev.argtypes = rsig
    L.dart_rmpc_solve_batch_dev.restype = ctypes.c_int
    L.dart_rmpc_nw.argtypes = [ctypes.c_int]
    L.dart_rmpc_nw.restype = ctypes.c_int
    lsig = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 12
    L.dart_lmpc_solve_batch.argtypes = lsig
    L.dart_lmpc_solve_batch.restype = ctypes.c_int
    L.dart_lmpc_solve_batch_dev.argtypes = lsig
    L.dart_lmpc_solve_batch_dev.restype = ctypes.c_int
    L.dart_lmpc_nw.argtypes = [ctypes.c_int]
    L.dart_lmpc_nw.restype = ctypes.c_int
    L.dart_lmpc_policy_config_default.argtypes = [ctypes.c_void_p]
    L.dart_lmpc_policy_config_default.restype = None
    L.dart_lmpc_policy_step.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 13
    L.dart_lmpc_policy_step.restype = ctypes.c_int
    L.dart_lmpc_policy_step_dev.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 14
    L.dart_lmpc_policy_step_dev.restype = ctypes.c_int
    psig = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 21
    L.dart_lmpc_policy_solve_batch.argtypes = psig
    L.dart_lmpc_policy_solve_batch.restype = ctypes.c_int
    L.dart_lmpc_policy_solve_batch_dev.argtypes = psig
    L.dart_lmpc_policy_solve_batch_dev.restype = ctypes.c_int
    L.dart_rls_update_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_double]
    L.dart_rls_update_batch.restype = ctypes.c_int
    L.dart_rls_update_batch_dev.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_double, ctypes.c_void_p]
    L.dart_rls_update_batch_dev.restype = ctypes.c_int
    L.dart_arm_config_default.argtypes = [ctypes.c_void_p]
    L.dart_arm_config_default.restype = None
    L.dart_arm_snapshot_len.argtypes = [ctypes.c_int]
    L.dart_arm_snapshot_len.restype = ctypes.c_int
    L.dart_arm_param_len.argtypes = [ctypes.c_int]
    L.dart_arm_param_len.restype = ctypes.c_int
    L.dart_arm_solve_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int] + [ctypes.c_void_p] * 5
    L.dart_arm_solve_batch.restype = ctypes.c_int
    L.dart_arm_solve_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6
    L.dart_arm_solve_batch_dev.restype = ctypes.c_int
    if hasattr(L, "dart_rmpc_rollout_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_plant_config_default.argtypes = [ctypes.POINTER(PlantConfig)]
        L.dart_plant_config_default.restype = None
        L.dart_rmpc_loop_config_default.argtypes = [ctypes.POINTER(RmpcLoopConfig)]
        L.dart_rmpc_loop_config_default.restype = None
        L.dart_rmpc_loop_step_dev.argtypes = [vp, vp, vp] + [ci] * 5 + [vp] * 30
        L.dart_pmpc_loop_step_dev.argtypes = [vp, vp] + [ci] * 5 + [vp] * 15
        for fn in (L.dart_rmpc_rollout_dev, L.dart_rmpc_rollout):
            fn.argtypes = [vp, vp, vp] + [ci] * 4 + [vp] * 24
        for fn in (L.dart_pmpc_rollout_dev, L.dart_pmpc_rollout):
            fn.argtypes = [vp, vp] + [ci] * 4 + [vp] * 11
        for fn in (L.dart_rmpc_loop_step_dev, L.dart_pmpc_loop_step_dev, L.dart_rmpc_rollout_dev,
                   L.dart_pmpc_rollout_dev, L.dart_rmpc_rollout, L.dart_pmpc_rollout):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_rollout_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_lmpc_loop_step_dev.argtypes = [vp, vp] + [ci] * 5 + [vp] * 19
        L.dart_lmpc_loop_step_dev.restype = ctypes.c_int
        for fn in (L.dart_lmpc_rollout_dev, L.dart_lmpc_rollout):
            fn.argtypes = [vp, vp, vp] + [ci] * 4 + [vp] * 24
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_pmpc_lm_rollout_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_pmpc_lm_loop_step_dev.argtypes = [vp, vp] + [ci] * 5 + [vp] * 19
        L.dart_rmpc_lm_loop_step_dev.argtypes = [vp, vp, vp] + [ci] * 5 + [vp] * 32
        for fn in (L.dart_pmpc_lm_rollout_dev, L.dart_pmpc_lm_rollout):
            fn.argtypes = [vp, vp] + [ci] * 4 + [vp] * 15
        for fn in (L.dart_rmpc_lm_rollout_dev, L.dart_rmpc_lm_rollout):
            fn.argtypes = [vp, vp, vp] + [ci] * 4 + [vp] * 26
        for fn in (L.dart_pmpc_lm_loop_step_dev, L.dart_rmpc_lm_loop_step_dev, L.dart_pmpc_lm_rollout_dev,
                   L.dart_pmpc_lm_rollout, L.dart_rmpc_lm_rollout_dev, L.dart_rmpc_lm_rollout):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_eval_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_lmpc_eval_loop_step_dev.argtypes = [vp, vp] + [ci] * 5 + [vp] * 20
        L.dart_lmpc_eval_loop_step_dev.restype = ctypes.c_int
        for fn in (L.dart_lmpc_eval_dev, L.dart_lmpc_eval):
            fn.argtypes = [vp, vp, vp] + [ci] * 5 + [vp] * 26
            fn.restype = ctypes.c_int
        L.dart_lmpc_eval_scores_dev.argtypes = [ci, ci, vp, vp, vp]
        L.dart_lmpc_eval_scores_dev.restype = ctypes.c_int
        L.dart_lmpc_eval_scores.argtypes = [ci, ci, vp, vp]
        L.dart_lmpc_eval_scores.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_collect_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.dart_lmpc_reward_config_default.argtypes = [ctypes.POINTER(RewardConfig)]
        L.dart_lmpc_reward_config_default.restype = None
        L.dart_lmpc_experience_step_dev.argtypes = [vp, vp, vp] + [ci] * 5 + [vp] * 37
        L.dart_lmpc_experience_step_dev.restype = ctypes.c_int
        for fn in (L.dart_lmpc_collect_dev, L.dart_lmpc_collect):
            fn.argtypes = [vp, vp, vp, vp] + [ci] * 6 + [vp] * 48
            fn.restype = ctypes.c_int
        L.dart_lmpc_gae_dev.argtypes = [ci, ci, cd, cd] + [vp] * 8
        L.dart_lmpc_gae_dev.restype = ctypes.c_int
        L.dart_lmpc_gae.argtypes = [ci, ci, cd, cd] + [vp] * 7
        L.dart_lmpc_gae.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_ppo_update_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_lmpc_ppo_config_default.argtypes = [ctypes.POINTER(PpoConfig)]
        L.dart_lmpc_ppo_config_default.restype = None
        L.dart_lmpc_ppo_workspace_bytes.argtypes = [ci, ci]
        L.dart_lmpc_ppo_workspace_bytes.restype = ctypes.c_size_t
        L.dart_lmpc_ppo_update_dev.argtypes = [vp, ci, ci] + [vp] * 17
        L.dart_lmpc_ppo_update.argtypes = [vp, ci, ci] + [vp] * 15
        L.dart_lmpc_ppo_prepare_dev.argtypes = [ci, ci] + [vp] * 7
        L.dart_lmpc_ppo_grad_dev.argtypes = [vp, ci, ci, ci] + [vp] * 11
        L.dart_lmpc_ppo_apply_dev.argtypes = [vp] * 9 + [ci, vp, vp]
        L.dart_lmpc_critic_value_dev.argtypes = [ci, vp, vp, vp, vp]
        L.dart_lmpc_critic_value.argtypes = [ci, vp, vp, vp]
        for fn in (L.dart_lmpc_ppo_update_dev, L.dart_lmpc_ppo_update, L.dart_lmpc_ppo_prepare_dev,
                   L.dart_lmpc_ppo_grad_dev, L.dart_lmpc_ppo_apply_dev, L.dart_lmpc_critic_value_dev,
                   L.dart_lmpc_critic_value):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_train_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
        L.dart_lmpc_philox_dev.argtypes = [ci, vp, vp, vp]
        L.dart_lmpc_noise_dev.argtypes = [u64, ci, ci, ci, vp, vp]
        L.dart_lmpc_noise.argtypes = [u64, ci, ci, ci, vp]
        L.dart_lmpc_perms_dev.argtypes = [u64, ci, ci, ci, vp, vp, vp]
        L.dart_lmpc_perms.argtypes = [u64, ci, ci, ci, vp, vp]
        L.dart_lmpc_mean_param_update_dev.argtypes = [vp, ci] + [vp] * 6
        L.dart_lmpc_mean_param_update.argtypes = [vp, ci] + [vp] * 5
        L.dart_lmpc_train_config_default.argtypes = [ctypes.POINTER(TrainConfig)]
        L.dart_lmpc_train_config_default.restype = None
        L.dart_lmpc_train_workspace_bytes.argtypes = [ci] * 5
        L.dart_lmpc_train_workspace_bytes.restype = ctypes.c_size_t
        for fn in (L.dart_lmpc_train_dev, L.dart_lmpc_train):
            fn.argtypes = [vp] * 6 + [ci, ci, vp, vp]
        for fn in (L.dart_lmpc_philox_dev, L.dart_lmpc_noise_dev, L.dart_lmpc_noise, L.dart_lmpc_perms_dev,
                   L.dart_lmpc_perms, L.dart_lmpc_mean_param_update_dev, L.dart_lmpc_mean_param_update,
                   L.dart_lmpc_train_dev, L.dart_lmpc_train):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_train_global_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci, cd, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
        L.dart_lmpc_choice_dev.argtypes = [u64, ci, ci, ci, vp, vp]
        L.dart_lmpc_choice.argtypes = [u64, ci, ci, ci, vp]
        L.dart_lmpc_perms_stream_dev.argtypes = [u64, ci, ci, ci, ci, vp, vp, vp]
        L.dart_lmpc_global_rows.argtypes = [ci, vp, vp]
        L.dart_lmpc_global_fill_after.argtypes = [ci, ci, ci]
        L.dart_lmpc_global_workspace_bytes.argtypes = [ci, ci, ci]
        L.dart_lmpc_global_workspace_bytes.restype = ctypes.c_size_t
        L.dart_lmpc_global_append_dev.argtypes = [vp, ci, ci, ci] + [vp] * 9
        L.dart_lmpc_global_append.argtypes = [vp, ci, ci, ci] + [vp] * 8
        L.dart_lmpc_gae_seq_dev.argtypes = [ci, cd, cd] + [vp] * 7
        L.dart_lmpc_gae_seq.argtypes = [ci, cd, cd] + [vp] * 6
        for fn in (L.dart_lmpc_train_global_dev, L.dart_lmpc_train_global):
            fn.argtypes = [vp] * 6 + [ci, ci, vp, vp, vp]
        for fn in (L.dart_lmpc_choice_dev, L.dart_lmpc_choice, L.dart_lmpc_perms_stream_dev, L.dart_lmpc_global_rows,
                   L.dart_lmpc_global_fill_after, L.dart_lmpc_global_append_dev, L.dart_lmpc_global_append,
                   L.dart_lmpc_gae_seq_dev, L.dart_lmpc_gae_seq, L.dart_lmpc_train_global_dev,
                   L.dart_lmpc_train_global):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_train_pop_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_lmpc_train_pop_workspace_bytes.argtypes = [ci] * 6
        L.dart_lmpc_train_pop_workspace_bytes.restype = ctypes.c_size_t
        for fn in (L.dart_lmpc_train_pop_dev, L.dart_lmpc_train_pop):
            fn.argtypes = [vp] * 6 + [ci, vp, ci, ci, vp, vp]
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_train_pop_global_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.dart_lmpc_global_pop_workspace_bytes.argtypes = [ci] * 5
        L.dart_lmpc_global_pop_workspace_bytes.restype = ctypes.c_size_t
        L.dart_lmpc_choice_pop_dev.argtypes = [ci, vp, ci, ci, ci, vp, vp]
        L.dart_lmpc_global_append_pop_dev.argtypes = [vp, ci, ci, ci, ci] + [vp] * 9
        L.dart_lmpc_gae_seq_pop_dev.argtypes = [ci, ci, ci, cd, cd] + [vp] * 7
        for fn in (L.dart_lmpc_train_pop_global_dev, L.dart_lmpc_train_pop_global):
            fn.argtypes = [vp] * 6 + [ci, vp, ci, ci, vp, vp, vp]
        for fn in (L.dart_lmpc_choice_pop_dev, L.dart_lmpc_global_append_pop_dev, L.dart_lmpc_gae_seq_pop_dev,
                   L.dart_lmpc_train_pop_global_dev, L.dart_lmpc_train_pop_global):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_lmpc_pbt_step_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        for fn in (L.dart_lmpc_train_pop_hyper_dev, L.dart_lmpc_train_pop_hyper):
            fn.argtypes = [vp] * 6 + [ci, vp, ci, ci, vp, vp, vp, vp]
            fn.restype = ctypes.c_int
        L.dart_lmpc_pbt_config_default.argtypes = [ctypes.POINTER(PbtConfig)]
        L.dart_lmpc_pbt_config_default.restype = None
        L.dart_lmpc_pbt_step_dev.argtypes = [vp, ci, vp, ci] + [vp] * 8
        L.dart_lmpc_pbt_step.argtypes = [vp, ci, vp, ci] + [vp] * 7
        L.dart_lmpc_pbt_step_dev.restype = L.dart_lmpc_pbt_step.restype = ctypes.c_int
    if hasattr(L, "dart_arm_dynamics_batch_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_arm_dyn_config_default.argtypes = [vp]
        L.dart_arm_dyn_config_default.restype = None
        L.dart_arm_model_len.argtypes = [ci]
        L.dart_arm_state_len.argtypes = [ci]
        L.dart_dual_arm_work_len.argtypes = [ci, ci]
        L.dart_arm_dynamics_batch_dev.argtypes = [vp, ci, ci, vp, ci] + [vp] * 4
        L.dart_arm_dynamics_batch.argtypes = [vp, ci, ci, vp, ci] + [vp] * 3
        L.dart_arm_control_batch_dev.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, ci] + [vp] * 7
        L.dart_arm_control_batch.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, ci] + [vp] * 6
        L.dart_dual_arm_control_dev.argtypes = [vp, vp, ci, ci] + [vp] * 7 + [ci] + [vp] * 8
        L.dart_dual_arm_control.argtypes = [vp, vp, ci, ci] + [vp] * 7 + [ci] + [vp] * 7
        L.dart_dual_arm_rollout_dev.argtypes = [vp, vp, ci, ci, ci, ci] + [vp] * 5 + [ci] + [vp] * 12
        L.dart_dual_arm_rollout.argtypes = [vp, vp, ci, ci, ci, ci] + [vp] * 5 + [ci] + [vp] * 10
        for fn in (L.dart_arm_model_len, L.dart_arm_state_len, L.dart_dual_arm_work_len, L.dart_arm_dynamics_batch_dev,
                   L.dart_arm_dynamics_batch, L.dart_arm_control_batch_dev, L.dart_arm_control_batch,
                   L.dart_dual_arm_control_dev, L.dart_dual_arm_control, L.dart_dual_arm_rollout_dev,
                   L.dart_dual_arm_rollout):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_pmpc_stack_rollout_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_stack_config_default.argtypes = [ctypes.POINTER(StackConfig)]
        L.dart_stack_config_default.restype = None
        L.dart_stack_work_len.argtypes = [ci, ci]
        L.dart_tray_from_arms_dev.argtypes = [ci] + [vp] * 7
        L.dart_tray_from_arms.argtypes = [ci] + [vp] * 6
        L.dart_pmpc_stack_loop_step_dev.argtypes = [vp, vp, vp] + [ci] * 7 + [vp] * 25
        L.dart_pmpc_stack_lm_loop_step_dev.argtypes = [vp, vp, vp] + [ci] * 7 + [vp] * 27
        L.dart_pmpc_stack_rollout_dev.argtypes = [vp] * 5 + [ci] * 6 + [vp] * 31
        L.dart_pmpc_stack_lm_rollout_dev.argtypes = [vp] * 5 + [ci] * 6 + [vp] * 34
        L.dart_pmpc_stack_rollout.argtypes = [vp] * 5 + [ci] * 6 + [vp] * 30
        L.dart_pmpc_stack_lm_rollout.argtypes = [vp] * 5 + [ci] * 6 + [vp] * 33
        for fn in (L.dart_stack_work_len, L.dart_tray_from_arms_dev, L.dart_tray_from_arms,
                   L.dart_pmpc_stack_loop_step_dev, L.dart_pmpc_stack_lm_loop_step_dev, L.dart_pmpc_stack_rollout_dev,
                   L.dart_pmpc_stack_lm_rollout_dev, L.dart_pmpc_stack_rollout, L.dart_pmpc_stack_lm_rollout):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_rmpc_stack_rollout_dev"):  # (absent only in older in-tree builds used for A/B timing)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.dart_rmpc_stack_loop_step_dev.argtypes = [vp] * 4 + [ci] * 7 + [vp] * 41
        L.dart_rmpc_stack_lm_loop_step_dev.argtypes = [vp] * 4 + [ci] * 7 + [vp] * 42
        L.dart_rmpc_stack_rollout_dev.argtypes = [vp] * 6 + [ci] * 6 + [vp] * 46
        L.dart_rmpc_stack_lm_rollout_dev.argtypes = [vp] * 6 + [ci] * 6 + [vp] * 47
        L.dart_rmpc_stack_rollout.argtypes = [vp] * 6 + [ci] * 6 + [vp] * 45
        L.dart_rmpc_stack_lm_rollout.argtypes = [vp] * 6 + [ci] * 6 + [vp] * 46
        for fn in (L.dart_rmpc_stack_loop_step_dev, L.dart_rmpc_stack_lm_loop_step_dev, L.dart_rmpc_stack_rollout_dev,
                   L.dart_rmpc_stack_lm_rollout_dev, L.dart_rmpc_stack_rollout, L.dart_rmpc_stack_lm_rollout):
            fn.restype = ctypes.c_int
    if hasattr(L, "dart_mpc_bind"):        # (absent only in older in-tree builds used for A/B timing)
        L.dart_mpc_bind.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 9
        L.dart_mpc_bind.restype = ctypes.c_int
        L.dart_mpc_solve_bound.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.dart_mpc_solve_bound.restype = ctypes.c_int
    if hasattr(L, "dart_mpc_serve_start"):  # (absent only in older in-tree builds used for A/B timing)
        L.dart_mpc_serve_start.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        L.dart_mpc_serve_start.restype = ctypes.c_int
        L.dart_mpc_serve_stop.argtypes = [ctypes.c_void_p]
        L.dart_mpc_serve_stop.restype = ctypes.c_int
        L.dart_mpc_serve_running.argtypes = [ctypes.c_void_p]
        L.dart_mpc_serve_running.restype = ctypes.c_int
    if hasattr(L, "dart_set_device"):       # (absent only in older in-tree builds used for A/B timing)
        L.dart_set_device.argtypes = [ctypes.c_int]
        L.dart_set_device.restype = ctypes.c_int
    if L.dart_mpc_abi_version() != ABI_VERSION:
        raise DartMPCError("libdartmpc.so ABI version mismatch")
    _check_build(L)
    _lib = L
    return L


def set_device(device: int):
    """Select the device of the stateless entries (RLS, policy step, arm QP) for this thread."""
    rc = lib().dart_set_device(int(device))
    if rc != 0:
        raise DartMPCError(f"dart_set_device({device}) failed ({rc})")


def wave_selftest():
    """Run the internal wave-primitive self-test kernel (DPP shifts and reductions) on device 0."""
    L = lib()
    L.dartmpc_selftest.argtypes = [ctypes.c_void_p]
    L.dartmpc_selftest.restype = ctypes.c_int
    out = np.zeros(265)
    rc = L.dartmpc_selftest(ctypes.c_void_p(out.ctypes.data))
    if rc != 0:
        raise DartMPCError(f"dartmpc_selftest failed ({rc})")
    return out


# -- device probes of csrc/wave.h and csrc/ocp_wave.h (csrc/wave_probe.hip; internal like dartmpc_selftest) --------
PROBE_MATH_FN = {"frcp": 0, "rcp_raw": 1, "lg2": 2, "log_fast": 3, "exp_econ": 4, "tanh_econ": 5, "sincos_small": 6,
                 "cos_small": 7, "sincos_econ": 8, "cos_econ": 9, "tilt_sincos": 10, "tilt_cos": 11,
                 "tilt_sincos_econ": 12, "tilt_cos_econ": 13}


def _probe_entry(name, waves):
    if waves not in (1, 2):
        raise DartMPCError(f"probe builds have one or two waves per instance, not {waves}")
    fn = getattr(lib(), f"{name}_wg{waves}")
    fn.restype = ctypes.c_int
    return fn


def probe_layout(waves=1):
    """Sizes compiled into the probes of the ``waves``-wave build (no GPU needed): threads, result rows of the
    primitive probe, doubles of the node-array images and the node slots of both engine forms, LDS struct bytes."""
    o = np.zeros(10, np.int32)
    fn = _probe_entry("dartmpc_probe_layout", waves)
    fn.restype = None
    fn(_ptr(o))
    keys = ("threads", "prim_slots", "aug_M", "aug_G", "s_M", "s_G", "aug_nmaxs", "s_nmaxs", "aug_bytes", "s_bytes")
    return dict(zip(keys, (int(v) for v in o)))


def probe_math(name, x, poly=True):
    """``name`` of wave.h (PROBE_MATH_FN) applied elementwise to ``x`` on device 0: (first, second) results as
    float64 arrays (second: the cosine of the sincos forms, else zeros)."""
    x = np.ascontiguousarray(x, np.float64).ravel()
    o0, o1 = np.empty_like(x), np.empty_like(x)
    L = lib()
    L.dartmpc_probe_math.restype = ctypes.c_int
    rc = L.dartmpc_probe_math(ctypes.c_int(PROBE_MATH_FN[name]), ctypes.c_int(int(bool(poly))), ctypes.c_int(x.size),
                              _ptr(x), _ptr(o0), _ptr(o1))
    if rc != 0:
        raise DartMPCError(f"dartmpc_probe_math({name}) failed ({rc})")
    return o0, o1


def probe_prims(d, f, p, waves=1):
    """Every wave primitive on one instance of the ``waves``-wave build: d [8, T] float64, f [8, T] float32,
    p [T] predicate -> [rows, T] float64 (T = 64 waves; the rows as numbered in csrc/wave_probe.hip)."""
    lay = probe_layout(waves)
    T = lay["threads"]
    d = np.ascontiguousarray(d, np.float64)
    f = np.ascontiguousarray(f, np.float32)
    p = np.ascontiguousarray(p, np.int32)
    if d.shape != (8, T) or f.shape != (8, T) or p.shape != (T,):
        raise DartMPCError(f"probe_prims takes [8, {T}] doubles, [8, {T}] floats and [{T}] predicates")
    out = np.zeros((lay["prim_slots"], T))
    rc = _probe_entry("dartmpc_probe_prims", waves)(_ptr(d), _ptr(f), _ptr(p), _ptr(out))
    if rc != 0:
        raise DartMPCError(f"dartmpc_probe_prims failed ({rc})")
    return out


def probe_riccati(form, N, M, H, G, dx0, waves=1):
    """The Riccati engine of csrc/ocp_wave.h on one instance: ``form`` "aug" (OcpLds<6>: sweep_aug), "s" or "sp"
    (OcpLdsS<5>, two subsystems: riccati_s_sweep / riccati_s_sweep_p).  M, H, G: the images of the node arrays
    (NodeArr strides, sizes of ``probe_layout``); dx0 [6] or [2, 5].  Returns dict(G, dx, du, lam, ok)."""
    lay = probe_layout(waves)
    aug = form == "aug"
    if form not in ("aug", "s", "sp"):
        raise DartMPCError(f"unknown engine form {form!r}")
    msz, gsz = (lay["aug_M"], lay["aug_G"]) if aug else (lay["s_M"], lay["s_G"])
    nmaxs = lay["aug_nmaxs"] if aug else lay["s_nmaxs"]
    nxa, nu, slots = (6, 2, nmaxs) if aug else (5, 1, 2 * nmaxs)
    M, H, G = (np.ascontiguousarray(a, np.float64).ravel() for a in (M, H, G))
    dx0 = np.ascontiguousarray(dx0, np.float64).ravel()
    if M.size != msz or H.size != gsz or G.size != gsz or dx0.size != (6 if aug else 10) or not 1 <= N < nmaxs:
        raise DartMPCError("probe_riccati: array sizes or N do not match the build's layout")
    Go, dx, du, lam = np.zeros(gsz), np.zeros((slots, nxa)), np.zeros((slots, nu)), np.zeros((slots, nxa))
    ok = np.zeros(lay["threads"], np.int32)
    if aug:
        rc = _probe_entry("dartmpc_probe_riccati_aug", waves)(ctypes.c_int(N), _ptr(M), _ptr(H), _ptr(G), _ptr(dx0),
                                                              _ptr(Go), _ptr(dx), _ptr(du), _ptr(lam), _ptr(ok))
    else:
        rc = _probe_entry("dartmpc_probe_riccati_s", waves)(ctypes.c_int(int(form == "sp")), ctypes.c_int(N), _ptr(M),
                                                            _ptr(H), _ptr(G), _ptr(dx0), _ptr(Go), _ptr(dx), _ptr(du),
                                                            _ptr(lam), _ptr(ok))
    if rc != 0:
        raise DartMPCError(f"dartmpc_probe_riccati({form}) failed ({rc})")
    return dict(G=Go, dx=dx, du=du, lam=lam, ok=ok)


def default_config(**over) -> Config:
    c = Config()
    lib().dart_mpc_config_default(ctypes.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _set_fields(c, over):
    names = [f[0] for f in c._fields_]
    for k, v in over.items():
        if k not in names:
            raise DartMPCError(f"{type(c).__name__} has no field {k!r} (fields: {names})")
        setattr(c, k, float(v))
    return c


def plant_config(**over) -> PlantConfig:
    """``dart_plant_config`` with the library's defaults (harness.TrayPlant's), fields overridden by keyword."""
    c = PlantConfig()
    lib().dart_plant_config_default(ctypes.byref(c))
    return _set_fields(c, over)


def rmpc_loop_config(**over) -> RmpcLoopConfig:
    """``dart_rmpc_loop_config`` with the library's defaults (harness.run_rmpc's), fields overridden by keyword."""
    c = RmpcLoopConfig()
    lib().dart_rmpc_loop_config_default(ctypes.byref(c))
    return _set_fields(c, over)


def stack_config(couple=STACK_ACHIEVED) -> StackConfig:
    """``dart_stack_config`` with the library's defaults; ``couple``: STACK_RIDE / STACK_ACHIEVED or "ride" / "achieved"."""
    c = StackConfig()
    lib().dart_stack_config_default(ctypes.byref(c))
    c.couple = {"ride": STACK_RIDE, "achieved": STACK_ACHIEVED}.get(couple, couple)
    return c


def _any_ptr(v):
    """A pointer argument from None, a device pointer (int) or a numpy array."""
    if v is None:
        return None
    return ctypes.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else ctypes.c_void_p(int(v))


def _loop_shape(B, width, **sizes):
    width = sizes[width] if isinstance(width, str) else width
    return (B, width) if width else (B,)


def loop_logs(spec, rows, B):
    """Host log arrays of a rollout, [rows, B, width] each: NaN (float) / LOG_INT_FILL (int32) prefilled."""
    return {name: np.full((rows,) + _loop_shape(B, width), np.nan if np.issubdtype(dt, np.floating) else LOG_INT_FILL, dt)
            for name, width, dt in spec}


def loop_metrics(B):
    """The metrics of a fresh cross-plant run, [B, 8] (METRIC_SLOTS): zeros, slot 1 (the convergence step) -1."""
    m = np.zeros((B, 8))
    m[:, 1] = -1.0
    return m


def _dev_ptrs(spec, arrays):
    """Device pointers (ints) of ``arrays`` (a mapping name -> int) in the order of ``spec``; ``arrays`` None: null
    pointers (the metrics-only mode of the cross-plant entries)."""
    if arrays is None:
        return [None] * len(spec)
    return [ctypes.c_void_p(int(arrays[name])) for name, _, _ in spec]


def _host_ptrs(spec, arrays, lead, **sizes):
    """Pointers of the numpy arrays of ``arrays`` in the order of ``spec``, shapes and dtypes checked."""
    if arrays is None:          # (the metrics-only mode of the cross-plant entries)
        return [None] * len(spec)
    out = []
    for name, width, dt in spec:
        a = arrays[name]
        shape = tuple(lead[:-1]) + _loop_shape(lead[-1], width, **sizes)
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
            raise DartMPCError(f"rollout array {name!r} must be a C-contiguous {np.dtype(dt).name} array of shape {shape}")
        out.append(_ptr(a))
    return out


# Handles still open at interpreter exit are destroyed by an atexit hook, before the HIP runtime's own teardown:
# a handle freed later, from a finaliser, would free device memory through a runtime that is already gone.
_LIVE = weakref.WeakSet()


@atexit.register
def _close_live_handles():
    for s in list(_LIVE):
        try:
            s.close()
        except Exception:
            pass


class Solver:
    """Owns one ``dart_mpc_handle`` (device workspace + stream) for a fixed N/Ts/tol.  ``max_soc`` is
    IPOPT's second-order-correction count (default 4, as ``mpc_3d.py:82`` leaves it; 0 = off).
    ``path``: "ipopt" (default) follows IPOPT's iterates on the full 6-state NLP; "reduced" is the
    faster opt-in that solves the (x, y) problem and rolls z out afterwards (same KKT point).
    ``restoration``: IPOPT's soft restoration and restoration phases after a failed filter line search
    (IPOPT's path, N <= 31; pmpc_resto.hip); off, or on the reduced path or beyond N = 31, such an instance
    ends at status -2."""

    PATHS = {"ipopt": 0, "reduced": 1}

    def __init__(self, N=20, Ts=0.002, tol=1e-8, max_iter=3000, B_max=1024, device=0, gravity=-9.81, max_soc=4,
                 path="ipopt", constr_mult_init_max=1000.0, restoration=True):
        self._h = ctypes.c_void_p()
        if path not in self.PATHS:
            raise DartMPCError(f"unknown PMPC path {path!r} (expected one of {sorted(self.PATHS)})")
        self.cfg = default_config(N=int(N), Ts=float(Ts), tol=float(tol), max_iter=int(max_iter), B_max=int(B_max),
                                  gravity=float(gravity), max_soc=int(max_soc), pmpc_path=self.PATHS[path],
                                  constr_mult_init_max=float(constr_mult_init_max),
                                  restoration=int(bool(restoration)))
        rc = lib().dart_mpc_create(ctypes.byref(self.cfg), int(device), ctypes.byref(self._h))
        _LIVE.add(self)
        if rc != 0:
            raise DartMPCError(f"dart_mpc_create failed with code {rc} (no gfx950 device or bad config)")
        self.N = int(N)
        self.nw = lib().dart_mpc_nw(self.N)

    def _err(self, rc, what):
        msg = lib().dart_mpc_last_error(self._h)
        raise DartMPCError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def solve_batch(self, x0, ref, prm, w_warm=None, want_w=False, out=None):
        """Host arrays in, host arrays out (blocking).  Returns dict(u0, f, w, status, iters).
        ``out``: a dict of preallocated u0[B,2], f[B], status[B] (int32), iters[B] (int32) and, with
        want_w, w[B,nw] arrays that are filled and returned instead of fresh ones."""
        x0 = np.ascontiguousarray(x0, np.float64).reshape(-1, 6)
        B = x0.shape[0]
        if out is not None:
            self._check_out(out, B, want_w)
        if w_warm is None and not want_w and B > 0:
            return self._solve_staged(B, x0, ref, prm, out)
        ref = np.ascontiguousarray(ref, np.float64).reshape(B, 6)
        prm = np.ascontiguousarray(prm, np.float64).reshape(B, 6)
        ww = None if w_warm is None else np.ascontiguousarray(w_warm, np.float64).reshape(B, self.nw)
        if out is not None:
            u0, f, st, it = out["u0"], out["f"], out["status"], out["iters"]
            w = out.get("w") if want_w else None
        else:
            u0 = np.empty((B, 2)); f = np.empty(B)
            w = np.empty((B, self.nw)) if want_w else None
            st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        rc = lib().dart_mpc_solve_batch(self._h, B, _ptr(x0), _ptr(ref), _ptr(prm), _ptr(ww), _ptr(u0), _ptr(f),
                                        _ptr(w), _ptr(st), _ptr(it), None)
        if rc != 0:
            self._err(rc, "dart_mpc_solve_batch")
        return dict(u0=u0, f=f, w=w, status=st, iters=it)

    def _check_out(self, out, B, want_w):
        """out= arrays: shapes of the batch, float64 u0 / f (/ w), int32 status / iters, C-contiguous."""
        u0, f, st, it = out["u0"], out["f"], out["status"], out["iters"]
        if (u0.shape != (B, 2) or f.shape != (B,) or st.shape != (B,) or it.shape != (B,) or u0.dtype != np.float64
                or f.dtype != np.float64 or st.dtype != np.int32 or it.dtype != np.int32
                or not all(a.flags.c_contiguous for a in (u0, f, st, it))):
            raise DartMPCError("out= arrays do not match the batch")
        if want_w:
            w = out.get("w")
            if w is None or w.shape != (B, self.nw) or w.dtype != np.float64 or not w.flags.c_contiguous:
                raise DartMPCError("out['w'] must be a C-contiguous float64 [B, nw] array when want_w")

    def _solve_staged(self, B, x0, ref, prm, out):
        """Cold-start call without w: inputs copied into per-batch-size buffers whose pointers are
        cached (building ctypes pointers costs ~1 us each, a third of the Python side of a call)."""
        cache = self.__dict__.setdefault("_staged", {})
        st_ = cache.get(B)
        if st_ is None:
            if len(cache) >= 8:
                cache.clear()
            bufs = (np.empty((B, 6)), np.empty((B, 6)), np.empty((B, 6)), np.empty((B, 2)), np.empty(B),
                    np.empty(B, np.int32), np.empty(B, np.int32))
            st_ = cache[B] = (bufs, tuple(b.ctypes.data for b in bufs), threading.Lock())
        (bx, br, bp, bu, bf, bs, bi), (px, pr, pp, pu, pf, ps, pi), lock = st_
        with lock:
            np.copyto(bx, x0)
            np.copyto(br, np.reshape(ref, (B, 6)))
            np.copyto(bp, np.reshape(prm, (B, 6)))
            rc = lib().dart_mpc_solve_batch(self._h, B, px, pr, pp, None, pu, pf, None, ps, pi, None)
            if rc != 0:
                self._err(rc, "dart_mpc_solve_batch")
            if out is not None:
                for k, src in (("u0", bu), ("f", bf), ("status", bs), ("iters", bi)):
                    np.copyto(out[k], src)
                return dict(u0=out["u0"], f=out["f"], w=None, status=out["status"], iters=out["iters"])
            return dict(u0=bu.copy(), f=bf.copy(), w=None, status=bs.copy(), iters=bi.copy())

    def solve_one(self, x0, ref, prm, want_w=False):
        """One instance (the per-control-step call of PMPC.solve / mpc_worker): the rows are copied
        into buffers allocated once, whose pointers are cached, so the Python side of a call is a few
        slice copies and one ctypes call.  Returns (u0[2], f, status, iters, w or None); the arrays
        are fresh copies."""
        one = getattr(self, "_one", None)
        if one is None:
            bufs = [np.empty(6), np.empty(6), np.empty(6), np.empty(2), np.empty(1), np.empty(self.nw),
                    np.empty(1, np.int32), np.empty(1, np.int32)]
            one = self._one = (threading.Lock(), bufs, [_ptr(b) for b in bufs])
        lock, (bx, br, bp, bu, bf, bw, bs, bi), ptrs = one
        with lock:
            bx[:] = x0; br[:] = ref; bp[:] = prm
            rc = lib().dart_mpc_solve_batch(self._h, 1, ptrs[0], ptrs[1], ptrs[2], None, ptrs[3], ptrs[4],
                                            ptrs[5] if want_w else None, ptrs[6], ptrs[7], None)
            if rc != 0:
                self._err(rc, "dart_mpc_solve_batch")
            return bu.copy(), float(bf[0]), int(bs[0]), int(bi[0]), (bw.copy() if want_w else None)

    def solve_batch_dev(self, B, x0, ref, prm, u0, f, status, iters, w_warm=0, w_out=0, stream=0):
        """Device pointers (ints) in/out, asynchronous on ``stream`` (an int hipStream_t, 0 = own)."""
        rc = lib().dart_mpc_solve_batch_dev(self._h, int(B), x0, ref, prm, w_warm or None, u0, f, w_out or None,
                                            status, iters, stream or None)
        if rc != 0:
            self._err(rc, "dart_mpc_solve_batch_dev")

    # -- device-resident closed loops: every dart_{pmpc,rmpc}[_lm]_{loop_step_dev,rollout_dev,rollout} entry goes
    # through these two
    def _loop_dev(self, entry, cfgs, dims, lead, specs, stream):
        """A device loop-step or rollout entry: the config structs, the int dimensions, the leading device pointers,
        then the pointers of every (spec, mapping) of ``specs``."""
        rc = getattr(lib(), entry)(self._h, *map(ctypes.byref, cfgs), *map(int, dims), *lead,
                                   *[q for spec, arrays in specs for q in _dev_ptrs(spec, arrays)], stream or None)
        if rc != 0:
            self._err(rc, entry)

    def _loop_host(self, entry, cfgs, k0, steps, rows, lead, state_spec, state, logs_spec, logs, **sizes):
        """A host rollout entry: ``lead`` is the (array, width) pairs of the leading inputs, [B, width] each."""
        B = state["x"].shape[0]
        lead = [np.ascontiguousarray(a, np.float64).reshape(_loop_shape(B, width)) for a, width in lead]
        rc = getattr(lib(), entry)(self._h, *map(ctypes.byref, cfgs), B, int(k0), int(steps), rows, *map(_ptr, lead),
                                   *_host_ptrs(state_spec, state, (B,), **sizes),
                                   *_host_ptrs(logs_spec, logs, (rows, B)), None)
        if rc != 0:
            self._err(rc, entry)

    # -- dart_pmpc_loop_step_dev / dart_pmpc_rollout_dev / dart_pmpc_rollout ----
    def loop_step_dev(self, B, k, do_post, do_pre, log_rows, prm, state, io, logs, plant=None, stream=0):
        """One loop-step launch: post(k) and / or the next step's pre.  ``state`` / ``io`` / ``logs`` map the names
        of PMPC_LOOP_STATE / PMPC_LOOP_IO / PMPC_LOOP_LOGS to device pointers (ints).  Asynchronous."""
        self._loop_dev("dart_pmpc_loop_step_dev", (plant or plant_config(),), (B, k, do_post, do_pre, log_rows), (prm,),
                       ((PMPC_LOOP_STATE, state), (PMPC_LOOP_IO, io), (PMPC_LOOP_LOGS, logs)), stream)

    def rollout_dev(self, B, k0, steps, log_rows, target, prm, state, logs, plant=None, stream=0):
        """``steps`` closed-loop steps from step ``k0`` on the device, no host synchronisation in between
        (device pointers as in ``loop_step_dev``; asynchronous on ``stream``)."""
        self._loop_dev("dart_pmpc_rollout_dev", (plant or plant_config(),), (B, k0, steps, log_rows), (target, prm),
                       ((PMPC_LOOP_STATE, state), (PMPC_LOOP_LOGS, logs)), stream)

    def rollout(self, k0, steps, target, prm, state, logs, plant=None):
        """Host arrays (blocking): ``state`` (PMPC_LOOP_STATE) is advanced and ``logs`` (``loop_logs``) rows
        k0 .. k0+steps-1 are filled in place."""
        self._loop_host("dart_pmpc_rollout", (plant or plant_config(),), k0, steps, logs["X"].shape[0],
                        ((target, 6), (prm, 6)), PMPC_LOOP_STATE, state, PMPC_LOOP_LOGS, logs)

    # -- the same loop on the LMPC plant (dart_pmpc_lm_loop_step_dev / dart_pmpc_lm_rollout_dev / dart_pmpc_lm_rollout) ----
    def loop_step_lm_dev(self, B, k, do_post, do_pre, log_rows, target, plant_pvec, pz_vz, state, io, logs, plant=None,
                         stream=0):
        """``loop_step_dev`` on the LMPC plant: ``state`` maps PMPC_LM_LOOP_STATE, ``logs`` PMPC_LM_LOOP_LOGS (None:
        metrics-only) to device pointers."""
        self._loop_dev("dart_pmpc_lm_loop_step_dev", (plant or plant_config(),), (B, k, do_post, do_pre, log_rows),
                       (target, plant_pvec, pz_vz),
                       ((PMPC_LM_LOOP_STATE, state), (PMPC_LOOP_IO, io), (PMPC_LM_LOOP_LOGS, logs)), stream)

    def rollout_lm_dev(self, B, k0, steps, log_rows, target, prm, plant_pvec, pz_vz, state, logs, plant=None, stream=0):
        """``rollout_dev`` on the LMPC plant with the true parameters ``plant_pvec`` [B, 34]: ``state`` maps
        PMPC_LM_LOOP_STATE (x [B, 8], tilt, metrics [B, 8], see ``loop_metrics``), ``logs`` PMPC_LM_LOOP_LOGS to device
        pointers; ``logs`` None is the metrics-only mode (no log row is written)."""
        self._loop_dev("dart_pmpc_lm_rollout_dev", (plant or plant_config(),), (B, k0, steps, log_rows),
                       (target, prm, plant_pvec, pz_vz), ((PMPC_LM_LOOP_STATE, state), (PMPC_LM_LOOP_LOGS, logs)), stream)

    def rollout_lm(self, k0, steps, target, prm, plant_pvec, pz_vz, state, logs, plant=None):
        """Host arrays (blocking): ``state`` (PMPC_LM_LOOP_STATE) is advanced and ``logs`` (``loop_logs`` of
        PMPC_LM_LOOP_LOGS) rows k0 .. k0+steps-1 are filled in place; ``logs`` None moves no log."""
        self._loop_host("dart_pmpc_lm_rollout", (plant or plant_config(),), k0, steps,
                        logs["X"].shape[0] if logs is not None else 0,
                        ((target, 6), (prm, 6), (plant_pvec, 34), (pz_vz, 2)), PMPC_LM_LOOP_STATE, state,
                        PMPC_LM_LOOP_LOGS, logs)

    # -- the loop through the dual-arm layer (dart_pmpc_stack[_lm]_loop_step_dev / _rollout_dev / _rollout) ----
    def _stack_logs(self, lm, logs, stack_logs, arm_logs=False):
        spec = PMPC_LM_LOOP_LOGS if lm else PMPC_LOOP_LOGS
        out = [_any_ptr(logs[name]) if logs is not None else None for name, _, _ in spec]
        out += [_any_ptr(stack_logs[name]) if stack_logs is not None else None for name, _, _ in STACK_LOGS]
        if arm_logs is not False:
            out += [_any_ptr(arm_logs[name]) if arm_logs is not None else None for name in ARM_LOOP_LOGS]
        return out

    def stack_loop_step_dev(self, E, n, k, phase, do_post, do_pre, log_rows, arrays, logs=None, stack_logs=None,
                            plant=None, scfg=None, lm=False, stream=0):
        """One launch of the loop through the arms: ``phase`` STACK_COMMAND (tray_cmd from u0 and tray_pos) or
        STACK_COUPLE (couple + post(k) and / or pre).  ``arrays`` maps the names of STACK_STEP_ARGS[lm] to device
        pointers (absent: null); ``logs`` (PMPC_[LM_]LOOP_LOGS) and ``stack_logs`` (STACK_LOGS) likewise, or None."""
        entry = "dart_pmpc_stack_lm_loop_step_dev" if lm else "dart_pmpc_stack_loop_step_dev"
        rc = getattr(lib(), entry)(self._h, ctypes.byref(plant or plant_config()), ctypes.byref(scfg or stack_config()),
                                   int(E), int(n), int(k), int(phase), int(do_post), int(do_pre), int(log_rows),
                                   *[_any_ptr(arrays.get(a)) for a in STACK_STEP_ARGS[bool(lm)]],
                                   *self._stack_logs(lm, logs, stack_logs), stream or None)
        if rc != 0:
            self._err(rc, entry)

    def _stack_rollout(self, entry, host, E, n, k0, steps, log_rows, arm_prm_stride, arrays, logs, stack_logs, arm_logs,
                       plant, scfg, dcfg, qcfg, lm, stream):
        from .arm import arm_config, arm_dyn_config
        names = [a for a in STACK_ROLLOUT_ARGS[bool(lm)] if not (host and a == "work")]
        rc = getattr(lib(), entry)(self._h, ctypes.byref(plant or plant_config()), ctypes.byref(scfg or stack_config()),
                                   ctypes.byref(dcfg or arm_dyn_config()), ctypes.byref(qcfg or arm_config()),
                                   int(E), int(n), int(k0), int(steps), int(log_rows), int(arm_prm_stride),
                                   *[_any_ptr(arrays.get(a)) for a in names],
                                   *self._stack_logs(lm, logs, stack_logs, arm_logs), stream or None)
        if rc != 0:
            self._err(rc, entry)

    def stack_rollout_dev(self, E, n, k0, steps, log_rows, arm_prm_stride, arrays, logs=None, stack_logs=None,
                          arm_logs=None, plant=None, scfg=None, dcfg=None, qcfg=None, lm=False, stream=0):
        """``steps`` steps of the loop through the arms from step ``k0`` on the device, asynchronous on ``stream``:
        ``arrays`` maps STACK_ROLLOUT_ARGS[lm] to device pointers; the three log groups are mappings or None."""
        self._stack_rollout("dart_pmpc_stack_lm_rollout_dev" if lm else "dart_pmpc_stack_rollout_dev", False, E, n, k0,
                            steps, log_rows, arm_prm_stride, arrays, logs, stack_logs, arm_logs, plant, scfg, dcfg, qcfg,
                            lm, stream)

    def stack_rollout(self, E, n, k0, steps, log_rows, arm_prm_stride, arrays, logs=None, stack_logs=None, arm_logs=None,
                      plant=None, scfg=None, dcfg=None, qcfg=None, lm=False):
        """The same on host arrays (C-contiguous numpy, no ``work``; blocking): state and metrics are advanced and the
        rows k0 .. k0+steps-1 of the logs given are filled in place."""
        for name, a in list(arrays.items()) + [kv for g in (logs, stack_logs, arm_logs) if g for kv in g.items()]:
            if a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous):
                raise DartMPCError(f"stack rollout array {name!r} must be a C-contiguous numpy array")
        self._stack_rollout("dart_pmpc_stack_lm_rollout" if lm else "dart_pmpc_stack_rollout", True, E, n, k0, steps,
                            log_rows, arm_prm_stride, arrays, logs, stack_logs, arm_logs, plant, scfg, dcfg, qcfg, lm, 0)

    def sync(self):
        rc = lib().dart_mpc_sync(self._h)
        if rc != 0:
            self._err(rc, "dart_mpc_sync")

    # -- resident solver (PMPC, IPOPT's path, N <= 31): dart_mpc_serve_start / _stop / _running ----
    def serve_start(self, B_serve=18, idle_timeout=1.0):
        """Keep a grid of ``B_serve`` waves resident; later ``solve_batch`` / ``solve_one`` calls with
        B <= B_serve are served without a kernel launch (bit-identical results)."""
        rc = lib().dart_mpc_serve_start(self._h, int(B_serve), float(idle_timeout))
        if rc != 0:
            self._err(rc, "dart_mpc_serve_start")
        return self

    def serve_stop(self):
        rc = lib().dart_mpc_serve_stop(self._h)
        if rc != 0:
            self._err(rc, "dart_mpc_serve_stop")

    def serving(self):
        return bool(lib().dart_mpc_serve_running(self._h))

    def bind(self):
        """In-place I/O (dart_mpc_bind): a ``Bound`` whose numpy views live in the handle's mapped, pinned
        I/O area.  Write the inputs of the first B rows, call ``bound.solve(B)``, read the outputs: no
        copies and a two-argument ctypes call per solve."""
        b = getattr(self, "_bound", None)
        if b is None:
            b = self._bound = Bound(self)
        return b

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._h:
            lib().dart_mpc_destroy(self._h)      # stops a resident grid first
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bound:
    """Views of a PMPC handle's in-place I/O area for B_max instances (Solver.bind)."""

    def __init__(self, solver):
        ptrs = [ctypes.c_void_p() for _ in range(9)]
        rc = lib().dart_mpc_bind(solver._h, *[ctypes.byref(p) for p in ptrs])
        if rc != 0:
            solver._err(rc, "dart_mpc_bind")
        Bm, nw = int(solver.cfg.B_max), solver.nw

        def view(p, shape, ct):
            n = int(np.prod(shape))
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(n,)).reshape(shape)

        d = ctypes.c_double
        self.x0, self.ref, self.prm = view(ptrs[0], (Bm, 6), d), view(ptrs[1], (Bm, 6), d), view(ptrs[2], (Bm, 6), d)
        self.w_warm = view(ptrs[3], (Bm, nw), d)
        self.u0, self.f, self.w_out = view(ptrs[4], (Bm, 2), d), view(ptrs[5], (Bm,), d), view(ptrs[6], (Bm, nw), d)
        self.status, self.iters = view(ptrs[7], (Bm,), ctypes.c_int32), view(ptrs[8], (Bm,), ctypes.c_int32)
        self._solver = solver
        self._fn = lib().dart_mpc_solve_bound
        self._h = solver._h

    def solve(self, B, w_warm=False, want_w=False):
        rc = self._fn(self._h, B, (1 if w_warm else 0) | (2 if want_w else 0))
        if rc != 0:
            self._solver._err(rc, "dart_mpc_solve_bound")


class RmpcSolver(Solver):
    """``dart_mpc_handle`` of variant RMPC (regressor NMPC + fused RLS), N <= 63 (N > 31: the two-wave build).  Defaults are the
    reference's options (np_mpc...:158-162: max_iter 200) and IPOPT's: constr_mult_init_max 1000, its soft
    restoration / restoration phases after a failed line search (restoration=False: status -2 there; a measured
    |v| above vmax at the pinned node 0 ends at status 2 with them) and max_soc 4 in the restoration phase."""

    def __init__(self, N=20, Ts=0.002, tol=1e-8, max_iter=200, B_max=1024, device=0, gravity=-9.81,
                 constr_mult_init_max=1000.0, restoration=True, max_soc=4):
        self._h = ctypes.c_void_p()
        self.cfg = default_config(variant=VARIANT_RMPC, N=int(N), Ts=float(Ts), tol=float(tol),
                                  max_iter=int(max_iter), B_max=int(B_max), gravity=float(gravity),
                                  constr_mult_init_max=float(constr_mult_init_max),
                                  restoration=int(bool(restoration)), max_soc=int(max_soc))
        rc = lib().dart_mpc_create(ctypes.byref(self.cfg), int(device), ctypes.byref(self._h))
        _LIVE.add(self)
        if rc != 0:
            raise DartMPCError(f"dart_mpc_create(RMPC) failed with code {rc} (no gfx950 device or bad config)")
        self.N = int(N)
        self.nw = lib().dart_rmpc_nw(self.N)

    def solve_batch(self, x0, u_prev, theta, Rref, prm, w_warm=None, want_w=False, rls_P=None, rls_phi=None,
                    rls_y=None, rls_lambda=0.995):
        """Host arrays in/out (blocking).  With ``rls_P`` the RLS update is fused: ``theta`` and
        ``rls_P`` are updated in place (returned in the dict as well)."""
        c = lambda a, n: np.ascontiguousarray(a, np.float64).reshape(-1, n)
        x0 = c(x0, 4)
        B = x0.shape[0]
        u_prev, theta, Rref, prm = c(u_prev, 2), c(theta, 14).copy(), c(Rref, 4 * (self.N + 1)), c(prm, 10)
        ww = None if w_warm is None else c(w_warm, self.nw)
        P = phi = y = None
        if rls_P is not None:
            P = np.ascontiguousarray(rls_P, np.float64).reshape(B, 2, 7, 7).copy()
            phi, y = c(rls_phi, 7), c(rls_y, 2)
        u0 = np.empty((B, 2)); f = np.empty(B)
        w = np.empty((B, self.nw)) if want_w else None
        st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        rc = lib().dart_rmpc_solve_batch(self._h, B, _ptr(x0), _ptr(u_prev), _ptr(theta), _ptr(P), _ptr(phi), _ptr(y),
                                         float(rls_lambda), _ptr(Rref), _ptr(prm), _ptr(ww), _ptr(u0), _ptr(f),
                                         _ptr(w), _ptr(st), _ptr(it), None)
        if rc != 0:
            self._err(rc, "dart_rmpc_solve_batch")
        return dict(u0=u0, f=f, w=w, status=st, iters=it, theta=theta, rls_P=P)

    def solve_batch_dev(self, B, x0, u_prev, theta, Rref, prm, u0, f, status, iters, w_warm=0, w_out=0,
                        rls_P=0, rls_phi=0, rls_y=0, rls_lambda=0.995, stream=0):
        rc = lib().dart_rmpc_solve_batch_dev(self._h, int(B), x0, u_prev, theta, rls_P or None, rls_phi or None,
                                             rls_y or None, float(rls_lambda), Rref, prm, w_warm or None, u0, f,
                                             w_out or None, status, iters, stream or None)
        if rc != 0:
            self._err(rc, "dart_rmpc_solve_batch_dev")

    # -- device-resident closed loop (dart_rmpc_loop_step_dev / dart_rmpc_rollout_dev / dart_rmpc_rollout) ----
    def loop_step_dev(self, B, k, do_post, do_pre, log_rows, target, prm, mu, state, io, logs, plant=None, loop=None,
                      stream=0):
        """One loop-step launch: post(k) and / or the next step's pre.  ``state`` / ``io`` / ``logs`` map the names
        of RMPC_LOOP_STATE (P and w are not needed) / RMPC_LOOP_IO / RMPC_LOOP_LOGS to device pointers (ints)."""
        spec = tuple(e for e in RMPC_LOOP_STATE if e[0] not in ("P", "w"))
        self._loop_dev("dart_rmpc_loop_step_dev", (plant or plant_config(), loop or rmpc_loop_config()),
                       (B, k, do_post, do_pre, log_rows), (target, prm, mu),
                       ((spec, state), (RMPC_LOOP_IO, io), (RMPC_LOOP_LOGS, logs)), stream)

    def rollout_dev(self, B, k0, steps, log_rows, target, prm, mu, state, logs, plant=None, loop=None, stream=0):
        """``steps`` closed-loop steps from step ``k0`` on the device, no host synchronisation in between: RLS
        features, governor, staged reference, warm-started solve with the fused RLS update, logs, plant step
        (device pointers as in ``loop_step_dev``; asynchronous on ``stream``).  Calling again with ``k0`` advanced
        continues the rollout."""
        self._loop_dev("dart_rmpc_rollout_dev", (plant or plant_config(), loop or rmpc_loop_config()),
                       (B, k0, steps, log_rows), (target, prm, mu), ((RMPC_LOOP_STATE, state), (RMPC_LOOP_LOGS, logs)),
                       stream)

    def rollout(self, k0, steps, target, prm, mu, state, logs, plant=None, loop=None):
        """Host arrays (blocking): ``state`` (RMPC_LOOP_STATE, see ``loop_state``) is advanced and ``logs``
        (``loop_logs``) are filled in place."""
        mu = np.broadcast_to(np.asarray(mu, np.float64), (state["x"].shape[0],))
        self._loop_host("dart_rmpc_rollout", (plant or plant_config(), loop or rmpc_loop_config()), k0, steps,
                        logs["x"].shape[0], ((target, 4), (prm, 10), (mu, 0)), RMPC_LOOP_STATE, state, RMPC_LOOP_LOGS,
                        logs, nw=self.nw)

    # -- the same loop on the LMPC plant (dart_rmpc_lm_loop_step_dev / dart_rmpc_lm_rollout_dev / dart_rmpc_lm_rollout) ----
    def loop_step_lm_dev(self, B, k, do_post, do_pre, log_rows, target, prm, plant_pvec, state, io, logs, plant=None,
                         loop=None, stream=0):
        """``loop_step_dev`` on the LMPC plant: ``state`` maps RMPC_LM_LOOP_STATE (P and w are not needed), ``logs``
        RMPC_LM_LOOP_LOGS (None: metrics-only) to device pointers."""
        spec = tuple(e for e in RMPC_LM_LOOP_STATE if e[0] not in ("P", "w"))
        self._loop_dev("dart_rmpc_lm_loop_step_dev", (plant or plant_config(), loop or rmpc_loop_config()),
                       (B, k, do_post, do_pre, log_rows), (target, prm, plant_pvec),
                       ((spec, state), (RMPC_LOOP_IO, io), (RMPC_LM_LOOP_LOGS, logs)), stream)

    def rollout_lm_dev(self, B, k0, steps, log_rows, target, prm, plant_pvec, state, logs, plant=None, loop=None, stream=0):
        """``rollout_dev`` on the LMPC plant with the true parameters ``plant_pvec`` [B, 34]: ``state`` maps
        RMPC_LM_LOOP_STATE (x [B, 8], ..., metrics [B, 8]), ``logs`` RMPC_LM_LOOP_LOGS to device pointers; ``logs`` None
        is the metrics-only mode (done / nlog still advance)."""
        self._loop_dev("dart_rmpc_lm_rollout_dev", (plant or plant_config(), loop or rmpc_loop_config()),
                       (B, k0, steps, log_rows), (target, prm, plant_pvec),
                       ((RMPC_LM_LOOP_STATE, state), (RMPC_LM_LOOP_LOGS, logs)), stream)

    def rollout_lm(self, k0, steps, target, prm, plant_pvec, state, logs, plant=None, loop=None):
        """Host arrays (blocking): ``state`` (RMPC_LM_LOOP_STATE, see ``loop_state_lm``) is advanced and ``logs``
        (``loop_logs`` of RMPC_LM_LOOP_LOGS) are filled in place; ``logs`` None moves no log."""
        self._loop_host("dart_rmpc_lm_rollout", (plant or plant_config(), loop or rmpc_loop_config()), k0, steps,
                        logs["x"].shape[0] if logs is not None else 0, ((target, 4), (prm, 10), (plant_pvec, 34)),
                        RMPC_LM_LOOP_STATE, state, RMPC_LM_LOOP_LOGS, logs, nw=self.nw)

    # -- the loop through the dual-arm layer (dart_rmpc_stack[_lm]_loop_step_dev / _rollout_dev / _rollout) ----
    def _rmpc_stack_logs(self, lm, rmpc_logs, stack_logs, arm_logs=False):
        spec = RMPC_LM_LOOP_LOGS if lm else RMPC_LOOP_LOGS
        out = [_any_ptr(rmpc_logs[name]) if rmpc_logs is not None else None for name, _, _ in spec]
        out += [_any_ptr(stack_logs[name]) if stack_logs is not None else None for name, _, _ in RMPC_STACK_LOGS]
        if arm_logs is not False:
            out += [_any_ptr(arm_logs[name]) if arm_logs is not None else None for name in ARM_LOOP_LOGS]
        return out

    def rmpc_stack_loop_step_dev(self, E, n, k, phase, do_post, do_pre, log_rows, arrays, rmpc_logs=None, stack_logs=None,
                                 plant=None, loop=None, scfg=None, lm=False, stream=0):
        """One launch of the RMPC loop through the arms: ``phase`` STACK_COMMAND (tray_cmd from u0 and tray_pos) or
        STACK_COUPLE (couple + post(k) and / or pre).  ``arrays`` maps the names of RMPC_STACK_STEP_ARGS[lm] to device
        pointers (absent: null); ``rmpc_logs`` (RMPC_[LM_]LOOP_LOGS) and ``stack_logs`` (RMPC_STACK_LOGS) likewise, or
        None."""
        entry = "dart_rmpc_stack_lm_loop_step_dev" if lm else "dart_rmpc_stack_loop_step_dev"
        rc = getattr(lib(), entry)(self._h, ctypes.byref(plant or plant_config()), ctypes.byref(loop or rmpc_loop_config()),
                                   ctypes.byref(scfg or stack_config()),
                                   int(E), int(n), int(k), int(phase), int(do_post), int(do_pre), int(log_rows),
                                   *[_any_ptr(arrays.get(a)) for a in RMPC_STACK_STEP_ARGS[bool(lm)]],
                                   *self._rmpc_stack_logs(lm, rmpc_logs, stack_logs), stream or None)
        if rc != 0:
            self._err(rc, entry)

    rmpc_stack_loop_step = rmpc_stack_loop_step_dev

    def _rmpc_stack_rollout(self, entry, host, E, n, k0, steps, log_rows, arm_prm_stride, arrays, rmpc_logs, stack_logs,
                            arm_logs, plant, loop, scfg, dcfg, qcfg, lm, stream):
        from .arm import arm_config, arm_dyn_config
        names = [a for a in RMPC_STACK_ROLLOUT_ARGS[bool(lm)] if not (host and a == "work")]
        rc = getattr(lib(), entry)(self._h, ctypes.byref(plant or plant_config()), ctypes.byref(loop or rmpc_loop_config()),
                                   ctypes.byref(scfg or stack_config()), ctypes.byref(dcfg or arm_dyn_config()),
                                   ctypes.byref(qcfg or arm_config()),
                                   int(E), int(n), int(k0), int(steps), int(log_rows), int(arm_prm_stride),
                                   *[_any_ptr(arrays.get(a)) for a in names],
                                   *self._rmpc_stack_logs(lm, rmpc_logs, stack_logs, arm_logs), stream or None)
        if rc != 0:
            self._err(rc, entry)

    def rmpc_stack_rollout_dev(self, E, n, k0, steps, log_rows, arm_prm_stride, arrays, rmpc_logs=None, stack_logs=None,
                               arm_logs=None, plant=None, loop=None, scfg=None, dcfg=None, qcfg=None, lm=False, stream=0):
        """``steps`` steps of the RMPC loop through the arms from step ``k0`` on the device, asynchronous on ``stream``:
        ``arrays`` maps RMPC_STACK_ROLLOUT_ARGS[lm] to device pointers; the three log groups are mappings or None."""
        self._rmpc_stack_rollout("dart_rmpc_stack_lm_rollout_dev" if lm else "dart_rmpc_stack_rollout_dev", False, E, n, k0,
                                 steps, log_rows, arm_prm_stride, arrays, rmpc_logs, stack_logs, arm_logs, plant, loop, scfg,
                                 dcfg, qcfg, lm, stream)

    def rmpc_stack_rollout(self, E, n, k0, steps, rows, arm_prm_stride, arrays, rmpc_logs=None, stack_logs=None,
                           arm_logs=None, plant=None, loop=None, scfg=None, dcfg=None, qcfg=None, lm=False):
        """The same on host arrays (C-contiguous numpy, no ``work``; blocking): state and metrics are advanced, the step
        rows k0 .. k0+steps-1 of the logs given and the episode rows from ``nlog`` on are filled in place."""
        for name, a in list(arrays.items()) + [kv for g in (rmpc_logs, stack_logs, arm_logs) if g for kv in g.items()]:
            if a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous):
                raise DartMPCError(f"stack rollout array {name!r} must be a C-contiguous numpy array")
        self._rmpc_stack_rollout("dart_rmpc_stack_lm_rollout" if lm else "dart_rmpc_stack_rollout", True, E, n, k0, steps,
                                 rows, arm_prm_stride, arrays, rmpc_logs, stack_logs, arm_logs, plant, loop, scfg, dcfg,
                                 qcfg, lm, 0)

    def loop_state_lm(self, x0, x_rot0=None, P0=1e3):
        """The state of a fresh cross-plant rollout from the measured states ``x0`` [B, 4] and the rotation states
        ``x_rot0`` [B, 4] (default zeros)."""
        x0 = np.asarray(x0, np.float64).reshape(-1, 4)
        B = x0.shape[0]
        st = {name: np.zeros(_loop_shape(B, width, nw=self.nw), dt) for name, width, dt in RMPC_LM_LOOP_STATE}
        st["x"][:, :4] = x0
        if x_rot0 is not None:
            st["x"][:, 4:] = np.asarray(x_rot0, np.float64).reshape(B, 4)
        st["prev"][:] = x0
        st["P"][:] = np.tile(np.eye(7) * float(P0), (2, 1, 1)).reshape(98)
        st["metrics"][:] = loop_metrics(B)
        return st

    def loop_state(self, x0, P0=1e3):
        """The state of a fresh rollout from the measured states ``x0`` [B, 4] (run_rmpc's initial values)."""
        x0 = np.asarray(x0, np.float64).reshape(-1, 4)
        B = x0.shape[0]
        st = {name: np.zeros(_loop_shape(B, width, nw=self.nw), dt) for name, width, dt in RMPC_LOOP_STATE}
        st["x"][:, :4] = x0
        st["prev"][:] = x0
        st["P"][:] = np.tile(np.eye(7) * float(P0), (2, 1, 1)).reshape(98)
        return st


LMPC_PRM_DEFAULT = np.array([200.0, 2.0, 200.0, 2.0, 0.0, 0.0, 0.0, 0.0,     # Q   LMPC/src/run.py:118
                             200.0, 2.0, 200.0, 2.0, 0.0, 0.0, 0.0, 0.0,     # Qt  :119
                             0.1, 0.1, 1.0, 1.0,                             # R   :120
                             -0.4, 0.4])                                     # u_bounds :121


class LmpcSolver(Solver):
    """``dart_mpc_handle`` of variant LMPC, N <= 63 (N > 31: the two-wave build).  Defaults are the reference's IPOPT options
    (LMPC/src/controller/rlmpc2.py:480-489): max_iter 50, tol 1e-4, acceptable_tol 1e-3,
    acceptable_iter 5, and IPOPT's defaults max_soc 4 (second-order correction; 0 = off),
    constr_mult_init_max 1000 (least-square starting multipliers; 0 = start from 0) and its soft
    restoration / restoration phases after a failed line search (restoration=False: status -2 there);
    max_cpu_time 0.05 s (rlmpc2.py:485; status -4 past it, measured per instance on the GPU clock; 0 = off)."""

    def __init__(self, N=20, Ts=0.002, tol=1e-4, max_iter=50, acceptable_tol=1e-3, acceptable_iter=5,
                 B_max=1024, device=0, max_soc=4, constr_mult_init_max=1000.0, restoration=True, max_cpu_time=0.05):
        self._h = ctypes.c_void_p()
        self.cfg = default_config(variant=VARIANT_LMPC, N=int(N), Ts=float(Ts), tol=float(tol), max_iter=int(max_iter),
                                  B_max=int(B_max), acceptable_tol=float(acceptable_tol),
                                  acceptable_iter=int(acceptable_iter), max_soc=int(max_soc),
                                  constr_mult_init_max=float(constr_mult_init_max),
                                  restoration=int(bool(restoration)), max_cpu_time=float(max_cpu_time))
        rc = lib().dart_mpc_create(ctypes.byref(self.cfg), int(device), ctypes.byref(self._h))
        _LIVE.add(self)
        if rc != 0:
            raise DartMPCError(f"dart_mpc_create(LMPC) failed with code {rc} (no gfx950 device or bad config)")
        self.N = int(N)
        self.nw = lib().dart_lmpc_nw(self.N)

    def solve_batch(self, state, u_prev, pvec, target, prm=None, w_warm=None, want_w=False):
        c = lambda a, n: np.ascontiguousarray(a, np.float64).reshape(-1, n)
        state = c(state, 8)
        B = state.shape[0]
        u_prev, pvec, target = c(u_prev, 2), c(pvec, 34), c(target, 8)
        prm = c(np.tile(LMPC_PRM_DEFAULT, (B, 1)) if prm is None else prm, 22)
        ww = None if w_warm is None else c(w_warm, self.nw)
        u0 = np.empty((B, 2)); f = np.empty(B)
        w = np.empty((B, self.nw)) if want_w else None
        st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        rc = lib().dart_lmpc_solve_batch(self._h, B, _ptr(state), _ptr(u_prev), _ptr(pvec), _ptr(target), _ptr(prm),
                                         _ptr(ww), _ptr(u0), _ptr(f), _ptr(w), _ptr(st), _ptr(it), None)
        if rc != 0:
            self._err(rc, "dart_lmpc_solve_batch")
        return dict(u0=u0, f=f, w=w, status=st, iters=it)

    def solve_batch_dev(self, B, state, u_prev, pvec, target, prm, u0, f, status, iters, w_warm=0, w_out=0, stream=0):
        rc = lib().dart_lmpc_solve_batch_dev(self._h, int(B), state, u_prev, pvec, target, prm, w_warm or None, u0, f,
                                             w_out or None, status, iters, stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_solve_batch_dev")

    def policy_solve_batch_dev(self, pcfg, B, weights, state, u_prev, target, current_k, obs_mean, obs_M2, obs_count,
                               history, timestep, noise, model_params, prm, u0, f, status, iters, action_out=0,
                               w_warm=0, w_out=0, stream=0):
        """Fused policy step + solve (dart_lmpc_policy_solve_batch_dev), device pointers, asynchronous;
        ``pcfg`` is a ``dart_mpc.lmpc.PolicyConfig``."""
        rc = lib().dart_lmpc_policy_solve_batch_dev(
            self._h, ctypes.byref(pcfg), int(B), weights, state, u_prev, target, current_k, obs_mean, obs_M2, obs_count,
            history, timestep, noise, model_params, action_out or None, prm, w_warm or None, u0, f, w_out or None,
            status, iters, stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_policy_solve_batch_dev")

    # -- device-resident closed loop (dart_lmpc_loop_step_dev / dart_lmpc_rollout_dev / dart_lmpc_rollout) ----
    def loop_step_dev(self, B, k, do_post, do_pre, log_rows, target, plant_pvec, state, io, logs, plant=None, stream=0):
        """One loop-step launch: post(k) and / or the next step's pre.  ``state`` / ``io`` / ``logs`` map the names
        of LMPC_LOOP_STATE (x, tilt, u_prev and model_params are needed) / LMPC_LOOP_IO / LMPC_LOOP_LOGS to device
        pointers (ints).  Asynchronous."""
        plant = plant or plant_config()
        rc = lib().dart_lmpc_loop_step_dev(
            self._h, ctypes.byref(plant), int(B), int(k), int(do_post), int(do_pre), int(log_rows), target, plant_pvec,
            *[ctypes.c_void_p(int(state[n])) for n in ("x", "tilt", "u_prev", "model_params")],
            *_dev_ptrs(LMPC_LOOP_IO, io), *_dev_ptrs(LMPC_LOOP_LOGS, logs), stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_loop_step_dev")

    def rollout_dev(self, B, k0, steps, log_rows, target, prm, plant_pvec, state, logs, pcfg=None, weights=0,
                    current_k=0, noise=0, plant=None, stream=0):
        """``steps`` closed-loop steps from step ``k0`` on the device, no host synchronisation in between: policy
        step and warm-started solve (one launch for B <= 32, N <= 31), log, plant step (device pointers as in
        ``loop_step_dev``; asynchronous on ``stream``).  ``weights`` = 0 runs the loop without a policy (every solve
        uses ``state["model_params"]`` as its pvec); ``noise`` = 0 means zero noise.  Calling again with ``k0``
        advanced continues the rollout."""
        plant = plant or plant_config()
        rc = lib().dart_lmpc_rollout_dev(self._h, ctypes.byref(plant), ctypes.byref(pcfg) if pcfg is not None else None,
                                         int(B), int(k0), int(steps), int(log_rows), target, prm, plant_pvec,
                                         current_k or None, weights or None, noise or None,
                                         *_dev_ptrs(LMPC_LOOP_STATE, state), *_dev_ptrs(LMPC_LOOP_LOGS, logs),
                                         stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_rollout_dev")

    def rollout(self, k0, steps, target, plant_pvec, state, logs, policy=None, prm=None, noise=None, plant=None):
        """Host arrays (blocking): ``state`` (LMPC_LOOP_STATE, see ``loop_state``) is advanced and ``logs``
        (``loop_logs``) rows k0 .. k0+steps-1 are filled in place.  ``policy`` (a ``dart_mpc.lmpc.LmpcPolicy``) gives
        the weights, the config and ``current_k``; None runs without a policy.  ``noise`` [rows, B, 34] fp32 holds
        step k's draws in row k (None: zero noise)."""
        B, rows = state["x"].shape[0], logs["X"].shape[0]
        c = lambda a, n: np.ascontiguousarray(a, np.float64).reshape(B, n)
        target, plant_pvec = c(target, 8), c(plant_pvec, 34)
        prm = c(np.tile(LMPC_PRM_DEFAULT, (B, 1)) if prm is None else prm, 22)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float32)
            if noise.shape != (rows, B, 34):
                raise DartMPCError(f"rollout noise must have shape {(rows, B, 34)}")
        pcfg = ck = wt = None
        if policy is not None:
            pcfg, wt = ctypes.byref(policy.cfg), np.ascontiguousarray(policy.weights, np.float32)
            ck = c(policy.current_k, 34)
        plant = plant or plant_config()
        rc = lib().dart_lmpc_rollout(self._h, ctypes.byref(plant), pcfg, B, int(k0), int(steps), rows, _ptr(target),
                                     _ptr(prm), _ptr(plant_pvec), _ptr(ck), _ptr(wt), _ptr(noise),
                                     *_host_ptrs(LMPC_LOOP_STATE, state, (B,), nw=self.nw),
                                     *_host_ptrs(LMPC_LOOP_LOGS, logs, (rows, B)), None)
        if rc != 0:
            self._err(rc, "dart_lmpc_rollout")

    # -- evaluation (dart_lmpc_eval_loop_step_dev / dart_lmpc_eval_dev / dart_lmpc_eval / dart_lmpc_eval_scores*) ----
    def eval_loop_step_dev(self, B, k, do_post, do_pre, log_rows, target, plant_pvec, state, io, logs, plant=None,
                           stream=0):
        """``loop_step_dev`` with the streaming metrics: ``state`` also maps ``metrics`` [B, 8]; ``logs`` None is the
        metrics-only mode (no log row is written)."""
        plant = plant or plant_config()
        rc = lib().dart_lmpc_eval_loop_step_dev(
            self._h, ctypes.byref(plant), int(B), int(k), int(do_post), int(do_pre), int(log_rows), target, plant_pvec,
            *[ctypes.c_void_p(int(state[n])) for n in ("x", "tilt", "u_prev", "model_params")],
            *_dev_ptrs(LMPC_LOOP_IO, io), ctypes.c_void_p(int(state["metrics"])), *_dev_ptrs(LMPC_LOOP_LOGS, logs),
            stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_eval_loop_step_dev")

    def evaluate_dev(self, P, B, k0, steps, log_rows, target, prm, plant_pvec, state, logs, pcfg=None, weights=0,
                     current_k=0, noise=0, scores=0, plant=None, stream=0):
        """``rollout_dev`` for P policies at once, with metrics: P learners of B instances each, stacked learner-major
        (every array [P B, ..], logs and noise [log_rows, P B, ..], ``weights`` [P, 39748]); ``state`` maps
        LMPC_EVAL_STATE (``metrics`` [P B, 8], see ``loop_metrics``) to device pointers; ``logs`` None is the
        metrics-only mode; ``scores`` [P, 8] (SCORE_SLOTS) is written after the last step when given."""
        plant = plant or plant_config()
        rc = lib().dart_lmpc_eval_dev(self._h, ctypes.byref(plant), ctypes.byref(pcfg) if pcfg is not None else None,
                                      int(P), int(B), int(k0), int(steps), int(log_rows), target, prm, plant_pvec,
                                      current_k or None, weights or None, noise or None,
                                      *_dev_ptrs(LMPC_EVAL_STATE, state), scores or None,
                                      *_dev_ptrs(LMPC_LOOP_LOGS, logs), stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_eval_dev")

    def evaluate(self, P, k0, steps, target, plant_pvec, state, logs, pcfg=None, weights=None, current_k=None, prm=None,
                 noise=None, scores=None, rows=None, plant=None):
        """Host arrays (blocking): ``state`` (LMPC_EVAL_STATE, [P B, ..]) is advanced, ``scores`` [P, 8] (or None)
        written, and rows k0 .. k0+steps-1 of ``logs`` (``loop_logs`` of LMPC_LOOP_LOGS over P B instances) filled in
        place; ``logs`` None is the metrics-only mode, which moves no log (``rows`` then bounds k0 + steps, default
        k0 + steps).  ``weights`` [P, 39748] fp32 with ``pcfg`` and ``current_k`` [P B, 34], or None for the loop
        without a policy; ``noise`` [rows, P B, 34] fp32 or None (zero noise)."""
        PB = state["x"].shape[0]
        if P < 1 or PB % P:
            raise DartMPCError(f"{PB} instances do not divide into {P} learners")
        B = PB // P
        rows = logs["X"].shape[0] if logs is not None else (int(k0) + int(steps) if rows is None else int(rows))
        c = lambda a, n: np.ascontiguousarray(a, np.float64).reshape(PB, n)
        target, plant_pvec = c(target, 8), c(plant_pvec, 34)
        prm = c(np.tile(LMPC_PRM_DEFAULT, (PB, 1)) if prm is None else prm, 22)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float32)
            if noise.shape != (rows, PB, 34):
                raise DartMPCError(f"evaluation noise must have shape {(rows, PB, 34)}")
        wt = ck = None
        if weights is not None:
            wt = np.ascontiguousarray(weights, np.float32).reshape(P, ACTOR_NWEIGHTS)
            ck = c(current_k, 34)
        if scores is not None:
            _inplace(scores, np.float64, 8 * P, "scores")
        plant = plant or plant_config()
        rc = lib().dart_lmpc_eval(self._h, ctypes.byref(plant), ctypes.byref(pcfg) if pcfg is not None else None, P, B,
                                  int(k0), int(steps), rows, _ptr(target), _ptr(prm), _ptr(plant_pvec), _ptr(ck), _ptr(wt),
                                  _ptr(noise), *_host_ptrs(LMPC_EVAL_STATE, state, (PB,), nw=self.nw), _ptr(scores),
                                  *_host_ptrs(LMPC_LOOP_LOGS, logs, (rows, PB)), None)
        if rc != 0:
            self._err(rc, "dart_lmpc_eval")

    @staticmethod
    def eval_scores(metrics):
        """The score kernel alone on host arrays: metrics [P, B, 8] -> scores [P, 8] (SCORE_SLOTS)."""
        m = np.ascontiguousarray(metrics, np.float64)
        if m.ndim != 3 or m.shape[2] != 8:
            raise DartMPCError("metrics must have shape [P, B, 8]")
        out = np.empty((m.shape[0], 8))
        _rc(lib().dart_lmpc_eval_scores(m.shape[0], m.shape[1], _ptr(m), _ptr(out)), "dart_lmpc_eval_scores")
        return out

    def loop_state(self, x0, policy=None, model_params=None):
        """The state of a fresh rollout from the states ``x0`` [B, 8]: ``model_params`` starts at the policy's (its
        ``current_k`` for a fresh policy), or at the given fixed parameter vectors without one; zeros elsewhere."""
        x0 = np.asarray(x0, np.float64).reshape(-1, 8)
        B = x0.shape[0]
        st = {name: np.zeros(_loop_shape(B, width, nw=self.nw), dt) for name, width, dt in LMPC_LOOP_STATE}
        st["x"][:] = x0
        if policy is not None:
            for name in ("obs_mean", "obs_M2", "obs_count", "timestep", "model_params"):
                st[name][:] = getattr(policy, name)
            st["history"][:] = np.asarray(policy.history, np.float32).reshape(B, 520)
        if model_params is not None:
            st["model_params"][:] = np.asarray(model_params, np.float64).reshape(B, 34)
        return st

    # -- experience collection (dart_lmpc_experience_step_dev / dart_lmpc_collect_dev / dart_lmpc_collect) ----
    def experience_step_dev(self, B, k, log_rows, rec_rows, reset_rows, pcfg, rcfg, weights, critic, action, log_X,
                            target, plant_pvec, state, cstate, logs, rec, pool=None, solve_state=0, mean_out=0, stream=0):
        """One experience launch for step k (after post(k)).  ``state`` (history, timestep, u_prev, x, tilt),
        ``cstate`` (LMPC_COLLECT_STATE), ``logs`` (LMPC_COLLECT_LOGS), ``rec`` (LMPC_COLLECT_REC) and ``pool``
        (LMPC_COLLECT_POOL) map names to device pointers (ints).  Asynchronous."""
        pool = pool or {}
        p = lambda v: ctypes.c_void_p(int(v)) if v else None
        rc = lib().dart_lmpc_experience_step_dev(
            self._h, ctypes.byref(pcfg) if pcfg is not None else None, ctypes.byref(rcfg) if rcfg is not None else None,
            int(B), int(k), int(log_rows), int(rec_rows), int(reset_rows), p(weights), p(critic), p(state["history"]),
            p(action), p(log_X), p(state["timestep"]), p(state["u_prev"]), p(target), p(plant_pvec), p(state["x"]),
            p(state["tilt"]), p(solve_state), *_dev_ptrs(LMPC_COLLECT_STATE, cstate),
            *[p(pool.get(n, 0)) for n, _, _ in LMPC_COLLECT_POOL], *_dev_ptrs(LMPC_COLLECT_LOGS, logs),
            *[p(rec.get(n, 0)) for n, _, _ in LMPC_COLLECT_REC], p(mean_out), stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_experience_step_dev")

    def collect_dev(self, B, k0, steps, log_rows, rec_rows, reset_rows, target, prm, plant_pvec, state, cstate, logs,
                    clogs, rec, pcfg, rcfg, weights, critic, current_k, noise=0, pool=None, plant=None, stream=0):
        """``rollout_dev`` with experience collection: device pointers (ints) as there, plus ``cstate``
        (LMPC_COLLECT_STATE), ``clogs`` (LMPC_COLLECT_LOGS), ``rec`` (LMPC_COLLECT_REC) and ``pool``
        (LMPC_COLLECT_POOL, with ``reset_rows`` > 0).  ``target`` and ``plant_pvec`` are rewritten by resets."""
        plant = plant or plant_config()
        pool = pool or {}
        p = lambda v: ctypes.c_void_p(int(v)) if v else None
        rc = lib().dart_lmpc_collect_dev(
            self._h, ctypes.byref(plant), ctypes.byref(pcfg) if pcfg is not None else None,
            ctypes.byref(rcfg) if rcfg is not None else None, int(B), int(k0), int(steps), int(log_rows), int(rec_rows),
            int(reset_rows), p(target), p(prm), p(plant_pvec), p(current_k), p(weights), p(critic), p(noise),
            *_dev_ptrs(LMPC_LOOP_STATE, state), *_dev_ptrs(LMPC_COLLECT_STATE, cstate),
            *[p(pool.get(n, 0)) for n, _, _ in LMPC_COLLECT_POOL], *_dev_ptrs(LMPC_LOOP_LOGS, logs),
            *_dev_ptrs(LMPC_COLLECT_LOGS, clogs), *[p(rec.get(n, 0)) for n, _, _ in LMPC_COLLECT_REC], stream or None)
        if rc != 0:
            self._err(rc, "dart_lmpc_collect_dev")

    def collect(self, k0, steps, target, plant_pvec, state, cstate, logs, clogs, rec, policy, rcfg=None, prm=None,
                noise=None, pool=None, plant=None):
        """Host arrays (blocking): ``rollout`` with experience collection.  ``target`` [B, 8] and ``plant_pvec``
        [B, 34] (float64, C-contiguous) are updated in place by resets, ``cstate`` (``collect_state``) is advanced,
        ``clogs`` (``loop_logs(LMPC_COLLECT_LOGS, rows, B)``) rows k0 .. k0+steps-1 and the records ``rec``
        (``loop_logs(LMPC_COLLECT_REC, rec_rows, B)``) are filled in place.  ``policy`` (a ``dart_mpc.lmpc.LmpcPolicy``
        with ``critic_weights``) is required; ``pool`` maps the names of LMPC_COLLECT_POOL to [reset_rows, B, width]
        arrays (None: episode ends only reset the counters)."""
        B, rows = state["x"].shape[0], logs["X"].shape[0]
        rec_rows = rec["rec_reward"].shape[0]
        reset_rows = 0 if not pool else pool["reset_x"].shape[0]
        prm = np.ascontiguousarray(np.tile(LMPC_PRM_DEFAULT, (B, 1)) if prm is None else prm, np.float64).reshape(B, 22)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float32)
            if noise.shape != (rows, B, 34):
                raise DartMPCError(f"collect noise must have shape {(rows, B, 34)}")
        tg, pp = _host_ptrs((("target", 8, np.float64), ("plant_pvec", 34, np.float64)),
                            {"target": target, "plant_pvec": plant_pvec}, (B,))
        pcfg = wt = cw = ck = None
        if policy is not None:
            pcfg, wt = ctypes.byref(policy.cfg), np.ascontiguousarray(policy.weights, np.float32)
            cw = None if policy.critic_weights is None else np.ascontiguousarray(policy.critic_weights, np.float32)
            ck = np.ascontiguousarray(policy.current_k, np.float64).reshape(B, 34)
        rcfg = rcfg if rcfg is not None else reward_config()
        plant = plant or plant_config()
        pool_ptrs = (_host_ptrs(LMPC_COLLECT_POOL, pool, (reset_rows, B)) if reset_rows else [None] * 3)
        rc = lib().dart_lmpc_collect(
            self._h, ctypes.byref(plant), pcfg, ctypes.byref(rcfg), B, int(k0), int(steps), rows, rec_rows, reset_rows,
            tg, _ptr(prm), pp, _ptr(ck), _ptr(wt), _ptr(cw), _ptr(noise),
            *_host_ptrs(LMPC_LOOP_STATE, state, (B,), nw=self.nw), *_host_ptrs(LMPC_COLLECT_STATE, cstate, (B,)),
            *pool_ptrs, *_host_ptrs(LMPC_LOOP_LOGS, logs, (rows, B)), *_host_ptrs(LMPC_COLLECT_LOGS, clogs, (rows, B)),
            *_host_ptrs(LMPC_COLLECT_REC, rec, (rec_rows, B)), None)
        if rc != 0:
            self._err(rc, "dart_lmpc_collect")

    # -- whole PPO iterations on the device (dart_lmpc_train_dev / dart_lmpc_train) ----
    def train_dev(self, B, reset_rows, target, prm, plant_pvec, current_k, weights, critic, state, cstate, logs, clogs,
                  rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool=None, plant=None, stream=0):
        """``tcfg.iterations`` complete PPO iterations enqueued on one stream, no host work in between
        (dart_lmpc_train_dev).  Device pointers (ints) as in ``collect_dev``; ``weights``, ``critic`` and
        ``current_k`` are updated in place; ``train`` maps the names of LMPC_TRAIN_ARRAYS (adam, adam_step,
        train_log [iterations, 12], best_return, best_weights, best_iter, workspace of ``train_workspace_bytes``) to
        device pointers.  The logs have ``tcfg.steps`` rows and the records steps / record_every."""
        _train_dev(self, "train_dev", (), (), B, reset_rows, target, prm, plant_pvec, current_k, weights, critic, state,
                        cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool, plant, stream)

    def train_global_dev(self, B, reset_rows, target, prm, plant_pvec, current_k, weights, critic, state, cstate, logs,
                         clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, gbuf, pool=None, plant=None, stream=0):
        """``train_dev`` with the global-buffer update (dart_lmpc_train_global_dev): ``gbuf`` is a ``global_buffer``
        struct of device pointers (capacity >= G of ``global_rows``, ``fill`` the rows held now, ``global_log``
        [iterations, 6], ``workspace`` of ``global_workspace_bytes``), or None for ``train_dev`` itself.  The next
        call's fill is ``global_fill_after(n, gbuf.fill, tcfg.iterations)``."""
        _train_dev(self, "train_global_dev", (), (gbuf,), B, reset_rows, target, prm, plant_pvec, current_k, weights,
                        critic, state, cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool, plant, stream)

    # -- a population of learners in one device-resident iteration (dart_lmpc_train_pop_dev / dart_lmpc_train_pop) ----
    def train_pop_dev(self, P, seeds, B, reset_rows, target, prm, plant_pvec, current_k, weights, critic, state, cstate,
                      logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool=None, plant=None, stream=0):
        """``train_dev`` for ``P`` independent learners of ``B`` instances each in the same launches
        (dart_lmpc_train_pop_dev).  Device pointers as in ``train_dev`` with the instances stacked learner-major
        (instance l B + b: every per-instance array has P B in place of B) and, per learner, ``weights`` [P, 39748],
        ``critic`` [P, POP_CRITIC_STRIDE], adam [P, 2, 77317], adam_step [P], train_log [P, iterations, 12],
        best_return [P], best_weights [P, 77317], best_iter [P]; the workspace has ``train_pop_workspace_bytes``.
        ``seeds`` are P integers (``tcfg.seed`` is ignored); learner l is bit for bit ``train_dev`` on its arrays with
        seed ``seeds[l]``."""
        _train_dev(self, "train_pop_dev", (P, seeds), (), B, reset_rows, target, prm, plant_pvec, current_k, weights,
                        critic, state, cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool, plant, stream)

    def train_pop_global_dev(self, P, seeds, B, reset_rows, target, prm, plant_pvec, current_k, weights, critic, state,
                             cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, gbuf, pool=None, plant=None,
                             stream=0):
        """``train_pop_dev`` with the global-buffer update (dart_lmpc_train_pop_global_dev): ``gbuf`` is a
        ``global_buffer`` struct of device pointers to P buffers stacked learner-major, ``capacity`` rows apart (obs
        [P, capacity, 520], ..., ``global_log`` [P, iterations, 6], ``workspace`` of ``global_pop_workspace_bytes``;
        ``fill`` is one number for all learners), or None for ``train_pop_dev`` itself.  Learner l is bit for bit
        ``train_global_dev`` on its arrays, its buffer and seed ``seeds[l]``."""
        _train_dev(self, "train_pop_global_dev", (P, seeds), (gbuf,), B, reset_rows, target, prm, plant_pvec, current_k,
                        weights, critic, state, cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool, plant,
                        stream)

    def train_pop_hyper_dev(self, P, seeds, B, reset_rows, target, prm, plant_pvec, current_k, weights, critic, state,
                            cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, gbuf=None, hyper=0, pool=None,
                            plant=None, stream=0):
        """``train_pop_global_dev`` with per-learner hyper-parameters (dart_lmpc_train_pop_hyper_dev): ``hyper`` is
        the device pointer of a float64 table [P, HYPER_COLS] (``hyper_table``), row l the first nine fields of
        ``ppo_cfg`` for learner l (HYPER_FIELDS), read by the update's kernels when they run -- a table rewritten on
        the same stream between two calls takes effect.  ``hyper`` 0 is ``train_pop_global_dev``, ``gbuf`` None no
        global update.  Learner l is bit for bit ``train_global_dev`` with ``ppo_config(**row l)``."""
        _train_dev(self, "train_pop_hyper_dev", (P, seeds), (gbuf,), B, reset_rows, target, prm, plant_pvec, current_k,
                   weights, critic, state, cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool, plant,
                   stream, hyper=(hyper,))

    @staticmethod
    def pbt_step_dev(cfg, P, fitness, fitness_stride, weights, critic, adam, adam_step, hyper, rank_out, parent_out,
                     stream=0):
        """The exploit/explore step of population-based training on device pointers (dart_lmpc_pbt_step_dev;
        asynchronous): ``cfg`` is a ``pbt_config``, ``fitness`` + l ``fitness_stride`` learner l's figure of merit
        (float64; ``scores + 8 * slot, 8`` reads a column of ``evaluate_dev``'s scores), the other arrays those of
        ``train_pop_dev`` and the table of ``train_pop_hyper_dev``; ``rank_out`` and ``parent_out`` are int32 [P].
        ``ppo.pbt_plan`` states the rule in numpy."""
        _rc(lib().dart_lmpc_pbt_step_dev(ctypes.byref(cfg), int(P), _vp(fitness), int(fitness_stride), _vp(weights),
                                         _vp(critic), _vp(adam), _vp(adam_step), _vp(hyper), _vp(rank_out),
                                         _vp(parent_out), stream or None), "dart_lmpc_pbt_step_dev")

    def _train_host(self, entry, who, B, nl, nets, target, plant_pvec, state, cstate, logs, clogs, rec, pcfg, adam,
                    adam_step, train_log, best_return, best_weights, best_iter, ppo_cfg, tcfg, rcfg, prm, pool, plant,
                    global_buffer, global_log, hyper=None):
        """``train`` and ``train_pop``: ``nl`` learners of ``B`` instances each, their arrays stacked; ``nets`` are
        the checked current_k, actor and critic arrays, ``who`` is () or (P, the seeds' pointer).  With
        ``global_buffer`` the entry is ``entry`` + "_global"; with ``hyper`` (a checked table) it is ``entry`` +
        "_hyper", which takes the buffer (or NULL) and the table."""
        NI, K = state["x"].shape[0], int(tcfg.steps)
        rcfg = rcfg if rcfg is not None else reward_config()
        R = K // max(int(rcfg.record_every), 1)
        reset_rows = 0 if not pool else pool["reset_x"].shape[0]
        prm = np.ascontiguousarray(np.tile(LMPC_PRM_DEFAULT, (NI, 1)) if prm is None else prm, np.float64).reshape(NI, 22)
        plant = plant or plant_config()
        head = [("target", 8, np.float64), ("plant_pvec", 34, np.float64)]
        tg, pp = _host_ptrs(head, {"target": target, "plant_pvec": plant_pvec}, (NI,))
        tail = [_inplace(adam, np.float32, nl * 2 * PPO_NPARAMS, "adam"), _inplace(adam_step, np.int32, nl, "adam_step"),
                _inplace(train_log, np.float64, nl * TRAIN_LOG_COLS * int(tcfg.iterations), "train_log"),
                _inplace(best_return, np.float64, nl, "best_return"),
                _inplace(best_weights, np.float32, nl * PPO_NPARAMS, "best_weights"),
                _inplace(best_iter, np.int32, nl, "best_iter")]
        ptrs = ([tg, _ptr(prm), pp] + [_ptr(a) for a in nets]
                + _host_ptrs(LMPC_LOOP_STATE, state, (NI,), nw=self.nw) + _host_ptrs(LMPC_COLLECT_STATE, cstate, (NI,))
                + (_host_ptrs(LMPC_COLLECT_POOL, pool, (reset_rows, NI)) if reset_rows else [None] * 3)
                + _host_ptrs(LMPC_LOOP_LOGS, logs, (K, NI)) + _host_ptrs(LMPC_COLLECT_LOGS, clogs, (K, NI))
                + _host_ptrs(LMPC_COLLECT_REC, rec, (R, NI)) + [_ptr(a) for a in tail] + [None])
        buf = _train_buffers([0 if q is None else q.value for q in ptrs])
        g = []
        if global_buffer is not None:
            g = [_host_global(global_buffer, nl * int(tcfg.iterations), global_log, learners=nl)]
            entry += "_global"
        tail = [ctypes.byref(q) for q in g]
        if hyper is not None:
            entry = entry[:-len("_global")] if g else entry
            entry += "_hyper"
            tail = (tail or [None]) + [_ptr(hyper)]
        rc = getattr(lib(), entry)(self._h, ctypes.byref(plant), ctypes.byref(pcfg), ctypes.byref(rcfg),
                                   ctypes.byref(ppo_cfg), ctypes.byref(tcfg), *who, B, reset_rows, buf, *tail, None)
        if rc != 0:
            self._err(rc, entry)
        if g:
            global_buffer["fill"] = global_fill_after(R * B, g[0].fill, int(tcfg.iterations))

    def train_pop(self, P, seeds, target, plant_pvec, state, cstate, logs, clogs, rec, pcfg, weights, critic, current_k,
                  adam, adam_step, train_log, best_return, best_weights, best_iter, ppo_cfg, tcfg, rcfg=None, prm=None,
                  pool=None, plant=None, global_buffer=None, global_log=None, hyper=None):
        """Host arrays (blocking, dart_lmpc_train_pop): ``train`` for ``P`` learners, all arrays stacked as
        ``train_pop_dev`` takes them (``ppo.population_stack`` builds them, ``ppo.train_population`` wraps this) and
        updated in place: ``weights`` [P, 39748], ``critic`` [P, POP_CRITIC_STRIDE], ``current_k`` [P B, 34], ``adam``
        [P, 2, 77317], ``adam_step`` [P], ``train_log`` [P, iterations, 12], ``best_return`` [P], ``best_weights``
        [P, 77317], ``best_iter`` [P]; ``state`` / ``cstate`` hold P B instances.  With ``global_buffer`` (a
        ``ppo.new_population_global_buffer`` dict: P stacked buffers and one ``fill``) every iteration also runs the
        global-buffer update (dart_lmpc_train_pop_global): the dict's arrays and ``fill`` are updated in place and
        ``global_log`` [P, iterations, 6] (float64) receives one row per learner and iteration.  With ``hyper`` (a
        float64 table [P, HYPER_COLS], ``hyper_table``; read only) learner l trains with row l in place of the first
        nine fields of ``ppo_cfg`` (dart_lmpc_train_pop_hyper); None takes the entries above, unchanged."""
        P, NI = int(P), state["x"].shape[0]
        if hyper is not None:
            hyper = np.ascontiguousarray(hyper, np.float64)
            if hyper.shape != (P, HYPER_COLS):
                raise DartMPCError(f"train_pop: hyper must have shape {(P, HYPER_COLS)}, got {hyper.shape}")
        B = NI // max(P, 1)
        if P >= 1 and B * P != NI:
            raise DartMPCError(f"train_pop: {NI} instances are not {P} learners of equal size")
        seeds = None if seeds is None else np.ascontiguousarray(seeds, np.uint64).reshape(-1)
        if seeds is not None and seeds.size != P:
            raise DartMPCError(f"train_pop needs {P} seeds, got {seeds.size}")
        nl = max(P, 1)
        nets = (_inplace(current_k, np.float64, 34 * NI, "current_k"),
                _inplace(weights, np.float32, nl * ACTOR_NWEIGHTS, "weights"),
                _inplace(critic, np.float32, nl * POP_CRITIC_STRIDE, "critic"))
        self._train_host("dart_lmpc_train_pop", (P, _ptr(seeds)), B, nl, nets, target, plant_pvec, state, cstate, logs,
                         clogs, rec, pcfg, adam, adam_step, train_log, best_return, best_weights, best_iter, ppo_cfg,
                         tcfg, rcfg, prm, pool, plant, global_buffer, global_log, hyper=hyper)

    def train(self, target, plant_pvec, state, cstate, logs, clogs, rec, policy, adam, adam_step, train_log,
              best_return, best_weights, best_iter, ppo_cfg, tcfg, rcfg=None, prm=None, pool=None, plant=None,
              global_buffer=None, global_log=None):
        """Host arrays (blocking, dart_lmpc_train): state, weights, Adam's state and the reset pool are staged in
        once, ``tcfg.iterations`` iterations run on the device, the results are staged out once.  Updated in place:
        ``target``, ``plant_pvec``, ``state``, ``cstate``, ``policy.weights`` / ``critic_weights`` / ``current_k``,
        ``adam`` [2, 77317], ``adam_step`` [1], ``best_return`` [1] (float64, start at -inf), ``best_weights``
        [77317], ``best_iter`` [1]; ``logs`` / ``clogs`` ([steps, B, ..]) and ``rec`` ([steps / record_every, B, ..])
        receive the last iteration's values, ``train_log`` [iterations, 12] one row per iteration.  With
        ``global_buffer`` (a ``ppo.new_global_buffer`` dict) every iteration also runs the global-buffer update
        (dart_lmpc_train_global): the dict's arrays and ``fill`` are updated in place and ``global_log``
        [iterations, 6] (float64) receives one row per iteration."""
        B = state["x"].shape[0]
        if policy.critic_weights is None:
            raise DartMPCError("training needs a policy with critic_weights")
        policy.current_k = _inplace(policy.current_k, np.float64, 34 * B, "policy.current_k")
        nets = (policy.current_k, _inplace(policy.weights, np.float32, ACTOR_NWEIGHTS, "policy.weights"),
                _inplace(policy.critic_weights, np.float32, CRITIC_NWEIGHTS, "policy.critic_weights"))
        self._train_host("dart_lmpc_train", (), B, 1, nets, target, plant_pvec, state, cstate, logs, clogs, rec,
                         policy.cfg, adam, adam_step, train_log, best_return, best_weights, best_iter, ppo_cfg, tcfg,
                         rcfg, prm, pool, plant, global_buffer, global_log)

    @staticmethod
    def collect_state(u_prev):
        """The collection state of a fresh collection: ``prev_cmd`` and ``control_seen`` start at the initial
        ``u_prev`` [B, 2] (rlmpc2.py:564), every counter at zero."""
        u_prev = np.asarray(u_prev, np.float64).reshape(-1, 2)
        B = u_prev.shape[0]
        st = {name: np.zeros(_loop_shape(B, width), dt) for name, width, dt in LMPC_COLLECT_STATE}
        st["prev_cmd"][:] = u_prev
        st["control_seen"][:] = u_prev
        return st


def reward_config(**over) -> RewardConfig:
    """``dart_lmpc_reward_config`` with the library's defaults (what LMPC/src/run.py effectively runs with), fields
    overridden by keyword (``tray_limit``: a pair)."""
    c = RewardConfig()
    lib().dart_lmpc_reward_config_default(ctypes.byref(c))
    names = [f[0] for f in c._fields_]
    for k, v in over.items():
        if k not in names:
            raise DartMPCError(f"RewardConfig has no field {k!r} (fields: {names})")
        if k == "tray_limit":
            c.tray_limit[0], c.tray_limit[1] = float(v[0]), float(v[1])
        elif k in ("max_episode_steps", "record_every", "done_sticky", "reserved"):
            setattr(c, k, int(v))
        else:
            setattr(c, k, float(v))
    return c


def gae(nrec, rec_reward, rec_value, rec_done, last_value, gamma=0.99, lam=0.95, adv=None, ret=None):
    """Generalised advantage estimation on the GPU (dart_lmpc_gae) over the records [rec_rows, B] of B instances,
    instance b using its first ``nrec[b]`` rows and ``last_value[b]``.  Returns (adv, ret = adv + value), float64
    [rec_rows, B]; rows >= nrec[b] keep the contents of ``adv`` / ``ret`` (NaN in fresh arrays)."""
    rw = np.ascontiguousarray(rec_reward, np.float64)
    rows, B = rw.shape
    c = lambda a, dt, shape: np.ascontiguousarray(a, dt).reshape(shape)
    nrec, lv = c(nrec, np.int32, (B,)), c(last_value, np.float32, (B,))
    rv, rd = c(rec_value, np.float32, (rows, B)), c(rec_done, np.float32, (rows, B))
    adv = np.full((rows, B), np.nan) if adv is None else adv
    ret = np.full((rows, B), np.nan) if ret is None else ret
    for a in (adv, ret):
        if a.dtype != np.float64 or a.shape != (rows, B) or not a.flags.c_contiguous:
            raise DartMPCError(f"gae adv / ret must be C-contiguous float64 arrays of shape {(rows, B)}")
    rc = lib().dart_lmpc_gae(B, rows, float(gamma), float(lam), _ptr(nrec), _ptr(rw), _ptr(rv), _ptr(rd), _ptr(lv),
                             _ptr(adv), _ptr(ret))
    if rc != 0:
        raise DartMPCError(f"dart_lmpc_gae failed ({rc})")
    return adv, ret


def ppo_config(**over) -> PpoConfig:
    """``dart_lmpc_ppo_config`` with the library's defaults (the reference's, rlmpc2.py:202-226, 561), fields
    overridden by keyword."""
    c = PpoConfig()
    lib().dart_lmpc_ppo_config_default(ctypes.byref(c))
    names = [f[0] for f in c._fields_]
    for k, v in over.items():
        if k not in names:
            raise DartMPCError(f"PpoConfig has no field {k!r} (fields: {names})")
        setattr(c, k, int(v) if k in ("epochs", "mini_batch_size") else float(v))
    return c


def hyper_table(P, **over):
    """A population's hyper-parameter table, float64 [P, HYPER_COLS]: every row the library's defaults for
    HYPER_FIELDS (the first nine fields of ``ppo_config()``, in its order), each field overridden by keyword with a
    scalar (all learners) or a sequence of P values (one per learner)."""
    P = int(P)
    if not 1 <= P <= POP_MAX:
        raise DartMPCError(f"hyper_table: 1 <= P <= {POP_MAX}, got {P}")
    c = ppo_config()
    t = np.tile(np.array([getattr(c, f) for f in HYPER_FIELDS], np.float64), (P, 1))
    for k, v in over.items():
        if k not in HYPER_FIELDS:
            raise DartMPCError(f"hyper_table has no column {k!r} (columns: {HYPER_FIELDS})")
        v = np.asarray(v, np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.size != P):
            raise DartMPCError(f"hyper_table: {k!r} takes a scalar or {P} values, got shape {v.shape}")
        t[:, HYPER_FIELDS.index(k)] = v
    return t


def pbt_config(**over) -> PbtConfig:
    """``dart_lmpc_pbt_config`` with the library's defaults, fields overridden by keyword: ``lo`` / ``hi`` take
    HYPER_COLS values or a dict column name -> bound, ``explore_mask`` an integer or a sequence of column names."""
    c = PbtConfig()
    lib().dart_lmpc_pbt_config_default(ctypes.byref(c))
    names = [f[0] for f in c._fields_]
    for k, v in over.items():
        if k not in names:
            raise DartMPCError(f"PbtConfig has no field {k!r} (fields: {names})")
        if k in ("lo", "hi"):
            arr = getattr(c, k)
            if isinstance(v, dict):
                for name, b in v.items():
                    if name not in HYPER_FIELDS:
                        raise DartMPCError(f"pbt_config: no column {name!r} (columns: {HYPER_FIELDS})")
                    arr[HYPER_FIELDS.index(name)] = float(b)
            else:
                v = np.asarray(v, np.float64).reshape(-1)
                if v.size != HYPER_COLS:
                    raise DartMPCError(f"pbt_config: {k} takes {HYPER_COLS} values, got {v.size}")
                for i in range(HYPER_COLS):
                    arr[i] = float(v[i])
        elif k == "explore_mask" and not isinstance(v, (int, np.integer)):
            bad = [n for n in v if n not in HYPER_FIELDS]
            if bad:
                raise DartMPCError(f"pbt_config: no column {bad[0]!r} (columns: {HYPER_FIELDS})")
            c.explore_mask = sum(1 << HYPER_FIELDS.index(n) for n in set(v))
        elif k in ("factor_down", "factor_up"):
            setattr(c, k, float(v))
        else:
            setattr(c, k, int(v))
    return c


def pbt_step(cfg, fitness, weights, critic, adam, adam_step, hyper, fitness_stride=1):
    """The exploit/explore step on host arrays (blocking, dart_lmpc_pbt_step): ``weights`` [P, 39748], ``critic``
    [P, POP_CRITIC_STRIDE], ``adam`` [P, 2, 77317], ``adam_step`` [P] and ``hyper`` [P, HYPER_COLS] are updated in
    place; ``fitness`` (float64) is read at ``l * fitness_stride``.  Returns (rank, parent), int32 [P]."""
    hyper_a = np.asarray(hyper)
    P = hyper_a.shape[0] if hyper_a.ndim == 2 else 0
    fitness = np.ascontiguousarray(fitness, np.float64).reshape(-1)
    if P >= 1 and int(fitness_stride) >= 1 and fitness.size < (P - 1) * int(fitness_stride) + 1:
        raise DartMPCError(f"pbt_step: fitness holds {fitness.size} values, stride {fitness_stride} needs "
                           f"{(P - 1) * int(fitness_stride) + 1}")
    nl = max(P, 1)
    arrs = (_inplace(weights, np.float32, nl * ACTOR_NWEIGHTS, "weights"),
            _inplace(critic, np.float32, nl * POP_CRITIC_STRIDE, "critic"),
            _inplace(adam, np.float32, nl * 2 * PPO_NPARAMS, "adam"), _inplace(adam_step, np.int32, nl, "adam_step"),
            _inplace(hyper, np.float64, nl * HYPER_COLS, "hyper"))
    rank, parent = np.full(nl, -1, np.int32), np.full(nl, -1, np.int32)
    _rc(lib().dart_lmpc_pbt_step(ctypes.byref(cfg), P, _ptr(fitness), int(fitness_stride), *[_ptr(a) for a in arrs],
                                 _ptr(rank), _ptr(parent)), "dart_lmpc_pbt_step")
    return rank, parent


def ppo_workspace_bytes(n, mini_batch_size):
    """Bytes of the device workspace of the PPO entries for ``n`` samples and mini-batches of up to
    ``mini_batch_size``."""
    b = int(lib().dart_lmpc_ppo_workspace_bytes(int(n), int(mini_batch_size)))
    if b == 0:
        raise DartMPCError(f"no PPO workspace for n = {n}, mini_batch_size = {mini_batch_size} (n >= 1, 1 .. 1024)")
    return b


def _vp(v):
    return ctypes.c_void_p(int(v)) if v else None


def _rc(rc, what):
    if rc != 0:
        raise DartMPCError(f"{what} failed ({rc}: {'invalid argument' if rc == -1 else 'HIP error'})")


def ppo_update_dev(cfg, n, rec_total, sample, perm, rec_obs, rec_action, rec_logp, adv, ret, weights, critic, adam,
                   adam_step, stats, workspace, step_log=0, adv_norm_out=0, ret_norm_out=0, stream=0):
    """dart_lmpc_ppo_update_dev: the whole update on device pointers (ints), asynchronous.  ``perm`` holds
    ``cfg.epochs`` rows of n; weights, critic, adam and adam_step are updated in place."""
    _rc(lib().dart_lmpc_ppo_update_dev(
        ctypes.byref(cfg), int(n), int(rec_total), _vp(sample), _vp(perm), _vp(rec_obs), _vp(rec_action),
        _vp(rec_logp), _vp(adv), _vp(ret), _vp(weights), _vp(critic), _vp(adam), _vp(adam_step), _vp(stats),
        _vp(step_log), _vp(adv_norm_out), _vp(ret_norm_out), _vp(workspace), stream or None),
        "dart_lmpc_ppo_update_dev")


def ppo_prepare_dev(n, rec_total, sample, adv, ret, workspace, adv_norm_out=0, ret_norm_out=0, stream=0):
    """dart_lmpc_ppo_prepare_dev: the normalised returns and advantages into the workspace (device pointers)."""
    _rc(lib().dart_lmpc_ppo_prepare_dev(int(n), int(rec_total), _vp(sample), _vp(adv), _vp(ret), _vp(adv_norm_out),
                                        _vp(ret_norm_out), _vp(workspace), stream or None),
        "dart_lmpc_ppo_prepare_dev")


def ppo_grad_dev(cfg, n, rec_total, M, sample, idx, rec_obs, rec_action, rec_logp, weights, critic, grad_out,
                 terms_out, workspace, stream=0):
    """dart_lmpc_ppo_grad_dev: the gradient of one mini-batch ``idx`` [M] (after ``ppo_prepare_dev`` on the same
    workspace) into ``grad_out`` [77317] and ``terms_out`` [4] (device pointers)."""
    _rc(lib().dart_lmpc_ppo_grad_dev(
        ctypes.byref(cfg), int(n), int(rec_total), int(M), _vp(sample), _vp(idx), _vp(rec_obs), _vp(rec_action),
        _vp(rec_logp), _vp(weights), _vp(critic), _vp(grad_out), _vp(terms_out), _vp(workspace), stream or None),
        "dart_lmpc_ppo_grad_dev")


def ppo_apply_dev(cfg, grad, weights, critic, adam, adam_step, workspace, terms=0, stats=0, step_log=0, step_in_call=0,
                  stream=0):
    """dart_lmpc_ppo_apply_dev: clip + Adam step of a packed gradient, in place (device pointers)."""
    _rc(lib().dart_lmpc_ppo_apply_dev(
        ctypes.byref(cfg), _vp(grad), _vp(terms), _vp(weights), _vp(critic), _vp(adam), _vp(adam_step), _vp(stats),
        _vp(step_log), int(step_in_call), _vp(workspace), stream or None), "dart_lmpc_ppo_apply_dev")


def _ppo_records(sample, rec_obs, rec_action, rec_logp, adv, ret):
    c = lambda a, dt: np.ascontiguousarray(a, dt)
    rec_logp = c(rec_logp, np.float32).reshape(-1)
    total = rec_logp.size
    return (c(sample, np.int32).reshape(-1), c(rec_obs, np.float32).reshape(total, 520),
            c(rec_action, np.float32).reshape(total, 34), rec_logp, c(adv, np.float64).reshape(total),
            c(ret, np.float64).reshape(total), total)


def _inplace(a, dt, size, name):
    if not isinstance(a, np.ndarray) or a.dtype != dt or a.size != size or not a.flags.c_contiguous:
        raise DartMPCError(f"{name} must be a C-contiguous {np.dtype(dt).name} array of {size} entries (updated in place)")
    return a


def ppo_update(cfg, sample, perm, rec_obs, rec_action, rec_logp, adv, ret, weights, critic, adam, adam_step):
    """The whole PPO update on host arrays (dart_lmpc_ppo_update, blocking).  The record arrays [rec_total, ..],
    ``adv`` and ``ret`` (float64 [rec_total]) are indexed through ``sample`` [n]; ``perm`` is [cfg.epochs, n].
    ``weights`` [39748], ``critic`` [37569], ``adam`` [2, 77317] (float32) and ``adam_step`` [1] (int32) are updated
    in place.  Returns dict(policy_loss, value_loss, entropy, step_log [steps, 4], adv_norm [n], ret_norm [n])."""
    sample, ro, ra, rl, adv, ret, total = _ppo_records(sample, rec_obs, rec_action, rec_logp, adv, ret)
    n = sample.size
    perm = np.ascontiguousarray(perm, np.int32).reshape(-1)
    if perm.size != int(cfg.epochs) * n:
        raise DartMPCError(f"perm must hold cfg.epochs = {cfg.epochs} rows of n = {n} entries")
    _inplace(weights, np.float32, ACTOR_NWEIGHTS, "weights"); _inplace(critic, np.float32, CRITIC_NWEIGHTS, "critic")
    _inplace(adam, np.float32, 2 * PPO_NPARAMS, "adam"); _inplace(adam_step, np.int32, 1, "adam_step")
    mb = max(int(cfg.mini_batch_size), 1)
    steps = int(cfg.epochs) * (-(-n // mb))
    stats, log = np.zeros(3), np.full((steps, 4), np.nan, np.float32)
    an, rn = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    _rc(lib().dart_lmpc_ppo_update(ctypes.byref(cfg), n, total, _ptr(sample), _ptr(perm), _ptr(ro), _ptr(ra), _ptr(rl),
                                   _ptr(adv), _ptr(ret), _ptr(weights), _ptr(critic), _ptr(adam), _ptr(adam_step),
                                   _ptr(stats), _ptr(log), _ptr(an), _ptr(rn)), "dart_lmpc_ppo_update")
    return dict(policy_loss=float(stats[0]), value_loss=float(stats[1]), entropy=float(stats[2]), step_log=log,
                adv_norm=an, ret_norm=rn)


def _torch_dev(*arrays):
    """Device copies (torch tensors: the package's device-memory plumbing) of numpy arrays."""
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def ppo_grad(cfg, sample, idx, rec_obs, rec_action, rec_logp, adv, ret, weights, critic):
    """The gradient of one mini-batch on host arrays (blocking): ``ppo_prepare_dev`` over the n samples, then
    ``ppo_grad_dev`` on ``idx`` [M] (positions in ``sample``).  Returns (grad float32 [77317] in the packed order,
    terms float32 [4]: policy loss, value loss, entropy, gradient norm)."""
    import torch
    sample, ro, ra, rl, adv, ret, total = _ppo_records(sample, rec_obs, rec_action, rec_logp, adv, ret)
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
    n, M = sample.size, idx.size
    d = _torch_dev(sample, idx, ro, ra, rl, adv, ret, np.ascontiguousarray(weights, np.float32),
                   np.ascontiguousarray(critic, np.float32))
    ws = torch.zeros(ppo_workspace_bytes(n, M), dtype=torch.uint8, device="cuda")
    grad = torch.empty(PPO_NPARAMS, dtype=torch.float32, device="cuda")
    terms = torch.empty(4, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = [t.data_ptr() for t in d]
    ppo_prepare_dev(n, total, p[0], p[5], p[6], ws.data_ptr(), stream=s)
    ppo_grad_dev(cfg, n, total, M, p[0], p[1], p[2], p[3], p[4], p[7], p[8], grad.data_ptr(), terms.data_ptr(),
                 ws.data_ptr(), stream=s)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), terms.cpu().numpy()


def ppo_apply(cfg, grad, weights, critic, adam, adam_step, terms=None):
    """One clip + Adam step of a packed gradient on host arrays (blocking); ``weights``, ``critic``, ``adam`` and
    ``adam_step`` are updated in place.  Returns the logged row (policy loss, value loss, entropy as given in
    ``terms``, gradient norm before the clip)."""
    import torch
    _inplace(weights, np.float32, ACTOR_NWEIGHTS, "weights"); _inplace(critic, np.float32, CRITIC_NWEIGHTS, "critic")
    _inplace(adam, np.float32, 2 * PPO_NPARAMS, "adam"); _inplace(adam_step, np.int32, 1, "adam_step")
    g = np.ascontiguousarray(grad, np.float32).reshape(PPO_NPARAMS)
    t = np.zeros(3, np.float32) if terms is None else np.ascontiguousarray(terms, np.float32).reshape(-1)[:3].copy()
    dg, dt, dw, dc, da, ds = _torch_dev(g, t, weights, critic, adam, adam_step)
    ws = torch.zeros(ppo_workspace_bytes(1, 1), dtype=torch.uint8, device="cuda")
    log = torch.empty(4, dtype=torch.float32, device="cuda")
    ppo_apply_dev(cfg, dg.data_ptr(), dw.data_ptr(), dc.data_ptr(), da.data_ptr(), ds.data_ptr(), ws.data_ptr(),
                  terms=dt.data_ptr(), step_log=log.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    weights[...] = dw.cpu().numpy().reshape(weights.shape); critic[...] = dc.cpu().numpy().reshape(critic.shape)
    adam[...] = da.cpu().numpy().reshape(adam.shape); adam_step[...] = ds.cpu().numpy().reshape(adam_step.shape)
    return log.cpu().numpy()


# the training arrays of dart_lmpc_train_buffers behind those of dart_lmpc_collect_dev, in the struct's order
LMPC_TRAIN_ARRAYS = ("adam", "adam_step", "train_log", "best_return", "best_weights", "best_iter", "workspace")
TRAIN_LOG_COLS = 12
TRAIN_LOG_FIELDS = ("n", "episodes_ended", "mean_return", "max_return", "mean_step_reward", "status_nonzero",
                    "policy_loss", "value_loss", "entropy", "nrec_mismatch", "best_return", "snapshot")
_TRAIN_NPTR = 6 + len(LMPC_LOOP_STATE) + len(LMPC_COLLECT_STATE) + len(LMPC_COLLECT_POOL) + len(LMPC_LOOP_LOGS) \
    + len(LMPC_COLLECT_LOGS) + len(LMPC_COLLECT_REC) + len(LMPC_TRAIN_ARRAYS)


def _train_buffers(values):
    """``struct dart_lmpc_train_buffers`` (pointers only, so an array of pointers has its layout) from addresses
    (ints, 0 / None: NULL) in the struct's order."""
    if len(values) != _TRAIN_NPTR:
        raise DartMPCError(f"dart_lmpc_train_buffers has {_TRAIN_NPTR} pointers, got {len(values)}")
    return (ctypes.c_void_p * _TRAIN_NPTR)(*[int(v) if v else None for v in values])


def _train_dev(solver, entry, who, gbuf, B, reset_rows, target, prm, plant_pvec, current_k, weights, critic, state,
               cstate, logs, clogs, rec, train, pcfg, rcfg, ppo_cfg, tcfg, pool, plant, stream, hyper=()):
    """The device training entries of ``LmpcSolver``: ``entry`` names the C function, ``who`` is () or (P, seeds),
    ``gbuf`` () or (the ``global_buffer`` struct or None,) and ``hyper`` () or (the table's device pointer or 0,), each
    passed where the entry takes it.  (``solver`` is any handle's wrapper: the library refuses one that is not an LMPC
    handle.)"""
    if who:
        P, seeds = who
        seeds = None if seeds is None else np.ascontiguousarray(seeds, np.uint64).reshape(-1)
        if seeds is not None and seeds.size != int(P):
            raise DartMPCError(f"{entry} needs {P} seeds, got {seeds.size}")
        who = (int(P), _ptr(seeds))
    plant = plant or plant_config()
    buf = _train_buffers([target, prm, plant_pvec, current_k, weights, critic]
                         + [state[n] for n, _, _ in LMPC_LOOP_STATE] + [cstate[n] for n, _, _ in LMPC_COLLECT_STATE]
                         + [(pool or {}).get(n, 0) for n, _, _ in LMPC_COLLECT_POOL]
                         + [logs[n] for n, _, _ in LMPC_LOOP_LOGS] + [clogs[n] for n, _, _ in LMPC_COLLECT_LOGS]
                         + [rec[n] for n, _, _ in LMPC_COLLECT_REC] + [train[n] for n in LMPC_TRAIN_ARRAYS])
    rc = getattr(lib(), "dart_lmpc_" + entry)(
        solver._h, ctypes.byref(plant), ctypes.byref(pcfg), ctypes.byref(rcfg), ctypes.byref(ppo_cfg),
        ctypes.byref(tcfg), *who, int(B), int(reset_rows), buf,
        *[ctypes.byref(g) if g is not None else None for g in gbuf], *[_vp(q) for q in hyper], stream or None)
    if rc != 0:
        solver._err(rc, "dart_lmpc_" + entry)


def train_config(**over) -> TrainConfig:
    """``dart_lmpc_train_config`` with the library's defaults, fields overridden by keyword."""
    c = TrainConfig()
    lib().dart_lmpc_train_config_default(ctypes.byref(c))
    names = [f[0] for f in c._fields_]
    for k, v in over.items():
        if k not in names:
            raise DartMPCError(f"TrainConfig has no field {k!r} (fields: {names})")
        setattr(c, k, float(v) if k in ("gamma", "lam") else int(v))
    return c


def train_workspace_bytes(B, K, record_every, epochs, mini_batch_size):
    """Bytes of the device workspace of ``LmpcSolver.train_dev``."""
    b = int(lib().dart_lmpc_train_workspace_bytes(int(B), int(K), int(record_every), int(epochs), int(mini_batch_size)))
    if b == 0:
        raise DartMPCError(f"no training workspace for B = {B}, K = {K}, record_every = {record_every}, epochs = "
                           f"{epochs}, mini_batch_size = {mini_batch_size} (K a positive multiple of record_every)")
    return b


POP_MAX = 32                    # DART_LMPC_POP_MAX: learners per population
POP_CRITIC_STRIDE = 37572       # DART_LMPC_POP_CRITIC_STRIDE: floats between the critics of a population (16-byte rows)


def train_pop_workspace_bytes(P, B, K, record_every, epochs, mini_batch_size):
    """Bytes of the device workspace of ``LmpcSolver.train_pop_dev``; 0 for a bad shape."""
    return int(lib().dart_lmpc_train_pop_workspace_bytes(int(P), int(B), int(K), int(record_every), int(epochs),
                                                         int(mini_batch_size)))


def philox_dev(n, inputs, out, stream=0):
    """dart_lmpc_philox_dev: Philox4x32-10 on ``inputs`` [n, 6] uint32 (counter[4], key[2]) into ``out`` [n, 4]
    (device pointers)."""
    _rc(lib().dart_lmpc_philox_dev(int(n), _vp(inputs), _vp(out), stream or None), "dart_lmpc_philox_dev")


def noise_dev(seed, iteration, steps, B, noise_out, stream=0):
    """dart_lmpc_noise_dev: the standard-normal draws [steps, B, 34] (fp32) of (seed, iteration) (device pointer)."""
    _rc(lib().dart_lmpc_noise_dev(int(seed), int(iteration), int(steps), int(B), _vp(noise_out), stream or None),
        "dart_lmpc_noise_dev")


def noise(seed, iteration, steps, B):
    """The exploration noise of (seed, iteration) from the device generator (dart_lmpc_noise, blocking): float32
    [steps, B, 34], the array ``LmpcSolver.collect`` takes."""
    out = np.empty((int(steps), int(B), 34), np.float32)
    _rc(lib().dart_lmpc_noise(int(seed), int(iteration), int(steps), int(B), _ptr(out)), "dart_lmpc_noise")
    return out


def perms_dev(seed, iteration, epochs, n, perm_out, key_out=0, stream=0):
    """dart_lmpc_perms_dev: the mini-batch permutations [epochs, n] (int32) of (seed, iteration); ``key_out``
    [epochs, n] (uint32, optional) receives the raw keys (device pointers)."""
    _rc(lib().dart_lmpc_perms_dev(int(seed), int(iteration), int(epochs), int(n), _vp(perm_out), _vp(key_out),
                                  stream or None), "dart_lmpc_perms_dev")


def perms(seed, iteration, epochs, n, want_keys=False):
    """The permutations of (seed, iteration) from the device generator (dart_lmpc_perms, blocking): int32
    [epochs, n], and with ``want_keys`` the uint32 keys they sort."""
    out = np.empty((int(epochs), int(n)), np.int32)
    keys = np.empty((int(epochs), int(n)), np.uint32) if want_keys else None
    _rc(lib().dart_lmpc_perms(int(seed), int(iteration), int(epochs), int(n), _ptr(out), _ptr(keys)), "dart_lmpc_perms")
    return (out, keys) if want_keys else out


# ---- the global-buffer update (rlmpc2.py:823-874) ----
GLOBAL_LOG_COLS = 6
GLOBAL_LOG_FIELDS = ("global_fill", "global_update", "global_rows", "global_policy_loss", "global_value_loss",
                     "global_entropy")
# the buffer's arrays in the struct's order: (name, row width, dtype)
LMPC_GLOBAL_ARRAYS = (("obs", 520, np.float32), ("action", 34, np.float32), ("logp", 0, np.float32),
                      ("value", 0, np.float32), ("reward", 0, np.float64), ("done", 0, np.float32))


def perms_stream_dev(seed, iteration, rng_stream, epochs, n, perm_out, key_out=0, stream=0):
    """dart_lmpc_perms_stream_dev: ``perms_dev`` with the generator's stream index given (1: the local update's
    permutations, 3: the global update's)."""
    _rc(lib().dart_lmpc_perms_stream_dev(int(seed), int(iteration), int(rng_stream), int(epochs), int(n),
                                         _vp(perm_out), _vp(key_out), stream or None), "dart_lmpc_perms_stream_dev")


def choice_dev(seed, iteration, n, m, choice_out, stream=0):
    """dart_lmpc_choice_dev: ``m`` of ``n`` without replacement (int32 [m]) for (seed, iteration): the first m
    entries of the generator's permutation on stream 2 (device pointer)."""
    _rc(lib().dart_lmpc_choice_dev(int(seed), int(iteration), int(n), int(m), _vp(choice_out), stream or None),
        "dart_lmpc_choice_dev")


def choice(seed, iteration, n, m):
    """The choice of (seed, iteration) from the device generator (dart_lmpc_choice, blocking): int32 [m]."""
    out = np.empty(max(int(m), 0), np.int32)
    _rc(lib().dart_lmpc_choice(int(seed), int(iteration), int(n), int(m), _ptr(out)), "dart_lmpc_choice")
    return out


def global_rows(n):
    """(m, G) of dart_lmpc_global_rows: m = max(1, n // 4) records are drawn per iteration, and the global buffer is
    updated on when it holds G = ceil(n / m) m rows (its capacity)."""
    m, G = ctypes.c_int32(), ctypes.c_int32()
    _rc(lib().dart_lmpc_global_rows(int(n), ctypes.byref(m), ctypes.byref(G)), "dart_lmpc_global_rows")
    return int(m.value), int(G.value)


def global_fill_after(n, fill, iterations):
    """The global buffer's fill after ``iterations`` more iterations (dart_lmpc_global_fill_after, host arithmetic)."""
    f = int(lib().dart_lmpc_global_fill_after(int(n), int(fill), int(iterations)))
    if f < 0:
        raise DartMPCError(f"no global fill for n = {n}, fill = {fill}, iterations = {iterations} "
                           f"(fill a multiple of m in [0, n))")
    return f


def global_workspace_bytes(n, epochs, mini_batch_size):
    """Bytes of the device workspace of the global update (``LmpcSolver.train_global_dev``)."""
    b = int(lib().dart_lmpc_global_workspace_bytes(int(n), int(epochs), int(mini_batch_size)))
    if b == 0:
        raise DartMPCError(f"no global workspace for n = {n}, epochs = {epochs}, mini_batch_size = {mini_batch_size}")
    return b


def global_pop_workspace_bytes(P, n, capacity, epochs, mini_batch_size):
    """Bytes of the device workspace of a population's global update (``LmpcSolver.train_pop_global_dev``) for P
    buffers of ``capacity`` rows; 0 for a bad shape."""
    return int(lib().dart_lmpc_global_pop_workspace_bytes(int(P), int(n), int(capacity), int(epochs),
                                                          int(mini_batch_size)))


def choice_pop_dev(seeds, iteration, n, m, choice_out, stream=0):
    """dart_lmpc_choice_pop_dev: ``choice_dev`` for every seed of ``seeds`` in one launch, int32 [P, m]."""
    seeds = np.ascontiguousarray(seeds, np.uint64).reshape(-1)
    _rc(lib().dart_lmpc_choice_pop_dev(int(seeds.size), _ptr(seeds), int(iteration), int(n), int(m), _vp(choice_out),
                                       stream or None), "dart_lmpc_choice_pop_dev")


def global_append_pop_dev(g, P, m, n, rec_total, sample, choice, rec, stream=0):
    """dart_lmpc_global_append_pop_dev: ``global_append_dev`` for P learners in one launch; ``g`` holds the P buffers
    stacked ``g.capacity`` rows apart, ``sample`` is [P, n] and ``choice`` [P, m]."""
    _rc(lib().dart_lmpc_global_append_pop_dev(ctypes.byref(g), int(P), int(m), int(n), int(rec_total), _vp(sample),
                                              _vp(choice), *[_vp(rec[k]) for k, _, _ in LMPC_COLLECT_REC],
                                              stream or None), "dart_lmpc_global_append_pop_dev")


def gae_seq_pop_dev(P, capacity, G, gamma, lam, reward, value, done, last_value, adv, ret, stream=0):
    """dart_lmpc_gae_seq_pop_dev: ``gae_seq_dev`` for P sequences in one launch, arrays [P, capacity],
    ``last_value`` [P]."""
    _rc(lib().dart_lmpc_gae_seq_pop_dev(int(P), int(capacity), int(G), float(gamma), float(lam), _vp(reward),
                                        _vp(value), _vp(done), _vp(last_value), _vp(adv), _vp(ret), stream or None),
        "dart_lmpc_gae_seq_pop_dev")


def global_buffer(arrays, capacity, fill, global_log=0, workspace=0) -> GlobalBuffer:
    """``struct dart_lmpc_global_buffer`` from addresses (ints): ``arrays`` maps obs, action, logp, value, reward,
    done to device (or host) pointers of ``capacity`` rows."""
    g = GlobalBuffer()
    for name, _, _ in LMPC_GLOBAL_ARRAYS:
        setattr(g, name, int(arrays[name]) or None)
    g.capacity, g.fill = int(capacity), int(fill)
    g.global_log, g.workspace = int(global_log) or None, int(workspace) or None
    return g


def _host_global(buf, need_log_rows=None, global_log=None, learners=1):
    """GlobalBuffer over the host arrays of a ``ppo.new_global_buffer`` dict (checked: dtype, size, contiguity);
    ``learners`` > 1: of a ``ppo.new_population_global_buffer`` dict, ``learners`` buffers stacked."""
    total = int(np.asarray(buf["logp"]).size)
    if learners < 1 or total % learners:
        raise DartMPCError(f"global_buffer: {total} rows are not {learners} buffers of equal capacity")
    cap = total // learners
    ptrs = {}
    for name, width, dt in LMPC_GLOBAL_ARRAYS:
        ptrs[name] = _inplace(buf[name], dt, total * max(width, 1), "global_buffer[%r]" % name).ctypes.data
    log = 0
    if need_log_rows is not None:
        log = _inplace(global_log, np.float64, GLOBAL_LOG_COLS * need_log_rows, "global_log").ctypes.data
    return global_buffer(ptrs, cap, int(buf["fill"]), global_log=log)


def global_append_dev(g, m, n, rec_total, sample, choice, rec, stream=0):
    """dart_lmpc_global_append_dev: rows ``g.fill`` .. ``g.fill + m - 1`` of the buffer ``g`` (``global_buffer``)
    <- records ``sample[choice[j]]``; ``rec`` maps the names of LMPC_COLLECT_REC to device pointers."""
    _rc(lib().dart_lmpc_global_append_dev(ctypes.byref(g), int(m), int(n), int(rec_total), _vp(sample), _vp(choice),
                                          *[_vp(rec[k]) for k, _, _ in LMPC_COLLECT_REC], stream or None),
        "dart_lmpc_global_append_dev")


def global_append(buf, sample, choice, rec):
    """The record gather on host arrays (dart_lmpc_global_append, blocking): the rows ``buf['fill']`` .. of the
    ``ppo.new_global_buffer`` dict ``buf`` receive records ``sample[choice[j]]`` of ``rec`` (the record arrays
    [rec_rows, B, ..]); ``buf['fill']`` advances by ``len(choice)``."""
    sample = np.ascontiguousarray(sample, np.int32).reshape(-1)
    choice = np.ascontiguousarray(choice, np.int32).reshape(-1)
    total = int(np.asarray(rec["rec_logp"]).size)
    r = [np.ascontiguousarray(rec[k], dt).reshape(total, max(w, 1)) for k, w, dt in LMPC_COLLECT_REC]
    g = _host_global(buf)
    _rc(lib().dart_lmpc_global_append(ctypes.byref(g), choice.size, sample.size, total, _ptr(sample), _ptr(choice),
                                      *[_ptr(a) for a in r]), "dart_lmpc_global_append")
    buf["fill"] = int(buf["fill"]) + choice.size


def gae_seq_dev(G, gamma, lam, reward, value, done, last_value, adv, ret, stream=0):
    """dart_lmpc_gae_seq_dev: compute_gae over rows 0 .. G-1 as one chain (device pointers)."""
    _rc(lib().dart_lmpc_gae_seq_dev(int(G), float(gamma), float(lam), _vp(reward), _vp(value), _vp(done),
                                    _vp(last_value), _vp(adv), _vp(ret), stream or None), "dart_lmpc_gae_seq_dev")


def gae_seq(reward, value, done, last_value, gamma=0.99, lam=0.95):
    """compute_gae over one sequence on the GPU (dart_lmpc_gae_seq, blocking): (adv, ret = adv + value), float64
    [G]."""
    rw = np.ascontiguousarray(reward, np.float64).reshape(-1)
    G = rw.size
    vl, dn = (np.ascontiguousarray(a, np.float32).reshape(G) for a in (value, done))
    lv = np.ascontiguousarray(last_value, np.float32).reshape(1)
    adv, ret = np.full(G, np.nan), np.full(G, np.nan)
    _rc(lib().dart_lmpc_gae_seq(G, float(gamma), float(lam), _ptr(rw), _ptr(vl), _ptr(dn), _ptr(lv), _ptr(adv),
                                _ptr(ret)), "dart_lmpc_gae_seq")
    return adv, ret


def mean_param_update_dev(pcfg, B, weights, history, model_params, current_k, mean_out=0, stream=0):
    """dart_lmpc_mean_param_update_dev: the mean-based parameter write of rlmpc2.py:876-896 (device pointers)."""
    _rc(lib().dart_lmpc_mean_param_update_dev(ctypes.byref(pcfg), int(B), _vp(weights), _vp(history), _vp(model_params),
                                              _vp(current_k), _vp(mean_out), stream or None),
        "dart_lmpc_mean_param_update_dev")


def mean_param_update(pcfg, weights, history, model_params, current_k):
    """The mean-based parameter write on host arrays (dart_lmpc_mean_param_update, blocking): ``model_params`` and
    ``current_k`` [B, 34] (float64) are updated in place; returns the actor's mean, float32 [B, 34]."""
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.size != ACTOR_NWEIGHTS:
        raise DartMPCError(f"policy weights have {w.size} floats, not {ACTOR_NWEIGHTS}")
    hist = np.ascontiguousarray(history, np.float32).reshape(-1, 520)
    B = hist.shape[0]
    _inplace(model_params, np.float64, 34 * B, "model_params"); _inplace(current_k, np.float64, 34 * B, "current_k")
    mean = np.empty((B, 34), np.float32)
    _rc(lib().dart_lmpc_mean_param_update(ctypes.byref(pcfg), B, _ptr(w), _ptr(hist), _ptr(model_params),
                                          _ptr(current_k), _ptr(mean)), "dart_lmpc_mean_param_update")
    return mean


def critic_value_dev(n, critic, obs, value_out, stream=0):
    """dart_lmpc_critic_value_dev: value_net on obs [n, 520] into value_out [n] (device pointers)."""
    _rc(lib().dart_lmpc_critic_value_dev(int(n), _vp(critic), _vp(obs), _vp(value_out), stream or None),
        "dart_lmpc_critic_value_dev")


def critic_value(critic, obs):
    """value_net (Policy :48-55) on obs [n, 520] on the GPU (dart_lmpc_critic_value, blocking): float32 [n]."""
    cw = np.ascontiguousarray(critic, np.float32).reshape(-1)
    if cw.size != CRITIC_NWEIGHTS:
        raise DartMPCError(f"critic weights have {cw.size} floats, not {CRITIC_NWEIGHTS}")
    ob = np.ascontiguousarray(obs, np.float32).reshape(-1, 520)
    out = np.empty(ob.shape[0], np.float32)
    _rc(lib().dart_lmpc_critic_value(ob.shape[0], _ptr(cw), _ptr(ob), _ptr(out)), "dart_lmpc_critic_value")
    return out


def rls_update_batch(theta, P, phi, y, lam=0.995):
    """Batched RLS.update on the GPU (B filters of p = 7).  Returns updated (theta[B,7], P[B,7,7])."""
    th = np.ascontiguousarray(theta, np.float64).reshape(-1, 7).copy()
    B = th.shape[0]
    Pm = np.ascontiguousarray(P, np.float64).reshape(B, 7, 7).copy()
    ph = np.ascontiguousarray(phi, np.float64).reshape(B, 7)
    yy = np.ascontiguousarray(y, np.float64).reshape(B)
    rc = lib().dart_rls_update_batch(B, _ptr(th), _ptr(Pm), _ptr(ph), _ptr(yy), float(lam))
    if rc != 0:
        raise DartMPCError(f"dart_rls_update_batch failed ({rc})")
    return th, Pm
