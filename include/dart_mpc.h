/*
 * dart_mpc.h -- C ABI of the MI355X-native batched tray-tilt NMPC solver.
 *
 * This is the drop-in boundary for DART's per-timestep MPC solve.  Each entry
 * point replaces one reference interface (paths relative to the reference root):
 *
 *   dart_mpc_create        <- PMPC.__init__ building the CasADi NLP and
 *                             ca.nlpsol('solver','ipopt',...)
 *                             PMPC/src/controller/mpc_3d.py:12-85 (:82)
 *   dart_mpc_solve_batch   <- PMPC.solve(target) -> (U_opt[0], loss), one call
 *                             per instance today: mpc_3d.py:115-138, called from
 *                             the worker loop PMPC/main_parallel_enhanced.py:51-53
 *   dart_mpc_solve_batch_dev  same, with device-resident inputs/outputs
 *   dart_rmpc_solve_batch(_dev) <- AdaptiveNPMPCSmooth.solve + the driver's RLS updates
 *                             RMPC/dev_dual/controller/np_mpc_adaptive_with_linear_regressor.py
 *                             :212-222 (RLS :10-30), RMPC/dev_dual/rob_ctrl.py:335-352
 *   dart_lmpc_solve_batch(_dev) <- the solve of RLMPC._solver_worker
 *                             LMPC/src/controller/rlmpc2.py:229-533 (NLP :239-491, solver call
 *                             and warm start :510-520), fed by RLMPC.solve :986-1021
 *   dart_lmpc_policy_step(_dev) <- the inference / parameter-write half of RLMPC._rl_worker
 *                             rlmpc2.py:537-769 (Policy :33-80, write_params_to_shm :606-616)
 *   dart_lmpc_policy_solve_batch(_dev) <- one control step of the LMPC stack: the policy step
 *                             above, then the solve with the parameters it wrote
 *                             (views["model_params"], rlmpc2.py:506-515), in ONE launch
 *   dart_arm_solve_batch(_dev) <- ARMCONTROL.solver_worker, the per-arm impedance QP
 *                             PMPC/src/controller/arm.py:266-457 (same code in
 *                             RMPC/dev_dual/controller/parallel.py, LMPC/src/controller/parallel.py),
 *                             fed by ARMCONTROL.compute_torque / compute_dynamics :111-231
 *   dart_mpc_sync / dart_mpc_last_error / dart_mpc_destroy
 *                           <- process-lifetime handling of the solver object in
 *                             mpc_worker (main_parallel_enhanced.py:22-55)
 *
 * Plain C types only: no torch, no HIP types in signatures (streams are void*).
 *
 * Layouts (row-major, fp64):
 *   x0  [B][6]  state  [px, vx, py, vy, pz, vz]             (mpc_3d.py:106-113)
 *   ref [B][6]  target [px, vx, py, vy, pz, vz]             (mpc_3d.py:34, P[nx:])
 *   prm [B][6]  [mu, Qp, Qv, R, u_lo, u_hi]                 (mpc_3d.py:12 ctor args)
 *   w   [B][nw] decision vector in the reference order: x_0..x_N (6 each) then
 *               u_0..u_{N-1} (2 each), nw = 6(N+1) + 2N     (mpc_3d.py:69)
 *   u0  [B][2]  first control U_opt[0] = [theta_x, theta_y] (mpc_3d.py:137-138)
 *   f   [B]     objective value at the solution ("loss")    (mpc_3d.py:134)
 *   status[B]   DART_MPC_SOLVED (0), DART_MPC_MAXITER (-1), DART_MPC_LS_FAIL (-2),
 *               DART_MPC_INERTIA_FAIL (-3), DART_MPC_MAXTIME (-4, LMPC's max_cpu_time),
 *               DART_MPC_INFEASIBLE (2, RMPC / LMPC: the restoration phase converged to local
 *               infeasibility, e.g. an RMPC start with a measured |v| above vmax at the pinned node 0).
 *               As in the reference (which never
 *               checks IPOPT's status, mpc_3d.py:133-138) u0 is written anyway.
 *   iters[B]    interior-point iterations taken.
 *
 * Errors: every int-returning call returns 0 on success or a negative
 * DART_MPC_E* code; dart_mpc_last_error() describes the last failure.
 * Threading: every entry taking a handle locks the handle's mutex, so several
 * host threads may share one handle (the reference calls its controllers from
 * background threads, RMPC/dev_dual/controller/convimp.py:435): their calls
 * take turns on the handle's staging buffers and stream.  For calls that run
 * side by side, give each thread its own handle.  The stateless entries (RLS,
 * arm QP, policy step) lock a per-device stage the same way.
 */
#ifndef DART_MPC_H
#define DART_MPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DART_MPC_ABI_VERSION 8

enum dart_mpc_variant {
    DART_MPC_PMPC = 0,      /* PMPC/src/controller/mpc_3d.py, N <= 63 */
    DART_MPC_RMPC = 1,      /* RMPC/dev_dual/controller/np_mpc_adaptive_with_linear_regressor.py, N <= 63 */
    DART_MPC_LMPC = 2       /* LMPC/src/controller/rlmpc2.py, N <= 63 */
};

enum dart_mpc_status {
    DART_MPC_SOLVED = 0,
    DART_MPC_ACCEPTABLE = 1,       /* IPOPT "Solved To Acceptable Level" (LMPC: acceptable_tol / _iter) */
    DART_MPC_INFEASIBLE = 2,       /* IPOPT "Infeasible Problem Detected" (RMPC / LMPC: the restoration phase converged) */
    DART_MPC_MAXITER = -1,
    DART_MPC_LS_FAIL = -2,         /* IPOPT "Restoration Failed" (or the failed line search, restoration = 0) */
    DART_MPC_INERTIA_FAIL = -3,
    DART_MPC_MAXTIME = -4          /* IPOPT "Maximum CpuTime Exceeded" (LMPC: dart_mpc_config.max_cpu_time, ABI 7) */
};

enum dart_mpc_error {
    DART_MPC_OK = 0,
    DART_MPC_EINVAL = -1,     /* bad argument (null pointer, N out of range, B > B_max) */
    DART_MPC_EHIP = -2,       /* HIP runtime error (message in dart_mpc_last_error) */
    DART_MPC_ENODEV = -3      /* no usable gfx950 device */
};

/* Solver configuration.  Defaults (dart_mpc_config_default) follow the
 * reference: N = 20 (mpc_3d.py:12), Ts = 0.002 (MuJoCo default timestep),
 * IPOPT tol = 1e-8 and max_iter = 3000 (IPOPT defaults; mpc_3d.py:82 sets
 * neither), gravity = -9.81 (world xml line 5). */
typedef struct dart_mpc_config {
    int32_t variant;    /* enum dart_mpc_variant */
    int32_t N;          /* horizon, 1 <= N <= 63 */
    double Ts;          /* sampling time [s] */
    double tol;         /* IPOPT-style scaled optimality tolerance */
    int32_t max_iter;   /* interior-point iteration cap (>= 1; PMPC also 0: the start point at status -1) */
    int32_t B_max;      /* largest batch the handle's device workspace serves */
    double gravity;     /* model.opt.gravity[2] (mpc_3d.py:23), default -9.81 */
    double acceptable_tol;   /* IPOPT acceptable_tol; used by LMPC (rlmpc2.py:487: 1e-3) */
    int32_t acceptable_iter; /* IPOPT acceptable_iter, 0 = off; used by LMPC (rlmpc2.py:488: 5) */
    int32_t max_soc;    /* IPOPT max_soc (second-order corrections per line search), default 4, 0 = off,
                           <= 8; used by PMPC, LMPC and RMPC's restoration phase (the reference leaves
                           IPOPT's default, mpc_3d.py:82, np_mpc...:158-162, rlmpc2.py:480-489) */
    int32_t pmpc_path;  /* PMPC only (ABI 5): 0 = IPOPT's path on the full 6-state NLP (default; the z
                           defect rows of mpc_3d.py:37, :48 in theta, the filter, the error measures and
                           the second-order correction); 1 = the reduced (x, y) path, opt-in: same KKT
                           point to the tolerance, fewer iterations, but not IPOPT's iterates */
    int32_t restoration;  /* LMPC (ABI 6), RMPC and PMPC (ABI 8): 1 = IPOPT's soft restoration and
                           restoration phases after a failed filter line search (default;
                           MinC_1NrmRestorationPhase, the fallback of every nlpsol call, mpc_3d.py:82,
                           np_mpc...:158-162, rlmpc2.py:480-489); 0 = stop with status -2 there.  PMPC and
                           LMPC batches of at most 32 with N <= 31 run them in the solving wave (unless the
                           environment sets DART_RESTO_FUSE=0); larger batches, N > 31 (the two-wave builds)
                           and RMPC hand the failed instances to a second kernel queued on the same stream.
                           PMPC: on
                           IPOPT's path; for N > 31 the soft phase only (the restoration phase proper and the
                           reduced path keep -2).  RMPC / LMPC: at every N */
    double constr_mult_init_max;  /* IPOPT constr_mult_init_max (default 1000): the starting equality
                           multipliers are IPOPT's least-square estimate unless its max norm exceeds this
                           (then 0); 0 = always start from 0.  Used by PMPC, RMPC and LMPC */
    double max_cpu_time;  /* LMPC (ABI 7): IPOPT max_cpu_time [s], default 0.05 (rlmpc2.py:485): a solve
                           that is still running when this much wall-clock time has passed since its
                           instance started ends with status -4 (Maximum_CpuTime_Exceeded) and the current
                           iterate, checked where IPOPT checks it (after max_iter, each iteration and each
                           restoration iteration); measured on the GPU's 100 MHz constant clock; 0 = off */
} dart_mpc_config;

typedef struct dart_mpc_handle dart_mpc_handle;

void dart_mpc_config_default(dart_mpc_config *cfg);

int dart_mpc_create(const dart_mpc_config *cfg, int device, dart_mpc_handle **out);

/* Host-pointer entry: stages inputs to HBM, solves, copies results back and
 * blocks until they are in host memory.  It returns as soon as every
 * instance's results are visible in host memory, which can be a moment before
 * the stream retires the kernel; the next entry on the handle (or
 * dart_mpc_sync) settles that stream first and reports a late stream error as
 * the previous call's.  w_warm (nullable) is an initial
 * guess in the w layout; NULL = the reference's cold start (mpc_3d.py:123).
 * w_out is nullable. */
int dart_mpc_solve_batch(dart_mpc_handle *h, int B,
                         const double *x0, const double *ref, const double *prm,
                         const double *w_warm,
                         double *u0, double *f, double *w_out,
                         int32_t *status, int32_t *iters, void *hip_stream);

/* Resident solver (ABI 5, PMPC with pmpc_path 0 and N <= 31): dart_mpc_serve_start launches one
 * long-lived grid of B_serve waves on a stream of its own; every later dart_mpc_solve_batch on the
 * handle with B <= B_serve and a NULL stream is then served by it through a mailbox in mapped host
 * memory (inputs and outputs at fixed mapped addresses, completion words as before): no kernel
 * launch, no dispatch and a warm instruction cache per call; the results are bit-identical to a
 * launch.  Replaces nothing in the reference; it is the low-latency form of PMPC.solve's per-step
 * call (mpc_3d.py:115-138, main_parallel_enhanced.py:22-55).  The waves leave when
 * dart_mpc_serve_stop (or dart_mpc_destroy) is called, or after idle_timeout_s seconds without a
 * request (the next call then restarts the grid transparently).  dart_mpc_serve_running reports
 * whether the grid is resident.  Larger batches, caller streams and the _dev entry still launch. */
int dart_mpc_serve_start(dart_mpc_handle *h, int B_serve, double idle_timeout_s);

/* In-place I/O (ABI 5, PMPC): dart_mpc_bind returns host pointers into the handle's mapped, pinned
 * I/O area for B_max instances (any argument may be NULL): inputs x0 / ref / prm [B_max][6] and
 * w_warm [B_max][nw], outputs u0 [B_max][2], f, w_out [B_max][nw], status, iters.  A caller writes
 * the first B rows of the inputs in place and calls dart_mpc_solve_bound(h, B, flags); the results
 * are in the output views when it returns (blocking, like dart_mpc_solve_batch, served by the resident
 * solver when it runs).  No copy on either side of the call.  flags: DART_MPC_BOUND_W_WARM (use w_warm),
 * DART_MPC_BOUND_W_OUT (fill w_out).  The pointers stay valid until dart_mpc_destroy. */
#define DART_MPC_BOUND_W_WARM 1
#define DART_MPC_BOUND_W_OUT 2
int dart_mpc_bind(dart_mpc_handle *h, double **x0, double **ref, double **prm, double **w_warm,
                  double **u0, double **f, double **w_out, int32_t **status, int32_t **iters);
int dart_mpc_solve_bound(dart_mpc_handle *h, int B, int flags);
int dart_mpc_serve_stop(dart_mpc_handle *h);
int dart_mpc_serve_running(dart_mpc_handle *h);

/* Device-pointer entry: all pointers are device memory; asynchronous on
 * hip_stream (NULL = the handle's own stream).  Call dart_mpc_sync or
 * synchronise the stream before reading results. */
int dart_mpc_solve_batch_dev(dart_mpc_handle *h, int B,
                             const double *x0, const double *ref, const double *prm,
                             const double *w_warm,
                             double *u0, double *f, double *w_out,
                             int32_t *status, int32_t *iters, void *hip_stream);

/* RMPC (handle created with variant DART_MPC_RMPC).  Replaces
 * AdaptiveNPMPCSmooth.solve(x0, u_prev, theta_hat, Rref_flat)
 * (RMPC/dev_dual/controller/np_mpc_adaptive_with_linear_regressor.py:212-222) and, when
 * rls_P != NULL, the two RLS.update calls that precede it in the driver
 * (RMPC/dev_dual/rob_ctrl.py:335-343; RLS :10-30), fused into the same launch.
 *   x0 [B][4], u_prev [B][2]
 *   theta [B][14]   theta_hat = [theta_x(7); theta_y(7)]; with rls_P != NULL it is the RLS
 *                   estimate, updated in place before the solve
 *   rls_P [B][2][7][7] (nullable, in/out), rls_phi [B][7] = phi(prev state), rls_y [B][2] =
 *                   measured accelerations, rls_lambda = forgetting factor (0.995 in the driver)
 *   Rref [B][4(N+1)] staged reference (np_mpc...:201-210)
 *   prm [B][10] = [Qp, Qv, Ru, Rdu, u_lo, u_hi, du_lo, du_hi, vmax, v_eps]
 *   w_warm [B][4(N+1)+2N] (nullable: zeros, the reference's first call :168), w_out same layout
 *   (x_0..x_N then u_0..u_{N-1}, :144). */
int dart_rmpc_solve_batch(dart_mpc_handle *h, int B,
                          const double *x0, const double *u_prev, double *theta,
                          double *rls_P, const double *rls_phi, const double *rls_y, double rls_lambda,
                          const double *Rref, const double *prm, const double *w_warm,
                          double *u0, double *f, double *w_out,
                          int32_t *status, int32_t *iters, void *hip_stream);

int dart_rmpc_solve_batch_dev(dart_mpc_handle *h, int B,
                              const double *x0, const double *u_prev, double *theta,
                              double *rls_P, const double *rls_phi, const double *rls_y, double rls_lambda,
                              const double *Rref, const double *prm, const double *w_warm,
                              double *u0, double *f, double *w_out,
                              int32_t *status, int32_t *iters, void *hip_stream);

/* Number of fp64 entries of the RMPC w for horizon N: 4(N+1) + 2N. */
int dart_rmpc_nw(int N);

/* LMPC (handle created with variant DART_MPC_LMPC).  Replaces the solver call of
 * RLMPC._solver_worker (LMPC/src/controller/rlmpc2.py:510-520): one NLP per instance with
 *   state [B][8] = [px, vx, py, vy, theta_x, omega_x, theta_y, omega_y] (views["state"], :503)
 *   u_prev [B][2] (views["control"], the last applied control, :505)
 *   pvec [B][34] (views["model_params"], :506; squashed inside as |p| + 1e-6 where the
 *                 reference does, :296-344)
 *   target [B][8] (views["target"], :504)
 *   prm [B][22] = [Q(8), Qt(8), R(4), u_lo, u_hi]   (LMPC/src/run.py:118-121)
 *   w_warm [B][8(N+1)+2N] nullable (the worker's w0 <- w_opt, :492, :519), w_out same layout.
 * Termination follows IPOPT with the handle's tol, max_iter, acceptable_tol and acceptable_iter
 * (the reference: 1e-4, 50, 1e-3, 5); status DART_MPC_ACCEPTABLE when the acceptable test ends it. */
int dart_lmpc_solve_batch(dart_mpc_handle *h, int B,
                          const double *state, const double *u_prev, const double *pvec, const double *target,
                          const double *prm, const double *w_warm,
                          double *u0, double *f, double *w_out,
                          int32_t *status, int32_t *iters, void *hip_stream);

int dart_lmpc_solve_batch_dev(dart_mpc_handle *h, int B,
                              const double *state, const double *u_prev, const double *pvec, const double *target,
                              const double *prm, const double *w_warm,
                              double *u0, double *f, double *w_out,
                              int32_t *status, int32_t *iters, void *hip_stream);

/* Number of fp64 entries of the LMPC w for horizon N: 8(N+1) + 2N. */
int dart_lmpc_nw(int N);

/* LMPC parameter policy: the inference half of RLMPC._rl_worker
 * (LMPC/src/controller/rlmpc2.py:537-769) for B independent controllers, producing the
 * 34-vector model parameters the next solve reads (views["model_params"]).  Per call:
 * Welford-normalised observation [state, target, control, current_k] (:648-666), 10-step
 * history (:668-670), mean_net MLP 520 -> 64 -> 64 -> 34 with tanh (Policy :33-80, fp32),
 * raw action = mean + exp(clamp(log_std)) * noise (Normal.rsample, :674-680; noise [B][34] are
 * the standard-normal draws), and every update_every-th step the logit-space update
 * (:742-756, fp32) followed by the EMA + tanh soft clip of write_params_to_shm (:606-616).
 * Weights (fp32) are given input-major: W1[520][64], b1[64], W2[64][64], b2[64], W3[64][34],
 * b3[34], log_std[34] packed in this order (39748 floats); nn.Linear stores W transposed. */
typedef struct dart_lmpc_policy_config {
    int32_t update_every;      /* 8 (:742) */
    int32_t reserved;
    double max_delta;          /* max_delta_abs, 0.02 (LMPC/src/run.py:140) */
    double k_max;              /* max_param_abs, 2.0 (run.py:139) */
    double min_k;              /* 1e-2 (:560) */
    double k_ceiling_margin;   /* max(1e-3, 0.05 k_max) (:563) */
    double action_scale;       /* 1.0 (:564) */
    double smooth_alpha;       /* shm_smooth_alpha, 0.5 (:609) */
    double log_std_min;        /* log(policy_std_min = 1e-2) (:60) */
    double log_std_max;        /* log(policy_std_max = 2.0) (:61) */
} dart_lmpc_policy_config;

#define DART_LMPC_POLICY_NWEIGHTS 39748

void dart_lmpc_policy_config_default(dart_lmpc_policy_config *cfg);

/* Device pointers, asynchronous on hip_stream.  In/out: obs_mean[B][52], obs_M2[B][52],
 * obs_count[B], history[B][10][52] (fp32), timestep[B], model_params[B][34]; action_out
 * [B][34] (fp32) nullable. */
int dart_lmpc_policy_step_dev(const dart_lmpc_policy_config *cfg, int B, const float *weights,
                              const double *state, const double *target, const double *control,
                              const double *current_k, double *obs_mean, double *obs_M2, int32_t *obs_count,
                              float *history, int32_t *timestep, const float *noise, double *model_params,
                              float *action_out, void *hip_stream);

/* Host pointers (stages through device memory and blocks). */
int dart_lmpc_policy_step(const dart_lmpc_policy_config *cfg, int B, const float *weights,
                          const double *state, const double *target, const double *control,
                          const double *current_k, double *obs_mean, double *obs_M2, int32_t *obs_count,
                          float *history, int32_t *timestep, const float *noise, double *model_params,
                          float *action_out);

/* Fused LMPC control step (handle of variant DART_MPC_LMPC): for every instance, the policy
 * step of dart_lmpc_policy_step with control = u_prev (views["control"] is both the policy's
 * observation input, rlmpc2.py:650, and the solver's u_prev, :505), then the LMPC solve of
 * dart_lmpc_solve_batch with pvec = the model_params the step leaves behind (:506) -- one
 * kernel launch; the learned parameter net runs in the prologue of the kernel that evaluates the
 * shooting defects it parameterises (BASELINE.json config C5).  Results equal a policy step
 * followed by a solve.  Policy state arrays (obs_mean, obs_M2, obs_count, history, timestep,
 * model_params) are in/out as in dart_lmpc_policy_step; action_out nullable. */
int dart_lmpc_policy_solve_batch_dev(dart_mpc_handle *h, const dart_lmpc_policy_config *pcfg, int B,
                                     const float *weights, const double *state, const double *u_prev,
                                     const double *target, const double *current_k, double *obs_mean,
                                     double *obs_M2, int32_t *obs_count, float *history, int32_t *timestep,
                                     const float *noise, double *model_params, float *action_out,
                                     const double *prm, const double *w_warm,
                                     double *u0, double *f, double *w_out,
                                     int32_t *status, int32_t *iters, void *hip_stream);

/* Host pointers (stages through the handle's pinned buffers and blocks). */
int dart_lmpc_policy_solve_batch(dart_mpc_handle *h, const dart_lmpc_policy_config *pcfg, int B,
                                 const float *weights, const double *state, const double *u_prev,
                                 const double *target, const double *current_k, double *obs_mean,
                                 double *obs_M2, int32_t *obs_count, float *history, int32_t *timestep,
                                 const float *noise, double *model_params, float *action_out,
                                 const double *prm, const double *w_warm,
                                 double *u0, double *f, double *w_out,
                                 int32_t *status, int32_t *iters, void *hip_stream);

/* Batched standalone RLS.update (np_mpc...:17-27) for B independent p = 7 filters:
 * theta [B][7] and P [B][7][7] updated in place with regressors phi [B][7], targets y [B],
 * forgetting factor lambda.  The host entry stages through device memory and blocks. */
int dart_rls_update_batch(int B, double *theta, double *P, const double *phi, const double *y, double lambda);

/* Device of the stateless entries (dart_rls_update_batch*, dart_lmpc_policy_step*, dart_arm_solve_batch*)
 * for the calling thread: they run on the HIP current device.  Returns DART_MPC_ENODEV for a device
 * that does not exist.  (Handles carry their own device.) */
int dart_set_device(int device);
int dart_rls_update_batch_dev(int B, double *theta, double *P, const double *phi, const double *y, double lambda,
                              void *hip_stream);

/* Per-arm impedance QP: the body of ARMCONTROL.solver_worker (PMPC/src/controller/arm.py:266-457)
 * for B independent arm snapshots (two per dual-arm simulation step).  Stateless (no handle).
 *   snap [B][dart_arm_snapshot_len(n)] = the shared-memory fields the worker reads (:314-324):
 *        q[n] qd[n] qdd_prev[n] mocap_pos[3] ee_pos[3] rotvec[3] jac[6][n] jacDot[6][n] M[n][n]
 *        h[n] Mx_inv[6][6]
 *   prm  [B or 1][dart_arm_param_len(n)] = the worker's params (:290-302):
 *        Wimp[6][6] Wpos[n][n] Wsmooth[n][n] Qmin[n] Qmax[n] Qdotmin[n] Qdotmax[n] taumin[n]
 *        taumax[n] K[6][6] K_null[n][n] dt;   prm_stride = 0 shares one row across the batch,
 *        else dart_arm_param_len(n)
 *   qdd [B][n] the optimal joint accelerations (the next qdd_prev, :431), tau [B][n] = M qdd + h
 *   (torque_out, :424/:432), loss [B] = the objective value (loss_out, :425/:433),
 *   status [B] (DART_ARM_*), iters [B] interior-point iterations.
 * The QP is strictly convex (Wpos > 0); IPOPT's answer is its unique KKT point with the bounds
 * relaxed by bound_relax_factor = 1e-8, which is what the solver returns (scaled KKT error <= tol).
 * n <= DART_ARM_NMAX; bounds with |value| >= 1e19 are treated as absent (IPOPT's convention). */
#define DART_ARM_NMAX 8

enum dart_arm_status {
    DART_ARM_SOLVED = 0,
    DART_ARM_ACCEPTABLE = 1,     /* normal matrix lost definiteness with the KKT error <= acceptable_tol */
    DART_ARM_MAXITER = -1,
    DART_ARM_BREAKDOWN = -2,     /* a pivot of the normal matrix not positive above acceptable_tol (indefinite H), or a
                                  * non-finite (NaN / inf) entry in the snapshot or in the parameter row that reaches
                                  * the QP or the outputs: never a status >= 0.  iters is then 0, loss is NaN and qdd,
                                  * tau are not meaningful.  (A NaN bound is an absent bound.)  Other instances of the
                                  * batch are not affected. */
    DART_ARM_INFEASIBLE = -3     /* multipliers diverging: the bounds admit no qdd */
};

typedef struct dart_arm_config {
    double tol;                  /* scaled KKT tolerance, default 1e-10 */
    double acceptable_tol;       /* default 1e-7 */
    int32_t max_iter;            /* default 60 */
    int32_t reserved;
} dart_arm_config;

void dart_arm_config_default(dart_arm_config *cfg);
int dart_arm_snapshot_len(int n);
int dart_arm_param_len(int n);

/* Device pointers, asynchronous on hip_stream. */
int dart_arm_solve_batch_dev(const dart_arm_config *cfg, int B, int n, const double *snap, const double *prm,
                             int prm_stride, double *qdd, double *tau, double *loss, int32_t *status,
                             int32_t *iters, void *hip_stream);

/* Host pointers (stages through device memory and blocks). */
int dart_arm_solve_batch(const dart_arm_config *cfg, int B, int n, const double *snap, const double *prm,
                         int prm_stride, double *qdd, double *tau, double *loss, int32_t *status, int32_t *iters);

/* Arm rigid-body dynamics on the device (added within ABI 8: new entries only): ARMCONTROL.compute_dynamics
 * (PMPC/src/controller/arm.py:111-199) without MuJoCo, for a serial chain of n <= DART_ARM_NMAX hinge joints.
 *   model [B or 1][dart_arm_model_len(n) = 22 n + 18] (model_stride 0 shares one row):
 *        base_pos[3] base_quat[4] | per link: pos[3] quat[4] axis[3] armature damping mass com[3]
 *        inertia[6] (xx yy zz xy xz yz about the com, body frame) | ee_pos[3] ee_quat[4] offset gravity[3];
 *        quaternions (w, x, y, z) and axes are unit (dart_mpc.arm_model.ArmModel.row() normalises them)
 *   state [B][dart_arm_state_len(n) = 3 n + 7] = q[n] qd[n] qdd_prev[n] mocap_pos[3] mocap_quat[4]
 *   snap  [B][dart_arm_snapshot_len(n)] the row dart_arm_solve_batch reads; ee_quat [B][4] nullable.
 * jac is taken at the EE body's origin, ee_pos at origin + offset z; M is bit-symmetric; Mx_inv = J M^-1 J' by a
 * Cholesky factor (NaN on a non-positive pivot, which the QP reports as DART_ARM_BREAKDOWN); h is the bias force at
 * qdd = 0 (Coriolis, centrifugal, gravity; no damping).  jacdot_point selects the point jacDot differentiates:
 * DART_ARM_JACDOT_REFERENCE the world point (0, 0, offset) attached to the EE body (the reference's mj_jacDot call
 * read literally), DART_ARM_JACDOT_BODY the EE body origin.  Stateless; EINVAL before any device work for n < 1,
 * n > DART_ARM_NMAX, B < 1, a null pointer, a model_stride that is neither 0 nor the row length, an unknown
 * jacdot_point. */
#define DART_ARM_JACDOT_REFERENCE 0
#define DART_ARM_JACDOT_BODY 1
#define DART_ARM_NMETRIC 6

typedef struct dart_arm_dyn_config {
    int32_t jacdot_point;        /* DART_ARM_JACDOT_*, default DART_ARM_JACDOT_REFERENCE */
    int32_t reserved[7];
} dart_arm_dyn_config;

void dart_arm_dyn_config_default(dart_arm_dyn_config *cfg);
int dart_arm_model_len(int n);
int dart_arm_state_len(int n);

int dart_arm_dynamics_batch_dev(const dart_arm_dyn_config *dcfg, int B, int n, const double *model, int model_stride,
                                const double *state, double *snap, double *ee_quat, void *hip_stream);
int dart_arm_dynamics_batch(const dart_arm_dyn_config *dcfg, int B, int n, const double *model, int model_stride,
                            const double *state, double *snap, double *ee_quat);

/* Dynamics, then the unchanged QP launch on the same stream: state -> qdd, tau, loss, status, iters (as
 * dart_arm_solve_batch).  snap [B][dart_arm_snapshot_len(n)]: the snapshots in between (device entry: required, it
 * is the QP's input; host entry: nullable, copied back when set). */
int dart_arm_control_batch_dev(const dart_arm_dyn_config *dcfg, const dart_arm_config *cfg, int B, int n,
                               const double *model, int model_stride, const double *state, const double *prm,
                               int prm_stride, double *snap, double *qdd, double *tau, double *loss,
                               int32_t *status, int32_t *iters, void *hip_stream);
int dart_arm_control_batch(const dart_arm_dyn_config *dcfg, const dart_arm_config *cfg, int B, int n,
                           const double *model, int model_stride, const double *state, const double *prm,
                           int prm_stride, double *snap, double *qdd, double *tau, double *loss, int32_t *status,
                           int32_t *iters);

/* DACTL.control (PMPC/src/dualctl.py:22-66) for E experiments; instance 2 e + a is arm a (0 left, 1 right) of
 * experiment e.  tray_pose [E][7] (pos, quat); grasp [2][7] the grasp transforms (pos, quat) in the tray frame; the
 * mocap target of arm a is tray_pose o grasp[a], by quaternion products.  q, qd, qdd_prev [E][2][n]; models
 * [2][dart_arm_model_len(n)]; prm as dart_arm_solve_batch over the 2 E instances.  Outputs over the 2 E instances;
 * snap as dart_arm_control_batch; mocap [2 E][7] nullable: the targets. */
int dart_dual_arm_control_dev(const dart_arm_dyn_config *dcfg, const dart_arm_config *cfg, int E, int n,
                              const double *tray_pose, const double *grasp, const double *q, const double *qd,
                              const double *qdd_prev, const double *models, const double *prm, int prm_stride,
                              double *snap, double *mocap, double *qdd, double *tau, double *loss, int32_t *status,
                              int32_t *iters, void *hip_stream);
int dart_dual_arm_control(const dart_arm_dyn_config *dcfg, const dart_arm_config *cfg, int E, int n,
                          const double *tray_pose, const double *grasp, const double *q, const double *qd,
                          const double *qdd_prev, const double *models, const double *prm, int prm_stride,
                          double *snap, double *mocap, double *qdd, double *tau, double *loss, int32_t *status,
                          int32_t *iters);

/* Device-resident closed loop of the arm layer: `steps` steps of E dual-arm experiments on one stream, nothing on the
 * host in between.  Per step: tray pose -> mocap targets, dynamics with `models`, the QP, then this library's own
 * plant step with `plant_models` ([2][model_len]; not MuJoCo's integrator):
 *   (M_p + dt diag(d)) a = tau - h_p - d o qd,  qd += dt a,  q += dt qd      (d: the plant rows' damping)
 * with tau the QP's where status >= 0 and zero otherwise; qdd_prev becomes the QP's solution where status >= 0.
 *   tray_poses [tray_rows][E][7], tray_rows == steps or 1 (held)
 *   q, qd, qdd_prev [E][2][n] in / out;  metrics [2 E][DART_ARM_NMETRIC] in / out (zeros to start): final and largest
 *   |ee_pos - mocap_pos|, final |rotvec|, steps with status != 0, QP iterations, largest |tau_i| / taumax_i
 *   logs, all NULL (metrics only) or all set: q_log, qd_log, tau_log [steps][2 E][n] (the state the step's dynamics
 *   saw, the applied torque), ee_log [steps][2 E][3], loss_log [steps][2 E], status_log [steps][2 E]
 *   work (device entry): dart_dual_arm_work_len(E, n) doubles of device memory.
 * Two calls of K1 and K2 steps give the bits of one call of K1 + K2 steps. */
int dart_dual_arm_work_len(int E, int n);
int dart_dual_arm_rollout_dev(const dart_arm_dyn_config *dcfg, const dart_arm_config *cfg, int E, int n, int steps,
                              int tray_rows, const double *tray_poses, const double *grasp, const double *models,
                              const double *plant_models, const double *prm, int prm_stride, double *q, double *qd,
                              double *qdd_prev, double *metrics, double *work, double *q_log, double *qd_log,
                              double *tau_log, double *ee_log, double *loss_log, int32_t *status_log,
                              void *hip_stream);
int dart_dual_arm_rollout(const dart_arm_dyn_config *dcfg, const dart_arm_config *cfg, int E, int n, int steps,
                          int tray_rows, const double *tray_poses, const double *grasp, const double *models,
                          const double *plant_models, const double *prm, int prm_stride, double *q, double *qd,
                          double *qdd_prev, double *metrics, double *q_log, double *qd_log, double *tau_log,
                          double *ee_log, double *loss_log, int32_t *status_log);

/* Device-resident closed-loop rollouts (added within ABI 8: new entries only, nothing existing changes).
 * A K-step closed loop of B experiments on one stream with no host synchronisation between the steps: per step
 * one loop-step kernel (csrc/loop_step.hip) and the unchanged solve.  They do what the drivers do around a
 * solve -- RMPC/dev_dual/rob_ctrl.py:331-416 (RLS features and targets, reference governor, staged reference
 * np_mpc...:201-210, episode log, stop at the position tolerance) and the PMPC worker loop
 * PMPC/main_parallel_enhanced.py:290-419 (log, tilt -> quaternion :333-348) -- with the batched tray plant of
 * dart_mpc/harness.py (first-order tilt lag, the reference model plus Coulomb friction, RK4 at Ts) in place of
 * MuJoCo.  The launch sequence of a call is
 *     pre(k0), [solve, post(k) + pre(k+1)] for k = k0 .. k0+steps-2, solve, post(k0+steps-1)
 * The loop state is caller-owned device memory, in/out, so a rollout is continued by calling again with
 * k0 advanced; two calls of K1 and K2 steps give bit for bit what one call of K1 + K2 steps gives.
 *
 * RMPC state: x [B][6] plant state [px vx py vy pz vz], tilt [B][2], prev [B][4] (the previous measured state),
 *   u_prev [B][2], r_v [B][4] (governor), theta [B][14], P [B][2][7][7] (RLS), w [B][nw] (warm start: read and
 *   rewritten in place by every solve), done [B], nlog [B] (int32: episode closed; episode rows logged).
 *   A fresh rollout starts from x = [x0, 0, 0], prev = x0, P = P0 I and zeros elsewhere.
 * RMPC logs, [log_rows][B][...]: episode rows at index nlog[b], written while !done[b] (rob_ctrl.py:64-76):
 *   pos_err [2], pos_err_norm, u_cmd [2], timestep = k Ts; step rows at index k, always written: x [4] (the
 *   solve's x0), theta [14] (after the step's RLS update), r_v [4], f, status, iters (int32).
 * PMPC state: x [B][6], tilt [B][2]; logs at row k: X [6], U_cmd [2], quat_tray [4], loss, status, iters.
 * Rows that a call does not write keep their contents.  target / prm as in the solve entries; mu [B] is the
 * plant's viscous friction (PMPC: prm[0]); RMPC's feature scale v_eps is prm[9]. */
typedef struct dart_plant_config {
    double tau;     /* tilt lag time constant [s], 0.03; <= 0: the tilt follows the command at once */
    double mu_c;    /* Coulomb friction coefficient the MPC model does not have, 0.02 (not used by the LMPC plant) */
    double v_c;     /* its tanh velocity scale [m/s], 0.01 (not used by the LMPC plant) */
} dart_plant_config;

typedef struct dart_rmpc_loop_config {
    double dr_max;          /* governor step clip, 0.01 (rob_ctrl.py:346-348) */
    double alpha_rg;        /* governor gain, 0.5 */
    double step_fraction;   /* staged reference, 0.2 (rob_ctrl.py:351) */
    double rls_lambda;      /* RLS forgetting factor, 0.995 */
    double pos_tol;         /* episode ends below this position error [m], 0.01 (rob_ctrl.py:323) */
} dart_rmpc_loop_config;

void dart_plant_config_default(dart_plant_config *cfg);
void dart_rmpc_loop_config_default(dart_rmpc_loop_config *cfg);

/* One loop-step launch (for callers that sequence their own loop): post(k) if do_post, then pre of the next
 * step if do_pre.  The solve's per-step arrays are the caller's: pre writes x0 [B][4], Rref [B][4(N+1)],
 * phi [B][7], y [B][2]; post reads u0 [B][2], f, status, iters [B].  Device pointers, asynchronous. */
int dart_rmpc_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                            int B, int k, int do_post, int do_pre, int log_rows,
                            const double *target, const double *prm, const double *mu,
                            double *x, double *tilt, double *prev, double *u_prev, double *r_v, const double *theta,
                            int32_t *done, int32_t *nlog,
                            double *x0, double *Rref, double *phi, double *y,
                            const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                            double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                            double *log_x, double *log_theta, double *log_r_v, double *log_f,
                            int32_t *log_status, int32_t *log_iters, void *hip_stream);

int dart_pmpc_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                            int B, int k, int do_post, int do_pre, int log_rows, const double *prm,
                            double *x, double *tilt, double *x0,
                            const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                            double *log_X, double *log_U, double *log_quat, double *log_loss,
                            int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* `steps` closed-loop steps k0 .. k0+steps-1 (k0 + steps <= log_rows); steps = 0 does nothing.  Device
 * pointers, asynchronous on hip_stream (NULL = the handle's own).  The solve's per-step arrays live in the
 * handle (B <= B_max).  The RMPC solves are warm-started from w and fuse the RLS update; the PMPC solves are
 * cold-started, as in the reference. */
int dart_rmpc_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                          int B, int k0, int steps, int log_rows,
                          const double *target, const double *prm, const double *mu,
                          double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                          double *P, double *w, int32_t *done, int32_t *nlog,
                          double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                          double *log_x, double *log_theta, double *log_r_v, double *log_f,
                          int32_t *log_status, int32_t *log_iters, void *hip_stream);

int dart_pmpc_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                          int B, int k0, int steps, int log_rows, const double *target, const double *prm,
                          double *x, double *tilt,
                          double *log_X, double *log_U, double *log_quat, double *log_loss,
                          int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* Host pointers: state and logs are staged through device memory; blocks until they are back.  Of the logs
 * only the rows the call can write travel (the step rows k0 .. k0+steps-1, the episode rows from the smallest
 * nlog on). */
int dart_rmpc_rollout(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                      int B, int k0, int steps, int log_rows,
                      const double *target, const double *prm, const double *mu,
                      double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                      double *P, double *w, int32_t *done, int32_t *nlog,
                      double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                      double *log_x, double *log_theta, double *log_r_v, double *log_f,
                      int32_t *log_status, int32_t *log_iters, void *hip_stream);

int dart_pmpc_rollout(dart_mpc_handle *h, const dart_plant_config *plant,
                      int B, int k0, int steps, int log_rows, const double *target, const double *prm,
                      double *x, double *tilt,
                      double *log_X, double *log_U, double *log_quat, double *log_loss,
                      int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* Cross-plant closed loops (added within ABI 8): the PMPC and RMPC loops above on the plant of the LMPC loop below
 * (dart_mpc/harness.py LmpcPlant: the tilt lag of dart_plant_config.tau, then one RK4 step at Ts of the LMPC model
 * with the instance's true parameters plant_pvec [B][34]; mu_c / v_c are not used), so that the three controllers
 * can be compared on the same objects.  Same launch sequence, same handle-owned per-step arrays and the same
 * warm / cold starts as dart_rmpc_rollout_dev / dart_pmpc_rollout_dev; two calls of K1 and K2 steps give bit for bit
 * what one call of K1 + K2 steps gives, metrics included.
 *
 * State: x [B][8] = [px vx py vy th_x om_x th_y om_y] (LmpcPlant's layout) replaces x [B][6]; mu is gone.  tilt
 *   [B][2] keeps its meaning, the lagged command: tilt += a_lag (u - tilt).  The PMPC / RMPC command convention is
 *   a = g sin(theta) with g = -9.81 (mpc_3d.py:91-92) and the LMPC model has G = m g sin(a) with g = +9.81
 *   (rlmpc2.py:353-357), so the model's input is sin(-tilt): the next x is bit for bit what dart_lmpc_loop_step_dev
 *   computes for (x, -tilt, -u0, plant_pvec).  PMPC's solve sees x0 = [x[0..3], pz_vz]: pz_vz [B][2] is a constant
 *   input (the tray plant never moves pz, vz either).  RMPC's solve sees x[0..3] and prev as before.
 * metrics [B][8] (fp64, in/out; a fresh run starts from zeros with slot 1 = -1), updated by every post with
 *   e_k = |X_k[[0, 2]] - target[[0, 2]]| of the state that solve k saw:
 *     0 e of the last step                      4 steps with status != 0
 *     1 first k with e_k < 0.01, -1 while none  5 sum of iters
 *     2 sum of |u_k| Ts                         6 max of |th_x|, |th_y| over the states the solves saw
 *     3 max e_k                                 7 steps accumulated
 *   Slots 0 .. 2 are AsyncLogger's steady-state error, convergence step and control effort (logger.py:158-183).
 * Logs: the rows of the tray-plant entries (the state rows take x[0..3]; PMPC's log_X = [x[0..3], pz_vz]) plus
 *   log_rot [log_rows][B][4] = x[4..7].  Metrics-only mode: every log pointer NULL -- no log row is written,
 *   log_rows is not consulted, the host entries move no log; RMPC's done / nlog still advance.  Some log pointers
 *   NULL and others not is DART_MPC_EINVAL. */
int dart_pmpc_lm_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                               int B, int k, int do_post, int do_pre, int log_rows,
                               const double *target, const double *plant_pvec, const double *pz_vz,
                               double *x, double *tilt, double *metrics, double *x0,
                               const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                               double *log_X, double *log_U, double *log_quat, double *log_loss,
                               int32_t *log_status, int32_t *log_iters, double *log_rot, void *hip_stream);

int dart_rmpc_lm_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                               int B, int k, int do_post, int do_pre, int log_rows,
                               const double *target, const double *prm, const double *plant_pvec,
                               double *x, double *tilt, double *prev, double *u_prev, double *r_v, const double *theta,
                               int32_t *done, int32_t *nlog, double *metrics,
                               double *x0, double *Rref, double *phi, double *y,
                               const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                               double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                               double *log_x, double *log_theta, double *log_r_v, double *log_f,
                               int32_t *log_status, int32_t *log_iters, double *log_rot, void *hip_stream);

/* Device pointers, asynchronous on hip_stream (NULL = the handle's own). */
int dart_pmpc_lm_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                             int B, int k0, int steps, int log_rows,
                             const double *target, const double *prm, const double *plant_pvec, const double *pz_vz,
                             double *x, double *tilt, double *metrics,
                             double *log_X, double *log_U, double *log_quat, double *log_loss,
                             int32_t *log_status, int32_t *log_iters, double *log_rot, void *hip_stream);

int dart_rmpc_lm_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                             int B, int k0, int steps, int log_rows,
                             const double *target, const double *prm, const double *plant_pvec,
                             double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                             double *P, double *w, int32_t *done, int32_t *nlog, double *metrics,
                             double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                             double *log_x, double *log_theta, double *log_r_v, double *log_f,
                             int32_t *log_status, int32_t *log_iters, double *log_rot, void *hip_stream);

/* Host pointers: staged through device memory; blocks until state, metrics and (unless metrics-only) the rows of the
 * logs that the call can write are back. */
int dart_pmpc_lm_rollout(dart_mpc_handle *h, const dart_plant_config *plant,
                         int B, int k0, int steps, int log_rows,
                         const double *target, const double *prm, const double *plant_pvec, const double *pz_vz,
                         double *x, double *tilt, double *metrics,
                         double *log_X, double *log_U, double *log_quat, double *log_loss,
                         int32_t *log_status, int32_t *log_iters, double *log_rot, void *hip_stream);

int dart_rmpc_lm_rollout(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                         int B, int k0, int steps, int log_rows,
                         const double *target, const double *prm, const double *plant_pvec,
                         double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                         double *P, double *w, int32_t *done, int32_t *nlog, double *metrics,
                         double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                         double *log_x, double *log_theta, double *log_r_v, double *log_f,
                         int32_t *log_status, int32_t *log_iters, double *log_rot, void *hip_stream);

/* LMPC closed loop (handle of variant DART_MPC_LMPC; added within ABI 8).  What LMPC/src/run.py:256-286 does around
 * ctlr.solve -- the policy step and the warm-started solve (rlmpc2.py:494-524), the log, the plant step, the next
 * state -- with the plant of dart_mpc/harness.py (LmpcPlant) in place of MuJoCo: the first-order tilt lag of
 * dart_plant_config.tau, then one RK4 step at Ts of the LMPC model itself (safe_dynamics, rlmpc2.py:260-429) with
 * the lagged tilt as input and the instance's true parameters plant_pvec [B][34].  mu_c / v_c of dart_plant_config
 * are not used here: the model's Stribeck terms are its Coulomb friction.  The driver's u_cmd *= -1 and the
 * quaternion (run.py:257-261) are MuJoCo tray conventions and are not applied, as in the other two plants.  The
 * launch sequence of a call is that of the RMPC rollout,
 *     pre(k0), [solve launch(es), post(k) + pre(k+1)] for k = k0 .. k0+steps-2, solve launch(es), post(k0+steps-1)
 * where the solve launches are exactly what dart_lmpc_policy_solve_batch_dev enqueues for that B and N.
 *
 * State (caller-owned, in/out): x [B][8], tilt [B][2], u_prev [B][2], w [B][nw] (warm start; the final iterate of
 *   every call), and the policy state of dart_lmpc_policy_step: obs_mean, obs_M2 [B][52], obs_count [B],
 *   history [B][10][52] (fp32), timestep [B], model_params [B][34].  A fresh rollout starts from x = x0,
 *   model_params = current_k and zeros elsewhere.
 * Inputs: target [B][8], prm [B][22], plant_pvec [B][34], current_k [B][34], weights (DART_LMPC_POLICY_NWEIGHTS
 *   fp32), pcfg, noise [log_rows][B][34] fp32 (row k: the standard-normal draws of step k; NULL: zero noise).
 *   weights == NULL runs the loop without a policy: every solve uses model_params as a fixed pvec through
 *   dart_lmpc_solve_batch_dev; pcfg, current_k, noise and the other policy state arrays are then not read.
 * Logs [log_rows][B][...], row k: X [8] (the state the solve saw), U_cmd [2], pos_error (the norm of
 *   x_next[[0, 2]] - target[[0, 2]] after the plant step, run.py:274), pvec [34] (the parameter row the solve
 *   used), loss, status, iters (int32).  Rows that a call does not write keep their contents.
 * Two calls of K1 and K2 steps give bit for bit what one call of K1 + K2 steps gives. */

/* One loop-step launch: post(k) if do_post, then the next step's pre if do_pre.  pre writes the solve's state
 * [B][8]; post reads u0 [B][2], f, status, iters [B] and model_params, writes u_prev.  Device pointers, asynchronous. */
int dart_lmpc_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                            int B, int k, int do_post, int do_pre, int log_rows,
                            const double *target, const double *plant_pvec,
                            double *x, double *tilt, double *u_prev, const double *model_params, double *state,
                            const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                            double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                            int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* `steps` closed-loop steps k0 .. k0+steps-1 (k0 + steps <= log_rows); steps = 0 does nothing.  Device pointers,
 * asynchronous on hip_stream (NULL = the handle's own).  The solve's per-step arrays, two warm-start buffers the
 * solves alternate between (the first solve of a call reads w, the last writes it) and the zero noise row live in
 * the handle (B <= B_max). */
int dart_lmpc_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                          int B, int k0, int steps, int log_rows,
                          const double *target, const double *prm, const double *plant_pvec, const double *current_k,
                          const float *weights, const float *noise,
                          double *x, double *tilt, double *u_prev, double *w, double *obs_mean, double *obs_M2,
                          int32_t *obs_count, float *history, int32_t *timestep, double *model_params,
                          double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                          int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* Host pointers: state, inputs and logs are staged through device memory; blocks until they are back.  Of the
 * logs and of the noise only rows k0 .. k0+steps-1 travel. */
int dart_lmpc_rollout(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                      int B, int k0, int steps, int log_rows,
                      const double *target, const double *prm, const double *plant_pvec, const double *current_k,
                      const float *weights, const float *noise,
                      double *x, double *tilt, double *u_prev, double *w, double *obs_mean, double *obs_M2,
                      int32_t *obs_count, float *history, int32_t *timestep, double *model_params,
                      double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                      int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* LMPC evaluation (added within ABI 8: new entries only): the loop of dart_lmpc_rollout, unchanged in what it
 * computes per step (policy step, warm-started solve, plant step), with
 *   - the streaming metrics of the cross-plant loops, metrics [.][8] (fp64, in/out; same slots, see above; a fresh
 *     run starts from zeros with slot 1 = -1), updated by every post from what the logs would hold: e_k of the state
 *     that solve k saw (log_X row k) against target[[0, 2]], u0, status, iters, th_x = x[4], th_y = x[6];
 *   - logs that may be absent: the seven log pointers all NULL is the metrics-only mode (no log row is written, the
 *     host entry reserves and moves no log buffer), all set gives bit for bit the rows of dart_lmpc_rollout; some NULL
 *     and others not is DART_MPC_EINVAL.  log_rows still bounds k0 + steps (and the rows of the noise);
 *   - P weight sets in one call: P learners of B instances each, stacked learner-major (instance i = l B + b, as in
 *     dart_lmpc_train_pop), every per-instance array [P B][..], logs and noise [log_rows][P B][..], weights
 *     [P][39748]; learner l's instances step with weight row l.  P = 1 runs the single-policy launches, so a
 *     population of one is dart_lmpc_rollout bit for bit.  weights == NULL: no policy, as in dart_lmpc_rollout, on
 *     all P B instances.  h needs B_max >= P B.
 * Launch sequence: dart_lmpc_rollout_dev's with the evaluation's loop-step kernel in the place of the rollout's, and
 * when scores is not NULL one score launch after the last post.  Two calls of K1 and K2 steps give bit for bit what
 * one call of K1 + K2 steps gives, metrics included (k0 carries the step index into slot 1).
 *
 * scores [P][8] (fp64, out): per learner over its B instances in their order, sequential fp64 sums:
 *     0 mean steady-state error  (sum m[0]) / B       4 max error        max m[3]
 *     1 converged fraction       #(m[1] >= 0) / B     5 status nonzero   sum m[4]
 *     2 mean convergence step    sum of the m[1] >= 0 over their count; -1 when there is none
 *     3 mean control effort      (sum m[2]) / B       6 iters per solve  (sum m[5]) / (sum m[7]); 0 when that is 0
 *                                                     7 max rotation     max m[6]
 *
 * DART_MPC_EINVAL with a message, nothing enqueued: P < 1 or P > DART_LMPC_POP_MAX, P B > B_max, a negative count,
 * k0 + steps > log_rows, logs partly NULL, metrics NULL, a NULL among the required arrays, policy state NULL while
 * weights is set. */

/* One loop-step launch: dart_lmpc_loop_step_dev plus metrics [B][8], with the logs all set or all NULL. */
int dart_lmpc_eval_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                                 int B, int k, int do_post, int do_pre, int log_rows,
                                 const double *target, const double *plant_pvec,
                                 double *x, double *tilt, double *u_prev, const double *model_params, double *state,
                                 const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                                 double *metrics,
                                 double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                                 int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* Device pointers, asynchronous on hip_stream (NULL = the handle's own). */
int dart_lmpc_eval_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                       int P, int B, int k0, int steps, int log_rows,
                       const double *target, const double *prm, const double *plant_pvec, const double *current_k,
                       const float *weights, const float *noise,
                       double *x, double *tilt, double *u_prev, double *w, double *obs_mean, double *obs_M2,
                       int32_t *obs_count, float *history, int32_t *timestep, double *model_params,
                       double *metrics, double *scores,
                       double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                       int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* Host pointers: staged through device memory; blocks until state, metrics, scores (when not NULL) and, unless
 * metrics-only, rows k0 .. k0+steps-1 of the logs are back.  Of the noise only those rows travel. */
int dart_lmpc_eval(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                   int P, int B, int k0, int steps, int log_rows,
                   const double *target, const double *prm, const double *plant_pvec, const double *current_k,
                   const float *weights, const float *noise,
                   double *x, double *tilt, double *u_prev, double *w, double *obs_mean, double *obs_M2,
                   int32_t *obs_count, float *history, int32_t *timestep, double *model_params,
                   double *metrics, double *scores,
                   double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                   int32_t *log_status, int32_t *log_iters, void *hip_stream);

/* The score reduction alone: metrics [P][B][8] -> scores [P][8] (1 <= P <= DART_LMPC_POP_MAX, B >= 1; else
 * DART_MPC_EINVAL).  Device pointers, asynchronous; host pointers, blocking. */
int dart_lmpc_eval_scores_dev(int P, int B, const double *metrics, double *scores, void *hip_stream);
int dart_lmpc_eval_scores(int P, int B, const double *metrics, double *scores);

/* LMPC experience collection (handle of variant DART_MPC_LMPC; added within ABI 8): the training half of
 * RLMPC._rl_worker (rlmpc2.py:537-938) up to the PPO update, on the device.  dart_lmpc_collect is
 * dart_lmpc_rollout with one experience launch after every post(k) (+ pre(k+1)) launch:
 *     pre(k0), [solve launch(es), post(k) + pre(k+1), experience(k)] for k = k0 .. k0+steps-2,
 *     solve launch(es), post(k0+steps-1), experience(k0+steps-1)
 * The experience launch evaluates, for step k and on obs_k (history), raw_k (the policy's action, kept in a
 * handle-owned buffer) and x_k (log_X row k):
 *   - value_net(obs_k) (Policy :48-55, fp32) and the actor's mean recomputed in the policy kernel's own
 *     accumulation order (bit for bit its mean); log-probability Normal(mean, std).log_prob(raw).sum() (:699);
 *   - reward and done (:703-740): proximity w_pos e_p + w_vel e_p e_v, e = exp(-err^2 / (2 sigma^2)), minus
 *     w_change |delta_z| (fp32, damped to max_per_dim_rms; the damping enters the reward only), minus w_d_ctrl
 *     sum |control_k - prev_cmd|, minus the time penalty (+ time_penalty_rate per step), + success_bonus with both
 *     errors below success_tol; |x_k[0]| > tray_limit[0] or |x_k[2]| > tray_limit[1]: - oob_penalty and done bit 1;
 *     ++episode_step >= max_episode_steps: done bit 2.  The in_contact penalty (:735) has no counterpart in the
 *     LMPC plant and is left out;
 *   - the per-step logs reward (f64), done (int32), value, logp (fp32), row k;
 *   - every record_every-th policy step (:742) a record obs [520], action [34], logp, value (fp32), reward (f64),
 *     done (fp32 0 / 1) in row nrec[b]++ of the record arrays [rec_rows][B][..] while nrec[b] < rec_rows (a full
 *     buffer drops further records).  Fields are stored under their own names: the reference's buf.add (:744)
 *     swaps value and reward against RolloutBuffer.add (:93); that is not reproduced.  done_sticky = 1 stores the
 *     OR of every done since the previous record (0 = the reference: this step's done only);
 *   - at done: last_return, last_steps, episodes++, episode_return / episode_step / time_penalty zeroed, and with
 *     reset_rows > 0 the reset x <- reset_x[e][b], tilt <- 0, target <- reset_target[e][b], plant_pvec <-
 *     reset_pvec[e][b], e = (episodes - 1) % reset_rows (pool arrays [reset_rows][B][8 / 8 / 34]); the next
 *     solve's input is overwritten with the same x.  u_prev, w, the policy's state and prev_cmd carry over, as the
 *     reference's shared views do.  target and plant_pvec are therefore in/out here.
 * Collection state (caller-owned, in/out): prev_cmd, control_seen [B][2] (both start at the initial u_prev),
 * ep_step, ep_return, time_penalty, episodes, last_return, last_steps, nrec, sticky [B] (start at zero).
 * Two calls of K1 and K2 steps give bit for bit what one call of K1 + K2 steps gives. */
typedef struct dart_lmpc_reward_config {
    double sigma_pos, sigma_vel;   /* 0.02 (:712) */
    double w_pos, w_vel;           /* 40, 0.1 (rl_packet, rlmpc2.py:202-226) */
    double w_change;               /* 1e-3 (:713) */
    double w_d_ctrl;               /* 5 (:714) */
    double success_tol;            /* 0.01 (:720) */
    double success_bonus;          /* 20 (:721) */
    double oob_penalty;            /* 20 (:728) */
    double tray_limit[2];          /* {0.2, 0.15} (:726) */
    double max_per_dim_rms;        /* 0.5 (:691) */
    double time_penalty_rate;      /* 1e-4 (:772) */
    int32_t max_episode_steps;     /* 20000 (rl_packet) */
    int32_t record_every;          /* 8 (:742) */
    int32_t done_sticky;           /* 0 */
    int32_t reserved;
} dart_lmpc_reward_config;

/* value_net, fp32, input-major like the actor: V1[520][64], c1[64], V2[64][64], c2[64], V3[64], c3[1].  The
 * experience and collect entries need both weight arrays 16-byte aligned on the device (EINVAL otherwise). */
#define DART_LMPC_CRITIC_NWEIGHTS 37569

void dart_lmpc_reward_config_default(dart_lmpc_reward_config *cfg);

/* One experience launch for step k, for callers that sequence their own loop (after post(k) of
 * dart_lmpc_loop_step_dev).  Device pointers, asynchronous.  action [B][34] is the action_out of step k's policy
 * launch; state (the next solve's input) and mean_out [B][34] (the recomputed actor mean) are nullable; the reset
 * pool is read only with reset_rows > 0. */
int dart_lmpc_experience_step_dev(dart_mpc_handle *h, const dart_lmpc_policy_config *pcfg,
                                  const dart_lmpc_reward_config *rcfg,
                                  int B, int k, int log_rows, int rec_rows, int reset_rows,
                                  const float *weights, const float *critic,
                                  const float *history, const float *action, const double *log_X,
                                  const int32_t *timestep, const double *u_prev,
                                  double *target, double *plant_pvec, double *x, double *tilt, double *state,
                                  double *prev_cmd, double *control_seen, int32_t *ep_step, double *ep_return,
                                  double *time_penalty, int32_t *episodes, double *last_return, int32_t *last_steps,
                                  int32_t *nrec, int32_t *sticky,
                                  const double *reset_x, const double *reset_target, const double *reset_pvec,
                                  double *log_reward, int32_t *log_done, float *log_value, float *log_logp,
                                  float *rec_obs, float *rec_action, float *rec_logp, float *rec_value,
                                  double *rec_reward, float *rec_done, float *mean_out, void *hip_stream);

/* `steps` closed-loop steps with experience collection; arguments of dart_lmpc_rollout_dev plus the critic, the
 * reward config, the collection state, the reset pool, the per-step logs and the records.  A policy is required
 * (weights == NULL is DART_MPC_EINVAL).  Device pointers, asynchronous. */
int dart_lmpc_collect_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                          const dart_lmpc_reward_config *rcfg,
                          int B, int k0, int steps, int log_rows, int rec_rows, int reset_rows,
                          double *target, const double *prm, double *plant_pvec, const double *current_k,
                          const float *weights, const float *critic, const float *noise,
                          double *x, double *tilt, double *u_prev, double *w, double *obs_mean, double *obs_M2,
                          int32_t *obs_count, float *history, int32_t *timestep, double *model_params,
                          double *prev_cmd, double *control_seen, int32_t *ep_step, double *ep_return,
                          double *time_penalty, int32_t *episodes, double *last_return, int32_t *last_steps,
                          int32_t *nrec, int32_t *sticky,
                          const double *reset_x, const double *reset_target, const double *reset_pvec,
                          double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                          int32_t *log_status, int32_t *log_iters,
                          double *log_reward, int32_t *log_done, float *log_value, float *log_logp,
                          float *rec_obs, float *rec_action, float *rec_logp, float *rec_value,
                          double *rec_reward, float *rec_done, void *hip_stream);

/* Host pointers, staged as dart_lmpc_rollout stages (of the logs and the noise only rows k0 .. k0+steps-1 travel,
 * of the records the rows min nrec .. max nrec + ceil(steps / record_every) - 1, both ways); blocks. */
int dart_lmpc_collect(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                      const dart_lmpc_reward_config *rcfg,
                      int B, int k0, int steps, int log_rows, int rec_rows, int reset_rows,
                      double *target, const double *prm, double *plant_pvec, const double *current_k,
                      const float *weights, const float *critic, const float *noise,
                      double *x, double *tilt, double *u_prev, double *w, double *obs_mean, double *obs_M2,
                      int32_t *obs_count, float *history, int32_t *timestep, double *model_params,
                      double *prev_cmd, double *control_seen, int32_t *ep_step, double *ep_return,
                      double *time_penalty, int32_t *episodes, double *last_return, int32_t *last_steps,
                      int32_t *nrec, int32_t *sticky,
                      const double *reset_x, const double *reset_target, const double *reset_pvec,
                      double *log_X, double *log_U, double *log_pos_error, double *log_pvec, double *log_loss,
                      int32_t *log_status, int32_t *log_iters,
                      double *log_reward, int32_t *log_done, float *log_value, float *log_logp,
                      float *rec_obs, float *rec_action, float *rec_logp, float *rec_value,
                      double *rec_reward, float *rec_done, void *hip_stream);

/* Generalised advantage estimation (compute_gae, rlmpc2.py:592-599) per instance over its nrec[b] records
 * (record arrays [rec_rows][B]), fp64, bootstrapped from last_value [B]: adv and ret = adv + value, [rec_rows][B];
 * rows >= nrec[b] are left untouched.  Stateless (the HIP current device); normalising over the batch is a
 * statistic of the whole buffer and is left to the caller. */
int dart_lmpc_gae_dev(int B, int rec_rows, double gamma, double lam, const int32_t *nrec,
                      const double *rec_reward, const float *rec_value, const float *rec_done,
                      const float *last_value, double *adv, double *ret, void *hip_stream);
int dart_lmpc_gae(int B, int rec_rows, double gamma, double lam, const int32_t *nrec,
                  const double *rec_reward, const float *rec_value, const float *rec_done,
                  const float *last_value, double *adv, double *ret);

/* PPO update of the LMPC policy on the device (added within ABI 8): the clipped-surrogate update of
 * RLMPC._rl_worker (rlmpc2.py:783-819) on the records dart_lmpc_collect wrote and the advantages dart_lmpc_gae
 * wrote, fp32 like the reference's torch nets.  Stateless (the HIP current device), plain launches in stream
 * order, no atomics: two runs give the same bits.
 *   prepare, once:  ret_n = (ret - mean) / (std + 1e-8) in fp64 with the population std (:783, numpy);
 *                   adv_n = (adv - mean) / (std + 1e-8) in fp32 with the unbiased std (:788-790, torch; n = 1
 *                   gives NaN as torch does);
 *   per mini-batch of M samples (mini_batch_size, the last of an epoch shorter):
 *     grad:   both nets forward and backward on rows gathered through perm -> sample -> record row; loss
 *             -mean(min(ratio adv, clamp(ratio, 1 - clip_eps, 1 + clip_eps) adv)) + vf_coef mse(value, ret_n)
 *             - ent_coef entropy (:812-815), means over M; exact gradients of it (torch.clamp(std, min=1e-6) and
 *             the softplus branch of :802-805 cannot be reached, std >= 1e-2);
 *     apply:  clip_grad_norm_ (coef = min(1, max_grad_norm / (norm + 1e-6)), :818), then torch.optim.Adam with L2
 *             weight decay (:561) on weights, critic, adam and adam_step in place.
 * Parameters, gradients and Adam's moments share one packed order: the actor [39748] as dart_lmpc_policy_* reads
 * it, then the critic [37569]. */
typedef struct dart_lmpc_ppo_config {
    double clip_eps;               /* 0.2 (rl_packet, rlmpc2.py:202-226) */
    double vf_coef;                /* 0.25 (:202-226) */
    double ent_coef;               /* 0.01 (:202-226) */
    double max_grad_norm;          /* 0.5 (:202-226, :818) */
    double lr;                     /* 3e-4 (:561) */
    double beta1, beta2;           /* 0.9, 0.999 (:561, torch.optim.Adam's defaults) */
    double adam_eps;               /* 1e-8 (:561, Adam's default) */
    double weight_decay;           /* 1e-5 (:561) */
    double log_std_min;            /* log 1e-2 (Policy, :33-80) */
    double log_std_max;            /* log 2 */
    int32_t epochs;                /* 8 (:202-226) */
    int32_t mini_batch_size;       /* 64 (:202-226); 1 .. 1024 */
} dart_lmpc_ppo_config;

#define DART_LMPC_PPO_NPARAMS 77317

void dart_lmpc_ppo_config_default(dart_lmpc_ppo_config *cfg);

/* Bytes of the caller-provided device workspace for n samples and mini-batches of up to mini_batch_size samples
 * (0 for n < 1 or a mini_batch_size outside 1 .. 1024). */
size_t dart_lmpc_ppo_workspace_bytes(int n, int mini_batch_size);

/* The whole update: prepare, then for each of cfg->epochs rows of perm [epochs][n] the mini-batches
 * perm[e][0:M], perm[e][M:2M], ... each as one gradient launch and one apply launch.  Device pointers,
 * asynchronous.  sample [n] holds flat indices row * B + b into the record arrays (rec_rows_times_B entries of
 * 520 / 34 / 1 floats); record rows that sample does not name are never read.  adv, ret: the fp64
 * [rec_rows][B] arrays of dart_lmpc_gae_dev.  weights [39748], critic [37569] (16-byte aligned, EINVAL otherwise),
 * adam [2][77317] (m then v) and adam_step [1] are updated in place.  stats [3] (fp64): the means over this call's
 * steps of policy loss, value loss and entropy; step_log [steps][4] (fp32, nullable): policy loss, value loss,
 * entropy and gradient norm before the clip, one row per step of this call; adv_norm_out, ret_norm_out [n]
 * (fp32, nullable): the normalised inputs.  Calls of e1 and e2 epochs with the Adam state carried over and perm
 * rows 0 .. e1-1, then e1 .. e1+e2-1, give bit for bit what one call of e1 + e2 epochs gives. */
int dart_lmpc_ppo_update_dev(const dart_lmpc_ppo_config *cfg, int n, int rec_rows_times_B,
                             const int32_t *sample, const int32_t *perm,
                             const float *rec_obs, const float *rec_action, const float *rec_logp,
                             const double *adv, const double *ret,
                             float *weights, float *critic, float *adam, int32_t *adam_step,
                             double *stats, float *step_log, float *adv_norm_out, float *ret_norm_out,
                             void *workspace, void *hip_stream);

/* The same on host pointers: stages, blocks.  Before any device work it returns DART_MPC_EINVAL for n < 1, a
 * mini_batch_size outside 1 .. 1024, epochs < 0, a sample entry outside [0, rec_rows_times_B), a perm entry
 * outside [0, n), weights or critic not 16-byte aligned, or a null pointer. */
int dart_lmpc_ppo_update(const dart_lmpc_ppo_config *cfg, int n, int rec_rows_times_B,
                         const int32_t *sample, const int32_t *perm,
                         const float *rec_obs, const float *rec_action, const float *rec_logp,
                         const double *adv, const double *ret,
                         float *weights, float *critic, float *adam, int32_t *adam_step,
                         double *stats, float *step_log, float *adv_norm_out, float *ret_norm_out);

/* The launches of the update one by one, for callers that sequence their own loop (device pointers,
 * asynchronous, one workspace of dart_lmpc_ppo_workspace_bytes(n, largest M) throughout).  prepare writes the
 * normalised inputs into the workspace.  grad: one mini-batch idx [M] (positions in sample) -> the packed
 * gradient grad_out [77317] and terms_out [4] = policy loss, value loss, entropy, gradient norm (the gradient
 * launch, then the apply launch with its step switched off).  apply: a packed gradient grad [77317] into weights,
 * critic, adam and adam_step; terms [3] (nullable: zeros) are the loss terms it logs in row step_in_call of
 * step_log (nullable) and averages into stats (nullable) over step_in_call + 1 steps.  The full update gives bit
 * for bit what prepare followed by grad and apply for every mini-batch gives. */
int dart_lmpc_ppo_prepare_dev(int n, int rec_rows_times_B, const int32_t *sample, const double *adv,
                              const double *ret, float *adv_norm_out, float *ret_norm_out, void *workspace,
                              void *hip_stream);
int dart_lmpc_ppo_grad_dev(const dart_lmpc_ppo_config *cfg, int n, int rec_rows_times_B, int M,
                           const int32_t *sample, const int32_t *idx,
                           const float *rec_obs, const float *rec_action, const float *rec_logp,
                           const float *weights, const float *critic, float *grad_out, float *terms_out,
                           void *workspace, void *hip_stream);
int dart_lmpc_ppo_apply_dev(const dart_lmpc_ppo_config *cfg, const float *grad, const float *terms,
                            float *weights, float *critic, float *adam, int32_t *adam_step,
                            double *stats, float *step_log, int step_in_call, void *workspace, void *hip_stream);

/* value_net (Policy :48-55, fp32) on obs [n][520]: value_out [n]; the bootstrap value of :776-779.  Stateless. */
int dart_lmpc_critic_value_dev(int n, const float *critic, const float *obs, float *value_out, void *hip_stream);
int dart_lmpc_critic_value(int n, const float *critic, const float *obs, float *value_out);

/* Whole PPO training iterations of the LMPC policy on the device (added within ABI 8; csrc/lmpc_train.hip): the
 * loop of RLMPC._rl_worker (rlmpc2.py:537-938) without the host between its steps.  dart_lmpc_train(_dev) runs the
 * local update of every iteration (:783-819); dart_lmpc_train_global(_dev), further down, also runs the loop's second,
 * global-buffer update (:823-874) inside the iteration, before the parameter write.
 *
 * Random numbers.  One counter-based generator, Philox4x32-10 with the standard constants (multipliers 0xD2511F53,
 * 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85), key (seed & 0xffffffff, seed >> 32), counter
 * (c, iteration, stream, epoch); block c yields the four 32-bit words of elements 4c .. 4c+3.
 *   noise (stream 0, epoch 0): noise_out [steps][B][34] fp32 in the layout dart_lmpc_collect_dev reads; flat element
 *     e takes word e % 4 of block e / 4; a word r becomes u = ((r >> 9) + 0.5) 2^-23 (exact in fp32, never 0 or 1);
 *     words 0, 1 give one Box-Muller pair sqrt(-2 ln u0) (cos, sin)(2 pi u1), words 2, 3 the second; a tail of 1 to 3
 *     elements uses the leading words of its block.
 *   permutations (stream 1): perm_out [epochs][n] int32; the key of position i in epoch e is word i % 4 of block
 *     i / 4 with the epoch in the counter, and the permutation is the argsort of (key, i), ties broken on the index
 *     (np.lexsort((arange(n), key))).  key_out [epochs][n] (nullable) receives the raw keys.
 * dart_lmpc_philox_dev evaluates the generator on n given inputs in [n][6] = counter[4], key[2] into out [n][4]
 * (the known answers of the Philox paper's reference implementation can be checked through it).
 * The _dev entries take device pointers and are asynchronous on hip_stream; the host twins stage and block.
 * Stateless (the HIP current device).  EINVAL: a negative size, a null pointer with a positive size. */
int dart_lmpc_philox_dev(int n, const uint32_t *in, uint32_t *out, void *hip_stream);
int dart_lmpc_noise_dev(uint64_t seed, int iteration, int steps, int B, float *noise_out, void *hip_stream);
int dart_lmpc_noise(uint64_t seed, int iteration, int steps, int B, float *noise_out);
int dart_lmpc_perms_dev(uint64_t seed, int iteration, int epochs, int n, int32_t *perm_out, uint32_t *key_out,
                        void *hip_stream);
int dart_lmpc_perms(uint64_t seed, int iteration, int epochs, int n, int32_t *perm_out, uint32_t *key_out);

/* The mean-based parameter write after an update (rlmpc2.py:876-896) for B controllers: the actor on the current
 * history [B][520] -- no Welford update, no history shift, zero noise (the action is the mean, in the policy
 * kernel's accumulation order: its mean bit for bit), timestep untouched -- then the logit-space update (fp32), the
 * EMA and the tanh soft clip (fp64) of the policy step, applied unconditionally into model_params [B][34], and
 * current_k [B][34] <- model_params (:896).  mean_out [B][34] (fp32, nullable) receives the mean. */
int dart_lmpc_mean_param_update_dev(const dart_lmpc_policy_config *cfg, int B, const float *weights,
                                    const float *history, double *model_params, double *current_k,
                                    float *mean_out, void *hip_stream);
int dart_lmpc_mean_param_update(const dart_lmpc_policy_config *cfg, int B, const float *weights,
                                const float *history, double *model_params, double *current_k, float *mean_out);

typedef struct dart_lmpc_train_config {
    uint64_t seed;                 /* 0: of the noise and the permutations */
    int32_t iterations;            /* 1 */
    int32_t it0;                   /* 0: index of the first iteration (calls chain: it0 = iterations done so far) */
    int32_t steps;                 /* 256: closed-loop steps K per iteration; a multiple of record_every */
    int32_t mean_update;           /* 1: the parameter write of :876-896 after every update */
    int32_t track_best;            /* 1: the best-policy snapshot */
    int32_t reserved;
    double gamma;                  /* 0.99 */
    double lam;                    /* 0.95 */
} dart_lmpc_train_config;

#define DART_LMPC_TRAIN_LOG_COLS 12

/* The arrays of dart_lmpc_train(_dev): those of dart_lmpc_collect_dev in its order (weights, critic and current_k
 * are in/out here), Adam's state of dart_lmpc_ppo_update_dev, and the training outputs.  The logs have `steps`
 * rows and the records R = steps / record_every rows; after the call both hold the last iteration's values. */
typedef struct dart_lmpc_train_buffers {
    double *target; const double *prm; double *plant_pvec; double *current_k; float *weights; float *critic;
    double *x, *tilt, *u_prev, *w, *obs_mean, *obs_M2; int32_t *obs_count; float *history; int32_t *timestep;
    double *model_params;
    double *prev_cmd, *control_seen; int32_t *ep_step; double *ep_return, *time_penalty; int32_t *episodes;
    double *last_return; int32_t *last_steps, *nrec, *sticky;
    const double *reset_x, *reset_target, *reset_pvec;
    double *log_X, *log_U, *log_pos_error, *log_pvec, *log_loss; int32_t *log_status, *log_iters;
    double *log_reward; int32_t *log_done; float *log_value, *log_logp;
    float *rec_obs, *rec_action, *rec_logp, *rec_value; double *rec_reward; float *rec_done;
    float *adam;                   /* [2][77317] */
    int32_t *adam_step;            /* [1] */
    double *train_log;             /* [iterations][12], written */
    double *best_return;           /* [1] in/out, starts at -inf */
    float *best_weights;           /* [77317] actor then critic, written at a snapshot */
    int32_t *best_iter;            /* [1] written at a snapshot */
    void *workspace;               /* dart_lmpc_train_workspace_bytes; device memory (NULL for the host entry) */
} dart_lmpc_train_buffers;

void dart_lmpc_train_config_default(dart_lmpc_train_config *cfg);

/* Bytes of the workspace (noise, bootstrap values, advantages, returns, sample list, permutations, the update's
 * statistics and its workspace); 0 for a bad shape (B < 1, record_every < 1, K < record_every, K not a multiple of
 * record_every, epochs < 0, mini_batch_size outside 1 .. 1024). */
size_t dart_lmpc_train_workspace_bytes(int B, int K, int record_every, int epochs, int mini_batch_size);

/* Enqueues cfg->iterations complete PPO iterations on one stream (NULL: the handle's), plain launches in stream
 * order, no host work, no host random numbers and no staging between them.  For it = it0 .. it0+iterations-1:
 *   1. nrec <- 0; the noise of (seed, it) into the workspace;
 *   2. dart_lmpc_collect_dev with k0 = 0, steps = log_rows = K and the weights as they are now;
 *   3. dart_lmpc_critic_value_dev on history: the bootstrap value (:776-779);
 *   4. dart_lmpc_gae_dev (gamma, lam);
 *   5. the sample list 0 .. n-1, n = R B with R = K / record_every records per instance (K % record_every != 0 is
 *      DART_MPC_EINVAL: n must be known on the host);
 *   6. the permutations of (seed, it), then dart_lmpc_ppo_update_dev on weights, critic, adam, adam_step in place;
 *   7. with mean_update: dart_lmpc_mean_param_update_dev (current_k is in/out);
 *   8. row it - it0 of train_log, fp64, fixed-order sums: n; episodes ended in this iteration; mean and maximum of
 *      last_return over the instances whose episodes advanced (NaN if none); mean step reward over K x B; share of
 *      solves with status != 0; policy loss, value loss, entropy (the update's means); the number of instances with
 *      nrec[b] != R; best_return after this iteration; 1 if a snapshot was taken.  With track_best, a maximum above
 *      best_return replaces it, copies actor and critic (after this iteration's update) into best_weights and stores
 *      it in best_iter.  (The reference compares every episode's return at its end, :918-922; this entry compares
 *      once per iteration.)
 * Two calls of i1 and i2 iterations (it0 = 0, then i1) give bit for bit what one call of i1 + i2 gives. */
int dart_lmpc_train_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                        const dart_lmpc_reward_config *rcfg, const dart_lmpc_ppo_config *ppo,
                        const dart_lmpc_train_config *cfg, int B, int reset_rows,
                        const dart_lmpc_train_buffers *buf, void *hip_stream);

/* Host pointers: state, weights, Adam's state and the reset pool are staged in once, all iterations run, and the
 * results are staged out once (of logs and records what the last iteration wrote); blocks.  Instances whose
 * timestep differ are DART_MPC_EINVAL before any device work (they are the only way to nrec[b] != R). */
int dart_lmpc_train(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                    const dart_lmpc_reward_config *rcfg, const dart_lmpc_ppo_config *ppo,
                    const dart_lmpc_train_config *cfg, int B, int reset_rows,
                    const dart_lmpc_train_buffers *buf, void *hip_stream);

/* The global-buffer update of the training loop (rlmpc2.py:823-874; added within ABI 8: new entries only).  After
 * its local update every iteration of RLMPC._rl_worker draws m = max(1, n / 4) of its n records without
 * replacement (:823-827), appends them in the drawn order to a second buffer that survives across iterations
 * (glob_buf, :581) and, once that buffer holds at least n records, runs compute_gae over it as ONE sequence
 * bootstrapped from the critic on its last observation (:830-834), normalises and runs a second full PPO update on
 * the same optimizer (:835-871), and clears the buffer (:874); only then comes the mean-based parameter write.
 * The buffer is updated on when it holds G = ceil(n / m) m rows; G > n when n % 4 != 0 (n = 90: m = 22, G = 110).
 *
 * dart_lmpc_choice(_dev): choice_out [m] = the first m entries of the permutation of n elements that the generator
 * of dart_lmpc_perms gives for (seed, iteration, stream 2, epoch 0): the argsort of (key, index), ties on the index.
 * Nothing past choice_out[m - 1] is written.  EINVAL: iteration < 0, m < 1, m > n, a null pointer.
 * dart_lmpc_perms_stream_dev: dart_lmpc_perms_dev with the generator's stream index given (1: the local update's
 * permutations, what dart_lmpc_perms_dev draws; 3: the global update's). */
int dart_lmpc_choice_dev(uint64_t seed, int iteration, int n, int m, int32_t *choice_out, void *hip_stream);
int dart_lmpc_choice(uint64_t seed, int iteration, int n, int m, int32_t *choice_out);
int dart_lmpc_perms_stream_dev(uint64_t seed, int iteration, int rng_stream, int epochs, int n, int32_t *perm_out,
                               uint32_t *key_out, void *hip_stream);

#define DART_LMPC_GLOBAL_LOG_COLS 6

/* The global buffer: `capacity` rows of a record's six fields, device arrays for the _dev entries and host arrays
 * for the host entries.  fill is the number of rows held when a call starts; the host knows it (calls never read
 * it from the device) and advances it with dart_lmpc_global_fill_after. */
typedef struct dart_lmpc_global_buffer {
    float *obs;                    /* [capacity][520], 16-byte aligned (EINVAL otherwise) */
    float *action;                 /* [capacity][34] */
    float *logp;                   /* [capacity] */
    float *value;                  /* [capacity] */
    double *reward;                /* [capacity] */
    float *done;                   /* [capacity] */
    int32_t capacity;              /* >= G of dart_lmpc_global_rows */
    int32_t fill;                  /* rows held when the call starts */
    double *global_log;            /* [iterations][6], written by dart_lmpc_train_global(_dev) */
    void *workspace;               /* dart_lmpc_global_workspace_bytes; device memory (NULL for the host entries) */
} dart_lmpc_global_buffer;

/* m = max(1, n / 4) and G = ceil(n / m) m for n samples per iteration.  EINVAL: n < 1 or a null pointer. */
int dart_lmpc_global_rows(int n, int32_t *m_out, int32_t *G_out);
/* The fill after `iterations` more iterations started at `fill` (each appends m rows; a fill that reaches n is
 * updated on and becomes 0).  Pure host arithmetic, so calls chain.  Negative (DART_MPC_EINVAL) for n < 1,
 * iterations < 0 or a fill that is negative, >= n or not a multiple of m. */
int dart_lmpc_global_fill_after(int n, int fill, int iterations);
/* Bytes of the global update's workspace (the choice [m], the sequence's advantages and returns [G], the
 * bootstrap value, the sample list [G], the permutations [epochs][G], the update's statistics and
 * dart_lmpc_ppo_workspace_bytes(G, mini_batch_size)); 0 for n < 1, epochs < 0 or a mini_batch_size outside
 * 1 .. 1024. */
size_t dart_lmpc_global_workspace_bytes(int n, int epochs, int mini_batch_size);

/* Buffer row g->fill + j <- record sample[choice[j]] for j < m: sample [n] holds flat record indices row * B + b into
 * the record arrays of rec_rows_times_B entries (as dart_lmpc_ppo_update_dev reads them), choice [m] positions in
 * sample.  All six fields are copied bit for bit; nothing outside rows fill .. fill + m - 1 is written.  EINVAL
 * before any device work: m < 1, n < 1, g->fill < 0, g->fill + m > g->capacity, a null pointer; the device entry
 * also refuses rec_obs or g->obs not 16-byte aligned (the observation rows move in 16-byte pieces), the host entry a
 * choice entry outside [0, n) and a sample entry outside [0, rec_rows_times_B) (on the device such an entry writes
 * nothing).  global_log and workspace are not used. */
int dart_lmpc_global_append_dev(const dart_lmpc_global_buffer *g, int m, int n, int rec_rows_times_B,
                                const int32_t *sample, const int32_t *choice,
                                const float *rec_obs, const float *rec_action, const float *rec_logp,
                                const float *rec_value, const double *rec_reward, const float *rec_done,
                                void *hip_stream);
int dart_lmpc_global_append(const dart_lmpc_global_buffer *g, int m, int n, int rec_rows_times_B,
                            const int32_t *sample, const int32_t *choice,
                            const float *rec_obs, const float *rec_action, const float *rec_logp,
                            const float *rec_value, const double *rec_reward, const float *rec_done);

/* compute_gae (rlmpc2.py:592-599) over rows 0 .. G-1 as a single chain, fp64, bootstrapped from last_value [1]:
 * adv [G] and ret = adv + value [G]; rows >= G are left untouched.  One workgroup evaluates the recurrence
 * gae_t = delta_t + gamma lam (1 - done_t) gae_{t+1} as a suffix scan of affine maps, so the result is the sequential
 * recursion's up to reassociation: |d adv_t| <= 32 * 2^-52 * A_t for G <= 4096, A the same recursion on |delta_t|
 * (DESIGN.md section 6a has the count of roundings).  delta_t itself has the sequential recursion's bits. */
int dart_lmpc_gae_seq_dev(int G, double gamma, double lam, const double *reward, const float *value,
                          const float *done, const float *last_value, double *adv, double *ret, void *hip_stream);
int dart_lmpc_gae_seq(int G, double gamma, double lam, const double *reward, const float *value,
                      const float *done, const float *last_value, double *adv, double *ret);

/* dart_lmpc_train(_dev) with the global-buffer update; with g == NULL they are dart_lmpc_train(_dev), bit for bit.
 * With n = R B, (m, G) = dart_lmpc_global_rows(n) and the running fill starting at g->fill, every iteration `it`
 * runs steps 1 - 6 of dart_lmpc_train_dev, then
 *   6a. dart_lmpc_choice_dev(seed, it, n, m) and dart_lmpc_global_append_dev at the running fill (fill += m);
 *   6b. if the fill has reached n (it then equals G): dart_lmpc_critic_value_dev on row G - 1's observation,
 *       dart_lmpc_gae_seq_dev (gamma, lam), the sample list 0 .. G-1, dart_lmpc_perms_stream_dev with stream 3 over
 *       G, and dart_lmpc_ppo_update_dev on the buffer's arrays (n = rec_rows_times_B = G) with the same weights,
 *       critic, adam and adam_step in place -- Adam's step count runs on through both updates, as the reference's
 *       single optimizer does; the fill returns to 0;
 * then steps 7 and 8: the parameter write and the snapshot see the weights after both updates.  Row it - it0 of
 * global_log: the fill after the append, 1 if the update ran, G, and that update's mean policy loss, value loss and
 * entropy (NaN when it did not run).  The host computes the whole launch sequence from n and g->fill.
 * EINVAL before any device work: a fill that is negative, >= n or not a multiple of m, capacity < G, a null
 * pointer, obs or rec_obs not 16-byte aligned.  Calls chain: g->fill of the next call is
 * dart_lmpc_global_fill_after(n, g->fill, iterations). */
int dart_lmpc_train_global_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                               const dart_lmpc_policy_config *pcfg, const dart_lmpc_reward_config *rcfg,
                               const dart_lmpc_ppo_config *ppo, const dart_lmpc_train_config *cfg, int B,
                               int reset_rows, const dart_lmpc_train_buffers *buf,
                               const dart_lmpc_global_buffer *g, void *hip_stream);
/* Host pointers: as dart_lmpc_train, and the buffer's held rows (0 .. g->fill - 1) are staged in once and the rows
 * held at the end (0 .. dart_lmpc_global_fill_after(...) - 1) are staged out; other rows of the host arrays are
 * left untouched. */
int dart_lmpc_train_global(dart_mpc_handle *h, const dart_plant_config *plant,
                           const dart_lmpc_policy_config *pcfg, const dart_lmpc_reward_config *rcfg,
                           const dart_lmpc_ppo_config *ppo, const dart_lmpc_train_config *cfg, int B,
                           int reset_rows, const dart_lmpc_train_buffers *buf,
                           const dart_lmpc_global_buffer *g, void *hip_stream);

int dart_mpc_sync(dart_mpc_handle *h);

const char *dart_mpc_last_error(const dart_mpc_handle *h);

void dart_mpc_destroy(dart_mpc_handle *h);

/* Number of fp64 entries of w for horizon N: 6(N+1) + 2N. */
int dart_mpc_nw(int N);

/* A population of P independent learners trained in the launches of one (added within ABI 8: new entries only).
 * Every learner has its own actor, critic, Adam state, seed, controllers, reset pool, log and best-policy snapshot;
 * learner l is, bit for bit, the run dart_lmpc_train(_dev) gives for its arrays and cfg->seed = seeds[l] alone.  The
 * shared configs (plant, policy, reward, PPO; gamma, lam, steps, mean_update, track_best) apply to every learner.
 *
 * Layout, with dart_lmpc_train_buffers unchanged: the P B controllers are stacked learner-major, instance
 * i = l B + b, and every per-instance array keeps its meaning with P B in place of B (state and collection state
 * [P B][..], logs [K][P B][..], records [R][P B][..], reset pool [reset_rows][P B][..]).  Per learner: weights
 * [P][39748]; critic [P][DART_LMPC_POP_CRITIC_STRIDE] (37569 weights and three pad floats that are never read or
 * written, so that every critic is 16-byte aligned); adam [P][2][77317]; adam_step [P]; train_log
 * [P][iterations][12]; best_return [P]; best_weights [P][77317]; best_iter [P].
 *
 * seeds [P] (host memory, read before the entry returns; cfg->seed is ignored): learner l's noise and permutations
 * are those of dart_lmpc_noise_dev / dart_lmpc_perms_dev for (seeds[l], it); element (k, b, j) of its noise is
 * stored at [k][l B + b][j] of the stacked noise.  Its sample list is r B + b -> r (P B) + l B + b.
 *
 * The launch sequence per iteration is dart_lmpc_train_dev's, each step issued once for the whole population (the
 * update: prepare once, then gradient + apply per mini-batch index with every learner in each launch).  Calls chain
 * through it0 as the single entry's do.  The global-buffer update has its population form below
 * (dart_lmpc_train_pop_global); the rollout's population form is dart_lmpc_eval; per-learner hyper-parameters and
 * the exploit/explore step of population-based training follow it (dart_lmpc_train_pop_hyper, dart_lmpc_pbt_step);
 * dart_lmpc_collect has no population form. */
#define DART_LMPC_POP_MAX 32
#define DART_LMPC_POP_CRITIC_STRIDE 37572

/* Bytes of the workspace; 0 for a bad shape (P outside 1 .. DART_LMPC_POP_MAX, or what
 * dart_lmpc_train_workspace_bytes refuses). */
size_t dart_lmpc_train_pop_workspace_bytes(int P, int B, int K, int record_every, int epochs, int mini_batch_size);

/* Device pointers; h needs B_max >= P B.  DART_MPC_EINVAL before any device work: P < 1, P > DART_LMPC_POP_MAX,
 * P B > B_max, null seeds or a null required pointer, weights or critic not 16-byte aligned, steps not a multiple of
 * record_every, a handle of the wrong variant. */
int dart_lmpc_train_pop_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                            const dart_lmpc_reward_config *rcfg, const dart_lmpc_ppo_config *ppo,
                            const dart_lmpc_train_config *cfg, int P, const uint64_t *seeds, int B, int reset_rows,
                            const dart_lmpc_train_buffers *buf, void *hip_stream);

/* Host pointers: staged in once, all iterations, staged out once; blocks.  Instances (all P B) whose timestep
 * differ are DART_MPC_EINVAL before any device work. */
int dart_lmpc_train_pop(dart_mpc_handle *h, const dart_plant_config *plant, const dart_lmpc_policy_config *pcfg,
                        const dart_lmpc_reward_config *rcfg, const dart_lmpc_ppo_config *ppo,
                        const dart_lmpc_train_config *cfg, int P, const uint64_t *seeds, int B, int reset_rows,
                        const dart_lmpc_train_buffers *buf, void *hip_stream);

/* The population with the global-buffer update (added within ABI 8: new entries only): learner l is, bit for bit,
 * the run dart_lmpc_train_global(_dev) gives for its arrays, its buffer and cfg->seed = seeds[l] alone.
 *
 * Layout: one dart_lmpc_global_buffer holds the P buffers stacked learner-major, `capacity` rows apart: obs
 * [P][capacity][520] (capacity * 520 * 4 bytes is a multiple of 16, so every learner's obs is 16-byte aligned when
 * the base is), action [P][capacity][34], logp, value, done [P][capacity], reward [P][capacity] (fp64), global_log
 * [P][iterations][6].  All learners share n = R B, so they share m, G and the fill period: fill is one number for the
 * whole population, known to the host and advanced with dart_lmpc_global_fill_after as for one learner.  The
 * workspace is dart_lmpc_global_pop_workspace_bytes; it depends on capacity, because the sequences' advantages and
 * returns are laid out [P][capacity] like the buffers' rows: learner l's sample list over its buffer is
 * i -> l capacity + i, and the update's kernels reach rows, advantages and returns through that one index.
 *
 * Per iteration: dart_lmpc_train_pop_dev's sequence, and between the local update and the parameter write steps 6a
 * and 6b of dart_lmpc_train_global_dev, each issued once for all learners: the choices [P][m] (learner l's is
 * dart_lmpc_choice_dev's for seeds[l]), the append of row sample_l[choice_l[j]] of the stacked records into row
 * fill + j of buffer l, and when the fill reaches n the critics' values on row G - 1 of every buffer, the sequence
 * GAE with one workgroup per learner, the sample lists, the permutations of stream 3 over G per learner, and the
 * update's launches on the buffers' rows with every learner's own Adam state and step count. */

/* Bytes of the population's global workspace; 0 for a bad shape (P outside 1 .. DART_LMPC_POP_MAX, capacity < G,
 * or what dart_lmpc_global_workspace_bytes refuses). */
size_t dart_lmpc_global_pop_workspace_bytes(int P, int n, int capacity, int epochs, int mini_batch_size);

/* The steps of the population's global update alone, device pointers.  choice_out [P][m]: row l is
 * dart_lmpc_choice_dev(seeds[l], ...).  Append: g holds P stacked buffers, sample [P][n], choice [P][m]; learner l
 * writes rows g->fill .. g->fill + m - 1 of its buffer and nothing else.  Sequence GAE: reward, value, done, adv, ret
 * [P][capacity], last_value [P]; rows >= G of every learner are left untouched.  EINVAL as the single entries', and
 * for P outside 1 .. DART_LMPC_POP_MAX, null seeds, capacity < G. */
int dart_lmpc_choice_pop_dev(int P, const uint64_t *seeds, int iteration, int n, int m, int32_t *choice_out,
                             void *hip_stream);
int dart_lmpc_global_append_pop_dev(const dart_lmpc_global_buffer *g, int P, int m, int n, int rec_rows_times_PB,
                                    const int32_t *sample, const int32_t *choice,
                                    const float *rec_obs, const float *rec_action, const float *rec_logp,
                                    const float *rec_value, const double *rec_reward, const float *rec_done,
                                    void *hip_stream);
int dart_lmpc_gae_seq_pop_dev(int P, int capacity, int G, double gamma, double lam, const double *reward,
                              const float *value, const float *done, const float *last_value, double *adv,
                              double *ret, void *hip_stream);

/* Device pointers.  With g == NULL it is dart_lmpc_train_pop_dev, launch for launch.  DART_MPC_EINVAL before any
 * device work: what dart_lmpc_train_pop_dev refuses, what dart_lmpc_train_global_dev refuses of g (a fill that is
 * negative, >= n or not a multiple of m, capacity < G, a null field, obs not 16-byte aligned), rec_obs not 16-byte
 * aligned.  Calls chain: g->fill of the next call is dart_lmpc_global_fill_after(n, g->fill, iterations). */
int dart_lmpc_train_pop_global_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                                   const dart_lmpc_policy_config *pcfg, const dart_lmpc_reward_config *rcfg,
                                   const dart_lmpc_ppo_config *ppo, const dart_lmpc_train_config *cfg, int P,
                                   const uint64_t *seeds, int B, int reset_rows, const dart_lmpc_train_buffers *buf,
                                   const dart_lmpc_global_buffer *g, void *hip_stream);

/* Host pointers: as dart_lmpc_train_pop, and of every learner's buffer the held rows (0 .. g->fill - 1) are staged in
 * once and the rows held at the end staged out; other rows of the host arrays are left untouched.  global_log
 * [P][iterations][6] comes down. */
int dart_lmpc_train_pop_global(dart_mpc_handle *h, const dart_plant_config *plant,
                               const dart_lmpc_policy_config *pcfg, const dart_lmpc_reward_config *rcfg,
                               const dart_lmpc_ppo_config *ppo, const dart_lmpc_train_config *cfg, int P,
                               const uint64_t *seeds, int B, int reset_rows, const dart_lmpc_train_buffers *buf,
                               const dart_lmpc_global_buffer *g, void *hip_stream);

/* Per-learner hyper-parameters of a population (added within ABI 8: new entries only).  hyper
 * [P][DART_LMPC_HYPER_COLS], fp64: row l holds, for learner l, the first nine doubles of dart_lmpc_ppo_config in the
 * struct's order -- clip_eps, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, adam_eps, weight_decay -- and takes
 * their place in both updates (local and global buffer) of every iteration.  epochs and mini_batch_size (the host
 * computes the launch sequence from them), log_std_min / log_std_max and gamma / lam stay shared and come from ppo and
 * cfg.  Learner l is, bit for bit, the run dart_lmpc_train_global(_dev) gives for its arrays, seeds[l] and ppo with row
 * l in place of its first nine fields: the update's kernels convert a row exactly as the host converts a config
 * (clip bounds (float)(1 -+ clip_eps) formed in fp64; vf_coef, ent_coef, max_grad_norm, adam_eps, weight_decay cast to
 * fp32; lr, beta1, beta2 kept in fp64).
 *
 * The device entry never reads the table on the host: the kernels read row l when they run, so a table rewritten on
 * the same stream between two chained calls (by dart_lmpc_pbt_step_dev, or a copy) takes effect, and any contents,
 * NaN included, are safe (they enter arithmetic only).  With hyper == NULL it is dart_lmpc_train_pop_global_dev,
 * launch for launch; with g == NULL there is no global update.  DART_MPC_EINVAL as dart_lmpc_train_pop_global_dev.
 *
 * The host entry stages the table in (read only) with the other arrays, and refuses with DART_MPC_EINVAL, before any
 * device work, a row that would be refused as a config (a negative or NaN clip_eps, lr, adam_eps or max_grad_norm, a
 * beta outside [0, 1)). */
#define DART_LMPC_HYPER_COLS 9

int dart_lmpc_train_pop_hyper_dev(dart_mpc_handle *h, const dart_plant_config *plant,
                                  const dart_lmpc_policy_config *pcfg, const dart_lmpc_reward_config *rcfg,
                                  const dart_lmpc_ppo_config *ppo, const dart_lmpc_train_config *cfg, int P,
                                  const uint64_t *seeds, int B, int reset_rows, const dart_lmpc_train_buffers *buf,
                                  const dart_lmpc_global_buffer *g, const double *hyper, void *hip_stream);
int dart_lmpc_train_pop_hyper(dart_mpc_handle *h, const dart_plant_config *plant,
                              const dart_lmpc_policy_config *pcfg, const dart_lmpc_reward_config *rcfg,
                              const dart_lmpc_ppo_config *ppo, const dart_lmpc_train_config *cfg, int P,
                              const uint64_t *seeds, int B, int reset_rows, const dart_lmpc_train_buffers *buf,
                              const dart_lmpc_global_buffer *g, const double *hyper, void *hip_stream);

/* The exploit/explore step of population-based training (added within ABI 8: new entries only): the k worst of P
 * learners restart from the nets, the optimizer state and the hyper-parameters of one of the k best, and their
 * hyper-parameters are perturbed -- on the device, in two launches on the caller's stream (a rank kernel of one wave,
 * then a copy kernel), so that train -> evaluate -> step -> train needs no host work in between.
 *
 * fitness[l * fitness_stride] is learner l's figure of merit: dart_lmpc_eval's scores + slot with stride 8 reads a
 * column of the scores where they lie, a column of train_log works the same way.  Layouts are dart_lmpc_train_pop's:
 * weights [P][39748], critic [P][DART_LMPC_POP_CRITIC_STRIDE], adam [P][2][77317], adam_step [P]; hyper
 * [P][DART_LMPC_HYPER_COLS]; rank_out, parent_out [P].
 *
 * The rule, exact:
 *   Ranking.  Learner a is better than b if its fitness is strictly better in the configured direction
 *     (higher_is_better != 0: greater), or if the two compare equal and a < b.  A NaN is worse than every non-NaN,
 *     NaNs are ordered among themselves by index, +-inf are ordinary values.  rank_out[l] is the number of learners
 *     better than l: 0 is the best.
 *   Exploit.  With k = n_replace (0: P / 4), the children are the learners of rank >= P - k and the donors those of
 *     ranks 0 .. k - 1; 2 k <= P, so no donor is ever written.  Child l takes the Philox4x32-10 block at counter
 *     (l, generation, 4, 0), key (seed & 0xffffffff, seed >> 32) as dart_lmpc_noise forms it; its parent is the learner
 *     of rank word0 % k.  parent_out[l] = l for everyone else.  The child receives, bit for bit, the parent's actor
 *     row, its 37569 critic weights (the three pad floats of a row are never read or written), both Adam moments and
 *     adam_step.
 *   Explore, children only.  For column c, v = hyper[parent][c]; if bit c of explore_mask is set,
 *     v = v * (w >> 31 ? factor_up : factor_down) with w = word c % 4 of the block at counter
 *     (l, generation, 4, 1 + c / 4), one fp64 product; then v < lo[c] ? lo[c] : (v > hi[c] ? hi[c] : v) for every
 *     column, so a NaN passes through; hyper[l][c] = v.
 * Left alone: everything of a surviving learner, and of a child its instances' controller and environment state,
 * observation statistics (they are per controller instance and describe the child's own trajectories, not the net),
 * history, current_k, reset pool, seed, logs and best-policy snapshot.
 *
 * P = 1, or an effective k = 0 (P < 4 with n_replace = 0), writes rank_out and parent_out = self and nothing else.
 * DART_MPC_EINVAL before any device work: P outside 1 .. DART_LMPC_POP_MAX, n_replace < 0 or 2 k > P,
 * fitness_stride < 1, generation < 0, lo[c] > hi[c] or a NaN bound, a factor <= 0 or NaN, a null pointer, weights or
 * critic not 16-byte aligned. */
typedef struct dart_lmpc_pbt_config {
    uint64_t seed;                 /* 0: the generator key of the parent draws and the perturbations */
    int32_t generation;            /* 0: the counter's second word; advance it by one per step */
    int32_t n_replace;             /* 0 = P / 4: learners replaced (k) */
    int32_t higher_is_better;      /* 0: a lower fitness is better (steady-state error); 1 for returns */
    uint32_t explore_mask;         /* bit c: column c is perturbed; default lr | clip_eps | ent_coef = 0x15 */
    double factor_down, factor_up; /* 0.8, 1.25 */
    double lo[DART_LMPC_HYPER_COLS]; /* clamp of every column of a child's row; the defaults lie inside what the */
    double hi[DART_LMPC_HYPER_COLS]; /* training entries accept: clip_eps [0.01, 0.5], ent_coef [0, 0.1],
                                      * lr [1e-6, 1e-2], beta1, beta2 [0, 0.999999], max_grad_norm, adam_eps
                                      * [0, inf], vf_coef, weight_decay [-inf, inf] */
} dart_lmpc_pbt_config;

void dart_lmpc_pbt_config_default(dart_lmpc_pbt_config *cfg);

/* Device pointers, asynchronous on hip_stream (NULL: the default stream). */
int dart_lmpc_pbt_step_dev(const dart_lmpc_pbt_config *cfg, int P, const double *fitness, int fitness_stride,
                           float *weights, float *critic, float *adam, int32_t *adam_step, double *hyper,
                           int32_t *rank_out, int32_t *parent_out, void *hip_stream);

/* Host pointers (fitness [(P - 1) fitness_stride + 1] read at the stride): staged in, the step, staged out; blocks. */
int dart_lmpc_pbt_step(const dart_lmpc_pbt_config *cfg, int P, const double *fitness, int fitness_stride,
                       float *weights, float *critic, float *adam, int32_t *adam_step, double *hyper,
                       int32_t *rank_out, int32_t *parent_out);

/* The PMPC closed loop through the dual-arm layer (added within ABI 8: new entries only).  One device-resident loop
 * for E experiments of two arms each (arm instances 2 e, 2 e + 1), the reference's driver loop
 * (PMPC/main_parallel_enhanced.py:290-419: u_cmd -> quaternion -> DACTL.control -> torques -> step).  Per step k, six
 * launches on one stream:
 *   solve        dart_mpc_solve_batch_dev                                     x0 -> u0
 *   command      tray_cmd[e] = (tray_pos[e] | quaternion of u0[e]), the expressions of the rollouts' log_quat
 *   arm dynamics of the joint state q_k against tray_cmd (dart_dual_arm_control_dev's), EE orientations kept
 *   arm QP       dart_arm_solve_batch_dev
 *   arm plant    dart_dual_arm_rollout_dev's plant step, arm metrics and logs   q_k -> q_{k+1}
 *   couple + object   the tray the two arms hold at q_k, then post(k) / pre(k+1) of dart_pmpc[_lm]_loop_step_dev
 *
 * Coupling (dart_tray_from_arms): with grasp [2][7] (pos | quat wxyz, tray frame) and the arms' EE points ee_pos and
 * orientations ee_quat, q_a = unit(ee_quat_a (x) conj(g_q_a)), q_R flipped into q_L's hemisphere, q_t = unit(q_L + q_R)
 * with w >= 0, p_t = 1/2 sum_a (ee_pos_a - rot(q_t, g_p_a)); roll = atan2(2(wx + yz), 1 - 2(x^2 + y^2)),
 * pitch = asin(clamp(2(wy - zx), -1, 1)), yaw = atan2(2(wz + xy), 1 - 2(y^2 + z^2)) (the inverse of the command's
 * Euler xyz [u1, -u0, 0]); achieved tilt = [-pitch, roll]; diag = yaw, grasp gap | |ee_R - ee_L| - |g_R - g_L| |,
 * disagreement angle 2 atan2(|v|, |w|) of q_L (x) conj(q_R).  The result does not change under a sign flip of either
 * ee_quat.  Non-finite input gives non-finite output, never a fault.
 *
 * couple selects the tilt the object plant sees:
 *   DART_STACK_RIDE      the lagged command, exactly dart_pmpc[_lm]_rollout; the arms ride along and are measured
 *   DART_STACK_ACHIEVED  tilt := the achieved tilt of q_k, held over the step; no lag, plant->tau is not used.  A
 *                        non-finite achieved tilt is not passed on: the last tilt is held and the step counted.
 *
 * Arrays.  The PMPC loop's: target, prm [E][6], x [E][6] (LMPC plant: x [E][8], plant_pvec [E][34], pz_vz [E][2]), tilt
 * [E][2], metrics [E][8] (the cross-plant loops' slots, kept for the tray plant too, whose slot 6 stays 0; in/out, a
 * fresh run starts from zeros with slot 1 = -1).  The arm rollout's: grasp, models, plant_models [2][model_len], arm_prm
 * (arm_prm_stride 0 or the row length), q, qd, qdd_prev [2 E][n], arm_metrics [2 E][6], all as dart_dual_arm_rollout;
 * work: dart_stack_work_len(E, n) doubles of device memory (it starts with the arm rollout's work, so the step's
 * snapshot rows are its first 2 E dart_arm_snapshot_len(n) doubles).  tray_pos [E][3].  stack_metrics [E][8], in/out, a
 * fresh run starts from zeros: 0 max_i |tilt_achieved - u0|_i of the last step with a finite achieved tilt, 1 its
 * maximum over the steps, 2 max |yaw|, 3 max grasp gap, 4 max disagreement angle, 5 max |p_t - tray_pos|, 6 steps with
 * a held tilt, 7 steps.  A maximum ignores a NaN.  Every metric is in/out: two calls of K1 and K2 steps (k0 = 0, then
 * k0 = K1) give the bits of one call of K1 + K2.
 *
 * Logs [log_rows][.]..., row k0 + j for step j, in three groups, each given whole or all null: the PMPC rollout's
 * (log_X, log_U, log_quat, log_loss, log_status, log_iters; LMPC plant: and log_rot); log_tilt [..][E][2] (the achieved
 * tilt as measured) and log_tray [..][E][7] (the achieved pose); the arm rollout's six ([..][2 E][.]).  With no group
 * given log_rows is not consulted (metrics-only), on both plants.
 *
 * DART_MPC_EINVAL before any HIP call: a handle that is not PMPC's, a null config or required pointer, a group of logs
 * given in part, k0 + steps > log_rows with a group given, E < 1 or E > B_max, couple neither of the two, and what
 * dart_dual_arm_rollout refuses of n, arm_prm_stride and the two arm configs. */
#define DART_STACK_RIDE 0
#define DART_STACK_ACHIEVED 1
#define DART_STACK_COMMAND 0 /* phase of a loop-step launch: the command kernel ... */
#define DART_STACK_COUPLE 1  /* ... or couple + object */

typedef struct dart_stack_config {
    int32_t couple;        /* DART_STACK_ACHIEVED */
    int32_t reserved[7];   /* 0 */
} dart_stack_config;

void dart_stack_config_default(dart_stack_config *cfg);
int dart_stack_work_len(int E, int n); /* doubles; DART_MPC_EINVAL as dart_dual_arm_work_len */

/* The coupling alone: ee_pos [2 E][3], ee_quat [2 E][4], grasp [2][7] -> tray [E][7], tilt [E][2], diag [E][3].
 * DART_MPC_EINVAL: E < 1 or > 2^20, a null pointer. */
int dart_tray_from_arms_dev(int E, const double *ee_pos, const double *ee_quat, const double *grasp, double *tray,
                            double *tilt, double *diag, void *hip_stream);
int dart_tray_from_arms(int E, const double *ee_pos, const double *ee_quat, const double *grasp, double *tray,
                        double *tilt, double *diag);

/* One launch of the loop (device pointers, asynchronous), the pattern of dart_pmpc_loop_step_dev.  phase
 * DART_STACK_COMMAND: tray_cmd [E][7] from u0 and tray_pos (only these three are read; do_post / do_pre are not
 * consulted).  phase DART_STACK_COUPLE: couple + post(k) and / or pre; snap [2 E][dart_arm_snapshot_len(n)] and ee_quat
 * [2 E][4] are what the step's arm dynamics wrote (read by post only); x0, u0, f, status, iters are the solve's
 * per-step arrays; tray_cmd is not read. */
int dart_pmpc_stack_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_stack_config *scfg,
                                  int E, int n, int k, int phase, int do_post, int do_pre, int log_rows,
                                  const double *target, const double *prm, const double *tray_pos, const double *grasp,
                                  const double *snap, const double *ee_quat,
                                  double *x, double *tilt, double *metrics, double *stack_metrics,
                                  double *x0, double *tray_cmd,
                                  const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                                  double *log_X, double *log_U, double *log_quat, double *log_loss,
                                  int32_t *log_status, int32_t *log_iters, double *log_tilt, double *log_tray,
                                  void *hip_stream);
int dart_pmpc_stack_lm_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_stack_config *scfg,
                                     int E, int n, int k, int phase, int do_post, int do_pre, int log_rows,
                                     const double *target, const double *plant_pvec, const double *pz_vz,
                                     const double *tray_pos, const double *grasp,
                                     const double *snap, const double *ee_quat,
                                     double *x, double *tilt, double *metrics, double *stack_metrics,
                                     double *x0, double *tray_cmd,
                                     const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                                     double *log_X, double *log_U, double *log_quat, double *log_loss,
                                     int32_t *log_status, int32_t *log_iters, double *log_rot,
                                     double *log_tilt, double *log_tray, void *hip_stream);

/* `steps` steps from step k0, no host synchronisation in between.  Device pointers, asynchronous on hip_stream
 * (NULL: the handle's stream). */
int dart_pmpc_stack_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_stack_config *scfg,
                                const dart_arm_dyn_config *dcfg, const dart_arm_config *qcfg,
                                int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                                const double *target, const double *prm, double *x, double *tilt, double *metrics,
                                const double *grasp, const double *models, const double *plant_models,
                                const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                                double *work, const double *tray_pos, double *stack_metrics,
                                double *log_X, double *log_U, double *log_quat, double *log_loss,
                                int32_t *log_status, int32_t *log_iters, double *log_tilt, double *log_tray,
                                double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                                int32_t *status_log, void *hip_stream);
int dart_pmpc_stack_lm_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_stack_config *scfg,
                                   const dart_arm_dyn_config *dcfg, const dart_arm_config *qcfg,
                                   int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                                   const double *target, const double *prm, const double *plant_pvec,
                                   const double *pz_vz, double *x, double *tilt, double *metrics,
                                   const double *grasp, const double *models, const double *plant_models,
                                   const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                                   double *work, const double *tray_pos, double *stack_metrics,
                                   double *log_X, double *log_U, double *log_quat, double *log_loss,
                                   int32_t *log_status, int32_t *log_iters, double *log_rot,
                                   double *log_tilt, double *log_tray,
                                   double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                                   int32_t *status_log, void *hip_stream);

/* Host pointers: the arrays are staged through the handle's arena around the device form (no work argument; the rows
 * k0 .. k0 + steps - 1 of the logs given come down); blocks. */
int dart_pmpc_stack_rollout(dart_mpc_handle *h, const dart_plant_config *plant, const dart_stack_config *scfg,
                            const dart_arm_dyn_config *dcfg, const dart_arm_config *qcfg,
                            int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                            const double *target, const double *prm, double *x, double *tilt, double *metrics,
                            const double *grasp, const double *models, const double *plant_models,
                            const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                            const double *tray_pos, double *stack_metrics,
                            double *log_X, double *log_U, double *log_quat, double *log_loss,
                            int32_t *log_status, int32_t *log_iters, double *log_tilt, double *log_tray,
                            double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                            int32_t *status_log, void *hip_stream);
int dart_pmpc_stack_lm_rollout(dart_mpc_handle *h, const dart_plant_config *plant, const dart_stack_config *scfg,
                               const dart_arm_dyn_config *dcfg, const dart_arm_config *qcfg,
                               int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                               const double *target, const double *prm, const double *plant_pvec,
                               const double *pz_vz, double *x, double *tilt, double *metrics,
                               const double *grasp, const double *models, const double *plant_models,
                               const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                               const double *tray_pos, double *stack_metrics,
                               double *log_X, double *log_U, double *log_quat, double *log_loss,
                               int32_t *log_status, int32_t *log_iters, double *log_rot,
                               double *log_tilt, double *log_tray,
                               double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                               int32_t *status_log, void *hip_stream);

/* ---- The RMPC loop closed through the dual-arm layer (added within ABI 8) ------------------------------------------
 * RMPC/dev_dual/rob_ctrl.py:331-416 on one stream without the host: per step k of E experiments (arm instances 2 e, 2 e + 1)
 *   solve        dart_rmpc_solve_batch_dev, warm-started in place on w, with the fused RLS on theta, P, phi, y
 *   command      tray_cmd[e] = (tray_pos[e] | quaternion of u0[e]), the launch of the PMPC stack loop
 *   arm dynamics, arm QP, arm plant     as in the PMPC stack loop                 q_k -> q_{k+1}
 *   couple + object   the tray the two arms hold at q_k (dart_tray_from_arms), then post(k) / pre(k+1) of
 *                     dart_rmpc[_lm]_loop_step_dev
 * One pre launch precedes the first solve: six launches per step.  couple as above: DART_STACK_RIDE is exactly
 * dart_rmpc[_lm]_rollout on the object side (the arms ride along and are measured); DART_STACK_ACHIEVED sets tilt := the
 * achieved tilt of q_k and drives the plant with it (a non-finite one is not passed on: the last tilt is held and the
 * step counted).  u_prev := u0 in both modes: the controller's own last command (rob_ctrl.py:416).  The RLS sees the
 * measured states either way, so in achieved mode it identifies the object on the tray the arms hold.
 *
 * Arrays.  The RMPC loop's, as dart_rmpc[_lm]_rollout: target [E][4], prm [E][10], mu [E] (LMPC plant: plant_pvec
 * [E][34]), x [E][6] (LMPC plant: [E][8]), tilt, prev, u_prev, r_v, theta, P, w, done, nlog; metrics [E][8] kept on both
 * plants (the tray plant's slot 6 stays 0).  The arm rollout's, work (dart_stack_work_len(E, n)), tray_pos and
 * stack_metrics [E][8] as dart_pmpc_stack_rollout.  All state and metrics are in/out: two calls of K1 and K2 steps give
 * the bits of one call of K1 + K2.
 *
 * Logs [log_rows][.]..., in three groups, each given whole or all null; with none given log_rows is not consulted
 * (metrics-only; done and nlog still advance), on both plants:
 *   the RMPC rollout's ten (LMPC plant: and log_rot): episode rows at nlog[e] while !done[e], step rows at k0 + j;
 *   log_U [..][E][2] the command u0, log_quat [..][E][4] its quaternion (the bits of tray_cmd[:, 3:]), log_tilt
 *   [..][E][2] the achieved tilt as measured, log_tray [..][E][7] the achieved pose;
 *   the arm rollout's six ([..][2 E][.]); tau_log rows [2 e | 2 e + 1] are the reference's torques_log of experiment e.
 *
 * DART_MPC_EINVAL before any HIP call: a handle that is not RMPC's, a null config or required pointer, what
 * dart_rmpc_rollout refuses of the plant and loop configs, a group of logs given in part, k0 + steps > log_rows with a
 * group given, E < 1 or E > B_max, couple neither of the two, what dart_dual_arm_rollout refuses of n, arm_prm_stride
 * and the two arm configs, and (host form) a negative nlog. */

/* One launch (device pointers, asynchronous).  phase DART_STACK_COMMAND: tray_cmd from u0 and tray_pos (only these
 * three are read).  phase DART_STACK_COUPLE: couple + post(k) and / or pre; snap and ee_quat are what the step's arm
 * dynamics wrote; x0, Rref [E][4 (N + 1)], phi [E][7], y [E][2], u0, f, status, iters are the solve's per-step arrays. */
int dart_rmpc_stack_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                                  const dart_stack_config *scfg,
                                  int E, int n, int k, int phase, int do_post, int do_pre, int log_rows,
                                  const double *target, const double *prm, const double *mu,
                                  const double *tray_pos, const double *grasp, const double *snap, const double *ee_quat,
                                  double *x, double *tilt, double *prev, double *u_prev, double *r_v, const double *theta,
                                  int32_t *done, int32_t *nlog, double *metrics, double *stack_metrics,
                                  double *x0, double *Rref, double *phi, double *y, double *tray_cmd,
                                  const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                                  double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                                  double *log_x, double *log_theta, double *log_r_v, double *log_f,
                                  int32_t *log_status, int32_t *log_iters,
                                  double *log_U, double *log_quat, double *log_tilt, double *log_tray, void *hip_stream);
int dart_rmpc_stack_lm_loop_step_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                                     const dart_stack_config *scfg,
                                     int E, int n, int k, int phase, int do_post, int do_pre, int log_rows,
                                     const double *target, const double *prm, const double *plant_pvec,
                                     const double *tray_pos, const double *grasp, const double *snap, const double *ee_quat,
                                     double *x, double *tilt, double *prev, double *u_prev, double *r_v, const double *theta,
                                     int32_t *done, int32_t *nlog, double *metrics, double *stack_metrics,
                                     double *x0, double *Rref, double *phi, double *y, double *tray_cmd,
                                     const double *u0, const double *f, const int32_t *status, const int32_t *iters,
                                     double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                                     double *log_x, double *log_theta, double *log_r_v, double *log_f,
                                     int32_t *log_status, int32_t *log_iters, double *log_rot,
                                     double *log_U, double *log_quat, double *log_tilt, double *log_tray, void *hip_stream);

/* `steps` steps from step k0, no host synchronisation in between.  Device pointers, asynchronous on hip_stream
 * (NULL: the handle's stream). */
int dart_rmpc_stack_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                                const dart_stack_config *scfg, const dart_arm_dyn_config *dcfg, const dart_arm_config *qcfg,
                                int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                                const double *target, const double *prm, const double *mu,
                                double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                                double *P, double *w, int32_t *done, int32_t *nlog, double *metrics,
                                const double *grasp, const double *models, const double *plant_models,
                                const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                                double *work, const double *tray_pos, double *stack_metrics,
                                double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                                double *log_x, double *log_theta, double *log_r_v, double *log_f,
                                int32_t *log_status, int32_t *log_iters,
                                double *log_U, double *log_quat, double *log_tilt, double *log_tray,
                                double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                                int32_t *status_log, void *hip_stream);
int dart_rmpc_stack_lm_rollout_dev(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                                   const dart_stack_config *scfg, const dart_arm_dyn_config *dcfg,
                                   const dart_arm_config *qcfg,
                                   int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                                   const double *target, const double *prm, const double *plant_pvec,
                                   double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                                   double *P, double *w, int32_t *done, int32_t *nlog, double *metrics,
                                   const double *grasp, const double *models, const double *plant_models,
                                   const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                                   double *work, const double *tray_pos, double *stack_metrics,
                                   double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                                   double *log_x, double *log_theta, double *log_r_v, double *log_f,
                                   int32_t *log_status, int32_t *log_iters, double *log_rot,
                                   double *log_U, double *log_quat, double *log_tilt, double *log_tray,
                                   double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                                   int32_t *status_log, void *hip_stream);

/* Host pointers: the arrays are staged through the handle's arena around the device form (no work argument); the step
 * rows k0 .. k0 + steps - 1 of the logs given come down, the episode rows travel both ways over the rows
 * min nlog .. max nlog + steps; blocks. */
int dart_rmpc_stack_rollout(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                            const dart_stack_config *scfg, const dart_arm_dyn_config *dcfg, const dart_arm_config *qcfg,
                            int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                            const double *target, const double *prm, const double *mu,
                            double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                            double *P, double *w, int32_t *done, int32_t *nlog, double *metrics,
                            const double *grasp, const double *models, const double *plant_models,
                            const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                            const double *tray_pos, double *stack_metrics,
                            double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                            double *log_x, double *log_theta, double *log_r_v, double *log_f,
                            int32_t *log_status, int32_t *log_iters,
                            double *log_U, double *log_quat, double *log_tilt, double *log_tray,
                            double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                            int32_t *status_log, void *hip_stream);
int dart_rmpc_stack_lm_rollout(dart_mpc_handle *h, const dart_plant_config *plant, const dart_rmpc_loop_config *loop,
                               const dart_stack_config *scfg, const dart_arm_dyn_config *dcfg, const dart_arm_config *qcfg,
                               int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                               const double *target, const double *prm, const double *plant_pvec,
                               double *x, double *tilt, double *prev, double *u_prev, double *r_v, double *theta,
                               double *P, double *w, int32_t *done, int32_t *nlog, double *metrics,
                               const double *grasp, const double *models, const double *plant_models,
                               const double *arm_prm, double *q, double *qd, double *qdd_prev, double *arm_metrics,
                               const double *tray_pos, double *stack_metrics,
                               double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep,
                               double *log_x, double *log_theta, double *log_r_v, double *log_f,
                               int32_t *log_status, int32_t *log_iters, double *log_rot,
                               double *log_U, double *log_quat, double *log_tilt, double *log_tray,
                               double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log,
                               int32_t *status_log, void *hip_stream);

/* ABI version (DART_MPC_ABI_VERSION) of the loaded library. */
int dart_mpc_abi_version(void);

/* Build identity (round 6): the first 16 hex digits of the SHA-1 of the sources the library was compiled from
 * (the Makefile's SRC then HDR lists, concatenated), and the diagnostic flavour of the build: "" for the product
 * library, "stamps" / "trace" for the phase-stamp and restoration-trace builds.  The Python binding refuses a
 * library whose identity is not that of the sources beside it (a stale build). */
const char *dart_mpc_build_id(void);
const char *dart_mpc_build_flavor(void);

#ifdef __cplusplus
}
#endif

#endif /* DART_MPC_H */
