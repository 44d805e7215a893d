// dart_mpc_rmpc_stack.hip -- the RMPC stack entries of include/dart_mpc.h (host side): the RMPC closed loop through
// the dual-arm layer.  Per step the unchanged RMPC solve with its fused RLS (warm-started in place, as
// dart_rmpc_rollout), stack_command_kernel (stack_step.hip), the arm layer's step (dart_mpc_arm.hip dual_arm_step:
// dynamics, QP, plant) and rmpc_stack_step_kernel (rmpc_stack_step.hip), on one stream.
#include "abi_internal.h"
#include "arm_dyn.h"
#include "rmpc_stack_step.h"

namespace {

// every array of the RMPC stack loop, as the entries take them (the tray plant's entries leave plant_pvec and log_rot
// null, the LMPC plant's mu)
struct RmpcStackBuf {
    const double *target, *prm, *mu, *plant_pvec;
    double *x, *tilt, *prev, *u_prev, *r_v, *theta, *P, *w;
    int32_t *done, *nlog;
    double* metrics;
    const double *grasp, *models, *plant_models, *arm_prm;
    double *q, *qd, *qdd_prev, *arm_metrics, *work;
    const double* tray_pos;
    double* stack_metrics;
    double *log_pos_err, *log_pos_err_norm, *log_u_cmd, *log_timestep;     // the RMPC group: episode rows ...
    double *log_x, *log_theta, *log_r_v, *log_f;                          // ... and step rows
    int32_t *log_status, *log_iters;
    double* log_rot;
    double *log_U, *log_quat, *log_tilt, *log_tray;                       // the stack group
    double *q_log, *qd_log, *tau_log, *ee_log, *loss_log;                 // the arm group
    int32_t* status_log;
};

// which log groups are given
struct RmpcStackLogs {
    int rmpc, stack, arm;
};

// 0 / 1: a group all null / all given; -1: given in part
int group_given(std::initializer_list<const void*> ps) {
    int set = 0;
    for (const void* p : ps) set += p != nullptr;
    return set == 0 ? 0 : set == (int)ps.size() ? 1 : -1;
}

// the checks that the loop-step and the rollout entries share: handle, configs (the rules of the RMPC loop entries and
// of the PMPC stack entries), counts, log groups
int common_check(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_rmpc_loop_config* c,
                 const dart_stack_config* scfg, int E, int n, int k, int steps, int log_rows, const RmpcStackBuf& p,
                 bool arm_logs, RmpcStackLogs* lg) {
    if (h->cfg.variant != DART_MPC_RMPC) return fail(h, DART_MPC_EINVAL, variant_text(DART_MPC_RMPC));
    if (!plant || !c || !scfg) return fail(h, DART_MPC_EINVAL, "null plant, loop or stack config");
    if (!lm && (!(plant->v_c > 0.0) || !(plant->mu_c >= 0.0)))
        return fail(h, DART_MPC_EINVAL, "plant config: v_c > 0, mu_c >= 0");
    if (!(c->rls_lambda > 0.0) || !(c->dr_max >= 0.0) || !(c->step_fraction >= 0.0 && c->step_fraction <= 1.0))
        return fail(h, DART_MPC_EINVAL, "loop config: rls_lambda > 0, dr_max >= 0, 0 <= step_fraction <= 1");
    if (scfg->couple != DART_STACK_RIDE && scfg->couple != DART_STACK_ACHIEVED)
        return fail(h, DART_MPC_EINVAL, "stack config: couple is DART_STACK_RIDE or DART_STACK_ACHIEVED");
    if (E < 1 || k < 0 || steps < 0 || log_rows < 0) return fail(h, DART_MPC_EINVAL, "bad experiment, step or row count");
    if (E > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "more experiments than B_max");
    if (n < 1 || n > DART_ARM_NMAX) return fail(h, DART_MPC_EINVAL, "joint count outside 1 .. DART_ARM_NMAX");
    lg->rmpc = lm ? group_given({p.log_pos_err, p.log_pos_err_norm, p.log_u_cmd, p.log_timestep, p.log_x, p.log_theta,
                                 p.log_r_v, p.log_f, p.log_status, p.log_iters, p.log_rot})
                  : group_given({p.log_pos_err, p.log_pos_err_norm, p.log_u_cmd, p.log_timestep, p.log_x, p.log_theta,
                                 p.log_r_v, p.log_f, p.log_status, p.log_iters});
    lg->stack = group_given({p.log_U, p.log_quat, p.log_tilt, p.log_tray});
    lg->arm = arm_logs ? group_given({p.q_log, p.qd_log, p.tau_log, p.ee_log, p.loss_log, p.status_log}) : 0;
    if (lg->rmpc < 0 || lg->stack < 0 || lg->arm < 0)
        return fail(h, DART_MPC_EINVAL, "null and non-null log pointers in one group (a group is given whole or not at all)");
    if ((lg->rmpc || lg->stack || lg->arm) && (long long)k + steps > log_rows)
        return fail(h, DART_MPC_EINVAL, "k0 + steps exceeds log_rows");
    return DART_MPC_OK;
}

dartmpc::RmpcStackStepArgs step_args(const dart_mpc_handle* h, const dart_plant_config* plant,
                                     const dart_rmpc_loop_config* c, const dart_stack_config* scfg, int E, int n, int k,
                                     int do_post, int do_pre, int log_rows, const RmpcStackLogs& lg, const RmpcStackBuf& p,
                                     const double* snap, const double* ee_quat, const LoopIo& io) {
    dartmpc::RmpcStackStepArgs a{};
    a.E = E; a.N = h->cfg.N; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
    a.logs = lg.rmpc; a.stack_logs = lg.stack; a.couple = scfg->couple;
    a.ee_stride = dartmpc::arm_snap_len(n);
    a.plant = plant_args(h, plant); a.a_lag = a.plant.a_lag;
    a.Ts = h->cfg.Ts; a.dr_max = c->dr_max; a.alpha_rg = c->alpha_rg; a.step_fraction = c->step_fraction;
    a.pos_tol = c->pos_tol;
    a.target = p.target; a.prm = p.prm; a.mu = p.mu; a.plant_pvec = p.plant_pvec; a.tray_pos = p.tray_pos;
    a.grasp = p.grasp;
    a.ee_pos = snap ? snap + 3 * n + 3 : nullptr;       // (the snapshot row: q qd qdd_prev mocap_pos ee_pos ...)
    a.ee_quat = ee_quat;
    a.x = p.x; a.tilt = p.tilt; a.prev = p.prev; a.u_prev = p.u_prev; a.r_v = p.r_v; a.theta = p.theta;
    a.done = p.done; a.nlog = p.nlog; a.metrics = p.metrics; a.stack_metrics = p.stack_metrics;
    a.x0 = io.x0; a.Rref = io.Rref; a.phi = io.phi; a.y = io.y; a.u0 = io.u0; a.f = io.f; a.status = io.status;
    a.iters = io.iters;
    a.log_pos_err = p.log_pos_err; a.log_pos_err_norm = p.log_pos_err_norm; a.log_u_cmd = p.log_u_cmd;
    a.log_timestep = p.log_timestep; a.log_x = p.log_x; a.log_theta = p.log_theta; a.log_r_v = p.log_r_v;
    a.log_f = p.log_f; a.log_status = p.log_status; a.log_iters = p.log_iters; a.log_rot = p.log_rot;
    a.log_U = p.log_U; a.log_quat = p.log_quat; a.log_tilt = p.log_tilt; a.log_tray = p.log_tray;
    return a;
}

template <class T> T* mut(const T* p) { return const_cast<T*>(p); }

// a loop-step entry: the checks, then one launch
int loop_step(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_rmpc_loop_config* c,
              const dart_stack_config* scfg, int E, int n, int k, int phase, int do_post, int do_pre, int log_rows,
              const RmpcStackBuf& p, const double* snap, const double* ee_quat, double* tray_cmd, const LoopIo& io,
              void* stream) {
    RmpcStackLogs lg{};
    if (int rc = common_check(h, lm, plant, c, scfg, E, n, k, phase == DART_STACK_COUPLE && do_post ? 1 : 0, log_rows, p,
                              false, &lg))
        return rc;
    if (phase != DART_STACK_COMMAND && phase != DART_STACK_COUPLE)
        return fail(h, DART_MPC_EINVAL, "phase is DART_STACK_COMMAND or DART_STACK_COUPLE");
    if (phase == DART_STACK_COMMAND) {
        if (any_null({io.u0, p.tray_pos, tray_cmd})) return fail(h, DART_MPC_EINVAL, "null pointer");
        HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
        const dartmpc::StackCommandArgs cmd{E, io.u0, p.tray_pos, tray_cmd};
        HIPCHK(h, dartmpc_launch_stack_command(&cmd, stream_of(h, stream)), "stack command kernel launch");
        return DART_MPC_OK;
    }
    if (any_null({p.target, p.prm, p.tray_pos, p.grasp, snap, ee_quat, p.x, p.tilt, p.prev, p.u_prev, p.r_v, p.theta,
                  p.done, p.nlog, p.metrics, p.stack_metrics, io.x0, io.Rref, io.phi, io.y, io.u0, io.f, io.status,
                  io.iters}) ||
        (lm ? !p.plant_pvec : !p.mu))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (!do_post && !do_pre) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    const dartmpc::RmpcStackStepArgs a = step_args(h, plant, c, scfg, E, n, k, do_post, do_pre, log_rows, lg, p, snap,
                                                   ee_quat, io);
    HIPCHK(h, dartmpc_launch_rmpc_stack_step(&a, lm, stream_of(h, stream)), "RMPC stack step kernel launch");
    return DART_MPC_OK;
}

// every check of a rollout entry (`host`: no work array, nlog is host memory)
int rollout_check(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_rmpc_loop_config* c,
                  const dart_stack_config* scfg, const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg, int E, int n,
                  int k0, int steps, int log_rows, int prm_stride, const RmpcStackBuf& p, bool host, RmpcStackLogs* lg) {
    if (int rc = common_check(h, lm, plant, c, scfg, E, n, k0, steps, log_rows, p, true, lg)) return rc;
    if (steps > (1 << 24) || !arm_dyn_ok(dcfg, E, n) || !arm_qp_ok(qcfg, n, prm_stride))
        return fail(h, DART_MPC_EINVAL, "arm dynamics or QP configuration (as dart_dual_arm_rollout)");
    if (any_null({p.target, p.prm, p.x, p.tilt, p.prev, p.u_prev, p.r_v, p.theta, p.P, p.w, p.done, p.nlog, p.metrics,
                  p.grasp, p.models, p.plant_models, p.arm_prm, p.q, p.qd, p.qdd_prev, p.arm_metrics, p.tray_pos,
                  p.stack_metrics}) ||
        (lm ? !p.plant_pvec : !p.mu) || (!host && !p.work))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (host)
        for (int b = 0; b < E; ++b)
            if (p.nlog[b] < 0) return fail(h, DART_MPC_EINVAL, "negative nlog");
    return DART_MPC_OK;
}

// the closed loop on device pointers, the handle's lock held: every check, then the launches
int closed_loop(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_rmpc_loop_config* c,
                const dart_stack_config* scfg, const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg, int E, int n,
                int k0, int steps, int log_rows, int prm_stride, const RmpcStackBuf& p, void* stream) {
    RmpcStackLogs lg{};
    if (int rc = rollout_check(h, lm, plant, c, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, prm_stride, p, false, &lg))
        return rc;
    if (steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    LoopIo L;
    if (int rc = loop_scratch(h, L)) return rc;
    hipStream_t s = stream_of(h, stream);
    const double* snap = p.work;
    double* ee_quat = p.work + dart_dual_arm_work_len(E, n);
    double* tray_cmd = ee_quat + 8 * (size_t)E;
    auto step = [&](int k, int post, int pre) {
        const dartmpc::RmpcStackStepArgs a = step_args(h, plant, c, scfg, E, n, k, post, pre, log_rows, lg, p, snap,
                                                       ee_quat, L);
        HIPCHK(h, dartmpc_launch_rmpc_stack_step(&a, lm, s), "RMPC stack step kernel launch");
        return (int)DART_MPC_OK;
    };
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        // the warm start in place and the fused RLS, exactly as dart_rmpc_rollout_dev calls the solve
        if (int rc = dart_rmpc_solve_batch_dev(h, E, L.x0, p.u_prev, p.theta, p.P, L.phi, L.y, c->rls_lambda, L.Rref, p.prm,
                                               p.w, L.u0, L.f, p.w, L.status, L.iters, s))
            return rc;
        const dartmpc::StackCommandArgs cmd{E, L.u0, p.tray_pos, tray_cmd};
        HIPCHK(h, dartmpc_launch_stack_command(&cmd, s), "stack command kernel launch");
        if (int rc = dual_arm_step(dcfg, qcfg, E, n, tray_cmd, p.grasp, p.models, p.plant_models, p.arm_prm, prm_stride,
                                   p.q, p.qd, p.qdd_prev, p.arm_metrics, p.work, ee_quat, (size_t)(k0 + j),
                                   lg.arm ? p.q_log : nullptr, p.qd_log, p.tau_log, p.ee_log, p.loss_log, p.status_log, s))
            return fail(h, rc, "arm step launch");
        if (int rc = step(k0 + j, 1, j + 1 < steps)) return rc;
    }
    return DART_MPC_OK;
}

// the host form: the arrays staged into the handle's arena around closed_loop; a log group that is not given is
// neither laid out nor moved; the episode rows travel both ways over the rows nlog .. nlog + steps
int closed_loop_host(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_rmpc_loop_config* c,
                     const dart_stack_config* scfg, const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg, int E,
                     int n, int k0, int steps, int log_rows, int prm_stride, const RmpcStackBuf& p, void* stream) {
    RmpcStackLogs lg{};
    if (int rc = rollout_check(h, lm, plant, c, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, prm_stride, p, true, &lg))
        return rc;
    if (steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream_of(h, stream);
    const size_t d = sizeof(double), i4 = sizeof(int32_t), nE = (size_t)E, B = 2 * nE, nn = (size_t)n;
    const size_t ML = dartmpc::arm_model_len(n), PL = dartmpc::arm_prm_len(n), nw = (size_t)dart_rmpc_nw(h->cfg.N);
    const size_t R = (size_t)log_rows, r0 = (size_t)k0, r1 = (size_t)k0 + steps;
    // episode rows: an experiment writes rows nlog[b] .. nlog[b] + steps - 1 at most
    int e0 = log_rows, e1 = 0;
    if (lg.rmpc) {
        for (int b = 0; b < E; ++b) {
            e0 = p.nlog[b] < e0 ? p.nlog[b] : e0;
            e1 = p.nlog[b] > e1 ? p.nlog[b] : e1;
        }
        e1 = (long long)e1 + steps < log_rows ? e1 + steps : log_rows;
        e0 = e0 < e1 ? e0 : e1;
    }
    RollStage S;
    auto up = [&](const void* host, size_t bytes) { return host ? S.add(host, bytes, false) : -1; };
    auto both = [&](void* host, size_t bytes) { return S.add(host, bytes, true); };
    auto log = [&](int given, void* host, size_t rowbytes) { return given ? S.add_log(host, R, rowbytes, r0, r1, false) : -1; };
    auto episode = [&](void* host, size_t rowbytes) {
        return lg.rmpc ? S.add_log(host, R, rowbytes, (size_t)e0, (size_t)e1, true) : -1;
    };
    const int i_target = up(p.target, d * 4 * nE), i_prm = up(p.prm, d * 10 * nE), i_mu = up(p.mu, d * nE);
    const int i_pvec = up(p.plant_pvec, d * 34 * nE);
    const int i_grasp = up(p.grasp, d * 14), i_models = up(p.models, d * 2 * ML), i_plantm = up(p.plant_models, d * 2 * ML);
    const int i_aprm = up(p.arm_prm, d * (prm_stride ? PL * B : PL)), i_tpos = up(p.tray_pos, d * 3 * nE);
    const int i_x = both(p.x, d * (lm ? 8 : 6) * nE), i_tilt = both(p.tilt, d * 2 * nE), i_prev = both(p.prev, d * 4 * nE);
    const int i_uprev = both(p.u_prev, d * 2 * nE), i_rv = both(p.r_v, d * 4 * nE), i_theta = both(p.theta, d * 14 * nE);
    const int i_P = both(p.P, d * 98 * nE), i_w = both(p.w, d * nw * nE);
    const int i_done = both(p.done, i4 * nE), i_nlog = both(p.nlog, i4 * nE), i_met = both(p.metrics, d * 8 * nE);
    const int i_q = both(p.q, d * nn * B), i_qd = both(p.qd, d * nn * B), i_qp = both(p.qdd_prev, d * nn * B);
    const int i_amet = both(p.arm_metrics, d * dartmpc::ARM_NMETRIC * B);
    const int i_smet = both(p.stack_metrics, d * dartmpc::STACK_NMETRIC * nE);
    const int i_work = S.add_rows(nullptr, 1, d * (size_t)dart_stack_work_len(E, n), 0, 0, false, false);
    const int l_perr = episode(p.log_pos_err, d * 2 * nE), l_pnorm = episode(p.log_pos_err_norm, d * nE);
    const int l_ucmd = episode(p.log_u_cmd, d * 2 * nE), l_time = episode(p.log_timestep, d * nE);
    const int l_x = log(lg.rmpc, p.log_x, d * 4 * nE), l_theta = log(lg.rmpc, p.log_theta, d * 14 * nE);
    const int l_rv = log(lg.rmpc, p.log_r_v, d * 4 * nE), l_f = log(lg.rmpc, p.log_f, d * nE);
    const int l_status = log(lg.rmpc, p.log_status, i4 * nE), l_iters = log(lg.rmpc, p.log_iters, i4 * nE);
    const int l_rot = log(lg.rmpc && lm, p.log_rot, d * 4 * nE);
    const int l_U = log(lg.stack, p.log_U, d * 2 * nE), l_quat = log(lg.stack, p.log_quat, d * 4 * nE);
    const int l_tilt = log(lg.stack, p.log_tilt, d * 2 * nE), l_tray = log(lg.stack, p.log_tray, d * 7 * nE);
    const int l_q = log(lg.arm, p.q_log, d * nn * B), l_qd = log(lg.arm, p.qd_log, d * nn * B);
    const int l_tau = log(lg.arm, p.tau_log, d * nn * B), l_ee = log(lg.arm, p.ee_log, d * 3 * B);
    const int l_aloss = log(lg.arm, p.loss_log, d * B), l_astatus = log(lg.arm, p.status_log, i4 * B);
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    auto D = [&](int i) { return S.dev<double>(h, i); };
    auto I = [&](int i) { return S.dev<int32_t>(h, i); };
    RmpcStackBuf v{};
    v.target = D(i_target); v.prm = D(i_prm); v.mu = D(i_mu); v.plant_pvec = D(i_pvec); v.grasp = D(i_grasp);
    v.models = D(i_models); v.plant_models = D(i_plantm); v.arm_prm = D(i_aprm); v.tray_pos = D(i_tpos);
    v.x = D(i_x); v.tilt = D(i_tilt); v.prev = D(i_prev); v.u_prev = D(i_uprev); v.r_v = D(i_rv); v.theta = D(i_theta);
    v.P = D(i_P); v.w = D(i_w); v.done = I(i_done); v.nlog = I(i_nlog); v.metrics = D(i_met);
    v.q = D(i_q); v.qd = D(i_qd); v.qdd_prev = D(i_qp); v.arm_metrics = D(i_amet); v.stack_metrics = D(i_smet);
    v.work = D(i_work);
    v.log_pos_err = D(l_perr); v.log_pos_err_norm = D(l_pnorm); v.log_u_cmd = D(l_ucmd); v.log_timestep = D(l_time);
    v.log_x = D(l_x); v.log_theta = D(l_theta); v.log_r_v = D(l_rv); v.log_f = D(l_f); v.log_status = I(l_status);
    v.log_iters = I(l_iters); v.log_rot = D(l_rot);
    v.log_U = D(l_U); v.log_quat = D(l_quat); v.log_tilt = D(l_tilt); v.log_tray = D(l_tray);
    v.q_log = D(l_q); v.qd_log = D(l_qd); v.tau_log = D(l_tau); v.ee_log = D(l_ee); v.loss_log = D(l_aloss);
    v.status_log = I(l_astatus);
    if (int rc = closed_loop(h, lm, plant, c, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, prm_stride, v, s)) return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

}  // namespace

// the entries' parameter lists, stated once: the RMPC loop's in/out state, the three log groups
#define RS_STATE double *x, double *tilt, double *prev, double *u_prev, double *r_v
#define RS_RMPC_LOGS_DECL                                                                                    \
    double *log_pos_err, double *log_pos_err_norm, double *log_u_cmd, double *log_timestep, double *log_x,  \
        double *log_theta, double *log_r_v, double *log_f, int32_t *log_status, int32_t *log_iters
#define RS_STACK_LOGS_DECL double *log_U, double *log_quat, double *log_tilt, double *log_tray
#define RS_ARM_LOGS_DECL \
    double *q_log, double *qd_log, double *tau_log, double *ee_log, double *loss_log, int32_t *status_log
#define RS_ARM_DECL                                                                                              \
    const double *grasp, const double *models, const double *plant_models, const double *arm_prm, double *q, \
        double *qd, double *qdd_prev, double *arm_metrics
#define RS_SET_RMPC_LOGS(p)                                                                                            \
    p.log_pos_err = log_pos_err; p.log_pos_err_norm = log_pos_err_norm; p.log_u_cmd = log_u_cmd;                       \
    p.log_timestep = log_timestep; p.log_x = log_x; p.log_theta = log_theta; p.log_r_v = log_r_v; p.log_f = log_f;     \
    p.log_status = log_status; p.log_iters = log_iters;                                                                \
    p.log_U = log_U; p.log_quat = log_quat; p.log_tilt = log_tilt; p.log_tray = log_tray
#define RS_SET_STATE(p)                                                                                                \
    p.target = target; p.prm = prm; p.x = x; p.tilt = tilt; p.prev = prev; p.u_prev = u_prev; p.r_v = r_v;             \
    p.done = done; p.nlog = nlog; p.metrics = metrics; p.tray_pos = tray_pos; p.grasp = grasp;                         \
    p.stack_metrics = stack_metrics
#define RS_SET_ROLLOUT(p)                                                                                              \
    RS_SET_STATE(p); p.theta = theta; p.P = P; p.w = w; p.models = models; p.plant_models = plant_models;              \
    p.arm_prm = arm_prm; p.q = q; p.qd = qd; p.qdd_prev = qdd_prev; p.arm_metrics = arm_metrics;                       \
    RS_SET_RMPC_LOGS(p);                                                                                               \
    p.q_log = q_log; p.qd_log = qd_log; p.tau_log = tau_log; p.ee_log = ee_log; p.loss_log = loss_log;                 \
    p.status_log = status_log

int dart_rmpc_stack_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                                  const dart_stack_config* scfg, int E, int n, int k, int phase, int do_post, int do_pre,
                                  int log_rows, const double* target, const double* prm, const double* mu,
                                  const double* tray_pos, const double* grasp, const double* snap, const double* ee_quat,
                                  RS_STATE, const double* theta, int32_t* done, int32_t* nlog, double* metrics,
                                  double* stack_metrics, double* x0, double* Rref, double* phi, double* y, double* tray_cmd,
                                  const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                                  RS_RMPC_LOGS_DECL, RS_STACK_LOGS_DECL, void* stream) {
    DART_ENTER(h, -1);
    RmpcStackBuf p{};
    RS_SET_STATE(p); p.mu = mu; p.theta = mut(theta);
    RS_SET_RMPC_LOGS(p);
    return loop_step(h, false, plant, loop, scfg, E, n, k, phase, do_post, do_pre, log_rows, p, snap, ee_quat, tray_cmd,
                     {x0, Rref, phi, y, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

int dart_rmpc_stack_lm_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                                     const dart_stack_config* scfg, int E, int n, int k, int phase, int do_post, int do_pre,
                                     int log_rows, const double* target, const double* prm, const double* plant_pvec,
                                     const double* tray_pos, const double* grasp, const double* snap, const double* ee_quat,
                                     RS_STATE, const double* theta, int32_t* done, int32_t* nlog, double* metrics,
                                     double* stack_metrics, double* x0, double* Rref, double* phi, double* y,
                                     double* tray_cmd, const double* u0, const double* f, const int32_t* status,
                                     const int32_t* iters, RS_RMPC_LOGS_DECL, double* log_rot, RS_STACK_LOGS_DECL,
                                     void* stream) {
    DART_ENTER(h, -1);
    RmpcStackBuf p{};
    RS_SET_STATE(p); p.plant_pvec = plant_pvec; p.theta = mut(theta);
    RS_SET_RMPC_LOGS(p); p.log_rot = log_rot;
    return loop_step(h, true, plant, loop, scfg, E, n, k, phase, do_post, do_pre, log_rows, p, snap, ee_quat, tray_cmd,
                     {x0, Rref, phi, y, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

int dart_rmpc_stack_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                                const dart_stack_config* scfg, const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg,
                                int E, int n, int k0, int steps, int log_rows, int arm_prm_stride, const double* target,
                                const double* prm, const double* mu, RS_STATE, double* theta, double* P, double* w,
                                int32_t* done, int32_t* nlog, double* metrics, RS_ARM_DECL, double* work,
                                const double* tray_pos, double* stack_metrics, RS_RMPC_LOGS_DECL, RS_STACK_LOGS_DECL,
                                RS_ARM_LOGS_DECL, void* stream) {
    DART_ENTER(h, -1);
    RmpcStackBuf p{};
    RS_SET_ROLLOUT(p); p.mu = mu; p.work = work;
    return closed_loop(h, false, plant, loop, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride, p, stream);
}

int dart_rmpc_stack_lm_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                                   const dart_stack_config* scfg, const dart_arm_dyn_config* dcfg,
                                   const dart_arm_config* qcfg, int E, int n, int k0, int steps, int log_rows,
                                   int arm_prm_stride, const double* target, const double* prm, const double* plant_pvec,
                                   RS_STATE, double* theta, double* P, double* w, int32_t* done, int32_t* nlog,
                                   double* metrics, RS_ARM_DECL, double* work, const double* tray_pos,
                                   double* stack_metrics, RS_RMPC_LOGS_DECL, double* log_rot, RS_STACK_LOGS_DECL,
                                   RS_ARM_LOGS_DECL, void* stream) {
    DART_ENTER(h, -1);
    RmpcStackBuf p{};
    RS_SET_ROLLOUT(p); p.plant_pvec = plant_pvec; p.work = work; p.log_rot = log_rot;
    return closed_loop(h, true, plant, loop, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride, p, stream);
}

int dart_rmpc_stack_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                            const dart_stack_config* scfg, const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg,
                            int E, int n, int k0, int steps, int log_rows, int arm_prm_stride, const double* target,
                            const double* prm, const double* mu, RS_STATE, double* theta, double* P, double* w,
                            int32_t* done, int32_t* nlog, double* metrics, RS_ARM_DECL, const double* tray_pos,
                            double* stack_metrics, RS_RMPC_LOGS_DECL, RS_STACK_LOGS_DECL, RS_ARM_LOGS_DECL, void* stream) {
    DART_ENTER(h, -1);
    RmpcStackBuf p{};
    RS_SET_ROLLOUT(p); p.mu = mu;
    return closed_loop_host(h, false, plant, loop, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride, p, stream);
}

int dart_rmpc_stack_lm_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                               const dart_stack_config* scfg, const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg,
                               int E, int n, int k0, int steps, int log_rows, int arm_prm_stride, const double* target,
                               const double* prm, const double* plant_pvec, RS_STATE, double* theta, double* P, double* w,
                               int32_t* done, int32_t* nlog, double* metrics, RS_ARM_DECL, const double* tray_pos,
                               double* stack_metrics, RS_RMPC_LOGS_DECL, double* log_rot, RS_STACK_LOGS_DECL,
                               RS_ARM_LOGS_DECL, void* stream) {
    DART_ENTER(h, -1);
    RmpcStackBuf p{};
    RS_SET_ROLLOUT(p); p.plant_pvec = plant_pvec; p.log_rot = log_rot;
    return closed_loop_host(h, true, plant, loop, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride, p, stream);
}
