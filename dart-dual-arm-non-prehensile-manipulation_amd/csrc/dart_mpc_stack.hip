// dart_mpc_stack.hip -- the stack entries of include/dart_mpc.h (host side): the PMPC closed loop through the dual-arm
// layer.  Per step the unchanged PMPC solve, stack_command_kernel, the arm layer's step (dart_mpc_arm.hip
// dual_arm_step: dynamics, QP, plant) and stack_step_kernel (stack_step.hip), on one stream.
#include "abi_internal.h"
#include "arm_dyn.h"
#include "stack_step.h"

void dart_stack_config_default(dart_stack_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->couple = DART_STACK_ACHIEVED;
}

// the arm rollout's work, then ee_quat [2 E][4] and tray_cmd [E][7]
int dart_stack_work_len(int E, int n) {
    const int arm = dart_dual_arm_work_len(E, n);
    return arm < 0 ? arm : arm + 15 * E;
}

namespace {

static_assert(DART_STACK_RIDE == dartmpc::STACK_RIDE && DART_STACK_ACHIEVED == dartmpc::STACK_ACHIEVED, "one couple enum");

// every array of the stack loop, as the entries take them (the tray plant's entries leave plant_pvec, pz_vz and
// log_rot null)
struct StackBuf {
    const double *target, *prm, *plant_pvec, *pz_vz;
    double *x, *tilt, *metrics;
    const double *grasp, *models, *plant_models, *arm_prm;
    double *q, *qd, *qdd_prev, *arm_metrics, *work;
    const double* tray_pos;
    double* stack_metrics;
    double *log_X, *log_U, *log_quat, *log_loss;
    int32_t *log_status, *log_iters;
    double* log_rot;
    double *log_tilt, *log_tray;
    double *q_log, *qd_log, *tau_log, *ee_log, *loss_log;
    int32_t* status_log;
};

// which log groups are given
struct StackLogs {
    int pmpc, stack, arm;
};

// 0 / 1: a group all null / all given; -1: given in part
int group_given(std::initializer_list<const void*> ps) {
    int set = 0;
    for (const void* p : ps) set += p != nullptr;
    return set == 0 ? 0 : set == (int)ps.size() ? 1 : -1;
}

// the checks that the loop-step and the rollout entries share: handle, configs, counts, log groups
int stack_common_check(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_stack_config* scfg, int E,
                       int n, int k, int steps, int log_rows, const StackBuf& p, bool arm_logs, StackLogs* lg) {
    if (h->cfg.variant != DART_MPC_PMPC) return fail(h, DART_MPC_EINVAL, variant_text(DART_MPC_PMPC));
    if (!plant || !scfg) return fail(h, DART_MPC_EINVAL, "null plant or stack config");
    if (!lm && (!(plant->v_c > 0.0) || !(plant->mu_c >= 0.0)))
        return fail(h, DART_MPC_EINVAL, "plant config: v_c > 0, mu_c >= 0");
    if (scfg->couple != DART_STACK_RIDE && scfg->couple != DART_STACK_ACHIEVED)
        return fail(h, DART_MPC_EINVAL, "stack config: couple is DART_STACK_RIDE or DART_STACK_ACHIEVED");
    if (E < 1 || k < 0 || steps < 0 || log_rows < 0) return fail(h, DART_MPC_EINVAL, "bad experiment, step or row count");
    if (E > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "more experiments than B_max");
    if (n < 1 || n > DART_ARM_NMAX) return fail(h, DART_MPC_EINVAL, "joint count outside 1 .. DART_ARM_NMAX");
    lg->pmpc = lm ? group_given({p.log_X, p.log_U, p.log_quat, p.log_loss, p.log_status, p.log_iters, p.log_rot})
                  : group_given({p.log_X, p.log_U, p.log_quat, p.log_loss, p.log_status, p.log_iters});
    lg->stack = group_given({p.log_tilt, p.log_tray});
    lg->arm = arm_logs ? group_given({p.q_log, p.qd_log, p.tau_log, p.ee_log, p.loss_log, p.status_log}) : 0;
    if (lg->pmpc < 0 || lg->stack < 0 || lg->arm < 0)
        return fail(h, DART_MPC_EINVAL, "null and non-null log pointers in one group (a group is given whole or not at all)");
    if ((lg->pmpc || lg->stack || lg->arm) && (long long)k + steps > log_rows)
        return fail(h, DART_MPC_EINVAL, "k0 + steps exceeds log_rows");
    return DART_MPC_OK;
}

dartmpc::StackStepArgs step_args(const dart_mpc_handle* h, const dart_plant_config* plant, const dart_stack_config* scfg,
                                 int E, int n, int k, int do_post, int do_pre, int log_rows, const StackLogs& lg,
                                 const StackBuf& p, const double* snap, const double* ee_quat, const LoopIo& io) {
    dartmpc::StackStepArgs a{};
    a.E = E; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
    a.logs = lg.pmpc; a.stack_logs = lg.stack; a.couple = scfg->couple;
    a.ee_stride = dartmpc::arm_snap_len(n);
    a.plant = plant_args(h, plant); a.a_lag = a.plant.a_lag; a.Ts = h->cfg.Ts;
    a.prm = p.prm; a.target = p.target; a.plant_pvec = p.plant_pvec; a.pz_vz = p.pz_vz;
    a.tray_pos = p.tray_pos; a.grasp = p.grasp;
    a.ee_pos = snap ? snap + 3 * n + 3 : nullptr;       // (the snapshot row: q qd qdd_prev mocap_pos ee_pos ...)
    a.ee_quat = ee_quat;
    a.x = p.x; a.tilt = p.tilt; a.metrics = p.metrics; a.stack_metrics = p.stack_metrics;
    a.x0 = io.x0; a.u0 = io.u0; a.f = io.f; a.status = io.status; a.iters = io.iters;
    a.log_X = p.log_X; a.log_U = p.log_U; a.log_quat = p.log_quat; a.log_loss = p.log_loss;
    a.log_status = p.log_status; a.log_iters = p.log_iters; a.log_rot = p.log_rot;
    a.log_tilt = p.log_tilt; a.log_tray = p.log_tray;
    return a;
}

template <class T> T* mut(const T* p) { return const_cast<T*>(p); }

// a loop-step entry: the checks, then one launch
int stack_loop_step(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_stack_config* scfg, int E,
                    int n, int k, int phase, int do_post, int do_pre, int log_rows, const StackBuf& p, const double* snap,
                    const double* ee_quat, double* tray_cmd, const LoopIo& io, void* stream) {
    StackLogs lg{};
    if (int rc = stack_common_check(h, lm, plant, scfg, E, n, k, phase == DART_STACK_COUPLE && do_post ? 1 : 0, log_rows, p,
                                    false, &lg))
        return rc;
    if (phase != DART_STACK_COMMAND && phase != DART_STACK_COUPLE)
        return fail(h, DART_MPC_EINVAL, "phase is DART_STACK_COMMAND or DART_STACK_COUPLE");
    if (phase == DART_STACK_COMMAND) {
        if (any_null({io.u0, p.tray_pos, tray_cmd})) return fail(h, DART_MPC_EINVAL, "null pointer");
        HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
        const dartmpc::StackCommandArgs c{E, io.u0, p.tray_pos, tray_cmd};
        HIPCHK(h, dartmpc_launch_stack_command(&c, stream_of(h, stream)), "stack command kernel launch");
        return DART_MPC_OK;
    }
    if (any_null({p.target, p.tray_pos, p.grasp, snap, ee_quat, p.x, p.tilt, p.metrics, p.stack_metrics, io.x0, io.u0,
                  io.f, io.status, io.iters}) ||
        (lm ? any_null({p.plant_pvec, p.pz_vz}) : any_null({p.prm})))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (!do_post && !do_pre) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    const dartmpc::StackStepArgs a = step_args(h, plant, scfg, E, n, k, do_post, do_pre, log_rows, lg, p, snap, ee_quat, io);
    HIPCHK(h, dartmpc_launch_stack_step(&a, lm, stream_of(h, stream)), "stack step kernel launch");
    return DART_MPC_OK;
}

// every check of a rollout entry (`host`: no work array)
int stack_rollout_check(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_stack_config* scfg,
                        const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg, int E, int n, int k0, int steps,
                        int log_rows, int prm_stride, const StackBuf& p, bool host, StackLogs* lg) {
    if (int rc = stack_common_check(h, lm, plant, scfg, E, n, k0, steps, log_rows, p, true, lg)) return rc;
    if (steps > (1 << 24) || !arm_dyn_ok(dcfg, E, n) || !arm_qp_ok(qcfg, n, prm_stride))
        return fail(h, DART_MPC_EINVAL, "arm dynamics or QP configuration (as dart_dual_arm_rollout)");
    if (any_null({p.target, p.prm, p.x, p.tilt, p.metrics, p.grasp, p.models, p.plant_models, p.arm_prm, p.q, p.qd,
                  p.qdd_prev, p.arm_metrics, p.tray_pos, p.stack_metrics}) ||
        (lm && any_null({p.plant_pvec, p.pz_vz})) || (!host && !p.work))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    return DART_MPC_OK;
}

// the closed loop on device pointers, the handle's lock held: every check, then the launches
int stack_closed_loop(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_stack_config* scfg,
                      const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg, int E, int n, int k0, int steps,
                      int log_rows, int prm_stride, const StackBuf& p, void* stream) {
    StackLogs lg{};
    if (int rc = stack_rollout_check(h, lm, plant, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, prm_stride, p, false, &lg))
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
        const dartmpc::StackStepArgs a = step_args(h, plant, scfg, E, n, k, post, pre, log_rows, lg, p, snap, ee_quat, L);
        HIPCHK(h, dartmpc_launch_stack_step(&a, lm, s), "stack step kernel launch");
        return (int)DART_MPC_OK;
    };
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        if (int rc = dart_mpc_solve_batch_dev(h, E, L.x0, p.target, p.prm, nullptr, L.u0, L.f, nullptr, L.status, L.iters, s))
            return rc;
        const dartmpc::StackCommandArgs c{E, L.u0, p.tray_pos, tray_cmd};
        HIPCHK(h, dartmpc_launch_stack_command(&c, s), "stack command kernel launch");
        if (int rc = dual_arm_step(dcfg, qcfg, E, n, tray_cmd, p.grasp, p.models, p.plant_models, p.arm_prm, prm_stride,
                                   p.q, p.qd, p.qdd_prev, p.arm_metrics, p.work, ee_quat, (size_t)(k0 + j),
                                   lg.arm ? p.q_log : nullptr, p.qd_log, p.tau_log, p.ee_log, p.loss_log, p.status_log, s))
            return fail(h, rc, "arm step launch");
        if (int rc = step(k0 + j, 1, j + 1 < steps)) return rc;
    }
    return DART_MPC_OK;
}

// the host form: the arrays staged into the handle's arena around stack_closed_loop; a log group that is not given is
// neither laid out nor moved
int stack_closed_loop_host(dart_mpc_handle* h, bool lm, const dart_plant_config* plant, const dart_stack_config* scfg,
                           const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg, int E, int n, int k0, int steps,
                           int log_rows, int prm_stride, const StackBuf& p, void* stream) {
    StackLogs lg{};
    if (int rc = stack_rollout_check(h, lm, plant, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, prm_stride, p, true, &lg))
        return rc;
    if (steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    if (int rc = settle_pending(h)) return rc;
    hipStream_t s = stream_of(h, stream);
    const size_t d = sizeof(double), nE = (size_t)E, B = 2 * nE, nn = (size_t)n;
    const size_t ML = dartmpc::arm_model_len(n), PL = dartmpc::arm_prm_len(n);
    const size_t R = (size_t)log_rows, r0 = (size_t)k0, r1 = (size_t)k0 + steps;
    RollStage S;
    auto up = [&](const void* host, size_t bytes) { return host ? S.add(host, bytes, false) : -1; };
    auto both = [&](void* host, size_t bytes) { return S.add(host, bytes, true); };
    auto log = [&](int given, void* host, size_t rowbytes) { return given ? S.add_log(host, R, rowbytes, r0, r1, false) : -1; };
    const int i_target = up(p.target, d * 6 * nE), i_prm = up(p.prm, d * 6 * nE);
    const int i_pvec = up(p.plant_pvec, d * 34 * nE), i_pzvz = up(p.pz_vz, d * 2 * nE);
    const int i_grasp = up(p.grasp, d * 14), i_models = up(p.models, d * 2 * ML), i_plantm = up(p.plant_models, d * 2 * ML);
    const int i_aprm = up(p.arm_prm, d * (prm_stride ? PL * B : PL)), i_tpos = up(p.tray_pos, d * 3 * nE);
    const int i_x = both(p.x, d * (lm ? 8 : 6) * nE), i_tilt = both(p.tilt, d * 2 * nE), i_met = both(p.metrics, d * 8 * nE);
    const int i_q = both(p.q, d * nn * B), i_qd = both(p.qd, d * nn * B), i_qp = both(p.qdd_prev, d * nn * B);
    const int i_amet = both(p.arm_metrics, d * dartmpc::ARM_NMETRIC * B);
    const int i_smet = both(p.stack_metrics, d * dartmpc::STACK_NMETRIC * nE);
    const int i_work = S.add_rows(nullptr, 1, d * (size_t)dart_stack_work_len(E, n), 0, 0, false, false);
    const int l_X = log(lg.pmpc, p.log_X, d * 6 * nE), l_U = log(lg.pmpc, p.log_U, d * 2 * nE);
    const int l_quat = log(lg.pmpc, p.log_quat, d * 4 * nE), l_loss = log(lg.pmpc, p.log_loss, d * nE);
    const int l_status = log(lg.pmpc, p.log_status, sizeof(int32_t) * nE), l_iters = log(lg.pmpc, p.log_iters, sizeof(int32_t) * nE);
    const int l_rot = log(lg.pmpc && lm, p.log_rot, d * 4 * nE);
    const int l_tilt = log(lg.stack, p.log_tilt, d * 2 * nE), l_tray = log(lg.stack, p.log_tray, d * 7 * nE);
    const int l_q = log(lg.arm, p.q_log, d * nn * B), l_qd = log(lg.arm, p.qd_log, d * nn * B);
    const int l_tau = log(lg.arm, p.tau_log, d * nn * B), l_ee = log(lg.arm, p.ee_log, d * 3 * B);
    const int l_aloss = log(lg.arm, p.loss_log, d * B), l_astatus = log(lg.arm, p.status_log, sizeof(int32_t) * B);
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    StackBuf v{};
    v.target = S.dev<double>(h, i_target); v.prm = S.dev<double>(h, i_prm); v.plant_pvec = S.dev<double>(h, i_pvec);
    v.pz_vz = S.dev<double>(h, i_pzvz); v.grasp = S.dev<double>(h, i_grasp); v.models = S.dev<double>(h, i_models);
    v.plant_models = S.dev<double>(h, i_plantm); v.arm_prm = S.dev<double>(h, i_aprm); v.tray_pos = S.dev<double>(h, i_tpos);
    v.x = S.dev<double>(h, i_x); v.tilt = S.dev<double>(h, i_tilt); v.metrics = S.dev<double>(h, i_met);
    v.q = S.dev<double>(h, i_q); v.qd = S.dev<double>(h, i_qd); v.qdd_prev = S.dev<double>(h, i_qp);
    v.arm_metrics = S.dev<double>(h, i_amet); v.stack_metrics = S.dev<double>(h, i_smet); v.work = S.dev<double>(h, i_work);
    v.log_X = S.dev<double>(h, l_X); v.log_U = S.dev<double>(h, l_U); v.log_quat = S.dev<double>(h, l_quat);
    v.log_loss = S.dev<double>(h, l_loss); v.log_status = S.dev<int32_t>(h, l_status); v.log_iters = S.dev<int32_t>(h, l_iters);
    v.log_rot = S.dev<double>(h, l_rot); v.log_tilt = S.dev<double>(h, l_tilt); v.log_tray = S.dev<double>(h, l_tray);
    v.q_log = S.dev<double>(h, l_q); v.qd_log = S.dev<double>(h, l_qd); v.tau_log = S.dev<double>(h, l_tau);
    v.ee_log = S.dev<double>(h, l_ee); v.loss_log = S.dev<double>(h, l_aloss); v.status_log = S.dev<int32_t>(h, l_astatus);
    if (int rc = stack_closed_loop(h, lm, plant, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, prm_stride, v, s)) return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

bool tray_from_arms_ok(int E, std::initializer_list<const void*> ps) { return E >= 1 && E <= (1 << 20) && !any_null(ps); }

}  // namespace

int dart_tray_from_arms_dev(int E, const double* ee_pos, const double* ee_quat, const double* grasp, double* tray,
                            double* tilt, double* diag, void* stream) {
    if (!tray_from_arms_ok(E, {ee_pos, ee_quat, grasp, tray, tilt, diag})) return DART_MPC_EINVAL;
    const dartmpc::TrayFromArmsArgs a{E, 3, ee_pos, ee_quat, grasp, tray, tilt, diag};
    return dartmpc_launch_tray_from_arms(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_tray_from_arms(int E, const double* ee_pos, const double* ee_quat, const double* grasp, double* tray,
                        double* tilt, double* diag) {
    if (!tray_from_arms_ok(E, {ee_pos, ee_quat, grasp, tray, tilt, diag})) return DART_MPC_EINVAL;
    const size_t nE = (size_t)E;
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(sizeof(double) * (14 * nE + 14) + 3 * 256, sizeof(double) * 12 * nE + 3 * 256) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    const double* d_pos = S.in(ee_pos, 6 * nE);
    const double* d_quat = S.in(ee_quat, 8 * nE);
    const double* d_grasp = S.in(grasp, 14);
    double* d_tray = S.out<double>(7 * nE);
    double* d_tilt = S.out<double>(2 * nE);
    double* d_diag = S.out<double>(3 * nE);
    if (!D->run([&](hipStream_t s) {
            return dart_tray_from_arms_dev(E, d_pos, d_quat, d_grasp, d_tray, d_tilt, d_diag, s) == DART_MPC_OK
                       ? hipSuccess : hipErrorUnknown;
        }))
        return DART_MPC_EHIP;
    S.take(tray, d_tray, 7 * nE); S.take(tilt, d_tilt, 2 * nE); S.take(diag, d_diag, 3 * nE);
    return DART_MPC_OK;
}

#define STACK_PMPC_LOGS log_X, log_U, log_quat, log_loss, log_status, log_iters
#define STACK_ARM_LOGS q_log, qd_log, tau_log, ee_log, loss_log, status_log

int dart_pmpc_stack_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_stack_config* scfg,
                                  int E, int n, int k, int phase, int do_post, int do_pre, int log_rows,
                                  const double* target, const double* prm, const double* tray_pos, const double* grasp,
                                  const double* snap, const double* ee_quat,
                                  double* x, double* tilt, double* metrics, double* stack_metrics,
                                  double* x0, double* tray_cmd,
                                  const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                                  double* log_X, double* log_U, double* log_quat, double* log_loss,
                                  int32_t* log_status, int32_t* log_iters, double* log_tilt, double* log_tray,
                                  void* stream) {
    DART_ENTER(h, -1);
    StackBuf p{};
    p.target = target; p.prm = prm; p.tray_pos = tray_pos; p.grasp = grasp; p.x = x; p.tilt = tilt; p.metrics = metrics;
    p.stack_metrics = stack_metrics; p.log_X = log_X; p.log_U = log_U; p.log_quat = log_quat; p.log_loss = log_loss;
    p.log_status = log_status; p.log_iters = log_iters; p.log_tilt = log_tilt; p.log_tray = log_tray;
    return stack_loop_step(h, false, plant, scfg, E, n, k, phase, do_post, do_pre, log_rows, p, snap, ee_quat, tray_cmd,
                           {x0, nullptr, nullptr, nullptr, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

int dart_pmpc_stack_lm_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_stack_config* scfg,
                                     int E, int n, int k, int phase, int do_post, int do_pre, int log_rows,
                                     const double* target, const double* plant_pvec, const double* pz_vz,
                                     const double* tray_pos, const double* grasp,
                                     const double* snap, const double* ee_quat,
                                     double* x, double* tilt, double* metrics, double* stack_metrics,
                                     double* x0, double* tray_cmd,
                                     const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                                     double* log_X, double* log_U, double* log_quat, double* log_loss,
                                     int32_t* log_status, int32_t* log_iters, double* log_rot,
                                     double* log_tilt, double* log_tray, void* stream) {
    DART_ENTER(h, -1);
    StackBuf p{};
    p.target = target; p.plant_pvec = plant_pvec; p.pz_vz = pz_vz; p.tray_pos = tray_pos; p.grasp = grasp; p.x = x;
    p.tilt = tilt; p.metrics = metrics; p.stack_metrics = stack_metrics; p.log_X = log_X; p.log_U = log_U;
    p.log_quat = log_quat; p.log_loss = log_loss; p.log_status = log_status; p.log_iters = log_iters; p.log_rot = log_rot;
    p.log_tilt = log_tilt; p.log_tray = log_tray;
    return stack_loop_step(h, true, plant, scfg, E, n, k, phase, do_post, do_pre, log_rows, p, snap, ee_quat, tray_cmd,
                           {x0, nullptr, nullptr, nullptr, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

namespace {

StackBuf rollout_buf(const double* target, const double* prm, const double* plant_pvec, const double* pz_vz, double* x,
                     double* tilt, double* metrics, const double* grasp, const double* models, const double* plant_models,
                     const double* arm_prm, double* q, double* qd, double* qdd_prev, double* arm_metrics, double* work,
                     const double* tray_pos, double* stack_metrics, double* log_X, double* log_U, double* log_quat,
                     double* log_loss, int32_t* log_status, int32_t* log_iters, double* log_rot, double* log_tilt,
                     double* log_tray, double* q_log, double* qd_log, double* tau_log, double* ee_log, double* loss_log,
                     int32_t* status_log) {
    StackBuf p{};
    p.target = target; p.prm = prm; p.plant_pvec = plant_pvec; p.pz_vz = pz_vz; p.x = x; p.tilt = tilt; p.metrics = metrics;
    p.grasp = grasp; p.models = models; p.plant_models = plant_models; p.arm_prm = arm_prm; p.q = q; p.qd = qd;
    p.qdd_prev = qdd_prev; p.arm_metrics = arm_metrics; p.work = work; p.tray_pos = tray_pos; p.stack_metrics = stack_metrics;
    p.log_X = log_X; p.log_U = log_U; p.log_quat = log_quat; p.log_loss = log_loss; p.log_status = log_status;
    p.log_iters = log_iters; p.log_rot = log_rot; p.log_tilt = log_tilt; p.log_tray = log_tray;
    p.q_log = q_log; p.qd_log = qd_log; p.tau_log = tau_log; p.ee_log = ee_log; p.loss_log = loss_log; p.status_log = status_log;
    return p;
}

}  // namespace

int dart_pmpc_stack_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_stack_config* scfg,
                                const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg,
                                int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                                const double* target, const double* prm, double* x, double* tilt, double* metrics,
                                const double* grasp, const double* models, const double* plant_models,
                                const double* arm_prm, double* q, double* qd, double* qdd_prev, double* arm_metrics,
                                double* work, const double* tray_pos, double* stack_metrics,
                                double* log_X, double* log_U, double* log_quat, double* log_loss,
                                int32_t* log_status, int32_t* log_iters, double* log_tilt, double* log_tray,
                                double* q_log, double* qd_log, double* tau_log, double* ee_log, double* loss_log,
                                int32_t* status_log, void* stream) {
    DART_ENTER(h, -1);
    return stack_closed_loop(h, false, plant, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride,
                             rollout_buf(target, prm, nullptr, nullptr, x, tilt, metrics, grasp, models, plant_models,
                                         arm_prm, q, qd, qdd_prev, arm_metrics, work, tray_pos, stack_metrics,
                                         STACK_PMPC_LOGS, nullptr, log_tilt, log_tray, STACK_ARM_LOGS), stream);
}

int dart_pmpc_stack_lm_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_stack_config* scfg,
                                   const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg,
                                   int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                                   const double* target, const double* prm, const double* plant_pvec,
                                   const double* pz_vz, double* x, double* tilt, double* metrics,
                                   const double* grasp, const double* models, const double* plant_models,
                                   const double* arm_prm, double* q, double* qd, double* qdd_prev, double* arm_metrics,
                                   double* work, const double* tray_pos, double* stack_metrics,
                                   double* log_X, double* log_U, double* log_quat, double* log_loss,
                                   int32_t* log_status, int32_t* log_iters, double* log_rot,
                                   double* log_tilt, double* log_tray,
                                   double* q_log, double* qd_log, double* tau_log, double* ee_log, double* loss_log,
                                   int32_t* status_log, void* stream) {
    DART_ENTER(h, -1);
    return stack_closed_loop(h, true, plant, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride,
                             rollout_buf(target, prm, plant_pvec, pz_vz, x, tilt, metrics, grasp, models, plant_models,
                                         arm_prm, q, qd, qdd_prev, arm_metrics, work, tray_pos, stack_metrics,
                                         STACK_PMPC_LOGS, log_rot, log_tilt, log_tray, STACK_ARM_LOGS), stream);
}

int dart_pmpc_stack_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_stack_config* scfg,
                            const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg,
                            int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                            const double* target, const double* prm, double* x, double* tilt, double* metrics,
                            const double* grasp, const double* models, const double* plant_models,
                            const double* arm_prm, double* q, double* qd, double* qdd_prev, double* arm_metrics,
                            const double* tray_pos, double* stack_metrics,
                            double* log_X, double* log_U, double* log_quat, double* log_loss,
                            int32_t* log_status, int32_t* log_iters, double* log_tilt, double* log_tray,
                            double* q_log, double* qd_log, double* tau_log, double* ee_log, double* loss_log,
                            int32_t* status_log, void* stream) {
    DART_ENTER(h, -1);
    return stack_closed_loop_host(h, false, plant, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride,
                                  rollout_buf(target, prm, nullptr, nullptr, x, tilt, metrics, grasp, models, plant_models,
                                              arm_prm, q, qd, qdd_prev, arm_metrics, nullptr, tray_pos, stack_metrics,
                                              STACK_PMPC_LOGS, nullptr, log_tilt, log_tray, STACK_ARM_LOGS), stream);
}

int dart_pmpc_stack_lm_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_stack_config* scfg,
                               const dart_arm_dyn_config* dcfg, const dart_arm_config* qcfg,
                               int E, int n, int k0, int steps, int log_rows, int arm_prm_stride,
                               const double* target, const double* prm, const double* plant_pvec,
                               const double* pz_vz, double* x, double* tilt, double* metrics,
                               const double* grasp, const double* models, const double* plant_models,
                               const double* arm_prm, double* q, double* qd, double* qdd_prev, double* arm_metrics,
                               const double* tray_pos, double* stack_metrics,
                               double* log_X, double* log_U, double* log_quat, double* log_loss,
                               int32_t* log_status, int32_t* log_iters, double* log_rot,
                               double* log_tilt, double* log_tray,
                               double* q_log, double* qd_log, double* tau_log, double* ee_log, double* loss_log,
                               int32_t* status_log, void* stream) {
    DART_ENTER(h, -1);
    return stack_closed_loop_host(h, true, plant, scfg, dcfg, qcfg, E, n, k0, steps, log_rows, arm_prm_stride,
                                  rollout_buf(target, prm, plant_pvec, pz_vz, x, tilt, metrics, grasp, models, plant_models,
                                              arm_prm, q, qd, qdd_prev, arm_metrics, nullptr, tray_pos, stack_metrics,
                                              STACK_PMPC_LOGS, log_rot, log_tilt, log_tray, STACK_ARM_LOGS), stream);
}
