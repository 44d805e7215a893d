// dart_mpc_arm.hip -- the arm-dynamics entries of include/dart_mpc.h (host side): state -> snapshot (arm_dyn.hip),
// dynamics + the unchanged QP launch, the dual-arm coordinator and the device-resident loop of the arm layer.
#include "abi_internal.h"
#include "arm_dyn.h"

void dart_arm_dyn_config_default(dart_arm_dyn_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof *c);
    c->jacdot_point = DART_ARM_JACDOT_REFERENCE;
}

int dart_arm_model_len(int n) { return (n >= 1 && n <= DART_ARM_NMAX) ? dartmpc::arm_model_len(n) : DART_MPC_EINVAL; }
int dart_arm_state_len(int n) { return (n >= 1 && n <= DART_ARM_NMAX) ? dartmpc::arm_state_len(n) : DART_MPC_EINVAL; }
int dart_dual_arm_work_len(int E, int n) {
    if (E < 1 || E > (1 << 20) || n < 1 || n > DART_ARM_NMAX) return DART_MPC_EINVAL;
    return 2 * E * (dartmpc::arm_snap_len(n) + 2 * n + 3);
}

using dartmpc::ArmDynArgs;
using dartmpc::ArmPlantArgs;

bool arm_dyn_ok(const dart_arm_dyn_config* c, int B, int n) {
    return c && B >= 1 && n >= 1 && n <= DART_ARM_NMAX &&
           (c->jacdot_point == DART_ARM_JACDOT_REFERENCE || c->jacdot_point == DART_ARM_JACDOT_BODY);
}
// the QP configuration, as dart_arm_solve_batch checks it
bool arm_qp_ok(const dart_arm_config* c, int n, int prm_stride) {
    return c && (prm_stride == 0 || prm_stride == dartmpc::arm_prm_len(n)) && c->tol > 0.0 &&
           c->acceptable_tol >= c->tol && c->max_iter >= 1 && c->max_iter <= 100000;
}

namespace {

bool dyn_ok(const dart_arm_dyn_config* c, int B, int n) { return arm_dyn_ok(c, B, n); }
bool qp_ok(const dart_arm_config* c, int n, int prm_stride) { return arm_qp_ok(c, n, prm_stride); }
int hip_rc(hipError_t e) { return e == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP; }
hipError_t as_hip(int rc) { return rc == DART_MPC_OK ? hipSuccess : hipErrorUnknown; }

// dynamics of state rows [B][3 n + 7]
ArmDynArgs state_args(const dart_arm_dyn_config* c, int B, int n, const double* model, int model_stride,
                      const double* state, double* snap, double* ee_quat) {
    ArmDynArgs a{};
    const int STL = dartmpc::arm_state_len(n);
    a.B = B; a.n = n; a.jacdot_point = c->jacdot_point;
    a.model = model; a.model_stride = model_stride; a.model_mod = 0;
    a.q = state; a.qd = state + n; a.qp = state + 2 * n; a.q_stride = STL;
    a.mocap = state + 3 * n; a.mocap_stride = STL;
    a.snap = snap; a.ee_quat = ee_quat;
    return a;
}
// dynamics of the dual-arm coordinator: instance 2 e + a, models [2][ML], targets from the tray pose
ArmDynArgs dual_args(const dart_arm_dyn_config* c, int E, int n, const double* tray, const double* grasp,
                     const double* q, const double* qd, const double* qp, const double* models, double* snap,
                     double* mocap) {
    ArmDynArgs a{};
    a.B = 2 * E; a.n = n; a.jacdot_point = c->jacdot_point;
    a.model = models; a.model_stride = dartmpc::arm_model_len(n); a.model_mod = 2;
    a.q = q; a.qd = qd; a.qp = qp; a.q_stride = n;
    a.tray = tray; a.grasp = grasp;
    a.snap = snap; a.mocap_out = mocap;
    return a;
}

}  // namespace

int dart_arm_dynamics_batch_dev(const dart_arm_dyn_config* dcfg, int B, int n, const double* model, int model_stride,
                                const double* state, double* snap, double* ee_quat, void* stream) {
    if (!dyn_ok(dcfg, B, n) || !model || !state || !snap) return DART_MPC_EINVAL;
    if (model_stride != 0 && model_stride != dartmpc::arm_model_len(n)) return DART_MPC_EINVAL;
    const ArmDynArgs a = state_args(dcfg, B, n, model, model_stride, state, snap, ee_quat);
    return hip_rc(dartmpc_launch_arm_dyn(&a, (hipStream_t)stream));
}

int dart_arm_dynamics_batch(const dart_arm_dyn_config* dcfg, int B, int n, const double* model, int model_stride,
                            const double* state, double* snap, double* ee_quat) {
    if (!dyn_ok(dcfg, B, n) || !model || !state || !snap) return DART_MPC_EINVAL;
    if (model_stride != 0 && model_stride != dartmpc::arm_model_len(n)) return DART_MPC_EINVAL;
    const size_t SL = dartmpc::arm_snap_len(n), ML = dartmpc::arm_model_len(n), STL = dartmpc::arm_state_len(n);
    const size_t nm = model_stride ? ML * B : ML;
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(sizeof(double) * (nm + STL * B) + 2 * 256, sizeof(double) * (SL + 4) * B + 2 * 256) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    const double* d_model = S.in(model, nm);
    const double* d_state = S.in(state, STL * B);
    double* d_snap = S.out<double>(SL * B);
    double* d_eq = ee_quat ? S.out<double>((size_t)4 * B) : nullptr;
    if (!D->run([&](hipStream_t s) {
            return as_hip(dart_arm_dynamics_batch_dev(dcfg, B, n, d_model, model_stride, d_state, d_snap, d_eq, s));
        }))
        return DART_MPC_EHIP;
    S.take(snap, d_snap, SL * B);
    S.take(ee_quat, d_eq, (size_t)4 * B);
    return DART_MPC_OK;
}

int dart_arm_control_batch_dev(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int B, int n,
                               const double* model, int model_stride, const double* state, const double* prm,
                               int prm_stride, double* snap, double* qdd, double* tau, double* loss, int32_t* status,
                               int32_t* iters, void* stream) {
    if (!dyn_ok(dcfg, B, n) || !qp_ok(cfg, n, prm_stride)) return DART_MPC_EINVAL;
    if (any_null({model, state, prm, snap, qdd, tau, loss, status, iters})) return DART_MPC_EINVAL;
    if (int rc = dart_arm_dynamics_batch_dev(dcfg, B, n, model, model_stride, state, snap, nullptr, stream)) return rc;
    return dart_arm_solve_batch_dev(cfg, B, n, snap, prm, prm_stride, qdd, tau, loss, status, iters, stream);
}

int dart_arm_control_batch(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int B, int n,
                           const double* model, int model_stride, const double* state, const double* prm,
                           int prm_stride, double* snap, double* qdd, double* tau, double* loss, int32_t* status,
                           int32_t* iters) {
    if (!dyn_ok(dcfg, B, n) || !qp_ok(cfg, n, prm_stride)) return DART_MPC_EINVAL;
    if (any_null({model, state, prm, qdd, tau, loss, status, iters})) return DART_MPC_EINVAL;
    if (model_stride != 0 && model_stride != dartmpc::arm_model_len(n)) return DART_MPC_EINVAL;
    const size_t SL = dartmpc::arm_snap_len(n), ML = dartmpc::arm_model_len(n), STL = dartmpc::arm_state_len(n);
    const size_t PL = dartmpc::arm_prm_len(n), nm = model_stride ? ML * B : ML, np = prm_stride ? PL * B : PL;
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(sizeof(double) * (nm + STL * B + np + SL * B) + 4 * 256,
                  sizeof(double) * (2 * (size_t)n * B + B) + sizeof(int32_t) * 2 * B + 5 * 256) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    const double* d_model = S.in(model, nm);
    const double* d_state = S.in(state, STL * B);
    const double* d_prm = S.in(prm, np);
    double* d_qdd = S.out<double>((size_t)n * B);
    double* d_tau = S.out<double>((size_t)n * B);
    double* d_loss = S.out<double>(B);
    int32_t* d_status = S.out<int32_t>(B);
    int32_t* d_iters = S.out<int32_t>(B);
    // the snapshots stay in device memory between the two kernels; they come back only when asked for
    double* d_snap = snap ? S.inout(snap, SL * B) : const_cast<double*>(S.in_with<double>(SL * B, [](double*) {}));
    if (!D->run([&](hipStream_t s) {
            return as_hip(dart_arm_control_batch_dev(dcfg, cfg, B, n, d_model, model_stride, d_state, d_prm, prm_stride,
                                                     d_snap, d_qdd, d_tau, d_loss, d_status, d_iters, s));
        }))
        return DART_MPC_EHIP;
    S.take(qdd, d_qdd, (size_t)n * B); S.take(tau, d_tau, (size_t)n * B); S.take(loss, d_loss, B);
    S.take(status, d_status, B); S.take(iters, d_iters, B);
    return DART_MPC_OK;
}

int dart_dual_arm_control_dev(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int E, int n,
                              const double* tray_pose, const double* grasp, const double* q, const double* qd,
                              const double* qdd_prev, const double* models, const double* prm, int prm_stride,
                              double* snap, double* mocap, double* qdd, double* tau, double* loss, int32_t* status,
                              int32_t* iters, void* stream) {
    if (E > (1 << 20) || !dyn_ok(dcfg, E, n) || !qp_ok(cfg, n, prm_stride)) return DART_MPC_EINVAL;
    if (any_null({tray_pose, grasp, q, qd, qdd_prev, models, prm, snap, qdd, tau, loss, status, iters}))
        return DART_MPC_EINVAL;
    const ArmDynArgs a = dual_args(dcfg, E, n, tray_pose, grasp, q, qd, qdd_prev, models, snap, mocap);
    if (dartmpc_launch_arm_dyn(&a, (hipStream_t)stream) != hipSuccess) return DART_MPC_EHIP;
    return dart_arm_solve_batch_dev(cfg, 2 * E, n, snap, prm, prm_stride, qdd, tau, loss, status, iters, stream);
}

int dart_dual_arm_control(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int E, int n,
                          const double* tray_pose, const double* grasp, const double* q, const double* qd,
                          const double* qdd_prev, const double* models, const double* prm, int prm_stride,
                          double* snap, double* mocap, double* qdd, double* tau, double* loss, int32_t* status,
                          int32_t* iters) {
    if (E > (1 << 20) || !dyn_ok(dcfg, E, n) || !qp_ok(cfg, n, prm_stride)) return DART_MPC_EINVAL;
    if (any_null({tray_pose, grasp, q, qd, qdd_prev, models, prm, qdd, tau, loss, status, iters})) return DART_MPC_EINVAL;
    const size_t B = 2 * (size_t)E, SL = dartmpc::arm_snap_len(n), ML = dartmpc::arm_model_len(n);
    const size_t PL = dartmpc::arm_prm_len(n), np = prm_stride ? PL * B : PL;
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(sizeof(double) * (7 * (size_t)E + 14 + 3 * n * B + 2 * ML + np + SL * B) + 9 * 256,
                  sizeof(double) * (2 * n * B + B + 7 * B) + sizeof(int32_t) * 2 * B + 6 * 256) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    const double* d_tray = S.in(tray_pose, 7 * (size_t)E);
    const double* d_grasp = S.in(grasp, 14);
    const double* d_q = S.in(q, n * B);
    const double* d_qd = S.in(qd, n * B);
    const double* d_qp = S.in(qdd_prev, n * B);
    const double* d_models = S.in(models, 2 * ML);
    const double* d_prm = S.in(prm, np);
    double* d_qdd = S.out<double>(n * B);
    double* d_tau = S.out<double>(n * B);
    double* d_loss = S.out<double>(B);
    double* d_mocap = mocap ? S.out<double>(7 * B) : nullptr;
    int32_t* d_status = S.out<int32_t>(B);
    int32_t* d_iters = S.out<int32_t>(B);
    double* d_snap = snap ? S.inout(snap, SL * B) : const_cast<double*>(S.in_with<double>(SL * B, [](double*) {}));
    if (!D->run([&](hipStream_t s) {
            return as_hip(dart_dual_arm_control_dev(dcfg, cfg, E, n, d_tray, d_grasp, d_q, d_qd, d_qp, d_models, d_prm,
                                                    prm_stride, d_snap, d_mocap, d_qdd, d_tau, d_loss, d_status,
                                                    d_iters, s));
        }))
        return DART_MPC_EHIP;
    S.take(qdd, d_qdd, n * B); S.take(tau, d_tau, n * B); S.take(loss, d_loss, B); S.take(mocap, d_mocap, 7 * B);
    S.take(status, d_status, B); S.take(iters, d_iters, B);
    return DART_MPC_OK;
}

namespace {

bool rollout_ok(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int E, int n, int steps, int tray_rows,
                int prm_stride, std::initializer_list<const void*> need, std::initializer_list<const void*> logs) {
    if (E > (1 << 20) || !dyn_ok(dcfg, E, n) || !qp_ok(cfg, n, prm_stride)) return false;
    if (steps < 0 || steps > (1 << 24) || (tray_rows != 1 && tray_rows != steps)) return false;
    if (any_null(need)) return false;
    int set = 0;
    for (const void* p : logs) set += p != nullptr;
    return set == 0 || set == (int)logs.size();
}

}  // namespace

int dual_arm_step(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int E, int n, const double* tray,
                  const double* grasp, const double* models, const double* plant_models, const double* prm,
                  int prm_stride, double* q, double* qd, double* qdd_prev, double* metrics, double* work,
                  double* ee_quat, size_t log_row, double* q_log, double* qd_log, double* tau_log, double* ee_log,
                  double* loss_log, int32_t* status_log, hipStream_t s) {
    const size_t B = 2 * (size_t)E, SL = dartmpc::arm_snap_len(n);
    double* snap = work;
    double* qdd = snap + SL * B;
    double* tau = qdd + n * B;
    double* loss = tau + n * B;
    int32_t* status = reinterpret_cast<int32_t*>(loss + B);
    int32_t* iters = reinterpret_cast<int32_t*>(loss + 2 * B);
    ArmDynArgs a = dual_args(dcfg, E, n, tray, grasp, q, qd, qdd_prev, models, snap, nullptr);
    a.ee_quat = ee_quat;
    if (dartmpc_launch_arm_dyn(&a, s) != hipSuccess) return DART_MPC_EHIP;
    if (int rc = dart_arm_solve_batch_dev(cfg, (int)B, n, snap, prm, prm_stride, qdd, tau, loss, status, iters, s)) return rc;
    ArmPlantArgs p{};
    p.B = (int)B; p.n = n;
    p.model = plant_models; p.model_stride = dartmpc::arm_model_len(n); p.model_mod = 2;
    p.prm = prm; p.prm_stride = prm_stride; p.snap = snap;
    p.qdd = qdd; p.tau = tau; p.loss = loss; p.status = status; p.iters = iters;
    p.q = q; p.qd = qd; p.qp = qdd_prev; p.metrics = metrics;
    if (q_log) {
        const size_t r = log_row * B;
        p.q_log = q_log + r * n; p.qd_log = qd_log + r * n; p.tau_log = tau_log + r * n;
        p.ee_log = ee_log + r * 3; p.loss_log = loss_log + r; p.status_log = status_log + r;
    }
    return dartmpc_launch_arm_plant(&p, s) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_dual_arm_rollout_dev(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int E, int n, int steps,
                              int tray_rows, const double* tray_poses, const double* grasp, const double* models,
                              const double* plant_models, const double* prm, int prm_stride, double* q, double* qd,
                              double* qdd_prev, double* metrics, double* work, double* q_log, double* qd_log,
                              double* tau_log, double* ee_log, double* loss_log, int32_t* status_log, void* stream) {
    if (!rollout_ok(dcfg, cfg, E, n, steps, tray_rows, prm_stride,
                    {tray_poses, grasp, models, plant_models, prm, q, qd, qdd_prev, metrics, work},
                    {q_log, qd_log, tau_log, ee_log, loss_log, status_log}))
        return DART_MPC_EINVAL;
    for (int k = 0; k < steps; ++k) {
        const double* tray = tray_poses + (tray_rows == 1 ? 0 : (size_t)k * 7 * E);
        if (int rc = dual_arm_step(dcfg, cfg, E, n, tray, grasp, models, plant_models, prm, prm_stride, q, qd, qdd_prev,
                                   metrics, work, nullptr, (size_t)k, q_log, qd_log, tau_log, ee_log, loss_log, status_log,
                                   (hipStream_t)stream))
            return rc;
    }
    return DART_MPC_OK;
}

int dart_dual_arm_rollout(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int E, int n, int steps,
                          int tray_rows, const double* tray_poses, const double* grasp, const double* models,
                          const double* plant_models, const double* prm, int prm_stride, double* q, double* qd,
                          double* qdd_prev, double* metrics, double* q_log, double* qd_log, double* tau_log,
                          double* ee_log, double* loss_log, int32_t* status_log) {
    if (!rollout_ok(dcfg, cfg, E, n, steps, tray_rows, prm_stride,
                    {tray_poses, grasp, models, plant_models, prm, q, qd, qdd_prev, metrics},
                    {q_log, qd_log, tau_log, ee_log, loss_log, status_log}))
        return DART_MPC_EINVAL;
    const size_t B = 2 * (size_t)E, ML = dartmpc::arm_model_len(n), PL = dartmpc::arm_prm_len(n);
    const size_t np = prm_stride ? PL * B : PL, nt = (size_t)tray_rows * 7 * E, K = (size_t)steps;
    const size_t nwork = (size_t)dart_dual_arm_work_len(E, n);
    const bool logs = q_log != nullptr;
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(sizeof(double) * (nt + 14 + 4 * ML + np + nwork + 3 * n * B + dartmpc::ARM_NMETRIC * B) + 12 * 256,
                  (logs ? sizeof(double) * K * B * (3 * n + 4) + sizeof(int32_t) * K * B : 0) + 7 * 256) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    const double* d_tray = S.in(tray_poses, nt);
    const double* d_grasp = S.in(grasp, 14);
    const double* d_models = S.in(models, 2 * ML);
    const double* d_plant = S.in(plant_models, 2 * ML);
    const double* d_prm = S.in(prm, np);
    double* d_work = const_cast<double*>(S.in_with<double>(nwork, [](double*) {}));
    double *l_q = nullptr, *l_qd = nullptr, *l_tau = nullptr, *l_ee = nullptr, *l_loss = nullptr;
    int32_t* l_status = nullptr;
    if (logs) {
        l_q = S.out<double>(K * B * n); l_qd = S.out<double>(K * B * n); l_tau = S.out<double>(K * B * n);
        l_ee = S.out<double>(K * B * 3); l_loss = S.out<double>(K * B); l_status = S.out<int32_t>(K * B);
    }
    double* d_q = S.inout(q, n * B);
    double* d_qd = S.inout(qd, n * B);
    double* d_qp = S.inout(qdd_prev, n * B);
    double* d_met = S.inout(metrics, dartmpc::ARM_NMETRIC * B);
    if (!D->run([&](hipStream_t s) {
            return as_hip(dart_dual_arm_rollout_dev(dcfg, cfg, E, n, steps, tray_rows, d_tray, d_grasp, d_models, d_plant,
                                                    d_prm, prm_stride, d_q, d_qd, d_qp, d_met, d_work, l_q, l_qd, l_tau,
                                                    l_ee, l_loss, l_status, s));
        }))
        return DART_MPC_EHIP;
    S.take(q_log, l_q, K * B * n); S.take(qd_log, l_qd, K * B * n); S.take(tau_log, l_tau, K * B * n);
    S.take(ee_log, l_ee, K * B * 3); S.take(loss_log, l_loss, K * B); S.take(status_log, l_status, K * B);
    return DART_MPC_OK;
}
