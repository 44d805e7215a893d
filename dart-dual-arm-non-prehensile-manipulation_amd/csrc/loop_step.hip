// loop_step.hip -- the closed-loop glue between two solves, on the device.  One kernel per controller.
//
// rmpc_loop_kernel<LM>: post(k) = the log rows, the episode end and the plant step of harness.run_rmpc; pre(k+1) =
// the RLS features / targets, the reference governor and the staged reference of the next solve
// (RMPC/dev_dual/rob_ctrl.py:335-351).  pmpc_loop_kernel<LM>: the same for harness.run_pmpc
// (PMPC/main_parallel_enhanced.py:333-348: log, tilt -> quaternion, plant step, next state).  Both are compiled for
// two plants: LM = false steps harness.TrayPlant (x [6]), LM = true harness.LmpcPlant (x [8], harness.run_pmpc /
// run_rmpc with plant_pvec) and also keeps the streaming metrics and the rotation log of loop_step.h; what a plant
// does not have is under `if constexpr (LM)` and is not in the other instantiation.  lmpc_loop_kernel: the same glue
// for harness.run_lmpc (LMPC/src/run.py:256-286: log, plant step of the LMPC model, next state); its lane mapping is
// described at the kernel.  lmpc_eval_loop_kernel: that step with the streaming metrics and optional logs, for the
// evaluation of P policies in one call (dart_lmpc_eval*); lmpc_eval_scores_kernel reduces its metrics per learner.
//
// RMPC / PMPC: one wave64 per instance, kLoopWaves instances per block; lane i owns horizon node i (the staged
// reference), the per-instance scalars are computed by every lane and stored by one.  All three: plain fp64 in the
// operation order of the numpy code (no contraction into fma), no LDS.  A lane only ever reads state that this
// launch does not write, or keeps it in registers across the post and pre halves: nothing is read back from memory
// in a launch.
#include "loop_step.h"
#include "loop_plant.h"

#pragma clang fp contract(off)

namespace dartmpc {

constexpr int kLoopWave = 64;
constexpr int kLoopWaves = 4;

// ---------------------------------------------------------------------------------------------------------------
// LMPC (harness.run_lmpc): post(k) = the log row, u_prev, the tilt lag and one RK4 step of the LMPC model
// (safe_dynamics, rlmpc2.py:260-429) with the plant's own parameter vector; pre(k+1) = the solve's state.
//
// kLmGroup = 8 lanes per instance, 8 instances per wave64 (there is no per-node reference to own); the lane mapping
// of a stage is lm_plant_dyn's (loop_plant.h).  The serial chain of a step is 4 x (one Stribeck + one sine) in place
// of 4 x (six + two).
constexpr int kLmLoopThreads = 256;
__global__ __launch_bounds__(kLmLoopThreads) void lmpc_loop_kernel(LmpcLoopArgs a) {
    const int r = threadIdx.x & (kLmGroup - 1);
    const int b = (blockIdx.x * kLmLoopThreads + threadIdx.x) / kLmGroup;
    if (b >= a.B) return;                    // uniform over the group (the shuffles stay inside it)
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = a.x[8 * b + i];

    if (a.do_post) {
        double tilt[2] = {a.tilt[2 * b], a.tilt[2 * b + 1]};
        const double u[2] = {a.u0[2 * b], a.u0[2 * b + 1]};
        const size_t row = (size_t)a.k * a.B + b;
        for (int i = r; i < 34; i += kLmGroup) a.log_pvec[34 * row + i] = a.model_params[34 * b + i];
        if (r == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) a.log_X[8 * row + i] = x[i];
            a.log_U[2 * row] = u[0]; a.log_U[2 * row + 1] = u[1];
            a.log_loss[row] = a.f[b];
            a.log_status[row] = a.status[b];
            a.log_iters[row] = a.iters[b];
            a.u_prev[2 * b] = u[0]; a.u_prev[2 * b + 1] = u[1];
        }
        // harness.LmpcPlant.step
        tilt[0] += a.a_lag * (u[0] - tilt[0]);
        tilt[1] += a.a_lag * (u[1] - tilt[1]);
        const double* pv = a.plant_pvec + 34 * b;
        LmPlantPrm P;
        P.m_x = lm_squash(pv[0]); P.m_y = lm_squash(pv[1]); P.c_x = lm_squash(pv[2]); P.c_y = lm_squash(pv[3]);
        P.k_x = lm_squash(pv[4]); P.k_y = lm_squash(pv[5]); P.I_x = lm_squash(pv[16]); P.I_y = lm_squash(pv[17]);
        P.r_x = lm_squash(pv[18]); P.r_y = lm_squash(pv[19]); P.c_rot_x = lm_squash(pv[20]); P.c_rot_y = lm_squash(pv[21]);
        P.h_com_x = lm_squash(pv[32]); P.h_com_y = lm_squash(pv[33]);
        {       // Stribeck rows [F_s, F_c, B, v_s, eps] (:301-334): x 6.., y 11.., rot x 22.., rot y 27..
            const int t = r < 6 ? r : r - 6;
            const int o = t == 0 || t == 2 ? 6 : t == 1 || t == 3 ? 11 : t == 4 ? 22 : 27;
            P.Fs = pv[o]; P.Fc = pv[o + 1]; P.Bv = pv[o + 2]; P.vs = lm_squash(pv[o + 3]); P.eps = lm_squash(pv[o + 4]);
        }
        const double st = sin((r & 1) ? tilt[1] : tilt[0]);
        const double sa = __shfl(st, 0, kLmGroup), sb = __shfl(st, 1, kLmGroup);
        const double h = a.Ts;
        double k1[8], k2[8], k3[8], k4[8], y[8];
        lm_plant_dyn(P, r, x, sa, sb, k1);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = x[i] + 0.5 * h * k1[i];
        lm_plant_dyn(P, r, y, sa, sb, k2);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = x[i] + 0.5 * h * k2[i];
        lm_plant_dyn(P, r, y, sa, sb, k3);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = x[i] + h * k3[i];
        lm_plant_dyn(P, r, y, sa, sb, k4);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = x[i] + h * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) / 6;
        if (r == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) a.x[8 * b + i] = x[i];
            a.tilt[2 * b] = tilt[0]; a.tilt[2 * b + 1] = tilt[1];
            const double dx = x[0] - a.target[8 * b], dy = x[2] - a.target[8 * b + 2];
            a.log_pos_error[row] = sqrt(dx * dx + dy * dy);
        }
    }
    if (a.do_pre && r == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) a.state[8 * b + i] = x[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LMPC evaluation (dart_lmpc_eval*): lmpc_loop_kernel's step with the streaming metrics and with logs that may be
// absent.  Same lane mapping (kLmGroup lanes per instance, lane r evaluates Stribeck term r), same post(k) / pre(k+1)
// split, the same expressions in the same order, so x, tilt, u_prev, state and (a.logs) the log rows are bit for bit
// lmpc_loop_kernel's.  The step is that kernel's text again, not shared with it, so that kernel keeps its
// instructions.  Lane 0 of the group feeds loop_metrics_step what harness.rollout_metrics takes from the logs: e of
// the state the solve saw (x as loaded, before the plant step), u0, status, iters, th_x = x[4], th_y = x[6].
__global__ __launch_bounds__(kLmLoopThreads) void lmpc_eval_loop_kernel(LmpcEvalLoopArgs ea) {
    const LmpcLoopArgs& a = ea.l;
    const int r = threadIdx.x & (kLmGroup - 1);
    const int b = (blockIdx.x * kLmLoopThreads + threadIdx.x) / kLmGroup;
    if (b >= a.B) return;                    // uniform over the group (the shuffles stay inside it)
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = a.x[8 * b + i];

    if (a.do_post) {
        double tilt[2] = {a.tilt[2 * b], a.tilt[2 * b + 1]};
        const double u[2] = {a.u0[2 * b], a.u0[2 * b + 1]};
        const size_t row = (size_t)a.k * a.B + b;
        if (ea.logs)
            for (int i = r; i < 34; i += kLmGroup) a.log_pvec[34 * row + i] = a.model_params[34 * b + i];
        if (r == 0) {
            const int status = a.status[b], iters = a.iters[b];
            if (ea.logs) {
#pragma unroll
                for (int i = 0; i < 8; ++i) a.log_X[8 * row + i] = x[i];
                a.log_U[2 * row] = u[0]; a.log_U[2 * row + 1] = u[1];
                a.log_loss[row] = a.f[b];
                a.log_status[row] = status;
                a.log_iters[row] = iters;
            }
            a.u_prev[2 * b] = u[0]; a.u_prev[2 * b + 1] = u[1];
            const double ex = x[0] - a.target[8 * b], ey = x[2] - a.target[8 * b + 2];
            loop_metrics_step(ea.metrics + 8 * b, a.k, a.Ts, sqrt(ex * ex + ey * ey), u, status, iters, x[4], x[6]);
        }
        // harness.LmpcPlant.step
        tilt[0] += a.a_lag * (u[0] - tilt[0]);
        tilt[1] += a.a_lag * (u[1] - tilt[1]);
        const double* pv = a.plant_pvec + 34 * b;
        LmPlantPrm P;
        P.m_x = lm_squash(pv[0]); P.m_y = lm_squash(pv[1]); P.c_x = lm_squash(pv[2]); P.c_y = lm_squash(pv[3]);
        P.k_x = lm_squash(pv[4]); P.k_y = lm_squash(pv[5]); P.I_x = lm_squash(pv[16]); P.I_y = lm_squash(pv[17]);
        P.r_x = lm_squash(pv[18]); P.r_y = lm_squash(pv[19]); P.c_rot_x = lm_squash(pv[20]); P.c_rot_y = lm_squash(pv[21]);
        P.h_com_x = lm_squash(pv[32]); P.h_com_y = lm_squash(pv[33]);
        {       // Stribeck rows [F_s, F_c, B, v_s, eps] (:301-334): x 6.., y 11.., rot x 22.., rot y 27..
            const int t = r < 6 ? r : r - 6;
            const int o = t == 0 || t == 2 ? 6 : t == 1 || t == 3 ? 11 : t == 4 ? 22 : 27;
            P.Fs = pv[o]; P.Fc = pv[o + 1]; P.Bv = pv[o + 2]; P.vs = lm_squash(pv[o + 3]); P.eps = lm_squash(pv[o + 4]);
        }
        const double st = sin((r & 1) ? tilt[1] : tilt[0]);
        const double sa = __shfl(st, 0, kLmGroup), sb = __shfl(st, 1, kLmGroup);
        const double h = a.Ts;
        double k1[8], k2[8], k3[8], k4[8], y[8];
        lm_plant_dyn(P, r, x, sa, sb, k1);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = x[i] + 0.5 * h * k1[i];
        lm_plant_dyn(P, r, y, sa, sb, k2);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = x[i] + 0.5 * h * k2[i];
        lm_plant_dyn(P, r, y, sa, sb, k3);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = x[i] + h * k3[i];
        lm_plant_dyn(P, r, y, sa, sb, k4);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = x[i] + h * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) / 6;
        if (r == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) a.x[8 * b + i] = x[i];
            a.tilt[2 * b] = tilt[0]; a.tilt[2 * b + 1] = tilt[1];
            if (ea.logs) {
                const double dx = x[0] - a.target[8 * b], dy = x[2] - a.target[8 * b + 2];
                a.log_pos_error[row] = sqrt(dx * dx + dy * dy);
            }
        }
    }
    if (a.do_pre && r == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) a.state[8 * b + i] = x[i];
    }
}

// metrics [P][B][8] -> scores [P][8] (loop_step.h): one work-group per learner, lane s owns score slot s and walks
// its learner's instances b = 0 .. B-1 in that order, so every sum is the sequential fp64 sum that
// harness.population_scores restates (B >= 1)
constexpr int kScoreThreads = 64;
__global__ __launch_bounds__(kScoreThreads) void lmpc_eval_scores_kernel(int B, const double* metrics, double* scores) {
    const int l = blockIdx.x, s = threadIdx.x;
    if (s >= 8) return;
    const double* m = metrics + 8 * (size_t)l * B;
    // the metrics slot a score reads: 0 e, 1 and 2 the convergence step, 3 effort, 4 max e, 5 bad steps, 6 iters (over
    // the steps, slot 7), 7 rotation
    const int c = s == 0 ? 0 : s <= 2 ? 1 : s - 1;
    double acc = 0.0, cnt = 0.0;
    for (int b = 0; b < B; ++b) {
        const double v = m[8 * (size_t)b + c];
        if (s == 1) { if (v >= 0.0) acc += 1.0; }
        else if (s == 2) { if (v >= 0.0) { acc += v; cnt += 1.0; } }
        else if (s == 4 || s == 7) { if (b == 0 || v > acc) acc = v; }
        else {
            acc += v;
            if (s == 6) cnt += m[8 * (size_t)b + 7];
        }
    }
    double out = acc;
    if (s == 0 || s == 1 || s == 3) out = acc / (double)B;
    else if (s == 2) out = cnt > 0.0 ? acc / cnt : -1.0;
    else if (s == 6) out = cnt != 0.0 ? acc / cnt : 0.0;
    scores[8 * (size_t)l + s] = out;
}

// The plant steps (tray_plant_step; lm_cross_plant_step: the LMPC plant under the PMPC / RMPC kernels, every aligned
// group of kLmGroup lanes running the step the way lmpc_loop_kernel's group does) and loop_metrics_step are
// loop_plant.h's, shared with stack_step.hip.
//
// One plant step of instance b with the command u, and the new state stored by lane 0.  Tray: mu is the instance's
// viscous friction, and x[0..3] are stored (pz, vz do not move).  LMPC plant: every aligned group of kLmGroup lanes
// runs the step the way lmpc_loop_kernel's group does, so all 64 lanes hold the same next state; x[0..7] are stored.
template <bool LM, class Args>
__device__ __forceinline__ void loop_plant_step(const Args& a, int b, int lane, const double* mu, const double* u,
                                                double* x, double* tilt) {
    if constexpr (LM) lm_cross_plant_step(a.plant_pvec + 34 * b, lane & (kLmGroup - 1), a.a_lag, a.Ts, u, x, tilt);
    else tray_plant_step(a.plant, *mu, u, x, tilt);
    if (lane == 0) {
        constexpr int NX = LM ? 8 : 6;
#pragma unroll
        for (int i = 0; i < (LM ? 8 : 4); ++i) a.x[NX * b + i] = x[i];
        a.tilt[2 * b] = tilt[0]; a.tilt[2 * b + 1] = tilt[1];
    }
}

template <bool LM>
__global__ __launch_bounds__(kLoopWave* kLoopWaves) void rmpc_loop_kernel(RmpcLoopArgs a) {
    constexpr int NX = LM ? 8 : 6;
    const int lane = threadIdx.x & (kLoopWave - 1);
    const int b = blockIdx.x * kLoopWaves + (threadIdx.x >> 6);
    if (b >= a.B) return;                    // wave-uniform
    const size_t B = (size_t)a.B;
    const int logs = LM ? a.logs : 1;        // (the tray plant's loop always logs)
    const double* tg = a.target + 4 * b;
    const double t0 = tg[0], t2 = tg[2];
    double x[NX], tilt[2], prev[4], rv[4];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = a.x[NX * b + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) rv[i] = a.r_v[4 * b + i];

    if (a.do_post) {
        tilt[0] = a.tilt[2 * b]; tilt[1] = a.tilt[2 * b + 1];
        const double u[2] = {a.u0[2 * b], a.u0[2 * b + 1]};
        const size_t row = (size_t)a.k * B + b;
        const double dx = x[0] - t0, dy = x[2] - t2;
        const double en = sqrt(dx * dx + dy * dy);
        if (logs && lane < 14) a.log_theta[14 * row + lane] = a.theta[14 * b + lane];
        if (lane == 0) {
            const int nl = a.nlog[b];
            if (!a.done[b]) {
                if (logs && nl >= 0 && nl < a.log_rows) {
                    const size_t er = (size_t)nl * B + b;
                    a.log_pos_err[2 * er] = t0 - x[0]; a.log_pos_err[2 * er + 1] = t2 - x[2];
                    a.log_pos_err_norm[er] = en;
                    a.log_u_cmd[2 * er] = u[0]; a.log_u_cmd[2 * er + 1] = u[1];
                    a.log_timestep[er] = a.k * a.Ts;
                }
                a.nlog[b] = nl + 1;
                if (en < a.pos_tol) a.done[b] = 1;
            }
            const int status = a.status[b], iters = a.iters[b];
            if (logs) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a.log_x[4 * row + i] = x[i];
                    a.log_r_v[4 * row + i] = rv[i];
                    if constexpr (LM) a.log_rot[4 * row + i] = x[4 + i];
                }
                a.log_status[row] = status;
                a.log_iters[row] = iters;
                a.log_f[row] = a.f[b];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) a.prev[4 * b + i] = x[i];
            a.u_prev[2 * b] = u[0]; a.u_prev[2 * b + 1] = u[1];
            if constexpr (LM) loop_metrics_step(a.metrics + 8 * b, a.k, a.Ts, en, u, status, iters, x[4], x[6]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) prev[i] = x[i];
        loop_plant_step<LM>(a, b, lane, LM ? nullptr : a.mu + b, u, x, tilt);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) prev[i] = a.prev[4 * b + i];
    }

    if (a.do_pre) {
        const double veps = a.prm[10 * b + 9];
        // reference governor (rob_ctrl.py:346-348) on the two position entries
        auto govern = [&](double r, double t) { return r + a.alpha_rg * fmin(fmax(t - r, -a.dr_max), a.dr_max); };
        rv[0] = govern(rv[0], t0);
        rv[2] = govern(rv[2], t2);
        if (lane <= a.N) {      // staged reference, node `lane` (np_mpc...:201-210)
            const double wgt = 1.0 - pow(1.0 - a.step_fraction, (double)(lane + 1));
            double* R = a.Rref + 4 * ((size_t)(a.N + 1) * b + lane);
            R[0] = rv[0] + wgt * (t0 - rv[0]); R[1] = 0.0;
            R[2] = rv[2] + wgt * (t2 - rv[2]); R[3] = 0.0;
        }
        if (lane == 0) {
            a.r_v[4 * b] = rv[0]; a.r_v[4 * b + 2] = rv[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a.x0[4 * b + i] = x[i]; a.phi[7 * b + i] = prev[i]; }
            a.phi[7 * b + 4] = tanh(prev[1] / veps);
            a.phi[7 * b + 5] = tanh(prev[3] / veps);
            a.phi[7 * b + 6] = 1.0;
            a.y[2 * b] = (x[1] - prev[1]) / a.Ts;
            a.y[2 * b + 1] = (x[3] - prev[3]) / a.Ts;
        }
    }
}

template <bool LM>
__global__ __launch_bounds__(kLoopWave* kLoopWaves) void pmpc_loop_kernel(PmpcLoopArgs a) {
    constexpr int NX = LM ? 8 : 6;
    const int lane = threadIdx.x & (kLoopWave - 1);
    const int b = blockIdx.x * kLoopWaves + (threadIdx.x >> 6);
    if (b >= a.B) return;                    // wave-uniform
    const int logs = LM ? a.logs : 1;        // (the tray plant's loop always logs)
    double x[NX], tilt[2];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = a.x[NX * b + i];
    // the solve's x0[4..5]: the tray's own x[4..5]; the LMPC plant has none, so the caller's pz_vz
    const double pz = LM ? a.pz_vz[2 * b] : x[4], vz = LM ? a.pz_vz[2 * b + 1] : x[5];

    if (a.do_post) {
        tilt[0] = a.tilt[2 * b]; tilt[1] = a.tilt[2 * b + 1];
        const double u[2] = {a.u0[2 * b], a.u0[2 * b + 1]};
        const size_t row = (size_t)a.k * a.B + b;
        // pmpc.tilt_to_quat: Euler xyz [u1, -u0, 0] -> (w, x, y, z)
        const double ax = u[1] / 2.0, ay = -u[0] / 2.0;
        const double cx = cos(ax), cy = cos(ay), cz = 1.0, sx = sin(ax), sy = sin(ay), sz = 0.0;
        if (lane == 0) {
            const int status = a.status[b], iters = a.iters[b];
            if (logs) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a.log_X[6 * row + i] = x[i];
                    if constexpr (LM) a.log_rot[4 * row + i] = x[4 + i];
                }
                a.log_X[6 * row + 4] = pz; a.log_X[6 * row + 5] = vz;
                a.log_U[2 * row] = u[0]; a.log_U[2 * row + 1] = u[1];
                a.log_quat[4 * row] = cx * cy * cz + sx * sy * sz;
                a.log_quat[4 * row + 1] = sx * cy * cz - cx * sy * sz;
                a.log_quat[4 * row + 2] = cx * sy * cz + sx * cy * sz;
                a.log_quat[4 * row + 3] = cx * cy * sz - sx * sy * cz;
                a.log_loss[row] = a.f[b];
                a.log_status[row] = status;
                a.log_iters[row] = iters;
            }
            if constexpr (LM) {
                const double dx = x[0] - a.target[6 * b], dy = x[2] - a.target[6 * b + 2];
                loop_metrics_step(a.metrics + 8 * b, a.k, a.Ts, sqrt(dx * dx + dy * dy), u, status, iters, x[4], x[6]);
            }
        }
        loop_plant_step<LM>(a, b, lane, LM ? nullptr : a.prm + 6 * b, u, x, tilt);
    }
    if (a.do_pre && lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a.x0[6 * b + i] = x[i];
        a.x0[6 * b + 4] = pz; a.x0[6 * b + 5] = vz;
    }
}

// the early return of an empty launch, the block count (`per_block` instances in a block of 256 threads), the launch
template <class Args>
hipError_t launch_loop(void (*kernel)(Args), const Args& a, int per_block, hipStream_t stream, bool valid = true) {
    static_assert(kLoopWave * kLoopWaves == kLmLoopThreads, "one block size for the three kernels");
    if (a.B <= 0 || (!a.do_post && !a.do_pre)) return hipSuccess;
    if (!valid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((a.B + per_block - 1) / per_block), dim3(kLmLoopThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dartmpc

using namespace dartmpc;

extern "C" hipError_t dartmpc_launch_rmpc_loop(const RmpcLoopArgs* args, int lm, hipStream_t stream) {
    // (lane i owns node i of the staged reference)
    return launch_loop(lm ? rmpc_loop_kernel<true> : rmpc_loop_kernel<false>, *args, kLoopWaves, stream,
                       args->N >= 1 && args->N <= 63);
}

extern "C" hipError_t dartmpc_launch_pmpc_loop(const PmpcLoopArgs* args, int lm, hipStream_t stream) {
    return launch_loop(lm ? pmpc_loop_kernel<true> : pmpc_loop_kernel<false>, *args, kLoopWaves, stream);
}

extern "C" hipError_t dartmpc_launch_lmpc_loop(const LmpcLoopArgs* args, hipStream_t stream) {
    return launch_loop(lmpc_loop_kernel, *args, kLmLoopThreads / kLmGroup, stream);
}

extern "C" hipError_t dartmpc_launch_lmpc_eval_loop(const LmpcEvalLoopArgs* args, hipStream_t stream) {
    const LmpcLoopArgs& a = args->l;
    if (a.B <= 0 || (!a.do_post && !a.do_pre)) return hipSuccess;
    const int per_block = kLmLoopThreads / kLmGroup;
    hipLaunchKernelGGL(lmpc_eval_loop_kernel, dim3((a.B + per_block - 1) / per_block), dim3(kLmLoopThreads), 0, stream,
                       *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_eval_scores(int P, int B, const double* metrics, double* scores,
                                                      hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    if (B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lmpc_eval_scores_kernel, dim3(P), dim3(kScoreThreads), 0, stream, B, metrics, scores);
    return hipGetLastError();
}
