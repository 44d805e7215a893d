// rmpc_stack_step.hip -- the RMPC closed loop through the dual-arm layer: the kernel between the arm layer's step and
// the next RMPC solve (rmpc_stack_step.h).  rmpc_stack_step_kernel<LM> measures the tray the two arms hold
// (stack_couple.h, shared with stack_step.hip) and is then rmpc_loop_kernel<LM>'s post / pre (loop_step.hip), in its
// expressions and order, with the tilt the plant sees chosen by `couple`; the command launch is stack_step.hip's.
//
// One wave64 per experiment, kStackWaves experiments per block; lane i owns node i of the staged reference, everything
// else is computed by every lane alike and stored by lane 0 (the LMPC plant's step wants its groups of kLmGroup lanes).
// Plain fp64, no contraction into fma, no LDS, no scratch.  A lane only reads state that this launch does not write,
// or keeps it in registers across the post and pre halves.
#include "rmpc_stack_step.h"

#include "arm_dyn.h"
#include "loop_plant.h"
#include "stack_couple.h"

#pragma clang fp contract(off)

namespace dartmpc {

// One plant step of experiment b with the tilt command `up`, the new state stored by lane 0: loop_step.hip's
// loop_plant_step for these arguments (tray: x[0..3] are stored, pz and vz do not move)
template <bool LM>
__device__ __forceinline__ void rmpc_stack_plant_step(const RmpcStackStepArgs& a, int b, int lane, const double* up,
                                                      double* x, double* tilt) {
    if constexpr (LM) lm_cross_plant_step(a.plant_pvec + 34 * b, lane & (kLmGroup - 1), a.a_lag, a.Ts, up, x, tilt);
    else tray_plant_step(a.plant, a.mu[b], up, x, tilt);
    if (lane == 0) {
        constexpr int NX = LM ? 8 : 6;
#pragma unroll
        for (int i = 0; i < (LM ? 8 : 4); ++i) a.x[NX * b + i] = x[i];
        a.tilt[2 * b] = tilt[0]; a.tilt[2 * b + 1] = tilt[1];
    }
}

template <bool LM>
__global__ __launch_bounds__(kStackWave* kStackWaves) void rmpc_stack_step_kernel(RmpcStackStepArgs a) {
    constexpr int NX = LM ? 8 : 6;
    const int lane = threadIdx.x & (kStackWave - 1);
    const int b = blockIdx.x * kStackWaves + (threadIdx.x >> 6);
    if (b >= a.E) return;                    // wave-uniform
    const size_t E = (size_t)a.E;
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
        const size_t row = (size_t)a.k * E + b;
        const double dx = x[0] - t0, dy = x[2] - t2;
        const double en = sqrt(dx * dx + dy * dy);
        const Q4 qc = tilt_quat(u);
        const double* ep = a.ee_pos + (size_t)a.ee_stride * 2 * b;
        const TrayMeasure m = tray_from_arms(ep, ep + a.ee_stride, a.ee_quat + 8 * (size_t)b,
                                             a.ee_quat + 8 * (size_t)b + 4, a.grasp);
        const bool held = tilt_held(m);
        if (a.logs && lane < 14) a.log_theta[14 * row + lane] = a.theta[14 * b + lane];
        if (lane == 0) {
            const int nl = a.nlog[b];
            if (!a.done[b]) {
                if (a.logs && nl >= 0 && nl < a.log_rows) {
                    const size_t er = (size_t)nl * E + b;
                    a.log_pos_err[2 * er] = t0 - x[0]; a.log_pos_err[2 * er + 1] = t2 - x[2];
                    a.log_pos_err_norm[er] = en;
                    a.log_u_cmd[2 * er] = u[0]; a.log_u_cmd[2 * er + 1] = u[1];
                    a.log_timestep[er] = a.k * a.Ts;
                }
                a.nlog[b] = nl + 1;
                if (en < a.pos_tol) a.done[b] = 1;
            }
            const int status = a.status[b], iters = a.iters[b];
            if (a.logs) {
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
            loop_metrics_step(a.metrics + 8 * b, a.k, a.Ts, en, u, status, iters, LM ? x[4] : 0.0, LM ? x[6] : 0.0);
            stack_metrics_step(a.stack_metrics + STACK_NMETRIC * b, m, u, a.tray_pos + 3 * b);
            if (a.stack_logs) {
                a.log_U[2 * row] = u[0]; a.log_U[2 * row + 1] = u[1];
                a.log_quat[4 * row] = qc.w; a.log_quat[4 * row + 1] = qc.x;
                a.log_quat[4 * row + 2] = qc.y; a.log_quat[4 * row + 3] = qc.z;
                stack_log_row(a.log_tilt, a.log_tray, row, m);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) prev[i] = x[i];
        double up[2] = {u[0], u[1]};
        if (a.couple == STACK_ACHIEVED) {
            // tilt := the achieved tilt (the last one where it is not finite); driven with itself the lag leaves it
            if (!held) { tilt[0] = m.tilt[0]; tilt[1] = m.tilt[1]; }
            up[0] = tilt[0]; up[1] = tilt[1];
        }
        rmpc_stack_plant_step<LM>(a, b, lane, up, x, tilt);
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

}  // namespace dartmpc

using namespace dartmpc;

extern "C" hipError_t dartmpc_launch_rmpc_stack_step(const RmpcStackStepArgs* args, int lm, hipStream_t stream) {
    if (args->E <= 0 || (!args->do_post && !args->do_pre)) return hipSuccess;
    // (lane i owns node i of the staged reference)
    if (args->N < 1 || args->N > kStackWave - 1) return hipErrorInvalidValue;
    const dim3 grid((args->E + kStackWaves - 1) / kStackWaves), block(kStackWave * kStackWaves);
    if (lm) hipLaunchKernelGGL(rmpc_stack_step_kernel<true>, grid, block, 0, stream, *args);
    else hipLaunchKernelGGL(rmpc_stack_step_kernel<false>, grid, block, 0, stream, *args);
    return hipGetLastError();
}
