// stack_step.hip -- the PMPC closed loop through the dual-arm layer: the two small kernels between the unchanged solve
// and the unchanged arm kernels (stack_step.h).  stack_command_kernel turns the solve's u0 into the tray pose that
// arm_dyn_kernel's coordinator prologue reads; stack_step_kernel<LM> measures the tray the two arms hold and is then
// pmpc_loop_kernel<LM>'s post / pre with the tilt the plant sees chosen by `couple`; tray_from_arms_kernel is the
// measurement alone.
//
// One wave64 per experiment, kStackWaves experiments per block, as pmpc_loop_kernel: the measurement is a few dozen
// fp64 operations on uniform loads, computed by every lane alike and stored by lane 0; the LMPC plant's step wants its
// groups of kLmGroup lanes.  Plain fp64, no contraction into fma (the command quaternion is log_quat's expressions, so a
// pose built here and one built from a logged log_quat are the same bits; the plant steps are loop_plant.h's), no LDS,
// no scratch.  A lane only reads state that this launch does not write, or keeps it in registers.
#include "stack_step.h"

#include "arm_dyn.h"
#include "loop_plant.h"
#include "stack_couple.h"

#pragma clang fp contract(off)

namespace dartmpc {

__global__ __launch_bounds__(kStackWave* kStackWaves) void tray_from_arms_kernel(TrayFromArmsArgs a) {
    const int lane = threadIdx.x & (kStackWave - 1);
    const int e = blockIdx.x * kStackWaves + (threadIdx.x >> 6);
    if (e >= a.E) return;                    // wave-uniform
    const double* ep = a.ee_pos + (size_t)a.ee_stride * 2 * e;
    const TrayMeasure m = tray_from_arms(ep, ep + a.ee_stride, a.ee_quat + 8 * (size_t)e, a.ee_quat + 8 * (size_t)e + 4,
                                         a.grasp);
    if (lane == 0) {
        double* t = a.tray + 7 * (size_t)e;
        st3(t, m.p);
        t[3] = m.q.w; t[4] = m.q.x; t[5] = m.q.y; t[6] = m.q.z;
        a.tilt[2 * e] = m.tilt[0]; a.tilt[2 * e + 1] = m.tilt[1];
        a.diag[3 * e] = m.yaw; a.diag[3 * e + 1] = m.gap; a.diag[3 * e + 2] = m.angle;
    }
}

__global__ __launch_bounds__(kStackWave* kStackWaves) void stack_command_kernel(StackCommandArgs a) {
    const int lane = threadIdx.x & (kStackWave - 1);
    const int e = blockIdx.x * kStackWaves + (threadIdx.x >> 6);
    if (e >= a.E) return;                    // wave-uniform
    const double u[2] = {a.u0[2 * e], a.u0[2 * e + 1]};
    const Q4 q = tilt_quat(u);
    if (lane == 0) {
        double* t = a.tray_cmd + 7 * (size_t)e;
        t[0] = a.tray_pos[3 * e]; t[1] = a.tray_pos[3 * e + 1]; t[2] = a.tray_pos[3 * e + 2];
        t[3] = q.w; t[4] = q.x; t[5] = q.y; t[6] = q.z;
    }
}

// The plant hook: one step of experiment b's object with the tilt command `up` through the plant's lag, the new state
// stored by lane 0 (loop_step.hip's loop_plant_step for these arguments).  A controller whose loop is closed through
// the arms the same way supplies its own arguments and calls this.
template <bool LM>
__device__ __forceinline__ void stack_plant_step(const StackStepArgs& a, int b, int lane, const double* up, double* x,
                                                 double* tilt) {
    if constexpr (LM) lm_cross_plant_step(a.plant_pvec + 34 * b, lane & (kLmGroup - 1), a.a_lag, a.Ts, up, x, tilt);
    else tray_plant_step(a.plant, a.prm[6 * b], up, x, tilt);
    if (lane == 0) {
        constexpr int NX = LM ? 8 : 6;
#pragma unroll
        for (int i = 0; i < (LM ? 8 : 4); ++i) a.x[NX * b + i] = x[i];
        a.tilt[2 * b] = tilt[0]; a.tilt[2 * b + 1] = tilt[1];
    }
}

template <bool LM>
__global__ __launch_bounds__(kStackWave* kStackWaves) void stack_step_kernel(StackStepArgs a) {
    constexpr int NX = LM ? 8 : 6;
    const int lane = threadIdx.x & (kStackWave - 1);
    const int b = blockIdx.x * kStackWaves + (threadIdx.x >> 6);
    if (b >= a.E) return;                    // wave-uniform
    double x[NX], tilt[2];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = a.x[NX * b + i];
    const double pz = LM ? a.pz_vz[2 * b] : x[4], vz = LM ? a.pz_vz[2 * b + 1] : x[5];

    if (a.do_post) {
        tilt[0] = a.tilt[2 * b]; tilt[1] = a.tilt[2 * b + 1];
        const double u[2] = {a.u0[2 * b], a.u0[2 * b + 1]};
        const size_t row = (size_t)a.k * a.E + b;
        const Q4 qc = tilt_quat(u);
        const double* ep = a.ee_pos + (size_t)a.ee_stride * 2 * b;
        const TrayMeasure m = tray_from_arms(ep, ep + a.ee_stride, a.ee_quat + 8 * (size_t)b,
                                             a.ee_quat + 8 * (size_t)b + 4, a.grasp);
        const bool held = !(isfinite(m.tilt[0]) && isfinite(m.tilt[1]));
        if (lane == 0) {
            const int status = a.status[b], iters = a.iters[b];
            if (a.logs) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a.log_X[6 * row + i] = x[i];
                    if constexpr (LM) a.log_rot[4 * row + i] = x[4 + i];
                }
                a.log_X[6 * row + 4] = pz; a.log_X[6 * row + 5] = vz;
                a.log_U[2 * row] = u[0]; a.log_U[2 * row + 1] = u[1];
                a.log_quat[4 * row] = qc.w; a.log_quat[4 * row + 1] = qc.x;
                a.log_quat[4 * row + 2] = qc.y; a.log_quat[4 * row + 3] = qc.z;
                a.log_loss[row] = a.f[b];
                a.log_status[row] = status;
                a.log_iters[row] = iters;
            }
            const double dx = x[0] - a.target[6 * b], dy = x[2] - a.target[6 * b + 2];
            loop_metrics_step(a.metrics + 8 * b, a.k, a.Ts, sqrt(dx * dx + dy * dy), u, status, iters, LM ? x[4] : 0.0,
                              LM ? x[6] : 0.0);
            stack_metrics_step(a.stack_metrics + STACK_NMETRIC * b, m, u, a.tray_pos + 3 * b);
            if (a.stack_logs) {
                a.log_tilt[2 * row] = m.tilt[0]; a.log_tilt[2 * row + 1] = m.tilt[1];
                double* t = a.log_tray + 7 * row;
                st3(t, m.p);
                t[3] = m.q.w; t[4] = m.q.x; t[5] = m.q.y; t[6] = m.q.z;
            }
        }
        double up[2] = {u[0], u[1]};
        if (a.couple == STACK_ACHIEVED) {
            // tilt := the achieved tilt (the last one where it is not finite); driven with itself the lag leaves it
            if (!held) { tilt[0] = m.tilt[0]; tilt[1] = m.tilt[1]; }
            up[0] = tilt[0]; up[1] = tilt[1];
        }
        stack_plant_step<LM>(a, b, lane, up, x, tilt);
    }
    if (a.do_pre && lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a.x0[6 * b + i] = x[i];
        a.x0[6 * b + 4] = pz; a.x0[6 * b + 5] = vz;
    }
}

}  // namespace dartmpc

using namespace dartmpc;

namespace {
dim3 stack_grid(int E) { return dim3((E + kStackWaves - 1) / kStackWaves); }
const dim3 kStackBlock(kStackWave* kStackWaves);
}  // namespace

extern "C" hipError_t dartmpc_launch_tray_from_arms(const TrayFromArmsArgs* args, hipStream_t stream) {
    if (args->E <= 0) return hipSuccess;
    hipLaunchKernelGGL(tray_from_arms_kernel, stack_grid(args->E), kStackBlock, 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_stack_command(const StackCommandArgs* args, hipStream_t stream) {
    if (args->E <= 0) return hipSuccess;
    hipLaunchKernelGGL(stack_command_kernel, stack_grid(args->E), kStackBlock, 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_stack_step(const StackStepArgs* args, int lm, hipStream_t stream) {
    if (args->E <= 0 || (!args->do_post && !args->do_pre)) return hipSuccess;
    if (lm) hipLaunchKernelGGL(stack_step_kernel<true>, stack_grid(args->E), kStackBlock, 0, stream, *args);
    else hipLaunchKernelGGL(stack_step_kernel<false>, stack_grid(args->E), kStackBlock, 0, stream, *args);
    return hipGetLastError();
}
