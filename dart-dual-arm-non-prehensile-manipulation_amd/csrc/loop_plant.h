// loop_plant.h -- the plant steps and the streaming metrics that the closed-loop glue kernels share (loop_step.hip:
// pmpc_loop_kernel / rmpc_loop_kernel; stack_step.hip: the PMPC loop closed through the dual-arm layer).  Device
// functions only, plain fp64 in the operation order of the numpy code (harness.TrayPlant, harness.LmpcPlant,
// harness.rollout_metrics): the including unit compiles them with contraction into fma off.
#pragma once
#include <hip/hip_runtime.h>

#include "loop_step.h"

#pragma clang fp contract(off)

namespace dartmpc {

// harness.TrayPlant.step: x [6], tilt [2] in/out
__host__ __device__ __forceinline__ void tray_plant_step(const PlantArgs& p, double mu, const double* u, double* x,
                                                double* tilt) {
    tilt[0] += p.a_lag * (u[0] - tilt[0]);
    tilt[1] += p.a_lag * (u[1] - tilt[1]);
    const double s0 = sin(tilt[0]), s1 = sin(tilt[1]);
    const double fric = p.mu_c * fabs(p.g);
    const double h = p.dt, h2 = h / 2, h6 = h / 6;
    auto acc = [&](double s, double v) { return p.g * s - mu * v - fric * tanh(v / p.v_c); };
    const double k1x = x[1], k1y = x[3];
    const double a1x = acc(s0, k1x), a1y = acc(s1, k1y);
    const double k2x = x[1] + h2 * a1x, k2y = x[3] + h2 * a1y;
    const double a2x = acc(s0, k2x), a2y = acc(s1, k2y);
    const double k3x = x[1] + h2 * a2x, k3y = x[3] + h2 * a2y;
    const double a3x = acc(s0, k3x), a3y = acc(s1, k3y);
    const double k4x = x[1] + h * a3x, k4y = x[3] + h * a3y;
    const double a4x = acc(s0, k4x), a4y = acc(s1, k4y);
    x[0] = x[0] + h6 * (k1x + 2 * k2x + 2 * k3x + k4x);
    x[1] = x[1] + h6 * (a1x + 2 * a2x + 2 * a3x + a4x);
    x[2] = x[2] + h6 * (k1y + 2 * k2y + 2 * k3y + k4y);
    x[3] = x[3] + h6 * (a1y + 2 * a2y + 2 * a3y + a4y);
    // (pz, vz: zero derivative)
}

// The LMPC model as a plant (safe_dynamics, rlmpc2.py:260-429): kLmGroup = 8 lanes per instance.  An RK4 stage has
// six independent Stribeck terms (tanh + exp each) and two sines: lane r of a group evaluates term r (lanes 6, 7
// repeat terms 0, 1) and the sine of th_x (even r) or th_y (odd r), the same instructions on every lane, and the
// group exchanges the eight values by shuffles; the cheap combination is computed by every lane.  Every term is
// computed by exactly one expression in numpy's order (harness.LmpcPlant), so the result does not depend on the lane
// mapping.
constexpr int kLmGroup = 8;
constexpr double kLmG = 9.81;      // rlmpc2.py:354

// squash_param (:296-298)
__device__ __forceinline__ double lm_squash(double p) { return fabs(p) + 1e-6; }

struct LmPlantPrm {
    double m_x, m_y, c_x, c_y, k_x, k_y, I_x, I_y, r_x, r_y, c_rot_x, c_rot_y, h_com_x, h_com_y;
    double Fs, Fc, Bv, vs, eps;     // the Stribeck term of this lane
};

// safe_dynamics at x with sin(tilt) = (sa, sb): xdot [8].  r = lane in the group.
__device__ __forceinline__ void lm_plant_dyn(const LmPlantPrm& P, int r, const double* x, double sa, double sb,
                                             double* d) {
    const double px = x[0], vx = x[1], py = x[2], vy = x[3], th_x = x[4], om_x = x[5], th_y = x[6], om_y = x[7];
    const double v_slip_x = vx - P.r_x * om_y;                          // :387-391
    const double v_slip_y = vy - (-P.r_y * om_x);
    const int t = r < 6 ? r : r - 6;
    const double v = t == 0 ? vx : t == 1 ? vy : t == 2 ? v_slip_x : t == 3 ? v_slip_y : t == 4 ? om_x : om_y;
    const double e = exp(-fabs(v) / (P.vs + 1e-12));                    // :372-376
    const double F = tanh(v / P.eps) * (P.Fc + (P.Fs - P.Fc) * e) + P.Bv * v;
    const double s = sin((r & 1) ? th_y : th_x);
    const double Ff_x = __shfl(F, 0, kLmGroup), Ff_y = __shfl(F, 1, kLmGroup);
    const double F_roll_x = __shfl(F, 2, kLmGroup), F_roll_y = __shfl(F, 3, kLmGroup);
    const double T_noslip_x = __shfl(F, 4, kLmGroup), T_noslip_y = __shfl(F, 5, kLmGroup);
    const double s_thx = __shfl(s, 0, kLmGroup), s_thy = __shfl(s, 1, kLmGroup);
    const double Gx = P.m_x * (kLmG * sa), Gy = P.m_y * (kLmG * sb);   // :353-357
    const double tau_slip_x = -P.r_y * F_roll_y, tau_slip_y = -P.r_x * F_roll_x;      // :402-403
    const double T_damp_x = P.c_rot_x * om_x, T_damp_y = P.c_rot_y * om_y;            // :410-411
    const double tau_topple_x = -P.m_y * kLmG * P.h_com_x * s_thx;      // :414-415
    const double tau_topple_y = -P.m_x * kLmG * P.h_com_y * s_thy;
    const double tau_x = tau_slip_x - T_noslip_x - T_damp_x + tau_topple_x;           // :418-419
    const double tau_y = tau_slip_y - T_noslip_y - T_damp_y + tau_topple_y;
    const double rhs_x = Gx - P.c_x * vx - P.k_x * px - Ff_x - F_roll_x;              // :427
    const double rhs_y = Gy - P.c_y * vy - P.k_y * py - Ff_y - F_roll_y;
    d[0] = vx; d[1] = rhs_x / P.m_x; d[2] = vy; d[3] = rhs_y / P.m_y;                 // :429
    d[4] = om_x; d[5] = tau_x / (P.I_x + 1e-12); d[6] = om_y; d[7] = tau_y / (P.I_y + 1e-12);   // :422-423
}

constexpr double kMetricTol = 0.01;     // logger.py:162

// harness.LmpcPlant.step with the command -u: tilt is the lagged PMPC / RMPC command, the model's input sin(-tilt)
__device__ __forceinline__ void lm_cross_plant_step(const double* pv, int r, double a_lag, double h, const double* u,
                                                    double* x, double* tilt) {
    tilt[0] += a_lag * (u[0] - tilt[0]);
    tilt[1] += a_lag * (u[1] - tilt[1]);
    LmPlantPrm P;
    P.m_x = lm_squash(pv[0]); P.m_y = lm_squash(pv[1]); P.c_x = lm_squash(pv[2]); P.c_y = lm_squash(pv[3]);
    P.k_x = lm_squash(pv[4]); P.k_y = lm_squash(pv[5]); P.I_x = lm_squash(pv[16]); P.I_y = lm_squash(pv[17]);
    P.r_x = lm_squash(pv[18]); P.r_y = lm_squash(pv[19]); P.c_rot_x = lm_squash(pv[20]); P.c_rot_y = lm_squash(pv[21]);
    P.h_com_x = lm_squash(pv[32]); P.h_com_y = lm_squash(pv[33]);
    {
        const int t = r < 6 ? r : r - 6;
        const int o = t == 0 || t == 2 ? 6 : t == 1 || t == 3 ? 11 : t == 4 ? 22 : 27;
        P.Fs = pv[o]; P.Fc = pv[o + 1]; P.Bv = pv[o + 2]; P.vs = lm_squash(pv[o + 3]); P.eps = lm_squash(pv[o + 4]);
    }
    const double st = sin((r & 1) ? -tilt[1] : -tilt[0]);
    const double sa = __shfl(st, 0, kLmGroup), sb = __shfl(st, 1, kLmGroup);
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
}

// harness.rollout_metrics, one step: m [8] in/out, the instance's row in memory, read whole before it is written
// (one lane per instance)
__device__ __forceinline__ void loop_metrics_step(double* m, int k, double Ts, double e, const double* u, int status,
                                                  int iters, double th_x, double th_y) {
    const double first = m[1], eff = m[2], emax = m[3], bad = m[4], its = m[5], rot = m[6], n = m[7];
    const double un = sqrt(u[0] * u[0] + u[1] * u[1]);
    const double th = fabs(th_x) > fabs(th_y) ? fabs(th_x) : fabs(th_y);
    m[0] = e;
    m[1] = (first < 0.0 && e < kMetricTol) ? (double)k : first;
    m[2] = eff + un * Ts;
    m[3] = e > emax ? e : emax;
    m[4] = status != 0 ? bad + 1.0 : bad;
    m[5] = its + (double)iters;
    m[6] = th > rot ? th : rot;
    m[7] = n + 1.0;
}

}  // namespace dartmpc
