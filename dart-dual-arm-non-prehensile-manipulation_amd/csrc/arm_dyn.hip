// arm_dyn.hip -- the dynamics snapshot of a serial arm (ARMCONTROL.compute_dynamics) and a plant step, for gfx950.
//
// arm_dyn_kernel replaces the MuJoCo calls of ARMCONTROL.compute_dynamics (PMPC/src/controller/arm.py:111-199) for
// a chain of n <= ARM_NMAX hinge joints described by one model row (arm_dyn.h): from (q, qd) and the mocap target it
// writes the snapshot row arm_qp_kernel reads (arm_qp.h:arm_snap_len),
//   jac     [jacp; jacr] at the EE body's frame origin (mj_jacBody, :120-126)
//   M       composite rigid bodies + armature (mj_fullM, :128-131), bit-symmetric
//   Mx_inv  J M^-1 J' through a Cholesky factor of M (mj_solveM, :133-139); NaN on a non-positive pivot
//   jacDot  of the world point (0, 0, offset) attached to the EE body (the reference's call read literally,
//           :141-152) or of the EE body origin (ARM_JACDOT_BODY)
//   h       Newton-Euler at qdd = 0 with gravity (qfrc_bias, :155)
//   ee_pos  origin + offset R[:, 2] (:158-165);  rotvec of mocap_quat (x) conj(ee_quat) as scipy's as_rotvec (:175-183)
// With args.tray set the mocap target is DACTL._resolve_ee_pos's (PMPC/src/dualctl.py:22-56): tray pose b / 2 composed
// with grasp transform b % 2 by quaternion products.
//
// Mapping (the small-batch regime: 36 arms per dual-arm step): one wave64 per arm, everything in LDS, fp64.  The chain
// recursions are short and latency-bound: every lane runs them alike on uniform LDS reads and lane i keeps link i, so
// no lane waits on another; columns of J / jacDot are lane-per-joint, M and Mx_inv lane-per-entry, the Cholesky
// factor lives in the registers of every lane and lane c solves for column c of J'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arm_dyn.h"

namespace dartmpc {

struct ArmDynShared {
    double mdl[ARM_LINK_LEN * ARM_NMAX + 18];
    double snap[ARM_NMAX * ARM_NMAX + 16 * ARM_NMAX + 45];
    double mq[4];                 // mocap_quat
    double Y[6][ARM_NMAX];        // L^-1 J'
    ArmKin K;
};

template <int n>
__global__ __launch_bounds__(kWave) void arm_dyn_kernel(ArmDynArgs a) {
    __shared__ ArmDynShared SH;
    const int b = blockIdx.x, l = threadIdx.x;
    constexpr int SL = arm_snap_len(n), ML = arm_model_len(n);
    double* q = SH.snap;
    double* qd = q + n;
    double* qp = q + 2 * n;
    double* mocap = q + 3 * n;
    double* ee = mocap + 3;
    double* rv = ee + 3;
    double* J = q + 3 * n + 9;
    double* Jd = J + 6 * n;
    double* M = Jd + 6 * n;
    double* hb = M + n * n;
    double* Mxi = hb + n;
    {
        const double* gm = a.model + (size_t)a.model_stride * (a.model_mod ? b % a.model_mod : b);
        for (int e = l; e < ML; e += kWave) SH.mdl[e] = gm[e];
        const size_t qo = (size_t)a.q_stride * b;
        if (l < n) { q[l] = a.q[qo + l]; qd[l] = a.qd[qo + l]; qp[l] = a.qp[qo + l]; }
        if (a.tray) {
            if (l == 0) {   // T_world,ee = T_world,tray T_tray,grasp
                const double* tp = a.tray + (size_t)7 * (b >> 1);
                const double* gr = a.grasp + 7 * (b & 1);
                const Q4 qt = qunit(ld4(tp + 3));
                st3(mocap, ld3(tp) + qrot(qt, ld3(gr)));
                const Q4 r = qmul(qt, qunit(ld4(gr + 3)));
                SH.mq[0] = r.w; SH.mq[1] = r.x; SH.mq[2] = r.y; SH.mq[3] = r.z;
            }
        } else if (l < 7) {
            const double v = a.mocap[(size_t)a.mocap_stride * b + l];
            if (l < 3) mocap[l] = v; else SH.mq[l - 3] = v;
        }
    }
    __syncthreads();
    ArmKin& K = SH.K;
    arm_kin_M_h<n>(K, SH.mdl, q, qd, l);

    const double* ep = SH.mdl + 7 + ARM_LINK_LEN * n;
    const double offset = ep[7];
    if (l < n) {    // column l of jac and jacDot
        const V3 z = ld3(K.z[l]), p = ld3(K.p[l]), pe = ld3(K.pe), we = ld3(K.we);
        const V3 pt = a.jacdot_point == ARM_JACDOT_BODY ? pe : V3{0.0, 0.0, offset};
        const V3 vpt = ld3(K.ve) + cross(we, pt - pe);
        const V3 jp = cross(z, pe - p);
        const V3 zd = cross(ld3(K.w[l]), z);
        const V3 jdp = cross(zd, pt - p) + cross(z, vpt - ld3(K.v[l]));
        J[0 * n + l] = jp.x; J[1 * n + l] = jp.y; J[2 * n + l] = jp.z;
        J[3 * n + l] = z.x; J[4 * n + l] = z.y; J[5 * n + l] = z.z;
        Jd[0 * n + l] = jdp.x; Jd[1 * n + l] = jdp.y; Jd[2 * n + l] = jdp.z;
        Jd[3 * n + l] = zd.x; Jd[4 * n + l] = zd.y; Jd[5 * n + l] = zd.z;
        hb[l] = K.h[l];
    }
    if (l < n * n) M[l] = K.M[l];
    if (l == ARM_NMAX) {   // ee_pos and the orientation error
        const Q4 Qe = ld4(K.Qe);
        st3(ee, ld3(K.pe) + offset * qrot(Qe, V3{0.0, 0.0, 1.0}));
        Q4 e = qunit(qmul(ld4(SH.mq), Q4{Qe.w, -Qe.x, -Qe.y, -Qe.z}));
        if (e.w < 0.0) e = Q4{-e.w, -e.x, -e.y, -e.z};
        const double vn = sqrt(e.x * e.x + e.y * e.y + e.z * e.z);
        const double th = 2.0 * atan2(vn, e.w), t2 = th * th;
        const double sc = th <= 1e-3 ? 2.0 + t2 * (1.0 / 12.0) + 7.0 * (t2 * t2) * (1.0 / 2880.0) : th / vn;
        rv[0] = sc * e.x; rv[1] = sc * e.y; rv[2] = sc * e.z;
    }
    __syncthreads();
    {   // Mx_inv = (L^-1 J')' (L^-1 J')
        double L[n * (n + 1) / 2], iD[n], y[n];
        const bool ok = chol_factor<n>(K.M, n, L, iD);
        const int c = l < 6 ? l : 0;
#pragma unroll
        for (int k = 0; k < n; ++k) y[k] = J[c * n + k];
        chol_forward<n>(L, iD, y);
        if (l < 6) {
#pragma unroll
            for (int k = 0; k < n; ++k) SH.Y[l][k] = y[k];
        }
        __syncthreads();
        if (l < 36) {
            const int r = l / 6, cc = l % 6, lo = r < cc ? r : cc, hi = r < cc ? cc : r;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < n; ++k) s = fma(SH.Y[lo][k], SH.Y[hi][k], s);
            Mxi[l] = ok ? s : __builtin_nan("");
        }
    }
    __syncthreads();
    double* gs = a.snap + (size_t)SL * b;
    for (int e = l; e < SL; e += kWave) gs[e] = SH.snap[e];
    if (a.ee_quat && l < 4) a.ee_quat[(size_t)4 * b + l] = K.Qe[l];
    if (a.mocap_out && l < 7) a.mocap_out[(size_t)7 * b + l] = l < 3 ? mocap[l] : SH.mq[l - 3];
}

struct ArmPlantShared {
    double mdl[ARM_LINK_LEN * ARM_NMAX + 18];
    double q[ARM_NMAX], qd[ARM_NMAX], tau[ARM_NMAX], rhs[ARM_NMAX];
    ArmKin K;
};

template <int n>
__global__ __launch_bounds__(kWave) void arm_plant_kernel(ArmPlantArgs a) {
    __shared__ ArmPlantShared SH;
    const int b = blockIdx.x, l = threadIdx.x;
    constexpr int SL = arm_snap_len(n), ML = arm_model_len(n), PL = arm_prm_len(n);
    const double* gm = a.model + (size_t)a.model_stride * (a.model_mod ? b % a.model_mod : b);
    const double* gp = a.prm + (size_t)a.prm_stride * b;
    const double* gs = a.snap + (size_t)SL * b;
    const size_t ob = (size_t)n * b;
    const double dt = gp[PL - 1];
    const int st = a.status[b];
    for (int e = l; e < ML; e += kWave) SH.mdl[e] = gm[e];
    if (l < n) {
        SH.q[l] = a.q[ob + l];
        SH.qd[l] = a.qd[ob + l];
        SH.tau[l] = st >= 0 ? a.tau[ob + l] : 0.0;     // a failed solve commands zero torque (arm.py:438-442)
    }
    __syncthreads();
    ArmKin& K = SH.K;
    arm_kin_M_h<n>(K, SH.mdl, SH.q, SH.qd, l);
    if (l < n) {
        const double d = SH.mdl[7 + ARM_LINK_LEN * l + 11];
        K.M[l * n + l] += dt * d;
        SH.rhs[l] = SH.tau[l] - K.h[l] - d * SH.qd[l];
    }
    __syncthreads();
    double L[n * (n + 1) / 2], iD[n], x[n];
    chol_factor<n>(K.M, n, L, iD);        // (a lost pivot leaves NaN in the state: nothing to report it to)
#pragma unroll
    for (int k = 0; k < n; ++k) x[k] = SH.rhs[k];
    chol_forward<n>(L, iD, x);
    chol_backward<n>(L, iD, x);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < n; ++k) acc = k == l ? x[k] : acc;
    if (l < n) {
        const double qd1 = fma(dt, acc, SH.qd[l]);
        a.qd[ob + l] = qd1;
        a.q[ob + l] = fma(dt, qd1, SH.q[l]);
        if (st >= 0) a.qp[ob + l] = a.qdd[ob + l];     // (a failed solve keeps the last solution, as the worker does)
        if (a.q_log) {
            a.q_log[ob + l] = SH.q[l];
            a.qd_log[ob + l] = SH.qd[l];
            a.tau_log[ob + l] = SH.tau[l];
        }
    }
    const double* mocap = gs + 3 * n;
    if (a.q_log && l < 3) a.ee_log[(size_t)3 * b + l] = mocap[3 + l];
    if (l == 0) {
        if (a.q_log) { a.loss_log[b] = a.loss[b]; a.status_log[b] = st; }
        double* m = a.metrics + (size_t)ARM_NMETRIC * b;
        const double ex = mocap[3] - mocap[0], ey = mocap[4] - mocap[1], ez = mocap[5] - mocap[2];
        const double err = sqrt(ex * ex + ey * ey + ez * ez);
        const double* tmax = gp + 36 + 2 * n * n + 5 * n;
        double tr = 0.0;
#pragma unroll
        for (int k = 0; k < n; ++k) tr = fmax(tr, fabs(SH.tau[k]) / tmax[k]);
        m[0] = err;
        m[1] = fmax(m[1], err);
        m[2] = sqrt(mocap[6] * mocap[6] + mocap[7] * mocap[7] + mocap[8] * mocap[8]);
        m[3] += st != 0 ? 1.0 : 0.0;
        m[4] += (double)a.iters[b];
        m[5] = fmax(m[5], tr);
    }
}

}  // namespace dartmpc

#define DART_ARM_N_SWITCH(KERNEL, args, stream)                                                        \
    switch ((args)->n) { /* joint count as a compile-time constant: every chain loop unrolls */        \
        case 1: hipLaunchKernelGGL(dartmpc::KERNEL<1>, g, w, 0, stream, *(args)); break;               \
        case 2: hipLaunchKernelGGL(dartmpc::KERNEL<2>, g, w, 0, stream, *(args)); break;               \
        case 3: hipLaunchKernelGGL(dartmpc::KERNEL<3>, g, w, 0, stream, *(args)); break;               \
        case 4: hipLaunchKernelGGL(dartmpc::KERNEL<4>, g, w, 0, stream, *(args)); break;               \
        case 5: hipLaunchKernelGGL(dartmpc::KERNEL<5>, g, w, 0, stream, *(args)); break;               \
        case 6: hipLaunchKernelGGL(dartmpc::KERNEL<6>, g, w, 0, stream, *(args)); break;               \
        case 7: hipLaunchKernelGGL(dartmpc::KERNEL<7>, g, w, 0, stream, *(args)); break;               \
        case 8: hipLaunchKernelGGL(dartmpc::KERNEL<8>, g, w, 0, stream, *(args)); break;               \
        default: return hipErrorInvalidValue;                                                          \
    }

extern "C" hipError_t dartmpc_launch_arm_dyn(const dartmpc::ArmDynArgs* args, hipStream_t stream) {
    if (args->B <= 0) return hipSuccess;
    const dim3 g(args->B), w(dartmpc::kWave);
    DART_ARM_N_SWITCH(arm_dyn_kernel, args, stream)
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_arm_plant(const dartmpc::ArmPlantArgs* args, hipStream_t stream) {
    if (args->B <= 0) return hipSuccess;
    const dim3 g(args->B), w(dartmpc::kWave);
    DART_ARM_N_SWITCH(arm_plant_kernel, args, stream)
    return hipGetLastError();
}
