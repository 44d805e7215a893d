// stack_couple.h -- what the kernels that close an MPC loop through the dual-arm layer share (stack_step.hip: PMPC;
// rmpc_stack_step.hip: RMPC): the command quaternion, the tray two arms hold, and the stack metrics' row update.
// Device functions only, plain fp64 in the operation order of tests/stack_refs.py: the including unit compiles them
// with contraction into fma off.
#pragma once
#include <hip/hip_runtime.h>

#include "arm_dyn.h"
#include "stack_step.h"

#pragma clang fp contract(off)

namespace dartmpc {

constexpr int kStackWave = 64;
constexpr int kStackWaves = 4;

__device__ __forceinline__ Q4 qconj(Q4 a) { return Q4{a.w, -a.x, -a.y, -a.z}; }
__device__ __forceinline__ Q4 qneg(Q4 a) { return Q4{-a.w, -a.x, -a.y, -a.z}; }
__device__ __forceinline__ double norm3(V3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }

// pmpc.tilt_to_quat, the expressions of pmpc_loop_kernel's log_quat: Euler xyz [u1, -u0, 0] -> (w, x, y, z)
__device__ __forceinline__ Q4 tilt_quat(const double* u) {
    const double ax = u[1] / 2.0, ay = -u[0] / 2.0;
    const double cx = cos(ax), cy = cos(ay), cz = 1.0, sx = sin(ax), sy = sin(ay), sz = 0.0;
    return Q4{cx * cy * cz + sx * sy * sz, sx * cy * cz - cx * sy * sz, cx * sy * cz + sx * cy * sz,
              cx * cy * sz - sx * sy * cz};
}

// the tray two arms hold (stack_step.h): EE points eL, eR, EE orientations, grasp [2][7]
struct TrayMeasure {
    V3 p;
    Q4 q;
    double tilt[2], yaw, gap, angle;
};

__device__ __forceinline__ TrayMeasure tray_from_arms(const double* ee_L, const double* ee_R, const double* eq_L,
                                                      const double* eq_R, const double* grasp) {
    TrayMeasure m;
    const V3 eL = ld3(ee_L), eR = ld3(ee_R), gL = ld3(grasp), gR = ld3(grasp + 7);
    const Q4 qL = qunit(qmul(ld4(eq_L), qconj(ld4(grasp + 3))));
    Q4 qR = qunit(qmul(ld4(eq_R), qconj(ld4(grasp + 10))));
    if (qL.w * qR.w + qL.x * qR.x + qL.y * qR.y + qL.z * qR.z < 0.0) qR = qneg(qR);
    Q4 qt = qunit(Q4{qL.w + qR.w, qL.x + qR.x, qL.y + qR.y, qL.z + qR.z});
    if (qt.w < 0.0) qt = qneg(qt);
    m.q = qt;
    m.p = 0.5 * ((eL - qrot(qt, gL)) + (eR - qrot(qt, gR)));
    // Euler xyz angles of qt, the inverse of tilt_quat (a NaN passes the clamp)
    const double roll = atan2(2.0 * (qt.w * qt.x + qt.y * qt.z), 1.0 - 2.0 * (qt.x * qt.x + qt.y * qt.y));
    const double sp = 2.0 * (qt.w * qt.y - qt.z * qt.x);
    const double pitch = asin(sp > 1.0 ? 1.0 : sp < -1.0 ? -1.0 : sp);
    m.yaw = atan2(2.0 * (qt.w * qt.z + qt.x * qt.y), 1.0 - 2.0 * (qt.y * qt.y + qt.z * qt.z));
    m.tilt[0] = -pitch;
    m.tilt[1] = roll;
    m.gap = fabs(norm3(eR - eL) - norm3(gR - gL));
    const Q4 d = qmul(qL, qconj(qR));
    m.angle = 2.0 * atan2(norm3(V3{d.x, d.y, d.z}), fabs(d.w));
    return m;
}

// the achieved tilt is passed on only where it is finite.  (stack_step_kernel states this test and the log row below in
// its own text: taken from here they change its instructions)
__device__ __forceinline__ bool tilt_held(const TrayMeasure& m) { return !(isfinite(m.tilt[0]) && isfinite(m.tilt[1])); }

// one step of the stack metrics (stack_step.h): s [STACK_NMETRIC] in/out, the experiment's row in memory, read whole
// before it is written (one lane per experiment); u the command, tp the commanded tray position [3]
__device__ __forceinline__ void stack_metrics_step(double* s, const TrayMeasure& m, const double* u, const double* tp) {
    const bool held = tilt_held(m);
    const double last = s[0], dmax = s[1], yaw = s[2], gap = s[3], ang = s[4], perr = s[5], nheld = s[6], n = s[7];
    const double d0 = fabs(m.tilt[0] - u[0]), d1 = fabs(m.tilt[1] - u[1]);
    const double dev = d0 > d1 ? d0 : d1;
    const double ay = fabs(m.yaw);
    const double pe = norm3(m.p - ld3(tp));
    s[0] = held ? last : dev;
    s[1] = (!held && dev > dmax) ? dev : dmax;
    s[2] = ay > yaw ? ay : yaw;
    s[3] = m.gap > gap ? m.gap : gap;
    s[4] = m.angle > ang ? m.angle : ang;
    s[5] = pe > perr ? pe : perr;
    s[6] = held ? nheld + 1.0 : nheld;
    s[7] = n + 1.0;
}

// the stack log group's row of a step: the achieved tilt as measured and the achieved pose
__device__ __forceinline__ void stack_log_row(double* log_tilt, double* log_tray, size_t row, const TrayMeasure& m) {
    log_tilt[2 * row] = m.tilt[0]; log_tilt[2 * row + 1] = m.tilt[1];
    double* t = log_tray + 7 * row;
    st3(t, m.p);
    t[3] = m.q.w; t[4] = m.q.x; t[5] = m.q.y; t[6] = m.q.z;
}

}  // namespace dartmpc
