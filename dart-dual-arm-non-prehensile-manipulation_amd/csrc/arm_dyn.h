// arm_dyn.h -- rigid-body dynamics of a serial hinge chain on one wave64: launch arguments of arm_dyn.hip and the
// device functions its two kernels share (world kinematics, joint-space inertia M, bias forces h, Cholesky solve).
//
// Model row (fp64, arm_model_len(n) = 22 n + 18):
//   base_pos[3] base_quat[4]                 world pose of the frame the first link hangs in
//   per link: pos[3] quat[4] axis[3] armature damping mass com[3] inertia[6] (xx yy zz xy xz yz, about the com, body frame)
//   ee_pos[3] ee_quat[4] offset gravity[3]   EE body frame in the last link's frame; offset along its z
// Quaternions are (w, x, y, z) and unit, axes unit (dart_mpc/arm_model.py normalises both).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arm_qp.h"
#include "wave.h"

namespace dartmpc {

constexpr int ARM_LINK_LEN = 22;
constexpr int ARM_NMETRIC = 6;
constexpr int ARM_JACDOT_REFERENCE = 0, ARM_JACDOT_BODY = 1;
__host__ __device__ constexpr int arm_model_len(int n) { return ARM_LINK_LEN * n + 18; }
__host__ __device__ constexpr int arm_state_len(int n) { return 3 * n + 7; }

// state -> snapshot.  Instance b reads q / qd / qdd_prev at q_stride b and its model row at
// model_stride (model_mod ? b % model_mod : b); its mocap target is mocap + mocap_stride b (pos[3] quat[4]) or, with
// tray set, the dual-arm coordinator's: tray pose b / 2 composed with grasp transform b % 2.
struct ArmDynArgs {
    int B, n, jacdot_point;
    int model_stride, model_mod, q_stride, mocap_stride;
    const double* model;
    const double *q, *qd, *qp;
    const double* mocap;
    const double* tray;          // [B / 2][7] or null
    const double* grasp;         // [2][7]
    double* snap;                // [B][arm_snap_len(n)]
    double* ee_quat;             // [B][4] or null
    double* mocap_out;           // [B][7] or null: the targets the snapshot was taken against
};

// one plant step behind the QP: (M_p + dt diag d) a = tau - h_p - d o qd, qd += dt a, q += dt qd; logs and metrics
struct ArmPlantArgs {
    int B, n;
    int model_stride, model_mod, prm_stride;
    const double* model;         // the plant's model rows
    const double* prm;           // the QP's parameter rows (dt, taumax)
    const double* snap;          // [B][arm_snap_len(n)] of this step (ee_pos, mocap_pos, rotvec)
    const double *qdd, *tau, *loss;
    const int32_t *status, *iters;
    double *q, *qd, *qp;         // [B][n] in / out (qp: the next qdd_prev = the QP's solution)
    double* metrics;             // [B][ARM_NMETRIC] in / out
    double *q_log, *qd_log, *tau_log, *ee_log, *loss_log;   // this step's rows ([B][.]) or all null
    int32_t* status_log;
};

// ---- 3-vectors and quaternions in registers -------------------------------------------------------------------
struct V3 { double x, y, z; };
struct Q4 { double w, x, y, z; };
__device__ __forceinline__ V3 ld3(const double* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ Q4 ld4(const double* p) { return Q4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void st3(double* p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ Q4 qmul(Q4 a, Q4 b) {
    return Q4{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
              a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
__device__ __forceinline__ Q4 qunit(Q4 a) {
    const double s = 1.0 / sqrt(a.w * a.w + a.x * a.x + a.y * a.y + a.z * a.z);
    return Q4{s * a.w, s * a.x, s * a.y, s * a.z};
}
// v rotated by the unit quaternion a: v + 2 w (u x v) + 2 u x (u x v)
__device__ __forceinline__ V3 qrot(Q4 a, V3 v) {
    const V3 u{a.x, a.y, a.z};
    const V3 t = cross(u, v);
    return v + 2.0 * (a.w * t + cross(u, t));
}
// symmetric 3 x 3 (xx yy zz xy xz yz) times a vector
__device__ __forceinline__ V3 symv(const double* I, V3 v) {
    return V3{fma(I[0], v.x, fma(I[3], v.y, I[4] * v.z)), fma(I[3], v.x, fma(I[1], v.y, I[5] * v.z)),
              fma(I[4], v.x, fma(I[5], v.y, I[2] * v.z))};
}

// ---- world kinematics, M and h of one arm, in LDS ----------------------------------------------------------------
struct ArmKin {
    double ql[ARM_NMAX][4];                      // quat_i (x) Rot(axis_i, q_i)
    double p[ARM_NMAX][3], z[ARM_NMAX][3];       // link origins (= joint anchors) and joint axes
    double pc[ARM_NMAX][3], Iw[ARM_NMAX][6], m[ARM_NMAX];
    double w[ARM_NMAX][3], v[ARM_NMAX][3];       // angular velocity of link i, velocity of its origin
    double F[ARM_NMAX][3], N[ARM_NMAX][3];       // Newton-Euler at qdd = 0: force, moment about the com
    double mc[ARM_NMAX], cc[ARM_NMAX][3], Ic[ARM_NMAX][6];   // composite of links i .. n - 1 about its own com
    double pe[3], Qe[4], we[3], ve[3];           // EE body frame: origin, orientation, angular / linear velocity
    double M[ARM_NMAX * ARM_NMAX], h[ARM_NMAX];  // M row-major with stride n
};

// Every lane of the (one-wave) workgroup calls this at uniform control flow; mdl, q, qd are in LDS.
//   forward kinematics   X_i = X_parent (pos_i, quat_i) Rot(axis_i, q_i): lane i forms the local quaternion, the chain is
//                        composed by every lane alike (uniform LDS reads), lane i keeps frame i
//   velocities, Newton-Euler at qdd = 0 with the base accelerated by -gravity: the same way
//   h_i  = sum_{k >= i} z_i . (N_k + (pc_k - p_i) x F_k)            lane i
//   M_ij = z_j . (Ic_c z_i) + mc_c (z_j x (cc_c - p_j)) . (z_i x (cc_c - p_i)), c = max(i, j): composite rigid
//          bodies, lane (i, j >= i... mirrored): both triangles are written from one value; armature on the diagonal
template <int n>
__device__ __forceinline__ void arm_kin_M_h(ArmKin& K, const double* mdl, const double* q, const double* qd, int l) {
    const double* lk = mdl + 7;
    if (l < n) {
        const double* a = lk + ARM_LINK_LEN * l;
        double s, c;
        sincos(0.5 * q[l], &s, &c);
        const Q4 r = qmul(ld4(a + 3), Q4{c, s * a[7], s * a[8], s * a[9]});
        K.ql[l][0] = r.w; K.ql[l][1] = r.x; K.ql[l][2] = r.y; K.ql[l][3] = r.z;
    }
    __syncthreads();
    Q4 Q = ld4(mdl + 3), Qi = Q;
    V3 P = ld3(mdl), Pi = P;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        P = P + qrot(Q, ld3(lk + ARM_LINK_LEN * i));
        Q = qmul(Q, ld4(K.ql[i]));
        if (i == l) { Qi = Q; Pi = P; }
    }
    if (l < n) {
        const double* a = lk + ARM_LINK_LEN * l;
        // rotation matrix of the link: columns R e_x, R e_y, R e_z
        const V3 cx = qrot(Qi, V3{1.0, 0.0, 0.0}), cy = qrot(Qi, V3{0.0, 1.0, 0.0}), cz = qrot(Qi, V3{0.0, 0.0, 1.0});
        auto R = [&](V3 b) { return b.x * cx + (b.y * cy + b.z * cz); };
        st3(K.p[l], Pi);
        st3(K.z[l], R(ld3(a + 7)));
        st3(K.pc[l], Pi + R(ld3(a + 13)));
        K.m[l] = a[12];
        // Iw = R Ib R': T = R Ib by columns (Ib symmetric), then the six entries of T R'
        const double* Ib = a + 16;
        const V3 t0 = R(V3{Ib[0], Ib[3], Ib[4]}), t1 = R(V3{Ib[3], Ib[1], Ib[5]}), t2 = R(V3{Ib[4], Ib[5], Ib[2]});
        // (T R')_{ab} = t0_a cx_b + t1_a cy_b + t2_a cz_b
        K.Iw[l][0] = fma(t0.x, cx.x, fma(t1.x, cy.x, t2.x * cz.x));
        K.Iw[l][1] = fma(t0.y, cx.y, fma(t1.y, cy.y, t2.y * cz.y));
        K.Iw[l][2] = fma(t0.z, cx.z, fma(t1.z, cy.z, t2.z * cz.z));
        K.Iw[l][3] = fma(t0.x, cx.y, fma(t1.x, cy.y, t2.x * cz.y));
        K.Iw[l][4] = fma(t0.x, cx.z, fma(t1.x, cy.z, t2.x * cz.z));
        K.Iw[l][5] = fma(t0.y, cx.z, fma(t1.y, cy.z, t2.y * cz.z));
    }
    if (l == 0) {
        const double* e = lk + ARM_LINK_LEN * n;
        st3(K.pe, P + qrot(Q, ld3(e)));
        const Q4 r = qmul(Q, ld4(e + 3));
        K.Qe[0] = r.w; K.Qe[1] = r.x; K.Qe[2] = r.y; K.Qe[3] = r.z;
    }
    __syncthreads();
    {
        const V3 g = ld3(lk + ARM_LINK_LEN * n + 8);
        V3 w{0.0, 0.0, 0.0}, v = w, al = w, ac = -1.0 * g, pp = ld3(K.p[0]);
        V3 wi = w, vi = w, ali = w, aci = ac;
#pragma unroll
        for (int i = 0; i < n; ++i) {
            const V3 pi = ld3(K.p[i]), r = pi - pp, zq = qd[i] * ld3(K.z[i]);
            const V3 wr = cross(w, r);
            v = v + wr;
            ac = ac + (cross(al, r) + cross(w, wr));
            al = al + cross(w, zq);
            w = w + zq;
            pp = pi;
            if (i == l) { wi = w; vi = v; ali = al; aci = ac; }
        }
        if (l < n) {
            const V3 c = ld3(K.pc[l]) - ld3(K.p[l]);
            const V3 acom = aci + (cross(ali, c) + cross(wi, cross(wi, c)));
            st3(K.w[l], wi);
            st3(K.v[l], vi);
            st3(K.F[l], K.m[l] * acom);
            st3(K.N[l], symv(K.Iw[l], ali) + cross(wi, symv(K.Iw[l], wi)));
        }
        if (l == 0) {
            st3(K.we, w);
            st3(K.ve, v + cross(w, ld3(K.pe) - pp));
        }
    }
    __syncthreads();
    if (l < n) {
        const V3 zi = ld3(K.z[l]), pi = ld3(K.p[l]);
        double hs = 0.0, mc = 0.0;
        V3 mp{0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < n; ++k) {
            if (k >= l) {
                const V3 pck = ld3(K.pc[k]);
                hs += dot(zi, ld3(K.N[k]) + cross(pck - pi, ld3(K.F[k])));
                mc += K.m[k];
                mp = mp + K.m[k] * pck;
            }
        }
        K.h[l] = hs;
        const V3 cc = (1.0 / mc) * mp;
        double Ic[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < n; ++k) {
            if (k >= l) {
                const V3 d = ld3(K.pc[k]) - cc;
                const double mk = K.m[k];
                Ic[0] += K.Iw[k][0] + mk * (d.y * d.y + d.z * d.z);
                Ic[1] += K.Iw[k][1] + mk * (d.x * d.x + d.z * d.z);
                Ic[2] += K.Iw[k][2] + mk * (d.x * d.x + d.y * d.y);
                Ic[3] += K.Iw[k][3] - mk * (d.x * d.y);
                Ic[4] += K.Iw[k][4] - mk * (d.x * d.z);
                Ic[5] += K.Iw[k][5] - mk * (d.y * d.z);
            }
        }
        K.mc[l] = mc;
        st3(K.cc[l], cc);
#pragma unroll
        for (int e = 0; e < 6; ++e) K.Ic[l][e] = Ic[e];
    }
    __syncthreads();
    {
        const int i = l >> 3, j = l & 7;
        if (i < n && j <= i) {
            const V3 zi = ld3(K.z[i]), zj = ld3(K.z[j]), cc = ld3(K.cc[i]);
            const V3 ai = cross(zi, cc - ld3(K.p[i])), aj = cross(zj, cc - ld3(K.p[j]));
            double mij = dot(zj, symv(K.Ic[i], zi)) + K.mc[i] * dot(aj, ai);
            if (i == j) mij += lk[ARM_LINK_LEN * i + 10];
            K.M[i * n + j] = mij;
            K.M[j * n + i] = mij;
        }
    }
    __syncthreads();
}

// ---- Cholesky A = L L' of an n x n SPD matrix (row-major, stride lda, in LDS) in the registers of every lane alike;
// false on a pivot that is not positive (a NaN included) ---------------------------------------------------------
template <int n>
__device__ __forceinline__ bool chol_factor(const double* A, int lda, double (&L)[n * (n + 1) / 2], double (&iD)[n]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < n; ++j) {
#pragma unroll
        for (int i = j; i < n; ++i) {
            double s = A[i * lda + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-L[i * (i + 1) / 2 + k], L[j * (j + 1) / 2 + k], s);
            if (i == j) {
                ok = ok && s > 0.0;
                const double d = sqrt(s);
                L[j * (j + 1) / 2 + j] = d;
                iD[j] = 1.0 / d;
            } else {
                L[i * (i + 1) / 2 + j] = s * iD[j];
            }
        }
    }
    return ok;
}
// y = L^-1 b, in place
template <int n>
__device__ __forceinline__ void chol_forward(const double (&L)[n * (n + 1) / 2], const double (&iD)[n], double (&b)[n]) {
#pragma unroll
    for (int i = 0; i < n; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = fma(-L[i * (i + 1) / 2 + k], b[k], s);
        b[i] = s * iD[i];
    }
}
// x = L'^-1 y, in place
template <int n>
__device__ __forceinline__ void chol_backward(const double (&L)[n * (n + 1) / 2], const double (&iD)[n], double (&b)[n]) {
#pragma unroll
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int k = i + 1; k < n; ++k) s = fma(-L[k * (k + 1) / 2 + i], b[k], s);
        b[i] = s * iD[i];
    }
}

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_arm_dyn(const dartmpc::ArmDynArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_arm_plant(const dartmpc::ArmPlantArgs* args, hipStream_t stream);
