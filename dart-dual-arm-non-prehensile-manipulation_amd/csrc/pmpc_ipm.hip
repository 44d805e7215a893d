// pmpc_ipm.hip -- batched PMPC interior-point solve for gfx950 (MI355X / CDNA4).
//
// Replaces the per-timestep `ca.nlpsol('solver','ipopt',...)` call of
// PMPC.solve (PMPC/src/controller/mpc_3d.py:115-138) for a whole batch of
// independent tray-tilt NMPC instances.
//
// Structure exploited: the Newton system of the reference NLP
// (mpc_3d.py:28-85) splits into two independent scalar-input optimal-control
// problems -- the x axis (px, vx; theta_x) and the y axis (py, vy; theta_y) --
// plus the cost-free z sub-state (pz, vz).  Each axis is linear in its state
// with input sin(theta):  x+ = Phi x + Gamma sin(theta), Phi/Gamma being exactly
// the RK4 map of mpc_3d.py:99-104 applied to :91-92.  z is affine in its state
// and in vz_new = -g (theta_x^2 + theta_y^2) (:93-97): it carries no cost, so
// its multipliers stay 0 and it never enters the (x, y) Riccati solve, but its
// defect rows (:37, :48) are part of IPOPT's constraint violation.  The kernel
// therefore runs IPOPT's primal-dual barrier method on the FULL 6-state NLP:
// one mu, one step length, one filter; theta, the primal infeasibility, the
// tiny-step test and the second-order correction see the z rows, and z moves
// with its own Newton step (an affine scan driven by the tilt steps).
//
// Mapping: one wave64 per instance, lane k <-> shooting node k (0..N, N <= 63).
// Everything per node lives in VGPRs.  Stage-coupled recursions (Riccati
// backward sweep, forward state sweep, z sweep) are DPP scans or hand 2x2
// blocks to the neighbouring lane with DPP wave shifts (no LDS); norms and
// inner products are DPP row reductions.  No LDS and no global traffic inside
// the iteration loop.
// Horizons N = 32..63: this file built a third time with -DDART_WG=2 (Makefile: pmpc_wg2.o) -- the scan build
// (NAX = 1) on a workgroup of two waves per instance, wave w owning nodes 32 w .. 32 w + 31 with the one-wave lane
// roles (wave.h: the wave reductions and node shifts combine the two waves).  Every scan runs in both waves and is
// continued across the wave boundary by one LDS hand-over (pm_pass): the suffix scans of wave 0 start from the
// values of node 32 (wave 1), the prefix scans of wave 1 from those of node 31 (wave 0).  IPOPT's soft restoration
// phase runs in the kernel as in the sequential N > 31 build.  The build's symbols sit in their own namespace.
#if DART_WG == 2
#define dartmpc dartmpc_wg2
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <utility>

#include "launch_plan.h"
#include "pmpc_ipm.h"
#include "pmpc_model.h"
#include "pmpc_resto.h"
#include "stamps.h"
#include "wave.h"

namespace dartmpc {

// This file is compiled twice (Makefile): as is, it holds the scan instantiations for N > 15, the
// launcher and the self-test; with -DPMPC_SEQ, the one-row instantiation (N <= 15) and the
// sequential (throughput) ones behind dartmpc_launch_pmpc_seq, so that each set gets the
// optimisation level that is fastest for it.
#ifdef DART_STAMPS
#ifndef PMPC_SEQ
__device__ unsigned long long g_stamp[32];
#define STAMP_FLUSH(b) STAMP_FLUSH32_TO(g_stamp, b)
#else
__device__ unsigned long long g_stamp_seq[32];
#define STAMP_FLUSH(b) STAMP_FLUSH32_TO(g_stamp_seq, b)
#endif
#else
#define STAMP_FLUSH(b) STAMP_FLUSH_TO(g_stamp, b)
#endif

// values of node `src_node` of wave `src_wave` (lane src_node: axis x, lane src_node + 32: axis y) in every lane of
// the same axis half of both waves.  One barrier: every call site SITE has its own slots, and between two passes
// of one site both waves cross other barriers (the reductions and shifts of an iteration), each after its reads
// of the slot have completed (__syncthreads waits for the wave's LDS accesses), so no pass overwrites a slot that
// is still to be read.  Two-wave build only (the one-wave build names it in discarded branches).
#if DART_WG == 2
__shared__ double g_pm_x[4][2][4];
#endif
template <int SITE, int NV>
__device__ __forceinline__ void pm_pass(int src_wave, int src_node, const double (&v)[NV], double (&o)[NV]) {
    static_assert(NV <= 4 && SITE < 4, "four slots, four sites");
#if DART_WG == 1
    (void)src_wave; (void)src_node;
#pragma unroll
    for (int i = 0; i < NV; ++i) o[i] = v[i];
#else
    const int l = lane_id();
    if (wave_idx() == src_wave && (l & 31) == src_node) {
#pragma unroll
        for (int i = 0; i < NV; ++i) g_pm_x[SITE][l >> 5][i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) o[i] = g_pm_x[SITE][l >> 5][i];
#endif
}

// DPP move with an identity fill (FILL = 0.0 or 1.0) for lanes whose source is outside the row or
// masked out.  With every row enabled a zero half comes from bound_ctrl (the DPP writes 0 where the
// source is out of range): no initialising move; 1.0 only needs its high word 0x3ff00000 set first.
// Rows masked off keep the old value, so a partial ROWMASK initialises both words.
template <int CTRL, int ROWMASK, int FILL>
__device__ __forceinline__ double dpp_fill(double x) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const int blo = (int)(unsigned)(b & 0xffffffffu), bhi = (int)(unsigned)(b >> 32);
    constexpr int fhi = FILL ? 0x3ff00000 : 0;
    int rlo, rhi;
    if constexpr (ROWMASK == 0xf) {
        rlo = __builtin_amdgcn_mov_dpp(blo, CTRL, 0xf, 0xf, true);
        if constexpr (FILL) rhi = __builtin_amdgcn_update_dpp(fhi, bhi, CTRL, 0xf, 0xf, false);
        else rhi = __builtin_amdgcn_mov_dpp(bhi, CTRL, 0xf, 0xf, true);
    } else {
        rlo = __builtin_amdgcn_update_dpp(0, blo, CTRL, ROWMASK, 0xf, false);
        rhi = __builtin_amdgcn_update_dpp(fhi, bhi, CTRL, ROWMASK, 0xf, false);
    }
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)rhi << 32) | (unsigned)rlo);
}
// one Hillis-Steele level of an inclusive scan of 2-D affine maps x -> F x + c (later o earlier):
// (F, c) <- (F, c) o (P, q) = (F P, F q + c), (P, q) fetched by DPP, identity where out of range
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void affine_scan_level(double& f11, double& f12, double& f21, double& f22, double& c1,
                                                  double& c2) {
    const double p11 = dpp_fill<CTRL, ROWMASK, 1>(f11), p12 = dpp_fill<CTRL, ROWMASK, 0>(f12);
    const double p21 = dpp_fill<CTRL, ROWMASK, 0>(f21), p22 = dpp_fill<CTRL, ROWMASK, 1>(f22);
    const double q1 = dpp_fill<CTRL, ROWMASK, 0>(c1), q2 = dpp_fill<CTRL, ROWMASK, 0>(c2);
    const double n11 = fma(f11, p11, f12 * p21), n12 = fma(f11, p12, f12 * p22);
    const double n21 = fma(f21, p11, f22 * p21), n22 = fma(f21, p12, f22 * p22);
    c1 = fma(f11, q1, fma(f12, q2, c1));
    c2 = fma(f21, q1, fma(f22, q2, c2));
    f11 = n11; f12 = n12; f21 = n21; f22 = n22;
}

// A composition level whose source lanes already hold pure constants (their map is 0 because
// their window reaches node 0 of an inclusive prefix scan): only the constant is fetched, c <- F q + c
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void affine_scan_const(double f11, double f12, double f21, double f22, double& c1,
                                                  double& c2) {
    const double q1 = dpp_fill<CTRL, ROWMASK, 0>(c1), q2 = dpp_fill<CTRL, ROWMASK, 0>(c2);
    c1 = fma(f11, q1, fma(f12, q2, c1));
    c2 = fma(f21, q1, fma(f22, q2, c2));
}
// the same two levels for scalar affine maps z -> m z + c (the z sub-state's Newton sweep)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void affine1_scan_level(double& m, double& c) {
    const double pm = dpp_fill<CTRL, ROWMASK, 1>(m), pc = dpp_fill<CTRL, ROWMASK, 0>(c);
    c = fma(m, pc, c);
    m = m * pm;
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void affine1_scan_const(double m, double& c) {
    c = fma(m, dpp_fill<CTRL, ROWMASK, 0>(c), c);
}

// One level of a suffix scan of 4x4 matrices (T <- T * F, F fetched from lane k + d by DPP
// row_shl:d, identity where out of range)
template <int CTRL, bool FIRST = false>
__device__ __forceinline__ void mat4_scan_level(double* T) {
    // FIRST: T is a lane's own stage map, whose column 0 is (1, 0, X11, 0), and so is that of the
    // neighbour's map or of the identity fill: those entries are not fetched and their products
    // with 0 / 1 are dropped (the compiler keeps 0 * x for NaN semantics)
    constexpr bool fz[16] = {FIRST, false, false, false, FIRST, false, false, false,
                             false, false, false, false, FIRST, false, false, false};
    double F[16];
#pragma unroll
    for (int e = 0; e < 16; ++e)
        F[e] = fz[e] ? (e == 0 ? 1.0 : 0.0)
                     : (e % 5 == 0) ? dpp_fill<CTRL, 0xf, 1>(T[e]) : dpp_fill<CTRL, 0xf, 0>(T[e]);
    double N[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double acc = T[4 * i + 3] * F[12 + j];
            if (fz[12 + j]) acc = 0.0;
            acc = fma(T[4 * i + 2], F[8 + j], acc);
            if (!fz[4 + j]) acc = fma(T[4 * i + 1], F[4 + j], acc);
            if (FIRST && i == 0) acc += F[j];                                  // T[0] = 1
            else if (!(FIRST && (i == 1 || i == 3))) acc = fma(T[4 * i], F[j], acc);   // T[4] = T[12] = 0
            N[4 * i + j] = acc;
        }
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = N[e];
}

// ---------------------------------------------------------------------------
// the kernel: one wave64 = one instance.
//   NAX = 1 (N <= 31): lane = axis*32 + k, one axis per lane (x in lanes 0-31, y in 32-63)
//   NAX = 2 (N <= 63): lane = k, both axes in every lane
// ---------------------------------------------------------------------------
//   QSCAN: compile the quadratic-Riccati scan (latency regime); without it the kernel fits 2 waves
//   per SIMD (throughput regime)
//   ONEROW: N <= 15, every axis fits one 16-lane DPP row and the scans need no cross-row step (the
//   DART driver's default horizon is 15, main_parallel_enhanced.py:171-196)
//   SHORT2: N <= 23, the suffix of node 16 spans at most 8 lanes, so the quadratic scan stops
//   after 3 in-row levels and finishes rows 0 / 2 with two 4 x 2 compositions (no 4th 4 x 4 level)
//   (16 <= N <= 23 at one wave per SIMD; its two-wave instantiation, OCC2, also serves large N <= 15 batches)
//   Occupancy: the sequential NAX == 1 build is the throughput variant and must fit two waves per
//   SIMD (<= 256 registers); the ILP-oriented scheduler of this file (Makefile) would otherwise spend
//   the whole register file on one wave
//   RED: the reduced (x, y) path (opt-in, dart_mpc_config.pmpc_path = 1): theta, the filter and the
//   error measures leave the z rows out and there is no second-order correction, z is rolled out from
//   the final controls.  Same KKT point, fewer iterations, but not IPOPT's iterates.
// the solve of instance b by the calling wave (the body of pmpc_ipm_kernel and of the resident
// server pmpc_serve_kernel); true when the instance was handed over to IPOPT's restoration phases
// (status kPmNeedResto, no other output)
// branch-layout hints for the cold paths of the loop (inertia retries, the sequential fallback of the
// scan, the least-square iteration, second-order corrections, failures): C2 +2.1 % (A/B); the one-row
// build (N <= 15) measured 1 % slower with them and goes without
#define PM_EXPECT(x, v) (ONEROW ? (bool)(x) : (bool)__builtin_expect((long)(bool)(x), (v)))

// a double that holds the same value in every lane, as a scalar (two v_readfirstlane)
__device__ __forceinline__ double wave_uniform(double x) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b & 0xffffffffu));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// The per-lane stage constants of the Riccati factorisation (pmpc_solve derives them at its start).
struct PmStage {
    double f11, a12k, a22k, ai12k, ai22k, a22i, uonf, A11k, A12k, A22k;
};

// One attempt of the Riccati factorisation at the inertia perturbation delta: from the stage quantities of the
// current point (be, E, Rt0) the value function P, the gains W, 1 / Quu (iQs) of every node; returns ok (every
// Quu > 0 and finite), use_scan tells which recursion ran.  One function for the iteration loop of pmpc_solve
// (every attempt of the one-wave builds; the retries and the sequential fallback of the overlapped build) and
// for the factor wave of the overlapped build (attempt 0, delta = 0), so both run the same arithmetic.
template <int NAX, bool QSCAN, bool ONEROW, bool SHORT2>
__device__ __forceinline__ bool pmpc_riccati(const int lane, const int N, const bool uon, const bool lsm,
                                             const double delta, const double qp2, const double qv2,
                                             const PmStage& c, const double (&be1)[NAX], const double (&be2)[NAX],
                                             const double (&E11)[NAX], const double (&E12)[NAX],
                                             const double (&E22)[NAX], const double (&Rt0)[NAX], double (&P11)[NAX],
                                             double (&P12)[NAX], double (&P22)[NAX], double (&W1)[NAX],
                                             double (&W2)[NAX], double (&iQs)[NAX], bool& use_scan) {
    constexpr bool one_row = ONEROW;
    constexpr bool short2 = SHORT2 && !ONEROW;
    const double f11 = c.f11, a12k = c.a12k, a22k = c.a22k, ai12k = c.ai12k, ai22k = c.ai22k, a22i = c.a22i;
    const double uonf = c.uonf, A11k = c.A11k, A12k = c.A12k, A22k = c.A22k;
    (void)lane; (void)ai12k; (void)ai22k; (void)a22i; (void)uonf;
    const double X11d = lsm ? 1.0 : qp2 + delta, X22d = lsm ? 1.0 : qv2 + delta;
    double Quu[NAX], Rt[NAX];
#pragma unroll
    for (int j = 0; j < NAX; ++j) {      // terminal value function in every lane
        P11[j] = X11d; P12[j] = 0.0; P22[j] = X22d;
        Rt[j] = (lsm ? 1.0 : Rt0[j]) + delta;
    }
    // Quadratic part as a scan: with P = Y U^-1 the stage map P_k = X + A^T (P_{k+1}^-1 + G_k)^-1 A
    // (G_k = B_k B_k^T / R_k) is linear on [U; Y]: [U; Y]_k = S_k [U; Y]_{k+1},
    // S_k = [[A^-1, A^-1 G], [X A^-1, X A^-1 G + A^T]], so [U; Y]_k = S_k ... S_{N-1} [I; X]
    // is a suffix product (5 DPP levels).  Exact in the reals; in fp64 it matches the
    // sequential sweep to ~1e-15 while every stage is mildly stiff (B_k B_k^T X / R_k <= 2
    // per axis, checked here); otherwise, and for NAX == 2, the sequential sweep runs.
    use_scan = false;
    if constexpr (NAX == 1 && QSCAN) {
        const double ratio = fmax(E11[0] * X11d, E22[0] * X22d);
        use_scan = !wany(uon && !(Rt[0] > 0.0 && ratio <= 2.0 * Rt[0]));
    }
    if (PM_EXPECT(use_scan, 1)) {
        const double iR = uon ? frcp(Rt[0]) : 0.0;
        const double G11 = be1[0] * be1[0] * iR, G12 = be1[0] * be2[0] * iR, G22 = be2[0] * be2[0] * iR;
        const double g11 = G11 + ai12k * G12, g12 = G12 + ai12k * G22, g21 = ai22k * G12, g22 = ai22k * G22;
        // idle / terminal lanes: A^-1 = I, G = 0 (iR = 0), X = 0, A^T = I give T = I without a select
        const double X11k = X11d * uonf, X22k = X22d * uonf;
        double T[16] = {1.0, ai12k, g11, g12,
                        0.0, ai22k, g21, g22,
                        X11k, X11k * ai12k, fma(X11k, g11, 1.0), X11k * g12,
                        0.0, X22k * ai22k, fma(X22k, g21, a12k), fma(X22k, g22, a22i)};
        mat4_scan_level<0x101, true>(T);
        mat4_scan_level<0x102>(T);
        mat4_scan_level<0x104>(T);
        if constexpr (!short2 && !one_row) mat4_scan_level<0x108>(T);
        // [U; Y] = T [I; X] of the row-local suffix
        double W[8] = {fma(T[2], X11d, T[0]), fma(T[3], X22d, T[1]), fma(T[6], X11d, T[4]),
                       fma(T[7], X22d, T[5]), fma(T[10], X11d, T[8]), fma(T[11], X22d, T[9]),
                       fma(T[14], X11d, T[12]), fma(T[15], X22d, T[13])};
        if constexpr (short2 || one_row) {
            // after 3 levels lane k holds S_k ... S_{min(k+7, row end)}: lanes 16-23 (48-55)
            // already reach the terminal (N <= 23), lanes 8-15 the row end (and the terminal
            // when N <= 15).  Lanes 8-15 compose with the 4 x 2 of lane 16 (ds_swizzle; not
            // for N <= 15), then lanes 0-7 with that of lane k + 8 (DPP).  Lanes past the
            // terminal hold [I; X], so a suffix that is already complete stays unchanged.
            double F[8];
            if constexpr (short2) {
#pragma unroll
            for (int e = 0; e < 8; ++e) F[e] = half_bcast_c<16>(W[e]);
            if ((lane & 16) == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        W[2 * i + jj] = fma(T[4 * i], F[jj], fma(T[4 * i + 1], F[2 + jj],
                                            fma(T[4 * i + 2], F[4 + jj], T[4 * i + 3] * F[6 + jj])));
            }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) F[e] = dpp_fill<0x108, 0xf, 0>(W[e]);
            if ((lane & 24) == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        W[2 * i + jj] = fma(T[4 * i], F[jj], fma(T[4 * i + 1], F[2 + jj],
                                            fma(T[4 * i + 2], F[4 + jj], T[4 * i + 3] * F[6 + jj])));
            }
        } else if constexpr (!one_row && kWaves == 1) {
            // rows 0 and 2 of each half: [U; Y]_k = T_k(row) [U; Y]_16, the 4 x 2 of lane 16 (48)
            // fetched by ds_swizzle (bitmask mode, or_mask 16: no address, no LDS access)
            double F[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) F[e] = half_bcast_c<16>(W[e]);
            if ((lane & 16) == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        W[2 * i + jj] = fma(T[4 * i], F[jj], fma(T[4 * i + 1], F[2 + jj],
                                            fma(T[4 * i + 2], F[4 + jj], T[4 * i + 3] * F[6 + jj])));
            }
        }
        double pnx[3] = {0.0, 0.0, 0.0};      // two waves: P_32 (wave 1's node 32) in wave 0
        if constexpr (kWaves == 2) {
            // two waves (N >= 32, rows as above): wave 1's suffixes reach the terminal; wave 0's continue
            // from the value function of node 32, [U; Y]_k = T_k(..31) [I; P_32] (exact in the reals, as the
            // scan itself)
            auto rows = [&]() {
                double F[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) F[e] = half_bcast_c<16>(W[e]);
                if ((lane & 16) == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj)
                            W[2 * i + jj] = fma(T[4 * i], F[jj], fma(T[4 * i + 1], F[2 + jj],
                                                fma(T[4 * i + 2], F[4 + jj], T[4 * i + 3] * F[6 + jj])));
                }
            };
            double v[3] = {0.0, 0.0, 0.0}, pn[3];
            if (wave_idx() == 1) {
                rows();
                const double idet = frcp(fma(W[0], W[3], -W[1] * W[2]));
                v[0] = fma(W[4], W[3], -W[5] * W[2]) * idet;
                v[1] = 0.5 * (fma(W[5], W[0], -W[4] * W[1]) * idet + fma(W[6], W[3], -W[7] * W[2]) * idet);
                v[2] = fma(W[7], W[0], -W[6] * W[1]) * idet;
            }
            pm_pass<0>(1, 0, v, pn);
            pnx[0] = pn[0]; pnx[1] = pn[1]; pnx[2] = pn[2];
            if (wave_idx() == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    W[2 * i] = fma(T[4 * i + 3], pn[1], fma(T[4 * i + 2], pn[0], T[4 * i]));
                    W[2 * i + 1] = fma(T[4 * i + 3], pn[2], fma(T[4 * i + 2], pn[1], T[4 * i + 1]));
                }
                rows();
            }
        }
        // P = Y U^-1 (symmetrised)
        const double U11 = W[0], U12 = W[1], U21 = W[2], U22 = W[3];
        const double Y11 = W[4], Y12 = W[5], Y21 = W[6], Y22 = W[7];
        const double idet = frcp(fma(U11, U22, -U12 * U21));
        const double q11 = fma(Y11, U22, -Y12 * U21) * idet, q12 = fma(Y12, U11, -Y11 * U12) * idet;
        const double q21 = fma(Y21, U22, -Y22 * U21) * idet, q22 = fma(Y22, U11, -Y21 * U12) * idet;
        P11[0] = q11; P12[0] = 0.5 * (q12 + q21); P22[0] = q22;
        // the stage quantities of node k from P_{k+1}
        double n11, n12, n22;
        if constexpr (kWaves == 1) {
            n11 = from_next(P11[0]); n12 = from_next(P12[0]); n22 = from_next(P22[0]);
        } else {
            // two waves: node 32's value function is already in wave 0 (pnx), no exchange
            n11 = dpp<kWaveShl1>(P11[0]); n12 = dpp<kWaveShl1>(P12[0]); n22 = dpp<kWaveShl1>(P22[0]);
            if (wave_idx() == 0 && (lane & 31) == 31) { n11 = pnx[0]; n12 = pnx[1]; n22 = pnx[2]; }
        }
        const double e1 = be1[0], e2 = be2[0];
        const double Q = fma(E11[0], n11, fma(E12[0], n12, fma(E22[0], n22, Rt[0])));
        const double PB1 = fma(n11, e1, n12 * e2), PB2 = fma(n12, e1, n22 * e2);
        const double U1 = PB1, U2 = fma(PB1, a12k, PB2 * a22k);
        const double iQ = frcp(Q);
        W1[0] = iQ * U1; W2[0] = iQ * U2;
        Quu[0] = Q; iQs[0] = iQ;
    } else
    // backward sweep: every lane maps its neighbour's value function through its own
    // stage; after step j lane N-1-j is final.  Terminal/idle lanes have Phi = 0, B = 0.
    for (int step = 0; step < N; ++step) {
        double n11[NAX], n12[NAX], n22[NAX];
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            n11[j] = from_next(P11[j]); n12[j] = from_next(P12[j]); n22[j] = from_next(P22[j]);
        }
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            const double e1 = be1[j], e2 = be2[j];
            const double Q = fma(E11[j], n11[j], fma(E12[j], n12[j], fma(E22[j], n22[j], Rt[j])));
            const double PB1 = fma(n11[j], e1, n12[j] * e2), PB2 = fma(n12[j], e1, n22[j] * e2);
            const double U1 = PB1, U2 = fma(PB1, a12k, PB2 * a22k);
            const double X12 = fma(n11[j], a12k, n12[j] * a22k);
            const double X22 = fma(A11k, n11[j], fma(A12k, n12[j], fma(A22k, n22[j], X22d)));
            const double iQ = frcp(Q);
            const double w1 = iQ * U1, w2 = iQ * U2;
            P11[j] = fma(-w1, U1, fma(f11, n11[j], X11d));
            P12[j] = fma(-w1, U2, X12);
            P22[j] = fma(-w2, U2, X22);
            W1[j] = w1; W2[j] = w2;
            Quu[j] = Q; iQs[j] = iQ;
        }
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NAX; ++j) bad = bad || !(Quu[j] > 0.0) || !isfinite(Quu[j]);
    return !wany(bad);
}

// The overlapped build (OVL; NAX == 1, QSCAN, one wave per instance, launched with three waves): LDS hand-over
// between the solver wave (wave 0) and its two helper waves, the factor wave (wave 1) and the evaluation wave
// (wave 2).  [field][lane]: every access is one conflict-free 8-byte access per lane.
// Ownership: wave 0 writes pt (the point; mu is the same value in every lane, one unmasked write) before barrier A,
// the helper waves read it after it (the factor wave the rows up to kPtZu only), and wave 0 reads its own zl, zu
// back when the speculated point is taken.  Wave 1 writes fc and the verdict record's word x (use_scan, ok), wave 2
// its words y (converged, mu decreased) and z, w (the updated mu), all before barrier B; wave 0 reads the record after
// it with one 16-byte access beside the six factor rows, every read issued before the first wait.
// Wave 0 alone writes kFlStop.  Each buffer, and each word of the record, has one writer, and its next write comes
// after a barrier that the readers cross only with their reads complete, so single buffers are enough.
enum PmPt { kPtTh, kPtLp, kPtLv, kPtZl, kPtZu, kPtP, kPtV, kPtZ, kPtMu, kPtRows };      // the point and mu
enum PmFc { kFcP11, kFcP12, kFcP22, kFcW1, kFcW2, kFcIQs, kFcRows };                            // its factors
// stop (kFl*Time: the stamps build's helper-wave timers)
enum PmFlag { kFlStop, kFlFactorTime, kFlEvalTime, kFlWords = 4 };
// the bits of the verdict record's words x (the factor wave's) and y (the evaluation wave's)
enum PmVerdict : int { kVdUseScan = 1, kVdOk = 2, kVdConverged = 1, kVdMuDec = 2 };
struct PmOvlShared {
    double pt[kPtRows][kWave];
    double fc[kFcRows][kWave];
    int4 vd;       // the verdict record: x, y the helper waves' flag words, z and w the low and high half of the updated mu
    int flag[kFlWords];
};
static_assert(offsetof(PmOvlShared, vd) % 16 == 0, "the verdict record is read with one 16-byte access");
__shared__ PmOvlShared g_pm_ovl;       // only the overlapped instantiations name it (7.5 KB beside PrShared when fused)

// IPOPT's kappa_sigma safeguard of a bound multiplier after its step: z within [1e-10, 1e10] mu / slack
__device__ __forceinline__ double pm_clamp_mult(const double z, const double mu, const double islack) {
    return fmax(fmin(z, 1e10 * mu * islack), 1e-10 * mu * islack);
}

// The build of the kernel as one mask F (kScan | kShort2 | ...: launch_plan.h, the template argument of pmpc_ipm_kernel,
// pmpc_serve_kernel and pmpc_solve); the comment above PM_EXPECT says what each flag selects.

template <int NAX, unsigned F>
__device__ __forceinline__ bool pmpc_solve(const PmpcArgs& a, const int b) {
    constexpr bool QSCAN = (F & kScan) != 0, ONEROW = (F & kOneRow) != 0, SHORT2 = (F & kShort2) != 0;
    constexpr bool RED = (F & kRed) != 0, OVL = (F & kOvl) != 0;
    static_assert(!OVL || (NAX == 1 && QSCAN && !ONEROW && !RED && kWaves == 1), "the overlapped build: scan builds of N = 16..31");
    STAMP_DECL
    const int lane = (kWaves == 1 && !OVL) ? (int)threadIdx.x : lane_id();
    const int k = NAX == 1 ? node_base() + (lane & 31) : lane;      // shooting node of this lane
    const int ax0 = NAX == 1 ? (lane >> 5) : 0;               // axis of slot 0 (NAX == 1)
    const int N = a.N;
    const bool xon = k <= N, uon = k < N;
    constexpr bool one_row = ONEROW;
    constexpr bool short2 = SHORT2 && !ONEROW;
    const double h = a.Ts;

    // every input is read here, at the start (the host entry hands them over in mapped host memory,
    // dart_mpc_abi.hip)
    const double* st = a.x0 + 6 * b;
    const double* rf = a.ref + 6 * b;
    const double* pr = a.prm + 6 * b;
    const double mu_f = pr[0], Qp = pr[1], Qv = pr[2], R = pr[3], ulo = pr[4], uhi = pr[5];

    // RK4 map of the linear axis model applied to the basis: exact Phi = [[1,a12],[0,a22]], Gamma = [b1,b2]
    double a12, a22, b1, b2;
    axis_rk4(h, a.g, mu_f, 0.0, 0.0, 1.0, a12, a22);
    axis_rk4(h, a.g, mu_f, 1.0, 0.0, 0.0, b1, b2);
    // the same for the z sub-state, z+ = zA z + zC w with w = vz_new (mpc_3d.py:93-97, RK4 :99-104):
    // pz+ = pz + cp w, vz+ = av vz + cv w
    double zp1, zav, zcp, zcv;
    z_rk4(h, 0.0, 1.0, 1.0, zp1, zav);
    z_rk4(h, 1.0, 0.0, 0.0, zcp, zcv);
    const double lo = ulo - 1e-8 * fmax(1.0, fabs(ulo));       // IPOPT bound_relax_factor = 1e-8
    const double hi = uhi + 1e-8 * fmax(1.0, fabs(uhi));
    const bool poly = fmax(fabs(lo), fabs(hi)) <= 1.0;
    // per-lane stage map: the real Phi on stages k < N, zero on the terminal/idle lanes, so that the
    // backward sweep reproduces the terminal value function there without a branch
    const double f11 = uon ? 1.0 : 0.0, a12k = uon ? a12 : 0.0, a22k = uon ? a22 : 0.0;
    const double ai22 = 1.0 / a22, ai12 = -a12 * ai22;        // A^-1 = [[1, ai12], [0, ai22]]
    // the same per lane for the quadratic scan: identity stage maps on the terminal / idle lanes
    const double uonf = uon ? 1.0 : 0.0, ai12k = uon ? ai12 : 0.0, ai22k = uon ? ai22 : 1.0, a22i = uon ? a22 : 1.0;
    const double A11k = a12k * a12k, A12k = 2.0 * a12k * a22k, A22k = a22k * a22k;

    // per-lane axis slots; z slots: NAX == 1 keeps pz on the x half and vz on the y half, NAX == 2
    // keeps pz in slot 0 and vz in slot 1 of every lane
    double sp[NAX], sv[NAX], rp[NAX], rv[NAX];
    double p[NAX], v[NAX], th[NAX], lp[NAX], lv[NAX], zl[NAX], zu[NAX];
    double zA[NAX], zC[NAX], zs[NAX], zz[NAX];
    const int nw = 6 * (N + 1) + 2 * N;
    const double* ww = a.w_warm ? a.w_warm + (size_t)nw * b : nullptr;
    const double pushl = fmin(1e-2 * fmax(1.0, fabs(lo)), 1e-2 * (hi - lo));   // IPOPT bound_push / frac
    const double pushu = fmin(1e-2 * fmax(1.0, fabs(hi)), 1e-2 * (hi - lo));
    double gmax = 0.0;
#pragma unroll
    for (int j = 0; j < NAX; ++j) {
        const int ax = NAX == 1 ? ax0 : j;
        sp[j] = st[2 * ax]; sv[j] = st[2 * ax + 1];
        rp[j] = rf[2 * ax]; rv[j] = rf[2 * ax + 1];
        p[j] = xon ? (ww ? ww[6 * k + 2 * ax] : sp[j]) : 0.0;       // cold start: tile(state) (mpc_3d.py:123)
        v[j] = xon ? (ww ? ww[6 * k + 2 * ax + 1] : sv[j]) : 0.0;
        double t = uon ? (ww ? ww[6 * (N + 1) + 2 * k + ax] : 0.0) : 0.0;
        if (uon) t = fmin(fmax(t, lo + pushl), hi - pushu);
        th[j] = t;
        lp[j] = 0.0; lv[j] = 0.0;
        zl[j] = uon ? 1.0 : 0.0; zu[j] = uon ? 1.0 : 0.0;      // bound_mult_init_val = 1
        if (xon) gmax = fmax(gmax, fmax(fabs(2 * Qp * (p[j] - rp[j])), fabs(2 * Qv * (v[j] - rv[j]))));
        if (uon) gmax = fmax(gmax, fabs(2 * R * th[j]));
        // z slot (ax here is 0 = pz, 1 = vz)
        zA[j] = ax ? zav : zp1; zC[j] = ax ? zcv : zcp;
        zs[j] = st[4 + ax];
        zz[j] = xon ? (ww ? ww[6 * k + 4 + ax] : zs[j]) : 0.0;
    }
    gmax = wmax(gmax);
    const double sc = gmax > 100.0 ? 100.0 / gmax : 1.0;     // nlp_scaling_max_gradient = 100
    const double qp2 = sc * 2 * Qp, qv2 = sc * 2 * Qv, r2 = sc * 2 * R;
    const double scQp = sc * Qp, scQv = sc * Qv, scR = sc * R;
    const PmStage stg = {f11, a12k, a22k, ai12k, ai22k, a22i, uonf, A11k, A12k, A22k};
    // stage quantities of the quadratic (Riccati) pass at a point: B_k = Gamma cos(theta_k) (0 on idle lanes), its
    // products, and the Hessian of the Lagrangian in theta, 2R + lam_{k+1}^T Gamma sin(theta) + Sigma
    auto quad_stage = [&](double csj, double snj, double lpnj, double lvnj, double zlj, double islj, double zuj,
                          double isuj, double& e1, double& e2, double& e11, double& e12, double& e22, double& rt0) {
        e1 = b1 * csj; e2 = b2 * csj;
        e11 = e1 * e1; e12 = 2.0 * e1 * e2; e22 = e2 * e2;
        rt0 = uon ? fma(snj, fma(b1, lpnj, b2 * lvnj), r2 + zlj * islj + zuj * isuj) : 1.0;
    };
    const double tol = a.tol, mu_min = tol / 10;
    const double n_eq = 6.0 * (N + 1), n_b = 4.0 * N;       // IPOPT counts on the full NLP
    const double inv_neb = 1.0 / (n_eq + n_b), inv_nb = 1.0 / n_b;
    const double gam_th = 1e-5, gam_ph = 1e-8, s_th = 1.1, s_ph = 2.3, eta_ph = 1e-8, gam_al = 0.05;

    // defect g_k = x_k - f(x_{k-1}, u_{k-1}) (mpc_3d.py:48), g_0 = x_0 - state (:37)
    auto defects = [&](double pj, double vj, double sj, double spj, double svj, double& g1, double& g2) {
        const double fp = fma(a12, vj, fma(b1, sj, pj));
        const double fv = fma(a22, vj, b2 * sj);
        double ip, iv;
        if constexpr (kWaves == 1) {
            ip = from_prev(fp); iv = from_prev(fv);
        } else {       // two waves: one exchange for both shifts
            const double x2[2] = {fp, fv};
            double o2[2];
            from_prev_n(x2, o2);
            ip = o2[0]; iv = o2[1];
        }
        g1 = (k == 0) ? pj - spj : pj - ip;
        g2 = (k == 0) ? vj - svj : vj - iv;
    };
    // the sum over both axes of a per-axis quantity of this lane's node (NAX == 1: the other half's
    // lane k + 32 / k - 32 holds the other axis)
    auto axes_sum = [&](const double (&q)[NAX]) -> double {
        if constexpr (NAX == 1) return half_pair_sum(q[0]);
        else return q[0] + q[1];
    };
    // z defects of this lane's node from the z slots zj and this lane's w = vz_new: the node k - 1
    // prediction zA z + zC w comes from the previous lane
    auto zdefect = [&](double zj, double wj, int j) -> double {
        const double fz = fma(zA[j], zj, zC[j] * wj);
        const double ip = from_prev(fz);
        return (k == 0) ? zj - zs[j] : zj - ip;
    };
    // w = vz_new = -g (theta_x^2 + theta_y^2) at this lane's node (mpc_3d.py:93), 0 past the horizon
    auto vz_new = [&](const double (&t)[NAX]) -> double {
        double sq[NAX];
#pragma unroll
        for (int j = 0; j < NAX; ++j) sq[j] = uon ? t[j] * t[j] : 0.0;
        return -a.g * axes_sum(sq);
    };

    // OVL, the evaluation wave's verdict on a point: its optimality error (IPOPT eq. 5), the convergence test and the
    // monotone barrier update, statement for statement those of the iteration loop below (which the one-wave builds
    // run, and whose text stays untouched so that they keep their instructions; the bit-for-bit tests of the
    // overlapped builds against them hold the two together).  Of the lane values only those the error terms need:
    // the cosine and the next node's multipliers, not the reciprocal slacks.  Returns converged; mu is updated in
    // place and dec tells whether it decreased (BacktrackingLineSearch::Reset in the solving wave).
    auto point_verdict = [&](const double (&p)[NAX], const double (&v)[NAX], const double (&th)[NAX],
                             const double (&lp)[NAX], const double (&lv)[NAX], const double (&zl)[NAX],
                             const double (&zu)[NAX], const double (&g1)[NAX], const double (&g2)[NAX],
                             const double (&gz)[NAX], double& mu, bool& dec) -> bool {
        double dinf = 0.0, pinf = 0.0, c0 = 0.0, cmin = 1e300, suml = 0.0, sumz = 0.0;
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            const double c_ = tilt_cos_econ(poly, th[j]);
            const double cs = uon ? c_ : 0.0;
            const double ln = from_next(lp[j]), vn = from_next(lv[j]);       // unconditional: EXEC stays full
            const double lpn = uon ? ln : 0.0, lvn = uon ? vn : 0.0;
            const double sl = th[j] - lo, su = hi - th[j];
            const double r1 = fma(qp2, p[j] - rp[j], lp[j] - lpn);
            const double r2x = fma(qv2, v[j] - rv[j], lv[j] - fma(a12, lpn, a22 * lvn));
            const double ru = fma(r2, th[j], -cs * fma(b1, lpn, b2 * lvn)) - zl[j] + zu[j];
            dinf = fmax(dinf, xon ? fmax(fabs(r1), fabs(r2x)) : 0.0);
            dinf = fmax(dinf, uon ? fabs(ru) : 0.0);
            pinf = fmax(pinf, xon ? fmax(fmax(fabs(g1[j]), fabs(g2[j])), fabs(gz[j])) : 0.0);
            suml += xon ? fabs(lp[j]) + fabs(lv[j]) : 0.0;
            c0 = fmax(c0, uon ? fmax(zl[j] * sl, zu[j] * su) : 0.0);
            cmin = fmin(cmin, uon ? fmin(zl[j] * sl, zu[j] * su) : 1e300);
            sumz += zl[j] + zu[j];
        }
        float dinf_f = (float)dinf, pinf_f = (float)pinf, c0_f = (float)c0, cmin_f = (float)cmin;
        float suml_f = (float)suml, sumz_f = (float)sumz;
        wred_errors(dinf_f, pinf_f, c0_f, cmin_f, suml_f, sumz_f);
        const double dinf_w = dinf_f, pinf_w = pinf_f, c0_w = c0_f;
        const double cmin_w = cmin_f;
        const float sz_w = sumz_f;
        const double is_d = 100.0 * frcp(fmax(100.0, (double)(suml_f + sz_w) * inv_neb));
        const double is_c = 100.0 * frcp(fmax(100.0, (double)sz_w * inv_nb));
        dinf = dinf_w; pinf = pinf_w; c0 = c0_w;
        dec = false;
        if (fmax(dinf * is_d, fmax(pinf, c0 * is_c)) <= tol) return true;
        for (;;) {
            const double cmu = fmax(c0 - mu, mu - cmin_w);
            if (fmax(dinf * is_d, fmax(pinf, cmu * is_c)) > 10.0 * mu || mu <= mu_min) break;
            mu = fmax(mu_min, fmin(0.2 * mu, mu * sqrt(mu)));
            dec = true;
        }
        return false;
    };
    (void)point_verdict;
    if constexpr (OVL) {
        // The helper waves.  Each has derived the lane constants above from the same inputs with the same code as the
        // solver wave (the gradient scaling's wave reduction included).  Every round: wait for a point (barrier A),
        // run the role's body on it, publish the result (barrier B).  One skeleton for both roles, so they cannot
        // differ in how they meet the solver wave's barriers: a helper tests the stop word after every barrier and
        // leaves the kernel when it is set (pmpc_solve's exit funnel).
        // Rounds: the start point, then per iteration the speculated first trial point and, where that trial is not
        // the accepted step, the accepted point: at most 1 + 2 max_iter.  The bound only ends a wave that a protocol
        // slip would otherwise leave at a barrier for ever (a terminated wave takes no part in one).
        auto helper_rounds = [&](auto&& body) {
            const long long max_rounds = 2ll * a.max_iter + 8;
            for (long long round = 0; round < max_rounds; ++round) {
                __syncthreads();                                            // barrier A, or the stop barrier
                if (__builtin_amdgcn_readfirstlane(g_pm_ovl.flag[kFlStop])) return;
                body();
                __syncthreads();                                            // barrier B, or the stop barrier
                if (__builtin_amdgcn_readfirstlane(g_pm_ovl.flag[kFlStop])) return;
            }
        };
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (wv == 1) {
            // The factor wave: the point at delta = 0 (attempt 0 of the iteration's Riccati block).
            helper_rounds([&]() {
#ifdef DART_STAMPS
                const unsigned long long tf0 = __builtin_amdgcn_s_memtime();
#endif
                const double th1 = g_pm_ovl.pt[kPtTh][lane];
                const double lp1 = g_pm_ovl.pt[kPtLp][lane], lv1 = g_pm_ovl.pt[kPtLv][lane];
                const double zl1 = g_pm_ovl.pt[kPtZl][lane], zu1 = g_pm_ovl.pt[kPtZu][lane];
                // (the sine by the function and the mask of the trial and of the start point: the trial's bits)
                double s_, sc_;
                tilt_sincos(poly, th1, s_, sc_);
                const double sn1 = uon ? s_ : 0.0;
                const double c_ = tilt_cos_econ(poly, th1);
                const double cs1 = uon ? c_ : 0.0;
                const double ln = from_next(lp1), vn = from_next(lv1);
                const double lpn1 = uon ? ln : 0.0, lvn1 = uon ? vn : 0.0;
                const double sl = th1 - lo, su = hi - th1;
                const double isl1 = uon ? frcp(sl) : 0.0, isu1 = uon ? frcp(su) : 0.0;
                double be1[NAX], be2[NAX], E11[NAX], E12[NAX], E22[NAX], Rt0[NAX];
                quad_stage(cs1, sn1, lpn1, lvn1, zl1, isl1, zu1, isu1, be1[0], be2[0], E11[0], E12[0], E22[0], Rt0[0]);
                double W1[NAX], W2[NAX], P11[NAX], P12[NAX], P22[NAX], iQs[NAX];
                bool us = false;
                const bool okf = pmpc_riccati<NAX, QSCAN, ONEROW, SHORT2>(lane, N, uon, false, 0.0, qp2, qv2, stg, be1,
                                                                         be2, E11, E12, E22, Rt0, P11, P12, P22, W1,
                                                                         W2, iQs, us);
                g_pm_ovl.fc[kFcP11][lane] = P11[0]; g_pm_ovl.fc[kFcP12][lane] = P12[0]; g_pm_ovl.fc[kFcP22][lane] = P22[0];
                g_pm_ovl.fc[kFcW1][lane] = W1[0]; g_pm_ovl.fc[kFcW2][lane] = W2[0]; g_pm_ovl.fc[kFcIQs][lane] = iQs[0];
                if (lane == 0) g_pm_ovl.vd.x = (us ? kVdUseScan : 0) | (okf ? kVdOk : 0);
#ifdef DART_STAMPS
                // the factor wave's own time from barrier A to its arrival at barrier B, summed (slot 13 of wave 0)
                t_acc_[13] += __builtin_amdgcn_s_memtime() - tf0;
                if (lane == 0) g_pm_ovl.flag[kFlFactorTime] = (int)t_acc_[13];
#endif
            });
            return false;
        }
        if (wv == 2) {
            // The evaluation wave: the defects of the point by the expressions of the line-search trial that wave 0
            // carries them from (and of the start point), then point_verdict.  It indexes memory by lane only,
            // whatever the point holds.
            helper_rounds([&]() {
#ifdef DART_STAMPS
                const unsigned long long te0 = __builtin_amdgcn_s_memtime();
#endif
                const double th1[NAX] = {g_pm_ovl.pt[kPtTh][lane]};
                const double lp1[NAX] = {g_pm_ovl.pt[kPtLp][lane]}, lv1[NAX] = {g_pm_ovl.pt[kPtLv][lane]};
                const double zl1[NAX] = {g_pm_ovl.pt[kPtZl][lane]}, zu1[NAX] = {g_pm_ovl.pt[kPtZu][lane]};
                const double p1[NAX] = {g_pm_ovl.pt[kPtP][lane]}, v1[NAX] = {g_pm_ovl.pt[kPtV][lane]};
                const double zz1 = g_pm_ovl.pt[kPtZ][lane];
                double mu1 = wave_uniform(g_pm_ovl.pt[kPtMu][lane]);
                double g1e[NAX], g2e[NAX], gze[NAX];
                const double w1 = vz_new(th1);
                double s_, sc_;       // (the sine as the trial and the start point form it: the same bits)
                tilt_sincos(poly, th1[0], s_, sc_);
                const double sn1 = uon ? s_ : 0.0;
                defects(p1[0], v1[0], sn1, sp[0], sv[0], g1e[0], g2e[0]);
                gze[0] = zdefect(zz1, w1, 0);
                bool dec = false;
                const bool conv = point_verdict(p1, v1, th1, lp1, lv1, zl1, zu1, g1e, g2e, gze, mu1, dec);
                if (lane == 0) {
                    g_pm_ovl.vd.y = (conv ? kVdConverged : 0) | (dec ? kVdMuDec : 0);
                    g_pm_ovl.vd.z = __double2loint(mu1); g_pm_ovl.vd.w = __double2hiint(mu1);
                }
#ifdef DART_STAMPS
                // the evaluation wave's own time from barrier A to its arrival at barrier B, summed (slot 17 of wave 0)
                t_acc_[17] += __builtin_amdgcn_s_memtime() - te0;
                if (lane == 0) g_pm_ovl.flag[kFlEvalTime] = (int)t_acc_[17];
#endif
            });
            return false;
        }
        if (lane == 0) g_pm_ovl.flag[kFlStop] = 0;      // the solver wave, before its first barrier
    }

    // sines and defects of the current point: computed here once, then carried over from the
    // accepted line-search trial (the update x + alpha d repeats the trial's arithmetic exactly)
    double g1[NAX], g2[NAX], gz[NAX], snc[NAX];
    // OVL: the barrier logarithm log((theta - lo)(hi - theta)) of the current point is carried the same way (the
    // line-search preparation needs it at the point the accepted trial evaluated it at; mu multiplies it outside)
    double lgc[NAX];
    (void)lgc;
    double th0 = 0.0;
    {
        const double w0 = vz_new(th);
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            double s0, c0_;
            tilt_sincos(poly, th[j], s0, c0_);
            snc[j] = uon ? s0 : 0.0;
            if constexpr (OVL) lgc[j] = log_fast((th[j] - lo) * (hi - th[j]));
            defects(p[j], v[j], snc[j], sp[j], sv[j], g1[j], g2[j]);
            gz[j] = RED ? 0.0 : zdefect(zz[j], w0, j);
            if (xon) th0 += fabs(g1[j]) + fabs(g2[j]) + fabs(gz[j]);
        }
    }
    double theta = wsum(th0);                                  // filter's constraint violation
    const double th_max = 1e4 * fmax(1.0, theta), th_min = 1e-4 * fmax(1.0, theta);

    double fth = 0.0, fph = 0.0;      // filter entry held by lane (slot = lane id)
    int nfilt = 0;
    double mu = 0.1, delta_last = 0.0;
    int status = -1, it = 0;
    // IPOPT's soft restoration phase (round 5): in_soft while its steps are being taken, soft_count of them
    int in_soft = 0, soft_count = 0;
    STAMP(0);

    // OVL: the z scan's multipliers after its levels row_shr 1, 2, 4 (and 8: the full scan), lane constants of the
    // launch (Ts and the node index only), by the products the levels of direction() form
    double zsm[4] = {0.0, 0.0, 0.0, 0.0};
    (void)zsm;
    if constexpr (OVL) {
        double m = k == 0 ? 0.0 : zA[0], c = 0.0;
        affine1_scan_level<0x111, 0xf>(m, c); zsm[0] = m;
        affine1_scan_level<0x112, 0xf>(m, c); zsm[1] = m;
        affine1_scan_level<0x114, 0xf>(m, c); zsm[2] = m;
        if constexpr (!short2) { affine1_scan_level<0x118, 0xf>(m, c); zsm[3] = m; }
    }

    // OVL: the current point and mu to the helper waves, then barrier A.  Called for the start point at the first Newton
    // iteration, and in the accepted update where the step taken is not the line search's first trial point (that
    // point is handed over speculatively before the trial, below; the update then first crosses barrier B to drop
    // the factors and the verdict of the rejected point).  The scheduling barriers keep the compiler from moving the work that
    // follows (plain register arithmetic, which __syncthreads() does not order) ahead of barrier A.
    bool published = false;
    auto publish = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        g_pm_ovl.pt[kPtTh][lane] = th[0];
        g_pm_ovl.pt[kPtLp][lane] = lp[0]; g_pm_ovl.pt[kPtLv][lane] = lv[0];
        g_pm_ovl.pt[kPtZl][lane] = zl[0]; g_pm_ovl.pt[kPtZu][lane] = zu[0];
        g_pm_ovl.pt[kPtP][lane] = p[0]; g_pm_ovl.pt[kPtV][lane] = v[0];
        g_pm_ovl.pt[kPtZ][lane] = zz[0]; g_pm_ovl.pt[kPtMu][lane] = mu;
        __syncthreads();                                                    // barrier A
        __builtin_amdgcn_sched_barrier(0);
        published = true;
    };
#ifdef DART_STAMPS
    const unsigned long long t_loop0 = __builtin_amdgcn_s_memtime();
#endif
    // it = -1 (a.mult_init_max > 0): IPOPT's least-square estimate of the starting equality
    // multipliers (DefaultIterateInitializer::least_square_mults, constr_mult_init_max = 1000): the
    // step solve of the loop body with unit weights (X = I, R = 1), the gradient r = grad f - z_L + z_U
    // and a zero constraint right-hand side gives y = argmin ||r + J^T y|| as its new multipliers
    // (LeastSquareMultipliers: [I J^T; J 0] [d; y] = [-r; 0]).  Cold start: the z rows' input columns
    // vanish (theta = 0), so the estimate separates per axis and y_z = 0.
    for (it = a.mult_init_max > 0.0 ? -1 : 0; it < a.max_iter; ++it) {
        const bool lsm = it < 0;
#ifdef DART_STAMPS
        if (it == 1) t_acc_[12] = __builtin_amdgcn_s_memtime() - t_loop0;      // the first iteration (cold code)
#endif
        if constexpr (OVL) {
            // the start point (every later point is published by the line search of the iteration before, or by its
            // update); the least-square iteration keeps its factorisation (unit weights) in this wave and crosses
            // no barrier
            if (PM_EXPECT(!lsm && !published, 0)) publish();
        }
        // -------- point quantities and optimality error (IPOPT eq. 5) ------------
        // (OVL: this wave forms the lane values only.  The error terms, the convergence test and the mu update, the
        // statements under `if constexpr (!OVL)`, are the evaluation wave's, which states them in point_verdict; the
        // text here stays as it is, declarations and all, so that every other build keeps its instructions.)
        double sn[NAX], cs[NAX], isl[NAX], isu[NAX], lpn[NAX], lvn[NAX];
        double dinf = 0.0, pinf = 0.0, c0 = 0.0, cmin = 1e300, suml = 0.0, sumz = 0.0;
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            sn[j] = snc[j];
            const double c_ = tilt_cos_econ(poly, th[j]);
            cs[j] = uon ? c_ : 0.0;
            double ln, vn;       // unconditional: EXEC stays full
            if constexpr (kWaves == 1) {
                ln = from_next(lp[j]); vn = from_next(lv[j]);
            } else {
                const double x2[2] = {lp[j], lv[j]};
                double o2[2];
                from_next_n(x2, o2);
                ln = o2[0]; vn = o2[1];
            }
            lpn[j] = uon ? ln : 0.0; lvn[j] = uon ? vn : 0.0;
            const double sl = th[j] - lo, su = hi - th[j];
            isl[j] = uon ? frcp(sl) : 0.0; isu[j] = uon ? frcp(su) : 0.0;
            STAMP(16);      // (stamps build: the lane values end, the error terms begin)
            const double r1 = fma(qp2, p[j] - rp[j], lp[j] - lpn[j]);
            const double r2x = fma(qv2, v[j] - rv[j], lv[j] - fma(a12, lpn[j], a22 * lvn[j]));
            const double ru = fma(r2, th[j], -cs[j] * fma(b1, lpn[j], b2 * lvn[j])) - zl[j] + zu[j];
            if constexpr (!OVL) {
            dinf = fmax(dinf, xon ? fmax(fabs(r1), fabs(r2x)) : 0.0);
            dinf = fmax(dinf, uon ? fabs(ru) : 0.0);
            pinf = fmax(pinf, xon ? fmax(fmax(fabs(g1[j]), fabs(g2[j])), fabs(gz[j])) : 0.0);
            suml += xon ? fabs(lp[j]) + fabs(lv[j]) : 0.0;
            c0 = fmax(c0, uon ? fmax(zl[j] * sl, zu[j] * su) : 0.0);
            cmin = fmin(cmin, uon ? fmin(zl[j] * sl, zu[j] * su) : 1e300);
            sumz += zl[j] + zu[j];
            }
        }
        float dinf_f = (float)dinf, pinf_f = (float)pinf, c0_f = (float)c0, cmin_f = (float)cmin;
        float suml_f = (float)suml, sumz_f = (float)sumz;
        if constexpr (!OVL) wred_errors(dinf_f, pinf_f, c0_f, cmin_f, suml_f, sumz_f);
        const double dinf_w = dinf_f, pinf_w = pinf_f, c0_w = c0_f;
        const double cmin_w = cmin_f;
        // IPOPT's scalings s_d, s_c (>= 1) as reciprocals: one division each instead of one per test
        const float sz_w = sumz_f;
        const double is_d = 100.0 * frcp(fmax(100.0, (double)(suml_f + sz_w) * inv_neb));
        const double is_c = 100.0 * frcp(fmax(100.0, (double)sz_w * inv_nb));
        dinf = dinf_w; pinf = pinf_w; c0 = c0_w;
        STAMP(1);
        if constexpr (!OVL) {
        if (!lsm && fmax(dinf * is_d, fmax(pinf, c0 * is_c)) <= tol) { status = 0; break; }
        }
        // -------- monotone barrier update (Fiacco-McCormick, may fire repeatedly) --
        // max_i |z_i s_i - mu| = max(max z s - mu, mu - min z s): one reduction pair, scalar loop
        if constexpr (!OVL) {
        for (; !lsm;) {
            const double cmu = fmax(c0 - mu, mu - cmin_w);
            if (fmax(dinf * is_d, fmax(pinf, cmu * is_c)) > 10.0 * mu || mu <= mu_min) break;
            mu = fmax(mu_min, fmin(0.2 * mu, mu * sqrt(mu)));
            nfilt = 0; in_soft = 0;       // BacktrackingLineSearch::Reset: the filter and the soft phase
        }
        }
        double tau = fmax(0.99, 1.0 - mu);
        STAMP(2);

        // -------- Newton step: Riccati recursion + inertia correction ---------------
        double be1[NAX], be2[NAX], E11[NAX], E12[NAX], E22[NAX], Rt0[NAX], rt[NAX], q1[NAX], q2[NAX];
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            quad_stage(cs[j], sn[j], lpn[j], lvn[j], zl[j], isl[j], zu[j], isu[j], be1[j], be2[j], E11[j], E12[j],
                       E22[j], Rt0[j]);
            // the barrier gradient in theta (least-square estimate: r_u = grad f - z_L + z_U)
            // (OVL: mu comes with the factors, so the Newton iterations form it after barrier B)
            if (!OVL || lsm) rt[j] = uon ? (lsm ? r2 * th[j] - zl[j] + zu[j] : fma(r2, th[j], mu * (isu[j] - isl[j]))) : 0.0;
            q1[j] = qp2 * (p[j] - rp[j]); q2[j] = qv2 * (v[j] - rv[j]);
        }
        double W1[NAX], W2[NAX], P11[NAX], P12[NAX], P22[NAX], iQs[NAX];
        double delta = 0.0;
        bool ok = false;
        int attempt = 0;
        if constexpr (OVL) {
            // attempt 0 comes from the factor wave.  Where it did not take the scan or found a Quu <= 0, the loop
            // below runs in this wave from attempt 0 on, as in the one-wave build (the sequential sweep, the
            // inertia retries): cold paths, without the helper waves and so without barriers.
            // The evaluation wave's verdict on the point comes with the factors: converged (status 0 and out through
            // the funnel, with nothing outstanding: both helper waves are on their way to barrier A), the updated mu,
            // and whether it decreased (BacktrackingLineSearch::Reset, as in the one-wave mu update).
            if (!lsm) {
                __builtin_amdgcn_sched_barrier(0);      // everything above is done before this wave waits
                // (lgkmcnt(0): this wave's own LDS reads of the iteration before, the multipliers read back on a
                // hit, have long returned; stated here so that the compiler puts no guard of their registers
                // between the reads that follow the barrier)
                __builtin_amdgcn_s_waitcnt(0xc07f);
                SPAN_BEGIN(t_b);
                __syncthreads();                                            // barrier B
                SPAN_END(14, t_b);                      // (stamps build, slot 14: the wait alone)
                // One LDS round trip: the verdict record (one 16-byte read) and the six factor rows are all issued
                // ahead of the scheduling barrier; the scalars are taken and the branch on converged is made behind
                // it, so the first wait is for the record alone, with the factor rows on their way
                const int4 vd = g_pm_ovl.vd;
                P11[0] = g_pm_ovl.fc[kFcP11][lane]; P12[0] = g_pm_ovl.fc[kFcP12][lane]; P22[0] = g_pm_ovl.fc[kFcP22][lane];
                W1[0] = g_pm_ovl.fc[kFcW1][lane]; W2[0] = g_pm_ovl.fc[kFcW2][lane]; iQs[0] = g_pm_ovl.fc[kFcIQs][lane];
                __builtin_amdgcn_sched_barrier(0);
                const int vdf = __builtin_amdgcn_readfirstlane(vd.x), vde = __builtin_amdgcn_readfirstlane(vd.y);
                const double mun = __hiloint2double(__builtin_amdgcn_readfirstlane(vd.w), __builtin_amdgcn_readfirstlane(vd.z));
                const bool us = (vdf & kVdUseScan) != 0;
                const bool okf = (vdf & kVdOk) != 0;
                if (vde & kVdConverged) { status = 0; break; }
                mu = mun;
                if (vde & kVdMuDec) { nfilt = 0; in_soft = 0; }
                tau = fmax(0.99, 1.0 - mu);
                rt[0] = uon ? fma(r2, th[0], mu * (isu[0] - isl[0])) : 0.0;
                if (PM_EXPECT(us && okf, 1)) {
                    STAMP_ADD(11, 1);
                    ok = true; attempt = 1;
                }
            }
        }
        for (; attempt < 60 && !ok; ++attempt) {
            if (PM_EXPECT(attempt > 0, 0))
                delta = (attempt == 1) ? (delta_last == 0.0 ? 1e-4 : fmax(1e-20, delta_last * (1.0 / 3.0)))   // IPOPT perturb_dec_fact 1/3
                                       : delta * (delta_last == 0.0 ? 100.0 : 8.0);
            bool use_scan = false;
            ok = pmpc_riccati<NAX, QSCAN, ONEROW, SHORT2>(lane, N, uon, lsm, delta, qp2, qv2, stg, be1, be2, E11, E12,
                                                          E22, Rt0, P11, P12, P22, W1, W2, iQs, use_scan);
            STAMP_ADD(11, use_scan ? 1 : 0);
        }
        STAMP_ADD(9, attempt);
        STAMP(3);
        if (PM_EXPECT(!ok, 0)) { status = -3; break; }
        if (delta > 0.0) delta_last = delta;

        // -------- the step for the constraint right-hand side (g1, g2, gz) ---------------
        // One call site serves the Newton step and IPOPT's second-order correction passes
        // (FilterLSAcceptor::TrySecondOrderCorrection, kappa_soc 0.99): a correction re-solves the
        // factorised system with c_soc <- alpha_soc c_soc + c(x_trial) (from c(x), alpha_soc = alpha)
        // in place of the defects, so while it runs g1 / g2 / gz hold c_soc.
        double dp[NAX], dv[NAX], dth[NAX], dlp[NAX], dlv[NAX], dzl[NAX], dzu[NAX], dz[NAX];
        double amax = 1.0, az = 1.0;
        float am_lf = 1.0f, az_lf = 1.0f;     // this lane's fractions to the boundary (the wave minima: amax, az)
        const double (&g1o)[NAX] = g1, (&g2o)[NAX] = g2, (&gzo)[NAX] = gz;
        auto direction = [&]() {
            double p1[NAX], p2[NAX], kff[NAX], gn1[NAX], gn2[NAX], g1[NAX], g2[NAX], gz[NAX];
#pragma unroll
            for (int j = 0; j < NAX; ++j) {      // right-hand side: the defects (0 for the multiplier estimate)
                g1[j] = lsm ? 0.0 : g1o[j]; g2[j] = lsm ? 0.0 : g2o[j]; gz[j] = lsm ? 0.0 : gzo[j];
            }
            double nPw[3];       // two waves: P_{k+1} fetched with g_{k+1} in one exchange
            if constexpr (kWaves == 1) {
#pragma unroll
                for (int j = 0; j < NAX; ++j) { gn1[j] = from_next(g1[j]); gn2[j] = from_next(g2[j]); }
            } else {
                const double x5[5] = {g1[0], g2[0], P11[0], P12[0], P22[0]};
                double o5[5];
                from_next_n(x5, o5);
                gn1[0] = o5[0]; gn2[0] = o5[1]; nPw[0] = o5[2]; nPw[1] = o5[3]; nPw[2] = o5[4];
            }
            if constexpr (NAX == 1) {
                // linear part of the value function, p_k = M_k p_{k+1} + m_k with M_k = A_k^T - w_k e_k^T
                // and m_k = q_k - w_k rt_k - M_k P_{k+1} g_{k+1}: a suffix scan of affine maps (row_shl
                // 1/2/4/8 inside the rows, then row 1 -> row 0 of each half by a lane shuffle); the
                // terminal/idle lanes carry M = 0, so each suffix stops at node N
                const double e1 = be1[0], e2 = be2[0], w1 = W1[0], w2 = W2[0];
                const double nP11 = kWaves == 1 ? from_next(P11[0]) : nPw[0];
                const double nP12 = kWaves == 1 ? from_next(P12[0]) : nPw[1];
                const double nP22 = kWaves == 1 ? from_next(P22[0]) : nPw[2];
                const double t1 = fma(nP11, gn1[0], nP12 * gn2[0]), t2 = fma(nP12, gn1[0], nP22 * gn2[0]);
                double m11 = fma(-w1, e1, f11), m12 = -w1 * e2, m21 = fma(-w2, e1, a12k), m22 = fma(-w2, e2, a22k);
                const double rtk = rt[0];
                double c1 = fma(-w1, rtk, q1[0]) - fma(m11, t1, m12 * t2);
                double c2 = fma(-w2, rtk, q2[0]) - fma(m21, t1, m22 * t2);
                double p32[2] = {0.0, 0.0};      // two waves: p of node 32 (wave 1) in wave 0
                (void)p32;
                affine_scan_level<0x101, 0xf>(m11, m12, m21, m22, c1, c2);   // row_shl:1
                affine_scan_level<0x102, 0xf>(m11, m12, m21, m22, c1, c2);   // row_shl:2
                affine_scan_level<0x104, 0xf>(m11, m12, m21, m22, c1, c2);   // row_shl:4
                if constexpr (short2 || one_row) {
                    // N <= 23: lanes 16-23 (48-55) are final after 3 levels; lanes 8-15 compose with the
                    // constant of lane 16 (N <= 15: already final), then lanes 0-7 with the (final)
                    // constant of lane k + 8
                    if constexpr (short2) {
                        const double r1 = half_bcast_c<16>(c1), r2 = half_bcast_c<16>(c2);
                        if ((lane & 24) == 8) {
                            c1 = fma(m11, r1, fma(m12, r2, c1));
                            c2 = fma(m21, r1, fma(m22, r2, c2));
                        }
                    }
                    const double s1 = dpp_fill<0x108, 0xf, 0>(c1), s2 = dpp_fill<0x108, 0xf, 0>(c2);
                    if ((lane & 24) == 0) {
                        c1 = fma(m11, s1, fma(m12, s2, c1));
                        c2 = fma(m21, s1, fma(m22, s2, c2));
                    }
                } else {
                    affine_scan_level<0x108, 0xf>(m11, m12, m21, m22, c1, c2);   // row_shl:8
                    // rows 0 and 2 compose with the suffix held by the first lane of rows 1 and 3
                    const bool lo_row = (lane & 16) == 0;
                    if constexpr (kWaves == 1) {
                        const double r1 = half_bcast_c<16>(c1), r2 = half_bcast_c<16>(c2);   // only the constant is needed now
                        if (lo_row) {
                            c1 = fma(m11, r1, fma(m12, r2, c1));
                            c2 = fma(m21, r1, fma(m22, r2, c2));
                        }
                    } else {
                        auto rows = [&]() {
                            const double r1 = half_bcast_c<16>(c1), r2 = half_bcast_c<16>(c2);
                            if (lo_row) {
                                c1 = fma(m11, r1, fma(m12, r2, c1));
                                c2 = fma(m21, r1, fma(m22, r2, c2));
                            }
                        };
                        // two waves: wave 0's rows 1 / 3 (their maps span nodes k..31) continue from p_32 of wave 1
                        if (wave_idx() == 1) rows();
                        double r[2];
                        { const double v[2] = {c1, c2}; pm_pass<1>(1, 0, v, r); }
                        p32[0] = r[0]; p32[1] = r[1];
                        if (wave_idx() == 0) {
                            if (!lo_row) {
                                c1 = fma(m11, r[0], fma(m12, r[1], c1));
                                c2 = fma(m21, r[0], fma(m22, r[1], c2));
                            }
                            rows();
                        }
                    }
                }
                p1[0] = c1; p2[0] = c2;
                // feed-forward k_k = -(e^T h + rt) / Q with h = p_{k+1} - P_{k+1} g_{k+1}
                double np1, np2;
                if constexpr (kWaves == 1) {
                    np1 = from_next(c1); np2 = from_next(c2);
                } else {
                    // two waves: node 32's p is already in wave 0 (p32), no exchange
                    np1 = dpp<kWaveShl1>(c1); np2 = dpp<kWaveShl1>(c2);
                    if (wave_idx() == 0 && (lane & 31) == 31) { np1 = p32[0]; np2 = p32[1]; }
                }
                const double h1 = np1 - t1, h2 = np2 - t2;
                kff[0] = -iQs[0] * fma(e1, h1, fma(e2, h2, rtk));

                // forward sweep of the state step: dx_k = F_{k-1} dx_{k-1} + f_{k-1} - g_k as an
                // inclusive scan of affine maps within each 32-lane axis half (DPP row_shr 1/2/4/8 inside
                // the 16-lane rows, then row_bcast:15 into the second row of each half)
                double pw1, pw2, pkf, pb1, pb2;
                if constexpr (kWaves == 1) {
                    pw1 = from_prev(W1[0]); pw2 = from_prev(W2[0]); pkf = from_prev(kff[0]);
                    pb1 = from_prev(be1[0]); pb2 = from_prev(be2[0]);
                } else {
                    const double x5[5] = {W1[0], W2[0], kff[0], be1[0], be2[0]};
                    double o5[5];
                    from_prev_n(x5, o5);
                    pw1 = o5[0]; pw2 = o5[1]; pkf = o5[2]; pb1 = o5[3]; pb2 = o5[4];
                }
                double f11_ = 1.0 - pb1 * pw1, f12_ = fma(-pb1, pw2, a12), f21_ = -pb2 * pw1, f22_ = fma(-pb2, pw2, a22);
                double d1 = fma(pb1, pkf, -g1[0]), d2 = fma(pb2, pkf, -g2[0]);
                if (k == 0) { f11_ = 0.0; f12_ = 0.0; f21_ = 0.0; f22_ = 0.0; d1 = -g1[0]; d2 = -g2[0]; }
                affine_scan_level<0x111, 0xf>(f11_, f12_, f21_, f22_, d1, d2);   // row_shr:1
                affine_scan_level<0x112, 0xf>(f11_, f12_, f21_, f22_, d1, d2);   // row_shr:2
                affine_scan_level<0x114, 0xf>(f11_, f12_, f21_, f22_, d1, d2);   // row_shr:4
                // after 3 levels the windows of lanes 0-7 reach node 0 (map 0, a constant): with N <= 23
                // the row_shr:8 level only moves constants (row 1's lanes 16-23 read nothing); lane 15 is
                // a constant once row 0 is done, so the row_bcast:15 level into rows 1 / 3 is one too
                if constexpr (one_row || short2) affine_scan_const<0x118, 0xf>(f11_, f12_, f21_, f22_, d1, d2);
                else affine_scan_level<0x118, 0xf>(f11_, f12_, f21_, f22_, d1, d2);   // row_shr:8
                if constexpr (kWaves == 1) {
                    if constexpr (!one_row) affine_scan_const<0x142, 0xa>(f11_, f12_, f21_, f22_, d1, d2);   // row_bcast:15 -> rows 1, 3
                } else {
                    // two waves: wave 1's rows 0 / 2 (their maps span nodes 32..k) continue from dx_31 of wave 0
                    if (wave_idx() == 0) affine_scan_const<0x142, 0xa>(f11_, f12_, f21_, f22_, d1, d2);
                    double r[2];
                    { const double v[2] = {d1, d2}; pm_pass<2>(0, 31, v, r); }
                    if (wave_idx() == 1) {
                        if ((lane & 16) == 0) {
                            d1 = fma(f11_, r[0], fma(f12_, r[1], d1));
                            d2 = fma(f21_, r[0], fma(f22_, r[1], d2));
                        }
                        affine_scan_const<0x142, 0xa>(f11_, f12_, f21_, f22_, d1, d2);
                    }
                }
                dp[0] = d1; dv[0] = d2;
            } else {
                // linear part of the value function (sequential): p_k = q_k + A_k^T h - w_k (e^T h + rt)
                double nP11[NAX], nP12[NAX], nP22[NAX];
#pragma unroll
                for (int j = 0; j < NAX; ++j) {
                    nP11[j] = from_next(P11[j]); nP12[j] = from_next(P12[j]); nP22[j] = from_next(P22[j]);
                    p1[j] = q1[j]; p2[j] = q2[j]; kff[j] = 0.0;
                }
                for (int step = 0; step < N; ++step) {
                    double n1[NAX], n2[NAX];
#pragma unroll
                    for (int j = 0; j < NAX; ++j) { n1[j] = from_next(p1[j]); n2[j] = from_next(p2[j]); }
#pragma unroll
                    for (int j = 0; j < NAX; ++j) {
                        const double h1 = n1[j] - fma(nP11[j], gn1[j], nP12[j] * gn2[j]);
                        const double h2 = n2[j] - fma(nP12[j], gn1[j], nP22[j] * gn2[j]);
                        const double qu = fma(be1[j], h1, fma(be2[j], h2, rt[j]));
                        kff[j] = -iQs[j] * qu;
                        p1[j] = fma(-W1[j], qu, fma(f11, h1, q1[j]));
                        p2[j] = fma(-W2[j], qu, q2[j] + fma(a12k, h1, a22k * h2));
                    }
                }
#pragma unroll
                for (int j = 0; j < NAX; ++j) { dp[j] = -g1[j]; dv[j] = -g2[j]; }
                for (int step = 0; step < N; ++step) {
                    double op[NAX], ov[NAX];
#pragma unroll
                    for (int j = 0; j < NAX; ++j) {
                        const double dt_ = fma(-W1[j], dp[j], fma(-W2[j], dv[j], kff[j]));
                        op[j] = fma(a12, dv[j], fma(be1[j], dt_, dp[j]));
                        ov[j] = fma(a22, dv[j], be2[j] * dt_);
                    }
#pragma unroll
                    for (int j = 0; j < NAX; ++j) {
                        const double ip = from_prev(op[j]), iv = from_prev(ov[j]);
                        dp[j] = k >= 1 ? ip - g1[j] : dp[j];
                        dv[j] = k >= 1 ? iv - g2[j] : dv[j];
                    }
                }
            }
            double am = 1.0, az_ = 1.0, twd[NAX];
#pragma unroll
            for (int j = 0; j < NAX; ++j) {
                dth[j] = uon ? fma(-W1[j], dp[j], fma(-W2[j], dv[j], kff[j])) : 0.0;
                // new multipliers lam+ = -(P dx + p), step = lam+ - lam
                dlp[j] = xon ? -fma(P11[j], dp[j], fma(P12[j], dv[j], p1[j])) - lp[j] : 0.0;
                dlv[j] = xon ? -fma(P12[j], dp[j], fma(P22[j], dv[j], p2[j])) - lv[j] : 0.0;
                const double sl = th[j] - lo, su = hi - th[j];
                const double zlx = zl[j] * isl[j], zux = zu[j] * isu[j];
                dzl[j] = uon ? fma(-zlx, dth[j], fma(mu, isl[j], -zl[j])) : 0.0;
                dzu[j] = uon ? fma(zux, dth[j], fma(mu, isu[j], -zu[j])) : 0.0;
                const double ith = frcp(dth[j]);
                const double cand = dth[j] < 0 ? -tau * sl * ith : (dth[j] > 0 ? tau * su * ith : 1.0);
                const double czl = dzl[j] < 0 ? -tau * zl[j] * frcp(dzl[j]) : 1.0;
                const double czu = dzu[j] < 0 ? -tau * zu[j] * frcp(dzu[j]) : 1.0;
                am = fmin(am, uon ? cand : 1.0);
                az_ = fmin(az_, uon ? fmin(czl, czu) : 1.0);
                twd[j] = 2.0 * th[j] * dth[j];
            }
            // f32 minima rounded down (tau <= 0.99 leaves far more slack than the f32 rounding); reduced by the
            // caller (frac_minima, or with the line search's sums)
            am_lf = (float)am; az_lf = (float)az_;
            // z step: dz_k = zA dz_{k-1} + zC dw_{k-1} - gz_k, dw = -g (2 theta_x dtheta_x + 2 theta_y dtheta_y)
            const double wd = RED ? 0.0 : -a.g * axes_sum(twd);
            if constexpr (RED) {
#pragma unroll
                for (int j = 0; j < NAX; ++j) dz[j] = 0.0;
            } else if constexpr (NAX == 1) {
                const double src = from_prev(zC[0] * wd);
                double m = k == 0 ? 0.0 : zA[0], c = k == 0 ? -gz[0] : src - gz[0];
                if constexpr (OVL) {
                    // the multipliers are lane constants of the launch (zsm, formed before the loop)
                    affine1_scan_const<0x111, 0xf>(m, c);        // row_shr:1
                    affine1_scan_const<0x112, 0xf>(zsm[0], c);   // row_shr:2
                    affine1_scan_const<0x114, 0xf>(zsm[1], c);   // row_shr:4
                    affine1_scan_const<0x118, 0xf>(zsm[2], c);   // row_shr:8
                    m = short2 ? zsm[2] : zsm[3];
                } else {
                affine1_scan_level<0x111, 0xf>(m, c);   // row_shr:1
                affine1_scan_level<0x112, 0xf>(m, c);   // row_shr:2
                affine1_scan_level<0x114, 0xf>(m, c);   // row_shr:4
                if constexpr (one_row || short2) affine1_scan_const<0x118, 0xf>(m, c);
                else affine1_scan_level<0x118, 0xf>(m, c);   // row_shr:8
                }
                if constexpr (kWaves == 1) {
                    if constexpr (!one_row) affine1_scan_const<0x142, 0xa>(m, c);   // row_bcast:15 -> rows 1, 3
                } else {       // two waves: as the state sweep
                    if (wave_idx() == 0) affine1_scan_const<0x142, 0xa>(m, c);
                    double r[1];
                    { const double v[1] = {c}; pm_pass<3>(0, 31, v, r); }
                    if (wave_idx() == 1) {
                        if ((lane & 16) == 0) c = fma(m, r[0], c);
                        affine1_scan_const<0x142, 0xa>(m, c);
                    }
                }
                dz[0] = c;
            } else {
#pragma unroll
                for (int j = 0; j < NAX; ++j) dz[j] = -gz[j];
                for (int step = 0; step < N; ++step) {
#pragma unroll
                    for (int j = 0; j < NAX; ++j) {
                        const double ip = from_prev(fma(zA[j], dz[j], zC[j] * wd));
                        dz[j] = k >= 1 ? ip - gz[j] : dz[j];
                    }
                }
            }
        };

        // amax, az from this lane's fractions (f32 minima rounded down)
        auto frac_set = [&]() {
            amax = (double)am_lf * (1.0 - 1.0 / 1048576.0);
            az = (double)az_lf * (1.0 - 1.0 / 1048576.0);
        };

        // -------- filter line search (Waechter & Biegler 2006, Alg. A) with second-order correction
        double alpha = 1.0, amain = 1.0, th_t = 0.0, ph_t = 0.0, th_old = 0.0, phi = 0.0, gTd = 0.0, amin = 0.0;
        float lg_sw = 0.0f;
        bool accepted = false, ftype = false, tiny = false;
        int ls = 0, soc = 0;        // soc: 0 Newton step, 1.. correction pass, -1 Newton step again after failed passes
        double snt[NAX], g1t[NAX], g2t[NAX], gzt[NAX];     // the trial's sines and defects (carried on acceptance)
        double lgt[NAX];                                   // OVL: and its barrier logarithm
        (void)lgt;
        // trial point x + al d: defects, wave-summed theta and barrier objective
        auto trial = [&](double al) {
            double thl = 0.0, phl = 0.0, tt[NAX];
            if constexpr (kWaves == 2 && NAX == 1 && !RED) {
                // two waves: the three node shifts of the trial's defects (defects, zdefect) in one exchange
                const double pt = fma(al, dp[0], p[0]), vt = fma(al, dv[0], v[0]);
                tt[0] = fma(al, dth[0], th[0]);
                double s_, c_;
                tilt_sincos(poly, tt[0], s_, c_);
                snt[0] = uon ? s_ : 0.0;
                const double wt = vz_new(tt);
                const double zt = fma(al, dz[0], zz[0]);
                const double x3[3] = {fma(a12, vt, fma(b1, snt[0], pt)), fma(a22, vt, b2 * snt[0]),
                                      fma(zA[0], zt, zC[0] * wt)};
                double o3[3];
                from_prev_n(x3, o3);
                g1t[0] = (k == 0) ? pt - sp[0] : pt - o3[0];
                g2t[0] = (k == 0) ? vt - sv[0] : vt - o3[1];
                gzt[0] = (k == 0) ? zt - zs[0] : zt - o3[2];
                const double ep = pt - rp[0], ev = vt - rv[0];
                thl += xon ? fabs(g1t[0]) + fabs(g2t[0]) : 0.0;
                phl += xon ? fma(scQp * ep, ep, scQv * ev * ev) : 0.0;
                phl += uon ? fma(scR * tt[0], tt[0], -mu * log_fast((tt[0] - lo) * (hi - tt[0]))) : 0.0;
                thl += xon ? fabs(gzt[0]) : 0.0;
                wsum2(thl, phl);
                th_t = thl; ph_t = phl;
                return;
            }
#pragma unroll
            for (int j = 0; j < NAX; ++j) {
                const double pt = fma(al, dp[j], p[j]), vt = fma(al, dv[j], v[j]);
                tt[j] = fma(al, dth[j], th[j]);
                double s_, c_;
                tilt_sincos(poly, tt[j], s_, c_);
                snt[j] = uon ? s_ : 0.0;
                defects(pt, vt, snt[j], sp[j], sv[j], g1t[j], g2t[j]);
                const double ep = pt - rp[j], ev = vt - rv[j];
                thl += xon ? fabs(g1t[j]) + fabs(g2t[j]) : 0.0;
                phl += xon ? fma(scQp * ep, ep, scQv * ev * ev) : 0.0;
                if constexpr (OVL) {
                    lgt[j] = log_fast((tt[j] - lo) * (hi - tt[j]));
                    phl += uon ? fma(scR * tt[j], tt[j], -mu * lgt[j]) : 0.0;
                } else {
                    phl += uon ? fma(scR * tt[j], tt[j], -mu * log_fast((tt[j] - lo) * (hi - tt[j]))) : 0.0;
                }
            }
            if constexpr (RED) {
#pragma unroll
                for (int j = 0; j < NAX; ++j) gzt[j] = 0.0;
            } else {
                const double wt = vz_new(tt);
#pragma unroll
                for (int j = 0; j < NAX; ++j) {
                    gzt[j] = zdefect(fma(al, dz[j], zz[j]), wt, j);
                    thl += xon ? fabs(gzt[j]) : 0.0;
                }
            }
            wsum2(thl, phl);
            th_t = thl; ph_t = phl;
        };
        // filter acceptance of (th_t, ph_t) for the step size al_test (IPOPT alpha_primal_test)
        auto acceptable = [&](double al_test, bool& ft) {
            bool in_filter = !(th_t < th_max) || !isfinite(ph_t);
            in_filter = in_filter || wany_rep(lane < nfilt && th_t >= fth && ph_t >= fph);   // (replicated filter)
            if (in_filter) return false;
            const bool sw = gTd < 0.0 && lg2(al_test) > lg_sw;
            if (theta <= th_min && sw) {
                if (cmp_le(ph_t, phi + eta_ph * al_test * gTd, phi)) { ft = true; return true; }
                return false;
            }
            return cmp_le(th_t, (1 - gam_th) * theta, theta) || cmp_le(ph_t - phi, -gam_ph * theta, phi);
        };
        if (PM_EXPECT(lsm, 0)) {
            direction();
            // constr_mult_init_max: an estimate larger than it (max norm) is discarded (multipliers 0)
            double ym = 0.0;
#pragma unroll
            for (int j = 0; j < NAX; ++j) ym = fmax(ym, xon ? fmax(fabs(dlp[j]), fabs(dlv[j])) : 0.0);
            if (wmax(ym) <= a.mult_init_max) {
#pragma unroll
                for (int j = 0; j < NAX; ++j) { lp[j] += dlp[j]; lv[j] += dlv[j]; }
            }
            continue;
        }
        for (;;) {
            direction();
            if (PM_EXPECT(soc != 0, 0)) { wmin2f(am_lf, az_lf); frac_set(); }
            STAMP(4);
            if (PM_EXPECT(soc == 0, 1)) {
                if constexpr (OVL) {
                    // (the fraction minima alone come first: of the preparation the hand-over needs amax and az only.
                    // The sums, the tiny-step maximum and what follows from them feed the acceptance test after the
                    // first trial, so they are formed behind barrier A, where their reduction no longer stands
                    // between direction() and the helper waves' start; the scheduling barrier there keeps them from
                    // moving back up.  DESIGN §5.R12.)
                    wmin2f(am_lf, az_lf);
                    frac_set();
                    alpha = amax; amain = amax;
                    // The speculative hand-over.  The first trial is the Newton step at alpha = amax, and where it
                    // is accepted (most iterations) the accepted point is this trial point: theta, lambda and z by
                    // the expressions of the accepted update below, operand for operand.  The trial's sine is not
                    // handed over: the helper waves form it from theta as the trial does.  The factor wave starts
                    // on the point here (barrier A), so the trial, the acceptance test, the update, the evaluation
                    // and the mu update all run in its shadow.  This branch runs once per Newton iteration
                    // (soc == 0 is entered with ls == 0 only), always after this iteration's barrier B.
                    const double thc = fma(alpha, dth[0], th[0]);
                    const double il = frcp(thc - lo), iu = frcp(hi - thc);
                    const double zln = pm_clamp_mult(fma(az, dzl[0], zl[0]), mu, il);
                    const double zun = pm_clamp_mult(fma(az, dzu[0], zu[0]), mu, iu);
#ifdef DART_STAMPS
                    {
                        // Newton iterations (slot 18) in which no lane's primal fraction binds (19), no lane's dual
                        // fraction binds (20), neither (21), and no lane's multiplier comes within a factor 2 of a
                        // clamp bound at the hand-over (22): tools/stamps_pmpc_fractions.py, DESIGN §5.R13
                        const double cl = fma(az, dzl[0], zl[0]) * (thc - lo), cu = fma(az, dzu[0], zu[0]) * (hi - thc);
                        const bool near = uon && !(cl >= 2e-10 * mu && cl <= 0.5e10 * mu && cu >= 2e-10 * mu && cu <= 0.5e10 * mu);
                        STAMP_ADD(18, 1);
                        STAMP_ADD(19, am_lf == 1.0f ? 1 : 0);
                        STAMP_ADD(20, az_lf == 1.0f ? 1 : 0);
                        STAMP_ADD(21, am_lf == 1.0f && az_lf == 1.0f ? 1 : 0);
                        STAMP_ADD(22, wany(near) ? 0 : 1);
                    }
#endif
                    __builtin_amdgcn_sched_barrier(0);
                    g_pm_ovl.pt[kPtTh][lane] = thc;
                    g_pm_ovl.pt[kPtLp][lane] = fma(alpha, dlp[0], lp[0]); g_pm_ovl.pt[kPtLv][lane] = fma(alpha, dlv[0], lv[0]);
                    g_pm_ovl.pt[kPtZl][lane] = uon ? zln : 0.0; g_pm_ovl.pt[kPtZu][lane] = uon ? zun : 0.0;
                    g_pm_ovl.pt[kPtP][lane] = fma(alpha, dp[0], p[0]); g_pm_ovl.pt[kPtV][lane] = fma(alpha, dv[0], v[0]);
                    g_pm_ovl.pt[kPtZ][lane] = fma(alpha, dz[0], zz[0]); g_pm_ovl.pt[kPtMu][lane] = mu;
                    __syncthreads();                                        // barrier A
                    __builtin_amdgcn_sched_barrier(0);
                }
                double phil = 0.0, gtdl = 0.0;
#pragma unroll
                for (int j = 0; j < NAX; ++j) {
                    const double ep = p[j] - rp[j], ev = v[j] - rv[j];
                    const double sl = th[j] - lo, su = hi - th[j];
                    phil += xon ? fma(scQp * ep, ep, scQv * ev * ev) : 0.0;
                    gtdl += xon ? fma(qp2 * ep, dp[j], qv2 * ev * dv[j]) : 0.0;
                    // (OVL: sl * su has the bits of the accepted trial's argument, so its logarithm is carried)
                    if constexpr (OVL) phil += uon ? fma(scR * th[j], th[j], -mu * lgc[j]) : 0.0;
                    else phil += uon ? fma(scR * th[j], th[j], -mu * log_fast(sl * su)) : 0.0;
                    gtdl += uon ? rt[j] * dth[j] : 0.0;
                }
                // IPOPT's tiny-step test (max |d|/(1+|x|) < 10 eps_mach accepts the full step unfiltered): its maximum
                // rides with the two sums (one lock-step reduction; two waves: one exchange)
                float tn_w = 0.0f;
#pragma unroll
                for (int j = 0; j < NAX; ++j) {
                    tn_w = fmaxf(tn_w, xon ? fabsf((float)dp[j]) * __builtin_amdgcn_rcpf(1.0f + fabsf((float)p[j])) : 0.0f);
                    tn_w = fmaxf(tn_w, xon ? fabsf((float)dv[j]) * __builtin_amdgcn_rcpf(1.0f + fabsf((float)v[j])) : 0.0f);
                    tn_w = fmaxf(tn_w, xon ? fabsf((float)dz[j]) * __builtin_amdgcn_rcpf(1.0f + fabsf((float)zz[j])) : 0.0f);
                    tn_w = fmaxf(tn_w, uon ? fabsf((float)dth[j]) * __builtin_amdgcn_rcpf(1.0f + fabsf((float)th[j])) : 0.0f);
                }
                // (the fraction minima ride along; OVL: they were reduced ahead of the hand-over, and each chain takes
                // its own steps either way: the same bits)
                if constexpr (OVL) wsum2_maxf(phil, gtdl, tn_w);
                else {
                wsum2_maxf_min2f(phil, gtdl, tn_w, am_lf, az_lf);
                frac_set();
                }
                phi = phil; gTd = gtdl;
                // switching condition alpha (-gTd)^s_ph > delta theta^s_th, compared in log2 space
                const float lg_th = theta > 0.0 ? lg2(theta) : -3.0e38f;
                const float lg_gd = gTd < 0.0 ? lg2(-gTd) : 3.0e38f;
                lg_sw = (float)s_th * lg_th - (float)s_ph * lg_gd;    // log2(theta^s_th / (-gTd)^s_ph)
                amin = gam_th;
                if (gTd < 0.0) amin = fmin(gam_th, fmin(gam_ph * theta * frcp(-gTd), (double)__builtin_amdgcn_exp2f(fmaxf(lg_sw, -126.0f))));
                amin *= gam_al;
                tiny = tn_w < 2.2e-15f;
                alpha = amax; amain = amax;
            } else if (soc > 0) {
                alpha = amax;                 // alpha_soc: fraction to the boundary of the corrected step
            }
            STAMP(5);
            bool again = false;
            if constexpr ((NAX == 2 || kWaves == 2) && !RED) {
                if (PM_EXPECT(in_soft, 0)) break;      // in the soft restoration phase: its step only (below)
                if (PM_EXPECT(soc < 0 && alpha < amin, 0)) break;
            }
            for (;;) {
                trial(alpha);
                bool ft = false;
                if (PM_EXPECT(soc == 0 && tiny, 0)) { accepted = true; ftype = true; break; }
                if (acceptable(soc > 0 ? amain : alpha, ft)) { accepted = true; ftype = ft; break; }
                if (PM_EXPECT(!RED && soc == 0 && ls == 0 && a.max_soc > 0 && !(th_t < theta), 0)) {
                    // first correction: c_soc = alpha c(x) + c(x_trial)
#pragma unroll
                    for (int j = 0; j < NAX; ++j) {
                        g1[j] = fma(alpha, g1[j], g1t[j]); g2[j] = fma(alpha, g2[j], g2t[j]);
                        gz[j] = fma(alpha, gz[j], gzt[j]);
                    }
                    th_old = th_t; soc = 1; again = true;
                    break;
                }
                if (PM_EXPECT(soc > 0, 0)) {
                    if (soc < a.max_soc && th_t <= 0.99 * th_old) {      // next pass: c_soc <- alpha_soc c_soc + c(trial)
#pragma unroll
                        for (int j = 0; j < NAX; ++j) {
                            g1[j] = fma(alpha, g1[j], g1t[j]); g2[j] = fma(alpha, g2[j], g2t[j]);
                            gz[j] = fma(alpha, gz[j], gzt[j]);
                        }
                        th_old = th_t; ++soc; again = true;
                        break;
                    }
                    // the corrections failed: the defects of the current point back (the same
                    // arithmetic as their first evaluation), the Newton step again, backtrack from alpha/2
                    const double w0 = RED ? 0.0 : vz_new(th);
#pragma unroll
                    for (int j = 0; j < NAX; ++j) {
                        defects(p[j], v[j], snc[j], sp[j], sv[j], g1[j], g2[j]);
                        gz[j] = RED ? 0.0 : zdefect(zz[j], w0, j);
                    }
                    // (NAX == 2 or two waves, the soft phase below: always through the loop top, so that a line search that fails
                    // here leaves the plain step in the direction registers; alpha < amin stops it there)
                    soc = -1; ls = 1; alpha = 0.5 * amain;
                    again = ((NAX == 2 || kWaves == 2) && !RED) || !(alpha < amin);
                    break;
                }
                ++ls;
                alpha *= 0.5;
                if (alpha < amin || ls >= 80) break;
            }
            if (!again) break;
        }
        STAMP_ADD(10, ls + 1);
        STAMP_ADD(15, soc > 0 ? 1 : 0);
        STAMP(6);
        // A failed line search: IPOPT's soft restoration phase here (BacktrackingLineSearch::TrySoftRestoStep;
        // oracle/pmpc_ipm.c soft_resto_step), then, if it cannot proceed, the restoration phase proper in
        // pmpc_resto_solve (or status -2 without the phases).  The soft step is the plain primal-dual step damped
        // only by the fractions to the boundary (one length for x, lambda and z); it is taken if the original
        // filter accepts it with alpha_primal_test = 0 (the phase ends) or if it cuts IPOPT's primal-dual system
        // error at mu (the l1 norms of the primal and dual infeasibilities and of z s - mu, added) by 0.9999; at most
        // 10 such steps, and a mu decrease ends the phase.  Only for N > 31 (NAX == 2, two waves), where the restoration solve
        // on the LDS engine (pmpc_resto.h) does not fit: at the default options every PMPC line-search failure there
        // is settled in the soft phase (N = 40: 41 of C4's 1152 instances), which round 4 ended at -2.  For N <= 31
        // the handed-over instance is solved again on the LDS engine, whose sequential arithmetic takes the oracle's
        // iterations exactly; run here, the soft phase measured 87-93 % equal iteration counts on the restored
        // instances and cost C2 5 % (its register allocation; profiles/r05/pmpc_soft_in_register_kernel.txt).
        bool soft = false;
        if (PM_EXPECT(!accepted, 0)) {
            if constexpr (!RED && (NAX == 2 || kWaves == 2)) {
                if (a.soft) {
                    if (!in_soft) {       // PrepareRestoPhaseStart: the current point enters the filter
                        if (nfilt < kWave) {
                            if (lane == nfilt) { fth = (1 - gam_th) * theta; fph = phi - gam_ph * theta; }
                            ++nfilt;
                        }
                        soft_count = 0;
                    }
                    if (!(in_soft && ++soft_count > 10)) {
                        // the fractions to the boundary of the plain step in f64 (the line search's f32 minima
                        // are rounded down by up to 2^-20; a soft step takes them whole, so they are formed exactly)
                        double am = 1.0, a2 = 1.0;
#pragma unroll
                        for (int j = 0; j < NAX; ++j) {
                            if (uon) {
                                const double sl = th[j] - lo, su = hi - th[j];
                                if (dth[j] < 0) am = fmin(am, -tau * sl / dth[j]);
                                if (dth[j] > 0) am = fmin(am, tau * su / dth[j]);
                                if (dzl[j] < 0) a2 = fmin(a2, -tau * zl[j] / dzl[j]);
                                if (dzu[j] < 0) a2 = fmin(a2, -tau * zu[j] / dzu[j]);
                            }
                        }
                        const double as = fmin(wmin(am), wmin(a2));
                        trial(as);
                        bool ft_ = false;
                        const bool orig = acceptable(0.0, ft_);
                        bool take = orig;
                        if (!take && isfinite(ph_t)) {
                            // the primal-dual system error at the point (pass 0) and at the trial with every
                            // multiplier moved by as (pass 1); one code site for both
                            double pd[2];
#pragma unroll 1
                            for (int pass = 0; pass < 2; ++pass) {
                                const double sa = pass ? as : 0.0;
                                double t = 0.0;
#pragma unroll
                                for (int j = 0; j < NAX; ++j) {
                                    const double pp = fma(sa, dp[j], p[j]), vv = fma(sa, dv[j], v[j]);
                                    const double tt = fma(sa, dth[j], th[j]);
                                    const double lpv = fma(sa, dlp[j], lp[j]), lvv = fma(sa, dlv[j], lv[j]);
                                    const double zlv = uon ? fma(sa, dzl[j], zl[j]) : 0.0;
                                    const double zuv = uon ? fma(sa, dzu[j], zu[j]) : 0.0;
                                    const double ga = pass ? g1t[j] : g1[j], gb = pass ? g2t[j] : g2[j];
                                    const double gc = pass ? gzt[j] : gz[j];
                                    const double ln = from_next(lpv), vn = from_next(lvv);
                                    const double lpn_ = uon ? ln : 0.0, lvn_ = uon ? vn : 0.0;
                                    const double r1 = fma(qp2, pp - rp[j], lpv - lpn_);
                                    const double r2x = fma(qv2, vv - rv[j], lvv - fma(a12, lpn_, a22 * lvn_));
                                    const double c_ = tilt_cos_econ(poly, tt);
                                    const double ru = fma(r2, tt, -c_ * fma(b1, lpn_, b2 * lvn_)) - zlv + zuv;
                                    const double sl = tt - lo, su = hi - tt;
                                    t += xon ? fabs(r1) + fabs(r2x) + fabs(ga) + fabs(gb) + fabs(gc) : 0.0;
                                    t += uon ? fabs(ru) + fabs(zlv * sl - mu) + fabs(zuv * su - mu) : 0.0;
                                }
                                pd[pass] = wsum(t);
                            }
                            take = pd[1] <= 0.9999 * pd[0];
                        }
                        if (take) {
                            accepted = true; soft = true; alpha = as; az = as;
                            in_soft = orig ? 0 : 1;
                            if (orig) soft_count = 0;
                        }
                    }
                }
            }
            if (!accepted) { status = a.resto ? kPmNeedResto : -2; break; }
        }
        if (!soft && !ftype && nfilt < kWave) {
            if (lane == nfilt) { fth = (1 - gam_th) * theta; fph = phi - gam_ph * theta; }
            ++nfilt;
        }
        // -------- accept the step ----------------------------------------------------
        // (the quantities the helper waves need come first: a miss of the overlapped build hands them over before the rest)
        // OVL, hit: the step taken is the first trial point, which the helper waves already have and may be reading,
        // so nothing is written to pt and no barrier is crossed; z comes back from this wave's own pt entries (the
        // clamp was evaluated for the hand-over).  Miss (a backtracked step, an accepted correction pass, the Newton
        // step again after failed passes): barrier B first, the factors and the verdict of the rejected trial point
        // are dropped unread, then the accepted point goes over at barrier A as the start point did.
        const bool hit = OVL && soc == 0 && ls == 0;
        if constexpr (OVL) {
            STAMP_ADD(15, hit ? (1ull << 16) : (1ull << 32));      // (stamps build: hits, misses beside the corrections)
            if (PM_EXPECT(!hit, 0)) {
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();                                            // barrier B (discarded round)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            snc[j] = snt[j];
            lp[j] = fma(alpha, dlp[j], lp[j]); lv[j] = fma(alpha, dlv[j], lv[j]);
            th[j] = fma(alpha, dth[j], th[j]);
            if (OVL && PM_EXPECT(hit, 1)) {
                zl[j] = g_pm_ovl.pt[kPtZl][lane]; zu[j] = g_pm_ovl.pt[kPtZu][lane];
            } else {
                const double il = frcp(th[j] - lo), iu = frcp(hi - th[j]);
                const double zln = pm_clamp_mult(fma(az, dzl[j], zl[j]), mu, il);
                const double zun = pm_clamp_mult(fma(az, dzu[j], zu[j]), mu, iu);
                zl[j] = uon ? zln : 0.0; zu[j] = uon ? zun : 0.0;
            }
        }
        if constexpr (OVL) {
            // (the evaluation wave needs p, v and z of the accepted point as well: formed ahead of a miss's hand-over)
            p[0] = fma(alpha, dp[0], p[0]); v[0] = fma(alpha, dv[0], v[0]);
            zz[0] = fma(alpha, dz[0], zz[0]);
            if (PM_EXPECT(!hit, 0)) publish();
        }
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            g1[j] = g1t[j]; g2[j] = g2t[j]; gz[j] = gzt[j];
            if constexpr (OVL) lgc[j] = lgt[j];
            if constexpr (!OVL) {
                p[j] = fma(alpha, dp[j], p[j]); v[j] = fma(alpha, dv[j], v[j]);
                zz[j] = fma(alpha, dz[j], zz[j]);
            }
        }
        theta = th_t;
        STAMP(7);
    }
    if constexpr (OVL) {
        // The exit funnel of the overlapped build.  The iteration loop has no return, and every way out of it
        // (status 0 and status -3 after barrier B and before the line search's barrier A, nothing outstanding; the
        // failed line search with its hand-over to the restoration phases or status -2, after the barrier A of a
        // speculated point that is then not used; max_iter at the loop head, likewise after a barrier A; a loop
        // of no iterations) arrives here.  DESIGN §5.R10 has the table.
        // Invariant: this wave crosses barriers A, B, A, B, ... only in publish() (the first Newton iteration's
        // head, the update of a missed speculation), at the speculative hand-over of the line search (A), at the
        // head of the Riccati block (B) and in the update of a missed speculation (B) (none in the least-square
        // iteration, its `continue` included, in the retries or in the correction passes), then sets the stop word
        // and crosses exactly one more barrier, here.  Each helper wave (helper_rounds, one skeleton for both) crosses
        // a barrier, tests the stop word and goes on to the next barrier, so it meets each of this wave's barriers in
        // turn whatever their role, and leaves at the first test that finds the word set: after the stop barrier at
        // the latest (or earlier, having seen the word before this wave arrived; a terminated wave takes no part in a
        // barrier).  All waves thus execute the same number of barriers up to each helper's end, and nothing below
        // waits for a helper.
        if (lane == 0) g_pm_ovl.flag[kFlStop] = 1;
        __syncthreads();                                                    // the stop barrier
#ifdef DART_STAMPS
        t_acc_[13] = (unsigned)__builtin_amdgcn_readfirstlane(g_pm_ovl.flag[kFlFactorTime]);
        t_acc_[17] = (unsigned)__builtin_amdgcn_readfirstlane(g_pm_ovl.flag[kFlEvalTime]);
#endif
    }

    // -------- outputs ---------------------------------------------------------------
    if (PM_EXPECT(status == kPmNeedResto, 0)) {     // handed over: pmpc_resto_solve writes the outputs
        if constexpr (NAX == 1 && kWaves == 1 && !RED) {
            if (a.resto_buf) {      // the iterate of the failed iteration (pmpc_model.h kPmHo layout)
                double* ho = a.resto_buf + (size_t)kPmHo * b;
                double* row = ho + kPmHoRow * k;
                if (xon) {
                    row[2 * ax0] = p[0]; row[2 * ax0 + 1] = v[0]; row[4 + ax0] = zz[0];
                    row[8 + 2 * ax0] = lp[0]; row[8 + 2 * ax0 + 1] = lv[0]; row[8 + 4 + ax0] = 0.0;
                }
                if (uon) { row[6 + ax0] = th[0]; row[14 + ax0] = zl[0]; row[16 + ax0] = zu[0]; }
                if (lane < nfilt) { ho[kPmHoFilt + 2 * lane] = fth; ho[kPmHoFilt + 2 * lane + 1] = fph; }
                if (lane == 0) {
                    ho[kPmHoScal] = mu; ho[kPmHoScal + 1] = delta_last;
                    ho[kPmHoScal + 2] = (double)it; ho[kPmHoScal + 3] = (double)nfilt;
                }
            }
        }
        if (lane == 0 && wave_idx() == 0) a.status[b] = status;
        if (a.done && a.resto == 2) {
            __threadfence_system();
            if (lane == 0) __hip_atomic_store(a.done + b, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return true;
    }
    // objective (mpc_3d.py:44-46, :63-66), unscaled
    double fl = 0.0;
#pragma unroll
    for (int j = 0; j < NAX; ++j) {
        const double ep = p[j] - rp[j], ev = v[j] - rv[j];
        fl += xon ? Qp * ep * ep + Qv * ev * ev : 0.0;
        fl += uon ? R * th[j] * th[j] : 0.0;
    }
    const double fval = wsum(fl);
    // theta_x and theta_y of this lane's node
    double tx, ty;
    if (NAX == 1) {
        const double other = __shfl_xor(th[0], 32);
        tx = ax0 == 0 ? th[0] : other;
        ty = ax0 == 0 ? other : th[0];
    } else {
        tx = th[0]; ty = th[NAX - 1];
    }
    if (lane == 0 && wave_idx() == 0) {
        a.u0[2 * b] = tx;
        a.u0[2 * b + 1] = ty;
        a.f[b] = fval;
        a.status[b] = status;
        a.iters[b] = it;
    }
    if (a.w_out) {
        double* wo = a.w_out + (size_t)nw * b;
        if constexpr (RED) {
            // the z sub-state follows the final controls through the reference RK4 (mpc_3d.py:93-97, :99-104)
            const double w = uon ? -a.g * (tx * tx + ty * ty) : 0.0;
            double pz = st[4], vz = st[5];
            for (int step = 0; step < N; ++step) {
                double pzn, vzn;
                z_rk4(h, w, pz, vz, pzn, vzn);
                const double ip = from_prev(pzn), iv = from_prev(vzn);
                pz = k >= 1 ? ip : pz; vz = k >= 1 ? iv : vz;
            }
#pragma unroll
            for (int j = 0; j < NAX; ++j) zz[j] = (NAX == 1 ? ax0 : j) ? vz : pz;
        }
#pragma unroll
        for (int j = 0; j < NAX; ++j) {
            const int ax = NAX == 1 ? ax0 : j;
            if (xon) { wo[6 * k + 2 * ax] = p[j]; wo[6 * k + 2 * ax + 1] = v[j]; wo[6 * k + 4 + ax] = zz[j]; }
            if (uon) wo[6 * (N + 1) + 2 * k + ax] = th[j];
        }
    }
    if (a.done) {
        // release at system scope: the wave's output stores (any lane) are visible before the word
        __threadfence_system();
        if constexpr (kWaves == 2) __syncthreads();       // and those of the other wave
        if (lane == 0 && wave_idx() == 0) __hip_atomic_store(a.done + b, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    STAMP(8);
    STAMP_FLUSH(b);
    return false;
}

// IPOPT's restoration phases for instance b in the wave that handed it over (resto mode 3, batches of at
// most 32): a call, not inlined, so that the register kernel keeps its own register allocation; the
// launch arguments are read from the kernel's argument segment (PmpcArgs is the kernel's first argument,
// kernarg_addr; the resident server passes its request's sequence and w_warm / w_out flags, which its waves
// change).  The kernel takes pmpc_resto_solve's LDS (PrShared), which costs nothing at one instance per CU.
__device__ __noinline__ void pmpc_resto_tail(const int b, const uint32_t seq, const uint32_t fl,
                                             const unsigned long long kargs) {
    PmpcArgs a = kernarg_load<PmpcArgs>(kargs);
    a.seq = seq;
    if (!(fl & 1u)) a.w_warm = nullptr;
    if (!(fl & 2u)) a.w_out = nullptr;
    __syncthreads();            // the hand-off's status store (lane 0) is the only prior write
    pmpc_resto_solve(a, b);
}

// F: the build (kScan | kShort2 | ...).  kFuse: resto mode 3, the handed-over instance continues in pmpc_resto_tail
// (no second launch); kOcc2: compiled for two waves per SIMD
template <int NAX, unsigned F>
__global__ __launch_bounds__(kWave * kWaves * ((F & kOvl) ? 3 : 1))
__attribute__((amdgpu_waves_per_eu((F & kOcc2) ? 2 : (((F & kScan) || NAX == 2) ? 1 : 2))))
void pmpc_ipm_kernel(PmpcArgs a) {
    static_assert(F < 2 * kOvl && (!(F & (kOneRow | kShort2 | kOcc2 | kOvl)) || (F & kScan)),
                  "one-row, short-scan, two-waves-per-SIMD and overlapped builds are scan builds");
    static_assert(!(F & kFuse) || !(F & (kRed | kOcc2)), "the fused tail: IPOPT's path at one wave per SIMD");
    constexpr bool ONEROW = (F & kOneRow) != 0;      // (PM_EXPECT)
    // small batches: the launcher deals 8 blocks per instance and only every 8th works, so all
    // instances land on one XCD (blocks go round-robin over the 8 XCDs) and share its L2 for the code
    if (blockIdx.x % a.pack) return;
    const int b = blockIdx.x / a.pack;
    // OVL: launched with three waves; wave 0 solves, wave 1 factors and wave 2 evaluates for it, and both return false
    // when told to stop
    const bool handed = pmpc_solve<NAX, F & ~(kOcc2 | kFuse)>(a, b);
    if constexpr ((F & kFuse) != 0) {
        // OVL: pmpc_resto_tail and pmpc_resto_solve are written for one wave and cross __syncthreads(), real
        // barriers in a three-wave launch.  The solver wave enters here only past the stop barrier of pmpc_solve's
        // exit funnel, after which the helper waves run nothing but their way out of the kernel; a barrier waits only
        // for the waves of the workgroup that have not terminated, so the tail's barriers concern this wave alone.
        if (PM_EXPECT(handed, 0)) pmpc_resto_tail(b, a.seq, 3u, kernarg_addr());
    }
}

// Resident solver (dart_mpc_serve_start): the waves of one launch stay on the GPU and take request
// after request from a mailbox in mapped host memory, so a host call costs no kernel launch, no
// dispatch and no cold instruction cache.  Mailbox: one 64-bit request word written by the host in
// one release store, sequence | batch B << 32 | flags << 48 (bit 0: w_warm given, bit 1: w_out
// wanted) | stop << 56.  Inputs and outputs live at fixed mapped addresses (the PmpcArgs pointers).  Every
// wave leaves the loop on stop or after sv.idle_ticks of s_memrealtime (100 MHz) without a request,
// so the grid always drains.
// FUSE (B_serve <= 32, resto mode 3): a handed-over instance continues in pmpc_resto_tail, so the grid stays
// resident through a restoration
template <int NAX, unsigned F>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(1)))
void pmpc_serve_kernel(PmpcArgs a, PmpcServe sv) {
    static_assert((F & kScan) && !(F & (kRed | kOcc2 | kOvl)), "the server: one-wave scan builds on IPOPT's path");
    constexpr bool ONEROW = (F & kOneRow) != 0;      // (PM_EXPECT)
    if (blockIdx.x % a.pack) return;
    const int b = blockIdx.x / a.pack;
    uint32_t seen = a.seq;
    unsigned long long t_last = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        // one uncached 8-byte read over the link: the request word (sequence | batch << 32 | flags << 48 |
        // stop << 56), written by the host in one store
        const unsigned long long w =
            __hip_atomic_load((const unsigned long long*)sv.mailbox, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w & 0xffffffffu));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
        const uint32_t sq = lo;
        if (hi >> 24) break;                                            // stop
        if (sq == seen) {
            if (__builtin_amdgcn_s_memrealtime() - t_last > sv.idle_ticks) break;
            __builtin_amdgcn_s_sleep(4);
            continue;
        }
        seen = sq;
        const uint32_t B = hi & 0xffffu, fl = (hi >> 16) & 0xffu;
        if ((uint32_t)b < B) {
            PmpcArgs r = a;
            r.B = (int)B; r.seq = sq;
            r.w_warm = (fl & 1u) ? a.w_warm : nullptr;
            r.w_out = (fl & 2u) ? a.w_out : nullptr;
            const bool handed = pmpc_solve<NAX, F & ~kFuse>(r, b);
            if constexpr ((F & kFuse) != 0) {
                if (PM_EXPECT(handed, 0)) pmpc_resto_tail(b, sq, fl, kernarg_addr());
            }
        }
        t_last = __builtin_amdgcn_s_memrealtime();
    }
}

#if !defined(PMPC_SEQ) && DART_WG == 1
// self-test of the wave primitives: out[0..63] = from_next(lane), out[64..127] = from_prev(lane),
// out[128] = wsum(lane), out[129] = wmax(lane), out[130] = wmin(lane + 1),
// out[131..194] = relative error of the raw v_rcp_f64 on x_i = 1.37^(i-32)*pi (diagnostic),
// out[195] = wsumf(lane), out[196] = wmaxf(v), out[197] = wminf(v + 0.5) with v = (37 lane) mod 64,
// out[198] = wmaxf(0 except lane 40: inf), out[199] / out[200] = half_bcast<3>(lane) at lanes 0 / 40,
// out[201..264] = half_pair_sum(lane^2)
__global__ __launch_bounds__(kWave) void wave_selftest_kernel(double* out) {
    const double x = (double)threadIdx.x;
    const double n = from_next(x), p = from_prev(x);
    const double s = wsum(x), mx = wmax(x), mn = wmin(x + 1.0);
    out[threadIdx.x] = n;
    out[64 + threadIdx.x] = p;
    if (threadIdx.x == 0) { out[128] = s; out[129] = mx; out[130] = mn; }
    const double y = 3.141592653589793 * pow(1.37, (double)threadIdx.x - 32.0);
    out[131 + threadIdx.x] = fma(y, __builtin_amdgcn_rcp(y), -1.0);
    const float v = (float)((37 * threadIdx.x) % 64);
    const float sf = wsumf((float)threadIdx.x), mxf = wmaxf(v), mnf = wminf(v + 0.5f);
    const float inf1 = wmaxf(threadIdx.x == 40 ? __builtin_inff() : 0.0f);
    const double hb = half_bcast_c<3>(x);
    if (threadIdx.x == 0) { out[195] = sf; out[196] = mxf; out[197] = mnf; out[198] = inf1; out[199] = hb; }
    if (threadIdx.x == 40) out[200] = hb;
    out[201 + threadIdx.x] = half_pair_sum(x * x);
}

#endif  // PMPC_SEQ

// The launchers launch what a plan names (launch_plan.h: pmpc_plan, pmpc_serve_plan); the two helpers below hold the
// only launches of the two kernels.
struct IpmKernel {
    template <int NAX, unsigned F>
    static hipError_t launch(unsigned grid, unsigned block, hipStream_t stream, const PmpcArgs& a) {
        hipLaunchKernelGGL((pmpc_ipm_kernel<NAX, F>), dim3(grid), dim3(block), 0, stream, a);
        return hipGetLastError();
    }
};
struct ServeKernel {
    template <int NAX, unsigned F>
    static hipError_t launch(unsigned grid, unsigned block, hipStream_t stream, const PmpcArgs& a, const PmpcServe& sv) {
        hipLaunchKernelGGL((pmpc_serve_kernel<NAX, F>), dim3(grid), dim3(block), 0, stream, a, sv);
        return hipGetLastError();
    }
};
// kernel K's instantiation <nax, f> of list L, which is what instantiates the list for this object; a build the
// list does not hold is an error
template <class K, const auto& L, size_t... I, class... A>
static hipError_t launch_build_at(std::index_sequence<I...>, int nax, unsigned f, const A&... args) {
    hipError_t e = hipErrorInvalidValue;
    (void)((L[I].nax == nax && L[I].f == f && (e = K::template launch<L[I].nax, L[I].f>(args...), true)) || ...);
    return e;
}
template <class K, const auto& L, class... A>
static hipError_t launch_build(int nax, unsigned f, const A&... args) {
    return launch_build_at<K, L>(std::make_index_sequence<sizeof(L) / sizeof(L[0])>{}, nax, f, args...);
}

}  // namespace dartmpc

#if DART_WG == 2
// N = 32..63 on IPOPT's path: the scan build, one instance per two-wave workgroup; grid = B x pack blocks as for the
// one-wave builds
extern "C" hipError_t dartmpc_launch_pmpc_wg2(const void* args, int nax, unsigned f, unsigned grid, unsigned block,
                                              hipStream_t stream) {
    return dartmpc::launch_build<dartmpc::IpmKernel, dartmpc::kPmpcWg2Ipm>(
        nax, f, grid, block, stream, *static_cast<const dartmpc::PmpcArgs*>(args));
}
#elif defined(PMPC_SEQ)
// the one-row scan builds (N <= 15) and the sequential (throughput) builds
extern "C" hipError_t dartmpc_launch_pmpc_seq(const dartmpc::PmpcArgs* a, int nax, unsigned f, unsigned grid,
                                              unsigned block, hipStream_t stream) {
    return dartmpc::launch_build<dartmpc::IpmKernel, dartmpc::kPmpcSeqIpm>(nax, f, grid, block, stream, *a);
}
extern "C" hipError_t dartmpc_launch_pmpc_serve_seq(const dartmpc::PmpcArgs* a, const dartmpc::PmpcServe* sv, int nax,
                                                   unsigned f, unsigned grid, unsigned block, hipStream_t stream) {
    return dartmpc::launch_build<dartmpc::ServeKernel, dartmpc::kPmpcSeqServe>(nax, f, grid, block, stream, *a, *sv);
}
#ifdef DART_STAMPS
// diagnostic build only: the stamps of the one-row (N <= 15) and sequential builds of this object
extern "C" hipError_t dartmpc_read_stamps_seq(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(dartmpc::g_stamp_seq), sizeof(unsigned long long) * 32, 0,
                               hipMemcpyDeviceToHost);
}
#endif
#else
extern "C" hipError_t dartmpc_launch_pmpc_seq(const dartmpc::PmpcArgs* a, int nax, unsigned f, unsigned grid,
                                              unsigned block, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_pmpc_serve_seq(const dartmpc::PmpcArgs* a, const dartmpc::PmpcServe* sv, int nax,
                                                   unsigned f, unsigned grid, unsigned block, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_pmpc_wg2(const void* args, int nax, unsigned f, unsigned grid, unsigned block,
                                              hipStream_t stream);

// the resident server for B_serve slots (IPOPT's path, N <= 31)
extern "C" hipError_t dartmpc_launch_pmpc_serve(const dartmpc::PmpcArgs* args, const dartmpc::PmpcServe* sv,
                                               hipStream_t stream) {
    const dartmpc::PmpcPlan p = dartmpc::pmpc_serve_plan(args->N, args->B, args->resto, dartmpc::launch_knobs());
    if (!p.valid) return hipErrorInvalidValue;
    dartmpc::PmpcArgs a = *args;
    a.pack = p.pack;
    a.resto = p.resto;
    const unsigned grid = (unsigned)(a.B * a.pack), block = dartmpc::kWave * p.waves;
    if (p.object == dartmpc::kPmpcSeq) return dartmpc_launch_pmpc_serve_seq(&a, sv, p.nax, p.f, grid, block, stream);
    return dartmpc::launch_build<dartmpc::ServeKernel, dartmpc::kPmpcMainServe>(p.nax, p.f, grid, block, stream, a, *sv);
}

// DART_PMPC_OCC2_MIN_B, or two instances per SIMD of the device that is current at the first use
static int pmpc_occ2_min_b() {
    static const int v = [] {
        if (dartmpc::launch_knobs().occ2_min_b != dartmpc::LaunchKnobs::kNotSet) return dartmpc::launch_knobs().occ2_min_b;
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 0;
        return dartmpc::occ2_min_b_of(cus);
    }();
    return v;
}

extern "C" hipError_t dartmpc_launch_pmpc(const dartmpc::PmpcArgs* args, hipStream_t stream) {
    if (args->B <= 0) return hipSuccess;
    const dartmpc::PmpcPlan p = dartmpc::pmpc_plan(args->N, args->B, args->reduced, args->resto, dartmpc::launch_knobs(),
                                                   pmpc_occ2_min_b());
    if (!p.valid) return hipErrorInvalidValue;
    dartmpc::PmpcArgs a = *args;
    a.pack = p.pack;
    a.resto = p.resto;
    const unsigned grid = (unsigned)(a.B * a.pack), block = dartmpc::kWave * p.waves;
    const hipError_t e =
        p.object == dartmpc::kPmpcSeq   ? dartmpc_launch_pmpc_seq(&a, p.nax, p.f, grid, block, stream)
        : p.object == dartmpc::kPmpcWg2 ? dartmpc_launch_pmpc_wg2(&a, p.nax, p.f, grid, block, stream)
                                        : dartmpc::launch_build<dartmpc::IpmKernel, dartmpc::kPmpcMainIpm>(
                                              p.nax, p.f, grid, block, stream, a);
    if (e != hipSuccess || !p.resto_queued) return e;
    return dartmpc_launch_pmpc_resto(&a, stream);
}

// internal (not part of include/dart_mpc.h), for tests: the plan the launcher of `solver` would use in this process
// for the inputs `in`, as launch_plan.h's plan_query writes it; the number of ints written, -1 for an unknown solver
extern "C" int dartmpc_plan_query(int solver, const int* in, int* out) {
    return dartmpc::plan_query(solver, in, out, dartmpc::launch_knobs(), pmpc_occ2_min_b());
}

// internal (not part of include/dart_mpc.h): runs the wave-primitive self-test into device buffer d_out[131]
extern "C" hipError_t dartmpc_wave_selftest(double* d_out, hipStream_t stream) {
    hipLaunchKernelGGL(dartmpc::wave_selftest_kernel, dim3(1), dim3(dartmpc::kWave), 0, stream, d_out);
    return hipGetLastError();
}

#ifdef DART_STAMPS
// diagnostic build only: per-phase s_memtime cycles of block 0 from the last launch
extern "C" hipError_t dartmpc_read_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(dartmpc::g_stamp), sizeof(unsigned long long) * 32, 0,
                               hipMemcpyDeviceToHost);
}
#endif
#endif  // PMPC_SEQ
