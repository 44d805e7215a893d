// wave_probe.hip -- device probes of the two headers every solver kernel stands on: wave.h (scalar math, DPP
// shifts and reductions, the two-wave LDS exchanges) and ocp_wave.h (the LDS-staged Riccati engine).  Probe
// kernels and their host entries only: nothing here is on a solve's path.  The entries are internal like
// dartmpc_selftest (not in include/dart_mpc.h): host arrays in and out, their own device buffers, the null
// stream.  tests/test_gpu_wave_math.py, test_gpu_wave_primitives.py and test_gpu_ocp_riccati.py compare what
// they return with references that share no code with the kernels.
//
// Built twice (Makefile): wave_probe.o with one wave per instance and wave_probe_wg2.o with -DDART_WG=2, the
// two-wave forms of every primitive and of the engine.  The entry names carry the build's suffix; the second
// build's device symbols sit in their own namespace, as in rmpc_ipm.hip.
#ifndef DART_WG
#define DART_WG 1
#endif
#if DART_WG == 2
#define dartmpc dartmpc_wg2
#define PROBE_ENTRY(name) name##_wg2
#else
#define PROBE_ENTRY(name) name##_wg1
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ocp_wave.h"
#include "wave.h"

namespace dartmpc {

constexpr int kProbeT = kWave * kWaves;       // threads of a primitive / engine probe: one instance
constexpr int kPrimSlots = 128;               // result rows of the primitive probe (kProbeT lanes each)

#if DART_WG == 1
// ---------------------------------------------------------------------------------------------------------
// scalar math: one function per launch (fn and poly are launch-uniform), o0[i] (and o1[i]) = f(x[i])
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void math_probe_kernel(int fn, int poly_i, int n, const double* x, double* o0,
                                                         double* o1) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const bool poly = poly_i != 0;
    const double v = x[i];
    double a = 0.0, b = 0.0;
    switch (fn) {
        case 0: a = frcp(v); break;
        case 1: a = __builtin_amdgcn_rcp(v); break;
        case 2: a = (double)lg2(v); break;
        case 3: a = log_fast(v); break;
        case 4: a = exp_econ(v); break;
        case 5: a = tanh_econ(v); break;
        case 6: sincos_small(v, a, b); break;
        case 7: a = cos_small(v); break;
        case 8: sincos_econ(v, a, b); break;
        case 9: a = cos_econ(v); break;
        case 10: tilt_sincos(poly, v, a, b); break;
        case 11: a = tilt_cos(poly, v); break;
        case 12: tilt_sincos_econ(poly, v, a, b); break;
        default: a = tilt_cos_econ(poly, v); break;
    }
    o0[i] = a;
    o1[i] = b;
}
#endif

// ---------------------------------------------------------------------------------------------------------
// wave primitives: one instance (kWaves waves); d[v][t], f[v][t] (v < 8) the inputs of thread t, p[t] a
// predicate; out[slot][t] the result of every primitive in thread t.  Every call is at workgroup-uniform
// control flow (the two-wave forms contain barriers).  The slot numbers are restated in
// tests/test_gpu_wave_primitives.py.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kProbeT) void prim_probe_kernel(const double* din, const float* fin, const int* pin,
                                                             double* out) {
    const int t = (int)threadIdx.x;
    double d[8];
    float f[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) { d[v] = din[v * kProbeT + t]; f[v] = fin[v * kProbeT + t]; }
    const bool p = pin[t] != 0;
    int slot = 0;
    auto put = [&](double v) { out[slot * kProbeT + t] = v; ++slot; };
    // shifts and broadcasts
    put(from_next(d[0]));                                   // 0
    put(from_prev(d[0]));                                   // 1
    {
        const double x3[3] = {d[0], d[1], d[2]};
        double o3[3];
        from_next_n(x3, o3);
        put(o3[0]); put(o3[1]); put(o3[2]);                 // 2..4
        from_prev_n(x3, o3);
        put(o3[0]); put(o3[1]); put(o3[2]);                 // 5..7
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) put(row_bcast(d[0], i));    // 8..15
#pragma unroll
    for (int i = 0; i < 8; ++i) put(row_bcast_over(d[0], i, d[1]));   // 16..23
#pragma unroll
    for (int i = 0; i < 16; ++i) put(half_bcast(d[0], i));  // 24..39
    {
        double lo, hi;
        half_pair(d[0], lo, hi);
        put(lo); put(hi);                                   // 40, 41
        put(half_pair_sum(d[0]));                           // 42
    }
    // the separate f64 reductions
    put(wsum(d[0])); put(wmax(d[0])); put(wmin(d[0]));      // 43..45
    put(wsum(d[1])); put(wsum(d[2]));                       // 46, 47
    put(wmin(d[1])); put(wmax(d[1])); put(wmax(d[2]));      // 48..50
    put(wsum_rl(d[0])); put(wsum_rl(d[1]));                 // 51, 52
    // the lock-step f64 forms
    { double a = d[0], b = d[1]; wsum2(a, b); put(a); put(b); }                        // 53, 54
    { double a = d[0], b = d[1], c = d[2]; wsum3(a, b, c); put(a); put(b); put(c); }   // 55..57
    { double a = d[0], b = d[1]; wmin2d(a, b); put(a); put(b); }                       // 58, 59
    {
        double m0 = d[0], m1 = d[1], m2 = d[2], mn = d[0], s0 = d[0], s1 = d[1];
        wred_errors_f64(m0, m1, m2, mn, s0, s1);
        put(m0); put(m1); put(m2); put(mn); put(s0); put(s1);                          // 60..65
    }
    {
        double m0 = d[0], m1 = d[1], m2 = d[2], mn = d[0], s0 = d[0], s1 = d[1];
        wred_errors_f64_rl(m0, m1, m2, mn, s0, s1);
        put(m0); put(m1); put(m2); put(mn); put(s0); put(s1);                          // 66..71
    }
    { double a = d[0], b = d[1]; wsum2_rl(a, b); put(a); put(b); }                     // 72, 73
    // the separate f32 reductions (f[0..3] non-negative)
    put((double)wsumf(f[0])); put((double)wmaxf(f[0])); put((double)wminf(f[0]));      // 74..76
    put((double)wsumf(f[1])); put((double)wmaxf(f[1])); put((double)wminf(f[1]));      // 77..79
    put((double)wmaxf(f[2])); put((double)wmaxf(f[3]));                                // 80, 81
    // the lock-step forms with f32 members
    { float a = f[0], b = f[1]; wmin2f(a, b); put((double)a); put((double)b); }        // 82, 83
    { double a = d[0], b = d[1]; float m = f[0]; wsum2_maxf(a, b, m); put(a); put(b); put((double)m); }   // 84..86
    {
        double a = d[0], b = d[1];
        float m = f[0], n0 = f[0], n1 = f[1];
        wsum2_maxf_min2f(a, b, m, n0, n1);
        put(a); put(b); put((double)m); put((double)n0); put((double)n1);              // 87..91
    }
    {
        float m0 = f[0], m1 = f[1], m2 = f[2], mn = f[0], s0 = f[0], s1 = f[1];
        wred_errors(m0, m1, m2, mn, s0, s1);
        put((double)m0); put((double)m1); put((double)m2); put((double)mn); put((double)s0); put((double)s1);   // 92..97
    }
    {
        float m0 = f[0], m1 = f[1], m2 = f[2], m3 = f[3], mn = f[0], s0 = f[0], s1 = f[1];
        wred_errors4(m0, m1, m2, m3, mn, s0, s1);
        put((double)m0); put((double)m1); put((double)m2); put((double)m3); put((double)mn);
        put((double)s0); put((double)s1);                                              // 98..104
    }
    { double a = d[0], b = d[1]; float m = f[0]; wsum2_rl_maxf(a, b, m); put(a); put(b); put((double)m); }   // 105..107
    put(wany(p) ? 1.0 : 0.0);                                                          // 108
    // the NaN and signed-zero cases of the f32 maxima / minima go through f[4], f[5] (any bit patterns)
    put((double)wmaxf(f[4])); put((double)wminf(f[4]));                                // 109, 110
    put((double)wmaxf(f[5])); put((double)wminf(f[5]));                                // 111, 112
    put(wmax(d[3])); put(wmin(d[3]));                                                  // 113, 114
#if DART_WG == 2
    {
        // wg_errors on its own: the wave-uniform inputs are lane 0's values of each wave
        float m0 = readlanef(f[0], 0), m1 = readlanef(f[1], 0), m2 = readlanef(f[2], 0), m3 = readlanef(f[3], 0);
        float mn = readlanef(f[1], 0), s0 = readlanef(f[0], 0), s1 = readlanef(f[1], 0);
        wg_errors(m0, m1, m2, &m3, mn, s0, s1);
        put((double)m0); put((double)m1); put((double)m2); put((double)m3); put((double)mn);
        put((double)s0); put((double)s1);                                              // 115..121
    }
#endif
    static_assert(122 <= kPrimSlots, "result rows");
}

// ---------------------------------------------------------------------------------------------------------
// Riccati engine, instantiated as the solvers do: the host passes whole images of the M, H and G node arrays
// (NodeArr strides) and dx~_0; the probe runs sweep -> closed loop -> forward sweep -> multipliers and
// returns the G image, the sweep's flag of every thread and per node dx~, du = [K | k][dx~; 1], lam~.
// ---------------------------------------------------------------------------------------------------------
using AugLds = OcpLds<6, 32 * kWaves>;
using SLds = OcpLdsS<5, 32 * kWaves>;
struct SShared {
    SLds S;
    alignas(16) double Ps[2][SLds::NTP];      // the explicit value function of riccati_s_sweep_p
};
constexpr int kAugM = (int)(sizeof(AugLds::M) / sizeof(double)), kAugG = (int)(sizeof(AugLds::G) / sizeof(double));
constexpr int kSM = (int)(sizeof(SLds::M) / sizeof(double)), kSG = (int)(sizeof(SLds::G) / sizeof(double));
static_assert(sizeof(AugLds::H) == sizeof(AugLds::G) && sizeof(SLds::H) == sizeof(SLds::G), "H and G images alike");
static_assert(sizeof(AugLds) + 1024 <= 160 * 1024 && sizeof(SShared) + 1024 <= 160 * 1024, "fits the LDS of a CU");

__global__ __launch_bounds__(kProbeT) void riccati_aug_probe_kernel(int N, const double* Mi, const double* Hi,
                                                                    const double* Gi, const double* dx0, double* Go,
                                                                    double* dxo, double* duo, double* lamo, int* oko) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    AugLds* S = reinterpret_cast<AugLds*>(smem);
    constexpr int NXA = AugLds::NXA;
    const int t = (int)threadIdx.x;
    for (int i = t; i < kAugM; i += kProbeT) S->M.buf[i] = Mi[i];
    for (int i = t; i < kAugG; i += kProbeT) { S->H.buf[i] = Hi[i]; S->G.buf[i] = Gi[i]; }
    if (t < AugLds::NC) S->dx0[t] = t < NXA ? dx0[t] : 0.0;
    __syncthreads();
    const bool ok = riccati_sweep_aug(S, N);
    closed_loop(S, N);
    const int k = node_base() + (lane_id() & 31);
    const bool xon = k <= N, uon = k < N;
    double dx[NXA], dU[2], lam[NXA];
    forward_sweep(S, N, k, dx);
    {
        const double* K0 = S->KK[uon ? k : 0][0];
        const double* K1 = S->KK[uon ? k : 0][1];
        double d0 = K0[NXA], d1 = K1[NXA];
#pragma unroll
        for (int j = 0; j < NXA; ++j) { d0 = fma(K0[j], dx[j], d0); d1 = fma(K1[j], dx[j], d1); }
        dU[0] = uon ? d0 : 0.0; dU[1] = uon ? d1 : 0.0;
        node_multiplier(S, xon ? k : 0, dx, dU, lam);
    }
    if (lane_id() < 32 && xon) {
#pragma unroll
        for (int j = 0; j < NXA; ++j) { dxo[k * NXA + j] = dx[j]; lamo[k * NXA + j] = lam[j]; }
        duo[k * 2] = dU[0]; duo[k * 2 + 1] = dU[1];
    }
    oko[t] = ok ? 1 : 0;
    __syncthreads();
    for (int i = t; i < kAugG; i += kProbeT) Go[i] = S->G.buf[i];
}

template <bool PFORM>
__global__ __launch_bounds__(kProbeT) void riccati_s_probe_kernel(int N, const double* Mi, const double* Hi,
                                                                  const double* Gi, const double* dx0, double* Go,
                                                                  double* dxo, double* duo, double* lamo, int* oko) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SShared* SH = reinterpret_cast<SShared*>(smem);
    SLds* S = &SH->S;
    constexpr int NXA = SLds::NXA, NMAXS = SLds::NMAXS;
    const int t = (int)threadIdx.x;
    for (int i = t; i < kSM; i += kProbeT) S->M.buf[i] = Mi[i];
    for (int i = t; i < kSG; i += kProbeT) { S->H.buf[i] = Hi[i]; S->G.buf[i] = Gi[i]; }
    if (t < 2 * SLds::NC) {
        const int h = t / SLds::NC, j = t - h * SLds::NC;
        S->dx0[h][j] = j < NXA ? dx0[h * NXA + j] : 0.0;
    }
    if (t < 2 * SLds::NTP) SH->Ps[t / SLds::NTP][t % SLds::NTP] = 0.0;
    __syncthreads();
    const RiccatiSRoles RR = riccati_s_roles<SLds>();
    bool ok;
    if constexpr (PFORM) ok = riccati_s_sweep_p(S, SH->Ps, N, RR);
    else ok = riccati_s_sweep(S, N, RR);
    closed_loop_s(S, N);
    const int hf = lane_id() >> 5, k = node_base() + (lane_id() & 31), sl = hf * NMAXS + k;
    const bool xon = k <= N, uon = k < N;
    double dx[NXA], lam[NXA];
    forward_sweep_s(S, N, k, dx);
    const double* K = S->KK[uon ? sl : hf * NMAXS];
    double d0 = K[NXA];
#pragma unroll
    for (int j = 0; j < NXA; ++j) d0 = fma(K[j], dx[j], d0);
    const double dU = uon ? d0 : 0.0;
    node_multiplier_s(S, xon ? sl : hf * NMAXS, dx, dU, lam);
    if (xon) {
#pragma unroll
        for (int j = 0; j < NXA; ++j) { dxo[sl * NXA + j] = dx[j]; lamo[sl * NXA + j] = lam[j]; }
        duo[sl] = dU;
    }
    oko[t] = ok ? 1 : 0;
    __syncthreads();
    for (int i = t; i < kSG; i += kProbeT) Go[i] = S->G.buf[i];
}

}  // namespace dartmpc

namespace {

// device copies of a probe call's host arrays, freed at scope exit
struct ProbeBufs {
    static constexpr int kMax = 12;
    void* dev[kMax] = {};
    void* host[kMax] = {};
    size_t bytes[kMax] = {};
    int n = 0;
    hipError_t err = hipSuccess;
    template <class T>
    T* in(const T* h, size_t count) {
        T* d = out(const_cast<T*>(h), count);
        host[n - 1] = nullptr;
        if (err == hipSuccess) err = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    T* out(T* h, size_t count) {
        void* d = nullptr;
        if (n >= kMax) { err = hipErrorInvalidValue; return nullptr; }
        if (err == hipSuccess) err = hipMalloc(&d, count * sizeof(T));
        if (err == hipSuccess) err = hipMemset(d, 0, count * sizeof(T));
        dev[n] = d; host[n] = h; bytes[n] = count * sizeof(T);
        ++n;
        return static_cast<T*>(d);
    }
    int finish() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (int i = 0; i < n; ++i)
            if (err == hipSuccess && host[i]) err = hipMemcpy(host[i], dev[i], bytes[i], hipMemcpyDeviceToHost);
        return err == hipSuccess ? 0 : -2;
    }
    ~ProbeBufs() {
        for (int i = 0; i < n; ++i)
            if (dev[i]) (void)hipFree(dev[i]);
    }
};

}  // namespace

#if DART_WG == 1
// o0[n], o1[n] = the function fn of x[n] (fn as in math_probe_kernel; o1 the cosine of the sincos forms)
extern "C" int dartmpc_probe_math(int fn, int poly, int n, const double* x, double* o0, double* o1) {
    if (n <= 0 || fn < 0 || fn > 13) return -1;
    ProbeBufs B;
    const double* dx = B.in(x, (size_t)n);
    double* d0 = B.out(o0, (size_t)n);
    double* d1 = B.out(o1, (size_t)n);
    if (B.err == hipSuccess)
        hipLaunchKernelGGL(dartmpc::math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, fn, poly,
                           n, dx, d0, d1);
    return B.finish();
}
#endif

// layout of the build's probes: [threads, result rows of the primitive probe, doubles of the aug M image, of the
// aug H / G image, of the S M image, of the S H / G image, node slots of the aug arrays, node slots per half of
// the S arrays, bytes of the aug LDS struct, bytes of the S LDS struct]
extern "C" void PROBE_ENTRY(dartmpc_probe_layout)(int* o) {
    o[0] = dartmpc::kProbeT; o[1] = dartmpc::kPrimSlots;
    o[2] = dartmpc::kAugM; o[3] = dartmpc::kAugG; o[4] = dartmpc::kSM; o[5] = dartmpc::kSG;
    o[6] = dartmpc::AugLds::NMAXS; o[7] = dartmpc::SLds::NMAXS;
    o[8] = (int)sizeof(dartmpc::AugLds); o[9] = (int)sizeof(dartmpc::SLds);
}

// d[8][T], f[8][T], p[T] -> out[kPrimSlots][T] (T = 64 waves-per-instance threads)
extern "C" int PROBE_ENTRY(dartmpc_probe_prims)(const double* d, const float* f, const int* p, double* out) {
    constexpr size_t T = dartmpc::kProbeT;
    ProbeBufs B;
    const double* dd = B.in(d, 8 * T);
    const float* df = B.in(f, 8 * T);
    const int* dp = B.in(p, T);
    double* dout = B.out(out, dartmpc::kPrimSlots * T);
    if (B.err == hipSuccess)
        hipLaunchKernelGGL(dartmpc::prim_probe_kernel, dim3(1), dim3(dartmpc::kProbeT), 0, nullptr, dd, df, dp, dout);
    return B.finish();
}

template <class Kern>
static int riccati_probe_launch(Kern kern, size_t lds, int N, int nmaxs, int msz, int gsz, int nslots, int nxa, int nu,
                                const double* M, const double* H, const double* G, const double* dx0, int ndx0,
                                double* Go, double* dx, double* du, double* lam, int* ok) {
    if (N < 1 || N + 1 > nmaxs) return -1;
    ProbeBufs B;
    const double* dM = B.in(M, (size_t)msz);
    const double* dH = B.in(H, (size_t)gsz);
    const double* dG = B.in(G, (size_t)gsz);
    const double* d0 = B.in(dx0, (size_t)ndx0);
    double* dGo = B.out(Go, (size_t)gsz);
    double* ddx = B.out(dx, (size_t)nslots * nxa);
    double* ddu = B.out(du, (size_t)nslots * nu);
    double* dlam = B.out(lam, (size_t)nslots * nxa);
    int* dok = B.out(ok, (size_t)dartmpc::kProbeT);
    if (B.err == hipSuccess)
        B.err = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (B.err == hipSuccess)
        hipLaunchKernelGGL(kern, dim3(1), dim3(dartmpc::kProbeT), lds, nullptr, N, dM, dH, dG, d0, dGo, ddx, ddu, dlam, dok);
    return B.finish();
}

// OcpLds<6, 32 waves>: M, H, G the images of the node arrays, dx0[6]; Go the G image after the sweep, dx[NMAXS][6],
// du[NMAXS][2], lam[NMAXS][6] (rows past N untouched: zero), ok[T] the sweep's flag in every thread
extern "C" int PROBE_ENTRY(dartmpc_probe_riccati_aug)(int N, const double* M, const double* H, const double* G,
                                                      const double* dx0, double* Go, double* dx, double* du, double* lam,
                                                      int* ok) {
    using L = dartmpc::AugLds;
    return riccati_probe_launch(dartmpc::riccati_aug_probe_kernel, sizeof(L), N, L::NMAXS, dartmpc::kAugM, dartmpc::kAugG,
                                L::NMAXS, L::NXA, 2, M, H, G, dx0, L::NXA, Go, dx, du, lam, ok);
}

// OcpLdsS<5, 32 waves>, two subsystems (slot NMAXS h + k): dx0[2][5]; dx[2 NMAXS][5], du[2 NMAXS], lam[2 NMAXS][5];
// pform: riccati_s_sweep_p instead of riccati_s_sweep
extern "C" int PROBE_ENTRY(dartmpc_probe_riccati_s)(int pform, int N, const double* M, const double* H, const double* G,
                                                    const double* dx0, double* Go, double* dx, double* du, double* lam,
                                                    int* ok) {
    using L = dartmpc::SLds;
    if (pform)
        return riccati_probe_launch(dartmpc::riccati_s_probe_kernel<true>, sizeof(dartmpc::SShared), N, L::NMAXS,
                                    dartmpc::kSM, dartmpc::kSG, 2 * L::NMAXS, L::NXA, 1, M, H, G, dx0, 2 * L::NXA, Go, dx,
                                    du, lam, ok);
    return riccati_probe_launch(dartmpc::riccati_s_probe_kernel<false>, sizeof(dartmpc::SShared), N, L::NMAXS,
                                dartmpc::kSM, dartmpc::kSG, 2 * L::NMAXS, L::NXA, 1, M, H, G, dx0, 2 * L::NXA, Go, dx, du,
                                lam, ok);
}
