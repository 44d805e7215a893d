// lmpc_train.hip -- the kernels that close the LMPC training loop on the device, gfx950 (lmpc_train.h).
//
// philox_kernel            Philox4x32-10 on given counters and keys (known-answer tests)
// lmpc_noise_kernel        the exploration noise of one iteration: one thread per Philox block, two Box-Muller pairs
// lmpc_perm_kernel         the mini-batch permutations: a thread per element counts the (key, index) pairs below its
//                          own over LDS tiles of 256 keys and writes perm[rank] = i -- the argsort with ties broken on
//                          the index, deterministic without a sort (n is a few thousand)
// iota_kernel              the sample list 0 .. n-1
// lmpc_mean_update_kernel  rlmpc2.py:876-896, one wave64 per controller: the actor's mean on the current history in
//                          policy_step_wave's accumulation order (four fmaf chains in layer 1, two in layers 2 and 3,
//                          tanhf: the policy kernel's mean bit for bit; a third copy of that order next to
//                          lmpc_experience_kernel's, because policy_step_wave itself also advances the Welford state,
//                          the history and the timestep), then policy_step_wave's logit-space update (fp32), EMA and
//                          tanh soft clip (fp64) applied unconditionally, and current_k <- model_params (:896)
// lmpc_train_log_kernel    one workgroup: the iteration's log row (fp64 sums in a fixed order: a strided partial per
//                          thread, then a tree over LDS) and the best-policy snapshot
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_train.h"

namespace dartmpc {

namespace {

constexpr int kRngThreads = 256;
constexpr int kLogThreads = 1024;
constexpr int kObsN = PolicyArgs::kHist * PB;       // 520

__global__ __launch_bounds__(kRngThreads) void philox_kernel(PhiloxArgs a) {
    const int i = blockIdx.x * kRngThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t* q = a.in + 6 * (size_t)i;
    const Philox4 r = philox4x32_10(q[0], q[1], q[2], q[3], q[4], q[5]);
#pragma unroll
    for (int j = 0; j < 4; ++j) a.out[4 * (size_t)i + j] = r.w[j];
}

__device__ inline float unit_open(uint32_t r) {     // in (0, 1), exact in fp32
    return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-7f;
}

__global__ __launch_bounds__(kRngThreads) void lmpc_noise_kernel(NoiseArgs a) {
    const long long c = (long long)blockIdx.x * kRngThreads + threadIdx.x;
    if (4 * c >= a.n) return;
    const Philox4 r = philox4x32_10((uint32_t)c, a.iteration, kStreamNoise, 0u, a.key0, a.key1);
    float z[4];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float rad = sqrtf(-2.0f * logf(unit_open(r.w[2 * p])));
        float sn, cs;
        sincospif(2.0f * unit_open(r.w[2 * p + 1]), &sn, &cs);
        z[2 * p] = rad * cs;
        z[2 * p + 1] = rad * sn;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * c + j < a.n) a.out[4 * c + j] = z[j];
}

__device__ inline uint32_t perm_key(const PermArgs& a, int i, uint32_t epoch) {
    const Philox4 r = philox4x32_10((uint32_t)(i >> 2), a.iteration, kStreamPerm, epoch, a.key0, a.key1);
    return r.w[i & 3];
}

__global__ __launch_bounds__(kRngThreads) void lmpc_perm_kernel(PermArgs a) {
    __shared__ uint32_t tile[kRngThreads];
    const int t = threadIdx.x;
    const int i = blockIdx.x * kRngThreads + t;
    const uint32_t e = blockIdx.y;
    const bool live = i < a.n;
    const uint32_t mine = live ? perm_key(a, i, e) : 0u;
    int rank = 0;
    for (int j0 = 0; j0 < a.n; j0 += kRngThreads) {      // block-uniform trip count
        const int j = j0 + t;
        tile[t] = j < a.n ? perm_key(a, j, e) : 0u;
        __syncthreads();
        const int m = a.n - j0 < kRngThreads ? a.n - j0 : kRngThreads;
        if (live)
            for (int q = 0; q < m; ++q) {
                const uint32_t k = tile[q];
                rank += (k < mine || (k == mine && j0 + q < i)) ? 1 : 0;
            }
        __syncthreads();
    }
    if (live) {
        a.perm[(size_t)e * a.n + rank] = i;              // rank < n: at most n - 1 pairs lie below
        if (a.key_out) a.key_out[(size_t)e * a.n + i] = mine;
    }
}

__global__ __launch_bounds__(kRngThreads) void iota_kernel(IotaArgs a) {
    const int i = blockIdx.x * kRngThreads + threadIdx.x;
    if (i < a.n) a.out[i] = i;
}

struct MeanLds {
    float obs[kObsN];
    float h1[PH], h2[PH];
};

__global__ __launch_bounds__(64) void lmpc_mean_update_kernel(MeanUpdateArgs a) {
    __shared__ MeanLds L;
    const int l = threadIdx.x;
    const int b = blockIdx.x;
    if (b >= a.B) return;                    // block-uniform
    const PolicyWeights& W = a.w;
    const float* hist = a.history + (size_t)kObsN * b;
    for (int e = l; e < kObsN; e += 64) L.obs[e] = hist[e];
    __syncthreads();
    // ---- mean_net (fp32) in policy_step_wave's order: lane j owns hidden unit j --------------------------------
    {
        float s0 = W.b1[l], s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        static_assert(kObsN % 4 == 0, "layer 1 has no tail");
        for (int i = 0; i < kObsN; i += 4) {
            s0 = fmaf(W.W1[(i + 0) * PH + l], L.obs[i + 0], s0);
            s1 = fmaf(W.W1[(i + 1) * PH + l], L.obs[i + 1], s1);
            s2 = fmaf(W.W1[(i + 2) * PH + l], L.obs[i + 2], s2);
            s3 = fmaf(W.W1[(i + 3) * PH + l], L.obs[i + 3], s3);
        }
        L.h1[l] = tanhf((s0 + s1) + (s2 + s3));
    }
    __syncthreads();
    {
        float s0 = W.b2[l], s1 = 0.0f;
#pragma unroll 8
        for (int i = 0; i < PH; i += 2) {
            s0 = fmaf(W.W2[i * PH + l], L.h1[i], s0);
            s1 = fmaf(W.W2[(i + 1) * PH + l], L.h1[i + 1], s1);
        }
        L.h2[l] = tanhf(s0 + s1);
    }
    __syncthreads();
    if (l < PA) {
        float s0 = W.b3[l], s1 = 0.0f;
#pragma unroll 8
        for (int i = 0; i < PH; i += 2) {
            s0 = fmaf(W.W3[i * PA + l], L.h2[i], s0);
            s1 = fmaf(W.W3[(i + 1) * PA + l], L.h2[i + 1], s1);
        }
        const float raw = s0 + s1;           // zero noise: the action is the mean
        if (a.mean_out) a.mean_out[PA * b + l] = raw;
        // ---- logit-space update (fp32) + EMA + soft clip (fp64), as policy_step_wave -------------------------
        const double prev = a.model_params[PA * b + l];
        const float kmax = (float)a.k_max;
        const float minf = (float)(a.min_k / a.k_max);
        const float frac = fminf(fmaxf((float)prev / kmax, minf), 1.0f - 1e-6f);
        const float zp = logf(frac / (1.0f - frac));
        const float zn = zp + raw * (float)a.max_delta * (float)a.action_scale;
        const float kn = kmax * (1.0f / (1.0f + expf(-zn)));
        const double sm = a.smooth_alpha * (double)kn + (1.0 - a.smooth_alpha) * prev;
        const double lo = a.min_k, hi = a.k_max - a.k_ceiling_margin;
        const double c = 0.5 * (hi + lo), sc = 0.5 * (hi - lo) - 1e-3;
        const double prm = c + sc * tanh((sm - c) / sc);
        a.model_params[PA * b + l] = prm;
        a.current_k[PA * b + l] = prm;
    }
}

// sum / maximum over the workgroup in a fixed tree; the result in every thread
__device__ inline double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = kLogThreads / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

__device__ inline double block_max(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = kLogThreads / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = fmax(sh[t], sh[t + s]);
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(kLogThreads) void lmpc_train_log_kernel(TrainLogArgs a) {
    __shared__ double sh[kLogThreads];
    __shared__ int take;
    const int t = threadIdx.x;
    double ended = 0.0, nadv = 0.0, rsum = 0.0, rmax = -INFINITY, mism = 0.0;
    for (int b = t; b < a.B; b += kLogThreads) {
        const int d = a.episodes[b] - a.ep0[b];
        ended += (double)d;
        if (d > 0) {
            const double r = a.last_return[b];
            nadv += 1.0; rsum += r; rmax = fmax(rmax, r);
        }
        mism += a.nrec[b] != a.R ? 1.0 : 0.0;
    }
    double rew = 0.0, bad = 0.0;
    const long long KB = (long long)a.K * a.B;
    for (long long i = t; i < KB; i += kLogThreads) {
        rew += a.log_reward[i];
        bad += a.log_status[i] != 0 ? 1.0 : 0.0;
    }
    ended = block_sum(ended, sh); nadv = block_sum(nadv, sh); rsum = block_sum(rsum, sh);
    mism = block_sum(mism, sh); rew = block_sum(rew, sh); bad = block_sum(bad, sh);
    rmax = block_max(rmax, sh);
    if (t == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        double best = a.best_return[0];
        // (a NaN return never exceeds anything)
        const int snap = (a.track_best && nadv > 0.0 && rmax > best) ? 1 : 0;
        if (snap) {
            best = rmax;
            a.best_return[0] = best;
            a.best_iter[0] = a.iteration;
        }
        double* o = a.row;
        o[0] = (double)a.n; o[1] = ended;
        o[2] = nadv > 0.0 ? rsum / nadv : nan;
        o[3] = nadv > 0.0 ? rmax : nan;
        o[4] = KB > 0 ? rew / (double)KB : nan;
        o[5] = KB > 0 ? bad / (double)KB : nan;
        o[6] = a.stats[0]; o[7] = a.stats[1]; o[8] = a.stats[2];
        o[9] = mism; o[10] = best; o[11] = (double)snap;
        take = snap;
    }
    __syncthreads();
    if (take) {
        for (int i = t; i < kPpoActorN; i += kLogThreads) a.best_weights[i] = a.actor[i];
        for (int i = t; i < kPpoCriticN; i += kLogThreads) a.best_weights[kPpoActorN + i] = a.critic[i];
    }
}

inline int blocks_of(long long n, int per) { return (int)((n + per - 1) / per); }

}  // namespace

}  // namespace dartmpc

using namespace dartmpc;

extern "C" hipError_t dartmpc_launch_philox(const PhiloxArgs* a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(philox_kernel, dim3(blocks_of(a->n, kRngThreads)), dim3(kRngThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_noise(const NoiseArgs* a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    const long long nblk = (a->n + 3) / 4;
    hipLaunchKernelGGL(lmpc_noise_kernel, dim3(blocks_of(nblk, kRngThreads)), dim3(kRngThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_perms(const PermArgs* a, hipStream_t s) {
    if (a->n <= 0 || a->epochs <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_perm_kernel, dim3(blocks_of(a->n, kRngThreads), a->epochs), dim3(kRngThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_iota(const IotaArgs* a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_of(a->n, kRngThreads)), dim3(kRngThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_mean_update(const MeanUpdateArgs* a, hipStream_t s) {
    if (a->B <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_mean_update_kernel, dim3(a->B), dim3(64), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_train_log(const TrainLogArgs* a, hipStream_t s) {
    hipLaunchKernelGGL(lmpc_train_log_kernel, dim3(1), dim3(kLogThreads), 0, s, *a);
    return hipGetLastError();
}
