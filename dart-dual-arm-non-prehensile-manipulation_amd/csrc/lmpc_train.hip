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
// lmpc_gbuf_append_kernel  rlmpc2.py:823-827, one workgroup per drawn record: the record's six fields into the next
//                          row of the global buffer, bit for bit, the observation in 16-byte moves
// lmpc_gae_seq_kernel      compute_gae (:592-599) over the global buffer as one chain (:834): one workgroup, a suffix
//                          scan of affine maps in tiles of 1024 rows (shuffles in the wave, LDS across the waves)
// lmpc_global_log_kernel   one row of global_log
//
// A population of P learners (dart_lmpc_train_pop_dev; instance i = l B + b) runs in the launches of one:
// lmpc_noise_pop_kernel / lmpc_perm_pop_kernel take the learner from the grid and its generator key from the launch
// arguments, lmpc_pop_sample_kernel writes the per-learner sample lists, lmpc_mean_update_kernel<true> reads the actor
// of learner b / learner_B, and lmpc_train_log_pop_kernel is one workgroup per learner that visits its entries of the
// stacked logs in the single run's flat order, so that every fp64 sum has the single run's order.  The kernels of
// one learner are untouched instantiations: the bodies are shared, the arguments moved to the learner.
//
// The population's global-buffer update (dart_lmpc_train_pop_global_dev; P buffers stacked `capacity` rows apart):
// lmpc_perm_pop_kernel with limit = m draws every learner's choice, lmpc_gbuf_append_pop_kernel (grid (m, P)),
// lmpc_gae_seq_kernel<GaeSeqPopArgs> (a workgroup per learner) and lmpc_global_log_pop_kernel run the single
// kernels' bodies on the learner's rows, and lmpc_pop_global_sample_kernel writes the sample lists l capacity + i
// through which the update's population kernels reach the buffers' rows and adv / ret [P][capacity].
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

// the four draws of Philox block c of (key, iteration)
__device__ __forceinline__ void noise_block(uint32_t c, uint32_t iteration, uint32_t key0, uint32_t key1, float z[4]) {
    const Philox4 r = philox4x32_10(c, iteration, kStreamNoise, 0u, key0, key1);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float rad = sqrtf(-2.0f * logf(unit_open(r.w[2 * p])));
        float sn, cs;
        sincospif(2.0f * unit_open(r.w[2 * p + 1]), &sn, &cs);
        z[2 * p] = rad * cs;
        z[2 * p + 1] = rad * sn;
    }
}

__global__ __launch_bounds__(kRngThreads) void lmpc_noise_kernel(NoiseArgs a) {
    const long long c = (long long)blockIdx.x * kRngThreads + threadIdx.x;
    if (4 * c >= a.n) return;
    float z[4];
    noise_block((uint32_t)c, a.iteration, a.key0, a.key1, z);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * c + j < a.n) a.out[4 * c + j] = z[j];
}

// grid (blocks, P): learner y's generator; a block's four elements may lie in two instance rows (34 = 4 * 8 + 2)
__global__ __launch_bounds__(kRngThreads) void lmpc_noise_pop_kernel(NoisePopArgs a) {
    const long long c = (long long)blockIdx.x * kRngThreads + threadIdx.x;
    if (4 * c >= a.n) return;
    const int l = blockIdx.y;
    float z[4];
    noise_block((uint32_t)c, a.iteration, a.keys.k[l][0], a.keys.k[l][1], z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long e = 4 * c + j;
        if (e < a.n) {
            const long long row = e / PA, k = row / a.B;         // row = k B + b
            const int col = (int)(e - row * PA), b = (int)(row - k * a.B);
            a.out[((k * a.P + l) * a.B + b) * PA + col] = z[j];
        }
    }
}

__device__ inline uint32_t perm_key(const PermArgs& a, int i, uint32_t epoch) {
    const Philox4 r = philox4x32_10((uint32_t)(i >> 2), a.iteration, a.stream, epoch, a.key0, a.key1);
    return r.w[i & 3];
}

__device__ __forceinline__ void perm_body(const PermArgs& a) {
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
        // rank < n: at most n - 1 pairs lie below; limit = n for the permutations, m for a choice of m
        if (rank < a.limit) a.perm[(size_t)e * a.limit + rank] = i;
        if (a.key_out) a.key_out[(size_t)e * a.n + i] = mine;
    }
}

__global__ __launch_bounds__(kRngThreads) void lmpc_perm_kernel(PermArgs a) { perm_body(a); }

// grid (ceil(n / 256), epochs, P): learner z's key, its rows of perm [P][epochs][limit]
__global__ __launch_bounds__(kRngThreads) void lmpc_perm_pop_kernel(PermPopArgs p) {
    PermArgs a = p.a;
    const int l = blockIdx.z;
    a.key0 = p.keys.k[l][0]; a.key1 = p.keys.k[l][1];
    a.perm += (size_t)l * a.epochs * a.limit;
    a.key_out = nullptr;
    perm_body(a);
}

// grid (ceil(R B / 256), P)
__global__ __launch_bounds__(kRngThreads) void lmpc_pop_sample_kernel(PopSampleArgs a) {
    const int i = blockIdx.x * kRngThreads + threadIdx.x, l = blockIdx.y;
    const int n = a.R * a.B;
    if (i >= n) return;
    const int r = i / a.B, b = i - r * a.B;
    a.out[(size_t)l * n + i] = (r * a.P + l) * a.B + b;
}

__global__ __launch_bounds__(kRngThreads) void iota_kernel(IotaArgs a) {
    const int i = blockIdx.x * kRngThreads + threadIdx.x;
    if (i < a.n) a.out[i] = i;
}

struct MeanLds {
    float obs[kObsN];
    float h1[PH], h2[PH];
};

// POP: instance b reads the actor of learner b / learner_B (its own instantiation: the single-policy kernel keeps
// its instructions)
template <bool POP>
__global__ __launch_bounds__(64) void lmpc_mean_update_kernel(MeanUpdateArgs a) {
    __shared__ MeanLds L;
    const int l = threadIdx.x;
    const int b = blockIdx.x;
    if (b >= a.B) return;                    // block-uniform
    const PolicyWeights W = POP ? learner_weights(a.w, b, a.learner_B) : a.w;
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

// ld > 0 (a population): the logs are [K][ld] and this learner's B instances start at column `first`
__device__ __forceinline__ void train_log_body(const TrainLogArgs& a, const int ld, const int first) {
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
        long long at = i;
        if (ld > 0) {
            const long long k = i / a.B;
            at = k * ld + first + (i - k * a.B);
        }
        rew += a.log_reward[at];
        bad += a.log_status[at] != 0 ? 1.0 : 0.0;
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

__global__ __launch_bounds__(kLogThreads) void lmpc_train_log_kernel(TrainLogArgs a) { train_log_body(a, 0, 0); }

__global__ __launch_bounds__(kLogThreads) void lmpc_train_log_pop_kernel(TrainLogPopArgs p) {
    TrainLogArgs a = p.a;
    const size_t l = blockIdx.x, i0 = l * (size_t)a.B;
    a.ep0 += i0; a.episodes += i0; a.last_return += i0; a.nrec += i0;
    a.stats += 3 * l;
    a.actor += l * kPpoActorN; a.critic += l * kPopCriticStride;
    a.row += l * p.row_stride;
    a.best_return += l; a.best_weights += l * (size_t)kPpoParams; a.best_iter += l;
    train_log_body(a, p.P * a.B, (int)i0);
}

constexpr int kAppendThreads = 128;
constexpr int kObsVec = kObsN / 4;                  // 130 16-byte pieces of an observation row
static_assert(kObsN % 4 == 0, "an observation row is a whole number of 16-byte pieces");

__device__ __forceinline__ void gbuf_append_body(const GbufAppendArgs& a) {
    const int j = blockIdx.x, t = threadIdx.x;
    if (j >= a.m) return;                           // block-uniform, as are the two below
    const int c = a.choice[j];
    if (c < 0 || c >= a.n) return;
    const long long src = a.sample[c];
    if (src < 0 || src >= a.rec_total) return;
    const size_t s = (size_t)src, d = (size_t)a.fill + (size_t)j;
    // moves of integer words: no float operation touches a payload
    const uint4* so = reinterpret_cast<const uint4*>(a.rec_obs + s * kObsN);
    uint4* dob = reinterpret_cast<uint4*>(a.obs + d * kObsN);
    for (int e = t; e < kObsVec; e += kAppendThreads) dob[e] = so[e];
    const uint32_t* sa = reinterpret_cast<const uint32_t*>(a.rec_action + s * PA);
    uint32_t* da = reinterpret_cast<uint32_t*>(a.action + d * PA);
    if (t < PA) da[t] = sa[t];
    if (t == 64) reinterpret_cast<uint32_t*>(a.logp)[d] = reinterpret_cast<const uint32_t*>(a.rec_logp)[s];
    if (t == 65) reinterpret_cast<uint32_t*>(a.value)[d] = reinterpret_cast<const uint32_t*>(a.rec_value)[s];
    if (t == 66) reinterpret_cast<uint32_t*>(a.done)[d] = reinterpret_cast<const uint32_t*>(a.rec_done)[s];
    if (t == 67) reinterpret_cast<uint64_t*>(a.reward)[d] = reinterpret_cast<const uint64_t*>(a.rec_reward)[s];
}

__global__ __launch_bounds__(kAppendThreads) void lmpc_gbuf_append_kernel(GbufAppendArgs a) { gbuf_append_body(a); }

// grid (m, P): learner y's sample list and choice, its own buffer `capacity` rows behind the one before
__global__ __launch_bounds__(kAppendThreads) void lmpc_gbuf_append_pop_kernel(GbufAppendPopArgs p) {
    GbufAppendArgs a = p.a;
    const size_t l = blockIdx.y, r0 = l * (size_t)p.capacity;
    a.sample += l * (size_t)a.n; a.choice += l * (size_t)a.m;
    a.obs += r0 * kObsN; a.action += r0 * PA;
    a.logp += r0; a.value += r0; a.reward += r0; a.done += r0;
    gbuf_append_body(a);
}

// grid (ceil(G / 256), P)
__global__ __launch_bounds__(kRngThreads) void lmpc_pop_global_sample_kernel(PopGlobalSampleArgs a) {
    const int i = blockIdx.x * kRngThreads + threadIdx.x, l = blockIdx.y;
    if (i >= a.G) return;
    a.out[(size_t)l * a.G + i] = l * a.capacity + i;
}

constexpr int kSeqThreads = 1024, kSeqWaves = kSeqThreads / 64;

// One workgroup.  Row t is the affine map gae -> delta_t + c_t gae, c_t = gamma lam (1 - done_t); adv_t is the
// composition of the maps of rows t .. G-1 applied to 0.  Tiles of 1024 rows from the last to the first: a
// Hillis-Steele suffix scan in each wave64 (6 levels of shuffles), the 16 wave totals scanned the same way in wave 0
// (4 levels), one composition with the later waves' suffix, and one with the carry, the advantage of the first row
// of the tile behind (0 behind the last tile, where that composition is exact).  Rows past G are the identity map.
//
// One statement of the arithmetic, two entry points: lmpc_gae_seq_kernel<GaeSeqArgs> (one sequence, one workgroup)
// and lmpc_gae_seq_kernel<GaeSeqPopArgs> (a workgroup per learner).  The two are instantiations of the kernel and
// not callers of a shared __forceinline__ body, as the other kernels of this family are: with the tile loop inlined
// from a callee the compiler inverts the loop's exit branch (s_cmp_lg / scc0 for s_cmp_eq / scc1), and the single
// kernel has to keep its instructions; as an instantiation it does.
__device__ __forceinline__ const GaeSeqArgs& seq_args(const GaeSeqArgs& a) { return a; }
// learner blockIdx.x: its rows of the stacked buffers, its bootstrap value
__device__ __forceinline__ GaeSeqArgs seq_args(const GaeSeqPopArgs& p) {
    GaeSeqArgs a = p.a;
    const size_t l = blockIdx.x, r0 = l * (size_t)p.capacity;
    a.reward += r0; a.value += r0; a.done += r0; a.last_value += l;
    a.adv += r0; a.ret += r0;
    return a;
}

template <class Args>
__global__ __launch_bounds__(kSeqThreads) void lmpc_gae_seq_kernel(Args p) {
#pragma clang fp contract(off)
    const GaeSeqArgs a = seq_args(p);
    __shared__ double wa[kSeqWaves], wc[kSeqWaves];
    __shared__ double carry_sh;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int G = a.G;
    const double kappa = a.gamma * a.lam;
    double carry = 0.0;
    for (int tile = (G - 1) / kSeqThreads; tile >= 0; --tile) {      // block-uniform trip count
        const int i = tile * kSeqThreads + t;
        const bool live = i < G;
        double A = 0.0, C = 1.0, v = 0.0;
        if (live) {
            v = (double)a.value[i];
            const double nd = 1.0 - (double)a.done[i];
            const double v_next = i + 1 < G ? (double)a.value[i + 1] : (double)a.last_value[0];
            A = a.reward[i] + a.gamma * v_next * nd - v;             // delta_t, in lmpc_gae_kernel's order
            C = kappa * nd;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double a2 = __shfl_down(A, d), c2 = __shfl_down(C, d);
            if (lane + d < 64) { A = A + C * a2; C = C * c2; }
        }
        if (lane == 0) { wa[w] = A; wc[w] = C; }
        __syncthreads();
        if (w == 0) {
            double ta = lane < kSeqWaves ? wa[lane] : 0.0, tc = lane < kSeqWaves ? wc[lane] : 1.0;
#pragma unroll
            for (int d = 1; d < kSeqWaves; d <<= 1) {
                const double a2 = __shfl_down(ta, d), c2 = __shfl_down(tc, d);
                if (lane + d < kSeqWaves) { ta = ta + tc * a2; tc = tc * c2; }
            }
            // exclusive: wave l takes the composition of waves l + 1 .. 15
            const double ea = __shfl_down(ta, 1), ec = __shfl_down(tc, 1);
            if (lane < kSeqWaves) {
                wa[lane] = lane + 1 < kSeqWaves ? ea : 0.0;
                wc[lane] = lane + 1 < kSeqWaves ? ec : 1.0;
            }
        }
        __syncthreads();
        const double behind = wa[w] + wc[w] * carry;                 // the advantage of the next wave's first row
        const double g = A + C * behind;
        if (live) {
            a.adv[i] = g;
            a.ret[i] = g + v;
        }
        if (t == 0) carry_sh = g;
        __syncthreads();                                             // (also: wa / wc are free for the next tile)
        carry = carry_sh;
    }
}

__device__ __forceinline__ void global_log_body(const GlobalLogArgs& a) {
    const int t = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (t == 0) a.row[0] = (double)a.fill;
    if (t == 1) a.row[1] = (double)a.ran;
    if (t == 2) a.row[2] = (double)a.G;
    if (t >= 3 && t < kGlobalLogCols) a.row[t] = a.ran ? a.stats[t - 3] : nan;
}

__global__ __launch_bounds__(64) void lmpc_global_log_kernel(GlobalLogArgs a) { global_log_body(a); }

// one workgroup per learner: its row of global_log [P][iterations][6], its statistics of stats [P][3]
__global__ __launch_bounds__(64) void lmpc_global_log_pop_kernel(GlobalLogPopArgs p) {
    GlobalLogArgs a = p.a;
    const size_t l = blockIdx.x;
    a.stats += 3 * l;
    a.row += l * p.row_stride;
    global_log_body(a);
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
    if (a->learner_B > 0) hipLaunchKernelGGL(lmpc_mean_update_kernel<true>, dim3(a->B), dim3(64), 0, s, *a);
    else hipLaunchKernelGGL(lmpc_mean_update_kernel<false>, dim3(a->B), dim3(64), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_noise_pop(const NoisePopArgs* a, hipStream_t s) {
    if (a->n <= 0 || a->P <= 0) return hipSuccess;
    const long long nblk = (a->n + 3) / 4;
    hipLaunchKernelGGL(lmpc_noise_pop_kernel, dim3(blocks_of(nblk, kRngThreads), a->P), dim3(kRngThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_perms_pop(const PermPopArgs* a, hipStream_t s) {
    if (a->a.n <= 0 || a->a.epochs <= 0 || a->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_perm_pop_kernel, dim3(blocks_of(a->a.n, kRngThreads), a->a.epochs, a->P), dim3(kRngThreads),
                       0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_pop_sample(const PopSampleArgs* a, hipStream_t s) {
    if (a->P <= 0 || a->B <= 0 || a->R <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_pop_sample_kernel, dim3(blocks_of((long long)a->R * a->B, kRngThreads), a->P),
                       dim3(kRngThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_train_log_pop(const TrainLogPopArgs* a, hipStream_t s) {
    if (a->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_train_log_pop_kernel, dim3(a->P), dim3(kLogThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_train_log(const TrainLogArgs* a, hipStream_t s) {
    hipLaunchKernelGGL(lmpc_train_log_kernel, dim3(1), dim3(kLogThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_gbuf_append(const GbufAppendArgs* a, hipStream_t s) {
    if (a->m <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_gbuf_append_kernel, dim3(a->m), dim3(kAppendThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_gae_seq(const GaeSeqArgs* a, hipStream_t s) {
    if (a->G <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_gae_seq_kernel<GaeSeqArgs>, dim3(1), dim3(kSeqThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_global_log(const GlobalLogArgs* a, hipStream_t s) {
    hipLaunchKernelGGL(lmpc_global_log_kernel, dim3(1), dim3(64), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_pop_global_sample(const PopGlobalSampleArgs* a, hipStream_t s) {
    if (a->P <= 0 || a->G <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_pop_global_sample_kernel, dim3(blocks_of(a->G, kRngThreads), a->P), dim3(kRngThreads), 0, s,
                       *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_gbuf_append_pop(const GbufAppendPopArgs* a, hipStream_t s) {
    if (a->a.m <= 0 || a->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_gbuf_append_pop_kernel, dim3(a->a.m, a->P), dim3(kAppendThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_gae_seq_pop(const GaeSeqPopArgs* a, hipStream_t s) {
    if (a->a.G <= 0 || a->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_gae_seq_kernel<GaeSeqPopArgs>, dim3(a->P), dim3(kSeqThreads), 0, s, *a);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_global_log_pop(const GlobalLogPopArgs* a, hipStream_t s) {
    if (a->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(lmpc_global_log_pop_kernel, dim3(a->P), dim3(64), 0, s, *a);
    return hipGetLastError();
}
