// lmpc_ppo.hip -- the PPO update of the LMPC parameter policy on the device (lmpc_ppo.h): rlmpc2.py:783-819.
//
// ppo_prepare_kernel   once per update: normalised returns and advantages of the selected samples
// ppo_grad_kernel      once per mini-batch: one workgroup per (net, tile of 16 samples) gathers its rows from the
//                      record arrays, runs the net forward and backward and writes the tile's partial gradient
// ppo_apply_kernel     once per mini-batch, one workgroup: sums the partials in tile order, takes the L2 norm with
//                      a fixed tree, clips as clip_grad_norm_ does and applies torch.optim.Adam in place
// critic_value_kernel  value_net on [n][520] observations (the bootstrap value of :776-779)
// *_pop_kernel         the four above for a population of P learners in one launch (dart_lmpc_train_pop_dev): the
//                      learner is a grid coordinate, the body is the single kernel's on arguments moved to that
//                      learner's sample list, permutation rows, nets, Adam state and workspace (lmpc_ppo.h); with a
//                      hyper-parameter table (dart_lmpc_train_pop_hyper_dev) the gradient and the apply kernel also
//                      take the learner's row of it in place of the shared config's values (ppo_hyper)
// critic_value_stride_pop_kernel  critic_value_pop_kernel with the learners' observations a given number of rows
//                      apart: the bootstrap values of a population's global-buffer update (row G - 1 of P buffers)
//
// Everything is fp32 as the reference's torch nets are, except the statistics of the normalisation, the sum of
// squares of the gradient norm, and the running sums of the actor's forward layers and of its log-probability
// (fp64, rounded once to fp32; see fwd_layer).  Activations live in LDS transposed, [feature][sample], so that a thread
// that owns one output column and four samples reads its four inputs with one 16-byte broadcast load.
#include "lmpc_ppo.h"

namespace dartmpc {

namespace {

constexpr int kGradThreads = 256;       // 4 waves: column = t & 63, sample group = t >> 6 (4 samples each)
constexpr int kOneWg = 1024;            // the single-workgroup kernels
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;

struct alignas(16) PpoLds {
    float Xt[kPpoObs][kPpoTile];        // observations
    float H1t[kPpoHid][kPpoTile];       // tanh layers
    float H2t[kPpoHid][kPpoTile];
    float D1t[kPpoHid][kPpoTile];       // dL/d(pre-activation)
    float D2t[kPpoHid][kPpoTile];
    float Ot[kPpoAct][kPpoTile];        // the net's output: mean [34] or value [1]
    float DOt[kPpoAct][kPpoTile];       // dL/d(output)
    float At[kPpoAct][kPpoTile];        // actions
    float coef[kPpoTile];               // dL/d(logp) per sample
    float term[kPpoTile];               // the sample's surrogate / squared value error
    long long row[kPpoTile];            // record row, -1: not a sample of this tile
    int pos[kPpoTile];                  // position in the sample list
};

__device__ inline float4 ld4(const float (*Mt)[kPpoTile], int k, int g) {
    return *reinterpret_cast<const float4*>(&Mt[k][4 * g]);
}

// Outt[j][s] = act(b[j] + sum_k Int[k][s] W[k][j]) for the thread's column j and its four samples.  Acc is the
// type of the running sum: the actor's layers sum in fp64 and round once, because its mean enters the
// log-probability divided by var >= 1e-4, so that an error of the mean comes back 100 times larger in the ratio
// (with fp32 sums the gradient norm's error measured four times that of torch's fp32 path); inputs, weights and
// outputs are fp32 either way.
template <int NOUT, bool TANH, typename Acc>
__device__ inline void fwd_layer(const float* __restrict__ W, const float* __restrict__ b, int K,
                                 const float (*Int)[kPpoTile], float (*Outt)[kPpoTile]) {
    const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
    if (j < NOUT) {
        const Acc b0 = (Acc)b[j];
        Acc a0 = b0, a1 = b0, a2 = b0, a3 = b0;
#pragma unroll 8
        for (int k = 0; k < K; ++k) {
            const Acc w = (Acc)W[k * NOUT + j];
            const float4 x = ld4(Int, k, g);
            a0 += (Acc)x.x * w; a1 += (Acc)x.y * w; a2 += (Acc)x.z * w; a3 += (Acc)x.w * w;
        }
        float o0 = (float)a0, o1 = (float)a1, o2 = (float)a2, o3 = (float)a3;
        if (TANH) { o0 = tanhf(o0); o1 = tanhf(o1); o2 = tanhf(o2); o3 = tanhf(o3); }
        *reinterpret_cast<float4*>(&Outt[j][4 * g]) = make_float4(o0, o1, o2, o3);
    }
}

// gW[k][j] = sum_s Int[k][s] Dt[j][s], gb[j] = sum_s Dt[j][s], the 16 samples summed in index order
template <int NOUT>
__device__ inline void weight_grad(int K, const float (*Int)[kPpoTile], const float (*Dt)[kPpoTile],
                                   float* __restrict__ gW, float* __restrict__ gb) {
    const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
    if (j < NOUT) {
        const float4 d0 = ld4(Dt, j, 0), d1 = ld4(Dt, j, 1), d2 = ld4(Dt, j, 2), d3 = ld4(Dt, j, 3);
#pragma unroll 2
        for (int k = g; k < K; k += 4) {
            const float4 x0 = ld4(Int, k, 0), x1 = ld4(Int, k, 1), x2 = ld4(Int, k, 2), x3 = ld4(Int, k, 3);
            float s = x0.x * d0.x;
            s = fmaf(x0.y, d0.y, s); s = fmaf(x0.z, d0.z, s); s = fmaf(x0.w, d0.w, s);
            s = fmaf(x1.x, d1.x, s); s = fmaf(x1.y, d1.y, s); s = fmaf(x1.z, d1.z, s); s = fmaf(x1.w, d1.w, s);
            s = fmaf(x2.x, d2.x, s); s = fmaf(x2.y, d2.y, s); s = fmaf(x2.z, d2.z, s); s = fmaf(x2.w, d2.w, s);
            s = fmaf(x3.x, d3.x, s); s = fmaf(x3.y, d3.y, s); s = fmaf(x3.z, d3.z, s); s = fmaf(x3.w, d3.w, s);
            gW[k * NOUT + j] = s;
        }
        if (g == 0) {
            float s = d0.x + d0.y; s += d0.z; s += d0.w;
            s += d1.x; s += d1.y; s += d1.z; s += d1.w;
            s += d2.x; s += d2.y; s += d2.z; s += d2.w;
            s += d3.x; s += d3.y; s += d3.z; s += d3.w;
            gb[j] = s;
        }
    }
}

// Dt[k][s] = (1 - Ht[k][s]^2) sum_o W[k][o] DOutt[o][s] for the thread's hidden unit k and its four samples
template <int NOUT>
__device__ inline void hidden_grad(const float* __restrict__ W, const float (*DOutt)[kPpoTile],
                                   const float (*Ht)[kPpoTile], float (*Dt)[kPpoTile]) {
    const int k = threadIdx.x & 63, g = threadIdx.x >> 6;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 2
    for (int o = 0; o < NOUT; ++o) {
        const float w = W[k * NOUT + o];
        const float4 d = ld4(DOutt, o, g);
        a0 = fmaf(w, d.x, a0); a1 = fmaf(w, d.y, a1); a2 = fmaf(w, d.z, a2); a3 = fmaf(w, d.w, a3);
    }
    const float4 h = ld4(Ht, k, g);
    *reinterpret_cast<float4*>(&Dt[k][4 * g]) =
        make_float4(a0 * (1.f - h.x * h.x), a1 * (1.f - h.y * h.y), a2 * (1.f - h.z * h.z), a3 * (1.f - h.w * h.w));
}

// the tile's observations, transposed; rows that are not samples of the tile read as zero
__device__ inline void load_obs(PpoLds& L, const float* __restrict__ obs) {
    for (int o = threadIdx.x; o < kPpoTile * kPpoObs; o += blockDim.x) {
        const int s = o / kPpoObs, k = o - s * kPpoObs;
        const long long r = L.row[s];
        L.Xt[k][s] = r >= 0 ? obs[(size_t)r * kPpoObs + k] : 0.f;
    }
}

template <int NOUT, typename Acc>
__device__ inline void forward(PpoLds& L, const float* __restrict__ w) {
    const float* W1 = w;
    const float* b1 = W1 + kPpoObs * kPpoHid;
    const float* W2 = b1 + kPpoHid;
    const float* b2 = W2 + kPpoHid * kPpoHid;
    const float* W3 = b2 + kPpoHid;
    const float* b3 = W3 + kPpoHid * NOUT;
    fwd_layer<kPpoHid, true, Acc>(W1, b1, kPpoObs, L.Xt, L.H1t);
    __syncthreads();
    fwd_layer<kPpoHid, true, Acc>(W2, b2, kPpoHid, L.H1t, L.H2t);
    __syncthreads();
    fwd_layer<NOUT, false, Acc>(W3, b3, kPpoHid, L.H2t, L.Ot);
    __syncthreads();
}

// with L.DOt set: every gradient of the net's three layers into gp (the packed order of the weights)
template <int NOUT>
__device__ inline void backward(PpoLds& L, const float* __restrict__ w, float* __restrict__ gp) {
    constexpr int oW1 = 0, ob1 = oW1 + kPpoObs * kPpoHid, oW2 = ob1 + kPpoHid, ob2 = oW2 + kPpoHid * kPpoHid,
                  oW3 = ob2 + kPpoHid, ob3 = oW3 + kPpoHid * NOUT;
    weight_grad<NOUT>(kPpoHid, L.H2t, L.DOt, gp + oW3, gp + ob3);
    hidden_grad<NOUT>(w + oW3, L.DOt, L.H2t, L.D2t);
    __syncthreads();
    weight_grad<kPpoHid>(kPpoHid, L.H1t, L.D2t, gp + oW2, gp + ob2);
    hidden_grad<kPpoHid>(w + oW2, L.D2t, L.H1t, L.D1t);
    __syncthreads();
    weight_grad<kPpoHid>(kPpoObs, L.Xt, L.D1t, gp + oW1, gp + ob1);
}

// The bodies of the kernels take their arguments by reference: the single launches pass their own, a population's
// launches (the *_pop_kernel forms below) a copy moved to the block's learner.
__device__ __forceinline__ void ppo_grad_body(const PpoGradArgs& a) {
    __shared__ PpoLds L;
    const int t = threadIdx.x, tile = blockIdx.x;
    const bool is_critic = blockIdx.y == 1;
    const int first = tile * kPpoTile;
    if (first >= a.M) return;                               // block-uniform
    const float inv_m = 1.f / (float)a.M;
    if (t < kPpoTile) {
        long long r = -1;
        int p = 0;
        if (first + t < a.M) {
            p = a.idx[first + t];
            if (p >= 0 && p < a.n) {
                const long long q = a.sample[p];
                if (q >= 0 && q < a.rec_total) r = q;
            } else {
                p = 0;
            }
        }
        L.row[t] = r;
        L.pos[t] = p;
    }
    __syncthreads();
    load_obs(L, a.rec_obs);
    float* gp = a.part + (size_t)tile * kPpoPartStride;

    if (is_critic) {
        __syncthreads();
        forward<1, float>(L, a.critic);
        if (t < kPpoTile) {
            float d = 0.f;
            if (L.row[t] >= 0) d = L.Ot[0][t] - a.ret_n[L.pos[t]];
            L.term[t] = d * d;                                                  // mse_loss (:813)
            L.DOt[0][t] = a.vf_coef * 2.f * d * inv_m;
        }
        __syncthreads();
        if (t == 0) {
            float s = 0.f;
            for (int i = 0; i < kPpoTile; ++i) s += L.term[i];
            a.loss_part[2 * tile + 1] = s;
        }
        backward<1>(L, a.critic, gp + kPpoActorN);
        return;
    }

    for (int o = t; o < kPpoTile * kPpoAct; o += kGradThreads) {
        const int s = o / kPpoAct, j = o - s * kPpoAct;
        const long long r = L.row[s];
        L.At[j][s] = r >= 0 ? a.rec_action[(size_t)r * kPpoAct + j] : 0.f;
    }
    __syncthreads();
    forward<kPpoAct, double>(L, a.actor);
    const float* log_std = a.actor + (kPpoActorN - kPpoAct);
    if (t < kPpoTile) {
        // logp = Normal(mean, std).log_prob(a).sum() (:806-807), ratio and the clipped surrogate (:808-812)
        float c = 0.f, sur = 0.f;
        if (L.row[t] >= 0) {
            // the 34 fp32 terms are summed in fp64: logp is about 30 and exp() turns its absolute error into a
            // relative one of the ratio, which scales the sample's whole gradient (a sequential fp32 sum here
            // measured 1.7 times the error of torch's fp32 path on the actor's gradient)
            double lp = 0.0;
            for (int j = 0; j < kPpoAct; ++j) {
                const float lsd = fminf(fmaxf(log_std[j], a.log_std_min), a.log_std_max);
                const float sd = expf(lsd), z = L.At[j][t] - L.Ot[j][t];
                lp += (double)(-(z * z) / (2.f * (sd * sd)) - lsd - kLogSqrt2Pi);
            }
            const float adv = a.adv_n[L.pos[t]];
            const float ratio = expf((float)(lp - (double)a.rec_logp[L.row[t]]));
            const float s1 = ratio * adv, s2 = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi) * adv;
            sur = fminf(s1, s2);
            // torch.min over torch.clamp passes adv to the ratio inside the clip range (both branches tie and the
            // clamp is transparent) or where the unclipped term is the smaller one, and nothing otherwise
            const bool pass = (ratio >= a.clip_lo && ratio <= a.clip_hi) || s1 < s2;
            c = pass ? -(adv * ratio) * inv_m : 0.f;
        }
        L.coef[t] = c;
        L.term[t] = sur;
    }
    __syncthreads();
    for (int o = t; o < kPpoTile * kPpoAct; o += kGradThreads) {
        const int j = o / kPpoTile, s = o - j * kPpoTile;
        const float lsd = fminf(fmaxf(log_std[j], a.log_std_min), a.log_std_max);
        const float sd = expf(lsd);
        L.DOt[j][s] = L.coef[s] * (L.At[j][s] - L.Ot[j][s]) / (sd * sd);
    }
    if (t < kPpoAct) {
        // log_std: the data term sum_s coef (z^2 / var - 1) and, once per mini-batch, the entropy's -ent_coef;
        // the clamp passes neither when log_std lies strictly outside its range
        const float ls = log_std[t];
        float gl = 0.f;
        if (ls >= a.log_std_min && ls <= a.log_std_max) {
            const float sd = expf(ls), iv = 1.f / (sd * sd);
            for (int s = 0; s < kPpoTile; ++s) {
                const float z = L.At[t][s] - L.Ot[t][s];
                gl = fmaf(L.coef[s], z * z * iv - 1.f, gl);
            }
            if (tile == 0) gl -= a.ent_coef;
        }
        gp[kPpoActorN - kPpoAct + t] = gl;
    }
    if (t == 0) {
        float s = 0.f;
        for (int i = 0; i < kPpoTile; ++i) s += L.term[i];
        a.loss_part[2 * tile] = s;
    }
    __syncthreads();
    backward<kPpoAct>(L, a.actor, gp);
}

// sum over the workgroup in a fixed tree; every thread gets the result
__device__ inline double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = kOneWg / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kGradThreads) void ppo_grad_kernel(PpoGradArgs a) { ppo_grad_body(a); }

// p + bytes
template <class T> __device__ __forceinline__ T* moved(T* p, size_t bytes) {
    return p ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + bytes) : p;
}

// grid (tiles, 2, P): learner z on its sample list, its slice of the permutations, its nets and its workspace
__global__ __launch_bounds__(kGradThreads) void ppo_grad_pop_kernel(PpoGradPopArgs p) {
    PpoGradArgs a = p.a;
    const size_t l = blockIdx.z, ws = l * p.ws_stride;
    a.sample += l * (size_t)a.n; a.idx += l * p.idx_stride;
    a.adv_n = moved(a.adv_n, ws); a.ret_n = moved(a.ret_n, ws);
    a.actor += l * kPpoActorN; a.critic += l * kPopCriticStride;
    a.part = moved(a.part, ws); a.loss_part = moved(a.loss_part, ws);
    if (p.hyper) ppo_hyper_set(a, ppo_hyper(p.hyper + l * kHyperCols));     // block-uniform
    ppo_grad_body(a);
}

__device__ __forceinline__ void ppo_prepare_body(const PpoPrepareArgs& a) {
    __shared__ double red[kOneWg];
    const int t = threadIdx.x;
    auto at = [&](const double* v, int i) {
        const long long s = a.sample[i];
        return s >= 0 && s < a.rec_total ? v[s] : 0.0;
    };
    double sr = 0.0, sa = 0.0;
    for (int i = t; i < a.n; i += kOneWg) {
        sr += at(a.ret, i);
        sa += (double)(float)at(a.adv, i);
    }
    const double n = (double)a.n;
    const double mr = block_sum(sr, red) / n, ma = block_sum(sa, red) / n;
    double qr = 0.0, qa = 0.0;
    for (int i = t; i < a.n; i += kOneWg) {
        const double dr = at(a.ret, i) - mr, da = (double)(float)at(a.adv, i) - ma;
        qr += dr * dr;
        qa += da * da;
    }
    const double std_r = sqrt(block_sum(qr, red) / n);                          // numpy: population (:783)
    const float std_a = (float)sqrt(block_sum(qa, red) / (n - 1.0));            // torch: unbiased (:790)
    const float mean_a = (float)ma;
    for (int i = t; i < a.n; i += kOneWg) {
        const float rn = (float)((at(a.ret, i) - mr) / (std_r + 1e-8));
        const float an = ((float)at(a.adv, i) - mean_a) / (std_a + 1e-8f);
        a.ret_n[i] = rn;
        a.adv_n[i] = an;
        if (a.ret_out) a.ret_out[i] = rn;
        if (a.adv_out) a.adv_out[i] = an;
    }
}

__global__ __launch_bounds__(kOneWg) void ppo_prepare_kernel(PpoPrepareArgs a) { ppo_prepare_body(a); }

// one workgroup per learner: the statistics over its n samples, in the single kernel's order
__global__ __launch_bounds__(kOneWg) void ppo_prepare_pop_kernel(PpoPreparePopArgs p) {
    PpoPrepareArgs a = p.a;
    const size_t l = blockIdx.x, ws = l * p.ws_stride;
    a.sample += l * (size_t)a.n;
    a.adv_n = moved(a.adv_n, ws); a.ret_n = moved(a.ret_n, ws);
    ppo_prepare_body(a);
}

__device__ __forceinline__ void ppo_apply_body(const PpoApplyArgs& a) {
    __shared__ double red[kOneWg];
    __shared__ float sh[4];
    const int t = threadIdx.x;
    double sq = 0.0;
    // four of the thread's entries at a time, so that four loads are in flight per tile (one workgroup is bound by
    // the latency of its loads, not by bandwidth); the order of every sum is that of the plain loop
    for (int i0 = t; i0 < kPpoParams; i0 += 4 * kOneWg) {
        float g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kOneWg;
            g[u] = i < kPpoParams ? a.part[i] : 0.f;
        }
        for (int tl = 1; tl < a.tiles; ++tl) {
            const float* p = a.part + (size_t)tl * kPpoPartStride;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * kOneWg;
                if (i < kPpoParams) g[u] += p[i];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kOneWg;
            if (i < kPpoParams) {
                a.grad[i] = g[u];
                sq += (double)g[u] * (double)g[u];
            }
        }
    }
    const float norm = (float)sqrt(block_sum(sq, red));
    if (t == 0) {
        float pl = 0.f, vl = 0.f, en = 0.f;
        if (a.loss_part) {
            for (int tl = 0; tl < a.tiles; ++tl) { pl += a.loss_part[2 * tl]; vl += a.loss_part[2 * tl + 1]; }
            pl = -pl / (float)a.M;
            vl = vl / (float)a.M;
            const float* log_std = a.actor + (kPpoActorN - kPpoAct);
            for (int j = 0; j < kPpoAct; ++j)                                   // Normal.entropy().sum() (:814)
                en += 0.5f + kLogSqrt2Pi + fminf(fmaxf(log_std[j], a.log_std_min), a.log_std_max);
        } else if (a.terms_in) {
            pl = a.terms_in[0]; vl = a.terms_in[1]; en = a.terms_in[2];
        }
        a.terms[0] = pl; a.terms[1] = vl; a.terms[2] = en; a.terms[3] = norm;
        if (a.do_step) {
            const int step = a.adam_step[0] + 1;
            a.adam_step[0] = step;
            const double bc1 = 1.0 - pow(a.beta1, (double)step), bc2 = 1.0 - pow(a.beta2, (double)step);
            sh[0] = fminf(1.f, a.max_grad_norm / (norm + 1e-6f));               // clip_grad_norm_ (:818)
            sh[1] = (float)(a.lr / bc1);
            sh[2] = (float)sqrt(bc2);
            if (a.step_log) {
                float* row = a.step_log + 4 * (size_t)a.step_in_call;
                row[0] = pl; row[1] = vl; row[2] = en; row[3] = norm;
            }
            const float tv[3] = {pl, vl, en};
            for (int i = 0; i < 3; ++i) {
                const double s = (a.step_in_call > 0 ? a.stat_sum[i] : 0.0) + (double)tv[i];
                a.stat_sum[i] = s;
                if (a.stats) a.stats[i] = s / (double)(a.step_in_call + 1);
            }
        }
    }
    if (!a.do_step) return;                                 // block-uniform
    __syncthreads();                                        // (also: the entropy is read before log_std moves)
    const float coef = sh[0], step_size = sh[1], bc2s = sh[2];
    const float w1 = (float)(1.0 - a.beta1), w2 = (float)(1.0 - a.beta2), beta2 = (float)a.beta2;
#pragma unroll 4
    for (int i = t; i < kPpoParams; i += kOneWg) {
        float* wp = i < kPpoActorN ? a.actor + i : a.critic + (i - kPpoActorN);
        const float w = *wp;
        // every rounding spelled out as torch's CPU Adam places them (checked bit for bit against it on the host):
        // the moments cancel (m + 0.1 (g - m) with g near -9 m), so a last-bit difference in g would come out far
        // larger, relative to m, than the 1e-5 the update is held to
        const float g = fmaf(w, a.weight_decay, __fmul_rn(a.grad[i], coef));    // L2 decay after the clip (:561)
        float m = a.adam[i], v = a.adam[kPpoParams + i];
        m = fmaf(w1, __fsub_rn(g, m), m);
        v = fmaf(__fmul_rn(w2, g), g, __fmul_rn(beta2, v));
        a.adam[i] = m;
        a.adam[kPpoParams + i] = v;
        const float den = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), bc2s), a.adam_eps);
        *wp = __fadd_rn(w, __fdiv_rn(__fmul_rn(-step_size, m), den));
    }
}

__global__ __launch_bounds__(kOneWg) void ppo_apply_kernel(PpoApplyArgs a) { ppo_apply_body(a); }

// one workgroup per learner: its partials, its nets, its Adam state, its running means
__global__ __launch_bounds__(kOneWg) void ppo_apply_pop_kernel(PpoApplyPopArgs p) {
    PpoApplyArgs a = p.a;
    const size_t l = blockIdx.x, ws = l * p.ws_stride;
    a.part = moved(a.part, ws); a.loss_part = moved(a.loss_part, ws);
    a.grad = moved(a.grad, ws); a.terms = moved(a.terms, ws); a.stat_sum = moved(a.stat_sum, ws);
    a.actor += l * kPpoActorN; a.critic += l * kPopCriticStride;
    a.adam += l * 2 * (size_t)kPpoParams; a.adam_step += l;
    if (a.stats) a.stats += 3 * l;
    if (p.hyper) ppo_hyper_set(a, ppo_hyper(p.hyper + l * kHyperCols));     // block-uniform
    ppo_apply_body(a);
}

__device__ __forceinline__ void critic_value_body(const CriticValueArgs& a) {
    __shared__ PpoLds L;
    const int t = threadIdx.x, first = blockIdx.x * kPpoTile;
    if (first >= a.n) return;                               // block-uniform
    if (t < kPpoTile) L.row[t] = first + t < a.n ? first + t : -1;
    __syncthreads();
    load_obs(L, a.obs);
    __syncthreads();
    forward<1, float>(L, a.critic);
    if (t < kPpoTile && first + t < a.n) a.value[first + t] = L.Ot[0][t];
}

__global__ __launch_bounds__(kGradThreads) void critic_value_kernel(CriticValueArgs a) { critic_value_body(a); }

// grid (tiles of a.n, P): learner y's critic on its a.n observations (a sample's value does not depend on its tile)
__global__ __launch_bounds__(kGradThreads) void critic_value_pop_kernel(CriticValuePopArgs p) {
    CriticValueArgs a = p.a;
    const size_t l = blockIdx.y;
    a.critic += l * kPopCriticStride;
    a.obs += l * (size_t)a.n * kPpoObs; a.value += l * (size_t)a.n;
    critic_value_body(a);
}

// grid (tiles of a.n, P): as above, with learner y's observations obs_stride rows behind the ones before (the last
// rows of P stacked global buffers, `capacity` rows apart); its own entry point, so that critic_value_pop_kernel
// keeps its instructions
__global__ __launch_bounds__(kGradThreads) void critic_value_stride_pop_kernel(CriticValueStridePopArgs p) {
    CriticValueArgs a = p.a;
    const size_t l = blockIdx.y;
    a.critic += l * kPopCriticStride;
    a.obs += l * (size_t)p.obs_stride * kPpoObs; a.value += l * (size_t)a.n;
    critic_value_body(a);
}

}  // namespace

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_ppo_prepare(const dartmpc::PpoPrepareArgs* args, hipStream_t stream) {
    if (args->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(dartmpc::ppo_prepare_kernel, dim3(1), dim3(dartmpc::kOneWg), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_ppo_grad(const dartmpc::PpoGradArgs* args, hipStream_t stream) {
    if (args->M <= 0) return hipSuccess;
    const int tiles = (args->M + dartmpc::kPpoTile - 1) / dartmpc::kPpoTile;
    hipLaunchKernelGGL(dartmpc::ppo_grad_kernel, dim3(tiles, 2), dim3(dartmpc::kGradThreads), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_ppo_apply(const dartmpc::PpoApplyArgs* args, hipStream_t stream) {
    if (args->tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(dartmpc::ppo_apply_kernel, dim3(1), dim3(dartmpc::kOneWg), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_critic_value(const dartmpc::CriticValueArgs* args, hipStream_t stream) {
    if (args->n <= 0) return hipSuccess;
    const int blocks = (args->n + dartmpc::kPpoTile - 1) / dartmpc::kPpoTile;
    hipLaunchKernelGGL(dartmpc::critic_value_kernel, dim3(blocks), dim3(dartmpc::kGradThreads), 0, stream, *args);
    return hipGetLastError();
}

// ---- a population's launches: every learner in one grid ---------------------------------------------------------

extern "C" hipError_t dartmpc_launch_ppo_prepare_pop(const dartmpc::PpoPreparePopArgs* args, hipStream_t stream) {
    if (args->a.n <= 0 || args->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(dartmpc::ppo_prepare_pop_kernel, dim3(args->P), dim3(dartmpc::kOneWg), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_ppo_grad_pop(const dartmpc::PpoGradPopArgs* args, hipStream_t stream) {
    if (args->a.M <= 0 || args->P <= 0) return hipSuccess;
    const int tiles = (args->a.M + dartmpc::kPpoTile - 1) / dartmpc::kPpoTile;
    hipLaunchKernelGGL(dartmpc::ppo_grad_pop_kernel, dim3(tiles, 2, args->P), dim3(dartmpc::kGradThreads), 0, stream,
                       *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_ppo_apply_pop(const dartmpc::PpoApplyPopArgs* args, hipStream_t stream) {
    if (args->a.tiles <= 0 || args->P <= 0) return hipSuccess;
    hipLaunchKernelGGL(dartmpc::ppo_apply_pop_kernel, dim3(args->P), dim3(dartmpc::kOneWg), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_critic_value_pop(const dartmpc::CriticValuePopArgs* args, hipStream_t stream) {
    if (args->a.n <= 0 || args->P <= 0) return hipSuccess;
    const int blocks = (args->a.n + dartmpc::kPpoTile - 1) / dartmpc::kPpoTile;
    hipLaunchKernelGGL(dartmpc::critic_value_pop_kernel, dim3(blocks, args->P), dim3(dartmpc::kGradThreads), 0, stream,
                       *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_critic_value_stride_pop(const dartmpc::CriticValueStridePopArgs* args,
                                                             hipStream_t stream) {
    if (args->a.n <= 0 || args->P <= 0) return hipSuccess;
    const int blocks = (args->a.n + dartmpc::kPpoTile - 1) / dartmpc::kPpoTile;
    hipLaunchKernelGGL(dartmpc::critic_value_stride_pop_kernel, dim3(blocks, args->P), dim3(dartmpc::kGradThreads), 0,
                       stream, *args);
    return hipGetLastError();
}
