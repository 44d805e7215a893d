// lmpc_ppo.h -- launch arguments of the LMPC PPO kernels (lmpc_ppo.hip): the clipped-surrogate update of
// RLMPC._rl_worker (LMPC/src/controller/rlmpc2.py:783-819) on the records dart_lmpc_collect wrote -- return and
// advantage normalisation, forward and backward pass of both nets (fp32), gradient clipping and Adam -- and the
// critic's forward pass for the bootstrap value (:776-779).
//
// Plain launches on the caller's stream, in order: no cooperative launch, no grid barrier, no atomics.  Partial
// sums are combined in a fixed order, so two runs give the same bits.
//
// Unreachable in the reference and not reproduced: torch.clamp(std, min=1e-6) (:804) never binds because
// std = exp(clamp(log_std, log 1e-2, log 2)) >= 1e-2, and the softplus branch of :802-805 is not taken by Policy
// (:33-80), whose forward returns that std.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_policy.h"

namespace dartmpc {

constexpr int kPpoObs = 520, kPpoHid = 64, kPpoAct = 34;
// packed parameter order: the actor (W1 [520][64], b1, W2 [64][64], b2, W3 [64][34], b3, log_std [34]), then the
// critic (V1 [520][64], c1, V2 [64][64], c2, V3 [64], c3 [1]); gradients and Adam's m, v use the same order
constexpr int kPpoActorN = kPpoObs * kPpoHid + kPpoHid + kPpoHid * kPpoHid + kPpoHid + kPpoHid * kPpoAct + 2 * kPpoAct;
constexpr int kPpoCriticN = kPpoObs * kPpoHid + kPpoHid + kPpoHid * kPpoHid + kPpoHid + kPpoHid + 1;
constexpr int kPpoParams = kPpoActorN + kPpoCriticN;              // 39748 + 37569 = 77317
constexpr int kPpoTile = 16;                                      // samples per workgroup of the gradient kernel
constexpr int kPpoMaxBatch = 1024;                                // mini-batch limit (64 tiles)
constexpr int kPpoPartStride = (kPpoParams + 3) & ~3;             // one tile's partial gradient, 16-byte multiple
static_assert(kPpoActorN == kPolicyN && kPpoCriticN == kCriticN, "one pair of nets");

// Workspace layout (bytes from the base, every block 256-byte aligned) for n samples and mini-batches of up to mb.
// The blocks of fixed size come first and the tile partials last, so that every offset but `bytes` depends on n
// alone and the offsets of the apply launch on nothing: the entries that are not told mb (or n) find their blocks.
struct PpoWorkspace {
    size_t grad, terms, stat_sum, loss_part, adv_n, ret_n, part, bytes;
};
inline PpoWorkspace ppo_workspace(int n, int mb) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t tiles = (size_t)(mb + kPpoTile - 1) / kPpoTile;
    PpoWorkspace w;
    size_t o = 0;
    w.grad = o; o += al(sizeof(float) * kPpoPartStride);
    w.terms = o; o += al(sizeof(float) * 4);
    w.stat_sum = o; o += al(sizeof(double) * 3);
    w.loss_part = o; o += al(sizeof(float) * 2 * (kPpoMaxBatch / kPpoTile));
    w.adv_n = o; o += al(sizeof(float) * (size_t)n);
    w.ret_n = o; o += al(sizeof(float) * (size_t)n);
    w.part = o; o += al(sizeof(float) * tiles * kPpoPartStride);
    w.bytes = o;
    return w;
}

// returns (:783, numpy fp64, population std) and advantages (:788-790, fp32, torch's unbiased std) of the n
// selected samples, normalised; one workgroup
struct PpoPrepareArgs {
    int n;
    long long rec_total;        // entries of adv / ret (rec_rows * B); a sample outside [0, rec_total) reads as 0
    const int32_t* sample;      // [n] flat record indices row * B + b
    const double* adv;          // [rec_total]
    const double* ret;
    float* adv_n;               // [n] workspace
    float* ret_n;
    float* adv_out;             // [n] nullable copies
    float* ret_out;
};

// forward + backward of one mini-batch; grid (tiles, 2): y = 0 the actor, y = 1 the critic
struct PpoGradArgs {
    int n, M;                   // samples, mini-batch size (M <= 16 * tiles of the workspace)
    long long rec_total;
    float clip_lo, clip_hi;     // 1 - clip_eps, 1 + clip_eps
    float vf_coef, ent_coef, log_std_min, log_std_max;
    const int32_t* sample;      // [n]
    const int32_t* idx;         // [M] positions in sample (a slice of a permutation)
    const float* rec_obs;       // [rec_total][520]
    const float* rec_action;    // [rec_total][34]
    const float* rec_logp;      // [rec_total]
    const float* adv_n;         // [n]
    const float* ret_n;
    const float* actor;         // [39748]
    const float* critic;        // [37569]
    float* part;                // [tiles][kPpoPartStride] partial gradients
    float* loss_part;           // [tiles][2] sum of the surrogate, sum of (value - ret)^2
};

// sums the tile partials, norm, clip, Adam; one workgroup
struct PpoApplyArgs {
    int tiles, M;               // partials to sum (1: `part` is a packed gradient)
    int do_step;                // 0: only the gradient, the loss terms and the norm are written
    int step_in_call;           // row of step_log, and the count - 1 of the running means
    double lr, beta1, beta2;    // fp64 as torch holds them: 1 - beta and the bias corrections are formed in fp64
    float max_grad_norm, adam_eps, weight_decay, ent_coef, log_std_min, log_std_max;
    const float* part;          // [tiles][kPpoPartStride]
    const float* loss_part;     // [tiles][2]; null: the terms are read from terms_in
    const float* terms_in;      // [3] policy loss, value loss, entropy; nullable (zeros) when loss_part is null
    float* grad;                // [77317] the summed gradient, written
    float* terms;               // [4] policy loss, value loss, entropy, gradient norm before the clip, written
    float* actor;               // in/out with do_step
    float* critic;
    float* adam;                // [2][77317] m, v
    int32_t* adam_step;         // [1]
    float* step_log;            // [rows][4] nullable
    double* stat_sum;           // [3] workspace
    double* stats;              // [3] running means, nullable
};

// The hyper-parameters a learner may own (dart_lmpc_train_pop_hyper): a row of kHyperCols doubles, the first nine of
// dart_lmpc_ppo_config in the struct's order (clip_eps, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, adam_eps,
// weight_decay), and what the kernels take of them.  The conversion is stated here alone: the host launchers apply it
// to the shared config and the population's kernels to row l of the table, so a row that equals a config gives that
// config's launch arguments bit for bit.  The values enter arithmetic only, never an index or a trip count.
constexpr int kHyperCols = 9;
struct PpoHyper {
    float clip_lo, clip_hi;     // 1 - clip_eps, 1 + clip_eps, formed in fp64
    float vf_coef, ent_coef, max_grad_norm, adam_eps, weight_decay;
    double lr, beta1, beta2;
};
__host__ __device__ inline PpoHyper ppo_hyper(const double* row) {
    PpoHyper h;
    h.clip_lo = (float)(1.0 - row[0]); h.clip_hi = (float)(1.0 + row[0]);
    h.vf_coef = (float)row[1]; h.ent_coef = (float)row[2]; h.max_grad_norm = (float)row[3];
    h.lr = row[4]; h.beta1 = row[5]; h.beta2 = row[6];
    h.adam_eps = (float)row[7]; h.weight_decay = (float)row[8];
    return h;
}
__host__ __device__ inline void ppo_hyper_set(PpoGradArgs& a, const PpoHyper& h) {
    a.clip_lo = h.clip_lo; a.clip_hi = h.clip_hi; a.vf_coef = h.vf_coef; a.ent_coef = h.ent_coef;
}
__host__ __device__ inline void ppo_hyper_set(PpoApplyArgs& a, const PpoHyper& h) {
    a.max_grad_norm = h.max_grad_norm; a.lr = h.lr; a.beta1 = h.beta1; a.beta2 = h.beta2;
    a.adam_eps = h.adam_eps; a.weight_decay = h.weight_decay; a.ent_coef = h.ent_coef;
}

struct CriticValueArgs {
    int n;
    const float* critic;
    const float* obs;           // [n][520]
    float* value;               // [n]
};

// ---- a population of P learners in one launch (dart_lmpc_train_pop_dev) ------------------------------------------
// `a` holds learner 0's arguments.  Learner l works on them moved by l strides: its sample list [P][n], its slice of
// the permutations (idx_stride entries apart), its workspace (ws_stride bytes apart, a ppo_workspace each), its
// actor ([P][39748]), critic ([P][kPopCriticStride]), Adam state ([P][2][77317], adam_step [P]) and running means
// (stats [P][3]).  adv, ret and the record arrays are shared: the sample lists address them.  Every learner has the
// same n, so the same M in every step.
struct PpoPreparePopArgs {      // one workgroup per learner
    PpoPrepareArgs a;           // adv_out, ret_out: null
    int P;
    size_t ws_stride;
};
// hyper (device, nullable): the table [P][kHyperCols]; learner l takes ppo_hyper(row l) in place of a's values, read
// when the kernel runs.  Null: every learner runs with a's.
struct PpoGradPopArgs {         // grid (tiles, 2, P)
    PpoGradArgs a;
    int P;
    size_t ws_stride, idx_stride;
    const double* hyper;
};
struct PpoApplyPopArgs {        // one workgroup per learner
    PpoApplyArgs a;             // terms_in, step_log: null
    int P;
    size_t ws_stride;
    const double* hyper;
};
struct CriticValuePopArgs {     // grid (tiles of a.n, P): learner l's critic on rows l a.n .. (l + 1) a.n - 1
    CriticValueArgs a;
    int P;
};
// grid (tiles of a.n, P): learner l's critic on rows l obs_stride .. l obs_stride + a.n - 1 of obs, values [P][a.n]
// (the bootstrap of a population's global update: a.n = 1, obs at row G - 1 of buffer 0, obs_stride = capacity)
struct CriticValueStridePopArgs {
    CriticValueArgs a;
    int P;
    long long obs_stride;
};

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_critic_value_stride_pop(const dartmpc::CriticValueStridePopArgs* args,
                                                             hipStream_t stream);
extern "C" hipError_t dartmpc_launch_ppo_prepare_pop(const dartmpc::PpoPreparePopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_ppo_grad_pop(const dartmpc::PpoGradPopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_ppo_apply_pop(const dartmpc::PpoApplyPopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_critic_value_pop(const dartmpc::CriticValuePopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_ppo_prepare(const dartmpc::PpoPrepareArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_ppo_grad(const dartmpc::PpoGradArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_ppo_apply(const dartmpc::PpoApplyArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_critic_value(const dartmpc::CriticValueArgs* args, hipStream_t stream);
