// lmpc_train.h -- launch arguments of the kernels that close the LMPC training loop on the device
// (lmpc_train.hip): the exploration noise and the mini-batch permutations from one counter-based generator, the
// mean-based parameter write after an update (LMPC/src/controller/rlmpc2.py:876-896), and the iteration's log row
// with the best-policy snapshot (:918-922).  With them dart_lmpc_train_dev enqueues whole PPO iterations -- noise,
// dart_lmpc_collect_dev, critic value, GAE, permutations, dart_lmpc_ppo_update_dev, parameter write, log row -- on
// one stream without host work in between.  dart_lmpc_train_global_dev adds the loop's second update on the global
// buffer (:823-874) between the update and the parameter write: a choice without replacement (the permutation
// kernel on its own generator stream, cut to a prefix), the record gather into the persistent buffer, GAE over the
// buffer as one sequence, and the update's launches once more on the buffer's rows.
//
// Plain launches in stream order: no cooperative launch, no grid barrier, no atomics; every sum has a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_policy.h"
#include "lmpc_ppo.h"

namespace dartmpc {

// Philox4x32-10 (Salmon et al., SC'11) with the standard constants.  key = (seed & 0xffffffff, seed >> 32); the
// counter is (c, iteration, stream, epoch): block c yields the four words of elements 4c .. 4c+3.
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr uint32_t kStreamNoise = 0, kStreamPerm = 1;
// the global-buffer update (rlmpc2.py:823-874): its draw without replacement and its mini-batch permutations
constexpr uint32_t kStreamChoice = 2, kStreamGlobalPerm = 3;
// the exploit/explore step of a population (lmpc_pbt.h): counter (learner, generation, 4, block)
constexpr uint32_t kStreamPbt = 4;

struct Philox4 { uint32_t w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

struct PhiloxArgs {             // out[i] = philox(in[i][0:4], key in[i][4:6]), for the known-answer tests
    int n;
    const uint32_t* in;         // [n][6]
    uint32_t* out;              // [n][4]
};

// standard-normal draws [n] (n = steps * B * 34): element e takes word e % 4 of block e / 4; words 0, 1 and 2, 3
// each give one Box-Muller pair from u = ((r >> 9) + 0.5) 2^-23
struct NoiseArgs {
    long long n;
    uint32_t key0, key1, iteration;
    float* out;
};

// perm[e][rank of (key_i, i)] = i, key_i = word i % 4 of block i / 4 with `stream` and epoch e in the counter;
// grid (ceil(n / 256), epochs).  Only ranks below `limit` are written, in rows of `limit` entries: limit = n gives
// the permutations, limit = m < n their first m entries (a choice of m out of n without replacement)
struct PermArgs {
    int n, epochs, limit;
    uint32_t key0, key1, iteration, stream;
    int32_t* perm;              // [epochs][n]
    uint32_t* key_out;          // [epochs][n] the raw keys, nullable
};

struct IotaArgs {
    int n;
    int32_t* out;               // [n] 0 .. n-1
};

// ---- a population of P learners (dart_lmpc_train_pop_dev): instance i = l B + b, learner-major -------------------
// the generator keys of the learners travel in the launch arguments
struct PopKeys { uint32_t k[kPopMax][2]; };

// learner l's draws are those of NoiseArgs for its key: element (k, b, j), flat (k B + b) 34 + j of its generator
// (n = steps * B * 34 of them), is stored at out[k][l B + b][j]; grid (blocks, P)
struct NoisePopArgs {
    long long n;
    int B, P;
    uint32_t iteration;
    PopKeys keys;
    float* out;                 // [steps][P B][34]
};

// PermArgs per learner (limit = n, no key_out): perm [P][epochs][n]; grid (ceil(n / 256), epochs, P)
struct PermPopArgs {
    PermArgs a;                 // key0, key1 unused
    int P;
    PopKeys keys;
};

// the sample lists [P][n], n = R B: sample_l[r B + b] = r (P B) + l B + b, the flat index of record r of instance
// l B + b in the stacked record arrays
struct PopSampleArgs {
    int P, B, R;
    int32_t* out;
};

// the actor's mean on history (no Welford update, no shift, zero noise, timestep untouched), then the logit-space
// update, the EMA and the soft clip of policy_step_wave, unconditionally; current_k <- model_params
struct MeanUpdateArgs {
    int B;
    int learner_B;              // population: instance b reads the actor of learner b / learner_B; 0: one for all
    PolicyWeights w;
    const float* history;       // [B][520]
    double* model_params;       // [B][34] in/out
    double* current_k;          // [B][34] out
    float* mean_out;            // [B][34] nullable
    double max_delta, k_max, min_k, k_ceiling_margin, action_scale, smooth_alpha;
};

// rlmpc2.py:823-827: buffer row fill + j <- record sample[choice[j]] (flat index row * B + b), j < m, all six
// fields bit for bit; one workgroup per record, the observation row in 16-byte moves (both obs bases 16-byte
// aligned: 520 floats keep every row aligned).  A choice outside [0, n) or a record outside [0, rec_total) writes
// nothing.
struct GbufAppendArgs {
    int m, n, fill;
    long long rec_total;
    const int32_t* sample;      // [n]
    const int32_t* choice;      // [m]
    const float* rec_obs; const float* rec_action; const float* rec_logp; const float* rec_value;
    const double* rec_reward; const float* rec_done;
    float* obs; float* action; float* logp; float* value; double* reward; float* done;     // [capacity][..]
};

// compute_gae (rlmpc2.py:592-599) over rows 0 .. G-1 as one chain, fp64, bootstrapped from last_value [1]: one
// workgroup, a suffix scan of the affine maps gae -> delta_t + c_t gae over tiles of 1024 rows
struct GaeSeqArgs {
    int G;
    double gamma, lam;
    const double* reward;       // [G]
    const float* value;         // [G]
    const float* done;          // [G]
    const float* last_value;    // [1]
    double* adv;                // [G]
    double* ret;                // [G] adv + value
};

constexpr int kGlobalLogCols = 6;

// one row of global_log: fill after the append, 1 if the update ran, G, and the update's means (NaN without)
struct GlobalLogArgs {
    int fill, ran, G;
    const double* stats;        // [3], read when ran
    double* row;                // [6]
};

constexpr int kTrainLogCols = 12;

// one row of train_log and the best-policy snapshot; one workgroup
struct TrainLogArgs {
    int B, K, R, n, iteration, track_best;
    const int32_t* ep0;         // [B] episodes before the collection
    const int32_t* episodes;    // [B]
    const double* last_return;  // [B]
    const int32_t* nrec;        // [B]
    const double* log_reward;   // [K][B]
    const int32_t* log_status;  // [K][B]
    const double* stats;        // [3] of the update
    const float* actor;         // [39748]
    const float* critic;        // [37569]
    double* row;                // [12]
    double* best_return;        // [1] in/out
    float* best_weights;        // [77317]
    int32_t* best_iter;         // [1]
};

// one workgroup per learner: TrainLogArgs (learner 0's, B instances each) moved to learner l; log_reward and
// log_status are the stacked logs [K][P B], of which learner l visits its entries in the single run's flat order
// i = k B + b, read at [k][l B + b]; train_log is [P][iterations][12] (row_stride = iterations * 12), stats [P][3]
struct TrainLogPopArgs {
    TrainLogArgs a;
    int P;
    long long row_stride;
};

// ---- the global-buffer update of a population (dart_lmpc_train_pop_global_dev) -----------------------------------
// P buffers stacked learner-major, `capacity` rows apart: obs [P][capacity][520], ..., reward [P][capacity].  `a`
// holds learner 0's arguments; the kernels move them to the block's learner and run the single kernel's body.

// the sample lists over the buffers [P][G]: sample_l[i] = l capacity + i, the flat row of learner l's row i in the
// stacked buffer arrays (and in adv / ret [P][capacity]); grid (ceil(G / 256), P)
struct PopGlobalSampleArgs {
    int P, G, capacity;
    int32_t* out;
};

// grid (m, P): learner l gathers record sample_l[choice_l[j]] (sample [P][n], choice [P][m]; the record arrays are
// the stacked ones, shared) into row fill + j of its own buffer
struct GbufAppendPopArgs {
    GbufAppendArgs a;
    int P, capacity;
};

// one workgroup per learner: GaeSeqArgs on rows l capacity .. l capacity + G - 1, bootstrapped from last_value[l]
struct GaeSeqPopArgs {
    GaeSeqArgs a;               // adv, ret [P][capacity]
    int P, capacity;
};

// one workgroup per learner: row `a.row + l row_stride` of global_log [P][iterations][6] from stats [P][3]
struct GlobalLogPopArgs {
    GlobalLogArgs a;
    int P;
    long long row_stride;
};

// rows of the global buffer for n samples per iteration: m = max(1, n / 4) are drawn per iteration, and the buffer
// is updated on when it holds G = ceil(n / m) m >= n rows
inline void global_rows(int n, int& m, int& G) {
    m = n / 4 > 1 ? n / 4 : 1;
    G = (n + m - 1) / m * m;
}

// Workspace of a training iteration of P learners of B instances each (bytes from the base, every block 256-byte
// aligned): noise, last_value, adv, ret and ep0 over the P B instances, the per-learner sample lists, permutations
// and statistics, and P workspaces of the update, ppo_stride bytes apart.  P = 1 is dart_lmpc_train_dev's workspace,
// block for block.
struct TrainWorkspace {
    size_t noise, last_value, adv, ret, sample, perm, stats, ep0, ppo, ppo_stride, bytes;
};
inline TrainWorkspace train_workspace(int P, int B, int K, int record_every, int epochs, int mb) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t PB_ = (size_t)P * B, R = (size_t)(K / record_every), n = R * (size_t)B;
    TrainWorkspace w;
    size_t o = 0;
    w.noise = o; o += al(sizeof(float) * (size_t)K * PB_ * 34);
    w.last_value = o; o += al(sizeof(float) * PB_);
    w.adv = o; o += al(sizeof(double) * R * PB_);
    w.ret = o; o += al(sizeof(double) * R * PB_);
    w.sample = o; o += al(sizeof(int32_t) * n * P);
    w.perm = o; o += al(sizeof(int32_t) * n * P * (size_t)(epochs > 0 ? epochs : 1));
    w.stats = o; o += al(sizeof(double) * 3 * P);
    w.ep0 = o; o += al(sizeof(int32_t) * PB_);
    w.ppo_stride = ppo_workspace((int)n, mb).bytes;
    w.ppo = o; o += w.ppo_stride * P;
    w.bytes = o;
    return w;
}

// Workspace of the global update of P learners, their buffers `capacity` rows apart (bytes from the base, every block
// 256-byte aligned): the choices [P][m], adv and ret [P][capacity] (addressed by the sample lists, like the buffers'
// rows: the update's population kernels reach records, adv and ret through one index), the bootstrap values [P], the
// sample lists [P][G], the permutations [P][epochs][G], the statistics [P][3] and P workspaces of the update over G
// rows, ppo_stride bytes apart.  P = 1 with capacity = G is dart_lmpc_train_global_dev's workspace, block for block
// (one buffer is addressed by its rows below G, whatever its capacity).
struct GlobalWorkspace {
    size_t choice, adv, ret, last_value, sample, perm, stats, ppo, ppo_stride, bytes;
};
inline GlobalWorkspace global_workspace(int P, int n, int capacity, int epochs, int mb) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    int m, Gi;
    global_rows(n, m, Gi);
    const size_t G = (size_t)Gi, Pn = (size_t)P, cap = (size_t)capacity;
    GlobalWorkspace w;
    size_t o = 0;
    w.choice = o; o += al(sizeof(int32_t) * (size_t)m * Pn);
    w.adv = o; o += al(sizeof(double) * cap * Pn);
    w.ret = o; o += al(sizeof(double) * cap * Pn);
    w.last_value = o; o += al(sizeof(float) * Pn);
    w.sample = o; o += al(sizeof(int32_t) * G * Pn);
    w.perm = o; o += al(sizeof(int32_t) * G * Pn * (size_t)(epochs > 0 ? epochs : 1));
    w.stats = o; o += al(sizeof(double) * 3 * Pn);
    w.ppo_stride = ppo_workspace(Gi, mb).bytes;
    w.ppo = o; o += w.ppo_stride * Pn;
    w.bytes = o;
    return w;
}

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_philox(const dartmpc::PhiloxArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_noise(const dartmpc::NoiseArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_perms(const dartmpc::PermArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_iota(const dartmpc::IotaArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_noise_pop(const dartmpc::NoisePopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_perms_pop(const dartmpc::PermPopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_pop_sample(const dartmpc::PopSampleArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_train_log_pop(const dartmpc::TrainLogPopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_mean_update(const dartmpc::MeanUpdateArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_train_log(const dartmpc::TrainLogArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_gbuf_append(const dartmpc::GbufAppendArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_gae_seq(const dartmpc::GaeSeqArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_global_log(const dartmpc::GlobalLogArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_pop_global_sample(const dartmpc::PopGlobalSampleArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_gbuf_append_pop(const dartmpc::GbufAppendPopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_gae_seq_pop(const dartmpc::GaeSeqPopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_global_log_pop(const dartmpc::GlobalLogPopArgs* args, hipStream_t stream);
