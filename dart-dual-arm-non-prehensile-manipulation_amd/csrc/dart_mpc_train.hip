// dart_mpc_train.hip -- the training entries of include/dart_mpc.h (host side): GAE, the PPO update
// (lmpc_ppo.hip), the generator entries, the global buffer and whole training iterations (lmpc_train.hip).
#include <limits>

#include "abi_internal.h"

namespace {

hipError_t launch_gae(int B, int rec_rows, double gamma, double lam, const int32_t* nrec, const double* rec_reward,
                      const float* rec_value, const float* rec_done, const float* last_value, double* adv, double* ret,
                      hipStream_t s) {
    dartmpc::GaeArgs a;
    a.B = B; a.rec_rows = rec_rows; a.gamma = gamma; a.lam = lam; a.nrec = nrec; a.rec_reward = rec_reward;
    a.rec_value = rec_value; a.rec_done = rec_done; a.last_value = last_value; a.adv = adv; a.ret = ret;
    return dartmpc_launch_lmpc_gae(&a, s);
}

}  // namespace

int dart_lmpc_gae_dev(int B, int rec_rows, double gamma, double lam, const int32_t* nrec, const double* rec_reward,
                      const float* rec_value, const float* rec_done, const float* last_value, double* adv, double* ret,
                      void* stream) {
    if (B < 0 || rec_rows < 0) return DART_MPC_EINVAL;
    if (B == 0 || rec_rows == 0) return DART_MPC_OK;
    if (any_null({nrec, rec_reward, rec_value, rec_done, last_value, adv, ret})) return DART_MPC_EINVAL;
    return launch_gae(B, rec_rows, gamma, lam, nrec, rec_reward, rec_value, rec_done, last_value, adv, ret,
                      (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_gae(int B, int rec_rows, double gamma, double lam, const int32_t* nrec, const double* rec_reward,
                  const float* rec_value, const float* rec_done, const float* last_value, double* adv, double* ret) {
    if (B < 0 || rec_rows < 0) return DART_MPC_EINVAL;
    if (B == 0 || rec_rows == 0) return DART_MPC_OK;
    if (any_null({nrec, rec_reward, rec_value, rec_done, last_value, adv, ret})) return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    const size_t n = (size_t)B * rec_rows;
    if (S.reserve(sizeof(double) * 3 * n + sizeof(float) * (2 * n + B) + sizeof(int32_t) * B + 8 * 256, 0) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    const int32_t* d_nrec = S.in(nrec, (size_t)B);
    const double* d_rw = S.in(rec_reward, n);
    const float *d_vl = S.in(rec_value, n), *d_dn = S.in(rec_done, n), *d_lv = S.in(last_value, (size_t)B);
    double *d_adv = S.inout(adv, n), *d_ret = S.inout(ret, n);      // (rows >= nrec[b] keep the caller's contents)
    auto launch = [&](hipStream_t s) {
        return launch_gae(B, rec_rows, gamma, lam, d_nrec, d_rw, d_vl, d_dn, d_lv, d_adv, d_ret, s);
    };
    if (!D->run(launch)) return DART_MPC_EHIP;
    return DART_MPC_OK;
}

// ---- PPO update of the LMPC policy (lmpc_ppo.hip) ----------------------------------------------------------

void dart_lmpc_ppo_config_default(dart_lmpc_ppo_config* c) {
    if (!c) return;
    c->clip_eps = 0.2; c->vf_coef = 0.25; c->ent_coef = 0.01; c->max_grad_norm = 0.5;
    c->lr = 3e-4; c->beta1 = 0.9; c->beta2 = 0.999; c->adam_eps = 1e-8; c->weight_decay = 1e-5;
    c->log_std_min = std::log(1e-2); c->log_std_max = std::log(2.0);
    c->epochs = 8; c->mini_batch_size = 64;
}

size_t dart_lmpc_ppo_workspace_bytes(int n, int mini_batch_size) {
    if (n < 1 || mini_batch_size < 1 || mini_batch_size > dartmpc::kPpoMaxBatch) return 0;
    return dartmpc::ppo_workspace(n, mini_batch_size).bytes;
}

namespace {

bool ppo_cfg_ok(const dart_lmpc_ppo_config* c) {
    return c && c->mini_batch_size >= 1 && c->mini_batch_size <= dartmpc::kPpoMaxBatch && c->epochs >= 0 &&
           c->clip_eps >= 0.0 && c->lr >= 0.0 && c->beta1 >= 0.0 && c->beta1 < 1.0 && c->beta2 >= 0.0 &&
           c->beta2 < 1.0 && c->adam_eps >= 0.0 && c->max_grad_norm >= 0.0 && c->log_std_min <= c->log_std_max;
}

// A population's form of the three launches below: P learners, whose workspaces lie ws_stride bytes and whose rows of
// the permutations idx_stride entries apart (lmpc_ppo.h); P = 0: the single launch
struct PpoPop {
    int P = 0;
    size_t ws_stride = 0, idx_stride = 0;
    const double* hyper = nullptr;      // device table [P][kHyperCols] (lmpc_ppo.h); null: the shared config
};

// the shared config as a row of the hyper-parameter table: its first nine doubles
static_assert(offsetof(dart_lmpc_ppo_config, clip_eps) == 0 &&
              offsetof(dart_lmpc_ppo_config, weight_decay) == sizeof(double) * (dartmpc::kHyperCols - 1) &&
              DART_LMPC_HYPER_COLS == dartmpc::kHyperCols, "a config starts with a row of the table");
const double* hyper_row(const dart_lmpc_ppo_config* c) { return &c->clip_eps; }

// the launches of the PPO entries; ws is laid out for (n, mb) with M <= mb
hipError_t ppo_launch_prepare(int n, long long total, const int32_t* sample, const double* adv, const double* ret,
                              float* adv_out, float* ret_out, char* ws, int mb, hipStream_t s, PpoPop pop = {}) {
    const dartmpc::PpoWorkspace L = dartmpc::ppo_workspace(n, mb);
    dartmpc::PpoPrepareArgs a;
    a.n = n; a.rec_total = total; a.sample = sample; a.adv = adv; a.ret = ret;
    a.adv_n = reinterpret_cast<float*>(ws + L.adv_n); a.ret_n = reinterpret_cast<float*>(ws + L.ret_n);
    a.adv_out = adv_out; a.ret_out = ret_out;
    if (pop.P > 0) {
        const dartmpc::PpoPreparePopArgs q{a, pop.P, pop.ws_stride};
        return dartmpc_launch_ppo_prepare_pop(&q, s);
    }
    return dartmpc_launch_ppo_prepare(&a, s);
}

hipError_t ppo_launch_grad(const dart_lmpc_ppo_config* c, int n, long long total, int M, const int32_t* sample,
                           const int32_t* idx, const float* rec_obs, const float* rec_action, const float* rec_logp,
                           const float* weights, const float* critic, char* ws, int mb, hipStream_t s,
                           PpoPop pop = {}) {
    const dartmpc::PpoWorkspace L = dartmpc::ppo_workspace(n, mb);
    dartmpc::PpoGradArgs a;
    a.n = n; a.M = M; a.rec_total = total;
    dartmpc::ppo_hyper_set(a, dartmpc::ppo_hyper(hyper_row(c)));
    a.log_std_min = (float)c->log_std_min; a.log_std_max = (float)c->log_std_max;
    a.sample = sample; a.idx = idx; a.rec_obs = rec_obs; a.rec_action = rec_action; a.rec_logp = rec_logp;
    a.adv_n = reinterpret_cast<const float*>(ws + L.adv_n); a.ret_n = reinterpret_cast<const float*>(ws + L.ret_n);
    a.actor = weights; a.critic = critic;
    a.part = reinterpret_cast<float*>(ws + L.part); a.loss_part = reinterpret_cast<float*>(ws + L.loss_part);
    if (pop.P > 0) {
        const dartmpc::PpoGradPopArgs q{a, pop.P, pop.ws_stride, pop.idx_stride, pop.hyper};
        return dartmpc_launch_ppo_grad_pop(&q, s);
    }
    return dartmpc_launch_ppo_grad(&a, s);
}

// from_tiles: sum the workspace's partials of a mini-batch of M; otherwise take the packed gradient `grad`
hipError_t ppo_launch_apply(const dart_lmpc_ppo_config* c, int n, int M, bool from_tiles, const float* grad,
                            const float* terms_in, bool do_step, float* grad_out, float* terms_out, float* weights,
                            float* critic, float* adam, int32_t* adam_step, double* stats, float* step_log,
                            int step_in_call, char* ws, int mb, hipStream_t s, PpoPop pop = {}) {
    const dartmpc::PpoWorkspace L = dartmpc::ppo_workspace(n, mb);
    dartmpc::PpoApplyArgs a;
    a.tiles = from_tiles ? (M + dartmpc::kPpoTile - 1) / dartmpc::kPpoTile : 1;
    a.M = M; a.do_step = do_step ? 1 : 0; a.step_in_call = step_in_call;
    dartmpc::ppo_hyper_set(a, dartmpc::ppo_hyper(hyper_row(c)));
    a.log_std_min = (float)c->log_std_min; a.log_std_max = (float)c->log_std_max;
    a.part = from_tiles ? reinterpret_cast<const float*>(ws + L.part) : grad;
    a.loss_part = from_tiles ? reinterpret_cast<const float*>(ws + L.loss_part) : nullptr;
    a.terms_in = terms_in;
    a.grad = grad_out ? grad_out : reinterpret_cast<float*>(ws + L.grad);
    a.terms = terms_out ? terms_out : reinterpret_cast<float*>(ws + L.terms);
    a.actor = weights; a.critic = critic; a.adam = adam; a.adam_step = adam_step;
    a.step_log = step_log; a.stat_sum = reinterpret_cast<double*>(ws + L.stat_sum); a.stats = stats;
    if (pop.P > 0) {
        const dartmpc::PpoApplyPopArgs q{a, pop.P, pop.ws_stride, pop.hyper};
        return dartmpc_launch_ppo_apply_pop(&q, s);
    }
    return dartmpc_launch_ppo_apply(&a, s);
}

}  // namespace

int dart_lmpc_ppo_prepare_dev(int n, int rec_total, const int32_t* sample, const double* adv, const double* ret,
                              float* adv_norm_out, float* ret_norm_out, void* workspace, void* stream) {
    if (n < 1 || rec_total < 1 || !sample || !adv || !ret || !workspace) return DART_MPC_EINVAL;
    return ppo_launch_prepare(n, rec_total, sample, adv, ret, adv_norm_out, ret_norm_out, (char*)workspace, 1,
                              (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_ppo_grad_dev(const dart_lmpc_ppo_config* cfg, int n, int rec_total, int M, const int32_t* sample,
                           const int32_t* idx, const float* rec_obs, const float* rec_action, const float* rec_logp,
                           const float* weights, const float* critic, float* grad_out, float* terms_out,
                           void* workspace, void* stream) {
    if (!ppo_cfg_ok(cfg) || n < 1 || rec_total < 1 || M < 1 || M > dartmpc::kPpoMaxBatch) return DART_MPC_EINVAL;
    if (!sample || !idx || !rec_obs || !rec_action || !rec_logp || !weights || !critic || !grad_out || !terms_out ||
        !workspace) return DART_MPC_EINVAL;
    if (!aligned16(weights) || !aligned16(critic)) return DART_MPC_EINVAL;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = ppo_launch_grad(cfg, n, rec_total, M, sample, idx, rec_obs, rec_action, rec_logp, weights, critic,
                                   ws, M, s);
    if (e == hipSuccess)
        e = ppo_launch_apply(cfg, n, M, true, nullptr, nullptr, false, grad_out, terms_out, const_cast<float*>(weights),
                             const_cast<float*>(critic), nullptr, nullptr, nullptr, nullptr, 0, ws, M, s);
    return e == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_ppo_apply_dev(const dart_lmpc_ppo_config* cfg, const float* grad, const float* terms, float* weights,
                            float* critic, float* adam, int32_t* adam_step, double* stats, float* step_log,
                            int step_in_call, void* workspace, void* stream) {
    if (!ppo_cfg_ok(cfg) || !grad || !weights || !critic || !adam || !adam_step || !workspace || step_in_call < 0)
        return DART_MPC_EINVAL;
    if (!aligned16(weights) || !aligned16(critic)) return DART_MPC_EINVAL;
    // (the blocks this launch uses lie at fixed offsets in front of the workspace: the layout of any n serves)
    return ppo_launch_apply(cfg, 1, 1, false, grad, terms, true, nullptr, nullptr, weights, critic, adam, adam_step,
                            stats, step_log, step_in_call, (char*)workspace, 1, (hipStream_t)stream) == hipSuccess
               ? DART_MPC_OK : DART_MPC_EHIP;
}

namespace {

int ppo_update_check(const dart_lmpc_ppo_config* cfg, int n, int rec_total, const void* sample, const void* perm,
                     const void* rec_obs, const void* rec_action, const void* rec_logp, const void* adv,
                     const void* ret, const void* weights, const void* critic, const void* adam,
                     const void* adam_step, const void* stats) {
    if (!ppo_cfg_ok(cfg) || n < 1 || rec_total < 1) return DART_MPC_EINVAL;
    if (!sample || (!perm && cfg->epochs > 0) || !rec_obs || !rec_action || !rec_logp || !adv || !ret || !weights ||
        !critic || !adam || !adam_step || !stats) return DART_MPC_EINVAL;
    if (!aligned16(weights) || !aligned16(critic)) return DART_MPC_EINVAL;
    return DART_MPC_OK;
}

// The update's launch sequence, stated here alone: prepare, then for every epoch the mini-batches of its permutation
// (perm [epochs][n]; the last one ragged), each a grad and an apply.  ws is laid out for (n, mini_batch_size); with
// pop every launch is the population's (sample [P][n], perm [P][epochs][n], the nets, adam and stats per learner).
hipError_t ppo_launch_update(const dart_lmpc_ppo_config* c, int n, long long total, const int32_t* sample,
                             const int32_t* perm, const float* rec_obs, const float* rec_action,
                             const float* rec_logp, const double* adv, const double* ret, float* weights,
                             float* critic, float* adam, int32_t* adam_step, double* stats, float* step_log,
                             float* adv_out, float* ret_out, char* ws, hipStream_t s, PpoPop pop = {}) {
    const int mb = c->mini_batch_size;
    hipError_t e = ppo_launch_prepare(n, total, sample, adv, ret, adv_out, ret_out, ws, mb, s, pop);
    int step = 0;
    for (int ep = 0; ep < c->epochs && e == hipSuccess; ++ep) {
        const int32_t* row = perm + (size_t)ep * n;
        for (int start = 0; start < n && e == hipSuccess; start += mb, ++step) {
            const int M = n - start < mb ? n - start : mb;
            e = ppo_launch_grad(c, n, total, M, sample, row + start, rec_obs, rec_action, rec_logp, weights, critic, ws,
                                mb, s, pop);
            if (e == hipSuccess)
                e = ppo_launch_apply(c, n, M, true, nullptr, nullptr, true, nullptr, nullptr, weights, critic, adam,
                                     adam_step, stats, step_log, step, ws, mb, s, pop);
        }
    }
    return e;
}

}  // namespace

int dart_lmpc_ppo_update_dev(const dart_lmpc_ppo_config* cfg, int n, int rec_total, const int32_t* sample,
                             const int32_t* perm, const float* rec_obs, const float* rec_action,
                             const float* rec_logp, const double* adv, const double* ret, float* weights,
                             float* critic, float* adam, int32_t* adam_step, double* stats, float* step_log,
                             float* adv_norm_out, float* ret_norm_out, void* workspace, void* stream) {
    if (int rc = ppo_update_check(cfg, n, rec_total, sample, perm, rec_obs, rec_action, rec_logp, adv, ret, weights,
                                  critic, adam, adam_step, stats)) return rc;
    if (!workspace) return DART_MPC_EINVAL;
    return ppo_launch_update(cfg, n, rec_total, sample, perm, rec_obs, rec_action, rec_logp, adv, ret, weights, critic,
                             adam, adam_step, stats, step_log, adv_norm_out, ret_norm_out, (char*)workspace,
                             (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_ppo_update(const dart_lmpc_ppo_config* cfg, int n, int rec_total, const int32_t* sample,
                         const int32_t* perm, const float* rec_obs, const float* rec_action, const float* rec_logp,
                         const double* adv, const double* ret, float* weights, float* critic, float* adam,
                         int32_t* adam_step, double* stats, float* step_log, float* adv_norm_out,
                         float* ret_norm_out) {
    if (int rc = ppo_update_check(cfg, n, rec_total, sample, perm, rec_obs, rec_action, rec_logp, adv, ret, weights,
                                  critic, adam, adam_step, stats)) return rc;
    for (int i = 0; i < n; ++i)
        if (sample[i] < 0 || sample[i] >= rec_total) return DART_MPC_EINVAL;
    const size_t np = (size_t)cfg->epochs * n;
    for (size_t i = 0; i < np; ++i)
        if (perm[i] < 0 || perm[i] >= n) return DART_MPC_EINVAL;
    if (cfg->epochs == 0) { stats[0] = stats[1] = stats[2] = 0.0; }
    // only the rows sample names travel: they are compacted on the way up (the device entry gathers through
    // sample, so it is handed the identity) -- rows past an instance's record count are never read
    DART_DEVICE_STAGE(D, S);
    const size_t N = (size_t)n, P = dartmpc::kPpoParams;
    const size_t steps = (size_t)cfg->epochs * ((N + cfg->mini_batch_size - 1) / cfg->mini_batch_size);
    const size_t ws_bytes = dartmpc::ppo_workspace(n, cfg->mini_batch_size).bytes;
    const size_t staged = sizeof(int32_t) * (N + np + 1) + sizeof(float) * (N * (kHist + kAct + 1) + 3 * P + 4 * steps + 2 * N) +
                          sizeof(double) * (2 * N + 3) + 20 * 256;
    if (S.reserve(staged + ws_bytes, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    auto at = [&](size_t i) { return sample[i]; };
    auto iota = [n](int32_t* q) { for (int i = 0; i < n; ++i) q[i] = i; };
    const int32_t* d_id = S.in_with<int32_t>(N, iota);
    const float *d_obs = S.in_rows(rec_obs, N, kHist, at), *d_act = S.in_rows(rec_action, N, kAct, at);
    const float* d_lp = S.in_rows(rec_logp, N, 1, at);
    const double *d_adv = S.in_rows(adv, N, 1, at), *d_ret = S.in_rows(ret, N, 1, at);
    const int32_t* d_perm = S.in(perm, np);
    float* d_w = S.inout(weights, (size_t)dartmpc::kPpoActorN);
    float* d_c = S.inout(critic, (size_t)dartmpc::kPpoCriticN);
    float* d_adam = S.inout(adam, 2 * P);
    int32_t* d_step = S.inout(adam_step, (size_t)1);
    double* d_stats = S.inout(stats, (size_t)3);
    float* d_log = S.inout(step_log, 4 * steps);
    float* d_an = S.inout(adv_norm_out, N);
    float* d_rn = S.inout(ret_norm_out, N);
    char* ws = S.din + S.in_off;
    hipError_t e = S.upload(D->stream);
    int rc = DART_MPC_OK;
    if (e == hipSuccess)
        rc = dart_lmpc_ppo_update_dev(cfg, n, n, d_id, d_perm, d_obs, d_act, d_lp, d_adv, d_ret, d_w, d_c, d_adam, d_step,
                                      d_stats, d_log, d_an, d_rn, ws, D->stream);
    if (rc != DART_MPC_OK) {
        (void)hipStreamSynchronize(D->stream);
        return rc;
    }
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
    return DART_MPC_OK;
}

int dart_lmpc_critic_value_dev(int n, const float* critic, const float* obs, float* value_out, void* stream) {
    if (n < 0) return DART_MPC_EINVAL;
    if (n == 0) return DART_MPC_OK;
    if (!critic || !obs || !value_out) return DART_MPC_EINVAL;
    const dartmpc::CriticValueArgs a{n, critic, obs, value_out};
    return dartmpc_launch_critic_value(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_critic_value(int n, const float* critic, const float* obs, float* value_out) {
    if (n < 0) return DART_MPC_EINVAL;
    if (n == 0) return DART_MPC_OK;
    if (!critic || !obs || !value_out) return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    const size_t N = (size_t)n;
    if (S.reserve(sizeof(float) * (N * kHist + dartmpc::kPpoCriticN + N) + 4 * 256, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    dartmpc::CriticValueArgs a;
    a.n = n; a.critic = S.in(critic, (size_t)dartmpc::kPpoCriticN); a.obs = S.in(obs, N * kHist);
    a.value = S.inout(value_out, N);
    if (!D->run([&](hipStream_t s) { return dartmpc_launch_critic_value(&a, s); })) return DART_MPC_EHIP;
    return DART_MPC_OK;
}

// ---- whole PPO training iterations on the device (lmpc_train.hip) ---------------------------------------------

int dart_lmpc_philox_dev(int n, const uint32_t* in, uint32_t* out, void* stream) {
    if (n < 0) return DART_MPC_EINVAL;
    if (n == 0) return DART_MPC_OK;
    if (!in || !out) return DART_MPC_EINVAL;
    dartmpc::PhiloxArgs a;
    a.n = n; a.in = in; a.out = out;
    return dartmpc_launch_philox(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

namespace {

hipError_t launch_noise(uint64_t seed, int iteration, int steps, int B, float* out, hipStream_t s) {
    dartmpc::NoiseArgs a;
    a.n = (long long)steps * B * kAct;
    a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32); a.iteration = (uint32_t)iteration;
    a.out = out;
    return dartmpc_launch_lmpc_noise(&a, s);
}

// limit = n: the permutations; limit = m < n: their first m entries (rows of m)
hipError_t launch_perms(uint64_t seed, int iteration, int epochs, int n, int32_t* perm, uint32_t* key_out,
                        hipStream_t s, uint32_t rng_stream = dartmpc::kStreamPerm, int limit = -1) {
    dartmpc::PermArgs a;
    a.n = n; a.epochs = epochs; a.limit = limit < 0 ? n : limit;
    a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32); a.iteration = (uint32_t)iteration;
    a.stream = rng_stream;
    a.perm = perm; a.key_out = key_out;
    return dartmpc_launch_lmpc_perms(&a, s);
}

// (the Philox block index is 32 bits wide: 4 * 2^32 elements at the most)
bool noise_shape_ok(int iteration, int steps, int B) {
    return iteration >= 0 && steps >= 0 && B >= 0 && (long long)steps * B * kAct <= (1LL << 34);
}

int mean_update_args(const dart_lmpc_policy_config* cfg, int B, const float* weights, dartmpc::MeanUpdateArgs& a) {
    dartmpc::PolicyArgs pa;
    if (policy_args(cfg, B, weights, pa) != DART_MPC_OK) return DART_MPC_EINVAL;
    a.B = B; a.learner_B = 0; a.w = pa.w;
    a.max_delta = pa.max_delta; a.k_max = pa.k_max; a.min_k = pa.min_k; a.k_ceiling_margin = pa.k_ceiling_margin;
    a.action_scale = pa.action_scale; a.smooth_alpha = pa.smooth_alpha;
    return DART_MPC_OK;
}

}  // namespace

int dart_lmpc_noise_dev(uint64_t seed, int iteration, int steps, int B, float* noise_out, void* stream) {
    if (!noise_shape_ok(iteration, steps, B)) return DART_MPC_EINVAL;
    if (steps == 0 || B == 0) return DART_MPC_OK;
    if (!noise_out) return DART_MPC_EINVAL;
    return launch_noise(seed, iteration, steps, B, noise_out, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK
                                                                                                  : DART_MPC_EHIP;
}

int dart_lmpc_noise(uint64_t seed, int iteration, int steps, int B, float* noise_out) {
    if (!noise_shape_ok(iteration, steps, B)) return DART_MPC_EINVAL;
    if (steps == 0 || B == 0) return DART_MPC_OK;
    if (!noise_out) return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    const size_t n = (size_t)steps * B * kAct;
    if (S.reserve(0, sizeof(float) * n + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    float* d = S.out<float>(n);
    if (!D->run([&](hipStream_t s) { return launch_noise(seed, iteration, steps, B, d, s); })) return DART_MPC_EHIP;
    S.take(noise_out, d, n);
    return DART_MPC_OK;
}

int dart_lmpc_perms_dev(uint64_t seed, int iteration, int epochs, int n, int32_t* perm_out, uint32_t* key_out,
                        void* stream) {
    if (iteration < 0 || epochs < 0 || n < 0) return DART_MPC_EINVAL;
    if (epochs == 0 || n == 0) return DART_MPC_OK;
    if (!perm_out) return DART_MPC_EINVAL;
    return launch_perms(seed, iteration, epochs, n, perm_out, key_out, (hipStream_t)stream) == hipSuccess
               ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_perms(uint64_t seed, int iteration, int epochs, int n, int32_t* perm_out, uint32_t* key_out) {
    if (iteration < 0 || epochs < 0 || n < 0) return DART_MPC_EINVAL;
    if (epochs == 0 || n == 0) return DART_MPC_OK;
    if (!perm_out) return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    const size_t m = (size_t)epochs * n;
    if (S.reserve(0, 2 * (sizeof(int32_t) * m + 256)) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    int32_t* d = S.out<int32_t>(m);
    uint32_t* dk = key_out ? S.out<uint32_t>(m) : nullptr;
    auto launch = [&](hipStream_t s) { return launch_perms(seed, iteration, epochs, n, d, dk, s); };
    if (!D->run(launch)) return DART_MPC_EHIP;
    S.take(perm_out, d, m);
    S.take(key_out, dk, m);
    return DART_MPC_OK;
}

int dart_lmpc_mean_param_update_dev(const dart_lmpc_policy_config* cfg, int B, const float* weights,
                                    const float* history, double* model_params, double* current_k, float* mean_out,
                                    void* stream) {
    dartmpc::MeanUpdateArgs a;
    if (mean_update_args(cfg, B, weights, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    if (!history || !model_params || !current_k) return DART_MPC_EINVAL;
    a.history = history; a.model_params = model_params; a.current_k = current_k; a.mean_out = mean_out;
    return dartmpc_launch_lmpc_mean_update(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_mean_param_update(const dart_lmpc_policy_config* cfg, int B, const float* weights, const float* history,
                                double* model_params, double* current_k, float* mean_out) {
    dartmpc::MeanUpdateArgs a;
    if (mean_update_args(cfg, B, weights, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    if (!history || !model_params || !current_k) return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    const size_t nB = (size_t)B;
    if (S.reserve(sizeof(float) * ((size_t)DART_LMPC_POLICY_NWEIGHTS + kHist * nB) + sizeof(double) * 68 * nB + 8 * 256,
                  sizeof(float) * kAct * nB + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const float* d_w = S.in(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS);
    if (mean_update_args(cfg, B, d_w, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    a.history = S.in(history, kHist * nB);
    a.model_params = S.inout(model_params, kAct * nB);
    a.current_k = S.inout(current_k, kAct * nB);
    a.mean_out = mean_out ? S.out<float>(kAct * nB) : nullptr;
    if (!D->run([&](hipStream_t s) { return dartmpc_launch_lmpc_mean_update(&a, s); })) return DART_MPC_EHIP;
    S.take(mean_out, a.mean_out, kAct * nB);
    return DART_MPC_OK;
}

// ---- the global-buffer update (rlmpc2.py:823-874): choice, record gather, GAE over one sequence ----------------

int dart_lmpc_perms_stream_dev(uint64_t seed, int iteration, int rng_stream, int epochs, int n, int32_t* perm_out,
                               uint32_t* key_out, void* stream) {
    if (iteration < 0 || epochs < 0 || n < 0 || rng_stream < 0) return DART_MPC_EINVAL;
    if (epochs == 0 || n == 0) return DART_MPC_OK;
    if (!perm_out) return DART_MPC_EINVAL;
    return launch_perms(seed, iteration, epochs, n, perm_out, key_out, (hipStream_t)stream, (uint32_t)rng_stream) ==
                   hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_choice_dev(uint64_t seed, int iteration, int n, int m, int32_t* choice_out, void* stream) {
    if (iteration < 0 || m < 1 || m > n || !choice_out) return DART_MPC_EINVAL;
    return launch_perms(seed, iteration, 1, n, choice_out, nullptr, (hipStream_t)stream, dartmpc::kStreamChoice, m) ==
                   hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_choice(uint64_t seed, int iteration, int n, int m, int32_t* choice_out) {
    if (iteration < 0 || m < 1 || m > n || !choice_out) return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(0, sizeof(int32_t) * (size_t)m + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    int32_t* d = S.out<int32_t>((size_t)m);
    auto launch = [&](hipStream_t s) { return launch_perms(seed, iteration, 1, n, d, nullptr, s, dartmpc::kStreamChoice, m); };
    if (!D->run(launch)) return DART_MPC_EHIP;
    S.take(choice_out, d, (size_t)m);
    return DART_MPC_OK;
}

int dart_lmpc_global_rows(int n, int32_t* m_out, int32_t* G_out) {
    if (n < 1 || !m_out || !G_out) return DART_MPC_EINVAL;
    int m, G;
    dartmpc::global_rows(n, m, G);
    *m_out = m; *G_out = G;
    return DART_MPC_OK;
}

int dart_lmpc_global_fill_after(int n, int fill, int iterations) {
    if (n < 1 || iterations < 0 || fill < 0 || fill >= n) return DART_MPC_EINVAL;
    int m, G;
    dartmpc::global_rows(n, m, G);
    if (fill % m != 0) return DART_MPC_EINVAL;
    const long long period = G / m;
    return (int)(((long long)(fill / m) + iterations) % period) * m;
}

size_t dart_lmpc_global_workspace_bytes(int n, int epochs, int mini_batch_size) {
    if (n < 1 || epochs < 0 || mini_batch_size < 1 || mini_batch_size > dartmpc::kPpoMaxBatch) return 0;
    if ((long long)n + n / 4 > 0x7fffffffLL) return 0;
    int m, G;
    dartmpc::global_rows(n, m, G);
    return dartmpc::global_workspace(1, n, G, epochs, mini_batch_size).bytes;
}

namespace {

int global_append_check(const dart_lmpc_global_buffer* g, int m, int n, int rec_total, const void* sample,
                        const void* choice, const void* rec_obs, const void* rec_action, const void* rec_logp,
                        const void* rec_value, const void* rec_reward, const void* rec_done) {
    if (!g || m < 1 || n < 1 || rec_total < 1 || g->fill < 0 || (long long)g->fill + m > g->capacity)
        return DART_MPC_EINVAL;
    if (!sample || !choice || !rec_obs || !rec_action || !rec_logp || !rec_value || !rec_reward || !rec_done ||
        !g->obs || !g->action || !g->logp || !g->value || !g->reward || !g->done) return DART_MPC_EINVAL;
    return DART_MPC_OK;
}

hipError_t launch_global_append(const dart_lmpc_global_buffer* g, int fill, int m, int n, int rec_total,
                                const int32_t* sample, const int32_t* choice, const float* rec_obs,
                                const float* rec_action, const float* rec_logp, const float* rec_value,
                                const double* rec_reward, const float* rec_done, hipStream_t s) {
    dartmpc::GbufAppendArgs a;
    a.m = m; a.n = n; a.fill = fill; a.rec_total = rec_total; a.sample = sample; a.choice = choice;
    a.rec_obs = rec_obs; a.rec_action = rec_action; a.rec_logp = rec_logp; a.rec_value = rec_value;
    a.rec_reward = rec_reward; a.rec_done = rec_done;
    a.obs = g->obs; a.action = g->action; a.logp = g->logp; a.value = g->value; a.reward = g->reward; a.done = g->done;
    return dartmpc_launch_lmpc_gbuf_append(&a, s);
}

hipError_t launch_gae_seq(int G, double gamma, double lam, const double* reward, const float* value,
                          const float* done, const float* last_value, double* adv, double* ret, hipStream_t s) {
    dartmpc::GaeSeqArgs a;
    a.G = G; a.gamma = gamma; a.lam = lam; a.reward = reward; a.value = value; a.done = done;
    a.last_value = last_value; a.adv = adv; a.ret = ret;
    return dartmpc_launch_lmpc_gae_seq(&a, s);
}

// ---- a population's forms: every learner in one launch (lmpc_train.h) ----

bool pop_shape_ok(int P, const uint64_t* seeds) { return P >= 1 && P <= DART_LMPC_POP_MAX && seeds; }

// the learners' generator keys travel in the launch arguments
dartmpc::PopKeys pop_keys(int P, const uint64_t* seeds) {
    dartmpc::PopKeys keys{};
    for (int l = 0; l < P; ++l) {
        keys.k[l][0] = (uint32_t)(seeds[l] & 0xffffffffu);
        keys.k[l][1] = (uint32_t)(seeds[l] >> 32);
    }
    return keys;
}

// launch_perms per learner: perm [P][epochs][limit]
hipError_t launch_perms_pop(int P, const dartmpc::PopKeys& keys, int iteration, int epochs, int n, int32_t* perm,
                            hipStream_t s, uint32_t rng_stream, int limit) {
    dartmpc::PermPopArgs pa;
    pa.a.n = n; pa.a.epochs = epochs; pa.a.limit = limit; pa.a.key0 = pa.a.key1 = 0;
    pa.a.iteration = (uint32_t)iteration; pa.a.stream = rng_stream; pa.a.perm = perm; pa.a.key_out = nullptr;
    pa.P = P; pa.keys = keys;
    return dartmpc_launch_lmpc_perms_pop(&pa, s);
}

// g: P buffers stacked g->capacity rows apart; sample [P][n], choice [P][m]
hipError_t launch_global_append_pop(const dart_lmpc_global_buffer* g, int P, int fill, int m, int n,
                                    long long rec_total, const int32_t* sample, const int32_t* choice,
                                    const float* rec_obs, const float* rec_action, const float* rec_logp,
                                    const float* rec_value, const double* rec_reward, const float* rec_done,
                                    hipStream_t s) {
    dartmpc::GbufAppendPopArgs q;
    dartmpc::GbufAppendArgs& a = q.a;
    a.m = m; a.n = n; a.fill = fill; a.rec_total = rec_total; a.sample = sample; a.choice = choice;
    a.rec_obs = rec_obs; a.rec_action = rec_action; a.rec_logp = rec_logp; a.rec_value = rec_value;
    a.rec_reward = rec_reward; a.rec_done = rec_done;
    a.obs = g->obs; a.action = g->action; a.logp = g->logp; a.value = g->value; a.reward = g->reward; a.done = g->done;
    q.P = P; q.capacity = g->capacity;
    return dartmpc_launch_lmpc_gbuf_append_pop(&q, s);
}

hipError_t launch_gae_seq_pop(int P, int capacity, int G, double gamma, double lam, const double* reward,
                              const float* value, const float* done, const float* last_value, double* adv,
                              double* ret, hipStream_t s) {
    dartmpc::GaeSeqPopArgs q;
    q.a.G = G; q.a.gamma = gamma; q.a.lam = lam; q.a.reward = reward; q.a.value = value; q.a.done = done;
    q.a.last_value = last_value; q.a.adv = adv; q.a.ret = ret;
    q.P = P; q.capacity = capacity;
    return dartmpc_launch_lmpc_gae_seq_pop(&q, s);
}

}  // namespace

int dart_lmpc_choice_pop_dev(int P, const uint64_t* seeds, int iteration, int n, int m, int32_t* choice_out,
                             void* stream) {
    if (!pop_shape_ok(P, seeds) || iteration < 0 || m < 1 || m > n || !choice_out) return DART_MPC_EINVAL;
    return launch_perms_pop(P, pop_keys(P, seeds), iteration, 1, n, choice_out, (hipStream_t)stream,
                            dartmpc::kStreamChoice, m) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_global_append_pop_dev(const dart_lmpc_global_buffer* g, int P, int m, int n, int rec_total,
                                    const int32_t* sample, const int32_t* choice, const float* rec_obs,
                                    const float* rec_action, const float* rec_logp, const float* rec_value,
                                    const double* rec_reward, const float* rec_done, void* stream) {
    if (P < 1 || P > DART_LMPC_POP_MAX) return DART_MPC_EINVAL;
    if (int rc = global_append_check(g, m, n, rec_total, sample, choice, rec_obs, rec_action, rec_logp, rec_value,
                                     rec_reward, rec_done)) return rc;
    if (!aligned16(rec_obs) || !aligned16(g->obs)) return DART_MPC_EINVAL;
    return launch_global_append_pop(g, P, g->fill, m, n, rec_total, sample, choice, rec_obs, rec_action, rec_logp,
                                    rec_value, rec_reward, rec_done, (hipStream_t)stream) == hipSuccess
               ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_gae_seq_pop_dev(int P, int capacity, int G, double gamma, double lam, const double* reward,
                              const float* value, const float* done, const float* last_value, double* adv,
                              double* ret, void* stream) {
    if (P < 1 || P > DART_LMPC_POP_MAX || G < 0 || capacity < G) return DART_MPC_EINVAL;
    if (G == 0) return DART_MPC_OK;
    if (!reward || !value || !done || !last_value || !adv || !ret) return DART_MPC_EINVAL;
    return launch_gae_seq_pop(P, capacity, G, gamma, lam, reward, value, done, last_value, adv, ret,
                              (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_global_append_dev(const dart_lmpc_global_buffer* g, int m, int n, int rec_total, const int32_t* sample,
                                const int32_t* choice, const float* rec_obs, const float* rec_action,
                                const float* rec_logp, const float* rec_value, const double* rec_reward,
                                const float* rec_done, void* stream) {
    if (int rc = global_append_check(g, m, n, rec_total, sample, choice, rec_obs, rec_action, rec_logp, rec_value,
                                     rec_reward, rec_done)) return rc;
    if (!aligned16(rec_obs) || !aligned16(g->obs)) return DART_MPC_EINVAL;    // (the rows move in 16-byte pieces)
    return launch_global_append(g, g->fill, m, n, rec_total, sample, choice, rec_obs, rec_action, rec_logp, rec_value,
                                rec_reward, rec_done, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_global_append(const dart_lmpc_global_buffer* g, int m, int n, int rec_total, const int32_t* sample,
                            const int32_t* choice, const float* rec_obs, const float* rec_action,
                            const float* rec_logp, const float* rec_value, const double* rec_reward,
                            const float* rec_done) {
    if (int rc = global_append_check(g, m, n, rec_total, sample, choice, rec_obs, rec_action, rec_logp, rec_value,
                                     rec_reward, rec_done)) return rc;
    for (int j = 0; j < m; ++j)
        if (choice[j] < 0 || choice[j] >= n) return DART_MPC_EINVAL;
    for (int i = 0; i < n; ++i)
        if (sample[i] < 0 || sample[i] >= rec_total) return DART_MPC_EINVAL;
    // only the m drawn records travel: they are compacted on the way up (sample and choice become the identity)
    DART_DEVICE_STAGE(D, S);
    const size_t M = (size_t)m, F = sizeof(float);
    const size_t row = F * (kHist + kAct + 3) + sizeof(double);
    if (S.reserve(2 * (M * row + 8 * 256) + sizeof(int32_t) * M + 256, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    auto at = [&](size_t j) { return sample[choice[j]]; };
    auto iota = [m](int32_t* q) { for (int j = 0; j < m; ++j) q[j] = j; };
    const int32_t* d_id = S.in_with<int32_t>(M, iota);
    const float *d_obs = S.in_rows(rec_obs, M, kHist, at), *d_act = S.in_rows(rec_action, M, kAct, at);
    const float *d_lp = S.in_rows(rec_logp, M, 1, at), *d_vl = S.in_rows(rec_value, M, 1, at);
    const double* d_rw = S.in_rows(rec_reward, M, 1, at);
    const float* d_dn = S.in_rows(rec_done, M, 1, at);
    const size_t f0 = (size_t)g->fill;
    dart_lmpc_global_buffer d = *g;                 // rows fill .. fill + m - 1 alone, as rows 0 .. m - 1
    d.obs = S.inout(g->obs + f0 * kHist, M * kHist); d.action = S.inout(g->action + f0 * kAct, M * kAct);
    d.logp = S.inout(g->logp + f0, M); d.value = S.inout(g->value + f0, M);
    d.reward = S.inout(g->reward + f0, M); d.done = S.inout(g->done + f0, M);
    auto launch = [&](hipStream_t s) {
        return launch_global_append(&d, 0, m, m, m, d_id, d_id, d_obs, d_act, d_lp, d_vl, d_rw, d_dn, s);
    };
    if (!D->run(launch)) return DART_MPC_EHIP;
    return DART_MPC_OK;
}

int dart_lmpc_gae_seq_dev(int G, double gamma, double lam, const double* reward, const float* value,
                          const float* done, const float* last_value, double* adv, double* ret, void* stream) {
    if (G < 0) return DART_MPC_EINVAL;
    if (G == 0) return DART_MPC_OK;
    if (!reward || !value || !done || !last_value || !adv || !ret) return DART_MPC_EINVAL;
    return launch_gae_seq(G, gamma, lam, reward, value, done, last_value, adv, ret, (hipStream_t)stream) == hipSuccess
               ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_gae_seq(int G, double gamma, double lam, const double* reward, const float* value, const float* done,
                      const float* last_value, double* adv, double* ret) {
    if (G < 0) return DART_MPC_EINVAL;
    if (G == 0) return DART_MPC_OK;
    if (!reward || !value || !done || !last_value || !adv || !ret) return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    const size_t n = (size_t)G;
    if (S.reserve(sizeof(double) * 3 * n + sizeof(float) * (2 * n + 1) + 8 * 256, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const double* d_rw = S.in(reward, n);
    const float* d_vl = S.in(value, n);
    const float* d_dn = S.in(done, n);
    const float* d_lv = S.in(last_value, (size_t)1);
    double* d_adv = S.inout(adv, n);
    double* d_ret = S.inout(ret, n);
    auto launch = [&](hipStream_t s) { return launch_gae_seq(G, gamma, lam, d_rw, d_vl, d_dn, d_lv, d_adv, d_ret, s); };
    if (!D->run(launch)) return DART_MPC_EHIP;
    return DART_MPC_OK;
}

void dart_lmpc_train_config_default(dart_lmpc_train_config* c) {
    if (!c) return;
    c->seed = 0; c->iterations = 1; c->it0 = 0; c->steps = 256; c->mean_update = 1; c->track_best = 1;
    c->reserved = 0; c->gamma = 0.99; c->lam = 0.95;
}

size_t dart_lmpc_train_workspace_bytes(int B, int K, int record_every, int epochs, int mini_batch_size) {
    if (B < 1 || record_every < 1 || K < record_every || K % record_every != 0 || epochs < 0 || mini_batch_size < 1 ||
        mini_batch_size > dartmpc::kPpoMaxBatch) return 0;
    if ((long long)(K / record_every) * B > 0x7fffffffLL) return 0;
    return dartmpc::train_workspace(1, B, K, record_every, epochs, mini_batch_size).bytes;
}

namespace {

// the checks of the training entries that need neither the device nor the arrays' contents
int train_check(dart_mpc_handle* h, const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                const dart_lmpc_train_config* cfg, int B, const dart_lmpc_train_buffers* p, bool need_ws) {
    if (!cfg || !p || !rcfg) return fail(h, DART_MPC_EINVAL, "null training config, reward config or buffers");
    if (!ppo_cfg_ok(ppo)) return fail(h, DART_MPC_EINVAL, "bad PPO config");
    if (cfg->iterations < 0 || cfg->it0 < 0 || (long long)cfg->it0 + cfg->iterations > 0x7fffffffLL)
        return fail(h, DART_MPC_EINVAL, "training config: iterations >= 0, it0 >= 0");
    if (B < 1) return fail(h, DART_MPC_EINVAL, "training needs B >= 1");
    if (rcfg->record_every < 1 || cfg->steps < rcfg->record_every || cfg->steps % rcfg->record_every != 0)
        return fail(h, DART_MPC_EINVAL, "training config: steps must be a positive multiple of record_every");
    if ((long long)(cfg->steps / rcfg->record_every) * B > 0x7fffffffLL)
        return fail(h, DART_MPC_EINVAL, "too many samples");
    if (any_null({p->current_k, p->weights, p->critic, p->adam, p->adam_step, p->train_log, p->best_return,
                  p->best_weights, p->best_iter}) || (need_ws && !p->workspace))
        return fail(h, DART_MPC_EINVAL, "null pointer (training arrays)");
    return DART_MPC_OK;
}

// the checks of the global buffer that need neither the device nor the arrays' contents (n = R B samples)
int global_check(dart_mpc_handle* h, const dart_lmpc_global_buffer* g, int n, bool dev) {
    int m, G;
    dartmpc::global_rows(n, m, G);
    if (g->fill < 0 || g->fill >= n || g->fill % m != 0)
        return fail(h, DART_MPC_EINVAL, "global buffer: fill must be a multiple of m in [0, n)");
    if (g->capacity < G) return fail(h, DART_MPC_EINVAL, "global buffer: capacity below G");
    if (any_null({g->obs, g->action, g->logp, g->value, g->reward, g->done, g->global_log}) || (dev && !g->workspace))
        return fail(h, DART_MPC_EINVAL, "null pointer (global buffer)");
    if (dev && !aligned16(g->obs)) return fail(h, DART_MPC_EINVAL, "global buffer: obs is not 16-byte aligned");
    return DART_MPC_OK;
}

// the checks of a population's shape: P learners of B instances each, R records per instance
int pop_check(dart_mpc_handle* h, const dart_lmpc_reward_config* rcfg, const dart_lmpc_train_config* cfg, int P,
              const uint64_t* seeds, int B) {
    if (P < 1 || P > DART_LMPC_POP_MAX) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
    if (!seeds) return fail(h, DART_MPC_EINVAL, "population: null seeds");
    if ((long long)P * B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "population: P * B larger than B_max");
    if ((long long)(cfg->steps / rcfg->record_every) * P * B > 0x7fffffffLL)
        return fail(h, DART_MPC_EINVAL, "too many samples");
    return DART_MPC_OK;
}

// Who trains.  P = 0: one learner of B instances in the single-learner launches, its generator keyed by `seed`;
// P >= 1: P learners of B instances each, stacked learner-major, in the population's launches, keyed by `keys`.  (A
// population of one is not the single learner: the kernels differ, and the launch sequence is part of the entries.)
struct Learners {
    int P, B;
    uint64_t seed;
    dartmpc::PopKeys keys;
    int count() const { return P > 0 ? P : 1; }
};

// rows between the learners' blocks of the global workspace: the buffers' capacity; the single learner's workspace
// is addressed by its buffer's rows, all below G
int global_stride(int P, int n, const dart_lmpc_global_buffer* g) {
    int m, G;
    dartmpc::global_rows(n, m, G);
    return P > 0 && g ? g->capacity : G;
}

// ---- the steps of an iteration whose launch depends on the form, each stated once (with ppo_launch_* above) ----

// the sample lists [count][R B]: the flat indices of a learner's records in the record arrays
hipError_t launch_sample(const Learners& w, int R, int32_t* out, hipStream_t s) {
    if (w.P > 0) {
        const dartmpc::PopSampleArgs a{w.P, w.B, R, out};
        return dartmpc_launch_lmpc_pop_sample(&a, s);
    }
    const dartmpc::IotaArgs a{R * w.B, out};
    return dartmpc_launch_iota(&a, s);
}

// the sample lists [count][G] over the buffers' rows, the buffers `stride` rows apart
hipError_t launch_global_sample(const Learners& w, int G, int stride, int32_t* out, hipStream_t s) {
    if (w.P > 0) {
        const dartmpc::PopGlobalSampleArgs a{w.P, G, stride, out};
        return dartmpc_launch_lmpc_pop_global_sample(&a, s);
    }
    const dartmpc::IotaArgs a{G, out};
    return dartmpc_launch_iota(&a, s);
}

hipError_t launch_noise(const Learners& w, int iteration, int steps, float* out, hipStream_t s) {
    if (w.P == 0) return launch_noise(w.seed, iteration, steps, w.B, out, s);
    dartmpc::NoisePopArgs a;
    a.n = (long long)steps * w.B * kAct; a.B = w.B; a.P = w.P; a.iteration = (uint32_t)iteration; a.keys = w.keys;
    a.out = out;
    return dartmpc_launch_lmpc_noise_pop(&a, s);
}

// every learner's critic on its n rows of obs: the learners' rows follow one another (obs_stride = 0) or start
// obs_stride rows apart
hipError_t launch_value(const Learners& w, int n, const float* critic, const float* obs, long long obs_stride,
                        float* value, hipStream_t s) {
    const dartmpc::CriticValueArgs a{n, critic, obs, value};
    if (w.P == 0) return dartmpc_launch_critic_value(&a, s);
    if (obs_stride == 0) {
        const dartmpc::CriticValuePopArgs q{a, w.P};
        return dartmpc_launch_critic_value_pop(&q, s);
    }
    const dartmpc::CriticValueStridePopArgs q{a, w.P, obs_stride};
    return dartmpc_launch_critic_value_stride_pop(&q, s);
}

hipError_t launch_perms(const Learners& w, int iteration, int epochs, int n, int32_t* perm, hipStream_t s,
                        uint32_t rng_stream, int limit) {
    if (w.P > 0) return launch_perms_pop(w.P, w.keys, iteration, epochs, n, perm, s, rng_stream, limit);
    return launch_perms(w.seed, iteration, epochs, n, perm, nullptr, s, rng_stream, limit);
}

hipError_t launch_global_append(const Learners& w, const dart_lmpc_global_buffer* g, int fill, int m, int n,
                                long long rec_total, const int32_t* sample, const int32_t* choice,
                                const dart_lmpc_train_buffers& p, hipStream_t s) {
    if (w.P > 0)
        return launch_global_append_pop(g, w.P, fill, m, n, rec_total, sample, choice, p.rec_obs, p.rec_action,
                                        p.rec_logp, p.rec_value, p.rec_reward, p.rec_done, s);
    return launch_global_append(g, fill, m, n, (int)rec_total, sample, choice, p.rec_obs, p.rec_action, p.rec_logp,
                                p.rec_value, p.rec_reward, p.rec_done, s);
}

hipError_t launch_gae_seq(const Learners& w, const dart_lmpc_global_buffer* g, int G, double gamma, double lam,
                          const float* last_value, double* adv, double* ret, hipStream_t s) {
    if (w.P > 0)
        return launch_gae_seq_pop(w.P, g->capacity, G, gamma, lam, g->reward, g->value, g->done, last_value, adv, ret, s);
    return launch_gae_seq(G, gamma, lam, g->reward, g->value, g->done, last_value, adv, ret, s);
}

// the log rows: `a` is learner 0's, row j of its `iterations`
hipError_t launch_train_log(const Learners& w, const dartmpc::TrainLogArgs& a, int iterations, hipStream_t s) {
    if (w.P == 0) return dartmpc_launch_lmpc_train_log(&a, s);
    const dartmpc::TrainLogPopArgs q{a, w.P, (long long)dartmpc::kTrainLogCols * iterations};
    return dartmpc_launch_lmpc_train_log_pop(&q, s);
}

hipError_t launch_global_log(const Learners& w, const dartmpc::GlobalLogArgs& a, int iterations, hipStream_t s) {
    if (w.P == 0) return dartmpc_launch_lmpc_global_log(&a, s);
    const dartmpc::GlobalLogPopArgs q{a, w.P, (long long)dartmpc::kGlobalLogCols * iterations};
    return dartmpc_launch_lmpc_global_log_pop(&q, s);
}

// The device form of the training entries: whole iterations enqueued on one stream.  P = 0:
// dart_lmpc_train_global_dev (g == nullptr: dart_lmpc_train_dev); P >= 1: dart_lmpc_train_pop_global_dev, every step
// issued once for all P learners (the P buffers of g are stacked learner-major, g->capacity rows apart), and with
// `hyper` (device, [P][kHyperCols]) dart_lmpc_train_pop_hyper_dev: both updates' kernels read learner l's row when
// they run, the host never does.  Every check runs before the first launch.
int train_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
              const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo, const dart_lmpc_train_config* cfg,
              int P, const uint64_t* seeds, int B, int reset_rows, const dart_lmpc_train_buffers* p,
              const dart_lmpc_global_buffer* g, void* stream, const double* hyper = nullptr) {
    DART_ENTER(h, -1);
    if (int rc = train_check(h, rcfg, ppo, cfg, B, p, true)) return rc;
    if (hyper && P < 1) return fail(h, DART_MPC_EINVAL, "a hyper-parameter table needs a population");
    if (P > 0)
        if (int rc = pop_check(h, rcfg, cfg, P, seeds, B)) return rc;
    if (!aligned16(p->weights) || !aligned16(p->critic))
        return fail(h, DART_MPC_EINVAL, "policy and critic weights must be 16-byte aligned");
    // the learners' keys travel in the launch arguments: nothing is read from seeds after this
    const Learners w{P, B, cfg->seed, P > 0 ? pop_keys(P, seeds) : dartmpc::PopKeys{}};
    const int NI = w.count() * B;                   // instances, learner-major
    const int K = cfg->steps, R = K / rcfg->record_every, n = R * B, mb = ppo->mini_batch_size;
    const long long rec_total = (long long)R * NI;
    if (g) {
        if (int rc = global_check(h, g, n, true)) return rc;
        if ((long long)w.count() * g->capacity > 0x7fffffffLL) return fail(h, DART_MPC_EINVAL, "too many buffer rows");
        if (!aligned16(p->rec_obs)) return fail(h, DART_MPC_EINVAL, "rec_obs is not 16-byte aligned");
    }
    void* s = stream_of(h, stream);
    auto collect = [&](int steps, const float* noise) {
        return lmpc_closed_loop(h, plant, pcfg, rcfg, true, NI, 0, steps, K, R, reset_rows, *p, noise, s, P > 0 ? B : 0);
    };
    // every check of the collection (configs, null pointers, B <= B_max, the handle's variant): zero steps
    if (int rc = collect(0, nullptr)) return rc;
    dartmpc::MeanUpdateArgs ma;
    if (mean_update_args(pcfg, NI, p->weights, ma) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
    ma.learner_B = P > 0 ? B : 0;
    ma.history = p->history; ma.model_params = p->model_params; ma.current_k = p->current_k; ma.mean_out = nullptr;
    if (cfg->iterations == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    const dartmpc::TrainWorkspace L = dartmpc::train_workspace(w.count(), B, K, rcfg->record_every, ppo->epochs, mb);
    char* ws = (char*)p->workspace;
    float* noise = (float*)(ws + L.noise);
    float* last_value = (float*)(ws + L.last_value);
    double* adv = (double*)(ws + L.adv);
    double* ret = (double*)(ws + L.ret);
    int32_t* sample = (int32_t*)(ws + L.sample);
    int32_t* perm = (int32_t*)(ws + L.perm);
    double* stats = (double*)(ws + L.stats);
    int32_t* ep0 = (int32_t*)(ws + L.ep0);
    hipStream_t hs = (hipStream_t)s;
    const PpoPop pop{P, L.ppo_stride, (size_t)ppo->epochs * n, hyper};
    // the global update's sizes, workspace and running fill, one for all learners (they share n; the host knows
    // every launch from n and g->fill)
    int gm = 0, gG = 0, g_fill = g ? g->fill : 0;
    dartmpc::global_rows(n, gm, gG);
    const int g_stride = global_stride(P, n, g);
    const dartmpc::GlobalWorkspace GL = dartmpc::global_workspace(w.count(), n, g_stride, ppo->epochs, mb);
    char* gws = g ? (char*)g->workspace : nullptr;
    auto gp = [&](size_t off) { return gws ? gws + off : nullptr; };
    int32_t* g_choice = (int32_t*)gp(GL.choice);
    double* g_adv = (double*)gp(GL.adv);
    double* g_ret = (double*)gp(GL.ret);
    float* g_last = (float*)gp(GL.last_value);
    int32_t* g_sample = (int32_t*)gp(GL.sample);
    int32_t* g_perm = (int32_t*)gp(GL.perm);
    double* g_stats = (double*)gp(GL.stats);
    const PpoPop gpop{P, GL.ppo_stride, (size_t)ppo->epochs * gG, hyper};
    const size_t stats_bytes = sizeof(double) * 3 * (size_t)w.count();
    HIPCHK(h, launch_sample(w, R, sample, hs), "sample list launch");
    for (int j = 0; j < cfg->iterations; ++j) {
        const int it = cfg->it0 + j;
        HIPCHK(h, hipMemsetAsync(p->nrec, 0, sizeof(int32_t) * (size_t)NI, hs), "clear nrec");
        HIPCHK(h, hipMemcpyAsync(ep0, p->episodes, sizeof(int32_t) * (size_t)NI, hipMemcpyDeviceToDevice, hs),
               "copy episodes");
        // (with epochs = 0 the update leaves its statistics untouched)
        if (ppo->epochs == 0) HIPCHK(h, hipMemsetAsync(stats, 0, stats_bytes, hs), "clear stats");
        HIPCHK(h, launch_noise(w, it, K, noise, hs), "noise launch");
        if (int rc = collect(K, noise)) return rc;
        HIPCHK(h, launch_value(w, B, p->critic, p->history, 0, last_value, hs), "critic value launch");
        HIPCHK(h, launch_gae(NI, R, cfg->gamma, cfg->lam, p->nrec, p->rec_reward, p->rec_value, p->rec_done, last_value,
                             adv, ret, hs), "GAE launch");
        HIPCHK(h, launch_perms(w, it, ppo->epochs, n, perm, hs, dartmpc::kStreamPerm, n), "permutation launch");
        HIPCHK(h, ppo_launch_update(ppo, n, rec_total, sample, perm, p->rec_obs, p->rec_action, p->rec_logp, adv, ret,
                                    p->weights, p->critic, p->adam, p->adam_step, stats, nullptr, nullptr, nullptr,
                                    ws + L.ppo, hs, pop), "PPO update launch");
        if (g) {
            // 6a: every learner draws m of this iteration's records without replacement and appends them behind the
            // rows it holds
            HIPCHK(h, launch_perms(w, it, 1, n, g_choice, hs, dartmpc::kStreamChoice, gm), "choice launch");
            HIPCHK(h, launch_global_append(w, g, g_fill, gm, n, rec_total, sample, g_choice, *p, hs),
                   "global buffer append launch");
            g_fill += gm;
            const int ran = g_fill >= n ? 1 : 0;
            const int logged_fill = g_fill;
            if (ran) {
                // 6b: every buffer holds G rows: one sequence each for GAE, then a full update on the learner's
                // optimizer
                HIPCHK(h, launch_value(w, 1, p->critic, g->obs + (size_t)(gG - 1) * kHist, g_stride, g_last, hs),
                       "critic value launch (global buffer)");
                HIPCHK(h, launch_gae_seq(w, g, gG, cfg->gamma, cfg->lam, g_last, g_adv, g_ret, hs),
                       "sequence GAE launch");
                HIPCHK(h, launch_global_sample(w, gG, g_stride, g_sample, hs), "sample list launch (global buffer)");
                if (ppo->epochs == 0) HIPCHK(h, hipMemsetAsync(g_stats, 0, stats_bytes, hs), "clear stats");
                HIPCHK(h, launch_perms(w, it, ppo->epochs, gG, g_perm, hs, dartmpc::kStreamGlobalPerm, gG),
                       "permutation launch (global buffer)");
                HIPCHK(h, ppo_launch_update(ppo, gG, (long long)w.count() * g_stride, g_sample, g_perm, g->obs,
                                            g->action, g->logp, g_adv, g_ret, p->weights, p->critic, p->adam,
                                            p->adam_step, g_stats, nullptr, nullptr, nullptr, gws + GL.ppo, hs, gpop),
                       "PPO update launch (global buffer)");
                g_fill = 0;
            }
            dartmpc::GlobalLogArgs ga;
            ga.fill = logged_fill; ga.ran = ran; ga.G = gG; ga.stats = g_stats;
            ga.row = g->global_log + (size_t)dartmpc::kGlobalLogCols * j;
            HIPCHK(h, launch_global_log(w, ga, cfg->iterations, hs), "global log launch");
        }
        if (cfg->mean_update) HIPCHK(h, dartmpc_launch_lmpc_mean_update(&ma, hs), "mean parameter update launch");
        dartmpc::TrainLogArgs la;
        la.B = B; la.K = K; la.R = R; la.n = n; la.iteration = it; la.track_best = cfg->track_best ? 1 : 0;
        la.ep0 = ep0; la.episodes = p->episodes; la.last_return = p->last_return; la.nrec = p->nrec;
        la.log_reward = p->log_reward; la.log_status = p->log_status; la.stats = stats;
        la.actor = p->weights; la.critic = p->critic;
        la.row = p->train_log + (size_t)dartmpc::kTrainLogCols * j;
        la.best_return = p->best_return; la.best_weights = p->best_weights; la.best_iter = p->best_iter;
        HIPCHK(h, launch_train_log(w, la, cfg->iterations, hs), "training log launch");
    }
    return DART_MPC_OK;
}

// The host form of the training entries.  P = 0: dart_lmpc_train_global (g == nullptr: dart_lmpc_train); P >= 1:
// dart_lmpc_train_pop_global on P * B instances, the nets and the training arrays stacked per learner, and g (when
// given) P buffers stacked g->capacity rows apart
int train_host(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
               const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo, const dart_lmpc_train_config* cfg,
               int P, const uint64_t* seeds, int B, int reset_rows, const dart_lmpc_train_buffers* p,
               const dart_lmpc_global_buffer* g, void* stream, const double* hyper = nullptr) {
    DART_ENTER(h, -1);
    if (int rc = train_check(h, rcfg, ppo, cfg, B, p, false)) return rc;
    if (hyper) {
        // every row must be a config the entries would take: the shared one with the row in place of its first nine
        if (P < 1 || P > DART_LMPC_POP_MAX) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
        for (int l = 0; l < P; ++l) {
            dart_lmpc_ppo_config c = *ppo;
            std::memcpy(&c, hyper + (size_t)l * dartmpc::kHyperCols, sizeof(double) * dartmpc::kHyperCols);
            if (!ppo_cfg_ok(&c)) return fail(h, DART_MPC_EINVAL, "bad row of the hyper-parameter table");
        }
    }
    if (g)
        if (int rc = global_check(h, g, cfg->steps / rcfg->record_every * B, false)) return rc;
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, "handle is not an LMPC handle");
    if (P > 0)
        if (int rc = pop_check(h, rcfg, cfg, P, seeds, B)) return rc;
    const int learner_B = B, nl = P > 0 ? P : 1;
    B *= nl;                                       // every instance from here on
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if (reset_rows < 0) return fail(h, DART_MPC_EINVAL, "negative reset_rows");
    if (lmpc_null(*p, kLoop) || lmpc_null(*p, kPolicy) || lmpc_null(*p, kCollect) || lmpc_null(*p, kCollect, kRec))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (reset_rows > 0 && lmpc_null(*p, kCollect, kPool))
        return fail(h, DART_MPC_EINVAL, "reset_rows > 0 with a null reset pool");
    // instances that do not share timestep are the only way to nrec[b] != R
    for (int b = 1; b < B; ++b)
        if (p->timestep[b] != p->timestep[0]) return fail(h, DART_MPC_EINVAL, "instances differ in timestep");
    if (cfg->iterations == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream_of(h, stream);
    const size_t nB = (size_t)B, D = sizeof(double), F = sizeof(float);
    const size_t K = (size_t)cfg->steps, R = K / (size_t)rcfg->record_every;
    // every array of the closed loop and of the update whole: state both ways, logs and records down
    LmpcStagePlan m{};
    m.policy = m.collect = m.train = true;
    m.B = nB; m.nw = (size_t)dart_lmpc_nw(h->cfg.N); m.log_rows = m.r1 = K; m.rec_rows = m.q1 = R;
    m.reset_rows = (size_t)reset_rows; m.learners = (size_t)P;
    RollStage S;
    int idx[kLmpcArrays];
    lmpc_stage(S, *p, m, idx);
    const size_t log_rows = (size_t)cfg->iterations * (size_t)nl;
    const int i_log = S.add_log(p->train_log, log_rows, dartmpc::kTrainLogCols * D, 0, log_rows, false);
    // the workspace: a block of the arena that does not travel
    const size_t ws_bytes =
        dartmpc::train_workspace(nl, learner_B, (int)K, rcfg->record_every, ppo->epochs, ppo->mini_batch_size).bytes;
    const int i_ws = S.add_log(nullptr, 1, ws_bytes, 0, 0, false);
    const int i_hyper = hyper ? S.add(hyper, sizeof(double) * dartmpc::kHyperCols * (size_t)P, false) : -1;
    // the global buffer: blocks of the arena whose held rows travel by hand (those held at the start go up, those
    // held at the end come down), its log, and its workspace
    dart_lmpc_global_buffer gd;
    int gi[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    size_t g_rowbytes[6] = {kHist * F, kAct * F, F, F, D, F};
    const size_t g_bufs = (size_t)nl;                // buffers, g->capacity rows apart
    const int g_n = (int)R * learner_B;
    if (g) {
        gd = *g;
        const size_t cap = (size_t)g->capacity;
        if (g_bufs * cap > 0x7fffffffULL) return fail(h, DART_MPC_EINVAL, "too many buffer rows");
        for (int q = 0; q < 6; ++q) gi[q] = S.add_log(nullptr, 1, g_bufs * cap * g_rowbytes[q], 0, 0, false);
        gi[6] = S.add_log(g->global_log, log_rows, dartmpc::kGlobalLogCols * D, 0, log_rows, false);
        gi[7] = S.add_log(nullptr, 1,
                          dartmpc::global_workspace(nl, g_n, global_stride(P, g_n, g), ppo->epochs, ppo->mini_batch_size).bytes,
                          0, 0, false);
    }
    if (int rc = S.reserve(h)) return rc;
    dart_lmpc_train_buffers d{};
    lmpc_bind(S, h, idx, d);
    d.train_log = S.dev<double>(h, i_log);
    d.workspace = S.dev<char>(h, i_ws);
    if (int rc = S.upload(h, s)) return rc;
    void* g_host[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (g) {
        void* hp[6] = {g->obs, g->action, g->logp, g->value, g->reward, g->done};
        for (int q = 0; q < 6; ++q) g_host[q] = hp[q];
        gd.obs = S.dev<float>(h, gi[0]); gd.action = S.dev<float>(h, gi[1]); gd.logp = S.dev<float>(h, gi[2]);
        gd.value = S.dev<float>(h, gi[3]); gd.reward = S.dev<double>(h, gi[4]); gd.done = S.dev<float>(h, gi[5]);
        gd.global_log = S.dev<double>(h, gi[6]); gd.workspace = S.dev<char>(h, gi[7]);
        for (size_t l = 0; l < g_bufs; ++l)
            for (int q = 0; q < 6 && g->fill > 0; ++q) {
                const size_t off = l * (size_t)g->capacity * g_rowbytes[q];
                HIPCHK(h, hipMemcpyAsync(S.dev<char>(h, gi[q]) + off, (const char*)g_host[q] + off,
                                         (size_t)g->fill * g_rowbytes[q], hipMemcpyHostToDevice, s),
                       "copy global buffer");
            }
    }
    if (int rc = train_dev(h, plant, pcfg, rcfg, ppo, cfg, P, seeds, learner_B, reset_rows, &d, g ? &gd : nullptr, s,
                           S.dev<double>(h, i_hyper))) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    if (int rc = S.download(h, s)) return rc;
    if (g) {
        const int held = dart_lmpc_global_fill_after(g_n, g->fill, cfg->iterations);
        for (size_t l = 0; l < g_bufs; ++l)
            for (int q = 0; q < 6 && held > 0; ++q) {
                const size_t off = l * (size_t)g->capacity * g_rowbytes[q];
                HIPCHK(h, hipMemcpyAsync((char*)g_host[q] + off, S.dev<char>(h, gi[q]) + off,
                                         (size_t)held * g_rowbytes[q], hipMemcpyDeviceToHost, s),
                       "copy global buffer back");
            }
    }
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

}  // namespace

// ---- a population of P learners in the launches of one (lmpc_train.h, lmpc_ppo.h) --------------------------------

static_assert(DART_LMPC_POP_MAX == dartmpc::kPopMax && DART_LMPC_POP_CRITIC_STRIDE == dartmpc::kPopCriticStride,
              "the header's population constants are the kernels'");

size_t dart_lmpc_train_pop_workspace_bytes(int P, int B, int K, int record_every, int epochs, int mini_batch_size) {
    if (P < 1 || P > DART_LMPC_POP_MAX) return 0;
    if (dart_lmpc_train_workspace_bytes(B, K, record_every, epochs, mini_batch_size) == 0) return 0;
    if ((long long)(K / record_every) * P * B > 0x7fffffffLL) return 0;
    return dartmpc::train_workspace(P, B, K, record_every, epochs, mini_batch_size).bytes;
}

size_t dart_lmpc_global_pop_workspace_bytes(int P, int n, int capacity, int epochs, int mini_batch_size) {
    if (P < 1 || P > DART_LMPC_POP_MAX) return 0;
    if (dart_lmpc_global_workspace_bytes(n, epochs, mini_batch_size) == 0) return 0;
    int m, G;
    dartmpc::global_rows(n, m, G);
    if (capacity < G || (long long)P * capacity > 0x7fffffffLL) return 0;
    return dartmpc::global_workspace(P, n, capacity, epochs, mini_batch_size).bytes;
}

// (g == nullptr: dart_lmpc_train_dev)
int dart_lmpc_train_global_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                               const dart_lmpc_policy_config* pcfg, const dart_lmpc_reward_config* rcfg,
                               const dart_lmpc_ppo_config* ppo, const dart_lmpc_train_config* cfg, int B,
                               int reset_rows, const dart_lmpc_train_buffers* p, const dart_lmpc_global_buffer* g,
                               void* stream) {
    return train_dev(h, plant, pcfg, rcfg, ppo, cfg, 0, nullptr, B, reset_rows, p, g, stream);
}

int dart_lmpc_train_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                        const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                        const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                        void* stream) {
    return train_dev(h, plant, pcfg, rcfg, ppo, cfg, 0, nullptr, B, reset_rows, p, nullptr, stream);
}

// (g == nullptr: dart_lmpc_train_pop_dev)
int dart_lmpc_train_pop_global_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                                   const dart_lmpc_policy_config* pcfg, const dart_lmpc_reward_config* rcfg,
                                   const dart_lmpc_ppo_config* ppo, const dart_lmpc_train_config* cfg, int P,
                                   const uint64_t* seeds, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                                   const dart_lmpc_global_buffer* g, void* stream) {
    DART_ENTER(h, -1);
    if (P < 1) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
    return train_dev(h, plant, pcfg, rcfg, ppo, cfg, P, seeds, B, reset_rows, p, g, stream);
}

int dart_lmpc_train_pop_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                            const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                            const dart_lmpc_train_config* cfg, int P, const uint64_t* seeds, int B, int reset_rows,
                            const dart_lmpc_train_buffers* p, void* stream) {
    return dart_lmpc_train_pop_global_dev(h, plant, pcfg, rcfg, ppo, cfg, P, seeds, B, reset_rows, p, nullptr, stream);
}

// the population with a table of per-learner hyper-parameters (hyper == nullptr: dart_lmpc_train_pop_global_dev)
int dart_lmpc_train_pop_hyper_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                                  const dart_lmpc_policy_config* pcfg, const dart_lmpc_reward_config* rcfg,
                                  const dart_lmpc_ppo_config* ppo, const dart_lmpc_train_config* cfg, int P,
                                  const uint64_t* seeds, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                                  const dart_lmpc_global_buffer* g, const double* hyper, void* stream) {
    DART_ENTER(h, -1);
    if (P < 1) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
    return train_dev(h, plant, pcfg, rcfg, ppo, cfg, P, seeds, B, reset_rows, p, g, stream, hyper);
}

int dart_lmpc_train_pop_hyper(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                              const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                              const dart_lmpc_train_config* cfg, int P, const uint64_t* seeds, int B, int reset_rows,
                              const dart_lmpc_train_buffers* p, const dart_lmpc_global_buffer* g, const double* hyper,
                              void* stream) {
    DART_ENTER(h, -1);
    if (P < 1) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
    return train_host(h, plant, pcfg, rcfg, ppo, cfg, P, seeds, B, reset_rows, p, g, stream, hyper);
}

// (g == nullptr: dart_lmpc_train)
int dart_lmpc_train_global(dart_mpc_handle* h,const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                           const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                           const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                           const dart_lmpc_global_buffer* g, void* stream) {
    return train_host(h, plant, pcfg, rcfg, ppo, cfg, 0, nullptr, B, reset_rows, p, g, stream);
}

int dart_lmpc_train_pop(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                        const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                        const dart_lmpc_train_config* cfg, int P, const uint64_t* seeds, int B, int reset_rows,
                        const dart_lmpc_train_buffers* p, void* stream) {
    DART_ENTER(h, -1);
    if (P < 1) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
    return train_host(h, plant, pcfg, rcfg, ppo, cfg, P, seeds, B, reset_rows, p, nullptr, stream);
}

// (g == nullptr: dart_lmpc_train_pop)
int dart_lmpc_train_pop_global(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                               const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                               const dart_lmpc_train_config* cfg, int P, const uint64_t* seeds, int B, int reset_rows,
                               const dart_lmpc_train_buffers* p, const dart_lmpc_global_buffer* g, void* stream) {
    DART_ENTER(h, -1);
    if (P < 1) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
    return train_host(h, plant, pcfg, rcfg, ppo, cfg, P, seeds, B, reset_rows, p, g, stream);
}

int dart_lmpc_train(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                    const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                    const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                    void* stream) {
    return dart_lmpc_train_global(h, plant, pcfg, rcfg, ppo, cfg, B, reset_rows, p, nullptr, stream);
}

// ---- the exploit/explore step of population-based training (lmpc_pbt.hip) ----------------------------------------

void dart_lmpc_pbt_config_default(dart_lmpc_pbt_config* c) {
    if (!c) return;
    const double inf = std::numeric_limits<double>::infinity();
    c->seed = 0; c->generation = 0; c->n_replace = 0; c->higher_is_better = 0;
    c->explore_mask = (1u << 4) | (1u << 0) | (1u << 2);            // lr | clip_eps | ent_coef
    c->factor_down = 0.8; c->factor_up = 1.25;
    // clip_eps, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, adam_eps, weight_decay
    const double lo[DART_LMPC_HYPER_COLS] = {0.01, -inf, 0.0, 0.0, 1e-6, 0.0, 0.0, 0.0, -inf};
    const double hi[DART_LMPC_HYPER_COLS] = {0.5, inf, 0.1, inf, 1e-2, 0.999999, 0.999999, inf, inf};
    for (int i = 0; i < DART_LMPC_HYPER_COLS; ++i) { c->lo[i] = lo[i]; c->hi[i] = hi[i]; }
}

namespace {

// k of the step (0: P / 4), or -1 for a config or shape the entries refuse
int pbt_check(const dart_lmpc_pbt_config* c, int P, int fitness_stride) {
    if (!c || P < 1 || P > DART_LMPC_POP_MAX || fitness_stride < 1 || c->generation < 0 || c->n_replace < 0) return -1;
    const int k = c->n_replace == 0 ? P / 4 : c->n_replace;
    if (2 * (long long)k > P) return -1;
    if (!(c->factor_down > 0.0) || !(c->factor_up > 0.0)) return -1;
    for (int i = 0; i < DART_LMPC_HYPER_COLS; ++i)
        if (!(c->lo[i] <= c->hi[i])) return -1;                     // (a NaN bound fails the comparison)
    return k;
}

hipError_t pbt_launch(const dart_lmpc_pbt_config* c, int P, int k, const double* fitness, int fitness_stride,
                      float* weights, float* critic, float* adam, int32_t* adam_step, double* hyper,
                      int32_t* rank_out, int32_t* parent_out, hipStream_t s) {
    dartmpc::PbtRankArgs r;
    r.P = P; r.k = k; r.higher_is_better = c->higher_is_better; r.fitness_stride = fitness_stride;
    r.key0 = (uint32_t)(c->seed & 0xffffffffu); r.key1 = (uint32_t)(c->seed >> 32);
    r.generation = (uint32_t)c->generation; r.explore_mask = c->explore_mask;
    r.factor_down = c->factor_down; r.factor_up = c->factor_up;
    for (int i = 0; i < DART_LMPC_HYPER_COLS; ++i) { r.lo[i] = c->lo[i]; r.hi[i] = c->hi[i]; }
    r.fitness = fitness; r.hyper = hyper; r.rank_out = rank_out; r.parent_out = parent_out;
    hipError_t e = dartmpc_launch_lmpc_pbt_rank(&r, s);
    if (e != hipSuccess || k == 0) return e;                        // (no child: nothing to copy)
    const dartmpc::PbtCopyArgs q{P, parent_out, weights, critic, adam, adam_step};
    return dartmpc_launch_lmpc_pbt_copy(&q, s);
}

}  // namespace

int dart_lmpc_pbt_step_dev(const dart_lmpc_pbt_config* cfg, int P, const double* fitness, int fitness_stride,
                           float* weights, float* critic, float* adam, int32_t* adam_step, double* hyper,
                           int32_t* rank_out, int32_t* parent_out, void* stream) {
    const int k = pbt_check(cfg, P, fitness_stride);
    if (k < 0 || any_null({fitness, weights, critic, adam, adam_step, hyper, rank_out, parent_out}))
        return DART_MPC_EINVAL;
    if (!aligned16(weights) || !aligned16(critic)) return DART_MPC_EINVAL;
    return pbt_launch(cfg, P, k, fitness, fitness_stride, weights, critic, adam, adam_step, hyper, rank_out,
                      parent_out, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_pbt_step(const dart_lmpc_pbt_config* cfg, int P, const double* fitness, int fitness_stride,
                       float* weights, float* critic, float* adam, int32_t* adam_step, double* hyper,
                       int32_t* rank_out, int32_t* parent_out) {
    const int k = pbt_check(cfg, P, fitness_stride);
    if (k < 0 || any_null({fitness, weights, critic, adam, adam_step, hyper, rank_out, parent_out}))
        return DART_MPC_EINVAL;
    DART_DEVICE_STAGE(D, S);
    const size_t nP = (size_t)P, F = sizeof(float);
    const size_t bytes = sizeof(double) * nP * (1 + DART_LMPC_HYPER_COLS) + 3 * sizeof(int32_t) * nP +
                         F * nP * (dartmpc::kPpoActorN + dartmpc::kPopCriticStride + 2 * (size_t)dartmpc::kPpoParams);
    if (S.reserve(bytes + 10 * 256, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    // only the learners' own entries of the fitness travel (the device entry is handed stride 1)
    const double* d_fit = S.in_with<double>(nP, [&](double* q) {
        for (size_t l = 0; l < nP; ++l) q[l] = fitness[l * (size_t)fitness_stride];
    });
    float* d_w = S.inout(weights, nP * dartmpc::kPpoActorN);        // (every block of the stage is 256-byte aligned)
    float* d_c = S.inout(critic, nP * dartmpc::kPopCriticStride);
    float* d_adam = S.inout(adam, nP * 2 * dartmpc::kPpoParams);
    int32_t* d_step = S.inout(adam_step, nP);
    double* d_hyper = S.inout(hyper, nP * DART_LMPC_HYPER_COLS);
    int32_t* d_rank = S.inout(rank_out, nP);
    int32_t* d_par = S.inout(parent_out, nP);
    auto launch = [&](hipStream_t s) {
        return pbt_launch(cfg, P, k, d_fit, 1, d_w, d_c, d_adam, d_step, d_hyper, d_rank, d_par, s);
    };
    if (!D->run(launch)) return DART_MPC_EHIP;
    return DART_MPC_OK;
}
