// lmpc_experience.hip -- LMPC experience collection on the device, gfx950: what RLMPC._rl_worker
// (LMPC/src/controller/rlmpc2.py:537-938) does between the policy's draw and the PPO update.
//
// lmpc_experience_kernel runs once per closed-loop step, after that step's post(k) + pre(k+1) launch, one wave64
// per instance.  history[b] still holds obs_k, the action buffer raw_k and log_X row k the state x_k the solve saw;
// post(k) has already replaced u_prev by u_k, so the control that policy step k observed is carried as collection
// state (control_seen, and prev_cmd one step behind).
//
// The actor is recomputed with exactly policy_step_wave's accumulation order (four fmaf chains for layer 1, two for
// layers 2 and 3, tanhf), so `mean` is the policy kernel's mean bit for bit; the code is duplicated on purpose:
// policy_step_wave is inlined into the fused solve launch, whose register allocation is a measured quantity.  No
// MFMA: the bit parity is worth more here.  Lane j owns hidden unit j in layers 2 and 3, as in policy_step_wave;
// layer 1 maps its four chains onto the four 16-lane groups (see there).  The critic (520 -> 64 -> 64 -> 1, tanh)
// runs beside the actor on its own accumulators; its last layer and the sums over the 34 actions are wave sums in
// wave.h's fixed tree order.  Reward, done and the episode bookkeeping are fp64 in the operation order of
// harness.lmpc_reward_step (no contraction into fma), except change_cost, which the reference computes on fp32
// tensors (:680-709).  See lmpc_experience.h for the two deliberate differences from the reference.
//
// lmpc_gae_kernel: one lane per instance, the reversed recursion of compute_gae (:592-599) in fp64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_experience.h"
#include "wave.h"

#pragma clang fp contract(off)

namespace dartmpc {

constexpr int PO = PolicyArgs::kHist * PB;      // 520

struct alignas(16) ExperienceLds {
    float obs[PO];
    float h1[PH], h2[PH];       // actor
    float g1[PH], g2[PH];       // critic
    float part[2][4][PH];       // layer 1: the four chains of either net before they are combined
};

// POP: a population's launch (dart_lmpc_train_pop_dev), instance b reads the nets of learner b / learner_B; its own
// instantiation, so that the single-policy kernel keeps its instructions
template <bool POP>
__global__ __launch_bounds__(kWave) void lmpc_experience_kernel(ExperienceArgs a) {
    __shared__ ExperienceLds L;
    const int l = threadIdx.x;
    const int b = blockIdx.x;
    if (b >= a.B) return;                    // block-uniform
    const size_t B = (size_t)a.B;
    PolicyWeights W = a.w;
    CriticWeights C = a.c;
    if constexpr (POP) {
        W = learner_weights(a.w, b, a.learner_B);
        const size_t o = (size_t)(b / a.learner_B) * kPopCriticStride;
        C.V1 += o; C.c1 += o; C.V2 += o; C.c2 += o; C.V3 += o; C.c3 += o;
    }
    const RewardArgs& R = a.r;

    // ---- everything this launch both reads and writes, read first (lane-uniform) ----------------------------
    const size_t row = (size_t)a.k * B + b;
    const double* xk = a.log_X + 8 * row;
    const double px = xk[0], vx = xk[1], py = xk[2], vy = xk[3];
    const double tx = a.target[8 * b], ty = a.target[8 * b + 2];
    const double cs0 = a.control_seen[2 * b], cs1 = a.control_seen[2 * b + 1];
    const double pc0 = a.prev_cmd[2 * b], pc1 = a.prev_cmd[2 * b + 1];
    const double un0 = a.u_prev[2 * b], un1 = a.u_prev[2 * b + 1];
    const double tpen = a.time_penalty[b];
    const double eret = a.ep_return[b];
    const int estep = a.ep_step[b] + 1;
    const int nep = a.episodes[b];
    const int nr = a.nrec[b];
    const int stk = a.sticky[b];
    const int t = a.timestep[b] - 1;         // the policy's counter before its increment

    // ---- obs_k staged once -----------------------------------------------------------------------------------
    // (every load of a stage is issued before the first use: left to itself the compiler waits for each load, or
    // each pair of rows, where it is used, and the kernel becomes a chain of 9 + 32 + 32 L2 round trips)
    const float* hist = a.history + (size_t)PO * b;
    {
        constexpr int kObsLoads = (PO + 63) / 64;
        float ob[kObsLoads];
#pragma unroll
        for (int j = 0; j < kObsLoads; ++j) ob[j] = hist[l + 64 * j < PO ? l + 64 * j : PO - 1];
#pragma unroll
        for (int j = 0; j < kObsLoads; ++j)
            if (l + 64 * j < PO) L.obs[l + 64 * j] = ob[j];
    }
    // layer 2's weights do not depend on layer 1: in flight from here
    float w2[PH], v2[PH];
#pragma unroll
    for (int i = 0; i < PH; ++i) {
        w2[i] = W.W2[i * PH + l];
        v2[i] = C.V2[i * PH + l];
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    // ---- mean_net and value_net (fp32) --------------------------------------------------------------------
    // Layer 1 is 1040 weight rows of 256 B per instance, which one wave has to pull through its own load queue.
    // The four chains of policy_step_wave's loop (chain r takes the input rows i = r mod 4 in increasing order) are
    // spread over the four 16-lane groups (measured: 1.5 us of the launch's 24): group r runs chain r for
    // all 64 hidden units, four units per lane, with one 16-byte load per lane and row -- four times the bytes per
    // load of the lane-owns-a-unit mapping and the same sums, since each chain still adds its rows in the same
    // order and the chains are combined as (s0 + s1) + (s2 + s3) below.  kDepth row pairs (actor + critic) stay in
    // flight while one is consumed; static indices throughout.
    {
        const int g = l >> 4, u4 = (l & 15) * 4;
        constexpr int kChunks = PO / 4, kDepth = 5;
        static_assert(PO % 4 == 0 && kChunks % kDepth == 0, "layer-1 pipeline shape");
        float4 sa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), qa = sa;
        if (g == 0) {       // the bias starts chain 0
            sa = *reinterpret_cast<const float4*>(W.b1 + u4);
            qa = *reinterpret_cast<const float4*>(C.c1 + u4);
        }
        float4 wq[kDepth], vq[kDepth];
        auto load = [&](int c, float4& w, float4& v) {
            w = *reinterpret_cast<const float4*>(W.W1 + (4 * c + g) * PH + u4);
            v = *reinterpret_cast<const float4*>(C.V1 + (4 * c + g) * PH + u4);
        };
        auto consume = [&](int c, const float4& w, const float4& v) {
            const float o = L.obs[4 * c + g];
            sa.x = fmaf(w.x, o, sa.x); sa.y = fmaf(w.y, o, sa.y); sa.z = fmaf(w.z, o, sa.z); sa.w = fmaf(w.w, o, sa.w);
            qa.x = fmaf(v.x, o, qa.x); qa.y = fmaf(v.y, o, qa.y); qa.z = fmaf(v.z, o, qa.z); qa.w = fmaf(v.w, o, qa.w);
        };
#pragma unroll
        for (int d = 0; d < kDepth; ++d) load(d, wq[d], vq[d]);
        for (int c0 = 0; c0 < kChunks - kDepth; c0 += kDepth) {
#pragma unroll
            for (int d = 0; d < kDepth; ++d) {
                consume(c0 + d, wq[d], vq[d]);
                load(c0 + d + kDepth, wq[d], vq[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < kDepth; ++d) consume(kChunks - kDepth + d, wq[d], vq[d]);
        *reinterpret_cast<float4*>(&L.part[0][g][u4]) = sa;
        *reinterpret_cast<float4*>(&L.part[1][g][u4]) = qa;
    }
    __syncthreads();
    L.h1[l] = tanhf((L.part[0][0][l] + L.part[0][1][l]) + (L.part[0][2][l] + L.part[0][3][l]));
    L.g1[l] = tanhf((L.part[1][0][l] + L.part[1][1][l]) + (L.part[1][2][l] + L.part[1][3][l]));
    __syncthreads();
    // layer 3's weights (lanes past the 34 actions read column 33: in bounds, unused) and the critic's last row
    const int l3 = l < PA ? l : PA - 1;
    float w3[PH];
#pragma unroll
    for (int i = 0; i < PH; ++i) w3[i] = W.W3[i * PA + l3];
    const float v3 = C.V3[l];
    __builtin_amdgcn_sched_barrier(0);
    {
        float s0 = W.b2[l], s1 = 0.0f;
        float q0 = C.c2[l], q1 = 0.0f;
#pragma unroll
        for (int i = 0; i < PH; i += 2) {
            s0 = fmaf(w2[i], L.h1[i], s0);
            s1 = fmaf(w2[i + 1], L.h1[i + 1], s1);
            q0 = fmaf(v2[i], L.g1[i], q0);
            q1 = fmaf(v2[i + 1], L.g1[i + 1], q1);
        }
        L.h2[l] = tanhf(s0 + s1);
        L.g2[l] = tanhf(q0 + q1);
    }
    __syncthreads();
    float raw = 0.0f, lp = 0.0f, dz = 0.0f;
    if (l < PA) {
        float s0 = W.b3[l], s1 = 0.0f;
#pragma unroll
        for (int i = 0; i < PH; i += 2) {
            s0 = fmaf(w3[i], L.h2[i], s0);
            s1 = fmaf(w3[i + 1], L.h2[i + 1], s1);
        }
        const float mean = s0 + s1;
        if (a.mean_out) a.mean_out[PA * b + l] = mean;
        // Normal(mean, std).log_prob(raw) (:699), std = exp(clamp(log_std))
        const float lsd = fminf(fmaxf(W.log_std[l], (float)a.log_std_min), (float)a.log_std_max);
        const float sd = expf(lsd);
        raw = a.action[PA * b + l];
        const float z = raw - mean;
        lp = -(z * z) / (2.0f * (sd * sd)) - lsd - 0.91893853320467274178f;
        dz = raw * (float)(a.max_delta * a.action_scale);          // delta_z (:680)
    }
    const float logp = wsumf(lp);
    const float value = wsumf(v3 * L.g2[l]) + C.c3[0];

    // ---- change_cost = |delta_z| with the rms damping (:683-709), fp32 ------------------------------------
    float cnorm = sqrtf(wsumf(dz * dz));
    const double rms = (double)cnorm / sqrt((double)PA);
    if (rms > R.max_per_dim_rms) {           // wave-uniform; enters the reward only
        dz = dz * (float)(R.max_per_dim_rms / (rms + 1e-12));
        cnorm = sqrtf(wsumf(dz * dz));
    }

    // ---- reward and done (:703-740), fp64, every lane ------------------------------------------------------
    const double ex = fabs(tx - px), ey = fabs(ty - py);
    const double pos_err = sqrt(ex * ex + ey * ey);
    const double vel_err = sqrt(vx * vx + vy * vy);
    const double e_p = exp(-(pos_err * pos_err) / (2.0 * (R.sigma_pos * R.sigma_pos)));
    const double e_v = exp(-(vel_err * vel_err) / (2.0 * (R.sigma_vel * R.sigma_vel)));
    const double prox = R.w_pos * e_p + R.w_vel * e_p * e_v;
    const double rate = fabs(cs0 - pc0) + fabs(cs1 - pc1);
    double reward = prox - R.w_change * (double)cnorm - R.w_d_ctrl * rate - tpen;
    if (pos_err < R.success_tol && vel_err < R.success_tol) reward += R.success_bonus;
    int done = 0;
    if (fabs(px) > R.tray_limit[0] || fabs(py) > R.tray_limit[1]) {
        reward -= R.oob_penalty;
        done |= kDoneOob;
    }
    if (estep >= R.max_episode_steps) done |= kDoneMaxSteps;
    const double eret_new = eret + reward;

    // ---- record (:742-744) ------------------------------------------------------------------------------------
    int stk_new = stk | done;
    const bool rec_step = t % R.record_every == 0;
    if (rec_step) {
        if (nr >= 0 && nr < a.rec_rows) {
            const size_t rr = (size_t)nr * B + b;
            for (int e = l; e < PO; e += 64) a.rec_obs[PO * rr + e] = L.obs[e];
            if (l < PA) a.rec_action[PA * rr + l] = raw;
            if (l == 0) {
                a.rec_logp[rr] = logp;
                a.rec_value[rr] = value;
                a.rec_reward[rr] = reward;
                a.rec_done[rr] = ((R.done_sticky ? stk_new : done) != 0) ? 1.0f : 0.0f;
                a.nrec[b] = nr + 1;
            }
        }
        stk_new = 0;
    }

    // ---- logs and collection state ---------------------------------------------------------------------------
    if (l == 0) {
        a.log_reward[row] = reward;
        a.log_done[row] = done;
        a.log_value[row] = value;
        a.log_logp[row] = logp;
        a.prev_cmd[2 * b] = cs0; a.prev_cmd[2 * b + 1] = cs1;
        a.control_seen[2 * b] = un0; a.control_seen[2 * b + 1] = un1;
        a.sticky[b] = stk_new;
        if (done) {
            a.last_return[b] = eret_new;
            a.last_steps[b] = estep;
            a.episodes[b] = nep + 1;
            a.ep_return[b] = 0.0; a.ep_step[b] = 0; a.time_penalty[b] = 0.0;
        } else {
            a.ep_return[b] = eret_new; a.ep_step[b] = estep; a.time_penalty[b] = tpen + R.time_penalty_rate;
        }
    }
    // ---- reset into the next episode: u_prev, the warm start and the policy's state carry over ----------------
    if (done && a.reset_rows > 0) {
        // (episodes - 1) % reset_rows after the increment; a negative counter still lands inside the pool
        const size_t er = (size_t)((nep % a.reset_rows + a.reset_rows) % a.reset_rows) * B + b;
        if (l < 8) {
            const double v = a.reset_x[8 * er + l];
            a.x[8 * b + l] = v;
            if (a.state) a.state[8 * b + l] = v;
            a.target[8 * b + l] = a.reset_target[8 * er + l];
        }
        if (l < 2) a.tilt[2 * b + l] = 0.0;
        if (l < PA) a.plant_pvec[PA * b + l] = a.reset_pvec[PA * er + l];
    }
}

constexpr int kGaeThreads = 256;

__global__ __launch_bounds__(kGaeThreads) void lmpc_gae_kernel(GaeArgs a) {
    const int b = blockIdx.x * kGaeThreads + threadIdx.x;
    if (b >= a.B) return;
    const size_t B = (size_t)a.B;
    int n = a.nrec[b];
    n = n < 0 ? 0 : n > a.rec_rows ? a.rec_rows : n;
    double gae = 0.0, v_next = (double)a.last_value[b];
    for (int s = n - 1; s >= 0; --s) {
        const size_t i = (size_t)s * B + b;
        const double v = (double)a.rec_value[i], nd = 1.0 - (double)a.rec_done[i];
        const double delta = a.rec_reward[i] + a.gamma * v_next * nd - v;
        gae = delta + a.gamma * a.lam * nd * gae;
        a.adv[i] = gae;
        a.ret[i] = gae + v;
        v_next = v;
    }
}

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_lmpc_experience(const dartmpc::ExperienceArgs* args, hipStream_t stream) {
    if (args->B <= 0) return hipSuccess;
    if (args->learner_B > 0)
        hipLaunchKernelGGL(dartmpc::lmpc_experience_kernel<true>, dim3(args->B), dim3(dartmpc::kWave), 0, stream, *args);
    else
        hipLaunchKernelGGL(dartmpc::lmpc_experience_kernel<false>, dim3(args->B), dim3(dartmpc::kWave), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t dartmpc_launch_lmpc_gae(const dartmpc::GaeArgs* args, hipStream_t stream) {
    if (args->B <= 0 || args->rec_rows <= 0) return hipSuccess;
    const int blocks = (args->B + dartmpc::kGaeThreads - 1) / dartmpc::kGaeThreads;
    hipLaunchKernelGGL(dartmpc::lmpc_gae_kernel, dim3(blocks), dim3(dartmpc::kGaeThreads), 0, stream, *args);
    return hipGetLastError();
}
