// lmpc_experience.h -- launch arguments of the LMPC experience kernels (lmpc_experience.hip): the training half
// of RLMPC._rl_worker (LMPC/src/controller/rlmpc2.py:537-938) up to the PPO update -- critic, log-probability,
// reward, done, episode bookkeeping, rollout buffer, resets and GAE -- for a batch of controllers whose closed
// loop runs on the device (dart_lmpc_collect).
//
// Two deliberate differences from the reference:
//   * buf.add(obs, a, logp, value, reward, done) (:744) passes value and reward in swapped positions against
//     RolloutBuffer.add(o, a, logp, r, v, done) (:93), so compute_gae (:781) sees the values as rewards.  The swap
//     is not reproduced: every field is stored under its own name.
//   * the in_contact penalty (:735) has no counterpart in harness.LmpcPlant (there is no contact model) and is
//     left out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_policy.h"

namespace dartmpc {

// value_net weights, fp32, input-major like PolicyWeights.  The experience kernel reads W1 / b1 and V1 / c1 with
// 16-byte loads: both packed weight arrays are 16-byte aligned (checked by the ABI).
struct CriticWeights {
    const float* V1;        // [520][64]
    const float* c1;        // [64]
    const float* V2;        // [64][64]
    const float* c2;        // [64]
    const float* V3;        // [64]
    const float* c3;        // [1]
};

struct RewardArgs {
    double sigma_pos, sigma_vel, w_pos, w_vel, w_change, w_d_ctrl, success_tol, success_bonus, oob_penalty;
    double tray_limit[2];
    double max_per_dim_rms, time_penalty_rate;
    int max_episode_steps, record_every, done_sticky;
};

// done bits of log_done
constexpr int kDoneOob = 1;         // out of bounds (:727-730)
constexpr int kDoneMaxSteps = 2;    // max_episode_steps reached (:738-740)

// One launch = the experience of closed-loop step k for B instances, after that step's post(k) + pre(k+1).
struct ExperienceArgs {
    int B, k;
    int rec_rows, reset_rows;
    int learner_B;              // population: instance b reads the nets of learner b / learner_B (the actors kPolicyN
                                // and the critics kPopCriticStride floats apart); 0: one pair of nets for all
    PolicyWeights w;            // the actor (recomputed: mean) and log_std
    CriticWeights c;
    RewardArgs r;
    double max_delta, action_scale, log_std_min, log_std_max;      // of the policy config
    // step k's values, read
    const float* history;       // [B][520] obs_k
    const float* action;        // [B][34]  raw_k
    const double* log_X;        // [log_rows][B][8]; row k = x_k
    const int32_t* timestep;    // [B] the policy's counter after its increment
    const double* u_prev;       // [B][2] u_k (post(k) has written it): the control step k+1 will observe
    // loop state this kernel resets at an episode end, in/out
    double* target;             // [B][8]
    double* plant_pvec;         // [B][34]
    double* x;                  // [B][8]
    double* tilt;               // [B][2]
    double* state;              // [B][8] the next solve's input (pre(k+1) has written it); nullable
    // collection state, in/out
    double* prev_cmd;           // [B][2] the control step k-1 observed
    double* control_seen;       // [B][2] the control step k observed
    int32_t* ep_step;           // [B]
    double* ep_return;          // [B]
    double* time_penalty;       // [B]
    int32_t* episodes;          // [B]
    double* last_return;        // [B]
    int32_t* last_steps;        // [B]
    int32_t* nrec;              // [B]
    int32_t* sticky;            // [B] OR of the done bits since the previous record
    // reset pool [reset_rows][B][..], read at an episode end
    const double* reset_x;      // [..][8]
    const double* reset_target; // [..][8]
    const double* reset_pvec;   // [..][34]
    // per-step logs, row k
    double* log_reward;         // [log_rows][B]
    int32_t* log_done;
    float* log_value;
    float* log_logp;
    // records [rec_rows][B][..]
    float* rec_obs;             // [..][520]
    float* rec_action;          // [..][34]
    float* rec_logp;
    float* rec_value;
    double* rec_reward;
    float* rec_done;
    float* mean_out;            // [B][34] the recomputed actor mean, nullable
};

// compute_gae (:592-599) per instance over its nrec[b] records, fp64
struct GaeArgs {
    int B, rec_rows;
    double gamma, lam;
    const int32_t* nrec;        // [B]
    const double* rec_reward;   // [rec_rows][B]
    const float* rec_value;
    const float* rec_done;
    const float* last_value;    // [B]
    double* adv;                // [rec_rows][B]
    double* ret;                // [rec_rows][B]  adv + value
};

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_lmpc_experience(const dartmpc::ExperienceArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_gae(const dartmpc::GaeArgs* args, hipStream_t stream);
