// loop_step.h -- launch arguments of the closed-loop glue kernels (loop_step.hip): what the drivers do between
// two solves (RMPC/dev_dual/rob_ctrl.py:331-416, PMPC/main_parallel_enhanced.py:290-419, LMPC/src/run.py:256-286)
// and the plant, so that a K-step rollout stays on one stream without the host.  One kernel and one argument struct
// per controller; the PMPC and RMPC kernels are compiled for two plants (harness.TrayPlant, harness.LmpcPlant), and
// their structs hold the members of both: "tray:" / "LM:" marks a member that only that plant's instantiation reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dartmpc {

// harness.TrayPlant: first-order tilt lag, reference model + Coulomb friction, RK4 at dt
struct PlantArgs {
    double a_lag;       // 1 - exp(-dt / tau) (1 for tau <= 0)
    double mu_c, v_c;   // Coulomb friction coefficient and its tanh velocity scale
    double dt, g;
};

// Cross-plant loops (LM): the PMPC / RMPC closed loops on harness.LmpcPlant, with streaming metrics.  The plant state
// is LmpcPlant's x [B][8] = [px vx py vy th_x om_x th_y om_y], stepped by the LMPC model with plant_pvec.  tilt [B][2]
// is the lagged PMPC / RMPC command (a = g sin(theta), g = -9.81, mpc_3d.py:91-92); the LMPC model has
// G = m g sin(a) with g = +9.81 (rlmpc2.py:353-357), so its input is sin(-tilt) (run.py:257 flips the command for the
// same reason): the next state is bit for bit what lmpc_loop_kernel computes for (x, -tilt, -u, pvec).  mu_c / v_c
// of the plant are not used.
//
// metrics [B][8], in/out, updated by every post with e_k = |X_k[[0, 2]] - target[[0, 2]]| of the state that solve k
// saw: 0 e of the last step, 1 first k with e_k < 0.01 (-1 while there is none), 2 sum |u_k| Ts, 3 max e_k,
// 4 steps with status != 0, 5 sum of iters, 6 max of |th_x|, |th_y| over the states the solves saw, 7 steps
// accumulated.  A fresh run starts from zeros with slot 1 = -1.
//
// logs == 0 (LM only; every log pointer null): no log row is written and log_rows is not consulted.  The tray
// plant's loops always log.

// One launch = post(k) and / or pre(next step) for B instances.  All arrays are device memory.
struct RmpcLoopArgs {
    int B, N;
    int k;                      // step (log row) of the post half; timestep = k Ts
    int do_post, do_pre;
    int log_rows;
    int logs;                   // LM
    PlantArgs plant;            // tray
    double a_lag;               // LM
    double Ts, dr_max, alpha_rg, step_fraction, pos_tol;
    const double* target;       // [B][4]
    const double* prm;          // [B][10] (v_eps = prm[9] scales the RLS features)
    const double* mu;           // tray: [B] viscous friction of the plant
    const double* plant_pvec;   // LM: [B][34] the plant's parameter vector
    // loop state, in/out
    double* x;                  // tray: [B][6], LM: [B][8]
    double* tilt;               // [B][2]
    double* prev;               // [B][4]
    double* u_prev;             // [B][2]
    double* r_v;                // [B][4]
    const double* theta;        // [B][14] (updated by the solve's fused RLS; logged here)
    int32_t* done;              // [B]
    int32_t* nlog;              // [B] episode rows written so far (advances in metrics-only mode too)
    double* metrics;            // LM: [B][8]
    // the solve's per-step inputs (written by pre) and outputs (read by post)
    double* x0;                 // [B][4]
    double* Rref;               // [B][4(N+1)]
    double* phi;                // [B][7]
    double* y;                  // [B][2]
    const double* u0;           // [B][2]
    const double* f;            // [B]
    const int32_t* status;      // [B]
    const int32_t* iters;       // [B]
    // logs [log_rows][B][...]: episode rows (index nlog[b], while !done[b]) and step rows (index k)
    double* log_pos_err;        // [..][2]
    double* log_pos_err_norm;   // [..]
    double* log_u_cmd;          // [..][2]
    double* log_timestep;       // [..]
    double* log_x;              // [..][4] = x[0..3]
    double* log_theta;          // [..][14]
    double* log_r_v;            // [..][4]
    double* log_f;              // [..]
    int32_t* log_status;        // [..]
    int32_t* log_iters;         // [..]
    double* log_rot;            // LM: [..][4] = x[4..7]
};

struct PmpcLoopArgs {
    int B;
    int k, do_post, do_pre, log_rows;
    int logs;                   // LM
    PlantArgs plant;            // tray
    double a_lag, Ts;           // LM
    const double* prm;          // tray: [B][6] (mu = prm[0] is the plant's viscous friction)
    const double* target;       // LM: [B][6] (the metrics' error)
    const double* plant_pvec;   // LM: [B][34]
    const double* pz_vz;        // LM: [B][2] the solve's x0[4..5] (no plant moves them; the tray's are x[4..5])
    double* x;                  // tray: [B][6], LM: [B][8], in/out
    double* tilt;               // [B][2] in/out
    double* metrics;            // LM: [B][8] in/out
    double* x0;                 // [B][6] the solve's input (written by pre): [x[0..3], pz, vz]
    const double* u0;           // [B][2]
    const double* f;            // [B]
    const int32_t* status;      // [B]
    const int32_t* iters;       // [B]
    double* log_X;              // [log_rows][B][6] = [x[0..3], pz, vz]
    double* log_U;              // [..][2]
    double* log_quat;           // [..][4]
    double* log_loss;           // [..]
    int32_t* log_status;        // [..]
    int32_t* log_iters;         // [..]
    double* log_rot;            // LM: [..][4] = x[4..7]
};

// harness.LmpcPlant: the same tilt lag, then one RK4 step at Ts of the LMPC model itself (safe_dynamics,
// LMPC/src/controller/rlmpc2.py:260-429) with the lagged tilt as input and the instance's true parameters
// plant_pvec.  mu_c / v_c of dart_plant_config are not used: the model's Stribeck terms are its Coulomb friction.
// The driver's u_cmd *= -1 and the quaternion (LMPC/src/run.py:257-261) are MuJoCo tray conventions and are not
// applied, as in the other two plants.
struct LmpcLoopArgs {
    int B;
    int k, do_post, do_pre, log_rows;
    double a_lag, Ts;
    const double* target;       // [B][8]
    const double* plant_pvec;   // [B][34] the plant's parameter vector (index map of rlmpc2.py:301-334)
    double* x;                  // [B][8] in/out
    double* tilt;               // [B][2] in/out
    double* u_prev;             // [B][2] out (post): the next solve's u_prev and the policy's control
    const double* model_params; // [B][34] the parameter row the solve used (logged by post)
    double* state;              // [B][8] the solve's input (written by pre)
    const double* u0;           // [B][2]
    const double* f;            // [B]
    const int32_t* status;      // [B]
    const int32_t* iters;       // [B]
    double* log_X;              // [log_rows][B][8] the state the solve saw
    double* log_U;              // [..][2]
    double* log_pos_error;      // [..] |x_next[[0, 2]] - target[[0, 2]]| after the plant step (run.py:274)
    double* log_pvec;           // [..][34]
    double* log_loss;           // [..]
    int32_t* log_status;        // [..]
    int32_t* log_iters;         // [..]
};

// LMPC evaluation (lmpc_eval_loop_kernel): the LMPC loop step above with the streaming metrics of the cross-plant
// loops, metrics [B][8] in/out (same slots, e_k of the state that solve k saw, th_x = x[4], th_y = x[6]).  logs == 0:
// the seven log pointers of `l` are null and no log row is written (metrics-only); logs == 1: they are all set and
// the rows are lmpc_loop_kernel's.  B counts all instances of a population (P learners of B each, learner-major);
// the kernel does not know about learners.
struct LmpcEvalLoopArgs {
    LmpcLoopArgs l;
    int logs;
    double* metrics;            // [B][8] in/out
};

// Scores (lmpc_eval_scores_kernel): metrics [P][B][8] -> scores [P][8], per learner over its instances b = 0 .. B-1 in
// that order, sequential fp64 sums:
//   0 mean steady-state error  (sum m[0]) / B           4 max error        max m[3]
//   1 converged fraction       #(m[1] >= 0) / B         5 status nonzero   sum m[4]
//   2 mean convergence step    sum of the m[1] >= 0 over their count; -1 when none
//   3 mean control effort      (sum m[2]) / B           6 iters per solve  (sum m[5]) / (sum m[7]); 0 when that is 0
//                                                       7 max rotation     max m[6]

}  // namespace dartmpc

// (lm: 0 the tray plant's instantiation, 1 the LMPC plant's)
extern "C" hipError_t dartmpc_launch_lmpc_loop(const dartmpc::LmpcLoopArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_rmpc_loop(const dartmpc::RmpcLoopArgs* args, int lm, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_pmpc_loop(const dartmpc::PmpcLoopArgs* args, int lm, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_lmpc_eval_loop(const dartmpc::LmpcEvalLoopArgs* args, hipStream_t stream);
// (B >= 1; P <= 0 launches nothing)
extern "C" hipError_t dartmpc_launch_lmpc_eval_scores(int P, int B, const double* metrics, double* scores,
                                                      hipStream_t stream);
