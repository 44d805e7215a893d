// stack_step.h -- launch arguments of stack_step.hip: the coupling between the PMPC closed loop (loop_step.hip) and
// the dual-arm layer (arm_dyn.hip, arm_qp.hip), so that one loop runs solve -> tilt command -> tray pose -> both arms'
// dynamics, impedance QP and plant -> the tray the arms hold -> object plant (PMPC/main_parallel_enhanced.py:290-419:
// u_cmd -> quaternion -> DACTL.control -> torques -> step) on one stream without the host.
//
// Experiment e owns arm instances 2 e (left) and 2 e + 1 (right).  Per step k:
//   command   tray_cmd[e] = (tray_pos[e] | tilt_to_quat(u0[e])), the pose arm_dyn_kernel's coordinator prologue reads
//   couple    from the two arms' EE poses of the state q_k that the step's dynamics saw: the tray they hold,
//             q_a = unit(ee_quat_a (x) conj(g_q_a)), q_R flipped into q_L's hemisphere, q_t = unit(q_L + q_R) with w >= 0,
//             p_t = 1/2 sum_a (ee_pos_a - rot(q_t, g_p_a)); its Euler xyz angles (roll, pitch, yaw) by the inverse of
//             tilt_to_quat, achieved tilt = [-pitch, roll]; diagnostics yaw, grasp gap | |ee_R - ee_L| - |g_R - g_L| | and
//             the disagreement angle 2 atan2(|v|, |w|) of q_L (x) conj(q_R)
//   object    post(k) / pre(k + 1) of pmpc_loop_kernel<LM> with the tilt the plant sees chosen by `couple`
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "loop_step.h"

namespace dartmpc {

constexpr int STACK_RIDE = 0, STACK_ACHIEVED = 1;
constexpr int STACK_NMETRIC = 8;

// the coupling alone (dart_tray_from_arms): E experiments, ee_pos rows at ee_stride (3 for a packed array, the
// snapshot length when they are read from the snapshot rows), ee_quat [2 E][4], grasp [2][7]
struct TrayFromArmsArgs {
    int E, ee_stride;
    const double *ee_pos, *ee_quat, *grasp;
    double* tray;       // [E][7] (pos | quat wxyz)
    double* tilt;       // [E][2]
    double* diag;       // [E][3] yaw, grasp gap, disagreement angle
};

// tray_cmd [E][7] from u0 [E][2] and tray_pos [E][3]
struct StackCommandArgs {
    int E;
    const double *u0, *tray_pos;
    double* tray_cmd;
};

// One launch = couple + post(k) and / or pre(next step) for E experiments; the members shared with PmpcLoopArgs mean
// what they mean there ("tray:" / "LM:" as in loop_step.h).  post:
//   logs (the PMPC group, logs != 0), the loop metrics (kept for both plants here; the tray plant has no rotation, its
//   slot 6 stays 0), the coupling, stack_metrics, the stack logs (stack_logs != 0), the plant step with
//     STACK_RIDE      the lagged command, exactly pmpc_loop_kernel's; the arms are measured only
//     STACK_ACHIEVED  tilt := achieved tilt, no lag (plant.a_lag / a_lag are not used); a non-finite achieved tilt is
//                     not passed on: the tilt of the last step is held
// stack_metrics [E][8], in/out (a fresh run starts from zeros): 0 max_i |tilt_achieved - u0|_i of the last step with a
// finite achieved tilt, 1 its maximum over the steps, 2 max |yaw|, 3 max grasp gap, 4 max disagreement angle,
// 5 max |p_t - tray_pos|, 6 steps whose achieved tilt was not finite (held), 7 steps.  A maximum ignores a NaN.
struct StackStepArgs {
    int E;
    int k, do_post, do_pre, log_rows;
    int logs, stack_logs, couple;
    int ee_stride;
    PlantArgs plant;            // tray
    double a_lag, Ts;           // LM
    const double* prm;          // tray: [E][6] (mu = prm[0])
    const double* target;       // [E][6]
    const double* plant_pvec;   // LM: [E][34]
    const double* pz_vz;        // LM: [E][2]
    const double* tray_pos;     // [E][3]
    const double* grasp;        // [2][7]
    const double* ee_pos;       // rows 2 e, 2 e + 1 at ee_stride
    const double* ee_quat;      // [2 E][4]
    double* x;                  // tray: [E][6], LM: [E][8], in/out
    double* tilt;               // [E][2] in/out
    double* metrics;            // [E][8] in/out
    double* stack_metrics;      // [E][8] in/out
    double* x0;                 // [E][6]
    const double* u0;           // [E][2]
    const double* f;            // [E]
    const int32_t* status;      // [E]
    const int32_t* iters;       // [E]
    double *log_X, *log_U, *log_quat, *log_loss;
    int32_t *log_status, *log_iters;
    double* log_rot;            // LM
    double* log_tilt;           // [log_rows][E][2] the achieved tilt as measured (NaN where it was not finite)
    double* log_tray;           // [log_rows][E][7] the achieved tray pose
};

}  // namespace dartmpc

extern "C" hipError_t dartmpc_launch_tray_from_arms(const dartmpc::TrayFromArmsArgs* args, hipStream_t stream);
extern "C" hipError_t dartmpc_launch_stack_command(const dartmpc::StackCommandArgs* args, hipStream_t stream);
// (lm: 0 the tray plant's instantiation, 1 the LMPC plant's)
extern "C" hipError_t dartmpc_launch_stack_step(const dartmpc::StackStepArgs* args, int lm, hipStream_t stream);
