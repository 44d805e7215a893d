// rmpc_stack_step.h -- launch arguments of rmpc_stack_step.hip: the RMPC closed loop through the dual-arm layer
// (RMPC/dev_dual/rob_ctrl.py:331-416: RLS update, reference governor, solve, Rot.from_euler('xyz', [u1, -u0, 0]),
// DACTL.control, step, torques logged).  Per step the unchanged RMPC solve with its fused RLS, stack_command_kernel
// (stack_step.hip), the arm layer's step, and rmpc_stack_step_kernel<LM>: the coupling of stack_step.h, then post(k) /
// pre(k + 1) of rmpc_loop_kernel<LM> with the tilt the plant sees chosen by `couple`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "loop_step.h"
#include "stack_step.h"

namespace dartmpc {

// One launch = couple + post(k) and / or pre(next step) for E experiments; experiment e owns arm instances 2 e and
// 2 e + 1.  The members shared with RmpcLoopArgs and StackStepArgs mean what they mean there ("tray:" / "LM:" as in
// loop_step.h).  post: rmpc_loop_kernel's (the RMPC log group where logs != 0; nlog and done advance without it), the
// loop metrics on both plants (the tray plant's slot 6 stays 0), the coupling, stack_metrics, the stack log group
// (stack_logs != 0), the plant step with
//   STACK_RIDE      the lagged command u0, exactly rmpc_loop_kernel's; the arms are measured only
//   STACK_ACHIEVED  tilt := achieved tilt, the plant driven with it; a non-finite achieved tilt is not passed on: the
//                   tilt of the last step is held and the step counted
// u_prev := u0 in both modes (rob_ctrl.py:416: the controller's own last command).  pre: rmpc_loop_kernel's.
struct RmpcStackStepArgs {
    int E, N;
    int k, do_post, do_pre, log_rows;
    int logs, stack_logs, couple;
    int ee_stride;
    PlantArgs plant;            // tray
    double a_lag;               // LM
    double Ts, dr_max, alpha_rg, step_fraction, pos_tol;
    const double* target;       // [E][4]
    const double* prm;          // [E][10]
    const double* mu;           // tray: [E]
    const double* plant_pvec;   // LM: [E][34]
    const double* tray_pos;     // [E][3]
    const double* grasp;        // [2][7]
    const double* ee_pos;       // rows 2 e, 2 e + 1 at ee_stride
    const double* ee_quat;      // [2 E][4]
    double* x;                  // tray: [E][6], LM: [E][8], in/out
    double* tilt;               // [E][2]
    double* prev;               // [E][4]
    double* u_prev;             // [E][2]
    double* r_v;                // [E][4]
    const double* theta;        // [E][14]
    int32_t* done;              // [E]
    int32_t* nlog;              // [E]
    double* metrics;            // [E][8] in/out
    double* stack_metrics;      // [E][8] in/out
    double *x0, *Rref, *phi, *y;        // the solve's inputs (pre)
    const double *u0, *f;               // its outputs (post)
    const int32_t *status, *iters;
    // the RMPC log group [log_rows][E][...]
    double *log_pos_err, *log_pos_err_norm, *log_u_cmd, *log_timestep;
    double *log_x, *log_theta, *log_r_v, *log_f;
    int32_t *log_status, *log_iters;
    double* log_rot;            // LM
    // the stack log group: the command, its quaternion (stack_command_kernel's bits), the achieved tilt and pose
    double *log_U, *log_quat, *log_tilt, *log_tray;
};

}  // namespace dartmpc

// (lm: 0 the tray plant's instantiation, 1 the LMPC plant's; N outside 1 .. 63: hipErrorInvalidValue)
extern "C" hipError_t dartmpc_launch_rmpc_stack_step(const dartmpc::RmpcStackStepArgs* args, int lm, hipStream_t stream);
