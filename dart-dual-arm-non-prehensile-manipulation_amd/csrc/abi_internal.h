// abi_internal.h -- what the units of the C ABI layer share: the handle, the staging of the host-pointer entries,
// error reporting, and the one internal view of the LMPC closed loop's arrays.
//   dart_mpc_abi.hip      handles, the solve entries of the three controllers, the policy entries, arm QP, RLS
//   dart_mpc_rollout.hip  loop-step and rollout entries, LMPC experience step and collection
//   dart_mpc_train.hip    GAE, PPO, generator entries, the global buffer and the training entries
//   dart_mpc_arm.hip      arm dynamics, dynamics + QP, the dual-arm coordinator and the arm layer's closed loop
//   dart_mpc_stack.hip    the PMPC closed loop through the dual-arm layer (stack_step.hip between the two)
// Nothing here is part of the library's surface (include/dart_mpc.h): everything below has hidden visibility.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "dart_mpc.h"
#include "launch_plan.h"
#include "pmpc_ipm.h"
#include "pmpc_model.h"
#include "wave.h"
#include "rmpc_ipm.h"
#include "lmpc_ipm.h"
#include "lmpc_policy.h"
#include "lmpc_experience.h"
#include "lmpc_ppo.h"
#include "lmpc_train.h"
#include "lmpc_pbt.h"
#include "arm_qp.h"
#include "loop_step.h"

#pragma GCC visibility push(hidden)

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// Staging of the host-pointer entries.  The inputs (and the in/out arrays) are packed into pinned
// host memory and reach HBM with ONE DMA copy; the kernel writes its outputs straight into mapped,
// coherent pinned host memory (a few bytes per instance, no copy back); in/out arrays return with
// one more DMA copy.  Against one pageable hipMemcpy per array this removes 5-10 copies per call.
// Capacities grow on demand; a stage is not thread-safe (one per handle, one per device for the
// stateless entries behind a mutex).
struct HostStage {
    char* hin = nullptr;            // pinned: packed inputs | in/out arrays
    char* din = nullptr;            // device mirror of hin
    char* hout = nullptr;           // pinned, mapped, coherent: kernel outputs
    char* dout = nullptr;           // device address of hout
    char* hzc = nullptr;            // pinned, mapped, coherent: zero-copy inputs (read by the kernel over PCIe)
    char* dzc = nullptr;            // device address of hzc
    size_t in_cap = 0, out_cap = 0, zc_cap = 0, in_off = 0, out_off = 0, zc_off = 0, io_first = 0;
    struct Back { void* dst; size_t off, bytes; };
    Back back[8];
    int nback = 0;

    // mapped, coherent pinned memory of at least `bytes` (zero-copy) and its device address
    static hipError_t grow_mapped(char*& host, char*& dev, size_t& cap, size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (host) (void)hipHostFree(host);
        host = dev = nullptr; cap = 0;
        hipError_t e = hipHostMalloc((void**)&host, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&dev, host, 0);
        if (e == hipSuccess) cap = bytes;
        else if (host) { (void)hipHostFree(host); host = dev = nullptr; }
        return e;
    }
    hipError_t reserve(size_t in_bytes, size_t out_bytes, size_t zc_bytes = 0) {
        hipError_t e = grow_mapped(hzc, dzc, zc_cap, zc_bytes);
        if (e == hipSuccess && in_bytes > in_cap) {
            release_in();
            e = hipHostMalloc((void**)&hin, in_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc((void**)&din, in_bytes);
            if (e != hipSuccess) { release_in(); return e; }
            in_cap = in_bytes;
        }
        return e == hipSuccess ? grow_mapped(hout, dout, out_cap, out_bytes) : e;
    }
    void release_in() {
        if (hin) (void)hipHostFree(hin);
        if (din) (void)hipFree(din);
        hin = din = nullptr; in_cap = 0;
    }
    void begin() { in_off = out_off = zc_off = 0; nback = 0; io_first = 0; }
    // device-visible pointer of an input the kernel reads straight from mapped host memory: no DMA
    // copy on the call path (for kernels that read their inputs once, at the start)
    template <class T> const T* in_zc(const T* src, size_t n) {
        if (!src) return nullptr;
        const size_t off = zc_off;
        std::memcpy(hzc + off, src, n * sizeof(T));
        zc_off += align256(n * sizeof(T));
        return reinterpret_cast<const T*>(dzc + off);
    }
    // device pointer of an input copied from src (n elements); nullptr stays nullptr
    template <class T> const T* in(const T* src, size_t n) {
        if (!src) return nullptr;
        const size_t off = in_off;
        std::memcpy(hin + off, src, n * sizeof(T));
        in_off += align256(n * sizeof(T));
        return reinterpret_cast<const T*>(din + off);
    }
    // device pointer of an input of n elements that `fill(T*)` writes in place ...
    template <class T, class Fill> const T* in_with(size_t n, Fill fill) {
        const size_t off = in_off;
        fill(reinterpret_cast<T*>(hin + off));
        in_off += align256(n * sizeof(T));
        return reinterpret_cast<const T*>(din + off);
    }
    // ... and of one gathered on the way up: row i is row index(i) of src, `width` elements each
    template <class T, class Index> const T* in_rows(const T* src, size_t rows, size_t width, Index index) {
        return in_with<T>(rows * width, [&](T* dst) {
            for (size_t i = 0; i < rows; ++i) std::memcpy(dst + i * width, src + (size_t)index(i) * width, sizeof(T) * width);
        });
    }
    // device pointer of an in/out array (read and updated by the kernel); call these last
    template <class T> T* inout(T* src, size_t n) {
        if (!src) return nullptr;
        if (nback == 0) io_first = in_off;
        const size_t off = in_off;
        in(src, n);
        back[nback++] = Back{src, off, n * sizeof(T)};
        return reinterpret_cast<T*>(din + off);
    }
    // device-visible pointer of an output slot (n elements) in mapped host memory
    template <class T> T* out(size_t n) {
        const size_t off = out_off;
        out_off += align256(n * sizeof(T));
        return reinterpret_cast<T*>(dout + off);
    }
    template <class T> const T* host_of(const T* dev_out) const {
        return reinterpret_cast<const T*>(hout + (reinterpret_cast<const char*>(dev_out) - dout));
    }
    hipError_t upload(hipStream_t s) const {
        return in_off ? hipMemcpyAsync(din, hin, in_off, hipMemcpyHostToDevice, s) : hipSuccess;
    }
    hipError_t download_inout(hipStream_t s) const {
        return nback ? hipMemcpyAsync(hin + io_first, din + io_first, in_off - io_first, hipMemcpyDeviceToHost, s)
                     : hipSuccess;
    }
    // after the stream synchronised: in/out arrays back to the caller, then outputs
    void finish_inout() const {
        for (int i = 0; i < nback; ++i) std::memcpy(back[i].dst, hin + back[i].off, back[i].bytes);
    }
    template <class T> void take(T* dst, const T* dev_out, size_t n) const {
        if (dst && dev_out) std::memcpy(dst, host_of(dev_out), n * sizeof(T));
    }
    void release() {
        release_in();
        if (hout) (void)hipHostFree(hout);
        if (hzc) (void)hipHostFree(hzc);
        hout = dout = hzc = dzc = nullptr; out_cap = zc_cap = 0;
    }
};

// stage + stream of the stateless host entries (arm QP, policy step, RLS, GAE, PPO, ...), one per device
struct DeviceStage {
    std::mutex mu;
    HostStage st;
    hipStream_t stream = nullptr;
    // what every stateless host entry does after staging its inputs: copy up, `launch(stream)`, the in/out arrays
    // back, wait; then the in/out arrays into the caller's memory (the outputs are taken by the caller)
    template <class Launch> bool run(Launch launch) {
        hipError_t e = st.upload(stream);
        if (e == hipSuccess) e = launch(stream);
        if (e == hipSuccess) e = st.download_inout(stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return false;
        st.finish_inout();
        return true;
    }
};

hipError_t device_stage(DeviceStage** out);
// the stage of a stateless host entry, locked for the rest of the entry: DeviceStage* D and its HostStage& S
#define DART_DEVICE_STAGE(D, S)                                      \
    DeviceStage* D = nullptr;                                        \
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;        \
    std::lock_guard<std::mutex> lock_##D(D->mu);                     \
    HostStage& S = D->st

struct dart_mpc_handle {
    dart_mpc_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    HostStage st;                  // staging of the host-pointer entries
    std::string err;
    uint32_t seq = 0;              // completion-word sequence of the host-pointer PMPC entry (wraps, skips 0)
    uint32_t* hdone = nullptr;     // PMPC: B_max completion words, mapped host memory (only ever
    uint32_t* ddone = nullptr;     //   hold 0 or sequence numbers of earlier calls) and their device address
    // the host PMPC entry returns once every completion word is visible, possibly before the stream
    // has retired the kernel's last instructions: the next entry on the handle settles that stream
    // first, so a late stream error is reported as the previous call's, not blamed on the new one
    hipStream_t pending = nullptr;
    // resident PMPC server (dart_mpc_serve_start): its own stream, a mailbox, inputs and outputs at
    // fixed mapped addresses for B_serve slots
    struct Server {
        bool wanted = false;               // serve_start called, serve_stop not yet
        bool running = false;
        int B = 0;
        hipStream_t stream = nullptr;
        uint32_t* mbox = nullptr;          // mapped: the 64-bit request word (pmpc_ipm.h PmpcServe)
        uint32_t* dmbox = nullptr;
        unsigned long long idle_ticks = 0;
        double idle_s = 0.0;
        std::chrono::steady_clock::time_point t_post;     // last request posted (or the grid launched)
    } srv;
    // PMPC in-place I/O area (dart_mpc_bind; the resident server's inputs and outputs): mapped,
    // coherent pinned memory for B_max instances at fixed addresses
    struct Io {
        char* hin = nullptr;  char* din = nullptr;      // x0 | ref | prm | w_warm
        char* hout = nullptr; char* dout = nullptr;     // u0 | f | w_out | status | iters
        size_t off_ref = 0, off_prm = 0, off_ww = 0, off_f = 0, off_wo = 0, off_st = 0, off_it = 0;
    } io;
    // Serialises the entries on this handle: the host-pointer entries share the pinned staging
    // buffers and the handle's stream, and every entry may write err.  Concurrent callers (the
    // reference runs controllers on background threads, RMPC/dev_dual/controller/convimp.py:435)
    // are safe but take turns; one handle per thread runs them side by side.
    std::recursive_mutex mu;     // recursive: the host entries call their _dev twins
    // LMPC: hand-off areas of the instances that enter IPOPT's restoration phases (lmpc_ipm.hip,
    // [B][64][16] doubles), one per launch stream -- launches in flight on different streams never share
    // one -- grown on demand by stream-ordered allocation (the old area is freed behind its last use on
    // that stream: no device-wide synchronisation, nothing else waits)
    struct RestoArea {
        hipStream_t s;
        double* buf;
        size_t cap;
        int xcd;                   // XCD of the stream's small batches (round robin over the streams)
    };
    std::vector<RestoArea> resto;
    unsigned xcd_next = 0;
    // closed-loop rollouts (dart_*_rollout*): the solve's per-step arrays for B_max instances, allocated on first
    // use, and the device arena of the host entries (state and logs), grown on demand
    char* loop_buf = nullptr;
    char* roll_buf = nullptr;
    size_t roll_cap = 0;
    // experience collection (dart_lmpc_collect*): the policy's raw actions of one step, [B_max][34] fp32,
    // allocated on first use
    float* action_buf = nullptr;
};

inline int fail(dart_mpc_handle* h, int code, const char* what, hipError_t e = hipSuccess) {
    if (h) {
        char buf[256];
        if (e != hipSuccess) std::snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        else std::snprintf(buf, sizeof buf, "%s", what);
        h->err = buf;
    }
    return code;
}

#define HIPCHK(h, call, what)                                          \
    do {                                                               \
        hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) return fail((h), DART_MPC_EHIP, (what), e_); \
    } while (0)

inline bool any_null(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (!p) return true;
    return false;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the stream of an entry's launches: the caller's, or the handle's own
inline hipStream_t stream_of(const dart_mpc_handle* h, void* stream) { return stream ? (hipStream_t)stream : h->stream; }

// what nearly every entry on a handle starts with: the handle's lock (held by the caller's guard) and its variant
inline const char* variant_text(int variant) {
    return variant == DART_MPC_RMPC   ? "handle is not an RMPC handle"
           : variant == DART_MPC_LMPC ? "handle is not an LMPC handle"
                                      : "handle is not a PMPC handle";
}
#define DART_ENTER(h, variant_)                                                                         \
    if (!(h)) return DART_MPC_EINVAL;                                                                   \
    std::unique_lock<std::recursive_mutex> lock_((h)->mu);                                              \
    if ((variant_) >= 0 && (h)->cfg.variant != (variant_)) return fail((h), DART_MPC_EINVAL, variant_text(variant_))

// widths of the LMPC arrays, per instance: the state, the control, the policy's base observation (52), its action =
// the model's parameter vector (34), its observation history = the nets' input (520), their hidden layer (64); the
// solve's parameters are dartmpc::LM_NPRM wide and the weights DART_LMPC_POLICY_NWEIGHTS / _CRITIC_NWEIGHTS
constexpr int kNx = 8, kNu = 2, kObs = dartmpc::PB, kAct = dartmpc::PA, kHist = dartmpc::kPpoObs, kHid = dartmpc::PH;
static_assert(kAct == dartmpc::LM_NPV && kHid == dartmpc::kPpoHid, "one policy, one parameter vector");

// the packed weights of the two nets (W1 | b1 | W2 | b2 | W3 | b3 [| log_std])
inline dartmpc::PolicyWeights policy_weights(const float* w) {
    dartmpc::PolicyWeights p;
    p.W1 = w; p.b1 = w + kHist * kHid; p.W2 = p.b1 + kHid; p.b2 = p.W2 + kHid * kHid;
    p.W3 = p.b2 + kHid; p.b3 = p.W3 + kHid * kAct; p.log_std = p.b3 + kAct;
    return p;
}
inline dartmpc::CriticWeights critic_weights(const float* c) {
    dartmpc::CriticWeights p;
    p.V1 = c; p.c1 = c + kHist * kHid; p.V2 = p.c1 + kHid; p.c2 = p.V2 + kHid * kHid;
    p.V3 = p.c2 + kHid; p.c3 = p.V3 + kHid;
    return p;
}

// dart_mpc_abi.hip
int policy_args(const dart_lmpc_policy_config* c, int B, const float* w, dartmpc::PolicyArgs& a);
int settle_pending(dart_mpc_handle* h);
// dart_lmpc_policy_solve_batch_dev with the learner block size of a population: instance b steps with the weights of
// learner b / learner_B, `weights` being [learners][39748]; 0: one policy for all (the public entry)
int lmpc_policy_solve_dev(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, int B, int learner_B,
                          const float* weights, const double* state, const double* u_prev, const double* target,
                          const double* current_k, double* obs_mean, double* obs_M2, int32_t* obs_count, float* history,
                          int32_t* timestep, const float* noise, double* model_params, float* action_out,
                          const double* prm, const double* w_warm, double* u0, double* f, double* w_out,
                          int32_t* status, int32_t* iters, void* stream);

// Device arena of the host rollout / collection / training entries: arrays laid out 256-byte aligned in the handle's
// roll_buf, copied up / down in part
struct RollArr {
    void* host;
    size_t lo, n;         // the byte range that travels
    bool up, down;
    size_t off;
};

struct RollStage {
    std::vector<RollArr> arr;
    size_t total = 0;
    // rows [r0, r1) of `rowbytes` each travel, up and / or down (a null host: a block that does not travel)
    int add_rows(const void* host, size_t rows, size_t rowbytes, size_t r0, size_t r1, bool up, bool down) {
        arr.push_back({const_cast<void*>(host), r0 * rowbytes, (r1 - r0) * rowbytes, up, down, total});
        total += align256(rows * rowbytes);
        return (int)arr.size() - 1;
    }
    // whole array, both ways (state) or up only (inputs)
    int add(const void* host, size_t bytes, bool down) { return add_rows(host, 1, bytes, 0, 1, true, down); }
    // a log: rows [r0, r1) come down (and go up where the call may leave entries of them untouched)
    int add_log(void* host, size_t rows, size_t rowbytes, size_t r0, size_t r1, bool up) {
        return add_rows(host, rows, rowbytes, r0, r1, up, true);
    }
    template <class T> T* dev(const dart_mpc_handle* h, int i) const {
        return i < 0 ? nullptr : reinterpret_cast<T*>(h->roll_buf + arr[i].off);
    }
    int reserve(dart_mpc_handle* h) {
        if (total <= h->roll_cap) return DART_MPC_OK;
        if (h->roll_buf) HIPCHK(h, hipFree(h->roll_buf), "hipFree (rollout arena)");
        h->roll_buf = nullptr; h->roll_cap = 0;
        HIPCHK(h, hipMalloc((void**)&h->roll_buf, total), "hipMalloc (rollout arena)");
        h->roll_cap = total;
        return DART_MPC_OK;
    }
    int upload(dart_mpc_handle* h, hipStream_t s) const {
        for (const auto& a : arr)
            if (a.up && a.n)
                HIPCHK(h, hipMemcpyAsync(h->roll_buf + a.off + a.lo, (const char*)a.host + a.lo, a.n, hipMemcpyHostToDevice, s),
                       "copy rollout state");
        return DART_MPC_OK;
    }
    int download(dart_mpc_handle* h, hipStream_t s) const {
        for (const auto& a : arr)
            if (a.down && a.n)
                HIPCHK(h, hipMemcpyAsync((char*)a.host + a.lo, h->roll_buf + a.off + a.lo, a.n, hipMemcpyDeviceToHost, s),
                       "copy rollout logs");
        return DART_MPC_OK;
    }
};

// ---- the LMPC closed loop's arrays (dart_mpc_rollout.hip) -----------------------------------------------------
// dart_lmpc_train_buffers names every array that the rollout, collection and training entries pass around; the
// entries build one from their positional arguments and the internal code takes that (the noise, which the
// struct lacks, goes beside it).  One table, kLmpcArr, describes each member once.
enum LmpcGroup : uint8_t { kLoop, kPolicy, kCollect, kTrain };        // the entries that take the array
enum LmpcKind : uint8_t {
    kUp,             // [B][width], up only
    kBoth,           // [B][width], both ways
    kBothCollect,    // up only in a plain rollout, both ways once resets rewrite it
    kBothTrain,      // up only unless training updates it
    kNet,            // [width] per call (weights), up only unless training updates it; never in a null list
    kCall,           // [width] per call, both ways
    kLog,            // [log_rows][B][width], the call's step rows come down
    kRec,            // [rec_rows][B][width]
    kPool,           // [reset_rows][B][width], up only, with reset_rows > 0
    kAnyState = 255  // (lmpc_null: every kind but kNet, kRec and kPool)
};
struct LmpcArr {
    size_t member;                // offsetof(dart_lmpc_train_buffers, ...)
    int width;                    // elements per instance (per call: kNet, kCall); -1: the solver's nw
    uint8_t size, kind, group;    // element size
};
constexpr int kLmpcArrays = 51;               // rows of the table (dart_mpc_rollout.hip kLmpcArr)

// what a host entry stages: which groups, which rows
struct LmpcStagePlan {
    bool policy, collect, train;
    size_t B, nw, log_rows, r0, r1;               // the step logs' rows and those that travel
    size_t rec_rows, q0, q1;                      // the records' (collect: both ways; train: down only)
    size_t reset_rows;
    size_t learners;                              // a population's host entry: B = learners * B each, the nets and the
                                                  // training arrays stacked per learner; 0: one learner
    bool no_logs;                                 // an evaluation in metrics-only mode: the loop's logs are not laid out
};

// true if a pointer of `group` (kind kAnyState: its state and log arrays; kRec / kPool: those) is null
bool lmpc_null(const dart_lmpc_train_buffers& p, int group, int kind = kAnyState);
// adds the arrays of `host` that the plan names to the arena's layout (idx[i]: block of kLmpcArr[i], -1 if absent) ...
void lmpc_stage(RollStage& S, const dart_lmpc_train_buffers& host, const LmpcStagePlan& plan, int idx[kLmpcArrays]);
// ... and, the arena reserved, their device addresses into `dev` (absent arrays: null)
void lmpc_bind(const RollStage& S, const dart_mpc_handle* h, const int idx[kLmpcArrays], dart_lmpc_train_buffers& dev);

// The closed loop of dart_lmpc_rollout_dev (collect false: no experience launches, weights may be null, rcfg unused)
// and of dart_lmpc_collect_dev on device pointers, the handle's lock held: every check, then the launches.
// learner_B > 0 (a population's collection): instance b acts and is valued with the nets of learner b / learner_B
// (weights [learners][39748], critic [learners][kPopCriticStride]); 0: one policy for all.
// ev != nullptr (dart_lmpc_eval*, never with collect): the loop step is lmpc_eval_loop_kernel's, which keeps
// ev->metrics [B][8]; the seven logs of `p` are all null (metrics-only) or all set; one score launch over the P
// learners (B = P * B each) follows the last post when ev->scores is set
struct LmpcEval {
    double* metrics;
    double* scores;
    int P;
};
int lmpc_closed_loop(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                     const dart_lmpc_reward_config* rcfg, bool collect, int B, int k0, int steps, int log_rows,
                     int rec_rows, int reset_rows, const dart_lmpc_train_buffers& p, const float* noise, void* stream,
                     int learner_B = 0, const LmpcEval* ev = nullptr);

// ---- what the stack entries (dart_mpc_stack.hip) take from the PMPC loop and from the arm layer -----------------
// the solve's per-step arrays of a PMPC / RMPC loop step: pre writes x0 (RMPC: and Rref, phi, y), post reads the rest
struct LoopIo {
    double *x0, *Rref, *phi, *y, *u0, *f;
    int32_t *status, *iters;
};
// dart_mpc_rollout.hip: the plant of a loop step; a rollout's own LoopIo in the handle's scratch (B_max instances)
dartmpc::PlantArgs plant_args(const dart_mpc_handle* h, const dart_plant_config* p);
int loop_scratch(dart_mpc_handle* h, LoopIo& L);
// dart_mpc_arm.hip: the configuration checks of the arm entries, and one step of the arm layer's loop on device
// pointers (the checks made): dynamics against the tray poses `tray` [E][7], the QP, the plant step.  `work` is
// dart_dual_arm_work_len(E, n) doubles and starts with the step's snapshot rows; ee_quat [2 E][4] or null; the logs
// [rows][2 E][.] all given or all null, row `log_row` is written.
bool arm_dyn_ok(const dart_arm_dyn_config* c, int B, int n);
bool arm_qp_ok(const dart_arm_config* c, int n, int prm_stride);
int dual_arm_step(const dart_arm_dyn_config* dcfg, const dart_arm_config* cfg, int E, int n, const double* tray,
                  const double* grasp, const double* models, const double* plant_models, const double* prm,
                  int prm_stride, double* q, double* qd, double* qdd_prev, double* metrics, double* work,
                  double* ee_quat, size_t log_row, double* q_log, double* qd_log, double* tau_log, double* ee_log,
                  double* loss_log, int32_t* status_log, hipStream_t s);

#pragma GCC visibility pop
