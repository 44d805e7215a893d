// dart_mpc_abi.hip -- the C ABI of include/dart_mpc.h (host side).
//
// Owns the device workspace for the host-pointer entry point and the
// per-handle stream; validates arguments the way PMPC.__init__/solve would
// fail (mpc_3d.py:12-138), then launches the batched kernel.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <chrono>
#include <mutex>
#include <initializer_list>
#include <vector>
#include <string>

#include "dart_mpc.h"
#include "pmpc_ipm.h"
#include "pmpc_model.h"
#include "wave.h"
#include "rmpc_ipm.h"
#include "lmpc_ipm.h"
#include "lmpc_policy.h"
#include "lmpc_experience.h"
#include "lmpc_ppo.h"
#include "lmpc_train.h"
#include "arm_qp.h"
#include "loop_step.h"

#include <cmath>

namespace {

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

    static size_t al(size_t n) { return (n + 255) & ~size_t(255); }
    hipError_t reserve(size_t in_bytes, size_t out_bytes, size_t zc_bytes = 0) {
        hipError_t e = hipSuccess;
        if (zc_bytes > zc_cap) {
            release_zc();
            e = hipHostMalloc((void**)&hzc, zc_bytes, hipHostMallocMapped | hipHostMallocCoherent);
            if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&dzc, hzc, 0);
            if (e != hipSuccess) { release_zc(); return e; }
            zc_cap = zc_bytes;
        }
        if (in_bytes > in_cap) {
            release_in();
            e = hipHostMalloc((void**)&hin, in_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc((void**)&din, in_bytes);
            if (e != hipSuccess) { release_in(); return e; }
            in_cap = in_bytes;
        }
        if (out_bytes > out_cap) {
            release_out();
            e = hipHostMalloc((void**)&hout, out_bytes, hipHostMallocMapped | hipHostMallocCoherent);
            if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&dout, hout, 0);
            if (e != hipSuccess) { release_out(); return e; }
            out_cap = out_bytes;
        }
        return e;
    }
    void release_in() {
        if (hin) (void)hipHostFree(hin);
        if (din) (void)hipFree(din);
        hin = din = nullptr; in_cap = 0;
    }
    void release_out() {
        if (hout) (void)hipHostFree(hout);
        hout = dout = nullptr; out_cap = 0;
    }
    void release_zc() {
        if (hzc) (void)hipHostFree(hzc);
        hzc = dzc = nullptr; zc_cap = 0;
    }
    void begin() { in_off = out_off = zc_off = 0; nback = 0; io_first = 0; }
    // device-visible pointer of an input the kernel reads straight from mapped host memory: no DMA
    // copy on the call path (for kernels that read their inputs once, at the start)
    template <class T> const T* in_zc(const T* src, size_t n) {
        if (!src) return nullptr;
        const size_t off = zc_off;
        std::memcpy(hzc + off, src, n * sizeof(T));
        zc_off += al(n * sizeof(T));
        return reinterpret_cast<const T*>(dzc + off);
    }
    // device pointer of an input copied from src (n elements); nullptr stays nullptr
    template <class T> const T* in(const T* src, size_t n) {
        if (!src) return nullptr;
        const size_t off = in_off;
        std::memcpy(hin + off, src, n * sizeof(T));
        in_off += al(n * sizeof(T));
        return reinterpret_cast<const T*>(din + off);
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
        out_off += al(n * sizeof(T));
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
    void release() { release_in(); release_out(); release_zc(); }
};

// stage + stream of the stateless host entries (arm QP, policy step, RLS), one per device
struct DeviceStage {
    std::mutex mu;
    HostStage st;
    hipStream_t stream = nullptr;
};

hipError_t device_stage(DeviceStage** out) {
    static DeviceStage stages[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    DeviceStage& d = stages[dev];
    std::lock_guard<std::mutex> g(d.mu);
    if (!d.stream) e = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
    *out = &d;
    return e;
}

}  // namespace

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

namespace {

int fail(dart_mpc_handle* h, int code, const char* what, hipError_t e = hipSuccess) {
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

int check_cfg(const dart_mpc_config* c) {
    if (!c) return 0;
    if (c->variant != DART_MPC_PMPC && c->variant != DART_MPC_RMPC && c->variant != DART_MPC_LMPC) return 0;
    if (c->N < 1 || c->N > 63) return 0;
    if (!(c->Ts > 0.0) || !(c->tol > 0.0) || !(c->gravity == c->gravity) || c->max_iter < 1 || c->B_max < 1) return 0;
    if (c->acceptable_iter < 0 || (c->acceptable_iter > 0 && !(c->acceptable_tol > 0.0))) return 0;
    if (c->max_soc < 0 || c->max_soc > 8) return 0;
    if (c->pmpc_path != 0 && c->pmpc_path != 1) return 0;
    if (!(c->constr_mult_init_max >= 0.0)) return 0;
    if (!(c->max_cpu_time >= 0.0) || c->max_cpu_time > 1e9) return 0;
    return 1;
}

void server_release(dart_mpc_handle* h) {
    auto& v = h->srv;
    if (v.mbox) (void)hipHostFree(v.mbox);
    if (v.stream) (void)hipStreamDestroy(v.stream);
    v = dart_mpc_handle::Server{};
}

void io_release(dart_mpc_handle* h) {
    auto& o = h->io;
    if (o.hin) (void)hipHostFree(o.hin);
    if (o.hout) (void)hipHostFree(o.hout);
    o = dart_mpc_handle::Io{};
}

// the in-place I/O area for B_max instances (allocated once)
hipError_t ensure_io(dart_mpc_handle* h) {
    auto& o = h->io;
    if (o.hin) return hipSuccess;
    const size_t nw = (size_t)dart_mpc_nw(h->cfg.N), Bm = (size_t)h->cfg.B_max;
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    o.off_ref = al(sizeof(double) * 6 * Bm); o.off_prm = 2 * o.off_ref; o.off_ww = 3 * o.off_ref;
    const size_t in_bytes = o.off_ww + al(sizeof(double) * nw * Bm);
    o.off_f = al(sizeof(double) * 2 * Bm); o.off_wo = o.off_f + al(sizeof(double) * Bm);
    o.off_st = o.off_wo + al(sizeof(double) * nw * Bm); o.off_it = o.off_st + al(sizeof(int32_t) * Bm);
    const size_t out_bytes = o.off_it + al(sizeof(int32_t) * Bm);
    const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
    hipError_t e = hipHostMalloc((void**)&o.hin, in_bytes, fl);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&o.din, o.hin, 0);
    if (e == hipSuccess) e = hipHostMalloc((void**)&o.hout, out_bytes, fl);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&o.dout, o.hout, 0);
    if (e != hipSuccess) { io_release(h); return e; }
    std::memset(o.hin, 0, in_bytes);
    std::memset(o.hout, 0, out_bytes);
    return hipSuccess;
}

// IPOPT's restoration phases for PMPC launches of this handle (pmpc_resto.h: IPOPT's path, N <= 31);
// `mode` 1 for launches whose restoration runs on the device without the host (the launcher runs it in the
// solving wave for B <= 32, else queues pmpc_resto_kernel behind the solve), 2 for launches whose handed-over
// instances the host sees in their completion words (it launches the kernel only then: host_resto)
int pmpc_resto_mode(const dart_mpc_handle* h, int mode) {
    return (h->cfg.restoration && h->cfg.pmpc_path == 0 && h->cfg.N <= 31) ? mode : 0;
}

// IPOPT's soft restoration phase in the register kernel: with the restoration phases on, on IPOPT's path, at every N
int pmpc_soft(const dart_mpc_handle* h) { return (h->cfg.restoration && h->cfg.pmpc_path == 0) ? 1 : 0; }

// the mode of a host-entry launch of B instances: in the solving wave (small batches), else host-driven
int host_resto_mode(const dart_mpc_handle* h, int B) { return pmpc_resto_mode(h, B <= 32 ? 1 : 2); }

// After the completion words of a host-driven (mode 2) launch: pmpc_resto_kernel for the handed-over
// instances (status kPmNeedResto, read from mapped host memory), only if there is one -- no restoration
// dispatch follows a batch that needs none
int host_resto(dart_mpc_handle* h, dartmpc::PmpcArgs a, const int32_t* host_status, hipStream_t s) {
    if (a.resto != 2) return DART_MPC_OK;
    bool any = false;
    for (int b = 0; b < a.B && !any; ++b)
        any = __atomic_load_n(host_status + b, __ATOMIC_ACQUIRE) == dartmpc::kPmNeedResto;
    if (!any) return DART_MPC_OK;
    a.done = nullptr;
    HIPCHK(h, dartmpc_launch_pmpc_resto(&a, s), "restoration kernel launch");
    HIPCHK(h, hipStreamSynchronize(s), "restoration kernel");
    return DART_MPC_OK;
}

int stream_state(dart_mpc_handle* h, int B, hipStream_t s, double** out, int* xcd);

// the restoration hand-off area of a PMPC launch of B instances on stream s (when the launch can hand over)
int pmpc_resto_buf(dart_mpc_handle* h, int B, hipStream_t s, dartmpc::PmpcArgs& a) {
    a.resto_buf = nullptr;
    // Resuming from the register kernel's failed iteration is opt-in (DART_PMPC_RESUME=1): the register kernel's
    // iterate differs from the sequential (oracle-ordered) arithmetic by rounding, and the restoration phase
    // turns that into different iteration counts on ~19 % of the restored instances (the same statuses, u0
    // within 1.3e-11; tools/pmpc_resume_check.py, profiles/r05/pmpc_resume.txt).  By default the restoration
    // solve starts over on the LDS engine and takes the oracle's iterations exactly.
    static const bool resume = [] {
        const char* e = getenv("DART_PMPC_RESUME");
        return e && e[0] == '1';
    }();
    if (!a.resto || !resume) return DART_MPC_OK;
    int xcd = 0;
    return stream_state(h, B, s, &a.resto_buf, &xcd);
}

// kernel arguments reading / writing the I/O area
dartmpc::PmpcArgs io_args(dart_mpc_handle* h, int B, bool ww, bool wo, int resto_mode = 1) {
    const auto& o = h->io;
    dartmpc::PmpcArgs a;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.max_iter = h->cfg.max_iter; a.g = h->cfg.gravity;
    a.max_soc = h->cfg.max_soc; a.reduced = h->cfg.pmpc_path; a.mult_init_max = h->cfg.constr_mult_init_max;
    a.x0 = (const double*)o.din; a.ref = (const double*)(o.din + o.off_ref); a.prm = (const double*)(o.din + o.off_prm);
    a.w_warm = ww ? (const double*)(o.din + o.off_ww) : nullptr;
    a.u0 = (double*)o.dout; a.f = (double*)(o.dout + o.off_f); a.w_out = wo ? (double*)(o.dout + o.off_wo) : nullptr;
    a.status = (int32_t*)(o.dout + o.off_st); a.iters = (int32_t*)(o.dout + o.off_it);
    a.done = h->ddone; a.seq = h->seq;
    a.resto = pmpc_resto_mode(h, resto_mode);
    a.soft = pmpc_soft(h);
    a.resto_buf = nullptr;        // (the caller sets it for its stream: pmpc_resto_buf)
    return a;
}

// (re)launch the resident grid; it takes every request with a sequence other than `seen`
hipError_t server_launch(dart_mpc_handle* h, uint32_t seen) {
    auto& v = h->srv;
    dartmpc::PmpcArgs a = io_args(h, v.B, true, true, 2);  // the flags of each request select w_warm / w_out
    a.seq = seen;
    if (pmpc_resto_buf(h, v.B, v.stream, a) != DART_MPC_OK) return hipErrorOutOfMemory;
    dartmpc::PmpcServe sv{v.dmbox, v.idle_ticks};
    const hipError_t e = dartmpc_launch_pmpc_serve(&a, &sv, v.stream);
    v.running = e == hipSuccess;
    v.t_post = std::chrono::steady_clock::now();
    return e;
}

// stop the resident server (if any) and wait until its grid has drained
int server_stop(dart_mpc_handle* h) {
    auto& v = h->srv;
    if (!v.stream) return DART_MPC_OK;
    __atomic_store_n((unsigned long long*)v.mbox, (unsigned long long)v.mbox[0] | (1ull << 56), __ATOMIC_RELEASE);
    const hipError_t e = hipStreamSynchronize(v.stream);
    v.running = false;
    server_release(h);
    return e == hipSuccess ? DART_MPC_OK : fail(h, DART_MPC_EHIP, "resident server", e);
}

// The per-stream state of PMPC / LMPC launches on stream s: the restoration hand-off area for B instances
// (device memory, stream-ordered growth: see dart_mpc_handle::resto; PMPC pmpc_model.h kPmHo doubles per
// instance, LMPC 64 x 16) and the XCD that a small LMPC batch's working blocks take -- streams get XCDs round
// robin, so that batches in flight on different streams of a handle run side by side on different XCDs instead
// of queueing for the CUs of one
int stream_state(dart_mpc_handle* h, int B, hipStream_t s, double** out, int* xcd) {
    *out = nullptr;
    // per instance: PMPC's hand-off state, LMPC's hand-off state (N > 31: and the two-wave build's second-order-
    // correction and restoration state, needed with or without the restoration phases), RMPC's two-wave
    // restoration state
    const bool wg2 = h->cfg.N > 31 || dartmpc::force_wg2();
    const size_t per = h->cfg.variant == DART_MPC_PMPC   ? (size_t)dartmpc::kPmHo
                       : h->cfg.variant == DART_MPC_RMPC ? (dartmpc_rmpc_wg2_resto_bytes() + 7) / 8
                       : wg2                             ? dartmpc_lmpc_wg2_area_doubles()
                                                         : (size_t)64 * 16;
    const size_t need = (h->cfg.restoration || (wg2 && h->cfg.variant == DART_MPC_LMPC)) ? (size_t)B * per : 0;
    dart_mpc_handle::RestoArea* r = nullptr;
    for (auto& e : h->resto)
        if (e.s == s) r = &e;
    if (!r) {
        // at most kMaxRestoAreas streams keep an area: the least recently used one is freed (a caller that makes
        // a new stream per call does not grow device memory without bound).  Its stream may be gone by now, so the
        // area is freed with hipFree, which waits for the device's outstanding work first (this rare path only).
        constexpr size_t kMaxRestoAreas = 8;
        if (h->resto.size() >= kMaxRestoAreas) {
            // (never the resident server's: its grid may hand an instance over into it at any time)
            size_t v = 0;
            while (v + 1 < h->resto.size() && h->srv.stream && h->resto[v].s == h->srv.stream) ++v;
            dart_mpc_handle::RestoArea old = h->resto[v];
            h->resto.erase(h->resto.begin() + v);
            if (old.buf) HIPCHK(h, hipFree(old.buf), "hipFree (restoration hand-off)");
        }
        h->resto.push_back({s, nullptr, 0, (int)(h->xcd_next++ & 7u)});
        r = &h->resto.back();
    } else if (r != &h->resto.back()) {     // most recently used last
        dart_mpc_handle::RestoArea cur = *r;
        h->resto.erase(h->resto.begin() + (r - h->resto.data()));
        h->resto.push_back(cur);
        r = &h->resto.back();
    }
    if (need > r->cap) {
        if (r->buf) HIPCHK(h, hipFreeAsync(r->buf, s), "hipFreeAsync (restoration hand-off)");
        r->buf = nullptr; r->cap = 0;
        HIPCHK(h, hipMallocAsync((void**)&r->buf, need * sizeof(double), s), "hipMallocAsync (restoration hand-off)");
        r->cap = need;
    }
    *out = r->buf;
    *xcd = r->xcd;
    return DART_MPC_OK;
}

int settle_pending(dart_mpc_handle* h) {
    if (!h->pending) return DART_MPC_OK;
    hipStream_t s = h->pending;
    h->pending = nullptr;
    hipError_t e = hipStreamQuery(s);
    if (e == hipErrorNotReady) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(h, DART_MPC_EHIP, "previous PMPC call's stream", e);
    return DART_MPC_OK;
}

int launch(dart_mpc_handle* h, int B, const double* x0, const double* ref, const double* prm, const double* w_warm,
           double* u0, double* f, double* w_out, int32_t* status, int32_t* iters, hipStream_t s) {
    dartmpc::PmpcArgs a;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.max_iter = h->cfg.max_iter; a.g = h->cfg.gravity;
    a.max_soc = h->cfg.max_soc; a.reduced = h->cfg.pmpc_path;
    a.mult_init_max = h->cfg.constr_mult_init_max;
    a.x0 = x0; a.ref = ref; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    a.done = nullptr; a.seq = 0;
    a.resto = pmpc_resto_mode(h, 1);
    a.soft = pmpc_soft(h);
    if (int rc = pmpc_resto_buf(h, B, s, a)) return rc;
    HIPCHK(h, dartmpc_launch_pmpc(&a, s), "kernel launch");
    return DART_MPC_OK;
}

// Wait for the B completion words of a host-pointer PMPC launch (mapped host memory, written last by
// every instance with a system-scope release).  Spinning on them returns as soon as the last store
// lands, without the stream-completion round trip; the stream is queried now and then, and if it is
// done (or failed) without every word set, the stream's own status decides.
int wait_done(dart_mpc_handle* h, hipStream_t s, const volatile uint32_t* done, int B, uint32_t seq) {
    for (unsigned n = 1;; ++n) {
        int b = 0;
        while (b < B && __atomic_load_n(done + b, __ATOMIC_ACQUIRE) == seq) ++b;
        if (b == B) return DART_MPC_OK;
        if ((n & 255) == 0 && hipStreamQuery(s) != hipErrorNotReady) break;
        __builtin_ia32_pause();
    }
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    for (int b = 0; b < B; ++b)
        if (__atomic_load_n(done + b, __ATOMIC_ACQUIRE) != seq) return fail(h, DART_MPC_EHIP, "kernel did not complete");
    return DART_MPC_OK;
}

// the next completion-word sequence of the handle (wraps, skipping 0; on a wrap every word is cleared so that
// no stale one can match: the words only ever hold 0 or sequences of earlier requests)
uint32_t next_seq(dart_mpc_handle* h) {
    if (++h->seq == 0) {
        std::memset(h->hdone, 0, sizeof(uint32_t) * h->cfg.B_max);
        h->seq = 1;
    }
    return h->seq;
}

// A served request's instances that the resident grid handed over (status kPmNeedResto: IPOPT's restoration
// phases): the grid is drained (its waves hold the SIMDs while they wait for requests) and pmpc_resto_kernel
// runs over the I/O area on the server's stream; the next request relaunches the grid.
int served_resto(dart_mpc_handle* h, int B, bool ww, bool wo) {
    auto& v = h->srv;
    const int32_t* st = (const int32_t*)(h->io.hout + h->io.off_st);
    bool any = false;
    for (int b = 0; b < B && !any; ++b) any = __atomic_load_n(st + b, __ATOMIC_ACQUIRE) == dartmpc::kPmNeedResto;
    if (!any) return DART_MPC_OK;
    __atomic_store_n((unsigned long long*)v.mbox, (unsigned long long)v.mbox[0] | (1ull << 56), __ATOMIC_RELEASE);
    v.running = false;
    HIPCHK(h, hipStreamSynchronize(v.stream), "resident server");
    dartmpc::PmpcArgs a = io_args(h, B, ww, wo, 1);
    a.done = nullptr;
    if (int rc = pmpc_resto_buf(h, v.B, v.stream, a)) return rc;      // the area the grid handed over into
    HIPCHK(h, dartmpc_launch_pmpc_resto(&a, v.stream), "restoration kernel launch");
    HIPCHK(h, hipStreamSynchronize(v.stream), "restoration kernel");
    return DART_MPC_OK;
}

// post a request to the resident server (inputs already in the I/O area) and wait for its B
// completion words; a grid that drained meanwhile (idle timeout) is relaunched and takes the request
int served_request(dart_mpc_handle* h, int B, bool ww, bool wo) {
    auto& v = h->srv;
    // Every wave leaves idle_timeout after the last request it saw, each on its own clock, so near the end of
    // an idle period part of the grid may have left while the rest still waits (and a request posted then
    // would reset the waiting waves' timers and wait out a whole idle period for the missing ones).  The host
    // knows when it posted last: from 90 % of the idle timeout on, it drains the grid itself (stop word) and
    // relaunches it before posting.  Before that point no wave can have left (each wave's last request is no
    // older than the host's last post).
    const double since = std::chrono::duration<double>(std::chrono::steady_clock::now() - v.t_post).count();
    // The margin between this check and a wave's own timeout is 10 % of the timeout + 2 ms, capped at half the
    // timeout (so that short timeouts still serve from the grid), but never below 2 ms: a host stall between the
    // check and the post longer than the margin could let part of the grid leave, and the request would then
    // wait out a further idle period.  Timeouts of 4 ms and less therefore pre-drain (relaunch) whenever more
    // than idle - 2 ms has passed: a latency cost, never a stall.
    const double margin = std::fmax(0.002, std::fmin(0.1 * v.idle_s + 0.002, 0.5 * v.idle_s));
    if (v.running && since > v.idle_s - margin) {
        __atomic_store_n((unsigned long long*)v.mbox, (unsigned long long)v.mbox[0] | (1ull << 56), __ATOMIC_RELEASE);
        v.running = false;
    }
    if (!v.running || hipStreamQuery(v.stream) != hipErrorNotReady) {     // drained (idle timeout or stop)
        v.running = false;
        HIPCHK(h, hipStreamSynchronize(v.stream), "resident server");
        __atomic_store_n((unsigned long long*)v.mbox, (unsigned long long)h->seq, __ATOMIC_RELEASE);   // no stop, no request
        HIPCHK(h, server_launch(h, h->seq), "resident server relaunch");
    }
    const uint32_t sq = next_seq(h);
    const unsigned long long fl = (ww ? 1ull : 0ull) | (wo ? 2ull : 0ull);
    __atomic_store_n((unsigned long long*)v.mbox, (unsigned long long)sq | ((unsigned long long)B << 32) | (fl << 48),
                     __ATOMIC_RELEASE);
    v.t_post = std::chrono::steady_clock::now();
    for (unsigned n = 1;; ++n) {
        int bb = 0;
        while (bb < B && __atomic_load_n(h->hdone + bb, __ATOMIC_ACQUIRE) == sq) ++bb;
        if (bb == B) return served_resto(h, B, ww, wo);
        if ((n & 1023) == 0 && hipStreamQuery(v.stream) != hipErrorNotReady) {
            bb = 0;
            while (bb < B && __atomic_load_n(h->hdone + bb, __ATOMIC_ACQUIRE) == sq) ++bb;
            if (bb == B) return served_resto(h, B, ww, wo);
            v.running = false;
            HIPCHK(h, hipStreamSynchronize(v.stream), "resident server");
            // the grid drained before it saw the request: relaunch with the request already posted
            HIPCHK(h, server_launch(h, sq - 1), "resident server relaunch");
        }
        __builtin_ia32_pause();
    }
}

// one launch over the I/O area (no resident server), completion words as the host entry
int bound_launch(dart_mpc_handle* h, int B, bool ww, bool wo) {
    next_seq(h);
    dartmpc::PmpcArgs a = io_args(h, B, ww, wo, B <= 32 ? 1 : 2);
    if (int rc = pmpc_resto_buf(h, B, h->stream, a)) return rc;
    HIPCHK(h, dartmpc_launch_pmpc(&a, h->stream), "kernel launch");
    int rc = wait_done(h, h->stream, h->hdone, B, a.seq);
    if (rc == DART_MPC_OK) rc = host_resto(h, a, (const int32_t*)(h->io.hout + h->io.off_st), h->stream);
    if (rc == DART_MPC_OK) h->pending = h->stream;
    return rc;
}

}  // namespace

extern "C" {

void dart_mpc_config_default(dart_mpc_config* c) {
    if (!c) return;
    c->variant = DART_MPC_PMPC;
    c->N = 20;
    c->Ts = 0.002;
    c->tol = 1e-8;
    c->max_iter = 3000;
    c->B_max = 1024;
    c->gravity = -9.81;
    c->acceptable_tol = 1e-6;      // IPOPT defaults
    c->acceptable_iter = 15;
    c->max_soc = 4;
    c->pmpc_path = 0;
    c->constr_mult_init_max = 1000.0;
    c->restoration = 1;
    c->max_cpu_time = 0.05;         // rlmpc2.py:485
}

int dart_mpc_nw(int N) { return 6 * (N + 1) + 2 * N; }

int dart_rmpc_nw(int N) { return 4 * (N + 1) + 2 * N; }

int dart_lmpc_nw(int N) { return 8 * (N + 1) + 2 * N; }

int dart_mpc_abi_version(void) { return DART_MPC_ABI_VERSION; }
#ifndef DART_BUILD_ID
#define DART_BUILD_ID "unknown"
#endif
const char* dart_mpc_build_id(void) { return DART_BUILD_ID; }
const char* dart_mpc_build_flavor(void) {
#if defined(DART_STAMPS)
    return "stamps";
#elif defined(DART_RESTO_TRACE)
    return "trace";
#else
    return "";
#endif
}

int dart_mpc_create(const dart_mpc_config* cfg, int device, dart_mpc_handle** out) {
    if (!out || !check_cfg(cfg)) return DART_MPC_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return DART_MPC_ENODEV;
    dart_mpc_handle* h = new dart_mpc_handle();
    h->cfg = *cfg;
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    // staging for B_max instances: inputs (+ in/out arrays) and outputs, 256-byte aligned per array
    const size_t B = (size_t)cfg->B_max, A = 8 * 256;
    size_t nin = 0, nout = 0;
    if (cfg->variant == DART_MPC_LMPC) {
        const size_t nw = (size_t)dart_lmpc_nw(cfg->N);
        nin = B * (8 + 2 + dartmpc::LM_NPV + 8 + dartmpc::LM_NPRM + nw);
        nout = B * (2 + 1 + nw + 1);
    } else if (cfg->variant == DART_MPC_RMPC) {
        const size_t nw = (size_t)dart_rmpc_nw(cfg->N);
        nin = B * (4 + 2 + 14 + 98 + 7 + 2 + 4 * (cfg->N + 1) + 10 + nw);
        nout = B * (2 + 1 + nw + 1);
    } else {
        const size_t nw = (size_t)dart_mpc_nw(cfg->N);
        nin = B * (6 + 6 + 6 + nw);
        nout = B * (2 + 1 + nw + 1);
    }
    // PMPC reads its inputs zero-copy (dart_mpc_solve_batch): their pinned buffer is the mapped one
    const bool zc = cfg->variant == DART_MPC_PMPC;
    if (e == hipSuccess)
        e = h->st.reserve(zc ? A : nin * sizeof(double) + A, nout * sizeof(double) + A, zc ? nin * sizeof(double) + A : 0);
    if (e == hipSuccess && zc) {
        e = hipHostMalloc((void**)&h->hdone, sizeof(uint32_t) * B, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) {
            std::memset(h->hdone, 0, sizeof(uint32_t) * B);
            e = hipHostGetDevicePointer((void**)&h->ddone, h->hdone, 0);
        }
    }
    if (e != hipSuccess) {
        dart_mpc_destroy(h);
        return DART_MPC_EHIP;
    }
    *out = h;
    return DART_MPC_OK;
}

int dart_mpc_solve_batch_dev(dart_mpc_handle* h, int B, const double* x0, const double* ref, const double* prm,
                             const double* w_warm, double* u0, double* f, double* w_out, int32_t* status,
                             int32_t* iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_PMPC) return fail(h, DART_MPC_EINVAL, "handle is not a PMPC handle");
    if (B < 0 || (B > 0 && (!x0 || !ref || !prm || !u0 || !f || !status || !iters)))
        return fail(h, DART_MPC_EINVAL, "null pointer or negative batch");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    if (int rc = settle_pending(h)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    return launch(h, B, x0, ref, prm, w_warm, u0, f, w_out, status, iters, s);
}

int dart_mpc_solve_batch(dart_mpc_handle* h, int B, const double* x0, const double* ref, const double* prm,
                         const double* w_warm, double* u0, double* f, double* w_out, int32_t* status,
                         int32_t* iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_PMPC) return fail(h, DART_MPC_EINVAL, "handle is not a PMPC handle");
    if (B < 0 || (B > 0 && (!x0 || !ref || !prm || !u0 || !f || !status || !iters)))
        return fail(h, DART_MPC_EINVAL, "null pointer or negative batch");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    if (int rc = settle_pending(h)) return rc;
    const size_t nw = (size_t)dart_mpc_nw(h->cfg.N);
    if (h->srv.wanted && B <= h->srv.B && !stream) {
        // resident server: inputs into the I/O area, the request posted by the request word
        const auto& o = h->io;
        std::memcpy(o.hin, x0, sizeof(double) * 6 * B);
        std::memcpy(o.hin + o.off_ref, ref, sizeof(double) * 6 * B);
        std::memcpy(o.hin + o.off_prm, prm, sizeof(double) * 6 * B);
        if (w_warm) std::memcpy(o.hin + o.off_ww, w_warm, sizeof(double) * nw * B);
        if (int rc = served_request(h, B, w_warm != nullptr, w_out != nullptr)) return rc;
        std::memcpy(u0, o.hout, sizeof(double) * 2 * B);
        std::memcpy(f, o.hout + o.off_f, sizeof(double) * B);
        if (w_out) std::memcpy(w_out, o.hout + o.off_wo, sizeof(double) * nw * B);
        std::memcpy(status, o.hout + o.off_st, sizeof(int32_t) * B);
        std::memcpy(iters, o.hout + o.off_it, sizeof(int32_t) * B);
        return DART_MPC_OK;
    }
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;

    HostStage& S = h->st;
    S.begin();
    // the PMPC kernel reads x0 / ref / prm / w_warm once, at its start: zero-copy from mapped host
    // memory instead of a DMA copy on the call path
    const double* d_x0 = S.in_zc(x0, 6 * B);
    const double* d_ref = S.in_zc(ref, 6 * B);
    const double* d_prm = S.in_zc(prm, 6 * B);
    const double* d_ww = S.in_zc(w_warm, nw * B);
    double* d_u0 = S.out<double>(2 * B);
    double* d_f = S.out<double>(B);
    double* d_wo = w_out ? S.out<double>(nw * B) : nullptr;
    int32_t* d_st = S.out<int32_t>(B);
    int32_t* d_it = S.out<int32_t>(B);
    uint32_t* d_done = h->ddone;
    HIPCHK(h, S.upload(s), "copy inputs");
    dartmpc::PmpcArgs a;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.max_iter = h->cfg.max_iter; a.g = h->cfg.gravity;
    a.max_soc = h->cfg.max_soc; a.reduced = h->cfg.pmpc_path;
    a.mult_init_max = h->cfg.constr_mult_init_max;
    a.x0 = d_x0; a.ref = d_ref; a.prm = d_prm; a.w_warm = d_ww;
    a.u0 = d_u0; a.f = d_f; a.w_out = d_wo; a.status = d_st; a.iters = d_it;
    a.done = d_done; a.seq = next_seq(h);
    a.resto = host_resto_mode(h, B);
    a.soft = pmpc_soft(h);
    if (int rc = pmpc_resto_buf(h, B, s, a)) return rc;
    HIPCHK(h, dartmpc_launch_pmpc(&a, s), "kernel launch");
    int rc = wait_done(h, s, h->hdone, B, a.seq);
    if (rc == DART_MPC_OK) rc = host_resto(h, a, S.host_of(d_st), s);
    if (rc) return rc;
    h->pending = s;
    S.take(u0, d_u0, 2 * B); S.take(f, d_f, B); S.take(w_out, d_wo, nw * B);
    S.take(status, d_st, B); S.take(iters, d_it, B);
    return DART_MPC_OK;
}

int dart_rmpc_solve_batch_dev(dart_mpc_handle* h, int B, const double* x0, const double* u_prev, double* theta,
                              double* rls_P, const double* rls_phi, const double* rls_y, double rls_lambda,
                              const double* Rref, const double* prm, const double* w_warm, double* u0, double* f,
                              double* w_out, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_RMPC) return fail(h, DART_MPC_EINVAL, "handle is not an RMPC handle");
    if (B < 0 || (B > 0 && (!x0 || !u_prev || !theta || !Rref || !prm || !u0 || !f || !status || !iters)))
        return fail(h, DART_MPC_EINVAL, "null pointer or negative batch");
    if (rls_P && (!rls_phi || !rls_y || !(rls_lambda > 0.0))) return fail(h, DART_MPC_EINVAL, "RLS inputs incomplete");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::RmpcArgs a;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.g = h->cfg.gravity; a.max_iter = h->cfg.max_iter; a.mult_init_max = h->cfg.constr_mult_init_max;
    a.resto = h->cfg.restoration; a.max_soc = h->cfg.max_soc;
    a.x0 = x0; a.u_prev = u_prev; a.theta = theta; a.rls_P = rls_P; a.rls_phi = rls_phi; a.rls_y = rls_y;
    a.rls_lambda = rls_lambda; a.Rref = Rref; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    a.resto_buf = nullptr;
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if ((a.N > 31 || dartmpc::force_wg2()) && a.resto) {      // the two-wave build's restoration state, one area per stream
        int xcd = 0;
        if (int rc = stream_state(h, B, s, &a.resto_buf, &xcd)) return rc;
    }
    HIPCHK(h, dartmpc_launch_rmpc(&a, s), "kernel launch");
    return DART_MPC_OK;
}

int dart_rmpc_solve_batch(dart_mpc_handle* h, int B, const double* x0, const double* u_prev, double* theta,
                          double* rls_P, const double* rls_phi, const double* rls_y, double rls_lambda,
                          const double* Rref, const double* prm, const double* w_warm, double* u0, double* f,
                          double* w_out, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_RMPC) return fail(h, DART_MPC_EINVAL, "handle is not an RMPC handle");
    if (B < 0 || (B > 0 && (!x0 || !u_prev || !theta || !Rref || !prm || !u0 || !f || !status || !iters)))
        return fail(h, DART_MPC_EINVAL, "null pointer or negative batch");
    if (rls_P && (!rls_phi || !rls_y || !(rls_lambda > 0.0))) return fail(h, DART_MPC_EINVAL, "RLS inputs incomplete");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t N = (size_t)h->cfg.N, nw = (size_t)dart_rmpc_nw(h->cfg.N);
    HostStage& S = h->st;
    S.begin();
    const double* d_x0 = S.in(x0, 4 * B);
    const double* d_up = S.in(u_prev, 2 * B);
    const double* d_phi = rls_P ? S.in(rls_phi, 7 * B) : nullptr;
    const double* d_y = rls_P ? S.in(rls_y, 2 * B) : nullptr;
    const double* d_R = S.in(Rref, 4 * (N + 1) * B);
    const double* d_prm = S.in(prm, 10 * B);
    const double* d_ww = S.in(w_warm, nw * B);
    // theta is updated in place only when the RLS step is fused
    double* d_th = rls_P ? S.inout(theta, 14 * B) : const_cast<double*>(S.in(theta, 14 * B));
    double* d_P = rls_P ? S.inout(rls_P, 98 * B) : nullptr;
    double* d_u0 = S.out<double>(2 * B);
    double* d_f = S.out<double>(B);
    double* d_wo = w_out ? S.out<double>(nw * B) : nullptr;
    int32_t* d_st = S.out<int32_t>(B);
    int32_t* d_it = S.out<int32_t>(B);
    HIPCHK(h, S.upload(s), "copy inputs");
    int rc = dart_rmpc_solve_batch_dev(h, B, d_x0, d_up, d_th, d_P, d_phi, d_y, rls_lambda, d_R, d_prm, d_ww, d_u0, d_f,
                                       d_wo, d_st, d_it, s);
    if (rc) return rc;
    HIPCHK(h, S.download_inout(s), "copy theta / rls_P");
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    S.finish_inout();
    S.take(u0, d_u0, 2 * B); S.take(f, d_f, B); S.take(w_out, d_wo, nw * B);
    S.take(status, d_st, B); S.take(iters, d_it, B);
    return DART_MPC_OK;
}

int dart_lmpc_solve_batch_dev(dart_mpc_handle* h, int B, const double* state, const double* u_prev,
                              const double* pvec, const double* target, const double* prm, const double* w_warm,
                              double* u0, double* f, double* w_out, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, "handle is not an LMPC handle");
    if (B < 0 || (B > 0 && (!state || !u_prev || !pvec || !target || !prm || !u0 || !f || !status || !iters)))
        return fail(h, DART_MPC_EINVAL, "null pointer or negative batch");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::LmpcArgs a;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.max_iter = h->cfg.max_iter;
    a.acc_tol = h->cfg.acceptable_tol; a.acc_iter = h->cfg.acceptable_iter; a.max_soc = h->cfg.max_soc; a.mult_init_max = h->cfg.constr_mult_init_max;
    a.resto = h->cfg.restoration;
    a.max_ticks = (long long)(h->cfg.max_cpu_time * 1e8);     // s_memrealtime: 100 MHz
    if (int rc = stream_state(h, B, stream ? (hipStream_t)stream : h->stream, &a.resto_buf, &a.xcd)) return rc;
    a.state = state; a.u_prev = u_prev; a.pvec = pvec; a.target = target; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    a.fuse_policy = 0;
    HIPCHK(h, dartmpc_launch_lmpc(&a, stream ? (hipStream_t)stream : h->stream), "kernel launch");
    return DART_MPC_OK;
}

int dart_lmpc_solve_batch(dart_mpc_handle* h, int B, const double* state, const double* u_prev, const double* pvec,
                          const double* target, const double* prm, const double* w_warm, double* u0, double* f,
                          double* w_out, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, "handle is not an LMPC handle");
    if (B < 0 || (B > 0 && (!state || !u_prev || !pvec || !target || !prm || !u0 || !f || !status || !iters)))
        return fail(h, DART_MPC_EINVAL, "null pointer or negative batch");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N);
    HostStage& S = h->st;
    S.begin();
    const double* d_st0 = S.in(state, 8 * B);
    const double* d_up = S.in(u_prev, 2 * B);
    const double* d_pv = S.in(pvec, dartmpc::LM_NPV * B);
    const double* d_tg = S.in(target, 8 * B);
    const double* d_prm = S.in(prm, dartmpc::LM_NPRM * B);
    const double* d_ww = S.in(w_warm, nw * B);
    double* d_u0 = S.out<double>(2 * B);
    double* d_f = S.out<double>(B);
    double* d_wo = w_out ? S.out<double>(nw * B) : nullptr;
    int32_t* d_st = S.out<int32_t>(B);
    int32_t* d_it = S.out<int32_t>(B);
    HIPCHK(h, S.upload(s), "copy inputs");
    int rc = dart_lmpc_solve_batch_dev(h, B, d_st0, d_up, d_pv, d_tg, d_prm, d_ww, d_u0, d_f, d_wo, d_st, d_it, s);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    S.take(u0, d_u0, 2 * B); S.take(f, d_f, B); S.take(w_out, d_wo, nw * B);
    S.take(status, d_st, B); S.take(iters, d_it, B);
    return DART_MPC_OK;
}

void dart_lmpc_policy_config_default(dart_lmpc_policy_config* c) {
    if (!c) return;
    c->update_every = 8;
    c->reserved = 0;
    c->max_delta = 0.02;
    c->k_max = 2.0;
    c->min_k = 1e-2;
    c->k_ceiling_margin = std::fmax(1e-3, 0.05 * c->k_max);
    c->action_scale = 1.0;
    c->smooth_alpha = 0.5;
    c->log_std_min = std::log(1e-2);
    c->log_std_max = std::log(2.0);
}

static int policy_args(const dart_lmpc_policy_config* c, int B, const float* w, dartmpc::PolicyArgs& a) {
    if (!c || B < 0 || !w || c->update_every < 1 || !(c->k_max > c->min_k) || !(c->min_k > 0.0)) return DART_MPC_EINVAL;
    a.B = B;
    a.w.W1 = w; a.w.b1 = w + 520 * 64; a.w.W2 = a.w.b1 + 64; a.w.b2 = a.w.W2 + 64 * 64;
    a.w.W3 = a.w.b2 + 64; a.w.b3 = a.w.W3 + 64 * 34; a.w.log_std = a.w.b3 + 34;
    a.update_every = c->update_every;
    a.max_delta = c->max_delta; a.k_max = c->k_max; a.min_k = c->min_k; a.k_ceiling_margin = c->k_ceiling_margin;
    a.action_scale = c->action_scale; a.smooth_alpha = c->smooth_alpha;
    a.log_std_min = c->log_std_min; a.log_std_max = c->log_std_max;
    return DART_MPC_OK;
}

int dart_lmpc_policy_step_dev(const dart_lmpc_policy_config* cfg, int B, const float* weights, const double* state,
                              const double* target, const double* control, const double* current_k, double* obs_mean,
                              double* obs_M2, int32_t* obs_count, float* history, int32_t* timestep, const float* noise,
                              double* model_params, float* action_out, void* stream) {
    dartmpc::PolicyArgs a;
    if (policy_args(cfg, B, weights, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    if (B > 0 && (!state || !target || !control || !current_k || !obs_mean || !obs_M2 || !obs_count || !history ||
                  !timestep || !noise || !model_params)) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    a.state = state; a.target = target; a.control = control; a.current_k = current_k; a.obs_mean = obs_mean;
    a.obs_M2 = obs_M2; a.obs_count = obs_count; a.history = history; a.timestep = timestep; a.noise = noise;
    a.model_params = model_params; a.action_out = action_out;
    return dartmpc_launch_policy(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_policy_step(const dart_lmpc_policy_config* cfg, int B, const float* weights, const double* state,
                          const double* target, const double* control, const double* current_k, double* obs_mean,
                          double* obs_M2, int32_t* obs_count, float* history, int32_t* timestep, const float* noise,
                          double* model_params, float* action_out) {
    dartmpc::PolicyArgs a;
    if (policy_args(cfg, B, weights, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    if (B > 0 && (!state || !target || !control || !current_k || !obs_mean || !obs_M2 || !obs_count || !history ||
                  !timestep || !noise || !model_params)) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t nin = sizeof(float) * ((size_t)DART_LMPC_POLICY_NWEIGHTS + (size_t)B * (34 + 520)) +
                       sizeof(double) * (size_t)B * (8 + 8 + 2 + 34 + 52 + 52 + 34) + sizeof(int32_t) * 2 * B + 16 * 256;
    if (S.reserve(nin, sizeof(float) * 34 * B + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const float* d_w = S.in(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS);
    a.w.W1 = d_w; a.w.b1 = d_w + 520 * 64; a.w.W2 = a.w.b1 + 64; a.w.b2 = a.w.W2 + 64 * 64;
    a.w.W3 = a.w.b2 + 64; a.w.b3 = a.w.W3 + 64 * 34; a.w.log_std = a.w.b3 + 34;
    a.state = S.in(state, 8 * (size_t)B); a.target = S.in(target, 8 * (size_t)B);
    a.control = S.in(control, 2 * (size_t)B); a.current_k = S.in(current_k, 34 * (size_t)B);
    a.noise = S.in(noise, 34 * (size_t)B);
    a.obs_mean = S.inout(obs_mean, 52 * (size_t)B); a.obs_M2 = S.inout(obs_M2, 52 * (size_t)B);
    a.model_params = S.inout(model_params, 34 * (size_t)B); a.history = S.inout(history, 520 * (size_t)B);
    a.obs_count = S.inout(obs_count, (size_t)B); a.timestep = S.inout(timestep, (size_t)B);
    a.action_out = S.out<float>(34 * (size_t)B);
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess) e = dartmpc_launch_policy(&a, D->stream);
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
    S.take(action_out, a.action_out, 34 * (size_t)B);
    return DART_MPC_OK;
}


// fused policy step + LMPC solve: one launch (lmpc_ipm.hip prologue = policy_step_wave)
int dart_lmpc_policy_solve_batch_dev(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, int B,
                                     const float* weights, const double* state, const double* u_prev,
                                     const double* target, const double* current_k, double* obs_mean, double* obs_M2,
                                     int32_t* obs_count, float* history, int32_t* timestep, const float* noise,
                                     double* model_params, float* action_out, const double* prm, const double* w_warm,
                                     double* u0, double* f, double* w_out, int32_t* status, int32_t* iters,
                                     void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, "handle is not an LMPC handle");
    dartmpc::LmpcArgs a;
    if (policy_args(pcfg, B, weights, a.pol) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
    if (B > 0 && (!state || !u_prev || !target || !current_k || !obs_mean || !obs_M2 || !obs_count || !history ||
                  !timestep || !noise || !model_params || !prm || !u0 || !f || !status || !iters))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    a.pol.state = state; a.pol.target = target; a.pol.control = u_prev; a.pol.current_k = current_k;
    a.pol.obs_mean = obs_mean; a.pol.obs_M2 = obs_M2; a.pol.obs_count = obs_count; a.pol.history = history;
    a.pol.timestep = timestep; a.pol.noise = noise; a.pol.model_params = model_params; a.pol.action_out = action_out;
    a.fuse_policy = 1;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.max_iter = h->cfg.max_iter;
    a.acc_tol = h->cfg.acceptable_tol; a.acc_iter = h->cfg.acceptable_iter; a.max_soc = h->cfg.max_soc; a.mult_init_max = h->cfg.constr_mult_init_max;
    a.resto = h->cfg.restoration;
    a.max_ticks = (long long)(h->cfg.max_cpu_time * 1e8);     // s_memrealtime: 100 MHz
    if (int rc = stream_state(h, B, stream ? (hipStream_t)stream : h->stream, &a.resto_buf, &a.xcd)) return rc;
    a.state = state; a.u_prev = u_prev; a.pvec = nullptr; a.target = target; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    HIPCHK(h, dartmpc_launch_lmpc(&a, stream ? (hipStream_t)stream : h->stream), "kernel launch");
    return DART_MPC_OK;
}

int dart_lmpc_policy_solve_batch(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, int B, const float* weights,
                                 const double* state, const double* u_prev, const double* target,
                                 const double* current_k, double* obs_mean, double* obs_M2, int32_t* obs_count,
                                 float* history, int32_t* timestep, const float* noise, double* model_params,
                                 float* action_out, const double* prm, const double* w_warm, double* u0, double* f,
                                 double* w_out, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, "handle is not an LMPC handle");
    dartmpc::PolicyArgs chk;
    if (policy_args(pcfg, B, weights, chk) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
    if (B > 0 && (!state || !u_prev || !target || !current_k || !obs_mean || !obs_M2 || !obs_count || !history ||
                  !timestep || !noise || !model_params || !prm || !u0 || !f || !status || !iters))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N), Bz = (size_t)B;
    HostStage& S = h->st;
    const size_t nin = sizeof(float) * ((size_t)DART_LMPC_POLICY_NWEIGHTS + Bz * (34 + 520)) +
                       sizeof(double) * Bz * (8 + 2 + 8 + 34 + dartmpc::LM_NPRM + nw + 52 + 52 + 34) +
                       sizeof(int32_t) * 2 * Bz + 24 * 256;
    const size_t nout = sizeof(double) * Bz * (2 + 1 + nw) + sizeof(int32_t) * 2 * Bz + sizeof(float) * 34 * Bz + 8 * 256;
    HIPCHK(h, S.reserve(nin, nout), "staging buffers");
    S.begin();
    const float* d_w = S.in(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS);
    const double* d_st0 = S.in(state, 8 * Bz);
    const double* d_up = S.in(u_prev, 2 * Bz);
    const double* d_tg = S.in(target, 8 * Bz);
    const double* d_ck = S.in(current_k, 34 * Bz);
    const float* d_nz = S.in(noise, 34 * Bz);
    const double* d_prm = S.in(prm, dartmpc::LM_NPRM * Bz);
    const double* d_ww = S.in(w_warm, nw * Bz);
    double* d_mean = S.inout(obs_mean, 52 * Bz);
    double* d_M2 = S.inout(obs_M2, 52 * Bz);
    double* d_mp = S.inout(model_params, 34 * Bz);
    float* d_hist = S.inout(history, 520 * Bz);
    int32_t* d_cnt = S.inout(obs_count, Bz);
    int32_t* d_ts = S.inout(timestep, Bz);
    double* d_u0 = S.out<double>(2 * Bz);
    double* d_f = S.out<double>(Bz);
    double* d_wo = w_out ? S.out<double>(nw * Bz) : nullptr;
    int32_t* d_stt = S.out<int32_t>(Bz);
    int32_t* d_it = S.out<int32_t>(Bz);
    float* d_act = action_out ? S.out<float>(34 * Bz) : nullptr;
    HIPCHK(h, S.upload(s), "copy inputs");
    int rc = dart_lmpc_policy_solve_batch_dev(h, pcfg, B, d_w, d_st0, d_up, d_tg, d_ck, d_mean, d_M2, d_cnt, d_hist, d_ts,
                                              d_nz, d_mp, d_act, d_prm, d_ww, d_u0, d_f, d_wo, d_stt, d_it, s);
    if (rc) return rc;
    HIPCHK(h, S.download_inout(s), "copy policy state");
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    S.finish_inout();
    S.take(u0, d_u0, 2 * Bz); S.take(f, d_f, Bz); S.take(w_out, d_wo, nw * Bz);
    S.take(status, d_stt, Bz); S.take(iters, d_it, Bz); S.take(action_out, d_act, 34 * Bz);
    return DART_MPC_OK;
}

int dart_rls_update_batch_dev(int B, double* theta, double* P, const double* phi, const double* y, double lambda,
                              void* stream) {
    if (B < 0 || (B > 0 && (!theta || !P || !phi || !y)) || !(lambda > 0.0)) return DART_MPC_EINVAL;
    return dartmpc_launch_rls(B, theta, P, phi, y, lambda, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_set_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return DART_MPC_ENODEV;
    return hipSetDevice(device) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_rls_update_batch(int B, double* theta, double* P, const double* phi, const double* y, double lambda) {
    if (B < 0 || (B > 0 && (!theta || !P || !phi || !y)) || !(lambda > 0.0)) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    if (S.reserve(sizeof(double) * (size_t)B * (7 + 49 + 7 + 1) + 4 * 256, 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const double* dphi = S.in(phi, 7 * (size_t)B);
    const double* dy = S.in(y, (size_t)B);
    double* dt = S.inout(theta, 7 * (size_t)B);
    double* dP = S.inout(P, 49 * (size_t)B);
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess) e = dartmpc_launch_rls(B, dt, dP, dphi, dy, lambda, D->stream);
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
    return DART_MPC_OK;
}

int dart_mpc_serve_start(dart_mpc_handle* h, int B_serve, double idle_timeout_s) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_PMPC) return fail(h, DART_MPC_EINVAL, "handle is not a PMPC handle");
    if (h->cfg.N > 31 || h->cfg.pmpc_path != 0)
        return fail(h, DART_MPC_EINVAL, "the resident server serves IPOPT's path with N <= 31");
    if (B_serve < 1 || B_serve > h->cfg.B_max || B_serve > 65535 || !(idle_timeout_s > 0.0) || idle_timeout_s > 3600.0)
        return fail(h, DART_MPC_EINVAL, "B_serve must be in [1, min(B_max, 65535)], idle timeout in (0, 3600] s");
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    if (int rc = settle_pending(h)) return rc;
    if (int rc = server_stop(h)) return rc;
    HIPCHK(h, ensure_io(h), "I/O area");
    auto& v = h->srv;
    hipError_t e = hipHostMalloc((void**)&v.mbox, 256, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&v.dmbox, v.mbox, 0);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&v.stream, hipStreamNonBlocking);
    if (e != hipSuccess) { server_release(h); return fail(h, DART_MPC_EHIP, "resident server buffers", e); }
    std::memset(v.mbox, 0, 256);
    v.B = B_serve;
    v.idle_ticks = (unsigned long long)(idle_timeout_s * 1.0e8);      // s_memrealtime: 100 MHz
    v.idle_s = idle_timeout_s;
    v.mbox[0] = h->seq;
    e = server_launch(h, h->seq);
    if (e != hipSuccess) { server_release(h); return fail(h, DART_MPC_EHIP, "resident server launch", e); }
    v.wanted = true;
    return DART_MPC_OK;
}

int dart_mpc_bind(dart_mpc_handle* h, double** x0, double** ref, double** prm, double** w_warm, double** u0, double** f,
                  double** w_out, int32_t** status, int32_t** iters) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_PMPC) return fail(h, DART_MPC_EINVAL, "handle is not a PMPC handle");
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    HIPCHK(h, ensure_io(h), "I/O area");
    const auto& o = h->io;
    if (x0) *x0 = (double*)o.hin;
    if (ref) *ref = (double*)(o.hin + o.off_ref);
    if (prm) *prm = (double*)(o.hin + o.off_prm);
    if (w_warm) *w_warm = (double*)(o.hin + o.off_ww);
    if (u0) *u0 = (double*)o.hout;
    if (f) *f = (double*)(o.hout + o.off_f);
    if (w_out) *w_out = (double*)(o.hout + o.off_wo);
    if (status) *status = (int32_t*)(o.hout + o.off_st);
    if (iters) *iters = (int32_t*)(o.hout + o.off_it);
    return DART_MPC_OK;
}

int dart_mpc_solve_bound(dart_mpc_handle* h, int B, int flags) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_PMPC) return fail(h, DART_MPC_EINVAL, "handle is not a PMPC handle");
    if (!h->io.hin) return fail(h, DART_MPC_EINVAL, "dart_mpc_bind first");
    if (B < 0 || B > h->cfg.B_max || (flags & ~3)) return fail(h, DART_MPC_EINVAL, "bad batch or flags");
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    if (int rc = settle_pending(h)) return rc;
    const bool ww = flags & DART_MPC_BOUND_W_WARM, wo = flags & DART_MPC_BOUND_W_OUT;
    if (h->srv.wanted && B <= h->srv.B) return served_request(h, B, ww, wo);
    return bound_launch(h, B, ww, wo);
}

int dart_mpc_serve_stop(dart_mpc_handle* h) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    return server_stop(h);
}

int dart_mpc_serve_running(dart_mpc_handle* h) {
    if (!h) return 0;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (!h->srv.running) return 0;
    if (hipStreamQuery(h->srv.stream) != hipErrorNotReady) h->srv.running = false;     // idle timeout: drained
    return h->srv.running ? 1 : 0;
}

int dart_mpc_sync(dart_mpc_handle* h) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = settle_pending(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize");
    return DART_MPC_OK;
}

// internal self-test of the wave primitives (not in include/dart_mpc.h): host_out[265]
int dartmpc_selftest(double* host_out) {
    double* d = nullptr;
    if (hipMalloc(&d, 265 * sizeof(double)) != hipSuccess) return DART_MPC_EHIP;
    hipError_t e = dartmpc_wave_selftest(d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(host_out, d, 265 * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

const char* dart_mpc_last_error(const dart_mpc_handle* h) { return h ? h->err.c_str() : "null handle"; }

void dart_mpc_destroy(dart_mpc_handle* h) {
    if (!h) return;
    (void)server_stop(h);                                     // the resident grid drains first
    if (h->stream) (void)hipStreamSynchronize(h->stream);    // no launch may still use the buffers below
    h->st.release();
    io_release(h);
    if (h->hdone) (void)hipHostFree(h->hdone);
    for (auto& e : h->resto)
        if (e.buf) (void)hipFree(e.buf);       // (synchronises with the area's last use)
    if (h->loop_buf) (void)hipFree(h->loop_buf);
    if (h->roll_buf) (void)hipFree(h->roll_buf);
    if (h->action_buf) (void)hipFree(h->action_buf);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// per-arm impedance QP (ARMCONTROL.solver_worker, PMPC/src/controller/arm.py:266-457)
void dart_arm_config_default(dart_arm_config* c) {
    if (!c) return;
    c->tol = 1e-10;
    c->acceptable_tol = 1e-7;
    c->max_iter = 60;
    c->reserved = 0;
}

int dart_arm_snapshot_len(int n) { return (n >= 1 && n <= DART_ARM_NMAX) ? dartmpc::arm_snap_len(n) : DART_MPC_EINVAL; }
int dart_arm_param_len(int n) { return (n >= 1 && n <= DART_ARM_NMAX) ? dartmpc::arm_prm_len(n) : DART_MPC_EINVAL; }

static int arm_args(const dart_arm_config* c, int B, int n, int prm_stride, dartmpc::ArmArgs& a) {
    if (!c || B < 0 || n < 1 || n > DART_ARM_NMAX) return DART_MPC_EINVAL;
    if (prm_stride != 0 && prm_stride != dartmpc::arm_prm_len(n)) return DART_MPC_EINVAL;
    if (!(c->tol > 0.0) || !(c->acceptable_tol >= c->tol) || c->max_iter < 1 || c->max_iter > 100000) return DART_MPC_EINVAL;
    a = dartmpc::ArmArgs{};
    a.B = B; a.n = n; a.prm_stride = prm_stride; a.max_iter = c->max_iter;
    a.tol = c->tol; a.acc_tol = c->acceptable_tol;
    return DART_MPC_OK;
}

int dart_arm_solve_batch_dev(const dart_arm_config* cfg, int B, int n, const double* snap, const double* prm,
                             int prm_stride, double* qdd, double* tau, double* loss, int32_t* status, int32_t* iters,
                             void* stream) {
    dartmpc::ArmArgs a;
    if (arm_args(cfg, B, n, prm_stride, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    if (!snap || !prm || !qdd || !tau || !loss || !status || !iters) return DART_MPC_EINVAL;
    a.snap = snap; a.prm = prm; a.qdd = qdd; a.tau = tau; a.loss = loss; a.status = status; a.iters = iters;
    return dartmpc_launch_arm(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_arm_solve_batch(const dart_arm_config* cfg, int B, int n, const double* snap, const double* prm,
                         int prm_stride, double* qdd, double* tau, double* loss, int32_t* status, int32_t* iters) {
    dartmpc::ArmArgs a;
    if (arm_args(cfg, B, n, prm_stride, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    if (!snap || !prm || !qdd || !tau || !loss || !status || !iters) return DART_MPC_EINVAL;
    const size_t SL = (size_t)dartmpc::arm_snap_len(n), PL = (size_t)dartmpc::arm_prm_len(n);
    const size_t np = prm_stride ? PL * B : PL;
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    if (S.reserve(sizeof(double) * (SL * B + np) + 2 * 256,
                  sizeof(double) * (2 * (size_t)n * B + B) + sizeof(int32_t) * 2 * B + 5 * 256) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    a.snap = S.in(snap, SL * B); a.prm = S.in(prm, np);
    a.qdd = S.out<double>((size_t)n * B); a.tau = S.out<double>((size_t)n * B); a.loss = S.out<double>(B);
    a.status = S.out<int32_t>(B); a.iters = S.out<int32_t>(B);
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess) e = dartmpc_launch_arm(&a, D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.take(qdd, a.qdd, (size_t)n * B); S.take(tau, a.tau, (size_t)n * B); S.take(loss, a.loss, B);
    S.take(status, a.status, B); S.take(iters, a.iters, B);
    return DART_MPC_OK;
}

// ---------------------------------------------------------------------------------------------
// device-resident closed-loop rollouts (loop_step.hip between the unchanged solves)
void dart_plant_config_default(dart_plant_config* c) {
    if (!c) return;
    c->tau = 0.03; c->mu_c = 0.02; c->v_c = 0.01;       // harness.TrayPlant
}

void dart_rmpc_loop_config_default(dart_rmpc_loop_config* c) {
    if (!c) return;
    c->dr_max = 0.01; c->alpha_rg = 0.5; c->step_fraction = 0.2; c->rls_lambda = 0.995; c->pos_tol = 0.01;
}

namespace {

bool any_null(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (!p) return true;
    return false;
}

dartmpc::PlantArgs plant_args(const dart_mpc_handle* h, const dart_plant_config* p) {
    dartmpc::PlantArgs a;
    a.a_lag = p->tau > 0.0 ? 1.0 - std::exp(-h->cfg.Ts / p->tau) : 1.0;
    a.mu_c = p->mu_c; a.v_c = p->v_c; a.dt = h->cfg.Ts; a.g = h->cfg.gravity;
    return a;
}

// the checks every rollout / loop-step entry shares: the call writes the log rows k .. k + steps - 1
int loop_check(dart_mpc_handle* h, int variant, const dart_plant_config* plant, int B, int k, int steps, int log_rows) {
    if (h->cfg.variant != variant)
        return fail(h, DART_MPC_EINVAL, variant == DART_MPC_RMPC   ? "handle is not an RMPC handle"
                                        : variant == DART_MPC_LMPC ? "handle is not an LMPC handle"
                                                                   : "handle is not a PMPC handle");
    if (!plant) return fail(h, DART_MPC_EINVAL, "null plant config");
    // (the LMPC plant does not use mu_c / v_c)
    if (variant != DART_MPC_LMPC && (!(plant->v_c > 0.0) || !(plant->mu_c >= 0.0)))
        return fail(h, DART_MPC_EINVAL, "plant config: v_c > 0, mu_c >= 0");
    if (B < 0 || k < 0 || steps < 0 || log_rows < 0) return fail(h, DART_MPC_EINVAL, "negative batch, step or row count");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if ((long long)k + steps > log_rows) return fail(h, DART_MPC_EINVAL, "k0 + steps exceeds log_rows");
    return DART_MPC_OK;
}

int rmpc_loop_cfg_check(dart_mpc_handle* h, const dart_rmpc_loop_config* c) {
    if (!c) return fail(h, DART_MPC_EINVAL, "null loop config");
    if (!(c->rls_lambda > 0.0) || !(c->dr_max >= 0.0) || !(c->step_fraction >= 0.0 && c->step_fraction <= 1.0))
        return fail(h, DART_MPC_EINVAL, "loop config: rls_lambda > 0, dr_max >= 0, 0 <= step_fraction <= 1");
    return DART_MPC_OK;
}

// the solve's per-step arrays of a rollout, in the handle (B_max instances)
struct LoopScratch {
    double *x0, *Rref, *phi, *y, *u0, *f;
    int32_t *status, *iters;
};

int loop_scratch(dart_mpc_handle* h, LoopScratch& L) {
    const size_t Bm = (size_t)h->cfg.B_max, N1 = (size_t)h->cfg.N + 1;
    const bool rm = h->cfg.variant == DART_MPC_RMPC;
    const size_t n_x0 = rm ? 4 : 6, n_R = rm ? 4 * N1 : 0, n_phi = rm ? 7 : 0, n_y = rm ? 2 : 0;
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    size_t off[9];
    const size_t cnt[8] = {8 * n_x0, 8 * n_R, 8 * n_phi, 8 * n_y, 8 * 2, 8, 4, 4};
    off[0] = 0;
    for (int i = 0; i < 8; ++i) off[i + 1] = off[i] + al(cnt[i] * Bm);
    // (no initialisation: pre writes what the solve reads, the solve writes what post reads)
    if (!h->loop_buf) HIPCHK(h, hipMalloc((void**)&h->loop_buf, off[8]), "hipMalloc (rollout scratch)");
    char* p = h->loop_buf;
    L.x0 = (double*)(p + off[0]); L.Rref = (double*)(p + off[1]); L.phi = (double*)(p + off[2]);
    L.y = (double*)(p + off[3]); L.u0 = (double*)(p + off[4]); L.f = (double*)(p + off[5]);
    L.status = (int32_t*)(p + off[6]); L.iters = (int32_t*)(p + off[7]);
    return DART_MPC_OK;
}

// device arena of the host rollout entries: arrays laid out 256-byte aligned, copied up / down in part
struct RollArr {
    void* host;
    size_t bytes;         // whole array
    size_t lo, n;         // the byte range that travels
    bool up, down;
    size_t off;
};

struct RollStage {
    std::vector<RollArr> arr;
    size_t total = 0;
    // whole array, both ways (state) or up only (inputs)
    int add(const void* host, size_t bytes, bool down) {
        arr.push_back({const_cast<void*>(host), bytes, 0, bytes, true, down, total});
        total += (bytes + 255) & ~size_t(255);
        return (int)arr.size() - 1;
    }
    // a log: rows [r0, r1) of `rowbytes` each travel (up only where the call may leave entries of them untouched)
    int add_log(void* host, size_t rows, size_t rowbytes, size_t r0, size_t r1, bool up) {
        arr.push_back({host, rows * rowbytes, r0 * rowbytes, (r1 - r0) * rowbytes, up, true, total});
        total += (rows * rowbytes + 255) & ~size_t(255);
        return (int)arr.size() - 1;
    }
    // an input with one row per step (LMPC's noise): rows [r0, r1) go up, nothing comes down
    int add_rows_in(const void* host, size_t rows, size_t rowbytes, size_t r0, size_t r1) {
        arr.push_back({const_cast<void*>(host), rows * rowbytes, r0 * rowbytes, (r1 - r0) * rowbytes, true, false, total});
        total += (rows * rowbytes + 255) & ~size_t(255);
        return (int)arr.size() - 1;
    }
    template <class T> T* dev(const dart_mpc_handle* h, int i) const { return reinterpret_cast<T*>(h->roll_buf + arr[i].off); }
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

}  // namespace

int dart_rmpc_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                            int B, int k, int do_post, int do_pre, int log_rows,
                            const double* target, const double* prm, const double* mu,
                            double* x, double* tilt, double* prev, double* u_prev, double* r_v, const double* theta,
                            int32_t* done, int32_t* nlog,
                            double* x0, double* Rref, double* phi, double* y,
                            const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                            double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                            double* log_x, double* log_theta, double* log_r_v, double* log_f,
                            int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_RMPC, plant, B, k, do_post ? 1 : 0, log_rows)) return rc;
    if (int rc = rmpc_loop_cfg_check(h, loop)) return rc;
    if (any_null({target, prm, mu, x, tilt, prev, u_prev, r_v, theta, done, nlog, x0, Rref, phi, y, u0, f, status, iters,
                  log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep, log_x, log_theta, log_r_v, log_f, log_status,
                  log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || (!do_post && !do_pre)) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::RmpcLoopArgs a;
    a.B = B; a.N = h->cfg.N; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
    a.plant = plant_args(h, plant);
    a.Ts = h->cfg.Ts; a.dr_max = loop->dr_max; a.alpha_rg = loop->alpha_rg; a.step_fraction = loop->step_fraction;
    a.pos_tol = loop->pos_tol;
    a.target = target; a.prm = prm; a.mu = mu;
    a.x = x; a.tilt = tilt; a.prev = prev; a.u_prev = u_prev; a.r_v = r_v; a.theta = theta; a.done = done; a.nlog = nlog;
    a.x0 = x0; a.Rref = Rref; a.phi = phi; a.y = y; a.u0 = u0; a.f = f; a.status = status; a.iters = iters;
    a.log_pos_err = log_pos_err; a.log_pos_err_norm = log_pos_err_norm; a.log_u_cmd = log_u_cmd;
    a.log_timestep = log_timestep; a.log_x = log_x; a.log_theta = log_theta; a.log_r_v = log_r_v; a.log_f = log_f;
    a.log_status = log_status; a.log_iters = log_iters;
    HIPCHK(h, dartmpc_launch_rmpc_loop(&a, stream ? (hipStream_t)stream : h->stream), "loop-step kernel launch");
    return DART_MPC_OK;
}

int dart_pmpc_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                            int B, int k, int do_post, int do_pre, int log_rows, const double* prm,
                            double* x, double* tilt, double* x0,
                            const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                            double* log_X, double* log_U, double* log_quat, double* log_loss,
                            int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_PMPC, plant, B, k, do_post ? 1 : 0, log_rows)) return rc;
    if (any_null({prm, x, tilt, x0, u0, f, status, iters, log_X, log_U, log_quat, log_loss, log_status, log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || (!do_post && !do_pre)) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::PmpcLoopArgs a;
    a.B = B; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
    a.plant = plant_args(h, plant);
    a.prm = prm; a.x = x; a.tilt = tilt; a.x0 = x0; a.u0 = u0; a.f = f; a.status = status; a.iters = iters;
    a.log_X = log_X; a.log_U = log_U; a.log_quat = log_quat; a.log_loss = log_loss; a.log_status = log_status;
    a.log_iters = log_iters;
    HIPCHK(h, dartmpc_launch_pmpc_loop(&a, stream ? (hipStream_t)stream : h->stream), "loop-step kernel launch");
    return DART_MPC_OK;
}

int dart_rmpc_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                          int B, int k0, int steps, int log_rows,
                          const double* target, const double* prm, const double* mu,
                          double* x, double* tilt, double* prev, double* u_prev, double* r_v, double* theta,
                          double* P, double* w, int32_t* done, int32_t* nlog,
                          double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                          double* log_x, double* log_theta, double* log_r_v, double* log_f,
                          int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_RMPC, plant, B, k0, steps, log_rows)) return rc;
    if (int rc = rmpc_loop_cfg_check(h, loop)) return rc;
    if (any_null({target, prm, mu, x, tilt, prev, u_prev, r_v, theta, P, w, done, nlog, log_pos_err, log_pos_err_norm,
                  log_u_cmd, log_timestep, log_x, log_theta, log_r_v, log_f, log_status, log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    LoopScratch L;
    if (int rc = loop_scratch(h, L)) return rc;
    void* s = stream ? stream : (void*)h->stream;
    auto step = [&](int k, int post, int pre) {
        return dart_rmpc_loop_step_dev(h, plant, loop, B, k, post, pre, log_rows, target, prm, mu, x, tilt, prev, u_prev,
                                       r_v, theta, done, nlog, L.x0, L.Rref, L.phi, L.y, L.u0, L.f, L.status, L.iters,
                                       log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep, log_x, log_theta, log_r_v,
                                       log_f, log_status, log_iters, s);
    };
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        // warm start in place: every element of w's row is read (at the solve's start) and written (at its end)
        // by the same wave, and an instance handed to the restoration kernel has not written its row
        if (int rc = dart_rmpc_solve_batch_dev(h, B, L.x0, u_prev, theta, P, L.phi, L.y, loop->rls_lambda, L.Rref, prm, w,
                                               L.u0, L.f, w, L.status, L.iters, s))
            return rc;
        if (int rc = step(k0 + j, 1, j + 1 < steps)) return rc;
    }
    return DART_MPC_OK;
}

int dart_pmpc_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                          int B, int k0, int steps, int log_rows, const double* target, const double* prm,
                          double* x, double* tilt,
                          double* log_X, double* log_U, double* log_quat, double* log_loss,
                          int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_PMPC, plant, B, k0, steps, log_rows)) return rc;
    if (any_null({target, prm, x, tilt, log_X, log_U, log_quat, log_loss, log_status, log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    LoopScratch L;
    if (int rc = loop_scratch(h, L)) return rc;
    void* s = stream ? stream : (void*)h->stream;
    auto step = [&](int k, int post, int pre) {
        return dart_pmpc_loop_step_dev(h, plant, B, k, post, pre, log_rows, prm, x, tilt, L.x0, L.u0, L.f, L.status, L.iters,
                                       log_X, log_U, log_quat, log_loss, log_status, log_iters, s);
    };
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        if (int rc = dart_mpc_solve_batch_dev(h, B, L.x0, target, prm, nullptr, L.u0, L.f, nullptr, L.status, L.iters, s))
            return rc;
        if (int rc = step(k0 + j, 1, j + 1 < steps)) return rc;
    }
    return DART_MPC_OK;
}

int dart_rmpc_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                      int B, int k0, int steps, int log_rows,
                      const double* target, const double* prm, const double* mu,
                      double* x, double* tilt, double* prev, double* u_prev, double* r_v, double* theta,
                      double* P, double* w, int32_t* done, int32_t* nlog,
                      double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                      double* log_x, double* log_theta, double* log_r_v, double* log_f,
                      int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_RMPC, plant, B, k0, steps, log_rows)) return rc;
    if (int rc = rmpc_loop_cfg_check(h, loop)) return rc;
    if (any_null({target, prm, mu, x, tilt, prev, u_prev, r_v, theta, P, w, done, nlog, log_pos_err, log_pos_err_norm,
                  log_u_cmd, log_timestep, log_x, log_theta, log_r_v, log_f, log_status, log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nB = (size_t)B, D = sizeof(double), I = sizeof(int32_t), nw = (size_t)dart_rmpc_nw(h->cfg.N);
    // episode rows: an instance writes rows nlog[b] .. nlog[b] + steps - 1 at most
    int e0 = log_rows, e1 = 0;
    for (int b = 0; b < B; ++b) {
        if (nlog[b] < 0) return fail(h, DART_MPC_EINVAL, "negative nlog");
        e0 = nlog[b] < e0 ? nlog[b] : e0;
        e1 = nlog[b] > e1 ? nlog[b] : e1;
    }
    e1 = (long long)e1 + steps < log_rows ? e1 + steps : log_rows;
    e0 = e0 < e1 ? e0 : e1;
    const size_t R = (size_t)log_rows, r0 = (size_t)k0, r1 = (size_t)k0 + steps;
    RollStage S;
    const int i_tg = S.add(target, 4 * nB * D, false), i_prm = S.add(prm, 10 * nB * D, false), i_mu = S.add(mu, nB * D, false);
    const int i_x = S.add(x, 6 * nB * D, true), i_tilt = S.add(tilt, 2 * nB * D, true), i_prev = S.add(prev, 4 * nB * D, true);
    const int i_up = S.add(u_prev, 2 * nB * D, true), i_rv = S.add(r_v, 4 * nB * D, true), i_th = S.add(theta, 14 * nB * D, true);
    const int i_P = S.add(P, 98 * nB * D, true), i_w = S.add(w, nw * nB * D, true);
    const int i_done = S.add(done, nB * I, true), i_nlog = S.add(nlog, nB * I, true);
    const int l_pe = S.add_log(log_pos_err, R, 2 * nB * D, e0, e1, true), l_pn = S.add_log(log_pos_err_norm, R, nB * D, e0, e1, true);
    const int l_uc = S.add_log(log_u_cmd, R, 2 * nB * D, e0, e1, true), l_ts = S.add_log(log_timestep, R, nB * D, e0, e1, true);
    const int l_x = S.add_log(log_x, R, 4 * nB * D, r0, r1, false), l_th = S.add_log(log_theta, R, 14 * nB * D, r0, r1, false);
    const int l_rv = S.add_log(log_r_v, R, 4 * nB * D, r0, r1, false), l_f = S.add_log(log_f, R, nB * D, r0, r1, false);
    const int l_st = S.add_log(log_status, R, nB * I, r0, r1, false), l_it = S.add_log(log_iters, R, nB * I, r0, r1, false);
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    if (int rc = dart_rmpc_rollout_dev(
            h, plant, loop, B, k0, steps, log_rows, S.dev<double>(h, i_tg), S.dev<double>(h, i_prm), S.dev<double>(h, i_mu),
            S.dev<double>(h, i_x), S.dev<double>(h, i_tilt), S.dev<double>(h, i_prev), S.dev<double>(h, i_up),
            S.dev<double>(h, i_rv), S.dev<double>(h, i_th), S.dev<double>(h, i_P), S.dev<double>(h, i_w),
            S.dev<int32_t>(h, i_done), S.dev<int32_t>(h, i_nlog), S.dev<double>(h, l_pe), S.dev<double>(h, l_pn),
            S.dev<double>(h, l_uc), S.dev<double>(h, l_ts), S.dev<double>(h, l_x), S.dev<double>(h, l_th),
            S.dev<double>(h, l_rv), S.dev<double>(h, l_f), S.dev<int32_t>(h, l_st), S.dev<int32_t>(h, l_it), s))
        return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

int dart_pmpc_rollout(dart_mpc_handle* h, const dart_plant_config* plant,
                      int B, int k0, int steps, int log_rows, const double* target, const double* prm,
                      double* x, double* tilt,
                      double* log_X, double* log_U, double* log_quat, double* log_loss,
                      int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_PMPC, plant, B, k0, steps, log_rows)) return rc;
    if (any_null({target, prm, x, tilt, log_X, log_U, log_quat, log_loss, log_status, log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    if (int rc = settle_pending(h)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nB = (size_t)B, D = sizeof(double), I = sizeof(int32_t);
    const size_t R = (size_t)log_rows, r0 = (size_t)k0, r1 = (size_t)k0 + steps;
    RollStage S;
    const int i_tg = S.add(target, 6 * nB * D, false), i_prm = S.add(prm, 6 * nB * D, false);
    const int i_x = S.add(x, 6 * nB * D, true), i_tilt = S.add(tilt, 2 * nB * D, true);
    const int l_X = S.add_log(log_X, R, 6 * nB * D, r0, r1, false), l_U = S.add_log(log_U, R, 2 * nB * D, r0, r1, false);
    const int l_Q = S.add_log(log_quat, R, 4 * nB * D, r0, r1, false), l_L = S.add_log(log_loss, R, nB * D, r0, r1, false);
    const int l_st = S.add_log(log_status, R, nB * I, r0, r1, false), l_it = S.add_log(log_iters, R, nB * I, r0, r1, false);
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    if (int rc = dart_pmpc_rollout_dev(h, plant, B, k0, steps, log_rows, S.dev<double>(h, i_tg), S.dev<double>(h, i_prm),
                                       S.dev<double>(h, i_x), S.dev<double>(h, i_tilt), S.dev<double>(h, l_X),
                                       S.dev<double>(h, l_U), S.dev<double>(h, l_Q), S.dev<double>(h, l_L),
                                       S.dev<int32_t>(h, l_st), S.dev<int32_t>(h, l_it), s))
        return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

// ---------------------------------------------------------------------------------------------
// LMPC closed loop (lmpc_loop_kernel between the unchanged policy + solve launches)
namespace {

// the solve's per-step arrays of an LMPC rollout, the two warm-start buffers the solves alternate between, and
// one zeroed noise row, in the handle (B_max instances)
struct LmpcLoopScratch {
    double *state, *u0, *f, *wbuf[2];
    int32_t *status, *iters;
    float* zero_noise;
};

int lmpc_loop_scratch(dart_mpc_handle* h, LmpcLoopScratch& L) {
    const size_t Bm = (size_t)h->cfg.B_max, nw = (size_t)dart_lmpc_nw(h->cfg.N);
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    const size_t cnt[8] = {8 * 8, 8 * 2, 8, 8 * nw, 8 * nw, 4, 4, 4 * 34};
    size_t off[9];
    off[0] = 0;
    for (int i = 0; i < 8; ++i) off[i + 1] = off[i] + al(cnt[i] * Bm);
    if (!h->loop_buf) {
        HIPCHK(h, hipMalloc((void**)&h->loop_buf, off[8]), "hipMalloc (rollout scratch)");
        // (only the noise row needs a value: pre writes what the solve reads, the solve what post reads)
        const hipError_t e = hipMemset(h->loop_buf + off[7], 0, off[8] - off[7]);
        if (e != hipSuccess) {
            (void)hipFree(h->loop_buf);
            h->loop_buf = nullptr;
            return fail(h, DART_MPC_EHIP, "hipMemset (rollout scratch)", e);
        }
    }
    char* p = h->loop_buf;
    L.state = (double*)(p + off[0]); L.u0 = (double*)(p + off[1]); L.f = (double*)(p + off[2]);
    L.wbuf[0] = (double*)(p + off[3]); L.wbuf[1] = (double*)(p + off[4]);
    L.status = (int32_t*)(p + off[5]); L.iters = (int32_t*)(p + off[6]); L.zero_noise = (float*)(p + off[7]);
    return DART_MPC_OK;
}

// the argument checks the three LMPC rollout entries share (after loop_check)
int lmpc_rollout_check(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, int B, const float* weights,
                       std::initializer_list<const void*> always, std::initializer_list<const void*> with_policy) {
    if (any_null(always)) return fail(h, DART_MPC_EINVAL, "null pointer");
    if (weights) {
        dartmpc::PolicyArgs chk;
        if (policy_args(pcfg, B, weights, chk) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
        if (any_null(with_policy)) return fail(h, DART_MPC_EINVAL, "null pointer (policy state)");
    }
    return DART_MPC_OK;
}

}  // namespace

int dart_lmpc_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                            int B, int k, int do_post, int do_pre, int log_rows,
                            const double* target, const double* plant_pvec,
                            double* x, double* tilt, double* u_prev, const double* model_params, double* state,
                            const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                            double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                            int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_LMPC, plant, B, k, do_post ? 1 : 0, log_rows)) return rc;
    if (any_null({target, plant_pvec, x, tilt, u_prev, model_params, state, u0, f, status, iters, log_X, log_U,
                  log_pos_error, log_pvec, log_loss, log_status, log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || (!do_post && !do_pre)) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::LmpcLoopArgs a;
    a.B = B; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
    a.a_lag = plant->tau > 0.0 ? 1.0 - std::exp(-h->cfg.Ts / plant->tau) : 1.0;
    a.Ts = h->cfg.Ts;
    a.target = target; a.plant_pvec = plant_pvec; a.x = x; a.tilt = tilt; a.u_prev = u_prev;
    a.model_params = model_params; a.state = state; a.u0 = u0; a.f = f; a.status = status; a.iters = iters;
    a.log_X = log_X; a.log_U = log_U; a.log_pos_error = log_pos_error; a.log_pvec = log_pvec; a.log_loss = log_loss;
    a.log_status = log_status; a.log_iters = log_iters;
    HIPCHK(h, dartmpc_launch_lmpc_loop(&a, stream ? (hipStream_t)stream : h->stream), "loop-step kernel launch");
    return DART_MPC_OK;
}

int dart_lmpc_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                          int B, int k0, int steps, int log_rows,
                          const double* target, const double* prm, const double* plant_pvec, const double* current_k,
                          const float* weights, const float* noise,
                          double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                          int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                          double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                          int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_LMPC, plant, B, k0, steps, log_rows)) return rc;
    if (int rc = lmpc_rollout_check(h, pcfg, B, weights,
                                    {target, prm, plant_pvec, x, tilt, u_prev, w, model_params, log_X, log_U,
                                     log_pos_error, log_pvec, log_loss, log_status, log_iters},
                                    {current_k, obs_mean, obs_M2, obs_count, history, timestep}))
        return rc;
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    LmpcLoopScratch L;
    if (int rc = lmpc_loop_scratch(h, L)) return rc;
    void* s = stream ? stream : (void*)h->stream;
    auto step = [&](int k, int post, int pre) {
        return dart_lmpc_loop_step_dev(h, plant, B, k, post, pre, log_rows, target, plant_pvec, x, tilt, u_prev,
                                       model_params, L.state, L.u0, L.f, L.status, L.iters, log_X, log_U, log_pos_error,
                                       log_pvec, log_loss, log_status, log_iters, s);
    };
    // Warm start: with the restoration phases on, an instance that <false> hands over has written the iterate of
    // its failed iteration to w_out before lmpc_solve<true> (the tail, or the second launch) redoes the set-up from
    // w_warm, so w_warm == w_out would change the scalings of the resumed solve.  The solves
    // alternate between two handle-owned buffers instead: the first reads the caller's w, the last writes it.
    // Without the restoration phases nothing is handed over and the row is rewritten in place.
    const bool in_place = !h->cfg.restoration;
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        const double* w_in = (in_place || j == 0) ? w : L.wbuf[(j - 1) & 1];
        double* w_out = (in_place || (j == steps - 1 && j > 0)) ? w : L.wbuf[j & 1];
        int rc;
        if (weights)
            rc = dart_lmpc_policy_solve_batch_dev(h, pcfg, B, weights, L.state, u_prev, target, current_k, obs_mean, obs_M2,
                                                  obs_count, history, timestep,
                                                  noise ? noise + ((size_t)k0 + j) * B * 34 : L.zero_noise, model_params,
                                                  nullptr, prm, w_in, L.u0, L.f, w_out, L.status, L.iters, s);
        else
            rc = dart_lmpc_solve_batch_dev(h, B, L.state, u_prev, model_params, target, prm, w_in, L.u0, L.f, w_out,
                                           L.status, L.iters, s);
        if (rc) return rc;
        if (w_out != w && j == steps - 1)       // a one-step call: the iterate back into the caller's w
            HIPCHK(h, hipMemcpyAsync(w, w_out, sizeof(double) * (size_t)dart_lmpc_nw(h->cfg.N) * B,
                                     hipMemcpyDeviceToDevice, (hipStream_t)s), "copy w");
        if ((rc = step(k0 + j, 1, j + 1 < steps))) return rc;
    }
    return DART_MPC_OK;
}

int dart_lmpc_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                      int B, int k0, int steps, int log_rows,
                      const double* target, const double* prm, const double* plant_pvec, const double* current_k,
                      const float* weights, const float* noise,
                      double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                      int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                      double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                      int32_t* log_status, int32_t* log_iters, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_LMPC, plant, B, k0, steps, log_rows)) return rc;
    if (int rc = lmpc_rollout_check(h, pcfg, B, weights,
                                    {target, prm, plant_pvec, x, tilt, u_prev, w, model_params, log_X, log_U,
                                     log_pos_error, log_pvec, log_loss, log_status, log_iters},
                                    {current_k, obs_mean, obs_M2, obs_count, history, timestep}))
        return rc;
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nB = (size_t)B, D = sizeof(double), I = sizeof(int32_t), F = sizeof(float);
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N);
    const size_t R = (size_t)log_rows, r0 = (size_t)k0, r1 = (size_t)k0 + steps;
    RollStage S;
    const int i_tg = S.add(target, 8 * nB * D, false), i_prm = S.add(prm, dartmpc::LM_NPRM * nB * D, false);
    const int i_pp = S.add(plant_pvec, 34 * nB * D, false);
    const int i_x = S.add(x, 8 * nB * D, true), i_tilt = S.add(tilt, 2 * nB * D, true), i_up = S.add(u_prev, 2 * nB * D, true);
    const int i_w = S.add(w, nw * nB * D, true), i_mp = S.add(model_params, 34 * nB * D, true);
    int i_ck = -1, i_wt = -1, i_nz = -1, i_om = -1, i_o2 = -1, i_oc = -1, i_hi = -1, i_ts = -1;
    if (weights) {
        i_ck = S.add(current_k, 34 * nB * D, false);
        i_wt = S.add(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS * F, false);
        if (noise) i_nz = S.add_rows_in(noise, R, 34 * nB * F, r0, r1);
        i_om = S.add(obs_mean, 52 * nB * D, true); i_o2 = S.add(obs_M2, 52 * nB * D, true);
        i_oc = S.add(obs_count, nB * I, true); i_hi = S.add(history, 520 * nB * F, true);
        i_ts = S.add(timestep, nB * I, true);
    }
    const int l_X = S.add_log(log_X, R, 8 * nB * D, r0, r1, false), l_U = S.add_log(log_U, R, 2 * nB * D, r0, r1, false);
    const int l_pe = S.add_log(log_pos_error, R, nB * D, r0, r1, false), l_pv = S.add_log(log_pvec, R, 34 * nB * D, r0, r1, false);
    const int l_L = S.add_log(log_loss, R, nB * D, r0, r1, false);
    const int l_st = S.add_log(log_status, R, nB * I, r0, r1, false), l_it = S.add_log(log_iters, R, nB * I, r0, r1, false);
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    auto dd = [&](int i) { return i < 0 ? nullptr : S.dev<double>(h, i); };
    auto di = [&](int i) { return i < 0 ? nullptr : S.dev<int32_t>(h, i); };
    auto df = [&](int i) { return i < 0 ? nullptr : S.dev<float>(h, i); };
    if (int rc = dart_lmpc_rollout_dev(h, plant, pcfg, B, k0, steps, log_rows, dd(i_tg), dd(i_prm), dd(i_pp), dd(i_ck),
                                       df(i_wt), df(i_nz), dd(i_x), dd(i_tilt), dd(i_up), dd(i_w), dd(i_om), dd(i_o2),
                                       di(i_oc), df(i_hi), di(i_ts), dd(i_mp), dd(l_X), dd(l_U), dd(l_pe), dd(l_pv),
                                       dd(l_L), di(l_st), di(l_it), s))
        return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

// ---------------------------------------------------------------------------------------------
// LMPC experience collection (lmpc_experience.hip after every post of the LMPC closed loop)
void dart_lmpc_reward_config_default(dart_lmpc_reward_config* c) {
    if (!c) return;
    c->sigma_pos = 0.02; c->sigma_vel = 0.02;
    c->w_pos = 40.0; c->w_vel = 0.1; c->w_change = 1e-3; c->w_d_ctrl = 5.0;
    c->success_tol = 0.01; c->success_bonus = 20.0; c->oob_penalty = 20.0;
    c->tray_limit[0] = 0.2; c->tray_limit[1] = 0.15;
    c->max_per_dim_rms = 0.5; c->time_penalty_rate = 1e-4;
    c->max_episode_steps = 20000; c->record_every = 8; c->done_sticky = 0; c->reserved = 0;
}

namespace {

// the configuration half of the experience launch's arguments, checked (after loop_check)
int experience_cfg(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, const dart_lmpc_reward_config* r, int B,
                   int rec_rows, int reset_rows, const float* weights, const float* critic,
                   dartmpc::ExperienceArgs& a) {
    if (!weights) return fail(h, DART_MPC_EINVAL, "experience collection needs a policy (null weights)");
    if (!critic) return fail(h, DART_MPC_EINVAL, "null critic weights");
    // (the experience kernel reads layer 1 of both nets with 16-byte loads)
    if ((reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(critic)) & 15)
        return fail(h, DART_MPC_EINVAL, "policy and critic weights must be 16-byte aligned");
    dartmpc::PolicyArgs pa;
    if (policy_args(pcfg, B, weights, pa) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
    if (!r) return fail(h, DART_MPC_EINVAL, "null reward config");
    if (r->record_every < 1 || !(r->sigma_pos > 0.0) || !(r->sigma_vel > 0.0))
        return fail(h, DART_MPC_EINVAL, "reward config: record_every >= 1, sigma_pos > 0, sigma_vel > 0");
    if (rec_rows < 0 || reset_rows < 0) return fail(h, DART_MPC_EINVAL, "negative rec_rows or reset_rows");
    a.B = B; a.rec_rows = rec_rows; a.reset_rows = reset_rows;
    a.w = pa.w;
    a.c.V1 = critic; a.c.c1 = critic + 520 * 64; a.c.V2 = a.c.c1 + 64; a.c.c2 = a.c.V2 + 64 * 64;
    a.c.V3 = a.c.c2 + 64; a.c.c3 = a.c.V3 + 64;
    a.r.sigma_pos = r->sigma_pos; a.r.sigma_vel = r->sigma_vel; a.r.w_pos = r->w_pos; a.r.w_vel = r->w_vel;
    a.r.w_change = r->w_change; a.r.w_d_ctrl = r->w_d_ctrl; a.r.success_tol = r->success_tol;
    a.r.success_bonus = r->success_bonus; a.r.oob_penalty = r->oob_penalty;
    a.r.tray_limit[0] = r->tray_limit[0]; a.r.tray_limit[1] = r->tray_limit[1];
    a.r.max_per_dim_rms = r->max_per_dim_rms; a.r.time_penalty_rate = r->time_penalty_rate;
    a.r.max_episode_steps = r->max_episode_steps; a.r.record_every = r->record_every; a.r.done_sticky = r->done_sticky;
    a.max_delta = pcfg->max_delta; a.action_scale = pcfg->action_scale;
    a.log_std_min = pcfg->log_std_min; a.log_std_max = pcfg->log_std_max;
    return DART_MPC_OK;
}

}  // namespace

#define DART_COLLECT_STATE_PARAMS                                                                                     \
    double *prev_cmd, double *control_seen, int32_t *ep_step, double *ep_return, double *time_penalty,               \
        int32_t *episodes, double *last_return, int32_t *last_steps, int32_t *nrec, int32_t *sticky,                 \
        const double *reset_x, const double *reset_target, const double *reset_pvec
#define DART_COLLECT_OUT_PARAMS                                                                                       \
    double *log_reward, int32_t *log_done, float *log_value, float *log_logp, float *rec_obs, float *rec_action,     \
        float *rec_logp, float *rec_value, double *rec_reward, float *rec_done
// (after experience_cfg) the pointer half: null checks, then the fields of `a`
#define DART_COLLECT_FILL(a)                                                                                          \
    do {                                                                                                              \
        if (any_null({prev_cmd, control_seen, ep_step, ep_return, time_penalty, episodes, last_return, last_steps,   \
                      nrec, sticky, log_reward, log_done, log_value, log_logp}))                                      \
            return fail(h, DART_MPC_EINVAL, "null pointer (collection state or logs)");                              \
        if (rec_rows > 0 && any_null({rec_obs, rec_action, rec_logp, rec_value, rec_reward, rec_done}))              \
            return fail(h, DART_MPC_EINVAL, "null pointer (records)");                                               \
        if (reset_rows > 0 && any_null({reset_x, reset_target, reset_pvec}))                                         \
            return fail(h, DART_MPC_EINVAL, "reset_rows > 0 with a null reset pool");                                \
        (a).prev_cmd = prev_cmd; (a).control_seen = control_seen; (a).ep_step = ep_step; (a).ep_return = ep_return;  \
        (a).time_penalty = time_penalty; (a).episodes = episodes; (a).last_return = last_return;                     \
        (a).last_steps = last_steps; (a).nrec = nrec; (a).sticky = sticky;                                           \
        (a).reset_x = reset_x; (a).reset_target = reset_target; (a).reset_pvec = reset_pvec;                         \
        (a).log_reward = log_reward; (a).log_done = log_done; (a).log_value = log_value; (a).log_logp = log_logp;    \
        (a).rec_obs = rec_obs; (a).rec_action = rec_action; (a).rec_logp = rec_logp; (a).rec_value = rec_value;      \
        (a).rec_reward = rec_reward; (a).rec_done = rec_done;                                                        \
    } while (0)

int dart_lmpc_experience_step_dev(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg,
                                  const dart_lmpc_reward_config* rcfg, int B, int k, int log_rows, int rec_rows,
                                  int reset_rows, const float* weights, const float* critic, const float* history,
                                  const float* action, const double* log_X, const int32_t* timestep,
                                  const double* u_prev, double* target, double* plant_pvec, double* x, double* tilt,
                                  double* state, DART_COLLECT_STATE_PARAMS, DART_COLLECT_OUT_PARAMS, float* mean_out,
                                  void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, "handle is not an LMPC handle");
    if (B < 0 || k < 0 || log_rows < 0) return fail(h, DART_MPC_EINVAL, "negative batch, step or row count");
    if (k >= log_rows) return fail(h, DART_MPC_EINVAL, "k exceeds log_rows");
    dartmpc::ExperienceArgs a;
    if (int rc = experience_cfg(h, pcfg, rcfg, B, rec_rows, reset_rows, weights, critic, a)) return rc;
    if (any_null({history, action, log_X, timestep, u_prev, target, plant_pvec, x, tilt}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    DART_COLLECT_FILL(a);
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    a.k = k;
    a.history = history; a.action = action; a.log_X = log_X; a.timestep = timestep; a.u_prev = u_prev;
    a.target = target; a.plant_pvec = plant_pvec; a.x = x; a.tilt = tilt; a.state = state; a.mean_out = mean_out;
    HIPCHK(h, dartmpc_launch_lmpc_experience(&a, stream ? (hipStream_t)stream : h->stream), "experience kernel launch");
    return DART_MPC_OK;
}

int dart_lmpc_collect_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                          const dart_lmpc_reward_config* rcfg, int B, int k0, int steps, int log_rows, int rec_rows,
                          int reset_rows, double* target, const double* prm, double* plant_pvec,
                          const double* current_k, const float* weights, const float* critic, const float* noise,
                          double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                          int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                          DART_COLLECT_STATE_PARAMS, double* log_X, double* log_U, double* log_pos_error,
                          double* log_pvec, double* log_loss, int32_t* log_status, int32_t* log_iters,
                          DART_COLLECT_OUT_PARAMS, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_LMPC, plant, B, k0, steps, log_rows)) return rc;
    dartmpc::ExperienceArgs ea;
    if (int rc = experience_cfg(h, pcfg, rcfg, B, rec_rows, reset_rows, weights, critic, ea)) return rc;
    if (int rc = lmpc_rollout_check(h, pcfg, B, weights,
                                    {target, prm, plant_pvec, x, tilt, u_prev, w, model_params, log_X, log_U,
                                     log_pos_error, log_pvec, log_loss, log_status, log_iters},
                                    {current_k, obs_mean, obs_M2, obs_count, history, timestep}))
        return rc;
    DART_COLLECT_FILL(ea);
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    LmpcLoopScratch L;
    if (int rc = lmpc_loop_scratch(h, L)) return rc;
    if (!h->action_buf)
        HIPCHK(h, hipMalloc((void**)&h->action_buf, sizeof(float) * 34 * (size_t)h->cfg.B_max), "hipMalloc (action buffer)");
    void* s = stream ? stream : (void*)h->stream;
    auto step = [&](int k, int post, int pre) {
        return dart_lmpc_loop_step_dev(h, plant, B, k, post, pre, log_rows, target, plant_pvec, x, tilt, u_prev,
                                       model_params, L.state, L.u0, L.f, L.status, L.iters, log_X, log_U, log_pos_error,
                                       log_pvec, log_loss, log_status, log_iters, s);
    };
    ea.history = history; ea.action = h->action_buf; ea.log_X = log_X; ea.timestep = timestep; ea.u_prev = u_prev;
    ea.target = target; ea.plant_pvec = plant_pvec; ea.x = x; ea.tilt = tilt; ea.mean_out = nullptr;
    // the launch sequence and the warm-start ping-pong of dart_lmpc_rollout_dev, with the policy's action kept and
    // one experience launch after every post; a reset at the last step of a call is picked up by the next call's pre
    const bool in_place = !h->cfg.restoration;
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        const double* w_in = (in_place || j == 0) ? w : L.wbuf[(j - 1) & 1];
        double* w_out = (in_place || (j == steps - 1 && j > 0)) ? w : L.wbuf[j & 1];
        int rc = dart_lmpc_policy_solve_batch_dev(h, pcfg, B, weights, L.state, u_prev, target, current_k, obs_mean,
                                                  obs_M2, obs_count, history, timestep,
                                                  noise ? noise + ((size_t)k0 + j) * B * 34 : L.zero_noise, model_params,
                                                  h->action_buf, prm, w_in, L.u0, L.f, w_out, L.status, L.iters, s);
        if (rc) return rc;
        if (w_out != w && j == steps - 1)       // a one-step call: the iterate back into the caller's w
            HIPCHK(h, hipMemcpyAsync(w, w_out, sizeof(double) * (size_t)dart_lmpc_nw(h->cfg.N) * B,
                                     hipMemcpyDeviceToDevice, (hipStream_t)s), "copy w");
        const int pre = j + 1 < steps;
        if ((rc = step(k0 + j, 1, pre))) return rc;
        ea.k = k0 + j;
        ea.state = pre ? L.state : nullptr;
        HIPCHK(h, dartmpc_launch_lmpc_experience(&ea, (hipStream_t)s), "experience kernel launch");
    }
    return DART_MPC_OK;
}

int dart_lmpc_collect(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                      const dart_lmpc_reward_config* rcfg, int B, int k0, int steps, int log_rows, int rec_rows,
                      int reset_rows, double* target, const double* prm, double* plant_pvec, const double* current_k,
                      const float* weights, const float* critic, const float* noise,
                      double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                      int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                      DART_COLLECT_STATE_PARAMS, double* log_X, double* log_U, double* log_pos_error,
                      double* log_pvec, double* log_loss, int32_t* log_status, int32_t* log_iters,
                      DART_COLLECT_OUT_PARAMS, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = loop_check(h, DART_MPC_LMPC, plant, B, k0, steps, log_rows)) return rc;
    {
        dartmpc::ExperienceArgs chk;
        if (int rc = experience_cfg(h, pcfg, rcfg, B, rec_rows, reset_rows, weights, critic, chk)) return rc;
        if (int rc = lmpc_rollout_check(h, pcfg, B, weights,
                                        {target, prm, plant_pvec, x, tilt, u_prev, w, model_params, log_X, log_U,
                                         log_pos_error, log_pvec, log_loss, log_status, log_iters},
                                        {current_k, obs_mean, obs_M2, obs_count, history, timestep}))
            return rc;
        DART_COLLECT_FILL(chk);
    }
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nB = (size_t)B, D = sizeof(double), I = sizeof(int32_t), F = sizeof(float);
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N);
    const size_t R = (size_t)log_rows, r0 = (size_t)k0, r1 = (size_t)k0 + steps;
    const size_t RR = (size_t)rec_rows, RS = (size_t)reset_rows;
    RollStage S;
    const int i_tg = S.add(target, 8 * nB * D, true), i_prm = S.add(prm, dartmpc::LM_NPRM * nB * D, false);
    const int i_pp = S.add(plant_pvec, 34 * nB * D, true);
    const int i_x = S.add(x, 8 * nB * D, true), i_tilt = S.add(tilt, 2 * nB * D, true), i_up = S.add(u_prev, 2 * nB * D, true);
    const int i_w = S.add(w, nw * nB * D, true), i_mp = S.add(model_params, 34 * nB * D, true);
    const int i_ck = S.add(current_k, 34 * nB * D, false);
    const int i_wt = S.add(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS * F, false);
    const int i_cr = S.add(critic, (size_t)DART_LMPC_CRITIC_NWEIGHTS * F, false);
    const int i_nz = noise ? S.add_rows_in(noise, R, 34 * nB * F, r0, r1) : -1;
    const int i_om = S.add(obs_mean, 52 * nB * D, true), i_o2 = S.add(obs_M2, 52 * nB * D, true);
    const int i_oc = S.add(obs_count, nB * I, true), i_hi = S.add(history, 520 * nB * F, true);
    const int i_ts = S.add(timestep, nB * I, true);
    const int c_pc = S.add(prev_cmd, 2 * nB * D, true), c_cs = S.add(control_seen, 2 * nB * D, true);
    const int c_es = S.add(ep_step, nB * I, true), c_er = S.add(ep_return, nB * D, true);
    const int c_tp = S.add(time_penalty, nB * D, true), c_ep = S.add(episodes, nB * I, true);
    const int c_lr = S.add(last_return, nB * D, true), c_ls = S.add(last_steps, nB * I, true);
    const int c_nr = S.add(nrec, nB * I, true), c_sk = S.add(sticky, nB * I, true);
    int p_x = -1, p_t = -1, p_p = -1;
    if (reset_rows > 0) {
        p_x = S.add(reset_x, RS * 8 * nB * D, false); p_t = S.add(reset_target, RS * 8 * nB * D, false);
        p_p = S.add(reset_pvec, RS * 34 * nB * D, false);
    }
    const int l_X = S.add_log(log_X, R, 8 * nB * D, r0, r1, false), l_U = S.add_log(log_U, R, 2 * nB * D, r0, r1, false);
    const int l_pe = S.add_log(log_pos_error, R, nB * D, r0, r1, false), l_pv = S.add_log(log_pvec, R, 34 * nB * D, r0, r1, false);
    const int l_L = S.add_log(log_loss, R, nB * D, r0, r1, false);
    const int l_st = S.add_log(log_status, R, nB * I, r0, r1, false), l_it = S.add_log(log_iters, R, nB * I, r0, r1, false);
    const int l_rw = S.add_log(log_reward, R, nB * D, r0, r1, false), l_dn = S.add_log(log_done, R, nB * I, r0, r1, false);
    const int l_vl = S.add_log(log_value, R, nB * F, r0, r1, false), l_lp = S.add_log(log_logp, R, nB * F, r0, r1, false);
    int r_ob = -1, r_ac = -1, r_lp = -1, r_vl = -1, r_rw = -1, r_dn = -1;
    if (rec_rows > 0) {
        // record rows: an instance writes rows nrec[b] .. nrec[b] + ceil(steps / record_every) - 1 at most; they
        // travel both ways, since an instance that records less leaves its entries of them untouched
        long long e0 = rec_rows, e1 = 0;
        for (int b = 0; b < B; ++b) {
            const long long n = nrec[b] < 0 ? 0 : nrec[b];
            e0 = n < e0 ? n : e0;
            e1 = n > e1 ? n : e1;
        }
        e1 += ((long long)steps + rcfg->record_every - 1) / rcfg->record_every;
        e1 = e1 < rec_rows ? e1 : rec_rows;
        e0 = e0 < e1 ? e0 : e1;
        const size_t q0 = (size_t)e0, q1 = (size_t)e1;
        r_ob = S.add_log(rec_obs, RR, 520 * nB * F, q0, q1, true); r_ac = S.add_log(rec_action, RR, 34 * nB * F, q0, q1, true);
        r_lp = S.add_log(rec_logp, RR, nB * F, q0, q1, true); r_vl = S.add_log(rec_value, RR, nB * F, q0, q1, true);
        r_rw = S.add_log(rec_reward, RR, nB * D, q0, q1, true); r_dn = S.add_log(rec_done, RR, nB * F, q0, q1, true);
    }
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    auto dd = [&](int i) { return i < 0 ? nullptr : S.dev<double>(h, i); };
    auto di = [&](int i) { return i < 0 ? nullptr : S.dev<int32_t>(h, i); };
    auto df = [&](int i) { return i < 0 ? nullptr : S.dev<float>(h, i); };
    if (int rc = dart_lmpc_collect_dev(
            h, plant, pcfg, rcfg, B, k0, steps, log_rows, rec_rows, reset_rows, dd(i_tg), dd(i_prm), dd(i_pp), dd(i_ck),
            df(i_wt), df(i_cr), df(i_nz), dd(i_x), dd(i_tilt), dd(i_up), dd(i_w), dd(i_om), dd(i_o2), di(i_oc), df(i_hi),
            di(i_ts), dd(i_mp), dd(c_pc), dd(c_cs), di(c_es), dd(c_er), dd(c_tp), di(c_ep), dd(c_lr), di(c_ls), di(c_nr),
            di(c_sk), dd(p_x), dd(p_t), dd(p_p), dd(l_X), dd(l_U), dd(l_pe), dd(l_pv), dd(l_L), di(l_st), di(l_it),
            dd(l_rw), di(l_dn), df(l_vl), df(l_lp), df(r_ob), df(r_ac), df(r_lp), df(r_vl), dd(r_rw), df(r_dn), s))
        return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

#undef DART_COLLECT_FILL
#undef DART_COLLECT_OUT_PARAMS
#undef DART_COLLECT_STATE_PARAMS

int dart_lmpc_gae_dev(int B, int rec_rows, double gamma, double lam, const int32_t* nrec, const double* rec_reward,
                      const float* rec_value, const float* rec_done, const float* last_value, double* adv, double* ret,
                      void* stream) {
    if (B < 0 || rec_rows < 0) return DART_MPC_EINVAL;
    if (B == 0 || rec_rows == 0) return DART_MPC_OK;
    if (!nrec || !rec_reward || !rec_value || !rec_done || !last_value || !adv || !ret) return DART_MPC_EINVAL;
    dartmpc::GaeArgs a;
    a.B = B; a.rec_rows = rec_rows; a.gamma = gamma; a.lam = lam; a.nrec = nrec; a.rec_reward = rec_reward;
    a.rec_value = rec_value; a.rec_done = rec_done; a.last_value = last_value; a.adv = adv; a.ret = ret;
    return dartmpc_launch_lmpc_gae(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_gae(int B, int rec_rows, double gamma, double lam, const int32_t* nrec, const double* rec_reward,
                  const float* rec_value, const float* rec_done, const float* last_value, double* adv, double* ret) {
    if (B < 0 || rec_rows < 0) return DART_MPC_EINVAL;
    if (B == 0 || rec_rows == 0) return DART_MPC_OK;
    if (!nrec || !rec_reward || !rec_value || !rec_done || !last_value || !adv || !ret) return DART_MPC_EINVAL;
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t n = (size_t)B * rec_rows;
    if (S.reserve(sizeof(double) * 3 * n + sizeof(float) * (2 * n + B) + sizeof(int32_t) * B + 8 * 256, 0) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    dartmpc::GaeArgs a;
    a.B = B; a.rec_rows = rec_rows; a.gamma = gamma; a.lam = lam;
    a.nrec = S.in(nrec, (size_t)B); a.rec_reward = S.in(rec_reward, n); a.rec_value = S.in(rec_value, n);
    a.rec_done = S.in(rec_done, n); a.last_value = S.in(last_value, (size_t)B);
    a.adv = S.inout(adv, n); a.ret = S.inout(ret, n);      // (rows >= nrec[b] keep the caller's contents)
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess) e = dartmpc_launch_lmpc_gae(&a, D->stream);
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
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

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the launches of the PPO entries; ws is laid out for (n, mb) with M <= mb
hipError_t ppo_launch_prepare(int n, long long total, const int32_t* sample, const double* adv, const double* ret,
                              float* adv_out, float* ret_out, char* ws, int mb, hipStream_t s) {
    const dartmpc::PpoWorkspace L = dartmpc::ppo_workspace(n, mb);
    dartmpc::PpoPrepareArgs a;
    a.n = n; a.rec_total = total; a.sample = sample; a.adv = adv; a.ret = ret;
    a.adv_n = reinterpret_cast<float*>(ws + L.adv_n); a.ret_n = reinterpret_cast<float*>(ws + L.ret_n);
    a.adv_out = adv_out; a.ret_out = ret_out;
    return dartmpc_launch_ppo_prepare(&a, s);
}

hipError_t ppo_launch_grad(const dart_lmpc_ppo_config* c, int n, long long total, int M, const int32_t* sample,
                           const int32_t* idx, const float* rec_obs, const float* rec_action, const float* rec_logp,
                           const float* weights, const float* critic, char* ws, int mb, hipStream_t s) {
    const dartmpc::PpoWorkspace L = dartmpc::ppo_workspace(n, mb);
    dartmpc::PpoGradArgs a;
    a.n = n; a.M = M; a.rec_total = total;
    a.clip_lo = (float)(1.0 - c->clip_eps); a.clip_hi = (float)(1.0 + c->clip_eps);
    a.vf_coef = (float)c->vf_coef; a.ent_coef = (float)c->ent_coef;
    a.log_std_min = (float)c->log_std_min; a.log_std_max = (float)c->log_std_max;
    a.sample = sample; a.idx = idx; a.rec_obs = rec_obs; a.rec_action = rec_action; a.rec_logp = rec_logp;
    a.adv_n = reinterpret_cast<const float*>(ws + L.adv_n); a.ret_n = reinterpret_cast<const float*>(ws + L.ret_n);
    a.actor = weights; a.critic = critic;
    a.part = reinterpret_cast<float*>(ws + L.part); a.loss_part = reinterpret_cast<float*>(ws + L.loss_part);
    return dartmpc_launch_ppo_grad(&a, s);
}

// from_tiles: sum the workspace's partials of a mini-batch of M; otherwise take the packed gradient `grad`
hipError_t ppo_launch_apply(const dart_lmpc_ppo_config* c, int n, int M, bool from_tiles, const float* grad,
                            const float* terms_in, bool do_step, float* grad_out, float* terms_out, float* weights,
                            float* critic, float* adam, int32_t* adam_step, double* stats, float* step_log,
                            int step_in_call, char* ws, int mb, hipStream_t s) {
    const dartmpc::PpoWorkspace L = dartmpc::ppo_workspace(n, mb);
    dartmpc::PpoApplyArgs a;
    a.tiles = from_tiles ? (M + dartmpc::kPpoTile - 1) / dartmpc::kPpoTile : 1;
    a.M = M; a.do_step = do_step ? 1 : 0; a.step_in_call = step_in_call;
    a.max_grad_norm = (float)c->max_grad_norm; a.lr = c->lr; a.beta1 = c->beta1;
    a.beta2 = c->beta2; a.adam_eps = (float)c->adam_eps; a.weight_decay = (float)c->weight_decay;
    a.ent_coef = (float)c->ent_coef; a.log_std_min = (float)c->log_std_min; a.log_std_max = (float)c->log_std_max;
    a.part = from_tiles ? reinterpret_cast<const float*>(ws + L.part) : grad;
    a.loss_part = from_tiles ? reinterpret_cast<const float*>(ws + L.loss_part) : nullptr;
    a.terms_in = terms_in;
    a.grad = grad_out ? grad_out : reinterpret_cast<float*>(ws + L.grad);
    a.terms = terms_out ? terms_out : reinterpret_cast<float*>(ws + L.terms);
    a.actor = weights; a.critic = critic; a.adam = adam; a.adam_step = adam_step;
    a.step_log = step_log; a.stat_sum = reinterpret_cast<double*>(ws + L.stat_sum); a.stats = stats;
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

}  // namespace

int dart_lmpc_ppo_update_dev(const dart_lmpc_ppo_config* cfg, int n, int rec_total, const int32_t* sample,
                             const int32_t* perm, const float* rec_obs, const float* rec_action,
                             const float* rec_logp, const double* adv, const double* ret, float* weights,
                             float* critic, float* adam, int32_t* adam_step, double* stats, float* step_log,
                             float* adv_norm_out, float* ret_norm_out, void* workspace, void* stream) {
    if (int rc = ppo_update_check(cfg, n, rec_total, sample, perm, rec_obs, rec_action, rec_logp, adv, ret, weights,
                                  critic, adam, adam_step, stats)) return rc;
    if (!workspace) return DART_MPC_EINVAL;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int mb = cfg->mini_batch_size;
    hipError_t e = ppo_launch_prepare(n, rec_total, sample, adv, ret, adv_norm_out, ret_norm_out, ws, mb, s);
    int step = 0;
    for (int ep = 0; ep < cfg->epochs && e == hipSuccess; ++ep) {
        const int32_t* row = perm + (size_t)ep * n;
        for (int start = 0; start < n && e == hipSuccess; start += mb, ++step) {
            const int M = n - start < mb ? n - start : mb;
            e = ppo_launch_grad(cfg, n, rec_total, M, sample, row + start, rec_obs, rec_action, rec_logp, weights,
                                critic, ws, mb, s);
            if (e == hipSuccess)
                e = ppo_launch_apply(cfg, n, M, true, nullptr, nullptr, true, nullptr, nullptr, weights, critic, adam,
                                     adam_step, stats, step_log, step, ws, mb, s);
        }
    }
    return e == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
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
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t N = (size_t)n, P = dartmpc::kPpoParams;
    const size_t steps = (size_t)cfg->epochs * ((N + cfg->mini_batch_size - 1) / cfg->mini_batch_size);
    const size_t ws_bytes = dartmpc::ppo_workspace(n, cfg->mini_batch_size).bytes;
    const size_t staged = sizeof(int32_t) * (N + np + 1) + sizeof(float) * (N * (520 + 34 + 1) + 3 * P + 4 * steps + 2 * N) +
                          sizeof(double) * (2 * N + 3) + 20 * 256;
    if (S.reserve(staged + ws_bytes, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    auto gather = [&](auto* dst, const auto* src, size_t width) {
        for (size_t i = 0; i < N; ++i) std::memcpy(dst + i * width, src + (size_t)sample[i] * width, sizeof(*dst) * width);
    };
    // (HostStage::in copies from a contiguous source: reserve the slots by hand for the gathered arrays)
    auto slot = [&](size_t bytes) { char* p = S.hin + S.in_off; S.in_off += HostStage::al(bytes); return p; };
    auto dev_of = [&](const void* h) { return S.din + ((const char*)h - S.hin); };
    int32_t* h_id = (int32_t*)slot(sizeof(int32_t) * N);
    for (int i = 0; i < n; ++i) h_id[i] = i;
    float* h_obs = (float*)slot(sizeof(float) * N * 520); gather(h_obs, rec_obs, 520);
    float* h_act = (float*)slot(sizeof(float) * N * 34); gather(h_act, rec_action, 34);
    float* h_lp = (float*)slot(sizeof(float) * N); gather(h_lp, rec_logp, 1);
    double* h_adv = (double*)slot(sizeof(double) * N); gather(h_adv, adv, 1);
    double* h_ret = (double*)slot(sizeof(double) * N); gather(h_ret, ret, 1);
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
        rc = dart_lmpc_ppo_update_dev(cfg, n, n, (const int32_t*)dev_of(h_id), d_perm, (const float*)dev_of(h_obs),
                                      (const float*)dev_of(h_act), (const float*)dev_of(h_lp),
                                      (const double*)dev_of(h_adv), (const double*)dev_of(h_ret), d_w, d_c, d_adam,
                                      d_step, d_stats, d_log, d_an, d_rn, ws, D->stream);
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
    dartmpc::CriticValueArgs a;
    a.n = n; a.critic = critic; a.obs = obs; a.value = value_out;
    return dartmpc_launch_critic_value(&a, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK : DART_MPC_EHIP;
}

int dart_lmpc_critic_value(int n, const float* critic, const float* obs, float* value_out) {
    if (n < 0) return DART_MPC_EINVAL;
    if (n == 0) return DART_MPC_OK;
    if (!critic || !obs || !value_out) return DART_MPC_EINVAL;
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t N = (size_t)n;
    if (S.reserve(sizeof(float) * (N * 520 + dartmpc::kPpoCriticN + N) + 4 * 256, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    dartmpc::CriticValueArgs a;
    a.n = n; a.critic = S.in(critic, (size_t)dartmpc::kPpoCriticN); a.obs = S.in(obs, N * 520);
    a.value = S.inout(value_out, N);
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess) e = dartmpc_launch_critic_value(&a, D->stream);
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
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
    a.n = (long long)steps * B * 34;
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
    return iteration >= 0 && steps >= 0 && B >= 0 && (long long)steps * B * 34 <= (1LL << 34);
}

int mean_update_args(const dart_lmpc_policy_config* cfg, int B, const float* weights, dartmpc::MeanUpdateArgs& a) {
    dartmpc::PolicyArgs pa;
    if (policy_args(cfg, B, weights, pa) != DART_MPC_OK) return DART_MPC_EINVAL;
    a.B = B; a.w = pa.w;
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
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t n = (size_t)steps * B * 34;
    if (S.reserve(0, sizeof(float) * n + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    float* d = S.out<float>(n);
    hipError_t e = launch_noise(seed, iteration, steps, B, d, D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
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
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t m = (size_t)epochs * n;
    if (S.reserve(0, 2 * (sizeof(int32_t) * m + 256)) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    int32_t* d = S.out<int32_t>(m);
    uint32_t* dk = key_out ? S.out<uint32_t>(m) : nullptr;
    hipError_t e = launch_perms(seed, iteration, epochs, n, d, dk, D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
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
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t nB = (size_t)B;
    if (S.reserve(sizeof(float) * ((size_t)DART_LMPC_POLICY_NWEIGHTS + 520 * nB) + sizeof(double) * 68 * nB + 8 * 256,
                  sizeof(float) * 34 * nB + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const float* d_w = S.in(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS);
    if (mean_update_args(cfg, B, d_w, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    a.history = S.in(history, 520 * nB);
    a.model_params = S.inout(model_params, 34 * nB);
    a.current_k = S.inout(current_k, 34 * nB);
    a.mean_out = mean_out ? S.out<float>(34 * nB) : nullptr;
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess) e = dartmpc_launch_lmpc_mean_update(&a, D->stream);
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
    S.take(mean_out, a.mean_out, 34 * nB);
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
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    if (S.reserve(0, sizeof(int32_t) * (size_t)m + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    int32_t* d = S.out<int32_t>((size_t)m);
    hipError_t e = launch_perms(seed, iteration, 1, n, d, nullptr, D->stream, dartmpc::kStreamChoice, m);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
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
    return dartmpc::global_workspace(n, epochs, mini_batch_size).bytes;
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

}  // namespace

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
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t M = (size_t)m, F = sizeof(float);
    const size_t row = F * (520 + 34 + 3) + sizeof(double);
    if (S.reserve(2 * (M * row + 8 * 256) + sizeof(int32_t) * M + 256, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    auto slot = [&](size_t bytes) { char* p = S.hin + S.in_off; S.in_off += HostStage::al(bytes); return p; };
    auto dev_of = [&](const void* hp) { return S.din + ((const char*)hp - S.hin); };
    auto gather = [&](auto* dst, const auto* src, size_t width) {
        for (size_t j = 0; j < M; ++j)
            std::memcpy(dst + j * width, src + (size_t)sample[choice[j]] * width, sizeof(*dst) * width);
    };
    int32_t* h_id = (int32_t*)slot(sizeof(int32_t) * M);
    for (int j = 0; j < m; ++j) h_id[j] = j;
    float* h_obs = (float*)slot(F * M * 520); gather(h_obs, rec_obs, 520);
    float* h_act = (float*)slot(F * M * 34); gather(h_act, rec_action, 34);
    float* h_lp = (float*)slot(F * M); gather(h_lp, rec_logp, 1);
    float* h_vl = (float*)slot(F * M); gather(h_vl, rec_value, 1);
    double* h_rw = (double*)slot(sizeof(double) * M); gather(h_rw, rec_reward, 1);
    float* h_dn = (float*)slot(F * M); gather(h_dn, rec_done, 1);
    const size_t f0 = (size_t)g->fill;
    dart_lmpc_global_buffer d = *g;                 // rows fill .. fill + m - 1 alone, as rows 0 .. m - 1
    d.obs = S.inout(g->obs + f0 * 520, M * 520); d.action = S.inout(g->action + f0 * 34, M * 34);
    d.logp = S.inout(g->logp + f0, M); d.value = S.inout(g->value + f0, M);
    d.reward = S.inout(g->reward + f0, M); d.done = S.inout(g->done + f0, M);
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess)
        e = launch_global_append(&d, 0, m, m, m, (const int32_t*)dev_of(h_id), (const int32_t*)dev_of(h_id),
                                 (const float*)dev_of(h_obs), (const float*)dev_of(h_act), (const float*)dev_of(h_lp),
                                 (const float*)dev_of(h_vl), (const double*)dev_of(h_rw), (const float*)dev_of(h_dn),
                                 D->stream);
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
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
    DeviceStage* D = nullptr;
    if (device_stage(&D) != hipSuccess) return DART_MPC_EHIP;
    std::lock_guard<std::mutex> lock(D->mu);
    HostStage& S = D->st;
    const size_t n = (size_t)G;
    if (S.reserve(sizeof(double) * 3 * n + sizeof(float) * (2 * n + 1) + 8 * 256, 0) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const double* d_rw = S.in(reward, n);
    const float* d_vl = S.in(value, n);
    const float* d_dn = S.in(done, n);
    const float* d_lv = S.in(last_value, (size_t)1);
    double* d_adv = S.inout(adv, n);
    double* d_ret = S.inout(ret, n);
    hipError_t e = S.upload(D->stream);
    if (e == hipSuccess) e = launch_gae_seq(G, gamma, lam, d_rw, d_vl, d_dn, d_lv, d_adv, d_ret, D->stream);
    if (e == hipSuccess) e = S.download_inout(D->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D->stream);
    if (e != hipSuccess) return DART_MPC_EHIP;
    S.finish_inout();
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
    return dartmpc::train_workspace(B, K, record_every, epochs, mini_batch_size).bytes;
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

// dart_lmpc_train_dev (g == nullptr) and dart_lmpc_train_global_dev
int train_dev_impl(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                   const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                   const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                   const dart_lmpc_global_buffer* g, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = train_check(h, rcfg, ppo, cfg, B, p, true)) return rc;
    const int K = cfg->steps, R = K / rcfg->record_every, n = R * B, mb = ppo->mini_batch_size;
    if (g) {
        if (int rc = global_check(h, g, n, true)) return rc;
        if (!aligned16(p->rec_obs)) return fail(h, DART_MPC_EINVAL, "rec_obs is not 16-byte aligned");
    }
    void* s = stream ? stream : (void*)h->stream;
    auto collect = [&](int steps, const float* noise) {
        return dart_lmpc_collect_dev(
            h, plant, pcfg, rcfg, B, 0, steps, K, R, reset_rows, p->target, p->prm, p->plant_pvec, p->current_k,
            p->weights, p->critic, noise, p->x, p->tilt, p->u_prev, p->w, p->obs_mean, p->obs_M2, p->obs_count,
            p->history, p->timestep, p->model_params, p->prev_cmd, p->control_seen, p->ep_step, p->ep_return,
            p->time_penalty, p->episodes, p->last_return, p->last_steps, p->nrec, p->sticky, p->reset_x,
            p->reset_target, p->reset_pvec, p->log_X, p->log_U, p->log_pos_error, p->log_pvec, p->log_loss,
            p->log_status, p->log_iters, p->log_reward, p->log_done, p->log_value, p->log_logp, p->rec_obs,
            p->rec_action, p->rec_logp, p->rec_value, p->rec_reward, p->rec_done, s);
    };
    // every check of the collection (configs, null pointers, B <= B_max) before any device work: zero steps
    if (int rc = collect(0, nullptr)) return rc;
    if (cfg->iterations == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    const dartmpc::TrainWorkspace L = dartmpc::train_workspace(B, K, rcfg->record_every, ppo->epochs, mb);
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
    // the global update's sizes, workspace and running fill (the host knows every launch from n and g->fill)
    int gm = 0, gG = 0, g_fill = g ? g->fill : 0;
    dartmpc::global_rows(n, gm, gG);
    const dartmpc::GlobalWorkspace GL = dartmpc::global_workspace(n, ppo->epochs, mb);
    char* gws = g ? (char*)g->workspace : nullptr;
    auto gp = [&](size_t off) { return gws ? gws + off : nullptr; };
    int32_t* g_choice = (int32_t*)gp(GL.choice);
    double* g_adv = (double*)gp(GL.adv);
    double* g_ret = (double*)gp(GL.ret);
    float* g_last = (float*)gp(GL.last_value);
    int32_t* g_sample = (int32_t*)gp(GL.sample);
    int32_t* g_perm = (int32_t*)gp(GL.perm);
    double* g_stats = (double*)gp(GL.stats);
    {
        dartmpc::IotaArgs ia;
        ia.n = n; ia.out = sample;
        HIPCHK(h, dartmpc_launch_iota(&ia, hs), "sample list launch");
    }
    for (int j = 0; j < cfg->iterations; ++j) {
        const int it = cfg->it0 + j;
        HIPCHK(h, hipMemsetAsync(p->nrec, 0, sizeof(int32_t) * (size_t)B, hs), "clear nrec");
        HIPCHK(h, hipMemcpyAsync(ep0, p->episodes, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToDevice, hs),
               "copy episodes");
        // (with epochs = 0 the update leaves its statistics untouched)
        if (ppo->epochs == 0) HIPCHK(h, hipMemsetAsync(stats, 0, sizeof(double) * 3, hs), "clear stats");
        HIPCHK(h, launch_noise(cfg->seed, it, K, B, noise, hs), "noise launch");
        if (int rc = collect(K, noise)) return rc;
        if (dart_lmpc_critic_value_dev(B, p->critic, p->history, last_value, s) != DART_MPC_OK)
            return fail(h, DART_MPC_EHIP, "critic value launch");
        if (dart_lmpc_gae_dev(B, R, cfg->gamma, cfg->lam, p->nrec, p->rec_reward, p->rec_value, p->rec_done,
                              last_value, adv, ret, s) != DART_MPC_OK)
            return fail(h, DART_MPC_EHIP, "GAE launch");
        HIPCHK(h, launch_perms(cfg->seed, it, ppo->epochs, n, perm, nullptr, hs), "permutation launch");
        if (int rc = dart_lmpc_ppo_update_dev(ppo, n, n, sample, perm, p->rec_obs, p->rec_action, p->rec_logp, adv,
                                              ret, p->weights, p->critic, p->adam, p->adam_step, stats, nullptr,
                                              nullptr, nullptr, ws + L.ppo, s))
            return fail(h, rc, "PPO update");
        if (g) {
            // 6a: m of this iteration's records, drawn without replacement, behind the rows held
            HIPCHK(h, launch_perms(cfg->seed, it, 1, n, g_choice, nullptr, hs, dartmpc::kStreamChoice, gm),
                   "choice launch");
            HIPCHK(h, launch_global_append(g, g_fill, gm, n, n, sample, g_choice, p->rec_obs, p->rec_action,
                                           p->rec_logp, p->rec_value, p->rec_reward, p->rec_done, hs),
                   "global buffer append launch");
            g_fill += gm;
            const int ran = g_fill >= n ? 1 : 0;
            const int logged_fill = g_fill;
            if (ran) {
                // 6b: the buffer holds G rows: one sequence for GAE, then a full update on the same optimizer
                if (dart_lmpc_critic_value_dev(1, p->critic, g->obs + (size_t)(gG - 1) * 520, g_last, s) != DART_MPC_OK)
                    return fail(h, DART_MPC_EHIP, "critic value launch (global buffer)");
                HIPCHK(h, launch_gae_seq(gG, cfg->gamma, cfg->lam, g->reward, g->value, g->done, g_last, g_adv, g_ret,
                                         hs), "sequence GAE launch");
                {
                    dartmpc::IotaArgs ia;
                    ia.n = gG; ia.out = g_sample;
                    HIPCHK(h, dartmpc_launch_iota(&ia, hs), "sample list launch (global buffer)");
                }
                if (ppo->epochs == 0) HIPCHK(h, hipMemsetAsync(g_stats, 0, sizeof(double) * 3, hs), "clear stats");
                HIPCHK(h, launch_perms(cfg->seed, it, ppo->epochs, gG, g_perm, nullptr, hs,
                                       dartmpc::kStreamGlobalPerm), "permutation launch (global buffer)");
                if (int rc = dart_lmpc_ppo_update_dev(ppo, gG, gG, g_sample, g_perm, g->obs, g->action, g->logp, g_adv,
                                                      g_ret, p->weights, p->critic, p->adam, p->adam_step, g_stats,
                                                      nullptr, nullptr, nullptr, gws + GL.ppo, s))
                    return fail(h, rc, "PPO update (global buffer)");
                g_fill = 0;
            }
            dartmpc::GlobalLogArgs ga;
            ga.fill = logged_fill; ga.ran = ran; ga.G = gG; ga.stats = g_stats;
            ga.row = g->global_log + (size_t)dartmpc::kGlobalLogCols * j;
            HIPCHK(h, dartmpc_launch_lmpc_global_log(&ga, hs), "global log launch");
        }
        if (cfg->mean_update)
            if (dart_lmpc_mean_param_update_dev(pcfg, B, p->weights, p->history, p->model_params, p->current_k,
                                                nullptr, s) != DART_MPC_OK)
                return fail(h, DART_MPC_EHIP, "mean parameter update launch");
        dartmpc::TrainLogArgs la;
        la.B = B; la.K = K; la.R = R; la.n = n; la.iteration = it; la.track_best = cfg->track_best ? 1 : 0;
        la.ep0 = ep0; la.episodes = p->episodes; la.last_return = p->last_return; la.nrec = p->nrec;
        la.log_reward = p->log_reward; la.log_status = p->log_status; la.stats = stats;
        la.actor = p->weights; la.critic = p->critic;
        la.row = p->train_log + (size_t)dartmpc::kTrainLogCols * j;
        la.best_return = p->best_return; la.best_weights = p->best_weights; la.best_iter = p->best_iter;
        HIPCHK(h, dartmpc_launch_lmpc_train_log(&la, hs), "training log launch");
    }
    return DART_MPC_OK;
}

// dart_lmpc_train (g == nullptr) and dart_lmpc_train_global
int train_host_impl(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                    const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                    const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                    const dart_lmpc_global_buffer* g, void* stream) {
    if (!h) return DART_MPC_EINVAL;
    std::unique_lock<std::recursive_mutex> lock_(h->mu);
    if (int rc = train_check(h, rcfg, ppo, cfg, B, p, false)) return rc;
    if (g)
        if (int rc = global_check(h, g, cfg->steps / rcfg->record_every * B, false)) return rc;
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, "handle is not an LMPC handle");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if (reset_rows < 0) return fail(h, DART_MPC_EINVAL, "negative reset_rows");
    if (any_null({p->target, p->prm, p->plant_pvec, p->x, p->tilt, p->u_prev, p->w, p->obs_mean, p->obs_M2,
                  p->obs_count, p->history, p->timestep, p->model_params, p->prev_cmd, p->control_seen, p->ep_step,
                  p->ep_return, p->time_penalty, p->episodes, p->last_return, p->last_steps, p->nrec, p->sticky,
                  p->log_X, p->log_U, p->log_pos_error, p->log_pvec, p->log_loss, p->log_status, p->log_iters,
                  p->log_reward, p->log_done, p->log_value, p->log_logp, p->rec_obs, p->rec_action, p->rec_logp,
                  p->rec_value, p->rec_reward, p->rec_done}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (reset_rows > 0 && any_null({p->reset_x, p->reset_target, p->reset_pvec}))
        return fail(h, DART_MPC_EINVAL, "reset_rows > 0 with a null reset pool");
    // instances that do not share timestep are the only way to nrec[b] != R
    for (int b = 1; b < B; ++b)
        if (p->timestep[b] != p->timestep[0]) return fail(h, DART_MPC_EINVAL, "instances differ in timestep");
    if (cfg->iterations == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nB = (size_t)B, D = sizeof(double), I = sizeof(int32_t), F = sizeof(float);
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N), P = dartmpc::kPpoParams;
    const size_t K = (size_t)cfg->steps, R = K / (size_t)rcfg->record_every, RS = (size_t)reset_rows;
    RollStage S;
    dart_lmpc_train_buffers d = *p;
    std::vector<std::pair<void**, int>> bind;       // device pointer of field <- arena block
    auto both = [&](auto*& field, size_t bytes) { bind.push_back({(void**)&field, S.add(field, bytes, true)}); };
    auto up = [&](auto*& field, size_t bytes) { bind.push_back({(void**)&field, S.add(field, bytes, false)}); };
    auto down = [&](auto*& field, size_t rows, size_t rowbytes) {
        bind.push_back({(void**)&field, S.add_log((void*)field, rows, rowbytes, 0, rows, false)});
    };
    both(d.target, 8 * nB * D); up(d.prm, dartmpc::LM_NPRM * nB * D); both(d.plant_pvec, 34 * nB * D);
    both(d.current_k, 34 * nB * D);
    both(d.weights, (size_t)DART_LMPC_POLICY_NWEIGHTS * F); both(d.critic, (size_t)DART_LMPC_CRITIC_NWEIGHTS * F);
    both(d.x, 8 * nB * D); both(d.tilt, 2 * nB * D); both(d.u_prev, 2 * nB * D); both(d.w, nw * nB * D);
    both(d.obs_mean, 52 * nB * D); both(d.obs_M2, 52 * nB * D); both(d.obs_count, nB * I);
    both(d.history, 520 * nB * F); both(d.timestep, nB * I); both(d.model_params, 34 * nB * D);
    both(d.prev_cmd, 2 * nB * D); both(d.control_seen, 2 * nB * D); both(d.ep_step, nB * I); both(d.ep_return, nB * D);
    both(d.time_penalty, nB * D); both(d.episodes, nB * I); both(d.last_return, nB * D); both(d.last_steps, nB * I);
    both(d.nrec, nB * I); both(d.sticky, nB * I);
    if (reset_rows > 0) {
        up(d.reset_x, RS * 8 * nB * D); up(d.reset_target, RS * 8 * nB * D); up(d.reset_pvec, RS * 34 * nB * D);
    } else {
        d.reset_x = d.reset_target = d.reset_pvec = nullptr;
    }
    down(d.log_X, K, 8 * nB * D); down(d.log_U, K, 2 * nB * D); down(d.log_pos_error, K, nB * D);
    down(d.log_pvec, K, 34 * nB * D); down(d.log_loss, K, nB * D); down(d.log_status, K, nB * I);
    down(d.log_iters, K, nB * I); down(d.log_reward, K, nB * D); down(d.log_done, K, nB * I);
    down(d.log_value, K, nB * F); down(d.log_logp, K, nB * F);
    down(d.rec_obs, R, 520 * nB * F); down(d.rec_action, R, 34 * nB * F); down(d.rec_logp, R, nB * F);
    down(d.rec_value, R, nB * F); down(d.rec_reward, R, nB * D); down(d.rec_done, R, nB * F);
    both(d.adam, 2 * P * F); both(d.adam_step, I);
    down(d.train_log, (size_t)cfg->iterations, dartmpc::kTrainLogCols * D);
    both(d.best_return, D); both(d.best_weights, P * F); both(d.best_iter, I);
    // the workspace: a block of the arena that does not travel
    const size_t ws_bytes = dartmpc::train_workspace(B, (int)K, rcfg->record_every, ppo->epochs,
                                                     ppo->mini_batch_size).bytes;
    const int i_ws = S.add_log(nullptr, 1, ws_bytes, 0, 0, false);
    // the global buffer: blocks of the arena whose held rows travel by hand (those held at the start go up, those
    // held at the end come down), its log, and its workspace
    dart_lmpc_global_buffer gd;
    int gi[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    size_t g_rowbytes[6] = {520 * F, 34 * F, F, F, D, F};
    if (g) {
        gd = *g;
        const size_t cap = (size_t)g->capacity;
        for (int q = 0; q < 6; ++q) gi[q] = S.add_log(nullptr, 1, cap * g_rowbytes[q], 0, 0, false);
        gi[6] = S.add_log(g->global_log, (size_t)cfg->iterations, dartmpc::kGlobalLogCols * D, 0,
                          (size_t)cfg->iterations, false);
        gi[7] = S.add_log(nullptr, 1, dartmpc::global_workspace((int)(R * nB), ppo->epochs, ppo->mini_batch_size).bytes,
                          0, 0, false);
    }
    if (int rc = S.reserve(h)) return rc;
    for (auto& b : bind) *b.first = S.dev<char>(h, b.second);
    d.workspace = S.dev<char>(h, i_ws);
    if (int rc = S.upload(h, s)) return rc;
    void* g_host[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (g) {
        void* hp[6] = {g->obs, g->action, g->logp, g->value, g->reward, g->done};
        for (int q = 0; q < 6; ++q) g_host[q] = hp[q];
        gd.obs = S.dev<float>(h, gi[0]); gd.action = S.dev<float>(h, gi[1]); gd.logp = S.dev<float>(h, gi[2]);
        gd.value = S.dev<float>(h, gi[3]); gd.reward = S.dev<double>(h, gi[4]); gd.done = S.dev<float>(h, gi[5]);
        gd.global_log = S.dev<double>(h, gi[6]); gd.workspace = S.dev<char>(h, gi[7]);
        for (int q = 0; q < 6 && g->fill > 0; ++q)
            HIPCHK(h, hipMemcpyAsync(S.dev<char>(h, gi[q]), g_host[q], (size_t)g->fill * g_rowbytes[q],
                                     hipMemcpyHostToDevice, s), "copy global buffer");
    }
    if (int rc = train_dev_impl(h, plant, pcfg, rcfg, ppo, cfg, B, reset_rows, &d, g ? &gd : nullptr, s)) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    if (int rc = S.download(h, s)) return rc;
    if (g) {
        const int held = dart_lmpc_global_fill_after((int)(R * nB), g->fill, cfg->iterations);
        for (int q = 0; q < 6 && held > 0; ++q)
            HIPCHK(h, hipMemcpyAsync(g_host[q], S.dev<char>(h, gi[q]), (size_t)held * g_rowbytes[q],
                                     hipMemcpyDeviceToHost, s), "copy global buffer back");
    }
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

}  // namespace

int dart_lmpc_train_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                        const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                        const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                        void* stream) {
    return train_dev_impl(h, plant, pcfg, rcfg, ppo, cfg, B, reset_rows, p, nullptr, stream);
}

int dart_lmpc_train(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                    const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                    const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                    void* stream) {
    return train_host_impl(h, plant, pcfg, rcfg, ppo, cfg, B, reset_rows, p, nullptr, stream);
}

int dart_lmpc_train_global_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                               const dart_lmpc_policy_config* pcfg, const dart_lmpc_reward_config* rcfg,
                               const dart_lmpc_ppo_config* ppo, const dart_lmpc_train_config* cfg, int B,
                               int reset_rows, const dart_lmpc_train_buffers* p, const dart_lmpc_global_buffer* g,
                               void* stream) {
    return train_dev_impl(h, plant, pcfg, rcfg, ppo, cfg, B, reset_rows, p, g, stream);
}

int dart_lmpc_train_global(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                           const dart_lmpc_reward_config* rcfg, const dart_lmpc_ppo_config* ppo,
                           const dart_lmpc_train_config* cfg, int B, int reset_rows, const dart_lmpc_train_buffers* p,
                           const dart_lmpc_global_buffer* g, void* stream) {
    return train_host_impl(h, plant, pcfg, rcfg, ppo, cfg, B, reset_rows, p, g, stream);
}
