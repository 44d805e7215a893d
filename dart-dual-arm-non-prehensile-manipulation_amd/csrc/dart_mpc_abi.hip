// dart_mpc_abi.hip -- the C ABI of include/dart_mpc.h (host side): handles, the solve entries of the three
// controllers, the policy entries, the arm QP and RLS.  (The closed-loop entries are in dart_mpc_rollout.hip, the
// training entries in dart_mpc_train.hip; abi_internal.h holds what the three share.)
//
// Owns the device workspace for the host-pointer entry point and the
// per-handle stream; validates arguments the way PMPC.__init__/solve would
// fail (mpc_3d.py:12-138), then launches the batched kernel.
#include "abi_internal.h"

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

namespace {

int check_cfg(const dart_mpc_config* c) {
    if (!c) return 0;
    if (c->variant != DART_MPC_PMPC && c->variant != DART_MPC_RMPC && c->variant != DART_MPC_LMPC) return 0;
    if (c->N < 1 || c->N > 63) return 0;
    // (PMPC takes max_iter = 0, as IPOPT does: no Newton iteration, the start point comes back at status -1)
    if (!(c->Ts > 0.0) || !(c->tol > 0.0) || !(c->gravity == c->gravity) || c->B_max < 1) return 0;
    if (c->max_iter < (c->variant == DART_MPC_PMPC ? 0 : 1)) return 0;
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
    auto al = align256;
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

// the mode of a host-entry launch of B instances: in the solving wave (small batches: one XCD), else host-driven
int host_mode_of(int B) { return dartmpc::xcd_pack(B) == 8 ? 1 : 2; }
int host_resto_mode(const dart_mpc_handle* h, int B) { return pmpc_resto_mode(h, host_mode_of(B)); }

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

// the configuration half of a PMPC launch's arguments (no completion words, no hand-off area)
dartmpc::PmpcArgs pmpc_cfg_args(const dart_mpc_handle* h, int B, int resto) {
    dartmpc::PmpcArgs a;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.max_iter = h->cfg.max_iter; a.g = h->cfg.gravity;
    a.max_soc = h->cfg.max_soc; a.reduced = h->cfg.pmpc_path; a.mult_init_max = h->cfg.constr_mult_init_max;
    a.done = nullptr; a.seq = 0;
    a.resto = resto; a.soft = pmpc_soft(h);
    a.resto_buf = nullptr;
    return a;
}

// the restoration hand-off area of a PMPC launch of B instances on stream s (when the launch can hand over)
int pmpc_resto_buf(dart_mpc_handle* h, int B, hipStream_t s, dartmpc::PmpcArgs& a) {
    a.resto_buf = nullptr;
    // Resuming from the register kernel's failed iteration is opt-in (DART_PMPC_RESUME=1): the register kernel's
    // iterate differs from the sequential (oracle-ordered) arithmetic by rounding, and the restoration phase
    // turns that into different iteration counts on ~19 % of the restored instances (the same statuses, u0
    // within 1.3e-11; tools/pmpc_resume_check.py, profiles/r05/pmpc_resume.txt).  By default the restoration
    // solve starts over on the LDS engine and takes the oracle's iterations exactly.
    if (!a.resto || !dartmpc::launch_knobs().pmpc_resume) return DART_MPC_OK;
    int xcd = 0;
    return stream_state(h, B, s, &a.resto_buf, &xcd);
}

// kernel arguments reading / writing the I/O area
dartmpc::PmpcArgs io_args(dart_mpc_handle* h, int B, bool ww, bool wo, int resto_mode = 1) {
    const auto& o = h->io;
    dartmpc::PmpcArgs a = pmpc_cfg_args(h, B, pmpc_resto_mode(h, resto_mode));
    a.x0 = (const double*)o.din; a.ref = (const double*)(o.din + o.off_ref); a.prm = (const double*)(o.din + o.off_prm);
    a.w_warm = ww ? (const double*)(o.din + o.off_ww) : nullptr;
    a.u0 = (double*)o.dout; a.f = (double*)(o.dout + o.off_f); a.w_out = wo ? (double*)(o.dout + o.off_wo) : nullptr;
    a.status = (int32_t*)(o.dout + o.off_st); a.iters = (int32_t*)(o.dout + o.off_it);
    a.done = h->ddone; a.seq = h->seq;
    return a;                     // (the caller sets resto_buf for its stream: pmpc_resto_buf)
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
    const bool wg2 = dartmpc::two_wave(h->cfg.N, dartmpc::launch_knobs());
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

}  // namespace

int settle_pending(dart_mpc_handle* h) {
    if (!h->pending) return DART_MPC_OK;
    hipStream_t s = h->pending;
    h->pending = nullptr;
    hipError_t e = hipStreamQuery(s);
    if (e == hipErrorNotReady) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(h, DART_MPC_EHIP, "previous PMPC call's stream", e);
    return DART_MPC_OK;
}

namespace {

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
    dartmpc::PmpcArgs a = io_args(h, B, ww, wo, host_mode_of(B));
    if (int rc = pmpc_resto_buf(h, B, h->stream, a)) return rc;
    HIPCHK(h, dartmpc_launch_pmpc(&a, h->stream), "kernel launch");
    int rc = wait_done(h, h->stream, h->hdone, B, a.seq);
    if (rc == DART_MPC_OK) rc = host_resto(h, a, (const int32_t*)(h->io.hout + h->io.off_st), h->stream);
    if (rc == DART_MPC_OK) h->pending = h->stream;
    return rc;
}

// the configuration half of an LMPC launch's arguments, and the per-stream state of the launch
int lmpc_cfg_args(dart_mpc_handle* h, int B, hipStream_t s, dartmpc::LmpcArgs& a) {
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.max_iter = h->cfg.max_iter;
    a.acc_tol = h->cfg.acceptable_tol; a.acc_iter = h->cfg.acceptable_iter; a.max_soc = h->cfg.max_soc;
    a.mult_init_max = h->cfg.constr_mult_init_max;
    a.resto = h->cfg.restoration;
    a.max_ticks = (long long)(h->cfg.max_cpu_time * 1e8);     // s_memrealtime: 100 MHz
    return stream_state(h, B, s, &a.resto_buf, &a.xcd);
}

// the outputs every solve entry has, staged in mapped host memory
struct SolveOut {
    double *u0, *f, *w;
    int32_t *status, *iters;
    SolveOut(HostStage& S, size_t B, size_t nw, bool want_w)
        : u0(S.out<double>(2 * B)), f(S.out<double>(B)), w(want_w ? S.out<double>(nw * B) : nullptr),
          status(S.out<int32_t>(B)), iters(S.out<int32_t>(B)) {}
    void take(const HostStage& S, size_t B, size_t nw, double* u0_, double* f_, double* w_, int32_t* status_,
              int32_t* iters_) const {
        S.take(u0_, u0, 2 * B); S.take(f_, f, B); S.take(w_, w, nw * B);
        S.take(status_, status, B); S.take(iters_, iters, B);
    }
};

// The argument checks a solve entry and its host twin share (after the variant's): the batch and the required
// pointers, [RMPC: the fused RLS step's inputs,] then the host entry's limit (the _dev entries pass B itself)
int solve_check(dart_mpc_handle* h, int B, int B_limit, std::initializer_list<const void*> required) {
    if (B < 0 || (B > 0 && any_null(required))) return fail(h, DART_MPC_EINVAL, "null pointer or negative batch");
    if (B > B_limit) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    return DART_MPC_OK;
}

int rmpc_solve_check(dart_mpc_handle* h, int B, int B_limit, std::initializer_list<const void*> required,
                     const double* rls_P, const double* rls_phi, const double* rls_y, double rls_lambda) {
    if (int rc = solve_check(h, B, B, required)) return rc;
    if (rls_P && (!rls_phi || !rls_y || !(rls_lambda > 0.0))) return fail(h, DART_MPC_EINVAL, "RLS inputs incomplete");
    return solve_check(h, B, B_limit, {});
}

}  // namespace

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
    DART_ENTER(h, DART_MPC_PMPC);
    if (int rc = solve_check(h, B, B, {x0, ref, prm, u0, f, status, iters})) return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    if (int rc = settle_pending(h)) return rc;
    hipStream_t s = stream_of(h, stream);
    dartmpc::PmpcArgs a = pmpc_cfg_args(h, B, pmpc_resto_mode(h, 1));
    a.x0 = x0; a.ref = ref; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    if (int rc = pmpc_resto_buf(h, B, s, a)) return rc;
    HIPCHK(h, dartmpc_launch_pmpc(&a, s), "kernel launch");
    return DART_MPC_OK;
}

int dart_mpc_solve_batch(dart_mpc_handle* h, int B, const double* x0, const double* ref, const double* prm,
                         const double* w_warm, double* u0, double* f, double* w_out, int32_t* status,
                         int32_t* iters, void* stream) {
    DART_ENTER(h, DART_MPC_PMPC);
    if (int rc = solve_check(h, B, h->cfg.B_max, {x0, ref, prm, u0, f, status, iters})) return rc;
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
    hipStream_t s = stream_of(h, stream);

    HostStage& S = h->st;
    S.begin();
    // the PMPC kernel reads x0 / ref / prm / w_warm once, at its start: zero-copy from mapped host
    // memory instead of a DMA copy on the call path
    const double* d_x0 = S.in_zc(x0, 6 * B);
    const double* d_ref = S.in_zc(ref, 6 * B);
    const double* d_prm = S.in_zc(prm, 6 * B);
    const double* d_ww = S.in_zc(w_warm, nw * B);
    const SolveOut o(S, B, nw, w_out != nullptr);
    uint32_t* d_done = h->ddone;
    HIPCHK(h, S.upload(s), "copy inputs");
    dartmpc::PmpcArgs a = pmpc_cfg_args(h, B, host_resto_mode(h, B));
    a.x0 = d_x0; a.ref = d_ref; a.prm = d_prm; a.w_warm = d_ww;
    a.u0 = o.u0; a.f = o.f; a.w_out = o.w; a.status = o.status; a.iters = o.iters;
    a.done = d_done; a.seq = next_seq(h);
    if (int rc = pmpc_resto_buf(h, B, s, a)) return rc;
    HIPCHK(h, dartmpc_launch_pmpc(&a, s), "kernel launch");
    int rc = wait_done(h, s, h->hdone, B, a.seq);
    if (rc == DART_MPC_OK) rc = host_resto(h, a, S.host_of(o.status), s);
    if (rc) return rc;
    h->pending = s;
    o.take(S, B, nw, u0, f, w_out, status, iters);
    return DART_MPC_OK;
}

int dart_rmpc_solve_batch_dev(dart_mpc_handle* h, int B, const double* x0, const double* u_prev, double* theta,
                              double* rls_P, const double* rls_phi, const double* rls_y, double rls_lambda,
                              const double* Rref, const double* prm, const double* w_warm, double* u0, double* f,
                              double* w_out, int32_t* status, int32_t* iters, void* stream) {
    DART_ENTER(h, DART_MPC_RMPC);
    if (int rc = rmpc_solve_check(h, B, B, {x0, u_prev, theta, Rref, prm, u0, f, status, iters}, rls_P, rls_phi, rls_y,
                                  rls_lambda))
        return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::RmpcArgs a;
    a.B = B; a.N = h->cfg.N; a.Ts = h->cfg.Ts; a.tol = h->cfg.tol; a.g = h->cfg.gravity; a.max_iter = h->cfg.max_iter; a.mult_init_max = h->cfg.constr_mult_init_max;
    a.resto = h->cfg.restoration; a.max_soc = h->cfg.max_soc;
    a.x0 = x0; a.u_prev = u_prev; a.theta = theta; a.rls_P = rls_P; a.rls_phi = rls_phi; a.rls_y = rls_y;
    a.rls_lambda = rls_lambda; a.Rref = Rref; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    a.resto_buf = nullptr;
    hipStream_t s = stream_of(h, stream);
    if (dartmpc::two_wave(a.N, dartmpc::launch_knobs()) && a.resto) {      // the two-wave build's restoration state, one area per stream
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
    DART_ENTER(h, DART_MPC_RMPC);
    if (int rc = rmpc_solve_check(h, B, h->cfg.B_max, {x0, u_prev, theta, Rref, prm, u0, f, status, iters}, rls_P,
                                  rls_phi, rls_y, rls_lambda))
        return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream_of(h, stream);
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
    const SolveOut o(S, B, nw, w_out != nullptr);
    HIPCHK(h, S.upload(s), "copy inputs");
    int rc = dart_rmpc_solve_batch_dev(h, B, d_x0, d_up, d_th, d_P, d_phi, d_y, rls_lambda, d_R, d_prm, d_ww, o.u0, o.f,
                                       o.w, o.status, o.iters, s);
    if (rc) return rc;
    HIPCHK(h, S.download_inout(s), "copy theta / rls_P");
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    S.finish_inout();
    o.take(S, B, nw, u0, f, w_out, status, iters);
    return DART_MPC_OK;
}

int dart_lmpc_solve_batch_dev(dart_mpc_handle* h, int B, const double* state, const double* u_prev,
                              const double* pvec, const double* target, const double* prm, const double* w_warm,
                              double* u0, double* f, double* w_out, int32_t* status, int32_t* iters, void* stream) {
    DART_ENTER(h, DART_MPC_LMPC);
    if (int rc = solve_check(h, B, B, {state, u_prev, pvec, target, prm, u0, f, status, iters})) return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::LmpcArgs a;
    if (int rc = lmpc_cfg_args(h, B, stream_of(h, stream), a)) return rc;
    a.state = state; a.u_prev = u_prev; a.pvec = pvec; a.target = target; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    a.fuse_policy = 0;
    HIPCHK(h, dartmpc_launch_lmpc(&a, stream_of(h, stream)), "kernel launch");
    return DART_MPC_OK;
}

int dart_lmpc_solve_batch(dart_mpc_handle* h, int B, const double* state, const double* u_prev, const double* pvec,
                          const double* target, const double* prm, const double* w_warm, double* u0, double* f,
                          double* w_out, int32_t* status, int32_t* iters, void* stream) {
    DART_ENTER(h, DART_MPC_LMPC);
    if (int rc = solve_check(h, B, h->cfg.B_max, {state, u_prev, pvec, target, prm, u0, f, status, iters})) return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream_of(h, stream);
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N);
    HostStage& S = h->st;
    S.begin();
    const double* d_st0 = S.in(state, 8 * B);
    const double* d_up = S.in(u_prev, 2 * B);
    const double* d_pv = S.in(pvec, dartmpc::LM_NPV * B);
    const double* d_tg = S.in(target, 8 * B);
    const double* d_prm = S.in(prm, dartmpc::LM_NPRM * B);
    const double* d_ww = S.in(w_warm, nw * B);
    const SolveOut o(S, B, nw, w_out != nullptr);
    HIPCHK(h, S.upload(s), "copy inputs");
    int rc = dart_lmpc_solve_batch_dev(h, B, d_st0, d_up, d_pv, d_tg, d_prm, d_ww, o.u0, o.f, o.w, o.status, o.iters, s);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    o.take(S, B, nw, u0, f, w_out, status, iters);
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

int policy_args(const dart_lmpc_policy_config* c, int B, const float* w, dartmpc::PolicyArgs& a) {
    if (!c || B < 0 || !w || c->update_every < 1 || !(c->k_max > c->min_k) || !(c->min_k > 0.0)) return DART_MPC_EINVAL;
    a.B = B;
    a.w = policy_weights(w);
    a.update_every = c->update_every; a.learner_B = 0;
    a.max_delta = c->max_delta; a.k_max = c->k_max; a.min_k = c->min_k; a.k_ceiling_margin = c->k_ceiling_margin;
    a.action_scale = c->action_scale; a.smooth_alpha = c->smooth_alpha;
    a.log_std_min = c->log_std_min; a.log_std_max = c->log_std_max;
    return DART_MPC_OK;
}

// what the policy step and its host twin check
static int policy_step_check(const dart_lmpc_policy_config* cfg, int B, const float* weights, dartmpc::PolicyArgs& a,
                             std::initializer_list<const void*> arrays) {
    if (policy_args(cfg, B, weights, a) != DART_MPC_OK) return DART_MPC_EINVAL;
    return B > 0 && any_null(arrays) ? DART_MPC_EINVAL : DART_MPC_OK;
}

// ... and the fused policy step + solve and its host twin (the _dev entry passes B itself as the limit)
static int policy_solve_check(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, int B, int B_limit,
                              const float* weights, dartmpc::PolicyArgs& a, std::initializer_list<const void*> arrays) {
    if (policy_args(pcfg, B, weights, a) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
    if (B > 0 && any_null(arrays)) return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B > B_limit) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    return DART_MPC_OK;
}

int dart_lmpc_policy_step_dev(const dart_lmpc_policy_config* cfg, int B, const float* weights, const double* state,
                              const double* target, const double* control, const double* current_k, double* obs_mean,
                              double* obs_M2, int32_t* obs_count, float* history, int32_t* timestep, const float* noise,
                              double* model_params, float* action_out, void* stream) {
    dartmpc::PolicyArgs a;
    if (policy_step_check(cfg, B, weights, a, {state, target, control, current_k, obs_mean, obs_M2, obs_count, history,
                                               timestep, noise, model_params})) return DART_MPC_EINVAL;
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
    if (policy_step_check(cfg, B, weights, a, {state, target, control, current_k, obs_mean, obs_M2, obs_count, history,
                                               timestep, noise, model_params})) return DART_MPC_EINVAL;
    if (B == 0) return DART_MPC_OK;
    DART_DEVICE_STAGE(D, S);
    const size_t nin = sizeof(float) * ((size_t)DART_LMPC_POLICY_NWEIGHTS + (size_t)B * (kAct + kHist)) +
                       sizeof(double) * (size_t)B * (8 + 8 + 2 + 2 * kAct + 2 * kObs) + sizeof(int32_t) * 2 * B + 16 * 256;
    if (S.reserve(nin, sizeof(float) * kAct * B + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    a.w = policy_weights(S.in(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS));
    a.state = S.in(state, 8 * (size_t)B); a.target = S.in(target, 8 * (size_t)B);
    a.control = S.in(control, 2 * (size_t)B); a.current_k = S.in(current_k, kAct * (size_t)B);
    a.noise = S.in(noise, kAct * (size_t)B);
    a.obs_mean = S.inout(obs_mean, kObs * (size_t)B); a.obs_M2 = S.inout(obs_M2, kObs * (size_t)B);
    a.model_params = S.inout(model_params, kAct * (size_t)B); a.history = S.inout(history, kHist * (size_t)B);
    a.obs_count = S.inout(obs_count, (size_t)B); a.timestep = S.inout(timestep, (size_t)B);
    a.action_out = S.out<float>(kAct * (size_t)B);
    if (!D->run([&](hipStream_t s) { return dartmpc_launch_policy(&a, s); })) return DART_MPC_EHIP;
    S.take(action_out, a.action_out, kAct * (size_t)B);
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
    return lmpc_policy_solve_dev(h, pcfg, B, 0, weights, state, u_prev, target, current_k, obs_mean, obs_M2, obs_count,
                                 history, timestep, noise, model_params, action_out, prm, w_warm, u0, f, w_out, status,
                                 iters, stream);
}

int lmpc_policy_solve_dev(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, int B, int learner_B,
                          const float* weights, const double* state, const double* u_prev, const double* target,
                          const double* current_k, double* obs_mean, double* obs_M2, int32_t* obs_count, float* history,
                          int32_t* timestep, const float* noise, double* model_params, float* action_out,
                          const double* prm, const double* w_warm, double* u0, double* f, double* w_out,
                          int32_t* status, int32_t* iters, void* stream) {
    DART_ENTER(h, DART_MPC_LMPC);
    if (learner_B < 0) return fail(h, DART_MPC_EINVAL, "negative learner block size");
    dartmpc::LmpcArgs a;
    if (int rc = policy_solve_check(h, pcfg, B, B, weights, a.pol,
                                    {state, u_prev, target, current_k, obs_mean, obs_M2, obs_count, history, timestep,
                                     noise, model_params, prm, u0, f, status, iters}))
        return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    a.pol.state = state; a.pol.target = target; a.pol.control = u_prev; a.pol.current_k = current_k;
    a.pol.obs_mean = obs_mean; a.pol.obs_M2 = obs_M2; a.pol.obs_count = obs_count; a.pol.history = history;
    a.pol.timestep = timestep; a.pol.noise = noise; a.pol.model_params = model_params; a.pol.action_out = action_out;
    a.pol.learner_B = learner_B;
    a.fuse_policy = 1;
    if (int rc = lmpc_cfg_args(h, B, stream_of(h, stream), a)) return rc;
    a.state = state; a.u_prev = u_prev; a.pvec = nullptr; a.target = target; a.prm = prm; a.w_warm = w_warm;
    a.u0 = u0; a.f = f; a.w_out = w_out; a.status = status; a.iters = iters;
    HIPCHK(h, dartmpc_launch_lmpc(&a, stream_of(h, stream)), "kernel launch");
    return DART_MPC_OK;
}

int dart_lmpc_policy_solve_batch(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, int B, const float* weights,
                                 const double* state, const double* u_prev, const double* target,
                                 const double* current_k, double* obs_mean, double* obs_M2, int32_t* obs_count,
                                 float* history, int32_t* timestep, const float* noise, double* model_params,
                                 float* action_out, const double* prm, const double* w_warm, double* u0, double* f,
                                 double* w_out, int32_t* status, int32_t* iters, void* stream) {
    DART_ENTER(h, DART_MPC_LMPC);
    dartmpc::PolicyArgs chk;
    if (int rc = policy_solve_check(h, pcfg, B, h->cfg.B_max, weights, chk,
                                    {state, u_prev, target, current_k, obs_mean, obs_M2, obs_count, history, timestep,
                                     noise, model_params, prm, u0, f, status, iters}))
        return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream_of(h, stream);
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N), Bz = (size_t)B;
    HostStage& S = h->st;
    const size_t nin = sizeof(float) * ((size_t)DART_LMPC_POLICY_NWEIGHTS + Bz * (kAct + kHist)) +
                       sizeof(double) * Bz * (8 + 2 + 8 + kAct + dartmpc::LM_NPRM + nw + kObs + kObs + kAct) +
                       sizeof(int32_t) * 2 * Bz + 24 * 256;
    const size_t nout = sizeof(double) * Bz * (2 + 1 + nw) + sizeof(int32_t) * 2 * Bz + sizeof(float) * kAct * Bz + 8 * 256;
    HIPCHK(h, S.reserve(nin, nout), "staging buffers");
    S.begin();
    const float* d_w = S.in(weights, (size_t)DART_LMPC_POLICY_NWEIGHTS);
    const double* d_st0 = S.in(state, 8 * Bz);
    const double* d_up = S.in(u_prev, 2 * Bz);
    const double* d_tg = S.in(target, 8 * Bz);
    const double* d_ck = S.in(current_k, kAct * Bz);
    const float* d_nz = S.in(noise, kAct * Bz);
    const double* d_prm = S.in(prm, dartmpc::LM_NPRM * Bz);
    const double* d_ww = S.in(w_warm, nw * Bz);
    double* d_mean = S.inout(obs_mean, kObs * Bz);
    double* d_M2 = S.inout(obs_M2, kObs * Bz);
    double* d_mp = S.inout(model_params, kAct * Bz);
    float* d_hist = S.inout(history, kHist * Bz);
    int32_t* d_cnt = S.inout(obs_count, Bz);
    int32_t* d_ts = S.inout(timestep, Bz);
    const SolveOut o(S, Bz, nw, w_out != nullptr);
    float* d_act = action_out ? S.out<float>(kAct * Bz) : nullptr;
    HIPCHK(h, S.upload(s), "copy inputs");
    int rc = dart_lmpc_policy_solve_batch_dev(h, pcfg, B, d_w, d_st0, d_up, d_tg, d_ck, d_mean, d_M2, d_cnt, d_hist, d_ts,
                                              d_nz, d_mp, d_act, d_prm, d_ww, o.u0, o.f, o.w, o.status, o.iters, s);
    if (rc) return rc;
    HIPCHK(h, S.download_inout(s), "copy policy state");
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    S.finish_inout();
    o.take(S, Bz, nw, u0, f, w_out, status, iters);
    S.take(action_out, d_act, kAct * Bz);
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
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(sizeof(double) * (size_t)B * (7 + 49 + 7 + 1) + 4 * 256, 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const double* dphi = S.in(phi, 7 * (size_t)B);
    const double* dy = S.in(y, (size_t)B);
    double* dt = S.inout(theta, 7 * (size_t)B);
    double* dP = S.inout(P, 49 * (size_t)B);
    auto launch = [&](hipStream_t s) { return dartmpc_launch_rls(B, dt, dP, dphi, dy, lambda, s); };
    if (!D->run(launch)) return DART_MPC_EHIP;
    return DART_MPC_OK;
}

int dart_mpc_serve_start(dart_mpc_handle* h, int B_serve, double idle_timeout_s) {
    DART_ENTER(h, DART_MPC_PMPC);
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
    DART_ENTER(h, DART_MPC_PMPC);
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
    DART_ENTER(h, DART_MPC_PMPC);
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
    DART_ENTER(h, -1);
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
    DART_ENTER(h, -1);
    if (int rc = settle_pending(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize");
    return DART_MPC_OK;
}

// internal self-test of the wave primitives (not in include/dart_mpc.h): host_out[265]
extern "C" int dartmpc_selftest(double* host_out) {
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
    DART_DEVICE_STAGE(D, S);
    if (S.reserve(sizeof(double) * (SL * B + np) + 2 * 256,
                  sizeof(double) * (2 * (size_t)n * B + B) + sizeof(int32_t) * 2 * B + 5 * 256) != hipSuccess)
        return DART_MPC_EHIP;
    S.begin();
    a.snap = S.in(snap, SL * B); a.prm = S.in(prm, np);
    a.qdd = S.out<double>((size_t)n * B); a.tau = S.out<double>((size_t)n * B); a.loss = S.out<double>(B);
    a.status = S.out<int32_t>(B); a.iters = S.out<int32_t>(B);
    if (!D->run([&](hipStream_t s) { return dartmpc_launch_arm(&a, s); })) return DART_MPC_EHIP;
    S.take(qdd, a.qdd, (size_t)n * B); S.take(tau, a.tau, (size_t)n * B); S.take(loss, a.loss, B);
    S.take(status, a.status, B); S.take(iters, a.iters, B);
    return DART_MPC_OK;
}
