// dart_mpc_rollout.hip -- the closed-loop entries of include/dart_mpc.h (host side): the loop-step and rollout entries
// of the three controllers (loop_step.hip between the unchanged solves), the LMPC evaluation (the LMPC loop with
// metrics, optional logs and P weight sets), LMPC experience step and collection (lmpc_experience.hip after every
// post of the LMPC closed loop).
#include "abi_internal.h"

void dart_plant_config_default(dart_plant_config* c) {
    if (!c) return;
    c->tau = 0.03; c->mu_c = 0.02; c->v_c = 0.01;       // harness.TrayPlant
}

void dart_rmpc_loop_config_default(dart_rmpc_loop_config* c) {
    if (!c) return;
    c->dr_max = 0.01; c->alpha_rg = 0.5; c->step_fraction = 0.2; c->rls_lambda = 0.995; c->pos_tol = 0.01;
}

dartmpc::PlantArgs plant_args(const dart_mpc_handle* h, const dart_plant_config* p) {
    dartmpc::PlantArgs a;
    a.a_lag = p->tau > 0.0 ? 1.0 - std::exp(-h->cfg.Ts / p->tau) : 1.0;
    a.mu_c = p->mu_c; a.v_c = p->v_c; a.dt = h->cfg.Ts; a.g = h->cfg.gravity;
    return a;
}

namespace {

// the checks every LMPC rollout / loop-step entry shares: the call writes the log rows k .. k + steps - 1.  (The
// LMPC plant does not use mu_c / v_c.)
int loop_check(dart_mpc_handle* h, const dart_plant_config* plant, int B, int k, int steps, int log_rows) {
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, variant_text(DART_MPC_LMPC));
    if (!plant) return fail(h, DART_MPC_EINVAL, "null plant config");
    if (B < 0 || k < 0 || steps < 0 || log_rows < 0) return fail(h, DART_MPC_EINVAL, "negative batch, step or row count");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    if ((long long)k + steps > log_rows) return fail(h, DART_MPC_EINVAL, "k0 + steps exceeds log_rows");
    return DART_MPC_OK;
}

// The handle's rollout scratch (B_max instances): n blocks of cnt[i] bytes per instance, 256-byte aligned, allocated
// on first use with the blocks from `zero_from` on cleared; ptr[i] receives block i
int scratch_blocks(dart_mpc_handle* h, int n, const size_t* cnt, int zero_from, char** ptr) {
    size_t off = 0;
    size_t at[16];
    for (int i = 0; i < n; ++i) {
        at[i] = off;
        off += align256(cnt[i] * (size_t)h->cfg.B_max);
    }
    if (!h->loop_buf) {
        HIPCHK(h, hipMalloc((void**)&h->loop_buf, off), "hipMalloc (rollout scratch)");
        const hipError_t e = zero_from < n ? hipMemset(h->loop_buf + at[zero_from], 0, off - at[zero_from]) : hipSuccess;
        if (e != hipSuccess) {
            (void)hipFree(h->loop_buf);
            h->loop_buf = nullptr;
            return fail(h, DART_MPC_EHIP, "hipMemset (rollout scratch)", e);
        }
    }
    for (int i = 0; i < n; ++i) ptr[i] = h->loop_buf + at[i];
    return DART_MPC_OK;
}

// (the entries never write through what they take const: the views' members are not const)
template <class T> T* mut(const T* p) { return const_cast<T*>(p); }

}  // namespace

// a rollout's own per-step arrays of the solve (abi_internal.h LoopIo), in the handle's scratch
int loop_scratch(dart_mpc_handle* h, LoopIo& L) {
    const size_t N1 = (size_t)h->cfg.N + 1;
    const bool rm = h->cfg.variant == DART_MPC_RMPC;
    const size_t r = rm ? 1 : 0;         // (Rref, phi and y are RMPC's)
    const size_t cnt[8] = {8 * (rm ? 4u : 6u), 8 * 4 * N1 * r, 8 * 7 * r, 8 * 2 * r, 8 * 2, 8, 4, 4};
    char* p[8];
    // (no initialisation: pre writes what the solve reads, the solve writes what post reads)
    if (int rc = scratch_blocks(h, 8, cnt, 8, p)) return rc;
    L.x0 = (double*)p[0]; L.Rref = (double*)p[1]; L.phi = (double*)p[2]; L.y = (double*)p[3];
    L.u0 = (double*)p[4]; L.f = (double*)p[5]; L.status = (int32_t*)p[6]; L.iters = (int32_t*)p[7];
    return DART_MPC_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------
// PMPC and RMPC closed loops (pmpc_loop_kernel / rmpc_loop_kernel between the unchanged solves), on the tray plant
// (dart_pmpc_* / dart_rmpc_*) and on the LMPC plant with streaming metrics (dart_pmpc_lm_* / dart_rmpc_lm_*).  The
// entries build one LoopBuf from their positional arguments; everything below the entries takes that.  One table,
// kLoopArr, describes each array once.
struct LoopBuf {
    const double *target, *prm, *mu, *plant_pvec, *pz_vz;
    double *x, *tilt, *prev, *u_prev, *r_v, *theta, *P, *w;
    int32_t *done, *nlog;
    double* metrics;
    double *log_pos_err, *log_pos_err_norm, *log_u_cmd, *log_timestep;     // RMPC's episode rows
    double *log_x, *log_theta, *log_r_v, *log_f;                          // RMPC's step rows
    double *log_X, *log_U, *log_quat, *log_loss;                          // PMPC's step rows
    int32_t *log_status, *log_iters;
    double* log_rot;
};

enum LoopKind : uint8_t {
    cUp,        // [B][width], up only
    cBoth,      // [B][width], both ways
    cEpisode,   // [log_rows][B][width], RMPC's episode rows: the rows the call can write travel both ways
    cStep       // [log_rows][B][width], the call's step rows come down
};
// A loop is one bit, 1 << (2 lm + rm); the masks of a controller's and of a plant's loops, so that kPm & kTray is
// PMPC on the tray plant
constexpr uint8_t kPm = 0x5, kRm = 0xA, kTray = 0x3, kLm = 0xC, kAny = 0xF;
constexpr uint8_t loop_bit(bool rm, bool lm) { return (rm ? kRm : kPm) & (lm ? kLm : kTray); }
constexpr int kNw = -1, kNxPlant = -2;      // widths: the solve's nw; the plant's state, 6 (tray) or 8 (LMPC plant)
struct LoopArr {
    size_t member;        // offsetof(LoopBuf, ...)
    int wp, wr;           // elements per instance under PMPC / RMPC; 0: not an array of that controller
    uint8_t size, kind;
    uint8_t plants;       // kTray, kLm or kAny: the plants whose loops have the array
    uint8_t solve_only;   // loops whose loop-step launch does not take the array (only the solve reads it)
};
#define ARR(member, wp, wr, type, kind, plants, solve_only) \
    {offsetof(LoopBuf, member), wp, wr, sizeof(type), kind, plants, solve_only}
const LoopArr kLoopArr[] = {
    ARR(target, 6, 4, double, cUp, kAny, kPm & kTray), ARR(prm, 6, 10, double, cUp, kAny, kPm & kLm),
    ARR(mu, 0, 1, double, cUp, kTray, 0), ARR(plant_pvec, 34, 34, double, cUp, kLm, 0), ARR(pz_vz, 2, 0, double, cUp, kLm, 0),
    ARR(x, kNxPlant, kNxPlant, double, cBoth, kAny, 0), ARR(tilt, 2, 2, double, cBoth, kAny, 0),
    ARR(prev, 0, 4, double, cBoth, kAny, 0), ARR(u_prev, 0, 2, double, cBoth, kAny, 0), ARR(r_v, 0, 4, double, cBoth, kAny, 0),
    ARR(theta, 0, 14, double, cBoth, kAny, 0), ARR(P, 0, 98, double, cBoth, kAny, kRm), ARR(w, 0, kNw, double, cBoth, kAny, kRm),
    ARR(done, 0, 1, int32_t, cBoth, kAny, 0), ARR(nlog, 0, 1, int32_t, cBoth, kAny, 0),
    ARR(metrics, 8, 8, double, cBoth, kLm, 0),
    ARR(log_pos_err, 0, 2, double, cEpisode, kAny, 0), ARR(log_pos_err_norm, 0, 1, double, cEpisode, kAny, 0),
    ARR(log_u_cmd, 0, 2, double, cEpisode, kAny, 0), ARR(log_timestep, 0, 1, double, cEpisode, kAny, 0),
    ARR(log_x, 0, 4, double, cStep, kAny, 0), ARR(log_theta, 0, 14, double, cStep, kAny, 0),
    ARR(log_r_v, 0, 4, double, cStep, kAny, 0), ARR(log_f, 0, 1, double, cStep, kAny, 0),
    ARR(log_X, 6, 0, double, cStep, kAny, 0), ARR(log_U, 2, 0, double, cStep, kAny, 0), ARR(log_quat, 4, 0, double, cStep, kAny, 0),
    ARR(log_loss, 1, 0, double, cStep, kAny, 0),
    ARR(log_status, 1, 1, int32_t, cStep, kAny, 0), ARR(log_iters, 1, 1, int32_t, cStep, kAny, 0),
    ARR(log_rot, 4, 4, double, cStep, kLm, 0),
};
#undef ARR
constexpr int kLoopArrays = sizeof kLoopArr / sizeof kLoopArr[0];

// (every member of LoopBuf is an object pointer)
void*& member(LoopBuf& d, const LoopArr& a) { return *reinterpret_cast<void**>(reinterpret_cast<char*>(&d) + a.member); }
const void* member(const LoopBuf& d, const LoopArr& a) {
    return *reinterpret_cast<void* const*>(reinterpret_cast<const char*>(&d) + a.member);
}

// elements per instance of `a` in the loop `bit`; 0: not an array of that loop
size_t loop_width(const LoopArr& a, uint8_t bit, size_t nw) {
    const int w = !(a.plants & bit) ? 0 : (bit & kRm) ? a.wr : a.wp;
    return w == kNw ? nw : w == kNxPlant ? ((bit & kLm) ? 8 : 6) : (size_t)w;
}

// Every argument check of the PMPC / RMPC loop entries, host and device forms alike (`step`: a loop-step entry, which
// does not take the arrays that only the solve reads).  LMPC plant: *logs is 1 with every log given, 0 in
// metrics-only mode (every log null, log_rows not consulted), and mu_c / v_c of the plant config are not used, as
// in the LMPC loop.  Tray plant: every log is required.
int loop_buf_check(dart_mpc_handle* h, int variant, bool lm, const dart_plant_config* plant, const dart_rmpc_loop_config* c,
               int B, int k, int steps, int log_rows, const LoopBuf& p, bool step, int* logs) {
    if (h->cfg.variant != variant) return fail(h, DART_MPC_EINVAL, variant_text(variant));
    if (!plant) return fail(h, DART_MPC_EINVAL, "null plant config");
    if (!lm && (!(plant->v_c > 0.0) || !(plant->mu_c >= 0.0)))
        return fail(h, DART_MPC_EINVAL, "plant config: v_c > 0, mu_c >= 0");
    const bool rm = variant == DART_MPC_RMPC;
    if (rm) {
        if (!c) return fail(h, DART_MPC_EINVAL, "null loop config");
        if (!(c->rls_lambda > 0.0) || !(c->dr_max >= 0.0) || !(c->step_fraction >= 0.0 && c->step_fraction <= 1.0))
            return fail(h, DART_MPC_EINVAL, "loop config: rls_lambda > 0, dr_max >= 0, 0 <= step_fraction <= 1");
    }
    if (B < 0 || k < 0 || steps < 0 || log_rows < 0) return fail(h, DART_MPC_EINVAL, "negative batch, step or row count");
    if (B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "batch larger than B_max");
    const uint8_t bit = loop_bit(rm, lm);
    int given = 0, absent = 0;
    for (const LoopArr& a : kLoopArr) {
        if (!loop_width(a, bit, 1) || (step && (a.solve_only & bit))) continue;
        const bool log = a.kind == cEpisode || a.kind == cStep;
        if (!member(p, a) && !(log && lm)) return fail(h, DART_MPC_EINVAL, "null pointer");
        if (log) ++(member(p, a) ? given : absent);
    }
    if (given && absent) return fail(h, DART_MPC_EINVAL, "null and non-null log pointers (metrics-only mode: every log null)");
    if (given && (long long)k + steps > log_rows) return fail(h, DART_MPC_EINVAL, "k0 + steps exceeds log_rows");
    *logs = given ? 1 : 0;
    return DART_MPC_OK;
}

// one loop-step launch (the checks made)
int loop_step(dart_mpc_handle* h, bool rm, bool lm, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
              int B, int k, int do_post, int do_pre, int log_rows, int logs, const LoopBuf& p, const LoopIo& io,
              void* stream) {
    if (B == 0 || (!do_post && !do_pre)) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    const dartmpc::PlantArgs pa = plant_args(h, plant);
    if (rm) {
        dartmpc::RmpcLoopArgs a;
        a.B = B; a.N = h->cfg.N; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
        a.logs = logs; a.plant = pa; a.a_lag = pa.a_lag;
        a.Ts = h->cfg.Ts; a.dr_max = loop->dr_max; a.alpha_rg = loop->alpha_rg; a.step_fraction = loop->step_fraction;
        a.pos_tol = loop->pos_tol;
        a.target = p.target; a.prm = p.prm; a.mu = p.mu; a.plant_pvec = p.plant_pvec;
        a.x = p.x; a.tilt = p.tilt; a.prev = p.prev; a.u_prev = p.u_prev; a.r_v = p.r_v; a.theta = p.theta;
        a.done = p.done; a.nlog = p.nlog; a.metrics = p.metrics;
        a.x0 = io.x0; a.Rref = io.Rref; a.phi = io.phi; a.y = io.y; a.u0 = io.u0; a.f = io.f; a.status = io.status;
        a.iters = io.iters;
        a.log_pos_err = p.log_pos_err; a.log_pos_err_norm = p.log_pos_err_norm; a.log_u_cmd = p.log_u_cmd;
        a.log_timestep = p.log_timestep; a.log_x = p.log_x; a.log_theta = p.log_theta; a.log_r_v = p.log_r_v;
        a.log_f = p.log_f; a.log_status = p.log_status; a.log_iters = p.log_iters; a.log_rot = p.log_rot;
        HIPCHK(h, dartmpc_launch_rmpc_loop(&a, lm, stream_of(h, stream)), "loop-step kernel launch");
    } else {
        dartmpc::PmpcLoopArgs a;
        a.B = B; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows; a.logs = logs;
        a.plant = pa; a.a_lag = pa.a_lag; a.Ts = h->cfg.Ts;
        a.prm = p.prm; a.target = p.target; a.plant_pvec = p.plant_pvec; a.pz_vz = p.pz_vz; a.x = p.x; a.tilt = p.tilt;
        a.metrics = p.metrics; a.x0 = io.x0; a.u0 = io.u0; a.f = io.f; a.status = io.status; a.iters = io.iters;
        a.log_X = p.log_X; a.log_U = p.log_U; a.log_quat = p.log_quat; a.log_loss = p.log_loss;
        a.log_status = p.log_status; a.log_iters = p.log_iters; a.log_rot = p.log_rot;
        HIPCHK(h, dartmpc_launch_pmpc_loop(&a, lm, stream_of(h, stream)), "loop-step kernel launch");
    }
    return DART_MPC_OK;
}

// a loop-step entry: the checks of the buffer and of the solve's per-step arrays, then the launch
int loop_step_entry(dart_mpc_handle* h, int variant, bool lm, const dart_plant_config* plant,
                    const dart_rmpc_loop_config* loop, int B, int k, int do_post, int do_pre, int log_rows,
                    const LoopBuf& p, const LoopIo& io, void* stream) {
    int logs = 0;
    if (int rc = loop_buf_check(h, variant, lm, plant, loop, B, k, do_post ? 1 : 0, log_rows, p, true, &logs)) return rc;
    const bool rm = variant == DART_MPC_RMPC;
    if (any_null({io.x0, io.u0, io.f, io.status, io.iters}) || (rm && any_null({io.Rref, io.phi, io.y})))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    return loop_step(h, rm, lm, plant, loop, B, k, do_post, do_pre, log_rows, logs, p, io, stream);
}

// the closed loop on device pointers, the handle's lock held: every check, then the launches (RMPC warm-started in
// place with the fused RLS, PMPC cold-started)
int closed_loop(dart_mpc_handle* h, int variant, bool lm, const dart_plant_config* plant,
                const dart_rmpc_loop_config* loop, int B, int k0, int steps, int log_rows, const LoopBuf& p, void* stream) {
    int logs = 0;
    if (int rc = loop_buf_check(h, variant, lm, plant, loop, B, k0, steps, log_rows, p, false, &logs)) return rc;
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    const bool rm = variant == DART_MPC_RMPC;
    LoopIo L;
    if (int rc = loop_scratch(h, L)) return rc;
    void* s = stream_of(h, stream);
    auto step = [&](int k, int post, int pre) {
        return loop_step(h, rm, lm, plant, loop, B, k, post, pre, log_rows, logs, p, L, s);
    };
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        // RMPC's warm start in place: every element of w's row is read (at the solve's start) and written (at its
        // end) by the same wave, and an instance handed to the restoration kernel has not written its row
        const int rc = rm ? dart_rmpc_solve_batch_dev(h, B, L.x0, p.u_prev, p.theta, p.P, L.phi, L.y, loop->rls_lambda, L.Rref,
                                                      p.prm, p.w, L.u0, L.f, p.w, L.status, L.iters, s)
                          : dart_mpc_solve_batch_dev(h, B, L.x0, p.target, p.prm, nullptr, L.u0, L.f, nullptr, L.status,
                                                     L.iters, s);
        if (rc) return rc;
        if (int rc2 = step(k0 + j, 1, j + 1 < steps)) return rc2;
    }
    return DART_MPC_OK;
}

// the host form: the arrays of `p` staged into the handle's arena around closed_loop; in metrics-only mode no log
// is laid out or moved
int closed_loop_host(dart_mpc_handle* h, int variant, bool lm, const dart_plant_config* plant,
                     const dart_rmpc_loop_config* loop, int B, int k0, int steps, int log_rows, const LoopBuf& p,
                     void* stream) {
    int logs = 0;
    if (int rc = loop_buf_check(h, variant, lm, plant, loop, B, k0, steps, log_rows, p, false, &logs)) return rc;
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    const bool rm = variant == DART_MPC_RMPC;
    if (!rm)
        if (int rc = settle_pending(h)) return rc;
    hipStream_t s = stream_of(h, stream);
    const size_t nB = (size_t)B, nw = rm ? (size_t)dart_rmpc_nw(h->cfg.N) : 0;
    const size_t R = (size_t)log_rows, r0 = (size_t)k0, r1 = (size_t)k0 + steps;
    // episode rows: an instance writes rows nlog[b] .. nlog[b] + steps - 1 at most
    int e0 = log_rows, e1 = 0;
    if (rm && logs) {
        for (int b = 0; b < B; ++b) {
            if (p.nlog[b] < 0) return fail(h, DART_MPC_EINVAL, "negative nlog");
            e0 = p.nlog[b] < e0 ? p.nlog[b] : e0;
            e1 = p.nlog[b] > e1 ? p.nlog[b] : e1;
        }
        e1 = (long long)e1 + steps < log_rows ? e1 + steps : log_rows;
        e0 = e0 < e1 ? e0 : e1;
    }
    RollStage S;
    int idx[kLoopArrays];
    for (int i = 0; i < kLoopArrays; ++i) {
        const LoopArr& a = kLoopArr[i];
        const size_t row = loop_width(a, loop_bit(rm, lm), nw) * a.size * nB;
        idx[i] = -1;
        if (!row) continue;
        switch (a.kind) {
        case cUp: idx[i] = S.add(member(p, a), row, false); break;
        case cBoth: idx[i] = S.add(member(p, a), row, true); break;
        case cEpisode: if (logs) idx[i] = S.add_log(const_cast<void*>(member(p, a)), R, row, e0, e1, true); break;
        case cStep: if (logs) idx[i] = S.add_log(const_cast<void*>(member(p, a)), R, row, r0, r1, false); break;
        }
    }
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    LoopBuf d{};
    for (int i = 0; i < kLoopArrays; ++i) member(d, kLoopArr[i]) = S.dev<char>(h, idx[i]);
    if (int rc = closed_loop(h, variant, lm, plant, loop, B, k0, steps, log_rows, d, s)) return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

// (the tray plant's entries leave plant_pvec, pz_vz, metrics and log_rot null, the LMPC plant's mu)
LoopBuf pmpc_buf(const double* target, const double* prm, const double* plant_pvec, const double* pz_vz, double* x,
                 double* tilt, double* metrics, double* log_X, double* log_U, double* log_quat, double* log_loss,
                 int32_t* log_status, int32_t* log_iters, double* log_rot) {
    LoopBuf p{};
    p.target = target; p.prm = prm; p.plant_pvec = plant_pvec; p.pz_vz = pz_vz; p.x = x; p.tilt = tilt;
    p.metrics = metrics; p.log_X = log_X; p.log_U = log_U; p.log_quat = log_quat; p.log_loss = log_loss;
    p.log_status = log_status; p.log_iters = log_iters; p.log_rot = log_rot;
    return p;
}

LoopBuf rmpc_buf(const double* target, const double* prm, const double* mu, const double* plant_pvec, double* x,
                 double* tilt, double* prev, double* u_prev, double* r_v, double* theta, double* P, double* w,
                 int32_t* done, int32_t* nlog, double* metrics, double* log_pos_err, double* log_pos_err_norm,
                 double* log_u_cmd, double* log_timestep, double* log_x, double* log_theta, double* log_r_v,
                 double* log_f, int32_t* log_status, int32_t* log_iters, double* log_rot) {
    LoopBuf p{};
    p.target = target; p.prm = prm; p.mu = mu; p.plant_pvec = plant_pvec; p.x = x; p.tilt = tilt; p.prev = prev;
    p.u_prev = u_prev; p.r_v = r_v; p.theta = theta; p.P = P; p.w = w; p.done = done; p.nlog = nlog; p.metrics = metrics;
    p.log_pos_err = log_pos_err; p.log_pos_err_norm = log_pos_err_norm; p.log_u_cmd = log_u_cmd;
    p.log_timestep = log_timestep; p.log_x = log_x; p.log_theta = log_theta; p.log_r_v = log_r_v; p.log_f = log_f;
    p.log_status = log_status; p.log_iters = log_iters; p.log_rot = log_rot;
    return p;
}

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
    DART_ENTER(h, -1);
    return loop_step_entry(h, DART_MPC_RMPC, false, plant, loop, B, k, do_post, do_pre, log_rows,
                           rmpc_buf(target, prm, mu, nullptr, x, tilt, prev, u_prev, r_v, mut(theta), nullptr, nullptr, done,
                                    nlog, nullptr, log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep, log_x, log_theta,
                                    log_r_v, log_f, log_status, log_iters, nullptr),
                           {x0, Rref, phi, y, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

int dart_pmpc_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                            int B, int k, int do_post, int do_pre, int log_rows, const double* prm,
                            double* x, double* tilt, double* x0,
                            const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                            double* log_X, double* log_U, double* log_quat, double* log_loss,
                            int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    return loop_step_entry(h, DART_MPC_PMPC, false, plant, nullptr, B, k, do_post, do_pre, log_rows,
                           pmpc_buf(nullptr, prm, nullptr, nullptr, x, tilt, nullptr, log_X, log_U, log_quat, log_loss,
                                    log_status, log_iters, nullptr),
                           {x0, nullptr, nullptr, nullptr, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

int dart_rmpc_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                          int B, int k0, int steps, int log_rows,
                          const double* target, const double* prm, const double* mu,
                          double* x, double* tilt, double* prev, double* u_prev, double* r_v, double* theta,
                          double* P, double* w, int32_t* done, int32_t* nlog,
                          double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                          double* log_x, double* log_theta, double* log_r_v, double* log_f,
                          int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop(h, DART_MPC_RMPC, false, plant, loop, B, k0, steps, log_rows,
                       rmpc_buf(target, prm, mu, nullptr, x, tilt, prev, u_prev, r_v, theta, P, w, done, nlog, nullptr,
                                log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep, log_x, log_theta, log_r_v, log_f,
                                log_status, log_iters, nullptr), stream);
}

int dart_pmpc_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                          int B, int k0, int steps, int log_rows, const double* target, const double* prm,
                          double* x, double* tilt,
                          double* log_X, double* log_U, double* log_quat, double* log_loss,
                          int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop(h, DART_MPC_PMPC, false, plant, nullptr, B, k0, steps, log_rows,
                       pmpc_buf(target, prm, nullptr, nullptr, x, tilt, nullptr, log_X, log_U, log_quat, log_loss,
                                log_status, log_iters, nullptr), stream);
}

int dart_rmpc_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                      int B, int k0, int steps, int log_rows,
                      const double* target, const double* prm, const double* mu,
                      double* x, double* tilt, double* prev, double* u_prev, double* r_v, double* theta,
                      double* P, double* w, int32_t* done, int32_t* nlog,
                      double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                      double* log_x, double* log_theta, double* log_r_v, double* log_f,
                      int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop_host(h, DART_MPC_RMPC, false, plant, loop, B, k0, steps, log_rows,
                            rmpc_buf(target, prm, mu, nullptr, x, tilt, prev, u_prev, r_v, theta, P, w, done, nlog, nullptr,
                                     log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep, log_x, log_theta, log_r_v,
                                     log_f, log_status, log_iters, nullptr), stream);
}

int dart_pmpc_rollout(dart_mpc_handle* h, const dart_plant_config* plant,
                      int B, int k0, int steps, int log_rows, const double* target, const double* prm,
                      double* x, double* tilt,
                      double* log_X, double* log_U, double* log_quat, double* log_loss,
                      int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop_host(h, DART_MPC_PMPC, false, plant, nullptr, B, k0, steps, log_rows,
                            pmpc_buf(target, prm, nullptr, nullptr, x, tilt, nullptr, log_X, log_U, log_quat, log_loss,
                                     log_status, log_iters, nullptr), stream);
}

int dart_pmpc_lm_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                               int B, int k, int do_post, int do_pre, int log_rows,
                               const double* target, const double* plant_pvec, const double* pz_vz,
                               double* x, double* tilt, double* metrics, double* x0,
                               const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                               double* log_X, double* log_U, double* log_quat, double* log_loss,
                               int32_t* log_status, int32_t* log_iters, double* log_rot, void* stream) {
    DART_ENTER(h, -1);
    return loop_step_entry(h, DART_MPC_PMPC, true, plant, nullptr, B, k, do_post, do_pre, log_rows,
                           pmpc_buf(target, nullptr, plant_pvec, pz_vz, x, tilt, metrics, log_X, log_U, log_quat, log_loss,
                                    log_status, log_iters, log_rot),
                           {x0, nullptr, nullptr, nullptr, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

int dart_rmpc_lm_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                               int B, int k, int do_post, int do_pre, int log_rows,
                               const double* target, const double* prm, const double* plant_pvec,
                               double* x, double* tilt, double* prev, double* u_prev, double* r_v, const double* theta,
                               int32_t* done, int32_t* nlog, double* metrics,
                               double* x0, double* Rref, double* phi, double* y,
                               const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                               double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                               double* log_x, double* log_theta, double* log_r_v, double* log_f,
                               int32_t* log_status, int32_t* log_iters, double* log_rot, void* stream) {
    DART_ENTER(h, -1);
    return loop_step_entry(h, DART_MPC_RMPC, true, plant, loop, B, k, do_post, do_pre, log_rows,
                           rmpc_buf(target, prm, nullptr, plant_pvec, x, tilt, prev, u_prev, r_v, mut(theta), nullptr,
                                    nullptr, done, nlog, metrics, log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep,
                                    log_x, log_theta, log_r_v, log_f, log_status, log_iters, log_rot),
                           {x0, Rref, phi, y, mut(u0), mut(f), mut(status), mut(iters)}, stream);
}

int dart_pmpc_lm_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                             int B, int k0, int steps, int log_rows,
                             const double* target, const double* prm, const double* plant_pvec, const double* pz_vz,
                             double* x, double* tilt, double* metrics,
                             double* log_X, double* log_U, double* log_quat, double* log_loss,
                             int32_t* log_status, int32_t* log_iters, double* log_rot, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop(h, DART_MPC_PMPC, true, plant, nullptr, B, k0, steps, log_rows,
                       pmpc_buf(target, prm, plant_pvec, pz_vz, x, tilt, metrics, log_X, log_U, log_quat, log_loss,
                                log_status, log_iters, log_rot), stream);
}

int dart_pmpc_lm_rollout(dart_mpc_handle* h, const dart_plant_config* plant,
                         int B, int k0, int steps, int log_rows,
                         const double* target, const double* prm, const double* plant_pvec, const double* pz_vz,
                         double* x, double* tilt, double* metrics,
                         double* log_X, double* log_U, double* log_quat, double* log_loss,
                         int32_t* log_status, int32_t* log_iters, double* log_rot, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop_host(h, DART_MPC_PMPC, true, plant, nullptr, B, k0, steps, log_rows,
                            pmpc_buf(target, prm, plant_pvec, pz_vz, x, tilt, metrics, log_X, log_U, log_quat, log_loss,
                                     log_status, log_iters, log_rot), stream);
}

int dart_rmpc_lm_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                             int B, int k0, int steps, int log_rows,
                             const double* target, const double* prm, const double* plant_pvec,
                             double* x, double* tilt, double* prev, double* u_prev, double* r_v, double* theta,
                             double* P, double* w, int32_t* done, int32_t* nlog, double* metrics,
                             double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                             double* log_x, double* log_theta, double* log_r_v, double* log_f,
                             int32_t* log_status, int32_t* log_iters, double* log_rot, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop(h, DART_MPC_RMPC, true, plant, loop, B, k0, steps, log_rows,
                       rmpc_buf(target, prm, nullptr, plant_pvec, x, tilt, prev, u_prev, r_v, theta, P, w, done, nlog,
                                metrics, log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep, log_x, log_theta, log_r_v,
                                log_f, log_status, log_iters, log_rot), stream);
}

int dart_rmpc_lm_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_rmpc_loop_config* loop,
                         int B, int k0, int steps, int log_rows,
                         const double* target, const double* prm, const double* plant_pvec,
                         double* x, double* tilt, double* prev, double* u_prev, double* r_v, double* theta,
                         double* P, double* w, int32_t* done, int32_t* nlog, double* metrics,
                         double* log_pos_err, double* log_pos_err_norm, double* log_u_cmd, double* log_timestep,
                         double* log_x, double* log_theta, double* log_r_v, double* log_f,
                         int32_t* log_status, int32_t* log_iters, double* log_rot, void* stream) {
    DART_ENTER(h, -1);
    return closed_loop_host(h, DART_MPC_RMPC, true, plant, loop, B, k0, steps, log_rows,
                            rmpc_buf(target, prm, nullptr, plant_pvec, x, tilt, prev, u_prev, r_v, theta, P, w, done, nlog,
                                     metrics, log_pos_err, log_pos_err_norm, log_u_cmd, log_timestep, log_x, log_theta,
                                     log_r_v, log_f, log_status, log_iters, log_rot), stream);
}

// ---------------------------------------------------------------------------------------------
// LMPC closed loop (lmpc_loop_kernel between the unchanged policy + solve launches), with or without experience
// collection.  The entries build one dart_lmpc_train_buffers from their positional arguments; everything below
// the entries takes that.

// every array of the LMPC closed loop, once, in the order the host entries lay the arena out
#define ARR(member, width, type, kind, group) {offsetof(dart_lmpc_train_buffers, member), width, sizeof(type), kind, group}
static const LmpcArr kLmpcArr[] = {
    ARR(target, kNx, double, kBothCollect, kLoop), ARR(prm, dartmpc::LM_NPRM, double, kUp, kLoop),
    ARR(plant_pvec, kAct, double, kBothCollect, kLoop),
    ARR(x, kNx, double, kBoth, kLoop), ARR(tilt, 2, double, kBoth, kLoop), ARR(u_prev, kNu, double, kBoth, kLoop),
    ARR(w, -1, double, kBoth, kLoop), ARR(model_params, kAct, double, kBoth, kLoop),
    ARR(current_k, kAct, double, kBothTrain, kPolicy), ARR(weights, DART_LMPC_POLICY_NWEIGHTS, float, kNet, kPolicy),
    ARR(critic, DART_LMPC_CRITIC_NWEIGHTS, float, kNet, kCollect),
    ARR(obs_mean, kObs, double, kBoth, kPolicy), ARR(obs_M2, kObs, double, kBoth, kPolicy),
    ARR(obs_count, 1, int32_t, kBoth, kPolicy), ARR(history, kHist, float, kBoth, kPolicy),
    ARR(timestep, 1, int32_t, kBoth, kPolicy),
    ARR(prev_cmd, kNu, double, kBoth, kCollect), ARR(control_seen, kNu, double, kBoth, kCollect),
    ARR(ep_step, 1, int32_t, kBoth, kCollect), ARR(ep_return, 1, double, kBoth, kCollect),
    ARR(time_penalty, 1, double, kBoth, kCollect), ARR(episodes, 1, int32_t, kBoth, kCollect),
    ARR(last_return, 1, double, kBoth, kCollect), ARR(last_steps, 1, int32_t, kBoth, kCollect),
    ARR(nrec, 1, int32_t, kBoth, kCollect), ARR(sticky, 1, int32_t, kBoth, kCollect),
    ARR(reset_x, kNx, double, kPool, kCollect), ARR(reset_target, kNx, double, kPool, kCollect),
    ARR(reset_pvec, kAct, double, kPool, kCollect),
    ARR(log_X, kNx, double, kLog, kLoop), ARR(log_U, kNu, double, kLog, kLoop), ARR(log_pos_error, 1, double, kLog, kLoop),
    ARR(log_pvec, kAct, double, kLog, kLoop), ARR(log_loss, 1, double, kLog, kLoop),
    ARR(log_status, 1, int32_t, kLog, kLoop), ARR(log_iters, 1, int32_t, kLog, kLoop),
    ARR(log_reward, 1, double, kLog, kCollect), ARR(log_done, 1, int32_t, kLog, kCollect),
    ARR(log_value, 1, float, kLog, kCollect), ARR(log_logp, 1, float, kLog, kCollect),
    ARR(rec_obs, kHist, float, kRec, kCollect), ARR(rec_action, kAct, float, kRec, kCollect),
    ARR(rec_logp, 1, float, kRec, kCollect), ARR(rec_value, 1, float, kRec, kCollect),
    ARR(rec_reward, 1, double, kRec, kCollect), ARR(rec_done, 1, float, kRec, kCollect),
    ARR(adam, 2 * dartmpc::kPpoParams, float, kCall, kTrain), ARR(adam_step, 1, int32_t, kCall, kTrain),
    ARR(best_return, 1, double, kCall, kTrain), ARR(best_weights, dartmpc::kPpoParams, float, kCall, kTrain),
    ARR(best_iter, 1, int32_t, kCall, kTrain),
};
#undef ARR
static_assert(sizeof kLmpcArr / sizeof kLmpcArr[0] == kLmpcArrays, "kLmpcArrays counts the table's rows");

namespace {

// (every member of dart_lmpc_train_buffers is an object pointer)
void*& member(dart_lmpc_train_buffers& d, const LmpcArr& a) {
    return *reinterpret_cast<void**>(reinterpret_cast<char*>(&d) + a.member);
}
const void* member(const dart_lmpc_train_buffers& d, const LmpcArr& a) {
    return *reinterpret_cast<void* const*>(reinterpret_cast<const char*>(&d) + a.member);
}

}  // namespace

bool lmpc_null(const dart_lmpc_train_buffers& p, int group, int kind) {
    for (const LmpcArr& a : kLmpcArr) {
        const bool apart = a.kind == kRec || a.kind == kPool;
        if (a.group == group && a.kind != kNet && (kind == kAnyState ? !apart : a.kind == kind) && !member(p, a))
            return true;
    }
    return false;
}

void lmpc_stage(RollStage& S, const dart_lmpc_train_buffers& host, const LmpcStagePlan& m, int idx[kLmpcArrays]) {
    for (int i = 0; i < kLmpcArrays; ++i) {
        const LmpcArr& a = kLmpcArr[i];
        idx[i] = -1;
        if ((a.group == kPolicy && !m.policy) || (a.group == kCollect && !m.collect) || (a.group == kTrain && !m.train))
            continue;
        const void* p = member(host, a);
        // [width]; a population's: [learners][width], the critics kPopCriticStride apart
        const bool is_critic = a.member == offsetof(dart_lmpc_train_buffers, critic);
        const size_t call = m.learners ? m.learners * (is_critic ? dartmpc::kPopCriticStride : (size_t)a.width) * a.size
                                       : (size_t)a.width * a.size;
        const size_t row = (a.width < 0 ? m.nw : (size_t)a.width) * a.size * m.B;       // [B][width]
        switch (a.kind) {
        case kUp: idx[i] = S.add(p, row, false); break;
        case kBoth: idx[i] = S.add(p, row, true); break;
        case kBothCollect: idx[i] = S.add(p, row, m.collect); break;
        case kBothTrain: idx[i] = S.add(p, row, m.train); break;
        case kNet: idx[i] = S.add(p, call, m.train); break;
        case kCall: idx[i] = S.add(p, call, true); break;
        case kLog:
            if (!(m.no_logs && a.group == kLoop)) idx[i] = S.add_rows(p, m.log_rows, row, m.r0, m.r1, false, true);
            break;
        // (collection: both ways, since an instance that records less leaves its entries of the rows untouched)
        case kRec: if (m.rec_rows) idx[i] = S.add_rows(p, m.rec_rows, row, m.q0, m.q1, !m.train, true); break;
        case kPool: if (m.reset_rows) idx[i] = S.add(p, m.reset_rows * row, false); break;
        }
    }
}

void lmpc_bind(const RollStage& S, const dart_mpc_handle* h, const int idx[kLmpcArrays], dart_lmpc_train_buffers& dev) {
    for (int i = 0; i < kLmpcArrays; ++i) member(dev, kLmpcArr[i]) = S.dev<char>(h, idx[i]);
}

namespace {

// the solve's per-step arrays of an LMPC rollout, the two warm-start buffers the solves alternate between, and
// one zeroed noise row
struct LmpcLoopScratch {
    double *state, *u0, *f, *wbuf[2];
    int32_t *status, *iters;
    float* zero_noise;
};

int lmpc_loop_scratch(dart_mpc_handle* h, LmpcLoopScratch& L) {
    const size_t nw = (size_t)dart_lmpc_nw(h->cfg.N);
    const size_t cnt[8] = {8 * kNx, 8 * kNu, 8, 8 * nw, 8 * nw, 4, 4, 4 * kAct};
    char* p[8];
    // (only the noise row needs a value: pre writes what the solve reads, the solve what post reads)
    if (int rc = scratch_blocks(h, 8, cnt, 7, p)) return rc;
    L.state = (double*)p[0]; L.u0 = (double*)p[1]; L.f = (double*)p[2]; L.wbuf[0] = (double*)p[3];
    L.wbuf[1] = (double*)p[4]; L.status = (int32_t*)p[5]; L.iters = (int32_t*)p[6]; L.zero_noise = (float*)p[7];
    return DART_MPC_OK;
}

// the configuration half of the experience launch's arguments, checked (after loop_check)
int experience_cfg(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg, const dart_lmpc_reward_config* r, int B,
                   int rec_rows, int reset_rows, const float* weights, const float* critic,
                   dartmpc::ExperienceArgs& a) {
    if (!weights) return fail(h, DART_MPC_EINVAL, "experience collection needs a policy (null weights)");
    if (!critic) return fail(h, DART_MPC_EINVAL, "null critic weights");
    // (the experience kernel reads layer 1 of both nets with 16-byte loads)
    if (!aligned16(weights) || !aligned16(critic))
        return fail(h, DART_MPC_EINVAL, "policy and critic weights must be 16-byte aligned");
    dartmpc::PolicyArgs pa;
    if (policy_args(pcfg, B, weights, pa) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
    if (!r) return fail(h, DART_MPC_EINVAL, "null reward config");
    if (r->record_every < 1 || !(r->sigma_pos > 0.0) || !(r->sigma_vel > 0.0))
        return fail(h, DART_MPC_EINVAL, "reward config: record_every >= 1, sigma_pos > 0, sigma_vel > 0");
    if (rec_rows < 0 || reset_rows < 0) return fail(h, DART_MPC_EINVAL, "negative rec_rows or reset_rows");
    a.B = B; a.rec_rows = rec_rows; a.reset_rows = reset_rows; a.learner_B = 0;
    a.w = pa.w;
    a.c = critic_weights(critic);
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

// (after experience_cfg) the pointer half: the null checks of the collection's groups, then the fields of `a` that
// the view holds (the caller sets k, action, state and mean_out)
int experience_ptrs(dart_mpc_handle* h, int rec_rows, int reset_rows, const dart_lmpc_train_buffers& p,
                    dartmpc::ExperienceArgs& a) {
    if (lmpc_null(p, kCollect)) return fail(h, DART_MPC_EINVAL, "null pointer (collection state or logs)");
    if (rec_rows > 0 && lmpc_null(p, kCollect, kRec)) return fail(h, DART_MPC_EINVAL, "null pointer (records)");
    if (reset_rows > 0 && lmpc_null(p, kCollect, kPool))
        return fail(h, DART_MPC_EINVAL, "reset_rows > 0 with a null reset pool");
    a.history = p.history; a.log_X = p.log_X; a.timestep = p.timestep; a.u_prev = p.u_prev;
    a.target = p.target; a.plant_pvec = p.plant_pvec; a.x = p.x; a.tilt = p.tilt;
    a.prev_cmd = p.prev_cmd; a.control_seen = p.control_seen; a.ep_step = p.ep_step; a.ep_return = p.ep_return;
    a.time_penalty = p.time_penalty; a.episodes = p.episodes; a.last_return = p.last_return;
    a.last_steps = p.last_steps; a.nrec = p.nrec; a.sticky = p.sticky;
    a.reset_x = p.reset_x; a.reset_target = p.reset_target; a.reset_pvec = p.reset_pvec;
    a.log_reward = p.log_reward; a.log_done = p.log_done; a.log_value = p.log_value; a.log_logp = p.log_logp;
    a.rec_obs = p.rec_obs; a.rec_action = p.rec_action; a.rec_logp = p.rec_logp; a.rec_value = p.rec_value;
    a.rec_reward = p.rec_reward; a.rec_done = p.rec_done;
    return DART_MPC_OK;
}

// the loop's logs of an evaluation: 1 all given, 0 all null (metrics-only), -1 some of each
int lmpc_logs_given(const dart_lmpc_train_buffers& p) {
    int given = 0, absent = 0;
    for (const LmpcArr& a : kLmpcArr)
        if (a.group == kLoop && a.kind == kLog) ++(member(p, a) ? given : absent);
    return given && absent ? -1 : given ? 1 : 0;
}

// every argument check of the rollout (ea == nullptr), collection and evaluation (ev != nullptr) entries, host and
// device forms alike; a collection's experience arguments are left in *ea
int lmpc_loop_check(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                    const dart_lmpc_reward_config* rcfg, int B, int k0, int steps, int log_rows, int rec_rows,
                    int reset_rows, const dart_lmpc_train_buffers& p, dartmpc::ExperienceArgs* ea,
                    const LmpcEval* ev = nullptr) {
    if (int rc = loop_check(h, plant, B, k0, steps, log_rows)) return rc;
    if (ea)
        if (int rc = experience_cfg(h, pcfg, rcfg, B, rec_rows, reset_rows, p.weights, p.critic, *ea)) return rc;
    if (ev) {
        if (lmpc_logs_given(p) < 0)
            return fail(h, DART_MPC_EINVAL, "null and non-null log pointers (metrics-only mode: every log null)");
        if (!ev->metrics) return fail(h, DART_MPC_EINVAL, "null metrics");
        if (lmpc_null(p, kLoop, kUp) || lmpc_null(p, kLoop, kBoth) || lmpc_null(p, kLoop, kBothCollect))
            return fail(h, DART_MPC_EINVAL, "null pointer");
    } else if (lmpc_null(p, kLoop)) {
        return fail(h, DART_MPC_EINVAL, "null pointer");
    }
    if (p.weights) {
        dartmpc::PolicyArgs chk;
        if (policy_args(pcfg, B, p.weights, chk) != DART_MPC_OK) return fail(h, DART_MPC_EINVAL, "bad policy config");
        if (lmpc_null(p, kPolicy)) return fail(h, DART_MPC_EINVAL, "null pointer (policy state)");
    }
    return ea ? experience_ptrs(h, rec_rows, reset_rows, p, *ea) : DART_MPC_OK;
}

}  // namespace

int dart_lmpc_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                            int B, int k, int do_post, int do_pre, int log_rows,
                            const double* target, const double* plant_pvec,
                            double* x, double* tilt, double* u_prev, const double* model_params, double* state,
                            const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                            double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                            int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    if (int rc = loop_check(h, plant, B, k, do_post ? 1 : 0, log_rows)) return rc;
    if (any_null({target, plant_pvec, x, tilt, u_prev, model_params, state, u0, f, status, iters, log_X, log_U,
                  log_pos_error, log_pvec, log_loss, log_status, log_iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    if (B == 0 || (!do_post && !do_pre)) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::LmpcLoopArgs a;
    a.B = B; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
    a.a_lag = plant_args(h, plant).a_lag;
    a.Ts = h->cfg.Ts;
    a.target = target; a.plant_pvec = plant_pvec; a.x = x; a.tilt = tilt; a.u_prev = u_prev;
    a.model_params = model_params; a.state = state; a.u0 = u0; a.f = f; a.status = status; a.iters = iters;
    a.log_X = log_X; a.log_U = log_U; a.log_pos_error = log_pos_error; a.log_pvec = log_pvec; a.log_loss = log_loss;
    a.log_status = log_status; a.log_iters = log_iters;
    HIPCHK(h, dartmpc_launch_lmpc_loop(&a, stream_of(h, stream)), "loop-step kernel launch");
    return DART_MPC_OK;
}

namespace {

// one launch of the evaluation's loop step, the checks made (lg: the seven logs, all set or all null)
int lmpc_eval_step(dart_mpc_handle* h, const dart_plant_config* plant, int B, int k, int do_post, int do_pre,
                   int log_rows, const double* target, const double* plant_pvec, double* x, double* tilt, double* u_prev,
                   const double* model_params, double* state, const double* u0, const double* f, const int32_t* status,
                   const int32_t* iters, double* metrics, const dart_lmpc_train_buffers& lg, void* stream) {
    if (B == 0 || (!do_post && !do_pre)) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    dartmpc::LmpcEvalLoopArgs e;
    dartmpc::LmpcLoopArgs& a = e.l;
    a.B = B; a.k = k; a.do_post = do_post ? 1 : 0; a.do_pre = do_pre ? 1 : 0; a.log_rows = log_rows;
    a.a_lag = plant_args(h, plant).a_lag;
    a.Ts = h->cfg.Ts;
    a.target = target; a.plant_pvec = plant_pvec; a.x = x; a.tilt = tilt; a.u_prev = u_prev;
    a.model_params = model_params; a.state = state; a.u0 = u0; a.f = f; a.status = status; a.iters = iters;
    a.log_X = lg.log_X; a.log_U = lg.log_U; a.log_pos_error = lg.log_pos_error; a.log_pvec = lg.log_pvec;
    a.log_loss = lg.log_loss; a.log_status = lg.log_status; a.log_iters = lg.log_iters;
    e.logs = lg.log_X ? 1 : 0;
    e.metrics = metrics;
    HIPCHK(h, dartmpc_launch_lmpc_eval_loop(&e, stream_of(h, stream)), "loop-step kernel launch");
    return DART_MPC_OK;
}

}  // namespace

int dart_lmpc_eval_loop_step_dev(dart_mpc_handle* h, const dart_plant_config* plant,
                                 int B, int k, int do_post, int do_pre, int log_rows,
                                 const double* target, const double* plant_pvec,
                                 double* x, double* tilt, double* u_prev, const double* model_params, double* state,
                                 const double* u0, const double* f, const int32_t* status, const int32_t* iters,
                                 double* metrics,
                                 double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                                 int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    if (int rc = loop_check(h, plant, B, k, do_post ? 1 : 0, log_rows)) return rc;
    dart_lmpc_train_buffers lg{};
    lg.log_X = log_X; lg.log_U = log_U; lg.log_pos_error = log_pos_error; lg.log_pvec = log_pvec; lg.log_loss = log_loss;
    lg.log_status = log_status; lg.log_iters = log_iters;
    if (lmpc_logs_given(lg) < 0)
        return fail(h, DART_MPC_EINVAL, "null and non-null log pointers (metrics-only mode: every log null)");
    if (!metrics) return fail(h, DART_MPC_EINVAL, "null metrics");
    if (any_null({target, plant_pvec, x, tilt, u_prev, model_params, state, u0, f, status, iters}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    return lmpc_eval_step(h, plant, B, k, do_post, do_pre, log_rows, target, plant_pvec, x, tilt, u_prev, model_params,
                          state, u0, f, status, iters, metrics, lg, stream);
}

int lmpc_closed_loop(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                     const dart_lmpc_reward_config* rcfg, bool collect, int B, int k0, int steps, int log_rows,
                     int rec_rows, int reset_rows, const dart_lmpc_train_buffers& p, const float* noise, void* stream,
                     int learner_B, const LmpcEval* ev) {
    dartmpc::ExperienceArgs ea;
    if (int rc = lmpc_loop_check(h, plant, pcfg, rcfg, B, k0, steps, log_rows, rec_rows, reset_rows, p,
                                 collect ? &ea : nullptr, ev))
        return rc;
    if (learner_B < 0) return fail(h, DART_MPC_EINVAL, "negative learner block size");
    if (ev && collect) return fail(h, DART_MPC_EINVAL, "an evaluation collects no experience");
    ea.learner_B = learner_B;
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    LmpcLoopScratch L;
    if (int rc = lmpc_loop_scratch(h, L)) return rc;
    if (collect && !h->action_buf)
        HIPCHK(h, hipMalloc((void**)&h->action_buf, sizeof(float) * kAct * (size_t)h->cfg.B_max), "hipMalloc (action buffer)");
    // a collection keeps the policy's action of the step for its experience launch
    float* action = collect ? h->action_buf : nullptr;
    ea.action = action; ea.mean_out = nullptr;
    void* s = stream_of(h, stream);
    auto step = [&](int k, int post, int pre) {
        if (ev)
            return lmpc_eval_step(h, plant, B, k, post, pre, log_rows, p.target, p.plant_pvec, p.x, p.tilt, p.u_prev,
                                  p.model_params, L.state, L.u0, L.f, L.status, L.iters, ev->metrics, p, s);
        return dart_lmpc_loop_step_dev(h, plant, B, k, post, pre, log_rows, p.target, p.plant_pvec, p.x, p.tilt, p.u_prev,
                                       p.model_params, L.state, L.u0, L.f, L.status, L.iters, p.log_X, p.log_U,
                                       p.log_pos_error, p.log_pvec, p.log_loss, p.log_status, p.log_iters, s);
    };
    // Warm start: with the restoration phases on, an instance that <false> hands over has written the iterate of
    // its failed iteration to w_out before lmpc_solve<true> (the tail, or the second launch) redoes the set-up from
    // w_warm, so w_warm == w_out would change the scalings of the resumed solve.  The solves
    // alternate between two handle-owned buffers instead: the first reads the caller's w, the last writes it.
    // Without the restoration phases nothing is handed over and the row is rewritten in place.
    const bool in_place = !h->cfg.restoration;
    if (int rc = step(k0, 0, 1)) return rc;
    for (int j = 0; j < steps; ++j) {
        const double* w_in = (in_place || j == 0) ? p.w : L.wbuf[(j - 1) & 1];
        double* w_out = (in_place || (j == steps - 1 && j > 0)) ? p.w : L.wbuf[j & 1];
        int rc;
        if (p.weights)       // (step k's draws are row k of the noise)
            rc = lmpc_policy_solve_dev(h, pcfg, B, learner_B, p.weights, L.state, p.u_prev, p.target, p.current_k,
                                       p.obs_mean, p.obs_M2, p.obs_count, p.history, p.timestep,
                                       noise ? noise + ((size_t)k0 + j) * B * kAct : L.zero_noise, p.model_params,
                                       action, p.prm, w_in, L.u0, L.f, w_out, L.status, L.iters, s);
        else
            rc = dart_lmpc_solve_batch_dev(h, B, L.state, p.u_prev, p.model_params, p.target, p.prm, w_in, L.u0, L.f,
                                           w_out, L.status, L.iters, s);
        if (rc) return rc;
        if (w_out != p.w && j == steps - 1)       // a one-step call: the iterate back into the caller's w
            HIPCHK(h, hipMemcpyAsync(p.w, w_out, sizeof(double) * (size_t)dart_lmpc_nw(h->cfg.N) * B,
                                     hipMemcpyDeviceToDevice, (hipStream_t)s), "copy w");
        const int pre = j + 1 < steps;
        if ((rc = step(k0 + j, 1, pre))) return rc;
        if (collect) {
            // one experience launch after every post; a reset at the last step of a call is picked up by the next
            // call's pre
            ea.k = k0 + j;
            ea.state = pre ? L.state : nullptr;
            HIPCHK(h, dartmpc_launch_lmpc_experience(&ea, (hipStream_t)s), "experience kernel launch");
        }
    }
    if (ev && ev->scores)
        HIPCHK(h, dartmpc_launch_lmpc_eval_scores(ev->P, B / ev->P, ev->metrics, ev->scores, (hipStream_t)s),
               "score kernel launch");
    return DART_MPC_OK;
}

namespace {

// the host form of the rollout and collection entries: the arrays of `p` staged into the handle's arena around
// lmpc_closed_loop (the step rows [k0, k0 + steps) of the logs and of the noise travel).  An evaluation (ev, host
// pointers): P weight rows go up, the metrics travel both ways, the scores come down, and in metrics-only mode no
// log is laid out or moved
int lmpc_closed_loop_host(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                          const dart_lmpc_reward_config* rcfg, bool collect, int B, int k0, int steps, int log_rows,
                          int rec_rows, int reset_rows, const dart_lmpc_train_buffers& p, const float* noise,
                          void* stream, int learner_B = 0, const LmpcEval* ev = nullptr) {
    dartmpc::ExperienceArgs chk;
    if (int rc = lmpc_loop_check(h, plant, pcfg, rcfg, B, k0, steps, log_rows, rec_rows, reset_rows, p,
                                 collect ? &chk : nullptr, ev))
        return rc;
    if (B == 0 || steps == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    hipStream_t s = stream_of(h, stream);
    LmpcStagePlan m{};
    m.policy = p.weights != nullptr; m.collect = collect;
    m.B = (size_t)B; m.nw = (size_t)dart_lmpc_nw(h->cfg.N);
    m.log_rows = (size_t)log_rows; m.r0 = (size_t)k0; m.r1 = (size_t)k0 + steps;
    m.reset_rows = collect ? (size_t)reset_rows : 0;
    if (ev) {
        m.learners = (size_t)ev->P;
        m.no_logs = lmpc_logs_given(p) == 0;
    }
    if (collect && rec_rows > 0) {
        // record rows: an instance writes rows nrec[b] .. nrec[b] + ceil(steps / record_every) - 1 at most
        long long e0 = rec_rows, e1 = 0;
        for (int b = 0; b < B; ++b) {
            const long long n = p.nrec[b] < 0 ? 0 : p.nrec[b];
            e0 = n < e0 ? n : e0;
            e1 = n > e1 ? n : e1;
        }
        e1 += ((long long)steps + rcfg->record_every - 1) / rcfg->record_every;
        e1 = e1 < rec_rows ? e1 : rec_rows;
        e0 = e0 < e1 ? e0 : e1;
        m.rec_rows = (size_t)rec_rows; m.q0 = (size_t)e0; m.q1 = (size_t)e1;
    }
    RollStage S;
    int idx[kLmpcArrays];
    lmpc_stage(S, p, m, idx);
    const int i_nz = (m.policy && noise) ? S.add_rows(noise, m.log_rows, kAct * m.B * sizeof(float), m.r0, m.r1, true, false)
                                         : -1;
    const int i_met = ev ? S.add(ev->metrics, 8 * sizeof(double) * m.B, true) : -1;
    const int i_sc = (ev && ev->scores) ? S.add_rows(ev->scores, 1, 8 * sizeof(double) * m.learners, 0, 1, false, true) : -1;
    if (int rc = S.reserve(h)) return rc;
    if (int rc = S.upload(h, s)) return rc;
    dart_lmpc_train_buffers d{};
    lmpc_bind(S, h, idx, d);
    LmpcEval dev_ev{S.dev<double>(h, i_met), S.dev<double>(h, i_sc), ev ? ev->P : 0};
    if (int rc = lmpc_closed_loop(h, plant, pcfg, rcfg, collect, B, k0, steps, log_rows, rec_rows, reset_rows, d,
                                  S.dev<float>(h, i_nz), s, learner_B, ev ? &dev_ev : nullptr))
        return rc;
    if (int rc = S.download(h, s)) return rc;
    HIPCHK(h, hipStreamSynchronize(s), "hipStreamSynchronize");
    return DART_MPC_OK;
}

}  // namespace

int dart_lmpc_rollout_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                          int B, int k0, int steps, int log_rows,
                          const double* target, const double* prm, const double* plant_pvec, const double* current_k,
                          const float* weights, const float* noise,
                          double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                          int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                          double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                          int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    // (the view's members in their order, up to model_params)
    dart_lmpc_train_buffers p = {mut(target), prm, mut(plant_pvec), mut(current_k), mut(weights), nullptr, x, tilt, u_prev, w,
                                 obs_mean, obs_M2, obs_count, history, timestep, model_params};
    p.log_X = log_X; p.log_U = log_U; p.log_pos_error = log_pos_error; p.log_pvec = log_pvec; p.log_loss = log_loss;
    p.log_status = log_status; p.log_iters = log_iters;
    return lmpc_closed_loop(h, plant, pcfg, nullptr, false, B, k0, steps, log_rows, 0, 0, p, noise, stream);
}

int dart_lmpc_rollout(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                      int B, int k0, int steps, int log_rows,
                      const double* target, const double* prm, const double* plant_pvec, const double* current_k,
                      const float* weights, const float* noise,
                      double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                      int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                      double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                      int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    // (the view's members in their order, up to model_params)
    dart_lmpc_train_buffers p = {mut(target), prm, mut(plant_pvec), mut(current_k), mut(weights), nullptr, x, tilt, u_prev, w,
                                 obs_mean, obs_M2, obs_count, history, timestep, model_params};
    p.log_X = log_X; p.log_U = log_U; p.log_pos_error = log_pos_error; p.log_pvec = log_pvec; p.log_loss = log_loss;
    p.log_status = log_status; p.log_iters = log_iters;
    return lmpc_closed_loop_host(h, plant, pcfg, nullptr, false, B, k0, steps, log_rows, 0, 0, p, noise, stream);
}

// ---------------------------------------------------------------------------------------------
// LMPC evaluation: the rollout's loop with the metrics kept on the device, logs that may be absent and P weight sets
// in one call (P learners of B instances each, stacked learner-major)
namespace {

// the shape checks of an evaluation, then the closed loop on device (host false) or host pointers
int lmpc_eval(dart_mpc_handle* h, bool host, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg, int P,
              int B, int k0, int steps, int log_rows, const dart_lmpc_train_buffers& p, const float* noise,
              double* metrics, double* scores, void* stream) {
    if (h->cfg.variant != DART_MPC_LMPC) return fail(h, DART_MPC_EINVAL, variant_text(DART_MPC_LMPC));
    if (P < 1 || P > DART_LMPC_POP_MAX) return fail(h, DART_MPC_EINVAL, "population: 1 <= P <= DART_LMPC_POP_MAX");
    if (B < 0) return fail(h, DART_MPC_EINVAL, "negative batch, step or row count");
    if ((long long)P * B > h->cfg.B_max) return fail(h, DART_MPC_EINVAL, "population: P * B larger than B_max");
    const LmpcEval ev{metrics, scores, P};
    // (a population of one runs the single-policy launches)
    const int learner_B = P > 1 ? B : 0;
    return host ? lmpc_closed_loop_host(h, plant, pcfg, nullptr, false, P * B, k0, steps, log_rows, 0, 0, p, noise, stream,
                                        learner_B, &ev)
                : lmpc_closed_loop(h, plant, pcfg, nullptr, false, P * B, k0, steps, log_rows, 0, 0, p, noise, stream,
                                   learner_B, &ev);
}

}  // namespace

int dart_lmpc_eval_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                       int P, int B, int k0, int steps, int log_rows,
                       const double* target, const double* prm, const double* plant_pvec, const double* current_k,
                       const float* weights, const float* noise,
                       double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                       int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                       double* metrics, double* scores,
                       double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                       int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    // (the view's members in their order, up to model_params)
    dart_lmpc_train_buffers p = {mut(target), prm, mut(plant_pvec), mut(current_k), mut(weights), nullptr, x, tilt, u_prev, w,
                                 obs_mean, obs_M2, obs_count, history, timestep, model_params};
    p.log_X = log_X; p.log_U = log_U; p.log_pos_error = log_pos_error; p.log_pvec = log_pvec; p.log_loss = log_loss;
    p.log_status = log_status; p.log_iters = log_iters;
    return lmpc_eval(h, false, plant, pcfg, P, B, k0, steps, log_rows, p, noise, metrics, scores, stream);
}

int dart_lmpc_eval(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                   int P, int B, int k0, int steps, int log_rows,
                   const double* target, const double* prm, const double* plant_pvec, const double* current_k,
                   const float* weights, const float* noise,
                   double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                   int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                   double* metrics, double* scores,
                   double* log_X, double* log_U, double* log_pos_error, double* log_pvec, double* log_loss,
                   int32_t* log_status, int32_t* log_iters, void* stream) {
    DART_ENTER(h, -1);
    // (the view's members in their order, up to model_params)
    dart_lmpc_train_buffers p = {mut(target), prm, mut(plant_pvec), mut(current_k), mut(weights), nullptr, x, tilt, u_prev, w,
                                 obs_mean, obs_M2, obs_count, history, timestep, model_params};
    p.log_X = log_X; p.log_U = log_U; p.log_pos_error = log_pos_error; p.log_pvec = log_pvec; p.log_loss = log_loss;
    p.log_status = log_status; p.log_iters = log_iters;
    return lmpc_eval(h, true, plant, pcfg, P, B, k0, steps, log_rows, p, noise, metrics, scores, stream);
}

namespace {

int eval_scores_check(int P, int B, const double* metrics, const double* scores) {
    return (P < 1 || P > DART_LMPC_POP_MAX || B < 1 || !metrics || !scores) ? DART_MPC_EINVAL : DART_MPC_OK;
}

}  // namespace

int dart_lmpc_eval_scores_dev(int P, int B, const double* metrics, double* scores, void* stream) {
    if (int rc = eval_scores_check(P, B, metrics, scores)) return rc;
    return dartmpc_launch_lmpc_eval_scores(P, B, metrics, scores, (hipStream_t)stream) == hipSuccess ? DART_MPC_OK
                                                                                                     : DART_MPC_EHIP;
}

int dart_lmpc_eval_scores(int P, int B, const double* metrics, double* scores) {
    if (int rc = eval_scores_check(P, B, metrics, scores)) return rc;
    DART_DEVICE_STAGE(D, S);
    const size_t n = 8 * (size_t)P * B;
    if (S.reserve(sizeof(double) * n + 256, sizeof(double) * 8 * P + 256) != hipSuccess) return DART_MPC_EHIP;
    S.begin();
    const double* d_m = S.in(metrics, n);
    double* d_s = S.out<double>(8 * (size_t)P);
    if (!D->run([&](hipStream_t s) { return dartmpc_launch_lmpc_eval_scores(P, B, d_m, d_s, s); })) return DART_MPC_EHIP;
    S.take(scores, d_s, 8 * (size_t)P);
    return DART_MPC_OK;
}

// ---------------------------------------------------------------------------------------------
// LMPC experience collection
void dart_lmpc_reward_config_default(dart_lmpc_reward_config* c) {
    if (!c) return;
    c->sigma_pos = 0.02; c->sigma_vel = 0.02;
    c->w_pos = 40.0; c->w_vel = 0.1; c->w_change = 1e-3; c->w_d_ctrl = 5.0;
    c->success_tol = 0.01; c->success_bonus = 20.0; c->oob_penalty = 20.0;
    c->tray_limit[0] = 0.2; c->tray_limit[1] = 0.15;
    c->max_per_dim_rms = 0.5; c->time_penalty_rate = 1e-4;
    c->max_episode_steps = 20000; c->record_every = 8; c->done_sticky = 0; c->reserved = 0;
}

int dart_lmpc_experience_step_dev(dart_mpc_handle* h, const dart_lmpc_policy_config* pcfg,
                                  const dart_lmpc_reward_config* rcfg, int B, int k, int log_rows, int rec_rows,
                                  int reset_rows, const float* weights, const float* critic, const float* history,
                                  const float* action, const double* log_X, const int32_t* timestep,
                                  const double* u_prev, double* target, double* plant_pvec, double* x, double* tilt,
                                  double* state, double* prev_cmd, double* control_seen, int32_t* ep_step,
                                  double* ep_return, double* time_penalty, int32_t* episodes, double* last_return,
                                  int32_t* last_steps, int32_t* nrec, int32_t* sticky, const double* reset_x,
                                  const double* reset_target, const double* reset_pvec, double* log_reward,
                                  int32_t* log_done, float* log_value, float* log_logp, float* rec_obs,
                                  float* rec_action, float* rec_logp, float* rec_value, double* rec_reward,
                                  float* rec_done, float* mean_out, void* stream) {
    DART_ENTER(h, DART_MPC_LMPC);
    if (B < 0 || k < 0 || log_rows < 0) return fail(h, DART_MPC_EINVAL, "negative batch, step or row count");
    if (k >= log_rows) return fail(h, DART_MPC_EINVAL, "k exceeds log_rows");
    dartmpc::ExperienceArgs a;
    if (int rc = experience_cfg(h, pcfg, rcfg, B, rec_rows, reset_rows, weights, critic, a)) return rc;
    if (any_null({history, action, log_X, timestep, u_prev, target, plant_pvec, x, tilt}))
        return fail(h, DART_MPC_EINVAL, "null pointer");
    dart_lmpc_train_buffers p{};
    p.history = mut(history); p.log_X = mut(log_X); p.timestep = mut(timestep); p.u_prev = mut(u_prev);
    p.target = target; p.plant_pvec = plant_pvec; p.x = x; p.tilt = tilt;
    p.prev_cmd = prev_cmd; p.control_seen = control_seen; p.ep_step = ep_step; p.ep_return = ep_return;
    p.time_penalty = time_penalty; p.episodes = episodes; p.last_return = last_return; p.last_steps = last_steps;
    p.nrec = nrec; p.sticky = sticky; p.reset_x = reset_x; p.reset_target = reset_target; p.reset_pvec = reset_pvec;
    p.log_reward = log_reward; p.log_done = log_done; p.log_value = log_value; p.log_logp = log_logp;
    p.rec_obs = rec_obs; p.rec_action = rec_action; p.rec_logp = rec_logp; p.rec_value = rec_value;
    p.rec_reward = rec_reward; p.rec_done = rec_done;
    if (int rc = experience_ptrs(h, rec_rows, reset_rows, p, a)) return rc;
    if (B == 0) return DART_MPC_OK;
    HIPCHK(h, hipSetDevice(h->device), "hipSetDevice");
    a.k = k; a.action = action; a.state = state; a.mean_out = mean_out;
    HIPCHK(h, dartmpc_launch_lmpc_experience(&a, stream_of(h, stream)), "experience kernel launch");
    return DART_MPC_OK;
}

int dart_lmpc_collect_dev(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                          const dart_lmpc_reward_config* rcfg, int B, int k0, int steps, int log_rows, int rec_rows,
                          int reset_rows, double* target, const double* prm, double* plant_pvec,
                          const double* current_k, const float* weights, const float* critic, const float* noise,
                          double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                          int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                          double* prev_cmd, double* control_seen, int32_t* ep_step, double* ep_return,
                          double* time_penalty, int32_t* episodes, double* last_return, int32_t* last_steps,
                          int32_t* nrec, int32_t* sticky, const double* reset_x, const double* reset_target,
                          const double* reset_pvec, double* log_X, double* log_U, double* log_pos_error,
                          double* log_pvec, double* log_loss, int32_t* log_status, int32_t* log_iters,
                          double* log_reward, int32_t* log_done, float* log_value, float* log_logp, float* rec_obs,
                          float* rec_action, float* rec_logp, float* rec_value, double* rec_reward, float* rec_done,
                          void* stream) {
    DART_ENTER(h, -1);
    // (the arguments are the view's members in their order, up to rec_done, but for the noise)
    const dart_lmpc_train_buffers p = {
        target, prm, plant_pvec, mut(current_k), mut(weights), mut(critic), x, tilt, u_prev, w, obs_mean, obs_M2, obs_count,
        history, timestep, model_params, prev_cmd, control_seen, ep_step, ep_return, time_penalty, episodes, last_return,
        last_steps, nrec, sticky, reset_x, reset_target, reset_pvec, log_X, log_U, log_pos_error, log_pvec, log_loss,
        log_status, log_iters, log_reward, log_done, log_value, log_logp, rec_obs, rec_action, rec_logp, rec_value,
        rec_reward, rec_done};
    return lmpc_closed_loop(h, plant, pcfg, rcfg, true, B, k0, steps, log_rows, rec_rows, reset_rows, p, noise, stream);
}

int dart_lmpc_collect(dart_mpc_handle* h, const dart_plant_config* plant, const dart_lmpc_policy_config* pcfg,
                      const dart_lmpc_reward_config* rcfg, int B, int k0, int steps, int log_rows, int rec_rows,
                      int reset_rows, double* target, const double* prm, double* plant_pvec, const double* current_k,
                      const float* weights, const float* critic, const float* noise,
                      double* x, double* tilt, double* u_prev, double* w, double* obs_mean, double* obs_M2,
                      int32_t* obs_count, float* history, int32_t* timestep, double* model_params,
                      double* prev_cmd, double* control_seen, int32_t* ep_step, double* ep_return,
                      double* time_penalty, int32_t* episodes, double* last_return, int32_t* last_steps,
                      int32_t* nrec, int32_t* sticky, const double* reset_x, const double* reset_target,
                      const double* reset_pvec, double* log_X, double* log_U, double* log_pos_error,
                      double* log_pvec, double* log_loss, int32_t* log_status, int32_t* log_iters,
                      double* log_reward, int32_t* log_done, float* log_value, float* log_logp, float* rec_obs,
                      float* rec_action, float* rec_logp, float* rec_value, double* rec_reward, float* rec_done,
                      void* stream) {
    DART_ENTER(h, -1);
    // (the arguments are the view's members in their order, up to rec_done, but for the noise)
    const dart_lmpc_train_buffers p = {
        target, prm, plant_pvec, mut(current_k), mut(weights), mut(critic), x, tilt, u_prev, w, obs_mean, obs_M2, obs_count,
        history, timestep, model_params, prev_cmd, control_seen, ep_step, ep_return, time_penalty, episodes, last_return,
        last_steps, nrec, sticky, reset_x, reset_target, reset_pvec, log_X, log_U, log_pos_error, log_pvec, log_loss,
        log_status, log_iters, log_reward, log_done, log_value, log_logp, rec_obs, rec_action, rec_logp, rec_value,
        rec_reward, rec_done};
    return lmpc_closed_loop_host(h, plant, pcfg, rcfg, true, B, k0, steps, log_rows, rec_rows, reset_rows, p, noise,
                                 stream);
}

