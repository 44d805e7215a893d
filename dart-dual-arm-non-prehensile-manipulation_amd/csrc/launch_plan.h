// launch_plan.h -- which compiled build of a solver serves a call, as pure functions of (N, B, path, restoration)
// and the process's knobs.  Plain C++17 with no HIP in it: the launchers (pmpc_ipm.hip, pmpc_resto.hip, rmpc_ipm.hip,
// lmpc_ipm.hip) launch what a plan names and decide nothing themselves, and tests/test_launch_plan.py holds every
// plan to a table on the host (tests/native/launch_plan_table.cpp).
//
// A new PMPC build flag is added in three places: one row in the owning object's list (kPmpcMain / kPmpcSeq /
// kPmpcWg2 below), one line in pmpc_plan, one row in the test's table.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdlib.h>

namespace dartmpc {

// ---------------------------------------------------------------------------------------------------------------
// knobs (environment, experiments and A/B runs): read once per process
struct LaunchKnobs {
    static constexpr int kNotSet = INT_MIN;
    int qscan_max_b = 1 << 30;   // DART_PMPC_QSCAN_MAX_B: PMPC batches above it take the sequential builds
    int occ2_min_b = kNotSet;    // DART_PMPC_OCC2_MIN_B: PMPC batches from it on take two waves per SIMD (not set:
                                 // occ2_min_b_of the device's CUs)
    bool seq_long = false;       // DART_PMPC_SEQ_LONG=1: PMPC N = 32..63 on the one-wave sequential build (NAX = 2)
    bool overlap = true;         // DART_PMPC_OVERLAP=0: the one-wave PMPC builds everywhere
    bool resto_fuse = true;      // DART_RESTO_FUSE=0: a queued restoration kernel behind every launch (the round-4 form)
    bool force_wg2 = false;      // DART_FORCE_WG2=1: RMPC and LMPC on their two-wave builds at every N (tools/wg2_ab.py)
    bool pmpc_resume = false;    // DART_PMPC_RESUME=1: PMPC's restoration resumes from the register kernel's iterate
};

inline LaunchKnobs knobs_from_env() {
    LaunchKnobs k;
    const auto is = [](const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; };
    if (const char* e = getenv("DART_PMPC_QSCAN_MAX_B")) k.qscan_max_b = atoi(e);
    if (const char* e = getenv("DART_PMPC_OCC2_MIN_B")) k.occ2_min_b = atoi(e);
    k.seq_long = is("DART_PMPC_SEQ_LONG", '1');
    k.overlap = !is("DART_PMPC_OVERLAP", '0');
    k.resto_fuse = !is("DART_RESTO_FUSE", '0');
    k.force_wg2 = is("DART_FORCE_WG2", '1');
    k.pmpc_resume = is("DART_PMPC_RESUME", '1');
    return k;
}

// the process's knobs, read on first use (tests and tools run each setting in a child process)
inline const LaunchKnobs& launch_knobs() {
    static const LaunchKnobs k = knobs_from_env();
    return k;
}

// DART_PMPC_OCC2_MIN_B when it is not set: two instances per SIMD of the device (2048 on MI355X); `cus` <= 0: the
// device could not be asked, and no batch takes the two-waves-per-SIMD builds
constexpr int occ2_min_b_of(int cus) { return cus > 0 ? 2 * 4 * cus : 1 << 30; }

// Batches of at most 32: the launchers deal 8 blocks per instance and only every 8th works, so all instances land on
// one XCD (blocks go round-robin over the 8 XCDs; <= 32 waves fit one XCD's CUs) and share its L2 for the code
constexpr int xcd_pack(int B) { return B <= 32 ? 8 : 1; }

// RMPC and LMPC: the two-wave builds (rmpc_wg2.o, lmpc_wg2.o; N = 32..63) serve the call
inline bool two_wave(int N, const LaunchKnobs& k) { return N > 31 || k.force_wg2; }

// ---------------------------------------------------------------------------------------------------------------
// PMPC.  The build of the kernel as one mask (the template argument F of pmpc_ipm_kernel, pmpc_serve_kernel and
// pmpc_solve); the comment above PM_EXPECT (pmpc_ipm.hip) says what each selects.  kOcc2 and kFuse concern the kernels
// only.
enum : unsigned { kScan = 1u, kOneRow = 2u, kShort2 = 4u, kRed = 8u, kOcc2 = 16u, kFuse = 32u, kOvl = 64u };

struct PmpcBuild {
    int nax;
    unsigned f;
};
// what the kernels' own static_asserts ask of F
constexpr bool pmpc_flags_ok(unsigned f) {
    return f < 2 * kOvl && (!(f & (kOneRow | kShort2 | kOcc2 | kOvl)) || (f & kScan)) &&
           (!(f & kFuse) || !(f & (kRed | kOcc2)));
}

// The instantiations each of the three objects built from pmpc_ipm.hip holds (Makefile: as is, -DPMPC_SEQ,
// -DDART_WG=2); a plan names one of them
enum PmpcObject { kPmpcMain = 0, kPmpcSeq = 1, kPmpcWg2 = 2 };
inline constexpr PmpcBuild kPmpcMainIpm[] = {
    {1, kScan}, {1, kScan | kShort2}, {1, kScan | kRed}, {1, kScan | kShort2 | kRed},
    {1, kScan | kOcc2}, {1, kScan | kShort2 | kOcc2}, {1, kScan | kFuse}, {1, kScan | kShort2 | kFuse},
    {1, kScan | kOvl}, {1, kScan | kShort2 | kOvl}, {1, kScan | kFuse | kOvl}, {1, kScan | kShort2 | kFuse | kOvl}};
inline constexpr PmpcBuild kPmpcMainServe[] = {
    {1, kScan}, {1, kScan | kShort2}, {1, kScan | kFuse}, {1, kScan | kShort2 | kFuse}};
inline constexpr PmpcBuild kPmpcSeqIpm[] = {
    {1, 0u}, {1, kScan | kOneRow}, {1, kRed}, {1, kScan | kOneRow | kRed}, {1, kScan | kOneRow | kFuse},
    {2, 0u}, {2, kRed}};
inline constexpr PmpcBuild kPmpcSeqServe[] = {{1, kScan | kOneRow}, {1, kScan | kOneRow | kFuse}};
inline constexpr PmpcBuild kPmpcWg2Ipm[] = {{1, kScan}};

template <size_t M>
constexpr bool pmpc_build_in(const PmpcBuild (&list)[M], int nax, unsigned f) {
    for (size_t i = 0; i < M; ++i)
        if (list[i].nax == nax && list[i].f == f) return true;
    return false;
}

struct PmpcPlan {
    bool valid = true;
    PmpcObject object = kPmpcMain;
    int nax = 1;
    unsigned f = 0;
    int waves = 1;           // per block: 3 the overlapped builds, 2 the two-wave workgroups
    int pack = 1;            // grid = B x pack blocks
    int resto = 0;           // the mode the kernel is given (PmpcArgs::resto)
    bool resto_queued = false;   // pmpc_resto_kernel behind the solve on the same stream
};

// dartmpc_launch_pmpc: a batch of B > 0 instances.  `occ2_min_b`: the threshold in force (the knob, or occ2_min_b_of
// the device)
inline PmpcPlan pmpc_plan(int N, int B, int reduced, int resto, const LaunchKnobs& k, int occ2_min_b) {
    PmpcPlan p;
    p.pack = xcd_pack(B);
    // The quadratic scan shortens the dependent chain but needs more registers (one wave per SIMD
    // instead of two).  On IPOPT's path (z rows, second-order correction) the sequential build no
    // longer fits two waves per SIMD without scratch spills, and the scan build is faster at every
    // batch size measured (B = 4096: 15.9 against 14.7 M solves/s; 18432: 18.1 against 17.4 M), so
    // it serves every N <= 31 batch; the sequential builds remain for N > 31 and for the
    // DART_PMPC_QSCAN_MAX_B experiment knob (the round-2 crossover was ~1.7 k instances).
    const bool scan = B <= k.qscan_max_b;
    // From two instances per SIMD of the device on (2048 on MI355X), batches of N <= 31 take the scan build
    // compiled for two waves per SIMD (40 VGPRs spilled, 164 B of scratch): the second wave fills the
    // first's dependency stalls (VALU busy ~63 % alone).  Below that, one wave per SIMD and no spills win
    // (N = 20, B = 1152: 10.8 against 9.4 M solves/s; even at 1536; B = 2048: 15.2 against 13.7 M; 18432:
    // 20.5-20.9 against 17.8 M; N = 31, 18432: 6.4 against 6.1 M).  N <= 15 takes the short-scan build there
    // (the one-row build loses at two waves, 19.4-19.7 against 19.9 M; the short-scan one wins, 2048: 15.4-15.5
    // against 15.0 M, 18432: 22.2-22.8 against 20.0 M).  profiles/r04/occ2_ab.txt; DART_PMPC_OCC2_MIN_B
    // overrides the threshold (experiments).
    const bool occ2 = !reduced && B >= occ2_min_b && scan;
    // batches of at most 32 (one XCD, one instance per CU): IPOPT's restoration phases run in the wave that
    // handed the instance over (resto mode 3, pmpc_resto_tail), so no restoration launch follows the solve.
    // Only the branches below that name a kFuse build take mode 3 (not the two-waves-per-SIMD build, not
    // the sequential builds past DART_PMPC_QSCAN_MAX_B): everywhere else the queued pmpc_resto_kernel (mode 1) stays
    if (resto == 1 && p.pack == 8 && !reduced && N <= 31 && !occ2 && scan && k.resto_fuse) resto = 3;
    const unsigned fuse = resto == 3 ? kFuse : 0u, red = reduced ? kRed : 0u;
    // The overlapped builds (three waves per instance: the second factors the Riccati scan of the point and the third
    // forms its error measures, tests convergence and updates mu while the first runs the line search's trial and
    // the update) where a CU has SIMDs to spare: batches of at most 32 (one instance per
    // CU of one XCD) on IPOPT's path at N = 16..31.  Larger batches, the resident server and the rollout
    // kernels keep the one-wave builds.  DART_PMPC_OVERLAP=0: the one-wave builds here too (A/B).
    const bool ovl = p.pack == 8 && !reduced && !occ2 && N >= 16 && N <= 31 && scan && k.overlap;
    const unsigned short2 = N <= 23 ? kShort2 : 0u;
    if (ovl) {
        p.f = kScan | short2 | fuse | kOvl;
        p.waves = 3;
    } else if (N <= 23 && occ2) {     // (N <= 15 too: the short-scan build at two waves beats the one-row build at one)
        p.f = kScan | kShort2 | kOcc2;
    } else if (N <= 15 && scan) {     // the one-row scan build
        p.object = kPmpcSeq;
        p.f = kScan | kOneRow | (fuse && !reduced ? kFuse : red);
    } else if (N <= 31 && scan) {
        p.f = kScan | short2 | (occ2 ? kOcc2 : fuse ? kFuse : red);
    } else if (N > 31 && !reduced && !resto && !k.seq_long) {
        // N = 32..63 on IPOPT's path: the scan build on two waves per instance (DART_PMPC_SEQ_LONG=1: the one-wave
        // sequential build, NAX = 2, for A/B)
        p.object = kPmpcWg2;
        p.f = kScan;
        p.waves = 2;
        p.valid = N <= 63;
    } else {
        // the sequential (throughput) builds: two waves per SIMD, used once B exceeds the scan limit or N > 31
        p.object = kPmpcSeq;
        p.nax = N <= 31 ? 1 : 2;
        p.f = red;
    }
    p.resto = resto;
    p.resto_queued = resto == 1;      // the instances whose line search failed, with IPOPT's restoration phases
    return p;
}

// dartmpc_launch_pmpc_serve: the resident server for B slots (IPOPT's path, N <= 31): one wave per slot, one XCD when
// it fits
inline PmpcPlan pmpc_serve_plan(int N, int B, int resto, const LaunchKnobs& k) {
    PmpcPlan p;
    p.valid = B > 0 && N <= 31;
    p.pack = xcd_pack(B);
    // B <= 32: the restoration phases run in the wave that handed the instance over (mode 3); larger
    // servers hand it to the host (mode 2: dart_mpc_abi.hip served_resto)
    p.resto = !resto ? 0 : (p.pack == 8 && k.resto_fuse) ? 3 : 2;
    const unsigned fuse = p.resto == 3 ? kFuse : 0u;
    if (N <= 15) {
        p.object = kPmpcSeq;
        p.f = kScan | kOneRow | fuse;
    } else {
        p.f = kScan | (N <= 23 ? kShort2 : 0u) | fuse;
    }
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// LMPC.  lmpc_ipm_kernel<RESTO, FUSE, POP>: the instantiations of the two objects built from lmpc_ipm.hip
struct LmpcBuild {
    bool resto, fuse, pop;
};
inline constexpr LmpcBuild kLmpcMainBuilds[] = {
    {false, false, false}, {true, false, false}, {false, true, false}, {false, false, true}, {false, true, true}};
inline constexpr LmpcBuild kLmpcWg2Builds[] = {{false, false, false}, {true, false, false}};

// the dynamic LDS of a launch, one value per size (lmpc_ipm.hip maps them to bytes: the structs live there)
enum LmpcLds {
    kLdsShared,          // sizeof(LmShared)
    kLdsPolicy,          // LmShared, then the policy prologue's PolicyLds
    kLdsResto,           // LmShared, then the restoration state LmResto
    kLdsPolicyOrResto,   // the larger of the last two
    kLdsFull             // kLmLdsBytes: the maximum (what the per-device opt-in covers)
};

struct LmpcPlan {
    bool valid = true;
    bool wg2 = false;            // lmpc_wg2.o: one instance per two-wave workgroup, grid B
    bool fuse = false, pop = false;      // the first launch is lmpc_ipm_kernel<false, fuse, pop>
    int pack = 1;
    bool policy_first = false;   // the policy step of every instance as a launch of its own first (two-wave build)
    bool second = false;         // lmpc_ipm_kernel<true> follows on the same grid: IPOPT's restoration phases for the
                                 // instances the first launch handed off (the others return at once)
    LmpcLds lds_first = kLdsShared, lds_second = kLdsResto;
};

inline LmpcPlan lmpc_plan(int N, int B, int resto, bool has_resto_buf, int fuse_policy, int learner_B,
                          const LaunchKnobs& k) {
    LmpcPlan p;
    if (two_wave(N, k) && N < 64) {
        p.wg2 = true;
        p.valid = N >= 1 && has_resto_buf;      // the device area is needed with or without resto
        p.policy_first = fuse_policy != 0;
        p.second = resto != 0;
        p.lds_first = p.lds_second = kLdsFull;
        return p;
    }
    p.valid = N >= 1 && N <= 31 && !(resto && !has_resto_buf);
    p.pack = xcd_pack(B);            // one XCD (and its L2) for the code of a small batch
    p.pop = fuse_policy && learner_B > 0;       // a population's policies in the prologue
    // the policy prologue's LDS only when the launch runs it (the opt-in covers the maximum)
    p.lds_first = fuse_policy ? kLdsPolicy : kLdsShared;
    if (resto && p.pack == 8 && k.resto_fuse) {      // restoration in the solving wave: one launch
        p.fuse = true;
        p.lds_first = fuse_policy ? kLdsPolicyOrResto : kLdsResto;
    } else {
        p.second = resto != 0;
    }
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// RMPC.  rmpc_ipm_kernel<false>, then (resto) rmpc_ipm_kernel<true> for the instances whose line search failed
struct RmpcPlan {
    bool valid = true;
    bool wg2 = false;        // rmpc_wg2.o: one instance per two-wave workgroup
    int pack = 1;            // first launch: grid B x pack
    bool second = false;     // rmpc_ipm_kernel<true>, grid B, pack 1
};

inline RmpcPlan rmpc_plan(int N, int B, int resto, bool has_resto_buf, const LaunchKnobs& k) {
    RmpcPlan p;
    p.second = resto != 0;
    if (two_wave(N, k) && N < 64) {
        p.wg2 = true;
        p.valid = N >= 1 && !(resto && !has_resto_buf);
        return p;
    }
    p.valid = N >= 1 && N <= 31;
    p.pack = xcd_pack(B);            // blocks go round-robin over the 8 XCDs: one XCD, one L2 for the code
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// A plan as a row of ints, for the tests (the library's dartmpc_plan_query and tests/native/launch_plan_table.cpp):
//   kQueryPmpc   in N, B, reduced, resto     out valid, object, NAX, F, waves, pack, resto given, resto queued
//   kQueryServe  in N, B, resto              out as kQueryPmpc
//   kQueryLmpc   in N, B, resto, has resto_buf, fuse_policy, learner_B
//                out valid, two-wave, FUSE, POP, pack, policy first, second launch, LDS of the first, of the second
//   kQueryRmpc   in N, B, resto, has resto_buf     out valid, two-wave, pack, second launch
// Returns the number of ints written, -1 for an unknown solver.
enum PlanQuery { kQueryPmpc = 0, kQueryServe = 1, kQueryLmpc = 2, kQueryRmpc = 3 };
inline int plan_query(int solver, const int* in, int* out, const LaunchKnobs& k, int occ2_min_b) {
    if (solver == kQueryPmpc || solver == kQueryServe) {
        const PmpcPlan p = solver == kQueryPmpc ? pmpc_plan(in[0], in[1], in[2], in[3], k, occ2_min_b)
                                                : pmpc_serve_plan(in[0], in[1], in[2], k);
        const int row[] = {p.valid, p.object, p.nax, (int)p.f, p.waves, p.pack, p.resto, p.resto_queued};
        for (int i = 0; i < 8; ++i) out[i] = row[i];
        return 8;
    }
    if (solver == kQueryLmpc) {
        const LmpcPlan p = lmpc_plan(in[0], in[1], in[2], in[3] != 0, in[4], in[5], k);
        const int row[] = {p.valid, p.wg2, p.fuse, p.pop, p.pack, p.policy_first, p.second, p.lds_first, p.lds_second};
        for (int i = 0; i < 9; ++i) out[i] = row[i];
        return 9;
    }
    if (solver == kQueryRmpc) {
        const RmpcPlan p = rmpc_plan(in[0], in[1], in[2], in[3] != 0, k);
        const int row[] = {p.valid, p.wg2, p.pack, p.second};
        for (int i = 0; i < 4; ++i) out[i] = row[i];
        return 4;
    }
    return -1;
}

}  // namespace dartmpc
