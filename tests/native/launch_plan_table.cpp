// Host program for tests/test_launch_plan.py: csrc/launch_plan.h with g++ alone (no HIP, no library, no GPU).
//
//   launch_plan_table query   reads one query per line from stdin, `<knobs> <solver> <inputs...>`, and prints the ints
//                             that plan_query writes for it, one line per query.  <knobs>: `default` or a comma-
//                             separated list of name=value (the fields of LaunchKnobs; occ2_min_b defaults to 2048,
//                             the value on a device of 256 CUs).  <solver>: 0 PMPC, 1 resident server, 2 LMPC, 3 RMPC.
//   launch_plan_table sweep   every PMPC and server plan over N = 1..63, B in {1, 32, 33, 2047, 2048}, both paths,
//                             resto 0..2 and the knob settings of the test's table: a valid plan names a build of
//                             the owning object's list, its pack is xcd_pack(B), and its F passes the kernels' own
//                             static_asserts.  Prints the number of plans checked; a violation is printed and fails.
//   launch_plan_table env     prints knobs_from_env() of this process.
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "launch_plan.h"

using namespace dartmpc;

static bool set_knob(LaunchKnobs& k, const std::string& name, int v) {
    if (name == "qscan_max_b") k.qscan_max_b = v;
    else if (name == "occ2_min_b") k.occ2_min_b = v;
    else if (name == "seq_long") k.seq_long = v != 0;
    else if (name == "overlap") k.overlap = v != 0;
    else if (name == "resto_fuse") k.resto_fuse = v != 0;
    else if (name == "force_wg2") k.force_wg2 = v != 0;
    else if (name == "pmpc_resume") k.pmpc_resume = v != 0;
    else return false;
    return true;
}

static bool parse_knobs(const std::string& spec, LaunchKnobs& k) {
    k = LaunchKnobs{};
    k.occ2_min_b = occ2_min_b_of(256);
    if (spec == "default") return true;
    std::stringstream ss(spec);
    std::string item;
    while (std::getline(ss, item, ',')) {
        const size_t eq = item.find('=');
        if (eq == std::string::npos || !set_knob(k, item.substr(0, eq), atoi(item.c_str() + eq + 1))) return false;
    }
    return true;
}

static int query() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        std::stringstream ss(line);
        std::string spec;
        int solver = -1, in[8] = {}, out[16] = {};
        if (!(ss >> spec >> solver)) continue;
        for (int i = 0; i < 8 && (ss >> in[i]); ++i) {}
        LaunchKnobs k;
        if (!parse_knobs(spec, k)) { printf("bad knobs %s\n", spec.c_str()); return 2; }
        const int n = plan_query(solver, in, out, k, k.occ2_min_b);
        if (n < 0) { printf("bad solver %d\n", solver); return 2; }
        for (int i = 0; i < n; ++i) printf(i ? " %d" : "%d", out[i]);
        printf("\n");
    }
    return 0;
}

static bool in_object(const PmpcPlan& p, bool serve) {
    if (serve) return p.object == kPmpcMain ? pmpc_build_in(kPmpcMainServe, p.nax, p.f)
                                            : p.object == kPmpcSeq && pmpc_build_in(kPmpcSeqServe, p.nax, p.f);
    return p.object == kPmpcMain  ? pmpc_build_in(kPmpcMainIpm, p.nax, p.f)
           : p.object == kPmpcSeq ? pmpc_build_in(kPmpcSeqIpm, p.nax, p.f)
                                  : pmpc_build_in(kPmpcWg2Ipm, p.nax, p.f);
}

static int sweep() {
    const char* settings[] = {"default", "occ2_min_b=1", "qscan_max_b=0", "seq_long=1", "overlap=0", "resto_fuse=0"};
    const int Bs[] = {1, 32, 33, 2047, 2048};
    long checked = 0, bad = 0;
    for (const char* spec : settings) {
        LaunchKnobs k;
        parse_knobs(spec, k);
        for (int N = 1; N <= 63; ++N)
            for (int B : Bs)
                for (int resto = 0; resto <= 2; ++resto)
                    for (int serve = 0; serve <= 1; ++serve)
                        for (int reduced = 0; reduced <= 1 - serve; ++reduced) {
                            const PmpcPlan p = serve ? pmpc_serve_plan(N, B, resto, k)
                                                     : pmpc_plan(N, B, reduced, resto, k, k.occ2_min_b);
                            if (!p.valid) continue;
                            ++checked;
                            const bool ok = in_object(p, serve != 0) && p.pack == xcd_pack(B) && pmpc_flags_ok(p.f) &&
                                            (!serve || ((p.f & kScan) && !(p.f & (kRed | kOcc2 | kOvl))));
                            if (!ok) {
                                ++bad;
                                printf("VIOLATION %s serve=%d N=%d B=%d reduced=%d resto=%d: object %d <%d,%u> pack %d\n", spec,
                                       serve, N, B, reduced, resto, (int)p.object, p.nax, p.f, p.pack);
                            }
                        }
    }
    printf("checked %ld\n", checked);
    return bad ? 1 : 0;
}

static int env() {
    const LaunchKnobs k = knobs_from_env();
    printf("qscan_max_b=%d occ2_min_b=", k.qscan_max_b);
    if (k.occ2_min_b == LaunchKnobs::kNotSet) printf("unset");
    else printf("%d", k.occ2_min_b);
    printf(" seq_long=%d overlap=%d resto_fuse=%d force_wg2=%d pmpc_resume=%d\n", k.seq_long, k.overlap, k.resto_fuse,
           k.force_wg2, k.pmpc_resume);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "query")) return query();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !strcmp(argv[1], "env")) return env();
    fprintf(stderr, "usage: %s query|sweep|env\n", argv[0]);
    return 2;
}
