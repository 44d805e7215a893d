"""Which compiled build serves a call (csrc/launch_plan.h), on the host: tests/native/launch_plan_table.cpp compiled
with g++ against the header alone -- no library, no GPU.  Every plan below was derived by hand from the if-ladders the
launchers held before the header existed; tests/test_gpu_launch_plan.py holds the library on a device to the same rows.

Knobs are passed to the program explicitly, so one process answers for every setting; `default` is fuse on, overlap on
and occ2_min_b = 2048 (a device of 256 CUs).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

PMPC, SERVE, LMPC, RMPC = 0, 1, 2, 3
OBJECTS = ("main", "seq", "wg2")
LDS = ("shared", "policy", "resto", "policy_or_resto", "full")


def fmt(solver, v):
    """The ints of plan_query (launch_plan.h) as the text of the tables below."""
    if not v[0]:
        return "invalid"
    if solver in (PMPC, SERVE):
        return "%s <%d,%d> waves %d pack %d resto %d %s" % (OBJECTS[v[1]], v[2], v[3], v[4], v[5], v[6],
                                                            "queued" if v[7] else "not queued")
    if solver == LMPC:
        s = ("two-wave " if v[1] else "one-wave ") + ("policy first, " if v[5] else "")
        s += "<false,%d,%d> pack %d lds %s" % (v[2], v[3], v[4], LDS[v[7]])
        return s + (" then <true> lds %s" % LDS[v[8]] if v[6] else "")
    return ("two-wave" if v[1] else "one-wave") + " pack %d" % v[2] + (" then <true> grid B" if v[3] else "")


# (knobs, N or Ns, B or Bs, reduced, resto in): object <NAX,F> waves, pack, resto given, pmpc_resto_kernel queued
PMPC_TABLE = [
    # N <= 15: the one-row build of the -DPMPC_SEQ object; fused restoration for B <= 32
    ("default", 15, (1, 32), 0, 0, "seq <1,3> waves 1 pack 8 resto 0 not queued"),
    ("default", 15, (1, 32), 0, 1, "seq <1,35> waves 1 pack 8 resto 3 not queued"),
    ("default", 15, 33, 0, 0, "seq <1,3> waves 1 pack 1 resto 0 not queued"),
    ("default", 15, 33, 0, 1, "seq <1,3> waves 1 pack 1 resto 1 queued"),
    ("default", 15, 33, 0, 2, "seq <1,3> waves 1 pack 1 resto 2 not queued"),
    ("default", 15, 2047, 0, 0, "seq <1,3> waves 1 pack 1 resto 0 not queued"),
    # N = 16..23: short scan; three waves for B <= 32 (the 15/16 and 32/33 boundaries)
    ("default", (16, 20, 23), (1, 18, 32), 0, 0, "main <1,69> waves 3 pack 8 resto 0 not queued"),
    ("default", (16, 20, 23), (1, 18, 32), 0, 1, "main <1,101> waves 3 pack 8 resto 3 not queued"),
    ("default", (16, 23), 33, 0, 0, "main <1,5> waves 1 pack 1 resto 0 not queued"),
    ("default", (16, 23), 33, 0, 1, "main <1,5> waves 1 pack 1 resto 1 queued"),
    ("default", (16, 23), 33, 0, 2, "main <1,5> waves 1 pack 1 resto 2 not queued"),
    ("default", 20, 1152, 0, 2, "main <1,5> waves 1 pack 1 resto 2 not queued"),
    # N = 24..31: the full scan (the 23/24 boundary)
    ("default", (24, 31), (1, 32), 0, 0, "main <1,65> waves 3 pack 8 resto 0 not queued"),
    ("default", (24, 31), (1, 32), 0, 1, "main <1,97> waves 3 pack 8 resto 3 not queued"),
    ("default", (24, 31), 33, 0, 0, "main <1,1> waves 1 pack 1 resto 0 not queued"),
    ("default", (24, 31), 33, 0, 1, "main <1,1> waves 1 pack 1 resto 1 queued"),
    ("default", (24, 31), 33, 0, 2, "main <1,1> waves 1 pack 1 resto 2 not queued"),
    # N = 32..63 on IPOPT's path without restoration: two waves per instance (the 31/32 boundary)
    ("default", (32, 63), (1, 32), 0, 0, "wg2 <1,1> waves 2 pack 8 resto 0 not queued"),
    ("default", 32, 33, 0, 0, "wg2 <1,1> waves 2 pack 1 resto 0 not queued"),
    ("default", 64, 1, 0, 0, "invalid"),
    # ... with restoration (no caller asks for it): the sequential NAX = 2 build, the restoration kernel queued
    ("default", 40, 32, 0, 1, "seq <2,0> waves 1 pack 8 resto 1 queued"),
    # the reduced path
    ("default", 15, 32, 1, 0, "seq <1,11> waves 1 pack 8 resto 0 not queued"),
    ("default", 20, 32, 1, 0, "main <1,13> waves 1 pack 8 resto 0 not queued"),
    ("default", 31, 32, 1, 0, "main <1,9> waves 1 pack 8 resto 0 not queued"),
    ("default", 40, 32, 1, 0, "seq <2,8> waves 1 pack 8 resto 0 not queued"),
    # from occ2_min_b on: two waves per SIMD, never fused, never on the reduced path
    ("default", (15, 20), 2048, 0, 1, "main <1,21> waves 1 pack 1 resto 1 queued"),
    ("default", 31, 2048, 0, 1, "main <1,17> waves 1 pack 1 resto 1 queued"),
    ("default", 20, 2048, 1, 0, "main <1,13> waves 1 pack 1 resto 0 not queued"),
    ("occ2_min_b=1", (15, 16, 20, 23), (1, 18, 32), 0, 0, "main <1,21> waves 1 pack 8 resto 0 not queued"),
    ("occ2_min_b=1", (15, 16, 20, 23), (1, 18, 32), 0, 1, "main <1,21> waves 1 pack 8 resto 1 queued"),
    ("occ2_min_b=1", (15, 16, 23), 33, 0, 0, "main <1,21> waves 1 pack 1 resto 0 not queued"),
    ("occ2_min_b=1", (15, 16, 23), 33, 0, 2, "main <1,21> waves 1 pack 1 resto 2 not queued"),
    ("occ2_min_b=1", (24, 31), (1, 32), 0, 0, "main <1,17> waves 1 pack 8 resto 0 not queued"),
    ("occ2_min_b=1", (24, 31), (1, 32), 0, 1, "main <1,17> waves 1 pack 8 resto 1 queued"),
    ("occ2_min_b=1", (24, 31), 33, 0, 0, "main <1,17> waves 1 pack 1 resto 0 not queued"),
    ("occ2_min_b=1", (24, 31), 33, 0, 2, "main <1,17> waves 1 pack 1 resto 2 not queued"),
    ("occ2_min_b=1", 32, (1, 32), 0, 0, "wg2 <1,1> waves 2 pack 8 resto 0 not queued"),
    ("occ2_min_b=1", 32, 33, 0, 0, "wg2 <1,1> waves 2 pack 1 resto 0 not queued"),
    ("occ2_min_b=1", 15, 32, 1, 0, "seq <1,11> waves 1 pack 8 resto 0 not queued"),
    ("occ2_min_b=1", 20, 32, 1, 0, "main <1,13> waves 1 pack 8 resto 0 not queued"),
    ("occ2_min_b=1", 31, 32, 1, 0, "main <1,9> waves 1 pack 8 resto 0 not queued"),
    ("occ2_min_b=1", 40, 32, 1, 0, "seq <2,8> waves 1 pack 8 resto 0 not queued"),
    # past qscan_max_b: the sequential builds, the restoration kernel queued
    ("qscan_max_b=0", (15, 16, 20, 23, 24, 31), (1, 18, 32), 0, 0, "seq <1,0> waves 1 pack 8 resto 0 not queued"),
    ("qscan_max_b=0", (15, 16, 20, 23, 24, 31), (1, 18, 32), 0, 1, "seq <1,0> waves 1 pack 8 resto 1 queued"),
    ("qscan_max_b=0", (15, 16, 23, 24, 31), 33, 0, 0, "seq <1,0> waves 1 pack 1 resto 0 not queued"),
    ("qscan_max_b=0", (15, 16, 23, 24, 31), 33, 0, 2, "seq <1,0> waves 1 pack 1 resto 2 not queued"),
    ("qscan_max_b=0", (32, 40), (1, 32), 0, 0, "wg2 <1,1> waves 2 pack 8 resto 0 not queued"),
    ("qscan_max_b=0", 32, 33, 0, 0, "wg2 <1,1> waves 2 pack 1 resto 0 not queued"),
    ("qscan_max_b=0", (15, 20, 31), 32, 1, 0, "seq <1,8> waves 1 pack 8 resto 0 not queued"),
    ("qscan_max_b=0", 40, 32, 1, 0, "seq <2,8> waves 1 pack 8 resto 0 not queued"),
    ("seq_long=1", 40, 32, 0, 0, "seq <2,0> waves 1 pack 8 resto 0 not queued"),
    # overlap off: the one-wave builds for B <= 32 too
    ("overlap=0", 15, (1, 32), 0, 0, "seq <1,3> waves 1 pack 8 resto 0 not queued"),
    ("overlap=0", 15, (1, 32), 0, 1, "seq <1,35> waves 1 pack 8 resto 3 not queued"),
    ("overlap=0", 15, 33, 0, 0, "seq <1,3> waves 1 pack 1 resto 0 not queued"),
    ("overlap=0", 15, 33, 0, 2, "seq <1,3> waves 1 pack 1 resto 2 not queued"),
    ("overlap=0", (16, 20, 23), (1, 18, 32), 0, 0, "main <1,5> waves 1 pack 8 resto 0 not queued"),
    ("overlap=0", (16, 20, 23), (1, 18, 32), 0, 1, "main <1,37> waves 1 pack 8 resto 3 not queued"),
    ("overlap=0", (16, 23), 33, 0, 0, "main <1,5> waves 1 pack 1 resto 0 not queued"),
    ("overlap=0", (16, 23), 33, 0, 2, "main <1,5> waves 1 pack 1 resto 2 not queued"),
    ("overlap=0", (24, 31), (1, 18, 32), 0, 0, "main <1,1> waves 1 pack 8 resto 0 not queued"),
    ("overlap=0", (24, 31), (1, 18, 32), 0, 1, "main <1,33> waves 1 pack 8 resto 3 not queued"),
    ("overlap=0", (24, 31), 33, 0, 0, "main <1,1> waves 1 pack 1 resto 0 not queued"),
    ("overlap=0", (24, 31), 33, 0, 2, "main <1,1> waves 1 pack 1 resto 2 not queued"),
    ("overlap=0", 32, (1, 32), 0, 0, "wg2 <1,1> waves 2 pack 8 resto 0 not queued"),
    ("overlap=0", 32, 33, 0, 0, "wg2 <1,1> waves 2 pack 1 resto 0 not queued"),
    ("overlap=0", 15, 32, 1, 0, "seq <1,11> waves 1 pack 8 resto 0 not queued"),
    ("overlap=0", 20, 32, 1, 0, "main <1,13> waves 1 pack 8 resto 0 not queued"),
    ("overlap=0", 31, 32, 1, 0, "main <1,9> waves 1 pack 8 resto 0 not queued"),
    ("overlap=0", 40, 32, 1, 0, "seq <2,8> waves 1 pack 8 resto 0 not queued"),
    # fuse off: three waves, the restoration kernel queued
    ("resto_fuse=0", 20, 18, 0, 1, "main <1,69> waves 3 pack 8 resto 1 queued"),
    ("resto_fuse=0", 15, 18, 0, 1, "seq <1,3> waves 1 pack 8 resto 1 queued"),
]

# (knobs, N, B, resto in): the resident server
SERVE_TABLE = [
    ("default", 15, 18, 1, "seq <1,35> waves 1 pack 8 resto 3 not queued"),
    ("default", 20, 18, 1, "main <1,37> waves 1 pack 8 resto 3 not queued"),
    ("default", 31, 18, 1, "main <1,33> waves 1 pack 8 resto 3 not queued"),
    ("default", 15, 18, 0, "seq <1,3> waves 1 pack 8 resto 0 not queued"),
    ("default", 20, 18, 0, "main <1,5> waves 1 pack 8 resto 0 not queued"),
    ("default", 31, 18, 0, "main <1,1> waves 1 pack 8 resto 0 not queued"),
    ("default", 20, 33, 1, "main <1,5> waves 1 pack 1 resto 2 not queued"),
    ("default", 20, 18, 2, "main <1,37> waves 1 pack 8 resto 3 not queued"),
    ("resto_fuse=0", 20, 18, 1, "main <1,5> waves 1 pack 8 resto 2 not queued"),
    ("default", 32, 18, 0, "invalid"),
    ("default", 20, 0, 0, "invalid"),
]

# (knobs, N, B, resto, has resto_buf, fuse_policy, learner_B)
LMPC_TABLE = [
    ("default", 30, 18, 1, 1, 1, 0, "one-wave <false,1,0> pack 8 lds policy_or_resto"),
    ("default", 30, 18, 1, 1, 1, 4, "one-wave <false,1,1> pack 8 lds policy_or_resto"),
    ("default", 30, 18, 1, 1, 0, 0, "one-wave <false,1,0> pack 8 lds resto"),
    ("default", 30, 18, 1, 1, 0, 4, "one-wave <false,1,0> pack 8 lds resto"),
    ("default", 30, 18, 0, 0, 0, 0, "one-wave <false,0,0> pack 8 lds shared"),
    ("default", 30, 18, 0, 0, 1, 4, "one-wave <false,0,1> pack 8 lds policy"),
    ("resto_fuse=0", 30, 18, 1, 1, 1, 0, "one-wave <false,0,0> pack 8 lds policy then <true> lds resto"),
    ("default", 30, 33, 1, 1, 1, 4, "one-wave <false,0,1> pack 1 lds policy then <true> lds resto"),
    ("default", 31, 33, 1, 1, 0, 0, "one-wave <false,0,0> pack 1 lds shared then <true> lds resto"),
    ("default", 32, 18, 1, 1, 1, 4, "two-wave policy first, <false,0,0> pack 1 lds full then <true> lds full"),
    ("default", 32, 18, 1, 1, 0, 0, "two-wave <false,0,0> pack 1 lds full then <true> lds full"),
    ("default", 63, 33, 0, 1, 0, 0, "two-wave <false,0,0> pack 1 lds full"),
    ("force_wg2=1", 20, 18, 1, 1, 0, 0, "two-wave <false,0,0> pack 1 lds full then <true> lds full"),
    ("default", 0, 18, 0, 1, 0, 0, "invalid"),               # N < 1
    ("default", 64, 18, 0, 1, 0, 0, "invalid"),              # N > 63
    ("default", 30, 18, 1, 0, 0, 0, "invalid"),              # restoration without its hand-off area
    ("default", 32, 18, 0, 0, 0, 0, "invalid"),              # the two-wave build needs the area always
    ("force_wg2=1", 0, 18, 0, 1, 0, 0, "invalid"),
    ("force_wg2=1", 20, 18, 0, 0, 0, 0, "invalid"),
]

# (knobs, N, B, resto, has resto_buf)
RMPC_TABLE = [
    ("default", 31, 32, 0, 0, "one-wave pack 8"),
    ("default", 31, 32, 1, 0, "one-wave pack 8 then <true> grid B"),
    ("default", 31, 33, 0, 0, "one-wave pack 1"),
    ("default", 31, 33, 1, 0, "one-wave pack 1 then <true> grid B"),
    ("default", 32, 32, 0, 0, "two-wave pack 1"),
    ("default", 32, 33, 0, 0, "two-wave pack 1"),
    ("default", 32, 32, 1, 1, "two-wave pack 1 then <true> grid B"),
    ("default", 32, 33, 1, 1, "two-wave pack 1 then <true> grid B"),
    ("default", 32, 32, 1, 0, "invalid"),                    # the two-wave build's restoration state
    ("force_wg2=1", 20, 32, 1, 1, "two-wave pack 1 then <true> grid B"),
    ("force_wg2=1", 20, 33, 0, 0, "two-wave pack 1"),
    ("default", 0, 32, 0, 0, "invalid"),
    ("default", 64, 32, 0, 1, "invalid"),
    ("force_wg2=1", 0, 32, 0, 1, "invalid"),
]


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


def pmpc_rows():
    """{(knobs, N, B, reduced, resto in): row} of PMPC_TABLE, its N and B tuples written out."""
    rows = {}
    for knobs, Ns, Bs, red, resto, row in PMPC_TABLE:
        for N in _tuple(Ns):
            for B in _tuple(Bs):
                assert (knobs, N, B, red, resto) not in rows
                rows[(knobs, N, B, red, resto)] = row
    return rows


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "launch_plan_table.cpp"), "-o", exe], check=True)
    return exe


def _query(program, solver, queries):
    """The rows of `queries` ((knobs, ints...) each), formatted."""
    text = "".join("%s %d %s\n" % (q[0], solver, " ".join(str(int(i)) for i in q[1:])) for q in queries)
    r = subprocess.run([program, "query"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(queries)
    return [fmt(solver, [int(t) for t in line.split()]) for line in lines]


def test_pmpc_plans_equal_the_table(program):
    rows = pmpc_rows()
    keys = list(rows)
    got = _query(program, PMPC, keys)
    wrong = [(k, g, rows[k]) for k, g in zip(keys, got) if g != rows[k]]
    assert not wrong, wrong


@pytest.mark.parametrize("solver,table", [(SERVE, SERVE_TABLE), (LMPC, LMPC_TABLE), (RMPC, RMPC_TABLE)],
                         ids=["serve", "lmpc", "rmpc"])
def test_server_lmpc_and_rmpc_plans_equal_the_table(program, solver, table):
    got = _query(program, solver, [row[:-1] for row in table])
    wrong = [(row[:-1], g, row[-1]) for row, g in zip(table, got) if g != row[-1]]
    assert not wrong, wrong


def test_every_plan_of_the_sweep_names_a_build_its_object_holds(program):
    """N = 1..63, B in {1, 32, 33, 2047, 2048}, both paths, resto 0..2, every knob setting of the table, launches and
    the server: the build is in the owning object's list (the list the .hip files instantiate from), pack is
    xcd_pack(B), F passes the kernels' static_asserts."""
    r = subprocess.run([program, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["checked", "14130"], r.stdout


ENV_DEFAULT = dict(qscan_max_b=str(1 << 30), occ2_min_b="unset", seq_long="0", overlap="1", resto_fuse="1",
                   force_wg2="0", pmpc_resume="0")
# variable -> (field, its value with the variable "0", "1", "")
ENV_KNOBS = {
    "DART_PMPC_QSCAN_MAX_B": ("qscan_max_b", "0", "1", "0"),       # atoi
    "DART_PMPC_OCC2_MIN_B": ("occ2_min_b", "0", "1", "0"),         # atoi
    "DART_PMPC_SEQ_LONG": ("seq_long", "0", "1", "0"),             # on with a leading '1'
    "DART_FORCE_WG2": ("force_wg2", "0", "1", "0"),
    "DART_PMPC_RESUME": ("pmpc_resume", "0", "1", "0"),
    "DART_PMPC_OVERLAP": ("overlap", "0", "1", "1"),               # off with a leading '0'
    "DART_RESTO_FUSE": ("resto_fuse", "0", "1", "1"),
}


def _env_knobs(program, extra):
    env = {k: v for k, v in os.environ.items() if k not in ENV_KNOBS}
    env.update(extra)
    r = subprocess.run([program, "env"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(t.split("=") for t in r.stdout.split())


def test_knobs_from_env_unset(program):
    assert _env_knobs(program, {}) == ENV_DEFAULT


@pytest.mark.parametrize("var", sorted(ENV_KNOBS))
def test_knobs_from_env(program, var):
    """Each variable set to "0", "1" and "" in a child process: its field as the launchers read it before, every
    other field at its default."""
    field, *want = ENV_KNOBS[var]
    for value, w in zip(("0", "1", ""), want):
        assert _env_knobs(program, {var: value}) == dict(ENV_DEFAULT, **{field: w}), (var, value)
