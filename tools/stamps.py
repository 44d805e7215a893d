"""Diagnostic: per-phase cycle shares of the PMPC kernel (block 0) from the DART_STAMPS build.

Loads dart_mpc/libdartmpc_stamps.so (make -C <pkg>/csrc stamps) in place of the
product library, solves the C2 batch once and prints s_memtime cycles per phase.
Stamps fence the kernel, so read the shares, not the absolute length.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
from dart_mpc import _lib  # noqa: E402
from dart_mpc.workload import pmpc_batch  # noqa: E402

_lib.LIB_PATH = os.path.join(_lib.PKG_DIR, os.environ.get("DART_STAMPS_LIB", "libdartmpc_stamps.so"))
L = _lib.lib()
N = int(os.environ.get("DART_STAMPS_N", "20"))
B = int(os.environ.get("DART_STAMPS_B", "18"))
# the one-row (N <= 15) and the sequential (B above the scan limit, or N > 31) builds live in the
# PMPC_SEQ object, which has its own stamp array
read = L.dartmpc_read_stamps_seq if (N <= 15 or N > 31 or B > 1664) else L.dartmpc_read_stamps
read.argtypes = [ctypes.c_void_p]
# (phase, slot): the evaluation is split where the per-lane values the Newton step needs end and the error terms begin
PHASES = [("setup", 0), ("eval lanes", 16), ("eval errors", 1), ("mu update", 2), ("riccati", 3), ("direction", 4),
          ("ls prep", 5), ("ls trials", 6), ("update", 7), ("outputs", 8)]
S, T, P = pmpc_batch(-(-B // 18))
S, T, P = S[:B], T[:B], P[:B]
s = _lib.Solver(N=N, B_max=B, path=os.environ.get("DART_PMPC_PATH", "ipopt"))
for rep in range(3):
    out = s.solve_batch(S, T, P)
st = np.zeros(32, dtype=np.uint64)
read(ctypes.c_void_p(st.ctypes.data))
tot = float(sum(st[i] for _, i in PHASES))
print(f"block0 iters={out['iters'][0]} total cycles={tot:.0f}")
for n, i in PHASES:
    print(f"  {n:12s} {int(st[i]):10d}  {100 * st[i] / tot:5.1f}%  per-iter {st[i] / max(1, out['iters'][0]):9.0f}")
print(f"  scan-path Riccati passes {int(st[11])}")
it0 = int(tot - st[0] - st[8])
print(f"  first iteration {int(st[12])} cycles, mean iteration {it0 / max(1, out['iters'][0]):.0f} cycles")
print(f"  riccati passes {int(st[9])}, line-search trials {int(st[10])}, iterations with a correction {int(st[15]) & 0xffff}")
if st[13]:
    # the overlapped build hands the first line-search trial point over before the trial: accepted updates that
    # found it right (hits) and that had to drop its factors and hand the accepted point over (misses); slot 15
    # holds both beside the corrections, 16 bits each
    print(f"  speculative hand-over: {(int(st[15]) >> 16) & 0xffff} hits, {(int(st[15]) >> 32) & 0xffff} misses")
    # the overlapped build (B <= 32, N = 16..31): the riccati span above is the solving wave's wait for the factor
    # wave plus its LDS read; this is the factor wave's own time from barrier A to its arrival at barrier B
    print(f"  factor wave: {int(st[13])} cycles between its barriers, per-iter {st[13] / max(1, out['iters'][0]):.0f}")
    print(f"  solving wave: {int(st[14])} cycles waiting at barrier B, per-iter {st[14] / max(1, out['iters'][0]):.0f}")
if st[17]:
    # the evaluation wave of the overlapped build: its own time from barrier A to its arrival at barrier B
    print(f"  evaluation wave: {int(st[17])} cycles between its barriers, per-iter {st[17] / max(1, out['iters'][0]):.0f}")
print("batch iters:", out["iters"].tolist())
