"""The wave primitives of csrc/wave.h on the device, in the one-wave and the two-wave (DART_WG = 2) build, against
numpy restatements of their documented semantics (csrc/wave_probe.hip writes every lane's result of every
primitive; the row numbers below are the ones of prim_probe_kernel).

Shifts and broadcasts: exact per lane, no lane excluded -- every lane's source is stated in wave.h (one wave:
lane 63 of from_next and lane 0 of from_prev read 0; two waves: lanes 31 / 63 of wave 0 and 0 / 32 of wave 1 hand
over, lane 63 of wave 1 and lane 0 of wave 0 read 0).  Reductions: uniform over all lanes, bit for bit equal to the
butterfly in the order of DART_LEVELS (two waves: wave 0's total combined with wave 1's), exact on integers and
within 64 kWaves eps sum|x| of math.fsum on random values.  Lock-step forms: the same bits as the separate calls."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVES = (1, 2)
L64 = np.arange(64)
# sources of the four in-row levels: quad_perm [1,0,3,2], [2,3,0,1], row_ror 4, 8 (lane i takes lane i - n of its row)
ROW_LEVELS = (L64 ^ 1, L64 ^ 2, (L64 & ~15) | ((L64 - 4) & 15), (L64 & ~15) | ((L64 - 8) & 15))
PNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _wave_total(x, op, bcast=True):
    """The butterfly of wreduce on one wave's 64 values."""
    x = np.array(x)
    for src in ROW_LEVELS:
        x = op(x, x[src])
    if not bcast:                                   # the four row totals read from lanes 0, 16, 32, 48
        return op(op(x[0], x[16]), op(x[32], x[48]))
    y = x.copy()                                    # row_bcast:15 into rows 1 and 3
    y[16:32] = op(x[16:32], x[15]); y[48:64] = op(x[48:64], x[47])
    z = y.copy()                                    # row_bcast:31 into rows 2 and 3
    z[32:64] = op(y[32:64], y[31])
    return z[63]


def _reduce(x, op, bcast=True):
    """wreduce over the instance: the waves' totals combined in wave order."""
    tot = [_wave_total(w, op, bcast) for w in np.asarray(x).reshape(-1, 64)]
    return tot[0] if len(tot) == 1 else op(tot[0], tot[1])


def _add(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return a + b


def _umax(a, b):      # the unsigned order of the f32 bit patterns (wreduce_nn)
    return np.maximum(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)).view(np.float32)


def _umin(a, b):
    return np.minimum(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)).view(np.float32)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _same_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.broadcast_to(np.asarray(want, np.float64), np.shape(got))
    both_nan = np.isnan(got) & np.isnan(want)
    bad = ~both_nan & (_bits(got) != _bits(np.ascontiguousarray(want)))
    assert not bad.any(), f"{what}: lanes {np.flatnonzero(bad)[:8]} got {got[bad][:4]!r} want {want[bad][:4]!r}"


def _shift_next(x):
    x = x.reshape(-1, 64)
    o = np.zeros_like(x)
    o[:, :63] = x[:, 1:]                            # lane 63 reads 0
    if x.shape[0] == 2:
        o[0, 31], o[0, 63] = x[1, 0], x[1, 32]
    return o.ravel()


def _shift_prev(x):
    x = x.reshape(-1, 64)
    o = np.zeros_like(x)
    o[:, 1:] = x[:, :63]                            # lane 0 reads 0
    if x.shape[0] == 2:
        o[1, 0], o[1, 32] = x[0, 31], x[0, 63]
    return o.ravel()


def _inputs(kind, T, pos=0):
    """d [8, T] float64, f [8, T] float32 (f[0..3] non-negative), p [T]."""
    t = np.arange(T, dtype=np.float64)
    d, f, p = np.zeros((8, T)), np.zeros((8, T), np.float32), np.zeros(T, np.int32)
    if kind == "lanes":
        d[0], d[1], d[2], d[3] = t, 100.0 - t, (t * 7) % T - 20.0, t - 50.0
        f[0], f[1], f[2], f[3] = t, T - t + 0.5, (t * 5) % T, t / 2
        f[4] = t + 1; f[5] = t + 1
    elif kind == "random":
        rng = np.random.default_rng(101)
        d[:] = rng.choice([-1.0, 1.0], (8, T)) * 10.0 ** rng.uniform(-30, 30, (8, T))
        f[:] = (10.0 ** rng.uniform(-30, 30, (8, T))).astype(np.float32)
        d[3, 3], d[3, T - 2] = np.inf, -np.inf
        f[4, 5] = PNAN                                  # a NaN is the largest of wmaxf / wminf's order
        f[5, T - 3] = -0.0                              # and -0 (outside their domain) larger still
        p[:] = rng.random(T) < 0.3
    elif kind == "nonneg":
        rng = np.random.default_rng(102)
        f[:] = rng.random((8, T)).astype(np.float32)
        f[0, ::7] = 0.0
        f[0, 1::9] = np.float32(1e-41)                  # subnormal
        f[1, 2] = np.inf
        f[2] = (rng.integers(0, 1 << 20, T).astype(np.uint32)).view(np.float32)     # zeros and subnormals only
        f[3, ::2] = np.inf; f[3, 1::2] = 0.0
        f[4, :] = PNAN; f[4, T - 1] = 3.0               # all NaN but one
        f[5, :] = 0.0; f[5, 7] = -0.0
        d[3, ::2] = 0.0; d[3, 1::2] = -0.0              # wmax / wmin order -0 below +0
        d[0] = t
    elif kind == "one":
        d[0, pos], d[1, pos], d[2, pos], d[3, pos] = 1.0, -1.0, 2.0, -0.0
        f[:, pos] = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0)
        p[pos] = 1
    return d, f, p


CASES = {1: [("lanes", 0), ("random", 0), ("nonneg", 0)] + [("one", q) for q in (0, 31, 32, 63)],
         2: [("lanes", 0), ("random", 0), ("nonneg", 0)] + [("one", q) for q in (0, 31, 32, 63, 64, 95, 96, 127)]}


@pytest.fixture(scope="module")
def runs():
    """Every input set through the probe of both builds, once: {(waves, kind, pos): (d, f, p, out)}."""
    from dart_mpc import _lib
    res = {}
    for waves in WAVES:
        T = _lib.probe_layout(waves)["threads"]
        assert T == 64 * waves
        for kind, pos in CASES[waves]:
            d, f, p = _inputs(kind, T, pos)
            res[(waves, kind, pos)] = (d, f, p, _lib.probe_prims(d, f, p, waves))
    return res


def _ids():
    return [(w, k, q) for w in WAVES for k, q in CASES[w]]


@pytest.mark.parametrize("key", _ids(), ids=lambda k: f"wg{k[0]}-{k[1]}{k[2]}")
def test_shifts_and_broadcasts(runs, key):
    d, f, p, out = runs[key]
    T = d.shape[1]
    lane = np.arange(T) % 64
    base = np.arange(T) - lane
    _same_bits(out[0], _shift_next(d[0]), "from_next")
    _same_bits(out[1], _shift_prev(d[0]), "from_prev")
    for i in range(3):
        _same_bits(out[2 + i], _shift_next(d[i]), f"from_next_n[{i}]")
        _same_bits(out[5 + i], _shift_prev(d[i]), f"from_prev_n[{i}]")
    for i in range(8):
        want = d[0][base + (lane & ~15) + i]
        _same_bits(out[8 + i], want, f"row_bcast<{i}>")
        _same_bits(out[16 + i], want, f"row_bcast_over<{i}>")      # the dead value never shows
    for i in range(16):
        _same_bits(out[24 + i], d[0][base + (lane & 32) + i], f"half_bcast({i})")
    lo, hi = d[0][base + (lane & 31)], d[0][base + (lane & 31) + 32]
    _same_bits(out[40], lo, "half_pair lo")
    _same_bits(out[41], hi, "half_pair hi")
    _same_bits(out[42], lo + hi, "half_pair_sum")


@pytest.mark.parametrize("key", _ids(), ids=lambda k: f"wg{k[0]}-{k[1]}{k[2]}")
def test_reductions(runs, key):
    waves, kind, _ = key
    d, f, p, out = runs[key]
    T = d.shape[1]
    # row -> (input, restated butterfly)
    sums64 = {43: d[0], 46: d[1], 47: d[2]}
    want = {r: _reduce(x, _add) for r, x in sums64.items()}
    want.update({51: _reduce(d[0], _add, False), 52: _reduce(d[1], _add, False)})
    want.update({44: np.max(d[0]), 49: np.max(d[1]), 50: np.max(d[2]), 45: np.min(d[0]), 48: np.min(d[1])})
    want.update({74: _reduce(f[0], _add), 77: _reduce(f[1], _add)})
    want.update({75: _reduce(f[0], _umax), 78: _reduce(f[1], _umax), 80: _reduce(f[2], _umax), 81: _reduce(f[3], _umax),
                 76: _reduce(f[0], _umin), 79: _reduce(f[1], _umin)})
    want[108] = float(p.any())
    for r, w in want.items():
        _same_bits(out[r], np.float64(w), f"row {r}")           # uniform over every lane, bit for bit
    # the f32 maxima / minima are the IEEE ones on their domain (+0, positive, inf)
    for r, x, fn in ((75, f[0], np.max), (78, f[1], np.max), (80, f[2], np.max), (81, f[3], np.max), (76, f[0], np.min),
                     (79, f[1], np.min)):
        assert out[r, 0] == fn(x)
    # sums: exact on integers, within T eps sum|x| of the exactly rounded sum otherwise
    for r, x, eps in ((43, d[0], 2.0 ** -53), (46, d[1], 2.0 ** -53), (47, d[2], 2.0 ** -53), (51, d[0], 2.0 ** -53),
                      (52, d[1], 2.0 ** -53), (74, f[0], 2.0 ** -24), (77, f[1], 2.0 ** -24)):
        xs = [float(v) for v in x]
        if not np.all(np.isfinite(xs)):
            continue
        exact = math.fsum(xs)
        if kind in ("lanes", "one"):
            assert out[r, 0] == exact, (r, out[r, 0], exact)
        else:
            assert abs(out[r, 0] - exact) <= T * eps * math.fsum(abs(v) for v in xs), (r, out[r, 0], exact)


# lock-step rows -> the rows of the separate calls on the same inputs
LOCKSTEP = {"wsum2": ((53, 54), (43, 46)), "wsum3": ((55, 56, 57), (43, 46, 47)), "wmin2d": ((58, 59), (45, 48)),
            "wred_errors_f64": (range(60, 66), (44, 49, 50, 45, 43, 46)),
            "wred_errors_f64_rl": (range(66, 72), (44, 49, 50, 45, 51, 52)), "wsum2_rl": ((72, 73), (51, 52)),
            "wmin2f": ((82, 83), (76, 79)), "wsum2_maxf": ((84, 85, 86), (43, 46, 75)),
            "wsum2_maxf_min2f": (range(87, 92), (43, 46, 75, 76, 79)),
            "wred_errors": (range(92, 98), (75, 78, 80, 76, 74, 77)),
            "wred_errors4": (range(98, 105), (75, 78, 80, 81, 76, 74, 77)),
            "wsum2_rl_maxf": ((105, 106, 107), (51, 52, 75))}


@pytest.mark.parametrize("key", _ids(), ids=lambda k: f"wg{k[0]}-{k[1]}{k[2]}")
def test_lockstep_forms_give_the_bits_of_the_separate_calls(runs, key):
    out = runs[key][3]
    for name, (rows, sep) in LOCKSTEP.items():
        for r, s in zip(rows, sep):
            _same_bits(out[r], out[s], f"{name} row {r} against row {s}")


@pytest.mark.parametrize("waves", WAVES)
def test_nan_and_signed_zero_order(runs, waves):
    """wmaxf / wminf run on the unsigned order of the bit patterns: a NaN is the largest value (wave.h), and -0,
    outside their domain, larger than any of it.  wmax / wmin (fmax / fmin) order -0 below +0 and handle inf."""
    d, f, p, out = runs[(waves, "random", 0)]
    assert np.all(np.isnan(out[109])) and np.all(out[110] == np.min(np.delete(f[4], 5)))
    _same_bits(out[111], -0.0, "wmaxf with a -0")
    assert np.all(out[112] == np.min(np.delete(f[5], f.shape[1] - 3)))
    assert np.all(out[113] == np.inf) and np.all(out[114] == -np.inf)
    d, f, p, out = runs[(waves, "nonneg", 0)]
    assert np.all(np.isnan(out[109])) and np.all(out[110] == 3.0)          # all NaN but one lane
    _same_bits(out[111], -0.0, "wmaxf of +0 and one -0")
    _same_bits(out[112], 0.0, "wminf of +0 and one -0")
    _same_bits(out[113], 0.0, "wmax of +-0")
    _same_bits(out[114], -0.0, "wmin of +-0")


def test_wany_cases(runs):
    """All false; one true lane at every distinguished position (two waves: also in wave 1 only)."""
    assert np.all(runs[(1, "lanes", 0)][3][108] == 0.0) and np.all(runs[(2, "lanes", 0)][3][108] == 0.0)
    for (waves, kind, pos), (d, f, p, out) in runs.items():
        if kind == "one":
            assert p.sum() == 1 and np.all(out[108] == 1.0), (waves, pos)


def test_wg_errors_combines_the_two_waves(runs):
    for kind, pos in CASES[2]:
        d, f, p, out = runs[(2, kind, pos)]
        a, b = f[:, 0], f[:, 64]
        want = [_umax(a[0], b[0]), _umax(a[1], b[1]), _umax(a[2], b[2]), _umax(a[3], b[3]), _umin(a[1], b[1]),
                np.float32(a[0]) + np.float32(b[0]), np.float32(a[1]) + np.float32(b[1])]
        for i, w in enumerate(want):
            _same_bits(out[115 + i], np.float64(w), f"wg_errors value {i} ({kind}{pos})")
