"""Inputs and references of the device tests of csrc/wave.h's scalar math (tests/test_gpu_wave_math.py) and their
host-only checks (tests/test_wave_refs.py).  Nothing here shares code with the kernels: the references are numpy
``longdouble`` library functions, the input generators are seeded."""
import numpy as np

LD = np.longdouble
NREG = 1 << 18                     # points per region
LOG2E = 1.4426950408889634         # the reduction constant of exp_econ / tanh_econ, as wave.h writes it
SQRT_HALF = 0.70710678118654752440  # the mantissa switch of log_core


def require_longdouble():
    """The references need the 64-bit mantissa of x87 extended precision: 2^-11 of a double's ulp."""
    assert np.finfo(LD).eps < 2e-19, "numpy longdouble is not wider than double here: no reference for these tests"


def ulp_unit(ref):
    """Spacing of the doubles at the reference value (longdouble); 2^-1074 for references below 2^-1022."""
    _, e = np.frexp(np.abs(np.asarray(ref, LD)))
    return np.ldexp(LD(1), np.maximum(e, -1021).astype(np.int64) - 53)


def err_ulps(got, ref):
    return np.abs(np.asarray(got, LD) - ref) / ulp_unit(ref)


def worst(got, ref, x):
    """(largest error in ulps, the argument where it occurs)."""
    e = err_ulps(got, ref)
    i = int(np.argmax(e))
    return float(e[i]), float(np.asarray(x).ravel()[i])


def _step(x, j):
    """x moved by j doubles (j may be an array)."""
    x = np.asarray(x, np.float64)
    i = x.view(np.int64) + np.where(x < 0, -1, 1) * np.asarray(j, np.int64)
    return i.view(np.float64)


def _pow2_neg(kmax):
    return np.ldexp(1.0, -np.arange(0, kmax + 1))


def _mant_exp(rng, elo, ehi, n=NREG):
    return np.ldexp(1.0 + rng.random(n), rng.integers(elo, ehi + 1, n))


# ---------------------------------------------------------------------------------------------------------
# input regions: name -> array, per function
# ---------------------------------------------------------------------------------------------------------
def rcp_inputs(seed=11):
    rng = np.random.default_rng(seed)
    x = _mant_exp(rng, -300, 300) * rng.choice([-1.0, 1.0], NREG)
    p2 = np.ldexp(1.0, np.arange(-300, 301))
    edge = np.array([1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52])
    return {"mantissa x exponent": x, "powers of two, 1 +- 2^-52": np.concatenate([p2, -p2, edge, -edge])}


def log_seam_inputs():
    """sqrt(1/2) 2^e and the doubles up to four steps either side of it, e = -1020 .. 1020 (step 20)."""
    e = np.arange(-1020, 1021, 20)
    j = np.arange(-4, 5)
    m = _step(np.full(j.size, np.float64(SQRT_HALF)), j)
    return np.ldexp(m[None, :], e[:, None]).ravel()


def log_inputs(seed=12):
    rng = np.random.default_rng(seed)
    k = np.arange(1, 53)
    return {"exponents -1020..1020": _mant_exp(rng, -1020, 1020),
            "[0.5, 1.5]": 0.5 + rng.random(NREG),
            "1 +- 2^-k": np.concatenate([1.0 + np.ldexp(1.0, -k), 1.0 - np.ldexp(1.0, -k)]),
            "mantissa switch": log_seam_inputs()}


LOG_NAN_INPUTS = np.array([-1.0, -1e-300, -0.0, 0.0, -np.inf, np.inf, np.nan, 1.0e308, 1.5e308, -5e-324])


def log_subnormal_inputs(seed=13):
    rng = np.random.default_rng(seed)
    x = np.ldexp(1.0 + rng.random(4096), rng.integers(-1074, -1022, 4096))     # rounds into the subnormals
    x = x[(x > 0) & (x < 2.0 ** -1022)]
    return np.concatenate([x, np.ldexp(1.0, np.arange(-1074, -1022))])


def exp_tie_inputs(nlo=-1075, nhi=1022):
    """(n + 1/2) ln 2 rounded to double and the doubles up to three steps either side, n = nlo .. nhi."""
    n = np.arange(nlo, nhi + 1)
    t = ((n.astype(LD) + LD(0.5)) * np.log(LD(2))).astype(np.float64)
    j = np.arange(-3, 4)
    return _step(np.repeat(t, j.size), np.tile(j, n.size)), np.repeat(n, j.size)


def exp_inputs(seed=14):
    rng = np.random.default_rng(seed)
    p = _pow2_neg(1074)
    ties = exp_tie_inputs()[0]
    return {"[-708, 709]": -708.0 + 1417.0 * rng.random(NREG),
            "+-2^-k": np.concatenate([p, -p]),
            "reduction ties": ties[(ties >= -745.0) & (ties <= 709.0)],
            "[-745, -708] (subnormal results)": -745.0 + 37.0 * rng.random(NREG)}


EXP_CLAMP_LOW = np.array([-745.0000000000001, -746.0, -1000.0, -1e10, -1e308, -np.inf])
EXP_CLAMP_HIGH = np.array([709.0000000000001, 709.5, 710.0, 1e10, 1e308, np.inf])


def tanh_inputs(seed=15):
    rng = np.random.default_rng(seed)
    p = _pow2_neg(1074)
    big = np.array([40.0, 40.5, 41.0, 45.0, 50.0, 100.0, 1e3, 1e10, 1e100, 1e308])
    return {"[-45, 45]": -45.0 + 90.0 * rng.random(NREG),
            "[-2, 2]": -2.0 + 4.0 * rng.random(NREG),
            "[-0.6, 0.6]": -0.6 + 1.2 * rng.random(NREG),
            "+-2^-k, +-0": np.concatenate([p, -p, [0.0, -0.0]]),
            "|x| >= 40": np.concatenate([big, -big])}


def sincos_inputs(seed=16):
    rng = np.random.default_rng(seed)
    p = _pow2_neg(1074)
    return {"[-1, 1]": -1.0 + 2.0 * rng.random(NREG), "+-2^-k, +-1, 0": np.concatenate([p, -p, [0.0]])}


def sincos_wide_inputs(seed=17):
    """|x| up to 3: only the library branch (poly == false) is valid there."""
    rng = np.random.default_rng(seed)
    return np.concatenate([-3.0 + 6.0 * rng.random(300), [-3.0, 3.0, -1.0, 1.0, 1.0000000000000002]])


def lg2_inputs(seed=18):
    rng = np.random.default_rng(seed)
    k = np.arange(1, 53)
    return {"all exponents": _mant_exp(rng, -1022, 1023),
            "near 1": np.concatenate([1.0 + np.ldexp(1.0, -k), 1.0 - np.ldexp(1.0, -k), 0.9 + 0.2 * rng.random(4096)])}


# ---------------------------------------------------------------------------------------------------------
# references (longdouble in, longdouble out)
# ---------------------------------------------------------------------------------------------------------
def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


REFS = {"rcp": lambda x: LD(1) / _ld(x), "log": lambda x: np.log(_ld(x)), "exp": lambda x: np.exp(_ld(x)),
        "tanh": lambda x: np.tanh(_ld(x)), "sin": lambda x: np.sin(_ld(x)), "cos": lambda x: np.cos(_ld(x)),
        "log2": lambda x: np.log2(_ld(x))}

# every region of every function, for the host-only cross-check of the references: (reference name, generator)
REGIONS = (("rcp", rcp_inputs), ("log", log_inputs), ("exp", exp_inputs), ("tanh", tanh_inputs),
           ("sin", sincos_inputs), ("cos", sincos_inputs), ("log2", lg2_inputs))


def reduction_index(x, scale=1.0):
    """n of the Cody-Waite reduction of exp_econ (scale 1) / tanh_econ (scale 2) as the kernels form it in double."""
    return np.rint(scale * np.asarray(x, np.float64) * LOG2E)
