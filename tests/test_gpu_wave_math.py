"""The scalar math of csrc/wave.h run on the device (csrc/wave_probe.hip) against numpy ``longdouble`` references.

Each test prints the largest error in ulps and the argument where it occurs before it asserts.  A ulp is the
spacing of the doubles at the reference value (2^-1074 for references below 2^-1022).  The raw reciprocal's
largest relative error delta is measured first; D = delta^2 2^53 is what one Newton step leaves of it, in ulps,
and enters the bounds of frcp and tanh_econ.  tests/test_wave_refs.py checks the references and generators."""
import numpy as np
import pytest

import wave_refs as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    wr.require_longdouble()
    from dart_mpc import _lib
    return _lib.probe_math


@pytest.fixture(scope="module")
def delta(probe):
    """Largest relative error of v_rcp_f64 over the reciprocal sample, and D = delta^2 2^53."""
    worst_d, at = 0.0, 0.0
    for x in wr.rcp_inputs().values():
        r, _ = probe("rcp_raw", x)
        rel = np.abs(r.astype(wr.LD) * x.astype(wr.LD) - 1)
        i = int(np.argmax(rel))
        if float(rel[i]) > worst_d:
            worst_d, at = float(rel[i]), float(x[i])
    print(f"raw v_rcp_f64: delta = {worst_d:.3e} at x = {at!r}; D = {worst_d ** 2 * 2.0 ** 53:.3f} ulp")
    return worst_d, worst_d ** 2 * 2.0 ** 53


def _measure(probe, name, regions, ref, second=False, poly=True, label=None):
    out = {}
    for reg, x in regions.items():
        got = probe(name, x, poly)[1 if second else 0]
        w, at = wr.worst(got, wr.REFS[ref](x), x)
        print(f"{label or name} [{reg}]: max {w:.3f} ulp at x = {at!r}")
        out[reg] = w
    return out


def test_raw_reciprocal_delta(delta):
    """The premise of frcp: one Newton step on an estimate delta off leaves delta^2; 1e-14 needs delta <= 1e-7."""
    assert delta[0] <= 1e-7


def test_frcp(probe, delta):
    w = _measure(probe, "frcp", wr.rcp_inputs(), "rcp")
    assert max(w.values()) <= 1.0 + delta[1]


def test_log_fast(probe):
    w = _measure(probe, "log_fast", wr.log_inputs(), "log")
    assert max(w.values()) <= 1.5


def test_log_fast_contract(probe):
    """NaN for x <= 0, +-0, inf, NaN and x >= 1e308; the subnormal arguments are measured and recorded."""
    got, _ = probe("log_fast", wr.LOG_NAN_INPUTS)
    assert np.all(np.isnan(got)), got
    x = wr.log_subnormal_inputs()
    got, _ = probe("log_fast", x)
    w, at = wr.worst(got, wr.REFS["log"](x), x)
    print(f"log_fast [subnormal arguments]: max {w:.3f} ulp at x = {at!r}")
    assert np.all(np.isfinite(got))
    assert w <= 1.5      # measured within the bound of the normal arguments: no exception to state in wave.h


def test_exp_econ(probe):
    regions = wr.exp_inputs()
    normal, sub = 0.0, 0.0
    for reg, x in regions.items():
        got, _ = probe("exp_econ", x)
        ref = wr.REFS["exp"](x)
        e = wr.err_ulps(got, ref)
        s = ref < wr.LD(2.0) ** -1022
        for part, m in (("normal", ~s), ("subnormal", s)):
            if m.any():
                i = int(np.argmax(np.where(m, e, -1)))
                print(f"exp_econ [{reg}, {part} results]: max {float(e[i]):.3f} at x = {float(x[i])!r}")
        normal = max(normal, float(np.max(e[~s], initial=0.0)))
        sub = max(sub, float(np.max(e[s], initial=0.0)))
    assert normal <= 1.0      # ulps
    assert sub <= 1.0         # units of 2^-1074


def test_exp_econ_clamps(probe):
    """Arguments below -745 and above 709 give the function's value at the clamp, finite."""
    lo, _ = probe("exp_econ", np.concatenate([[-745.0], wr.EXP_CLAMP_LOW]))
    hi, _ = probe("exp_econ", np.concatenate([[709.0], wr.EXP_CLAMP_HIGH]))
    print("exp_econ clamps:", lo[0], hi[0])
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
    assert np.all(lo == lo[0]) and np.all(hi == hi[0])
    assert wr.err_ulps(lo[:1], wr.REFS["exp"]([-745.0]))[0] <= 1.0 and wr.err_ulps(hi[:1], wr.REFS["exp"]([709.0]))[0] <= 1.0


def test_tanh_econ(probe, delta):
    regions = wr.tanh_inputs()
    w = {}
    for reg, x in regions.items():
        got, _ = probe("tanh_econ", x)
        w[reg], at = wr.worst(got, wr.REFS["tanh"](x), x)
        print(f"tanh_econ [{reg}]: max {w[reg]:.3f} ulp at x = {at!r}; max |T| = {np.max(np.abs(got))!r}")
        assert np.all(np.abs(got) <= 1.0)
    assert max(w.values()) <= 3.5 + delta[1]


def test_exp_tanh_nan_documented(probe):
    """A NaN argument passes the clamps fmin(fmax(.)) and comes out finite, as wave.h states: tanh_econ -1,
    exp_econ its value at -745.  (The callers carry the NaN through their linear terms.)"""
    t, _ = probe("tanh_econ", np.array([np.nan]))
    e, _ = probe("exp_econ", np.array([np.nan, -745.0]))
    print("tanh_econ(NaN), exp_econ(NaN):", t[0], e[0])
    assert t[0] == -1.0
    assert e[0] == e[1] and np.isfinite(e[0])


@pytest.mark.parametrize("name", ["sincos_small", "sincos_econ", "tilt_sincos", "tilt_sincos_econ"])
def test_sincos(probe, name):
    s = _measure(probe, name, wr.sincos_inputs(), "sin", label=name + " sin")
    c = _measure(probe, name, wr.sincos_inputs(), "cos", second=True, label=name + " cos")
    assert max(s.values()) <= 1.1 and max(c.values()) <= 1.1


@pytest.mark.parametrize("name", ["cos_small", "cos_econ", "tilt_cos", "tilt_cos_econ"])
def test_cos(probe, name):
    c = _measure(probe, name, wr.sincos_inputs(), "cos")
    assert max(c.values()) <= 1.1


def test_tilt_library_branch(probe):
    """poly == false (a box wider than 1 rad): the library sincos / cos, to 1 ulp on [-3, 3]."""
    x = {"[-3, 3]": wr.sincos_wide_inputs()}
    for name in ("tilt_sincos", "tilt_sincos_econ"):
        s = _measure(probe, name, x, "sin", poly=False, label=name + " (library) sin")
        c = _measure(probe, name, x, "cos", second=True, poly=False, label=name + " (library) cos")
        assert max(s.values()) <= 1.0 and max(c.values()) <= 1.0
    for name in ("tilt_cos", "tilt_cos_econ"):
        c = _measure(probe, name, x, "cos", poly=False, label=name + " (library)")
        assert max(c.values()) <= 1.0


def test_lg2(probe):
    """|lg2(x) - log2 x| <= 2^-21 max(1, |log2 x|): three f32 roundings and the f32 rounding of the mantissa."""
    for reg, x in wr.lg2_inputs().items():
        got, _ = probe("lg2", x)
        ref = wr.REFS["log2"](x)
        rel = np.abs(got.astype(wr.LD) - ref) / np.maximum(1, np.abs(ref))
        i = int(np.argmax(rel))
        print(f"lg2 [{reg}]: max {float(rel[i]) * 2.0 ** 21:.3f} x 2^-21 at x = {float(x[i])!r}")
        assert float(rel[i]) <= 2.0 ** -21
