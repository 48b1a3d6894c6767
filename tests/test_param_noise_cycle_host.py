"""``ssc_param_noise_cycle`` without a GPU: every bad argument comes back with its code before any HIP call."""
import ctypes

import pytest

N_ACTOR = 2 * 64 + 64 + 64 * 32 + 32 + 32 + 1
SRC, DST, OBS, SD, DIST = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20     # never dereferenced


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def desc(ffi, obs_dim=2, h1=64, h2=32, base=SRC):
    d = ffi.ActorDesc()
    d.obs_dim, d.h1, d.h2, d.act_dim = obs_dim, h1, h2, 1
    o = base
    for k, count in (("W1", obs_dim * h1), ("b1", h1), ("W2", h1 * h2), ("b2", h2), ("W3", h2), ("b3", 1)):
        setattr(d, k, o)
        o += 4 * count
    d.last_layer_tanh, d.precision, d.obs_clip = 1, ffi.SSC_PREC_F32, 5.0
    return d, (o - base) // 4


def call(ffi, **kw):
    d, n = desc(ffi, **{k: kw.pop(k) for k in ("obs_dim", "h1", "h2", "base") if k in kw})
    a = dict(m=64, obs=OBS, rms=None, n=n, src=SRC, skip=(0, 0, 0, 0), seed=1, ga=0, gb=1, desired=0.2, coef=1.01, sd=SD,
             dist=DIST, dst=DST)
    a.update(kw)
    return ffi.lib().ssc_param_noise_cycle(ctypes.byref(d), a["m"], a["obs"], a["rms"], a["n"], a["src"], *a["skip"], a["seed"],
                                           a["ga"], a["gb"], a["desired"], a["coef"], a["sd"], a["dist"], a["dst"], None)


def test_cycle_argument_errors(ffi):
    E, lib = ffi.SSC_EINVAL, ffi.lib()
    for bad in (dict(m=0), dict(m=-1), dict(m=4097), dict(n=0), dict(n=-5), dict(coef=1.0), dict(coef=0.99), dict(coef=-2.0),
                dict(coef=float("nan")), dict(dst=SRC), dict(dst=None), dict(obs=None), dict(src=None), dict(sd=None),
                dict(dist=None), dict(skip=(8, 4, 0, 0)), dict(skip=(10, 20, 19, 30)), dict(skip=(0, 0, 0, N_ACTOR + 1)),
                dict(ga=1 << 56), dict(gb=1 << 56),
                dict(n=N_ACTOR - 1),                  # b3 lies outside the flat array
                dict(base=SRC - 4)):                  # W1 starts in front of it
        assert call(ffi, **bad) == E, bad
        assert b"ssc_param_noise_cycle" in lib.ssc_last_error(), bad
    assert call(ffi, m=4097) == E and b"4096" in lib.ssc_last_error()
    assert call(ffi, dst=SRC) == E and b"d_dst == d_src" in lib.ssc_last_error()
    assert lib.ssc_param_noise_cycle(None, 64, OBS, None, N_ACTOR, SRC, 0, 0, 0, 0, 1, 0, 1, 0.2, 1.01, SD, DIST, DST, None) == E


def test_cycle_shape_too_large_for_lds(ffi):
    """400-300: the adaptive copy alone (122 201 floats) exceeds the 160 KB; the message carries the byte count"""
    lib = ffi.lib()
    assert call(ffi, obs_dim=3, h1=400, h2=300) == ffi.SSC_EUNSUPPORTED
    msg = lib.ssc_last_error().decode()
    # copy padded to 4 floats + a 4-row tile: inputs, both networks' two activation layers, LayerNorm statistics, reduction
    need = 4 * (122204 + 4 * 3 + 2 * 4 * 401 + 2 * 4 * 301 + 16 + 36)
    assert "LDS" in msg and str(need) in msg and "163840" in msg, msg
    # a copy that fits while a 4-row tile beside it does not
    assert call(ffi, obs_dim=8, h1=512, h2=64) == ffi.SSC_EUNSUPPORTED and "LDS" in lib.ssc_last_error().decode()
