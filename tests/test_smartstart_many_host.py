"""ssc_actor_forward_many / ssc_smartstart_rollout_step_many and navigator.PlanPool.window: what they decide on the host, so
none of this needs a GPU.  Struct layouts against the ctypes mirrors; ssc_actor_many_class over a shape table against the
rule ssc_actor_forward's dispatcher follows at m > 32; the windowed pool's bookkeeping against a plain PlanPool's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


@pytest.mark.parametrize("name,mirror,fn", [("ssc_actor_many_item", "ActorManyItem", "ssc_actor_forward_many"),
                                            ("ssc_smartstart_pair", "SmartStartPair", "ssc_smartstart_rollout_step_many")])
def test_struct_layout_matches_header(ffi, tmp_path, name, mirror, fn):
    M = getattr(ffi, mirror)
    assert ffi.STRUCTS[name] is M and fn in ffi._SIGNATURES
    fields = [f for f, _ in M._fields_]
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {f}));' for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssc.h"\nint main(){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(M) and got[1:] == [getattr(M, f).offset for f in fields], got
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssc.h")).read(), flags=re.S)
    body = re.search(r"struct\s+%s\s*\{(.*?)\}\s*;" % name, text, flags=re.S).group(1)
    members = [x for decl in body.split(";") if decl.strip() for x in decl.split(",")]
    assert len(members) == len(fields), members
    assert ffi.lib().ssc_version() == 108                # additive: the ABI version does not move


def dispatcher_body(obs, act, h1, h2, bf16, ln):
    """the kernel ssc_actor_forward launches for this descriptor at m > 32 (actor.hip), as ssc_actor_many_class numbers it"""
    if not (1 <= obs <= 8 and 1 <= act <= 4 and h1 >= 1 and h2 >= 1) or (ln and bf16):
        return -1
    if bf16:
        if act != 1 or obs not in (2, 3) or h1 > 224 or h2 > 128:
            return -1
        if h1 > 128 or h2 > 64:
            return 6 + obs - 2
        return (2 if h1 <= 64 and h2 <= 32 else 4) + obs - 2
    if not ln and act == 1 and (h1, h2) == (64, 32) and obs in (2, 3):
        return obs - 2
    if h1 > 512 or (h1 + (h2 if ln else 0)) * 256 > 160 * 1024:
        return -1
    return 8


def test_actor_many_class_is_the_single_dispatchers_rule(ffi):
    lib, seen = ffi.lib(), set()
    for obs in (0, 1, 2, 3, 4, 8, 9):
        for act in (0, 1, 2, 4, 5):
            for h1, h2 in ((64, 32), (64, 33), (65, 32), (128, 64), (129, 64), (128, 65), (200, 100), (224, 128), (225, 128),
                           (224, 129), (48, 24), (512, 200), (513, 8), (0, 8), (8, 0), (400, 300), (512, 4096)):
                for bf16 in (False, True):
                    for ln in (False, True):
                        a = ffi.ActorDesc()
                        a.obs_dim, a.act_dim, a.h1, a.h2 = obs, act, h1, h2
                        a.precision = ffi.SSC_PREC_BF16_MFMA if bf16 else ffi.SSC_PREC_F32
                        if ln:
                            a.ln1_g = a.ln1_b = a.ln2_g = a.ln2_b = 0x1000
                        body = dispatcher_body(obs, act, h1, h2, bf16, ln)
                        for rms in (0, 1):
                            want = -1 if body < 0 else 2 * body + rms
                            assert lib.ssc_actor_many_class(ctypes.byref(a), rms) == want, (obs, act, h1, h2, bf16, ln, rms)
                        seen.add(body)
    assert seen == {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8}
    a = ffi.ActorDesc()
    a.obs_dim, a.act_dim, a.h1, a.h2, a.precision = 2, 1, 64, 32, 7
    assert lib.ssc_actor_many_class(ctypes.byref(a), 0) == -1 and lib.ssc_actor_many_class(None, 0) == -1


class HostTensorPool:
    """navigator.PlanPool on host tensors (its arithmetic does not depend on the device)"""

    def __new__(cls, *a, **kw):
        from smartstartcontinuous_amd import navigator as nav
        return nav.PlanPool(*a, device="cpu", **kw)


def _plan(rng, d, w):
    return rng.normal(size=(w, d)), np.abs(rng.normal(size=w)), rng.uniform(0.1, 1.0, d)


def test_a_window_behaves_as_a_pool_of_its_own():
    import warnings
    rng = np.random.default_rng(0)
    d, w_max = 2, 6
    big = HostTensorPool(30, 12, w_max, d)
    before = {k: getattr(big, k).clone() for k in ("wp", "left", "wp_len", "radii", "plan_of", "cur_idx")}
    win = big.window(env0=7, n_envs=11, slot0=4, n_slots=5)
    plain = HostTensorPool(11, 5, w_max, d)
    assert (win.P, win.n_slots, win.slot0, win.triple, plain.slot0, plain.triple) == (11, 5, 4, (0, 0, 5), 0, (0, 0, 5))
    assert win.plan_of.data_ptr() == big.plan_of[7:].data_ptr() and win.cur_idx.shape == (11,)
    now = 0
    for n_plans in (2, 2, 3, 1, 5, 4):                       # round-robin over 5 slots, wrapping
        plans = [_plan(rng, d, int(rng.integers(1, w_max + 1))) for _ in range(n_plans)]
        with warnings.catch_warnings(record=True) as ww:
            warnings.simplefilter("always")
            win.publish(plans, now=now, min_age=20)
        with warnings.catch_warnings(record=True) as wp:
            warnings.simplefilter("always")
            plain.publish(plans, now=now, min_age=20)
        assert [str(x.message) for x in ww] == [str(x.message) for x in wp]          # the young-slot warning, word for word
        now += 7
        assert win.triple == plain.triple == tuple(plain.pool.tolist())
        assert (win._next, win.published) == (plain._next, plain.published)
        for k in ("wp", "left", "wp_len", "radii"):
            assert (getattr(win, k) == getattr(plain, k)).all(), k
    assert any("re-published" in str(x.message) for x in ww) or getattr(win, "_warned", False)
    # the window wrote slots [4, 9) of the shared arrays and nothing else
    assert (big.wp.view(12, w_max, d)[4:9] == plain.wp.view(5, w_max, d)).all() and (big.wp_len[4:9] == plain.wp_len).all()
    for k, rows in (("wp", w_max), ("left", w_max), ("wp_len", 1), ("radii", 1)):
        t, b = getattr(big, k), before[k]
        assert (t[:4 * rows] == b[:4 * rows]).all() and (t[9 * rows:] == b[9 * rows:]).all(), k
    assert (big.plan_of == before["plan_of"]).all() and tuple(big.pool.tolist()) == (0, 0, 12) == big.triple
    for bad in (dict(env0=25, n_envs=6, slot0=0, n_slots=1), dict(env0=0, n_envs=1, slot0=8, n_slots=5),
                dict(env0=0, n_envs=1, slot0=0, n_slots=0), dict(env0=-1, n_envs=1, slot0=0, n_slots=1)):
        with pytest.raises(ValueError):
            big.window(**bad)
