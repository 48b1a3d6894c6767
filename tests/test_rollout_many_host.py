"""ssc_rollout_many / ssc_replay_append_many / ssc_decay_schedule_many / ssc_obs_rms_update_many: everything the four entry
points decide on the host, before any HIP call -- so none of this needs a GPU.  The pointers are made-up addresses: a call
that passed validation with work to do would launch, so every case here either fails validation or has nothing to launch."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ITEMS, D_CURSORS = 0x7000_0000, 0x7100_0000          # "device copies": never read on the host


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


# ---- ssc_rollout_many ------------------------------------------------------------------------------------------------
def population(ffi, P, kind=0, rms=False, log=True, ring=True, **actor):
    """P valid pairs of the served shape (bf16 MFMA 64-32 actor, device epsilon), every array at an address of its own"""
    items = (ffi.RolloutManyItem * P)()
    obs_dim = 2 if kind == ffi.SSC_ENV_MOUNTAINCAR else 3
    for p, it in enumerate(items):
        base = 0x100_0000 * (p + 1)
        it.params = ffi.default_params(kind, 1.0, 200)
        pol = it.policy
        pol.kind = ffi.SSC_POLICY_ACTOR
        pol.act_low, pol.act_high = (-1.0, 1.0) if obs_dim == 2 else (-2.0, 2.0)
        a = pol.actor
        a.obs_dim, a.h1, a.h2, a.act_dim = obs_dim, 64, 32, 1
        for k, name in enumerate(("W1", "b1", "W2", "b2", "W3", "b3")):
            setattr(a, name, base + 0x1000 * k)
        a.last_layer_tanh, a.precision, a.obs_clip = 1, ffi.SSC_PREC_BF16_MFMA, 5.0
        for k, v in actor.items():
            setattr(a, k, v)
        pol.ou.mu, pol.ou.sigma, pol.ou.theta, pol.ou.dt, pol.ou.d_epsilon = 0.4, 0.6, 0.15, 1e-2, base + 0x8000
        it.n = 8 + p
        st = it.state
        st.s0, st.s1, st.steps, st.ep_ret, st.ou_x = (base + 0x10000 + 0x1000 * k for k in range(5))
        it.has_log, it.has_ring = int(log), int(ring)
        if log:
            for c in range(obs_dim):
                it.log.obs[c] = base + 0x20000 + 0x1000 * c
                it.log.obs2[c] = base + 0x30000 + 0x1000 * c
            it.log.act, it.log.rew, it.log.done = base + 0x24000, base + 0x25000, base + 0x26000
        if ring:
            it.ring.env_id, it.ring.length, it.ring.ret, it.ring.cursor = (base + 0x40000 + 0x1000 * k for k in range(4))
            it.ring.capacity = 64
        it.d_stats, it.seed, it.env_id0 = base + 0x50000, 11 + p, 1000 * p
        it.d_rms = base + 0x60000 if rms else None
    return items


def call(ffi, items, K=0, n=None, d_items=D_ITEMS, cursors="own", d_cursors=D_CURSORS):
    cur = (ffi.PairCursor * max(len(items) if items is not None else 1, 1))() if cursors == "own" else cursors
    rc = ffi.lib().ssc_rollout_many(None if items is None else ctypes.addressof(items), d_items,
                                    None if cur is None else ctypes.addressof(cur), d_cursors,
                                    len(items) if n is None else n, K, None)
    return rc, ffi.lib().ssc_last_error()


def test_rollout_null_arrays_and_empty_population(ffi):
    items = population(ffi, 2)
    assert call(ffi, None, n=2)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, d_items=None)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, cursors=None)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, d_cursors=None)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_pairs" in msg
    assert call(ffi, items, n=-3)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, K=-1)[0] == ffi.SSC_EINVAL


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("rms", [False, True])
def test_rollout_no_steps_is_ok_without_a_launch(ffi, kind, rms):
    assert call(ffi, population(ffi, 4, kind=kind, rms=rms))[0] == ffi.SSC_OK
    assert call(ffi, population(ffi, 3, kind=kind, rms=rms, log=False, ring=False))[0] == ffi.SSC_OK
    items = population(ffi, 3, kind=kind, rms=rms)          # has_ring is per pair
    items[1].has_ring = 0
    assert call(ffi, items)[0] == ffi.SSC_OK


def test_rollout_every_item_passes_the_single_call_checks(ffi):
    items = population(ffi, 3)
    items[1].n = 0
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"n = 0" in msg
    items = population(ffi, 3)
    items[2].state.ep_ret = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"NULL state" in msg
    items = population(ffi, 3)
    items[0].log.rew = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 0" in msg and b"NULL log" in msg
    items = population(ffi, 3)
    items[1].ring.cursor = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"ring" in msg
    items = population(ffi, 3)
    items[2].policy.actor.W2 = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"NULL actor" in msg
    items = population(ffi, 3)
    items[1].state.ou_x = None                               # device epsilon: the noise path runs
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"ou_x" in msg
    items = population(ffi, 2)
    items[1].params.max_position = 3.0                       # validate_mc_params
    rc, msg = call(ffi, items)
    assert rc != ffi.SSC_OK and b"pair 1" in msg
    items = population(ffi, 2)
    items[1].log.row_stride = items[1].n - 1
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"stride" in msg


def test_rollout_one_instantiation_per_launch(ffi):
    items = population(ffi, 3)                               # env kind
    pend = population(ffi, 3, kind=1)
    ctypes.memmove(ctypes.addressof(items[2]), ctypes.addressof(pend[2]), ctypes.sizeof(ffi.RolloutManyItem))
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"env kind" in msg
    items = population(ffi, 4)                               # the policy class ssc_rollout would choose: action bounds
    items[2].policy.act_low, items[2].policy.act_high = -2.0, 2.0
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"generic" in msg and b"fused" in msg
    items = population(ffi, 4)                               # ... an observation clip that acts on raw observations
    items[1].policy.actor.obs_clip = 0.5
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"generic" in msg
    items = population(ffi, 4, rms=True)                     # (normalised observations are clipped inside the fused policy)
    items[1].policy.actor.obs_clip = 0.5
    assert call(ffi, items)[0] == ffi.SSC_OK
    items = population(ffi, 4)                               # ... exploration noise off
    items[3].policy.ou.d_epsilon, items[3].policy.ou.epsilon = None, 0.0
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 3" in msg
    items = population(ffi, 3)                               # last_layer_tanh is a template argument of the fused policy
    items[1].policy.actor.last_layer_tanh = 0
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"last_layer_tanh" in msg
    for kw in (dict(kind=1), dict(kind=0)):                  # ... and a run-time value of the generic one
        items = population(ffi, 3, **kw)
        for it in items:
            it.policy.act_low, it.policy.act_high = -2.0, 2.0
        items[1].policy.actor.last_layer_tanh = 0
        assert call(ffi, items)[0] == ffi.SSC_OK
    items = population(ffi, 3, rms=True)                     # statistics for all pairs or for none
    items[1].d_rms = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"d_rms" in msg
    items = population(ffi, 3)
    items[2].d_rms = 0x5000
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"d_rms" in msg
    items = population(ffi, 3)                               # a log for all pairs or for none
    items[1].has_log = 0
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"has_log" in msg
    items = population(ffi, 3)                               # one pair outside the packed-log form: the generic stores serve all
    items[1].log.obs[0], items[1].log.act = items[1].log.act, items[1].log.obs[0]
    assert call(ffi, items)[0] == ffi.SSC_OK


@pytest.mark.parametrize("change", [dict(h1=128), dict(h2=64), dict(h1=200, h2=100), dict(precision=0), dict(precision=2),
                                    dict(act_dim=2), dict(ln="fp32"), "random"])
def test_rollout_other_policies_are_unsupported_and_name_the_pair(ffi, change):
    items = population(ffi, 4)
    if change == "random":
        items[2].policy.kind = ffi.SSC_POLICY_RANDOM
    elif "ln" in change:                                     # LayerNorm actors run on the fp32 policy
        a = items[2].policy.actor
        a.precision = ffi.SSC_PREC_F32
        a.ln1_g, a.ln1_b, a.ln2_g, a.ln2_b = 0x9000, 0x9100, 0x9200, 0x9300
    else:
        for k, v in change.items():
            setattr(items[2].policy.actor, k, v)
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EUNSUPPORTED and b"pair 2" in msg, msg


def _get(item, path):
    for name in path.split("."):
        item = item[int(name)] if name.isdigit() else getattr(item, name)
    return item


def _set(item, path, value):
    *head, last = path.split(".")
    for name in head:
        item = item[int(name)] if name.isdigit() else getattr(item, name)
    if last.isdigit():
        item[int(last)] = value
    else:
        setattr(item, last, value)


@pytest.mark.parametrize("mine,theirs", [("state.s0", "state.s0"), ("state.ou_x", "state.ou_x"), ("state.steps", "state.ep_ret"),
                                         ("log.obs.1", "log.obs.1"), ("log.done", "log.done"), ("log.obs2.0", "log.act"),
                                         ("ring.env_id", "ring.env_id"), ("ring.cursor", "ring.cursor"), ("d_stats", "d_stats")])
def test_rollout_two_pairs_on_one_array_are_refused(ffi, mine, theirs):
    for K in (3, 0):                                         # ... whether or not there is anything to launch
        items = population(ffi, 5)
        _set(items[3], mine, _get(items[1], theirs))
        rc, msg = call(ffi, items, K=K)
        assert rc == ffi.SSC_EINVAL and b"share" in msg and b"pairs 1 and 3" in msg, msg


# ---- ssc_replay_append_many ------------------------------------------------------------------------------------------
def rings(ffi, P, obs_dim=2, indexed=False, K=0):
    items = (ffi.ReplayAppendItem * P)()
    for p, it in enumerate(items):
        base = 0x100_0000 * (p + 1)
        r = it.ring
        r.s, r.a, r.r, r.t, r.s2 = (base + 0x1000 * k for k in range(5))
        r.capacity, r.obs_dim, r.act_dim = 100, obs_dim, 1
        if indexed:
            r.ep_steps, r.ep_run = base + 0x6000, base + 0x7000
        for c in range(obs_dim):
            it.log.obs[c], it.log.obs2[c] = base + 0x10000 + 0x1000 * c, base + 0x14000 + 0x1000 * c
        it.log.act, it.log.rew, it.log.done = base + 0x18000, base + 0x19000, base + 0x1A000
        it.K, it.n, it.reward_scale = K, 24, 1.0 + p
    return items


def append(ffi, items, n=None, starts=None, d_items=D_ITEMS, d_cursors=D_CURSORS, cursors="own"):
    cur = (ffi.PairCursor * max(len(items) if items is not None else 1, 1))() if cursors == "own" else cursors
    for c, s in zip(cur or (), starts or ()):
        c.replay_start = s
    rc = ffi.lib().ssc_replay_append_many(None if items is None else ctypes.addressof(items), d_items,
                                          None if cur is None else ctypes.addressof(cur), d_cursors,
                                          len(items) if n is None else n, None)
    return rc, ffi.lib().ssc_last_error()


def test_append_validation(ffi):
    items = rings(ffi, 3)
    assert append(ffi, items)[0] == ffi.SSC_OK                                  # nothing to append: no launch
    assert append(ffi, rings(ffi, 3, obs_dim=3, indexed=True))[0] == ffi.SSC_OK
    assert append(ffi, None, n=3)[0] == ffi.SSC_EINVAL
    assert append(ffi, items, d_items=None)[0] == ffi.SSC_EINVAL
    assert append(ffi, items, cursors=None)[0] == ffi.SSC_EINVAL
    assert append(ffi, items, d_cursors=None)[0] == ffi.SSC_EINVAL
    rc, msg = append(ffi, items, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_pairs" in msg
    items = rings(ffi, 3)
    items[2].ring.obs_dim = 3
    rc, msg = append(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"obs_dim" in msg
    items = rings(ffi, 3, indexed=True)
    items[1].ring.ep_steps = items[1].ring.ep_run = None
    rc, msg = append(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"episode index" in msg
    items = rings(ffi, 3, indexed=True)
    items[1].ring.ep_run = None
    rc, msg = append(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"come together" in msg
    items = rings(ffi, 3)
    items[1].K = -1
    rc, msg = append(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg
    rc, msg = append(ffi, rings(ffi, 3), starts=[0, 0, -5])
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg
    items = rings(ffi, 3, K=7)                                                  # the single call's array checks
    items[0].ring.s2 = None
    rc, msg = append(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 0" in msg and b"NULL ring" in msg
    items = rings(ffi, 3, K=7)
    items[2].log.obs2[1] = None
    rc, msg = append(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"NULL obs column" in msg
    rc, msg = append(ffi, rings(ffi, 3, indexed=True, K=7), starts=[0, 24, 25])    # an indexed ring takes whole steps
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"whole steps" in msg


@pytest.mark.parametrize("mine,theirs", [("s", "s"), ("t", "t"), ("r", "a"), ("ep_steps", "ep_steps"), ("ep_run", "ep_run")])
def test_append_two_pairs_on_one_ring_array_are_refused(ffi, mine, theirs):
    items = rings(ffi, 4, indexed=True)
    setattr(items[2].ring, mine, getattr(items[0].ring, theirs))
    rc, msg = append(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"share" in msg and b"pairs 0 and 2" in msg, msg


# ---- ssc_decay_schedule_many -----------------------------------------------------------------------------------------
def schedules(ffi, P, n_sched=0):
    items = (ffi.DecayItem * P)()
    for p, it in enumerate(items):
        base = 0x100_0000 * (p + 1)
        it.d_finished, it.finished0, it.per_generation, it.n_sched, it.d_state = base, 0.0, 8.0, n_sched, base + 0x1000
        for i in range(4):
            it.factor[i], it.floor[i] = 0.99, 0.1
    return items


def decay(ffi, items, n=None, d_items=D_ITEMS):
    rc = ffi.lib().ssc_decay_schedule_many(None if items is None else ctypes.addressof(items), d_items,
                                           len(items) if n is None else n, None)
    return rc, ffi.lib().ssc_last_error()


def test_decay_validation(ffi):
    assert decay(ffi, schedules(ffi, 3))[0] == ffi.SSC_OK                       # no schedule anywhere: no launch
    assert decay(ffi, None, n=2)[0] == ffi.SSC_EINVAL
    assert decay(ffi, schedules(ffi, 2), d_items=None)[0] == ffi.SSC_EINVAL
    rc, msg = decay(ffi, schedules(ffi, 2), n=0)
    assert rc == ffi.SSC_EINVAL and b"n_pairs" in msg
    for field, value, word in (("n_sched", 5, b"n_sched"), ("per_generation", 0.0, b"per_generation"), ("d_state", None, b"NULL"),
                               ("d_finished", None, b"NULL")):
        items = schedules(ffi, 3)
        setattr(items[1], field, value)
        rc, msg = decay(ffi, items)
        assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and word in msg, msg
    items = schedules(ffi, 3, n_sched=2)
    items[2].factor[1] = -0.5
    rc, msg = decay(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"factor" in msg
    items = schedules(ffi, 4)
    items[3].d_state = items[1].d_state
    rc, msg = decay(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"share" in msg and b"pairs 1 and 3" in msg


# ---- ssc_obs_rms_update_many -----------------------------------------------------------------------------------------
def blocks(ffi, P, obs_dim=2):
    items = (ffi.ObsRmsItem * P)()
    need = ffi.lib().ssc_obs_rms_update_workspace_bytes(obs_dim)
    for p, it in enumerate(items):
        base = 0x100_0000 * (p + 1)
        for c in range(obs_dim):
            it.log.obs[c] = base + 0x1000 * c
        it.k0, it.K, it.n, it.d_rms, it.d_workspace, it.workspace_bytes = 0, 4, 64, base + 0x8000, base + 0x10000, need
    return items


def rms(ffi, items, obs_dim=2, n=None, d_items=D_ITEMS):
    rc = ffi.lib().ssc_obs_rms_update_many(obs_dim, None if items is None else ctypes.addressof(items), d_items,
                                           len(items) if n is None else n, None)
    return rc, ffi.lib().ssc_last_error()


def test_obs_rms_validation(ffi):
    assert rms(ffi, None, n=2)[0] == ffi.SSC_EINVAL
    assert rms(ffi, blocks(ffi, 2), d_items=None)[0] == ffi.SSC_EINVAL
    rc, msg = rms(ffi, blocks(ffi, 2), n=0)
    assert rc == ffi.SSC_EINVAL and b"n_pairs" in msg
    assert rms(ffi, blocks(ffi, 2), obs_dim=0)[0] == ffi.SSC_EINVAL
    assert rms(ffi, blocks(ffi, 2), obs_dim=4)[0] == ffi.SSC_EINVAL             # a transition log holds up to 3 columns
    for field, value, word in (("d_rms", None, b"NULL"), ("K", 0, b"k0"), ("k0", -1, b"k0"), ("n", 0, b"n < 1"),
                               ("workspace_bytes", 16, b"workspace"), ("d_workspace", None, b"workspace")):
        items = blocks(ffi, 3)
        setattr(items[2], field, value)
        rc, msg = rms(ffi, items)
        assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and word in msg, msg
    items = blocks(ffi, 3, obs_dim=3)
    items[1].log.obs[2] = None
    rc, msg = rms(ffi, items, obs_dim=3)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"column 2" in msg
    items = blocks(ffi, 3)
    items[0].log.row_stride = 10
    rc, msg = rms(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 0" in msg and b"stride" in msg
    for field in ("d_rms", "d_workspace"):
        items = blocks(ffi, 4)
        setattr(items[3], field, getattr(items[0], field))
        rc, msg = rms(ffi, items)
        assert rc == ffi.SSC_EINVAL and b"share" in msg and b"pairs 0 and 3" in msg


# ---- layouts ---------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"ssc_pair_cursor": "PairCursor", "ssc_rollout_many_item": "RolloutManyItem",
               "ssc_replay_append_item": "ReplayAppendItem", "ssc_decay_item": "DecayItem", "ssc_obs_rms_item": "ObsRmsItem"}


def test_new_struct_layouts_match_header(ffi, tmp_path):
    """sizeof() and offsetof() of every field of the new structs as the C compiler sees them == the ctypes mirrors; all
    sit in the struct-layout table of _ffi.py, and the header's field lists hold nothing the mirrors lack."""
    for c_name, py_name in NEW_STRUCTS.items():
        assert ffi.STRUCTS[c_name] is getattr(ffi, py_name)
    assert ctypes.sizeof(ffi.PairCursor) == 16
    fields = [(n, f) for n, m in NEW_STRUCTS.items() for f, _ in getattr(ffi, m)._fields_]
    lines = [f'printf("%zu\\n", sizeof({n}));' for n in NEW_STRUCTS]
    lines += [f'printf("%zu\\n", offsetof({n}, {f}));' for n, f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssc.h"\nint main(){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    sizes, offsets = got[:len(NEW_STRUCTS)], got[len(NEW_STRUCTS):]
    assert sizes == [ctypes.sizeof(getattr(ffi, m)) for m in NEW_STRUCTS.values()], sizes
    expect = [getattr(getattr(ffi, NEW_STRUCTS[n]), f).offset for n, f in fields]
    assert offsets == expect, [(n, f, o, e) for (n, f), o, e in zip(fields, offsets, expect) if o != e]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssc.h")).read(), flags=re.S)
    for n, m in NEW_STRUCTS.items():
        body = re.search(r"struct\s+%s\s*\{(.*?)\}\s*;" % n, text, flags=re.S).group(1)
        members = [x for decl in body.split(";") if decl.strip() for x in decl.split(",")]
        assert len(members) == len(getattr(ffi, m)._fields_), (n, members)
