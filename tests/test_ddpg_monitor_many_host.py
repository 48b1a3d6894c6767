"""ssc_ddpg_eval_rollout_many / ssc_ddpg_stats_many: everything the two entry points decide on the host, before any HIP
call -- so none of this needs a GPU.  The pointers are made-up addresses: a call that passed validation with work to do
would launch, so every case here either fails validation or has nothing to launch (K == 0, every m == 0)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ITEMS, D_CURSORS = 0x7000_0000, 0x7100_0000          # "device copies": never read on the host
NET_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")
LN_KEYS = ("ln1_g", "ln1_b", "ln2_g", "ln2_b")


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def point(desc, base, obs_dim, h1, h2, ln=False):
    desc.obs_dim, desc.h1, desc.h2, desc.act_dim = obs_dim, h1, h2, 1
    for k, name in enumerate(NET_KEYS + (LN_KEYS if ln else ())):
        setattr(desc, name, base + 0x1000 * k)
    desc.last_layer_tanh, desc.obs_clip = 1, 5.0


# ---- ssc_ddpg_eval_rollout_many --------------------------------------------------------------------------------------
def eval_population(ffi, P, kind=0, shapes=((64, 32),), rms=False, ln=False):
    """P valid pairs, every array at an address of its own; pair p has the layer sizes shapes[p % len(shapes)]"""
    items = (ffi.DdpgEvalManyItem * P)()
    obs_dim = 2 if kind == ffi.SSC_ENV_MOUNTAINCAR else 3
    for p, it in enumerate(items):
        base = 0x100_0000 * (p + 1)
        h1, h2 = shapes[p % len(shapes)]
        it.params = ffi.default_params(kind, 1.0, 200)
        point(it.actor, base, obs_dim, h1, h2, ln)
        point(it.critic, base + 0x10000, obs_dim, h1, h2, ln)
        it.act_low, it.act_high = (-1.0, 1.0) if obs_dim == 2 else (-2.0, 2.0)
        it.n = 1 + 16 * p
        st = it.state
        st.s0, st.s1, st.steps, st.ep_ret = (base + 0x20000 + 0x1000 * k for k in range(4))
        it.d_rms = base + 0x30000 if rms else None
        it.d_out, it.d_workspace = base + 0x40000, base + 0x50000
        it.workspace_bytes = ffi.lib().ssc_ddpg_eval_workspace_bytes(it.n)
        it.seed, it.env_id0 = 11 + p, 1000 * p
    return items


def eval_call(ffi, items, K=0, n=None, d_items=D_ITEMS, cursors="own", d_cursors=D_CURSORS, zero_returns=1):
    cur = (ffi.PairCursor * max(len(items) if items is not None else 1, 1))() if cursors == "own" else cursors
    rc = ffi.lib().ssc_ddpg_eval_rollout_many(None if items is None else ctypes.addressof(items), d_items,
                                              None if cur is None else ctypes.addressof(cur), d_cursors,
                                              len(items) if n is None else n, K, zero_returns, None)
    return rc, ffi.lib().ssc_last_error()


def test_eval_null_arrays_and_empty_population(ffi):
    items = eval_population(ffi, 2)
    assert eval_call(ffi, None, n=2)[0] == ffi.SSC_EINVAL
    assert eval_call(ffi, items, d_items=None)[0] == ffi.SSC_EINVAL
    assert eval_call(ffi, items, cursors=None)[0] == ffi.SSC_EINVAL
    assert eval_call(ffi, items, d_cursors=None)[0] == ffi.SSC_EINVAL
    rc, msg = eval_call(ffi, items, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_pairs" in msg
    assert eval_call(ffi, items, n=-3)[0] == ffi.SSC_EINVAL
    rc, msg = eval_call(ffi, items, K=-1)
    assert rc == ffi.SSC_EINVAL and b"K = -1" in msg


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("rms", [False, True])
def test_eval_no_steps_is_ok_without_a_launch(ffi, kind, rms):
    assert eval_call(ffi, eval_population(ffi, 4, kind=kind, rms=rms))[0] == ffi.SSC_OK
    assert eval_call(ffi, eval_population(ffi, 4, kind=kind, rms=rms), zero_returns=0)[0] == ffi.SSC_OK
    # per pair at run time: the shapes (64-32 | a LayerNorm-sized odd one | 128-64 | 200-100: its weights stay in global
    # memory), the statistics, LayerNorm, last_layer_tanh
    items = eval_population(ffi, 5, kind=kind, rms=rms, shapes=((64, 32), (7, 5), (128, 64), (200, 100)))
    items[1].d_rms = None if rms else 0x5000
    items[2].actor.last_layer_tanh = items[2].critic.last_layer_tanh = 0
    for name in LN_KEYS:
        setattr(items[1].actor, name, 0x9000 + 0x100 * LN_KEYS.index(name))
        setattr(items[1].critic, name, 0xA000 + 0x100 * LN_KEYS.index(name))
    assert eval_call(ffi, items)[0] == ffi.SSC_OK
    assert eval_call(ffi, eval_population(ffi, 3, kind=kind, ln=True))[0] == ffi.SSC_OK


def test_eval_every_item_passes_the_single_call_checks(ffi):
    def bad(change, code=None, pair=1, word=b""):
        items = eval_population(ffi, 3)
        change(items[pair])
        rc, msg = eval_call(ffi, items)
        assert rc == (ffi.SSC_EINVAL if code is None else code), msg
        assert b"pair %d" % pair in msg and word in msg, msg

    bad(lambda it: setattr(it, "d_out", None), word=b"output block")
    bad(lambda it: setattr(it, "n", 0), word=b"n = 0")
    bad(lambda it: setattr(it, "n", (1 << 30) + 1), pair=2)
    bad(lambda it: setattr(it.params, "kind", 7), word=b"env kind")
    bad(lambda it: setattr(it.actor, "obs_dim", 3), word=b"obs_dim")
    bad(lambda it: setattr(it.critic, "obs_dim", 3), pair=0, word=b"obs_dim")
    bad(lambda it: setattr(it.critic, "act_dim", 2), word=b"act_dim")

    def two_actions(it):
        it.actor.act_dim = it.critic.act_dim = 2
    bad(two_actions, code=ffi.SSC_EUNSUPPORTED, word=b"act_dim 2")
    bad(lambda it: setattr(it.actor, "h2", 0), word=b"hidden sizes")
    bad(lambda it: setattr(it, "act_low", 3.0), word=b"act_low")
    bad(lambda it: setattr(it.state, "ep_ret", None), pair=2, word=b"NULL state")
    bad(lambda it: setattr(it.actor, "W2", None), word=b"actor")
    bad(lambda it: setattr(it.critic, "b3", None), word=b"critic")
    bad(lambda it: setattr(it.actor, "ln2_g", 0x9000), word=b"LayerNorm")
    bad(lambda it: setattr(it.params, "max_position", 3.0), code=ffi.SSC_EUNSUPPORTED, pair=2, word=b"position")   # validate_mc_params

    def wide(it):                                                            # a tile's activations alone exceed LDS
        it.actor.h1 = it.critic.h1 = 3000
    bad(wide, code=ffi.SSC_EUNSUPPORTED, word=b"LDS")


def test_eval_undersized_workspace_is_refused(ffi):
    items = eval_population(ffi, 3)
    items[2].workspace_bytes -= 1
    rc, msg = eval_call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"workspace" in msg
    items = eval_population(ffi, 3)
    items[1].n = 33                                                          # a third workgroup: a third record
    rc, msg = eval_call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 1" in msg and b"workspace" in msg
    items = eval_population(ffi, 3)
    items[0].d_workspace = None
    rc, msg = eval_call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 0" in msg and b"workspace" in msg


def test_eval_env_kind_is_uniform(ffi):
    items = eval_population(ffi, 3)
    pend = eval_population(ffi, 3, kind=1)
    ctypes.memmove(ctypes.addressof(items[2]), ctypes.addressof(pend[2]), ctypes.sizeof(ffi.DdpgEvalManyItem))
    rc, msg = eval_call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"env kind" in msg and b"pair 0" in msg


@pytest.mark.parametrize("mine,theirs", [("state.s0", "state.s0"), ("state.s1", "state.s1"), ("state.steps", "state.ep_ret"),
                                         ("state.ep_ret", "state.ep_ret"), ("d_out", "d_out"), ("d_workspace", "d_workspace"),
                                         ("d_out", "d_workspace")])
def test_eval_two_pairs_on_one_array_are_refused(ffi, mine, theirs):
    def get(item, path):
        for name in path.split("."):
            item = getattr(item, name)
        return item

    for K in (3, 0):                                                         # ... whether or not there is anything to launch
        items = eval_population(ffi, 5)
        *head, last = mine.split(".")
        setattr(get(items[3], ".".join(head)) if head else items[3], last, get(items[1], theirs))
        rc, msg = eval_call(ffi, items, K=K)
        assert rc == ffi.SSC_EINVAL and b"share" in msg and b"pairs 1 and 3" in msg, msg


def test_eval_shared_weights_are_accepted(ffi):
    """weights are only read: one agent evaluated on two env sets, and the same statistics block, are legal"""
    items = eval_population(ffi, 4, rms=True)
    for name in NET_KEYS:
        setattr(items[2].actor, name, getattr(items[0].actor, name))
        setattr(items[2].critic, name, getattr(items[0].critic, name))
    items[2].d_rms = items[0].d_rms
    assert eval_call(ffi, items)[0] == ffi.SSC_OK


# ---- ssc_ddpg_stats_many ---------------------------------------------------------------------------------------------
def stats_population(ffi, P, m=0, obs_dim=2, pert=False, rms=False):
    items = (ffi.DdpgStatsManyItem * P)()
    for p, it in enumerate(items):
        base = 0x100_0000 * (p + 1)
        point(it.actor, base, obs_dim, 64, 32)
        point(it.critic, base + 0x10000, obs_dim, 64, 32)
        if pert:
            point(it.perturbed, base + 0x20000, obs_dim, 64, 32)
            it.has_perturbed, it.d_param_noise_stddev = 1, base + 0x28000
        it.m = m
        it.d_obs, it.d_act = base + 0x30000, base + 0x38000
        it.d_rms = base + 0x3C000 if rms else None
        it.d_out, it.d_workspace = base + 0x40000, base + 0x50000
        it.workspace_bytes = ffi.lib().ssc_ddpg_stats_workspace_bytes(max(m, 1))
    return items


def stats_call(ffi, items, n=None, d_items=D_ITEMS):
    rc = ffi.lib().ssc_ddpg_stats_many(None if items is None else ctypes.addressof(items), d_items,
                                       len(items) if n is None else n, None)
    return rc, ffi.lib().ssc_last_error()


def test_stats_null_arrays_and_empty_population(ffi):
    items = stats_population(ffi, 2)
    assert stats_call(ffi, None, n=2)[0] == ffi.SSC_EINVAL
    assert stats_call(ffi, items, d_items=None)[0] == ffi.SSC_EINVAL
    rc, msg = stats_call(ffi, items, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_pairs" in msg
    assert stats_call(ffi, items, n=-1)[0] == ffi.SSC_EINVAL


def test_stats_no_sample_anywhere_is_ok_without_a_launch(ffi):
    assert stats_call(ffi, stats_population(ffi, 4))[0] == ffi.SSC_OK
    assert stats_call(ffi, stats_population(ffi, 3, obs_dim=3, pert=True, rms=True))[0] == ffi.SSC_OK
    items = stats_population(ffi, 3)                         # a skipped pair's item is not read at all
    ctypes.memset(ctypes.addressof(items[1]), 0, ctypes.sizeof(ffi.DdpgStatsManyItem))
    items[2].d_out = items[0].d_out
    assert stats_call(ffi, items)[0] == ffi.SSC_OK


def test_stats_every_item_passes_the_single_call_checks(ffi):
    """reached with a sample on the faulty pair only: the others are skipped, and validation fails before any launch"""
    def bad(change, code=None, pair=1, word=b"", **kw):
        items = stats_population(ffi, 3, **kw)
        items[pair].m = 16
        change(items[pair])
        rc, msg = stats_call(ffi, items)
        assert rc == (ffi.SSC_EINVAL if code is None else code), msg
        assert b"pair %d" % pair in msg and word in msg, msg

    bad(lambda it: setattr(it, "d_out", None), word=b"output block")
    bad(lambda it: setattr(it, "m", 4097), word=b"4097")
    bad(lambda it: setattr(it, "m", -2), pair=2, word=b"-2")
    bad(lambda it: setattr(it.actor, "obs_dim", 9), word=b"obs_dim")
    bad(lambda it: setattr(it.critic, "obs_dim", 3), pair=0, word=b"critic")
    bad(lambda it: setattr(it.critic, "h1", 0), word=b"hidden sizes")
    bad(lambda it: setattr(it.perturbed, "h1", 63), word=b"perturbed", pert=True)
    bad(lambda it: setattr(it, "d_obs", None), word=b"NULL sample")
    bad(lambda it: setattr(it, "d_act", None), pair=2, word=b"NULL sample")
    bad(lambda it: setattr(it.actor, "W3", None), word=b"actor")
    bad(lambda it: setattr(it.critic, "W1", None), word=b"critic")
    bad(lambda it: setattr(it.perturbed, "b2", None), word=b"perturbed actor", pert=True)
    bad(lambda it: setattr(it.critic, "ln1_b", 0x9000), word=b"LayerNorm")
    bad(lambda it: setattr(it, "workspace_bytes", it.workspace_bytes - 1), word=b"workspace")
    bad(lambda it: setattr(it, "m", 17), word=b"workspace")                  # a second tile: a second record
    bad(lambda it: setattr(it, "d_workspace", None), pair=0, word=b"workspace")

    def wide(it):
        it.actor.h1 = it.critic.h1 = 3000
    bad(wide, code=ffi.SSC_EUNSUPPORTED, word=b"LDS")


@pytest.mark.parametrize("mine,theirs", [("d_out", "d_out"), ("d_workspace", "d_workspace"), ("d_workspace", "d_out")])
def test_stats_two_pairs_on_one_block_are_refused(ffi, mine, theirs):
    items = stats_population(ffi, 5, m=16)
    items[0].m = 0
    setattr(items[3], mine, getattr(items[1], theirs))
    items[4].d_obs = items[2].d_obs                          # samples and weights are only read: shared ones are legal
    for name in NET_KEYS:
        setattr(items[4].actor, name, getattr(items[2].actor, name))
    rc, msg = stats_call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"share" in msg and b"pairs 1 and 3" in msg, msg


# ---- layouts ---------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"ssc_ddpg_eval_many_item": "DdpgEvalManyItem", "ssc_ddpg_stats_many_item": "DdpgStatsManyItem"}


def test_new_struct_layouts_match_header(ffi, tmp_path):
    """sizeof() and offsetof() of every field of the new structs as the C compiler sees them == the ctypes mirrors; both
    sit in the struct-layout table of _ffi.py, and the header's field lists hold nothing the mirrors lack."""
    for c_name, py_name in NEW_STRUCTS.items():
        assert ffi.STRUCTS[c_name] is getattr(ffi, py_name)
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
