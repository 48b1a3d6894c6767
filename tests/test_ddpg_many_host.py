"""ssc_ddpg_train_many / ssc_replay_sample_many: everything the two entry points decide on the host, before any HIP
call -- so none of this needs a GPU.  The pointers are made-up addresses: a call that passed validation with work to do
would launch, so every case here either fails validation or has nothing to launch."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ITEMS = 0x7000_0000          # "device copy": never read on the host
ARRAYS = ("actor", "critic", "target_actor", "target_critic", "adam_m_actor", "adam_v_actor", "adam_m_critic", "adam_v_critic",
          "adam_t")


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def population(ffi, P, n_iters=1, rms=False, **desc):
    """P valid items of the shipped shape, every array at an address of its own"""
    items = (ffi.DdpgManyItem * P)()
    for p, it in enumerate(items):
        d = it.ddpg
        d.obs_dim, d.act_dim, d.actor_h1, d.actor_h2, d.critic_h1, d.critic_h2 = 2, 1, 64, 32, 64, 32
        d.last_layer_tanh, d.batch_size = 1, 64
        base = 0x10_0000 * (p + 1)
        for k, name in enumerate(ARRAYS):
            setattr(d, name, base + 0x1000 * k)
        d.gamma, d.tau, d.actor_lr, d.critic_lr = 0.99, 0.001, 1e-4, 1e-3
        d.beta1, d.beta2, d.epsilon, d.obs_clip = 0.9, 0.999, 1e-8, 5.0
        for k, v in desc.items():
            setattr(d, k, v)
        r = it.replay
        r.s, r.a, r.r, r.t, r.s2, r.capacity = base + 0xA000, base + 0xB000, base + 0xC000, base + 0xD000, base + 0xE000, 256
        it.d_batch_idx, it.d_losses = base + 0xF000, base + 0xF800
        it.d_rms = base + 0xFC00 if rms else None
        it.n_iters = n_iters
    return items


def call(ffi, items, n=None, d_items=D_ITEMS):
    rc = ffi.lib().ssc_ddpg_train_many(None if items is None else ctypes.addressof(items), d_items,
                                       len(items) if n is None else n, None)
    return rc, ffi.lib().ssc_last_error()


def test_null_arrays_and_empty_population(ffi):
    items = population(ffi, 2, n_iters=0)
    assert call(ffi, None, n=2)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, d_items=None)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_agents" in msg
    assert call(ffi, items, n=-3)[0] == ffi.SSC_EINVAL


def test_all_zero_iterations_is_ok_without_a_launch(ffi):
    assert call(ffi, population(ffi, 4, n_iters=0))[0] == ffi.SSC_OK
    items = population(ffi, 3, n_iters=0)       # an agent with nothing to do may bring no arrays at all
    for name in ARRAYS:
        setattr(items[1].ddpg, name, None)
    items[1].d_batch_idx = None
    assert call(ffi, items)[0] == ffi.SSC_OK


@pytest.mark.parametrize("field,value", [("actor_h1", 128), ("critic_h2", 64), ("batch_size", 128), ("layer_norm", 1),
                                         ("critic_l2_reg", 1e-2), ("clip_norm", 0.5), ("obs_dim", 4), ("act_dim", 2)])
def test_other_shapes_are_unsupported_and_name_the_agent(ffi, field, value):
    items = population(ffi, 4, n_iters=0)
    setattr(items[2].ddpg, field, value)
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EUNSUPPORTED and b"agent 2" in msg, msg


def test_every_item_passes_the_single_agent_checks(ffi):
    items = population(ffi, 3)
    items[1].n_iters = -1
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"agent 1" in msg and b"n_iters" in msg
    items = population(ffi, 3)
    items[2].ddpg.adam_v_critic = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"agent 2" in msg and b"NULL" in msg
    items = population(ffi, 3)
    items[0].d_batch_idx = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"agent 0" in msg
    items = population(ffi, 2)
    items[1].ddpg.batch_size = 0
    assert call(ffi, items)[0] == ffi.SSC_EINVAL


def test_one_instantiation_per_launch(ffi):
    items = population(ffi, 3, n_iters=0)
    items[2].ddpg.obs_dim = 3
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"agent 2" in msg and b"obs_dim" in msg
    items = population(ffi, 3, n_iters=0)
    items[1].ddpg.last_layer_tanh = 0
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"agent 1" in msg and b"last_layer_tanh" in msg


def test_statistics_for_all_agents_or_for_none(ffi):
    items = population(ffi, 3, n_iters=0, rms=True)
    assert call(ffi, items)[0] == ffi.SSC_OK
    items[1].d_rms = None
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"agent 1" in msg and b"d_rms" in msg
    items = population(ffi, 3, n_iters=0)
    items[2].d_rms = 0x5000
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"agent 2" in msg


@pytest.mark.parametrize("mine,theirs", [("critic", "critic"), ("adam_t", "adam_t"), ("target_actor", "actor"),
                                         ("adam_m_actor", "adam_v_critic")])
def test_two_agents_on_one_array_are_refused(ffi, mine, theirs):
    items = population(ffi, 5)
    setattr(items[3].ddpg, mine, getattr(items[1].ddpg, theirs))
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"share" in msg and b"1" in msg and b"3" in msg, msg
    items = population(ffi, 5, n_iters=0)          # ... whether or not there is anything to launch
    setattr(items[3].ddpg, mine, getattr(items[1].ddpg, theirs))
    assert call(ffi, items)[0] == ffi.SSC_EINVAL


# ---- ssc_replay_sample_many ----------------------------------------------------------------------------------------
def keys(ffi, sizes):
    ks = (ffi.ReplaySampleKey * len(sizes))()
    for p, (k, size) in enumerate(zip(ks, sizes)):
        k.seed, k.counter0, k.size = 11 + p, 100 * p, size
    return ks


def sample(ffi, ks, n_batches=3, batch=64, n=None, d_keys=D_ITEMS, d_idx=0x6000_0000):
    rc = ffi.lib().ssc_replay_sample_many(None if ks is None else ctypes.addressof(ks), d_keys, len(ks) if n is None else n,
                                          n_batches, batch, d_idx, None)
    return rc, ffi.lib().ssc_last_error()


def test_sampler_validation(ffi):
    ks = keys(ffi, [64, 1000, 70])
    assert sample(ffi, None, n=3)[0] == ffi.SSC_EINVAL
    assert sample(ffi, ks, d_keys=None)[0] == ffi.SSC_EINVAL
    assert sample(ffi, ks, n=0)[0] == ffi.SSC_EINVAL
    rc, msg = sample(ffi, ks, batch=65)
    assert rc == ffi.SSC_EUNSUPPORTED and b"65" in msg
    assert sample(ffi, ks, batch=0)[0] == ffi.SSC_EINVAL
    assert sample(ffi, ks, n_batches=-1)[0] == ffi.SSC_EINVAL
    rc, msg = sample(ffi, keys(ffi, [64, 63, 70]))
    assert rc == ffi.SSC_EINVAL and b"agent 1" in msg and b"63" in msg
    assert sample(ffi, keys(ffi, [64, 70, 1 << 31]))[0] == ffi.SSC_EINVAL        # int32 indices
    assert sample(ffi, ks, d_idx=None)[0] == ffi.SSC_EINVAL
    assert sample(ffi, ks, n_batches=0, d_idx=None)[0] == ffi.SSC_OK             # nothing to draw
    assert sample(ffi, keys(ffi, [17, 17]), n_batches=0, batch=17)[0] == ffi.SSC_OK


# ---- layouts ---------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"ssc_ddpg_many_item": "DdpgManyItem", "ssc_replay_sample_key": "ReplaySampleKey"}


def test_new_struct_layouts_match_header(ffi, tmp_path):
    """sizeof() and offsetof() of every field of the two new structs as the C compiler sees them == the ctypes mirrors;
    both sit in the struct-layout table of _ffi.py, and the header's field lists hold nothing the mirrors lack."""
    for c_name, py_name in NEW_STRUCTS.items():
        assert ffi.STRUCTS[c_name] is getattr(ffi, py_name)
    assert all(issubclass(v, ctypes.Structure) for v in ffi.STRUCTS.values())
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
