"""ssc_ddpg_train_many_wide / ssc_ddpg_train_many_wide_plan / ssc_ddpg_learner_path: everything the grouped
multi-workgroup learner decides on the host, before any HIP call -- so none of this needs a GPU.  The pointers are made-up
addresses (the plan builder only copies them): every call of the launching entry point here fails validation or has
nothing to launch."""
import ctypes
import os
import re
import subprocess

import pytest

from tests.test_ddpg_layout_host import PATHS, _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_PLAN = 0x7000_0000           # "device copy": never read on the host
ARRAYS = ("actor", "critic", "target_actor", "target_critic", "adam_m_actor", "adam_v_actor", "adam_m_critic", "adam_v_critic",
          "adam_t")
# shapes ssc_ddpg_train_ws runs on the multi-workgroup kernels: (actor, critic, batch, extra descriptor fields)
SHAPES = [((128, 64), (64, 32), 64, {}), ((200, 100), (200, 100), 17, {}), ((7, 5), (9, 3), 16, dict(obs_dim=3, last_layer_tanh=0)),
          ((64, 32), (64, 32), 48, dict(layer_norm=1)), ((64, 32), (64, 32), 64, dict(critic_l2_reg=1e-2, clip_norm=0.5))]


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


@pytest.fixture(autouse=True)
def _no_path_switches(monkeypatch):
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)


def fill(ffi, it, p, shape, n_iters=1, rms=False):
    """a valid item of SHAPES[shape] with every array, its workspace included, at an address of its own"""
    (a1, a2), (c1, c2), batch, extra = SHAPES[shape % len(SHAPES)]
    d = it.ddpg
    d.obs_dim, d.act_dim, d.actor_h1, d.actor_h2, d.critic_h1, d.critic_h2 = 2, 1, a1, a2, c1, c2
    d.last_layer_tanh, d.batch_size = 1, batch
    base = 0x1000_0000 * (p + 1)
    for k, name in enumerate(ARRAYS):
        setattr(d, name, base + 0x10_0000 * k)
    d.gamma, d.tau, d.actor_lr, d.critic_lr = 0.99, 0.001, 1e-4, 1e-3
    d.beta1, d.beta2, d.epsilon, d.obs_clip = 0.9, 0.999, 1e-8, 5.0
    for k, v in extra.items():
        setattr(d, k, v)
    r = it.replay
    r.s, r.a, r.r, r.t, r.s2, r.capacity = base + 0xA0_0000, base + 0xA1_0000, base + 0xA2_0000, base + 0xA3_0000, base + 0xA4_0000, 256
    it.d_batch_idx, it.d_losses = base + 0xA5_0000, base + 0xA6_0000
    it.d_rms = base + 0xA7_0000 if rms else None
    it.n_iters = n_iters
    it.d_workspace, it.workspace_bytes = base + 0x100_0000, ffi.lib().ssc_ddpg_train_workspace_bytes(ctypes.byref(d))


def population(ffi, P, n_iters=1, rms=False, shapes=None):
    items = (ffi.DdpgManyWideItem * P)()
    for p, it in enumerate(items):
        fill(ffi, it, p, p if shapes is None else shapes[p], n_iters, rms)
    return items


def plan(ffi, items, n=None, short=0, buf="make"):
    """-> (rc, message, plan bytes)"""
    lib = ffi.lib()
    n = len(items) if n is None else n
    nbytes = lib.ssc_ddpg_train_many_wide_plan_bytes(max(n, 1))
    mem = (ctypes.c_uint64 * ((nbytes + 7) // 8))() if buf == "make" else buf
    rc = lib.ssc_ddpg_train_many_wide_plan(None if items is None else ctypes.addressof(items), n,
                                           None if mem is None else ctypes.addressof(mem), nbytes - short)
    return rc, lib.ssc_last_error(), None if mem is None else bytes(mem)[:nbytes]


def train(ffi, items, h_plan, n=None, d_plan=D_PLAN):
    lib = ffi.lib()
    keep = None if h_plan is None else ctypes.create_string_buffer(h_plan, len(h_plan))
    rc = lib.ssc_ddpg_train_many_wide(None if items is None else ctypes.addressof(items), None if keep is None else ctypes.addressof(keep),
                                      d_plan, len(items) if n is None else n, None)
    return rc, lib.ssc_last_error()


def refused_by_both(ffi, items, code, *words):
    """the plan builder and the launching call walk the items the same way"""
    ok = plan(ffi, population(ffi, len(items), n_iters=0))[2]         # any buffer of the right size
    for rc, msg in (plan(ffi, items)[:2], train(ffi, items, ok)):
        assert rc == code and all(w in msg for w in words), (rc, msg)


def test_null_arrays_and_empty_population(ffi):
    items = population(ffi, 2, n_iters=0)
    rc, _, ok = plan(ffi, items)
    assert rc == ffi.SSC_OK
    assert plan(ffi, None, n=2)[0] == ffi.SSC_EINVAL and train(ffi, None, ok, n=2)[0] == ffi.SSC_EINVAL
    assert plan(ffi, items, buf=None)[0] == ffi.SSC_EINVAL
    assert train(ffi, items, None)[0] == ffi.SSC_EINVAL and train(ffi, items, ok, d_plan=None)[0] == ffi.SSC_EINVAL
    for n in (0, -3):
        rc, msg, _ = plan(ffi, items, n=n)
        assert rc == ffi.SSC_EINVAL and b"n_agents" in msg
        rc, msg = train(ffi, items, ok, n=n)
        assert rc == ffi.SSC_EINVAL and b"n_agents" in msg


def test_all_zero_iterations_is_ok_without_a_launch(ffi):
    items = population(ffi, 4, n_iters=0)
    rc, _, h_plan = plan(ffi, items)
    assert rc == ffi.SSC_OK and train(ffi, items, h_plan)[0] == ffi.SSC_OK
    items = population(ffi, 3, n_iters=0)          # an agent with nothing to do may bring no arrays at all
    for name in ARRAYS:
        setattr(items[1].ddpg, name, None)
    items[1].d_batch_idx = items[1].d_workspace = None
    items[1].workspace_bytes = 0
    rc, _, h_plan = plan(ffi, items)
    assert rc == ffi.SSC_OK and train(ffi, items, h_plan)[0] == ffi.SSC_OK


def test_every_item_passes_the_single_agent_checks(ffi):
    items = population(ffi, 3)
    items[1].n_iters = -1
    refused_by_both(ffi, items, ffi.SSC_EINVAL, b"agent 1", b"n_iters")
    items = population(ffi, 3)
    items[2].ddpg.adam_v_critic = None
    refused_by_both(ffi, items, ffi.SSC_EINVAL, b"agent 2", b"NULL")
    items = population(ffi, 3)
    items[0].d_batch_idx = None
    refused_by_both(ffi, items, ffi.SSC_EINVAL, b"agent 0")
    items = population(ffi, 2)
    items[1].ddpg.batch_size = 0
    refused_by_both(ffi, items, ffi.SSC_EINVAL, b"agent 1")
    items = population(ffi, 2)
    items[1].ddpg.critic_l2_reg = -1.0
    refused_by_both(ffi, items, ffi.SSC_EINVAL, b"agent 1")
    items = population(ffi, 2)
    items[0].ddpg.batch_size = 4097                # wide_batch_check
    items[0].workspace_bytes = 1 << 40
    rc, msg, _ = plan(ffi, items)
    assert rc == ffi.SSC_EUNSUPPORTED and b"agent 0" in msg and b"4097" in msg


def test_an_agent_of_another_path_is_unsupported_and_named(ffi, monkeypatch):
    shipped = dict(actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, batch_size=64)
    for fields, word in ((shipped, b"one-workgroup"), (dict(shipped, batch_size=128), b"tiled"),
                         (dict(shipped, actor_h1=48, actor_h2=24, critic_h1=48, critic_h2=24), b"interpreter")):
        items = population(ffi, 4, shapes=[0, 1, 0, 1])
        for k, v in fields.items():
            setattr(items[2].ddpg, k, v)
        refused_by_both(ffi, items, ffi.SSC_EUNSUPPORTED, b"agent 2", word)
        items[2].n_iters = 0                       # ... only where there is something to run
        assert plan(ffi, items)[0] == ffi.SSC_OK
    items = population(ffi, 4, shapes=[0, 1, 0, 1])
    for k, v in shipped.items():
        setattr(items[2].ddpg, k, v)
    monkeypatch.setenv("SSC_DDPG_WIDE", "1")       # the switch sends the shipped shape to these kernels
    assert plan(ffi, items)[0] == ffi.SSC_OK


def test_short_workspace_and_short_plan(ffi):
    items = population(ffi, 3)
    items[1].workspace_bytes -= 1
    refused_by_both(ffi, items, ffi.SSC_EINVAL, b"agent 1", b"workspace")
    items = population(ffi, 3)
    items[2].d_workspace = None
    refused_by_both(ffi, items, ffi.SSC_EINVAL, b"agent 2", b"workspace")
    items = population(ffi, 3)
    rc, msg, _ = plan(ffi, items, short=1)
    assert rc == ffi.SSC_EINVAL and b"plan" in msg
    assert plan(ffi, items, short=0)[0] == ffi.SSC_OK


def test_a_tile_above_the_lds_is_unsupported(ffi):
    items = population(ffi, 2)
    d = items[1].ddpg
    d.actor_h1 = d.actor_h2 = d.critic_h1 = d.critic_h2 = 800
    items[1].workspace_bytes = ffi.lib().ssc_ddpg_train_workspace_bytes(ctypes.byref(d))
    refused_by_both(ffi, items, ffi.SSC_EUNSUPPORTED, b"LDS")


@pytest.mark.parametrize("mine,theirs", [("critic", "critic"), ("adam_t", "adam_t"), ("target_actor", "actor"),
                                         ("adam_m_actor", "adam_v_critic"), ("d_workspace", "d_workspace"), ("d_workspace", "critic")])
def test_two_agents_on_one_array_or_workspace_are_refused(ffi, mine, theirs):
    for n_iters in (1, 0):                         # ... whether or not there is anything to launch
        items = population(ffi, 5, n_iters=n_iters)
        src = items[1] if theirs == "d_workspace" else items[1].ddpg
        setattr(items[3] if mine == "d_workspace" else items[3].ddpg, mine, getattr(src, theirs))
        refused_by_both(ffi, items, ffi.SSC_EINVAL, b"share", b"1", b"3")


def test_a_stale_plan_is_refused(ffi):
    items = population(ffi, 3)
    rc, _, h_plan = plan(ffi, items)
    assert rc == ffi.SSC_OK
    items[1].n_iters = 2
    rc, msg = train(ffi, items, h_plan)
    assert rc == ffi.SSC_EINVAL and b"plan" in msg
    items = population(ffi, 3)
    items[2].d_losses += 64
    rc, msg = train(ffi, items, h_plan)
    assert rc == ffi.SSC_EINVAL and b"plan" in msg


def test_plan_bytes_grow_linearly(ffi):
    f = ffi.lib().ssc_ddpg_train_many_wide_plan_bytes
    one = f(1)
    assert one > 0 and one % 8 == 0 and f(0) == 0 and f(-1) == 0
    assert [f(P) for P in (2, 5, 33, 180, 65535)] == [P * one for P in (2, 5, 33, 180, 65535)]


def test_an_agents_part_of_the_plan_depends_on_its_item_alone(ffi):
    """row p of a plan of five == the row of the same item planned alone, byte for byte (statistics on two of them)"""
    lib = ffi.lib()
    five = population(ffi, 5, n_iters=3)
    five[1].d_rms, five[4].d_rms = 0x5550_0000, 0x5560_0000
    five[2].n_iters = 0
    rc, _, whole = plan(ffi, five)
    assert rc == ffi.SSC_OK
    row = (lib.ssc_ddpg_train_many_wide_plan_bytes(2) - lib.ssc_ddpg_train_many_wide_plan_bytes(1)) - 16      # + four list slots
    assert row > 0 and lib.ssc_ddpg_train_many_wide_plan_bytes(1) == row + 16
    for p in range(5):
        one = (ffi.DdpgManyWideItem * 1)()
        ctypes.memmove(ctypes.addressof(one), ctypes.addressof(five[p]), ctypes.sizeof(ffi.DdpgManyWideItem))
        rc, _, alone = plan(ffi, one)
        assert rc == ffi.SSC_OK
        assert whole[p * row:(p + 1) * row] == alone[:row], p
        assert (alone[:row] == bytes(row)) == (p == 2)         # no iterations: a zeroed row
    # the four lists behind the rows: gradient launch without / with statistics, apply launch plain / prepared
    lists = [list(ctypes.cast(ctypes.create_string_buffer(whole[5 * row + 20 * k:5 * row + 20 * (k + 1)]),
                              ctypes.POINTER(ctypes.c_int32))[:5]) for k in range(4)]
    assert lists[0][:2] == [0, 3] and lists[1][:2] == [1, 4] and lists[2][:3] == [0, 1, 3] and lists[3][:1] == [4]


ENV = {(False, False): {}, (True, False): {"SSC_DDPG_INTERPRETER": "1"}, (False, True): {"SSC_DDPG_WIDE": "1"},
       (True, True): {"SSC_DDPG_INTERPRETER": "1", "SSC_DDPG_WIDE": "1"}}


@pytest.mark.parametrize("row", range(len(PATHS)))
def test_learner_path_is_the_pinned_table(ffi, monkeypatch, row):
    """ssc_ddpg_learner_path == the table tests/test_ddpg_layout_host.py pins for ddpg_learner_path, the two switches read
    from the environment"""
    kw, have_ws, have_rms, want_interp, want_wide, want = PATHS[row]
    for k, v in ENV[(want_interp, want_wide)].items():
        monkeypatch.setenv(k, v)
    assert ffi.lib().ssc_ddpg_learner_path(ctypes.byref(_desc(**kw)), int(have_ws), int(have_rms)) == want
    assert want == (ffi.SSC_DDPG_PATH_FIXED, ffi.SSC_DDPG_PATH_FIXED_TILED, ffi.SSC_DDPG_PATH_INTERPRETER, ffi.SSC_DDPG_PATH_WIDE,
                    ffi.SSC_DDPG_PATH_NEEDS_WORKSPACE)[want]


def test_learner_path_refuses_what_it_cannot_size(ffi):
    lib = ffi.lib()
    assert lib.ssc_ddpg_learner_path(None, 1, 0) == ffi.SSC_EINVAL
    assert lib.ssc_ddpg_learner_path(ctypes.byref(_desc(B=0)), 1, 0) == ffi.SSC_EINVAL
    monkey = _desc()
    monkey.actor_h1 = 0
    assert lib.ssc_ddpg_learner_path(ctypes.byref(monkey), 1, 0) == ffi.SSC_EINVAL


def test_new_struct_layout_matches_header(ffi, tmp_path):
    """sizeof() and offsetof() of every field of ssc_ddpg_many_wide_item as the C compiler sees them == the ctypes mirror,
    which extends ssc_ddpg_many_item's and sits in the struct-layout table; the path constants agree too."""
    n, M = "ssc_ddpg_many_wide_item", ffi.DdpgManyWideItem
    assert ffi.STRUCTS[n] is M and M._fields_[:len(ffi.DdpgManyItem._fields_)] == ffi.DdpgManyItem._fields_
    fields = [f for f, _ in M._fields_]
    lines = [f'printf("%zu\\n", sizeof({n}));'] + [f'printf("%zu\\n", offsetof({n}, {f}));' for f in fields]
    lines += [f'printf("%d\\n", (int){c});' for c in ("SSC_DDPG_PATH_FIXED", "SSC_DDPG_PATH_FIXED_TILED", "SSC_DDPG_PATH_INTERPRETER",
                                                      "SSC_DDPG_PATH_WIDE", "SSC_DDPG_PATH_NEEDS_WORKSPACE")]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssc.h"\nint main(){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(M)
    assert got[1:1 + len(fields)] == [getattr(M, f).offset for f in fields]
    assert got[1 + len(fields):] == [0, 1, 2, 3, 4]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssc.h")).read(), flags=re.S)
    body = re.search(r"struct\s+%s\s*\{(.*?)\}\s*;" % n, text, flags=re.S).group(1)
    assert len([x for decl in body.split(";") if decl.strip() for x in decl.split(",")]) == len(fields)
