"""ssc_param_noise_cycle_many: everything the entry point decides on the host, before any HIP call -- so none of this needs a
GPU -- and the host bookkeeping of ``DDPGPopulation.param_noise_cycle``.  The pointers are made-up addresses: a call that
passed validation with work to do would launch, so every library case here either fails validation or has nothing to
launch (every n == 0)."""
import ctypes
import os
import re
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ITEMS, D_CURSORS = 0x7000_0000, 0x7100_0000          # "device copies": never read on the host
NET_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")
LN_ORDER = ("W1", "b1", "ln1_b", "ln1_g", "W2", "b2", "ln2_b", "ln2_g", "W3", "b3")


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def counts(obs_dim, h1, h2):
    return dict(W1=obs_dim * h1, b1=h1, W2=h1 * h2, b2=h2, W3=h2, b3=1, ln1_b=h1, ln1_g=h1, ln2_b=h2, ln2_g=h2)


def fill(it, base, obs_dim=2, h1=64, h2=32, ln=False):
    """a valid item: the flat array at base, dst 1 MiB above it, every other array at an address of its own"""
    c = counts(obs_dim, h1, h2)
    it.actor.obs_dim, it.actor.h1, it.actor.h2, it.actor.act_dim = obs_dim, h1, h2, 1
    off, at = 0, {}
    for k in (LN_ORDER if ln else NET_KEYS):
        setattr(it.actor, k, base + 4 * off)
        at[k] = off
        off += c[k]
    it.actor.last_layer_tanh, it.actor.obs_clip = 1, 5.0
    it.n, it.d_src, it.d_dst = off, base, base + 0x10_0000
    if ln:
        it.skip0_begin, it.skip0_end = at["ln1_b"], at["ln1_b"] + 2 * h1
        it.skip1_begin, it.skip1_end = at["ln2_b"], at["ln2_b"] + 2 * h2
    it.d_obs, it.d_idx, it.d_rms = base + 0x20_0000, base + 0x30_0000, None
    it.seed, it.desired, it.coefficient = 11, 0.1, 1.01
    it.d_stddev, it.d_distance = base + 0x40_0000, base + 0x40_0004


def population(ffi, P, m=64, shapes=((2, 64, 32, False),)):
    items, cursors = (ffi.ParamNoiseManyItem * P)(), (ffi.ParamNoiseCursor * P)()
    for p in range(P):
        fill(items[p], 0x1000_0000 * (p + 1), *shapes[p % len(shapes)])
        items[p].seed = 11 + p
        cursors[p].generation_adaptive, cursors[p].generation_acting, cursors[p].m = 2 * p, 2 * p + 1, m
    return items, cursors


def call(ffi, items, cursors, n=None, d_items=D_ITEMS, d_cursors=D_CURSORS):
    rc = ffi.lib().ssc_param_noise_cycle_many(None if items is None else ctypes.addressof(items), d_items,
                                              None if cursors is None else ctypes.addressof(cursors), d_cursors,
                                              len(items) if n is None else n, None)
    return rc, ffi.lib().ssc_last_error()


def bad(ffi, change, code=None, pair=1, word=b"", P=3, **kw):
    """validation fails on `pair` before any launch, with the code of the single call and the pair's index in the message"""
    items, cursors = population(ffi, P, **kw)
    change(items[pair], cursors[pair])
    rc, msg = call(ffi, items, cursors)
    assert rc == (ffi.SSC_EINVAL if code is None else code), (rc, msg)
    assert b"pair %d" % pair in msg and word in msg, msg


def test_null_arrays_and_pair_count(ffi):
    items, cursors = population(ffi, 2)
    assert call(ffi, None, cursors, n=2)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, None)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, cursors, d_items=None)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, cursors, d_cursors=None)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, cursors, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_pairs" in msg
    assert call(ffi, items, cursors, n=-1)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, cursors, n=65536)                 # refused on the count alone: the arrays are not walked
    assert rc == ffi.SSC_EUNSUPPORTED and b"65536" in msg


def test_all_empty_pairs_are_ok_without_a_launch(ffi):
    items, cursors = population(ffi, 4)
    for it in items:
        it.n = 0
    assert call(ffi, items, cursors)[0] == ffi.SSC_OK
    # nothing else of a skipped pair's item is read, and it owns nothing
    ctypes.memset(ctypes.addressof(items[1]), 0, ctypes.sizeof(ffi.ParamNoiseManyItem))
    items[2].d_stddev = items[0].d_stddev
    cursors[3].m = 9999
    assert call(ffi, items, cursors)[0] == ffi.SSC_OK


def test_every_pair_passes_the_single_call_checks(ffi):
    def put(name, value, cursor=False):
        return lambda it, cu: setattr(cu if cursor else it, name, value)

    bad(ffi, put("m", -1, cursor=True), word=b"m -1")
    bad(ffi, put("m", 4097, cursor=True), pair=2, word=b"4097")
    bad(ffi, put("n", -5), word=b"n -5")
    bad(ffi, put("n", 1 << 30), word=b"out of range")
    bad(ffi, put("coefficient", 1.0), word=b"coefficient")
    bad(ffi, put("generation_acting", 1 << 56, cursor=True), pair=0, word=b"2^56")
    bad(ffi, put("generation_adaptive", 1 << 56, cursor=True), word=b"2^56")
    bad(ffi, put("skip0_end", 1 << 20), word=b"skip ranges")
    bad(ffi, put("d_obs", None), word=b"NULL obs")
    bad(ffi, put("d_dst", None), word=b"NULL obs")
    bad(ffi, put("d_stddev", None), word=b"stddev")
    bad(ffi, put("d_distance", None), pair=2, word=b"distance")
    bad(ffi, lambda it, cu: setattr(it, "d_dst", it.d_src), word=b"d_dst == d_src")
    bad(ffi, lambda it, cu: setattr(it.actor, "obs_dim", 9), word=b"obs_dim")
    bad(ffi, lambda it, cu: setattr(it.actor, "h2", 0), word=b"hidden sizes")
    bad(ffi, lambda it, cu: setattr(it.actor, "ln1_g", it.d_src), word=b"LayerNorm")
    # actor pointers outside d_src[0 .. n): below it, beyond it, and a segment that starts inside and ends outside
    bad(ffi, lambda it, cu: setattr(it.actor, "W2", it.d_src - 4), word=b"inside d_src")
    bad(ffi, lambda it, cu: setattr(it.actor, "b3", it.d_src + 4 * it.n), word=b"inside d_src")
    bad(ffi, lambda it, cu: setattr(it.actor, "W2", it.d_src + 4 * (it.n - 10)), pair=0, word=b"inside d_src")
    bad(ffi, lambda it, cu: setattr(it.actor, "W1", None), word=b"inside d_src")
    bad(ffi, lambda it, cu: setattr(it.actor, "ln2_b", it.d_src - 64), word=b"inside d_src", shapes=((8, 8, 8, True),))


def test_perturb_only_pairs_need_neither_batch_nor_indices(ffi):
    """m == 0 with NULL d_obs / d_idx passes validation: reached through a later pair that fails it"""
    items, cursors = population(ffi, 3)
    cursors[0].m, items[0].d_obs, items[0].d_idx = 0, None, None
    items[1].d_idx = None                                        # m > 0: d_obs holds the batch itself
    items[2].coefficient = 0.5
    rc, msg = call(ffi, items, cursors)
    assert rc == ffi.SSC_EINVAL and b"pair 2" in msg and b"coefficient" in msg


def test_an_actor_beyond_lds_is_refused_with_the_byte_count(ffi):
    for m in (64, 0):                                            # ... whatever the interval: the pair will adapt later
        items, cursors = population(ffi, 3, m=m, shapes=((2, 64, 32, False), (3, 400, 300, False), (3, 200, 100, False)))
        rc, msg = call(ffi, items, cursors)
        assert rc == ffi.SSC_EUNSUPPORTED and b"pair 1" in msg and b"400-300" in msg, msg
        nbytes = int(re.search(rb"need (\d+) bytes of LDS", msg).group(1))
        n = items[1].n
        # the adaptive copy, a 4-row tile of obs, both networks' two activation layers, the LayerNorm statistics, the reduction
        assert nbytes == 4 * ((n + 3) // 4 * 4 + 4 * 3 + 2 * 4 * 401 + 2 * 4 * 301 + 16 + 36) > 160 * 1024


@pytest.mark.parametrize("shift", [0, 4, 4 * 100, -4 * 100])
def test_overlapping_destinations_are_refused(ffi, shift):
    items, cursors = population(ffi, 5)
    items[3].d_dst = items[1].d_dst + shift                      # equal, one float apart, partly over each other
    rc, msg = call(ffi, items, cursors)
    assert rc == ffi.SSC_EINVAL and b"pairs 1 and 3" in msg and b"d_dst" in msg, msg
    items[3].d_dst = items[1].d_dst + 4 * items[1].n             # back to back is legal: reached through pair 4's fault
    items[4].coefficient = 1.0
    rc, msg = call(ffi, items, cursors)
    assert rc == ffi.SSC_EINVAL and b"pair 4" in msg


@pytest.mark.parametrize("where", ["start", "inside", "last float", "own"])
def test_a_destination_inside_a_source_is_refused(ffi, where):
    items, cursors = population(ffi, 3)
    if where == "own":                                           # partly over its own source (d_dst == d_src is the single check)
        items[1].d_dst = items[1].d_src + 4 * 7
        pairs = b"pairs 1 and 1"
    else:
        items[1].d_dst = items[0].d_src + {"start": -4 * (items[1].n - 1), "inside": 4 * 50, "last float": 4 * (items[0].n - 1)}[where]
        pairs = b"pairs 0 and 1"
    rc, msg = call(ffi, items, cursors)
    assert rc == ffi.SSC_EINVAL and pairs in msg and b"d_src" in msg, msg


@pytest.mark.parametrize("mine,theirs", [("d_stddev", "d_stddev"), ("d_distance", "d_distance"), ("d_distance", "d_stddev")])
def test_shared_scalars_are_refused(ffi, mine, theirs):
    items, cursors = population(ffi, 4)
    setattr(items[2], mine, getattr(items[0], theirs))
    rc, msg = call(ffi, items, cursors)
    assert rc == ffi.SSC_EINVAL and b"pairs 0 and 2" in msg and b"share" in msg, msg


def test_what_is_only_read_may_be_shared(ffi):
    """one actor perturbed into two destinations, one ring, one index batch, one statistics block: legal.  A call that
    passes would launch, so the case is reached through a cross-pair fault of two OTHER pairs, which the sorted checks find
    only after the shared arrays of pairs 0 and 1 went through them."""
    items, cursors = population(ffi, 4)
    for name in ("d_src", "d_obs", "d_idx", "n"):
        setattr(items[1], name, getattr(items[0], name))
    for k in NET_KEYS:
        setattr(items[1].actor, k, getattr(items[0].actor, k))
    items[0].d_rms = items[1].d_rms = 0x5000
    items[3].d_stddev = items[2].d_stddev
    rc, msg = call(ffi, items, cursors)
    assert rc == ffi.SSC_EINVAL and b"pairs 2 and 3" in msg and b"share" in msg, msg


# ---- layouts ---------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"ssc_param_noise_many_item": "ParamNoiseManyItem", "ssc_param_noise_cursor": "ParamNoiseCursor"}


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
    assert ctypes.sizeof(ffi.ParamNoiseCursor) == 24
    expect = [getattr(getattr(ffi, NEW_STRUCTS[n]), f).offset for n, f in fields]
    assert offsets == expect, [(n, f, o, e) for (n, f), o, e in zip(fields, offsets, expect) if o != e]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssc.h")).read(), flags=re.S)
    for n, m in NEW_STRUCTS.items():
        body = re.search(r"struct\s+%s\s*\{(.*?)\}\s*;" % n, text, flags=re.S).group(1)
        members = [x for decl in body.split(";") if decl.strip() for x in decl.split(",")]
        assert len(members) == len(getattr(ffi, m)._fields_), (n, members)


# ---- the wrapper's bookkeeping ---------------------------------------------------------------------------------------
class Ring:
    """what the bookkeeping reads of a DeviceReplayBuffer"""

    def __init__(self, records, seed):
        self.records, self.seed, self._batches_drawn = records, seed, 3

    def __len__(self):
        return self.records


def test_wrapper_bookkeeping_on_stub_agents(ffi):
    """``DDPGPopulation.param_noise_plan`` -- the host half of ``param_noise_cycle``: per noisy agent the interval (m), the two
    generations and the ring's sampling key, and what ``param_noise_commit`` then advances: generations + 2 / + 1,
    ``_batches_drawn`` only for rings at or above ``batch_size``; an agent without parameter noise is not in the launch."""
    from smartstartcontinuous_amd.agents import DDPGPopulation

    def agent(noisy, generation):
        return types.SimpleNamespace(param_noise=object() if noisy else None, batch_size=64, param_noise_generation=generation,
                                     perturbed_generation=None, device="cpu")

    agents = [agent(True, 5), agent(False, 0), agent(True, 9), agent(True, 0)]
    rings = [Ring(64, 100), Ring(1000, 101), Ring(63, 102), Ring(5000, 103)]
    pop = DDPGPopulation.__new__(DDPGPopulation)
    pop.agents = agents
    plan = pop.param_noise_plan(rings)
    assert [e["p"] for e in plan] == [0, 2, 3]
    assert [e["m"] for e in plan] == [64, 0, 64]
    assert [(e["generation_adaptive"], e["generation_acting"]) for e in plan] == [(5, 6), (9, 9), (0, 1)]
    assert [e["key"] for e in plan] == [(100, 3, 64), None, (103, 3, 5000)]
    # planning moves nothing
    assert [a.param_noise_generation for a in agents] == [5, 0, 9, 0] and all(r._batches_drawn == 3 for r in rings)
    pop.param_noise_commit(plan, rings)
    assert [a.param_noise_generation for a in agents] == [7, 0, 10, 2]
    assert [a.perturbed_generation for a in agents] == [6, None, 9, 1]
    assert [r._batches_drawn for r in rings] == [4, 3, 3, 4]
    plan = pop.param_noise_plan(rings)                           # the next interval goes on from there
    assert [(e["generation_adaptive"], e["generation_acting"]) for e in plan] == [(7, 8), (10, 10), (2, 3)]
    assert [e["key"] for e in plan] == [(100, 4, 64), None, (103, 4, 5000)]
