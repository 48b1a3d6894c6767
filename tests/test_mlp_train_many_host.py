"""ssc_mlp_train_steps_many and navigator.DynamicsModelPopulation: everything they decide on the host, before any HIP call
-- so none of this needs a GPU.  The pointers are made-up addresses: a call that passed validation with work to do would
launch, so every library call here either fails validation or has nothing to launch (every n_steps == 0)."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ITEMS = 0x7000_0000                                  # the "device copy": never read on the host
ARRAYS = ("W", "b", "mW", "vW", "mb", "vb")


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def population(ffi, P, n_steps=2, shapes=((3, 32, 2),), batch=33):
    """P valid models, every array at an address of its own; model p has the layer widths shapes[p % len(shapes)]"""
    items = (ffi.MlpTrainManyItem * P)()
    for p, it in enumerate(items):
        base = 0x1000_0000 * (p + 1)
        dims = shapes[p % len(shapes)]
        it.net.n_layers = len(dims) - 1
        for l, d in enumerate(dims):
            it.net.dims[l] = d
        for l in range(len(dims) - 1):
            for k, name in enumerate(ARRAYS):
                getattr(it.net, name)[l] = base + 0x10_0000 * (l * len(ARRAYS) + k + 1)
        it.net.adam_t = base + 0x300_0000
        it.net.lr, it.net.beta1, it.net.beta2, it.net.epsilon = 1e-3, 0.9, 0.999, 1e-8
        it.d_X, it.d_Z, it.d_idx = base + 0x400_0000, base + 0x500_0000, base + 0x600_0000
        it.batch, it.n_steps = batch + p, n_steps
        it.d_loss = base + 0x700_0000
        it.d_workspace = base + 0x800_0000
        it.workspace_bytes = ffi.lib().ssc_mlp_train_workspace_bytes(ctypes.byref(it.net), it.batch)
    return items


def call(ffi, items, n=None, d_items=D_ITEMS):
    rc = ffi.lib().ssc_mlp_train_steps_many(None if items is None else ctypes.addressof(items), d_items,
                                            len(items) if n is None else n, None)
    return rc, ffi.lib().ssc_last_error()


def refused(ffi, change, code=None, model=1, word=b"", **kw):
    """the call with one item changed fails with `code`, naming the model -- before any launch"""
    items = population(ffi, 3, **kw)
    change(items[model])
    rc, msg = call(ffi, items)
    assert rc == (ffi.SSC_EINVAL if code is None else code), msg
    assert b"model %d" % model in msg and word in msg, msg


def test_null_arrays_and_population_size(ffi):
    items = population(ffi, 2, n_steps=0)
    assert call(ffi, None, n=2)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, d_items=None)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_models" in msg
    assert call(ffi, items, n=-4)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, n=65536)                  # refused on the count alone: item 2 .. 65535 do not exist
    assert rc == ffi.SSC_EUNSUPPORTED and b"65536" in msg
    assert ffi.lib().ssc_version() == 108                # additive: the ABI version does not move


def test_no_steps_anywhere_is_ok_without_a_launch(ffi):
    assert call(ffi, population(ffi, 4, n_steps=0))[0] == ffi.SSC_OK
    assert call(ffi, population(ffi, 1, n_steps=0))[0] == ffi.SSC_OK
    # a skipped model's item is not read at all: garbage, another class, arrays of its neighbour
    items = population(ffi, 3, n_steps=0)
    ctypes.memset(ctypes.addressof(items[1]), 0xFF, ctypes.sizeof(ffi.MlpTrainManyItem))
    items[1].n_steps = 0
    items[2].net.W[0] = items[0].net.W[0]
    assert call(ffi, items)[0] == ffi.SSC_OK
    rc, msg = call(ffi, population(ffi, 3, n_steps=-1))
    assert rc == ffi.SSC_EINVAL and b"model 0" in msg and b"n_steps" in msg


def test_a_skipped_model_beside_a_refused_one(ffi):
    """garbage in a skipped item changes nothing about what the others are told"""
    items = population(ffi, 3)
    ctypes.memset(ctypes.addressof(items[0]), 0xFF, ctypes.sizeof(ffi.MlpTrainManyItem))
    items[0].n_steps = 0
    items[2].workspace_bytes -= 1
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"model 2" in msg and b"workspace" in msg


def test_every_item_passes_the_single_calls_checks(ffi):
    refused(ffi, lambda it: setattr(it, "batch", 0), word=b"batch")
    refused(ffi, lambda it: setattr(it, "batch", 65537), model=2, word=b"batch")
    refused(ffi, lambda it: setattr(it.net, "n_layers", 9), word=b"n_layers")
    refused(ffi, lambda it: setattr(it.net, "n_layers", 0), model=0, word=b"n_layers")
    refused(ffi, lambda it: it.net.dims.__setitem__(1, 0), word=b"dims[1]")
    refused(ffi, lambda it: it.net.dims.__setitem__(2, 9000), word=b"dims[2]")
    for name in ARRAYS:
        refused(ffi, lambda it: getattr(it.net, name).__setitem__(1, None), word=b"layer 1")
    refused(ffi, lambda it: setattr(it.net, "adam_t", None), word=b"NULL pointer")
    refused(ffi, lambda it: setattr(it, "d_X", None), model=2, word=b"NULL pointer")
    refused(ffi, lambda it: setattr(it, "d_Z", None), word=b"NULL pointer")
    refused(ffi, lambda it: setattr(it, "d_idx", None), model=0, word=b"NULL pointer")
    refused(ffi, lambda it: setattr(it, "n_steps", -3), word=b"n_steps")


def test_undersized_workspace_is_refused(ffi):
    refused(ffi, lambda it: setattr(it, "workspace_bytes", it.workspace_bytes - 1), model=2, word=b"workspace")
    refused(ffi, lambda it: setattr(it, "d_workspace", None), model=0, word=b"workspace")
    refused(ffi, lambda it: setattr(it, "batch", 513), word=b"workspace")          # more workgroups: more partials
    refused(ffi, lambda it: setattr(it, "workspace_bytes", 0), word=b"workspace")


def test_one_instantiation_per_call(ffi):
    for shapes, first, other in ((((3, 32, 2), (3, 32, 2), (4, 32, 3)), b"<3,2>", b"<4,3>"),
                                 (((4, 100, 3), (3, 16, 3), (12, 64, 8)), b"<4,3>", b"<12,8>"),
                                 (((5, 16, 1), (12, 512, 8), (3, 500, 2)), b"<12,8>", b"<3,2>")):
        rc, msg = call(ffi, population(ffi, 3, shapes=shapes))
        assert rc == ffi.SSC_EINVAL and b"model 2" in msg and b"model 0" in msg and first in msg and other in msg, msg
    # the first TRAINED model sets the class: a skipped model of another class does not
    items = population(ffi, 3, shapes=((4, 32, 3), (3, 32, 2), (3, 32, 1)), n_steps=0)
    assert call(ffi, items)[0] == ffi.SSC_OK
    items = population(ffi, 4, shapes=((4, 32, 3), (3, 32, 2), (3, 17, 1), (12, 16, 8)))
    items[0].n_steps = 0
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"model 3" in msg and b"model 1" in msg and b"<12,8>" in msg and b"<3,2>" in msg, msg
    # widths, batch sizes and step counts inside a class are the models' own: nothing to refuse but the launch itself,
    # so the same population with nothing to do is accepted
    assert call(ffi, population(ffi, 4, shapes=((3, 32, 2), (1, 500, 1), (2, 1, 2), (3, 17, 1)), n_steps=0))[0] == ffi.SSC_OK


def test_models_outside_the_fused_kernel_are_unsupported(ffi):
    U = ffi.SSC_EUNSUPPORTED
    assert "SSC_DYN_TRAIN_GENERIC" not in os.environ
    for dims in ((3, 32, 32, 2), (3, 2), (3, 513, 2), (13, 32, 2), (3, 32, 9), (3, 40, 24, 16, 2)):
        def reshape(it, dims=dims):
            fresh = population(ffi, 3, shapes=(dims,))
            ctypes.memmove(ctypes.addressof(it), ctypes.addressof(fresh[1]), ctypes.sizeof(ffi.MlpTrainManyItem))
        refused(ffi, reshape, code=U, word=b"fused")
    # ... and so is everything once the A/B switch of the single call is set (read once per process: a child)
    prog = ("import ctypes, sys; sys.path.insert(0, %r)\n"
            "from tests.test_mlp_train_many_host import population, call\n"
            "from smartstartcontinuous_amd import _ffi\n"
            "rc, msg = call(_ffi, population(_ffi, 2))\n"
            "print(rc, msg.decode())\n" % ROOT)
    out = subprocess.check_output([sys.executable, "-c", prog], env=dict(os.environ, SSC_DYN_TRAIN_GENERIC="1"), text=True)
    assert out.startswith("%d " % U) and "model 0" in out, out


def _both(ffi, P=5):
    return population(ffi, P, n_steps=3)


@pytest.mark.parametrize("mine,theirs", [("W0", "W0"), ("b1", "b1"), ("mW0", "vW0"), ("mb1", "vb1"), ("vW1", "W1"), ("adam_t", "adam_t"),
                                         ("d_loss", "d_loss"), ("d_workspace", "d_workspace"), ("d_loss", "d_workspace"),
                                         ("W1", "d_workspace"), ("adam_t", "d_loss"),
                                         ("W0", "d_X"), ("d_workspace", "d_Z"), ("d_loss", "d_idx"), ("d_X", "W1"), ("d_idx", "b0")])
def test_what_one_model_writes_no_other_model_touches(ffi, mine, theirs):
    def ref(item, name):
        if name.startswith("d_"):
            return item, name, None
        if name == "adam_t":
            return item.net, name, None
        return getattr(item.net, name[:-1]), None, int(name[-1])

    def get(item, name):
        obj, attr, k = ref(item, name)
        return getattr(obj, attr) if k is None else obj[k]

    def put(item, name, value):
        obj, attr, k = ref(item, name)
        if k is None:
            setattr(obj, attr, value)
        else:
            obj[k] = value

    items = _both(ffi)
    put(items[3], mine, get(items[1], theirs))
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"overlap" in msg and b"models 1 and 3" in msg, msg
    if theirs != "adam_t":           # a partial overlap is one too: the range begins inside the other model's
        items = _both(ffi)
        put(items[3], mine, get(items[1], theirs) + 4)
        rc, msg = call(ffi, items)
        assert rc == ffi.SSC_EINVAL and b"overlap" in msg and b"models 1 and 3" in msg, msg
    # a skipped model takes no part: the table is walked in address order, and the pair behind it is the one reported
    items = _both(ffi)
    put(items[3], mine, get(items[1], theirs))
    items[3].n_steps = 0
    items[4].d_workspace = items[2].d_workspace
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"overlap" in msg and b"models 2 and 4" in msg, msg


def test_what_is_only_read_may_be_shared(ffi):
    """X, Z and the index stream of one model given to all: legal, and with nothing to launch the call says so"""
    items = population(ffi, 4, n_steps=0)
    for it in items:
        it.d_X, it.d_Z, it.d_idx, it.batch = items[0].d_X, items[0].d_Z, items[0].d_idx, items[0].batch
    assert call(ffi, items)[0] == ffi.SSC_OK
    # with steps everywhere the shared reads pass the overlap check as well: the one thing wrong is reported instead
    items = population(ffi, 4, n_steps=3)
    for it in items:
        it.d_X, it.d_Z, it.d_idx, it.batch = items[0].d_X, items[0].d_Z, items[0].d_idx, items[0].batch
        it.workspace_bytes = ffi.lib().ssc_mlp_train_workspace_bytes(ctypes.byref(it.net), it.batch)
    items[3].d_loss = items[2].d_loss
    rc, msg = call(ffi, items)
    assert rc == ffi.SSC_EINVAL and b"models 2 and 3" in msg and b"written" in msg and b"read range" not in msg, msg


# ---- layout ----------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header(ffi, tmp_path):
    """sizeof() and offsetof() of every field as the C compiler sees them == the ctypes mirror, which sits in the
    struct-layout table of _ffi.py; the header's field list holds nothing the mirror lacks."""
    n, M = "ssc_mlp_train_many_item", ffi.MlpTrainManyItem
    assert ffi.STRUCTS[n] is M and "ssc_mlp_train_steps_many" in ffi._SIGNATURES
    fields = [f for f, _ in M._fields_]
    lines = [f'printf("%zu\\n", sizeof({n}));'] + [f'printf("%zu\\n", offsetof({n}, {f}));' for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssc.h"\nint main(){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(M) and got[1:] == [getattr(M, f).offset for f in fields], got
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssc.h")).read(), flags=re.S)
    body = re.search(r"struct\s+%s\s*\{(.*?)\}\s*;" % n, text, flags=re.S).group(1)
    members = [x for decl in body.split(";") if decl.strip() for x in decl.split(",")]
    assert len(members) == len(fields), members


# ---- the population's grouping (stub models: no GPU) -------------------------------------------------------------------
def stub(*dims, device="cuda:0"):
    return types.SimpleNamespace(W=[np.zeros((dims[l], dims[l + 1]), np.float32) for l in range(len(dims) - 1)], device=device)


def test_population_groups_models_by_instantiation(monkeypatch):
    from smartstartcontinuous_amd import navigator as nav
    monkeypatch.delenv("SSC_DYN_TRAIN_GENERIC", raising=False)
    monkeypatch.setattr(nav, "DYN_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "DYN_POPULATION_MIN_GROUP", 2)
    models = [stub(3, 32, 2), stub(4, 500, 3), stub(3, 500, 500, 2), stub(1, 16, 1), stub(12, 256, 8), stub(4, 17, 2),
              stub(3, 513, 2), stub(3, 100, 3), stub(5, 3)]
    pop = nav.DynamicsModelPopulation(models)
    assert pop.ways == ["fused<3,2>", "fused<4,3>", "alone", "fused<3,2>", "alone", "fused<4,3>", "alone", "fused<4,3>", "alone"]
    assert not pop.fused                                                    # <12,8> has one member, three are ineligible
    assert nav.DynamicsModelPopulation([stub(3, 32, 2)] * 3).fused
    monkeypatch.setattr(nav, "DYN_POPULATION_MIN_GROUP", 3)
    assert pop.ways == ["alone", "fused<4,3>", "alone", "alone", "alone", "fused<4,3>", "alone", "fused<4,3>", "alone"]
    monkeypatch.setattr(nav, "DYN_POPULATION_MIN_GROUP", 1)
    assert pop.ways[4] == "fused<12,8>" and pop.ways[2] == "alone" and pop.ways[8] == "alone"
    monkeypatch.setattr(nav, "DYN_POPULATION_GROUPED", False)
    assert pop.ways == ["alone"] * 9 and not pop.fused
    monkeypatch.setattr(nav, "DYN_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "DYN_POPULATION_MIN_GROUP", 2)
    monkeypatch.setenv("SSC_DYN_TRAIN_GENERIC", "1")                         # the library would refuse every model
    assert pop.ways == ["alone"] * 9
    monkeypatch.delenv("SSC_DYN_TRAIN_GENERIC")
    # a model on another device than the first trains alone, and may take its group below the minimum
    two = nav.DynamicsModelPopulation([stub(3, 32, 2), stub(3, 32, 2, device="cuda:1"), stub(3, 16, 2)])
    assert two.ways == ["fused<3,2>", "alone", "fused<3,2>"]
    assert nav.DynamicsModelPopulation([stub(3, 32, 2), stub(3, 32, 2, device="cuda:1")]).ways == ["alone", "alone"]
    with pytest.raises(ValueError):
        nav.DynamicsModelPopulation([])
    assert isinstance(nav.DYN_POPULATION_MIN_GROUP, int) and nav.DYN_POPULATION_MIN_GROUP >= 1


def test_population_train_needs_one_generator_per_model():
    from smartstartcontinuous_amd import navigator as nav
    pop = nav.DynamicsModelPopulation([stub(3, 32, 2), stub(3, 32, 2)])
    data = [(np.zeros((8, 3)), np.zeros((8, 2)), np.zeros((0, 3)), np.zeros((0, 2)))] * 2
    shared = np.random.RandomState(0)
    for rngs in (None, shared, [shared, shared], [np.random.RandomState(0)], [np.random.RandomState(0), None],
                 [np.random, np.random.RandomState(1)]):
        with pytest.raises(ValueError, match="rngs"):
            pop.train(data, 1, 0.0, rngs=rngs)
    with pytest.raises(ValueError):
        pop.train(data, [1, 2, 3], 0.0, rngs=[np.random.RandomState(0), np.random.RandomState(1)])
    from smartstartcontinuous_amd.agents import train_dynamics_models
    with pytest.raises(ValueError):
        train_dynamics_models([object(), object()], shared)


# ---- the index helper against the loop DynamicsModel.train ran before it was moved out ---------------------------------
def epochs_before(n_old, n_new, nEpoch, fraction_use_new, batchsize, rng):
    """the batching of ``DynamicsModel.train`` as it stood (dynamics_model.py:60-122), index matrices collected per epoch"""
    b_new = n_new if n_new < batchsize * fraction_use_new else int(batchsize * fraction_use_new)
    b_old = int(batchsize - b_new)
    perm_new = np.arange(n_new)
    out = []
    for _ in range(nEpoch):
        old = rng.choice(np.arange(n_old), size=(n_old,), replace=False)
        if b_old > 0:
            batches = []
            for batch in range(int(np.floor(n_old / b_old))):
                new_idx = rng.randint(0, n_new, (b_new,)) if n_new > 0 else np.zeros(0, np.int64)
                batches.append(np.concatenate([old[batch * b_old:(batch + 1) * b_old], n_old + perm_new[new_idx]]))
        else:
            batches = [n_old + perm_new[b * b_new:(b + 1) * b_new] for b in range(int(np.floor(n_new / b_new)))]
            perm_new = perm_new[rng.permutation(n_new)]
        out.append(np.stack(batches).astype(np.int32) if batches else None)
    return out


@pytest.mark.parametrize("n_old,n_new,frac,batchsize", [
    (700, 300, 0.25, 64),        # b_old > 0: a walk through the old rows, new rows drawn per batch
    (100, 300, 1.0, 64),         # b_old == 0: new rows only, permuted after every epoch
    (700, 0, 0.5, 64),           # n_new == 0: nothing to mix in
    (700, 10, 0.5, 64),          # n_new < batchsize * fraction: every batch takes n_new draws
    (40, 5, 0.25, 64),           # fewer old rows than one batch needs: an epoch without a batch
    (513, 100, 0.1, 512),        # the shipped batch size, one batch per epoch
])
def test_index_helper_reproduces_the_loop_it_was_moved_out_of(n_old, n_new, frac, batchsize):
    from smartstartcontinuous_amd import navigator as nav
    want_rng, got_rng = np.random.RandomState(11), np.random.RandomState(11)
    want = epochs_before(n_old, n_new, 3, frac, batchsize, want_rng)
    got = list(nav.train_index_batches(n_old, n_new, 3, frac, batchsize, got_rng))
    assert len(got) == 3
    for w, g in zip(want, got):
        assert (w is None) == (g is None)
        if w is not None:
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w)
            assert g.shape[1] == batchsize and g.min() >= 0 and g.max() < n_old + n_new
    assert want_rng.randint(1 << 30) == got_rng.randint(1 << 30)             # the same calls in the same order: same state after
    assert any(g is not None for g in got) == (n_old >= 64 or frac == 1.0)
