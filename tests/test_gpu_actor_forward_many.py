"""ssc_actor_forward_many: every actor class (the five device bodies ssc_actor_forward dispatches at m > 32, obs_dim 2 and 3,
with and without the observation statistics block) in one launch for a population of actors, against the actors' own calls.

The contract is bit equality, so there is no tolerance: items of 1, 20, 63, 64, 65, 255 and 257 rows (below / at / above a
wave and a 256-row block; the 1- and 20-row items go through actor_row_kernel in the single call, whose bits are the generic
kernel's), listed out of row order with an empty item between them, a gap of unowned rows inside and guard rows at both ends.
Both buffers start from the same sentinel; after the many-call the WHOLE buffer equals the one the per-item
ssc_actor_forward[_rms] calls on the slices left -- so owned rows are the single call's bits and every other row is untouched.
Every item has weights, flags (last_layer_tanh, obs_clip) and statistics of its own."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROWS = (64, 1, 257, 0, 20, 255, 63, 65)          # table order; 0: the empty item
FRONT, GAP_AFTER, GAP, BACK = 3, 2, 5, 4          # guard rows, and a gap of unowned rows behind the third item
SENTINEL = 12345.0

# (name, precision, h1, h2, layer_norm)
CLASSES = [("f32_64-32", "f32", 64, 32, False), ("bf16_64-32", "bf16", 64, 32, False), ("bf16_128-64", "bf16", 128, 64, False),
           ("bf16_200-100", "bf16", 200, 100, False), ("generic_48-24", "f32", 48, 24, False),
           ("generic_48-24_ln", "f32", 48, 24, True)]


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def make_actor(ffi, rng, obs_dim, h1, h2, prec, ln, j):
    """descriptor + the tensors it points at; every item differs in weights, last_layer_tanh and obs_clip"""
    shapes = dict(W1=(obs_dim, h1), b1=(h1,), W2=(h1, h2), b2=(h2,), W3=(h2, 1), b3=(1,))
    w = {k: torch.as_tensor(rng.normal(0, 0.5 / np.sqrt(s[0]) if len(s) == 2 else 0.1, s).astype(np.float32), device="cuda")
         for k, s in shapes.items()}
    if ln:
        for k, n in (("ln1_g", h1), ("ln1_b", h1), ("ln2_g", h2), ("ln2_b", h2)):
            w[k] = torch.as_tensor((rng.normal(0, 0.2, n) + (1.0 if k.endswith("g") else 0.0)).astype(np.float32), device="cuda")
    a = ffi.ActorDesc()
    a.obs_dim, a.h1, a.h2, a.act_dim = obs_dim, h1, h2, 1
    ffi.set_net_ptrs(a, w)
    a.last_layer_tanh, a.obs_clip = j % 2, (5.0, 0.0, 1.5)[j % 3]
    a.precision = ffi.SSC_PREC_F32 if prec == "f32" else ffi.SSC_PREC_BF16_MFMA
    return a, w


def layout():
    """row0 per item of ROWS: in ascending row order items 1, 4, 6, (gap) 0, 7, 5, 2 -- not the table's order"""
    order, row0, at = [1, 4, 6, 0, 7, 5, 2], {}, FRONT
    for n, j in enumerate(order):
        row0[j] = at
        at += ROWS[j] + (GAP if n == GAP_AFTER else 0)
    row0[3] = 10 ** 12                          # the empty item: nothing of it is read
    return row0, at + BACK


@pytest.mark.parametrize("has_rms", [False, True], ids=["plain", "rms"])
@pytest.mark.parametrize("obs_dim", [2, 3])
@pytest.mark.parametrize("cls", CLASSES, ids=[c[0] for c in CLASSES])
def test_many_call_is_the_single_calls_bits(ssc, cls, obs_dim, has_rms):
    from smartstartcontinuous_amd.population import DeviceItems
    ffi, lib = ssc._ffi, ssc._ffi.lib()
    _, prec, h1, h2, ln = cls
    rng = np.random.default_rng(hash((h1, h2, obs_dim, has_rms, ln)) % 2 ** 31)
    row0, m = layout()
    obs = torch.as_tensor(rng.normal(0, 2.0, (m, obs_dim)).astype(np.float32), device="cuda")
    got = torch.full((m, 1), SENTINEL, dtype=torch.float32, device="cuda")
    want = got.clone()
    items = DeviceItems(ffi.ActorManyItem, len(ROWS), "cuda")
    keep, classes = [], set()
    for j, rows in enumerate(ROWS):
        a, w = make_actor(ffi, rng, obs_dim, h1, h2, prec, ln, j)
        blk = None
        if has_rms:                              # RunningMeanStd block: sum | sumsq | count, a different one per item
            cnt, mean, var = 100.0 + j, rng.normal(0, 0.5, obs_dim), rng.uniform(0.5, 3.0, obs_dim)
            blk = torch.as_tensor(np.concatenate([mean * cnt, (var + mean ** 2) * cnt, [cnt]]), dtype=torch.float64, device="cuda")
        keep.append((w, blk))
        it = items.items[j]
        it.actor, it.d_rms, it.row0, it.rows = a, (blk.data_ptr() if has_rms else None), row0[j], rows
        if rows == 0:
            continue
        classes.add(lib.ssc_actor_many_class(ctypes.byref(a), int(has_rms)))
        o, dst = obs[row0[j]:row0[j] + rows], want[row0[j]:row0[j] + rows]
        if has_rms:
            ffi.check(lib.ssc_actor_forward_rms(ctypes.byref(a), rows, ffi.ptr(o), ffi.ptr(dst), None, ffi.ptr(blk)))
        else:
            ffi.check(lib.ssc_actor_forward(ctypes.byref(a), rows, ffi.ptr(o), ffi.ptr(dst), None))
    assert len(classes) == 1 and min(classes) >= 0 and min(classes) % 2 == int(has_rms), classes
    items.upload()
    ffi.check(lib.ssc_actor_forward_many(items.h_ptr, items.d_ptr, len(ROWS), m, ffi.ptr(obs), ffi.ptr(got), None))
    torch.cuda.synchronize()
    g, w_ = got.cpu().numpy().view(np.int32).ravel(), want.cpu().numpy().view(np.int32).ravel()
    owned = np.zeros(m, bool)
    for j, rows in enumerate(ROWS):
        if rows:
            owned[row0[j]:row0[j] + rows] = True
    sent = np.float32(SENTINEL).view(np.int32)
    assert (w_[~owned] == sent).all() and (w_[owned] != sent).all()      # the reference itself wrote exactly the owned rows
    bad = np.nonzero(g != w_)[0]
    assert bad.size == 0, (cls[0], obs_dim, has_rms, bad[:8], got.cpu().numpy().ravel()[bad[:8]], want.cpu().numpy().ravel()[bad[:8]])


def test_a_mixed_class_call_is_refused_naming_both_items(ssc):
    from smartstartcontinuous_amd.population import DeviceItems
    ffi, lib = ssc._ffi, ssc._ffi.lib()
    rng = np.random.default_rng(5)
    items = DeviceItems(ffi.ActorManyItem, 3, "cuda")
    keep = []
    for j, (prec, h1, h2, rows) in enumerate((("f32", 64, 32, 40), ("f32", 64, 32, 0), ("bf16", 64, 32, 40))):
        a, w = make_actor(ffi, rng, 2, h1, h2, prec, False, j)
        keep.append(w)
        items.items[j].actor, items.items[j].row0, items.items[j].rows = a, 40 * j, rows
    items.upload()
    obs = torch.zeros((120, 2), dtype=torch.float32, device="cuda")
    act = torch.full((120, 1), SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib.ssc_actor_forward_many(items.h_ptr, items.d_ptr, 3, 120, ffi.ptr(obs), ffi.ptr(act), None)
    msg = lib.ssc_last_error()
    assert rc == ffi.SSC_EUNSUPPORTED and b"items 0 and 2" in msg and b"classes 0 and 4" in msg, msg
    torch.cuda.synchronize()
    assert (act == SENTINEL).all()               # refused before any launch
