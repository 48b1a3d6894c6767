"""ssc_mpc_forward_sim_many_mfma (csrc/dyn_mfma_many.hip: dyn_mfma_sim_many_kernel<UT, NFC, BIASK>, the seven classes):
contiguous problem ranges of one call simulated with different bf16-MFMA models in ONE launch.  The definition is the
population's yardstick: per working item the model's own ssc_mpc_forward_sim(.., SSC_PREC_BF16_MFMA_PREPARED) into a scratch
pre-filled from the item's rows of S, with problem_id0 + problem0 and the mask from byte problem0 on, then a strided copy
back.  The many-call must leave the same bits (torch.equal on whole sentinel-filled S and A_out), and the sentinels must
survive exactly where no wave works.  Two items are also held to the fp64 oracle under the bf16 bound of tests/sim_cases.py
and their actions to the oracle's Philox stream.  The models come from the generators of tests/sim_cases.py."""
import ctypes
import functools
import zlib

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import sim_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENT_S, SENT_A = 123.0, -7.0
N, H4 = 19, 4
COUNTS = (1, 13, 14, 27, 0, 2)          # 19, 247, 266 (a second tile of 10 rows), 513 (a third tile of one row), 0, 38 rows
GAP = 1                                  # problem 1 has no owner: item 1 starts at row 38, no multiple of 16
P = sum(COUNTS) + 1

# class -> (hidden layers, the depth of each item's model): every depth inside the class, its edges included
CLASSES = {
    "<1,1>": (1, (32, 1, 20, 31, 7, 32)),
    "<4,1>": (1, (128, 33, 100, 64, 127, 128)),
    "<16,1>": (1, (500, 129, 512, 300, 257, 500)),
    "<1,2>": (2, (31, 32, 31, 32, 31, 32)),
    "<1,2,biask>": (2, (30, 1, 24, 16, 29, 30)),
    "<4,2>": (2, (127, 128, 127, 128, 127, 128)),
    "<4,2,biask>": (2, (100, 33, 126, 64, 96, 100)),
}
CLASS_ID = {"<1,1>": 0, "<4,1>": 1, "<16,1>": 2, "<1,2>": 3, "<1,2,biask>": 4, "<4,2>": 5, "<4,2,biask>": 6}
IO = [(3, 2), (4, 3)]


@pytest.fixture(scope="module")
def nav():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import navigator
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return navigator


@functools.lru_cache(maxsize=None)
def fresh_model(nav, dims, tag):
    rng = np.random.default_rng(zlib.crc32(("many_mfma_%s_%s" % (dims, tag)).encode()))
    d, a = dims[-1], dims[0] - dims[-1]
    Ws, bs = SC.make_mlp(rng, dims)
    return nav.DynamicsModel(Ws, bs, SC.make_norm(rng, d, a), state_dim=d, act_dim=a, precision="bf16_mfma")


def class_layout(nav, cls, io):
    """(model, problem0, n_problems) per item: COUNTS back to back behind the gap problem"""
    from smartstartcontinuous_amd import _ffi as ffi
    nfc, depths = CLASSES[cls]
    layout, at = [], 0
    for k, (n, depth) in enumerate(zip(COUNTS, depths)):
        if k == 1:
            at += 1                                           # the gap
        mo = fresh_model(nav, (io[0],) + (depth,) * nfc + (io[1],), "item%d" % k)
        assert ffi.lib().ssc_dyn_mfma_many_class(ctypes.byref(mo.desc), mo.state_dim, mo.act_dim) == CLASS_ID[cls]
        layout.append((mo, at, n))
        at += n
    assert at == P
    return layout


def item_table(ffi, layout):
    items = (ffi.MpcSimManyMfmaItem * len(layout))()
    for it, (model, p0, n) in zip(items, layout):
        img = model._mfma_image()
        it.mlp, it.d_image, it.image_bytes, it.problem0, it.n_problems = model.desc, img.data_ptr(), img.numel(), p0, n
    dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    return items, dev


def many(ffi, layout, sp, m, H, d, a, s0, S_out, A_out):
    items, dev = item_table(ffi, layout)
    s0_rows = 1 if s0.dim() == 1 else s0.shape[0]
    rc = ffi.lib().ssc_mpc_forward_sim_many_mfma(ctypes.addressof(items), dev.data_ptr(), len(layout), ctypes.byref(sp), m, H,
                                                 d, a, ffi.ptr(s0), s0_rows, ffi.ptr(A_out), ffi.ptr(S_out), ffi.stream())
    torch.cuda.synchronize()
    return rc


def buffers(m, H, d, a):
    return torch.full((H + 1, m, d), SENT_S, device="cuda"), torch.full((m, H, a), SENT_A, device="cuda")


def own_calls(nav, layout, n_samples, low, high, pid0, t, t_base, mask_t, m, H, s0, S_out, A_out):
    """the definition: the model's own prepared MFMA call on the item's rows, scratch in, strided copy back"""
    for model, p0, n in layout:
        if n == 0:
            continue
        rows = slice(p0 * n_samples, (p0 + n) * n_samples)
        s0_p = s0 if s0.dim() == 1 else (s0[p0:p0 + n] if s0.shape[0] * n_samples == m else s0[rows])
        sp = nav.mpc_sampling(n_samples, low, high, SC.SEED, pid0 + p0, t, t_base=t_base,
                              active=None if mask_t is None else mask_t[p0:])
        scratch = S_out[:, rows].contiguous()
        A_p = A_out[rows]
        model.do_forward_sim_sampled(s0_p.contiguous(), sp, n * n_samples, H, precision="bf16_mfma", out=scratch, A_out=A_p)
        S_out[:, rows] = scratch
    torch.cuda.synchronize()


def worked_rows(layout, n_samples, total, mask):
    """rows some wave writes: a wave (32 rows counted from ITS ITEM's first row) works when one of its rows is live"""
    out = np.zeros(total * n_samples, bool)
    for _, p0, n in layout:
        live = np.repeat(np.ones(n, bool) if mask is None else mask[p0:p0 + n].astype(bool), n_samples)
        for w in range(0, live.size, 32):
            out[p0 * n_samples + w:p0 * n_samples + min(w + 32, live.size)] = live[w:w + 32].any()
    return out


def check_equal_to_own_calls(nav, layout, total, n_samples, H, d, a, s0, mask=None, pid0=SC.PID0, t=SC.T_STEP, t_base=None):
    from smartstartcontinuous_amd import _ffi as ffi
    low, high = SC.ACT_LOW[:a], SC.ACT_HIGH[:a]
    m = total * n_samples
    mask_t = None if mask is None else torch.as_tensor(mask, device="cuda")
    want_S, want_A = buffers(m, H, d, a)
    own_calls(nav, layout, n_samples, low, high, pid0, t, t_base, mask_t, m, H, s0, want_S, want_A)
    got_S, got_A = buffers(m, H, d, a)
    sp = nav.mpc_sampling(n_samples, low, high, SC.SEED, pid0, t, t_base=t_base, active=mask_t)
    assert many(ffi, layout, sp, m, H, d, a, s0, got_S, got_A) == ffi.SSC_OK, ffi.lib().ssc_last_error()
    assert torch.equal(got_S, want_S) and torch.equal(got_A, want_A)
    rows = torch.as_tensor(worked_rows(layout, n_samples, total, mask), device="cuda")
    # the sentinel is where no wave works and nowhere else (so the comparison above compared results, not sentinels)
    assert (got_S[:, ~rows] == SENT_S).all() and (got_A[~rows] == SENT_A).all()
    assert not (got_S[:, rows] == SENT_S).any() and not (got_A[rows] == SENT_A).any()
    assert torch.isfinite(got_S).all()
    # d_A_out NULL: the same states
    only_S, _ = buffers(m, H, d, a)
    assert many(ffi, layout, sp, m, H, d, a, s0, only_S, None) == ffi.SSC_OK
    assert torch.equal(only_S, want_S)
    return got_S, got_A, rows


def start_states(kind, total, n_samples, d):
    rng = np.random.default_rng(zlib.crc32(("s0_mfma_%s_%d_%d_%d" % (kind, total, n_samples, d)).encode()))
    shape = (d,) if kind == "call" else (total if kind == "problem" else total * n_samples, d)
    return torch.as_tensor((rng.normal(size=shape) * 0.3).astype(np.float32), device="cuda")


def the_mask(layout):
    """one problem inside a live wave of the 14-problem item off, and the first five problems of the 27-problem item: the run
    starts at a wave boundary of its item (its first row) and covers its waves 0 and 1 (rows 0 .. 63 of 95) entirely"""
    mask = np.ones(P, np.uint8)
    mask[layout[2][1] + 3] = 0
    mask[layout[3][1]:layout[3][1] + 5] = 0
    worked = worked_rows(layout, N, P, mask)
    lo = layout[3][1] * N
    assert not worked[lo:lo + 64].any() and worked[lo + 64:lo + 95].all()        # two whole waves skipped, the third is live
    lo = (layout[2][1] + 3) * N
    assert worked[lo:lo + N].all()                                               # switched off, yet inside live waves
    return mask


@pytest.mark.parametrize("io", IO, ids=["3to2", "4to3"])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_class_equals_the_models_own_calls(nav, cls, io):
    """unmasked (one start state per problem), masked (per row), with d_t_base (per call), d_A_out NULL inside each; H = 1"""
    layout = class_layout(nav, cls, io)
    d, a = io[1], io[0] - io[1]
    check_equal_to_own_calls(nav, layout, P, N, H4, d, a, start_states("problem", P, N, d))
    check_equal_to_own_calls(nav, layout, P, N, H4, d, a, start_states("row", P, N, d), mask=the_mask(layout))
    t_base = torch.tensor([3], dtype=torch.int64, device="cuda")                # t + *d_t_base = T_STEP
    got, _, _ = check_equal_to_own_calls(nav, layout, P, N, H4, d, a, start_states("call", P, N, d), t=SC.T_STEP - 3, t_base=t_base)
    same, _, _ = check_equal_to_own_calls(nav, layout, P, N, H4, d, a, start_states("call", P, N, d))
    assert torch.equal(got, same)
    check_equal_to_own_calls(nav, layout, P, N, 1, d, a, start_states("problem", P, N, d), mask=the_mask(layout))


@pytest.mark.parametrize("name,cls", [("1x500_k4", 2), ("2x100_k4", 6)])
def test_an_item_meets_the_fp64_oracle_and_its_actions(nav, name, cls):
    """the second working item IS the case's network on the case's inputs (rows, start state per row, H = 20) once the call's
    problem_id0 puts its first problem at SC.PID0: its rows meet the oracle under the bf16 bound the own call is held to;
    every owned problem's actions are O.mpc_action_samples of its GLOBAL problem index"""
    from smartstartcontinuous_amd import _ffi as ffi
    case = next(c for c in SC.CASES if c.name == name)
    inp = SC.build_inputs(case)
    ref, emu = SC.references(inp)
    assert case.s0_kind == "row" and not case.walk
    model = nav.DynamicsModel([w.copy() for w in inp.Ws], [b.copy() for b in inp.bs], inp.norm, state_dim=inp.d, act_dim=inp.a,
                              precision="bf16_mfma")
    assert ffi.lib().ssc_dyn_mfma_many_class(ctypes.byref(model.desc), inp.d, inp.a) == cls
    other = fresh_model(nav, case.dims, "oracle_neighbour")
    layout = [(other, 0, 1), (model, 2, case.P)]                                # problem 1 has no owner
    total = 2 + case.P
    s0 = start_states("row", total, case.N, inp.d)
    lo, hi = 2 * case.N, total * case.N
    s0[lo:hi] = torch.as_tensor(inp.s0, device="cuda")
    pid0 = SC.PID0 - 2
    got_S, got_A, _ = check_equal_to_own_calls(nav, layout, total, case.N, case.H, inp.d, inp.a, s0, pid0=pid0)
    X = got_S[:, lo:hi].cpu().numpy()
    assert np.array_equal(X[0], inp.s0_rows)
    r = SC.bound_ratios(X, ref, emu)
    print("SIMRATIO many_mfma", name, " ".join(f"{k}={v:.3f}" for k, v in r.items()), flush=True)
    assert np.isfinite(X).all() and SC.within_bf16_bound(r, SC.C_BF16), r
    A_np = got_A.cpu().numpy()
    assert np.array_equal(A_np[lo:hi], inp.A)
    for _, p0, n in layout:
        for p in range(p0, p0 + n):
            cand = O.mpc_action_samples(SC.SEED, pid0 + p, case.N, case.H, inp.a, SC.T_STEP, SC.ACT_LOW[:inp.a], SC.ACT_HIGH[:inp.a])
            assert np.array_equal(A_np[p * case.N:(p + 1) * case.N], cand), p
    assert (A_np[case.N:2 * case.N] == SENT_A).all()


def test_a_table_of_two_classes_is_refused_and_writes_nothing(nav):
    from smartstartcontinuous_amd import _ffi as ffi
    layout = class_layout(nav, "<16,1>", (3, 2))
    s0 = start_states("problem", P, N, 2)
    sp = nav.mpc_sampling(N, SC.ACT_LOW[:1], SC.ACT_HIGH[:1], SC.SEED, SC.PID0, SC.T_STEP)
    bad = [list(layout), list(layout), list(layout)]
    bad[0][3] = (fresh_model(nav, (3, 128, 2), "other_class"), layout[3][1], layout[3][2])   # <4,1> among <16,1>
    bad[1][1] = (fresh_model(nav, (3, 500, 500, 2), "streamed"), layout[1][1], layout[1][2])  # no class at all
    bad[2][5] = (layout[5][0], layout[3][1] + 26, 2)                                         # overlaps the 27-problem item
    for lay, code in zip(bad, (ffi.SSC_EUNSUPPORTED, ffi.SSC_EUNSUPPORTED, ffi.SSC_EINVAL)):
        S_out, A_out = buffers(P * N, H4, 2, 1)
        assert many(ffi, lay, sp, P * N, H4, 2, 1, s0, S_out, A_out) == code
        assert (S_out == SENT_S).all() and (A_out == SENT_A).all()
    assert b"classes 2 and 1" in many_error(ffi, bad[0], sp, s0)


def many_error(ffi, lay, sp, s0):
    S_out, A_out = buffers(P * N, H4, 2, 1)
    many(ffi, lay, sp, P * N, H4, 2, 1, s0, S_out, A_out)
    return ffi.lib().ssc_last_error()


def test_population_routes_mfma_classes_fp32_and_alone_to_the_same_bits(nav, monkeypatch):
    """DynamicsModelPopulation.do_forward_sim_sampled: one many-call per grouped MFMA class next to the fp32 one, a scratch and
    a strided copy for the rest (a streamed 2 x 500 model and a lone 2 x 100 one), NAV_POPULATION_GROUPED = False for
    everyone -- all the bits of each model's own call on its own problems"""
    f32 = lambda dims, tag: nav.DynamicsModel(*SC.make_mlp(np.random.default_rng(zlib.crc32(tag.encode())), dims),
                                              SC.make_norm(np.random.default_rng(5), 2, 1), state_dim=2, act_dim=1, precision="f32")
    models = [fresh_model(nav, (3, 500, 2), "pop0"), f32((3, 32, 2), "pop1"), fresh_model(nav, (3, 100, 100, 2), "pop2"),
              fresh_model(nav, (3, 400, 2), "pop3"), f32((3, 30, 2), "pop4"), fresh_model(nav, (3, 500, 500, 2), "pop5"),
              fresh_model(nav, (3, 64, 2), "pop6"), fresh_model(nav, (3, 33, 2), "pop7")]
    counts, n_samples, H = [2, 1, 3, 14, 2, 1, 0, 2], 21, 4
    total = sum(counts)
    s0 = start_states("problem", total, n_samples, 2)
    low, high = SC.ACT_LOW[:1], SC.ACT_HIGH[:1]
    want_S, want_A = buffers(total * n_samples, H, 2, 1)
    at = 0
    for mo, n in zip(models, counts):
        if n:
            sp = nav.mpc_sampling(n_samples, low, high, SC.SEED, SC.PID0 + at, SC.T_STEP)
            A_p = torch.empty((n * n_samples, H, 1), device="cuda")
            want_S[:, at * n_samples:(at + n) * n_samples] = mo.do_forward_sim_sampled(s0[at:at + n], sp, n * n_samples, H, A_out=A_p)
            want_A[at * n_samples:(at + n) * n_samples] = A_p
        at += n
    pop = nav.DynamicsModelPopulation(models)
    monkeypatch.setattr(nav, "NAV_POPULATION_MFMA_MIN_GROUP", 2)
    A, B, C = "alone", "mfma<16,1>", "mfma<4,1>"
    for grouped, ways in ((True, [B, "many", A, B, "many", A, C, C]), (False, [A] * 8)):
        monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", grouped)
        assert pop.sim_ways == ways
        got_S, got_A = buffers(total * n_samples, H, 2, 1)
        sp = nav.mpc_sampling(n_samples, low, high, SC.SEED, SC.PID0, SC.T_STEP)
        out = pop.do_forward_sim_sampled(s0, sp, counts, H, out=got_S, A_out=got_A)
        torch.cuda.synchronize()
        assert out is got_S and torch.equal(got_S, want_S) and torch.equal(got_A, want_A), grouped
        assert sorted(pop._sim_mfma) == ([B, C] if grouped else [])
