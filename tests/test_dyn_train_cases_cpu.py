"""The dynamics-model training step's case table (tests/dyn_train_cases.py) held to its own premises, without the kernel:
the dispatch classes it reaches, the ReLU margin of the bounded batch, the constants of the bound, the float32 emulation
inside the bound and inside the step-1 checks of the GPU test, the emulation mutants outside it, and the gradient
restatement against O.mlp_train_step.

Recorded with this table: max r_case = 4.27 (gradients, g_l1_b500), 1.50 (loss, f128_h16_b513), so C_GRAD = 17.5 and
C_LOSS = 6.0; rows that pass the margin: 40 .. 100 % of the candidates; nearest mutant: drop_k_chunk at g_l4, 41.8
bounds away, every other mutant x case >= 76 bounds; the emulated step 1 uses at most 0.25 of the moment checks and
stays inside the parameter interval.  The two B = 65536 rows are not emulated (dyn_train_cases.py says why)."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import dyn_train_cases as D

EMULATED = [c for c in D.CASES if c.emulate]


@pytest.fixture(scope="module")
def table():
    """per emulated case: the float32 emulation of its first batch, computed once"""
    return {c.name: D.emu32_of(c) for c in EMULATED}


def test_table_reaches_every_dispatch_class():
    fused = [c for c in D.CASES if c.path == "fused"]
    gen = [c for c in D.CASES if c.path == "generic"]
    # fused: every instantiation with in / out at the template size and below it
    for k, (IN, OUT) in (("<3,2>", (3, 2)), ("<4,3>", (4, 3)), ("<12,8>", (12, 8))):
        mine = [c for c in fused if c.kernel == k]
        assert any(c.dims[0] == IN and c.dims[2] == OUT for c in mine), k
        assert any(c.dims[0] < IN for c in mine) and any(c.dims[2] < OUT for c in mine), k
    assert {c.dims[1] for c in fused} >= {1, 16, 17, 32, 33, 100, 256, 257, 500, 512}
    assert {c.hd_pad for c in fused} == {16, 32, 64, 128, 256, 512} and {c.S for c in fused} == {32, 16, 8, 4, 2, 1}
    assert any(c.lds_optin and c.hd_pad == 512 for c in fused) and any(c.lds_optin and c.kernel == "<12,8>" and c.hd_pad == 256 for c in fused)
    assert any(not c.lds_optin for c in fused)
    assert {c.p_class for c in fused} == {"lt512", "512_2048", "gt2048"}
    assert any(c.dims == (4, 500, 3) and c.P == 4003 for c in fused)
    assert {c.B for c in fused} >= {1, 31, 32, 33, 512, 2049, 65536} and {c.B for c in fused} & {513, 544}
    assert {c.G for c in fused} >= {1, 2, 16, 17, 65, 2048}
    assert any(c.B == 65536 and c.dims == (3, 32, 2) for c in fused)
    # generic: every depth, one hidden layer just outside each limit of the fused kernel
    assert {len(c.dims) - 1 for c in gen} == {1, 2, 3, 4} and D.SSC_MAX_LAYERS == 4
    two = [c.dims for c in gen if len(c.dims) == 3]
    assert any(d[0] == 13 for d in two) and any(d[1] == 513 for d in two) and any(d[2] == 9 for d in two)
    assert any(len(c.dims) == 5 and len(set(c.dims[1:-1])) == 3 for c in gen)
    # every GEMM role meets every class of the wave split and of the double-buffered loop
    for role in ("fwd", "bwd", "wgrad"):
        mine = [g for c in gen for g in c.gemms if g[0] == role]
        assert {g[4] for g in mine} == {"one_wave", "c32", "c64", "c96", "c97+"}, role
        assert any(D.last_wave_short(g[3]) for g in mine), role
        assert any(g[3] == 500 for g in mine), role
        if role != "wgrad":          # row operands: the 16-byte path and the scalar path (the gradient GEMM reads columns)
            assert {g[5] for g in mine} == {False, True}, role
            assert any(g[5] and g[3] > 8 for g in mine) and any(not g[5] and g[3] > 8 for g in mine), role
    # tile edges
    Ns = {g[2] for c in gen for g in c.gemms}
    assert {32, 33} <= Ns
    ones_rows = {g[1] - 1 for c in gen for g in c.gemms if g[0] == "wgrad"}
    assert {31, 32} <= ones_rows
    assert any(c.dims[-1] == 33 and c.B > 32 for c in gen)
    assert {c.B for c in gen} >= {1, 33, 77, 513, 65536}
    assert any(c.B == 65536 and max(c.dims) <= 8 for c in gen)
    assert [c.name for c in D.CASES if not c.emulate] == [c.name for c in D.CASES if c.B == 65536]
    assert {c.path for c in D.CASES if c.null_loss} == {"fused", "generic"}


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_generator_margin_and_rows(case):
    d, ref = D.case_data(case), D.reference(case)
    n, idx0 = d["X"].shape[0], d["idx"][0]
    assert d["idx"].shape == (4, case.B) and len(set(idx0.tolist())) == case.B
    assert n - 1 in idx0 and (0 in idx0 if case.B > 1 else d["idx"][1, 0] == 0)
    assert d["idx"].min() >= 0 and d["idx"].max() < n
    assert ref["margin"] >= D.THR and np.all(D.row_margin(d["Ws"], d["bs"], d["X"][idx0]) >= D.THR)
    assert d["good_share"] >= 0.4       # the margin is a choice of inputs, not a filter that keeps a special few
    assert np.isfinite(ref["loss"]) and all(np.isfinite(g).all() for g in ref["gW"] + ref["gb"])


@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.name)
def test_margin_covers_float32(table, case):
    """sequential float32 moves no hidden pre-activation by more than half the margin: no mask of the batch can flip"""
    ref, e = D.reference(case), table[case.name]
    for p64, p32 in zip(ref["pre"], e["pre"]):
        assert np.max(np.abs(p32 - p64)) <= D.THR / 2
        assert np.array_equal(p32 > 0, p64 > 0)


@pytest.mark.parametrize("case", [c for c in EMULATED if c.B * max(c.dims) <= 40000], ids=lambda c: c.name)
def test_gradient_restatement_equals_oracle(case):
    """grad64 IS O.mlp_train_step's gradient: after one step from zero moments the oracle's m = (1 - beta1) g, v = (1 - beta2) g^2"""
    d, ref = D.case_data(case), D.reference(case)
    L = len(d["Ws"])
    zero = dict(mW=[np.zeros(w.shape) for w in d["Ws"]], vW=[np.zeros(w.shape) for w in d["Ws"]],
                mb=[np.zeros(b.shape) for b in d["bs"]], vb=[np.zeros(b.shape) for b in d["bs"]], t=0)
    _, _, new, loss = O.mlp_train_step(d["Ws"], d["bs"], zero, d["X"][d["idx"][0]], d["Z"][d["idx"][0]], lr=D.LR)
    assert abs(loss - ref["loss"]) <= 1e-14 * max(1.0, ref["loss"])
    for l in range(L):
        for m, v, g in ((new["mW"][l], new["vW"][l], ref["gW"][l]), (new["mb"][l], new["vb"][l], ref["gb"][l])):
            assert np.allclose(m, (1 - 0.9) * g, rtol=1e-12, atol=1e-300) and np.allclose(v, (1 - 0.999) * g * g, rtol=1e-12, atol=1e-300)


def test_bound_constants_cover_the_table(table):
    rg = {c.name: D.grad_ratio(D.reference(c), table[c.name]["gW"], table[c.name]["gb"]) for c in EMULATED}
    rl = {c.name: D.loss_ratio(D.reference(c), table[c.name]["loss"]) for c in EMULATED}
    print("r_case gradients:", {k: round(v, 2) for k, v in rg.items()})
    print("r_case loss:", {k: round(v, 2) for k, v in rl.items()})
    print("max r_case: gradients %.3f (%s), loss %.3f (%s)" % (max(rg.values()), max(rg, key=rg.get), max(rl.values()), max(rl, key=rl.get)))
    for C, r in ((D.C_GRAD, rg), (D.C_LOSS, rl)):      # 4 * max r_case, rounded up to the next half
        assert C == np.ceil(2 * 4 * max(r.values())) / 2, (C, 4 * max(r.values()))


@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.name)
def test_emulation_passes_the_bound_and_the_step1_checks(table, case):
    d, ref, e = D.case_data(case), D.reference(case), table[case.name]
    assert D.grad_ratio(ref, e["gW"], e["gb"]) <= D.C_GRAD and D.loss_ratio(ref, e["loss"]) <= D.C_LOSS
    worst = np.zeros(3)
    for l in range(len(e["gW"])):
        for theta, g32, g64, A in ((d["Ws"][l], e["gW"][l], ref["gW"][l], ref["A_W"][l]), (d["bs"][l], e["gb"][l], ref["gb"][l], ref["A_b"][l])):
            m, v, theta1 = D.adam1_32(theta, g32)
            worst = np.maximum(worst, D.step1_ratios(theta, g64, A, m, v, theta1))
    print(case.name, "emulated step 1, err / allowed of (m, v, theta):", worst.round(3))
    assert np.all(worst <= 1.0), worst


def test_bound_rejects_every_mutant(table):
    """every mutant is outside the bound wherever it changes the step at all (a case where it changes nothing, such as the
    two scale mutants at out = 1 or the mask mutant without a hidden layer, does not count), and on several cases each"""
    caught = {m: 0 for m in D.MUTANTS}
    for c in EMULATED:
        ref, e = D.reference(c), table[c.name]
        dists = {}
        for m in D.MUTANTS:
            x = D.emu32_of(c, m)
            if all(np.array_equal(a, b) for a, b in zip(x["gW"] + x["gb"] + [x["loss"]], e["gW"] + e["gb"] + [e["loss"]])):
                continue
            dists[m] = max(D.grad_ratio(ref, x["gW"], x["gb"]) / D.C_GRAD, D.loss_ratio(ref, x["loss"]) / D.C_LOSS)
            caught[m] += dists[m] > 1.0
        print(c.name, "mutant distance / bound:", {k: round(v, 1) for k, v in dists.items()})
        for m, v in dists.items():
            assert v > 1.0, (c.name, m, v)
    assert all(n >= 3 for n in caught.values()), caught
