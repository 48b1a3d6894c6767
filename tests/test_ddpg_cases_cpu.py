"""The DDPG learner's case matrix (tests/ddpg_cases.py) held to its own premises, without the kernel: the kernels the table
reaches against the dispatch (restated from the shapes, and through the library's host-only ssc_ddpg_learner_path), the
conditions on the inputs, the gradient restatement against O.ddpg_train_step, the constants of the bound, the float32
emulation inside the bound and inside the step-1 checks of the GPU test, and the mutants outside it.

Recorded with this table: max r_case = 1.029 (gradients, op_l2), 1.515 (losses, fx_o2_relu), so C_GRAD = 4.5 and C_LOSS = 6.5;
r_case of the gradients 0.038 (ln_37_19_o8_b77_floor) .. 1.029 over the whole table, the LayerNorm cases at 0.038 .. 0.431; rows that pass
the margin: 59 .. 100 % of the candidates; nearest mutant: drop_last_row at wd_128_64_b4096, 246 bounds (665 at the LayerNorm case of
batch 256); the older moment check accepts a dropped row at ft_o2_relu_b1024, ft_o3_relu_b4096 and wd_128_64_b4096.  Not emulated (they use
the other cases' constants): the four batch-4096 cases and wd_200_100_o3_b1024.  The per-case table is NOTEBOOK section 21."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import ddpg_cases as D

CASES, EMULATED = D.CASES, D.EMULATED


@pytest.fixture(scope="module")
def table():
    """per emulated case: the float32 emulation of its batch, computed once"""
    return {c.name: D.step(D.case_data(c), f32=True) for c in EMULATED}


# ------------------------------------------------------------------------------------------------------------ dispatch --
def test_table_reaches_every_learner_kernel():
    by = lambda path: [c for c in CASES if c.path == path]
    kernels = {k for c in CASES for k in c.kernels}
    # all 16 instantiations of the shape-specialised kernel: O x TANH2 x TILED x statistics
    for o in (2, 3):
        for tanh2 in ("true", "false"):
            for tiled in ("true", "false"):
                for rms in ("", ", const double *"):
                    assert "ddpg_train_fixed_kernel<%d, %s, %s%s>" % (o, tanh2, tiled, rms) in kernels
    assert len([k for k in kernels if k.startswith("ddpg_train_fixed_kernel")]) == 16
    assert all(c.B == 64 for c in by(D.FIXED)) and {c.B for c in by(D.FIXED_TILED)} >= {128, 1024, 4096}
    assert {c.stats for c in by(D.FIXED)} == {c.stats for c in by(D.FIXED_TILED)} == {None, "floor", "wide"}
    assert any(c.path == D.FIXED_TILED and "ddpg_wide_apply_kernel<true>" in c.kernels for c in CASES)
    # where the older moment check is blind: the tiled batches the vectorised loop trains on, both activations at 4096
    assert any(c.path == D.FIXED_TILED and c.obs == 3 and c.B == 1024 and not c.llt and c.stats is None for c in CASES)
    assert {c.llt for c in by(D.FIXED_TILED) if c.B == 4096} == {True, False}
    # the step interpreter: ragged unit groups, the widest observation, the shipped shape forced, an actor narrower than its critic
    interp = by(D.INTERPRETER)
    assert all(c.kernels == ("ddpg_train_kernel",) and c.B == 64 and c.stats is None for c in interp)
    assert any(c.ah == (24, 20) and c.ch == (24, 20) for c in interp) and any(c.obs == 8 and c.ah == (64, 32) for c in interp)
    assert {c.obs for c in interp if c.env == D.I_ and c.ah == (64, 32)} == {2, 3}
    assert any(c.ah[0] < c.ch[0] and c.ah[1] < c.ch[1] for c in interp)
    assert {c.llt for c in interp} == {True, False}
    # the multi-workgroup kernels
    wide = by(D.WIDE)
    assert {"ddpg_wide_grad_kernel<>", "ddpg_wide_grad_kernel<const double *>", "ddpg_wide_apply_kernel<false>",
            "ddpg_wide_apply_kernel<true>", "ddpg_wide_prepare_kernel"} <= kernels
    plain = [c for c in wide if c.stats is None and c.env is None and not c.ln and not c.l2 and not c.clip]
    assert {(128, 64), (200, 100), (37, 19)} <= {c.ah for c in plain} and any(c.ah != c.ch for c in plain)
    assert any(c.ah[0] > c.ch[0] for c in plain) and any(c.ah[0] < c.ch[0] for c in plain)
    assert {16, 17, 32, 50, 77, 4096} <= {c.B for c in plain} and any(c.obs == 8 and c.ah == (37, 19) for c in plain)
    assert {c.B for c in wide if c.env == D.W_ and c.ah == (64, 32) and c.stats is None} >= {64, 1024}
    # the shapes that reach them only BECAUSE statistics are present, and wide shapes with statistics
    rer = [c for c in wide if c.stats and D.learner_path(c.obs, c.ah, c.ch, c.B, c.ln, c.l2, c.clip, False, c.env == D.I_, c.env == D.W_) == D.INTERPRETER]
    assert any(c.ah == (24, 20) for c in rer) and any(c.obs == 8 for c in rer) and any(c.env == D.I_ for c in rer)
    assert any(c.stats and c.env == D.W_ and c.B == 1024 for c in wide) and any(c.stats and c.ah == (200, 100) for c in wide)
    assert {c.stats for c in wide} == {None, "floor", "wide"}
    # LayerNorm, critic_l2_reg alone, clip_norm alone (binding for all, some, none), all three
    assert any(c.ln and not c.l2 and not c.clip for c in wide) and any(c.ln and c.stats for c in wide)
    assert any(c.l2 and not c.clip and not c.ln for c in wide)
    assert {c.clip for c in wide if c.clip and not c.l2 and not c.ln} == {"all", "some", "none"}
    assert len([c for c in wide if c.ln and c.l2 and c.clip]) >= 2
    assert {c.llt for c in wide} == {True, False}
    # both soft-update rates on every path, plain and prepared apply pass
    for path in (D.FIXED, D.FIXED_TILED, D.INTERPRETER, D.WIDE):
        assert {c.tau for c in by(path)} == set(D.TAUS), path
    assert any(c.tau == 0.3 and "ddpg_wide_apply_kernel<true>" in c.kernels for c in CASES)
    # the cases left out of the sequential emulation
    assert [c.name for c in CASES if not c.emulate] == [c.name for c in CASES if c.B == 4096 or (c.B == 1024 and max(c.ah + c.ch) >= 200)]
    assert len(CASES) == len(D.CASE_BY_NAME)


def test_restated_dispatch_is_the_pinned_table():
    """D.learner_path == the rows of tests/test_ddpg_layout_host.py's table that bring a workspace (act_dim 1)"""
    from tests.test_ddpg_layout_host import PATHS
    n = 0
    for kw, have_ws, have_rms, want_interp, want_wide, want in PATHS:
        if not have_ws or kw.get("act", 1) != 1:
            continue
        h = kw.get("h", (64, 32))
        got = D.learner_path(kw.get("obs", 2), tuple(h), tuple(kw.get("critic_h") or h), kw.get("B", 64), bool(kw.get("layer_norm", 0)),
                             kw.get("critic_l2_reg", 0.0), kw.get("clip_norm", 0.0) or None, have_rms, want_interp, want_wide)
        assert got == want, (kw, have_rms, want_interp, want_wide)
        n += 1
    assert n >= 30


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_library_sends_the_case_where_the_table_says(ffi, monkeypatch, case):
    """the library's own host-only rule, the two switches read from the environment as train_on's call reads them"""
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)
    if case.env:
        monkeypatch.setenv(case.env, "1")
    d = ffi.DdpgDesc()
    d.obs_dim, d.act_dim, d.batch_size, d.last_layer_tanh = case.obs, 1, case.B, int(case.llt)
    (d.actor_h1, d.actor_h2), (d.critic_h1, d.critic_h2) = case.ah, case.ch
    d.layer_norm, d.critic_l2_reg, d.clip_norm = int(case.ln), case.l2, D.case_data(case)["clip_norm"] or 0.0
    assert ffi.lib().ssc_ddpg_learner_path(ctypes.byref(d), 1, int(case.stats is not None)) == case.path


# -------------------------------------------------------------------------------------------------------------- inputs --
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_generator_conditions(case):
    d, ref = D.case_data(case), D.reference(case)
    bi = d["idx"][0]
    n = d["s"].shape[0]
    assert n == 3 * case.B and d["idx"].shape == (1, case.B) and len(set(bi.tolist())) == case.B and 0 <= bi.min() and bi.max() < n
    assert d["good_share"] >= 0.5               # the margin is a choice of inputs, not a filter that keeps a special few
    assert np.all(D.row_margin(d, bi) >= D.THR) and min(float(np.abs(p).min()) for p in ref["relu_pre"]) >= D.THR
    # the conditioning of the older learner tests: every parameter perturbed, targets offset, terminals, s2 near s
    for net in ("actor", "critic"):
        assert all(np.all(v != 0) for v in d[net].values())
        assert all(np.all(d["target_" + net][k] != v) for k, v in d[net].items())
    assert (n < 150 or 0.03 <= d["t"].mean() <= 0.2) and (case.B < 64 or d["t"][bi].any()) and not d["t"][bi].all()
    assert 0 < np.abs(d["s2"] - d["s"]).max() < 0.1
    if case.stats:
        xh = [np.clip((x[bi].astype(np.float64) - d["mean"]) / d["std"].astype(np.float64), -5, 5) for x in (d["s"], d["s2"])]
        assert np.all(np.abs(d["mean"]) > 0.05)
        if case.stats == "floor":       # inputs on both clips, most rows clear of them
            assert np.all(d["std"] == np.float32(0.1))
            for x in xh:
                assert (x == 5).any() and (x == -5).any() and np.mean((np.abs(x) < 5).all(axis=1)) >= 0.5
        else:
            assert np.all(d["std"] > 0.2) and all(np.abs(x).max() < 5 for x in xh)
    elif case.obs == 3:
        assert (np.abs(d["s"][bi]) > 5).any()
    assert all(np.isfinite(g).all() for net in ("actor", "critic") for g in ref["g"][net].values())
    # clip_norm: no variable's norm within 1 % of the threshold, and it binds what the case claims
    norms = np.array([v for net in ("actor", "critic") for v in d["norms"][net].values()])
    assert len(norms) == (20 if case.ln else 12)
    if case.clip:
        c = d["clip_norm"]
        assert np.all(np.abs(norms / c - 1.0) > 0.01)
        bound = int((norms > c).sum())
        assert ref["n_bound"] == bound
        assert {"all": bound == len(norms), "none": bound == 0, "some": 2 <= bound <= len(norms) - 2}[case.clip], (bound, len(norms))
    else:
        assert d["clip_norm"] is None


@pytest.mark.parametrize("kind", ["floor", "wide"])
@pytest.mark.parametrize("obs_dim", [2, 3, 8])
def test_edge_statistics_are_the_mean_std_the_package_derives(obs_dim, kind):
    """D.edge_stats restates obs_rms.mean_std_f32 on its own block"""
    from smartstartcontinuous_amd.obs_rms import mean_std_f32
    block, mean, std, _ = D.edge_stats(obs_dim, kind)
    m, s = mean_std_f32(block, obs_dim)
    assert m.tobytes() == mean.tobytes() and s.tobytes() == std.tobytes()


@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.name)
def test_margin_covers_float32(table, case):
    """sequential float32 moves no relu pre-activation by more than half the margin: no mask of the batch can flip"""
    for p64, p32 in zip(D.reference(case)["relu_pre"], table[case.name]["relu_pre"]):
        assert np.max(np.abs(p32 - p64)) <= D.THR / 2 and np.array_equal(p32 > 0, p64 > 0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gradient_restatement_equals_oracle(case):
    """D.step IS O.ddpg_train_step's gradient: after one step from zero moments the oracle's m = 0.1 g and v = 0.001 g^2;
    its losses are the oracle's"""
    d, ref = D.case_data(case), D.reference(case)
    bi = d["idx"][0]
    nets = [{k: v.astype(np.float64) for k, v in d[n].items()} for n in ("actor", "critic", "target_actor", "target_critic")]
    nA, nC = D.flat(nets[0]).size, D.flat(nets[1]).size
    adam = dict(m_actor=np.zeros(nA), v_actor=np.zeros(nA), t_actor=0, m_critic=np.zeros(nC), v_critic=np.zeros(nC), t_critic=0)
    xs = [x[bi].astype(np.float64) for x in (d["s"], d["s2"])]
    if case.stats:
        xs = [(x - d["mean"].astype(np.float64)) / d["std"].astype(np.float64) for x in xs]
    out = O.ddpg_train_step(*nets, adam, (xs[0], d["a"][bi], d["r"][bi], d["t"][bi], xs[1]), gamma=D.GAMMA, tau=case.tau, actor_lr=D.LR,
                            critic_lr=D.LR, last_layer_tanh=case.llt, obs_clip=D.OBS_CLIP, critic_l2_reg=case.l2, clip_norm=d["clip_norm"])
    new, cl, al = out[4], out[5], out[6]
    assert abs(cl - float(ref["loss"][0])) <= 1e-12 * max(1.0, abs(cl)) and abs(al - float(ref["loss"][1])) <= 1e-12 * max(1.0, abs(al))
    for net in ("actor", "critic"):
        g = D.flat(ref["g"][net])
        scale = np.abs(g).max()
        assert np.allclose(new["m_" + net], (1 - 0.9) * g, rtol=1e-9, atol=1e-12 * scale)
        assert np.allclose(new["v_" + net], (1 - 0.999) * g * g, rtol=1e-9, atol=1e-12 * scale * scale)


# -------------------------------------------------------------------------------------------------------------- bounds --
def test_bound_constants_cover_the_table(table):
    rg = {c.name: D.grad_ratio(D.reference(c), table[c.name]["g"]) for c in EMULATED}
    rl = {c.name: max(D.loss_ratios(D.reference(c), table[c.name]["loss"])) for c in EMULATED}
    for c in EMULATED:
        print("DDPG_CASES %-26s r_case gradients %.3f losses %.3f" % (c.name, rg[c.name], rl[c.name]))
    lo = min(v for v in rg.values() if v > 0)
    print("r_case: gradients %.3f (%s) .. %.3f (%s), losses up to %.3f (%s)" % (lo, min(rg, key=rg.get), max(rg.values()), max(rg, key=rg.get),
                                                                           max(rl.values()), max(rl, key=rl.get)))
    for C, r in ((D.C_GRAD, rg), (D.C_LOSS, rl)):       # 4 * max r_case rounded up: not below it, not more than twice it
        assert 4 * max(r.values()) <= C <= 2 * 4 * max(r.values()), (C, 4 * max(r.values()))
    # A follows the error across the whole table, LayerNorm included: no family of cases sticks out
    assert lo > 0 and max(rg.values()) / lo <= 50, (lo, max(rg.values()))


@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.name)
def test_emulation_passes_the_bound_and_the_step1_checks(table, case):
    d, ref, e = D.case_data(case), D.reference(case), table[case.name]
    assert D.grad_ratio(ref, e["g"]) <= D.C_GRAD and max(D.loss_ratios(ref, e["loss"])) <= D.C_LOSS
    worst = np.zeros(4)
    for net in ("actor", "critic"):
        for k, theta in d[net].items():
            m, v, theta1 = D.adam1_32(theta, e["g"][net][k])
            f = np.float32
            target1 = (f(1) - f(case.tau)) * d["target_" + net][k] + f(case.tau) * theta1
            worst = np.maximum(worst, D.step1_ratios(theta, ref["g"][net][k], ref["A"][net][k], m, v, theta1)
                               + (D.target_ratio(d["target_" + net][k], theta1, target1, case.tau),))
    print(case.name, "emulated step 1, err / allowed of (m, v, theta, target):", worst.round(3))
    assert np.all(worst <= 1.0), worst


def _changed(a, b):
    return any(not np.array_equal(a["g"][n][k], b["g"][n][k]) for n in ("actor", "critic") for k in a["g"][n]) or \
        tuple(map(float, a["loss"])) != tuple(map(float, b["loss"]))


_DIST = {}


def _mutant_distances(case):
    """{mutant: distance from the fp64 gradients in bounds (C_GRAD / C_LOSS included)} over the mutants that change the case"""
    if case.name not in _DIST:
        d, ref = D.case_data(case), D.reference(case)
        out = {}
        for m in D.MUTANTS:
            if (m == "rows_16_31_twice" and case.B < 32) or (m == "bias_missing_tile" and case.B <= 16):
                continue
            x = D.step(d, mut=m, sizes=False)
            if _changed(x, ref):
                out[m] = max(D.grad_ratio(ref, x["g"]) / D.C_GRAD, max(D.loss_ratios(ref, x["loss"])) / D.C_LOSS)
        _DIST[case.name] = out
    return _DIST[case.name]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bound_rejects_every_mutant(case):
    """every mutant, stated on the fp64 algebra, is at least MUTANT_MIN bounds out wherever it changes the iteration at all; a
    case a mutant cannot change -- no statistics, no regulariser, a clip that binds nowhere -- does not count"""
    dists = _mutant_distances(case)
    print("DDPG_MUTANTS", case.name, {k: float("%.3g" % v) for k, v in dists.items()})
    always = set(D.MUTANTS) - {"l2_on_biases", "clip_global_norm", "neighbour_mean", "no_obs_clip", "terminal_ignored"}
    always -= {"rows_16_31_twice"} if case.B < 32 else set()
    always -= {"bias_missing_tile"} if case.B <= 16 else set()
    always -= {"dq_1_over_B"} if case.clip == "all" else set()          # a clip that binds everywhere divides the scale out again
    assert always <= set(dists), always - set(dists)
    assert ("l2_on_biases" in dists) == bool(case.l2) and ("neighbour_mean" in dists) == bool(case.stats)
    assert case.clip in (None, "none") or "clip_global_norm" in dists
    assert case.stats != "floor" or "no_obs_clip" in dists
    assert ("terminal_ignored" in dists) == bool(D.case_data(case)["t"][D.case_data(case)["idx"][0]].any())
    for m, v in dists.items():
        assert v >= D.MUTANT_MIN, (case.name, m, v)


@pytest.mark.parametrize("case", [c for c in EMULATED if c.B <= 256], ids=lambda c: c.name)
def test_bound_rejects_every_mutant_of_the_emulation(table, case):
    """the same mutants applied to the float32 emulation: at least 2 bounds out wherever they change it, and never further
    from their fp64 statement than the emulation is from the reference -- C_GRAD / 4 bounds -- by more than a bound"""
    d, ref, e = D.case_data(case), D.reference(case), table[case.name]
    for m, v64 in _mutant_distances(case).items():
        x = D.step(d, f32=True, mut=m)
        if not _changed(x, e):
            continue
        v32 = max(D.grad_ratio(ref, x["g"]) / D.C_GRAD, max(D.loss_ratios(ref, x["loss"])) / D.C_LOSS)
        assert v32 >= 2.0, (case.name, m, v32)
        assert v32 >= v64 - 1.0 or v32 >= 100, (case.name, m, v32, v64)


def test_every_mutant_is_caught_on_several_cases():
    caught = {m: sum(m in _mutant_distances(c) for c in CASES) for m in D.MUTANTS}
    near = min(((v, m, c.name) for c in CASES for m, v in _mutant_distances(c).items()))
    print("nearest mutant: %s at %s, %.2f bounds" % (near[1], near[2], near[0]))
    assert all(n >= 3 for n in caught.values()), caught


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_target_bound_rejects_the_pre_step_parameters(case):
    """a soft update that mixes in the parameters from BEFORE the Adam step: every element is off by tau * |step|"""
    d, ref = D.case_data(case), D.reference(case)
    f = np.float32
    for net in ("actor", "critic"):
        for k, theta in d[net].items():
            _, _, theta1 = D.adam1_32(theta, ref["g"][net][k])
            mutant = (f(1) - f(case.tau)) * d["target_" + net][k] + f(case.tau) * theta
            moved = theta1 != theta
            assert moved.any()
            t0 = d["target_" + net][k]
            tau = float(np.float32(case.tau))
            want = (1.0 - tau) * t0.astype(np.float64) + tau * theta1.astype(np.float64)
            allowed = 4 * D.EPS32 * (np.abs(t0) + tau * np.abs(theta1))
            # nine in ten of the elements that moved miss the bound by a factor two (the rest have gradients next to zero -- units
            # few rows switch on -- and steps far below lr), every variable has some
            assert np.mean((np.abs(mutant - want) / allowed)[moved] >= 2.0) >= 0.9
            # and at tau = 0.3 the miss is tau * |step|, about 3e-4
            if case.tau == 0.3:
                assert np.median(np.abs(mutant - ((1 - 0.3) * t0 + 0.3 * theta1.astype(np.float64)))[moved]) > 1e-4


def test_dropped_row_passes_the_older_moment_check_and_fails_the_bound():
    """The gap this matrix closes: at the tiled batch sizes a dropped batch row stays inside
    allclose(m, m64, rtol=1e-3, atol=1e-7), the moment check of _ddpg_kernel_vs_oracle -- and is far outside the bound."""
    accepted = []
    for c in CASES:
        if c.B < 1024:
            continue
        d, ref = D.case_data(c), D.reference(c)
        x = D.step(d, mut="drop_last_row", sizes=False)
        for net in ("actor", "critic"):
            g, gm = D.flat(ref["g"][net]), D.flat(x["g"][net])
            if np.allclose(0.1 * gm, 0.1 * g, rtol=1e-3, atol=1e-7):
                accepted.append((c.name, net))
        assert D.grad_ratio(ref, x["g"]) / D.C_GRAD >= D.MUTANT_MIN, c.name
    print("the older moment check accepts a dropped row at:", accepted)
    assert {c for c, _ in accepted} & {c.name for c in CASES if c.B == 1024} and {c for c, _ in accepted} & {c.name for c in CASES if c.B == 4096}
