"""The Pop-Art learner's case matrix (tests/popart_grad_cases.py) held to its own premises, without the kernel: the kernels
the table claims against the one Pop-Art path, the conditions on the inputs and on the four starting blocks, the restatement
against tests/popart_cases.popart_step and against torch autograd, the constants of the bounds from the float32 emulation,
the emulation inside every check the GPU test applies, and the mutants outside them.

Recorded with this table: max r = 0.802 (gradients, pa_l2), 0.349 (losses, pa_all_64_64) -- 4 r is under C_GRAD = 4.5 and
C_LOSS = 6.5 of the plain learner, which are used unchanged; 0.723 (y, pa_mixed_a200_c64), 0.780 (W3' / b3', pr_o8_wide_stats),
0.365 (scalars, pa_mixed_a128_c200; zero at the other cases), so C_Y = 3.0, C_RESC = 3.5, C_STAT = 2.0 (one unit in the last
place).  Nearest mutant: moments_rescaled at pa_ln_64_64_b256, 4.9 bounds (the large block, sigma moved by 0.2 %); every mutant
under 100 bounds is at a large-block case.  The per-case table is NOTEBOOK section 23."""
import numpy as np
import pytest

from tests import ddpg_cases as D
from tests import popart_cases as PC
from tests import popart_grad_cases as P

CASES, EMULATED = P.CASES, P.EMULATED


@pytest.fixture(scope="module")
def table():
    """per emulated case: the float32 emulation of its iteration, computed once"""
    return {c.name: P.popart_step1(P.case_data(c), f32=True) for c in EMULATED}


# --------------------------------------------------------------------------------------------------------------- table --
def test_table_reaches_every_popart_kernel():
    kernels = {k for c in CASES for k in c.kernels}
    assert {"ddpg_wide_grad_kernel<PopTarget>", "ddpg_wide_grad_kernel<PopGrad>", "ddpg_wide_grad_kernel<const double *, PopTarget>",
            "ddpg_wide_grad_kernel<const double *, PopGrad>", "ddpg_popart_renorm_kernel", "ddpg_wide_apply_kernel<false>",
            "ddpg_wide_apply_kernel<true>", "ddpg_wide_prepare_kernel"} == kernels
    # the dispatch restated: Pop-Art always takes the multi-workgroup path -- also at the shapes the plain call sends to the
    # one-workgroup kernels -- with the statistics build iff there are observation statistics and the prepared apply pass
    # iff critic_l2_reg or clip_norm is set
    for c in CASES:
        rms = "const double *, " if c.stats else ""
        want = ["ddpg_wide_grad_kernel<%sPopTarget>" % rms, "ddpg_popart_renorm_kernel", "ddpg_wide_grad_kernel<%sPopGrad>" % rms]
        want += ["ddpg_wide_prepare_kernel", "ddpg_wide_apply_kernel<true>"] if (c.l2 or c.clip) else ["ddpg_wide_apply_kernel<false>"]
        assert list(c.kernels) == want, c.name
    assert any(D.learner_path(c.obs, c.ah, c.ch, c.B, c.ln, c.l2, c.clip, False, False, False) == D.FIXED for c in CASES)
    plain = [c for c in CASES if not c.stats and not c.ln and not c.l2 and not c.clip]
    assert {1, 16, 17, 50, 64, 77, 256, 4096} <= {c.B for c in plain}
    assert {(64, 32), (37, 19), (128, 64), (200, 100)} <= {c.ah for c in plain}
    assert any(c.ah[0] < c.ch[0] for c in plain) and any(c.ah[0] > c.ch[0] for c in plain)
    assert any(c.obs == 8 and c.ah == (37, 19) and c.B == 77 for c in plain)
    assert any(c.ln and not c.l2 and not c.clip for c in CASES) and any(c.l2 and not c.clip and not c.ln for c in CASES)
    assert any(c.clip == "some" and not c.l2 and not c.ln for c in CASES) and any(c.ln and c.l2 and c.clip == "all" for c in CASES)
    stats = [c for c in CASES if c.stats]
    assert len(stats) == 3 and {c.stats for c in stats} == {"floor", "wide"} and any(c.obs == 8 for c in stats)
    assert {c.llt for c in CASES} == {True, False} and len([c for c in CASES if c.tau == 0.3]) >= 3
    assert any(c.tau == 0.3 and "ddpg_wide_apply_kernel<true>" in c.kernels for c in CASES)
    # every starting block at least twice
    for kind in P.BLOCKS:
        assert len([c for c in CASES if c.block == kind]) >= 2, kind
    # kept out of the sequential emulation as in the plain table
    assert [c.name for c in CASES if not c.emulate] == [c.name for c in CASES if c.B == 4096 or (c.B >= 1024 and max(c.ah + c.ch) >= 200)]
    assert len(CASES) == len(P.CASE_BY_NAME) and 16 <= len(CASES) <= 20


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_workspace_is_laid_out_as_the_gpu_test_reads_it(ffi, case):
    """the library's own host-only size rule: [the plain step's workspace | y | partials | scalars], each part rounded up to
    256 bytes -- where agent.popart_workspace() takes y, the partials and the scalars from"""
    import ctypes
    d = ffi.DdpgDesc()
    d.obs_dim, d.act_dim, d.batch_size, d.last_layer_tanh = case.obs, 1, case.B, int(case.llt)
    (d.actor_h1, d.actor_h2), (d.critic_h1, d.critic_h2) = case.ah, case.ch
    d.layer_norm, d.critic_l2_reg, d.clip_norm = int(case.ln), case.l2, P.case_data(case)["clip_norm"] or 0.0
    up = lambda x: (int(x) + 255) // 256 * 256
    plain = ffi.lib().ssc_ddpg_train_workspace_bytes(ctypes.byref(d))
    want = up(plain) + up(4 * case.B) + up(16 * ((case.B + 15) // 16)) + 256
    assert ffi.lib().ssc_ddpg_train_popart_workspace_bytes(ctypes.byref(d)) == want


def test_statistics_are_the_mean_std_the_package_derives():
    """P.mean_std32 restates obs_rms.mean_std_f32 (tests/popart_cases.ret_mean_std) at every block of the table, old and new"""
    for c in CASES:
        for block in (P.case_data(c)["ret_block"], P.reference(c)["block"]):
            assert P.mean_std32(block) == PC.ret_mean_std(block), c.name


def test_partial_sums_follow_the_butterfly():
    y = np.random.default_rng(0).normal(3, 5, 37).astype(np.float32)
    p = P.partial_sums(y)
    assert p.shape == (3, 2)
    y64 = y.astype(np.float64)
    for b in range(3):
        v = np.zeros(16)
        v[:len(y64[16 * b:16 * b + 16])] = y64[16 * b:16 * b + 16]
        for m in (8, 4, 2, 1):          # lane i adds lane i ^ m: what lane 0 ends with
            v = v + v[np.arange(16) ^ m]
        assert p[b, 0] == v[0]
    assert np.allclose(p.sum(0), [y64.sum(), (y64 * y64).sum()], rtol=1e-14, atol=0)


# -------------------------------------------------------------------------------------------------------------- inputs --
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_generator_conditions(case):
    d, ref = P.case_data(case), P.reference(case)
    bi = d["idx"][0]
    n = d["s"].shape[0]
    assert d["idx"].shape == (1, case.B) and len(set(bi.tolist())) == case.B and 0 <= bi.min() and bi.max() < n
    assert d["good_share"] >= 0.5
    # the margin: actor at s, the RESCALED critic at (s, a) and (s, pi(s))
    resc = dict(d, critic={k: np.asarray(ref["critic"][k]) for k in D.keys_of(d["critic"])})
    assert np.all(D.row_margin(d, bi) >= D.THR) and np.all(D.row_margin(resc, bi) >= D.THR)
    assert min(float(np.abs(p).min()) for p in ref["relu_pre"]) >= D.THR
    for net in ("actor", "critic"):
        assert all(np.all(v != 0) for v in d[net].values())
        assert all(np.all(d["target_" + net][k] != v) for k, v in d[net].items())
    assert 0.03 <= d["t"].mean() <= 0.2 and (case.B < 64 or d["t"][bi].any()) and not d["t"][bi].all()
    assert all(np.isfinite(g).all() for net in ("actor", "critic") for g in ref["g"][net].values())
    # the starting block and what the batch does to it; no variance within the margin of the floor
    mu_o, sg_o, mu_n, sg_n = ref["scalars"]
    b0 = d["ret_block"]
    assert "near" not in ref["floor_state"], (ref["floor_state"], ref["var64"])
    if case.block == "fresh":
        assert b0.tolist() == [0.0, 1e-2, 1e-2] and (mu_o, sg_o) == (0.0, 1.0) and ref["floor_state"] == ("off", "off")
    elif case.block == "floor":
        assert ref["floor_state"] == ("floor", "floor") and sg_o == sg_n == float(P.FLOOR32) and ref["E_scalars"][1] == ref["E_scalars"][3] == 0.0
        assert ref["var64"] < 5e-3 and mu_n != mu_o
    elif case.block == "moving":
        assert ref["floor_state"] == ("off", "off") and 4.0 <= sg_o <= 25.0 and abs(sg_n / sg_o - 1.0) >= 0.1 and abs(mu_n - mu_o) > 0.1
    else:
        assert ref["floor_state"] == ("off", "off") and abs(b0[2] - 1e6) < 1.0 and abs(abs(mu_o) / sg_o - 20.0) < 1e-3
        # float32 leaves sigma_n about 800 roundings (5e-5) of relative error here, C_GRAD times that is 2.2e-4 in the seed's
        # bound and MUTANT_MIN bounds are 5e-4: the batch moves sigma by three times that, or the old sigma cannot be told
        assert case.B >= 256 and abs(sg_n / sg_o - 1.0) >= 1.5e-3 and abs(mu_n - mu_o) >= 1e-3
        yn = (ref["y"] - mu_n) / sg_n                     # the normalised targets cancel: |y| + |mu| against |y - mu|
        assert np.median((np.abs(ref["y"]) + abs(mu_n)) / np.abs(ref["y"] - mu_n)) > 10 and np.median(np.abs(yn)) < 5
    if case.B == 1:
        assert ref["floor_state"][1] == "floor"
    assert ref["block"][2] == b0[2] + case.B
    norms = np.array([v for net in ("actor", "critic") for v in d["norms"][net].values()])
    if case.clip:
        c = d["clip_norm"]
        assert np.all(np.abs(norms / c - 1.0) > 0.01)
        bound = int((norms > c).sum())
        assert ref["n_bound"] == bound
        assert {"all": bound == len(norms), "some": 2 <= bound <= len(norms) - 2}[case.clip], (bound, len(norms))
    else:
        assert d["clip_norm"] is None


@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.name)
def test_margin_covers_float32(table, case):
    for p64, p32 in zip(P.reference(case)["relu_pre"], table[case.name]["relu_pre"]):
        assert np.max(np.abs(p32 - p64)) <= D.THR / 2 and np.array_equal(p32 > 0, p64 > 0)


def _net_inputs(case, d):
    bi = d["idx"][0]
    xs = [x[bi].astype(np.float64) for x in (d["s"], d["s2"])]
    if case.stats:
        xs = [(x - d["mean"].astype(np.float64)) / d["std"].astype(np.float64) for x in xs]
    return xs


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_restatement_equals_popart_step(case):
    """P.popart_step1 IS tests/popart_cases.popart_step (the restatement the six-iteration device test uses): y, block, the
    four scalars, both rescaled output layers, both losses, and the gradients through its first Adam step from zero moments"""
    d, ref = P.case_data(case), P.reference(case)
    bi = d["idx"][0]
    nets = [{k: v.astype(np.float64) for k, v in d[n].items()} for n in ("actor", "critic", "target_actor", "target_critic")]
    nA, nC = D.flat(nets[0]).size, D.flat(nets[1]).size
    adam = dict(m_actor=np.zeros(nA), v_actor=np.zeros(nA), t_actor=0, m_critic=np.zeros(nC), v_critic=np.zeros(nC), t_critic=0)
    xs = _net_inputs(case, d)
    out = PC.popart_step(*nets, adam, d["ret_block"], (xs[0], d["a"][bi], d["r"][bi], d["t"][bi], xs[1]), llt=case.llt, gamma=D.GAMMA,
                         tau=case.tau, actor_lr=D.LR, critic_lr=D.LR, critic_l2_reg=case.l2, clip_norm=d["clip_norm"])
    new, block, cl, al, y, sc = out[4], out[5], out[6], out[7], out[8], out[9]
    assert tuple(sc) == tuple(ref["scalars"])
    assert np.allclose(y.reshape(-1), ref["y"], rtol=1e-11, atol=1e-12 * np.abs(y).max()) and np.allclose(block, ref["block"], rtol=1e-12, atol=0)
    assert abs(cl - float(ref["loss"][0])) <= 1e-11 * max(1.0, abs(cl)) and abs(al - float(ref["loss"][1])) <= 1e-11 * max(1.0, abs(al))
    for net, p0 in (("critic", nets[1]), ("target_critic", nets[3])):
        want = PC.rescale_output_layer(p0, *sc)
        for k in ("W3", "b3"):
            assert np.allclose(ref[net][k], want[k], rtol=1e-13, atol=1e-15), (net, k)
    for net in ("actor", "critic"):
        g = D.flat(ref["g"][net])
        scale = np.abs(g).max()
        assert np.allclose(new["m_" + net], (1 - 0.9) * g, rtol=1e-8, atol=1e-11 * scale)
        assert np.allclose(new["v_" + net], (1 - 0.999) * g * g, rtol=1e-8, atol=1e-11 * scale * scale)


@pytest.mark.parametrize("name", ["pa_128_64_b256_relu", "pa_mixed_a128_c200"])
def test_gradients_match_autograd(name):
    """the restatement's gradients against torch autograd in float64 at a relu second layer and at mixed sizes: 1e-10"""
    import torch
    case = P.CASE_BY_NAME[name]
    d, ref = P.case_data(case), P.reference(case)
    assert not case.ln and not case.l2 and not case.clip and not case.stats
    tt = lambda x: torch.tensor(np.asarray(x, np.float64))
    act2 = torch.tanh if case.llt else torch.relu

    def critic_t(p, s, a):
        return act2(torch.cat([torch.relu(s @ p["W1"] + p["b1"]), a], dim=1) @ p["W2"] + p["b2"]) @ p["W3"] + p["b3"]

    def actor_t(p, s):
        return torch.tanh(act2(torch.relu(s @ p["W1"] + p["b1"]) @ p["W2"] + p["b2"]) @ p["W3"] + p["b3"])

    bi = d["idx"][0]
    mu_n, sg_n = ref["scalars"][2:]
    s, a = tt(np.clip(d["s"][bi].astype(np.float64), -5, 5)), tt(d["a"][bi])
    pc = {k: tt(ref["critic"][k]).requires_grad_() for k in D.KEYS}
    pa = {k: tt(d["actor"][k]).requires_grad_() for k in D.KEYS}
    closs = ((critic_t(pc, s, a) - tt((ref["y"].reshape(-1, 1) - mu_n) / sg_n)) ** 2).mean()
    aloss = -(critic_t(pc, s, actor_t(pa, s)) * sg_n + mu_n).mean()
    assert float(ref["loss"][0]) == pytest.approx(closs.item(), rel=1e-12) and float(ref["loss"][1]) == pytest.approx(aloss.item(), rel=1e-12)
    for net, p, loss in (("critic", pc, closs), ("actor", pa, aloss)):
        for k, g in zip(p, torch.autograd.grad(loss, list(p.values()))):
            w = g.numpy()
            assert np.max(np.abs(ref["g"][net][k] - w)) <= 1e-10 * np.max(np.abs(w)), (net, k)


# -------------------------------------------------------------------------------------------------------------- bounds --
def test_bound_constants_cover_the_table(table):
    rr = {c.name: P.raw_ratios(P.reference(c), table[c.name]) for c in EMULATED}
    for c in EMULATED:
        r = rr[c.name]
        print("POPART_CASES %-22s %-6s r_case gradients %.3f losses %.3f %.3f y %.3f rescaled %.3f scalars %.3f" % (
            c.name, c.block, r["grad"], r["loss_c"], r["loss_a"], r["y"], r["resc"], r["stat"]))
    top = lambda *keys: max(max(r[k] for k in keys) for r in rr.values())
    where = lambda *keys: max(rr, key=lambda n: max(rr[n][k] for k in keys))
    for name, keys in (("gradients", ("grad",)), ("losses", ("loss_c", "loss_a")), ("y", ("y",)), ("rescaled", ("resc",)), ("scalars", ("stat",))):
        print("max r %-9s %.3f (%s)" % (name, top(*keys), where(*keys)))
    # gradients and losses: 4 max r is under the plain learner's constants, which are used as they are
    assert 4 * top("grad") <= D.C_GRAD == P.C_GRAD_POP and 4 * top("loss_c", "loss_a") <= D.C_LOSS == P.C_LOSS_POP
    # the new ones: 4 max r rounded up -- not below it, not more than twice it -- and never below one unit in the last place
    for C, r, ulp in ((P.C_Y, top("y"), 0.0), (P.C_RESC, top("resc"), 2.0), (P.C_STAT, top("stat"), 2.0)):
        assert max(4 * r, ulp) <= C <= max(2 * 4 * r, ulp), (C, 4 * r)
    lo = min(r["grad"] for r in rr.values())
    assert lo > 0


@pytest.mark.parametrize("case", EMULATED, ids=lambda c: c.name)
def test_emulation_passes_every_check(table, case):
    """the float32 emulation, taken through the float32 Adam step, inside everything the GPU test asserts"""
    d, ref, e = P.case_data(case), P.reference(case), table[case.name]
    ch = P.checks(d, ref, P.as_device(d, e))
    print(case.name, "emulated iteration, err / allowed:", {k: float("%.3g" % ch[k]) for k in P.GROUPS})
    assert P.worst(ch)[0] <= 1.0, P.worst(ch)
    if ref["floor_state"][1] == "floor":
        assert e["scalars"][3] == float(P.FLOOR32)
    # the fp64 iteration itself is inside by construction
    assert P.worst(P.checks(d, ref, P.as_device(d, ref)))[0] <= 1e-6
    assert np.allclose(P.partial_sums(e["y"]).sum(0) + d["ret_block"][:2], e["block"][:2], rtol=1e-14, atol=0)


def _same(a, b):
    """two iterations leave the same of everything the checks read"""
    return all(np.array_equal(a["g"][n][k], b["g"][n][k]) for n in ("actor", "critic") for k in a["g"][n]) and \
        tuple(map(float, a["loss"])) == tuple(map(float, b["loss"])) and np.array_equal(a["y"], b["y"]) and \
        np.array_equal(a["block"], b["block"]) and tuple(a["scalars"]) == tuple(b["scalars"]) and \
        all(np.array_equal(a[n][k], b[n][k]) for n in ("critic", "target_critic") for k in ("W3", "b3"))


def _applies(case, m):
    return not ((m == "rows_16_31_twice" and case.B < 32) or (m == "bias_missing_tile" and case.B <= 16))


def _must_change(case, d, ref):
    """the mutants that cannot leave the case as it is"""
    mu_o, sg_o, mu_n, sg_n = ref["scalars"]
    out = {m for m in P.MUTANTS if _applies(case, m)}
    if sg_o == sg_n:                       # on the floor before and after
        out -= {"seed_sigma_old", "moments_rescaled"}
    if mu_o == 0.0:
        out -= {"mu_left_out_of_y"}
    if case.B % 16 == 0:
        out -= {"count_16_blocks", "padding_y_summed"}
    if not d["t"][d["idx"][0]].any():
        out -= {"terminal_ignored"}
    return out


_DIST = {}


def _mutant_distances(case):
    """{mutant: (largest err / allowed over the GPU test's checks, its group)} over the mutants that change the case; a mutant
    that does not is asserted to change NOTHING, and to be one that cannot"""
    if case.name not in _DIST:
        d, ref = P.case_data(case), P.reference(case)
        must, out = _must_change(case, d, ref), {}
        for m in P.MUTANTS:
            if not _applies(case, m):
                continue
            x = P.popart_step1(d, mut=m, sizes=False)
            if _same(x, ref):
                assert m not in must, (case.name, m)
                continue
            assert m in must, (case.name, m)
            out[m] = P.worst(P.checks(d, ref, P.as_device(d, x)))
        _DIST[case.name] = out
    return _DIST[case.name]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bounds_reject_every_mutant(case):
    """every mutant, stated on the fp64 algebra and taken through the fp64 Adam step, is at least MUTANT_MIN bounds outside one
    of the GPU test's checks wherever it changes the iteration at all; target_not_rescaled on the target bound"""
    dists = _mutant_distances(case)
    print("POPART_MUTANTS", case.name, {k: "%.3g %s" % v for k, v in dists.items()})
    for m, (v, group) in dists.items():
        assert v >= P.MUTANT_MIN, (case.name, m, v, group)
    if "target_not_rescaled" in dists:
        d, ref = P.case_data(case), P.reference(case)
        ch = P.checks(d, ref, P.as_device(d, P.popart_step1(d, mut="target_not_rescaled", sizes=False)))
        assert ch["target"] >= P.MUTANT_MIN and ch["where"]["target"] in ("critic.W3", "critic.b3")
        assert max(ch[k] for k in P.GROUPS if k != "target") <= 1e-6        # nothing else sees it


@pytest.mark.parametrize("case", [c for c in EMULATED if c.B <= 256], ids=lambda c: c.name)
def test_bounds_reject_every_mutant_of_the_emulation(table, case):
    """the same mutants applied to the float32 emulation: at least 2 bounds out wherever they change it"""
    d, ref, e = P.case_data(case), P.reference(case), table[case.name]
    for m in _mutant_distances(case):
        x = P.popart_step1(d, f32=True, mut=m)
        if _same(x, e):
            continue
        v, group = P.worst(P.checks(d, ref, P.as_device(d, x)))
        assert v >= 2.0, (case.name, m, v, group)


def test_every_mutant_is_caught_on_several_cases():
    caught = {m: sum(m in _mutant_distances(c) for c in CASES) for m in P.MUTANTS}
    for m in P.MUTANTS:
        v, name, group = min((_mutant_distances(c)[m][0], c.name, _mutant_distances(c)[m][1]) for c in CASES if m in _mutant_distances(c))
        print("POPART_NEAREST %-22s %10.3g bounds at %-22s (%s), caught at %d cases" % (m, v, name, group, caught[m]))
    assert all(n >= 3 for n in caught.values()), caught
