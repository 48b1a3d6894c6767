"""tests/forward_cases.py without a GPU: C_FWD recomputed, the reference held to the oracle, the dispatch restatement held to
the sources, every mutant out of the bound and every honest variant inside it."""
import os
import re

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import forward_cases as F

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smartstartcontinuous_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def r_cases():
    """r_case of every emulated case, printed; computed once"""
    out = {}
    for c in F.EMULATED:
        out[c.name] = F.case_ratio(c, F.emulate(c))
        print("r_case %-36s %-44s %.3f" % (c.name, c.kernel, out[c.name]))
    return out


def test_c_fwd_is_four_times_the_largest_r_case(r_cases):
    worst = max(r_cases, key=r_cases.get)
    c_fwd = np.ceil(4.0 * r_cases[worst] * 2.0) / 2.0
    print("largest r_case %.4f at %s -> C_FWD %.1f" % (r_cases[worst], worst, c_fwd))
    assert c_fwd == F.C_FWD
    assert F.RELU_BAND > F.C_FWD
    kinds = {(c.kind, c.ln, c.stats is not None) for c in F.EMULATED}
    for kind in ("actor", "critic", "stats", "eval", "cycle"):      # the constant rests on every family
        assert any(k[0] == kind for k in kinds)
    assert {(k[1], k[2]) for k in kinds} == {(False, False), (False, True), (True, False), (True, True)}


def test_no_emulated_element_needs_the_relu_band():
    """A under the plain fp64 relu mask (ddpg_cases' rule) is never larger than under the band; the emulation stays within
    C_FWD of the reference under it as well, at every element: the band decides nothing the constant rests on."""
    n_units = 0
    for c in F.EMULATED:
        banded, plain = F.reference_streams(c), F.streams(c, relu_band=None)
        emu = F.streams(c, f32=True)
        for k in banded:
            assert np.array_equal(banded[k][0], plain[k][0])
            assert np.all(plain[k][1] <= banded[k][1])
            n_units += int(np.sum(plain[k][1] < banded[k][1]))
            r = F.value_ratio(emu[k][0], *plain[k])
            assert r <= F.C_FWD, (c.name, k, r)
    print("elements whose A the band enlarges: %d" % n_units)


def test_reductions_of_the_emulation_are_inside_their_bounds():
    for c in F.EMULATED:
        ref, emu = F.reference_streams(c), F.streams(c, f32=True)
        for k, (o, A) in ref.items():
            e = emu[k][0].astype(np.float64)
            rm, rs = F.mean_ratio(e.mean(), o, A), F.std_ratio(e.std(), o, A)
            assert rm <= F.C_FWD and rs <= F.C_FWD, (c.name, k, rm, rs)
        if c.kind == "cycle":
            rd = F.distance_ratio(F.distance64(emu["pi"][0], emu["pp"][0]), ref["pi"][0], ref["pi"][1], ref["pp"][0], ref["pp"][1])
            print("distance %-28s %.3f" % (c.name, rd))
            assert rd <= F.C_FWD, (c.name, rd)


def test_reference_is_the_oracle():
    for c in F.CASES:
        d, ref = F.case_data(c), F.reference_streams(c)
        x = F.x_hat64(d["obs"], d["mean"], d["std"], c.clip)
        want = {}
        for k, w in (("pi", d["actor"]), ("pp", d["pert"])):
            if k in ref:
                want[k] = O.actor_forward(x, **F.oracle_kw(w), last_layer_tanh=c.llt)
        for k, a in (("q", d["act"]), ("qpi", want.get("pi"))):
            if k in ref:
                want[k] = O.critic_forward(x, a, **F.oracle_kw(d["critic"]), last_layer_tanh=c.llt)
        assert set(want) == set(ref)
        for k in ref:
            assert ref[k][0].shape == want[k].shape == ref[k][1].shape
            assert np.all(np.abs(ref[k][0] - want[k]) <= 1e-12 * np.maximum(1.0, np.abs(want[k]).max())), (c.name, k)
            assert np.all(np.isfinite(ref[k][1])) and np.all(ref[k][1] > 0), (c.name, k)


def test_the_restated_forward_is_net_fwd():
    """_fwd_alt, where the internal mutants and variants act, unchanged: the bits of ddpg_cases._net_fwd in both precisions"""
    for c in F.CASES:
        for f32 in (False, True):
            if f32 and not c.emulate:
                continue
            a, b = F.streams(c, f32=f32), F.streams(c, f32=f32, mut=F.RESTATED)
            for k in a:
                assert a[k][0].dtype == b[k][0].dtype and np.array_equal(a[k][0], b[k][0]), (c.name, k, f32)


def test_case_inputs_reach_the_edges():
    for c in F.CASES:
        d = F.case_data(c)
        assert d["obs"].shape == (c.m, c.obs) and d["obs"].dtype == np.float32
        if c.kind == "eval":
            continue
        x = F.x_hat64(d["obs"], d["mean"], d["std"], clip=False)
        assert np.abs(x[0]).max() > F.OBS_CLIP                          # row 0 lies beyond the clip
        if c.m >= 4:
            assert abs(abs(x[1, 0]) - F.OBS_CLIP) <= 1e-6 and abs(abs(x[1, -1]) - F.OBS_CLIP) <= 1e-6
            assert not d["obs"][2].any() and np.signbit(d["obs"][2, 0])
            assert x[3].min() < -F.OBS_CLIP
        if c.m == 257:
            assert np.abs(x[256]).max() > F.OBS_CLIP


def test_launched_against_the_sources():
    # every kernel name is a __global__ of its file, and every instantiation is claimed by a case
    names = {f: F.kernel_names_in_source(_src(f)) for f in set(F.KERNEL_SOURCE.values())}
    for k in F.ALL_KERNELS:
        base = k.split("<")[0]
        assert base in names[F.KERNEL_SOURCE[base]], k
    claimed = {c.kernel for c in F.CASES}
    assert claimed == set(F.ALL_KERNELS), set(F.ALL_KERNELS) ^ claimed
    for c in F.CASES:
        h = c.ah if c.ah is not None else c.ch
        assert c.kernel == F.launched(c.kind, c.obs, h[0], h[1], c.act, c.ln, c.m, c.stats is not None, critic=c.ch) != F.REFUSED
        assert 1 <= c.obs <= F.SSC_MAX_STATE and 1 <= c.act <= F.SSC_MAX_ACT
    for kind, od, h1, h2, ad, ln, m in F.REFUSED_CASES:
        assert F.launched(kind, od, h1, h2, ad, ln, m, False) == F.REFUSED
        assert F.launched(kind, od, h1, h2 - 1, ad, ln, m, False) != F.REFUSED     # one unit less is exactly 160 KB
        lds = F.actor_lds(h1, h2 - 1, ln) if kind == "actor" else F.critic_lds(h1, h2 - 1, ad, ln)
        assert lds == F.LDS_MAX
    assert F.launched("actor", 8, 513, 8, 1, False, 1, False) == F.REFUSED
    # every family with LayerNorm and without, with statistics and without
    for base in set(F.KERNEL_SOURCE) - {"actor_f32_kernel"}:
        seen = {(c.ln, c.stats is not None) for c in F.CASES if c.kernel.split("<")[0] == base}
        assert seen == {(False, False), (False, True), (True, False), (True, True)}, (base, seen)
    # the thresholds restated in Python are the literals of the launchers
    actor, critic = _src("actor.hip"), _src("smartstart.hip")
    assert "if (a->h1 > %d) return set_error(SSC_EUNSUPPORTED" % F.ACTOR_MAX_H1 in actor
    assert "if (m <= %d && a->h2 <= %d) {" % (F.ROW_MAX_M, F.ROW_MAX_H2) in actor
    assert "a->act_dim == 1 && a->h1 == 64 && a->h2 == 32 && (a->obs_dim == 2 || a->obs_dim == 3)" in actor
    assert "const size_t lds = (size_t)(a->h1 + (ln ? a->h2 : 0)) * 64 * sizeof(float);" in actor
    assert "const size_t lds = (size_t)(c->h1 + c->act_dim + (ln ? c->h2 : 0)) * 64 * sizeof(float);" in critic
    assert "c->h1 + c->act_dim <= %d" % F.CRITIC_MAX_IN2 in critic
    for src in (actor, critic):
        assert "if (lds > %d * 1024) return set_error(SSC_EUNSUPPORTED" % (F.LDS_MAX // 1024) in src
        assert "if (lds > %d * 1024) {" % (F.LDS_DEFAULT // 1024) in src
    assert F.LANE_BYTES == 64 * 4
    # the evaluation kernel's staging rule: the carve and the fit restated from ddpg_eval.hip
    ev, rows = _src("ddpg_eval.hip"), _src("ddpg_rows.h")
    assert "constexpr int kSR = %d;" % F.K_SR in rows and "constexpr int kEStreams = 3;" in ev and "constexpr int kEPart = 3 * kEStreams + 1;" in ev
    assert F.K_EPART == 3 * 3 + 1
    assert "constexpr size_t kLdsBytes = %d * 1024;" % (F.LDS_MAX // 1024) in ev
    assert "bool weights_fit(const EvalCarve &c) { return (size_t)(c.act_floats + c.weight_floats) * sizeof(float) <= kLdsBytes; }" in ev
    assert "const bool wlds = weights_fit(carve) && !global_weights_forced();" in ev
    for line in ("c.off_RED = (int32_t)q; q += (int64_t)kSR * kEPart * 2;", "c.off_XA = (int32_t)q;  q += (int64_t)od * kSR;",
                 "c.off_XC = (int32_t)q;  q += (int64_t)od * kSR;", "c.off_H1 = (int32_t)q;  q += (ah1 > (int64_t)ch1 + 1 ? ah1 : (int64_t)ch1 + 1) * kSR;",
                 "c.off_H2 = (int32_t)q;  q += (int64_t)(ah2 > ch2 ? ah2 : ch2) * kSR;", "c.off_PI = (int32_t)q;  q += kSR;", "c.off_Q = (int32_t)q;   q += kSR;",
                 "const int64_t wa = net_floats(od, 0, ah1, ah2, 1, aln), wc = net_floats(od, 1, ch1, ch2, 1, cln);",
                 "return (int64_t)in_dim * h1 + h1 + ((int64_t)h1 + n_extra) * h2 + h2 + (int64_t)h2 * out_dim + out_dim + (ln ? 2 * ((int64_t)h1 + h2) : 0);"):
        assert line in ev, line
    assert F.eval_weights_fit(2, (128, 64), (128, 64), False) and not F.eval_weights_fit(2, (200, 100), (200, 100), False)
    fit = {c.name: F.eval_weights_fit(c.obs, c.ah, c.ch, c.ln) for c in F.CASES if c.kind == "eval"}
    assert set(fit.values()) == {True, False}          # both answers of the rule are in the table
    for c in F.CASES:
        if c.kind == "eval":
            assert c.kernel == F.EVAL % ("true" if fit[c.name] else "false")
            assert F.launched("eval", c.obs, *c.ah, 1, c.ln, c.m, False, global_weights=True, critic=c.ch) == F.EVAL % "false"
    # the raised-LDS launches are in the table
    assert any(c.kernel.startswith("actor_generic") and not c.ln and F.actor_lds(*c.ah, False) == 128 * 1024 for c in F.CASES)
    assert any(c.kernel.startswith("critic") and F.critic_lds(*c.ch, c.act, c.ln) > F.LDS_DEFAULT for c in F.CASES)
    header = _src(os.path.join("..", "..", "include", "ssc.h"))
    assert re.search(r"#define\s+SSC_MAX_STATE\s+%d\b" % F.SSC_MAX_STATE, header)
    assert re.search(r"#define\s+SSC_MAX_ACT\s+%d\b" % F.SSC_MAX_ACT, header)


def _mutant_table(mut):
    """per case where the mutant changes anything: (bounds out in the fp64 algebra, bounds out in the emulation or None)"""
    rows = {}
    for c in F.CASES:
        ref = F.reference_streams(c)
        got = {k: v[0] for k, v in F.streams(c, mut=mut).items()}
        if all(np.array_equal(got[k], ref[k][0]) for k in ref):
            continue
        r64 = F.case_ratio(c, got) / F.C_FWD
        r32 = F.case_ratio(c, {k: v[0] for k, v in F.streams(c, f32=True, mut=mut).items()}) / F.C_FWD if c.emulate else None
        rows[c.name] = (r64, r32)
    return rows


# (mutant, case) pairs that stay inside MUTANT_MIN bounds, with the reason; NOTEBOOK has the ratios
NEARLY_INVISIBLE = {}


@pytest.mark.parametrize("mut", F.MUTANTS)
def test_mutant_is_out_of_the_bound(mut):
    rows = _mutant_table(mut)
    assert rows, "the mutant changes nothing anywhere"
    nearest = min(rows, key=lambda k: min(v for v in rows[k] if v is not None))
    print("mutant %-22s changes %2d cases; nearest %-36s %.2f bounds (fp64) %s (emulation)"
          % (mut, len(rows), nearest, rows[nearest][0], "-" if rows[nearest][1] is None else "%.2f" % rows[nearest][1]))
    inside = {k: v for k, v in rows.items() if min(x for x in v if x is not None) < F.MUTANT_MIN and (mut, k) not in NEARLY_INVISIBLE}
    assert not inside, inside


def test_output_chain_from_the_bias_is_outside_the_bound():
    """Why critic_kernel and net_rows add b3 behind a chain that starts from zero: the kernels' chains with the critic's
    output layer started from b3 as well (F.BIAS_FIRST) leave the bound at a b3 = 20 head, where every partial sum of the
    chain rounds at the size of b3; with b3 last (``fma_kernels``) the same cases are inside.  The chain may not go back."""
    out = {}
    for c in F.EMULATED:
        if c.ch is None:
            continue
        first = F.case_ratio(c, {k: v[0] for k, v in F.streams(c, f32=True, mut=F.BIAS_FIRST).items()})
        last = F.case_ratio(c, {k: v[0] for k, v in F.streams(c, f32=True, mut="fma_kernels").items()})
        assert last <= F.C_FWD, (c.name, last)
        if first > F.C_FWD:
            out[c.name] = (first, last)
    print("bias-first output chain outside C_FWD %.1f: %s" % (F.C_FWD, {k: "%.3f (b3 last: %.3f)" % v for k, v in out.items()}))
    assert out and all(F.CASE_BY_NAME[k].head == "big" for k in out)


@pytest.mark.parametrize("var", F.VARIANTS)
def test_honest_variant_is_inside_the_bound(var):
    worst, changed = 0.0, 0
    for c in F.EMULATED:
        got = {k: v[0] for k, v in F.streams(c, f32=True, mut=var).items()}
        plain = F.streams(c, f32=True)
        changed += any(not np.array_equal(got[k], plain[k][0]) for k in got)
        r = F.case_ratio(c, got)
        worst = max(worst, r)
        assert r <= F.C_FWD, (var, c.name, r)
    print("variant %-16s changes %2d cases; largest ratio %.3f of C_FWD %.1f" % (var, changed, worst, F.C_FWD))
    assert changed
