"""The step-kernel case table (tests/step_cases.py) held to its own premises, without the kernel: the class census and the
option coverage of every case, the decision margins, the checker accepting the float32 model of the kernel on every case,
and the checker rejecting every mutant of that model on at least one case of every (env, form) the mutant applies to."""
import numpy as np
import pytest

from tests import step_cases as S


def _run_model(case, mutant=None, report=None):
    """three model launches through check_step; raises AssertionError where the checker refuses one"""
    dev = S.initial_device_state(case)
    for j in range(S.LAUNCHES):
        if j:
            S.apply_inputs(case, j, dev)
        after = S.model_step(case, dev, mutant)
        S.check_step(case, S.model_got(case, dev, after), S.expected_step(case, j), report)
        dev = after


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_census_margins_and_model(case):
    d = S.case_data(case)
    line = S.census_line(case)
    print(line)
    c = S.census(case)
    need = S.required_classes(case)
    if case.n >= 64:
        assert all(c.get(k, 0) >= 4 for k in need), {k: c.get(k, 0) for k in need}
    if case.n >= 255 and case.form != "mpc":                        # the done classes crossed with the new-episode outcomes
        cross = [dc + "*" + oc for dc in S.DONE_CLASSES[case.env] for oc in S.OUTCOMES if oc in need]
        assert all(c.get(k, 0) >= 1 for k in cross), {k: c.get(k, 0) for k in cross}
    if case.n == 600:
        i = np.arange(d["n_alloc"])
        for blk in (i < S.BLOCK, i >= 2 * S.BLOCK):
            cb = S.census(case, envs=blk)
            assert all(cb.get(k, 0) >= 1 for k in need), {k: cb.get(k, 0) for k in need}
    # the labels are what the oracle's step does, launch by launch
    for j in range(S.LAUNCHES):
        st, e = d["steps"][j], S.expected_step(case, j)
        inp = st["inp"]
        assert e["margin"][d["live"]].min() >= S.MARGIN
        for i in np.nonzero(d["live"])[0]:
            a, dn = st["act_cls"][i], st["done_cls"][i]
            assert e["done"][i] == (dn != "none") and e["goal"][i] == (dn in ("goal", "both"))
            assert (inp["steps"][i] == S.MAX_STEPS - 1) == (dn in ("tl", "both"))
            if a in S.NAV:
                assert e["navigating_in"][i]
                assert e["at_goal"][i] == (a in ("near", "final") or (a == "clamped" and inp["actions_done"][i] == S.FINAL_STEPS - 1))
                if not e["done"][i]:
                    moved = a in ("adv_dc", "adv_dn", "give_up")
                    want = inp["cur_idx"][i] + 1 if moved else min(inp["cur_idx"][i], S.W_PLAN - 1)
                    assert e["cur_idx"][i] == want and e["actions_done"][i] == (0 if moved else inp["actions_done"][i] + 1)
            else:
                assert not e["navigating_in"][i] and case.form != "mpc"
                lo, hi = S.BOUNDS[case.env]
                sat = {"sat_lo": lo, "sat_hi": hi, "sat2_lo": lo, "sat2_hi": hi}
                if a in sat:
                    assert e["act"][i] == sat[a]
                else:
                    assert lo * 0.96 < e["act"][i] < hi * 0.96
        if case.form == "mpc":
            assert (inp["start_idx"][d["live"]] != 0).all()
    assert min(float(np.nanmin(d["radii"][np.isfinite(d["radii"])])), 1.0) >= np.float32(S.MIN_RADIUS)
    assert S.PROBLEM_ID0 != d["env_id0"] and S.NOISE_SEED != S.ENV_SEED
    rep = {}
    _run_model(case, None, rep)
    assert rep and max(rep.values()) <= 1.0


def test_options_reach_every_env_and_form():
    for env in S.ENVS:
        for form in S.FORMS:
            cs = [c for c in S.CASES if (c.env, c.form) == (env, form)]
            o = lambda k: {c.opts[k] for c in cs}
            assert o("log") == {"none", "packed", "strided"} and o("ring") == {"none", "full", "small"}
            assert o("at_goal") == {True, False} and o("stats") == {True, False} and o("noise") == {0.0, 0.005}
            assert {c.opts["k0"] for c in cs if c.opts["log"] != "none"} == {0, 2}
            assert (1 << 32) + 3 in o("t0") and {(t + j) % 4 for t in o("t0") for j in range(S.LAUNCHES)} == {0, 1, 2, 3}
            if form != "mpc":
                assert o("mode_log") == {True, False}
                pairs = [p for c in cs for p in S.pairs_of(c)]
                assert any(p["count"] == 0 for p in pairs) and any(p["eps"] > 0 for p in pairs)
                assert any(p["eps"] < 0 for p in pairs) and any(p["eps"] == 0 for p in pairs)
                assert any(p["first"] + p["count"] > p["slots"] and p["first"] > 0 for p in pairs)
            if form == "ss":
                assert o("n_live") == {True, False}
                assert {c.n for c in cs} == set(S.SIZES)
            if form == "mpc":
                assert o("ou_col") == {True, False} and {c.n for c in cs} == set(S.SIZES)
            if form == "many":
                for c in cs:
                    p = S.pairs_of(c)
                    assert [q["n_envs"] for q in p] == [1, 300, 70, 256] and p[0]["env0"] == 3
                    assert p[2]["env0"] - (p[1]["env0"] + p[1]["n_envs"]) == 5
                    assert [q["eta"] for q in p] == [0.0, 0.4, 1.0, 1.0] and [q["eps"] for q in p] == [0.8, -0.3, 0.8, 0.0]
                    w = [(q["slot0"], q["slot0"] + q["slots"]) for q in p]
                    assert all(a[1] <= b[0] for a, b in zip(w, w[1:]))
            # a small ring is smaller than the number of finishing envs
            for c in cs:
                if c.opts["ring"] == "small":
                    assert sum(int(S.expected_step(c, j)["done"].sum()) for j in range(S.LAUNCHES)) > S.ring_capacity(c)
            assert any(S.n_blocks(c) > 1 for c in cs)
        assert {c.opts["v1"] for c in S.CASES if c.env == "pend"} == {True, False}


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_checker_rejects_the_mutant(mutant):
    """on at least one case of every (env, form) the mutant applies to (smallest cases first)"""
    caught = {}
    for env in S.ENVS:
        for form in S.FORMS:
            if not S.mutant_applies(mutant, env, form):
                continue
            for case in sorted((c for c in S.CASES if (c.env, c.form) == (env, form) and c.n >= 64), key=lambda c: c.n):
                try:
                    _run_model(case, mutant)
                except AssertionError as e:
                    caught[env, form] = (case.name, str(e.args[0])[:60] if e.args else "")
                    break
            else:
                caught[env, form] = None
    print("MUTANT %s rejected at: %s" % (mutant, {"%s/%s" % k: v for k, v in caught.items()}))
    assert caught and all(v is not None for v in caught.values()), caught
