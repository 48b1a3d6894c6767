"""The MPC scorer's case table (tests/mpc_cases.py) held to its own premises, without the kernel: the redraw share, the
decision-margin threshold, the window edges, the constant of the bound and the emulation mutants that bound must reject.

Recorded with this table: max r_case = 1.03 (s16_d3_p5), C_SCORE = 4.2; redraw share 0 .. 0.6 % (tp_d2_str); nearest
mutant: sums_drop_ragged at tp_unstaged, 1.76 bounds away (one sample of 15 873 left out of the two global sums), every
other mutant x case >= 15 bounds."""
import numpy as np
import pytest

from tests import mpc_cases as M
from oracle import ssc_oracle as O


@pytest.fixture(scope="module")
def table():
    """per case: the fp64 walk and the float32 emulation of every problem, computed once"""
    out = {}
    for c in M.CASES:
        probs = M.case_data(c)["problems"]
        out[c.name] = [(q, M.walk64_of(c, q), M.emu32_of(c, q)) for q in probs]
    return out


def test_table_reaches_every_instantiation_and_fork():
    kernels = {c.kernel for c in M.CASES}
    assert {"small<%d,%d>" % (g, d) for g in (16, 32, 64) for d in (0, 1, 2, 3)} <= kernels
    assert {(c.kernel, c.walk) for c in M.CASES if c.N > 64} >= {("pass_a<%d>+pass_b<%d>" % (d, d), w) for d in (0, 1, 2, 3)
                                                                 for w in ("pre", "str")}
    assert {c.d for c in M.CASES if c.N > 64 and c.d > 3 and c.walk == "str"} >= {5, 8}
    assert {c.staging for c in M.CASES if c.N > 64} == {"one_trip", "trips", "unstaged"}
    by = M.CASE_BY_NAME
    assert ((by["tp_npart256"].N + 255) // 256) * (by["tp_npart256"].H + 1) * 2 == 256
    edges = {(W, cur) for c in M.CASES for (W, cur) in c.plans}
    assert any(cur == 0 for W, cur in edges) and any(cur == W - 2 and W > 2 for W, cur in edges)
    assert any(cur == W - 1 and W > 2 for W, cur in edges) and {(2, 0), (2, 1), (6000, 3000)} <= edges
    assert {c.per_row for c in M.CASES} == {False, True} and {1.0, 0.3} <= {c.gamma for c in M.CASES}
    assert 0.0 in {c.hpf for c in M.CASES} and len({c.theta for c in M.CASES}) >= 3
    assert {c.walk for c in M.CASES if c.along} == {"pre", "str"}
    assert {(c.N > 64, c.walk) for c in M.CASES if c.along} == {(False, "pre"), (False, "str"), (True, "pre"), (True, "str")}


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_case_premises(table, case):
    redrawn, dmax = 0, 0.0
    for p, (q, wk, _) in enumerate(table[case.name]):
        ref = O.mpc_scores_add_delta(q["S"], q["wp"], q["left"], q["radii"], q["cur"], case.theta, case.gamma, case.hpf, case.per_row)
        # the walk that carries the margins and A_n IS the oracle's walk
        assert np.array_equal(ref[3], wk["final_idx"]) and np.allclose(ref[0], wk["scores"], rtol=1e-13, atol=1e-13)
        assert np.isfinite(wk["scores"]).all() and wk["margin"].min() >= M.THR
        redrawn += q["redrawn"]
        dmax = max(dmax, wk["dmax"])
        if p in case.along:      # a sample whose waypoint index advances on every horizon step: the window's far edge
            assert (wk["final_idx"] - q["cur"] == case.H + 1).any(), p
    assert redrawn <= 0.02 * case.P * case.N
    assert M.THR >= 64 * (case.d + 3) * M.EPS32 * dmax


def test_bound_constant_covers_the_table(table):
    r = {name: max(float(np.max(np.abs(e - wk["scores"]) / (M.EPS32 * wk["A"]))) for _, wk, e in rows) for name, rows in table.items()}
    print("r_case:", {k: round(v, 2) for k, v in r.items()})
    assert 4 * max(r.values()) <= M.C_SCORE
    assert M.C_SCORE <= 4 * max(r.values()) * 1.05          # and is not kept wider than the table needs


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_bound_rejects_every_mutant(table, case):
    """a mutant that changes any score of a case puts at least one sample of that case outside the bound"""
    dists = {}
    for m in M.MUTANTS:
        worst = None
        for q, wk, e in table[case.name]:
            x = M.emu32_of(case, q, m)
            if np.array_equal(x, e, equal_nan=True):
                continue
            with np.errstate(invalid="ignore"):
                dd = np.abs(x - wk["scores"]) / (M.C_SCORE * M.EPS32 * wk["A"])
            worst = max(worst or 0.0, float(np.where(np.isnan(dd), np.inf, dd).max()))
        dists[m] = worst
    print(case.name, "mutant distance / bound:", dists)
    for m, v in dists.items():
        assert v is None or v > 1.0, (m, v)
    assert sum(v is not None for v in dists.values()) >= 3      # no case is blind to most of the list
