"""The selection kernels' case tables (tests/select_cases.py) held to their own premises, without the kernels: the shapes and
query classes the tables claim, the fp64 restatement that carries the error scale against the oracle (and the oracle
against scipy), the two constants, and the emulation mutants the KDE bound must reject.

Recorded with these tables: KDE max r_case = 0.646 (k2_n1025_m77), C_KDE = 2.6; UCB max r_case = 0.884 (u257), C_UCB = 3.6.
Every mutant is rejected: its largest distance over the cases is 3.0e5 bounds at the least (skip_last_wave, at
k0_d8_n4097_m77), inf for qi_le_m (a slot past m written) and 5e44 for dead_lanes_one.  Nearest mutant x case that differs from the
emulation at all: wh_transposed at k2_n4096_m9, 0.11 bounds (isotropic data 1000 sigma from the origin: the whitening is
diagonal to 2 %, its transpose moves the pdf by less than the cancellation the scale allows there), then wh_transposed
at k3_n5121_m7, 0.41 (isotropic again); every other mutant x case that differs is >= 8.6 bounds away (wh_transposed,
k0_d5_n9217_m7)."""
import numpy as np
import pytest

from tests import select_cases as S
from oracle import ssc_oracle as O


@pytest.fixture(scope="module")
def table():
    """per KDE case: (inputs, reference with scale and bound, float32 emulation), computed once"""
    return {c.name: (S.kde_case_data(c), S.kde_reference(c), S.kde_emu32_of(c)) for c in S.KDE_CASES}


def test_tables_cover_what_they_claim(table):
    assert 18 <= len(S.KDE_CASES) <= 24 and max(c.n for c in S.KDE_CASES) <= 9300 and max(c.m for c in S.KDE_CASES) <= 77
    assert {c.n for c in S.KDE_CASES} == {1, 5, 63, 1023, 1024, 1025, 4095, 4096, 4097, 5121, 9217}
    assert {c.m for c in S.KDE_CASES} == {1, 7, 8, 9, 77}
    assert {c.d for c in S.KDE_CASES} == {1, 2, 3, 4, 5, 8}
    assert {c.kernel for c in S.KDE_CASES} == {"kde_kernel<%d>" % k for k in (0, 1, 2, 3)}
    assert all(c.kernel == "kde_kernel<%d>" % (c.d if c.d <= 3 else 0) for c in S.KDE_CASES)      # ssc_kde_evaluate's dispatch
    assert {c.data for c in S.KDE_CASES} == {"iso", "scaled", "corr", "mcar", "pend", "off30", "off1000"}
    assert all(c.d == 3 for c in S.KDE_CASES if c.data == "pend") and all(c.d == 2 for c in S.KDE_CASES if c.data == "mcar")
    # the shapes of the data loop: 5121 = one trip + a full first slot + one point, 9217 = two trips + that
    assert S.TRIP == 4096 and 5121 == S.TRIP + S.K_THREADS + 1 and 9217 == 2 * S.TRIP + S.K_THREADS + 1
    for k in (0, 1, 2, 3):      # every instantiation: a ragged last trip, a ragged last query group, every query class
        rows = [c for c in S.KDE_CASES if c.kernel == "kde_kernel<%d>" % k]
        assert any(c.n % S.TRIP for c in rows) and any(c.m % S.K_Q for c in rows) and any(c.n > S.TRIP for c in rows)
        assert set(S.MIX) <= {q for c in rows for q in table[c.name][0]["cls"]}
    wh = table["k2_n1023_m9"][0]["wh"]       # rho = 0.999: upper triangular, far from symmetric
    assert wh[1, 0] == 0.0 and abs(wh[0, 1]) > 0.9 * abs(wh[0, 0]) and abs(wh[0, 0]) > 10 * abs(wh[1, 1])
    assert {c.m for c in S.UCB_CASES} == {1, 63, 64, 65, 255, 256, 257, 1000, 4096}
    for c in S.UCB_CASES:
        labels = {p[0] for p in S.ucb_placements(c)}
        waves = {"wave%d" % w for w in range(4) if 64 * w + 5 < c.m} | {"wave0"}
        assert waves | {"base", "inf1", "allnan"} <= labels
        assert c.m == 1 or {"dup", "inf2", "nan"} <= labels
        assert c.m <= 256 or any(l.startswith("late") for l in labels)
        assert np.float32(c.alpha) == c.alpha and np.float32(c.beta) == c.beta
    wave = lambda r: r % 256 // 64
    for m, dup in S.UCB_DUP_ROWS.items():
        if dup is None:
            continue
        star, copies = dup
        assert all(0 <= r < m for r in (star, *copies)) and min(copies) < star < max(copies) and len({star, *copies}) == 1 + len(copies)
        # a lower and a higher copy in another wave than the row they copy; two copies in one wave; two in one thread
        assert m < 129 or (wave(min(copies)) != wave(star) and wave(max(copies)) != wave(star))
        assert any(wave(a) == wave(b) and a // 256 == b // 256 for a in copies for b in copies if a < b) or m < 129
        assert m <= 256 or any(a % 256 == b % 256 for a in copies for b in copies if a < b)


@pytest.mark.parametrize("case", S.KDE_CASES, ids=lambda c: c.name)
def test_kde_case_premises(table, case):
    cd, r, _ = table[case.name]
    # the restatement that carries A_i IS the oracle, on the float32 inputs the kernel receives
    ref = O.kde_evaluate(cd["data"], cd["points"], cd["wh"].astype(np.float64), cd["norm"])
    assert np.allclose(ref, r["ref"], rtol=1e-10, atol=1e-300)
    if cd["own_bandwidth"]:
        _, wh, norm = O.kde_scott(cd["data"])
        assert np.array_equal(cd["wh"], wh.astype(np.float32)) and cd["norm"] == norm
    assert r["band_free"].all()
    flushed = r["flushed"]
    assert np.array_equal(flushed, np.array([c == "far" or cd["cls"][cd["dup_of"].get(i, i)] == "far" for i, c in enumerate(cd["cls"])]))
    assert flushed.mean() <= 0.25
    assert (r["ref"][flushed] > 0).all() and (r["ref"][flushed] < cd["norm"] * case.n * 2.0 ** -150).all()
    for i, src in cd["dup_of"].items():
        assert np.array_equal(cd["points"][i], cd["points"][src]) and i != src
    assert np.isfinite(r["A"]).all() and (r["A"] > 0).all()


def test_every_query_class_is_present(table):
    far = 0
    for k in (0, 1, 2, 3):
        low = 0
        for c in (c for c in S.KDE_CASES if c.kernel == "kde_kernel<%d>" % k):
            _, r, _ = table[c.name]
            live = ~r["flushed"]
            low += int((r["ref"][live] < 1e-3 * r["ref"].max()).sum())
            far += int(r["flushed"].sum())
        assert low >= 1, k
    assert far >= 1
    # between the data: a midpoint query's largest term is below the self-term 1 of a copy
    cd, r, _ = table["k2_n5_m8"]
    assert all(r["wmax"][i] == 1.0 for i, c in enumerate(cd["cls"]) if c == "copy")
    assert all(r["wmax"][i] < 1.0 for i, c in enumerate(cd["cls"]) if c in ("mid", "out1", "out2", "out3"))


def test_kde_constant_covers_the_table(table):
    r = {name: float(np.max(np.abs(e[:len(ref["ref"])].astype(np.float64) - ref["ref"]) / (S.EPS32 * ref["A"])))
         for name, (_, ref, e) in table.items()}
    print("KDE r_case:", {k: round(v, 3) for k, v in r.items()})
    assert 4 * max(r.values()) <= S.C_KDE
    assert S.C_KDE <= 4 * max(r.values()) * 1.05          # and is not kept wider than the table needs
    for name, (_, ref, e) in table.items():               # the emulation flushes what the kernel flushes
        assert (e[:len(ref["ref"])][ref["flushed"]] == 0.0).all() and np.isnan(e[len(ref["ref"]):]).all(), name


def test_ucb_constant_covers_the_table():
    r = {}
    for c in S.UCB_CASES:
        worst = 0.0
        for label, v, p, best in S.ucb_placements(c):
            ref, A = S.ucb_scale(v, p, c)
            with np.errstate(divide="ignore", invalid="ignore"):
                o_ref, o_best = O.smart_start_ucb(v, p, c.buffer_len, c.volume, c.alpha, c.beta)
            assert np.array_equal(ref, o_ref, equal_nan=True)
            emu = S.ucb_emu32(v, p, c)
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(emu), np.isnan(ref)) and np.array_equal(np.isposinf(emu), np.isposinf(ref) & ~np.isnan(ref))
            assert np.array_equal(np.isposinf(ref), np.asarray(p) == 0.0)
            if fin.any():
                worst = max(worst, float(np.max(np.abs(emu[fin] - ref[fin]) / (S.EPS32 * A[fin]))))
            if best is not None and label != "allnan":     # the placed winner is the oracle's, by far more than the bound
                assert o_best == best, (c.name, label)
                others = np.delete(ref, [i for i in range(c.m) if ref[i] == ref[best]])
                others = others[~np.isnan(others)]
                assert others.size == 0 or np.isposinf(ref[best]) or ref[best] - others.max() > 0.5
        r[c.name] = worst
    print("UCB r_case:", {k: round(v, 3) for k, v in r.items()})
    assert 4 * max(r.values()) <= S.C_UCB
    assert S.C_UCB <= 4 * max(r.values()) * 1.05


def test_bound_rejects_every_mutant(table):
    """every mutant is more than one bound from the reference on at least one case (a case whose output a mutant leaves
    as the emulation's is not counted: n = 4096 has no ragged tail)"""
    far = {m: 0.0 for m in S.KDE_MUTANTS}
    nearest = (np.inf, None, None)
    for c in S.KDE_CASES:
        _, ref, e = table[c.name]
        dists = {}
        for m in S.KDE_MUTANTS:
            x = S.kde_emu32_of(c, m)
            if np.array_equal(x, e, equal_nan=True):
                dists[m] = None
                continue
            dists[m] = S.kde_distance(x, ref["ref"], ref["bound"])
            far[m] = max(far[m], dists[m])
            nearest = min(nearest, (dists[m], m, c.name))
        print(c.name, "mutant distance / bound:", {k: (v if v is None else float("%.3g" % v)) for k, v in dists.items()})
        assert S.kde_distance(e, ref["ref"], ref["bound"]) <= 0.25 * 1.0001       # the emulation itself: r_case / C_KDE
    print("largest distance per mutant:", {k: float("%.3g" % v) for k, v in far.items()}, "nearest differing:", nearest)
    for m, v in far.items():
        assert v > 1.0, (m, v)


def test_oracle_kde_matches_scipy_on_table_rows(table):
    try:
        import scipy.stats
    except ImportError:
        pytest.skip("scipy is not installed: oracle.kde_evaluate stays pinned by tests/test_oracle_networks.py only")
    for name in ("k1_n63_m7", "k3_n63_m9", "k2_n1023_m9"):
        cd = table[name][0]
        data, pts = cd["data"].astype(np.float64), cd["points"].astype(np.float64)
        cov, wh, norm = O.kde_scott(data)
        k = scipy.stats.gaussian_kde(data.T, bw_method="scott")
        assert np.allclose(np.atleast_2d(cov), k.covariance, rtol=1e-12)
        assert np.allclose(O.kde_evaluate(data, pts, wh, norm), k(pts.T), rtol=1e-9, atol=1e-300), name
