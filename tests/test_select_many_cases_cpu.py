"""tests/select_many_cases.py on the CPU: the numpy restatement of the device's d x d algebra against numpy.linalg, the
top-k rule, the validity predicate and its mutants, and the case table's own claims."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import select_cases as S
from tests import select_many_cases as M

SCOTT_CASES = [c for c in S.KDE_CASES if c.n >= c.d + 2]


def _cpu_order_spread(data):
    """tests/test_gpu_select_matrix.py's measure: O.kde_scott against the two-pass form summed in reverse row order"""
    x = np.asarray(data, np.float64)[::-1]
    n, d = x.shape
    xc = x - np.cumsum(x, axis=0)[-1] / n
    cov = np.cumsum(xc[:, :, None] * xc[:, None, :], axis=0)[-1] / (n - 1) * (n ** (-1.0 / (d + 4))) ** 2
    wh = np.linalg.cholesky(np.linalg.inv(cov)).T
    norm = 1.0 / (n * np.sqrt(np.linalg.det(2 * np.pi * cov)))
    _, wh_ref, norm_ref = O.kde_scott(data)
    return float(np.abs(wh - wh_ref).max()), float(abs(norm / norm_ref - 1.0))


@pytest.mark.parametrize("source", ["numpy_cov", "device_order_cov"])
@pytest.mark.parametrize("case", SCOTT_CASES, ids=lambda c: c.name)
def test_explicit_algebra_against_numpy_linalg(case, source):
    """the explicit loops on numpy's own covariance (the algebra alone), and on the covariance summed in the device's order
    (what the kernel computes, up to its fused multiply-adds)"""
    data = S.kde_case_data(case)["data"]
    cov_ref, wh_ref, norm_ref = O.kde_scott(data)
    wh, norm = M.scott_algebra(cov_ref if source == "numpy_cov" else M.scott_covariance(data), case.n)
    wh_spread, norm_spread = _cpu_order_spread(data)
    want = wh_ref.astype(np.float32)
    tol = np.maximum(np.spacing(np.abs(want)).astype(np.float64), wh_spread)
    assert wh.dtype == np.float32 and np.all(np.abs(wh.astype(np.float64) - want.astype(np.float64)) <= tol)
    assert np.all(wh[np.tril_indices(case.d, -1)] == 0.0)
    assert abs(norm / norm_ref - 1.0) <= max(1e-12, 4.0 * norm_spread)


def test_algebra_refuses_what_numpy_refuses():
    with pytest.raises(M.NoFactor):
        M.scott_algebra(np.zeros((2, 2)), 5)                          # an all-equal data set
    with pytest.raises(M.NoFactor):
        M.scott_algebra(np.array([[1.0, 2.0], [2.0, 1.0]]), 5)        # indefinite
    with pytest.raises(M.NoFactor):
        M.scott_algebra(np.array([[np.nan]]), 5)
    with pytest.raises(M.NoFactor):
        M.scott_algebra(np.array([[np.inf]]), 5)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(np.linalg.inv(np.zeros((2, 2))))


def test_topk_rule():
    nan, inf = np.float32("nan"), np.float32("inf")
    idx = np.array([10, 11, -1, 13, 14, 15, 16], np.int32)
    ucb = np.array([1.0, 3.0, 99.0, 3.0, nan, -inf, inf], np.float32)
    assert M.topk_rule(ucb, idx, 1).tolist() == [16]                                   # +inf first; the masked 99 never
    assert M.topk_rule(ucb, idx, 3).tolist() == [16, 11, 13]                           # the tie: lowest slot first
    assert M.topk_rule(ucb, idx, 7).tolist() == [16, 11, 13, 10, 15, 14, -1]           # NaN below -inf, then -1
    assert M.topk_rule(np.full(3, nan, np.float32), np.array([-1, 7, 8]), 1).tolist() == [7]   # all NaN: the first live slot
    assert M.topk_rule(np.array([-0.0, 0.0], np.float32), np.array([4, 5]), 2).tolist() == [4, 5]   # -0 = +0
    assert M.topk_rule(np.zeros(3, np.float32), np.array([-1, -1, -1]), 2).tolist() == [-1, -1]


def test_validity_predicate_and_its_mutants():
    rng = np.random.default_rng(5)
    ref = rng.normal(size=40)
    bound = np.full(40, 1e-6)
    live = np.ones(40, bool)
    live[::7] = False
    order = [i for i in np.argsort(-ref) if live[i]]
    good = order[:5]
    assert M.topk_valid(good, ref, bound, live)
    assert M.topk_valid(good[:1], ref, bound, live)
    # two ranks swapped outside the bound: inside the chosen list, and across its edge
    assert not M.topk_valid([good[1], good[0]] + good[2:], ref, bound, live)
    assert not M.topk_valid(good[:4] + [order[5]], ref, bound, live)
    assert not M.topk_valid(good[:4] + [good[0]], ref, bound, live)                    # a duplicate
    dead = int(np.nonzero(~live)[0][0])
    assert not M.topk_valid(good[:4] + [dead], ref, bound, live)                       # a masked slot
    # ... and inside the bound either order passes
    wide = np.full(40, 10.0)
    assert M.topk_valid([good[1], good[0]] + good[2:], ref, wide, live)


def test_case_table_claims():
    names = [it.name for it in M.ITEMS_2D] + [it.name for v in M.ITEMS_ND.values() for it in v]
    assert len(set(names)) == len(names)
    n_data = lambda it: -(-(it.size + 1) // it.stride)
    by = {it.name: it for it in M.ITEMS_2D}
    assert {it.n_ss for it in M.ITEMS_2D} >= {1, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1025}
    assert n_data(by["two_states"]) == 2 and n_data(by["d_plus_2"]) == 4 and n_data(by["wrapped_1025"]) == 4097
    assert n_data(by["wrapped_s3"]) == 1366 and 4097 % 3 != 0 and 401 % 3 != 0
    for d, items in M.ITEMS_ND.items():
        assert {it.stride for it in items} >= {1} and any(n_data(it) == d + 2 for it in items)
    for it in M.ITEMS_2D:
        arr = M.ring_arrays(it, 2, 1)
        valid = O.smart_start_valid(arr["ep_steps"], it.cap, arr["count"], it.n_envs) if arr["count"] else np.zeros(0, bool)
        if it.ring == "gone":
            assert not valid.any()
        if it.ring == "few":
            assert valid.sum() == 3 and it.n_plans == 4
        if it.ring == "wrapped":
            assert arr["count"] > it.cap and arr["count"] % it.cap != 0
        if it.ring == "flat":
            with pytest.raises(M.NoFactor):
                M.scott_algebra(M.scott_covariance(M.all_states(arr, it.cap)), it.size + 1)
