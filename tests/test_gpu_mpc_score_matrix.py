"""Every kernel ssc_mpc_score / ssc_mpc_score_select can launch (csrc/mpc.hip: mpc_small_kernel<16|32|64, 1|2|3|0>,
mpc_pass_a_kernel / mpc_pass_b_kernel<1|2|3|0>) and every run-time fork inside them, held to the fp64 oracle by the bound
of tests/mpc_cases.py: |score - ref| <= C_SCORE * 2^-24 * A_n for every sample of every problem, a bound fixed on the CPU
from a float32 emulation of the kernel's arithmetic (tests/test_mpc_cases_cpu.py) -- about what float32 costs, where
the older checks of tests/test_gpu_navigator.py accept 1e-3 of the largest score.  Then what no oracle comparison pins:
ties, the NaN policy, the plan pool with its clamped waypoint index, the active mask and the live list of the
one-launch scorer, and ssc_mpc_score_select == ssc_mpc_score + ssc_mpc_select_action over both selection epilogues.

Measured on an MI355X (worst |score - ref| / bound per instantiation): NOTEBOOK §15."""
import functools

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import mpc_cases as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nav():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import navigator
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return navigator


def _oracle(case, q, S=None):
    return O.mpc_scores_add_delta(q["S"] if S is None else S, q["wp"], q["left"], q["radii"], q["cur"], case.theta, case.gamma,
                                  case.hpf, case.per_row)[0]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """per problem (oracle scores, accepted error of every sample); computed once per case, never modified"""
    case = M.CASE_BY_NAME[name]
    out = []
    for q in M.case_data(case)["problems"]:
        ref, bound = _oracle(case, q), M.bound_of(case, q)
        ref.setflags(write=False)
        bound.setflags(write=False)
        out.append((ref, bound))
    return out


def _problem_set(nav, case, probs):
    return nav.MpcProblemSet([q["wp"] for q in probs], [q["left"] for q in probs], [q["radii"] for q in probs],
                             [q["cur"] for q in probs], theta=case.theta, gamma=case.gamma, horizontal_penalty_factor=case.hpf,
                             per_row_projection=case.per_row)


def _score(nav, case, S, ps=None):
    """S [H + 1, P, N, d] float32 -> numpy (scores [P, N], best [P], best_score [P])"""
    ps = ps if ps is not None else _problem_set(nav, case, M.case_data(case)["problems"])
    H1, P, N, d = S.shape
    out = nav.mpc_score(ps, torch.as_tensor(np.array(S).reshape(H1, P * N, d), device="cuda"))      # (a copy: the case data is read-only)
    return tuple(x.cpu().numpy() for x in out)


def _assert_argmax(scores, best, best_score):
    for p in range(len(scores)):
        assert best[p] == int(np.argmax(scores[p])), p                     # np.argmax: the lowest index on ties
        assert best_score[p].tobytes() == scores[p].max().tobytes(), p


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_scores_within_float32_bound_of_oracle(nav, case):
    scores, best, best_score = _score(nav, case, M.case_data(case)["S"])
    worst = 0.0
    for p, (ref, bound) in enumerate(_reference(case.name)):
        err = np.abs(scores[p] - ref)
        worst = max(worst, float(np.max(err / bound)))
    print("MPC_MATRIX %s %s walk=%s staging=%s worst |score - ref| / bound = %.3f" % (case.name, case.kernel, case.walk,
                                                                                       case.staging, worst))
    for p, (ref, bound) in enumerate(_reference(case.name)):
        assert np.all(np.abs(scores[p] - ref) <= bound), (p, float(np.max(np.abs(scores[p] - ref) / bound)))
        assert ref[best[p]] >= ref.max() - bound[best[p]] - bound[int(np.argmax(ref))], p
    _assert_argmax(scores, best, best_score)


# ------------------------------------------------------------------------------------------------------------- ties --
@pytest.mark.parametrize("name,rows", [("tp_d3_pre", (3, 67, 259)), ("tp_d2_pre", (3, 67)), ("tp_d0_str8", (1, 65, 129)),
                                       ("s64_d0_p5", (5, 21, 37)), ("s16_d2_p17", (2, 9)), ("s32_d3_p3", (4, 16))])
def test_duplicate_trajectories_lowest_index_wins(nav, name, rows):
    """the oracle's best trajectory of every problem copied to rows of other waves (n, n + 64) and other blocks (n + 256):
    their scores are the same bits and the lowest row wins"""
    case = M.CASE_BY_NAME[name]
    probs = M.case_data(case)["problems"]
    S = M.case_data(case)["S"].copy()
    expect = []
    for p, (ref, bound) in enumerate(_reference(name)):
        star = int(np.argmax(ref))
        S[:, p, list(rows)] = S[:, p, star][:, None]
        dup = sorted(set(rows) | {star})
        ref2 = _oracle(case, probs[p], S[:, p])
        others = np.delete(ref2, dup)
        # premise (oracle only): the copies stay the best by more than the kernel's error, so the winner is one of them
        assert ref2[dup].min() > others.max() + 4 * bound.max(), p
        expect.append(dup)
    scores, best, best_score = _score(nav, case, S)
    for p, dup in enumerate(expect):
        assert len({scores[p, n].tobytes() for n in dup}) == 1, p
        assert best[p] == dup[0], (p, best[p], dup)
    _assert_argmax(scores, best, best_score)


# -------------------------------------------------------------------------------------------------------- NaN policy --
@pytest.mark.parametrize("name", ["tp_d2_pre", "tp_d0_str8", "s16_d0_p5", "s64_d0_p5"])
def test_nan_rows_are_skipped_by_the_argmax_with_per_row_projection(nav, name):
    """per_row_projection = 1: rows are independent; a NaN trajectory scores NaN, the argmax skips it (np.argmax would
    return it), every other score keeps its bits; a problem of nothing but NaN rows answers best = 0"""
    case = M.CASE_BY_NAME[name]
    assert case.per_row
    base = M.case_data(case)["S"]
    clean, clean_best, _ = _score(nav, case, base)
    S = base.copy()
    nan_rows = sorted({0, 5 % case.N, case.N - 1, int(clean_best[0])})
    S[:, 0, nan_rows] = np.nan
    S[:, 1] = np.nan
    scores, best, best_score = _score(nav, case, S)
    assert np.isnan(scores[0, nan_rows]).all() and np.isnan(scores[1]).all() and best[1] == 0
    keep = np.setdiff1d(np.arange(case.N), nan_rows)
    assert scores[0, keep].tobytes() == clean[0, keep].tobytes()
    assert best[0] == keep[int(np.argmax(clean[0, keep]))] and best_score[0] == clean[0, keep].max()
    assert scores[2:].tobytes() == clean[2:].tobytes() and np.array_equal(best[2:], clean_best[2:])


@pytest.mark.parametrize("name", ["tp_d3_pre", "tp_d2_str", "s16_d2_p17", "s64_d2_p3"])
def test_one_nan_row_poisons_a_batch_global_problem(nav, name):
    """batch-global projection: one NaN row makes both global sums NaN, so every score of the problem is NaN and best = 0;
    the other problems keep their bits"""
    case = M.CASE_BY_NAME[name]
    assert not case.per_row and case.hpf != 0.0
    base = M.case_data(case)["S"]
    clean, clean_best, _ = _score(nav, case, base)
    S = base.copy()
    S[:, 1, case.N // 2] = np.nan
    scores, best, _ = _score(nav, case, S)
    assert np.isnan(scores[1]).all() and best[1] == 0
    rest = [p for p in range(case.P) if p != 1]
    assert scores[rest].tobytes() == clean[rest].tobytes() and np.array_equal(best[rest], clean_best[rest])


# --------------------------------------------------------------------------------------------------------- plan pool --
POOL_LENS = (40, 12, 2)
POOL = dict(theta=1.0, gamma=0.9, hpf=0.5, per_row=False)


def _pool_setup(nav, N, H, d, P, seed, clamp):
    """P envs following three pooled plans; cur_idx of some envs lies behind their plan's length (``clamp``: those are
    given as wp_len - 1 instead).  Rows behind a plan's length are NaN.  Returns (pool, S, [(ref, bound)])."""
    rng = np.random.default_rng(seed)
    plans = [M.make_plan(rng, W, d) for W in POOL_LENS]
    pool = nav.PlanPool(P, len(plans), max(POOL_LENS), d, theta=POOL["theta"], gamma=POOL["gamma"],
                        horizontal_penalty_factor=POOL["hpf"], per_row_projection=POOL["per_row"])
    pool.publish(plans)
    for q, W in enumerate(POOL_LENS):
        pool.wp.view(len(plans), max(POOL_LENS), d)[q, W:] = float("nan")
        pool.left.view(len(plans), max(POOL_LENS))[q, W:] = float("nan")
    plan_of = np.arange(P) % len(plans)
    cur = np.array([[0, 5, 38, 39, 45, 6000][(p // 3) % 6] if plan_of[p] == 0 else [0, 10, 11, 12, 50][(p // 3) % 5]
                    if plan_of[p] == 1 else [0, 1, 2, 7][(p // 3) % 4] for p in range(P)])
    eff = np.minimum(cur, np.asarray(POOL_LENS)[plan_of] - 1)
    assert (cur > eff).sum() >= 3
    pool.plan_of.copy_(torch.as_tensor(plan_of.astype(np.int32)))
    pool.cur_idx.copy_(torch.as_tensor((eff if clamp else cur).astype(np.int32)))
    case = M.MpcCase("pool", P, N, H, d, POOL["theta"], POOL["gamma"], POOL["hpf"], POOL["per_row"], (), (), "", "", "")
    probs = [M.make_problem(rng, POOL_LENS[plan_of[p]], int(eff[p]), N, H, d, case.theta, case.gamma, case.hpf, case.per_row,
                            plan=plans[plan_of[p]]) for p in range(P)]
    S = np.stack([q["S"] for q in probs], axis=1)
    return pool, S, [(_oracle(case, q), M.bound_of(case, q)) for q in probs], case


@pytest.mark.parametrize("N,H,d", [(16, 7, 2), (33, 8, 3), (300, 4, 2), (257, 9, 5)])
def test_plan_pool_shared_plans_and_clamped_waypoint_index(nav, N, H, d):
    P = 19
    pool, S, refs, case = _pool_setup(nav, N, H, d, P, 5, clamp=False)
    scores, best, best_score = _score(nav, case, S, ps=pool)
    assert np.isfinite(scores).all()                      # nothing read the NaN rows behind wp_len
    for p, (ref, bound) in enumerate(refs):
        assert np.all(np.abs(scores[p] - ref) <= bound), (p, float(np.max(np.abs(scores[p] - ref) / bound)))
    _assert_argmax(scores, best, best_score)
    pool2, S2, _, _ = _pool_setup(nav, N, H, d, P, 5, clamp=True)
    assert S2.tobytes() == S.tobytes()
    scores2, best2, best_score2 = _score(nav, case, S2, ps=pool2)
    assert scores2.tobytes() == scores.tobytes() and np.array_equal(best2, best) and best_score2.tobytes() == best_score.tobytes()


# -------------------------------------------------------------------------------------- active mask, live list (N <= 64) --
def _score_out(nav, pool, S):
    """run with sentinel-filled outputs; numpy (scores, best, best_score)"""
    H1, P, N, d = S.shape
    out = dict(scores=torch.full((P * N,), -7.0, device="cuda"), best=torch.full((P,), -3, dtype=torch.int32, device="cuda"),
               best_score=torch.full((P,), -9.0, device="cuda"))
    res = nav.mpc_score(pool, torch.as_tensor(np.ascontiguousarray(S).reshape(H1, P * N, d), device="cuda"), out=out)
    return tuple(x.cpu().numpy() for x in res)


def _assert_served(got, full, served):
    P = len(full[1])
    served = np.asarray(sorted(served), np.int64)
    rest = np.setdiff1d(np.arange(P), served)
    assert got[0][served].tobytes() == full[0][served].tobytes()
    assert np.array_equal(got[1][served], full[1][served]) and got[2][served].tobytes() == full[2][served].tobytes()
    assert (got[0][rest] == -7.0).all() and (got[1][rest] == -3).all() and (got[2][rest] == -9.0).all()


@pytest.mark.parametrize("N,H,d", [(16, 7, 2), (17, 8, 1), (64, 4, 3), (33, 2, 5)])
def test_active_mask_and_live_list_of_the_one_launch_scorer(nav, N, H, d):
    P = 21
    per_block = 256 // (16 if N <= 16 else 32 if N <= 32 else 64)
    pool, S, _, _ = _pool_setup(nav, N, H, d, P, 9, clamp=False)
    full = _score_out(nav, pool, S)
    _assert_served(full, full, range(P))
    rng = np.random.default_rng(3)
    mask = (rng.random(P) < 0.5).astype(np.uint8) * np.array([1, 2, 255], np.uint8)[np.arange(P) % 3]
    mask[0], mask[P - 1] = 0, 7
    pool.active = torch.as_tensor(mask, device="cuda")
    _assert_served(_score_out(nav, pool, S), full, np.nonzero(mask)[0])
    pool.active = torch.zeros(P, dtype=torch.uint8, device="cuda")
    _assert_served(_score_out(nav, pool, S), full, [])
    pool.active = None
    order = rng.permutation(np.arange(1, P))                 # problem 0 is never listed; the list is in no order
    counts = [0, 1, per_block - 1 if per_block - 1 < P - 1 else 3, per_block + 1 if per_block + 1 < P - 1 else 5, P - 1]
    for n_live in counts:
        lst = np.zeros(P, np.int32)
        lst[:n_live] = order[:n_live]
        pool.live_list = torch.as_tensor(lst, device="cuda")
        pool.n_live = torch.tensor([n_live], dtype=torch.int32, device="cuda")
        _assert_served(_score_out(nav, pool, S), full, order[:n_live])
    pool.live_list = torch.as_tensor(rng.permutation(P).astype(np.int32), device="cuda")          # n_live = P
    pool.n_live = torch.tensor([P], dtype=torch.int32, device="cuda")
    _assert_served(_score_out(nav, pool, S), full, range(P))


# ------------------------------------------------------------------------- score_select == score + select_action --
LOW, HIGH = [-2.0, -1.0, 0.0, -0.5], [2.0, 1.0, 3.0, 0.5]


@pytest.mark.parametrize("N,act,H,d", [(16, 1, 4, 2), (32, 2, 3, 3), (64, 3, 4, 2), (300, 4, 1, 3), (300, 3, 7, 2), (16, 4, 5, 8),
                                       (64, 2, 1, 1), (300, 2, 8, 5), (32, 4, 2, 2)])
def test_score_select_equals_score_then_select_bitwise(nav, N, act, H, d):
    """both selection epilogues (G lanes of the one-launch kernel, the last block of pass B), act_dim 1..4, H * act a multiple
    of 4 and not; the winner's first action read from the action matrix and regenerated from the sampling specification
    ("word ai of the sample's first Philox call"), with and without a device step counter; sampling key != noise key"""
    P, s_seed, s_pid0, n_seed, n_pid0, noise = 5, 8, 50, 13, 70, 0.005
    low, high = LOW[:act], HIGH[:act]
    rng = np.random.default_rng([N, act, H, d])
    probs = [M.make_problem(rng, 30, [0, 3, 28, 29, 11][p], N, H, d, 1.0, 0.75, 0.5, False) for p in range(P)]
    case = M.MpcCase("sel", P, N, H, d, 1.0, 0.75, 0.5, False, (), (), "", "", "")
    ps = _problem_set(nav, case, probs)
    S = torch.as_tensor(np.stack([q["S"] for q in probs], axis=1).reshape(H + 1, P * N, d), device="cuda")
    t_base = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    for (t, tb) in ((11, None), (2, t_base)):
        t_eff = t + (0 if tb is None else 5)
        A = nav.mpc_sample_actions(P, N, H, low, high, seed=s_seed, problem_id0=s_pid0, t=t, t_base=tb)
        scores, best, best_score = nav.mpc_score(ps, S)
        action, path = nav.mpc_select_action(A, S, best, P, noise, n_seed, n_pid0, t_eff)
        sp = nav.mpc_sampling(N, low, high, s_seed, s_pid0, t, t_base=tb)
        got = [nav.mpc_score_select(ps, S, A=A, act_dim=act, noise_amount=noise, seed=n_seed, problem_id0=n_pid0, t=t_eff),
               nav.mpc_score_select(ps, S, sampling=sp, act_dim=act, noise_amount=noise, seed=n_seed, problem_id0=n_pid0, t=t)]
        for sc, b, a, pth in got:
            assert torch.equal(sc, scores) and torch.equal(b, best) and torch.equal(a, action) and torch.equal(pth, path)
        _, _, clean, _ = nav.mpc_score_select(ps, S, sampling=sp, act_dim=act, noise_amount=0.0, seed=n_seed, problem_id0=n_pid0, t=t)
        action, clean, path, best, Sn = (x.cpu().numpy() for x in (action, clean, path, best, S))
        for p in range(P):
            first = O.mpc_action_samples(s_seed, s_pid0 + p, N, H, act, t_eff, low, high)[best[p], 0]
            assert np.array_equal(clean[p], first)
            for ai in range(act):
                g = O.mpc_noise_gaussian(n_seed, np.array([n_pid0 + p], np.uint64), t_eff, ai)[0]
                assert abs(action[p, ai] - (first[ai] + noise * g)) <= 1e-6, (p, ai)
            assert np.array_equal(path[p], Sn[:, p * N + best[p]])
