"""Dispatch matrix of the MPC trajectory scorer (csrc/mpc.hip: ssc_mpc_score / ssc_mpc_score_select): the case table, each
case's inputs, the fp64 walk with its decision margins and per-sample error scale, a float32 emulation of the kernel's
arithmetic, the bound derived from the two, and the emulation mutants that bound must reject.  Shared by the CPU test
(tests/test_mpc_cases_cpu.py) and the GPU tests (tests/test_gpu_mpc_score_matrix.py, tests/test_gpu_nav_kernels.py);
numpy + oracle only.

The bound.  ``ref`` = O.mpc_scores_add_delta in fp64 on the float32 inputs the kernel receives, ``emu`` = ``emu32``: the same
walk in float32, one rounding per operation in the order of ``walk_step`` (no fma), the two batch-global sums in fp64 and
their quotient rounded to float32.  Beside the fp64 walk every sample gets the size of the terms its score is made of,

    A_n = sum_t gamma^t (|prev_t| + |end_t|) + hpf * gamma * sum_t (|a_t| + |c_t| |b_t|)

and r_case = max_n |emu - ref| / (2^-24 A_n) is what float32 costs at that case in units of one rounding of A_n.  A score
X of the kernel is accepted when |X - ref| <= C_SCORE * 2^-24 * A_n with C_SCORE = 4 * max_cases r_case: the factor 4
covers fma contraction and the kernel's summation order.  C_SCORE is fixed here, without the kernel.

Stability.  The walk's ``move`` decision is discontinuous; a near tie (dc close to theta, dn close to dc) may flip in
float32 and, in batch-global mode, move the projection scalar of the whole problem.  The generator therefore computes
every sample's decision margin in fp64 and redraws the trajectories whose margin is below THR (the shared start state
when the tie is at t = 0) until none is left; after that no sample is excluded from any assertion.
"""
import zlib
from collections import namedtuple

import numpy as np

EPS32 = 2.0 ** -24
THR = 1e-4              # smallest decision margin a kept trajectory may have, radii-scaled units
C_SCORE = 4.2           # 4 * max r_case of the table below, rounded up (tests/test_mpc_cases_cpu.py recomputes it)

# name, problems, samples, horizon, state dim, theta, gamma, hpf, per_row_projection, ((W, cur) per problem), the problems
# that must hold a sample advancing on every horizon step, and what mpc_score_common launches for it (read off the dispatch
# code): kernel instantiation(s), walk (pre = prefetched: H + 1 <= 8 and d <= 4; str = streamed), pass A sums (deferred
# block sums with the prefetched walk, per-step wave butterflies with the streamed one), pass B partial staging.
MpcCase = namedtuple("MpcCase", "name P N H d theta gamma hpf per_row plans along kernel walk staging")


def _c(name, N, H, d, theta, gamma, hpf, per_row, plans, along=(), staging="-"):
    P = len(plans)
    walk = "pre" if (H + 1 <= 8 and d <= 4) else "str"
    D = d if d <= 3 else 0
    if N <= 64:
        kernel = "small<%d,%d>" % (16 if N <= 16 else 32 if N <= 32 else 64, D)
    else:
        kernel = "pass_a<%d>+pass_b<%d>" % (D, D)
        nblk = (N + 255) // 256
        n_part = nblk * (H + 1) * 2
        staging = "unstaged" if n_part * 8 > 32 * 1024 else "one_trip" if n_part <= 256 else "trips"
    return MpcCase(name, P, N, H, d, theta, gamma, hpf, per_row, tuple(plans), tuple(along), kernel, walk, staging)


CASES = [
    # ---- one-launch kernel, every <G, D>; P leaves shadow groups in the last block (256 / G groups per block)
    _c("s16_d1_p1", 1, 0, 1, 0.7, 1.0, 0.5, False, [(2, 0)]),
    _c("s16_d2_p17", 16, 7, 2, 1.0, 0.3, 2.0, False, [(40, 0), (40, 38), (40, 39), (2, 0), (2, 1), (6000, 3000)] + [(12 + p, p) for p in range(11)],
       along=(0, 5)),
    _c("s16_d3_p5", 16, 8, 3, 1.3, 0.75, 0.0, False, [(30, 0), (30, 28), (30, 29), (2, 1), (30, 9)], along=(0, 4)),
    _c("s16_d0_p5", 16, 1, 4, 0.7, 1.0, 0.5, True, [(9, 0), (9, 7), (9, 8), (2, 0), (9, 4)]),
    _c("s32_d1_p5", 17, 8, 1, 1.0, 0.3, 0.5, False, [(25, 0), (25, 23), (25, 24), (2, 0), (25, 5)], along=(4,)),
    _c("s32_d2_p9", 32, 1, 2, 0.7, 0.9, 2.0, False, [(7, c) for c in (0, 5, 6, 3)] + [(2, 0), (2, 1), (11, 4), (11, 9), (11, 10)]),
    _c("s32_d3_p3", 17, 7, 3, 1.0, 1.0, 0.5, True, [(20, 0), (20, 18), (20, 19)], along=(0,)),
    _c("s32_d0_p5", 32, 32, 5, 0.8, 0.9, 0.5, False, [(60, 0), (60, 58), (60, 59), (2, 0), (60, 11)], along=(4,)),
    _c("s64_d1_p5", 33, 7, 1, 1.3, 0.75, 0.5, False, [(14, 0), (14, 12), (14, 13), (2, 1), (14, 3)]),
    _c("s64_d2_p3", 64, 32, 2, 1.0, 1.0, 0.5, False, [(6000, 3000), (50, 48), (50, 2)], along=(0, 2)),
    _c("s64_d3_p2", 33, 0, 3, 1.0, 0.3, 2.0, True, [(5, 0), (5, 4)]),
    _c("s64_d0_p5", 64, 8, 8, 0.7, 0.75, 0.5, True, [(30, 0), (30, 28), (30, 29), (2, 0), (30, 13)], along=(4,)),
    # ---- two-pass path, every <D> on both walks, several problems each
    _c("tp_d1_pre", 65, 7, 1, 1.0, 0.3, 0.5, False, [(20, 0), (20, 18), (20, 19)], along=(0,)),
    _c("tp_d1_str", 255, 8, 1, 0.7, 1.0, 2.0, False, [(30, 5), (2, 0)], along=(0,)),
    _c("tp_d2_pre", 256, 1, 2, 1.3, 0.9, 0.5, True, [(8, 0), (8, 6), (2, 1)]),
    _c("tp_d2_str", 257, 32, 2, 1.0, 0.75, 0.5, False, [(6000, 3000), (50, 0)], along=(0, 1)),
    _c("tp_d3_pre", 513, 7, 3, 0.7, 1.0, 0.5, False, [(25, 24), (25, 3)], along=(1,)),
    _c("tp_d3_str", 257, 8, 3, 1.0, 0.3, 0.0, False, [(30, 28), (30, 7), (2, 0)], along=(1,)),
    _c("tp_d0_pre4", 257, 7, 4, 1.0, 0.75, 2.0, False, [(22, 0), (22, 9)], along=(1,)),
    _c("tp_d0_str5", 513, 1, 5, 0.8, 1.0, 0.5, False, [(10, 8), (10, 2)]),
    _c("tp_d0_str8", 255, 8, 8, 0.7, 0.3, 0.5, True, [(30, 29), (30, 6)], along=(1,)),
    _c("tp_h0", 65, 0, 2, 1.0, 0.75, 0.5, False, [(6, 0), (6, 5), (2, 0)]),
    # ---- pass B partial staging: n_part = nblk * (H + 1) * 2 doubles: <= 256 one trip, more in several trips, > 32 KB not staged
    _c("tp_npart256", 4096, 7, 2, 1.0, 0.75, 0.5, False, [(40, 11), (40, 38)], along=(0,)),
    _c("tp_npart272", 4097, 7, 2, 1.0, 0.9, 0.5, False, [(40, 0), (2, 0)], along=(0,)),
    _c("tp_trips_str", 2049, 32, 3, 1.0, 0.75, 0.5, False, [(60, 7)], along=(0,)),
    _c("tp_unstaged", 62 * 256 + 1, 32, 2, 1.0, 0.75, 0.5, False, [(80, 20)], along=(0,)),
]
CASE_BY_NAME = {c.name: c for c in CASES}

MUTANTS = ("cproj_prev_step", "sums_drop_ragged", "penalty_gamma_pow_t", "b_is_idx", "window_base_plus_one", "prev_not_carried",
           "left_pre_move")


# ---------------------------------------------------------------------------------------------------------- generator --
def make_plan(rng, W, d, spacing=0.8):
    """A plan of W waypoints whose consecutive waypoints are about ``spacing`` apart in radii-scaled units: float32
    (wp [W, d], left [W], radii [d]).  The radii differ in every dimension."""
    radii = (0.02 * (1.0 + 0.5 * np.arange(d))).astype(np.float32)
    drift = rng.normal(size=d)
    steps = rng.normal(size=(W, d)) + 0.6 * drift / np.linalg.norm(drift) * np.sqrt(d)
    steps *= spacing * rng.uniform(0.75, 1.25, size=(W, 1)) / np.linalg.norm(steps, axis=1, keepdims=True)
    offset = np.where(np.arange(d) % 2 == 0, -0.5, 0.25)
    wp = ((np.cumsum(steps, axis=0) - steps[0]) * radii + offset).astype(np.float32)
    return wp, distances_left32(wp, radii), radii


def distances_left32(wp, radii):
    """NND_MB_agent.py:411-418 (O.distances_left) as a reversed cumulative sum, rounded to the float32 the kernel is given"""
    seg = np.sqrt((((wp[1:].astype(np.float64) - wp[:-1]) / radii.astype(np.float64)) ** 2).sum(axis=1))
    return np.concatenate([np.cumsum(seg[::-1])[::-1], [0.0]]).astype(np.float32)


def _pos(wp64, u):
    """point at (real-valued) plan position u on the polyline through the waypoints"""
    u = np.clip(u, 0.0, len(wp64) - 1.0)
    i = np.minimum(np.floor(u).astype(np.int64), len(wp64) - 2)
    f = (u - i)[..., None]
    return wp64[i] * (1.0 - f) + wp64[i + 1] * f


def _draw_traj(rng, n, H, d, first_fast=False):
    """plan positions (relative to cur) [H + 1, n] and radii-scaled noise [H + 1, n, d] of n fresh trajectories: one in
    eight steps along the plan one waypoint per horizon step with little noise, the others at a random slower pace"""
    fast = rng.random(n) < 0.125
    fast[0] |= first_fast
    mean = np.where(fast, 1.0, rng.uniform(0.0, 1.0, n))
    speed = np.minimum(mean * np.where(fast, 1.0, rng.uniform(0.5, 1.5, size=(H + 1, n))), 1.0)
    u = np.cumsum(speed, axis=0) - speed[0]
    noise = rng.normal(size=(H + 1, n, d)) * (np.where(fast, 0.05, 0.3) / np.sqrt(d))[None, :, None]
    return u, noise


def make_problem(rng, W, cur, N, H, d, theta, gamma, hpf, per_row, thr=THR, plan=None):
    """One navigation problem with N stable candidate trajectories.  Returns a dict: wp, left, radii (float32), cur, S
    [H + 1, N, d] float32, redrawn (trajectories drawn again because a decision margin was below thr; a redrawn start
    state counts as N).  ``plan``: (wp, left, radii) of make_plan to use instead of a fresh one."""
    wp, left, radii = make_plan(rng, W, d) if plan is None else plan
    wp64, r64 = wp.astype(np.float64), radii.astype(np.float64)
    start_noise = rng.normal(size=d) * 0.3 / np.sqrt(d)
    u, noise = _draw_traj(rng, N, H, d, first_fast=True)
    redrawn = 0
    for _ in range(200):
        noise[0] = start_noise          # the N candidates of a problem start in the env's state
        S = (_pos(wp64, cur + u) + noise * r64).astype(np.float32)
        wk = walk64(S, wp, left, radii, cur, theta, gamma, hpf, per_row)
        if wk["margin_t"][0].min() < thr:
            start_noise = rng.normal(size=d) * 0.3 / np.sqrt(d)
            redrawn += N
            continue
        bad = np.nonzero(wk["margin"] < thr)[0]
        if bad.size == 0:
            return dict(wp=wp, left=left, radii=radii, cur=int(cur), S=S, redrawn=redrawn)
        redrawn += bad.size
        u[:, bad], noise[:, bad] = _draw_traj(rng, bad.size, H, d)
    raise AssertionError("no stable draw")


_CACHE = {}


def case_data(case):
    """dict(problems=[make_problem ...], S [H + 1, P, N, d] float32); deterministic in the case's name, computed once."""
    if case.name not in _CACHE:
        probs = []
        for p, (W, cur) in enumerate(case.plans):
            rng = np.random.default_rng([zlib.crc32(case.name.encode()), p])
            probs.append(make_problem(rng, W, cur, case.N, case.H, case.d, case.theta, case.gamma, case.hpf, case.per_row))
        S = np.stack([q["S"] for q in probs], axis=1)
        S.setflags(write=False)
        _CACHE[case.name] = dict(problems=probs, S=S)
    return _CACHE[case.name]


# ----------------------------------------------------------------------------------------------------------- fp64 walk --
def walk64(S, wp, left, radii, cur, theta, gamma, hpf, per_row):
    """O.mpc_scores_add_delta restated with what the bound needs computed beside it: scores [N], final_idx [N], margin_t
    [H + 1, N] (distance of each step's move decision from flipping, inf where the index is at the last waypoint),
    margin [N] = min over t, A [N] the error scale of the docstring above, dmax the largest distance met."""
    S, wp, left, radii = (np.asarray(x, np.float64) for x in (S, wp, left, radii))
    H1, N, _ = S.shape
    W = len(wp)

    def dist(a, b):
        return np.sqrt((((a - b) / radii) ** 2).sum(axis=-1))
    idx = np.full(N, int(cur), np.int64)
    prev = left[idx] + dist(S[0], wp[idx])
    scores, A = np.zeros(N), np.zeros(N)
    margin_t = np.empty((H1, N))
    dmax = float(np.max(prev - left[idx]))
    for t in range(H1):
        pts = S[t]
        dc, dn = dist(wp[idx], pts), dist(wp[np.minimum(idx + 1, W - 1)], pts)
        dmax = max(dmax, float(dc.max()), float(dn.max()))
        a_, b_ = dc <= theta, dn <= dc
        m1, m2 = np.abs(dc - theta), np.abs(dn - dc)
        # move = a_ or b_: both must flip where both hold, the one that holds where one does, either where neither does
        m = np.where(a_ & b_, np.maximum(m1, m2), np.where(a_, m1, np.where(b_, m2, np.minimum(m1, m2))))
        margin_t[t] = np.where(idx != W - 1, m, np.inf)
        move = (a_ | b_) & (idx != W - 1)
        idx = idx + move
        dc = np.where(move, dn, dc)
        end = left[idx] + dc
        scores = scores + (prev - end) * gamma ** t
        A += gamma ** t * (np.abs(prev) + np.abs(end))
        prev = end
        b = np.maximum(idx - 1, 0)
        a_s, b_s = (pts - wp[b]) / radii, (wp[b + 1] - wp[b]) / radii
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (a_s * b_s).sum(axis=1) / (b_s * b_s).sum(axis=1) if per_row else np.full(N, (a_s * b_s).sum() / (b_s * b_s).sum())
        pen = np.sqrt(((c[:, None] * b_s - a_s) ** 2).sum(axis=1))
        scores = scores - pen * hpf * gamma
        A += hpf * gamma * (np.sqrt((a_s ** 2).sum(axis=1)) + np.abs(c) * np.sqrt((b_s ** 2).sum(axis=1)))
    return dict(scores=scores, final_idx=idx, margin_t=margin_t, margin=margin_t.min(axis=0), A=A, dmax=dmax)


def walk64_of(case, prob):
    return walk64(prob["S"], prob["wp"], prob["left"], prob["radii"], prob["cur"], case.theta, case.gamma, case.hpf, case.per_row)


def bound_of(case, prob):
    """the accepted |score - ref| of every sample of a problem"""
    return C_SCORE * EPS32 * walk64_of(case, prob)["A"]


# ---------------------------------------------------------------------------------------------------- fp32 emulation --
def emu32(S, wp, left, radii, cur, theta, gamma, hpf, per_row, mutant=None):
    """The scorer in float32 numpy in the operation order of walk_step (csrc/mpc.hip), one rounding per operation (no
    fma), window-relative indices, fp64 sums for the two batch-global scalars and their quotient rounded to float32.
    ``mutant``: one of MUTANTS, a wrong kernel."""
    f = np.float32
    S, wp, left, radii = (np.asarray(x, f) for x in (S, wp, left, radii))
    H1, N, d = S.shape
    Wabs = len(wp)
    theta, gamma, hpf = f(theta), f(gamma), f(hpf)
    inv_r = f(1.0) / radii
    wb = max(int(cur) - 1, 0)                         # load_window_at
    W, idx0 = Wabs - wb, int(cur) - wb
    src = np.minimum(wb + (1 if mutant == "window_base_plus_one" else 0) + np.arange(W + 1), Wabs - 1)
    wps, lefts = wp[src], left[src]

    def ell(x, y):
        s = np.zeros(N, f)
        for k in range(d):
            v = (x[:, k] - y[:, k]) * inv_r[k]
            s = s + v * v
        return np.sqrt(s)

    n_sum = N if mutant != "sums_drop_ragged" else 256 * (N // 256)
    cproj = np.zeros(H1, f)
    for PASS in (0, 1):
        idx = np.full(N, idx0, np.int64)
        score, gpow = np.zeros(N, f), np.ones(N, f)
        prev = lefts[idx] + ell(S[0], wps[idx])
        for t in range(H1):
            pt = S[t]
            idx_pre = idx
            dc, dn = ell(wps[idx], pt), ell(wps[np.minimum(idx + 1, W - 1)], pt)
            move = ((dc <= theta) | (dn <= dc)) & (idx != W - 1)
            idx = idx + move
            dc = np.where(move, dn, dc)
            end = lefts[idx_pre if mutant == "left_pre_move" else idx] + dc
            if PASS == 1:
                score = score + (prev - end) * gpow
            if mutant != "prev_not_carried":
                prev = end
            b = idx if mutant == "b_is_idx" else np.maximum(idx - 1, 0)
            ab, bb = np.zeros(N, f), np.zeros(N, f)
            av, bv = np.empty((N, d), f), np.empty((N, d), f)
            for k in range(d):
                av[:, k] = (pt[:, k] - wps[b, k]) * inv_r[k]
                bv[:, k] = (wps[b + 1, k] - wps[b, k]) * inv_r[k]
                ab = ab + av[:, k] * bv[:, k]
                bb = bb + bv[:, k] * bv[:, k]
            with np.errstate(divide="ignore", invalid="ignore"):
                if PASS == 0:
                    cproj[t] = f(ab[:n_sum].astype(np.float64).sum() / bb[:n_sum].astype(np.float64).sum())
                    continue
                c = ab / bb if per_row else np.full(N, cproj[max(t - 1, 0) if mutant == "cproj_prev_step" else t], f)
            s = np.zeros(N, f)
            for k in range(d):
                v = c * bv[:, k] - av[:, k]
                s = s + v * v
            w = gpow if mutant == "penalty_gamma_pow_t" else gamma
            score = score - np.sqrt(s) * hpf * w
            gpow = gpow * gamma
    return score


def emu32_of(case, prob, mutant=None):
    return emu32(prob["S"], prob["wp"], prob["left"], prob["radii"], prob["cur"], case.theta, case.gamma, case.hpf, case.per_row,
                 mutant)


# ------------------------------------------------------------------------------------------------- navigator observe --
def observe_margin(x, wp, radii, idx, theta):
    """distance of nav_observe's decisions at new state x from flipping: the move decision (as in walk64) and the
    near-the-goal test"""
    x, wp, radii = (np.asarray(v, np.float64) for v in (x, wp, radii))
    W = len(wp)
    dist = lambda a, b: float(np.sqrt((((a - b) / radii) ** 2).sum()))
    dc, dn, dg = dist(x, wp[idx]), dist(x, wp[min(idx + 1, W - 1)]), dist(x, wp[-1])
    m1, m2 = abs(dc - theta), abs(dn - dc)
    a_, b_ = dc <= theta, dn <= dc
    m = max(m1, m2) if (a_ and b_) else m1 if a_ else m2 if b_ else min(m1, m2)
    return min(m if idx != W - 1 else np.inf, abs(dg - theta))
