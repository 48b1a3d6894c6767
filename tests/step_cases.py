"""Cases for the fused MPC / SmartStart step kernel (csrc/rollout.hip: mpc_rollout_step_kernel, six instantiations behind
ssc_mpc_rollout_step, ssc_smartstart_rollout_step and ssc_smartstart_rollout_step_many), one launch at a time.

Every launch is one step from state the caller owns, so a case puts each env into the situation it wants: the builder
(``case_data``) assigns envs round-robin to the classes of NAV / BASE / DONE, builds each navigating env's plan AROUND the
state the oracle's step reaches (so every distance of the bookkeeping is chosen, not met by chance), and searches the env-id
base until every decision of the case -- ``dc <= theta``, ``dn <= dc``, ``near``, the MountainCar goal, the reset-state goal
test -- holds with the margin MARGIN in fp64.  ``expected_step`` re-derives everything a launch writes from the case's ARRAYS
with the functions of oracle/ssc_oracle.py (not from the builder's intentions), ``check_step`` compares a read-back with it,
and ``model_step`` is a float32 numpy model of the kernel with the mutants the checker has to reject
(tests/test_step_cases_cpu.py).  numpy and the oracle only: importable without torch or a GPU.

What the oracle lacks is added here: the waypoint-index clamp (``idx = min(idx, W - 1)``, mpc_device.h nav_observe_plan /
mpc.hip load_window: a re-published shorter plan under a live env), ``slot0`` of the population's plan windows, and the
``mpc`` form's episode end (``idx <- start_idx``, NND_MB_agent.start_new_episode_plan :383-384; ``ou_x <- 0``).

A case is three launches in a row.  The per-env inputs (state, mode, bookkeeping, ``best_idx``, ``actor_out``, ``A``) are
refreshed before every launch from the schedule -- classes rotate over the envs -- while the step counters, the ticket, the
log, the mode log, the episode ring and the statistics live on across the launches.  The class census of a case counts its
three launches.  The log has k0 + LAUNCHES + 1 rows (4 for k0 = 0): the rows before k0 and the one behind the last written
row keep their NaN prefill.

MARGIN is derived, not measured: the obs2 tolerances below divided by the smallest radius (0.05) move a distance by at most
3e-6 / 0.05 = 6e-5, the float32 evaluation of ell_dist adds less than 1e-6 relative, so 1e-3 leaves a factor above 10.
The teacher-forced re-evaluation at the kernel's own obs2 re-asserts MARGIN / 2.

Without a log the kernel's action and obs2 are not observable; the written-back state is then held to the oracle's step under
the oracle's action, at the obs2 tolerance plus the action tolerance times the step's sensitivity to the action
(MountainCar: power; Pendulum: 3 dt / (m l^2) for theta-dot, that times dt for theta), which is the same requirement."""
import functools
from collections import namedtuple

import numpy as np

from oracle import ssc_oracle as O

N_SAMPLES, HORIZON = 5, 3
THETA, GIVE_UP, FINAL_STEPS = 1.0, 5, 10
MARGIN = 1e-3
MIN_RADIUS = 0.05
MAX_STEPS = 40
WMAX = 6                     # waypoint rows per plan slot
W_PLAN = 5                   # waypoints of a per-env plan
LAUNCHES = 3
TAIL = 3                     # guard envs behind the last one
ENV_SEED, NOISE_SEED, PROBLEM_ID0 = 11, 23, 5000          # noise_seed != env_seed, problem_id0 != env_id0 (>= 1000, < 5000)
OU = dict(mu=0.05, sigma=0.2, theta=0.15, dt=0.01)
OBS = {"mc": 2, "pend": 3}
BOUNDS = {"mc": (-1.0, 1.0), "pend": (-2.0, 2.0)}
ENVS, FORMS = ("mc", "pend"), ("mpc", "ss", "many")
SIZES = (1, 64, 255, 256, 257, 600)
MANY_SIZES, MANY_ENV0 = (1, 300, 70, 256), (3, 4, 309, 379)     # 3 envs before pair 0, 5 between pairs 1 and 2
MANY_N = 635
BLOCK = 256

NAV = ("stay", "adv_dc", "adv_dn", "give_up", "last_wp", "near", "final", "clamped")
BASE = {"mc": ("inside", "sat_lo", "sat_hi"), "pend": ("inside2", "sat2_lo", "sat2_hi", "sat_lo", "sat_hi")}
DONE = {"mc": ("none", "tl", "none", "goal", "none", "both"), "pend": ("none", "tl")}
DONE_CLASSES = {"mc": ("tl", "goal", "both"), "pend": ("tl",)}
OUTCOMES = ("coin_gt", "new_nav", "new_close", "pool_empty")

# the project's tolerances
TOL_OBS2 = {"mc": np.array([2.4e-7, 1e-8]), "pend": np.array([3e-6, 3e-6, 3e-6])}
TOL_STATE = {"mc": np.array([2.4e-7, 1e-8]), "pend": np.array([3e-6, 3e-6])}
REW_REL = {"mc": 1e-6, "pend": 2e-5}
TOL_RESET_PEND = 2e-6
TOL_BASE_ACT = {e: 2e-5 * (BOUNDS[e][1] - BOUNDS[e][0]) / 2 for e in ENVS}
TOL_OU = 2e-5
TOL_NAV_ACT = 1e-6
# |d state' / d action| and |d reward / d action| / |action|: the widening where the action is not logged
SENS_STATE = {"mc": np.array([O.MC_BASE_POWER, O.MC_BASE_POWER]), "pend": np.array([3.0 * O.PEND_DT * O.PEND_DT, 3.0 * O.PEND_DT])}
SENS_REW = {"mc": 0.2, "pend": 0.002}

Case = namedtuple("Case", "name env form n idx opts")


def _opts(**kw):
    o = dict(log="packed", ring="full", at_goal=True, stats=True, noise=0.005, mode_log=True, n_live=False, t0=4, k0=0, eta=0.4,
             eps=0.8, pool_count=4, v1=False, ou_col=True)
    o.update(kw)
    return o


_SINGLE_OPTS = {
    1: _opts(eta=1.0),
    64: _opts(log="none", ring="none", at_goal=False, stats=False, noise=0.0, mode_log=False, n_live=True, t0=5, ou_col=False),
    255: _opts(log="strided", ring="small", t0=6, k0=2, eps=-0.3, v1=True),
    256: _opts(at_goal=False, noise=0.0, mode_log=False, t0=7, eta=1.0, eps=0.0, pool_count=0),
    257: _opts(n_live=True, t0=(1 << 32) + 3, k0=2),
    600: _opts(ring="small", t0=9),
}
_MANY_OPTS = (_opts(t0=4), _opts(log="none", ring="none", at_goal=False, stats=False, noise=0.0, mode_log=False, t0=(1 << 32) + 3, v1=True),
              _opts(log="strided", ring="small", t0=6, k0=2))


def _cases():
    out = []
    for env in ENVS:
        for form in ("mpc", "ss"):
            for k, n in enumerate(SIZES):
                out.append(Case("%s_%s_n%d" % (env, form, n), env, form, n, k, _SINGLE_OPTS[n]))
        for k, o in enumerate(_MANY_OPTS):
            out.append(Case("%s_many_%s" % (env, "abc"[k]), env, "many", MANY_N, k, o))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def pairs_of(case):
    """the pair table of the population form; the single forms are one pair over all envs"""
    o = case.opts
    if case.form != "many":
        return [dict(env0=0, n_envs=case.n, slot0=0, first=5, count=o["pool_count"], slots=7, eta=o["eta"], eps=o["eps"])]
    slots, slot0, first = (7, 6, 8, 5), (0, 9, 17, 27), (5, 4, 6, 3)                  # first + count > slots: the pick wraps
    return [dict(env0=MANY_ENV0[y], n_envs=MANY_SIZES[y], slot0=slot0[y], first=first[y], count=(4, 4, 4, 0)[y], slots=slots[y],
                 eta=(0.0, 0.4, 1.0, 1.0)[y], eps=(0.8, -0.3, 0.8, 0.0)[y]) for y in range(4)]


def n_blocks(case):
    """workgroups of one launch (the grid the ticket counts)"""
    pairs = pairs_of(case)
    return len(pairs) * ((max(p["n_envs"] for p in pairs) + BLOCK - 1) // BLOCK)


def log_rows(case):
    return case.opts["k0"] + LAUNCHES + 1


def strides(case):
    """(log row stride, done row stride, mode log stride) as the kernel uses them"""
    return (case.n + 5, case.n + 9, case.n + 2) if case.opts["log"] == "strided" else (case.n, case.n, case.n)


def ring_capacity(case):
    return {"none": 0, "full": LAUNCHES * case.n, "small": 5}[case.opts["ring"]]


def _f32(x):
    return np.asarray(x, np.float32)


def _f64(x):
    return np.asarray(x, np.float64)


def _layout(case):
    pairs = pairs_of(case)
    n_alloc = case.n + TAIL
    pair_of = np.full(n_alloc, -1)
    li = np.zeros(n_alloc, np.int64)
    for y, p in enumerate(pairs):
        pair_of[p["env0"]:p["env0"] + p["n_envs"]] = y
        li[p["env0"]:p["env0"] + p["n_envs"]] = np.arange(p["n_envs"])
    plan0 = max(p["slot0"] + 2 * p["slots"] for p in pairs) + 2
    return dict(pairs=pairs, n_alloc=n_alloc, pair_of=pair_of, li=li, live=pair_of >= 0, plan0=plan0,
                n_slots=plan0 + LAUNCHES * n_alloc + 8)


def _pair_col(d, key, dtype=np.float64):
    """per env: its pair's value of ``key`` (0 for an env of no pair)"""
    v = np.array([p[key] for p in d["pairs"]] + [0], dtype)
    return v[d["pair_of"]]


# ------------------------------------------------------------------------------------------------ oracle pieces --
def observe64(env, s0, s1):
    return np.stack([_f64(s0), _f64(s1)], axis=-1) if env == "mc" else O.pend_obs(s0, s1)


def step64(case, s0, s1, a):
    """(s0', s1', reward, goal) of the oracle's env step"""
    if case.env == "mc":
        return O.mc_step(s0, s1, a, power=float(np.float32(O.MC_BASE_POWER)))
    th, thd, r, _ = O.pend_step(s0, s1, a, v1_order=case.opts["v1"])
    return th, thd, r, np.zeros(np.shape(r), bool)


def reset64(case, ids, t):
    f = O.mc_reset_state if case.env == "mc" else O.pend_reset_state
    return f(ENV_SEED, ids, np.uint64(t))


def _ids(d):
    return np.uint64(d["env_id0"]) + np.arange(d["n_alloc"], dtype=np.uint64)


def _navigating(case, inp):
    return np.ones(len(inp["mode"]), bool) if case.form == "mpc" else inp["mode"] != 0


def oracle_action(case, d, inp, t):
    """fp64 (action, OU state after the action) of every env: NND_MB_agent.get_action's tail (:353-356) while navigating,
    DDPG_Baselines_agent.get_action (:206-240) with the OU draw of :72-75 otherwise"""
    n_alloc = d["n_alloc"]
    nav = _navigating(case, inp)
    i = np.arange(n_alloc)
    a = inp["A"][i, inp["best_idx"], 0].astype(np.float64)
    noise = float(np.float32(case.opts["noise"]))
    if noise != 0.0:
        a = a + noise * O.mpc_noise_gaussian(NOISE_SEED, np.uint64(PROBLEM_ID0) + i.astype(np.uint64), t)
    ou = inp["ou_x"].astype(np.float64).copy()
    if case.form != "mpc":
        low, high = BOUNDS[case.env]
        ids = _ids(d)
        for y, p in enumerate(d["pairs"]):
            sel = d["live"] & ~nav & (d["pair_of"] == y)
            if not sel.any():
                continue
            eps = float(np.float32(p["eps"]))
            if eps > 0:
                g = O.ou_gaussian(ENV_SEED, ids[sel], np.uint64(t))
                ou[sel] = O.ou_step(ou[sel], g, float(np.float32(OU["mu"])), float(np.float32(OU["sigma"])),
                                    float(np.float32(OU["theta"])), float(np.float32(OU["dt"])))
            a[sel] = O.ddpg_action(inp["actor_out"][sel].astype(np.float64), ou[sel], eps, low, high)
    return a, ou


def plan_of_slot(d, q):
    """(waypoints [W, d], radii [d]) of plan slot q, as fp64 of the float32 the kernel reads"""
    W = int(d["wp_len"][q])
    off = int(d["wp_off"][q])
    return d["wp"][off:off + W].astype(np.float64), d["radii"][q].astype(np.float64)


def bookkeeping(case, d, inp, x):
    """NND_MB_agent.observe (:360-373) + close_enough_to_goal (:425-432) of every navigating env at the new observation
    x [n_alloc, OBS], with the kernel's clamp of a waypoint index beyond a re-published shorter plan.
    Returns (cur_idx', actions_done', at_goal, margin): margin = the least distance of a comparison from its threshold."""
    nav = _navigating(case, inp) & d["live"]
    idx2, da2 = inp["cur_idx"].copy(), inp["actions_done"].copy()
    at_goal = np.zeros(len(idx2), bool)
    margin = np.full(len(idx2), np.inf)
    for i in np.nonzero(nav)[0]:
        wp, r = plan_of_slot(d, int(inp["plan_of"][i]))
        W = len(wp)
        idx = min(int(inp["cur_idx"][i]), max(W - 1, 0))            # the clamp the oracle lacks
        idx2[i], da2[i], at_goal[i] = O.nav_observe(x[i], wp, r, idx, int(inp["actions_done"][i]) + 1, THETA, GIVE_UP, FINAL_STEPS)
        dist = O.distance_func(r)
        dc, dg = dist(x[i], wp[idx]), dist(x[i], wp[-1])
        m = min(abs(dc - THETA), abs(dg - THETA))
        if idx != W - 1:
            m = min(m, abs(dist(x[i], wp[idx + 1]) - dc))
        margin[i] = m
    return idx2, da2, at_goal, margin


def new_episodes(case, d, inp, done, t):
    """SmartStartContinuous.start_new_episode (:341-370) of every finishing env on its reset state.
    Returns (slot taken or -1, navigating afterwards, margin of the reset-state goal test, reset s0, reset s1)."""
    n_alloc = d["n_alloc"]
    q = np.full(n_alloc, -1)
    navigating = np.zeros(n_alloc, bool)
    margin = np.full(n_alloc, np.inf)
    ids = _ids(d)
    r0, r1 = reset64(case, ids, t)
    if case.form == "mpc":
        return q, navigating, margin, r0, r1
    robs = observe64(case.env, r0, r1)
    for i in np.nonzero(done & d["live"])[0]:
        p = d["pairs"][d["pair_of"][i]]
        s = O.smartstart_new_episode(ENV_SEED, int(ids[i]), t, p["eta"], p["first"], p["count"], p["slots"])
        if s < 0:
            continue
        q[i] = p["slot0"] + s                                        # the pair's window of the plan pool
        wp, r = plan_of_slot(d, int(q[i]))
        dg = O.distance_func(r)(robs[i], wp[-1])                     # close_enough_to_goal on a fresh plan: the goal test alone
        navigating[i] = not dg <= THETA
        margin[i] = abs(dg - THETA)
    return q, navigating, margin, r0, r1


# ------------------------------------------------------------------------------------------------------ builder --
def _unit(rng, dim):
    u = rng.normal(size=dim)
    return u / np.linalg.norm(u)


def _classes(case, d, j):
    """round-robin: (action class, done class) of every env for launch j ('' for an env of no pair)"""
    acts = NAV if case.form == "mpc" else NAV + BASE[case.env]
    dn = DONE[case.env]
    L = len(acts)
    act = np.array([acts[(l + 3 * j) % L] if ok else "" for l, ok in zip(d["li"], d["live"])], dtype=object)
    done = np.array([dn[(l // L + l + j) % len(dn)] if ok else "" for l, ok in zip(d["li"], d["live"])], dtype=object)
    return act, done


_NAV_GEOM = {   # class: (cur_idx, dc, dn, d_goal, actions_done choices); idx W-1: dc IS the goal distance
    "stay": (1, 1.5, 2.5, 3.5, (1, GIVE_UP - 1)),
    "adv_dc": (1, 0.5, 2.0, 3.5, (1,)),
    "adv_dn": (1, 2.0, 1.5, 3.5, (1,)),
    "give_up": (1, 1.5, 2.5, 3.5, (GIVE_UP,)),
    "last_wp": (W_PLAN - 1, None, None, 1.5, (3, FINAL_STEPS - 2)),
    "near": (1, 1.5, 2.5, 0.5, (1,)),
    "final": (W_PLAN - 1, None, None, 1.5, (FINAL_STEPS - 1,)),
    "clamped": (W_PLAN + 3, None, None, 1.5, (3, FINAL_STEPS - 1)),
}


def _build_inputs(case, d, j):
    """per-env inputs of launch j (without the plans) and their class labels"""
    rng = np.random.default_rng([ENVS.index(case.env), FORMS.index(case.form), case.n, case.idx, j])
    n_alloc, live, li = d["n_alloc"], d["live"], d["li"]
    act_cls, done_cls = _classes(case, d, j)
    mc = case.env == "mc"
    is_nav = np.array([c in NAV for c in act_cls])
    goal_env = np.array([c in ("goal", "both") for c in done_cls])
    tl_env = np.array([c in ("tl", "both") for c in done_cls])
    if mc:
        s0 = np.where(goal_env, 0.449 - rng.uniform(0, 0.005, n_alloc), rng.uniform(-1.0, 0.3, n_alloc))
        s1 = np.where(goal_env, rng.uniform(0.02, 0.04, n_alloc), rng.uniform(-0.03, 0.03, n_alloc))
    else:
        s0, s1 = rng.uniform(-2.5, 2.5, n_alloc), rng.uniform(-3.0, 3.0, n_alloc)
    steps = np.where(tl_env, MAX_STEPS - 1, np.where(li % 7 == 0, MAX_STEPS - 2, rng.integers(0, MAX_STEPS - 2, n_alloc)))
    A = rng.uniform(-0.9, 0.9, (n_alloc, N_SAMPLES, HORIZON)) * (1.0 if mc else 1.6)
    A[goal_env] = np.abs(A[goal_env])                                # MountainCar goal: positive action
    best = np.array([0, N_SAMPLES - 1, 2, 1, 3])[(li + j) % 5]
    actor = np.zeros(n_alloc)
    lim = 0.6 if mc else 0.25
    for c, v in (("inside", None), ("inside2", None), ("sat_lo", -3.0), ("sat_hi", 3.0), ("sat2_lo", -0.78), ("sat2_hi", 0.78)):
        sel = act_cls == c
        actor[sel] = rng.uniform(-lim, lim, int(sel.sum())) if v is None else v
    actor[goal_env & (act_cls == "inside")] = np.abs(actor[goal_env & (act_cls == "inside")])
    inp = dict(s0=_f32(s0), s1=_f32(s1), steps=steps.astype(np.int32), ep_ret=_f32(rng.uniform(-5, 5, n_alloc)),
               ou_x=_f32(rng.uniform(-0.15, 0.15, n_alloc)), mode=is_nav.astype(np.uint8),
               plan_of=(d["plan0"] + j * n_alloc + np.arange(n_alloc)).astype(np.int32),
               cur_idx=np.zeros(n_alloc, np.int32), start_idx=(1 + li % 2).astype(np.int32), actions_done=np.zeros(n_alloc, np.int32),
               A=_f32(A), best_idx=best.astype(np.int32), actor_out=_f32(actor))
    for i in np.nonzero(is_nav & live)[0]:
        idx, _, _, _, das = _NAV_GEOM[act_cls[i]]
        inp["cur_idx"][i] = idx
        inp["actions_done"][i] = das[(li[i] // 3 + j) % len(das)]
    # envs of no pair: patterns the kernel must leave alone (indices stay valid)
    dead = ~live
    inp["s0"][dead], inp["s1"][dead], inp["ep_ret"][dead], inp["ou_x"][dead] = 771.0, -772.0, 773.0, -774.0
    inp["steps"][dead], inp["cur_idx"][dead], inp["actions_done"][dead], inp["start_idx"][dead] = -7, -8, -9, -10
    inp["mode"][dead], inp["actor_out"][dead], inp["best_idx"][dead] = 0x5A, 775.0, 0
    inp["plan_of"][dead] = -11
    return inp, act_cls, done_cls


def _build_plans(case, d, j, inp, act_cls, x, rng):
    """the per-env plans of launch j: navigating envs get the geometry of their class around the new observation x"""
    dim = OBS[case.env]
    for i in np.nonzero(d["live"])[0]:
        q = int(inp["plan_of"][i])
        r = rng.uniform(MIN_RADIUS, 0.3, dim)
        wp = np.stack([x[i] + (3.5 + 0.3 * k) * r * _unit(rng, dim) for k in range(W_PLAN)])
        if act_cls[i] in NAV:
            idx, dc, dn, dg, _ = _NAV_GEOM[act_cls[i]]
            wp[W_PLAN - 1] = x[i] + dg * r * _unit(rng, dim)
            if dc is not None:
                wp[idx] = x[i] + dc * r * _unit(rng, dim)
                wp[idx + 1] = x[i] + dn * r * _unit(rng, dim)
        d["wp"][q * WMAX:q * WMAX + W_PLAN] = wp
        d["wp_len"][q] = W_PLAN
        d["radii"][q] = np.maximum(_f32(r), np.float32(MIN_RADIUS))


def _episode_plans(case, d, rng):
    """the published slots of every pair's window: a goal the reset states are close to about half of the time"""
    dim = OBS[case.env]
    for p in d["pairs"]:
        for k in range(p["count"]):
            q = p["slot0"] + (p["first"] + k) % p["slots"]
            if case.env == "mc":
                goal = np.array([-0.5 + rng.uniform(-0.04, 0.04), 0.0])
                r = np.array([0.05, 0.05])
            else:
                th = rng.uniform(-np.pi, np.pi)
                goal = np.array([np.cos(th), np.sin(th), 0.0])
                r = np.array([1.5, 1.5, 1.5])
            W = 3
            wp = np.stack([goal + 6.0 * r * _unit(rng, dim) for _ in range(W)])       # waypoint 0: far from every reset state
            wp[W - 1] = goal
            d["wp"][q * WMAX:q * WMAX + W] = wp
            d["wp_len"][q] = W
            d["radii"][q] = r


def _build(case, env_id0):
    d = _layout(case)
    d["env_id0"] = env_id0
    dim = OBS[case.env]
    S = d["n_slots"]
    # unpublished and guard slots: length 1, NaN geometry -- whoever reads them decides nothing
    d["wp"] = np.full((S * WMAX, dim), np.nan, np.float32)
    d["left"] = np.full(S * WMAX, np.nan, np.float32)
    d["wp_off"] = (np.arange(S) * WMAX).astype(np.int32)
    d["wp_len"] = np.ones(S, np.int32)
    d["radii"] = np.full((S, dim), np.nan, np.float32)
    rng = np.random.default_rng([ENVS.index(case.env), FORMS.index(case.form), case.n, case.idx, 99])
    _episode_plans(case, d, rng)
    d["steps"] = []
    for j in range(LAUNCHES):
        inp, act_cls, done_cls = _build_inputs(case, d, j)
        t = case.opts["t0"] + j
        a, _ = oracle_action(case, d, inp, t)
        s0, s1, _, _ = step64(case, inp["s0"], inp["s1"], a)
        _build_plans(case, d, j, inp, act_cls, observe64(case.env, s0, s1), rng)
        d["steps"].append(dict(inp=inp, act_cls=act_cls, done_cls=done_cls))
    for k in range(S):
        W = d["wp_len"][k]
        seg = d["wp"][k * WMAX:k * WMAX + W].astype(np.float64)
        if np.isfinite(seg).all():                                   # distances_left of the oracle: the scorer's column, unused here
            d["left"][k * WMAX:k * WMAX + W] = O.distances_left(seg, O.distance_func(d["radii"][k]))
    return d


def decision_margin(case, d):
    """the least margin of any decision of the case's three launches, in its own units (distance; position for the goal)"""
    worst = np.inf
    for j in range(LAUNCHES):
        e = _expected(case, d, j)
        worst = min(worst, e["margin"][d["live"]].min())
    return worst


@functools.lru_cache(maxsize=None)
def _case_data(name):
    case = CASE_BY_NAME[name]
    for attempt in range(200):
        d = _build(case, 1000 + 17 * attempt)
        if decision_margin(case, d) >= MARGIN and _census_ok(case, d):
            d["attempts"] = attempt + 1
            return d
    raise AssertionError("no env-id base gives %s its margins and census" % name)


def case_data(case):
    """static arrays (plan pool, pair table, env_id0) and the three launches' per-env inputs; read-only by convention"""
    return _case_data(case.name)


# ---------------------------------------------------------------------------------------------------- expected --
def _expected(case, d, j, act=None, obs2=None):
    inp = d["steps"][j]["inp"]
    live, n_alloc = d["live"], d["n_alloc"]
    t = case.opts["t0"] + j
    nav = _navigating(case, inp)
    a, ou = oracle_action(case, d, inp, t)
    a_used = a if act is None else np.where(live, _f64(act), a)
    s0, s1, rew, goal = step64(case, inp["s0"], inp["s1"], a_used)
    x2 = observe64(case.env, s0, s1)
    x_used = x2 if obs2 is None else np.where(live[:, None], _f64(obs2), x2)
    margin = np.full(n_alloc, np.inf)
    if case.env == "mc":
        margin = np.abs(x_used[:, 0] - float(np.float32(O.MC_GOAL_POSITION)))
        goal = x_used[:, 0] >= float(np.float32(O.MC_GOAL_POSITION))
    el = inp["steps"].astype(np.int64) + 1
    done = np.asarray(O.time_limit(goal, el, MAX_STEPS)) & live
    idx2, da2, at_goal, m_nav = bookkeeping(case, d, inp, x_used)
    margin = np.minimum(margin, m_nav)
    mode2 = nav & ~at_goal                                           # :336-339: the base agent takes over at the goal
    q, nav_new, m_new, r0, r1 = new_episodes(case, d, inp, done, t)
    margin = np.minimum(margin, m_new)
    ep_ret2 = inp["ep_ret"].astype(np.float64) + rew
    out = dict(j=j, t=t, navigating_in=nav & live, act=a, ou_x=np.where(done, 0.0, ou), obs=observe64(case.env, inp["s0"], inp["s1"]),
               obs2=x2, rew=rew, goal=goal & live, done=done, el=el, ret=ep_ret2, at_goal=at_goal & live,
               s0=np.where(done, r0, s0), s1=np.where(done, r1, s1), steps=np.where(done, 0, el), ep_ret=np.where(done, 0.0, ep_ret2),
               mode=np.where(done, nav_new, mode2) & live, new_plan=q,
               cur_idx=np.where(done, np.where(q >= 0, 0, inp["start_idx"]), idx2),
               actions_done=np.where(done, 0, da2), margin=np.where(live, margin, np.inf))
    return out


_EXPECTED = {}


def expected_step(case, j, act=None, obs2=None):
    """Everything launch j of the case writes, per env and in fp64 from the oracle's functions.  ``act`` / ``obs2``: teacher
    forcing -- the env step under the kernel's logged action, the bookkeeping and the goal test at its logged obs2."""
    d = case_data(case)
    if act is None and obs2 is None:
        if (case.name, j) not in _EXPECTED:
            _EXPECTED[case.name, j] = _expected(case, d, j)
        return _EXPECTED[case.name, j]
    return _expected(case, d, j, act, obs2)


def outcomes(case, d, j, e=None):
    """per env: the new-episode outcome label of a finishing env ('' otherwise)"""
    e = e if e is not None else _expected(case, d, j)
    out = np.array([""] * d["n_alloc"], dtype=object)
    for i in np.nonzero(e["done"])[0]:
        if case.form == "mpc":
            out[i] = "mpc_reset"
        elif d["pairs"][d["pair_of"][i]]["count"] == 0:
            out[i] = "pool_empty"
        else:
            out[i] = "coin_gt" if e["new_plan"][i] < 0 else ("new_nav" if e["mode"][i] else "new_close")
    return out


def census(case, d=None, envs=None):
    """class -> number of (env, launch) it occurs in, over the case's three launches (``envs``: a mask to count within)"""
    d = d if d is not None else case_data(case)
    envs = d["live"] if envs is None else envs & d["live"]
    c = {}

    def add(k, n=1):
        c[k] = c.get(k, 0) + int(n)
    for j in range(LAUNCHES):
        st = d["steps"][j]
        e = _expected(case, d, j) if "attempts" not in d else expected_step(case, j)
        oc = outcomes(case, d, j, e)
        for i in np.nonzero(envs)[0]:
            add(st["act_cls"][i])
            if st["act_cls"][i] in NAV and st["inp"]["best_idx"][i] in (0, N_SAMPLES - 1):
                add("best0" if st["inp"]["best_idx"][i] == 0 else "bestN1")
            if e["done"][i]:
                add(st["done_cls"][i])
                add(oc[i])
                add(st["done_cls"][i] + "*" + oc[i])
            if case.form != "mpc" and st["act_cls"][i] not in NAV:
                add("eps>0" if d["pairs"][d["pair_of"][i]]["eps"] > 0 else "eps<=0")
    return c


def required_classes(case):
    """the classes that apply to a case (those its options rule out are not listed)"""
    req = list(NAV) + ["best0", "bestN1"] + list(DONE_CLASSES[case.env])
    if case.form == "mpc":
        return req + ["mpc_reset"]
    req += list(BASE[case.env])
    pairs = pairs_of(case)
    req += ["eps>0"] if any(p["eps"] > 0 for p in pairs) else []
    req += ["eps<=0"] if any(p["eps"] <= 0 for p in pairs) else []
    if any(p["count"] == 0 for p in pairs):
        req.append("pool_empty")
    if any(p["count"] > 0 and p["eta"] < 1.0 and p["n_envs"] >= 64 for p in pairs):
        req.append("coin_gt")
    if any(p["count"] > 0 and p["eta"] > 0.0 and p["n_envs"] >= 64 for p in pairs):
        req += ["new_nav", "new_close"]
    return req


def _census_ok(case, d):
    if case.n < 64:
        return True
    c = census(case, d)
    if any(c.get(k, 0) < 4 for k in required_classes(case)):
        return False
    if case.n == 600:                                                # ... and in the first and the last workgroup
        i = np.arange(d["n_alloc"])
        for blk in (i < BLOCK, i >= 2 * BLOCK):
            cb = census(case, d, blk)
            if any(cb.get(k, 0) < 1 for k in required_classes(case)):
                return False
    return True


def census_line(case):
    c = census(case)
    o = case.opts
    opts = "log=%s ring=%s at_goal=%d stats=%d noise=%g mode_log=%d n_live=%d t0=%d k0=%d v1=%d ou_col=%d" % (
        o["log"], o["ring"], o["at_goal"], o["stats"], o["noise"], o["mode_log"], o["n_live"], o["t0"], o["k0"], o["v1"], o["ou_col"])
    pairs = " ".join("[n=%d eta=%g eps=%g pool=%d/%d+%d@%d]" % (p["n_envs"], p["eta"], p["eps"], p["count"], p["slots"], p["first"],
                                                               p["slot0"]) for p in pairs_of(case))
    inst = "mpc_rollout_step_kernel<%s%s>" % ({"mc": "McEnv", "pend": "PendEnv"}[case.env],
                                              {"mpc": "", "ss": ", true", "many": ", true, const ssc_smartstart_pair *"}[case.form])
    return "STEPCASE %s %s n=%d blocks=%d %s %s census=%s" % (case.name, inst, case.n, n_blocks(case), opts, pairs,
                                                               " ".join("%s:%d" % kv for kv in sorted(c.items())))


# ------------------------------------------------------------------------------------------- device state layout --
PER_ENV_REFRESH = ("s0", "s1", "steps", "ep_ret", "ou_x", "mode", "plan_of", "cur_idx", "start_idx", "actions_done", "A", "best_idx",
                   "actor_out")


def initial_device_state(case):
    """every array the entry point reads or writes, as it stands before the first launch (prefill patterns included)"""
    d = case_data(case)
    o = case.opts
    n_alloc, dim = d["n_alloc"], OBS[case.env]
    rows = log_rows(case)
    rs, ds, ms = strides(case)
    cap = ring_capacity(case)
    dev = dict(wp=d["wp"].copy(), left=d["left"].copy(), wp_off=d["wp_off"].copy(), wp_len=d["wp_len"].copy(), radii=d["radii"].copy(),
               at_goal=np.full(n_alloc, 0xAB, np.uint8), plan_state=np.full((n_alloc, dim), np.nan, np.float32),
               log_obs=np.full((dim, rows, rs), np.nan, np.float32), log_obs2=np.full((dim, rows, rs), np.nan, np.float32),
               log_act=np.full((rows, rs), np.nan, np.float32), log_rew=np.full((rows, rs), np.nan, np.float32),
               log_done=np.full((rows, ds), 0xCD, np.uint8), mode_log=np.full((rows, ms), 0xEE, np.uint8),
               ring_env_id=np.full(cap + 2, -5, np.int64), ring_length=np.full(cap + 2, -6, np.int32),
               ring_ret=np.full(cap + 2, np.nan, np.float32), ring_cursor=np.zeros(1, np.uint32),
               stats=np.zeros((len(d["pairs"]) + 1, 4), np.float64), d_t=np.array([o["t0"]], np.uint64),
               d_k=np.array([o["k0"]], np.int32), ticket=np.zeros(1, np.int32), n_live=np.array([12345], np.int32),
               eta=np.array([d["pairs"][0]["eta"]], np.float32), eps=np.array([d["pairs"][0]["eps"]], np.float32),
               pool=np.array([d["pairs"][0]["first"], d["pairs"][0]["count"], d["pairs"][0]["slots"]], np.int32))
    dev["stats"][-1] = -1.0                                          # the row behind the last pair's
    apply_inputs(case, 0, dev)
    return dev


def apply_inputs(case, j, dev):
    """refresh what launch j consumes (the schedule's per-env inputs); everything else lives on"""
    inp = case_data(case)["steps"][j]["inp"]
    for k in PER_ENV_REFRESH:
        dev[k] = inp[k].copy()


# ------------------------------------------------------------------------------------------------- float32 model --
MUTANTS = ("dn_dropped", "give_up_ge", "final_lt", "no_clamp", "goal_wp0", "no_handover", "ou_while_nav", "ou_not_reset",
           "eps_not_clamped", "one_scale", "best_ignored", "noise_env_key", "pick_no_mod", "pick_no_slot0", "newep_idx_start",
           "reset_t_plus_1", "plan_state_pre_reset", "mode_log_after", "time_limit_gt", "ring_len_after_reset", "dt_per_workgroup")
_SS_ONLY = ("no_handover", "ou_while_nav", "eps_not_clamped", "one_scale", "pick_no_mod", "pick_no_slot0", "newep_idx_start",
            "mode_log_after")


def mutant_applies(mutant, env, form):
    if mutant in _SS_ONLY and form == "mpc":
        return False
    if mutant == "one_scale":
        return env == "pend"                                         # the identity bounds of MountainCar scale to themselves
    if mutant == "pick_no_slot0":
        return form == "many"
    return True


def _fma(a, b, c):
    return (_f64(a) * _f64(b) + _f64(c)).astype(np.float32)


def _observe32(env, s0, s1):
    if env == "mc":
        return np.stack([s0, s1], axis=-1)
    return np.stack([np.cos(_f64(s0)).astype(np.float32), np.sin(_f64(s0)).astype(np.float32), s1], axis=-1)


def _ell32(x, y, inv_r):
    s = np.zeros(len(x), np.float32)
    with np.errstate(invalid="ignore"):
        for c in range(x.shape[1]):
            v = (x[:, c] - y[:, c]) * inv_r[:, c]
            s = _fma(v, v, s)
        return np.sqrt(s)


def _step32(case, s0, s1, a):
    f = np.float32
    if case.env == "mc":
        force = np.minimum(np.maximum(a, f(-1)), f(1))
        cosv = np.cos(_f64(f(3) * s0)).astype(np.float32)
        v = s1 + _fma(force, f(O.MC_BASE_POWER), f(-0.0025) * cosv)
        v = np.minimum(np.maximum(v, f(-0.07)), f(0.07))
        p = s0 + v
        p = np.minimum(np.maximum(p, f(-1.2)), f(0.6))
        v = np.where((p == f(-1.2)) & (v < 0), f(0), v)
        goal = p >= f(0.45)
        rew = np.where(goal, f(100), f(0)) - a * a * f(0.1)
        return p, v, rew.astype(np.float32), goal
    u = np.minimum(np.maximum(a, f(-2)), f(2))
    two_pi = f(6.28318530717958647692)
    y = s0 + f(np.pi)
    r = _fma(-two_pi, np.floor(y * (f(1) / two_pi)), y)
    r = np.where(r < 0, r + two_pi, r)
    r = np.where(r >= two_pi, r - two_pi, r)
    an = r - f(np.pi)
    cost = _fma(an, an, _fma(f(0.1) * s1, s1, f(0.001) * (u * u)))
    nd = _fma(_fma(f(15.0), np.sin(_f64(s0)).astype(np.float32), f(3.0) * u), f(0.05), s1)
    if case.opts["v1"]:
        nd = np.minimum(np.maximum(nd, f(-8)), f(8))
        nt = _fma(nd, f(0.05), s0)
    else:
        nt = _fma(nd, f(0.05), s0)
        nd = np.minimum(np.maximum(nd, f(-8)), f(8))
    return nt, nd, (-cost).astype(np.float32), np.zeros(len(a), bool)


def model_step(case, dev, mutant=None):
    """What one launch of mpc_rollout_step_kernel leaves of the device state ``dev`` (a dict as initial_device_state makes
    it), in float32 numpy, written from csrc/rollout.hip line by line; ``mutant``: one of MUTANTS.  Returns the new dict."""
    d = case_data(case)
    o = case.opts
    f = np.float32
    dev = {k: v.copy() for k, v in dev.items()}
    E = np.nonzero(d["live"])[0]
    ss = case.form != "mpc"
    t, k = int(dev["d_t"][0]), int(dev["d_k"][0])
    ids = np.uint64(d["env_id0"]) + E.astype(np.uint64)
    pids = np.uint64(PROBLEM_ID0) + E.astype(np.uint64)
    s0, s1 = dev["s0"][E], dev["s1"][E]
    el, ep_ret = dev["steps"][E].copy(), dev["ep_ret"][E].copy()
    obs = _observe32(case.env, s0, s1)
    idx, done_act = dev["cur_idx"][E].copy(), dev["actions_done"][E].copy()
    plan = dev["plan_of"][E]
    navigating = dev["mode"][E] != 0 if ss else np.ones(len(E), bool)
    mode_in = navigating.copy()
    ou_x = dev["ou_x"][E].copy() if ss else np.zeros(len(E), np.float32)
    rs, ds, ms = strides(case)
    # action
    best = np.zeros(len(E), np.int64) if mutant == "best_ignored" else dev["best_idx"][E]
    a_nav = dev["A"][E, best, 0]
    if o["noise"] != 0.0:
        g = (O.mpc_noise_gaussian(ENV_SEED, ids, t) if mutant == "noise_env_key" else O.mpc_noise_gaussian(NOISE_SEED, pids, t))
        a_nav = a_nav + f(o["noise"]) * g.astype(np.float32)
    a = a_nav
    if ss:
        eps = _pair_col(d, "eps", np.float32)[E]
        if mutant != "eps_not_clamped":
            eps = np.maximum(eps, f(0))
        noisy = (eps != 0) if mutant == "eps_not_clamped" else (eps > 0)
        g = O.ou_gaussian(ENV_SEED, ids, np.uint64(t)).astype(np.float32)
        ou_new = _fma(f(OU["sigma"]) * np.sqrt(f(OU["dt"])), g, _fma(f(OU["theta"]) * f(OU["dt"]), f(OU["mu"]) - ou_x, ou_x))
        moves = noisy & (~navigating | (mutant == "ou_while_nav"))
        ou_x = np.where(moves, ou_new, ou_x)
        ab = dev["actor_out"][E]
        ab = np.where(noisy, _fma(ou_x, eps, ab), ab)
        ab = np.minimum(np.maximum(ab, f(-1)), f(1))
        low, high = f(BOUNDS[case.env][0]), f(BOUNDS[case.env][1])
        for rep in range(1 if mutant == "one_scale" else 2):
            ab = np.minimum(np.maximum(ab, f(-1)), f(1))
            if not (low == -1 and high == 1):
                ab = _fma((ab + f(1)) * f(0.5), high - low, low)
        a = np.where(navigating, a_nav, ab).astype(np.float32)
    n0, n1, rew, goal = _step32(case, s0, s1, a)
    obs2 = _observe32(case.env, n0, n1)
    el = el + 1
    done = goal | ((el > MAX_STEPS) if mutant == "time_limit_gt" else (el >= MAX_STEPS))
    ep_ret = (ep_ret + rew).astype(np.float32)
    if o["log"] != "none":
        for c in range(obs.shape[1]):
            dev["log_obs"][c, k, E] = obs[:, c]
            dev["log_obs2"][c, k, E] = obs2[:, c]
        dev["log_act"][k, E], dev["log_rew"][k, E] = a, rew
        dev["log_done"][k, E] = done
    # the navigator's bookkeeping (mpc_device.h nav_observe_plan)
    wp = np.concatenate([dev["wp"], np.full((4 * WMAX, obs.shape[1]), np.nan, np.float32)])
    off, W = dev["wp_off"][plan].astype(np.int64), dev["wp_len"][plan].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_r = f(1) / dev["radii"][plan]
        da = done_act + 1
        ix = idx.astype(np.int64) if mutant == "no_clamp" else np.minimum(idx, np.maximum(W - 1, 0)).astype(np.int64)
        dc = _ell32(obs2, wp[off + ix], inv_r)
        dn = _ell32(obs2, wp[off + np.minimum(ix + 1, W - 1)], inv_r)
        near = _ell32(obs2, wp[off + (0 if mutant == "goal_wp0" else W - 1)], inv_r) <= f(THETA)
        move = ((dc <= f(THETA)) | ((dn <= dc) & (mutant != "dn_dropped"))) & (ix != W - 1)
    gave_up = (da >= GIVE_UP) if mutant == "give_up_ge" else (da > GIVE_UP)
    adv = move | (gave_up & (ix != W - 1))
    ix2 = np.where(adv, ix + 1, ix)
    da2 = np.where(adv, 0, da)
    final = (FINAL_STEPS < da2) if mutant == "final_lt" else (FINAL_STEPS <= da2)
    at_goal = navigating & (near | ((ix2 == W - 1) & final))
    idx = np.where(navigating, ix2, idx).astype(np.int32)
    done_act = np.where(navigating, da2, done_act).astype(np.int32)
    if o["at_goal"]:
        dev["at_goal"][E] = at_goal
    if ss and mutant != "no_handover":
        navigating = navigating & ~at_goal
    # episode ends
    r0, r1 = reset64(case, ids, t + 1 if mutant == "reset_t_plus_1" else t)
    r0, r1 = _f32(r0), _f32(r1)
    fin = np.nonzero(done)[0]
    if o["ring"] != "none":
        cap = ring_capacity(case)
        for i in fin:
            slot = int(dev["ring_cursor"][0])
            dev["ring_cursor"][0] += 1
            if slot < cap:
                dev["ring_env_id"][slot] = int(ids[i])
                dev["ring_length"][slot] = 0 if mutant == "ring_len_after_reset" else el[i]
                dev["ring_ret"][slot] = ep_ret[i]
    pre0, pre1 = n0.copy(), n1.copy()
    n0, n1 = np.where(done, r0, n0), np.where(done, r1, n1)
    el = np.where(done, 0, el)
    ep_ret = np.where(done, f(0), ep_ret)
    idx = np.where(done, dev["start_idx"][E], idx)
    done_act = np.where(done, 0, done_act)
    if not ss and o["ou_col"] and mutant != "ou_not_reset":
        dev["ou_x"][E[fin]] = 0
    if ss:
        if mutant != "ou_not_reset":
            ou_x = np.where(done, f(0), ou_x)
        navigating = navigating & ~done
        w = O.rng_words(ENV_SEED, ids, np.uint64(t), O.TAG_SS_EPISODE)
        first, count, slots, slot0 = (_pair_col(d, c, np.int64)[E] for c in ("first", "count", "slots", "slot0"))
        eta = _pair_col(d, "eta", np.float32)[E]
        take = done & (count > 0) & (O.u01(w[0]) <= eta)
        pick = first + w[1].astype(np.int64) % np.maximum(count, 1)
        if mutant != "pick_no_mod":
            pick = pick % slots
        q = pick + (0 if mutant == "pick_no_slot0" else slot0)
        q = np.where(take, q, 0)
        dev["plan_of"][E[take]] = q[take]
        if mutant != "newep_idx_start":
            idx = np.where(take, 0, idx)
        robs = _observe32(case.env, n0, n1)
        Wq = dev["wp_len"][q].astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            goal_wp = wp[dev["wp_off"][q].astype(np.int64) + (0 if mutant == "goal_wp0" else Wq - 1)]
            close = _ell32(robs, goal_wp, f(1) / dev["radii"][q]) <= f(THETA)
        navigating = np.where(take, ~close, navigating)
        dev["mode"][E] = navigating
        dev["ou_x"][E] = ou_x
        if o["mode_log"]:
            dev["mode_log"][k, E] = navigating if mutant == "mode_log_after" else mode_in
        if o["n_live"]:
            dev["n_live"][0] = 0
    dev["s0"][E], dev["s1"][E], dev["steps"][E], dev["ep_ret"][E] = n0, n1, el, ep_ret
    dev["cur_idx"][E], dev["actions_done"][E] = idx, done_act
    dev["plan_state"][E] = _observe32(case.env, pre0, pre1) if mutant == "plan_state_pre_reset" else _observe32(case.env, n0, n1)
    if o["stats"]:
        for y in range(len(d["pairs"])):
            m = d["pair_of"][E] == y
            dev["stats"][y] += [rew[m].astype(np.float64).sum(), goal[m].sum(), m.sum(), done[m].sum()]
    dev["d_t"][0] = t + (n_blocks(case) if mutant == "dt_per_workgroup" else 1)
    dev["d_k"][0] = k + 1
    return dev


def model_got(case, before, after):
    """the read-back dict check_step takes, from a model launch"""
    got = dict(after)
    got["before"] = before
    got["obs_before"] = _observe32(case.env, before["s0"], before["s1"])
    got["obs_after"] = _observe32(case.env, after["s0"], after["s1"])
    return got


# ----------------------------------------------------------------------------------------------------- checker --
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    assert np.asarray(a).shape == np.asarray(b).shape and np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b))), what


def _worst(report, key, err, tol):
    """record max(err / tol) under ``key`` and return whether every element passes"""
    err, tol = np.broadcast_arrays(_f64(err), _f64(tol))
    if err.size:
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
        frac = np.where(np.isnan(frac), np.inf, frac)
        report[key] = max(report.get(key, 0.0), float(frac.max()))
        return bool((frac <= 1.0).all())
    return True


def check_step(case, got, expected, report=None):
    """Hold the read-back ``got`` of launch expected['j'] (numpy arrays under the names of initial_device_state, plus
    'before': the same dict as it stood before the launch, 'obs_before' / 'obs_after' [n_alloc, OBS]: the observation of the
    state before / after the launch through the library's own observe) to ``expected`` = expected_step(case, j).
    ``report``: a dict that receives the worst error of every toleranced quantity as a fraction of its tolerance."""
    d = case_data(case)
    o = case.opts
    report = {} if report is None else report
    j = expected["j"]
    before = got["before"]
    live = d["live"]
    E = np.nonzero(live)[0]
    dead = ~live
    env, dim = case.env, OBS[case.env]
    ss = case.form != "mpc"
    k = o["k0"] + j
    has_log = o["log"] != "none"
    inp = d["steps"][j]["inp"]
    # -- counters
    assert int(got["d_t"][0]) == o["t0"] + j + 1, ("d_t", int(got["d_t"][0]), o["t0"] + j + 1)
    assert int(got["d_k"][0]) == k + 1, ("d_k", int(got["d_k"][0]))
    assert int(got["ticket"][0]) == 0, "ticket"
    if ss and o["n_live"]:
        assert int(got["n_live"][0]) == 0, "n_live"
    else:
        _same(got["n_live"], before["n_live"], "n_live untouched")
    # -- the read-only inputs
    for name in ("wp", "left", "wp_off", "wp_len", "radii", "A", "best_idx", "actor_out", "start_idx", "eta", "eps", "pool"):
        _same(got[name], before[name], name + " is an input")
    # -- teacher forcing: the env step under the logged action, the decisions at the logged obs2
    if has_log:
        act = np.zeros(d["n_alloc"], np.float32)
        act[:case.n] = got["log_act"][k, :case.n]
        obs2 = np.zeros((d["n_alloc"], dim), np.float32)
        obs2[:case.n] = got["log_obs2"][:, k, :case.n].T
        assert np.isfinite(act[E]).all() and np.isfinite(obs2[E]).all(), "log row k not written"
        tol_a = np.where(expected["navigating_in"], TOL_NAV_ACT, TOL_BASE_ACT[env])
        ok = _worst(report, "nav_action", np.abs(act - expected["act"])[expected["navigating_in"]], TOL_NAV_ACT)
        base = live & ~expected["navigating_in"]
        ok &= _worst(report, "base_action", np.abs(act - expected["act"])[base], TOL_BASE_ACT[env])
        assert ok, ("action", float(np.max(np.abs(act - expected["act"])[E] / tol_a[E])))
        tf = expected_step(case, j, act=act, obs2=obs2)
        assert tf["margin"][E].min() >= MARGIN / 2, ("a decision at the kernel's obs2 misses MARGIN / 2", float(tf["margin"][E].min()))
        for c in range(dim):
            assert _worst(report, "obs2[%d]" % c, np.abs(obs2[E, c] - tf["obs2"][E, c]), TOL_OBS2[env][c]), ("obs2", c)
        rew = got["log_rew"][k, E]
        assert _worst(report, "reward", np.abs(rew - tf["rew"][E]), REW_REL[env] * np.maximum(1.0, np.abs(tf["rew"][E]))), "reward"
        assert np.array_equal(got["log_done"][k, E], tf["done"][E].astype(np.uint8)), "log done"
        _same(got["log_obs"][:, k, :case.n].T[E], got["obs_before"][E], "log obs row == observation of the state before the launch")
        widen_s, widen_r = np.zeros(2), 0.0
        # every other row, and the row's columns of envs of no pair and behind n
        for name in ("log_obs", "log_obs2", "log_act", "log_rew", "log_done"):
            g, b = got[name], before[name]
            rows = [r for r in range(g.shape[-2]) if r != k]
            _same(g[..., rows, :], b[..., rows, :], name + " rows != k")
            cols = np.ones(g.shape[-1], bool)
            cols[E] = False
            _same(g[..., k, cols], b[..., k, cols], name + " row k outside the envs")
    else:
        tf = expected
        tol_a = np.where(expected["navigating_in"], TOL_NAV_ACT, TOL_BASE_ACT[env])
        widen_s = SENS_STATE[env][None, :] * tol_a[:, None]
        widen_r = SENS_REW[env] * np.abs(expected["act"]) * tol_a
        for name in ("log_obs", "log_obs2", "log_act", "log_rew", "log_done"):
            _same(got[name], before[name], name + " without a log")
    done = tf["done"]
    nd = live & ~done
    # -- exact
    assert np.array_equal(got["steps"][E], tf["steps"][E]), "steps"
    assert np.array_equal(got["cur_idx"][E], tf["cur_idx"][E]), ("cur_idx", np.nonzero(got["cur_idx"] != np.where(live, tf["cur_idx"], got["cur_idx"]))[0][:8])
    assert np.array_equal(got["actions_done"][E], tf["actions_done"][E]), "actions_done"
    if o["at_goal"]:
        assert np.array_equal(got["at_goal"][E], tf["at_goal"][E].astype(np.uint8)), "at_goal"
        _same(got["at_goal"][dead], before["at_goal"][dead], "at_goal outside the envs")
    else:
        _same(got["at_goal"], before["at_goal"], "at_goal NULL")
    for name in ("s0", "s1", "steps", "ep_ret", "cur_idx", "actions_done", "plan_state", "mode", "plan_of", "ou_x"):
        _same(got[name][dead], before[name][dead], name + " outside the envs")
    if ss:
        assert np.array_equal(got["mode"][E], tf["mode"][E].astype(np.uint8)), ("mode", np.nonzero(live & (got["mode"] != tf["mode"]))[0][:8])
        took = live & (tf["new_plan"] >= 0)
        assert np.array_equal(got["plan_of"][took], tf["new_plan"][took]), "plan_of of a new plan"
        _same(got["plan_of"][~took], before["plan_of"][~took], "plan_of of envs that took no new plan")
        if o["mode_log"]:
            assert np.array_equal(got["mode_log"][k, E], expected["navigating_in"][E].astype(np.uint8)), "mode_log row k"
            rows = [r for r in range(got["mode_log"].shape[0]) if r != k]
            _same(got["mode_log"][rows], before["mode_log"][rows], "mode_log rows != k")
            cols = np.ones(got["mode_log"].shape[1], bool)
            cols[E] = False
            _same(got["mode_log"][k, cols], before["mode_log"][k, cols], "mode_log row k outside the envs")
        else:
            _same(got["mode_log"], before["mode_log"], "mode_log absent")
        # OU state: moves only where the base agent acted with epsilon > 0; zero after an episode end
        eps = _pair_col(d, "eps")
        moved = nd & ~expected["navigating_in"] & (eps > 0)
        still = nd & ~moved
        _same(got["ou_x"][still], before["ou_x"][still], "ou_x of navigating envs / epsilon <= 0")
        assert _worst(report, "ou_x", np.abs(got["ou_x"][moved] - expected["ou_x"][moved]), TOL_OU), "ou_x"
        assert (got["ou_x"][done] == 0).all(), "ou_x after an episode end"
    else:
        _same(got["mode"], before["mode"], "mode (mpc form)")
        _same(got["plan_of"], before["plan_of"], "plan_of (mpc form)")
        _same(got["mode_log"], before["mode_log"], "mode_log (mpc form)")
        _same(got["ou_x"][~done], before["ou_x"][~done], "ou_x (mpc form)")
        if o["ou_col"]:
            assert (got["ou_x"][done] == 0).all(), "ou_x after an episode end (mpc form)"
        else:
            _same(got["ou_x"], before["ou_x"], "ou_x column not given")
    # -- state
    state = np.stack([got["s0"], got["s1"]], axis=-1)
    ref = np.stack([tf["s0"], tf["s1"]], axis=-1)
    for c in range(2):
        wid = widen_s[:, c][nd] if np.ndim(widen_s) == 2 else 0.0
        assert _worst(report, "state[%d]" % c, np.abs(state[nd, c] - ref[nd, c]), TOL_STATE[env][c] + wid), ("state", c)
    if env == "mc":
        assert np.array_equal(state[done], ref[done].astype(np.float32)), "MountainCar reset state"
    else:
        assert _worst(report, "pend_reset", np.abs(state[done] - ref[done]), TOL_RESET_PEND), "Pendulum reset state"
    if has_log:                                                      # the written-back state IS the logged obs2
        if env == "mc":
            _same(state[nd], obs2[nd], "state == logged obs2")
        else:
            _same(state[nd, 1], obs2[nd, 2], "theta-dot == logged obs2")
    _same(got["plan_state"][E], got["obs_after"][E], "plan_state == observation of the written-back state")
    ref_obs = observe64(env, tf["s0"], tf["s1"])
    tol_o = TOL_OBS2[env][None, :] + (np.max(widen_s, axis=1)[:, None] if np.ndim(widen_s) == 2 else 0.0)
    assert _worst(report, "plan_state", np.abs(got["plan_state"][E] - ref_obs[E]), (tol_o * np.ones((d["n_alloc"], 1)))[E]), "plan_state"
    tol_r = REW_REL[env] * np.maximum(1.0, np.maximum(np.abs(tf["rew"]), np.abs(tf["ret"]))) + widen_r
    assert _worst(report, "ep_ret", np.abs(got["ep_ret"][nd] - tf["ep_ret"][nd]), tol_r[nd]), "ep_ret"
    assert (got["ep_ret"][done] == 0).all(), "ep_ret after an episode end"
    # -- ring and statistics: what this launch adds to what the launches before it left
    fin = np.nonzero(done)[0]
    tol_fin = tol_r
    if o["ring"] != "none":
        cap = ring_capacity(case)
        c0 = int(before["ring_cursor"][0])
        assert int(got["ring_cursor"][0]) == c0 + len(fin), ("ring cursor", int(got["ring_cursor"][0]), c0, len(fin))
        nb, nw = min(cap, c0), min(cap, c0 + len(fin))
        seen = set()
        for name in ("ring_env_id", "ring_length", "ring_ret"):
            _same(got[name][nw:], before[name][nw:], name + " beyond the written slots")
            _same(got[name][:nb], before[name][:nb], name + " of earlier launches")
        for s in range(nb, nw):
            i = int(got["ring_env_id"][s]) - int(d["env_id0"])
            assert 0 <= i < d["n_alloc"] and done[i] and i not in seen, ("ring env id", s, i)
            seen.add(i)
            assert int(got["ring_length"][s]) == int(tf["el"][i]), ("ring length", s, i)
            assert _worst(report, "ring_ret", abs(float(got["ring_ret"][s]) - tf["ret"][i]), tol_fin[i]), ("ring ret", s, i)
        if cap >= c0 + len(fin):
            assert seen == set(int(i) for i in fin), "ring multiset"
    else:
        for name in ("ring_env_id", "ring_length", "ring_ret", "ring_cursor"):
            _same(got[name], before[name], name + " without a ring")
    if o["stats"]:
        for y in range(len(d["pairs"])):
            m = live & (d["pair_of"] == y)
            s = got["stats"][y] - before["stats"][y]
            assert s[1] == tf["goal"][m].sum() and s[2] == m.sum() and s[3] == done[m].sum(), ("stats[1..3]", y, s)
            tol0 = (REW_REL[env] * np.maximum(1.0, np.abs(tf["rew"][m])) + (widen_r[m] if np.ndim(widen_r) else 0.0)).sum()
            assert _worst(report, "stats[0]", abs(s[0] - tf["rew"][m].sum()), tol0), ("stats[0]", y)
        _same(got["stats"][-1], before["stats"][-1], "stats row behind the last pair")
    else:
        _same(got["stats"], before["stats"], "stats NULL")
    return report
