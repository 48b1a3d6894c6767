"""CPU half of the bf16 actor matrix (tests/actor_cases.py): the bound C_ACT * e rejects every listed way an actor kernel
goes wrong at every case, with a factor of two to spare, and the case / rollout lists cover exactly what actor_forward()
(csrc/actor.hip) and dispatch_policy() (csrc/rollout.hip) can launch.  numpy + oracle only: no GPU, no torch."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import actor_cases as AC

SMALLEST = {}


@pytest.mark.parametrize("llt", [True, False])
@pytest.mark.parametrize("name", AC.CASE_IDS)
def test_actor_bound_rejects_every_mutant(name, llt):
    """ref and emu pass the bound, every mutant of actor_cases.mutants() fails it, and C_ACT is at most half the smallest
    mutant's distance from the emulation in units of e.  Smallest over all cases with these inputs: 3.80 e (o3_224-128,
    last_layer_tanh, b1 of the last real layer-1 unit zeroed), then 3.91 e (o2_200-100, swapped W2 rows); at the shipped
    output init (o2_64-32_init) 12.8 e."""
    inp = AC.build_inputs(AC.case_by_name(name))
    ref, emu = AC.references(inp, llt)
    e = AC.bf16_error(ref, emu)
    assert ref.shape == emu.shape == (AC.ROWS, 1)
    assert AC.within_bound(AC.bound_ratios(emu, ref, emu, e)) and AC.within_bound(AC.bound_ratios(ref, ref, emu, e))
    ms = AC.mutants(inp, llt)
    names = {n.split("_rows_")[0] for n, _ in ms}
    want = {"swap_w2", "drop_l1_last", "zero_b1_last", "drop_l2_last", "zero_b2_last", "drop_l1_unit0", "drop_l2_unit0",
            "swap_obs_0_1", "tiles_exchanged"}
    want |= {"ignore_obs_2", "no_obs_clip"} if inp.case.obs_dim == 3 else set()
    want |= {"b2_not_scaled_by_c", "w3_sum_without_last"} if llt else set()
    assert names == want
    dist = {}
    for n, X in ms:
        r = AC.bound_ratios(X, ref, emu, e)
        assert not AC.within_bound(r), (name, llt, n, r)
        dist[n] = r[0]
    n_min = min(dist, key=dist.get)
    print(f"ACTMUTANT {name} llt={int(llt)} e={e:.3e} smallest={dist[n_min]:.2f} ({n_min})", flush=True)
    assert AC.C_ACT <= 0.5 * dist[n_min], (name, llt, n_min, dist[n_min])
    SMALLEST[(name, llt)] = dist[n_min]


def test_actor_smallest_mutant_ratio():
    """the figure NOTEBOOK quotes (runs after the cases above in file order; on its own it recomputes them)"""
    if len(SMALLEST) < 2 * len(AC.CASES):
        for c in AC.CASES:
            for llt in (True, False):
                inp = AC.build_inputs(c)
                ref, emu = AC.references(inp, llt)
                SMALLEST[(c.name, llt)] = min(AC.bound_ratios(X, ref, emu)[0] for _, X in AC.mutants(inp, llt))
    k = min(SMALLEST, key=SMALLEST.get)
    print(f"ACTMUTANT smallest ratio over all cases: {SMALLEST[k]:.2f} at {k}", flush=True)
    assert AC.C_ACT <= 0.5 * SMALLEST[k]


def test_actor_cases_condition_the_edges_and_the_inputs():
    for c in AC.CASES:
        inp = AC.build_inputs(c)
        w = inp.w
        assert w["b1"][0] == w["b1"][c.h1 - 1] == np.float32(0.5) and w["b2"][c.h2 - 1] == np.float32(0.3)
        assert w["b2"][0] == np.float32(0.4 if c.h2 > 1 else 0.3)
        assert w["W3"][c.h2 - 1, 0] == np.float32(-c.w3_scale) and (c.h2 == 1 or w["W3"][0, 0] == np.float32(c.w3_scale))
        assert inp.obs.shape == (AC.ROWS, c.obs_dim) and inp.obs.dtype == np.float32
        if c.obs_dim == 2:
            assert inp.obs_clip is None and np.abs(inp.obs).max() <= 1.2
        else:
            assert inp.obs_clip == AC.OBS_CLIP
            AC.assert_inputs_reach_the_clip(inp.obs)
            assert np.abs(inp.obs[:, :2]).max() <= 1.0 and 5.0 < np.abs(inp.obs[:, 2]).max() <= 8.0
        # the swapped pair is live and crosses a group of 4
        h = AC.hidden1(inp)
        u, v = AC.swap_pair(h, w["W2"].astype(np.float64))
        assert u // 4 != v // 4 and (h[:, u] > 0).mean() >= 0.25 and (h[:, v] > 0).mean() >= 0.25


def test_actor_cases_cover_the_dispatch_of_actor_forward():
    """actor_forward() restated: LDS beyond 128-64, "small" up to 64-32, <O,4,2> between; obs_dim 2 or 3.  Every case's
    declared kernel is what that gives, all six kernels are there, with every ragged edge of their tiles."""
    for c in AC.CASES:
        assert AC.standalone_kernel(c.obs_dim, c.h1, c.h2) == c.kernel, c
    assert {c.kernel for c in AC.CASES} == {f"actor_mfma_kernel<{o},{t}>" for o in (2, 3) for t in ("2,1", "4,2")} | \
        {f"actor_mfma_lds_kernel<{o},7,4>" for o in (2, 3)}
    shapes = {o: {(c.h1, c.h2) for c in AC.CASES if c.obs_dim == o} for o in (2, 3)}
    for o in (2, 3):
        assert shapes[o] >= {(64, 32), (48, 24), (37, 19), (33, 1), (128, 64), (65, 33), (64, 33), (65, 32), (200, 100),
                             (224, 128), (129, 65), (128, 65), (129, 64)}
    assert any(c.w3_scale == 3e-3 and (c.obs_dim, c.h1, c.h2) == (2, 64, 32) for c in AC.CASES)
    # either side of both thresholds, in each dimension
    assert AC.standalone_kernel(2, 64, 32).endswith("<2,2,1>") and AC.standalone_kernel(2, 65, 32).endswith("<2,4,2>")
    assert AC.standalone_kernel(2, 64, 33).endswith("<2,4,2>") and AC.standalone_kernel(3, 128, 64).endswith("<3,4,2>")
    assert AC.standalone_kernel(3, 129, 64).startswith("actor_mfma_lds") and AC.standalone_kernel(3, 128, 65).startswith("actor_mfma_lds")
    assert AC.STANDALONE_M == (1, 33, 64, 65, 321) and AC.ROWS == 321
    with pytest.raises(AssertionError):
        AC.standalone_kernel(2, 225, 128)


def test_rollout_runs_cover_the_dispatch_of_dispatch_policy():
    """dispatch_policy() + mc_fused_policy() restated (actor_cases.rollout_policy): every run's declared policy class is
    what the predicates give for its settings, the declared set IS the reachable set, and the branches inside one class
    that the flat-tolerance tests never took are each there."""
    R = AC.ROLLOUTS
    for r in R:
        _, obs_dim, _, low, high = AC.ENV_OF[r.env]
        eps = 1.0 if r.eps == "host" else 0.0
        inst = AC.rollout_policy(obs_dim, r.precision, r.h1, r.h2, r.llt, low, high, eps, r.eps in AC.DEV_EPS, r.obs_clip, r.norm)
        assert inst == r.inst, (r.name, inst)
        assert not r.ln or r.precision == "f32"
    assert {r.inst for r in R} == AC.REACHABLE_POLICIES and len(AC.REACHABLE_POLICIES) == 2 + 8 + 4 + 12
    fused = [r for r in R if r.inst.startswith("ActorPolicyFused")]
    assert {r.eps for r in fused} >= {"host", "dev+", "dev0", "dev-"}                  # d_ou_epsilon: > 0, 0, clamped
    assert {(r.h1, r.h2) for r in fused} >= {(64, 32), (48, 24), (37, 19)}             # ragged sizes
    assert any(r.w3_scale == 3e-3 for r in fused)                                      # the shipped output init
    generic_mc = [r for r in R if r.inst == "ActorPolicy<ActorMfma<2,2,1,2>,false>"]
    assert any(r.obs_clip == 1.0 and r.eps != "none" for r in generic_mc)              # routed there by a clip that acts
    assert any(r.eps == "none" for r in generic_mc)
    for net in ("ActorMfma<", "ActorMfmaLds<"):
        assert {r.llt for r in R if net in r.inst} == {True, False}
        assert {r.env for r in R if net in r.inst} == {"mc", "pend"}
        assert {bool(r.norm) for r in R if net in r.inst} == {True, False}
    f32 = [r for r in R if r.precision == "f32"]
    assert any(r.ln for r in f32) and any(r.norm for r in f32) and any(not r.ln and not r.norm for r in f32)
    assert {r.norm for r in R} == {None, "wide", "floor"}
    # the predicates at their edges
    P = AC.rollout_policy
    assert P(2, "bf16_mfma", 64, 32, True, -1.0, 1.0, 1.0, False, 1.2, None).startswith("ActorPolicyFused")
    assert P(2, "bf16_mfma", 64, 32, True, -1.0, 1.0, 1.0, False, 1.19, None).startswith("ActorPolicy<ActorMfma<2,2,1,2>")
    assert P(2, "bf16_mfma", 64, 32, True, -1.0, 1.0, 1.0, False, 1.0, "wide") == "ActorPolicyFused<true,true>"
    assert P(2, "bf16_mfma", 64, 32, True, -1.0, 1.0, 0.0, False, 0.0, None).startswith("ActorPolicy<ActorMfma<2,2,1,2>")
    assert P(2, "bf16_mfma", 64, 32, True, -1.0, 1.0, 0.0, True, 0.0, None).startswith("ActorPolicyFused")
    assert P(2, "bf16_mfma", 64, 32, True, -2.0, 2.0, 1.0, False, 0.0, None).startswith("ActorPolicy<ActorMfma<2,2,1,2>")
    assert P(3, "bf16_mfma", 64, 32, True, -1.0, 1.0, 1.0, False, 0.0, None).startswith("ActorPolicy<ActorMfma<3,2,1,2>")
    assert P(2, "bf16_mfma", 65, 32, True, -1.0, 1.0, 1.0, False, 0.0, None).startswith("ActorPolicy<ActorMfma<2,4,2,2>")
    assert P(2, "bf16_mfma", 128, 65, True, -1.0, 1.0, 1.0, False, 0.0, None).startswith("ActorPolicy<ActorMfmaLds<2,7,4,2>")
    assert AC.ROLLOUT_N == (1, 33, 321) and (AC.ROLLOUT_K, AC.ROLLOUT_T0) == (11, 3)
    assert (AC.ROLLOUT_T0 + AC.ROLLOUT_K) % 4 == 2 and AC.ROLLOUT_T0 % 4 == 3          # head 1, two groups of 4, tail 2


def test_oracle_rollouts_keep_half_the_steps_inside_the_clip():
    """The condition on w3_scale, from the oracle alone (the GPU test asserts it on the run itself): at the run's start
    states, with an OU path of ROLLOUT_K steps from 0, the oracle's logged action stays strictly inside the bounds -- where
    it still carries the network -- on well over half of all env-steps."""
    for r in AC.ROLLOUTS:
        if r.precision == "random":
            continue
        _, obs_dim, _, low, high = AC.ENV_OF[r.env]
        n = 321
        w = AC.rollout_weights(r)
        s0, s1 = AC.initial_state(r, n)
        obs = np.stack([s0, s1], 1) if r.env == "mc" else np.stack([np.cos(s0), np.sin(s0), s1], 1)
        x = obs.astype(np.float64)
        if r.norm:
            x = AC.x_hat64(obs, *AC.host_mean_std(AC.rollout_stat_rows(r)), r.obs_clip)
        ln = ((w["ln1_g"], w["ln1_b"]), (w["ln2_g"], w["ln2_b"])) if r.ln else None
        net = O.actor_forward(x, **{k: w[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")}, last_layer_tanh=r.llt,
                              layer_norm=ln, obs_clip=r.obs_clip or None)[:, 0]
        eps = AC.DEV_EPS.get(r.eps, 1.0 if r.eps == "host" else 0.0)
        rng, ou, inside = np.random.default_rng(7), np.zeros(n), []
        for _ in range(AC.ROLLOUT_K):
            ou = O.ou_step(ou, rng.normal(size=n), 0.4, 0.6)
            inside.append(np.abs(O.ddpg_action(net, ou, eps, low, high)) < high)
        assert np.mean(inside) >= 0.6, (r.name, float(np.mean(inside)))
