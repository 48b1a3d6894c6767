"""The bf16 MFMA actor (csrc/actor.hip, csrc/actor_device.h, the actor policies of csrc/rollout.hip): the case list, each
case's weights and inputs, its fp64 reference and the emulation of the kernels' arithmetic, the bound derived from the two,
the emulation mutants that bound must reject, and the fused-rollout runs with the dispatch restated as predicates.  Shared
by the CPU tests (tests/test_actor_cases_cpu.py) and the GPU tests (tests/test_gpu_actor_matrix.py); numpy + oracle only.

The bound.  ``ref`` = O.actor_forward in fp64, ``emu`` = O.actor_forward_bf16emu(fold=True): layer 1 exact, hidden
activations rounded to bf16, and under last_layer_tanh the constant c = 2 log2(e) of the kernels' tanh folded into W2 and b2
BEFORE the bf16 conversion.  e = max |emu - ref| over the compared rows is what the bf16 arithmetic alone costs at this
case's inputs; a result X is accepted when

    max |X - emu| <= C_ACT * e        and        max |X - ref| <= (1 + C_ACT) * e

on the network's output (the unit action scale).  In a rollout the compared quantity is the logged action
scale(scale(clip(net + noise))) and e is taken on the oracle's logged actions themselves: on MountainCar's bounds that is the
unit scale; on Pendulum's (+-2) scale(scale(a)) = 2 clip(2 a), so a logged action strictly inside the bounds moves by FOUR
times what the network moves -- ((high - low) / 2) squared, not (high - low) / 2 (at which the emulation itself would sit
exactly on the fp64 side of the bound) -- and e carries that factor with it.  C_ACT = 1: "the kernel is closer to its arithmetic model
than the model is to fp64".  There is no flat number in it.  Every mutant of ``mutants()`` sits more than 2 * C_ACT * e
from the emulation at every case (asserted on the CPU), so C_ACT has a factor of two of room below the smallest wrong
kernel the list describes.

Not in the list: truncation instead of round-to-nearest-even in the bf16 conversions.  It moves the output by 0.9-2.4 e,
which a bound that is itself one rounding error wide cannot separate from an honest kernel.

Weights.  gpu_util.actor_weights, then the edges conditioned: unit 0 and the last real unit of both hidden layers get a
positive bias and a full-size outgoing weight, because a dead (or weightless) tail unit hides its own loss.
"""
import zlib
from collections import namedtuple

import numpy as np

from oracle import ssc_oracle as O
from tests.gpu_util import actor_weights

C_ACT = 1.0
OBS_CLIP = 5.0                      # DDPG's observation_range; acts on Pendulum's theta-dot (|.| <= 8), inert on MountainCar
ROWS = 321                          # a block (256) plus a wave (64) plus one
STANDALONE_M = (1, 33, 64, 65, 321)  # tile 0 only / one env in tile 1 / a full wave / a one-lane second wave / all rows

# name, obs_dim, h1, h2, w3_scale and the standalone instantiation actor_forward() selects for it; the fused rollout's
# ActorMfma<O,UT,JT,2> / ActorMfmaLds<O,7,4,2> / ActorMfma2 follow the same size classes (rollout_policy() below)
ActorCase = namedtuple("ActorCase", "name obs_dim h1 h2 w3_scale kernel")


def _cases():
    out = []
    for h1, h2 in [(64, 32), (48, 24), (37, 19), (33, 1)]:
        for o in (2, 3):
            out.append(ActorCase(f"o{o}_{h1}-{h2}", o, h1, h2, 0.4, f"actor_mfma_kernel<{o},2,1>"))
    out.append(ActorCase("o2_64-32_init", 2, 64, 32, 3e-3, "actor_mfma_kernel<2,2,1>"))   # the shipped output init
    for h1, h2 in [(128, 64), (65, 33), (64, 33), (65, 32)]:        # 65-33: one unit into the second tile of each layer
        for o in (2, 3):
            out.append(ActorCase(f"o{o}_{h1}-{h2}", o, h1, h2, 0.4, f"actor_mfma_kernel<{o},4,2>"))
    for h1, h2 in [(200, 100), (224, 128), (129, 65), (128, 65), (129, 64)]:   # 129-65: the smallest shape routed to LDS
        for o in (2, 3):
            out.append(ActorCase(f"o{o}_{h1}-{h2}", o, h1, h2, 0.4, f"actor_mfma_lds_kernel<{o},7,4>"))
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def standalone_kernel(obs_dim, h1, h2):
    """actor_forward() of csrc/actor.hip, precision SSC_PREC_BF16_MFMA, act_dim 1"""
    assert obs_dim in (2, 3) and h1 <= 224 and h2 <= 128, "SSC_EUNSUPPORTED"
    if h1 > 128 or h2 > 64:
        return f"actor_mfma_lds_kernel<{obs_dim},7,4>"
    small = h1 <= 64 and h2 <= 32
    return f"actor_mfma_kernel<{obs_dim},2,1>" if small else f"actor_mfma_kernel<{obs_dim},4,2>"


def condition_weights(w, w3_scale):
    """unit 0 and the last real unit of both hidden layers carry something on every row"""
    w = {k: np.array(v, np.float32) for k, v in w.items()}
    h1, h2 = w["W2"].shape
    w["b1"][0] = w["b1"][h1 - 1] = 0.5
    w["b2"][0] = 0.4
    w["b2"][h2 - 1] = 0.3
    w["W3"][0, 0] = w3_scale
    w["W3"][h2 - 1, 0] = -w3_scale
    return w


def make_obs(rng, obs_dim, rows):
    """uniform, different in every row and component: MountainCar's range for 2 components, (cos, sin, theta-dot) with
    |theta-dot| <= 8 for 3, so that OBS_CLIP acts on some rows"""
    if obs_dim == 2:
        return rng.uniform(-1.2, 1.2, size=(rows, 2)).astype(np.float32)
    th, thd = rng.uniform(-np.pi, np.pi, rows), rng.uniform(-8.0, 8.0, rows)
    return np.stack([np.cos(th), np.sin(th), thd], axis=1).astype(np.float32)


def assert_inputs_reach_the_clip(x, obs_clip=OBS_CLIP):
    """conditions on the INPUTS of a clip case: something beyond +clip and beyond -clip, at least half the rows clear"""
    x = np.asarray(x, np.float64)
    assert (x > obs_clip).any() and (x < -obs_clip).any()
    assert np.mean((np.abs(x) < obs_clip).all(axis=1)) >= 0.5


ActorInputs = namedtuple("ActorInputs", "case w obs obs_clip")


def build_inputs(case):
    """Deterministic weights and ROWS observations of a case.  obs_clip: OBS_CLIP where it can act (3 components), else None."""
    seed = zlib.crc32(case.name.encode())
    w = condition_weights(actor_weights(case.obs_dim, case.h1, case.h2, seed=seed, w3_scale=case.w3_scale), case.w3_scale)
    obs = make_obs(np.random.default_rng(seed + 1), case.obs_dim, ROWS)
    clip = OBS_CLIP if case.obs_dim == 3 else None
    if clip:
        assert_inputs_reach_the_clip(obs, clip)
    assert len(np.unique(obs)) >= obs.size - 2
    return ActorInputs(case, w, obs, clip)


def forward_ref(x, w, llt, obs_clip=None):
    return O.actor_forward(x, **w, last_layer_tanh=llt, obs_clip=obs_clip)


def forward_emu(x, w, llt, obs_clip=None):
    return O.actor_forward_bf16emu(x, **w, last_layer_tanh=llt, obs_clip=obs_clip, fold=True)


def references(inp, llt, x=None):
    """(ref, emu) at the case's observations, or at ``x`` (normalised inputs: ref sees the fp64 values, the emulation what
    fp32 holds of them)"""
    x = inp.obs if x is None else x
    return forward_ref(x, inp.w, llt, inp.obs_clip), forward_emu(x, inp.w, llt, inp.obs_clip)


def bf16_error(ref, emu):
    """e of a case: over ALL its compared rows (the e the CPU test proves the mutants' distances against).  A launch of
    fewer rows is held to the same e on its rows: over a single row |emu - ref| can be anything down to exactly 0 (33-1
    with the one ReLU unit off), which says nothing about what the arithmetic costs."""
    e = float(np.max(np.abs(emu - ref)))
    assert e > 0
    return e


def bound_ratios(X, ref, emu, e=None, rows=None):
    """(max |X - emu| / e, max |X - ref| / e) over ``rows`` (a slice or a mask; default all)"""
    e = bf16_error(ref, emu) if e is None else e
    sl = slice(None) if rows is None else rows
    X, ref, emu = np.asarray(X, np.float64)[sl], ref[sl], emu[sl]
    assert np.isfinite(X).all()
    return float(np.max(np.abs(X - emu))) / e, float(np.max(np.abs(X - ref))) / e


def within_bound(r, c=C_ACT, extra=0.0):
    """``extra``: an absolute allowance in units of e (the fp32 action tolerance of a noisy rollout, divided by e)"""
    return r[0] <= c + extra and r[1] <= 1.0 + c + extra


def hidden1(inp):
    """fp64 layer-1 activations at the case's (clipped) inputs"""
    x = O.clip_observation(inp.obs, inp.obs_clip)
    return np.maximum(x @ inp.w["W1"].astype(np.float64) + inp.w["b1"].astype(np.float64), 0.0)


def swap_pair(act, W_out):
    """two live units whose exchange matters, NOT in the same group of 4 (a k-slot slip crosses groups): among the 16 most
    often active ones, the pair with the largest mean |h_u - h_v| * max |W_out[u] - W_out[v]| (from the data, not by index)"""
    frac = (act > 0).mean(axis=0)
    live = [int(u) for u in np.argsort(-frac, kind="stable") if frac[u] >= 0.25][:16]
    best, pair = -1.0, None
    for i, u in enumerate(live):
        for v in live[i + 1:]:
            if u // 4 == v // 4:
                continue
            s = np.mean(np.abs(act[:, u] - act[:, v])) * np.max(np.abs(W_out[u] - W_out[v]))
            if s > best:
                best, pair = s, (min(u, v), max(u, v))
    assert pair is not None, "fewer than two live hidden units in different groups"
    return pair


def mutants(inp, llt):
    """The ways an actor kernel goes wrong, as (name, output of an emulation that computes the wrong thing): a k-slot
    permutation slip (W2 rows of two live layer-1 units swapped), padding / tail slips (the last real unit of either hidden
    layer dropped, or its bias), unit 0 of either layer dropped, observation components swapped, the odd k-step of the
    32x32x2 layer 1 lost (component 2 ignored), the tanh fold's slips (b2 not scaled by c; the b3 + sum W3 term without its
    last real j), the two 32-env tiles of a wave exchanged, the observation clip not applied."""
    w, obs, clip = inp.w, inp.obs, inp.obs_clip
    h1, h2 = w["W2"].shape
    out = []

    def emu_with(obs=obs, clip=clip, **edits):
        w2 = {k: v.copy() for k, v in w.items()}
        for k, f in edits.items():
            f(w2[k])
        return forward_emu(obs, w2, llt, clip)

    def zero(i):
        def f(a):
            a[i] = 0.0
        return f

    u, v = swap_pair(hidden1(inp), w["W2"].astype(np.float64))

    def swap(a):
        a[[u, v]] = a[[v, u]]
    out.append((f"swap_w2_rows_{u}_{v}", emu_with(W2=swap)))
    out.append(("drop_l1_last", emu_with(W2=zero(h1 - 1))))
    out.append(("zero_b1_last", emu_with(b1=zero(h1 - 1))))
    out.append(("drop_l2_last", emu_with(W3=zero(h2 - 1))))
    out.append(("zero_b2_last", emu_with(b2=zero(h2 - 1))))
    out.append(("drop_l1_unit0", emu_with(W2=zero(0))))
    out.append(("drop_l2_unit0", emu_with(W3=zero(0))))
    out.append(("swap_obs_0_1", emu_with(obs=obs[:, [1, 0] + list(range(2, obs.shape[1]))])))
    if obs.shape[1] == 3:
        out.append(("ignore_obs_2", emu_with(W1=zero(2))))
    if llt:
        c = O.ACTOR_TANH_FOLD

        def unscale(b):                      # the folded model adds b2 where it should add b2 * c
            b /= c
        out.append(("b2_not_scaled_by_c", emu_with(b2=unscale)))

        def short_sum(b):                    # b3 + sum_j W3[j] stops one real j early
            b -= w["W3"][h2 - 1, 0]
        out.append(("w3_sum_without_last", emu_with(b3=short_sum)))
    emu = forward_emu(obs, w, llt, clip)
    idx = np.arange(obs.shape[0]) ^ 32
    idx = np.where(idx < obs.shape[0], idx, np.arange(obs.shape[0]))
    out.append(("tiles_exchanged", emu[idx]))
    if clip:
        out.append(("no_obs_clip", emu_with(clip=None)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The fused rollout: dispatch_policy() + mc_fused_policy() of csrc/rollout.hip restated, and one run per reachable policy
# instantiation (and per branch inside one that today's tests never take).
# ---------------------------------------------------------------------------------------------------------------------
MC_OBS_BOUND = 1.2          # max(|min_position|, |max_position|, max_speed) of MountainCar


def rollout_policy(obs_dim, precision, h1, h2, llt, low, high, eps, dev_eps, obs_clip, norm):
    """The policy class dispatch_policy() launches.  eps: the host epsilon; dev_eps: epsilon comes in a device tensor."""
    n = "true" if norm else "false"
    if precision == "random":
        return f"RandomPolicy<{obs_dim}>"
    if precision == "f32":
        assert (h1, h2) in ((64, 32), (64, 64)), "SSC_EUNSUPPORTED"
        return f"ActorPolicy<ActorF32<{obs_dim},{h1},{h2}>,{n}>"
    assert precision == "bf16_mfma"
    if obs_dim == 2:
        clip_inert = not (obs_clip and obs_clip > 0) or obs_clip >= MC_OBS_BOUND
        if h1 <= 64 and h2 <= 32 and low == -1.0 and high == 1.0 and (eps > 0 or dev_eps) and (clip_inert or norm):
            return f"ActorPolicyFused<{'true' if llt else 'false'},{n}>"
    if h1 <= 64 and h2 <= 32:
        return f"ActorPolicy<ActorMfma<{obs_dim},2,1,2>,{n}>"
    if h1 <= 128 and h2 <= 64:
        return f"ActorPolicy<ActorMfma<{obs_dim},4,2,2>,{n}>"
    assert h1 <= 224 and h2 <= 128, "SSC_EUNSUPPORTED"
    return f"ActorPolicy<ActorMfmaLds<{obs_dim},7,4,2>,{n}>"


REACHABLE_POLICIES = (
    {f"RandomPolicy<{o}>" for o in (2, 3)}
    | {f"ActorPolicy<ActorF32<{o},64,{h2}>,{n}>" for o in (2, 3) for h2 in (32, 64) for n in ("true", "false")}
    | {f"ActorPolicyFused<{t},{n}>" for t in ("true", "false") for n in ("true", "false")}
    | {f"ActorPolicy<{net},{n}>" for o in (2, 3) for n in ("true", "false")
       for net in (f"ActorMfma<{o},2,1,2>", f"ActorMfma<{o},4,2,2>", f"ActorMfmaLds<{o},7,4,2>")})

# env: "mc" | "pend".  eps: "host" (ou_epsilon 1), "none" (ou_epsilon 0: no noise path), "dev+" / "dev0" / "dev-"
# (d_ou_epsilon holding 0.7 / 0 / -0.5).  norm: None | "wide" | "floor" (gpu_util.rms_edge_stats).  ln: LayerNorm (fp32 only).
RolloutRun = namedtuple("RolloutRun", "name env precision h1 h2 llt eps obs_clip norm ln w3_scale inst")
DEV_EPS = {"dev+": 0.7, "dev0": 0.0, "dev-": -0.5}
# the logged action is clip(net + eps * ou_x) -- through scale(scale(.)), which on Pendulum's bounds is 2 clip(2 a): the network
# shows only while |a| < 0.5 there -- so the output layer is scaled to keep at least half of all steps clear of the clip
W3_SCALE_OF = {"mc": 0.2, "pend": 0.05}


def _r(name, env, precision, h1, h2, llt, eps, obs_clip, norm, inst, ln=False, w3_scale=None):
    w3_scale = w3_scale or W3_SCALE_OF[env]
    return RolloutRun(name, env, precision, h1, h2, llt, eps, obs_clip, norm, ln, w3_scale, inst)


ROLLOUTS = [
    # ---- the straight-line fused policy (MountainCar, h1 <= 64, h2 <= 32, unit bounds, noise on) ---------------------
    _r("fused_64-32", "mc", "bf16_mfma", 64, 32, True, "host", 0.0, None, "ActorPolicyFused<true,false>"),
    _r("fused_64-32_relu", "mc", "bf16_mfma", 64, 32, False, "host", 5.0, None, "ActorPolicyFused<false,false>"),
    _r("fused_64-32_norm", "mc", "bf16_mfma", 64, 32, True, "host", 5.0, "wide", "ActorPolicyFused<true,true>"),
    _r("fused_64-32_relu_norm", "mc", "bf16_mfma", 64, 32, False, "host", 5.0, "floor", "ActorPolicyFused<false,true>"),
    _r("fused_48-24_dev+", "mc", "bf16_mfma", 48, 24, True, "dev+", 5.0, None, "ActorPolicyFused<true,false>"),
    _r("fused_37-19_dev0", "mc", "bf16_mfma", 37, 19, True, "dev0", 0.0, None, "ActorPolicyFused<true,false>"),
    _r("fused_37-19_dev-_relu", "mc", "bf16_mfma", 37, 19, False, "dev-", 0.0, None, "ActorPolicyFused<false,false>"),
    _r("fused_48-24_norm_floor", "mc", "bf16_mfma", 48, 24, True, "dev+", 5.0, "floor", "ActorPolicyFused<true,true>"),
    _r("fused_64-32_init", "mc", "bf16_mfma", 64, 32, True, "host", 0.0, None, "ActorPolicyFused<true,false>", w3_scale=3e-3),
    # ---- ActorMfma<OBS,2,1,2> ----------------------------------------------------------------------------------------
    _r("mfma21_mc_nonoise", "mc", "bf16_mfma", 64, 32, True, "none", 0.0, None, "ActorPolicy<ActorMfma<2,2,1,2>,false>"),
    _r("mfma21_mc_clip1", "mc", "bf16_mfma", 64, 32, True, "host", 1.0, None, "ActorPolicy<ActorMfma<2,2,1,2>,false>"),
    _r("mfma21_mc_clip1_relu_dev0", "mc", "bf16_mfma", 48, 24, False, "dev0", 1.0, None, "ActorPolicy<ActorMfma<2,2,1,2>,false>"),
    _r("mfma21_mc_norm_nonoise", "mc", "bf16_mfma", 37, 19, True, "none", 5.0, "wide", "ActorPolicy<ActorMfma<2,2,1,2>,true>"),
    _r("mfma21_pend", "pend", "bf16_mfma", 64, 32, True, "host", 5.0, None, "ActorPolicy<ActorMfma<3,2,1,2>,false>"),
    _r("mfma21_pend_relu_norm", "pend", "bf16_mfma", 37, 19, False, "dev+", 5.0, "wide", "ActorPolicy<ActorMfma<3,2,1,2>,true>"),
    # ---- ActorMfma<OBS,4,2,2> ----------------------------------------------------------------------------------------
    _r("mfma42_mc", "mc", "bf16_mfma", 128, 64, True, "host", 5.0, None, "ActorPolicy<ActorMfma<2,4,2,2>,false>"),
    _r("mfma42_mc_relu_norm", "mc", "bf16_mfma", 65, 33, False, "host", 5.0, "wide", "ActorPolicy<ActorMfma<2,4,2,2>,true>"),
    _r("mfma42_pend_relu", "pend", "bf16_mfma", 65, 33, False, "none", 5.0, None, "ActorPolicy<ActorMfma<3,4,2,2>,false>"),
    _r("mfma42_pend_norm", "pend", "bf16_mfma", 128, 64, True, "host", 5.0, "wide", "ActorPolicy<ActorMfma<3,4,2,2>,true>"),
    # ---- ActorMfmaLds<OBS,7,4,2> -------------------------------------------------------------------------------------
    _r("lds_mc", "mc", "bf16_mfma", 200, 100, True, "host", 5.0, None, "ActorPolicy<ActorMfmaLds<2,7,4,2>,false>"),
    _r("lds_mc_relu_norm", "mc", "bf16_mfma", 129, 65, False, "dev+", 5.0, "floor", "ActorPolicy<ActorMfmaLds<2,7,4,2>,true>"),
    _r("lds_pend_relu", "pend", "bf16_mfma", 224, 128, False, "none", 5.0, None, "ActorPolicy<ActorMfmaLds<3,7,4,2>,false>"),
    _r("lds_pend_norm", "pend", "bf16_mfma", 200, 100, True, "host", 5.0, "wide", "ActorPolicy<ActorMfmaLds<3,7,4,2>,true>"),
    # ---- fp32 policies, at the project's fp32 action tolerance; the random policy bit for bit --------------------------
    _r("f32_mc_64-32", "mc", "f32", 64, 32, True, "host", 5.0, None, "ActorPolicy<ActorF32<2,64,32>,false>"),
    _r("f32_mc_64-32_norm", "mc", "f32", 64, 32, False, "host", 5.0, "floor", "ActorPolicy<ActorF32<2,64,32>,true>"),
    _r("f32_mc_64-64_ln", "mc", "f32", 64, 64, True, "host", 5.0, None, "ActorPolicy<ActorF32<2,64,64>,false>", ln=True),
    _r("f32_mc_64-64_norm", "mc", "f32", 64, 64, True, "dev+", 5.0, "wide", "ActorPolicy<ActorF32<2,64,64>,true>"),
    _r("f32_pend_64-32_ln", "pend", "f32", 64, 32, True, "host", 5.0, None, "ActorPolicy<ActorF32<3,64,32>,false>", ln=True),
    _r("f32_pend_64-32_norm", "pend", "f32", 64, 32, True, "host", 5.0, "wide", "ActorPolicy<ActorF32<3,64,32>,true>"),
    _r("f32_pend_64-64", "pend", "f32", 64, 64, False, "none", 5.0, None, "ActorPolicy<ActorF32<3,64,64>,false>"),
    _r("f32_pend_64-64_norm", "pend", "f32", 64, 64, True, "host", 5.0, "wide", "ActorPolicy<ActorF32<3,64,64>,true>"),
    _r("random_mc", "mc", "random", 0, 0, True, "none", 0.0, None, "RandomPolicy<2>"),
    _r("random_pend", "pend", "random", 0, 0, True, "none", 0.0, None, "RandomPolicy<3>"),
]
ROLLOUT_IDS = [r.name for r in ROLLOUTS]
ROLLOUT_N = (1, 33, 321)
SEED, ID0 = 4321, 7           # Philox key of the runs: env i has global id ID0 + i
ROLLOUT_K, ROLLOUT_T0, ROLLOUT_STEPS_LEFT = 11, 3, 5     # 1 unaligned head step + 2 Philox groups + a 2-step tail
ENV_OF = {"mc": ("MountainCarContinuous-v0", 2, 999, -1.0, 1.0), "pend": ("Pendulum-v0", 3, 200, -2.0, 2.0)}
TOL_ACT_F32 = 2e-5         # the project's fp32 action tolerance on a replay (times (high - low) / 2)


def run_by_name(name):
    return next(r for r in ROLLOUTS if r.name == name)


def rollout_weights(run):
    seed = zlib.crc32(run.name.encode())
    obs_dim = ENV_OF[run.env][1]
    w = condition_weights(actor_weights(obs_dim, run.h1, run.h2, seed=seed, w3_scale=run.w3_scale), run.w3_scale)
    if run.ln:
        rng = np.random.default_rng(seed + 2)
        for k, h in (("ln1", run.h1), ("ln2", run.h2)):
            w[k + "_g"] = rng.uniform(0.5, 1.5, h).astype(np.float32)
            w[k + "_b"] = (0.1 * rng.normal(size=h)).astype(np.float32)
    return w


def initial_state(run, n):
    """(s0, s1) fp32 the envs start from, different in every env: MountainCar positions over [-1.1, 0.1] and velocities over
    +-0.06 (the time-limit reset inside the window then brings the env's own start states), Pendulum angles over the circle
    and theta-dot over +-8, beyond the observation clip.  Independent of n beyond its length."""
    rng, m = np.random.default_rng(zlib.crc32(run.name.encode()) + 3), max(ROLLOUT_N)
    assert n <= m                    # env i starts from the same state whatever n is: a smaller run is a prefix of the largest
    if run.env == "mc":
        s0, s1 = rng.uniform(-1.1, 0.1, m), rng.uniform(-0.06, 0.06, m)
    else:
        s0, s1 = rng.uniform(-np.pi, np.pi, m), rng.uniform(-8.0, 8.0, m)
    return s0[:n].astype(np.float32), s1[:n].astype(np.float32)


def rollout_stat_rows(run):
    """Rows that give the run's observation statistics (ObsRms.update_rows): non-zero means, different in every component;
    "wide": every std above the 0.1 floor and different, nothing the env can show is clipped; "floor" (MountainCar only:
    Pendulum's cos / sin span 20 floor stds): every std ON the floor, so positions further than 0.5 from the mean are
    clipped -- a third of the start states, none of the env's own reset states."""
    rng = np.random.default_rng(zlib.crc32(run.name.encode()) + 4)
    if run.env == "mc":
        mean, sd = [-0.5, 0.01], ([0.4, 0.25] if run.norm == "wide" else [0.02, 0.02])
    else:
        assert run.norm == "wide"
        mean, sd = [0.2, -0.1, 0.5], [0.5, 0.3, 2.0]
    return rng.normal(mean, sd, size=(400, len(mean))).astype(np.float32)


def host_mean_std(rows):
    """the fp32 (mean, std) a fresh RunningMeanStd holds after one update with ``rows`` (obs_rms.mean_std_f32 restated, for
    the CPU tests; the GPU tests read them back from the device block)"""
    x = np.asarray(rows, np.float64)
    cnt = 1e-2 + x.shape[0]
    mean = (x.sum(axis=0) / cnt).astype(np.float32)
    sq = ((1e-2 + (x * x).sum(axis=0)) / cnt).astype(np.float32)
    return mean, np.sqrt(np.maximum(sq - mean * mean, np.float32(1e-2))).astype(np.float32)


def x_hat64(x, mean, std, obs_clip=OBS_CLIP):
    return np.clip((np.asarray(x, np.float64) - mean.astype(np.float64)) / std.astype(np.float64), -obs_clip, obs_clip)


def action_limit(run):
    """|logged action| below which it still carries the network: scale(scale(clip(a))) saturates at ``high``"""
    return ENV_OF[run.env][4]
