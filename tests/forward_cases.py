"""Case matrix of the fp32 DDPG network forward, which six places restate: actor_f32_kernel<2|3,64,32>, actor_generic_kernel
and actor_row_kernel (csrc/actor.hip), critic_kernel (csrc/smartstart.hip), net_rows<false|true> (csrc/ddpg_rows.h, run by
ddpg_stats_rows_kernel and ddpg_eval_kernel<EnvT, WLDS>) and cycle_body (csrc/param_noise.hip).  The case table with the kernel
each case launches, each case's inputs, the fp64 forward with the size of its float32 error beside it, a float32 emulation,
the bound derived from the two, the mutants that bound must reject and the honest variants it must accept.  Shared by the CPU
test (tests/test_forward_cases_cpu.py) and the GPU test (tests/test_gpu_forward_matrix.py); numpy + oracle only (the weight
generator is tests/net_weights.py::make_net, the one tests/test_gpu_ddpg_stats.py uses).

  ref   ``forward(kind, p, obs, ...)``: tests/ddpg_cases.py's ``_inputs`` then ``_net_fwd`` in fp64 on the float32 weights,
        observations and fp32 (mean, std) the kernel receives.  The actor ends in tanh, the critic does not.  The critic's
        action is an exact float32 input (E = 0); for Q(s, pi(s)) it is the actor's fp64 output with E(pi).
  A     E(out) as ddpg_cases.py carries it (its docstring has the rules: inputs, dense, relu, tanh, LayerNorm), in units of
        2^-24.
  emu   the same pass with ``_Ar(f32=True)``: one rounding per operation, sums in index order; the actor's tanh by the
        tanh_fast formula, the critic's hidden tanh np.tanh rounded to float32 (critic_kernel and net_rows<true> call tanhf).

relu and E.  ddpg_cases masks E through a relu with the fp64 sign, which its learner batches can afford: they drop rows whose
pre-activations lie within THR of zero.  The forward is continuous in z and no row is dropped here, so the rule is:
a unit with z > 0, OR with |z| <= RELU_BAND 2^-24 E(z), keeps E(u) = E(z); every other unit has E(u) = 0.  (A unit that close
to zero may be positive in float32 and zero in fp64 or the other way round; either way u moves by no more than z does.)
RELU_BAND = 16 lies above C_FWD, so every unit whose float32 value the bound allows on the other side of zero is inside.
``_net_fwd(relu_band=None)`` is the learner's rule.  The CPU test shows that no emulated element needs the band: the
emulation stays within C_FWD of the reference under A computed with the plain fp64 mask as well.

The bound.  r_case = max |emu - ref| / (2^-24 A) over every element of every row; C_FWD = 4 max_cases r_case rounded up to a
multiple of 0.5 (the factor 4: fma contraction and tiling, as in C_GRAD and C_F32).  A device value x is accepted when
|x - ref| <= C_FWD 2^-24 A for every element of every row; where A == 0, x == ref.  No flat term, no element left out.
Reductions of m such values, without further constants: a mean is held to C_FWD 2^-24 mean(A), a population std to
C_FWD 2^-24 sqrt(mean(A^2)) (the std is 1-Lipschitz in the rms norm of the values), the parameter-noise distance
sqrt(mean((a - b)^2)) to C_FWD 2^-24 sqrt(mean((A_a + A_b)^2)).

Emulated cases: h1 <= 128 and m <= 129 (column ``emu`` of the table: ``case.emulate``); the others use the constant of those,
as ddpg_cases.py does with its large batches.  Mutants are applied to the fp64 algebra at every case and to the emulation at
the emulated ones; each must be MUTANT_MIN = 2 bounds out at every case where it changes anything, and change something
somewhere.  Honest variants are applied to the emulation and must lie inside the bound.

Inputs chosen for the mutants (NOTEBOOK section 30 has the ratios before and after): LayerNorm cases scale W1, b1, W2, b2 by
LN_INPUT_SCALE -- LayerNorm cancels the scale but for its epsilon, and a variance of 1e-3 is where 1e-5 for 1e-12 shows; the actors'
b3 is ACTOR_B3, away from tanh(x) = x; one-row cases are not the ones with one unit or a saturated output.

``fma_kernels`` restates the chains as the kernels run them: from the bias, but for the critic's output layer, which starts from
zero and adds b3 last.  With that chain from b3 as well (BIAS_FIRST, what critic_kernel and net_rows did) the emulation is 3.86
roundings of A out at ev_64_32_m85: b3 = 20 makes every partial sum round at its size.  That is why those kernels changed.
"""
import re
import zlib
from collections import namedtuple

import numpy as np

from oracle import ssc_oracle as O
from tests.ddpg_cases import EPS32, _Ar, _dense, _inputs, _net_fwd, edge_stats, ratio
from tests.net_weights import make_net, oracle_kw

C_FWD = 3.5             # 4 * max r_case over the emulated cases, rounded up to 0.5 (tests/test_forward_cases_cpu.py recomputes it)
RELU_BAND = 16.0        # roundings of E(z) within which a relu unit keeps its E (module docstring)
MUTANT_MIN = 2.0
OBS_CLIP = 5.0
ACTOR_B3 = 0.3                  # the actors' output bias: away from zero, where tanh(x) = x hides a missing output tanh
LN_INPUT_SCALE = 2.0 ** -5      # on W1, b1, W2, b2 of the LayerNorm cases (case_data)
SSC_MAX_STATE, SSC_MAX_ACT = 8, 4

# ---------------------------------------------------------------------------------------------------------- dispatch --
ACTOR_MAX_H1 = 512              # actor.hip: a->h1 > 512 is refused
ROW_MAX_M = 32                  # actor.hip: m <= 32 runs actor_row_kernel
ROW_MAX_H2 = 4096
LDS_DEFAULT = 64 * 1024         # beyond it a launch raises hipFuncAttributeMaxDynamicSharedMemorySize
LDS_MAX = 160 * 1024
CRITIC_MAX_IN2 = 600            # smartstart.hip: h1 + act_dim <= 600
LANE_BYTES = 64 * 4             # one unit of a 64-row block in LDS
REFUSED = "SSC_EUNSUPPORTED"
K_SR, K_EPART = 16, 10          # ddpg_rows.h: kSR; ddpg_eval.hip: kEPart = 3 * kEStreams + 1, kEStreams = 3

ACTOR_F32 = "actor_f32_kernel<%d, 64, 32%s>"
ACTOR_ROW, ACTOR_GENERIC, CRITIC = "actor_row_kernel<%s>", "actor_generic_kernel<%s>", "critic_kernel<%s>"
STATS, EVAL, CYCLE = "ddpg_stats_rows_kernel", "ddpg_eval_kernel<McEnv, %s>", "param_noise_cycle_kernel"
_RMS = "const double *"
ALL_KERNELS = tuple(ACTOR_F32 % (o, r) for o in (2, 3) for r in ("", ", " + _RMS)) + \
    tuple(k % r for k in (ACTOR_ROW, ACTOR_GENERIC, CRITIC) for r in ("", _RMS)) + (STATS, EVAL % "true", EVAL % "false", CYCLE)
KERNEL_SOURCE = {"actor_f32_kernel": "actor.hip", "actor_row_kernel": "actor.hip", "actor_generic_kernel": "actor.hip",
                 "critic_kernel": "smartstart.hip", "ddpg_stats_rows_kernel": "ddpg_stats.hip", "ddpg_eval_kernel": "ddpg_eval.hip",
                 "param_noise_cycle_kernel": "param_noise.hip"}


def actor_lds(h1, h2, ln):
    """actor_generic_kernel's dynamic LDS in bytes"""
    return (h1 + (h2 if ln else 0)) * LANE_BYTES


def critic_lds(h1, h2, act_dim, ln):
    """critic_kernel's dynamic LDS in bytes"""
    return (h1 + act_dim + (h2 if ln else 0)) * LANE_BYTES


def eval_weights_fit(obs_dim, ah, ch, ln):
    """ddpg_eval.hip: weights_fit(eval_carve(..)) -- the activations of a 16-env workgroup and both weight images in 160 KB"""
    net = lambda i, extra, h1, h2: i * h1 + h1 + (h1 + extra) * h2 + h2 + h2 * 1 + 1 + (2 * (h1 + h2) if ln else 0)
    act_floats = K_SR * K_EPART * 2 + 2 * obs_dim * K_SR + max(ah[0], ch[0] + 1) * K_SR + max(ah[1], ch[1]) * K_SR + 2 * K_SR
    return (act_floats + net(obs_dim, 0, *ah) + net(obs_dim, 1, *ch)) * 4 <= LDS_MAX


def launched(kind, obs_dim, h1, h2, act_dim, ln, m, with_rms, global_weights=False, critic=None):
    """The kernel an entry point launches, or REFUSED.  kind: "actor" (ssc_actor_forward[_rms], precision SSC_PREC_F32),
    "critic" (ssc_critic_forward[_rms]), "stats" (ssc_ddpg_stats), "eval" (ssc_ddpg_eval_rollout on MountainCar;
    ``global_weights``: SSC_DDPG_EVAL_GLOBAL_WEIGHTS is set; ``critic``: the critic's (h1, h2) where it differs from the
    actor's), "cycle" (ssc_param_noise_cycle)."""
    rms = _RMS if with_rms else ""
    if kind == "actor":
        if not ln and act_dim == 1 and (h1, h2) == (64, 32) and obs_dim in (2, 3):
            return ACTOR_F32 % (obs_dim, ", " + rms if rms else "")
        if h1 > ACTOR_MAX_H1:
            return REFUSED
        if m <= ROW_MAX_M and h2 <= ROW_MAX_H2:
            return ACTOR_ROW % rms
        if actor_lds(h1, h2, ln) > LDS_MAX:
            return REFUSED
        return ACTOR_GENERIC % rms
    if kind == "critic":
        assert h1 + act_dim <= CRITIC_MAX_IN2
        if critic_lds(h1, h2, act_dim, ln) > LDS_MAX:
            return REFUSED
        return CRITIC % rms
    if kind == "stats":
        return STATS
    if kind == "eval":      # the weights are staged in LDS where they fit, unless the switch keeps them in global memory
        wlds = eval_weights_fit(obs_dim, (h1, h2), critic or (h1, h2), ln) and not global_weights
        return EVAL % ("true" if wlds else "false")
    assert kind == "cycle"
    return CYCLE


def kernel_names_in_source(src):
    """the __global__ kernels of a .hip source"""
    return set(re.findall(r"__global__\s+(?:__launch_bounds__\(.*?\)\s+)?void\s+(\w+)\s*\(", src))


# ------------------------------------------------------------------------------------------------------------- cases --
# name; kind ("actor", "critic": one network through its own entry point; "stats": actor, perturbed actor and critic through
# ssc_ddpg_stats; "eval": actor and critic on MountainCar observations; "cycle": actor and perturbed actor); obs_dim; actor /
# critic (h1, h2) (None where the case has no such network); act_dim; LayerNorm; last_layer_tanh; stats: None | "floor" |
# "wide"; m rows; head: the critic's output layer, "big" (w3_scale 1.5, b3 = 20: Q of order 10) | "zero" (b3 = 0: Q cancels
# around zero); clip: False = obs_clip 0 (no clip); pert: a perturbed actor is present; kernel: what the entry point launches;
# emulate: part of the float32 emulation and of C_FWD
ForwardCase = namedtuple("ForwardCase", "name kind obs ah ch act ln llt stats m head clip pert kernel emulate")


def _c(name, kind, obs, ah, act, ln, llt, stats, m, ch=None, head="big", clip=True, pert=False):
    ah = tuple(ah) if ah is not None else None
    ch = tuple(ch) if ch is not None else (ah if kind in ("stats", "eval") else None)
    h = ah if ah is not None else ch
    kernel = launched(kind, obs, h[0], h[1], act, ln, m, stats is not None, critic=ch)
    widest = max((ah or (0,))[0], (ch or (0,))[0])
    return ForwardCase(name, kind, obs, ah, ch, act, bool(ln), bool(llt), stats, m, head, clip, pert, kernel, widest <= 128 and m <= 129)


def _a(name, obs, h, act, ln, llt, stats, m):
    return _c(name, "actor", obs, h, act, ln, llt, stats, m)


def _q(name, obs, h, act, ln, llt, stats, m, head, clip=True):
    return _c(name, "critic", obs, None, act, ln, llt, stats, m, ch=h, head=head, clip=clip)


CASES = [
    # ---- actor_f32_kernel<2|3, 64, 32[, const double *]>: 256 rows a block, m = 257: a second block of one row
    _a("f32_o2_m1_tanh", 2, (64, 32), 1, False, True, None, 1), _a("f32_o2_m65_tanh_floor", 2, (64, 32), 1, False, True, "floor", 65),
    _a("f32_o2_m256_relu_floor", 2, (64, 32), 1, False, False, "floor", 256), _a("f32_o2_m257_tanh_wide", 2, (64, 32), 1, False, True, "wide", 257),
    _a("f32_o2_m257_relu", 2, (64, 32), 1, False, False, None, 257),
    _a("f32_o3_m1_relu_wide", 3, (64, 32), 1, False, False, "wide", 1), _a("f32_o3_m65_relu", 3, (64, 32), 1, False, False, None, 65),
    _a("f32_o3_m256_tanh", 3, (64, 32), 1, False, True, None, 256), _a("f32_o3_m257_relu_floor", 3, (64, 32), 1, False, False, "floor", 257),
    _a("f32_o3_m257_tanh", 3, (64, 32), 1, False, True, None, 257),
    # ---- actor_row_kernel: one 256-thread block per row, units j, j + 256, .. to a thread
    _a("row_1_1_o1_m1", 1, (1, 1), 1, False, True, None, 1), _a("row_255_256_o8_a4_m32", 8, (255, 256), 4, False, False, "floor", 32),
    _a("row_256_257_o1_a4_ln_m32", 1, (256, 257), 4, True, True, "wide", 32), _a("row_257_1_o8_m32", 8, (257, 1), 1, False, False, None, 32),
    _a("row_257_256_o8_ln_m32", 8, (257, 256), 1, True, False, None, 32),
    _a("row_512_256_o8_a4_m32", 8, (512, 256), 4, False, True, "wide", 32), _a("row_512_257_o1_ln_m1", 1, (512, 257), 1, True, False, "floor", 1),
    _a("row_64_32_o2_ln_m32", 2, (64, 32), 1, True, True, None, 32), _a("row_24_12_o3_a3_ln_m32", 3, (24, 12), 3, True, False, "floor", 32),
    _a("row_37_19_o8_a4_m1", 8, (37, 19), 4, False, True, "wide", 1), _a("row_128_64_o8_a2_m32", 8, (128, 64), 2, False, False, None, 32),
    _a("row_8_8_o8_ln_m32", 8, (8, 8), 1, True, True, "floor", 32), _a("row_64_32_o8_m32", 8, (64, 32), 1, False, True, "floor", 32),
    # ---- actor_generic_kernel: one row a lane, 64 rows a block, (h1 + (ln ? h2 : 0)) * 256 B of LDS
    _a("gen_1_1_o1_m33", 1, (1, 1), 1, False, True, None, 33), _a("gen_255_256_o8_a4_m64", 8, (255, 256), 4, False, False, "floor", 64),
    _a("gen_256_257_o1_a4_ln_m65", 1, (256, 257), 4, True, True, "wide", 65),       # 128.25 KB: raised
    _a("gen_257_1_o8_m129", 8, (257, 1), 1, False, False, None, 129), _a("gen_257_256_o8_ln_m33", 8, (257, 256), 1, True, False, None, 33),
    _a("gen_512_256_o8_a4_m65", 8, (512, 256), 4, False, True, "wide", 65),         # 128 KB without LayerNorm: raised
    _a("gen_400_240_o2_ln_m33", 2, (400, 240), 1, True, True, "floor", 33),         # exactly 160 KB: accepted
    _a("gen_64_32_o2_ln_m65", 2, (64, 32), 1, True, True, None, 65), _a("gen_24_12_o3_a3_ln_m33", 3, (24, 12), 3, True, False, "floor", 33),
    _a("gen_37_19_o8_a4_m129", 8, (37, 19), 4, False, True, "wide", 129), _a("gen_128_64_o8_a2_m64", 8, (128, 64), 2, False, False, None, 64),
    _a("gen_8_8_o8_ln_m33", 8, (8, 8), 1, True, True, "floor", 33), _a("gen_64_32_o8_m33", 8, (64, 32), 1, False, True, "floor", 33),
    # ---- critic_kernel: one row a lane, in2 = h1 + act_dim, (in2 + (ln ? h2 : 0)) * 256 B of LDS
    _q("cr_1_1_o1_m63", 1, (1, 1), 1, False, True, None, 63, "big"), _q("cr_64_32_o2_m63_zero_floor", 2, (64, 32), 1, False, True, "floor", 63, "zero"),
    _q("cr_64_32_o3_a4_ln_m64_wide", 3, (64, 32), 4, True, False, "wide", 64, "big"), _q("cr_64_48_o8_a4_ln_m65_zero", 8, (64, 48), 4, True, True, None, 65, "zero"),
    _q("cr_400_300_o2_m65_floor", 2, (400, 300), 1, False, True, "floor", 65, "big"),            # 100.25 KB: raised
    _q("cr_400_236_o8_a4_ln_m64_zero", 8, (400, 236), 4, True, False, "wide", 64, "zero"),       # exactly 160 KB: accepted
    _q("cr_64_32_o2_m65_noclip", 2, (64, 32), 1, False, False, None, 65, "big", clip=False),
    _q("cr_24_12_o3_a2_ln_m1_zero", 3, (24, 12), 2, True, False, "floor", 1, "zero"), _q("cr_1_8_o2_a4_m63", 2, (1, 8), 4, False, False, "wide", 63, "big"),
    _q("cr_128_64_o3_m65_zero", 3, (128, 64), 1, False, False, None, 65, "zero"), _q("cr_64_32_o2_m64_zero_tanh", 2, (64, 32), 1, False, True, None, 64, "zero"),
    # ---- net_rows through ssc_ddpg_stats: 16 rows a workgroup, units part, part + 16, .. to a thread
    _c("st_37_19_c50_27_o2_m1", "stats", 2, (37, 19), 1, False, True, None, 1, ch=(50, 27), head="big", pert=True),
    _c("st_37_19_c50_27_o3_a2_ln_m15", "stats", 3, (37, 19), 2, True, False, "floor", 15, ch=(50, 27), head="zero", pert=True),
    _c("st_64_32_o2_m16_wide", "stats", 2, (64, 32), 1, False, True, "wide", 16, head="zero"),
    _c("st_24_12_c37_19_o8_a2_ln_m17", "stats", 8, (24, 12), 2, True, True, None, 17, ch=(37, 19), head="big", pert=True),
    _c("st_37_19_c128_64_o3_a2_m33_wide", "stats", 3, (37, 19), 2, False, False, "wide", 33, ch=(128, 64), head="zero", pert=True),
    # ---- net_rows through ssc_ddpg_eval_rollout on MountainCar (n = 17, K = 5: 85 logged rows; the GPU test takes the rows
    # from the device's own log, the CPU test draws them from the observation space)
    _c("ev_64_32_m85", "eval", 2, (64, 32), 1, False, True, None, 85), _c("ev_24_12_m85_wide", "eval", 2, (24, 12), 1, False, True, "wide", 85),
    _c("ev_24_12_ln_m85_zero", "eval", 2, (24, 12), 1, True, False, None, 85, head="zero"),
    _c("ev_200_100_m85", "eval", 2, (200, 100), 1, False, True, None, 85),           # 164.6 KB with the weights: they stay in global memory
    _c("ev_37_19_c50_27_ln_m85_floor", "eval", 2, (37, 19), 1, True, True, "floor", 85, ch=(50, 27)),
    # ---- cycle_body through ssc_param_noise_cycle (the GPU test takes the perturbed parameters from ssc_param_noise_perturb)
    _c("cy_2_64_32_m1", "cycle", 2, (64, 32), 1, False, True, None, 1, pert=True), _c("cy_2_64_32_m65_floor", "cycle", 2, (64, 32), 1, False, True, "floor", 65, pert=True),
    _c("cy_8_8_8_ln_m1_floor", "cycle", 8, (8, 8), 1, True, True, "floor", 1, pert=True), _c("cy_8_8_8_ln_m65", "cycle", 8, (8, 8), 1, True, True, None, 65, pert=True),
    _c("cy_2_64_32_m65_relu_wide", "cycle", 2, (64, 32), 1, False, False, "wide", 65, pert=True), _c("cy_2_64_32_m1_relu", "cycle", 2, (64, 32), 1, False, False, None, 1, pert=True),
    _c("cy_8_8_8_ln_m65_relu_wide", "cycle", 8, (8, 8), 1, True, False, "wide", 65, pert=True), _c("cy_8_8_8_ln_m1_relu_floor", "cycle", 8, (8, 8), 1, True, False, "floor", 1, pert=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
EMULATED = [c for c in CASES if c.emulate]
# shapes the entry points refuse: (kind, obs_dim, h1, h2, act_dim, ln, m)
REFUSED_CASES = [("actor", 2, 400, 241, 1, True, 33), ("critic", 8, 400, 237, 4, True, 64)]

MUTANTS = ("ln_eps_1e-5", "ln_var_n_minus_1", "ln_mean_n_minus_1", "gamma_beta_swapped", "drop_last_unit_h1", "drop_last_unit_h2",
           "action_row_before", "action_before_relu", "critic_output_tanh", "actor_no_output_tanh", "neighbour_mean",
           "clip_before_norm", "bf16_weights", "fp16_hidden", "w3_stride_1")
VARIANTS = ("fma", "fma_kernels", "tanh_exchanged", "rstd_rsqrt", "reciprocal_std")
BIAS_FIRST = "fma_bias_first"   # outside the bound (3.86 roundings of A at ev_64_32_m85): the reason the critic kernels add b3 last
RESTATED = "restated"      # no change: _fwd_alt as it stands (the CPU test holds it to _net_fwd bit for bit)
_INTERNAL = ("ln_eps_1e-5", "ln_var_n_minus_1", "ln_mean_n_minus_1", "fp16_hidden", "action_before_relu", RESTATED, BIAS_FIRST) + VARIANTS[:4]


# ---------------------------------------------------------------------------------------------------------- generator --
def _rows(rng, obs_dim, mean, std, lo, hi, n):
    """n observation rows; rows 0 .. 3 (as far as there are that many): a component beyond +clip, components exactly on
    +clip and -clip (with statistics: mean +- 5 std rounded to float32), an all-zero row that starts with -0.0, a component
    beyond -clip; every 64th row beyond +clip again (row 256 is the one row of a second 256-row block)"""
    f = np.float32
    if mean is None:
        x = rng.uniform(-1.5, 1.5, size=(n, obs_dim))
        at = lambda k, c: k
    else:
        x = rng.uniform(lo, hi, size=(n, obs_dim))
        at = lambda k, c: float(mean[c]) + k * float(std[c])
    x = x.astype(f)
    last = obs_dim - 1
    x[::64, 0] = at(7.0, 0)
    if n > 1:
        x[1, 0], x[1, last] = at(5.0, 0), at(-5.0, last)
    if n > 2:
        x[2] = 0.0
        x[2, 0] = -0.0
    if n > 3:
        x[3, last] = at(-7.5, last)
    return x


_DATA = {}


def case_data(case):
    """dict(actor, critic, pert (float32 weight dicts or None), obs [m, obs_dim], act [m, act_dim] (critic input) or None,
    mean, std (fp32 or None), block (the f64 RunningMeanStd vector or None)).  The weights and the row pool are drawn from
    the case's shape and options, not from m: a row case and a generic case of one shape share networks and leading rows.
    Computed once, read-only."""
    if case.name in _DATA:
        return _DATA[case.name]
    key = repr((case.kind, case.obs, case.ah, case.ch, case.act, case.ln, case.llt, case.stats, case.head, case.clip))
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    od, ad = case.obs, case.act
    actor = critic = pert = None
    if case.ah is not None:
        actor = make_net(rng, od, case.ah[0], 0, case.ah[1], ad, case.ln, 0.25, ACTOR_B3)
    if case.ch is not None:
        critic = make_net(rng, od, case.ch[0], ad, case.ch[1], 1, case.ln, 1.5, 20.0 if case.head == "big" else 0.0)
    for w in (actor, critic):       # LayerNorm is invariant to the scale of its input but for the variance epsilon: pre-activations
        if w is not None and case.ln:       # of order 2^-5 (variance 1e-3) are where an epsilon of 1e-5 for 1e-12 shows
            for k in ("W1", "b1", "W2", "b2"):
                w[k] = w[k] * np.float32(LN_INPUT_SCALE)
    if case.pert:       # actor + N(0, 0.2^2) on the perturbable variables (LayerNorm gamma / beta stay)
        pert = {k: (v + (0.2 * rng.normal(size=v.shape)).astype(np.float32) if not k.startswith("ln") else v) for k, v in actor.items()}
    block = mean = std = lo = hi = None
    if case.stats:
        block, mean, std, (lo, hi) = edge_stats(od, case.stats)
    if case.kind == "eval":     # MountainCar's observation space
        lo, hi = np.array([-1.2, -0.07]), np.array([0.6, 0.07])
        obs = rng.uniform(lo, hi, size=(300, od)).astype(np.float32)[:case.m]
    else:
        obs = _rows(rng, od, mean, std, lo, hi, 300)[:case.m].copy()
    act = rng.uniform(-1, 1, size=(300, ad)).astype(np.float32)[:case.m] if case.kind in ("critic", "stats") else None
    d = dict(actor=actor, critic=critic, pert=pert, obs=obs, act=act, mean=mean, std=std, block=block)
    for v in d.values():
        for arr in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
    _DATA[case.name] = d
    return d


# ----------------------------------------------------------------------------------------- the forward, fp64 or float32 --
class _ArF(_Ar):
    """ddpg_cases._Ar; ``exact_tanh``: the float32 pass takes np.tanh rounded to float32 (tanhf) instead of tanh_fast"""

    def __init__(self, f32, exact_tanh=False):
        super().__init__(f32)
        self.exact_tanh = exact_tanh

    def tanh(self, x):
        if self.f32 and self.exact_tanh:
            return np.tanh(x.astype(np.float64)).astype(np.float32)
        return super().tanh(x)


def _fma_dense(h, W, b, bias_first):
    """float32 h W + b as a chain of fused multiply-adds, inputs in index order, one rounding each (the product of two
    float32 is exact in fp64); the bias is what the chain starts from (``bias_first``) or is added behind it"""
    acc = np.broadcast_to(b if bias_first else np.float32(0), (h.shape[0], W.shape[1])).astype(np.float32)
    h64, W64 = h.astype(np.float64), W.astype(np.float64)
    for k in range(h.shape[1]):
        acc = (acc.astype(np.float64) + h64[:, k:k + 1] * W64[k:k + 1, :]).astype(np.float32)
    return acc if bias_first else acc + b


def _ln_alt(ar, z, p, which, mut):
    """ddpg_cases._ln_fwd's values with one thing changed (``mut``); None: the same operations (held equal on the CPU)"""
    if which + "_g" not in p:
        return z
    T, n = ar.t, z.shape[1]
    if mut == "ln_mean_n_minus_1" and n > 1:
        mean = ar.rowsum(z[:, :-1]) / T(n - 1)
    else:
        mean = ar.rowsum(z) / T(n)
    d = z - mean[:, None]
    var = ar.rowsum(d * d) / T(n - 1 if mut == "ln_var_n_minus_1" and n > 1 else n)
    v = var + T(1e-5 if mut == "ln_eps_1e-5" else 1e-12)
    if mut == "rstd_rsqrt" and ar.f32:
        rstd = (1.0 / np.sqrt(v.astype(np.float64))).astype(np.float32)      # one rounding, where 1 / sqrtf has two
    else:
        rstd = T(1) / np.sqrt(v)
    return (d * rstd[:, None]) * p[which + "_g"] + p[which + "_b"]


def _fwd_alt(ar, p, x, llt, act, actor, mut):
    """ddpg_cases._net_fwd's values with the inside of the network changed: the LayerNorm mutants, hidden activations
    rounded to fp16, and the variants fma / tanh_exchanged / rstd_rsqrt"""
    f16 = (lambda v: v.astype(np.float16).astype(ar.t)) if mut == "fp16_hidden" else (lambda v: v)
    # fma: every chain from zero, the bias behind it.  fma_kernels: the kernels' chains -- from the bias, but for the critic's
    # output layer, whose bias is added behind a chain from zero.  fma_bias_first: every chain from its bias, the critic's
    # output layer too (what critic_kernel and net_rows did before; not an accepted variant, see NOTEBOOK)
    first = {"fma": (False, False), "fma_kernels": (True, actor), "fma_bias_first": (True, True)}.get(mut) if ar.f32 else None
    dense = (lambda h, W, b, last=False: _dense(ar, h, None, W, b)[0]) if first is None else \
        (lambda h, W, b, last=False: _fma_dense(h, W, b, first[last]))
    exchanged = mut == "tanh_exchanged"      # the hidden tanh and the actor's output tanh both take the other function
    if exchanged:
        ar = _ArF(ar.f32, not ar.exact_tanh)
    z1 = dense(x, p["W1"], p["b1"])
    if mut == "action_before_relu" and act is not None:
        # the action joins z1 BEFORE LayerNorm and relu: it is counted in the layer's statistics, normalised (gamma 1, beta 0
        # for its columns) and passes the relu
        z1 = np.concatenate([z1, act], axis=1)
        if "ln1_g" in p:
            p = dict(p, ln1_g=np.concatenate([p["ln1_g"], np.ones(act.shape[1], ar.t)]), ln1_b=np.concatenate([p["ln1_b"], np.zeros(act.shape[1], ar.t)]))
        act = None
    a1 = f16(np.maximum(_ln_alt(ar, z1, p, "ln1", mut), ar.t(0)))
    if act is not None:
        a1 = np.concatenate([a1, act], axis=1)
    n2 = _ln_alt(ar, dense(a1, p["W2"], p["b2"]), p, "ln2", mut)
    a2 = f16(ar.tanh(n2) if llt else np.maximum(n2, ar.t(0)))
    out = dense(a2, p["W3"], p["b3"], True)
    return _ArF(ar.f32, exchanged).tanh(out) if actor else out


def forward(kind, p, obs, mean=None, std=None, llt=True, act=None, Eact=None, clip=True, f32=False, mut=None, relu_band=RELU_BAND):
    """One network on raw float32 observations: (out [m, out_dim], E(out) or None in float32).  kind "actor" | "critic";
    p: float32 weight dict; mean / std: the fp32 statistics or None; act / Eact: the critic's action and its E (None: exact);
    clip False: obs_clip 0; mut: one of MUTANTS or VARIANTS, or None (ddpg_cases' _inputs then _net_fwd)."""
    assert mut is None or mut in MUTANTS or mut in VARIANTS or mut in (RESTATED, BIAS_FIRST)
    actor = kind == "actor"
    ar = _ArF(f32, exact_tanh=not actor)
    T = ar.t
    p = {k: ar.arr(v) for k, v in p.items()}
    x = np.asarray(obs, np.float32)
    d = dict(mean=mean, std=std)
    imut = None if clip else "no_obs_clip"
    if mut == "neighbour_mean" and mean is not None:
        assert clip
        imut = mut
    elif mut == "clip_before_norm" and clip and mean is not None:
        x, imut = np.clip(x, np.float32(-OBS_CLIP), np.float32(OBS_CLIP)), "no_obs_clip"
    if mut == "reciprocal_std" and f32 and mean is not None:
        x = (x - mean) * (np.float32(1) / std)
        x, Ex = (np.clip(x, T(-OBS_CLIP), T(OBS_CLIP)) if clip else x), None
    else:
        x, Ex = _inputs(ar, d, x, imut)
    if not actor:
        act = ar.arr(act)
        if Eact is None and ar.sizes:
            Eact = np.zeros(act.shape)
    # ---- mutants that are a change of the inputs
    if mut == "gamma_beta_swapped" and "ln1_g" in p:
        p.update(ln1_g=p["ln1_b"], ln1_b=p["ln1_g"], ln2_g=p["ln2_b"], ln2_b=p["ln2_g"])
    elif mut in ("drop_last_unit_h1", "drop_last_unit_h2"):
        k = "W2" if mut == "drop_last_unit_h1" else "W3"
        w = p[k].copy()
        w[p["W1"].shape[1] - 1 if k == "W2" else -1] = 0
        p[k] = w
    elif mut == "action_row_before" and not actor:
        act = np.roll(act, 1, axis=0)
    elif mut == "bf16_weights":
        p = {k: ar.arr(O.round_bf16(np.asarray(v, np.float32))) for k, v in p.items()}
    elif mut == "w3_stride_1" and actor:
        h2, ad = p["W3"].shape
        flat = p["W3"].reshape(-1)
        p["W3"] = np.stack([flat[a:a + h2] for a in range(ad)], axis=1)
    if mut in _INTERNAL and not (mut == "action_before_relu" and actor):
        return _fwd_alt(ar, p, x, llt, act, actor, mut), None
    if mut == "actor_no_output_tanh" and actor:
        m = x.shape[0]
        out, E, _ = _net_fwd(ar, p, x, Ex, llt, ar.arr(np.zeros((m, 0))), np.zeros((m, 0)) if ar.sizes else None, relu_band=relu_band)
        return out, E
    out, E, _ = _net_fwd(ar, p, x, Ex, llt, act, Eact, relu_band=relu_band)
    if mut == "critic_output_tanh" and not actor:
        out = np.tanh(out) if not f32 else _ArF(True, True).tanh(out)
    return out, E


def streams(case, d=None, f32=False, mut=None, relu_band=RELU_BAND):
    """Every value stream of a case: {name: (out, E)}.  actor: "pi"; critic: "q"; stats: "q" = Q(s, a), "qpi" = Q(s, pi(s)),
    "pi", "pp" (the perturbed actor, where present); eval: "pi", "qpi"; cycle: "pi", "pp".  In float32 the critic of "qpi"
    takes the float32 "pi" as the kernels do.  ``d``: case_data(case) or a dict like it (the GPU test's device-made inputs)."""
    d = case_data(case) if d is None else d
    kw = dict(mean=d["mean"], std=d["std"], llt=case.llt, clip=case.clip, f32=f32, mut=mut, relu_band=relu_band)
    out = {}
    if case.kind != "critic":
        out["pi"] = forward("actor", d["actor"], d["obs"], **kw)
        if case.pert:
            out["pp"] = forward("actor", d["pert"], d["obs"], **kw)
    if case.kind in ("critic", "stats"):
        out["q"] = forward("critic", d["critic"], d["obs"], act=d["act"], **kw)
    if case.kind in ("stats", "eval"):
        out["qpi"] = forward("critic", d["critic"], d["obs"], act=out["pi"][0], Eact=out["pi"][1], **kw)
    return out


_REF = {}


def reference(case):
    """The fp64 forward of the case with the sizes A.  "actor" / "critic" cases: (out64, A); the others: {stream: (out64, A)}.
    Computed once, never modified."""
    if case.name not in _REF:
        s = streams(case)
        for o, A in s.values():
            o.setflags(write=False)
            A.setflags(write=False)
        _REF[case.name] = s[{"actor": "pi", "critic": "q"}[case.kind]] if case.kind in ("actor", "critic") else s
    return _REF[case.name]


def reference_streams(case):
    r = reference(case)
    return r if isinstance(r, dict) else {{"actor": "pi", "critic": "q"}[case.kind]: r}


def emulate(case, mut=None):
    """the float32 emulation of the case, as reference() shapes it, without the sizes"""
    s = {k: v[0] for k, v in streams(case, f32=True, mut=mut).items()}
    return s[{"actor": "pi", "critic": "q"}[case.kind]] if case.kind in ("actor", "critic") else s


# -------------------------------------------------------------------------------------------------------------- bounds --
def value_ratio(x, ref, A):
    """max |x - ref| / (2^-24 A) over every element (units of r_case); where A == 0 the value must be exact"""
    return ratio(np.abs(np.asarray(x, np.float64).reshape(ref.shape) - ref), EPS32 * A)


def case_ratio(case, got, ref=None):
    """the largest value_ratio over the streams of a case; got: {stream: values} (or the array of an actor / critic case)"""
    ref = reference_streams(case) if ref is None else ref
    if not isinstance(got, dict):
        got = {next(iter(ref)): got}
    return max(value_ratio(got[k], *ref[k]) for k in ref)


def mean_ratio(x, ref, A):
    """|x - mean(ref)| / (2^-24 mean(A))"""
    return ratio(abs(float(x) - float(np.mean(ref))), EPS32 * float(np.mean(A)))


def std_ratio(x, ref, A):
    """|x - std(ref)| / (2^-24 sqrt(mean(A^2))), population std"""
    return ratio(abs(float(x) - float(np.std(ref))), EPS32 * float(np.sqrt(np.mean(np.square(A)))))


def distance64(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def distance_ratio(x, a, Aa, b, Ab):
    """|x - sqrt(mean((a - b)^2))| / (2^-24 sqrt(mean((A_a + A_b)^2)))"""
    return ratio(abs(float(x) - distance64(a, b)), EPS32 * float(np.sqrt(np.mean(np.square(Aa + Ab)))))


def x_hat64(obs, mean, std, clip=True):
    """what the oracle is fed: clip((obs - mean) / std) in fp64 from the fp32 statistics"""
    x = np.asarray(obs, np.float64)
    if mean is not None:
        x = (x - mean.astype(np.float64)) / std.astype(np.float64)
    return np.clip(x, -OBS_CLIP, OBS_CLIP) if clip else x
