"""fp32 forward-simulation matrix of csrc/dyn_model.hip: the case list with the kernel instantiations each case launches, each
case's inputs, the fp64 reference with the size of its float32 error beside it, a float32 restatement of the kernels'
arithmetic, the bound derived from the two, the mutants that bound must reject and the honest variants it must accept.
Shared by the CPU test (tests/test_sim32_cases_cpu.py) and the GPU test (tests/test_gpu_sim32_matrix.py); numpy + oracle only.

Three quantities, all for the S[0..H] trajectories.

  ref   O.dyn_forward_sim in fp64 on the float32 inputs and statistics the kernel receives (sim_cases.norm32); restated
        here as ``simulate(inp)`` so that the mutants below have one place to act (the CPU test holds the two together).
  emu   ``simulate(inp, f32=True)``: the kernels' arithmetic in float32.  z-score fl(fl(x - mean) / std) by IEEE division,
        then NaN -> 0 and +-Inf -> +-FLT_MAX; every dense layer an index-ordered FMA chain per output (b first, inputs
        k = 0, 1, ..), ReLU; the update S + fma(z, std_z, mean_z).  An FMA is the fp64 product (exact for two float32)
        plus the sum, rounded once to float32.  The compiled gfx950 code of dyn_model.hip contracts the update in every
        kernel: v_fma_f32 / v_pk_fma_f32 of z, std_z and mean_z, then one v_add_f32 / v_pk_add_f32 of S.
  A     the size of the float32 error of every element of S, in units of 2^-24, carried beside the fp64 pass:
          inputs     E(s0) = 0, E(action) = 0
          normalise  E(v) = (E(x) + |x - mean|) / std + |v|   (an input with std == 0 has E = 0: its weights must be 0)
          dense      z = h W + b:  E(z) = sqrt(E(h)^2 W^2) + |h| |W| + |b| + R,  R = sqrt(sum_k s_k^2)
                     (tests/ddpg_cases.py: errors that different inputs bring in are independent and add in quadrature;
                     the terms' own size counts once; R is the chain's own rounding, one per partial sum
                     s_k = b + h_0 W_0 + .. + h_k W_k in index order, independent -- ddpg_cases' R of a batch sum.  Without
                     R a 513-long chain whose partial sums stay near its bias is off by 14 x sum |terms| 2^-24, and
                     C_F32 would be 56.5: hidden activations in fp16 would sit inside 2 bounds at small_d1_a2_128)
          ReLU       E(u) = E(z) * (the fp64 mask)
          update     E(S') = E(S) + std_z E(z) + |z std_z| + |z std_z + mean_z| + |S'|
        E(S_t) feeds the next step's normalise.

The bound.  r_case = max |emu - ref| / (2^-24 A) over every element of S at every t, and over the per-step increments
S[t+1] - S[t] against 2^-24 (A_t + A_{t+1}).  A result X is accepted when, elementwise at every t,
|X - ref| <= C_F32 2^-24 A and |dX - dref| <= C_F32 2^-24 (A_t + A_{t+1}); where A is 0 (S[0]) X must equal ref exactly.
C_F32 = 4 max_cases r_case, rounded up to a multiple of 0.5 (the CPU test recomputes it).  There is no flat term.

Mutants (``MUTANTS``; each applied to the fp64 algebra and to the float32 emulation, and at least 2 bounds out at every
case where it changes anything): ``net_mutants`` (sim_cases.mutants() per layer width), bf16 arithmetic
(O.mlp_forward_bf16emu), weights rounded to bf16, hidden activations rounded to fp16, inputs k >= 512 of a K > 512 layer
dropped, outputs c >= 256 given column c - 256's values, actions read at step t - 1, S[t] stored after the update, the
NaN -> 0 mapping missing.  Honest variants (``VARIANTS``; inside the bound): z-score by the float32 reciprocal of std,
the update without contraction, multiply-then-add instead of FMA in the chains.
"""
import re
import zlib
from collections import namedtuple

import numpy as np

from oracle import ssc_oracle as O
from tests import sim_cases as SC

EPS32 = 2.0 ** -24
C_F32 = 4.5             # 4 * max r_case rounded up to a multiple of 0.5 (tests/test_sim32_cases_cpu.py recomputes it)

# ---------------------------------------------------------------------------------------------------------- dispatch --
K_SMALL_MAX_DEPTH = 128          # kSmallMaxDepth
K_KCHUNK = 512                   # kKChunk: K staged through LDS per pass of mlp_layer_f32_kernel
K_COLS = 256                     # columns per pass of mlp_layer_f32_kernel (one per thread)
SSC_MAX_LAYERS = 4

PAIR = "dyn_small_sim_pair_kernel<%d,%s,%s>"
SMALL = "dyn_small_sim_kernel"
CHAIN_SIM = ("dyn_init_kernel", "dyn_prepare_kernel", "dyn_update_kernel")
LAYER = "mlp_layer_f32_kernel<%s>"
ALL_KERNELS = tuple(PAIR % (D, s, w) for D in (2, 3) for s in ("false", "true") for w in ("false", "true")) + \
    (SMALL,) + CHAIN_SIM + (LAYER % "true", LAYER % "false")


def _b(x):
    return "true" if x else "false"


def small_sim_shape(dims, d, a):
    """dyn_model.hip: small_sim_shape"""
    return len(dims) == 3 and dims[1] <= K_SMALL_MAX_DEPTH and d <= 3 and d + a <= 4 and a <= 3


def pair_shape(d, a, m, H, N=None, pid0=SC.PID0):
    """dyn_model.hip: launch_small_sim's condition for the two-rows-per-lane kernel (N None: actions from memory)"""
    return (d in (2, 3) and a == 1 and m * (H + 1) * d * 4 < 2 ** 31 and m * H * 4 < 2 ** 31
            and (N is None or (N >= 1 and pid0 + m // N < 2 ** 32)))


def layer_kernels(dims):
    return ((LAYER % "true",) if len(dims) > 2 else ()) + (LAYER % "false",)


def launched(dims, m, H, N, mode):
    """the fp32 instantiations ssc_dyn_forward_sim (mode 0) / ssc_mpc_forward_sim (mode 1) launch for a network"""
    d, a = dims[-1], dims[0] - dims[-1]
    if H >= 1 and small_sim_shape(dims, d, a):
        if pair_shape(d, a, m, H, N if mode == 1 else None):
            return (PAIR % (d, _b(mode == 1), _b(dims[1] % 4 == 0)),)
        return (SMALL,)
    return CHAIN_SIM + layer_kernels(dims)


def kernel_names_in_source(src):
    """the __global__ kernels of a .hip source"""
    return set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src))


# ------------------------------------------------------------------------------------------------------------- cases --
# name; network dims; horizon; problems x candidates (rows m = P N); start state per "call" / "problem" / "row"; family
# ("pair", "small", "chain"); zero_std: state input d - 1 has std 0 (its W1 row 0, it never moves; rows at its mean and
# off it: 0 / 0 and x / 0); kernels: the instantiations the case claims over both modes (held to launched() on the CPU)
Sim32Case = namedtuple("Sim32Case", "name dims H P N s0_kind family zero_std kernels")


def _c(name, dims, H, P, N, s0_kind, family, kernels, zero_std=False):
    return Sim32Case(name, tuple(dims), H, P, N, s0_kind, family, zero_std, tuple(kernels))


def _pair(D, sw):
    return (PAIR % (D, "false", _b(sw)), PAIR % (D, "true", _b(sw)))


_CH1 = CHAIN_SIM + (LAYER % "false",)
_CH = CHAIN_SIM + (LAYER % "true", LAYER % "false")
CASES = [
    # ---- dyn_small_sim_pair_kernel<D, SAMPLE, SW>: mode 0 = SAMPLE false, mode 1 = SAMPLE true; SW = depth % 4 == 0
    _c("pair_ref_32", (3, 32, 2), 4, 5, 51, "problem", "pair", _pair(2, True)),       # the reference shape, odd N
    _c("pair_lds_30_h9", (3, 30, 2), 9, 5, 33, "row", "pair", _pair(2, False)),      # LDS image, H % 4 != 0, odd m
    _c("pair_depth1_m513", (3, 1, 2), 4, 27, 19, "call", "pair", _pair(2, False)),   # depth 1; a second block of one row
    _c("pair_d3_128_h20", (4, 128, 3), 20, 4, 64, "problem", "pair", _pair(3, True)),   # depth = kSmallMaxDepth
    _c("pair_d3_127", (4, 127, 3), 4, 7, 37, "row", "pair", _pair(3, False)),
    # ---- dyn_small_sim_kernel: state 1, or state 2 with 2 actions
    _c("small_d1_m257", (2, 32, 1), 4, 1, 257, "call", "small", (SMALL,)),
    _c("small_d1_a3_h7", (4, 64, 1), 7, 3, 41, "problem", "small", (SMALL,)),         # Philox word groups straddle steps
    _c("small_d2_a2", (4, 100, 2), 4, 5, 20, "row", "small", (SMALL,)),
    _c("small_d1_a2_128", (3, 128, 1), 4, 2, 100, "problem", "small", (SMALL,)),
    # ---- the generic chain: dyn_init, then per step dyn_prepare, mlp_layer_f32<relu> .., <linear>, dyn_update
    _c("chain_d5", (7, 20, 5), 4, 3, 17, "problem", "chain", _CH),
    _c("chain_129_m17", (3, 129, 2), 4, 1, 17, "call", "chain", _CH),                 # depth just past the fused kernels
    _c("chain_513_m33", (3, 513, 513, 2), 2, 3, 11, "row", "chain", _CH),            # second K chunk, third column pass
    _c("chain_linear", (4, 3), 4, 4, 16, "problem", "chain", _CH1),                   # no hidden layer
    _c("chain_4layers", (5, 40, 24, 16, 3), 4, 2, 20, "problem", "chain", _CH),      # SSC_MAX_LAYERS
    _c("chain_d8_a4", (12, 64, 8), 4, 2, 25, "row", "chain", _CH),
    _c("chain_d3_a3", (6, 32, 3), 4, 4, 9, "call", "chain", _CH),                     # d + a > 4, one small hidden layer
    # ---- zero std, one per family
    _c("zstd_pair", (3, 32, 2), 4, 3, 21, "row", "pair", _pair(2, True), zero_std=True),
    _c("zstd_small", (4, 100, 2), 4, 4, 15, "problem", "small", (SMALL,), zero_std=True),
    _c("zstd_chain", (7, 20, 5), 4, 3, 17, "row", "chain", _CH, zero_std=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}
CASE_IDS = [c.name for c in CASES]

# ssc_mlp_forward in fp32 alone: the generic chain's networks at m = 1, 16, 17, 33
MlpCase = namedtuple("MlpCase", "name dims m kernels")
MLP_CASES = [MlpCase(f"mlp_{c.name[6:]}_m{m}", c.dims, m, layer_kernels(c.dims))
             for c in CASES if c.family == "chain" and not c.zero_std for m in (1, 16, 17, 33)]
MLP_BY_NAME = {c.name: c for c in MLP_CASES}


# ---------------------------------------------------------------------------------------------------------- generator --
Sim32Inputs = namedtuple("Sim32Inputs", "case Ws bs norm d a low high m rows s0 s0_rows A x0")


def condition_edge_units(x, Ws, bs):
    """sim_cases.build_inputs' edge-unit conditioning, per layer width: unit 0 and the last unit of every hidden layer are
    made active on every row of x by their bias (a mutant that loses one of them must be visible)"""
    h = np.asarray(x, np.float64)
    for l in range(len(Ws) - 1):
        pre = h @ Ws[l].astype(np.float64)
        for u in (0, Ws[l].shape[1] - 1):
            bs[l][u] = np.float32(max(float(bs[l][u]), 0.5 - float(pre[:, u].min())))
        h = np.maximum(pre + bs[l].astype(np.float64), 0.0)


def _normalised(s, A0, norm):
    nm = SC.norm32(norm)
    return np.concatenate([O.normalise(s, nm["mean_x"], nm["std_x"]), O.normalise(A0, nm["mean_y"], nm["std_y"])], axis=1)


_INPUTS = {}


def build_inputs(case):
    """Deterministic inputs of a case (sim_cases.build_inputs with per-layer edge units and the zero-std edit); read-only"""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    dims = case.dims
    d, a = dims[-1], dims[0] - dims[-1]
    Ws, bs = SC.make_mlp(rng, dims)
    norm = SC.make_norm(rng, d, a)
    m = case.P * case.N
    n_s0 = {"call": None, "problem": case.P, "row": m}[case.s0_kind]
    s0 = (rng.normal(size=d if n_s0 is None else (n_s0, d)) * 0.3).astype(np.float32)
    if case.zero_std:
        assert n_s0 is not None
        j = d - 1
        Ws[0][j, :] = 0.0
        norm["std_x"][j], norm["mean_x"][j], norm["std_z"][j], norm["mean_z"][j] = 0.0, 0.25, 0.0, 0.0
        s0[:, j] = 0.25 + np.array([0.0, 0.5, -0.5])[np.arange(n_s0) % 3]        # 0 / 0, x / 0 of both signs
    rows = np.arange(m)
    s0_rows = np.broadcast_to(s0, (m, d)).copy() if n_s0 is None else (s0[rows // case.N] if n_s0 == case.P else s0.copy())
    A = SC.action_rows(rows, case.N, case.H, a)
    x0 = _normalised(s0_rows, A[:, 0, :], norm)
    condition_edge_units(x0, Ws, bs)
    inp = Sim32Inputs(case, Ws, bs, norm, d, a, SC.ACT_LOW[:a], SC.ACT_HIGH[:a], m, rows, s0, s0_rows, A, x0)
    for arr in [s0, s0_rows, A, x0] + Ws + bs + list(norm.values()):
        arr.setflags(write=False)
    _INPUTS[case.name] = inp
    return inp


MlpInputs = namedtuple("MlpInputs", "case Ws bs x")


def mlp_inputs(case):
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    Ws, bs = SC.make_mlp(rng, case.dims)
    x = rng.normal(size=(case.m, case.dims[0])).astype(np.float32)
    condition_edge_units(x, Ws, bs)
    for arr in [x] + Ws + bs:
        arr.setflags(write=False)
    _INPUTS[case.name] = MlpInputs(case, Ws, bs, x)
    return _INPUTS[case.name]


# --------------------------------------------------------------------------------- the simulation, fp64 or float32 --
NET_MUTANTS = ("bf16_arith", "weights_bf16", "hidden_fp16", "drop_k512", "cols_256")
SIM_MUTANTS = ("actions_prev", "store_after_update", "no_nan_map")
MUTANTS = NET_MUTANTS + SIM_MUTANTS
VARIANTS = ("recip_std", "no_contract", "mul_add")


def _r16(x):
    return O.round_bf16(np.asarray(x, np.float32))


def _dense32(h, W, b, fma):
    """float32 z = h W + b: per output one chain in k order starting from b; fma: fp64 product + sum rounded once"""
    acc = np.broadcast_to(np.asarray(b, np.float32), (h.shape[0], W.shape[1])).copy()
    if fma:
        h64, W64 = h.astype(np.float64), np.asarray(W, np.float64)
        for k in range(W.shape[0]):
            acc = (acc.astype(np.float64) + h64[:, k:k + 1] * W64[k]).astype(np.float32)
    else:
        W32 = np.asarray(W, np.float32)
        for k in range(W.shape[0]):
            acc = acc + h[:, k:k + 1] * W32[k]
    return acc


def _chain_rounding(h, W64, b):
    """R = sqrt(sum_k s_k^2): the chain's own roundings, one per partial sum s_k = b + h_0 W_0 + .. + h_k W_k (index order),
    independent of one another.  sum |terms| alone misses a chain whose partial sums all sit near a large early term (the
    bias of a unit the generator keeps active): K roundings of that size add up to about sqrt(K) of them"""
    s = np.broadcast_to(np.asarray(b, np.float64), (h.shape[0], W64.shape[1])).copy()
    acc = np.zeros(s.shape)
    for k in range(W64.shape[0]):
        s += h[:, k:k + 1] * W64[k]
        acc += s * s
    return np.sqrt(acc)


def network(x, Ex, Ws, bs, f32=False, mut=None, fma=True):
    """feedforward_network in fp64 (with E beside it when Ex is not None) or as the kernels' float32 chains"""
    h, Eh = (np.asarray(x, np.float32) if f32 else np.asarray(x, np.float64)), Ex
    L = len(Ws)
    for l in range(L):
        W, b = np.asarray(Ws[l], np.float32), np.asarray(bs[l], np.float32)
        if (mut == "bf16_arith" and l > 0) or mut == "weights_bf16":
            W = _r16(W)
        if mut == "drop_k512" and W.shape[0] > K_KCHUNK:
            W = W.copy()
            W[K_KCHUNK:] = 0.0
        if f32:
            z = _dense32(h, W, b, fma)
        else:
            W64 = W.astype(np.float64)
            z = h @ W64 + b.astype(np.float64)
            if Eh is not None:
                Eh = np.sqrt((Eh * Eh) @ (W64 * W64)) + np.abs(h) @ np.abs(W64) + np.abs(b.astype(np.float64)) + _chain_rounding(h, W64, b)
        if mut == "cols_256" and z.shape[1] > K_COLS:
            z = z.copy()
            z[:, K_COLS:] = z[:, :z.shape[1] - K_COLS]
            if Eh is not None:
                Eh = Eh.copy()
                Eh[:, K_COLS:] = Eh[:, :z.shape[1] - K_COLS]
        if l == L - 1:
            return z, Eh
        mask = z > 0
        h = np.maximum(z, z.dtype.type(0))
        if Eh is not None:
            Eh = Eh * mask
        if mut == "bf16_arith":
            h = _r16(h).astype(h.dtype)
        elif mut == "hidden_fp16":
            h = h.astype(np.float16).astype(h.dtype)


def _normalise(x, Ex, mean, std, f32, mut, recip):
    """z-score with np.nan_to_num's mapping: (v, E(v)); mean / std: the float32 statistics"""
    mean32, std32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if f32:
            dx = np.asarray(x, np.float32) - mean32
            v = dx * (np.float32(1) / std32) if recip else dx / std32
        else:
            dx = np.asarray(x, np.float64) - mean32.astype(np.float64)
            v = dx / std32.astype(np.float64)
        E = None
        if Ex is not None:
            std64 = std32.astype(np.float64)
            E = np.where(std64 > 0, (Ex + np.abs(dx)) / np.where(std64 > 0, std64, 1.0) + np.abs(np.nan_to_num(v)), 0.0)
    big = np.finfo(v.dtype).max
    v = np.where(np.isinf(v), np.sign(v) * big, v)
    if mut != "no_nan_map":
        v = np.where(np.isnan(v), v.dtype.type(0), v)
    return v, E


def simulate(inp, f32=False, mut=None, variant=None, params=None, sizes=False):
    """[H+1, m, d] trajectories of every row (fp64, or float32 values as fp64) and, fp64 with ``sizes``, A of the same shape.
    ``mut``: one of MUTANTS, or None; ``variant``: one of VARIANTS (float32 only), or None; ``params``: (Ws, bs, norm)
    replacing the case's own (net_mutants)."""
    Ws, bs, norm = params if params is not None else (inp.Ws, inp.bs, inp.norm)
    nm = {k: np.asarray(v, np.float32) for k, v in norm.items()}
    T = np.float32 if f32 else np.float64
    sizes = sizes and not f32
    S = np.asarray(inp.s0_rows, T)
    E = np.zeros(S.shape) if sizes else None
    out, Eout = [], []
    for t in range(inp.case.H):
        out.append(S)
        Eout.append(E)
        A_t = inp.A[:, max(t - 1, 0) if mut == "actions_prev" else t, :]
        xs, Exs = _normalise(S, E, nm["mean_x"], nm["std_x"], f32, mut, variant == "recip_std")
        ys, Eys = _normalise(A_t, np.zeros(A_t.shape) if sizes else None, nm["mean_y"], nm["std_y"], f32, mut, variant == "recip_std")
        x = np.concatenate([xs, ys], axis=1)
        Ex = np.concatenate([Exs, Eys], axis=1) if sizes else None
        z, Ez = network(x, Ex, Ws, bs, f32, mut, fma=variant != "mul_add")
        if f32:
            if variant == "no_contract":
                u = z * nm["std_z"] + nm["mean_z"]
            else:
                u = (z.astype(np.float64) * nm["std_z"].astype(np.float64) + nm["mean_z"].astype(np.float64)).astype(np.float32)
            S = S + u
        else:
            zs = z * nm["std_z"].astype(np.float64)
            u = zs + nm["mean_z"].astype(np.float64)
            Sn = S + u
            if sizes:
                E = E + nm["std_z"].astype(np.float64) * Ez + np.abs(zs) + np.abs(u) + np.abs(Sn)
            S = Sn
    out.append(S)
    Eout.append(E)
    if mut == "store_after_update":
        out = out[1:] + out[-1:]
    X = np.stack(out).astype(np.float64)
    return (X, np.stack(Eout)) if sizes else X


def mlp_forward(inp, f32=False, mut=None, variant=None, params=None, sizes=False):
    """ssc_mlp_forward alone: [m, out] (and its A, fp64 with ``sizes``)"""
    Ws, bs = params if params is not None else (inp.Ws, inp.bs)
    Ex = np.zeros(inp.x.shape) if sizes and not f32 else None
    z, Ez = network(inp.x, Ex, Ws, bs, f32, mut, fma=variant != "mul_add")
    z = z.astype(np.float64)
    return (z, Ez) if sizes and not f32 else z


_REF = {}


def reference(case):
    """(ref, A) of a case, fp64; computed once, read-only"""
    if case.name not in _REF:
        inp = mlp_inputs(case) if isinstance(case, MlpCase) else build_inputs(case)
        ref, A = (mlp_forward if isinstance(case, MlpCase) else simulate)(inp, sizes=True)
        ref.setflags(write=False)
        A.setflags(write=False)
        _REF[case.name] = (ref, A)
    return _REF[case.name]


# -------------------------------------------------------------------------------------------------------------- bounds --
def ratio(err, allowed):
    """max err / allowed over all elements; where allowed is 0 err must be 0; a NaN counts as infinitely far"""
    err, allowed = np.asarray(err, np.float64), np.asarray(allowed, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(allowed > 0, err / allowed, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(np.max(q)) if q.size else 0.0


def bound_ratios(X, ref, A, c=C_F32):
    """(state, increment): max |X - ref| / (c 2^-24 A) and max |dX - dref| / (c 2^-24 (A_t + A_t+1)); a forward alone
    ([m, out]) has no increments (0)"""
    X = np.asarray(X, np.float64)
    state = ratio(np.abs(X - ref), c * EPS32 * A)
    if X.ndim < 3:
        return state, 0.0
    inc = ratio(np.abs(np.diff(X, axis=0) - np.diff(ref, axis=0)), c * EPS32 * (A[:-1] + A[1:]))
    return state, inc


def r_case(case, variant=None):
    """max of the two ratios of the float32 emulation in units of 2^-24 A (c = 1)"""
    ref, A = reference(case)
    inp = mlp_inputs(case) if isinstance(case, MlpCase) else build_inputs(case)
    X = (mlp_forward if isinstance(case, MlpCase) else simulate)(inp, f32=True, variant=variant)
    return max(bound_ratios(X, ref, A, 1.0))


# ------------------------------------------------------------------------------------------------------------ mutants --
def net_mutants(inp):
    """sim_cases.mutants() per layer width, as (name, Ws, bs, norm): two live hidden units' outgoing rows swapped, a live
    unit among each hidden layer's last 32 - width % 32 dropped, unit 0 dropped, one state input fed raw (among those with
    std != 0), the last action ignored, std_z of one output applied to another.  The network-only inputs of ssc_mlp_forward
    (MlpInputs) get the weight edits alone.  Equal to sim_cases.mutants() where that applies (the CPU test holds it)."""
    Ws, bs = inp.Ws, inp.bs
    sim = isinstance(inp, Sim32Inputs)
    x = inp.x0 if sim else inp.x
    norm = inp.norm if sim else None
    acts = SC.hidden_activity(x, Ws, bs)
    out = []

    def with_W(l, edit):
        W2 = [w.copy() for w in Ws]
        edit(W2[l])
        return W2

    def swap(u, v):
        def f(W):
            W[[u, v]] = W[[v, u]]
        return f

    def drop(u):
        def f(W):
            W[u] = 0.0
        return f

    for l, act in enumerate(acts):                    # hidden layer l feeds Ws[l + 1]
        tag = "last" if l == len(acts) - 1 else "w2"
        depth = act.shape[1]
        tail = list(range(depth - (32 - depth % 32), depth))
        if depth >= 2:
            u, v = SC._swap_pair(act, np.asarray(Ws[l + 1], np.float64))
            out.append((f"swap_{tag}_{u}_{v}", with_W(l + 1, swap(u, v)), bs, norm))
        live = SC._live_units(act)
        live_tail = [t for t in live if t in tail]
        assert live_tail and 0 in live, (inp.case.name, l, "the tail units / unit 0 are dead at these inputs")
        W_out = np.abs(np.asarray(Ws[l + 1], np.float64)).max(axis=1)
        t = max(live_tail, key=lambda q: act[:, q].mean() * W_out[q])
        out.append((f"drop_{tag}_tail_{t}", with_W(l + 1, drop(t)), bs, norm))
        out.append((f"drop_{tag}_unit0", with_W(l + 1, drop(0)), bs, norm))
    if not sim:
        return out
    nm = SC.norm32(norm)
    moving = np.nonzero(nm["std_x"] > 0)[0]
    j = int(moving[np.argmax(np.mean(np.abs(inp.x0[:, moving] - inp.s0_rows[:, moving]), axis=0))])
    n2 = {k: np.array(v, np.float64) for k, v in nm.items()}
    n2["mean_x"][j], n2["std_x"][j] = 0.0, 1.0
    out.append((f"skip_norm_x{j}", Ws, bs, n2))
    out.append(("ignore_last_action", with_W(0, drop(inp.case.dims[0] - 1)), bs, norm))
    n3 = {k: np.array(v, np.float64) for k, v in nm.items()}
    n3["std_z"] = np.roll(n3["std_z"], 1)
    out.append(("std_z_shifted", Ws, bs, n3))
    return out


def all_mutants(inp):
    """every mutant of a case as (name, kwargs of simulate / mlp_forward)"""
    sim = isinstance(inp, Sim32Inputs)
    out = [(name, dict(params=(W, b, n) if sim else (W, b))) for name, W, b, n in net_mutants(inp)]
    out += [(m, dict(mut=m)) for m in (MUTANTS if sim else NET_MUTANTS)]
    return out
