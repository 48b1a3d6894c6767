"""Dispatch matrix of the dynamics-model training step (csrc/dyn_train.hip: ssc_mlp_train_steps): the case table, each
case's inputs, the fp64 gradients with the size of the terms they are made of, a float32 emulation of the step, the
bound derived from the two, and the emulation mutants that bound must reject.  Shared by the CPU test
(tests/test_dyn_train_cases_cpu.py) and the GPU test (tests/test_gpu_dyn_train_matrix.py); numpy + oracle only.

Why gradients.  Adam is scale-invariant: from zero moments the first step is lr * sign(g) whatever |g| is, so a
gradient wrong by a constant factor, a row block counted twice or a mis-scaled bias gradient leaves the parameters where
the oracle puts them.  It shows in the moments only: after one step from zero moments m = (1 - beta1) g and
v = (1 - beta2) g^2, and that is where the device gradient is read back from.

The bound.  ``grad64`` = the algebra of O.mlp_train_step in fp64 on the float32 inputs the kernel receives, ``emu32`` =
the same step in float32, one rounding per operation (no fma), every dot product accumulated strictly in index order
(the least favourable order).  Beside the fp64 pass the same passes run on absolute values,

    Ha_0 = |x|,  Ha_{l+1} = Ha_l |W_l| + |b_l|          D_L = 2 (Ha_L + |z|) / (B out),  D_l = (D_{l+1} |W_l|^T) * mask_l
    A_W[l] = (Ha_l * mask_l)^T D_{l+1}                  A_b[l] = sum_rows D_{l+1}

(mask_l = the fp64 ReLU mask of layer l's input, all ones for l = 0), so A is the size of the terms a gradient element
is made of and r_case = max |emu32 - g64| / (2^-24 A) is what float32 costs at that case in units of one rounding of A.
A gradient g of the kernel is accepted when |g - g64| <= C_GRAD * 2^-24 * A with C_GRAD = 4 * max_cases r_case: the
factor 4 is for fma contraction, the MFMA's internal order and the block / wave / tile partial sums.  The loss is held
the same way against mean((Ha_L + |z|)^2) with C_LOSS.  Both constants are fixed here, without the kernel.

Stability.  ReLU is a discontinuity.  The generator computes every hidden pre-activation of every candidate row in fp64
and builds the batch of the bounded step only from rows whose smallest |pre| is at least THR; after that no element is
left out of any assertion.

The two B = 65536 rows are kept out of the sequential emulation (its python loop over the batch would dominate the CPU
test's time); their bound uses the C_GRAD / C_LOSS of the other rows.
"""
import zlib
from collections import namedtuple

import numpy as np

EPS32 = 2.0 ** -24
THR = 1e-4              # smallest |hidden pre-activation| a row of the bounded batch may have
C_GRAD = 17.5           # 4 * max r_case of the table below, rounded up to the next half (tests/test_dyn_train_cases_cpu.py recomputes it)
C_LOSS = 6.0            # the same for the loss
LR, BETA1, BETA2, EPSILON = 1e-3, 0.9, 0.999, 1e-8       # tf.train.AdamOptimizer defaults, as navigator.DynamicsModel passes them
SSC_MAX_LAYERS = 4

# the kernel's own float32 coefficients evaluated in fp64: 1 - 0.999f differs from 0.001 by 2e-6 relative
C1 = float(np.float32(1.0) - np.float32(BETA1))
C2 = float(np.float32(1.0) - np.float32(BETA2))
# the bias-corrected step size of step 1 as both paths compute it: in double from the float32 arguments, rounded to float32
LR1 = float(np.float32(float(np.float32(LR)) * np.sqrt(1.0 - float(np.float32(BETA2))) / (1.0 - float(np.float32(BETA1)))))

# name, layer widths, batch rows, and what ssc_mlp_train_steps launches for it (read off the dispatch code):
#   path "fused":   kernel = mlp_train_fused_kernel instantiation, hd_pad (S = 512 / hd_pad row sub-slices per unit), G = blocks,
#                   P = parameters and its class against the Adam loop's kU * kFT = 2048 stride, lds_optin = more than 64 KB of LDS
#   path "generic": gemms = (role, M, N, K, per-wave class of K, 16-byte loads) of every GEMM of the chain
# null_loss: the GPU test runs steps 2-4 a second time with d_loss = NULL; emulate: part of the sequential float32 emulation
DynCase = namedtuple("DynCase", "name dims B path kernel hd_pad S G P p_class lds_optin gemms null_loss emulate")


def k_class(K):
    """how gemm32_tile walks a contraction of length K: the 4 waves take ksz = roundup8(ceil(K / 4)) values each in
    double-buffered chunks of 32"""
    ksz = (((K + 3) >> 2) + 7) & ~7
    if K <= 8:
        return "one_wave"
    return "c32" if ksz <= 32 else "c64" if ksz <= 64 else "c96" if ksz <= 96 else "c97+"


def last_wave_short(K):
    ksz = (((K + 3) >> 2) + 7) & ~7
    return K > 3 * ksz and K - 3 * ksz < ksz


def _c(name, dims, B, null_loss=False):
    dims = tuple(dims)
    L = len(dims) - 1
    fused = L == 2 and dims[0] <= 12 and dims[1] <= 512 and dims[2] <= 8          # fused_eligible
    emulate = B < 65536
    if fused:
        i, h, o = dims
        IN, OUT = (3, 2) if (i <= 3 and o <= 2) else (4, 3) if (i <= 4 and o <= 3) else (12, 8)
        hd_pad = 16
        while hd_pad < h:
            hd_pad *= 2
        S = 512 // hd_pad
        lds = 32 * (hd_pad + 1) + hd_pad * OUT + 32 * IN + 2 * 32 * OUT + (512 * (IN + 1 + OUT) if S > 1 else 0) + 32 + 8
        P = i * h + h + h * o + o
        return DynCase(name, dims, B, "fused", "<%d,%d>" % (IN, OUT), hd_pad, S, (B + 31) // 32, P,
                       "lt512" if P < 512 else "512_2048" if P <= 2048 else "gt2048", lds * 4 > 64 * 1024, (), null_loss, emulate)
    gemms = []
    for l in range(L):
        gemms.append(("fwd", B, dims[l + 1], dims[l], k_class(dims[l]), dims[l] % 4 == 0))
    for l in range(L - 1, 0, -1):
        gemms.append(("bwd", B, dims[l], dims[l + 1], k_class(dims[l + 1]), dims[l + 1] % 4 == 0))
    for l in range(L):
        gemms.append(("wgrad", dims[l] + 1, dims[l + 1], B, k_class(B), False))
    return DynCase(name, dims, B, "generic", "gemm32", 0, 0, 0, sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(L)), "-",
                   False, tuple(gemms), null_loss, emulate)


CASES = [
    # ---- fused kernel <3,2>: in / out at the template size and below it, hd_pad 16 .. 512
    _c("f32_h32_b512", (3, 32, 2), 512, null_loss=True),       # the shipped example; G = 16: one full trip of the ordered sum
    _c("f32_h1_b1", (2, 1, 1), 1),
    _c("f32_h16_b31", (1, 16, 1), 31),
    _c("f32_h17_b33", (3, 17, 2), 33),
    _c("f32_h500_b513", (3, 500, 2), 513),                     # hd_pad 512 (S = 1, > 64 KB LDS), P = 3002, G = 17
    _c("f32_h32_b65536", (3, 32, 2), 65536),
    # ---- fused kernel <4,3>
    _c("f43_h33_b32", (4, 33, 3), 32),
    _c("f43_h100_b544", (3, 100, 3), 544, null_loss=True),     # P = 703, G = 17
    _c("f43_h17_b2049", (4, 17, 2), 2049),
    _c("f43_h256_b33", (4, 256, 3), 33),                       # P = 2051, just above one trip of the Adam loop
    _c("f43_h500_b512", (4, 500, 3), 512),                     # the class default; P = 4003
    _c("f43_h257_b1", (4, 257, 3), 1),
    # ---- fused kernel <12,8>
    _c("f128_h256_b33", (12, 256, 8), 33, null_loss=True),     # hd_pad 256 opts in to > 64 KB LDS as well
    _c("f128_h16_b513", (5, 16, 1), 513),
    _c("f128_h512_b31", (4, 512, 8), 31),
    _c("f128_h100_b32", (12, 100, 8), 32),
    _c("f128_h1_b33", (12, 1, 8), 33),
    # ---- generic chain: no hidden layer
    _c("g_l1_b33", (5, 3), 33),
    _c("g_l1_b500", (5, 3), 500),                              # weight gradient: K = 500, the last wave shorter than the others
    # ---- one hidden layer just outside the fused kernel's reach
    _c("g_in13", (13, 16, 3), 77, null_loss=True),
    _c("g_hd513", (4, 513, 3), 33),
    _c("g_out9", (4, 16, 9), 1),
    # ---- tile edges: dims 31 (ones row = last row of a tile), 32 (ones row alone in a second tile row), N = 32 / 33,
    #      out = 33 with B > 32 (loss_part: 3 x 2 tiles)
    _c("g_edges", (8, 31, 32, 33), 77, null_loss=True),
    # ---- every class of K for every GEMM role
    _c("g_k200", (3, 4, 200, 2), 200),
    _c("g_k300", (2, 3, 300, 1), 300),
    _c("g_k500", (3, 4, 500, 2), 33),
    _c("g_l4", (3, 40, 24, 16, 2), 77),                        # SSC_MAX_LAYERS, unequal widths: gradient tiles of the smaller layers leave early
    _c("g_b513", (3, 8, 8, 2), 513),
    _c("g_b65536", (3, 8, 8, 2), 65536),
]
CASE_BY_NAME = {c.name: c for c in CASES}

MUTANTS = ("delta_2_over_B", "drop_last_row", "bias_zero", "drop_k_chunk", "mask_ge0", "block_twice", "loss_div_B")


# ---------------------------------------------------------------------------------------------------------- generator --
def make_mlp(rng, dims):
    """xavier-normal weights AND biases (feedforward_network.py:8,14-23), float32"""
    Ws = [rng.normal(size=(dims[i], dims[i + 1])) * np.sqrt(2.0 / (dims[i] + dims[i + 1])) for i in range(len(dims) - 1)]
    bs = [rng.normal(size=dims[i + 1]) * np.sqrt(2.0 / (1 + dims[i + 1])) for i in range(len(dims) - 1)]
    return [w.astype(np.float32) for w in Ws], [b.astype(np.float32) for b in bs]


def row_margin(Ws, bs, X):
    """smallest |hidden pre-activation| of every row of X in fp64 (inf for a net without a hidden layer)"""
    h = np.asarray(X, np.float64)
    m = np.full(h.shape[0], np.inf)
    for W, b in zip(Ws[:-1], bs[:-1]):
        pre = h @ W.astype(np.float64) + b.astype(np.float64)
        m = np.minimum(m, np.abs(pre).min(axis=1))
        h = np.maximum(pre, 0.0)
    return m


_CACHE = {}


def case_data(case):
    """dict(Ws, bs, X [n, in], Z [n, out] float32, idx [4, B] int32): step 1 trains on rows idx[0], all of them at least
    THR from every ReLU kink and row 0 and row n - 1 among them (B = 1: row n - 1; row 0 leads idx[1]); steps 2-4 on
    idx[1:], any rows.  Deterministic in the case's name, computed once, read-only."""
    if case.name not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        B = case.B
        Ws, bs = make_mlp(rng, case.dims)
        n = 3 * B + 64
        X = rng.normal(size=(n, case.dims[0])).astype(np.float32)
        Z = (0.5 * rng.normal(size=(n, case.dims[-1]))).astype(np.float32)
        margin = row_margin(Ws, bs, X)
        for r in (0, n - 1):
            for _ in range(1000):
                if margin[r] >= THR:
                    break
                X[r] = rng.normal(size=case.dims[0]).astype(np.float32)
                margin[r] = row_margin(Ws, bs, X[r:r + 1])[0]
        good = np.nonzero(margin >= THR)[0]
        ends = [n - 1] if B == 1 else [0, n - 1]
        inner = good[(good != 0) & (good != n - 1)]
        assert margin[0] >= THR and margin[n - 1] >= THR and inner.size >= B - len(ends), (case.name, good.size)
        idx0 = rng.permutation(np.concatenate([ends, rng.permutation(inner)[:B - len(ends)]]))
        more = np.stack([rng.permutation(n)[:B] for _ in range(3)])
        more[0, 0] = 0 if 0 not in more[0] else more[0, 0]
        idx = np.concatenate([idx0[None], more]).astype(np.int32)
        out = dict(Ws=Ws, bs=bs, X=X, Z=Z, idx=idx, good_share=good.size / n)
        for a in Ws + bs + [X, Z, idx]:
            a.setflags(write=False)
        _CACHE[case.name] = out
    return _CACHE[case.name]


# ---------------------------------------------------------------------------------------------------- fp64 reference --
def grad64(Ws, bs, x, z):
    """O.mlp_train_step's forward, loss and back-propagation restated with what the bound needs computed beside them: dict
    gW, gb (lists, fp64), loss, A_W, A_b (the error scales of the docstring above), A_loss = mean((Ha_L + |z|)^2), margin =
    smallest |hidden pre-activation|, pre (list of the hidden pre-activations)."""
    Ws = [np.asarray(w, np.float64) for w in Ws]
    bs = [np.asarray(b, np.float64) for b in bs]
    L = len(Ws)
    acts, Ha, masks, pres = [np.asarray(x, np.float64)], [np.abs(np.asarray(x, np.float64))], [None], []
    for l in range(L):
        pre = acts[-1] @ Ws[l] + bs[l]
        ha = Ha[-1] @ np.abs(Ws[l]) + np.abs(bs[l])
        if l < L - 1:
            pres.append(pre)
            acts.append(np.maximum(pre, 0.0))
            masks.append(pre > 0)
            Ha.append(ha)
    y, zz = pre, np.asarray(z, np.float64)
    dz = 2.0 * (y - zz) / y.size
    D = 2.0 * (ha + np.abs(zz)) / y.size
    gW, gb, A_W, A_b = [None] * L, [None] * L, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        gW[l], gb[l] = acts[l].T @ dz, dz.sum(0)
        A_W[l], A_b[l] = (Ha[l] * masks[l] if l else Ha[l]).T @ D, D.sum(0)
        if l > 0:
            dz = (dz @ Ws[l].T) * masks[l]
            D = (D @ np.abs(Ws[l]).T) * masks[l]
    return dict(gW=gW, gb=gb, loss=float(np.mean((zz - y) ** 2)), A_W=A_W, A_b=A_b, A_loss=float(np.mean((ha + np.abs(zz)) ** 2)),
                margin=min([float(np.abs(p).min()) for p in pres] + [np.inf]), pre=pres)


_REF = {}


def reference(case):
    """grad64 of the case's first batch; computed once, never modified"""
    if case.name not in _REF:
        d = case_data(case)
        ref = grad64(d["Ws"], d["bs"], d["X"][d["idx"][0]], d["Z"][d["idx"][0]])
        for a in ref["gW"] + ref["gb"] + ref["A_W"] + ref["A_b"]:
            a.setflags(write=False)
        _REF[case.name] = ref
    return _REF[case.name]


def ratio(err, allowed):
    """max err / allowed over all elements; an element whose allowed error is zero (a unit no row of the batch activates:
    every term of its gradient is zero) must be exact"""
    err, allowed = np.asarray(err, np.float64), np.asarray(allowed, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(allowed > 0, err / allowed, np.where(err == 0, 0.0, np.inf))
    return float(np.max(q)) if q.size else 0.0


def grad_ratio(ref, gW, gb):
    """max |g - g64| / (2^-24 A) over every element of every parameter"""
    return max(max(ratio(np.abs(gW[l] - ref["gW"][l]), EPS32 * ref["A_W"][l]), ratio(np.abs(gb[l] - ref["gb"][l]), EPS32 * ref["A_b"][l]))
               for l in range(len(gW)))


def loss_ratio(ref, loss):
    return abs(float(loss) - ref["loss"]) / (EPS32 * ref["A_loss"])


def _u(g):
    """the fp64 Adam update of step 1 from zero moments, with the kernel's coefficients; monotone in g"""
    return LR1 * C1 * g / (np.sqrt(C2 * g * g) + EPSILON)


def step1_ratios(theta0, g64, A, m, v, theta1):
    """One parameter array after step 1 from zero moments against the fp64 gradient: (m, v, theta), each the largest
    err / allowed over all elements, <= 1 accepted.  delta = C_GRAD 2^-24 A;
        |m - c1 g64| <= c1 delta + 2^-24 |c1 g64|            |v - c2 g64^2| <= c2 (2 |g64| delta + delta^2) + 3 2^-24 c2 g64^2
        theta1 in theta0 - [u(g64 + delta), u(g64 - delta)] widened by w = 8 2^-24 |u| + 2^-23 |theta0|
    (theta: 1 + the distance outside the interval in units of w, so that inside is <= 1 as well)."""
    theta0, g64, A, m, v, theta1 = (np.asarray(a, np.float64) for a in (theta0, g64, A, m, v, theta1))
    delta = C_GRAD * EPS32 * A
    rm = ratio(np.abs(m - C1 * g64), C1 * delta + EPS32 * np.abs(C1 * g64))
    rv = ratio(np.abs(v - C2 * g64 * g64), C2 * (2 * np.abs(g64) * delta + delta * delta) + 3 * EPS32 * C2 * g64 * g64)
    u_hi, u_lo = _u(g64 + delta), _u(g64 - delta)
    w = 8 * EPS32 * np.maximum(np.abs(u_hi), np.abs(u_lo)) + 2 * EPS32 * np.abs(theta0)
    outside = np.maximum(np.maximum((theta0 - u_hi - w) - theta1, theta1 - (theta0 - u_lo + w)), 0.0)
    rt = ratio(np.where(outside > 0, outside + w, 0.0), w)
    return rm, rv, rt


# ---------------------------------------------------------------------------------------------------- fp32 emulation --
def _dot_seq(a, b, skip=()):
    """a [M, K] @ b [K, N] in float32, one rounding per multiplication and per addition, k strictly in order"""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        if k in skip:
            continue
        acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    return acc


def emu32(Ws, bs, x, z, mutant=None):
    """Forward, loss and back-propagation of one step in float32 numpy: dict gW, gb (lists), loss, pre (hidden
    pre-activations).  ``mutant``: one of MUTANTS, a wrong kernel:
      delta_2_over_B   output delta scaled by 2 / B instead of 2 / (B out)
      drop_last_row    the last row of the batch left out of every gradient sum and of the loss
      bias_zero        no ones row: the bias gradients are zero
      drop_k_chunk     the last 32-value chunk of wave 0 dropped from the last layer's weight-gradient GEMM (K = B)
      mask_ge0         the ReLU mask taken as activation >= 0, which holds for every unit: the delta of a unit that is
                       off reaches its bias and weight gradients
      block_twice      the first 32-row block summed twice into every gradient
      loss_div_B       the loss divided by B only"""
    f = np.float32
    assert mutant is None or mutant in MUTANTS
    Ws, bs = [np.asarray(w, f) for w in Ws], [np.asarray(b, f) for b in bs]
    x, z = np.asarray(x, f), np.asarray(z, f)
    L, (B, out) = len(Ws), z.shape
    acts, pres = [x], []
    for l in range(L):
        pre = _dot_seq(acts[-1], Ws[l]) + bs[l]
        if l < L - 1:
            pres.append(pre)
            acts.append(np.maximum(pre, f(0)))
    rows = B - 1 if (mutant == "drop_last_row" and B > 1) else B
    d = pre - z
    sq = d * d
    acc = f(0)
    for e in sq[:rows].reshape(-1):
        acc = acc + e
    loss = acc / (f(B) if mutant == "loss_div_B" else f(B * out))
    dz = d * (f(2) / (f(B) if mutant == "delta_2_over_B" else f(B * out)))
    gW, gb = [None] * L, [None] * L
    ones = np.ones((1, B), f)
    for l in range(L - 1, -1, -1):
        skip = ()
        if mutant == "drop_k_chunk" and l == L - 1:
            ke = min((((B + 3) >> 2) + 7) & ~7, B)
            skip = range(ke - ((ke - 1) % 32 + 1), ke)
        hT = np.ascontiguousarray(acts[l].T)
        gW[l], gb[l] = _dot_seq(hT[:, :rows], dz[:rows], skip), _dot_seq(ones[:, :rows], dz[:rows])[0]
        if mutant == "block_twice":
            gW[l], gb[l] = gW[l] + _dot_seq(hT[:, :32], dz[:32]), gb[l] + _dot_seq(ones[:, :32], dz[:32])[0]
        if mutant == "bias_zero":
            gb[l] = np.zeros_like(gb[l])
        if l > 0:
            back = _dot_seq(dz, np.ascontiguousarray(Ws[l].T))
            dz = np.where(acts[l] >= 0 if mutant == "mask_ge0" else acts[l] > 0, back, f(0))
    return dict(gW=gW, gb=gb, loss=loss, pre=pres)


def adam1_32(theta, g):
    """step 1 of Adam from zero moments in float32, one rounding per operation: (m, v, theta1)"""
    f = np.float32
    theta, g = np.asarray(theta, f), np.asarray(g, f)
    m = f(BETA1) * f(0) + (f(1) - f(BETA1)) * g
    v = f(BETA2) * f(0) + (f(1) - f(BETA2)) * g * g
    return m, v, theta - f(LR1) * m / (np.sqrt(v) + f(EPSILON))


def emu32_of(case, mutant=None):
    d = case_data(case)
    return emu32(d["Ws"], d["bs"], d["X"][d["idx"][0]], d["Z"][d["idx"][0]], mutant)
