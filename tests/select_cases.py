"""The SmartStart selection kernels (csrc/smartstart.hip: kde_kernel<1|2|3|0>, ucb_kernel): the case tables, each case's
inputs, the fp64 reference with its per-query error scale, a float32 emulation of each kernel's arithmetic, the bounds
derived from the two, and the emulation mutants the KDE bound must reject.  Shared by the CPU test
(tests/test_select_cases_cpu.py) and the GPU tests (tests/test_gpu_select_matrix.py, tests/test_gpu_agents.py); numpy only.

KDE bound.  ``ref`` = O.kde_evaluate in fp64 on the float32 data, queries and whitening the kernel receives.  In the
kernel's scaled units (whitening times kS = sqrt(0.5 log2 e), so that a term is w_ij = 2^-e_ij), with t = Whs x_q - Whs x_j
and Y = |Whs| |x| (absolute values elementwise: the size of the products a whitened coordinate is summed from),

    A_i = norm * sum_j w_ij * (2 + 1 + ln2 * (e_ij + 2 sum_r |t_r| (Yq_r + Yj_r + |t_r|))) + norm * n * 2^-126

is the size, in units of 2^-24, of what float32 can cost query i: 2 for the 1-ulp hardware exp2, 1 for the additions, the
ln2 (...) term for the error of the exponent (e itself through the rounded whitening and kS, and the cancellation in
Whs x_q - Whs x_j, which grows with the distance of the data from the origin), and the flush floor.  A pdf X is accepted
when |X - ref| <= C_KDE * 2^-24 * A_i, C_KDE = 4 * max_cases r_case, r_case = max_i |emu - ref| / (2^-24 A_i) with ``emu`` =
``kde_emu32``; the factor 4 covers contraction and ordering the emulation does not model.  Fixed here, without the kernel.

The flush band.  The raw hardware exp2 returns 0 below 2^-126 where fp64 does not.  The floor above stands in the scale,
i.e. it is multiplied by C_KDE * 2^-24 like everything else, so it covers flushed terms beside a term that survives (the
survivor is >= 2^-126, the flushed ones are 2^-24 of it each at most after a few bandwidths) and a query whose every
term is far below 2^-126 (ref < norm n 2^-150), but NOT a query whose largest term sits between about 2^-150 and 2^-100:
there the kernel returns 0 or a few surviving terms for a reference of the same size, a relative error of order one on a
density of 1e-38 of a single point's weight.  The next kernel turns either into a bonus beyond 1e17; no decision rests on
it.  The table keeps its queries out of that band (``band_free``, asserted by the CPU test): every query has a term
>= 2^-90 or none above 2^-160.

UCB bound.  ``ref`` = O.smart_start_ucb in fp64 on the float32 values and pdf.  ucb_kernel forms the bonus in fp64, rounds
it to float32 and adds alpha * value by one float32 multiply-add: two roundings, of sizes bonus and |ucb|.
A_i = |alpha v_i| + bonus_i + |ucb_i|; a score is accepted when |X - ref| <= C_UCB * 2^-24 * A_i, C_UCB = 4 * max r_case.
"""
import zlib
from collections import namedtuple

import numpy as np

EPS32 = 2.0 ** -24
FLUSH = 2.0 ** -126
KS64 = float(np.sqrt(0.5 * np.log2(np.e)))
KS32 = np.float32(0.84932180028801904272)       # kde_kernel's kS
K_THREADS, K_U, K_Q, K_WAVES = 1024, 4, 8, 16   # kKdeThreads, kKdeU, kKdeQ, waves per block
TRIP = K_THREADS * K_U                          # data points per trip of the data loop
PAD = 8                                         # NaN-prefilled output slots past m, which no kernel may touch
C_KDE = 2.6             # 4 * max r_case of KDE_CASES, rounded up (tests/test_select_cases_cpu.py recomputes it)
C_UCB = 3.6             # 4 * max r_case of UCB_CASES and their placements, rounded up

# name, state dim, data points, queries, data recipe, query recipe ("mix": every class in turn; else the one class of an
# m = 1 case), and the instantiation ssc_kde_evaluate launches for d (read off its dispatch: d <= 3 templated, else <0>)
KdeCase = namedtuple("KdeCase", "name d n m data queries kernel")


def _k(name, d, n, m, data, queries="mix"):
    return KdeCase(name, d, n, m, data, queries, "kde_kernel<%d>" % (d if d <= 3 else 0))


# n: 1, 5 below a wave; 63, 1023 below a block; 1024, 1025 one slot of a trip / one point into the second; 4095, 4096, 4097
# around one trip; 5121 = a trip + a full first slot + one point in the second; 9217 = two trips + that.
# m: 1; 7 below a query group; 8 one group; 9, 77 a ragged last group.
KDE_CASES = [
    _k("k1_n1_m1", 1, 1, 1, "iso", "out"),
    _k("k1_n63_m7", 1, 63, 7, "iso"),
    _k("k1_n4097_m9", 1, 4097, 9, "off30"),
    _k("k1_n9217_m77", 1, 9217, 77, "iso"),
    _k("k2_n5_m8", 2, 5, 8, "mcar"),
    _k("k2_n1023_m9", 2, 1023, 9, "corr"),
    _k("k2_n1024_m7", 2, 1024, 7, "iso"),
    _k("k2_n1025_m77", 2, 1025, 77, "mcar"),
    _k("k2_n4095_m8", 2, 4095, 8, "corr"),
    _k("k2_n4096_m9", 2, 4096, 9, "off1000"),
    _k("k2_n5121_m7", 2, 5121, 7, "mcar"),
    _k("k2_n9217_m1", 2, 9217, 1, "corr", "mid"),
    _k("k3_n63_m9", 3, 63, 9, "pend"),
    _k("k3_n1025_m8", 3, 1025, 8, "pend"),
    _k("k3_n4097_m77", 3, 4097, 77, "pend"),
    _k("k3_n5121_m7", 3, 5121, 7, "off30"),
    _k("k0_d4_n1_m7", 4, 1, 7, "iso"),
    _k("k0_d4_n4096_m9", 4, 4096, 9, "corr"),
    _k("k0_d5_n1025_m8", 5, 1025, 8, "scaled"),
    _k("k0_d5_n9217_m7", 5, 9217, 7, "off30"),
    _k("k0_d8_n5_m1", 8, 5, 1, "scaled", "copy"),
    _k("k0_d8_n4097_m77", 8, 4097, 77, "scaled"),
    _k("k0_d8_n5121_m9", 8, 5121, 9, "corr"),
]
KDE_CASE_BY_NAME = {c.name: c for c in KDE_CASES}
MIX = ("copy", "mid", "out1", "out2", "out3", "far", "dup")
FAR_BANDWIDTHS = 20.0      # kS^2 * 20^2 = 288: every float32 term is below 2^-126, the reference below norm n 2^-288

KDE_MUTANTS = ("drop_ragged_tail", "dead_lanes_one", "ks_sqrt_half", "wh_transposed", "skip_last_wave", "qi_le_m")


# ---------------------------------------------------------------------------------------------------------- generator --
def draw_data(recipe, rng, n, d):
    """n points of a data recipe, fp64 [n, d]"""
    z = rng.normal(size=(n, d))
    if recipe == "iso":
        return z
    if recipe == "scaled":
        return z * (1.0 + 0.5 * np.arange(d))
    if recipe == "corr":            # rho = 0.999 between the first two columns: a strongly non-symmetric whitening
        z[:, 1] = 0.999 * z[:, 0] + np.sqrt(1.0 - 0.999 ** 2) * z[:, 1]
        return z
    if recipe == "mcar":            # MountainCar: position 0.3 wide around -0.5, velocity 0.02 wide
        return z * np.array([0.3, 0.02]) + np.array([-0.5, 0.0])
    if recipe == "pend":            # Pendulum observations (cos theta, sin theta, theta-dot)
        th = rng.uniform(-np.pi, np.pi, n)
        return np.stack([np.cos(th), np.sin(th), np.clip(2.0 * z[:, 2], -8.0, 8.0)], axis=1)
    if recipe == "off30":
        return z + 30.0
    if recipe == "off1000":
        return z + 1000.0
    raise KeyError(recipe)


def bandwidth(sample, n):
    """Scott's bandwidth for n points with the covariance of ``sample`` (O.kde_scott when sample is the n points):
    (whitening float32 [d, d], norm)"""
    x = np.asarray(sample, np.float64)
    d = x.shape[1]
    cov = np.atleast_2d(np.cov(x, rowvar=False, bias=False)) * (n ** (-1.0 / (d + 4))) ** 2
    wh = np.linalg.cholesky(np.linalg.inv(cov)).T
    return np.ascontiguousarray(wh, np.float32), float(1.0 / (n * np.sqrt(np.linalg.det(2 * np.pi * cov))))


_CACHE = {}


def kde_case_data(case):
    """dict(data [n, d], points [m, d], wh [d, d] float32, norm, cls [m] query class names, dup_of {i: source query},
    own_bandwidth: the whitening is Scott's of the data itself (n >= d + 2; else of 512 draws of the same recipe)).
    Deterministic in the case's name, computed once, read-only."""
    if case.name in _CACHE:
        return _CACHE[case.name]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    n, d, m = case.n, case.d, case.m
    data = draw_data(case.data, rng, n, d).astype(np.float32)
    own = n >= d + 2
    wh, norm = bandwidth(data if own else draw_data(case.data, rng, 512, d), n)
    x = data.astype(np.float64)
    w64 = wh.astype(np.float64)
    y = x @ w64.T
    cls = [MIX[i % len(MIX)] for i in range(m)] if case.queries == "mix" else [case.queries] * m
    pts = np.zeros((m, d))
    dup_of = {}
    for i, c in enumerate(cls):
        if c == "copy":
            pts[i] = x[rng.integers(n)]
        elif c == "mid":
            pts[i] = 0.5 * (x[rng.integers(n)] + x[rng.integers(n)])
        elif c != "dup":            # k bandwidths beyond the outermost data point along a random whitened direction
            k = FAR_BANDWIDTHS if c == "far" else float(c[3:] or 1)
            u = rng.normal(size=d)
            u /= np.linalg.norm(u)
            pts[i] = x[int(np.argmax(y @ u))] + np.linalg.solve(w64, k * u)
    pts = pts.astype(np.float32)
    for i, c in enumerate(cls):
        if c == "dup":
            src = (i + 3) % m
            while cls[src] == "dup":
                src = (src + 1) % m
            pts[i] = pts[src]
            dup_of[i] = src
    for a in (data, pts, wh):
        a.setflags(write=False)
    _CACHE[case.name] = dict(data=data, points=pts, wh=wh, norm=norm, cls=cls, dup_of=dup_of, own_bandwidth=own)
    return _CACHE[case.name]


# ------------------------------------------------------------------------------------------ fp64 reference and scale --
def kde_scale(data, points, wh, norm):
    """fp64 on the kernel's float32 inputs -> dict(ref [m] = O.kde_evaluate restated as norm * sum 2^-e, A [m] the error
    scale of the module docstring, wmax [m] each query's largest term 2^-e)"""
    x, q = np.asarray(data, np.float64), np.asarray(points, np.float64)
    whs = np.asarray(wh, np.float64) * KS64
    n = len(x)
    yj, Yj = x @ whs.T, np.abs(x) @ np.abs(whs).T
    ref, A, wmax = np.empty(len(q)), np.empty(len(q)), np.empty(len(q))
    for i0 in range(0, len(q), 16):
        qq = q[i0:i0 + 16]
        t = np.abs((qq @ whs.T)[:, None, :] - yj[None, :, :])
        Yq = np.abs(qq) @ np.abs(whs).T
        e = (t * t).sum(-1)
        w = np.exp2(-e)
        inner = (t * (Yq[:, None, :] + Yj[None, :, :] + t)).sum(-1)
        ref[i0:i0 + 16] = norm * w.sum(1)
        A[i0:i0 + 16] = norm * (w * (3.0 + np.log(2.0) * (e + 2.0 * inner))).sum(1) + norm * n * FLUSH
        wmax[i0:i0 + 16] = w.max(1)
    return dict(ref=ref, A=A, wmax=wmax)


_REF = {}


def kde_reference(case):
    """kde_scale of a case plus bound = C_KDE * 2^-24 * A, flushed [m] (no float32 term survives) and band_free [m]
    (module docstring); computed once, read-only"""
    if case.name not in _REF:
        cd = kde_case_data(case)
        r = kde_scale(cd["data"], cd["points"], cd["wh"], cd["norm"])
        r["bound"] = C_KDE * EPS32 * r["A"]
        r["flushed"] = r["wmax"] < 2.0 ** -160
        r["band_free"] = (r["wmax"] >= 2.0 ** -90) | r["flushed"]
        for a in r.values():
            a.setflags(write=False)
        _REF[case.name] = r
    return _REF[case.name]


def kde_distance(x, ref, bound):
    """how far, in bounds, an output buffer [m + PAD] is from the reference: max_i |x_i - ref_i| / bound_i over the m
    queries (NaN counts as inf), inf if a slot past m no longer holds the NaN it was filled with"""
    m = len(ref)
    with np.errstate(invalid="ignore"):
        dd = np.abs(np.asarray(x[:m], np.float64) - ref) / bound
    worst = float(np.where(np.isnan(dd), np.inf, dd).max())
    return worst if np.isnan(x[m:]).all() else np.inf


# ---------------------------------------------------------------------------------------------------- fp32 emulation --
def _fma(a, b, c):
    """fmaf: the float32 product is exact in fp64, one rounding of the sum to fp64 and one to float32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _exp2_flush(neg_e):
    """exp2 correctly rounded to float32, results below 2^-126 flushed to 0"""
    x = np.exp2(np.asarray(neg_e, np.float64))
    return np.where(x < FLUSH, 0.0, x).astype(np.float32)


def kde_emu32(data, points, wh, norm, mutant=None):
    """kde_kernel in float32 numpy: wh * kS rounded to float32, the whitened points by fma chains over the columns, e by
    fma over the rows, exp2 correctly rounded and flushed, the float32 sum of thread j mod 1024 in the order of the data
    loop (trips of 4096, four slots of 1024 inside a trip), the fp64 wave butterfly and the fp64 sum over the 16 waves,
    one rounding of v * norm to float32.  Returns the output buffer [m + PAD], NaN beyond m.  ``mutant``: one of
    KDE_MUTANTS, a wrong kernel."""
    f = np.float32
    data, points, wh = (np.asarray(v, f) for v in (data, points, wh))
    (n, d), m = data.shape, len(points)
    whs = (wh * (f(np.sqrt(0.5)) if mutant == "ks_sqrt_half" else KS32)).astype(f)
    if mutant == "wh_transposed":
        whs = whs.T

    def whiten(x):
        y = np.zeros((len(x), d), f)
        for r in range(d):
            for c in range(d):
                y[:, r] = _fma(whs[r, c], x[:, c], y[:, r])
        return y

    yq, yj = whiten(points), whiten(data)
    slots = -(-n // K_THREADS)
    j = np.arange(slots * K_THREADS)
    live = j < (n if mutant != "drop_ragged_tail" else (n // TRIP) * TRIP)
    entered = (j // TRIP) * TRIP + j % K_THREADS < n       # the thread's j0 of that trip is below n: the trip runs
    lane = np.arange(64)
    out = np.full(m + PAD, np.nan, f)
    for q in range(m):
        e = np.zeros(n, f)
        for r in range(d):
            t = yq[q, r] - yj[:, r]
            e = _fma(t, t, e)
        term = np.zeros(len(j), f)
        term[:n] = _exp2_flush(-e)
        term[~live] = 0.0                                  # y[0] = inf: exp2(-inf) = 0
        if mutant == "dead_lanes_one":
            term[entered & ~live] = 1.0
        s = np.zeros(K_THREADS, f)
        for k in range(slots):
            s = s + term[k * K_THREADS:(k + 1) * K_THREADS]
        v = s.astype(np.float64).reshape(K_WAVES, 64)
        for msk in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ msk]
        tot = 0.0
        for w in range(K_WAVES - (1 if mutant == "skip_last_wave" else 0)):
            tot += v[w, 0]
        out[q] = f(tot * norm)
    if mutant == "qi_le_m" and m % K_Q != 0:               # thread m % 8 of the last group holds clamped query m - 1
        out[m] = out[m - 1]
    return out


def kde_emu32_of(case, mutant=None):
    cd = kde_case_data(case)
    return kde_emu32(cd["data"], cd["points"], cd["wh"], cd["norm"], mutant)


# ------------------------------------------------------------------------------------------------------------- UCB --
# name, candidates, exploitation alpha, exploration beta (both exact in float32), |D|, hyperellipsoid volume
UcbCase = namedtuple("UcbCase", "name m alpha beta buffer_len volume")
UCB_CASES = [UcbCase("u%d" % m, m, a, b, n, v) for m, a, b, n, v in [
    (1, 1.0, 2.0, 5000, 0.003), (63, 1.0, 2.0, 100000, 0.003), (64, 0.5, 2.0, 5000, 1.0), (65, 1.0, 0.5, 777, 6.3e-5),
    (255, 2.0, 2.0, 5000, 0.003), (256, 1.0, 2.0, 100000, 6.3e-5), (257, 1.0, 1.0, 5000, 0.003), (1000, 0.25, 2.0, 20000, 1.0),
    (4096, 1.0, 2.0, 500000, 0.003)]]
UCB_CASE_BY_NAME = {c.name: c for c in UCB_CASES}
# rows that hold exact copies of the best candidate: (the row it is built in, the copies).  A lower and a higher copy sit in
# another wave (row % 256 // 64) than that row wherever m has the waves; two copies share a wave in different lanes (the
# wave shuffle decides), and from m = 257 on two share a thread (rows 256 apart: the stride loop decides).
UCB_DUP_ROWS = {1: None, 63: (31, (3, 60)), 64: (33, (0, 63)), 65: (40, (2, 64)), 255: (100, (10, 20, 254)),
                256: (130, (5, 63, 255)), 257: (130, (0, 5, 256)), 1000: (300, (70, 100, 582, 999)),
                4096: (2049, (200, 250, 456, 4095))}


def ucb_base(case):
    """(values [m], pdf [m]) float32: values of a few units, densities over eight decades"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    values = (3.0 * rng.normal(size=case.m)).astype(np.float32)
    pdf = np.exp(rng.uniform(np.log(1e-6), np.log(1e2), case.m)).astype(np.float32)
    return values, pdf


def ucb_scale(values, pdf, case):
    """fp64 -> (ref = O.smart_start_ucb's scores, A the error scale); inf / NaN where the reference is"""
    v, p = np.asarray(values, np.float64), np.asarray(pdf, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bonus = np.sqrt(case.beta * np.log(case.buffer_len) / (case.buffer_len * p * case.volume))
        ref = case.alpha * v + bonus
        return ref, np.abs(case.alpha * v) + bonus + np.abs(ref)


def ucb_bound(values, pdf, case):
    return C_UCB * EPS32 * ucb_scale(values, pdf, case)[1]


def ucb_emu32(values, pdf, case):
    """ucb_kernel's two roundings: the fp64 bonus to float32, then fmaf(alpha, value, bonus)"""
    p = np.asarray(pdf, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bonus = np.sqrt(float(np.float32(case.beta)) * np.log(float(case.buffer_len)) / (case.buffer_len * p * case.volume))
        return _fma(np.float32(case.alpha), np.asarray(values, np.float32), bonus.astype(np.float32))


def ucb_placements(case):
    """[(label, values, pdf, best)]: the case's base rows with the winner placed -- in each of the four waves, in a row
    reached only on a later stride (>= 256), as exact copies in several rows (the lowest wins), behind one and two or three
    pdf = 0 rows (+inf: the lowest wins), among NaN values and NaN densities (a NaN score never wins), and with every score NaN
    (index 0).  ``best`` is what the kernel must return: the boosted winner leads the reference by 1, far beyond the
    bound; None where the rows are as drawn and only the kernel's own scores decide ("base", "nan")."""
    m = case.m
    v0, p0 = ucb_base(case)
    ref0, _ = ucb_scale(v0, p0, case)

    def boosted(rows):
        """the first of ``rows`` lifted 1 above every other score, the others made copies of it"""
        v, p = v0.copy(), p0.copy()
        i = rows[0]
        bonus_i = ref0[i] - case.alpha * float(v0[i])
        v[i] = np.float32((ref0.max() + 1.0 - bonus_i) / case.alpha)
        for k in rows[1:]:
            v[k], p[k] = v[i], p[i]
        return v, p

    out = [("base", v0, p0, None)]
    for w in range(4):
        if 64 * w + 5 < m or (w == 0 and m >= 1):
            i = min(64 * w + 5, m - 1)
            out.append(("wave%d" % w, *boosted([i]), i))
    if m > 256:
        for i in sorted({m - 1, min(256 + 70, m - 1)}):
            out.append(("late%d" % i, *boosted([i]), i))
    if UCB_DUP_ROWS[m]:
        star, copies = UCB_DUP_ROWS[m]
        out.append(("dup", *boosted([star, *copies]), min(star, *copies)))
    star = min(2, m - 1)                              # a finite leader at a low row: +inf must still beat it
    v, p = boosted([star])
    p1 = p.copy()
    p1[m - 1] = 0.0
    out.append(("inf1", v, p1, m - 1))
    if m > 1:                                         # two +inf in neighbouring lanes, and the one of inf1 in the last row
        zeros = sorted({(2 * m) // 3, min((2 * m) // 3 + 1, m - 1), m - 1})
        p2 = p.copy()
        p2[zeros] = 0.0
        out.append(("inf2", v, p2, zeros[0]))
    if m > 1:
        v, p = v0.copy(), p0.copy()
        v[[0, int(np.argmax(ref0))]] = np.nan          # the reference's winner and row 0 drop out
        p[m // 2] = np.nan
        out.append(("nan", v, p, None))
    out.append(("allnan", np.full(m, np.nan, np.float32), p0, 0))
    return out


# ----------------------------------------------------------------------------------------------------------- chain --
V_TOL = 2e-5            # tests/test_gpu_agents.py::test_critic_kde_ucb_kernels holds Q(s, pi(s)) to V_TOL * max(1, |V|max)


def chain_bound(values, pdf, pdf_bound, case):
    """Accepted |device score - reference score| of every candidate when the device ranks them with ITS values and ITS
    densities (critic -> kde_kernel -> ucb_kernel), the reference with fp64 ones.  With B(p) = bonus = K p^-1/2:

        |X - ref| <= |ucb_kernel(V', p') - U(V', p')| + alpha |V' - V| + |B(p') - B(p)|
                  <= C_UCB 2^-24 (A + 2 dU) + dU,     dU = alpha tol_V + B(p) ((1 - eps)^-1/2 - 1),

    tol_V = V_TOL max(1, |V|max) the critic's tolerance, eps = pdf_bound / pdf < 1 the KDE bound relative to the density
    (B is convex and decreasing: the worst case is p' = p (1 - eps), and dB/dp = -B / 2p to first order), and A + 2 dU
    bounds the UCB scale at the device's inputs by the scale at the reference's."""
    v, p = np.asarray(values, np.float64), np.asarray(pdf, np.float64)
    eps = np.asarray(pdf_bound, np.float64) / p
    assert (eps < 0.5).all(), "a candidate's density is not resolved by float32"
    ref, A = ucb_scale(v, p, case)
    bonus = ref - case.alpha * v
    dU = case.alpha * V_TOL * max(1.0, float(np.abs(v).max())) + bonus * ((1.0 - eps) ** -0.5 - 1.0)
    return C_UCB * EPS32 * (A + 2.0 * dU) + dU
