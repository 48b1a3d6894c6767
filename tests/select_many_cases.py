"""The grouped smart-start selection (ssc_*_many over ssc_select_many_item; csrc/replay.hip, csrc/smartstart.hip): the case
table of the GPU tests, a numpy fp64 restatement of the d x d algebra scott_bandwidth_many_kernel runs on the device, the
top-k rule of ucb_topk_many_kernel, and the validity predicate a chosen list is held to.  numpy only; shared by
tests/test_select_many_cases_cpu.py and tests/test_gpu_select_many.py.

Algebra.  The device has no LAPACK: it factors cov = L L^T by the textbook Cholesky loops, inverts L by forward
substitution, forms inv(cov) = L^-T L^-1, factors that again and transposes -- ``scott_algebra`` below, loop for loop.
kde_scott_bandwidth does the same with numpy.linalg (LU inverse, LAPACK Cholesky, LU determinant).  Both are backward
stable fp64 computations of the same quantities; the CPU test holds the restatement to numpy.linalg on the Scott covariances
of select_cases.KDE_CASES at the tolerances tests/test_gpu_select_matrix.py::test_kde_scott_bandwidth holds the host
function to (whitening: one float32 ulp; norm: 1e-12 relative, or 4 x the CPU order spread where that is larger).

Top-k rule.  Descending ucb; NaN below -inf; -0 = +0; lowest slot first on ties; masked slots (idx < 0) never; places past
the live slots -1.

Validity.  With ref the fp64 score and bound the per-slot bound (select_cases.chain_bound), a device ranking X with
|X - ref| <= bound that puts c ahead of j has X[c] >= X[j], hence ref[c] + bound[c] >= ref[j] - bound[j].  ``topk_valid``
asks that of every chosen c against every live slot that was not chosen, and of consecutive chosen entries."""
from collections import namedtuple

import numpy as np


class NoFactor(Exception):
    """a Cholesky pivot that is non-positive or not finite (the device's status 1)"""


def cholesky_lower(a):
    d = a.shape[0]
    l = np.zeros((d, d), np.float64)
    for i in range(d):
        for j in range(i + 1):
            v = a[i, j]
            for k in range(j):
                v -= l[i, k] * l[j, k]
            if i == j:
                if not v > 0.0 or np.isinf(v):
                    raise NoFactor((i, float(v)))
                l[i, i] = np.sqrt(v)
            else:
                l[i, j] = v / l[j, j]
    return l


def scott_algebra(cov, n):
    """(wh [d, d] float32, norm) of the Scott covariance ``cov`` (already scaled) of ``n`` points, as the device computes them"""
    cov = np.asarray(cov, np.float64)
    d = cov.shape[0]
    lo = cholesky_lower(cov)
    li = np.zeros((d, d), np.float64)
    det = 1.0
    for i in range(d):
        li[i, i] = 1.0 / lo[i, i]
        det *= 2.0 * np.pi * lo[i, i] * lo[i, i]
        for j in range(i):
            v = 0.0
            for k in range(j, i):
                v -= lo[i, k] * li[k, j]
            li[i, j] = v / lo[i, i]
    pinv = np.zeros((d, d), np.float64)
    for i in range(d):
        for j in range(i + 1):
            v = 0.0
            for k in range(i, d):
                v += li[k, i] * li[k, j]
            pinv[i, j] = pinv[j, i] = v
    m = cholesky_lower(pinv)
    return np.ascontiguousarray(m.T, np.float32), 1.0 / (n * np.sqrt(det))


def block_sum(partials):
    """scott_bandwidth_many_kernel's merge of 1024 per-thread partials [1024, ...]: the xor-shuffle tree inside each wave of
    64 lanes (masks 32 .. 1), then the 16 waves in order"""
    v = np.asarray(partials, np.float64).reshape((16, 64) + np.shape(partials)[1:])
    lane = np.arange(64)
    for msk in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ msk]
    total = np.zeros(v.shape[2:], np.float64)
    for w in range(16):
        total = total + v[w, 0]
    return total


def thread_partials(rows):
    """what thread t of 1024 accumulates over rows t, t + 1024, ... in order -> [1024, ...]"""
    rows = np.asarray(rows, np.float64)
    acc = np.zeros((1024,) + rows.shape[1:], np.float64)
    for j0 in range(0, len(rows), 1024):
        part = rows[j0:j0 + 1024]
        acc[:len(part)] = acc[:len(part)] + part
    return acc


def scott_covariance(data):
    """two-pass covariance (ddof = 1) times the Scott factor in the device's summation order (products rounded once more
    than the kernel's fused multiply-adds)"""
    x = np.asarray(data, np.float64)
    n, d = x.shape
    mean = block_sum(thread_partials(x)) / n
    xc = x - mean
    return block_sum(thread_partials(xc[:, :, None] * xc[:, None, :])) / (n - 1) * (n ** (-1.0 / (d + 4))) ** 2


def topk_rule(ucb, idx, n_plans):
    """d_chosen of ucb_topk_many_kernel for float32 scores ``ucb`` and buffer indices ``idx`` (-1: masked)"""
    ucb, idx = np.asarray(ucb, np.float32), np.asarray(idx)
    live = [i for i in range(len(idx)) if idx[i] >= 0]

    def key(i):
        u = ucb[i]
        return (0, 0.0, i) if np.isnan(u) else (-1, -float(u), i)        # numbers first (descending), NaN last; slot breaks ties
    order = sorted(live, key=key)[:n_plans]
    return np.array([idx[i] for i in order] + [-1] * (n_plans - len(order)), np.int32)


def topk_valid(chosen_slots, ref, bound, live):
    """the validity predicate (module docstring); ``chosen_slots`` in rank order, ``live`` a boolean mask"""
    chosen_slots = list(chosen_slots)
    if len(set(chosen_slots)) != len(chosen_slots) or not all(live[c] for c in chosen_slots):
        return False
    rest = [j for j in np.nonzero(live)[0] if j not in set(chosen_slots)]
    for c in chosen_slots:
        for j in rest:
            if not ref[c] + bound[c] >= ref[j] - bound[j]:
                return False
    for a, b in zip(chosen_slots, chosen_slots[1:]):
        if not ref[a] + bound[a] >= ref[b] - bound[b]:
            return False
    return True


# ---- the GPU stage table -------------------------------------------------------------------------------------------
# ring: "fresh" (not wrapped), "wrapped" (count > capacity: a logical range crosses the seam), "empty", "gone" (every
#       episode start has left the ring: all slots -1), "few" (three valid records), "flat" (an all-equal data set: status 1)
# n_ss: 1, 5, 1025 (a thread's second slot); 63, 64, 65 (critic rows around a block); 8, 9 (KDE queries around a group);
#       255, 256, 257 (ucb slots around the workgroup)
# size / stride give n_data = ceil((size + 1) / stride): 2, d + 2, 4097 at strides 1 and 3 with (size + 1) % 3 != 0
# net: "small" (64-32), "wide" (200-100 with LayerNorm, with observation statistics)
Item = namedtuple("Item", "name ring n_envs size cap stride n_ss n_plans max_len net")

ITEMS_2D = [
    Item("fresh_n5", "fresh", 4, 40, 64, 1, 5, 3, 1001, "small"),
    Item("two_states", "fresh", 1, 1, 8, 1, 1, 1, 1001, "small"),                # n_data = 2
    Item("d_plus_2", "fresh", 1, 3, 8, 1, 8, 1, 1001, "wide"),                   # n_data = d + 2 = 4
    Item("wrapped_1025", "wrapped", 16, 4096, 4096, 1, 1025, 3, 6, "wide"),      # n_data = 4097; paths cut by max_len
    Item("empty", "empty", 4, 0, 64, 1, 5, 3, 1001, "small"),
    Item("wrapped_s3", "wrapped", 16, 4096, 4096, 3, 9, 1, 1001, "small"),       # 4097 % 3 = 2: n_data = 1366
    Item("gone", "gone", 2, 32, 32, 1, 5, 3, 1001, "small"),
    Item("few", "few", 1, 30, 30, 1, 5, 4, 1001, "small"),                       # n_plans = live slots + 1
    Item("flat", "flat", 4, 40, 64, 1, 5, 3, 1001, "small"),
    Item("rows63", "fresh", 8, 400, 512, 3, 63, 3, 1001, "wide"),                # 401 % 3 = 2
    Item("rows64", "fresh", 8, 400, 512, 1, 64, 1, 1001, "small"),
    Item("rows65", "wrapped", 8, 512, 512, 1, 65, 3, 1001, "wide"),
    Item("slots255", "wrapped", 8, 512, 512, 1, 255, 3, 1001, "small"),
    Item("slots256", "fresh", 8, 400, 512, 1, 256, 1, 1001, "small"),
    Item("slots257", "fresh", 8, 400, 512, 1, 257, 3, 1001, "wide"),
]
# other state dimensions: candidates, bandwidth and KDE (kde_kernel<1>, <3>, and <0> for d = 4)
ITEMS_ND = {
    1: [Item("d1_fresh", "fresh", 2, 40, 64, 1, 9, 1, 1001, None), Item("d1_wrapped_s3", "wrapped", 16, 4096, 4096, 3, 8, 1, 1001, None),
        Item("d1_three", "fresh", 1, 2, 8, 1, 1, 1, 1001, None)],
    3: [Item("d3_fresh", "fresh", 2, 40, 64, 1, 9, 1, 1001, None), Item("d3_wrapped", "wrapped", 16, 4096, 4096, 1, 8, 1, 1001, None),
        Item("d3_five", "fresh", 1, 4, 8, 1, 1, 1, 1001, None)],
    4: [Item("d4_fresh", "fresh", 2, 40, 64, 1, 9, 1, 1001, None), Item("d4_wrapped_s3", "wrapped", 16, 4096, 4096, 3, 8, 1, 1001, None),
        Item("d4_six", "fresh", 1, 5, 8, 1, 1, 1, 1001, None)],
}


def ring_arrays(item, d, seed):
    """host arrays of a ring for ``item``: dict(s, s2 [cap, d] float32, ep_steps [cap] int32, count).  Record j (env j % n,
    step j // n) lives at row j % cap; episodes end at random except where the ring kind says otherwise."""
    rng = np.random.default_rng(seed)
    n, cap, size = item.n_envs, item.cap, item.size
    s, s2 = np.zeros((cap, d), np.float32), np.zeros((cap, d), np.float32)
    eps = np.zeros(cap, np.int32)
    if item.ring == "empty":
        return dict(s=s, s2=s2, ep_steps=eps, count=0)
    count = size + (3 * n if item.ring in ("wrapped", "gone", "few") else 0)
    if item.ring in ("wrapped", "gone", "few"):
        assert size == cap
    K = -(-count // n)
    if item.ring == "gone":
        done = np.zeros((K, n), bool)                       # one episode per env, begun before the ring's oldest record
    elif item.ring == "few":
        done = np.zeros((K, n), bool)
        done[K - 4, :] = True                               # the last three steps open the one episode that starts inside
    else:
        done = rng.random((K, n)) < 0.08
    run = np.zeros(n, np.int64)
    mix = rng.normal(size=(d, d)) + 2.0 * np.eye(d)
    for j in range(count):
        k, e = divmod(j, n)
        run[e] += 1
        x = (rng.normal(size=d) @ mix + 0.5).astype(np.float32) if item.ring != "flat" else np.full(d, 0.25, np.float32)
        y = (x + rng.normal(size=d).astype(np.float32) * 0.1).astype(np.float32) if item.ring != "flat" else x
        s[j % cap], s2[j % cap], eps[j % cap] = x, y, run[e]
        if done[k, e]:
            run[e] = 0
    return dict(s=s, s2=s2, ep_steps=eps, count=count)


def all_states(arr, cap):
    """get_all_states() of the ring on the host"""
    count = arr["count"]
    size = min(count, cap)
    order = (np.arange(size) + count - size) % cap
    return np.concatenate([arr["s"][order], arr["s2"][(count - 1) % cap][None]])
