"""The data path between the arithmetic kernels (csrc/replay.hip, csrc/dataset.hip, pack_tail_kernel of csrc/env_step.hip): the
case tables, the builders of synthetic chunks and rings, and the expected results from the restatements of
oracle/ssc_oracle.py.  Shared by the CPU test (tests/test_data_cases_cpu.py), which holds the tables to the edges they claim, and the
GPU test (tests/test_gpu_data_matrix.py); numpy only.

Synthetic content.  ``synthetic_chunk`` gives every (column, step, env) of a chunk its own integer below 2^24 (exact in fp32, and
exact after the reward scale 0.25); ``continuous_chunk`` does the same with a seeded permutation, obs2[k] = obs[k + 1] as inside an
episode, so that the data set's delta rows are as recognisable as its state rows.  Every byte a kernel may write is pre-filled with
FILL and lies between GUARD bytes of PAT; the expected arrays start from the same fill, so a row the restatement never writes must
keep it.

Extended for these tables: O.replay_sample_indices draws for the unresolved slots only (the dense draw of 1025 indices takes about
2000 rounds; the indices are unchanged)."""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np

from oracle import ssc_oracle as O

# ---- the kernels' constants, restated (csrc/replay.hip, csrc/dataset.hip, csrc/ssc_host.h) --------------------------------------
K_BLOCK = 256                       # kBlock: threads of the elementwise / append / path kernels
ENVS_PER_GROUP = 64                 # kGroup: envs per block of dataset_len / offsets / build
SCAN_THREADS = 1024                 # kScanThreads of dataset_group_scan_kernel
TILE_K = 64                         # kTileK: steps per tile of dataset_build_kernel
QUARTERS, LEN_UNROLL = 4, 8         # dataset_len_kernel: four waves, eight steps per trip
APPEND_UNROLL = 4                   # kU of the indexed append
STAT_BLOCKS, STAT_THREADS, STAT_ELEMS = 2048, 256, 16       # kStatBlocks; one block per 256 * 16 elements below the cap
PATH_GRID = 64                      # block cap of episode_path_kernel
ONE_WAVE = 64                       # largest batch of the one-wave sampler
ELEMS_PER_THREAD = 4                # kPerThread of the z-score kernels
NOISE_GROUP = 4                     # columns per Philox evaluation of add_noise_kernel
MAX_OBS = 3                         # SSC_MAX_OBS: obs_dim 2 and 3 are instantiated, 1 takes the guarded branch
SIZE_MAX = 2 ** 31 - 1              # the largest ring size the samplers admit

GUARD, PAT, FILL = 256, 0xA5, 0x5C
F32_MAX = float(np.finfo(np.float32).max)
U64 = 2.0 ** -53


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def filled(shape, dtype):
    """an array whose every byte is FILL"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(n, FILL, np.uint8).view(dtype).reshape(shape)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# ---- synthetic chunks ------------------------------------------------------------------------------------------------------------
def synthetic_chunk(K, n, d, step0=0):
    """obs / obs2 [d, K, n], act / rew [K, n] fp32: value ((column * KB + step) * EB + env) with EB >= n, KB * EB = 2^21, eight
    columns (obs 0..2, obs2 3..5, act 6, rew 7) -- below 2^24.  The step is the GLOBAL one (step0 + k), so chunks of one run differ;
    obs2 carries the step reversed and the env permuted, so it is no shifted copy of obs."""
    EB = 1 << int(max(n, 1) - 1).bit_length()
    KB = (1 << 21) // EB
    assert step0 + K <= KB and d <= MAX_OBS
    k = (step0 + np.arange(K, dtype=np.int64))[:, None]
    e = np.arange(n, dtype=np.int64)[None, :]
    cell = lambda col, kk, ee: ((col * KB + kk) * EB + ee).astype(np.float32)
    zero = np.zeros((K, n), np.int64)
    obs = np.stack([cell(c, k, e) for c in range(d)]) if d else np.zeros((0, K, n), np.float32)
    obs2 = np.stack([cell(3 + c, KB - 1 - k + zero, (5 * e + 3) % EB + zero) for c in range(d)])
    return dict(obs=obs, obs2=obs2, act=cell(6, k, e), rew=cell(7, k, e))


def continuous_chunk(K, n, d, seed):
    """A chunk of distinct integers below 2^24 in seeded random order with obs2[k] = obs[k + 1] (the last step's obs2 and the actions
    are further distinct integers): the rows (s, a, s' - s) of the data set then differ in every column, step and env."""
    rng = np.random.default_rng(seed)
    cells = d * K * n
    assert (2 * d + 1) * K * n < 2 ** 24
    obs = rng.permutation(cells).astype(np.float32).reshape(d, K, n)
    obs2 = np.empty_like(obs)
    obs2[:, :-1] = obs[:, 1:]
    obs2[:, -1] = (cells + rng.permutation(d * n)).astype(np.float32).reshape(d, n)
    act = (2 * cells + rng.permutation(K * n)).astype(np.float32).reshape(K, n)
    return dict(obs=obs, obs2=obs2, act=act, rew=np.zeros((K, n), np.float32))


# ---- 1. replay append --------------------------------------------------------------------------------------------------------------
# one append_chunk call: n envs, K steps from global step step0, the chunk layout, last_steps, the reward scale, the share of
# terminal steps (seeded) and terminal steps placed by hand ((step, env), ...)
Append = namedtuple("Append", "n K step0 packed last_steps reward_scale p_done done_at")
AppendCase = namedtuple("AppendCase", "name capacity appends")


def _a(n, K, step0, packed=True, last_steps=None, reward_scale=1.0, p_done=0.3, done_at=()):
    return Append(n, K, step0, packed, last_steps, reward_scale, p_done, done_at)


APPEND_CASES = [
    # three chunks of 37 x 5 into 400 rows: the third wraps; 400 is no multiple of 37; packed, dense, packed
    AppendCase("wrap3", 400, (_a(37, 5, 0), _a(37, 5, 5, packed=False), _a(37, 5, 10, reward_scale=0.25))),
    AppendCase("chunk_over_ring", 500, (_a(64, 9, 0, reward_scale=0.25),)),          # 576 records: first = 76
    AppendCase("smallest", 1, (_a(1, 1, 0),)),
    AppendCase("k5_two_blocks", 2000, (_a(300, 5, 0, packed=False),)),               # 300 envs: a second block of the indexed kernel
    AppendCase("k6", 64, (_a(5, 6, 0),)),
    AppendCase("k7", 64, (_a(5, 7, 0, packed=False, reward_scale=0.25),)),
    AppendCase("k8", 64, (_a(5, 8, 0),)),
    # last_steps = 3 of 8: the append starts at step 9, not at 4, so ep_run restarts; then a chunk that continues
    AppendCase("last_steps", 64, (_a(5, 4, 0, p_done=0.1), _a(5, 8, 4, last_steps=3), _a(5, 2, 12))),
    # steps 3 and 4 are missing between the first two appends: ep_run restarts; the third continues the second
    AppendCase("step0_gap", 100, (_a(7, 3, 0, p_done=0.15), _a(7, 3, 5, packed=False), _a(7, 3, 8, reward_scale=0.25))),
]
APPEND_BY_NAME = {c.name: c for c in APPEND_CASES}

# ssc_replay_append_shard: a whole chunk first (so the shards start at record 300 with running episodes), then 5 steps of 150 envs
# that wrap the ring of 1000, delivered as three unequal shards in shuffled order
SHARD_CASE = AppendCase("shards", 1000, (_a(150, 2, 0, p_done=0.1), _a(150, 5, 2, reward_scale=0.25)))
SHARDS = ((64, 37), (49, 101), (37, 0))             # (envs, env_off) in the order they are appended


def append_companions(case):
    """the two further pairs of the ssc_replay_append_many launch a case rides in: unequal n, K and capacity, one with K = 0"""
    m = len(case.appends)
    ls = [a.last_steps for a in case.appends]
    return (AppendCase(case.name + "+small", 16, tuple(_a(3, 2, 2 * i, packed=i % 2 == 0, last_steps=ls[i], reward_scale=0.25)
                                                       for i in range(m))),
            AppendCase(case.name + "+empty", 9, tuple(_a(11, 0, 0, last_steps=ls[i]) for i in range(m))))


def append_done(case, i):
    a = case.appends[i]
    done = (np.random.default_rng(_seed(case.name, i)).random((a.K, a.n)) < a.p_done).astype(np.uint8)
    if a.n > 1:
        done[:, 0] = 0                      # env 0 never ends an episode by chance: its step count runs through every chunk
    for k, e in a.done_at:
        done[k, e] = 1
    return done


def append_chunk_of(case, i, od):
    a = case.appends[i]
    return synthetic_chunk(a.K, a.n, od, a.step0)


def blank_ring(capacity, od, n_envs):
    return dict(s=filled((capacity, od), np.float32), a=filled((capacity, 1), np.float32), r=filled((capacity,), np.float32),
                t=filled((capacity,), np.uint8), s2=filled((capacity, od), np.float32),
                ep_steps=filled((capacity,), np.int32), ep_run=np.zeros(n_envs, np.int32))


@functools.lru_cache(maxsize=None)
def append_expected(name_or_case, od):
    """(ring arrays after the case's appends, count).  The five columns: O.replay_append; ep_steps / ep_run:
    O.replay_episode_steps, with DeviceReplayBuffer.append_chunk's rule that a chunk which does not continue the last one restarts
    every env's step count.  A plain ring is the same without the last two arrays."""
    case = APPEND_BY_NAME[name_or_case] if isinstance(name_or_case, str) else name_or_case
    n = case.appends[0].n
    ring, count, next_step0 = blank_ring(case.capacity, od, n), 0, None
    for i, a in enumerate(case.appends):
        ch, done = append_chunk_of(case, i, od), append_done(case, i)
        L = a.K if a.last_steps is None else min(a.last_steps, a.K)
        sl = slice(a.K - L, a.K)
        if next_step0 is not None and a.step0 + a.K - L != next_step0:
            ring["ep_run"][:] = 0
        next_step0 = a.step0 + a.K
        steps, run = O.replay_episode_steps(done[sl], ring["ep_run"])
        total = L * a.n
        first = max(0, total - case.capacity)
        pos = (count + np.arange(total)) % case.capacity
        ring["ep_steps"][pos[first:]] = steps.reshape(-1)[first:]
        ring["ep_run"][:] = run
        cols = lambda x: x[:, sl].reshape(od, -1).T
        count = O.replay_append(ring, count, cols(ch["obs"]), ch["act"][sl].reshape(-1, 1), ch["rew"][sl].reshape(-1),
                                done[sl].reshape(-1), cols(ch["obs2"]), a.reward_scale)
    for v in ring.values():
        v.setflags(write=False)
    return ring, count


# ---- 2. samplers -------------------------------------------------------------------------------------------------------------------
SampleCase = namedtuple("SampleCase", "name seed counter0 size n_batches batch")
SAMPLE_CASES = ([SampleCase("dense%d" % b, 40 + b, 3, b, 1 if b > 64 else 2, b) for b in (1, 2, 63, 64, 65, 1025)]
                + [SampleCase("largest_size_b64", 7, 0, SIZE_MAX, 2, 64), SampleCase("largest_size_b65", 8, 0, SIZE_MAX, 2, 65),
                   SampleCase("counter_high_word_wave", 9, 2 ** 32 - 2, 100, 4, 16),
                   SampleCase("counter_high_word_big", 10, 2 ** 32 - 2, 200, 4, 70),
                   SampleCase("no_batches", 11, 0, 10, 0, 4)])
SAMPLE_MANY = dict(batch=8, n_batches=3, keys=((11, 0, 8), (12, 2 ** 32 - 1, 100), (13, 5, SIZE_MAX)))     # (seed, counter0, size)


@functools.lru_cache(maxsize=None)
def sample_expected(seed, counter0, size, n_batches, batch):
    out = O.replay_sample_indices(seed, counter0, size, n_batches, batch)
    out.setflags(write=False)
    return out


# ---- 3. smart-start queries --------------------------------------------------------------------------------------------------------
# rings of 5 envs and 203 rows (no multiple of 5) built by the append model above
SmartCase = namedtuple("SmartCase", "name ring n_ss seed counter")
_twenty = lambda p: tuple(_a(5, 20, 20 * i, p_done=p) for i in range(3))
SMART_RINGS = [AppendCase("not_wrapped", 203, _twenty(0.1)[:1]), AppendCase("wrapped", 203, _twenty(0.1)),
               AppendCase("no_start_left", 203, _twenty(0.0))]        # no terminal step: every episode began at step 0, evicted
SMART_CASES = [SmartCase("not_wrapped", SMART_RINGS[0], 128, 77, 3), SmartCase("wrapped", SMART_RINGS[1], 256, 78, 2 ** 32 + 1),
               SmartCase("no_start_left", SMART_RINGS[2], 64, 79, 0)]
# one env: an episode of 500 steps, then one of 7000 still running, in 8192 rows; the path to the newest record is cut at 6000 steps
LONG_PATH = AppendCase("long_path", 8192, (_a(1, 500, 0, p_done=0.0, done_at=((499, 0),)), _a(1, 7000, 500, p_done=0.0)))
LONG_PATH_MAX_LEN = 6000
for _c in SMART_RINGS + [LONG_PATH, SHARD_CASE]:
    APPEND_BY_NAME[_c.name] = _c


def smart_valid(case, od=1):
    ring, count = append_expected(case.name, od)
    return O.smart_start_valid(ring["ep_steps"], case.capacity, count, case.appends[0].n)


def smart_expected(sc):
    """(idx [n_ss] with -1 = unfilled, n_out)"""
    idx = O.smart_start_indices(smart_valid(sc.ring), sc.n_ss, sc.seed, sc.counter)
    return idx.astype(np.int32), int((idx >= 0).sum())


def path_queries(case):
    """buffer indices to ask the path of: the oldest and newest record, the first and last valid one, one whose start is evicted
    (when there is one), and the two just outside the ring"""
    valid = smart_valid(case)
    size = len(valid)
    q = {0, size - 1, -1, size}
    if valid.any():
        q |= {int(np.flatnonzero(valid)[0]), int(np.flatnonzero(valid)[-1])}
    if not valid.all():
        q.add(int(np.flatnonzero(~valid)[-1]))
    return sorted(q)


def path_expected(case, od, buffer_index, max_len):
    """[rows, od] fp32 (rows = 0: no path -- len 0 and nothing written)"""
    ring, count = append_expected(case.name, od)
    size = min(count, case.capacity)
    if not 0 <= buffer_index < size:
        return np.zeros((0, od), np.float32)
    return np.asarray(O.replay_episode_path(ring["s"], ring["s2"], ring["ep_steps"], case.capacity, count, case.appends[0].n,
                                            buffer_index, max_len), np.float32).reshape(-1, od)


# ---- 4. data-set scan and build ----------------------------------------------------------------------------------------------------
DatasetCase = namedtuple("DatasetCase", "name K n d packed kind")
DIRECTED_K = (1, 2, 3, 4, 7, 8, 9, 10, 33, 130)
DATASET_CASES = ([DatasetCase("d1_k65_n70", 65, 70, 1, True, "random"), DatasetCase("d1_k130_n3", 130, 3, 1, False, "random"),
                  DatasetCase("groups_n65537", 3, 65537, 2, True, "ragged"), DatasetCase("groups_n70001", 3, 70001, 2, False, "ragged")]
                 + [DatasetCase("directed_k%d" % K, K, 70, 1 + i % 3, i % 2 == 0, "directed") for i, K in enumerate(DIRECTED_K)])
DATASET_BY_NAME = {c.name: c for c in DATASET_CASES}
CUT_CASES = [DatasetCase("cut_packed", 130, 70, 3, True, "long"), DatasetCase("cut_dense", 130, 70, 3, False, "long")]
DATASET_BY_NAME.update({c.name: c for c in CUT_CASES})


def directed_spots(K):
    """the steps at which one env has its only terminal step: both sides of every quarter edge and of every 8-step edge inside a
    quarter of dataset_len_kernel, and the chunk's first and last step"""
    per = (K + QUARTERS - 1) // QUARTERS
    spots = {0, K - 1}
    for q in range(QUARTERS):
        kb, ke = q * per, min(q * per + per, K)
        if q:
            spots |= {kb - 1, kb}
        for k0 in range(kb + LEN_UNROLL, ke, LEN_UNROLL):
            spots |= {k0 - 1, k0}
    return sorted(s for s in spots if 0 <= s < K)


def directed_multi(K):
    """terminal steps of the envs that have them in two and in three quarters: the last step of the earlier quarter(s) and the first
    of the latest -- the earliest must win whichever wave gets there first"""
    per = (K + QUARTERS - 1) // QUARTERS
    qs = [q for q in range(QUARTERS) if q * per < K]
    last = lambda q: min(q * per + per, K) - 1
    out = [(last(a), b * per) for a in qs for b in qs if a < b]
    out += [(last(a), last(b), c * per) for a in qs for b in qs for c in qs if a < b < c]
    return out


def dataset_done(case):
    K, n = case.K, case.n
    rng = np.random.default_rng(_seed(case.name))
    if case.kind == "ragged":               # lengths 1..3 of K = 3; a full-length rollout ends on its last step or not at all
        L = rng.integers(1, K + 1, n)
        done = np.zeros((K, n), np.uint8)
        ends = (L < K) | (rng.random(n) < 0.5)
        done[L[ends] - 1, np.flatnonzero(ends)] = 1
        return done
    if case.kind == "long":
        done = (rng.random((K, n)) < 0.004).astype(np.uint8)
        done[0, 1] = 1
        return done
    done = (rng.random((K, n)) < (0.1 if case.kind == "directed" else 0.02)).astype(np.uint8)
    if case.kind == "random":
        if n > 3:
            done[0, 1] = 1
        done[:, 2 % n] = 0
        return done
    # directed: entry 0 of the list has no terminal step, then one env per spot, then the multi-quarter envs; list entry i is env
    # (69 - 9 * i) % 70, which spreads them over the full group and the group of 6 live lanes
    assert n == 70
    plan = [()] + [(s,) for s in directed_spots(K)] + directed_multi(K)
    assert len(plan) <= n
    for i, steps in enumerate(plan):
        e = (n - 1 - 9 * i) % n
        done[:, e] = 0
        done[list(steps), e] = 1
    return done


def directed_envs(case):
    """{env: its planted terminal steps} of a directed case"""
    plan = [()] + [(s,) for s in directed_spots(case.K)] + directed_multi(case.K)
    return {(case.n - 1 - 9 * i) % case.n: steps for i, steps in enumerate(plan)}


def dataset_chunk(case):
    return continuous_chunk(case.K, case.n, case.d, _seed(case.name, "chunk"))


@functools.lru_cache(maxsize=None)
def dataset_expected(name):
    """dict(len [n] i32, off [n + 1] i64, X, Y, Z) from O.rollouts_from_chunk and the two generate_training_data_* restatements"""
    case = DATASET_BY_NAME[name]
    ch, done = dataset_chunk(case), dataset_done(case)
    states, controls = O.rollouts_from_chunk(ch["obs"].transpose(1, 2, 0), ch["act"][:, :, None], done)
    lens = np.array([len(s) for s in states], np.int32)
    off = np.concatenate([[0], np.cumsum(np.maximum(lens.astype(np.int64) - 1, 0))]).astype(np.int64)
    X, Y = O.generate_training_data_inputs(states, controls)
    Z = O.generate_training_data_outputs(states)
    out = dict(len=lens, off=off, X=X.astype(np.float32), Y=Y.astype(np.float32), Z=Z.astype(np.float32))
    assert out["X"].shape == (off[-1], case.d) and Z.dtype == np.float32
    for v in out.values():
        v.setflags(write=False)
    return out


def capacity_cuts(name):
    """the capacity_rows values of a cut case: everything, one row short, inside a 64-step tile of a rollout (its second tile), 1, 0"""
    ex = dataset_expected(name)
    rows = np.maximum(ex["len"].astype(np.int64) - 1, 0)
    i = int(np.flatnonzero(rows > TILE_K + 17)[-1])
    total = int(ex["off"][-1])
    return [total, total - 1, int(ex["off"][i]) + TILE_K + 17, 1, 0]


# ---- 5. column statistics, z-score, noise ----------------------------------------------------------------------------------------
StatsCase = namedtuple("StatsCase", "name rows cols")
STATS_CASES = [StatsCase("s_r%d_c%d" % (r, c), r, c) for c in (1, 2, 3, 7, 33, 64) for r in (1, 5, 257)]
STATS_CAPPED = StatsCase("s_capped", 1200001, 7)
# (mean, spread) of a column; column c of a case takes recipe (c + rows) % 5: a plain one, one whose one-pass variance fails (mean
# 1e4, spread 1e-2), a constant one, a small and a large one
STATS_RECIPES = ((0.5, 1.0), (1e4, 1e-2), (7.0, 0.0), (-2.0, 1e-3), (3.0, 50.0))


def stats_recipe(case, c):
    return STATS_RECIPES[(c + case.rows) % len(STATS_RECIPES)]


@functools.lru_cache(maxsize=None)
def stats_data(case):
    rng = np.random.default_rng(_seed(case.name))
    x = np.empty((case.rows, case.cols), np.float32)
    for c in range(case.cols):
        m, s = stats_recipe(case, c)
        x[:, c] = (m + s * rng.normal(size=case.rows)).astype(np.float32)
    x.setflags(write=False)
    return x


def stats_chain(rows, cols):
    """the launch of ssc_column_stats and m, the longest chain of fp64 additions an element passes through"""
    total = rows * cols
    A = (STAT_THREADS // cols) * cols                              # active threads of a block
    blocks = min(max(-(-total // (STAT_THREADS * STAT_ELEMS)), 1), STAT_BLOCKS)
    S = blocks * A
    T = -(-total // S)                                             # elements of the busiest thread
    trips = T // 4 + T % 4                                         # additions into a0: the four-way trips, then the tail
    return dict(A=A, cnt=A // cols, blocks=blocks, S=S, T=T, capped=total > STAT_BLOCKS * STAT_THREADS * STAT_ELEMS,
                m=trips + 2 + 8 + -(-blocks // 64) + 6)


def gamma(k):
    return k * U64 / (1 - k * U64)


def stats_reference_of(x):
    """mean, std, the bound on each and mean |x| per column of an fp32 matrix: math.fsum (correctly rounded sums).  The squared
    deviations are formed in fp64 before the exact sum: three roundings each, 3u relative on the variance, carried in the bound
    (derived in tests/test_gpu_data_matrix.py::test_column_stats_within_the_derived_bound)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    rows, cols = x.shape
    m = stats_chain(rows, cols)["m"]
    mean = np.array([math.fsum(x[:, c].tolist()) / rows for c in range(cols)])
    var = np.array([math.fsum(((x[:, c] - mean[c]) ** 2).tolist()) / rows for c in range(cols)])
    mabs = np.array([math.fsum(np.abs(x[:, c]).tolist()) / rows for c in range(cols)])
    std = np.sqrt(var)
    e_mean = gamma(m) * mabs
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = gamma(m + 3) + ((e_mean + U64 * np.abs(mean)) / std) ** 2 + 6 * U64
        e_std = np.where(std > 0, rel * std, 0.0)
    return dict(mean=mean, std=std, mabs=mabs, e_mean=e_mean, e_std=e_std)


@functools.lru_cache(maxsize=None)
def stats_reference(case):
    return stats_reference_of(stats_data(case))


ZSCORE_COLS, ZSCORE_ROWS, ZSCORE_COL0, ZSCORE_EXTRA = (5, 7, 64, 256), 1031, 2, 3      # out_stride = col0 + cols + extra
ZCONCAT = ((64, 3), (1, 255))


@functools.lru_cache(maxsize=None)
def zscore_data(cols, tag="z"):
    """(x fp32 [rows, cols], mean f64, std f64): column 1 is constant at its mean with std 0 (expected 0), column 2 has std 0 and
    values either side of its mean (expected -+ the largest finite fp32) -- where the matrix is that wide"""
    rng = np.random.default_rng(_seed(tag, cols))
    mean, std = rng.normal(size=cols) * 3.0, rng.uniform(0.5, 2.0, size=cols)
    x = (mean + std * rng.normal(size=(ZSCORE_ROWS, cols))).astype(np.float32)
    if cols > 1:
        mean[1], std[1] = 1.5, 0.0
        x[:, 1] = 1.5
    if cols > 2:
        mean[2], std[2] = -0.25, 0.0
        x[:, 2] = np.where(np.arange(ZSCORE_ROWS) % 2 == 0, 1.0, -1.0)
    for v in (x, mean, std):
        v.setflags(write=False)
    return x, mean, std


NOISE_COLS, NOISE_ROWS, NOISE_NTS, NOISE_SEED, NOISE_STREAM = (5, 8, 9, 64, 256), 300, 0.01, 1234, 2 ** 48 - 1


@functools.lru_cache(maxsize=None)
def noise_data(cols):
    """(x, mean): the means run positive, negative, zero, positive with the column, so half the columns must not move"""
    rng = np.random.default_rng(_seed("noise", cols))
    mean = np.array([(1, -1, 0, 1)[c % 4] * (1.0 + 0.1 * (c % 17)) for c in range(cols)])
    x = (mean + 0.5 * rng.normal(size=(NOISE_ROWS, cols))).astype(np.float32)
    x.setflags(write=False)
    mean.setflags(write=False)
    return x, mean


@functools.lru_cache(maxsize=None)
def noise_expected(cols):
    x, mean = noise_data(cols)
    ref = O.add_noise_keyed(x, mean, NOISE_NTS, NOISE_SEED, NOISE_STREAM)
    # device Box-Muller (~1e-6 relative on a gaussian below 6) and the sum rounded to fp32 on both sides
    tol = 2e-5 * np.abs(mean * NOISE_NTS)[None, :] + 1.2e-7 * np.maximum(np.abs(x), np.abs(ref))
    return ref, np.where(mean * NOISE_NTS > 0, tol, 0.0)


# ---- 6. ssc_pack_transitions -------------------------------------------------------------------------------------------------------
# offset: bytes by which d_out is moved off its 16-byte alignment
PackCase = namedtuple("PackCase", "name d n K g packed stats offset")
PACK_CASES = [PackCase("p1_vec", 1, 516, 4, 3, True, True, 0), PackCase("p1_scalar", 1, 7, 3, 3, False, False, 0),
              PackCase("p1_off4", 1, 8, 2, 1, True, True, 4), PackCase("p2_vec", 2, 8, 3, 3, False, False, 0),
              PackCase("p2_scalar", 2, 257, 5, 2, True, True, 0), PackCase("p2_off4", 2, 12, 4, 4, False, True, 4),
              PackCase("p3_vec", 3, 64, 5, 5, True, True, 0), PackCase("p3_scalar", 3, 1002, 3, 2, False, True, 0),
              PackCase("p3_off4", 3, 4, 6, 2, True, False, 4)]
PACK_STATS = np.array([-12.5, 3.0, 4096.0, 17.0])


def pack_takes_16_byte_path(c):
    """ssc_pack_transitions' choice, for chunk columns that start 16-byte aligned (dense, or packed with n % 4 == 0)"""
    return c.n % 4 == 0 and c.offset % 16 == 0


def pack_bytes(d, g, n):
    return ((g * n * (8 * d + 9) + 7) & ~7) + 32


def pack_done(c):
    k, e = np.arange(c.K)[:, None], np.arange(c.n)[None, :]
    return ((31 * k + 7 * e) % 255 + 1).astype(np.uint8)           # every byte of the done column is copied as it is


def pack_expected(c):
    """the buffer of include/ssc.h: [obs (d x g x n) f32 | act (g x n) | rew (g x n) | obs2 (d x g x n) | done (g x n) u8], then, 8-byte
    aligned, four doubles when statistics are passed; every other byte keeps FILL"""
    ch, done = synthetic_chunk(c.K, c.n, c.d), pack_done(c)
    tail = slice(c.K - c.g, c.K)
    body = np.concatenate([as_bytes(ch["obs"][:, tail]), as_bytes(ch["act"][tail]), as_bytes(ch["rew"][tail]),
                           as_bytes(ch["obs2"][:, tail]), as_bytes(done[tail])])
    out = np.full(pack_bytes(c.d, c.g, c.n), FILL, np.uint8)
    out[:len(body)] = body
    if c.stats:
        out[-32:] = as_bytes(PACK_STATS)
    return out
