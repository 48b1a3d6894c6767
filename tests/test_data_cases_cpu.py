"""The data-path case tables (tests/data_cases.py) held to the edges they claim, without the kernels: every edge of
csrc/replay.hip, csrc/dataset.hip and pack_tail_kernel that tests/test_gpu_data_matrix.py is there to reach is computed here
from the kernels' constants as data_cases restates them, so a table edited until it no longer reaches one fails on the CPU.
The restatements of oracle/ssc_oracle.py run on every case, which exercises their own edge handling."""
import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import data_cases as D


# ------------------------------------------------------------------------------------------------------------ synthetic content --
@pytest.mark.parametrize("K,n,d", [(5, 37, 3), (9, 64, 1), (7000, 1, 3), (3, 1002, 2)])
def test_synthetic_chunk_values_are_distinct_and_exact(K, n, d):
    ch = D.synthetic_chunk(K, n, d, step0=11)
    allv = np.concatenate([ch[k].reshape(-1) for k in ("obs", "obs2", "act", "rew")])
    assert allv.max() < 2 ** 24 and np.array_equal(allv, np.round(allv)) and len(np.unique(allv)) == allv.size
    assert np.array_equal((ch["rew"] * np.float32(0.25)).astype(np.float64), ch["rew"].astype(np.float64) / 4)
    assert not np.array_equal(D.synthetic_chunk(K, n, d, step0=12)["obs"], ch["obs"])


def test_continuous_chunk_rows_are_recognisable():
    ch = D.continuous_chunk(9, 70, 3, 5)
    allv = np.concatenate([ch["obs"].reshape(-1), ch["obs2"][:, -1].reshape(-1), ch["act"].reshape(-1)])
    assert len(np.unique(allv)) == allv.size and allv.max() < 2 ** 24
    assert np.array_equal(ch["obs2"][:, :-1], ch["obs"][:, 1:])
    z = (ch["obs2"] - ch["obs"])[0, :-1]
    assert len(np.unique(z)) > 0.8 * z.size                  # the deltas tell steps and envs apart too


# ------------------------------------------------------------------------------------------------------------------- 1. append --
def test_append_table_reaches_every_edge():
    by = D.APPEND_BY_NAME
    w = by["wrap3"]
    assert [(a.n, a.K) for a in w.appends] == [(37, 5)] * 3 and w.capacity == 400
    assert 2 * 185 < w.capacity < 3 * 185 and w.capacity % 37 != 0              # the third chunk wraps; capacity no multiple of n
    assert {a.packed for a in w.appends} == {True, False}
    big = by["chunk_over_ring"]
    assert (big.appends[0].n, big.appends[0].K, big.capacity) == (64, 9, 500) and 64 * 9 > 500           # first > 0
    assert (by["smallest"].capacity, by["smallest"].appends[0].n, by["smallest"].appends[0].K) == (1, 1, 1)
    ks = {a.K for c in D.APPEND_CASES for a in c.appends if a.last_steps is None}
    assert {5, 6, 7, 8} <= ks and {k % D.APPEND_UNROLL for k in ks} == {0, 1, 2, 3}
    assert any(a.n > D.K_BLOCK for c in D.APPEND_CASES for a in c.appends)          # a second block of the indexed kernel
    assert any(a.K * a.n > D.K_BLOCK for c in D.APPEND_CASES for a in c.appends)    # ... and of the plain one
    assert any(a.reward_scale == 0.25 for c in D.APPEND_CASES for a in c.appends)
    ls = by["last_steps"].appends
    assert ls[1].last_steps == 3 < ls[1].K and ls[1].step0 == ls[0].step0 + ls[0].K
    gap = by["step0_gap"].appends
    assert gap[1].step0 > gap[0].step0 + gap[0].K and gap[2].step0 == gap[1].step0 + gap[1].K
    for c in D.APPEND_CASES:                       # an indexed ring takes whole steps: one n per case
        assert len({a.n for a in c.appends}) == 1
        small, empty = D.append_companions(c)
        shapes = {(x.appends[0].n, x.appends[0].K, x.capacity) for x in (c, small, empty)}
        assert len(shapes) == 3 and len({s[0] for s in shapes}) == 3 and len({s[2] for s in shapes}) == 3
        assert all(a.K == 0 for a in empty.appends)
    sh = D.SHARD_CASE
    assert sorted(D.SHARDS, key=lambda s: s[1]) == [(37, 0), (64, 37), (49, 101)] and list(D.SHARDS) != sorted(D.SHARDS, key=lambda s: s[1])
    assert sum(s[0] for s in D.SHARDS) == 150 == sh.appends[1].n and any(off % 64 for _, off in D.SHARDS)
    start = sh.appends[0].n * sh.appends[0].K
    assert sh.appends[1].K * 150 <= sh.capacity < start + sh.appends[1].K * 150          # the shards fit and wrap


@pytest.mark.parametrize("od", [1, 2, 3])
@pytest.mark.parametrize("case", D.APPEND_CASES + [D.SHARD_CASE], ids=lambda c: c.name)
def test_append_model(case, od):
    """the expected ring: live rows hold the newest records, every other byte keeps the fill, ep_steps counts the episode"""
    ring, count = D.append_expected(case.name, od)
    size = min(count, case.capacity)
    live = np.zeros(case.capacity, bool)
    live[np.arange(count - size, count) % case.capacity] = True
    for k in ("s", "a", "r", "t", "s2", "ep_steps"):
        rows = D.as_bytes(ring[k]).reshape(case.capacity, -1)
        assert np.all(rows[~live] == D.FILL), k
        assert not np.any(np.all(rows[live] == D.FILL, axis=1)) or k == "t", k
    assert ring["ep_steps"][live].min() >= 1 and set(np.unique(ring["t"][live])) <= {0, 1}
    newest = (count - 1) % case.capacity                # the newest record is the last step's last env
    assert ring["s"][newest, od - 1] == D.append_chunk_of(case, len(case.appends) - 1, od)["obs"][od - 1, -1, -1]
    for extra in D.append_companions(case):
        r2, c2 = D.append_expected(extra, od)
        assert c2 == sum((a.K if a.last_steps is None else min(a.K, a.last_steps)) * a.n for a in extra.appends)


def test_append_model_restarts_ep_run_on_a_gap():
    ring, _ = D.append_expected("step0_gap", 2)
    # an env with no terminal step in any chunk: 3 steps, then the gap, then 6 consecutive ones
    quiet = [e for e in range(7) if not any(D.append_done(D.APPEND_BY_NAME["step0_gap"], i)[:, e].any() for i in range(3))]
    assert quiet and all(ring["ep_run"][e] == 6 for e in quiet)
    first = D.append_done(D.APPEND_BY_NAME["step0_gap"], 0)
    assert (~first.any(axis=0)).any()                       # ... so the restart is visible: its count would be 9 without it


# ----------------------------------------------------------------------------------------------------------------- 2. samplers --
def test_sample_table_reaches_every_edge():
    dense = {c.batch for c in D.SAMPLE_CASES if c.size == c.batch}
    assert dense == {1, 2, 63, 64, 65, 1025} and max(b for b in dense if b <= D.ONE_WAVE) == D.ONE_WAVE
    assert {c.batch for c in D.SAMPLE_CASES if c.size == D.SIZE_MAX} == {D.ONE_WAVE, D.ONE_WAVE + 1}
    hi = [c for c in D.SAMPLE_CASES if c.counter0 == 2 ** 32 - 2]
    assert {c.batch > D.ONE_WAVE for c in hi} == {True, False} and all(c.n_batches == 4 for c in hi)
    assert any(c.n_batches == 0 for c in D.SAMPLE_CASES)
    keys = D.SAMPLE_MANY["keys"]
    assert len(keys) == 3 and any(k[2] == D.SAMPLE_MANY["batch"] for k in keys) and D.SAMPLE_MANY["batch"] <= D.ONE_WAVE


@pytest.mark.parametrize("case", D.SAMPLE_CASES, ids=lambda c: c.name)
def test_sample_restatement(case):
    idx = D.sample_expected(*case[1:])
    assert idx.shape == (case.n_batches, case.batch)
    assert np.all(idx >= 0) and np.all(idx < case.size)
    for row in idx:
        assert len(set(row.tolist())) == case.batch
        if case.size == case.batch:
            assert sorted(row.tolist()) == list(range(case.size))
    if case.counter0 == 2 ** 32 - 2:          # the high counter word matters: batch 2 is not the batch of counter 0
        low = O.replay_sample_indices(case.seed, 0, case.size, 1, case.batch)
        assert not np.array_equal(idx[2], low[0])


# -------------------------------------------------------------------------------------------------------------- 3. smart start --
def test_smart_tables_reach_every_edge():
    nw, wr, no = (D.append_expected(c.name, 1) for c in D.SMART_RINGS)
    assert all(c.capacity == 203 and c.appends[0].n == 5 for c in D.SMART_RINGS)
    assert nw[1] < 203 < wr[1] and no[1] > 203
    for sc in D.SMART_CASES:
        valid = D.smart_valid(sc.ring)
        idx, n_out = D.smart_expected(sc)
        assert sc.n_ss > valid.sum() and n_out <= valid.sum()
        got = idx[idx >= 0]
        assert len(set(got.tolist())) == len(got) == n_out and valid[got].all()
        if sc.name == "no_start_left":
            assert not valid.any() and n_out == 0 and np.all(idx == -1)
        else:
            assert 0 < valid.sum() and n_out > 0.9 * valid.sum() and (sc.name == "not_wrapped" or not valid.all())
        assert {-1, len(valid)} <= set(D.path_queries(sc.ring))
    ring, count = D.append_expected(D.LONG_PATH.name, 3)
    assert count == 7500 < D.LONG_PATH.capacity == 8192 and ring["ep_steps"][7499] == 7000
    path = D.path_expected(D.LONG_PATH, 3, 7499, D.LONG_PATH_MAX_LEN)
    assert path.shape == (6001, 3) and path.size > D.PATH_GRID * D.K_BLOCK          # a second trip of the grid-stride loop
    ch = D.append_chunk_of(D.LONG_PATH, 1, 3)
    assert np.array_equal(path[:-1], ch["obs"][:, 1000:, 0].T) and np.array_equal(path[-1], ch["obs2"][:, -1, 0])
    assert D.path_expected(D.LONG_PATH, 3, 7499, 1).shape == (2, 3)
    assert D.path_expected(D.LONG_PATH, 3, -1, 5).shape == (0, 3) and D.path_expected(D.LONG_PATH, 3, 7500, 5).shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------------- 4. data set --
def test_dataset_table_reaches_every_edge():
    by = D.DATASET_BY_NAME
    assert {(c.K, c.n) for c in D.DATASET_CASES if c.d == 1 and c.kind == "random"} == {(65, 70), (130, 3)}
    assert all(c.K % D.TILE_K and c.n % D.ENVS_PER_GROUP for c in D.DATASET_CASES if c.kind == "random")
    many = [c for c in D.DATASET_CASES if c.kind == "ragged"]
    assert {c.n for c in many} == {65537, 70001} and all(c.K == 3 and c.d == 2 for c in many)
    spans = []
    for c in many:
        groups = -(-c.n // D.ENVS_PER_GROUP)
        span = -(-groups // D.SCAN_THREADS)
        spans.append((span, groups % span))
        lens = D.dataset_expected(c.name)["len"]
        assert set(np.unique(lens)) == {1, 2, 3}
    assert all(s >= 2 for s, _ in spans) and any(r for _, r in spans) and any(r == 0 for _, r in spans)   # ragged and full last span
    assert [c.K for c in D.DATASET_CASES if c.kind == "directed"] == list(D.DIRECTED_K)
    assert {c.d for c in D.DATASET_CASES if c.kind == "directed"} == {1, 2, 3}
    assert {c.packed for c in D.DATASET_CASES} == {True, False}
    for c in D.CUT_CASES:
        ex = D.dataset_expected(c.name)
        total, short, mid, one, zero = D.capacity_cuts(c.name)
        assert (total, short, one, zero) == (ex["off"][-1], ex["off"][-1] - 1, 1, 0) and 1 < mid < short
        i = np.searchsorted(ex["off"], mid, side="right") - 1             # the rollout the cut falls into
        inside = mid - ex["off"][i]
        assert 0 < inside < ex["len"][i] - 1 and inside % D.TILE_K not in (0, D.TILE_K - 1) and inside > D.TILE_K
    assert {c.packed for c in D.CUT_CASES} == {True, False}


@pytest.mark.parametrize("K", D.DIRECTED_K)
def test_directed_terminal_steps(K):
    case = D.DATASET_BY_NAME["directed_k%d" % K]
    assert case.n == 70 and case.n % D.ENVS_PER_GROUP == 6
    per = (K + D.QUARTERS - 1) // D.QUARTERS
    done, envs = D.dataset_done(case), D.directed_envs(case)
    lens = D.dataset_expected(case.name)["len"]
    single = {steps[0] for steps in envs.values() if len(steps) == 1}
    for q in range(1, D.QUARTERS):                       # both sides of every quarter edge inside the chunk
        assert {s for s in (q * per - 1, q * per) if 0 <= s < K} <= single
    for q in range(D.QUARTERS):                          # both sides of every 8-step edge inside a quarter
        for k0 in range(q * per + D.LEN_UNROLL, min(q * per + per, K), D.LEN_UNROLL):
            assert {k0 - 1, k0} <= single
    assert {0, K - 1} <= single
    quarters = lambda steps: len({s // per for s in steps})
    n_q = min(D.QUARTERS, -(-K // per))
    assert any(len(s) == 0 for s in envs.values())
    assert n_q < 2 or any(quarters(s) == 2 for s in envs.values())
    assert n_q < 3 or any(quarters(s) == 3 for s in envs.values())
    for e, steps in envs.items():
        assert np.array_equal(np.flatnonzero(done[:, e]), sorted(steps))
        assert lens[e] == (min(steps) + 1 if steps else K)             # the earliest terminal step wins
    assert any(e >= D.ENVS_PER_GROUP for e in envs) and any(e < D.ENVS_PER_GROUP for e in envs)


@pytest.mark.parametrize("case", D.DATASET_CASES + D.CUT_CASES, ids=lambda c: c.name)
def test_dataset_restatement(case):
    ex, ch, done = D.dataset_expected(case.name), D.dataset_chunk(case), D.dataset_done(case)
    assert ex["off"][0] == 0 and np.array_equal(np.diff(ex["off"]), np.maximum(ex["len"] - 1, 0))
    assert ex["X"].shape == ex["Z"].shape == (ex["off"][-1], case.d) and ex["Y"].shape == (ex["off"][-1], 1)
    assert (ex["len"] == 1).any() or case.n <= 3
    for e in sorted({0, 1 % case.n, case.n - 1, int(np.argmax(ex["len"]))}):
        o, L = ex["off"][e], ex["len"][e]
        assert not done[:L - 1, e].any() and (L == case.K or done[L - 1, e])
        assert np.array_equal(ex["X"][o:o + L - 1], ch["obs"][:, :L - 1, e].T)
        assert np.array_equal(ex["Y"][o:o + L - 1, 0], ch["act"][:L - 1, e])
        assert np.array_equal(ex["Z"][o:o + L - 1], (ch["obs2"][:, :L - 1, e] - ch["obs"][:, :L - 1, e]).T)


# ------------------------------------------------------------------------------------------------------------------ 5. statistics --
def test_stats_table_reaches_every_edge():
    assert {(c.rows, c.cols) for c in D.STATS_CASES} == {(r, c) for r in (1, 5, 257) for c in (1, 2, 3, 7, 33, 64)}
    chains = {c.name: D.stats_chain(c.rows, c.cols) for c in D.STATS_CASES + [D.STATS_CAPPED]}
    assert all(not chains[c.name]["capped"] for c in D.STATS_CASES)
    assert any(ch["A"] < D.STAT_THREADS and ch["cnt"] % 2 == 1 for ch in chains.values())        # idle threads, an odd tree
    assert any(ch["A"] == D.STAT_THREADS for ch in chains.values())
    cap = chains["s_capped"]
    assert (D.STATS_CAPPED.rows, D.STATS_CAPPED.cols) == (1200001, 7)
    assert cap["capped"] and cap["blocks"] == D.STAT_BLOCKS and 1200001 * 7 > D.STAT_BLOCKS * D.STAT_THREADS * D.STAT_ELEMS
    assert cap["T"] > 16 and cap["T"] % 4 and cap["m"] == 53           # four-way trips and a tail; the chain the docstring derives
    big = [c for c in D.STATS_CASES if c.rows == 257]
    recipes = {D.stats_recipe(c, col) for c in big + [D.STATS_CAPPED] for col in range(c.cols)}
    assert set(D.STATS_RECIPES) <= recipes and (1e4, 1e-2) in D.STATS_RECIPES and (7.0, 0.0) in D.STATS_RECIPES
    assert any(D.stats_recipe(c, 0) == (7.0, 0.0) for c in big if c.cols == 1)
    assert (7.0, 0.0) in {D.stats_recipe(D.STATS_CAPPED, col) for col in range(7)}


@pytest.mark.parametrize("case", D.STATS_CASES + [D.STATS_CAPPED], ids=lambda c: c.name)
def test_stats_reference_and_bound(case):
    """The fsum reference against exact rational arithmetic where that is cheap (rows <= 257): it is right to a few u, as the bound
    assumes.  O.column_stats (numpy adds the rows of a matrix one after the other: rows * u) agrees as far as that allows.  And the
    bound is tight enough to reject a one-pass variance."""
    from fractions import Fraction
    x, r = D.stats_data(case), D.stats_reference(case)
    m_np, s_np = O.column_stats(x)
    loose = D.gamma(case.rows + 8)
    assert np.all(np.abs(m_np - r["mean"]) <= loose * r["mabs"] + r["e_mean"])
    live = r["std"] > 0
    assert np.all(np.abs(s_np - r["std"])[live] <= (loose + r["e_std"][live] / r["std"][live]) * r["std"][live])
    assert np.all(r["e_std"][live] < 1e-9 * r["std"][live])
    if case.rows <= 257:
        for c in range(case.cols):
            col = [Fraction(float(v)) for v in x[:, c]]
            mean = sum(col) / case.rows
            var = sum((v - mean) ** 2 for v in col) / case.rows
            assert abs(Fraction(r["mean"][c]) - mean) <= D.U64 * abs(mean)
            assert abs(Fraction(r["std"][c]) ** 2 - var) <= 12 * D.U64 * var
    for c in range(case.cols):
        if D.stats_recipe(case, c) == (7.0, 0.0) or case.rows == 1:
            assert r["std"][c] == 0.0 and r["e_std"][c] == 0.0 and r["mean"][c] == float(x[0, c])
        if D.stats_recipe(case, c) == (1e4, 1e-2) and case.rows >= 257:
            x64 = x[:, c].astype(np.float64)
            one_pass = np.sqrt(abs(np.mean(x64 * x64) - np.mean(x64) ** 2))
            assert abs(one_pass - r["std"][c]) > 100 * r["e_std"][c]


def test_zscore_and_noise_tables_reach_every_edge():
    assert D.ZSCORE_COLS == (5, 7, 64, 256) and D.ZSCORE_COL0 > 0 and D.ZSCORE_EXTRA > 0 and max(D.ZSCORE_COLS) == D.K_BLOCK
    span = D.K_BLOCK * D.ELEMS_PER_THREAD
    assert D.ZSCORE_ROWS == 1031 and all(span % c for c in (5, 7)) and all(D.ZSCORE_ROWS * c > span for c in D.ZSCORE_COLS)
    for cols in D.ZSCORE_COLS:
        x, mean, std = D.zscore_data(cols)
        z = O.zscore(x, mean, std)
        assert std[1] == 0 and np.all(z[:, 1] == 0.0) and std[2] == 0
        assert set(np.unique(z[:, 2])) == {-D.F32_MAX, D.F32_MAX} and np.all(np.isfinite(z))
    assert D.ZCONCAT == ((64, 3), (1, 255)) and all(a + b <= D.K_BLOCK for a, b in D.ZCONCAT)
    assert D.NOISE_COLS == (5, 8, 9, 64, 256) and D.NOISE_STREAM == 2 ** 48 - 1 and D.NOISE_ROWS > D.K_BLOCK
    for cols in D.NOISE_COLS:
        x, mean = D.noise_data(cols)
        ref, tol = D.noise_expected(cols)
        moved = mean * D.NOISE_NTS > 0
        assert moved.any() and (~moved).any() and (mean < 0).any() and (mean == 0).any()
        assert np.array_equal(ref[:, ~moved], x[:, ~moved]) and np.all(tol[:, ~moved] == 0) and np.all(ref[:, moved] != x[:, moved])
        assert any(moved[c] for c in range(D.NOISE_GROUP, cols))                 # a moving column in a group above 0
        # ... whose draw is not group 0's: dropping the group from the counter is visible
        g0 = O.add_noise_keyed(x[:, :D.NOISE_GROUP], mean[:D.NOISE_GROUP], D.NOISE_NTS, D.NOISE_SEED, D.NOISE_STREAM)
        c = next(c for c in range(D.NOISE_GROUP, cols) if moved[c])
        j = c % D.NOISE_GROUP if moved[c % D.NOISE_GROUP] else None       # the column of group 0 that shares its words and output
        if j is not None:
            d0, dc = (g0[:, j] - x[:, j]) / mean[j], (ref[:, c] - x[:, c]) / mean[c]
            assert np.abs(d0 - dc).max() > 1e-3
    assert -(-max(D.NOISE_COLS) // D.NOISE_GROUP) - 1 < 2 ** 8                  # the group fits the counter's low byte


# ------------------------------------------------------------------------------------------------------------------------ 6. pack --
def test_pack_table_reaches_every_edge():
    seen = {(c.d, D.pack_takes_16_byte_path(c), c.n % 4 == 0) for c in D.PACK_CASES}
    for d in (1, 2, 3):
        assert {(d, True, True), (d, False, False), (d, False, True)} <= seen          # 16-byte; scalar by n; scalar by d_out
    assert {c.g < c.K for c in D.PACK_CASES} == {True, False} and {c.stats for c in D.PACK_CASES} == {True, False}
    assert {c.packed for c in D.PACK_CASES} == {True, False} and all(c.offset in (0, 4) for c in D.PACK_CASES)
    assert any(D.pack_takes_16_byte_path(c) and c.g * c.n // 4 > D.K_BLOCK for c in D.PACK_CASES)
    assert any(not D.pack_takes_16_byte_path(c) and c.g * c.n > D.K_BLOCK for c in D.PACK_CASES)
    assert any((c.g * c.n * (8 * c.d + 9)) % 8 for c in D.PACK_CASES if c.stats)      # padding in front of the statistics
    for c in D.PACK_CASES:
        out = D.pack_expected(c)
        per = c.g * c.n
        assert len(out) == D.pack_bytes(c.d, c.g, c.n)
        obs = out[:4 * c.d * per].view(np.float32).reshape(c.d, c.g, c.n)
        assert np.array_equal(obs, D.synthetic_chunk(c.K, c.n, c.d)["obs"][:, c.K - c.g:])
        assert np.array_equal(out[4 * (2 * c.d + 2) * per:][:per].reshape(c.g, c.n), D.pack_done(c)[c.K - c.g:])
        tail = out[(2 * c.d + 2) * 4 * per + per:]
        assert np.all(tail[:len(tail) - 32] == D.FILL)
        assert np.array_equal(tail[-32:].view(np.float64), D.PACK_STATS) if c.stats else np.all(tail == D.FILL)
