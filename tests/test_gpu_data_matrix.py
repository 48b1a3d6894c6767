"""The data path between the arithmetic kernels on the GPU, at every instantiation: csrc/replay.hip (replay_append_kernel<0|2|3>,
replay_append_indexed_kernel<0|2|3>, replay_append_many_kernel<*, *>, the shard form, the two samplers and the population sampler,
smart_start_indices_kernel, episode_path_kernel), csrc/dataset.hip (dataset_len / group_scan / offsets, dataset_build_kernel<1|2|3>,
column_partials / column_finalize, zscore_kernel<0>, zscore_concat_kernel<0, 0>, add_noise_kernel<0>) and pack_tail_kernel<1|4>
of csrc/env_step.hip, through the C ABI and the Python wrappers, against the restatements of oracle/ssc_oracle.py as
tests/data_cases.py applies them.  The tables are held to the edges they are there for by tests/test_data_cases_cpu.py.

These kernels move integers and copy floats: everything is compared bit for bit except the statistics (a derived fp64 bound, below),
the z-score (the project's 2e-7) and the noise (the device Box-Muller).  Every array a kernel writes lies between guard bands and is
pre-filled, and is compared WHOLE: a ring row, an output column or a data-set row past the cut that the restatement never writes
must keep its fill."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import data_cases as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


class Bands:
    """device arrays between GUARD bytes of PAT on either side, every byte between pre-filled with FILL (or ``init``)"""

    def __init__(self):
        self.raw = {}

    def new(self, name, shape, dtype, init=None):
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        raw = torch.full((D.GUARD + nbytes + D.GUARD,), D.PAT, dtype=torch.uint8, device="cuda")
        body = raw[D.GUARD:D.GUARD + nbytes]
        if init is None:
            body.fill_(D.FILL)
        else:
            body.copy_(torch.from_numpy(D.as_bytes(init).copy()))
        assert name not in self.raw
        self.raw[name] = raw
        return body.view(dtype).view(shape)

    def broken(self):
        return [k for k, raw in self.raw.items()
                if not (bool((raw[:D.GUARD] == D.PAT).all()) and bool((raw[-D.GUARD:] == D.PAT).all()))]


def dev_bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def same_bytes(t, expected):
    return np.array_equal(dev_bytes(t), D.as_bytes(expected))


def device_chunk(ssc, ch, done, packed, step0=0):
    d, K, n = ch["obs"].shape
    c = ssc.TransitionChunk(d, K, n, "cuda", packed=packed)
    for name in ("obs", "obs2", "act", "rew"):
        getattr(c, name).copy_(torch.from_numpy(ch[name]))
    c.done.copy_(torch.from_numpy(done))
    c.step0 = step0
    return c


def make_ring(bands, tag, capacity, od, indexed, n_envs, max_path_len=1001):
    """a DeviceReplayBuffer whose arrays are views into guarded, pre-filled buffers (ring_struct reads data_ptr() at each call)"""
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer
    rb = DeviceReplayBuffer(capacity, od, track_episodes=indexed, n_envs=n_envs if indexed else None, max_path_len=max_path_len)
    rb.s, rb.s2 = (bands.new(f"{tag}.{k}", (capacity, od), torch.float32) for k in ("s", "s2"))
    rb.a, rb.r = bands.new(tag + ".a", (capacity, 1), torch.float32), bands.new(tag + ".r", (capacity,), torch.float32)
    rb.t = bands.new(tag + ".t", (capacity,), torch.uint8)
    if indexed:
        rb.ep_steps = bands.new(tag + ".ep_steps", (capacity,), torch.int32)
        rb.ep_run = bands.new(tag + ".ep_run", (n_envs,), torch.int32, init=np.zeros(n_envs, np.int32))
    return rb


def expected_of(case, od):
    return D.append_expected(case.name if case.name in D.APPEND_BY_NAME else case, od)


def ring_mismatches(rb, case, od):
    """the ring arrays that differ from the restatement in any byte (live rows, untouched rows, ep_steps, ep_run), and the count"""
    ring, count = expected_of(case, od)
    keys = ("s", "a", "r", "t", "s2") + (("ep_steps", "ep_run") if rb.track_episodes else ())
    bad = [k for k in keys if not same_bytes(getattr(rb, k), ring[k])]
    return bad + ([] if rb.count == count else ["count"])


def ring_from_case(ssc, bands, tag, case, od, indexed=True, max_path_len=1001):
    rb = make_ring(bands, tag, case.capacity, od, indexed, case.appends[0].n, max_path_len)
    for i, a in enumerate(case.appends):
        rb.append_chunk(device_chunk(ssc, D.append_chunk_of(case, i, od), D.append_done(case, i), a.packed, a.step0),
                        reward_scale=a.reward_scale, last_steps=a.last_steps)
    return rb


# ------------------------------------------------------------------------------------------------------------------- 1. append --
@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])
@pytest.mark.parametrize("od", [1, 2, 3])
@pytest.mark.parametrize("case", D.APPEND_CASES, ids=lambda c: c.name)
def test_append_single_and_many(ssc, case, od, indexed):
    """Every case through ssc_replay_append, and again as pair 0 of an ssc_replay_append_many launch whose other pairs differ in
    n, K and capacity (one of them with K = 0): every byte of every ring equals O.replay_append / O.replay_episode_steps."""
    from smartstartcontinuous_amd.replay_buffer import DeviceReplayPopulation
    bands = Bands()
    trio = (case,) + D.append_companions(case)
    single = make_ring(bands, "single", case.capacity, od, indexed, case.appends[0].n)
    many = [make_ring(bands, "many%d" % p, c.capacity, od, indexed, c.appends[0].n) for p, c in enumerate(trio)]
    pop = DeviceReplayPopulation(many)
    for i, a in enumerate(case.appends):
        chunks = [device_chunk(ssc, D.append_chunk_of(c, i, od), D.append_done(c, i), c.appends[i].packed, c.appends[i].step0)
                  for c in trio]
        assert (chunks[0].act.stride(0) != a.n) == (a.packed and a.K > 0)            # packed: row_stride != n
        single.append_chunk(chunks[0], reward_scale=a.reward_scale, last_steps=a.last_steps)
        pop.append_chunks(chunks, reward_scale=[c.appends[i].reward_scale for c in trio], last_steps=a.last_steps)
        assert pop.fused
    torch.cuda.synchronize()
    assert ring_mismatches(single, case, od) == []
    for rb, c in zip(many, trio):
        assert ring_mismatches(rb, c, od) == [], c.name
    assert all(b == D.FILL for b in dev_bytes(many[2].s)[:16])                       # the K = 0 pair's ring is untouched
    assert bands.broken() == []


@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])
@pytest.mark.parametrize("od", [1, 3])
def test_append_shards_equal_the_whole_append(ssc, od, indexed):
    """150 envs per step delivered as shards of 37, 64 and 49 envs at offsets 0, 37 and 101, in shuffled order, one of them a dense
    copy: the ring equals append_chunk of the whole chunk, and the restatement, in every byte -- ep_run included."""
    case, bands = D.SHARD_CASE, Bands()
    whole = make_ring(bands, "whole", case.capacity, od, indexed, 150)
    sharded = make_ring(bands, "sharded", case.capacity, od, indexed, 150)
    a0, a1 = case.appends
    c0, c1 = (device_chunk(ssc, D.append_chunk_of(case, i, od), D.append_done(case, i), a.packed, a.step0)
              for i, a in enumerate(case.appends))
    for rb in (whole, sharded):
        rb.append_chunk(c0, reward_scale=a0.reward_scale)
    whole.append_chunk(c1, reward_scale=a1.reward_scale)
    shards = []
    for j, (n, off) in enumerate(D.SHARDS):
        cols = [c1.obs[:, :, off:off + n], c1.act[:, off:off + n], c1.rew[:, off:off + n], c1.obs2[:, :, off:off + n],
                c1.done[:, off:off + n]]
        if j == 1:
            cols = [x.contiguous() for x in cols]
        shards.append((ssc.TransitionChunk.from_columns(*cols), off))
    sharded.append_shards(shards, 150, reward_scale=a1.reward_scale)
    torch.cuda.synchronize()
    assert ring_mismatches(whole, case, od) == [] and ring_mismatches(sharded, case, od) == []
    assert bands.broken() == []


# ----------------------------------------------------------------------------------------------------------------- 2. samplers --
def sample_device(ssc, bands, name, seed, counter0, size, n_batches, batch, rows=None):
    from smartstartcontinuous_amd import _ffi
    idx = bands.new(name, (n_batches if rows is None else rows, batch), torch.int32)
    _ffi.check(_ffi.lib().ssc_replay_sample(seed, counter0, size, n_batches, batch, _ffi.ptr(idx), _ffi.stream()))
    torch.cuda.synchronize()
    return idx


@pytest.mark.parametrize("case", D.SAMPLE_CASES, ids=lambda c: c.name)
def test_samplers_at_the_edges_of_size(ssc, case):
    """size == batch_size (every index once), size = 2^31 - 1, a batch counter that crosses 2^32, and no batch at all: the
    one-wave kernel up to 64, the workgroup kernel above, bit for bit with O.replay_sample_indices."""
    bands = Bands()
    idx = sample_device(ssc, bands, "idx", *case[1:], rows=max(case.n_batches, 2))
    got = idx.cpu().numpy()
    ref = D.sample_expected(*case[1:])
    assert np.array_equal(got[:case.n_batches], ref)
    assert np.all(dev_bytes(idx[case.n_batches:]) == D.FILL) and bands.broken() == []
    if case.size == case.batch:
        assert all(sorted(row.tolist()) == list(range(case.size)) for row in got[:case.n_batches])
    assert np.all(got[:case.n_batches] < case.size) and np.all(got[:case.n_batches] >= 0)


def test_sample_many_equals_the_single_calls(ssc):
    from smartstartcontinuous_amd import _ffi
    from smartstartcontinuous_amd.population import DeviceItems
    bands, m = Bands(), D.SAMPLE_MANY
    keys = DeviceItems(_ffi.ReplaySampleKey, len(m["keys"]), "cuda")
    for it, (seed, counter0, size) in zip(keys.items, m["keys"]):
        it.seed, it.counter0, it.size = seed, counter0, size
    keys.upload()
    idx = bands.new("many", (len(m["keys"]), m["n_batches"], m["batch"]), torch.int32)
    _ffi.check(_ffi.lib().ssc_replay_sample_many(keys.h_ptr, keys.d_ptr, len(m["keys"]), m["n_batches"], m["batch"], _ffi.ptr(idx),
                                                 _ffi.stream()))
    torch.cuda.synchronize()
    for p, key in enumerate(m["keys"]):
        one = sample_device(ssc, bands, "one%d" % p, *key, m["n_batches"], m["batch"])
        assert torch.equal(idx[p], one) and np.array_equal(one.cpu().numpy(), D.sample_expected(*key, m["n_batches"], m["batch"]))
    assert bands.broken() == []


# -------------------------------------------------------------------------------------------------------------- 3. smart start --
def path_device(rb, bands, name, buffer_index, max_len):
    """ssc_replay_episode_path into a pre-filled buffer -> (len, the whole buffer [max_len + 1, od])"""
    from smartstartcontinuous_amd import _ffi
    path = bands.new(name + ".path", (max_len + 1, rb.obs_dim), torch.float32)
    plen = bands.new(name + ".len", (1,), torch.int32)
    bi = torch.tensor([buffer_index], dtype=torch.int32, device="cuda")
    ring = rb.ring_struct()
    _ffi.check(_ffi.lib().ssc_replay_episode_path(ctypes.byref(ring), rb.count, rb.n_envs, _ffi.ptr(bi), max_len, _ffi.ptr(path),
                                                  _ffi.ptr(plen), _ffi.stream()))
    torch.cuda.synchronize()
    return int(plen.item()), path


def path_as_expected(rb, bands, name, case, od, buffer_index, max_len):
    rows, path = path_device(rb, bands, name, buffer_index, max_len)
    ref = D.path_expected(case, od, buffer_index, max_len)
    whole = D.filled((max_len + 1, od), np.float32)
    whole[:len(ref)] = ref
    return rows == len(ref) and same_bytes(path, whole)


@pytest.mark.parametrize("od", [1, 3])
@pytest.mark.parametrize("sc", D.SMART_CASES, ids=lambda c: c.name)
def test_smart_start_candidates_and_paths(ssc, sc, od):
    """More candidates asked than there are valid records, on a ring not yet wrapped, a wrapped one and one whose every episode
    start is evicted (n_out 0, every entry -1): O.smart_start_indices bit for bit.  Then the paths to the records at the edges of
    the ring and of the valid set, at three max_len, and buffer_index -1 and size: len 0 and nothing written."""
    from smartstartcontinuous_amd import _ffi
    bands, case = Bands(), sc.ring
    rb = ring_from_case(ssc, bands, "ring", case, od)
    assert ring_mismatches(rb, case, od) == []
    lib = _ffi.lib()
    idx, n_out = bands.new("idx", (sc.n_ss,), torch.int32), bands.new("n_out", (1,), torch.int32)
    nb = int(lib.ssc_replay_smart_start_workspace_bytes(sc.n_ss))
    ws = bands.new("ws", (nb,), torch.uint8)
    ring = rb.ring_struct()
    _ffi.check(lib.ssc_replay_smart_start_indices(ctypes.byref(ring), rb.count, rb.n_envs, sc.n_ss, sc.seed, sc.counter, _ffi.ptr(idx),
                                                  _ffi.ptr(n_out), _ffi.ptr(ws), nb, _ffi.stream()))
    torch.cuda.synchronize()
    ref, ref_n = D.smart_expected(sc)
    assert np.array_equal(idx.cpu().numpy(), ref) and int(n_out.item()) == ref_n
    rb.seed, rb._queries = sc.seed ^ 0x5353, sc.counter          # the wrapper's key for the same draw
    got = rb.get_possible_smart_start_indices(sc.n_ss)
    assert (got is None and ref_n == 0) or np.array_equal(got.cpu().numpy(), ref[ref >= 0])
    for bi in D.path_queries(case):
        for max_len in (1001, 3, 1):
            assert path_as_expected(rb, bands, "q%d_%d" % (bi, max_len), case, od, bi, max_len), (bi, max_len)
    assert ring_mismatches(rb, case, od) == [] and bands.broken() == []          # the queries write nothing into the ring


def test_long_path_takes_a_second_grid_trip(ssc):
    """One env, an episode of 7000 steps in 8192 rows, max_path_len 6000, obs_dim 3: 18 003 path elements for a grid capped at 64
    blocks of 256 threads."""
    bands, case = Bands(), D.LONG_PATH
    rb = ring_from_case(ssc, bands, "ring", case, 3, max_path_len=D.LONG_PATH_MAX_LEN)
    assert ring_mismatches(rb, case, 3) == []
    for bi, max_len in ((7499, D.LONG_PATH_MAX_LEN), (7499, 1), (-1, D.LONG_PATH_MAX_LEN), (7500, D.LONG_PATH_MAX_LEN), (499, 8000)):
        assert path_as_expected(rb, bands, "q%d_%d" % (bi, max_len), case, 3, bi, max_len), (bi, max_len)
    got = rb.get_episodic_path_to_buffer_index(7499).cpu().numpy()
    assert np.array_equal(got, D.path_expected(case, 3, 7499, D.LONG_PATH_MAX_LEN)) and got.shape == (6001, 3)
    assert bands.broken() == []


# ------------------------------------------------------------------------------------------------------------------- 4. data set --
def scan_and_build(ssc, bands, case, capacity=None):
    """ssc_dataset_scan, then ssc_dataset_build with ``capacity_rows`` (None: the total) into X, Y, Z that hold the total"""
    from smartstartcontinuous_amd import _ffi
    lib = _ffi.lib()
    chunk = device_chunk(ssc, D.dataset_chunk(case), D.dataset_done(case), case.packed)
    n, K, d = case.n, case.K, case.d
    lens, off = bands.new("len", (n,), torch.int32), bands.new("off", (n + 1,), torch.int64)
    nb = int(lib.ssc_dataset_scan_workspace_bytes(n))
    ws = bands.new("ws", (nb,), torch.uint8)
    log = chunk.as_struct()
    _ffi.check(lib.ssc_dataset_scan(ctypes.byref(log), K, n, _ffi.ptr(lens), _ffi.ptr(off), _ffi.ptr(ws), nb, _ffi.stream()))
    total = int(off[n].item())
    X, Z = (bands.new(k, (total, d), torch.float32) for k in "XZ")
    Y = bands.new("Y", (total, 1), torch.float32)
    _ffi.check(lib.ssc_dataset_build(ctypes.byref(log), d, K, n, _ffi.ptr(lens), _ffi.ptr(off), total if capacity is None else capacity,
                                     _ffi.ptr(X), _ffi.ptr(Y), _ffi.ptr(Z), _ffi.stream()))
    torch.cuda.synchronize()
    return chunk, dict(len=lens, off=off, X=X, Y=Y, Z=Z)


@pytest.mark.parametrize("case", D.DATASET_CASES, ids=lambda c: c.name)
def test_dataset_scan_and_build(ssc, case):
    """dataset_build_kernel<1> off the tile grid; 1025 and 1094 groups of ragged rollouts (two groups per scan thread, a ragged and a
    full last span); one terminal step either side of every quarter edge and 8-step edge of dataset_len_kernel, terminal steps in
    two and three quarters, K from 1 up: len, off, off[n] and every row bit for bit, and the wrapper gives the same."""
    from smartstartcontinuous_amd import collect_samples as cs
    bands = Bands()
    chunk, got = scan_and_build(ssc, bands, case)
    ex = D.dataset_expected(case.name)
    assert [k for k in ("len", "off", "X", "Y", "Z") if not same_bytes(got[k], ex[k])] == []
    assert bands.broken() == []
    ts = cs.dataset_from_chunk(chunk)
    assert torch.equal(ts.dataX, got["X"]) and torch.equal(ts.dataY, got["Y"]) and torch.equal(ts.dataZ, got["Z"])
    assert torch.equal(ts.lens, got["len"]) and torch.equal(ts.offsets, got["off"])


@pytest.mark.parametrize("case", D.CUT_CASES, ids=lambda c: c.name)
def test_dataset_build_stops_at_capacity_rows(ssc, case):
    """capacity_rows = the total, one row short, a value inside the second 64-step tile of a rollout, 1 and 0: the rows below the cut
    equal the full build, the rows from the cut onward keep their fill."""
    ex = D.dataset_expected(case.name)
    for cut in D.capacity_cuts(case.name):
        bands = Bands()
        _, got = scan_and_build(ssc, bands, case, capacity=cut)
        for k in "XYZ":
            want = D.filled(ex[k].shape, np.float32)
            want[:cut] = ex[k][:cut]
            assert same_bytes(got[k], want), (k, cut)
        assert bands.broken() == []


# ------------------------------------------------------------------------------------------------------------------ 5. statistics --
def stats_device(bands, name, x):
    from smartstartcontinuous_amd import _ffi
    lib = _ffi.lib()
    rows, cols = x.shape
    mean, std = bands.new(name + ".mean", (cols,), torch.float64), bands.new(name + ".std", (cols,), torch.float64)
    nb = int(lib.ssc_column_stats_workspace_bytes(cols))
    ws = bands.new(name + ".ws", (nb,), torch.uint8)
    _ffi.check(lib.ssc_column_stats(_ffi.ptr(x), rows, cols, _ffi.ptr(mean), _ffi.ptr(std), _ffi.ptr(ws), nb, _ffi.stream()))
    torch.cuda.synchronize()
    return mean, std


@pytest.mark.parametrize("case", D.STATS_CASES + [D.STATS_CAPPED], ids=lambda c: c.name)
def test_column_stats_within_the_derived_bound(ssc, case):
    """The bound, from the kernel's summation order.  u = 2^-53.  An element of column c is added into one of a thread's four
    accumulators; the busiest thread holds T = ceil(total / S) elements (S = blocks * A active threads in all), so its first
    accumulator takes floor(T / 4) + T % 4 additions, the first of them into an exact zero.  Then the two combining additions
    (a0 + a1) + (a2 + a3), the 8 levels of the block's tree, ceil(blocks / 64) additions in a lane of the finalize wave and the 6
    butterfly levels: m additions in the longest chain (data_cases.stats_chain), each with relative error at most u, and one division
    by rows that the exact first addition pays for.  A sum of terms t_i through chains of at most m roundings is off by at most
    gamma_m * sum |t_i|, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, lemma 3.1 and section 4.2), so

        |mean - ref| <= gamma_m * sum |x_c| / rows                                                            =: E.

    Pass 1 adds (x - mean)^2 with the mean the kernel found: three more roundings per term (the subtraction, the product counted
    twice), all terms non-negative, so the sum is right to gamma_(m+3) RELATIVE to itself; it is the sum about the kernel's mean,
    which exceeds the sum about the true mean by rows * (mean - true)^2 exactly, i.e. by (E' / std)^2 relative with
    E' = E + u |mean| (the reference mean is rounded too); the division and the square root add u each and the reference, whose
    squared deviations are rounded before math.fsum adds them exactly, 3u more.  sqrt(1 + t) - 1 <= t, so

        |std - ref| <= (gamma_(m+3) + (E' / ref)^2 + 6u) * ref,        and std == 0.0 exactly where ref == 0.

    m = 53 for the capped case (T = 17, 2048 blocks), 18..21 for the small ones: 6e-15 and 3e-15 relative, where the hand-set
    tolerances were 1e-13 and 1e-12.  The reference is math.fsum on the same fp32 data (data_cases.stats_reference)."""
    bands = Bands()
    x = torch.from_numpy(np.array(D.stats_data(case))).cuda()
    mean, std = stats_device(bands, "a", x)
    r, chain = D.stats_reference(case), D.stats_chain(case.rows, case.cols)
    m, s = mean.cpu().numpy(), std.cpu().numpy()
    live = r["std"] > 0
    ratio_m = np.max(np.abs(m - r["mean"]) / np.maximum(r["e_mean"], 1e-300))
    ratio_s = np.max(np.abs(s - r["std"])[live] / r["e_std"][live]) if live.any() else 0.0
    print("DATA_MATRIX %s blocks=%d m=%d |mean - ref| / bound = %.3f  |std - ref| / bound = %.3f"
          % (case.name, chain["blocks"], chain["m"], ratio_m, ratio_s))
    assert np.all(np.abs(m - r["mean"]) <= r["e_mean"]), ratio_m
    assert np.all(np.abs(s - r["std"]) <= r["e_std"]), ratio_s
    assert np.all(s[~live] == 0.0)
    mean2, std2 = stats_device(bands, "b", x)                             # fixed summation order: the same bits again
    assert same_bytes(mean2, m) and same_bytes(std2, s) and bands.broken() == []


@pytest.mark.parametrize("cols", D.ZSCORE_COLS)
def test_zscore_run_time_column_counts(ssc, cols):
    """zscore_kernel<0> at 5, 7, 64 and 256 columns into columns [2, 2 + cols) of a wider matrix whose other columns keep their fill;
    1031 rows put block spans in the middle of rows; a zero std gives 0 where x is the mean and -+ the largest fp32 elsewhere."""
    from smartstartcontinuous_amd import collect_samples as cs
    bands = Bands()
    x, mean, std = D.zscore_data(cols)
    stride = D.ZSCORE_COL0 + cols + D.ZSCORE_EXTRA
    out = bands.new("out", (D.ZSCORE_ROWS, stride), torch.float32)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    cs.zscore_into(dev(x), dev(mean), dev(std), out, col0=D.ZSCORE_COL0)
    torch.cuda.synchronize()
    got, ref = out.cpu().numpy(), O.zscore(x, mean, std)
    inner = got[:, D.ZSCORE_COL0:D.ZSCORE_COL0 + cols]
    assert np.allclose(inner, ref, rtol=2e-7, atol=0)
    assert np.all(inner[:, 1] == 0.0) and np.array_equal(inner[:, 2], ref[:, 2]) and set(np.unique(inner[:, 2])) == {-D.F32_MAX, D.F32_MAX}
    outside = np.delete(out.cpu().numpy().view(np.uint8).reshape(D.ZSCORE_ROWS, stride, 4),
                        np.arange(D.ZSCORE_COL0, D.ZSCORE_COL0 + cols), axis=1)
    assert np.all(outside == D.FILL) and bands.broken() == []


@pytest.mark.parametrize("cx,cy", D.ZCONCAT)
def test_zscore_concat_run_time_column_counts(ssc, cx, cy):
    """zscore_concat_kernel<0, 0> at 64 + 3 and 1 + 255 columns: bit-equal to two ssc_zscore launches into the same matrix"""
    from smartstartcontinuous_amd import collect_samples as cs
    bands = Bands()
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    (x, mx, sx), (y, my, sy) = D.zscore_data(cx, "zx"), D.zscore_data(cy, "zy")
    one = bands.new("one", (D.ZSCORE_ROWS, cx + cy), torch.float32)
    two = bands.new("two", (D.ZSCORE_ROWS, cx + cy), torch.float32)
    xd, yd, mxd, sxd, myd, syd = (dev(a) for a in (x, y, mx, sx, my, sy))
    cs.zscore_concat(xd, mxd, sxd, yd, myd, syd, out=one)
    cs.zscore_into(xd, mxd, sxd, two, 0)
    cs.zscore_into(yd, myd, syd, two, cx)
    torch.cuda.synchronize()
    assert same_bytes(one, two.cpu().numpy()) and bands.broken() == []
    ref = np.concatenate([O.zscore(x, mx, sx), O.zscore(y, my, sy)], axis=1)
    assert np.allclose(one.cpu().numpy(), ref, rtol=2e-7, atol=0)


@pytest.mark.parametrize("cols", D.NOISE_COLS)
def test_add_noise_run_time_column_counts(ssc, cols):
    """add_noise_kernel<0> with 2 .. 64 column groups (the group rides in the low byte of the counter under stream_id = 2^48 - 1):
    the columns whose mean is not positive keep their bits, the others move by O.add_noise_keyed's draws."""
    from smartstartcontinuous_amd import collect_samples as cs
    bands = Bands()
    x, mean = D.noise_data(cols)
    xd = bands.new("x", x.shape, torch.float32, init=x)
    cs.add_noise_device(xd, D.NOISE_NTS, D.NOISE_SEED, stream_id=D.NOISE_STREAM, mean=torch.from_numpy(np.array(mean)).cuda())
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    ref, tol = D.noise_expected(cols)
    still = tol[0] == 0
    assert np.array_equal(got[:, still], x[:, still])
    err = np.abs(got.astype(np.float64) - ref)
    print("DATA_MATRIX noise cols=%d worst |x - ref| / tol = %.3f" % (cols, np.max(err[:, ~still] / tol[:, ~still])))
    assert np.all(err <= tol) and np.all(got[:, ~still] != x[:, ~still]) and bands.broken() == []


# ------------------------------------------------------------------------------------------------------------------------ 6. pack --
@pytest.mark.parametrize("c", D.PACK_CASES, ids=lambda c: c.name)
def test_pack_transitions_layout(ssc, c):
    """pack_tail_kernel<4> and <1> (by n % 4, and by a d_out 4 bytes off its alignment) for obs_dim 1, 2, 3, g < K and g == K, with
    and without the statistics block, packed and dense source chunks: every byte of the buffer as include/ssc.h lays it out, the
    padding and an absent statistics block left as they were."""
    from smartstartcontinuous_amd import _ffi
    lib, bands = _ffi.lib(), Bands()
    chunk = device_chunk(ssc, D.synthetic_chunk(c.K, c.n, c.d), D.pack_done(c), c.packed)
    nb = int(lib.ssc_pack_bytes(c.d, c.g, c.n))
    assert nb == D.pack_bytes(c.d, c.g, c.n)
    body = bands.new("out", (c.offset + nb,), torch.uint8)
    out = body[c.offset:]
    assert (out.data_ptr() % 16 == 0) == (c.offset == 0) and chunk.done.data_ptr() % 16 == 0
    stats = torch.from_numpy(D.PACK_STATS.copy()).cuda() if c.stats else None
    log = chunk.as_struct()
    _ffi.check(lib.ssc_pack_transitions(ctypes.byref(log), c.d, c.K, c.g, c.n, _ffi.ptr(stats), _ffi.ptr(out), _ffi.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), D.pack_expected(c))
    assert np.all(body[:c.offset].cpu().numpy() == D.FILL) and bands.broken() == []
