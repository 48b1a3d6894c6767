"""The rest of a population chunk in one launch each (ssc_rollout_many, ssc_replay_append_many, ssc_decay_schedule_many,
ssc_obs_rms_update_many; VecEnvPopulation, DeviceReplayPopulation, DecayScheduleGroup, ObsRmsGroup; the population loop on
them).  Every result is DEFINED as what the per-pair calls give, so every comparison here is torch.equal: no tolerance.  The
one exception is the f64 reward sum d_stats[0], which the workgroups of a pair add atomically in no fixed order in the
single launch too: for a pair of b workgroups it is held to (b - 1) * 2^-53 * sum |per-workgroup partial|, the right side
bounded from the log's reward column (b = 1: exact).  Episode-ring records are compared after sorting (their slot order is
an atomic's in both forms), the ring cursors exactly.

The kernel tests drive the C entry points on arrays of their own: every state and log array of every pair sits between
two guard bands."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import actor_weights

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G = 64                    # guard elements either side of every array
SENT = -12345.0
SENT_I = 0x5A5A5A5A
SENT_B = 0xA5


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


@pytest.fixture(autouse=True)
def _no_path_switches(monkeypatch):
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)


def guarded(values, dtype, sent):
    """1-d device tensor [G | values | G]"""
    v = np.asarray(values)
    full = np.full(v.size + 2 * G, sent, dtype=v.dtype)
    full[G:G + v.size] = v.reshape(-1)
    return torch.as_tensor(full, device="cuda").to(dtype)


def device_copy(items):
    return torch.frombuffer(bytearray(items), dtype=torch.uint8).cuda()


class Pairs:
    """P (env set, actor policy) pairs as raw arrays: per pair its own n, seed, env_id0, device epsilon, OU constants,
    obs_clip, actor weights, a state in mid-episode (steps 0..4 of max_episode_steps = 5), a packed log of K steps and an
    episode ring.  ``scramble``: the pair whose log keeps act at the LOWEST column address, so that its columns cannot be
    addressed from obs[0] (the generic, non-ONEBASE stores)."""

    def __init__(self, ffi, kind, ns, K, bounds, llt, stats, clips, log=True, ring=True, scramble=None, seed=0):
        self.ffi, self.kind, self.ns, self.K, self.P = ffi, kind, list(ns), K, len(ns)
        self.O = O = 2 if kind == ffi.SSC_ENV_MOUNTAINCAR else 3
        self.log, self.ring, self.bounds, self.llt = log, ring, bounds, llt
        rng = np.random.default_rng(500 + seed)
        self.T, self.W, self.eps, self.rms, self.meta = [], [], [], [], []
        ncol = 2 * O + 2
        for p, n in enumerate(self.ns):
            t = {}
            if kind == ffi.SSC_ENV_MOUNTAINCAR:
                t["s0"] = guarded(rng.uniform(-0.9, 0.3, n).astype(np.float32), torch.float32, SENT)
                t["s1"] = guarded(rng.uniform(-0.03, 0.03, n).astype(np.float32), torch.float32, SENT)
            else:
                t["s0"] = guarded(rng.uniform(-3.0, 3.0, n).astype(np.float32), torch.float32, SENT)
                t["s1"] = guarded(rng.uniform(-1.0, 1.0, n).astype(np.float32), torch.float32, SENT)
            t["steps"] = guarded(rng.integers(0, 5, n).astype(np.int32), torch.int32, SENT_I)
            t["ep_ret"] = guarded(rng.uniform(-2.0, 0.0, n).astype(np.float32), torch.float32, SENT)
            t["ou_x"] = guarded(rng.uniform(-0.3, 0.3, n).astype(np.float32), torch.float32, SENT)
            t["cols"] = guarded(np.full(K * ncol * n, SENT, np.float32), torch.float32, SENT)       # [K][ncol][n]
            t["done"] = guarded(np.full(K * n, SENT_B, np.uint8), torch.uint8, SENT_B)
            cap = 4 * n + 8
            t["ring_id"] = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
            t["ring_len"] = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
            t["ring_ret"] = torch.full((cap,), SENT, dtype=torch.float32, device="cuda")
            t["cursor"] = torch.zeros(1, dtype=torch.int32, device="cuda")
            t["stats"] = torch.zeros(4, dtype=torch.float64, device="cuda")
            self.T.append(t)
            w = actor_weights(O, 64, 32, seed=70 + 13 * p + seed, w3_scale=0.5)
            self.W.append({k: torch.as_tensor(v, device="cuda") for k, v in w.items()})
            self.eps.append(torch.tensor([0.3 + 0.2 * p], dtype=torch.float32, device="cuda"))
            if stats:
                mean, std, cnt = rng.uniform(-0.3, 0.3, O), rng.uniform(0.2, 0.9, O), 1000.0 + p
                self.rms.append(torch.as_tensor(np.concatenate([mean * cnt, (std * std + mean * mean) * cnt, [cnt]]), device="cuda"))
            else:
                self.rms.append(None)
            slots = list(range(ncol))
            if scramble == p:
                slots[0], slots[O] = slots[O], slots[0]          # obs[0] <-> act
            self.meta.append(dict(seed=1000 + 77 * p + seed, env_id0=(1 << 33) + 5 if p == 2 else 4096 * p, cap=cap, slots=slots,
                                  ou=(0.4 - 0.1 * p, 0.6 + 0.05 * p, 0.15 + 0.02 * p, 1e-2 * (1 + p)), clip=clips[p % len(clips)]))

    def clone(self):
        import copy
        other = copy.copy(self)
        other.T = [{k: v.clone() for k, v in t.items()} for t in self.T]        # weights, epsilon and statistics are read-only
        return other

    def view(self, p, name):
        n = self.ns[p]
        size = {"cols": self.K * (2 * self.O + 2) * n, "done": self.K * n}.get(name, n)
        return self.T[p][name][G:G + size]

    # ---- descriptors --------------------------------------------------------------------------------------------
    def params(self, p):
        prm = self.ffi.default_params(self.kind, 1.0 + 0.1 * p, 5)
        if self.kind == self.ffi.SSC_ENV_PENDULUM:
            prm.g, prm.pend_v1_order = 10.0 - p, p % 2
        return prm

    def policy(self, p):
        ffi, m = self.ffi, self.meta[p]
        pd = ffi.PolicyDesc()
        pd.kind, (pd.act_low, pd.act_high) = ffi.SSC_POLICY_ACTOR, self.bounds
        a = pd.actor
        a.obs_dim, a.h1, a.h2, a.act_dim = self.O, 64, 32, 1
        ffi.set_net_ptrs(a, self.W[p])
        a.last_layer_tanh, a.precision, a.obs_clip = int(self.llt if not isinstance(self.llt, (list, tuple)) else self.llt[p]), \
            ffi.SSC_PREC_BF16_MFMA, m["clip"]
        pd.ou.mu, pd.ou.sigma, pd.ou.theta, pd.ou.dt = m["ou"]
        pd.ou.epsilon, pd.ou.d_epsilon = 0.0, self.eps[p].data_ptr()
        return pd

    def state(self, p):
        return self.ffi.RolloutState(*(self.view(p, k).data_ptr() for k in ("s0", "s1", "steps", "ep_ret", "ou_x")))

    def log_struct(self, p):
        n, O, slots = self.ns[p], self.O, self.meta[p]["slots"]
        base = self.view(p, "cols").data_ptr()
        log = self.ffi.TransitionLog()
        for c in range(O):
            log.obs[c] = base + 4 * n * slots[c]
            log.obs2[c] = base + 4 * n * slots[O + 2 + c]
        log.act, log.rew = base + 4 * n * slots[O], base + 4 * n * slots[O + 1]
        log.done = self.view(p, "done").data_ptr()
        log.row_stride, log.done_row_stride = (2 * O + 2) * n, 0
        return log

    def ring_struct(self, p):
        t = self.T[p]
        r = self.ffi.EpisodeRing()
        r.env_id, r.length, r.ret, r.cursor = (t[k].data_ptr() for k in ("ring_id", "ring_len", "ring_ret", "cursor"))
        r.capacity = self.meta[p]["cap"]
        return r

    def column(self, p, c):
        """[K, n] view of fp32 log column c (obs.., act, rew, obs2..)"""
        n = self.ns[p]
        return self.view(p, "cols").view(self.K, 2 * self.O + 2, n)[:, self.meta[p]["slots"][c]]

    # ---- the two ways ---------------------------------------------------------------------------------------------
    def roll_single(self, step0, log=None):
        ffi, lib = self.ffi, self.ffi.lib()
        log = self.log if log is None else log
        for p, n in enumerate(self.ns):
            prm, pd, st, m = self.params(p), self.policy(p), self.state(p), self.meta[p]
            lg, rg = self.log_struct(p), self.ring_struct(p)
            ffi.check(lib.ssc_rollout_rms(ctypes.byref(prm), ctypes.byref(pd), n, self.K, ctypes.byref(st),
                                          ctypes.byref(lg) if log else None, ctypes.byref(rg) if self.ring else None,
                                          ffi.ptr(self.T[p]["stats"]), m["seed"], m["env_id0"], step0, ffi.stream(), ffi.ptr(self.rms[p])))
        torch.cuda.synchronize()

    def roll_many(self, step0):
        ffi = self.ffi
        items, cursors = (ffi.RolloutManyItem * self.P)(), (ffi.PairCursor * self.P)()
        for p, it in enumerate(items):
            m = self.meta[p]
            it.params, it.policy, it.n, it.state = self.params(p), self.policy(p), self.ns[p], self.state(p)
            it.has_log, it.has_ring = int(self.log), int(self.ring)
            if self.log:
                it.log = self.log_struct(p)
            if self.ring:
                it.ring = self.ring_struct(p)
            it.d_stats, it.seed, it.env_id0 = self.T[p]["stats"].data_ptr(), m["seed"], m["env_id0"]
            it.d_rms = None if self.rms[p] is None else self.rms[p].data_ptr()
            cursors[p].step0, cursors[p].replay_start = step0, -1       # (replay_start is the append's)
        d_items, d_cursors = device_copy(items), device_copy(cursors)
        ffi.check(ffi.lib().ssc_rollout_many(ctypes.addressof(items), d_items.data_ptr(), ctypes.addressof(cursors), d_cursors.data_ptr(),
                                             self.P, self.K, ffi.stream()))
        torch.cuda.synchronize()

    # ---- comparisons ----------------------------------------------------------------------------------------------
    def assert_guards(self):
        for p, t in enumerate(self.T):
            for name, sent in (("s0", SENT), ("s1", SENT), ("steps", SENT_I), ("ep_ret", SENT), ("ou_x", SENT), ("cols", SENT),
                               ("done", SENT_B)):
                x, size = t[name], self.view(p, name).numel()
                assert bool((x[:G] == sent).all()) and bool((x[G + size:] == sent).all()), (p, name)

    def assert_equal(self, ref, rewards, lanes_per_env):
        """``rewards[p]``: a [K, n] reward column of this call (for the bound on the reward sum)"""
        for p, n in enumerate(self.ns):
            a, b = self.T[p], ref.T[p]
            for name in ("s0", "s1", "steps", "ep_ret", "ou_x", "cols", "done", "cursor"):
                assert torch.equal(a[name], b[name]), (p, name)
            got, want = a["stats"].cpu().numpy(), b["stats"].cpu().numpy()
            assert np.array_equal(got[1:], want[1:]), (p, got, want)
            blocks = -(-n // (256 // lanes_per_env))
            # |partial| <= sum |rewards| (1 + 2^-24)^K: every env's fp32 running sum rounds K times
            bound = (blocks - 1) * 2.0 ** -53 * float(rewards[p].double().abs().sum()) * (1 + 2.0 ** -20)
            if blocks > 1:
                print(f"pair {p} n {n}: reward sum {got[0]!r} single {want[0]!r}: |got - want| = {abs(got[0] - want[0]):.3e}, "
                      f"bound {bound:.3e} ({blocks} workgroups)")
            assert abs(got[0] - want[0]) <= bound, (p, got[0], want[0], bound)
            if self.ring:
                k = int(a["cursor"].item())
                assert 0 < k <= self.meta[p]["cap"] or n * self.K < 5, (p, k)
                rec = lambda t: sorted(zip(t["ring_id"][:k].tolist(), t["ring_len"][:k].tolist(), t["ring_ret"][:k].tolist()))
                assert rec(a) == rec(b), p
                assert torch.equal(a["ring_id"][k:], b["ring_id"][k:]) and torch.equal(a["ring_ret"][k:], b["ring_ret"][k:])


NS = (1, 70, 129, 257)
MC, PEND = 0, 1
# (env, action bounds, last_layer_tanh, statistics, per-pair obs_clip, log + ring, the pair with a scrambled log, lanes per env)
CASES = {
    "mc-fused-tanh": (MC, (-1.0, 1.0), True, False, (5.0, 0.0, 1.2, 2.0), True, None, 1),
    "mc-fused-relu": (MC, (-1.0, 1.0), False, False, (5.0, 0.0, 1.2, 2.0), True, None, 1),
    "mc-fused-tanh-stats": (MC, (-1.0, 1.0), True, True, (5.0, 0.0, 0.5, 1.0), True, None, 1),
    "mc-fused-relu-stats": (MC, (-1.0, 1.0), False, True, (5.0, 0.0, 0.5, 1.0), True, None, 1),
    "mc-bounds2": (MC, (-2.0, 2.0), (True, False, True, False), False, (5.0, 0.0, 0.5, 1.0), True, None, 2),
    "pendulum": (PEND, (-2.0, 2.0), (True, False, False, True), False, (5.0, 0.0, 0.5, 2.0), True, None, 2),
    "pendulum-stats": (PEND, (-2.0, 2.0), (False, True, True, False), True, (5.0, 0.0, 0.5, 2.0), True, None, 2),
    "mc-fused-generic-log": (MC, (-1.0, 1.0), True, False, (5.0, 0.0, 1.2, 2.0), True, 2, 1),
    "mc-fused-no-log-no-ring": (MC, (-1.0, 1.0), True, False, (5.0, 0.0, 1.2, 2.0), False, None, 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_many_rollout_is_bitwise_the_single_rollouts(ssc, case):
    """P = 4 pairs of n = (1, 70, 129, 257) envs -- one lane, a ragged last wave, the second workgroup of the two-lanes-per-env
    policies (129 > 128), the second workgroup of the one-lane policies (257 > 256), and pairs with fewer workgroups than
    grid x -- K = 7 twice, from step0 = 0 and 7: head and tail of the 4-step Philox pipeline in one call, the first tail
    meeting the second head.  max_episode_steps = 5: every env resets and writes ring records inside a call.  State columns,
    ou_x, every log column, statistics and rings against ssc_rollout_rms pair by pair on twin buffers."""
    ffi = ssc._ffi
    kind, bounds, llt, stats, clips, logged, scramble, lpe = CASES[case]
    pop = Pairs(ffi, kind, NS, 7, bounds, llt, stats, clips, log=logged, ring=logged, scramble=scramble, seed=len(case))
    ref, before = pop.clone(), pop.clone()
    shadow = pop.clone()                 # a logged single run: the reward column of a call that keeps no log
    for step0 in (0, 7):
        for x in (pop, ref, shadow):
            for t in x.T:
                t["stats"].zero_()
        ref.roll_single(step0)
        shadow.roll_single(step0, log=True)
        pop.roll_many(step0)
        O = pop.O
        pop.assert_equal(ref, [shadow.column(p, O + 1) for p in range(pop.P)], lpe)
        pop.assert_guards()
        ref.assert_guards()
    assert all(not torch.equal(pop.view(p, "s0"), before.view(p, "s0")) for p in range(pop.P))          # it rolled
    if logged:
        assert all(int(t["cursor"].item()) >= 2 * n for t, n in zip(pop.T, NS))                        # every env reset twice
        assert all(bool((pop.view(p, "cols") != SENT).all()) and bool((pop.view(p, "done") <= 1).all()) for p in range(pop.P))
        acts = [pop.column(p, pop.O) for p in range(pop.P)]
        assert all(float(a.abs().max()) <= max(bounds) and float(a.std()) > 0 for a in acts[1:])
    else:
        assert all(bool((pop.view(p, "cols") == SENT).all()) for p in range(pop.P))                    # no log was written
        assert all(int(t["cursor"].item()) == 0 for t in pop.T)


def test_many_pairs(ssc):
    """P = 300 pairs of 8 envs, K = 4: more grid rows than compute units, every workgroup a ragged single wave."""
    ffi = ssc._ffi
    pop = Pairs(ffi, MC, [8] * 300, 4, (-1.0, 1.0), True, False, (5.0, 0.0), seed=9)
    ref = pop.clone()
    ref.roll_single(2)
    pop.roll_many(2)
    pop.assert_equal(ref, [ref.column(p, 3) for p in range(300)], 1)
    pop.assert_guards()
    assert sum(int(t["cursor"].item()) for t in pop.T) >= 300 * 4


# ---- ssc_replay_append_many ------------------------------------------------------------------------------------------
def random_chunk(ssc, rng, obs_dim, K, n, step0):
    c = ssc.TransitionChunk(obs_dim, K, n, "cuda")
    f = lambda *shape: torch.as_tensor(rng.normal(size=shape).astype(np.float32), device="cuda")
    c.obs.copy_(f(obs_dim, K, n)); c.obs2.copy_(f(obs_dim, K, n)); c.act.copy_(f(K, n)); c.rew.copy_(f(K, n))
    c.done.copy_(torch.as_tensor((rng.random((K, n)) < 0.2).astype(np.uint8), device="cuda"))
    c.step0 = step0
    return c


def skipped_log(chunk, K):
    """the log of the last K steps of a chunk, as DeviceReplayBuffer.append_chunk passes it"""
    log, skip = chunk.as_struct(), chunk.K - K
    for c in range(chunk.obs_dim):
        log.obs[c], log.obs2[c] = chunk.obs[c][skip:].data_ptr(), chunk.obs2[c][skip:].data_ptr()
    log.act, log.rew, log.done = chunk.act[skip:].data_ptr(), chunk.rew[skip:].data_ptr(), chunk.done[skip:].data_ptr()
    return log


RING_ARRAYS = ("s", "a", "r", "t", "s2", "ep_steps", "ep_run")


@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("obs_dim", [2, 3])
def test_many_append_is_bitwise_the_single_appends(ssc, obs_dim, indexed):
    """P = 3 rings of capacity (100, 250, 1000) fed 7-step chunks of n = (24, 24, 10) envs, twice: the first ring takes more
    records per append than it holds and wraps, the second keeps only the last 4 steps (last_steps < K: advanced log
    pointers), the reward scales differ.  Rings -- and ep_steps / ep_run -- against ssc_replay_append ring by ring."""
    ffi = ssc._ffi
    lib = ffi.lib()
    caps, ns, Ks, scales = (100, 250, 1000), (24, 24, 10), (7, 4, 7), (1.0, 0.5, 3.0)
    rng = np.random.default_rng(31 + obs_dim)
    mk = lambda: [ssc.DeviceReplayBuffer(caps[p], obs_dim, seed=p, track_episodes=indexed, n_envs=ns[p]) for p in range(3)]
    got, want = mk(), mk()
    for rs in (got, want):
        for r in rs:
            for name in ("s", "a", "r", "s2"):
                getattr(r, name).fill_(SENT)
            r.t.fill_(SENT_B)
    counts = [0, 0, 0]
    for call in range(2):
        chunks = [random_chunk(ssc, rng, obs_dim, 7, ns[p], 7 * call) for p in range(3)]
        items, cursors = (ffi.ReplayAppendItem * 3)(), (ffi.PairCursor * 3)()
        for p, it in enumerate(items):
            log = skipped_log(chunks[p], Ks[p])
            ring_w = want[p].ring_struct()
            ffi.check(lib.ssc_replay_append(ctypes.byref(ring_w), ctypes.byref(log), Ks[p], ns[p], counts[p], scales[p], ffi.stream()))
            it.ring, it.log, it.K, it.n, it.reward_scale = got[p].ring_struct(), log, Ks[p], ns[p], scales[p]
            cursors[p].replay_start, cursors[p].step0 = counts[p], 1 << 40        # (step0 is the rollout's)
        d_items, d_cursors = device_copy(items), device_copy(cursors)
        ffi.check(lib.ssc_replay_append_many(ctypes.addressof(items), d_items.data_ptr(), ctypes.addressof(cursors), d_cursors.data_ptr(),
                                             3, ffi.stream()))
        torch.cuda.synchronize()
        counts = [c + k * n for c, k, n in zip(counts, Ks, ns)]
        for p in range(3):
            for name in RING_ARRAYS:
                x, y = getattr(got[p], name), getattr(want[p], name)
                assert (x is None and y is None) or torch.equal(x, y), (call, p, name)
    assert bool((got[0].s != SENT).all()) and bool((got[2].s == SENT).any())       # ring 0 wrapped, ring 2 is not full
    assert not indexed or int(got[1].ep_steps.max()) >= 2


# ---- ssc_decay_schedule_many -----------------------------------------------------------------------------------------
def test_many_decay_equals_the_single_decays(ssc):
    """P = 3 schedule sets with different factors and floors, one already at its floor, one with two schedules; two
    updates as the episode counters move."""
    ffi = ssc._ffi
    lib = ffi.lib()
    factors, floors, starts = ([0.9], [0.5, 0.99], [0.8]), ([0.1], [0.2, 0.05], [0.3]), ([1.0], [0.2, 1.0], [0.9])
    per_gen, f0 = (4.0, 8.0, 2.0), (0.0, 16.0, 3.0)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    finished = [f64([9.0]), f64([50.0]), f64([3.0])]
    mk = lambda: ([f64([0.0] + s) for s in starts], [[torch.full((1,), SENT, dtype=torch.float32, device="cuda") for _ in s] for s in starts])
    (st_g, out_g), (st_w, out_w) = mk(), mk()
    for call in range(2):
        items = (ffi.DecayItem * 3)()
        for p, it in enumerate(items):
            n = len(starts[p])
            fa, fl = (ctypes.c_double * n)(*factors[p]), (ctypes.c_double * n)(*floors[p])
            outs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in out_w[p]])
            ffi.check(lib.ssc_decay_schedule(ffi.ptr(finished[p]), f0[p], per_gen[p], n, fa, fl, ffi.ptr(st_w[p]), outs, ffi.stream()))
            it.d_finished, it.finished0, it.per_generation, it.n_sched, it.d_state = finished[p].data_ptr(), f0[p], per_gen[p], n, st_g[p].data_ptr()
            for i in range(n):
                it.factor[i], it.floor[i], it.d_out[i] = factors[p][i], floors[p][i], out_g[p][i].data_ptr()
        d_items = device_copy(items)
        ffi.check(lib.ssc_decay_schedule_many(ctypes.addressof(items), d_items.data_ptr(), 3, ffi.stream()))
        torch.cuda.synchronize()
        for p in range(3):
            assert torch.equal(st_g[p], st_w[p]), (call, p, st_g[p], st_w[p])
            assert all(torch.equal(a, b) for a, b in zip(out_g[p], out_w[p])), (call, p)
        for f in finished:
            f += 21.0
    assert st_g[0][0].item() == 7.0 and st_g[1][1].item() == 0.2 and 0.05 <= st_g[1][2].item() < 1.0 and st_g[2][1].item() == 0.3


# ---- ssc_obs_rms_update_many -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_dim", [2, 3])
def test_many_statistics_are_bitwise_the_single_updates(ssc, obs_dim):
    """Pairs of n = 64 and n = 1000 envs with K - k0 = 1 and 5 rows: four different (gx, gy) partitions in one launch,
    twice (the second update adds onto the first).  Blocks against ssc_obs_rms_update block by block."""
    ffi = ssc._ffi
    lib = ffi.lib()
    from smartstartcontinuous_amd.obs_rms import ObsRms
    shapes = ((64, 6, 5), (64, 6, 1), (1000, 6, 5), (1000, 6, 1))       # (n, K, k0)
    rng = np.random.default_rng(5 + obs_dim)
    got, want = [ObsRms(obs_dim) for _ in shapes], [ObsRms(obs_dim) for _ in shapes]
    for call in range(2):
        chunks = [random_chunk(ssc, rng, obs_dim, K, n, 0) for n, K, _ in shapes]
        items = (ffi.ObsRmsItem * 4)()
        for p, (it, (n, K, k0)) in enumerate(zip(items, shapes)):
            want[p].update_chunk(chunks[p], k0, K)
            it.log, it.k0, it.K, it.n = chunks[p].as_struct(), k0, K, n
            it.d_rms, it.d_workspace, it.workspace_bytes = got[p].block.data_ptr(), got[p]._ws.data_ptr(), got[p]._ws.numel()
        d_items = device_copy(items)
        ffi.check(lib.ssc_obs_rms_update_many(obs_dim, ctypes.addressof(items), d_items.data_ptr(), 4, ffi.stream()))
        torch.cuda.synchronize()
        for p in range(4):
            assert torch.equal(got[p].block, want[p].block), (call, p, got[p].block, want[p].block)
    assert abs(got[2].block[2 * obs_dim].item() - 2000.01) < 1e-6 and abs(got[1].block[2 * obs_dim].item() - 640.01) < 1e-6


# ---- the wrappers ----------------------------------------------------------------------------------------------------
def make_agent(ssc, p, env_id="MountainCarContinuous-v0", **kw):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    kw.setdefault("num_train_iterations", 2)
    return DDPG_Baselines_agent(ssc.make(env_id), None, batch_size=64, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32,
                                lastLayerTanh=True, seed=40 + p, actor_lr=1e-4 * (1 + p), critic_lr=1e-3 / (1 + p), gamma=0.99 - 0.01 * p,
                                tau=0.001 * (1 + p), **kw)


ENV_STATE = ("s0", "s1", "steps", "ep_ret", "ou_x")


def _wrapper_setup(ssc, env_ids, ns, normalize):
    envs = [ssc.VecEnv(env_ids[p], ns[p], seed=20 + p, max_episode_steps=6) for p in range(len(ns))]
    agents = [make_agent(ssc, p, env_ids[p], normalize_observations=normalize[p], reward_scale=0.5 + 0.25 * p) for p in range(len(ns))]
    pds = [e.policy_desc(a.as_policy(device_epsilon=True)) for e, a in zip(envs, agents)]
    chunks = [ssc.TransitionChunk(e.obs_dim, 5, e.n, "cuda") for e in envs]
    rings = [ssc.EpisodeRing(4 * e.n, "cuda") for e in envs]
    replays = [ssc.DeviceReplayBuffer(3 * 5 * e.n // 2, e.obs_dim, seed=p, track_episodes=True, n_envs=e.n) for p, e in enumerate(envs)]
    return envs, agents, pds, chunks, rings, replays


@pytest.mark.parametrize("what,fused", [("served", True), ("mixed-envs", False), ("mixed-statistics", False)])
def test_wrappers_leave_the_objects_as_the_per_object_calls_do(ssc, what, fused):
    """VecEnvPopulation.rollout + DeviceReplayPopulation.append_chunks over three chunks (the second and third reuse the
    descriptors; the ring wraps in the second; last_steps = 4 of 5) against env.rollout + replay.append_chunk: env.t,
    chunk.step0 / env_id0, replay.count, _next_step0, and every array.  A mixed-env or mixed-statistics population takes the
    per-pair calls (fused is False) with the same results."""
    ids = ["MountainCarContinuous-v0"] * 3
    if what == "mixed-envs":
        ids[1] = "Pendulum-v0"
    norm = [what == "mixed-statistics" and p == 2 for p in range(3)]
    ns = (64, 100, 257)
    (envs, agents, pds, chunks, rings, replays), (t_envs, t_agents, t_pds, t_chunks, t_rings, t_replays) = \
        (_wrapper_setup(ssc, ids, ns, norm) for _ in range(2))
    env_pop, replay_pop = ssc.VecEnvPopulation(envs), ssc.DeviceReplayPopulation(replays)
    scales = [a.reward_scale for a in agents]
    for call in range(3):
        outs = env_pop.rollout(5, pds, chunks, rings)
        replay_pop.append_chunks(outs, reward_scale=scales, last_steps=4)
        assert env_pop.fused is fused and replay_pop.fused is (what != "mixed-envs")
        for p in range(3):
            out = t_envs[p].rollout(5, out=t_chunks[p], ring=t_rings[p], policy_desc=t_pds[p])
            t_replays[p].append_chunk(out, reward_scale=scales[p], last_steps=4)
            assert outs[p] is chunks[p] and (envs[p].t, outs[p].step0, outs[p].env_id0) == (t_envs[p].t, out.step0, out.env_id0) == \
                (5 * (call + 1), 5 * call, 0)
            assert (replays[p].count, replays[p]._next_step0) == (t_replays[p].count, t_replays[p]._next_step0) == (4 * ns[p] * (call + 1), 5 * (call + 1))
            for name in ENV_STATE:
                assert torch.equal(getattr(envs[p], name), getattr(t_envs[p], name)), (call, p, name)
            for x, y in zip(outs[p].columns(), out.columns()):
                assert torch.equal(x, y), (call, p)
            assert torch.equal(envs[p].stats[1:], t_envs[p].stats[1:]) and torch.equal(rings[p].cursor, t_rings[p].cursor)
            for name in RING_ARRAYS:
                assert torch.equal(getattr(replays[p], name), getattr(t_replays[p], name)), (call, p, name)
    assert int(rings[0].cursor.item()) >= 2 * 64 and replays[0].count > replays[0].capacity


def test_grouped_decay_and_statistics_wrappers(ssc):
    """DecayScheduleGroup.update and ObsRmsGroup.update_chunks against the per-object updates, descriptors reused."""
    from smartstartcontinuous_amd.obs_rms import ObsRms, ObsRmsGroup
    from smartstartcontinuous_amd.rl_train import DecaySchedule, DecayScheduleGroup
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    counters = [f64([0.0, 0.0, 0.0, 10.0 * (p + 1)]) for p in range(3)]
    mk = lambda: [DecaySchedule("cuda", 2.0 + p, [(1.0, 0.9 - 0.1 * p, 0.3, torch.zeros(1, device="cuda"))]) for p in range(3)]
    got, want = mk(), mk()
    group = DecayScheduleGroup(got)
    rng = np.random.default_rng(77)
    blocks, t_blocks = [ObsRms(2) for _ in range(3)], [ObsRms(2) for _ in range(3)]
    rms_group = ObsRmsGroup(blocks)
    for call in range(3):
        group.update([c[3:4] for c in counters], [1.0, 2.0, 3.0])
        chunks = [random_chunk(ssc, rng, 2, 6, n, 0) for n in (64, 100, 1000)]
        rms_group.update_chunks(chunks, 2, 6)
        assert group.fused is True and rms_group.fused is True
        for p in range(3):
            want[p].update(counters[p][3:4], float(p + 1))
            t_blocks[p].update_chunk(chunks[p], 2, 6)
            assert torch.equal(got[p].state, want[p].state) and torch.equal(got[p].outs[0], want[p].outs[0]), (call, p)
            assert torch.equal(blocks[p].block, t_blocks[p].block), (call, p)
            counters[p][3] += 7.0
    assert got[0].read()[0] >= 10


# ---- the loop --------------------------------------------------------------------------------------------------------
AGENT_STATE = ("actor_flat", "critic_flat", "target_actor_flat", "target_critic_flat", "_adam_t")


def agent_tensors(a):
    return [getattr(a, k) for k in AGENT_STATE] + list(a._adam_actor) + list(a._adam_critic)


def _loop_pairs(ssc, env_id, normalize):
    envs = [ssc.VecEnv(env_id, n, seed=20 + p, max_episode_steps=20) for p, n in enumerate((64, 100, 257))]
    for e in envs:
        e.reset()
    agents = [make_agent(ssc, p, env_id, normalize_observations=normalize, reward_scale=0.5 + 0.25 * p, num_train_iterations=5) for p in range(3)]
    return envs, agents


@pytest.mark.parametrize("env_id,normalize", [("MountainCarContinuous-v0", False), ("MountainCarContinuous-v0", True), ("Pendulum-v0", False)])
def test_population_loop_on_the_many_launches_is_bitwise_the_single_loops(ssc, env_id, normalize, monkeypatch):
    """Pairs of 64, 100 and 257 envs, 4 chunks of 16 steps (the last 12 kept), 3 iterations per chunk: parameters, losses,
    Summary records, rings, statistics and the final epsilon equal three separate rl_train_vec_ddpg runs, and the fused
    rollout and append were taken in every chunk."""
    from smartstartcontinuous_amd import replay_buffer, vec_env
    ways = []
    for cls, name in ((vec_env.VecEnvPopulation, "rollout"), (replay_buffer.DeviceReplayPopulation, "append_chunks")):
        def spy(self, *a, _inner=getattr(cls, name), _name=name, **kw):
            out = _inner(self, *a, **kw)
            ways.append((_name, self.fused))
            return out
        monkeypatch.setattr(cls, name, spy)
    kw = dict(num_chunks=4, chunk_steps=16, train_iters=3, replay_capacity=4096, replay_last_steps=12)
    envs, agents = _loop_pairs(ssc, env_id, normalize)
    got = ssc.rl_train_vec_ddpg_population(envs, agents, seed=[3, 4, 5], **kw)
    assert ways == [("rollout", True), ("append_chunks", True)] * 4
    t_envs, twins = _loop_pairs(ssc, env_id, normalize)
    for p in range(3):
        summary, losses, replay = ssc.rl_train_vec_ddpg(t_envs[p], twins[p], seed=3 + p, **kw)
        g_summary, g_losses, g_replay = got[p]
        assert len(losses) == 4 and len(g_losses) == 4 and all(torch.equal(x, y) for x, y in zip(g_losses, losses))
        # (the slot order of the episode ring is an atomic's once an env set spans several waves: sorted records)
        assert sorted(g_summary.episodes) == sorted(summary.episodes) and len(summary.episodes) >= 3 * envs[p].n
        assert g_summary.dropped_episode_records == summary.dropped_episode_records == 0
        assert g_replay.count == replay.count == 4 * 12 * envs[p].n and g_replay._batches_drawn == replay._batches_drawn == 12
        for name in ("s", "a", "r", "t", "s2"):
            assert torch.equal(getattr(g_replay, name), getattr(replay, name)), (p, name)
        for name in ENV_STATE:
            assert torch.equal(getattr(envs[p], name), getattr(t_envs[p], name)), (p, name)
        assert envs[p].t == t_envs[p].t == 64 and torch.equal(envs[p].stats[1:], t_envs[p].stats[1:])
        assert agents[p].decaying_ou_action_noise.epsilon == twins[p].decaying_ou_action_noise.epsilon < 1.0
        if normalize:
            assert torch.equal(agents[p].obs_rms.block, twins[p].obs_rms.block)
        for k, (x, y) in enumerate(zip(agent_tensors(agents[p]), agent_tensors(twins[p]))):
            assert torch.equal(x, y), (p, k)
