#!/usr/bin/env python3
"""Measurements of the population learner.

    python tools/exp_ddpg_population.py launch --out DIR   # one ssc_ddpg_train_many against P x ssc_ddpg_train; the samplers
    python tools/exp_ddpg_population.py loop --out DIR     # rl_train_vec_ddpg_population against P sequential rl_train_vec_ddpg
    python tools/exp_ddpg_population.py loop_fused --out DIR   # the population loop on the many-launches against its per-pair form
    python tools/exp_ddpg_population.py probe --agents P   # a few launches of each kind, for a profiler run of its own

launch: P in {1, 8, 64, 256, 512} agents of the shipped shape (64-32, obs_dim 2, tanh layer 2, batch 64), 10 iterations per
agent per call on rings of 4096 records.  HIP events around back-to-back calls on one stream after warm-up, median of 7
runs, the two ways alternating run by run in one process.  "loop" is the parent's way: P launches of the single-agent
kernel, one after the other.  The samplers (10 batches of 64 per ring) the same way.  At P = 1 the comparison is the cost
of the item fetch; the run-to-run spread of both sides is written beside it.
loop: P = 64 pairs of 1024 envs, 64-step chunks, 10 iterations per chunk; host clock around 8 chunks between two device
synchronisations, 3 runs per variant alternating after a warm-up run of each; "rollout_only" is the population loop with no
iterations (rollouts, epsilon decay, appends), i.e. the part one launch per pair still serialises.
loop_fused: the same protocol at P in {1, 8, 64}: "fused" is the loop as it is (one rollout, decay and append launch per
chunk for all pairs), "per_pair" the yardstick -- the same loop with rl_train.POPULATION_FUSED_CHUNK off, i.e. the
per-pair calls pair by pair as before those launches existed; both train in the one learner launch.  Medians and
(max - min) / median spreads per variant -> loop_fused.json."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd import _ffi  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent  # noqa: E402

ENV = "MountainCarContinuous-v0"
B, ITERS, CAP = 64, 10, 4096
NA, NC = 2 * 64 + 64 + 64 * 32 + 32 + 32 + 1, 2 * 64 + 64 + 65 * 32 + 32 + 32 + 1
ROW = 2560                 # floats between two agents' copies of an array (16-byte aligned rows)


class RawPopulation:
    """P agents as rows of 2-d device tensors, their descriptors, and the device copy of the launch items"""

    def __init__(self, P, seed=0):
        rng = np.random.default_rng(seed)
        dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
        self.P = P
        self.arr = {k: dev(rng.uniform(-0.3, 0.3, (P, ROW))) for k in ("actor", "critic", "target_actor", "target_critic")}
        self.arr.update({k: torch.zeros((P, ROW), device="cuda") for k in ("adam_m_actor", "adam_v_actor", "adam_m_critic", "adam_v_critic")})
        self.adam_t = torch.zeros((P, 4), dtype=torch.int32, device="cuda")
        s = rng.uniform(-1.2, 0.6, (P, CAP, 2))
        self.s, self.s2 = dev(s), dev(s + 0.01 * rng.normal(size=s.shape))
        self.a, self.r = dev(rng.uniform(-1, 1, (P, CAP, 1))), dev(0.5 * rng.normal(size=(P, CAP)))
        self.t = dev(rng.random((P, CAP)) < 0.1, torch.uint8)
        self.idx = torch.zeros((P, ITERS, B), dtype=torch.int32, device="cuda")
        self.losses = torch.zeros((P, ITERS, 2), device="cuda")
        self.items = (_ffi.DdpgManyItem * P)()
        self.descs, self.views = [], []
        for p, it in enumerate(self.items):
            d = _ffi.DdpgDesc()
            d.obs_dim, d.act_dim, d.actor_h1, d.actor_h2, d.critic_h1, d.critic_h2, d.last_layer_tanh, d.batch_size = 2, 1, 64, 32, 64, 32, 1, B
            for k, t in self.arr.items():
                setattr(d, k, t[p].data_ptr())
            d.adam_t = self.adam_t[p].data_ptr()
            d.gamma, d.tau, d.actor_lr, d.critic_lr = 0.99, 0.001, 1e-4, 1e-3
            d.beta1, d.beta2, d.epsilon, d.obs_clip = 0.9, 0.999, 1e-8, 5.0
            rv = _ffi.ReplayView(self.s[p].data_ptr(), self.a[p].data_ptr(), self.r[p].data_ptr(), self.t[p].data_ptr(),
                                 self.s2[p].data_ptr(), CAP)
            it.ddpg, it.replay, it.d_batch_idx, it.d_losses, it.n_iters = d, rv, self.idx[p].data_ptr(), self.losses[p].data_ptr(), ITERS
            self.descs.append(d)
            self.views.append(rv)
        self.d_items = torch.frombuffer(bytearray(self.items), dtype=torch.uint8).cuda()
        self.keys = (_ffi.ReplaySampleKey * P)()
        for p, k in enumerate(self.keys):
            k.seed, k.counter0, k.size = 100 + p, 0, CAP
        self.d_keys = torch.frombuffer(bytearray(self.keys), dtype=torch.uint8).cuda()
        self.sample_many()
        torch.cuda.synchronize()

    def train_many(self):
        _ffi.check(_ffi.lib().ssc_ddpg_train_many(ctypes.addressof(self.items), self.d_items.data_ptr(), self.P, _ffi.stream()))

    def train_loop(self):
        lib, st = _ffi.lib(), _ffi.stream()
        for p in range(self.P):
            _ffi.check(lib.ssc_ddpg_train(ctypes.byref(self.descs[p]), ctypes.byref(self.views[p]), self.idx[p].data_ptr(), ITERS,
                                          self.losses[p].data_ptr(), st))

    def sample_many(self):
        _ffi.check(_ffi.lib().ssc_replay_sample_many(ctypes.addressof(self.keys), self.d_keys.data_ptr(), self.P, ITERS, B,
                                                     self.idx.data_ptr(), _ffi.stream()))

    def sample_loop(self):
        lib, st = _ffi.lib(), _ffi.stream()
        for p, k in enumerate(self.keys):
            _ffi.check(lib.ssc_replay_sample(k.seed, k.counter0, k.size, ITERS, B, self.idx[p].data_ptr(), st))


def timed_pair(fa, fb, calls, warmup=3, runs=7):
    """per-call ms of ``calls`` back-to-back calls of fa and of fb, alternating run by run"""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    per = ([], [])
    for _ in range(runs):
        for f, out in ((fa, per[0]), (fb, per[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / calls)
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / statistics.median(v),
                          runs=v)
    return stat(per[0]), stat(per[1])


def launch(out_dir):
    rows = []
    for P in (1, 8, 64, 256, 512):
        pop = RawPopulation(P, seed=P)
        calls = max(2, 256 // P)
        many, loop = timed_pair(pop.train_many, pop.train_loop, calls)
        s_many, s_loop = timed_pair(pop.sample_many, pop.sample_loop, calls)
        row = dict(agents=P, iters=ITERS, calls_per_run=calls, train_many=many, train_loop=loop,
                   train_ratio=loop["median_ms"] / many["median_ms"],
                   us_per_agent_iteration_many=many["median_ms"] * 1e3 / (P * ITERS),
                   us_per_agent_iteration_loop=loop["median_ms"] * 1e3 / (P * ITERS),
                   sample_many=s_many, sample_loop=s_loop, sample_ratio=s_loop["median_ms"] / s_many["median_ms"])
        rows.append(row)
        print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
    one = rows[0]
    fetch = dict(many_median_ms=one["train_many"]["median_ms"], single_median_ms=one["train_loop"]["median_ms"],
                 difference_ms=one["train_many"]["median_ms"] - one["train_loop"]["median_ms"],
                 many_spread=one["train_many"]["spread"], single_spread=one["train_loop"]["spread"])
    fetch["within_spread"] = abs(fetch["difference_ms"]) <= max(fetch["many_spread"], fetch["single_spread"]) * fetch["single_median_ms"]
    result = dict(shape="64-32, obs_dim 2, tanh, batch 64, %d iterations per agent per call, rings of %d" % (ITERS, CAP),
                  device=torch.cuda.get_device_name(0), rows=rows, item_fetch_at_one_agent=fetch)
    with open(os.path.join(out_dir, "launch.json"), "w") as f:
        json.dump(result, f, indent=1)
    print("item fetch:", json.dumps(fetch), flush=True)
    return 0


def make_pairs(P, envs):
    agents = [DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=B, num_train_iterations=ITERS, actor_h1=64, actor_h2=32,
                                   critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=7 + p) for p in range(P)]
    vec = [ssc.VecEnv(ENV, envs, seed=50 + p) for p in range(P)]
    for e in vec:
        e.reset()
    return vec, agents


def loop(out_dir):
    P, envs, steps, chunks = 64, 1024, 64, 8
    kw = dict(chunk_steps=steps, replay_capacity=1 << 18, ring_capacity=1 << 16)

    def run(variant):
        vec, agents = make_pairs(P, envs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant == "sequential":
            for e, a in zip(vec, agents):
                ssc.rl_train_vec_ddpg(e, a, chunks, train_iters=ITERS, **kw)
        else:
            ssc.rl_train_vec_ddpg_population(vec, agents, chunks, train_iters=ITERS if variant == "population" else 0, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / chunks * 1e3

    variants = ("population", "sequential", "rollout_only")
    for v in variants:
        run(v)
    times = {v: [] for v in variants}
    for _ in range(3):
        for v in variants:
            times[v].append(run(v))
    med = {v: statistics.median(t) for v, t in times.items()}
    result = dict(shape=dict(pairs=P, envs_per_pair=envs, chunk_steps=steps, iters=ITERS, chunks=chunks, net="64-32"),
                  note="ms per chunk of all pairs, the finishing drain and read-backs of a run included; host clock between two synchronisations",
                  chunk_ms=times, median_ms=med, sequential_over_population=med["sequential"] / med["population"],
                  rollout_share_of_population_chunk=med["rollout_only"] / med["population"])
    with open(os.path.join(out_dir, "loop.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "chunk_ms"}), flush=True)
    return 0


def loop_fused(out_dir):
    from smartstartcontinuous_amd import rl_train
    envs, steps, chunks = 1024, 64, 8
    kw = dict(chunk_steps=steps, replay_capacity=1 << 18, ring_capacity=1 << 16, train_iters=ITERS)

    def run(P, fused):
        vec, agents = make_pairs(P, envs)
        rl_train.POPULATION_FUSED_CHUNK = fused
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ssc.rl_train_vec_ddpg_population(vec, agents, chunks, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / chunks * 1e3
        finally:
            rl_train.POPULATION_FUSED_CHUNK = True

    rows = []
    for P in (1, 8, 64):
        for fused in (True, False):
            run(P, fused)
        times = dict(fused=[], per_pair=[])
        for _ in range(3):
            times["fused"].append(run(P, True))
            times["per_pair"].append(run(P, False))
        stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs=v)
        f, y = stat(times["fused"]), stat(times["per_pair"])
        row = dict(pairs=P, fused=f, per_pair=y, gain_ms=y["median_ms"] - f["median_ms"], both_spreads_ms=f["spread_ms"] + y["spread_ms"],
                   per_pair_over_fused=y["median_ms"] / f["median_ms"])
        row["faster_by_more_than_the_spreads"] = row["gain_ms"] > row["both_spreads_ms"]
        row["not_slower_by_more_than_the_spreads"] = -row["gain_ms"] <= row["both_spreads_ms"]
        rows.append(row)
        print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
    result = dict(shape=dict(envs_per_pair=envs, chunk_steps=steps, iters=ITERS, chunks=chunks, net="64-32"), device=torch.cuda.get_device_name(0),
                  note="ms per chunk of all pairs, the finishing drain and read-backs of a run included; host clock between two "
                       "synchronisations; 3 runs per variant alternating after a warm-up run of each",
                  rows=rows)
    with open(os.path.join(out_dir, "loop_fused.json"), "w") as f:
        json.dump(result, f, indent=1)
    return 0


def probe(P):
    """the many-launch at P agents and at one agent, and the single-agent launch, a few times each (told apart in a trace by
    kernel name and grid size)"""
    big, one = RawPopulation(P, seed=P), RawPopulation(1, seed=1)
    for _ in range(6):
        big.train_many()
        torch.cuda.synchronize()
        one.train_many()
        torch.cuda.synchronize()
        one.train_loop()
        torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launch", "loop", "loop_fused", "probe"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ddpg_population"))
    ap.add_argument("--agents", type=int, default=256)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    sys.exit(launch(args.out) if args.what == "launch" else loop(args.out) if args.what == "loop" else
             loop_fused(args.out) if args.what == "loop_fused" else probe(args.agents))
