#!/usr/bin/env python3
"""Measurement of the population parameter-noise launch.

    python tools/exp_ddpg_population_param_noise.py call --out DIR     # DDPGPopulation.param_noise_cycle, P in {1, 8, 64, 256}
    python tools/exp_ddpg_population_param_noise.py loop --out DIR     # the population loop with noisy agents, 64 pairs
    python tools/exp_ddpg_population_param_noise.py single --out DIR [--other-lib LIB]   # the single ssc_param_noise_cycle

call: P agents of the shipped shape (64-32, obs_dim 2, tanh layer 2) with parameter noise, batch 64, every ring holding 4096
records.  "many" is ``DDPGPopulation.param_noise_cycle`` as it is (one ssc_replay_sample_many and one
ssc_param_noise_cycle_many per call), "loop" the yardstick: the wrapper's own fallback, P per-agent
``adapt_and_perturb(cycle=True)`` calls (ssc_replay_sample, index_select, an index cast, ssc_param_noise_cycle each), switched by
``agents.POPULATION_FUSED_PARAM_NOISE``.  HIP events around back-to-back calls on one stream after warm-up, median of 7 runs,
the two ways alternating run by run in one process on twin populations; the run-to-run spread (max - min) / median of both
sides is written beside every ratio, and P = 1 is a row like any other.  Before anything is timed both ways run once from the
same state and every agent's acting copy, stddev and distance are compared bit for bit.

loop: the loop_fused protocol of tools/exp_ddpg_population.py -- 64 pairs x 1024 envs, 64-step chunks, 10 iterations, 8 chunks;
host clock between two synchronisations, 3 runs per variant alternating after a warm-up run of each -- with every agent noisy.

single: ssc_param_noise_cycle on a 64-32 actor at batch 64 and 1024, this build alternating run by run with another build of
the library (``--other-lib``: e.g. the parent commit's), the same protocol as `call`.
-> param_noise.json (each mode writes its own key and keeps the others')."""
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
from smartstartcontinuous_amd import _ffi, agents as agents_mod  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent, DDPGPopulation  # noqa: E402

ENV = "MountainCarContinuous-v0"
B, ITERS, RECORDS = 64, 10, 4096


def noisy_agents(P):
    return [DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=B, num_train_iterations=ITERS, actor_h1=64, actor_h2=32,
                                 critic_h1=64, critic_h2=32, lastLayerTanh=True, seed=7 + p, param_noise_stddev=0.05 + 0.001 * (p % 50))
            for p in range(P)]


def rings(P):
    out = []
    for p in range(P):
        r = ssc.DeviceReplayBuffer(RECORDS, 2, seed=30 + p)
        r.s.copy_(torch.as_tensor(np.random.default_rng(90 + p).uniform(-1.2, 0.6, (RECORDS, 2)).astype(np.float32)).cuda())
        r.count = RECORDS
        out.append(r)
    return out


def stat(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / statistics.median(v), runs=v)


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
    return stat(per[0]), stat(per[1])


def compare(many, loop):
    """the ratio and whether the difference of the medians exceeds both sides' run-to-run ranges"""
    gain = loop["median_ms"] - many["median_ms"]
    ranges = (many["max_ms"] - many["min_ms"]) + (loop["max_ms"] - loop["min_ms"])
    return dict(loop_over_many=loop["median_ms"] / many["median_ms"], gain_ms=gain, both_ranges_ms=ranges,
                many_faster_by_more_than_the_spreads=gain > ranges, many_slower_by_more_than_the_spreads=-gain > ranges)


def merge(out_dir, key, value):
    path = os.path.join(out_dir, "param_noise.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    doc["device"] = torch.cuda.get_device_name(0)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def call(out_dir):
    rows = []
    for P in (1, 8, 64, 256):
        sides = {}
        for name in ("many", "loop"):
            ag, rg = noisy_agents(P), rings(P)
            sides[name] = (DDPGPopulation(ag), ag, rg)

        def run(name):
            pop, _ag, rg = sides[name]
            agents_mod.POPULATION_FUSED_PARAM_NOISE = name == "many"
            try:
                pop.param_noise_cycle(rg)
            finally:
                agents_mod.POPULATION_FUSED_PARAM_NOISE = True
            assert pop.pn_fused is (name == "many")

        run("many"); run("loop")
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int32)
        same = all(torch.equal(bits(getattr(a, k)), bits(getattr(b, k))) for a, b in zip(sides["many"][1], sides["loop"][1])
                   for k in ("perturbed_actor_flat", "d_param_noise_stddev", "d_param_noise_distance"))
        many, loop = timed_pair(lambda: run("many"), lambda: run("loop"), max(4, 256 // P))
        row = dict(agents=P, bits_equal=bool(same), many=many, loop=loop, cycle=compare(many, loop))
        rows.append(row)
        print(json.dumps(dict(agents=P, bits_equal=bool(same), many_ms=many["median_ms"], loop_ms=loop["median_ms"], **row["cycle"])), flush=True)
    merge(out_dir, "call", dict(
        shape="64-32, obs_dim 2, tanh; batch %d out of rings of %d records" % (B, RECORDS),
        protocol="HIP events around back-to-back DDPGPopulation.param_noise_cycle calls on one stream after 3 warm-up calls of each way, "
                 "median of 7 runs, the two ways alternating run by run in one process on twin populations; spread = (max - min) / median "
                 "of a side's 7 runs; loop = the wrapper's fallback (agents.POPULATION_FUSED_PARAM_NOISE off): P per-agent "
                 "adapt_and_perturb(cycle=True) calls",
        rows=rows))
    return 0


def loop(out_dir):
    P, envs, steps, chunks = 64, 1024, 64, 8
    kw = dict(chunk_steps=steps, replay_capacity=1 << 18, ring_capacity=1 << 16, train_iters=ITERS)

    def run(fused):
        ag = noisy_agents(P)
        vec = [ssc.VecEnv(ENV, envs, seed=50 + p) for p in range(P)]
        for e in vec:
            e.reset()
        agents_mod.POPULATION_FUSED_PARAM_NOISE = fused
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ssc.rl_train_vec_ddpg_population(vec, ag, chunks, param_noise_cycle=True, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / chunks * 1e3
        finally:
            agents_mod.POPULATION_FUSED_PARAM_NOISE = True

    for fused in (True, False):
        run(fused)
    times = dict(fused=[], per_agent=[])
    for _ in range(3):
        times["fused"].append(run(True))
        times["per_agent"].append(run(False))
    st = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs=v)
    f, y = st(times["fused"]), st(times["per_agent"])
    row = dict(pairs=P, fused=f, per_agent=y, gain_ms=y["median_ms"] - f["median_ms"], both_spreads_ms=f["spread_ms"] + y["spread_ms"],
               per_agent_over_fused=y["median_ms"] / f["median_ms"])
    row["faster_by_more_than_the_spreads"] = row["gain_ms"] > row["both_spreads_ms"]
    row["not_slower_by_more_than_the_spreads"] = -row["gain_ms"] <= row["both_spreads_ms"]
    print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
    merge(out_dir, "loop", dict(
        shape=dict(pairs=P, envs_per_pair=envs, chunk_steps=steps, iters=ITERS, chunks=chunks, net="64-32", noisy="every agent"),
        note="ms per chunk of all pairs, the finishing drain and read-backs of a run included; host clock between two synchronisations; "
             "3 runs per variant alternating after a warm-up run of each; per_agent = agents.POPULATION_FUSED_PARAM_NOISE off",
        row=row))
    return 0


def single(out_dir, other_lib):
    """ssc_param_noise_cycle of this build against another build of the library, batch 64 and 1024"""
    here = _ffi.lib()
    libs = {"this": here}
    if other_lib:
        other = ctypes.CDLL(os.path.abspath(other_lib))
        other.ssc_param_noise_cycle.restype, other.ssc_param_noise_cycle.argtypes = _ffi._SIGNATURES["ssc_param_noise_cycle"]
        libs["other"] = other
    a = noisy_agents(1)[0]
    rows = []
    for m in (64, 1024):
        obs = torch.as_tensor(np.random.default_rng(m).uniform(-1.2, 0.6, (m, 2)).astype(np.float32)).cuda()
        out = {k: (torch.empty_like(a.actor_flat), torch.full((1,), 0.1, device="cuda"), torch.zeros(1, device="cuda")) for k in libs}

        def kernel_only(k):
            dst, sd, dist = out[k]
            _ffi.check(libs[k].ssc_param_noise_cycle(ctypes.byref(a._desc), m, _ffi.ptr(obs), None, a.actor_flat.numel(), _ffi.ptr(a.actor_flat),
                                                     *a._pn_skip, 11, 2, 3, 0.01, 1.01, _ffi.ptr(sd), _ffi.ptr(dist), _ffi.ptr(dst), _ffi.stream()))
        def run(k):                                              # from the same stddev: the outputs are comparable
            out[k][1].fill_(0.1)
            kernel_only(k)
        row = dict(batch=m)
        if "other" in libs:
            run("this"); run("other")
            torch.cuda.synchronize()
            row["bits_equal"] = bool(all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out["this"], out["other"])))
            this, other_t = timed_pair(lambda: kernel_only("this"), lambda: kernel_only("other"), 200)
            row.update(this=this, other=other_t, gain_ms=other_t["median_ms"] - this["median_ms"],
                       both_ranges_ms=(this["max_ms"] - this["min_ms"]) + (other_t["max_ms"] - other_t["min_ms"]))
            row["moved_by_more_than_the_spreads"] = abs(row["gain_ms"]) > row["both_ranges_ms"]
        else:
            this, _ = timed_pair(lambda: kernel_only("this"), lambda: None, 200)
            row.update(this=this)
        rows.append(row)
        print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
    merge(out_dir, "single", dict(
        shape="ssc_param_noise_cycle, 64-32 actor, obs_dim 2, no statistics",
        protocol="HIP events around 200 back-to-back calls on one stream after warm-up, median of 7 runs, this build and the other build of "
                 "the library alternating run by run in one process; ms per call (the calls are launch-bound at batch 64)",
        other="the parent commit's param_noise.hip built with the same flags" if other_lib else None, rows=rows))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["call", "loop", "single"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ddpg_population"))
    ap.add_argument("--other-lib", default=None, help="single: another build of libssc.so to alternate with")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: there is no fallback")
    os.makedirs(args.out, exist_ok=True)
    sys.exit(call(args.out) if args.what == "call" else loop(args.out) if args.what == "loop" else single(args.out, args.other_lib))
