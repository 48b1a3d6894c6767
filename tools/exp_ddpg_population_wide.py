#!/usr/bin/env python3
"""Measurements of the grouped multi-workgroup population learner.

    python tools/exp_ddpg_population_wide.py population --out DIR   # grouped launches against the per-agent calls
    python tools/exp_ddpg_population_wide.py single --label NAME [--tree DIR] --out DIR   # the single-agent learner alone
    python tools/exp_ddpg_population_wide.py merge --out DIR        # population.json + single_*.json -> wide.json

population: DDPGPopulation.train_from on mixed-shape populations, 10 iterations per agent per call on rings of 4096 records.
Two arms in one process on the SAME agents and rings: "grouped" (agents.POPULATION_GROUPED_WIDE = True) and "per_agent"
(False: agent.train_from agent by agent, the code path before the grouped launches existed).  Each arm has a population
object of its own, so both keep their descriptors between calls.  A window is `calls` back-to-back calls between two device
synchronisations on the host clock (the per-agent arm is bound by its host enqueue, so the host clock is the fair one);
after 2 warm-up windows per arm, 7 windows per arm alternating.  A case is WON when the slowest grouped window is faster
than the fastest per-agent window.  Cases: the reference's hidden_layer_size_experiment grid (actor x critic from 64-32,
128-64, 200-100, two learning rates each: P = 36), the same with five seeds (P = 180), 8 agents of 200-100 at batch 1024,
and P = 2.  The LDS bytes per workgroup of every agent's gradient pass are read from the plan.

single: us per iteration of ssc_ddpg_train_ws for 64-32 x 64, 64-32 x 1024 and 200-100 x 1024 (tools/exp_ddpg_wide.py's
measurement, 7 windows of 400 iterations after 2 warm-up windows), for comparing two trees in one session: `--tree DIR`
imports the package from DIR (a checkout of the parent commit with its library built) instead of this one."""
import argparse
import glob
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((64, 32), (128, 64), (200, 100))
ITERS, CAP, WINDOWS, WARMUP = 10, 4096, 7, 2


def stat(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / statistics.median(v), windows=v)


def make_agent(ssc, p, actor, critic, batch, actor_lr=1e-4, critic_lr=1e-3, seed=0):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    return DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0", seed=1), None, batch_size=batch, num_train_iterations=ITERS,
                                actor_h1=actor[0], actor_h2=actor[1], critic_h1=critic[0], critic_h2=critic[1], lastLayerTanh=True,
                                actor_lr=actor_lr, critic_lr=critic_lr, seed=7 + 1000 * seed + p)


def make_replay(ssc, p):
    import numpy as np
    import torch
    rng = np.random.default_rng(90 + p)
    r = ssc.DeviceReplayBuffer(CAP, 2, seed=7 + p)
    dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
    s = rng.uniform(-1.2, 0.6, (CAP, 2))
    r.s.copy_(dev(s, torch.float32)); r.s2.copy_(dev(s + 0.01 * rng.normal(size=s.shape), torch.float32))
    r.a.copy_(dev(rng.uniform(-1, 1, (CAP, 1)), torch.float32)); r.r.copy_(dev(0.5 * rng.normal(size=CAP), torch.float32))
    r.t.copy_(dev(rng.random(CAP) < 0.1, torch.uint8))
    r.count = CAP
    return r


def grid(ssc, seeds):
    """the reference's data/ddpg_baselines_summaries/hidden_layer_size_experiment grid"""
    cells = itertools.product(range(seeds), SHAPES, SHAPES, (1e-4, 1e-3), (1e-3, 1e-2))
    return [make_agent(ssc, p, a, c, 64, alr, clr, seed) for p, (seed, a, c, alr, clr) in enumerate(cells)]


CASES = (("reference_grid", lambda ssc: grid(ssc, 1)),
         ("reference_grid_with_seeds", lambda ssc: grid(ssc, 5)),
         ("wide_large_batch", lambda ssc: [make_agent(ssc, p, (200, 100), (200, 100), 1024) for p in range(8)]),
         ("small", lambda ssc: [make_agent(ssc, 0, (128, 64), (128, 64), 64), make_agent(ssc, 1, (200, 100), (200, 100), 64)]))


def plan_lds_bytes(ssc, pop):
    """per wide agent, the dynamic LDS of its gradient workgroups: the last word of its plan row (WideRowTail::lds_bytes)"""
    import torch
    g = next(g for g in pop._groups if g.way == "wide")
    lib, W = ssc._ffi.lib(), len(g.ps)
    row = int(lib.ssc_ddpg_train_many_wide_plan_bytes(2) - lib.ssc_ddpg_train_many_wide_plan_bytes(1)) - 16
    words = g.plan.host[:W * row].view(torch.int32).view(W, row // 4)
    return [int(x) for x in words[:, -1]]


def population(out_dir):
    import torch
    import smartstartcontinuous_amd as ssc
    from smartstartcontinuous_amd import agents as agents_mod
    rows = []
    for name, make in CASES:
        agents = make(ssc)
        P = len(agents)
        replays = [make_replay(ssc, p) for p in range(P)]
        pops = dict(grouped=agents_mod.DDPGPopulation(agents), per_agent=agents_mod.DDPGPopulation(agents))
        calls = max(3, 600 // P)

        def window(arm):
            agents_mod.POPULATION_GROUPED_WIDE = arm == "grouped"
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    pops[arm].train_from(replays, ITERS)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / calls * 1e3
            finally:
                agents_mod.POPULATION_GROUPED_WIDE = True
        for _ in range(WARMUP):
            for arm in pops:
                window(arm)
        ways = {arm: list(pops[arm].ways) for arm in pops}
        assert set(ways["per_agent"]) == {"alone"}, ways["per_agent"]
        times = {arm: [] for arm in pops}
        for _ in range(WINDOWS):
            for arm in pops:
                times[arm].append(window(arm))
        g, y = stat(times["grouped"]), stat(times["per_agent"])
        lds = plan_lds_bytes(ssc, pops["grouped"]) if "wide" in pops["grouped"].ways else []
        row = dict(case=name, agents=P, batch=agents[0].batch_size, iters=ITERS, calls_per_window=calls,
                   ways={w: ways["grouped"].count(w) for w in ("one_workgroup", "wide", "alone")}, grouped=g, per_agent=y,
                   per_agent_over_grouped=y["median_ms"] / g["median_ms"], won=g["max_ms"] < y["min_ms"],
                   us_per_agent_iteration_grouped=g["median_ms"] * 1e3 / (P * ITERS),
                   us_per_agent_iteration_per_agent=y["median_ms"] * 1e3 / (P * ITERS),
                   gradient_lds_bytes=dict(per_agent_min=min(lds), launch=max(lds)) if lds else None)
        rows.append(row)
        print(json.dumps({k: (v["median_ms"] if k in ("grouped", "per_agent") else v) for k, v in row.items()}), flush=True)
        del pops, agents, replays
        torch.cuda.empty_cache()
    result = dict(note="ms per DDPGPopulation.train_from call of all agents (index draw included), host clock between two device "
                       "synchronisations; %d windows per arm alternating after %d warm-up windows; rings of %d" % (WINDOWS, WARMUP, CAP),
                  device=torch.cuda.get_device_name(0), rows=rows)
    with open(os.path.join(out_dir, "population.json"), "w") as f:
        json.dump(result, f, indent=1)
    return 0


def single(out_dir, label):
    import numpy as np
    import torch
    import smartstartcontinuous_amd as ssc
    os.environ.pop("SSC_DDPG_WIDE", None)
    os.environ.pop("SSC_DDPG_INTERPRETER", None)
    n_it, cap, rows = 400, 100000, []
    for (h1, h2), B in (((64, 32), 64), ((64, 32), 1024), ((200, 100), 1024)):
        rng = np.random.default_rng(0)
        agent = make_agent(ssc, 0, (h1, h2), (h1, h2), B)
        dev = lambda x, dt: torch.as_tensor(x, dtype=dt, device="cuda").contiguous()
        s, a = dev(rng.uniform(-1.2, 0.6, (cap, 2)), torch.float32), dev(rng.uniform(-1, 1, (cap, 1)), torch.float32)
        r, t = dev(rng.normal(size=cap), torch.float32), dev(rng.random(cap) < 0.01, torch.uint8)
        idx = torch.randint(0, cap, (n_it, B), dtype=torch.int32, device="cuda")
        us = []
        for w in range(WARMUP + WINDOWS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); agent.train_on(s, a, r, t, s, idx, n_it); e1.record()
            torch.cuda.synchronize()
            if w >= WARMUP:
                us.append(e0.elapsed_time(e1) / n_it * 1e3)
        row = dict(actor_critic="%d-%d" % (h1, h2), batch=B, median_us=statistics.median(us), min_us=min(us), max_us=max(us), windows=us)
        rows.append(row)
        print(json.dumps(dict(label=label, **{k: v for k, v in row.items() if k != "windows"})), flush=True)
    n = len(glob.glob(os.path.join(out_dir, "single_%s_*.json" % label)))
    with open(os.path.join(out_dir, "single_%s_%d.json" % (label, n)), "w") as f:
        json.dump(dict(label=label, tree=os.path.dirname(os.path.dirname(os.path.abspath(ssc.__file__))), rows=rows), f, indent=1)
    return 0


def merge(out_dir):
    """population.json and every single_<label>_<n>.json of the session -> wide.json; the single-agent learner is unchanged
    when this tree's median lies inside the parent's own window-to-window range (all its runs pooled)"""
    with open(os.path.join(out_dir, "population.json")) as f:
        result = json.load(f)
    runs = {}
    for path in sorted(glob.glob(os.path.join(out_dir, "single_*_*.json"))):
        with open(path) as f:
            one = json.load(f)
        runs.setdefault(one["label"], []).append(one["rows"])
    if runs:
        check = []
        for k, first in enumerate(next(iter(runs.values()))[0]):
            entry = dict(actor_critic=first["actor_critic"], batch=first["batch"])
            for label, sessions in runs.items():
                pooled = [u for rows in sessions for u in rows[k]["windows"]]
                entry[label] = dict(median_us=statistics.median(pooled), min_us=min(pooled), max_us=max(pooled), runs=[rows[k]["windows"] for rows in sessions])
            if "parent" in entry and "head" in entry:
                entry["head_within_parents_range"] = entry["parent"]["min_us"] <= entry["head"]["median_us"] <= entry["parent"]["max_us"]
                entry["head_not_slower_than_parents_range"] = entry["head"]["median_us"] <= entry["parent"]["max_us"]
                entry["head_over_parent"] = entry["head"]["median_us"] / entry["parent"]["median_us"]
            check.append(entry)
        result["single_agent"] = dict(note="us per iteration of ssc_ddpg_train_ws, device events around 400 iterations per window, %d windows per "
                                           "run after %d warm-up windows; parent commit and this tree alternating in one session" % (WINDOWS, WARMUP),
                                      rows=check)
    with open(os.path.join(out_dir, "wide.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result.get("single_agent", {}).get("rows", []))[:2000], flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["population", "single", "merge"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg_population"))
    ap.add_argument("--label", default="head")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    os.makedirs(args.out, exist_ok=True)
    sys.exit(population(args.out) if args.what == "population" else single(args.out, args.label) if args.what == "single" else merge(args.out))
