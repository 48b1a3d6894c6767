#!/usr/bin/env python3
"""Measurements of the grouped launches of Pop-Art agents.

    python tools/exp_ddpg_population_popart.py population --out DIR   # grouped launches against the per-agent calls
    python tools/exp_ddpg_population_popart.py single --label NAME [--tree DIR] --out DIR   # the single-agent Pop-Art learner alone
    python tools/exp_ddpg_population_popart.py merge --out DIR        # popart_population.json + popart_single_*.json -> popart.json

population: DDPGPopulation.train_from on populations of Pop-Art agents (normalize_returns + enable_popart), 10 iterations
per agent per call on rings of 4096 records, measured as tools/exp_ddpg_population_wide.py measures the plain agents: two
arms in one process on the SAME agents and rings, "grouped" (ssc_ddpg_train_many_popart; POPULATION_POPART_MIN_GROUP held
at 2 for the measurement, whatever the shipped value) and "per_agent" (POPULATION_GROUPED_WIDE = False: agent.train_from
agent by agent, four or five launches per agent and iteration).  A window is `calls` back-to-back calls between two device
synchronisations on the host clock; after 2 warm-up windows per arm, 7 windows per arm alternating.  A case is WON when the
slowest grouped window is faster than the fastest per-agent window.  Cases: the reference's hidden_layer_size_experiment
grid as Pop-Art agents (P = 36 at batch 64), the same with five seeds (P = 180), 8 agents of 200-100 at batch 1024, and
groups of 2, 3, 4 and 8 agents of 64-32 at batch 64 -- the smallest winning size is POPULATION_POPART_MIN_GROUP.

single: us per iteration of ssc_ddpg_train_ws_popart for 64-32 x 64, 64-32 x 1024 and 200-100 x 1024 (the shapes of
profiles/ddpg_popart/iter.json; 7 windows of 400 iterations after 2 warm-up windows), for comparing two trees in one
session: `--tree DIR` imports the package from DIR (a checkout of the parent commit with its library built)."""
import argparse
import glob
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_ddpg_population_wide import CAP, ITERS, SHAPES, WARMUP, WINDOWS, make_replay, stat  # noqa: E402


def make_agent(ssc, p, actor, critic, batch, actor_lr=1e-4, critic_lr=1e-3, seed=0):
    from smartstartcontinuous_amd.agents import DDPG_Baselines_agent
    return DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0", seed=1), None, batch_size=batch, num_train_iterations=ITERS,
                                actor_h1=actor[0], actor_h2=actor[1], critic_h1=critic[0], critic_h2=critic[1], lastLayerTanh=True,
                                actor_lr=actor_lr, critic_lr=critic_lr, seed=7 + 1000 * seed + p, normalize_returns=True, enable_popart=True)


def grid(ssc, seeds):
    """the reference's data/ddpg_baselines_summaries/hidden_layer_size_experiment grid"""
    cells = itertools.product(range(seeds), SHAPES, SHAPES, (1e-4, 1e-3), (1e-3, 1e-2))
    return [make_agent(ssc, p, a, c, 64, alr, clr, seed) for p, (seed, a, c, alr, clr) in enumerate(cells)]


def shipped(n):
    return lambda ssc: [make_agent(ssc, p, (64, 32), (64, 32), 64) for p in range(n)]


CASES = (("reference_grid", lambda ssc: grid(ssc, 1)),
         ("reference_grid_with_seeds", lambda ssc: grid(ssc, 5)),
         ("wide_large_batch", lambda ssc: [make_agent(ssc, p, (200, 100), (200, 100), 1024) for p in range(8)]),
         ("group_of_2", shipped(2)), ("group_of_3", shipped(3)), ("group_of_4", shipped(4)), ("group_of_8", shipped(8)))


def population(out_dir):
    import torch
    import smartstartcontinuous_amd as ssc
    from smartstartcontinuous_amd import agents as agents_mod
    agents_mod.POPULATION_POPART_MIN_GROUP = 2
    rows = []
    for name, make in CASES:
        agents = make(ssc)
        P = len(agents)
        replays = [make_replay(ssc, p) for p in range(P)]
        pops = dict(grouped=agents_mod.DDPGPopulation(agents), per_agent=agents_mod.DDPGPopulation(agents))
        calls = max(3, 1200 // P)

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
        assert set(ways["per_agent"]) == {"alone"} and set(ways["grouped"]) == {"wide_popart"}, ways
        times = {arm: [] for arm in pops}
        for _ in range(WINDOWS):
            for arm in pops:
                times[arm].append(window(arm))
        g, y = stat(times["grouped"]), stat(times["per_agent"])
        finite = all(bool(torch.isfinite(a.ret_rms.block).all()) and bool(torch.isfinite(a.critic_flat).all()) for a in agents)
        row = dict(case=name, agents=P, batch=agents[0].batch_size, iters=ITERS, calls_per_window=calls, grouped=g, per_agent=y,
                   per_agent_over_grouped=y["median_ms"] / g["median_ms"], won=g["max_ms"] < y["min_ms"],
                   us_per_agent_iteration_grouped=g["median_ms"] * 1e3 / (P * ITERS),
                   us_per_agent_iteration_per_agent=y["median_ms"] * 1e3 / (P * ITERS), all_finite=finite)
        rows.append(row)
        print(json.dumps({k: (v["median_ms"] if k in ("grouped", "per_agent") else v) for k, v in row.items()}), flush=True)
        del pops, agents, replays
        torch.cuda.empty_cache()
    sizes = sorted(r["agents"] for r in rows if r["case"].startswith("group_of_") and r["won"])
    result = dict(note="ms per DDPGPopulation.train_from call of all agents (index draw included), host clock between two device "
                       "synchronisations; %d windows per arm alternating after %d warm-up windows; rings of %d" % (WINDOWS, WARMUP, CAP),
                  device=torch.cuda.get_device_name(0), rows=rows, smallest_winning_group=sizes[0] if sizes else None)
    with open(os.path.join(out_dir, "popart_population.json"), "w") as f:
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
    n = len(glob.glob(os.path.join(out_dir, "popart_single_%s_*.json" % label)))
    with open(os.path.join(out_dir, "popart_single_%s_%d.json" % (label, n)), "w") as f:
        json.dump(dict(label=label, rows=rows), f, indent=1)
    return 0


def merge(out_dir):
    """popart_population.json and every popart_single_<label>_<n>.json of the session -> popart.json; the single-agent
    learner costs what it cost when this tree's median lies inside the parent's own window-to-window range (its runs pooled)"""
    with open(os.path.join(out_dir, "popart_population.json")) as f:
        result = json.load(f)
    runs = {}
    for path in sorted(glob.glob(os.path.join(out_dir, "popart_single_*_*.json"))):
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
        result["single_agent"] = dict(note="us per iteration of ssc_ddpg_train_ws_popart, device events around 400 iterations per window, %d "
                                           "windows per run after %d warm-up windows; parent commit and this tree alternating in one session"
                                           % (WINDOWS, WARMUP), rows=check)
    with open(os.path.join(out_dir, "popart.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result.get("single_agent", {}).get("rows", []))[:3000], flush=True)
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
