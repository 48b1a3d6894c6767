#!/usr/bin/env python3
"""The smart-start selection of a SmartStart population, grouped against per pair, timed.

    python tools/exp_smartstart_population_selection.py refresh --out profiles/smartstart_population
    python tools/exp_smartstart_population_selection.py chunk   --out profiles/smartstart_population
    python tools/exp_smartstart_population_selection.py single  --out profiles/smartstart_population --parent-lib <libssc.so of the parent commit>

refresh ONE ``VecSmartStartPopulation.refresh_plans`` (``select_plans_many``) against P per-pair ``refresh_plans`` calls on the
        same rings and agents: P = 1, 2, 16, 64; rings of 4 096, 65 536 and 500 000 states; 64-32 and 200-100 agents;
        n_ss 1000; n_plans 1 and 8.  Wall clock around a whole refresh (it ends with the host holding its plans); the host
        geometry (``plan_from_path``) is timed inside both arms and reported beside the rest ("select" = everything else:
        launches, waits, copies).  Library calls and observable host waits are counted in one untimed refresh per arm.
chunk   one chunk of ``rl_train_vec_smartstart_population`` at 64 pairs x 16 envs with and without ``grouped_selection``,
        1x32 fp32 and 1x500 bf16 models.
single  ``ssc_kde_evaluate`` at 2000 x 100 000 and a single pair's ``refresh_plans`` of this build against the parent commit's
        library in the same process: "unchanged" = this build's median inside the parent's own window range; the outputs'
        bits are compared.
All three merge their section into <out>/selection.json.

Protocol (tools/exp_smartstart_population.py): one session, both arms in one process on the same objects, arms alternating
window by window after warm-up windows, median [min, max] of 7 windows; a case is WON only if the slowest grouped window
beats the fastest per-pair window.  The per-pair arm is the parent's path."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd import _ffi, navigator as nav  # noqa: E402
from smartstartcontinuous_amd import smartstart as SS  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent  # noqa: E402
from smartstartcontinuous_amd.replay_buffer import DeviceReplayBuffer  # noqa: E402

WINDOWS, WARMUP = 7, 2
ENV, N_ENVS, MAX_STEPS = "MountainCarContinuous-v0", 16, 200


def stat(v):
    return dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), windows_us=v)


def mlp(rng, dims):
    Ws = [(rng.normal(size=(dims[i], dims[i + 1])) * np.sqrt(2.0 / (dims[i] + dims[i + 1]))).astype(np.float32) for i in range(len(dims) - 1)]
    bs = [(rng.normal(size=dims[i + 1]) * 0.1).astype(np.float32) for i in range(len(dims) - 1)]
    return Ws, bs


def norm(rng, d=2):
    return dict(mean_x=rng.normal(size=d) * 0.3, std_x=rng.uniform(0.05, 1.0, d), mean_y=rng.normal(size=1) * 0.1,
                std_y=rng.uniform(0.3, 1.2, 1), mean_z=rng.normal(size=d) * 0.01, std_z=rng.uniform(0.005, 0.05, d))


def population(P, hidden, n_plans, model=((3, 32, 2), "f32"), training=False, seed=3):
    rng = np.random.default_rng(seed)
    env = ssc.VecEnv(ENV, P * N_ENVS, seed=seed, max_episode_steps=MAX_STEPS)
    env.reset()
    agents = [DDPG_Baselines_agent(ssc.make(ENV), None, batch_size=64, num_train_iterations=1, actor_h1=hidden[0], actor_h2=hidden[1],
                                   critic_h1=hidden[0], critic_h2=hidden[1], lastLayerTanh=True, seed=seed + p, training=training,
                                   precision="f32") for p in range(P)]
    models = []
    for p in range(P):
        Ws, bs = mlp(rng, model[0])
        models.append(nav.DynamicsModel(Ws, bs, norm(rng), state_dim=2, act_dim=1, precision=model[1]))
    pop = ssc.VecSmartStartPopulation(env, agents, models, [N_ENVS] * P, eta=0.5, n_ss=1000, n_plans=n_plans, num_control_samples=16,
                                      horizon=4, chunk_steps=64, seed=seed)
    return env, pop


def ring_arrays(states, seed=1):
    """a MountainCar-like ring of ``states`` records of N_ENVS envs: random-walk states, episodes of <= MAX_STEPS steps"""
    rng = np.random.default_rng(seed)
    n, K = N_ENVS, -(-states // N_ENVS)
    done = rng.random((K, n)) < 1.0 / 120.0
    done[MAX_STEPS - 1::MAX_STEPS] = True
    k = np.arange(K)[:, None]
    last = np.maximum.accumulate(np.where(done, k, -1), axis=0)
    last = np.concatenate([np.full((1, n), -1), last[:-1]])           # the last done BEFORE step k
    eps = (k - last).astype(np.int32).reshape(-1)[:states]
    pos = np.cumsum(rng.normal(0, 0.01, (K, n)), axis=0).reshape(-1)[:states] % 1.8 - 1.2
    vel = rng.normal(0, 0.02, states)
    s = np.stack([pos, vel], 1).astype(np.float32)
    s2 = (s + rng.normal(0, 0.005, s.shape)).astype(np.float32)
    return s, s2, eps


def make_rings(P, states, arrays):
    s, s2, eps = (torch.as_tensor(x, device="cuda") for x in arrays)
    rings = []
    for p in range(P):
        r = DeviceReplayBuffer(states, 2, 1, "cuda", seed=10 + p, track_episodes=True, n_envs=N_ENVS, max_path_len=MAX_STEPS + 1)
        r.s.copy_(s), r.s2.copy_(s2), r.ep_steps.copy_(eps)
        r.count = states
        rings.append(r)
    return rings


class Counter:
    """library calls (each is one launch or none) and the host waits python can see, inside a ``with`` block"""

    def __enter__(self):
        self.calls = self.waits = 0
        self._check, self._item, self._cpu, self._sync = _ffi.check, torch.Tensor.item, torch.Tensor.cpu, torch.cuda.Event.synchronize
        me = self

        def check(rc):
            me.calls += 1
            return me._check(rc)

        def wrap(f):
            def g(*a, **k):
                me.waits += 1
                return f(*a, **k)
            return g
        _ffi.check = check
        torch.Tensor.item, torch.Tensor.cpu, torch.cuda.Event.synchronize = wrap(self._item), wrap(self._cpu), wrap(self._sync)
        return self

    def __exit__(self, *exc):
        _ffi.check = self._check
        torch.Tensor.item, torch.Tensor.cpu, torch.cuda.Event.synchronize = self._item, self._cpu, self._sync


def refresh_case(P, states, hidden, n_plans, arrays):
    env, pop = population(P, hidden, n_plans)
    rings = make_rings(P, states, arrays)
    geometry = [0.0]
    for pr in pop.pairs:
        real = pr.plan_from_path

        def timed(path, real=real):
            t = time.perf_counter()
            out = real(path)
            geometry[0] += time.perf_counter() - t
            return out
        pr.plan_from_path = timed
    arms = dict(grouped=lambda: pop.refresh_plans(rings), per_pair=lambda: [pr.refresh_plans(r) for pr, r in zip(pop.pairs, rings)])
    old = SS.SMARTSTART_POPULATION_SELECTION_MIN_GROUP
    SS.SMARTSTART_POPULATION_SELECTION_MIN_GROUP = 1               # the grouped arm is the grouped path at every P
    try:
        total, select, geo, counts = {k: [] for k in arms}, {k: [] for k in arms}, {k: [] for k in arms}, {}
        for w in range(WARMUP + WINDOWS):
            for name, f in arms.items():
                torch.cuda.synchronize()
                geometry[0] = 0.0
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                if w >= WARMUP:
                    total[name].append(1e6 * dt)
                    geo[name].append(1e6 * geometry[0])
                    select[name].append(1e6 * (dt - geometry[0]))
        for name, f in arms.items():
            with Counter() as c:
                f()
            counts[name] = dict(library_calls=c.calls, visible_host_waits=c.waits)
    finally:
        SS.SMARTSTART_POPULATION_SELECTION_MIN_GROUP = old
    g, b = stat(select["grouped"]), stat(select["per_pair"])
    return dict(P=P, ring_states=states, agent="%d-%d" % hidden, n_plans=n_plans, n_ss=1000,
                grouped=dict(select=g, geometry=stat(geo["grouped"]), total=stat(total["grouped"]), **counts["grouped"]),
                per_pair=dict(select=b, geometry=stat(geo["per_pair"]), total=stat(total["per_pair"]), **counts["per_pair"]),
                won=g["max_us"] < b["min_us"], ratio=b["median_us"] / g["median_us"],
                won_total=max(total["grouped"]) < min(total["per_pair"]),
                ratio_total=statistics.median(total["per_pair"]) / statistics.median(total["grouped"]))


def merge(out, key, value):
    path = os.path.join(out, "selection.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    json.dump(doc, open(path, "w"), indent=1)


def run_refresh(out, sizes, Ps):
    cases = []
    for states in sizes:
        arrays = ring_arrays(states)
        for hidden in ((64, 32), (200, 100)):
            for n_plans in (1, 8):
                for P in Ps:
                    c = refresh_case(P, states, hidden, n_plans, arrays)
                    cases.append(c)
                    g, b = c["grouped"], c["per_pair"]
                    print("refresh ring %6d agent %-7s plans %d P %2d: select grouped %9.1f [%9.1f, %9.1f] us / per pair %9.1f [%9.1f, %9.1f] us"
                          "  x%.2f %s | geometry %8.1f / %8.1f us | calls %d / %d, waits %d / %d"
                          % (states, c["agent"], n_plans, P, g["select"]["median_us"], g["select"]["min_us"], g["select"]["max_us"],
                             b["select"]["median_us"], b["select"]["min_us"], b["select"]["max_us"], c["ratio"], "WON" if c["won"] else "not won",
                             g["geometry"]["median_us"], b["geometry"]["median_us"], g["library_calls"], b["library_calls"],
                             g["visible_host_waits"], b["visible_host_waits"]), flush=True)
                    torch.cuda.empty_cache()
    merge(out, "refresh", dict(method="wall clock around one whole refresh of all pairs, device idle before and after; arms alternating "
                               "window by window, %d windows per arm after %d warm-up windows; select = total - plan_from_path time; "
                               "won = slowest grouped window < fastest per-pair window; visible_host_waits counts .item(), .cpu() and "
                               "Event.synchronize() (the boolean-mask index of the per-pair path waits too and is not seen)"
                               % (WINDOWS, WARMUP), cases=cases))


def run_chunk(out, P=64, chunks=4):
    cases = []
    for model in (((3, 32, 2), "f32"), ((3, 500, 2), "bf16_mfma")):
        per = dict(grouped=[], per_pair=[])
        kw = dict(chunk_steps=64, train_iters=1, replay_capacity=1 << 16, seed=list(range(P)))
        runs = {}
        for name in per:
            env, pop = population(P, (64, 32), 1, model=model, training=True)
            runs[name] = (env, pop)
            ssc.rl_train_vec_smartstart_population(env, pop, 2, grouped_selection=name == "grouped", **kw)      # allocations, capture
        for w in range(WARMUP + WINDOWS):
            for name, (env, pop) in runs.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                ssc.rl_train_vec_smartstart_population(env, pop, chunks, grouped_selection=name == "grouped", **kw)
                torch.cuda.synchronize()
                if w >= WARMUP:
                    per[name].append(1e6 * (time.perf_counter() - t) / chunks)
        g, b = stat(per["grouped"]), stat(per["per_pair"])
        cases.append(dict(P=P, envs_per_pair=N_ENVS, chunk_steps=64, model="1x%d %s" % (model[0][1], model[1]), grouped=g, per_pair=b,
                          won=g["max_us"] < b["min_us"], ratio=b["median_us"] / g["median_us"]))
        print("chunk %s: grouped %9.1f [%9.1f, %9.1f] us / per pair %9.1f [%9.1f, %9.1f] us per chunk  x%.2f %s"
              % (cases[-1]["model"], g["median_us"], g["min_us"], g["max_us"], b["median_us"], b["min_us"], b["max_us"], cases[-1]["ratio"],
                 "WON" if cases[-1]["won"] else "not won"), flush=True)
    merge(out, "chunk", dict(method="wall clock per chunk of rl_train_vec_smartstart_population (%d chunks per window, fresh rings each "
                             "window: <= %d records), %d pairs x %d envs, refresh_every 1; %d windows per arm after %d warm-up windows"
                             % (chunks, chunks * 64 * N_ENVS, P, N_ENVS, WINDOWS, WARMUP), cases=cases))


def bind(path):
    h = ctypes.CDLL(path)
    for name, (res, args) in _ffi._SIGNATURES.items():
        fn = getattr(h, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return h


def run_single(out, parent_lib):
    new, old = _ffi.lib(), bind(parent_lib)
    rng = np.random.default_rng(4)
    n, m, d = 100000, 2000, 2
    data = torch.as_tensor(rng.normal(size=(n, d)).astype(np.float32), device="cuda")
    pts = torch.as_tensor(rng.normal(size=(m, d)).astype(np.float32), device="cuda")
    wh, nrm = SS.kde_scott_bandwidth(data)
    whc = (ctypes.c_float * (d * d))(*wh.reshape(-1).tolist())
    outs = {k: torch.zeros(m, dtype=torch.float32, device="cuda") for k in ("new", "old")}
    call = lambda L, k: (lambda: _ffi.check(L.ssc_kde_evaluate(d, n, _ffi.ptr(data), m, _ffi.ptr(pts), whc, nrm, _ffi.ptr(outs[k]), _ffi.stream())))
    per = dict(new=[], old=[])
    for w in range(WARMUP + WINDOWS):
        for k, L in (("new", new), ("old", old)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                call(L, k)()
            b.record()
            torch.cuda.synchronize()
            if w >= WARMUP:
                per[k].append(1000.0 * a.elapsed_time(b) / 20)
    a, b = stat(per["new"]), stat(per["old"])
    cases = [dict(call="ssc_kde_evaluate", n=n, m=m, this_build=a, parent=b, unchanged=b["min_us"] <= a["median_us"] <= b["max_us"],
                  same_bits=bool(torch.equal(outs["new"], outs["old"])))]
    print("single ssc_kde_evaluate %d x %d: this %.2f us, parent %.2f [%.2f, %.2f] us unchanged %s same bits %s"
          % (m, n, a["median_us"], b["median_us"], b["min_us"], b["max_us"], cases[0]["unchanged"], cases[0]["same_bits"]), flush=True)
    # a single pair's refresh_plans (the per-pair path: python unchanged, the library swapped under it)
    env, pop = population(1, (64, 32), 8)
    ring = make_rings(1, 65536, ring_arrays(65536))[0]
    pr, per, chosen = pop.pairs[0], dict(new=[], old=[]), {}
    for w in range(WARMUP + WINDOWS):
        for k, L in (("new", new), ("old", old)):
            _ffi._lib = ring.lib = pr.agent.lib = L
            ring._queries = 0
            pr.last_radii = None
            torch.cuda.synchronize()
            t = time.perf_counter()
            pr.refresh_plans(ring)
            torch.cuda.synchronize()
            if w >= WARMUP:
                per[k].append(1e6 * (time.perf_counter() - t))
            chosen[k] = pr.last_chosen.clone()
    _ffi._lib = ring.lib = pr.agent.lib = new
    a, b = stat(per["new"]), stat(per["old"])
    cases.append(dict(call="refresh_plans, one pair, ring 65536, n_ss 1000, n_plans 8", this_build=a, parent=b,
                      unchanged=b["min_us"] <= a["median_us"] <= b["max_us"], same_bits=bool(torch.equal(chosen["new"], chosen["old"]))))
    print("single refresh_plans: this %.1f us, parent %.1f [%.1f, %.1f] us unchanged %s same chosen %s"
          % (a["median_us"], b["median_us"], b["min_us"], b["max_us"], cases[1]["unchanged"], cases[1]["same_bits"]), flush=True)
    merge(out, "single", dict(method="this build's call against the parent commit's library in the same process, arms alternating window "
                              "by window, %d windows after %d warm-up; unchanged = this build's median inside the parent's [min, max]"
                              % (WINDOWS, WARMUP), cases=cases))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("refresh", "chunk", "single"))
    ap.add_argument("--out", default="profiles/smartstart_population")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sizes", default="4096,65536,500000")
    ap.add_argument("--pairs", default="1,2,16,64")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.what == "refresh":
        run_refresh(args.out, [int(x) for x in args.sizes.split(",")], [int(x) for x in args.pairs.split(",")])
    elif args.what == "chunk":
        run_chunk(args.out)
    else:
        run_single(args.out, args.parent_lib)
