#!/usr/bin/env python3
"""A population of SmartStart pairs in one captured step, timed.

    python tools/exp_smartstart_population.py step   --out profiles/smartstart_population
    python tools/exp_smartstart_population.py actor  --out profiles/smartstart_population
    python tools/exp_smartstart_population.py single --out profiles/smartstart_population --parent-lib <libssc.so of the parent commit>

step   graph replay per env step: ONE VecSmartStartPopulation graph against P per-pair VecSmartStart graphs replayed back to
       back, on the same agents, models and plans; P = 1, 2, 4, 16, 64 pairs x 16 and x 1024 envs, 16 candidates, 1x32 fp32 and
       1x500 bf16 MFMA models  -> step.json
actor  ssc_actor_forward_many against P ssc_actor_forward calls on the slices, per kernel class  -> actor.json
single ssc_smartstart_rollout_step and ssc_actor_forward of this build against another build of the library loaded into
       the same process (the parent commit's): "unchanged" = the new median lies inside the parent's own window-to-window
       range  -> single.json

Protocol (tools/exp_nav_population.py, NOTEBOOK section 24): one session, both arms in one process on the same objects,
device events around a window of back-to-back calls, arms alternating window by window after warm-up windows, median
[min, max] in microseconds; a case is WON only if the slowest window of the first arm beats the fastest of the second."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd import _ffi, navigator as nav  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent  # noqa: E402
from smartstartcontinuous_amd.population import DeviceItems  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 7, 2
ENV = "MountainCarContinuous-v0"


def timed_pair(fa, fb, calls=CALLS, warmup=WARMUP, windows=WINDOWS):
    """us per call of ``calls`` back-to-back calls of fa and of fb, alternating window by window after warm-up windows"""
    per = ([], [])
    for w in range(warmup + windows):
        for f, out in ((fa, per[0]), (fb, per[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            torch.cuda.synchronize()
            if w >= warmup:
                out.append(1000.0 * a.elapsed_time(b) / calls)
    stat = lambda v: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), windows_us=v)
    return stat(per[0]), stat(per[1])


def method(what):
    return ("%s; device events around %d back-to-back calls, arms alternating window by window, %d windows per arm after %d "
            "warm-up windows; won = slowest window of the first arm < fastest window of the second" % (what, CALLS, WINDOWS, WARMUP))


def mlp(rng, dims):
    Ws = [(rng.normal(size=(dims[i], dims[i + 1])) * np.sqrt(2.0 / (dims[i] + dims[i + 1]))).astype(np.float32) for i in range(len(dims) - 1)]
    bs = [(rng.normal(size=dims[i + 1]) * 0.1).astype(np.float32) for i in range(len(dims) - 1)]
    return Ws, bs


def norm(rng, d=2):
    return dict(mean_x=rng.normal(size=d) * 0.3, std_x=rng.uniform(0.05, 1.0, d), mean_y=rng.normal(size=1) * 0.1,
                std_y=rng.uniform(0.3, 1.2, 1), mean_z=rng.normal(size=d) * 0.01, std_z=rng.uniform(0.005, 0.05, d))


def captured(smart, prepare):
    """capture ``smart``'s step without a transition log (the log row is a device counter that a free-running replay would
    push past the chunk) and return its graph"""
    prepare()
    e = smart.env
    smart._graphs.replay(1, e.device, lambda: smart.graph_key(1, None, None), lambda: smart.fused_step(None, None),
                         smart._state_tensors(), None)
    return list(smart._graphs.graphs.values())[-1]


def step_case(P, n, hidden, prec, seed=3):
    rng = np.random.default_rng(seed)
    agents, models = [], []
    for p in range(P):
        a = DDPG_Baselines_agent(ssc.make(ENV), None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True,
                                 seed=seed + p, training=False, ou_sigma=0.3, precision="bf16_mfma")
        a.decaying_ou_action_noise.epsilon = 0.5
        agents.append(a)
        Ws, bs = mlp(rng, (3, hidden, 2))
        models.append(nav.DynamicsModel(Ws, bs, norm(rng), state_dim=2, act_dim=1, precision=prec))
    kw = dict(eta=0.5, n_plans=2, num_control_samples=16, horizon=4, chunk_steps=64, seed=seed, w_max=64)
    env = ssc.VecEnv(ENV, P * n, seed=seed, max_episode_steps=60)
    env.reset()
    pop = ssc.VecSmartStartPopulation(env, agents, models, [n] * P, **kw)
    own = []
    for p in range(P):
        e = ssc.VecEnv(ENV, n, seed=seed, max_episode_steps=60, env_id0=p * n)
        e.reset()
        own.append(ssc.VecSmartStart(e, agents[p], models[p], **kw))
    path = np.stack([np.linspace(-0.55, -0.3, 12), np.linspace(0.0, 0.02, 12)], 1)
    for pr, o in zip(pop.pairs, own):
        plans = [o.plan_from_path(path), o.plan_from_path(path[::-1].copy())]
        pr.pool.publish(plans)
        o.pool.publish(plans)

    def prep_pop():
        pop.nav.begin_chunk(env)
        pop.sync_pair_table()
        pop.sync_actor_items()

    def prep_own(o):
        def f():
            o.nav.begin_chunk(o.env)
            o.d_eps.fill_(0.5)
            o.d_eta.fill_(o.eta)
        return f
    graphs = [captured(o, prep_own(o)) for o in own]          # the pairs first: a model's own call allocates its workspace
    g = captured(pop, prep_pop)
    a, b = timed_pair(g.replay, lambda: [x.replay() for x in graphs])
    return dict(P=P, envs_per_pair=n, model="1x%d %s" % (hidden, prec), population=a, per_pair=b,
                actor_ways=[w[0] for w in pop._actor_plan], sim_ways=pop.nav.sim_ways,
                won=a["max_us"] < b["min_us"], ratio=b["median_us"] / a["median_us"])


def run_step(out):
    cases = []
    for hidden, prec in ((32, "f32"), (500, "bf16_mfma")):
        for n in (16, 1024):
            for P in (1, 2, 4, 16, 64):
                c = step_case(P, n, hidden, prec)
                cases.append(c)
                print("step %-15s P %2d x %4d envs: population %7.1f [%7.1f, %7.1f] us, per-pair graphs %8.1f [%8.1f, %8.1f] us  x%.2f %s"
                      % (c["model"], P, n, c["population"]["median_us"], c["population"]["min_us"], c["population"]["max_us"],
                         c["per_pair"]["median_us"], c["per_pair"]["min_us"], c["per_pair"]["max_us"], c["ratio"],
                         "WON" if c["won"] else "not won"), flush=True)
                json.dump(dict(method=method("graph replay per env step, 16 candidates, horizon 4, eta 0.5, epsilon 0.5"), cases=cases),
                          open(os.path.join(out, "step.json"), "w"), indent=1)


ACTOR_CLASSES = [("f32 64-32", 64, 32, _ffi.SSC_PREC_F32), ("bf16 64-32", 64, 32, _ffi.SSC_PREC_BF16_MFMA),
                 ("bf16 200-100", 200, 100, _ffi.SSC_PREC_BF16_MFMA), ("generic 48-24", 48, 24, _ffi.SSC_PREC_F32)]


def actor_desc(rng, h1, h2, prec, keep, obs_dim=2):
    shapes = dict(W1=(obs_dim, h1), b1=(h1,), W2=(h1, h2), b2=(h2,), W3=(h2, 1), b3=(1,))
    w = {k: torch.as_tensor(rng.normal(0, 0.3, s).astype(np.float32), device="cuda") for k, s in shapes.items()}
    keep.append(w)
    a = _ffi.ActorDesc()
    a.obs_dim, a.h1, a.h2, a.act_dim, a.last_layer_tanh, a.precision, a.obs_clip = obs_dim, h1, h2, 1, 1, prec, 5.0
    _ffi.set_net_ptrs(a, w)
    return a


def run_actor(out):
    lib, cases, rng = _ffi.lib(), [], np.random.default_rng(1)
    for name, h1, h2, prec in ACTOR_CLASSES:
        for n in (16, 1024):
            for P in (1, 2, 4, 16, 64):
                keep = []
                descs = [actor_desc(rng, h1, h2, prec, keep) for _ in range(P)]
                obs = torch.as_tensor(rng.normal(size=(P * n, 2)).astype(np.float32), device="cuda")
                act = torch.zeros((P * n, 1), dtype=torch.float32, device="cuda")
                items = DeviceItems(_ffi.ActorManyItem, P, "cuda")
                for p, (it, d) in enumerate(zip(items.items, descs)):
                    it.actor, it.row0, it.rows = d, p * n, n
                items.upload()
                s = _ffi.stream()

                def many():
                    _ffi.check(lib.ssc_actor_forward_many(items.h_ptr, items.d_ptr, P, P * n, _ffi.ptr(obs), _ffi.ptr(act), s))

                def alone():
                    for p, d in enumerate(descs):
                        _ffi.check(lib.ssc_actor_forward(ctypes.byref(d), n, obs.data_ptr() + 8 * p * n, act.data_ptr() + 4 * p * n, s))
                a, b = timed_pair(many, alone, calls=50)
                c = dict(cls=name, P=P, rows_per_actor=n, many=a, per_pair=b, won=a["max_us"] < b["min_us"], ratio=b["median_us"] / a["median_us"])
                cases.append(c)
                print("actor %-13s P %2d x %4d rows: many %6.1f [%6.1f, %6.1f] us, per-pair calls %7.1f [%7.1f, %7.1f] us  x%.2f %s"
                      % (name, P, n, a["median_us"], a["min_us"], a["max_us"], b["median_us"], b["min_us"], b["max_us"], c["ratio"],
                         "WON" if c["won"] else "not won"), flush=True)
    json.dump(dict(method=method("one ssc_actor_forward_many against P ssc_actor_forward calls (50 calls per window)"), cases=cases),
              open(os.path.join(out, "actor.json"), "w"), indent=1)


def bind(path):
    h = ctypes.CDLL(path)
    for name in ("ssc_actor_forward", "ssc_smartstart_rollout_step", "ssc_last_error"):
        res, args = _ffi._SIGNATURES[name]
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    return h


def run_single(out, parent_lib):
    new, old = _ffi.lib(), bind(parent_lib)
    cases, rng, keep = [], np.random.default_rng(2), []
    for name, h1, h2, prec in ACTOR_CLASSES:
        for m in (1024, 65536):
            d = actor_desc(rng, h1, h2, prec, keep)
            obs = torch.as_tensor(rng.normal(size=(m, 2)).astype(np.float32), device="cuda")
            act = torch.zeros((m, 1), dtype=torch.float32, device="cuda")
            s = _ffi.stream()
            call = lambda L: (lambda: _ffi.check(L.ssc_actor_forward(ctypes.byref(d), m, _ffi.ptr(obs), _ffi.ptr(act), s)))
            a, b = timed_pair(call(new), call(old), calls=50)
            cases.append(dict(call="ssc_actor_forward", cls=name, rows=m, this_build=a, parent=b,
                              unchanged=b["min_us"] <= a["median_us"] <= b["max_us"]))
            print("single ssc_actor_forward %-13s m %5d: this %6.2f us, parent %6.2f [%6.2f, %6.2f] us %s"
                  % (name, m, a["median_us"], b["median_us"], b["min_us"], b["max_us"], cases[-1]["unchanged"]), flush=True)
    for n in (1024, 65536):                                 # the step kernel alone, on a VecSmartStart's own arguments
        env = ssc.VecEnv(ENV, n, seed=5, max_episode_steps=60)
        env.reset()
        agent = DDPG_Baselines_agent(ssc.make(ENV), None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32, lastLayerTanh=True,
                                     seed=5, training=False, precision="bf16_mfma")
        Ws, bs = mlp(rng, (3, 32, 2))
        smart = ssc.VecSmartStart(env, agent, nav.DynamicsModel(Ws, bs, norm(rng), state_dim=2, act_dim=1), eta=0.5, n_plans=2,
                                  num_control_samples=16, horizon=4, seed=5, w_max=64)
        path = np.stack([np.linspace(-0.55, -0.3, 12), np.linspace(0.0, 0.02, 12)], 1)
        smart.pool.publish([smart.plan_from_path(path)])
        b_ = smart.nav
        b_.begin_chunk(env)
        smart.d_eps.fill_(0.5)
        smart.fused_step(None, None)                        # fills A / best / scores once; the step kernel is then timed alone
        fb = b_._fused_buffers(env.device)
        st = smart.pool.as_struct(b_.N, b_.H)
        nv = _ffi.MpcNavState(smart.pool.cur_idx.data_ptr(), b_.start_idx.data_ptr(), b_.actions_done.data_ptr(),
                              b_.at_goal.data_ptr(), b_.give_up, b_.final_steps)
        rs, ss, s = env.rollout_state(), smart._step_struct(1), _ffi.stream()
        call = lambda L: (lambda: _ffi.check(L.ssc_smartstart_rollout_step(
            ctypes.byref(env.params), ctypes.byref(st), ctypes.byref(nv), ctypes.byref(ss), _ffi.ptr(fb["A"]), _ffi.ptr(fb["best"]),
            float(b_.noise_amount), b_.seed, b_.problem_id0, ctypes.byref(rs), None, None, _ffi.ptr(env.stats), env._seed,
            env.env_id0, _ffi.ptr(fb["t"]), _ffi.ptr(fb["k"]), _ffi.ptr(fb["ticket"]), _ffi.ptr(fb["plan"]), s)))
        a, b = timed_pair(call(new), call(old), calls=50)
        cases.append(dict(call="ssc_smartstart_rollout_step", envs=n, this_build=a, parent=b,
                          unchanged=b["min_us"] <= a["median_us"] <= b["max_us"]))
        print("single ssc_smartstart_rollout_step %5d envs: this %6.2f us, parent %6.2f [%6.2f, %6.2f] us %s"
              % (n, a["median_us"], b["median_us"], b["min_us"], b["max_us"], cases[-1]["unchanged"]), flush=True)
    json.dump(dict(method=method("this build's call against the parent commit's library in the same process (50 calls per window); "
                                 "unchanged = this build's median inside the parent's [min, max]"), cases=cases),
              open(os.path.join(out, "single.json"), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("step", "actor", "single"))
    ap.add_argument("--out", default="profiles/smartstart_population")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.what == "step":
        run_step(args.out)
    elif args.what == "actor":
        run_actor(args.out)
    else:
        run_single(args.out, args.parent_lib)
