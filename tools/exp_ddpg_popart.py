#!/usr/bin/env python3
"""Measurements of the Pop-Art learner path.

    python tools/exp_ddpg_popart.py iter --out DIR [--parent-lib libssc_parent.so]
        microseconds per training iteration: the Pop-Art path (four launches) against the plain path (two launches, or the
        one-workgroup kernel at 64-32 x 64) on the same replay rows and batch indices.  HIP events around one call of ITERS
        iterations; the variants alternate inside every one of 9 rounds after a warm-up call of each; median / min / max.
        --parent-lib: also time the plain paths through a library built from the parent commit.
    python tools/exp_ddpg_popart.py trace --shape 64-32x64
        the workload a kernel trace is taken of: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/... trace --shape S`
    python tools/exp_ddpg_popart.py trace-summary --csv kernel_stats.csv --shape S --out DIR
        per-kernel average durations of that trace -> DIR/kernels_S.json
    python tools/exp_ddpg_popart.py learn --out DIR
        3 seeds of the cadence of tests/test_gpu_vec_learning.py (4096 envs, 32-step chunks, 100 x batch 64 on the newest 4
        steps) on stock MountainCar with normalize_returns + enable_popart: late-window median return, mu and sigma at the end.
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd import _ffi  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent  # noqa: E402

ENV = "MountainCarContinuous-v0"
SHAPES = {"64-32x64": ((64, 32), 64), "64-32x1024": ((64, 32), 1024), "200-100x1024": ((200, 100), 1024)}
ITERS, ROWS = 200, 1 << 17


def make_agent(h, batch, popart):
    return DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=batch, actor_h1=h[0], actor_h2=h[1], critic_h1=h[0],
                                critic_h2=h[1], lastLayerTanh=True, actor_lr=1e-3, critic_lr=1e-3, seed=7,
                                normalize_returns=popart, enable_popart=popart)


def replay_rows(batch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, device="cuda")
    s = torch.stack([u(ROWS) * 1.8 - 1.2, u(ROWS) * 0.14 - 0.07], dim=1).contiguous()
    a = (u(ROWS, 1) * 2 - 1).contiguous()
    r = torch.where(u(ROWS) < 0.01, torch.full((ROWS,), 100.0, device="cuda"), -0.1 * a[:, 0] ** 2).contiguous()   # MountainCar's scales
    t = (u(ROWS) < 0.01).to(torch.uint8).contiguous()
    s2 = (s + 0.01 * (u(ROWS, 2) - 0.5)).contiguous()
    idx = torch.randint(0, ROWS, (ITERS, batch), generator=g, device="cuda", dtype=torch.int32).contiguous()
    return (s, a, r, t, s2), idx


def load_parent(path):
    handle = ctypes.CDLL(path)
    for name, (res, args) in _ffi._SIGNATURES.items():
        if hasattr(handle, name):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
    return handle


def iter_cmd(out_dir, parent_lib):
    results = {}
    parent = load_parent(parent_lib) if parent_lib else None
    for name, (h, batch) in SHAPES.items():
        rows, idx = replay_rows(batch)
        variants = {}

        def add(label, popart, wide, lib=None):
            agent = make_agent(h, batch, popart)
            if lib is not None:
                agent.lib = lib

            def call():
                if wide:
                    os.environ["SSC_DDPG_WIDE"] = "1"
                else:
                    os.environ.pop("SSC_DDPG_WIDE", None)
                agent.train_on(*rows, idx, ITERS)
            variants[label] = call
        add("popart", True, False)
        add("plain", False, False)                      # 64-32 x 64: the one-workgroup kernel; x 1024: the 64-row tiled kernel
        add("plain_wide", False, True)                  # the two-launch multi-workgroup path a Pop-Art agent's step extends
        if parent is not None:
            add("parent_plain", False, False, parent)
            add("parent_plain_wide", False, True, parent)
        for call in variants.values():
            call()
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(9):
            for label, call in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                torch.cuda.synchronize()
                us[label].append(a.elapsed_time(b) * 1e3 / ITERS)
        os.environ.pop("SSC_DDPG_WIDE", None)
        results[name] = {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), runs=v) for k, v in us.items()}
        print(name, json.dumps({k: round(v["median_us"], 2) for k, v in results[name].items()}), flush=True)
    with open(os.path.join(out_dir, "iter.json"), "w") as f:
        json.dump(dict(iters_per_call=ITERS, rounds=9, unit="microseconds per iteration", shapes=results), f, indent=1)
    return 0


def trace_cmd(shape):
    h, batch = SHAPES[shape]
    rows, idx = replay_rows(batch)
    agent = make_agent(h, batch, True)
    for _ in range(3):
        agent.train_on(*rows, idx, ITERS)
    torch.cuda.synchronize()
    return 0


def trace_summary_cmd(path, shape, out_dir):
    kernels = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "ddpg_" not in name:
                continue
            kernels[name] = dict(calls=int(float(row["Calls"])), average_us=float(row["AverageNs"]) / 1e3,
                                 min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    with open(os.path.join(out_dir, "kernels_%s.json" % shape), "w") as f:
        json.dump(dict(shape=shape, source="rocprofv3 --kernel-trace --stats", kernels=kernels), f, indent=1)
    for k, v in kernels.items():
        print("%8.2f us x %6d  %s" % (v["average_us"], v["calls"], k[:110]), flush=True)
    return 0


def learn_cmd(out_dir):
    n_envs, chunk, iters, batch, last, chunks, window = 4096, 32, 100, 64, 4, 1500, (90, 130)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ddpg_good_params_curves.npz"))
    p = json.loads(str(g["param_dict"]))
    runs = []
    for seed in (1, 2, 3):
        env = ssc.VecEnv(ENV, n_envs, seed=seed)
        env.reset()
        agent = DDPG_Baselines_agent(ssc.make(ENV), None, batch_size=batch, num_train_iterations=iters, ou_epsilon=p["ou_epsilon"],
                                     ou_min_epsilon=p["ou_min_epsilon"], ou_epsilon_decay_factor=p["ou_epsilon_decay_factor"],
                                     ou_mu=p["ou_mu"], ou_sigma=p["ou_sigma"], ou_theta=p["ou_theta"], actor_lr=p["actor_lr"],
                                     actor_h1=p["actor_h1"], actor_h2=p["actor_h2"], critic_lr=p["critic_lr"], critic_h1=p["critic_h1"],
                                     critic_h2=p["critic_h2"], gamma=p["gamma"], tau=p["tau"], lastLayerTanh=p["lastLayerTanh"],
                                     seed=seed, normalize_returns=True, enable_popart=True)
        summary, losses, replay = ssc.rl_train_vec_ddpg(env, agent, chunks, chunk_steps=chunk, replay_capacity=1 << 20, seed=seed,
                                                        replay_last_steps=last)
        torch.cuda.synchronize()
        ep = np.asarray(summary.episodes, np.float64).reshape(-1, 2)
        late = ep[window[0] * n_envs:window[1] * n_envs]
        mean, std = agent.ret_rms.mean_std()
        run = dict(seed=seed, episodes=len(ep), late_window_episodes=len(late),
                   late_median_return=float(np.median(late[:, 1])) if len(late) else None,
                   late_goal_share=float((late[:, 0] < 999).mean()) if len(late) else None,
                   ret_rms_mean=float(mean[0]), ret_rms_std=float(std[0]), count=float(agent.ret_rms.block[2].item()),
                   last_losses=losses[-1][-1].tolist())
        runs.append(run)
        print(json.dumps(run), flush=True)
    with open(os.path.join(out_dir, "learning.json"), "w") as f:
        json.dump(dict(setup=dict(env=ENV, envs=n_envs, chunk_steps=chunk, iters=iters, batch=batch, replay_last_steps=last,
                                  chunks=chunks, late_window_generations=window), runs=runs), f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["iter", "trace", "trace-summary", "learn"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg_popart"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--shape", choices=list(SHAPES), default="64-32x64")
    ap.add_argument("--csv", default=None)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.what == "iter":
        sys.exit(iter_cmd(args.out, args.parent_lib))
    if args.what == "trace":
        sys.exit(trace_cmd(args.shape))
    if args.what == "trace-summary":
        sys.exit(trace_summary_cmd(args.csv, args.shape, args.out))
    sys.exit(learn_cmd(args.out))
