#!/usr/bin/env python3
"""Measurements of the fused evaluation rollout.

    python tools/exp_ddpg_eval.py percall --out DIR    # ssc_ddpg_eval_rollout against what a user had to enqueue before
    python tools/exp_ddpg_eval.py chunk --out DIR      # chunk time of rl_train_vec_ddpg without / with evaluation

percall: HIP events around back-to-back calls on one stream after warm-up, median of 7 runs.  "by hand" is a noise-free
``env.rollout`` with a full transition log (fp32 actor, and separately bf16_mfma) + ``agent.critic`` on the K * E logged rows
+ torch mean / std of Q; the episode-ring drain it would also need (a host read) is left out, in its favour.
chunk: the README's loop shape (65 536 envs, 256-step chunks, 10 x batch 1024, 64-32; synchronous loop), host clock around 16
chunks between two device synchronisations, 5 runs per variant alternating in one process after a warm-up run of each."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent  # noqa: E402

ENV = "MountainCarContinuous-v0"


def make_agent(h, batch=64, iters=50):
    return DDPG_Baselines_agent(ssc.make(ENV, seed=1), None, batch_size=batch, num_train_iterations=iters, actor_h1=h[0],
                                actor_h2=h[1], critic_h1=h[0], critic_h2=h[1], lastLayerTanh=True, seed=7)


def timed(fn, calls, warmup, runs=7):
    """median / min / max over ``runs`` of the time per call (ms) of ``calls`` back-to-back calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / calls)
    return dict(median_ms=statistics.median(per), min_ms=min(per), max_ms=max(per), runs=per)


def percall(out_dir):
    rows = []
    for h, envs, K in (((64, 32), 1024, 1000), ((64, 32), 4096, 1000), ((200, 100), 1024, 100)):
        agent = make_agent(h)
        calls, warmup = (3, 2) if K >= 1000 else (5, 3)
        row = dict(net="%d-%d" % h, envs=envs, steps=K)
        eval_env = ssc.VecEnv(ENV, envs, seed=3)
        block = torch.empty(8, dtype=torch.float64, device="cuda")
        row["ssc_ddpg_eval_rollout"] = timed(lambda: agent.evaluate_device(eval_env, K, out=block), calls, warmup)
        row["block"] = block.cpu().tolist()
        for precision in ("f32", "bf16_mfma"):
            if precision == "f32" and h != (64, 32):
                continue                 # the fused fp32 rollout actor exists for 64-32 / 64-64 only
            env = ssc.VecEnv(ENV, envs, seed=3)
            env.reset()
            pd = env.policy_desc(ssc.ActorPolicy(agent.weights, last_layer_tanh=True, precision=precision, ou_epsilon=0.0,
                                                 obs_clip=5.0))
            chunk = ssc.TransitionChunk(env.obs_dim, K, envs, env.device)
            ring = ssc.EpisodeRing(1 << 16, env.device)
            stats = torch.empty(2, dtype=torch.float64, device="cuda")

            def by_hand():
                ring.cursor.zero_()
                env.rollout(K, out=chunk, ring=ring, policy_desc=pd)
                s, a = chunk.records()[:2]
                q = agent.critic(s, a).double()
                stats[0] = q.mean()
                stats[1] = q.std(unbiased=False)
            row["by_hand_" + precision] = timed(by_hand, calls, warmup)
        rows.append(row)
        print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in row.items() if k != "block"}), flush=True)
    gate = rows[0]
    result = dict(percall=rows, gate=dict(shape="64-32, 1024 envs x 1000 steps", new_median_ms=gate["ssc_ddpg_eval_rollout"]["median_ms"],
                                          by_hand_f32_median_ms=gate["by_hand_f32"]["median_ms"],
                                          holds=gate["ssc_ddpg_eval_rollout"]["median_ms"] <= gate["by_hand_f32"]["median_ms"]))
    with open(os.path.join(out_dir, "percall.json"), "w") as f:
        json.dump(result, f, indent=1)
    print("gate:", json.dumps(result["gate"]), flush=True)
    return 0 if result["gate"]["holds"] else 1


def chunk(out_dir):
    envs, steps, batch, iters, chunks = 65536, 256, 1024, 10, 16
    variants = {"without": None, "eval_every_1": 1, "eval_every_16": 16}

    def one(eval_every):
        agent = make_agent((64, 32), batch, iters)
        env = ssc.VecEnv(ENV, envs, seed=5)
        kw = {}
        if eval_every is not None:
            kw = dict(eval_env=ssc.VecEnv(ENV, 1024, seed=6, env_id0=envs), eval_every=eval_every, eval_steps=1000)
        clock = {}

        def on_chunk(i, _chunk, _env):       # the clock runs from the end of chunk 0 to the end of the last chunk
            if i in (0, chunks):
                torch.cuda.synchronize()
                clock[i] = time.perf_counter()
        ssc.rl_train_vec_ddpg(env, agent, chunks + 1, chunk_steps=steps, replay_capacity=1 << 20, replay_last_steps=16,
                              train_iters=iters, drain_every=chunks + 2, on_chunk=on_chunk, **kw)
        return (clock[chunks] - clock[0]) / chunks * 1e3

    for v in variants.values():
        one(v)
    times = {name: [] for name in variants}
    for _ in range(5):
        for name, v in variants.items():
            times[name].append(one(v))
    result = dict(shape=dict(envs=envs, chunk_steps=steps, batch=batch, iters=iters, chunks=chunks, net="64-32", eval_envs=1024,
                             eval_steps=1000),
                  chunk_ms=times, median_ms={k: statistics.median(v) for k, v in times.items()})
    with open(os.path.join(out_dir, "chunk.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result["median_ms"]), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["percall", "chunk"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ddpg_eval"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    sys.exit(percall(args.out) if args.what == "percall" else chunk(args.out))
