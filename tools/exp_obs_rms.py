#!/usr/bin/env python3
"""normalize_observations cost, with the statistics on and off (one JSON line):

  * the config-3 rollout: 65 536 MountainCar envs x 1024 steps, 64-32 bf16 MFMA actor, unit bounds, noise on
    (ActorPolicyFused: plain vs the NORM instantiation)
  * the learner: us per iteration of the 64-32 networks at batch 64 (one workgroup) and 1024 (64-row tiles)
  * the statistics update: one 64-step x 65 536-env chunk of 2-dim observations (33.5 MB of obs0 read)

    python3 tools/exp_obs_rms.py                 (all figures)
    python3 tools/exp_obs_rms.py --update-only   (the update alone, e.g. under rocprofv3 --kernel-trace --stats)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent  # noqa: E402
from smartstartcontinuous_amd.obs_rms import ObsRms  # noqa: E402
from smartstartcontinuous_amd.vec_env import TransitionChunk  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def agent(batch):
    return DDPG_Baselines_agent(ssc.make("MountainCarContinuous-v0"), None, actor_h1=64, actor_h2=32, critic_h1=64, critic_h2=32,
                                lastLayerTanh=True, precision="bf16_mfma", seed=1, batch_size=batch, training=False)


def stats():
    r = ObsRms(2)
    r.update_rows(np.random.default_rng(0).normal([-0.5, 0.0], [0.3, 0.02], size=(4096, 2)).astype(np.float32))
    return r


def main():
    out = {}
    rms = stats()
    # config-3 rollout
    n, K = 65536, 1024
    ag = agent(64)
    for name, r in (("off", None), ("on", rms)):
        env = ssc.VecEnv("MountainCarContinuous-v0", n, seed=3)
        env.reset()
        chunk = TransitionChunk(2, K, n, env.device)
        pd = env.policy_desc(ag.as_policy(obs_rms=r))
        med, mn = timed(lambda: env.rollout(K, out=chunk, policy_desc=pd), 7)
        out[f"rollout_c3_us_{name}"] = {"median": med, "min": mn}
    out["rollout_c3_ratio"] = out["rollout_c3_us_on"]["median"] / out["rollout_c3_us_off"]["median"]
    # learner
    rng = np.random.default_rng(1)
    cap, iters = 1 << 16, 200
    dev = lambda v, dt=torch.float32: torch.as_tensor(v, dtype=dt).cuda().contiguous()
    s = dev(rng.uniform(-1.2, 0.6, size=(cap, 2)))
    s2 = dev(rng.uniform(-1.2, 0.6, size=(cap, 2)))
    a, rew = dev(rng.uniform(-1, 1, size=(cap, 1))), dev(rng.normal(size=cap))
    t = dev(rng.random(cap) < 0.01, torch.uint8)
    for batch in (64, 1024):
        ag = agent(batch)
        idx = dev(rng.integers(0, cap, size=(iters, batch)), torch.int32)
        for name, r in (("off", None), ("on", rms)):
            med, mn = timed(lambda: ag.train_on(s, a, rew, t, s2, idx, iters, obs_rms=r), 5)
            out[f"learner_b{batch}_us_per_iter_{name}"] = {"median": med / iters, "min": mn / iters}
    out.update(update_figures())
    print(json.dumps(out))


def update_figures(calls=200):
    """The statistics update of one 64-step x 65 536-env x 2-dim chunk.  `update_us_single`: an event pair around ONE call
    (ctypes marshalling + two launches onto an idle GPU); `update_us_back_to_back`: `calls` calls queued between one event
    pair, per call -- the stream time the update costs inside a loop.  The kernels alone: run this under
    `rocprofv3 --kernel-trace --stats` (obs_rms_partial_kernel / obs_rms_final_kernel)."""
    chunk = TransitionChunk(2, 64, 65536, "cuda")
    chunk.obs.copy_(torch.randn(2, 64, 65536, device="cuda"))
    r = ObsRms(2)
    nbytes = 2 * 64 * 65536 * 4
    med, mn = timed(lambda: r.update_chunk(chunk), 50)

    def batch():
        for _ in range(calls):
            r.update_chunk(chunk)
    bmed, bmin = timed(batch, 5)
    per = bmed / calls
    return {"update_us_single": {"median": med, "min": mn}, "update_us_back_to_back": per,
            "update_GBps_back_to_back": nbytes / (per * 1e-6) / 1e9}


if __name__ == "__main__":
    if "--update-only" in sys.argv:
        print(json.dumps(update_figures()))
    else:
        main()
