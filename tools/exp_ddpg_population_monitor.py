#!/usr/bin/env python3
"""Measurement of the population evaluation and diagnostics launches.

    python tools/exp_ddpg_population_monitor.py --out DIR

P in {1, 8, 64, 256} agents of the shipped shape (64-32, obs_dim 2, tanh layer 2) on MountainCar.  Evaluation: 64 eval envs
per agent, 200 steps per call (the 999-step time limit: a call sees a few resets); diagnostics: a sample of m = 64 rows per
agent.  "many" is one ssc_ddpg_eval_rollout_many / ssc_ddpg_stats_many call for the population, "loop" the yardstick: P
per-agent calls of ssc_ddpg_eval_rollout / ssc_ddpg_stats one after the other on one stream.  HIP events around back-to-back
calls after warm-up, median of 7 runs, the two ways alternating run by run in one process; the run-to-run spread
(max - min) / median of both sides is written beside every ratio, and P = 1 is a row like any other.  Before anything is
timed the two ways run once from the same state at the timed sizes and their blocks are compared bit for bit.
-> monitor.json"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd import _ffi  # noqa: E402
from smartstartcontinuous_amd.population import DeviceItems, PairCursors  # noqa: E402

ENV = "MountainCarContinuous-v0"
N_EVAL, K_EVAL, M_STATS = 64, 200, 64
H1, H2 = 64, 32
KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")


def net(rng, kind, scale=1.0, bias=0.0):
    """device tensors of one 64-32 network and its descriptor"""
    extra = 1 if kind == "critic" else 0
    glorot = lambda i, o: rng.uniform(-1, 1, size=(i, o)) * np.sqrt(6.0 / (i + o))
    w = dict(W1=glorot(2, H1), b1=0.1 * rng.normal(size=H1), W2=glorot(H1 + extra, H2), b2=0.1 * rng.normal(size=H2),
             W3=rng.uniform(-scale, scale, size=(H2, 1)), b3=bias + 0.05 * rng.normal(size=1))
    t = {k: torch.as_tensor(v.astype(np.float32)).cuda().contiguous() for k, v in w.items()}
    d = _ffi.ActorDesc() if kind == "actor" else _ffi.CriticDesc()
    d.obs_dim, d.act_dim, d.h1, d.h2 = 2, 1, H1, H2
    for k in KEYS:
        setattr(d, k, t[k].data_ptr())
    d.last_layer_tanh, d.obs_clip = 1, 5.0
    return t, d


class RawPopulation:
    """P agents' networks, eval-env sets and diagnostics samples, and the launch items of both population calls"""

    def __init__(self, P, seed=0):
        rng = np.random.default_rng(seed)
        lib = _ffi.lib()
        self.P = P
        self.nets = [(net(rng, "actor", 0.25), net(rng, "critic", 1.5, 20.0)) for _ in range(P)]
        self.envs = [ssc.VecEnv(ENV, N_EVAL, seed=50 + p, env_id0=N_EVAL * p) for p in range(P)]
        for e in self.envs:
            e.reset()
        self.obs = torch.as_tensor(rng.uniform(-1.2, 0.6, (P, M_STATS, 2)).astype(np.float32)).cuda()
        self.act = torch.as_tensor(rng.uniform(-1, 1, (P, M_STATS, 1)).astype(np.float32)).cuda()
        e_ws, s_ws = int(lib.ssc_ddpg_eval_workspace_bytes(N_EVAL)), int(lib.ssc_ddpg_stats_workspace_bytes(M_STATS))
        row = lambda b: (b + 255) // 256 * 256
        self.e_ws = torch.empty((P, row(e_ws)), dtype=torch.uint8, device="cuda")
        self.s_ws = torch.empty((P, row(s_ws)), dtype=torch.uint8, device="cuda")
        self.e_out = torch.zeros((2, P, _ffi.SSC_DDPG_N_EVAL), dtype=torch.float64, device="cuda")      # [many | loop]
        self.s_out = torch.zeros((2, P, _ffi.SSC_DDPG_N_STATS), dtype=torch.float64, device="cuda")
        self.e_items, self.s_items = DeviceItems(_ffi.DdpgEvalManyItem, P, "cuda"), DeviceItems(_ffi.DdpgStatsManyItem, P, "cuda")
        self.states = []
        for p, (it, st, e) in enumerate(zip(self.e_items.items, self.s_items.items, self.envs)):
            (_, ad), (_, cd) = self.nets[p]
            it.params, it.actor, it.critic, it.act_low, it.act_high, it.n = e.params, ad, cd, -1.0, 1.0, N_EVAL
            self.states.append(e.rollout_state(ou=False))
            it.state = self.states[-1]
            it.d_out, it.d_workspace, it.workspace_bytes = self.e_out[0, p].data_ptr(), self.e_ws[p].data_ptr(), e_ws
            it.seed, it.env_id0 = e._seed, e.env_id0
            st.actor, st.critic, st.m = ad, cd, M_STATS
            st.d_obs, st.d_act = self.obs[p].data_ptr(), self.act[p].data_ptr()
            st.d_out, st.d_workspace, st.workspace_bytes = self.s_out[0, p].data_ptr(), self.s_ws[p].data_ptr(), s_ws
        self.e_items.upload()
        self.s_items.upload()
        self.cursors = PairCursors(P, "cuda")
        self.cursors.stage(step0=[0] * P).upload()               # the reset draws do not enter the cost: one step0 for all calls
        self.e_ws_bytes, self.s_ws_bytes = e_ws, s_ws
        torch.cuda.synchronize()

    def eval_many(self):
        _ffi.check(_ffi.lib().ssc_ddpg_eval_rollout_many(self.e_items.h_ptr, self.e_items.d_ptr, self.cursors.h_ptr, self.cursors.d_ptr,
                                                         self.P, K_EVAL, 1, _ffi.stream()))

    def eval_loop(self):
        lib, s = _ffi.lib(), _ffi.stream()
        for p, e in enumerate(self.envs):
            (_, ad), (_, cd) = self.nets[p]
            _ffi.check(lib.ssc_ddpg_eval_rollout(ctypes.byref(e.params), ctypes.byref(ad), ctypes.byref(cd), -1.0, 1.0, N_EVAL, K_EVAL,
                                                 ctypes.byref(self.states[p]), None, None, None, 1, self.e_out[1, p].data_ptr(),
                                                 self.e_ws[p].data_ptr(), self.e_ws_bytes, e._seed, e.env_id0, 0, s))

    def stats_many(self):
        _ffi.check(_ffi.lib().ssc_ddpg_stats_many(self.s_items.h_ptr, self.s_items.d_ptr, self.P, _ffi.stream()))

    def stats_loop(self):
        lib, s = _ffi.lib(), _ffi.stream()
        for p in range(self.P):
            (_, ad), (_, cd) = self.nets[p]
            _ffi.check(lib.ssc_ddpg_stats(ctypes.byref(ad), ctypes.byref(cd), None, M_STATS, self.obs[p].data_ptr(), self.act[p].data_ptr(),
                                          None, None, self.s_out[1, p].data_ptr(), self.s_ws[p].data_ptr(), self.s_ws_bytes, s))

    def same_bits(self):
        """both ways once from the same env state at the timed sizes -> (eval blocks equal, stats blocks equal)"""
        start = [{k: getattr(e, k).clone() for k in ("s0", "s1", "steps", "ep_ret")} for e in self.envs]
        self.eval_many()
        after = [{k: getattr(e, k).clone() for k in start[0]} for e in self.envs]
        for e, st in zip(self.envs, start):
            for k, v in st.items():
                getattr(e, k).copy_(v)
        self.eval_loop()
        self.stats_many()
        self.stats_loop()
        torch.cuda.synchronize()
        bits = lambda x: x.view(torch.int64)
        state_ok = all(torch.equal(getattr(e, k), v) for e, st in zip(self.envs, after) for k, v in st.items())
        return bool(torch.equal(bits(self.e_out[0]), bits(self.e_out[1])) and state_ok), bool(torch.equal(bits(self.s_out[0]), bits(self.s_out[1])))


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


def compare(many, loop):
    """the ratio and whether the difference of the medians exceeds both sides' run-to-run ranges"""
    gain = loop["median_ms"] - many["median_ms"]
    ranges = (many["max_ms"] - many["min_ms"]) + (loop["max_ms"] - loop["min_ms"])
    return dict(loop_over_many=loop["median_ms"] / many["median_ms"], gain_ms=gain, both_ranges_ms=ranges,
                many_faster_by_more_than_the_spreads=gain > ranges, many_slower_by_more_than_the_spreads=-gain > ranges)


def main(out_dir):
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: there is no fallback")
    rows = []
    for P in (1, 8, 64, 256):
        pop = RawPopulation(P, seed=P)
        eval_same, stats_same = pop.same_bits()
        e_many, e_loop = timed_pair(pop.eval_many, pop.eval_loop, max(2, 32 // P))
        s_many, s_loop = timed_pair(pop.stats_many, pop.stats_loop, max(4, 256 // P))
        row = dict(agents=P, eval_bits_equal=eval_same, stats_bits_equal=stats_same,
                   eval_many=e_many, eval_loop=e_loop, eval=compare(e_many, e_loop),
                   stats_many=s_many, stats_loop=s_loop, stats=compare(s_many, s_loop))
        rows.append(row)
        print(json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in row.items()}), flush=True)
    result = dict(shape="64-32, obs_dim 2, tanh; evaluation: %d envs x %d steps per agent per call; diagnostics: m = %d rows per agent"
                        % (N_EVAL, K_EVAL, M_STATS),
                  protocol="HIP events around back-to-back calls on one stream after 3 warm-up calls of each way, median of 7 runs, the "
                           "two ways alternating run by run in one process; spread = (max - min) / median of a side's 7 runs",
                  device=torch.cuda.get_device_name(0), rows=rows)
    with open(os.path.join(out_dir, "monitor.json"), "w") as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ddpg_population"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    sys.exit(main(args.out))
