#!/usr/bin/env python3
"""Measurements of the population forward simulation of bf16-MFMA models: ssc_mpc_forward_sim_many_mfma
against what it replaces, the whole MPC step of a NavigatorPopulation of class-default 1x500 models against per-seed
NavigatorBatch graphs, and the single-model MFMA kernels against another build of the library.  Protocol of
tools/exp_nav_population.py (NOTEBOOK section 24): one session, all arms in one process on the same models, device events
around a window of back-to-back calls, arms alternating window by window after warm-up windows, median [min, max]; a case is
WON only if the slowest grouped window beats the fastest window of every other arm.

    python tools/exp_nav_population_mfma.py sim    --out profiles/nav_population
    python tools/exp_nav_population_mfma.py step   --out profiles/nav_population
    python tools/exp_nav_population_mfma.py single --other-lib PATH/libssc.so --out profiles/nav_population

sim: P in {1, 2, 4, 16, 64} models of bf16 1x500 and of bf16 1x32 (in 3, out 2), 16 problems x 16 candidates per model (one
row tile each) and 1 problem x 5000 candidates, H = 4.  Arms: "grouped" = one many-call over one [H+1, P m_p, d] buffer;
"population_alone" = what DynamicsModelPopulation did before (each model's own call into a scratch, then a strided copy into
the shared buffer); "per_model" = plain own calls on own buffers.  -> mfma_sim.json with the smallest P that wins at every
shape (NAV_POPULATION_MFMA_MIN_GROUP).

step: graph replay of VecEnv.rollout(K, MpcPolicy(..)): 16 seeds x 16 envs x 16 candidates of 1x500 models in ONE
NavigatorPopulation against 16 (VecEnv, NavigatorBatch) graphs replayed one after the other.  -> mfma_step.json.

single: ssc_mpc_forward_sim(.., SSC_PREC_BF16_MFMA_PREPARED) at BASELINE config 4 (65 536 rows, 2x500, in 4, out 3, H = 4) and
at 1x500 with 5000 rows, this build against --other-lib (the parent commit's build), both loaded into this process on the
same packed image.  "inside": this build's median lies within the other build's own window range (or below it).
-> mfma_single.json."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from smartstartcontinuous_amd import _ffi  # noqa: E402
from smartstartcontinuous_amd import navigator as nav  # noqa: E402

H = 4
CALLS, WINDOWS, WARMUP = 50, 9, 3


def make_model(dims, seed):
    rng = np.random.default_rng(seed)
    d, a = dims[-1], dims[0] - dims[-1]
    n = len(dims) - 1
    Ws = [(rng.normal(size=(dims[l], dims[l + 1])) * np.sqrt(2.0 / (dims[l] + dims[l + 1]))).astype(np.float32) for l in range(n)]
    bs = [(rng.normal(size=dims[l + 1]) * 0.1).astype(np.float32) for l in range(n)]
    norm = dict(mean_x=rng.normal(size=d) * 0.3, std_x=rng.uniform(0.05, 1.0, d), mean_y=rng.normal(size=a) * 0.1,
                std_y=rng.uniform(0.3, 1.2, a), mean_z=rng.normal(size=d) * 0.01, std_z=rng.uniform(0.005, 0.05, d))
    return nav.DynamicsModel(Ws, bs, norm, state_dim=d, act_dim=a, precision="bf16_mfma")


class SimPopulation:
    """P models with `problems` problems x N candidates each: one shared buffer for the many-call, own buffers for the own calls"""

    def __init__(self, dims, P, problems, N):
        self.models = [make_model(dims, 100 + p) for p in range(P)]
        self.P, self.E, self.N, self.d, self.a = P, problems, N, dims[-1], dims[0] - dims[-1]
        d, a = self.d, self.a
        m_p, M = problems * N, P * problems * N
        rng = np.random.default_rng(5)
        self.s0 = torch.as_tensor((rng.normal(size=(P * problems, d)) * 0.3).astype(np.float32), device="cuda")
        self.S, self.Aout = torch.empty((H + 1, M, d), device="cuda"), torch.empty((M, H, a), device="cuda")
        self.S_p = [torch.empty((H + 1, m_p, d), device="cuda") for _ in range(P)]
        self.A_p = [torch.empty((m_p, H, a), device="cuda") for _ in range(P)]
        low, high = [-1.0] * a, [1.0] * a
        self.sp = nav.mpc_sampling(N, low, high, 7, 0, 3)
        self.sp_p = [nav.mpc_sampling(N, low, high, 7, p * problems, 3) for p in range(P)]
        self.images = [m._mfma_image() for m in self.models]
        self.items = (_ffi.MpcSimManyMfmaItem * P)()
        for p, (it, m, img) in enumerate(zip(self.items, self.models, self.images)):
            it.mlp, it.d_image, it.image_bytes, it.problem0, it.n_problems = m.desc, img.data_ptr(), img.numel(), p * problems, problems
        self.d_items = torch.frombuffer(bytearray(self.items), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()

    def grouped(self):
        _ffi.check(_ffi.lib().ssc_mpc_forward_sim_many_mfma(ctypes.addressof(self.items), self.d_items.data_ptr(), self.P,
                                                            ctypes.byref(self.sp), self.P * self.E * self.N, H, self.d, self.a,
                                                            self.s0.data_ptr(), self.P * self.E, self.Aout.data_ptr(),
                                                            self.S.data_ptr(), _ffi.stream()))

    def own_call(self, p, A_ptr, lib=None):
        lib, E, m = lib or _ffi.lib(), self.E, self.models[p]
        _ffi.check(lib.ssc_mpc_forward_sim(ctypes.byref(m.desc), ctypes.byref(m.norm), ctypes.byref(self.sp_p[p]), E * self.N, H,
                                           self.d, self.a, self.s0.data_ptr() + 4 * self.d * E * p, E, A_ptr, self.S_p[p].data_ptr(),
                                           _ffi.SSC_PREC_BF16_MFMA_PREPARED, self.images[p].data_ptr(), self.images[p].numel(),
                                           _ffi.stream()))

    def per_model(self, lib=None):
        for p in range(self.P):
            self.own_call(p, self.A_p[p].data_ptr(), lib)

    def population_alone(self):
        m_p = self.E * self.N
        for p in range(self.P):
            self.own_call(p, self.Aout.data_ptr() + 4 * p * m_p * H * self.a)
            self.S[:, p * m_p:(p + 1) * m_p].copy_(self.S_p[p])

    def same_bits(self):
        self.S.fill_(-1.0)
        self.Aout.fill_(-1.0)
        self.grouped()
        self.per_model()
        torch.cuda.synchronize()
        m_p = self.E * self.N
        return all(torch.equal(self.S[:, p * m_p:(p + 1) * m_p], self.S_p[p]) and torch.equal(self.Aout[p * m_p:(p + 1) * m_p], self.A_p[p])
                   for p in range(self.P))


def timed_arms(fs, calls=CALLS, warmup=WARMUP, windows=WINDOWS):
    """ms per call of ``calls`` back-to-back calls of every arm, the arms alternating window by window after warm-up windows"""
    per = [[] for _ in fs]
    for w in range(warmup + windows):
        for f, out in zip(fs, per):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            torch.cuda.synchronize()
            if w >= warmup:
                out.append(a.elapsed_time(b) / calls)
    return [dict(median_us=1000 * statistics.median(v), min_us=1000 * min(v), max_us=1000 * max(v), windows_ms=v) for v in per]


def method(what):
    return ("%s; device events around %d back-to-back calls, arms alternating window by window, %d windows per arm after %d "
            "warm-up windows; won = slowest window of the first arm < fastest window of every other arm" % (what, CALLS, WINDOWS, WARMUP))


SHAPES = (("16x16", 16, 16), ("1x5000", 1, 5000))
NETS = (("1x500", (3, 500, 2)), ("1x32", (3, 32, 2)))
SIZES = (1, 2, 4, 16, 64)


def cmd_sim(args):
    out = dict(method=method("one ssc_mpc_forward_sim_many_mfma against P own prepared-MFMA calls plus strided copies "
                             "(population_alone) and against P own calls on own buffers (per_model), H = %d" % H),
               device=torch.cuda.get_device_name(0), cases=[])
    for net, dims in NETS:
        for shape, E, N in SHAPES:
            for P in SIZES:
                pop = SimPopulation(dims, P, E, N)
                same = pop.same_bits()
                g, y, s = timed_arms([pop.grouped, pop.population_alone, pop.per_model])
                won = g["max_us"] < min(y["min_us"], s["min_us"])
                row = dict(net=net, shape=shape, P=P, rows=P * E * N, same_bits=same, grouped=g, population_alone=y, per_model=s,
                           won=won, ratio_population_alone=y["median_us"] / g["median_us"], ratio_per_model=s["median_us"] / g["median_us"])
                out["cases"].append(row)
                print("%-5s %-6s P=%-3d grouped %8.1f us [%.1f, %.1f]  population-alone %8.1f us [%.1f, %.1f]  per-model %8.1f us "
                      "[%.1f, %.1f]  x%.2f / x%.2f %s%s" % (
                          net, shape, P, g["median_us"], g["min_us"], g["max_us"], y["median_us"], y["min_us"], y["max_us"],
                          s["median_us"], s["min_us"], s["max_us"], row["ratio_population_alone"], row["ratio_per_model"],
                          "won" if won else "LOST", "" if same else "  BITS DIFFER"), flush=True)
                del pop
    # the smallest P from which every larger measured P wins, at EVERY net and shape; never below 2
    ok = [P for P in SIZES if P >= 2 and all(r["won"] for r in out["cases"] if r["P"] >= P)]
    out["smallest_P_winning_everywhere"] = min(ok) if ok else None
    out["min_group"] = min(ok) if ok else max(SIZES) + 1
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "mfma_sim.json"), "w"), indent=1)
    print(json.dumps(dict(smallest_P_winning_everywhere=out["smallest_P_winning_everywhere"], min_group=out["min_group"])))


def cmd_step(args):
    import smartstartcontinuous_amd as ssc
    P, E, N, K, D = 16, 16, 16, 32, 2
    rng = np.random.default_rng(3)
    paths = [np.cumsum(rng.normal(scale=[0.02, 0.004], size=(12, D)), axis=0) + [-0.5, 0.0] for _ in range(P * E)]
    radii = [np.array([0.05, 0.01])] * (P * E)
    lefts = [np.concatenate([np.cumsum(np.linalg.norm(np.diff(p, axis=0) / radii[0], axis=1)[::-1])[::-1], [0.0]]) for p in paths]
    models = [make_model((3, 500, 2), 100 + p) for p in range(P)]
    kw = dict(num_control_samples=N, horizon=H, seed=4)

    env = ssc.VecEnv("MountainCarContinuous-v0", P * E, seed=21)
    env.reset()
    pop = nav.NavigatorPopulation(models, nav.MpcProblemSet(paths, lefts, radii, [0] * (P * E)), E, **kw)
    pol = ssc.MpcPolicy(pop, graph=True)
    chunk = env.rollout(K, pol)
    singles = []
    for p in range(P):
        e = ssc.VecEnv("MountainCarContinuous-v0", E, seed=21, env_id0=E * p)
        e.reset()
        sl = slice(E * p, E * (p + 1))
        b = nav.NavigatorBatch(models[p], nav.MpcProblemSet(paths[sl], lefts[sl], radii[sl], [0] * E), problem_id0=E * p, **kw)
        singles.append((e, ssc.MpcPolicy(b, graph=True)))
    outs = [e.rollout(K, pl) for e, pl in singles]
    torch.cuda.synchronize()
    same = all(torch.equal(chunk.act[:, E * p:E * (p + 1)], outs[p].act) for p in range(P))

    def grouped():
        env.rollout(K, pol, out=chunk)

    def per_seed():
        for (e, pl), o in zip(singles, outs):
            e.rollout(K, pl, out=o)
    g, s = timed_arms([grouped, per_seed], calls=4)
    for st in (g, s):
        for k in ("median_us", "min_us", "max_us"):
            st[k + "_per_step"] = st.pop(k) / K
    won = g["max_us_per_step"] < s["min_us_per_step"]
    out = dict(method=method("graph replay of rollout(%d, MpcPolicy): one NavigatorPopulation of %d seeds x %d envs x %d candidates, "
                             "bf16 1x500 models, against %d NavigatorBatch graphs replayed one after the other; per MPC step of all "
                             "seeds; 4 rollouts per window" % (K, P, E, N, P)),
               device=torch.cuda.get_device_name(0), same_actions=same, sim_ways=pop.sim_ways, grouped=g, per_seed=s, won=won,
               ratio=s["median_us_per_step"] / g["median_us_per_step"])
    print("step  P=%d x %d envs (%s): population %.1f us/step [%.1f, %.1f]  per-seed graphs %.1f us/step [%.1f, %.1f]  x%.2f %s%s" % (
        P, E, pop.sim_ways[0], g["median_us_per_step"], g["min_us_per_step"], g["max_us_per_step"], s["median_us_per_step"],
        s["min_us_per_step"], s["max_us_per_step"], out["ratio"], "won" if won else "LOST", "" if same else "  ACTIONS DIFFER"), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "mfma_step.json"), "w"), indent=1)


def cmd_single(args):
    other = ctypes.CDLL(os.path.abspath(args.other_lib))
    other.ssc_mpc_forward_sim.restype = ctypes.c_int
    other.ssc_mpc_forward_sim.argtypes = _ffi._SIGNATURES["ssc_mpc_forward_sim"][1]
    out = dict(method=method("this build's ssc_mpc_forward_sim(.., BF16_MFMA_PREPARED) against --other-lib's on the same packed "
                             "image, H = %d" % H), device=torch.cuda.get_device_name(0), cases=[])
    if args.static and os.path.exists(args.static):
        out["static"] = json.load(open(args.static))
    for name, dims, E, N in (("config 4: 65536 rows (4096 x 16), 2x500 4->3", (4, 500, 500, 3), 4096, 16),
                             ("5000 rows (1 x 5000), 1x500 3->2", (3, 500, 2), 1, 5000),
                             ("256 rows (16 x 16), 1x500 3->2", (3, 500, 2), 16, 16)):
        pop = SimPopulation(dims, 1, E, N)
        this, oth = timed_arms([lambda: pop.per_model(_ffi.lib()), lambda: pop.per_model(other)])
        pop.per_model(_ffi.lib())
        mine = pop.S_p[0].clone()
        pop.per_model(other)
        torch.cuda.synchronize()
        same = torch.equal(mine, pop.S_p[0])
        inside = this["median_us"] <= oth["max_us"]
        out["cases"].append(dict(shape=name, this=this, other=oth, inside=inside, same_bits=same))
        print("%-46s this %8.2f us [%.2f, %.2f]  other %8.2f us [%.2f, %.2f]  %s%s" % (
            name, this["median_us"], this["min_us"], this["max_us"], oth["median_us"], oth["min_us"], oth["max_us"],
            "inside" if inside else "OUTSIDE", "" if same else "  BITS DIFFER"), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "mfma_single.json"), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["sim", "step", "single"])
    ap.add_argument("--out", default="profiles/nav_population")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--static", default=None, help="single: a JSON file with the compiler's resource-usage comparison to embed")
    a = ap.parse_args()
    {"sim": cmd_sim, "step": cmd_step, "single": cmd_single}[a.cmd](a)
