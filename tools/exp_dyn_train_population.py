#!/usr/bin/env python3
"""Measurements of the grouped dynamics-model step: ssc_mlp_train_steps_many against the per-model
ssc_mlp_train_steps calls it replaces, and the single-model call against another build of the library.

    python tools/exp_dyn_train_population.py steps  --out profiles/dyn_train_population
    python tools/exp_dyn_train_population.py single --other-lib PATH/libssc.so --out profiles/dyn_train_population

steps: P in {1, 2, 4, 16, 64} models of 1x32 and of 1x500 (in 3, out 2) at batch 512, 30 steps per call (one epoch of the
shipped training on ~15000 rows), and one population of 16 models of mixed widths.  "grouped" is one many-call, "per_model"
the same models, data sets and index streams through P single calls one after the other -- the library's own alternative
path, what DynamicsModelPopulation falls back to.  Device events around CALLS back-to-back calls on one stream after a warm-up
of every shape, the two arms alternating window by window in one process, WINDOWS windows per arm.  A case is WON only if the
slowest grouped window beats the fastest per-model window.  -> steps.json, with the smallest P that wins for every shape.

single: 1x32, 1x500 and 2x500 at batch 512, 30 steps per call, this build's ssc_mlp_train_steps against the same entry point
of --other-lib (the parent commit's build), both loaded into this process and alternating window by window.  "inside" says
whether this build's median lies within the other build's own window-to-window range.  -> single.json."""
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

BATCH, STEPS, ROWS = 512, 30, 16384
CALLS, WINDOWS, WARMUP = 4, 9, 3


class RawModel:
    """one model's device arrays, its descriptor, data set, index stream, losses and workspace"""

    def __init__(self, dims, seed, batch=BATCH, steps=STEPS):
        rng = np.random.default_rng(seed)
        dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
        L = len(dims) - 1
        self.dims, self.batch, self.steps = dims, batch, steps
        self.W = [dev(rng.normal(size=(dims[l], dims[l + 1])) * np.sqrt(2.0 / (dims[l] + dims[l + 1]))) for l in range(L)]
        self.b = [dev(rng.normal(size=dims[l + 1]) * 0.1) for l in range(L)]
        self.m = [[torch.zeros_like(t) for t in self.W + self.b] for _ in range(2)]
        self.t = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.X, self.Z = dev(rng.normal(size=(ROWS, dims[0]))), dev(0.5 * rng.normal(size=(ROWS, dims[-1])))
        self.idx = dev(rng.integers(0, ROWS, (steps, batch)), torch.int32)
        self.loss = torch.zeros(steps, device="cuda")
        d = _ffi.MlpTrainDesc()
        d.n_layers = L
        for l in range(L + 1):
            d.dims[l] = dims[l]
        for l in range(L):
            d.W[l], d.b[l] = self.W[l].data_ptr(), self.b[l].data_ptr()
            d.mW[l], d.vW[l] = self.m[0][l].data_ptr(), self.m[1][l].data_ptr()
            d.mb[l], d.vb[l] = self.m[0][L + l].data_ptr(), self.m[1][L + l].data_ptr()
        d.adam_t = self.t.data_ptr()
        d.lr, d.beta1, d.beta2, d.epsilon = 1e-3, 0.9, 0.999, 1e-8
        self.desc = d
        self.ws = torch.empty(int(_ffi.lib().ssc_mlp_train_workspace_bytes(ctypes.byref(d), batch)), dtype=torch.uint8, device="cuda")

    def alone(self, lib):
        _ffi.check(lib.ssc_mlp_train_steps(ctypes.byref(self.desc), self.X.data_ptr(), self.Z.data_ptr(), self.idx.data_ptr(),
                                           self.batch, self.steps, self.loss.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                           _ffi.stream()))


class RawPopulation:
    def __init__(self, shapes, seed=0):
        self.models = [RawModel(dims, seed + p) for p, dims in enumerate(shapes)]
        self.items = (_ffi.MlpTrainManyItem * len(self.models))()
        for it, m in zip(self.items, self.models):
            it.net, it.d_X, it.d_Z, it.d_idx = m.desc, m.X.data_ptr(), m.Z.data_ptr(), m.idx.data_ptr()
            it.batch, it.n_steps, it.d_loss = m.batch, m.steps, m.loss.data_ptr()
            it.d_workspace, it.workspace_bytes = m.ws.data_ptr(), m.ws.numel()
        self.d_items = torch.frombuffer(bytearray(self.items), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()

    def grouped(self):
        _ffi.check(_ffi.lib().ssc_mlp_train_steps_many(ctypes.addressof(self.items), self.d_items.data_ptr(), len(self.models),
                                                       _ffi.stream()))

    def per_model(self):
        lib = _ffi.lib()
        for m in self.models:
            m.alone(lib)


def timed_pair(fa, fb, calls=CALLS, warmup=WARMUP, windows=WINDOWS):
    """ms per call of ``calls`` back-to-back calls of fa and of fb, alternating window by window"""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    per = ([], [])
    for _ in range(windows):
        for f, out in ((fa, per[0]), (fb, per[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / calls)
    stat = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / statistics.median(v),
                          us_per_step=1000.0 * statistics.median(v) / STEPS, windows=v)
    return stat(per[0]), stat(per[1])


def cmd_steps(args):
    cases = [("1x32", P, [(3, 32, 2)] * P) for P in (1, 2, 4, 16, 64)] + [("1x500", P, [(3, 500, 2)] * P) for P in (1, 2, 4, 16, 64)]
    widths = (32, 500, 64, 256, 100, 17, 500, 32, 128, 16, 300, 500, 32, 64, 1, 500)
    cases.append(("mixed", len(widths), [(3, h, 2) for h in widths]))
    out = dict(method="device events around %d back-to-back calls of %d steps at batch %d, arms alternating window by window, %d windows "
                      "per arm after %d warm-up rounds; won = slowest grouped window < fastest per-model window" % (CALLS, STEPS, BATCH, WINDOWS, WARMUP),
               device=torch.cuda.get_device_name(0), cases=[])
    for name, P, shapes in cases:
        pop = RawPopulation(shapes)
        g, s = timed_pair(pop.grouped, pop.per_model)
        row = dict(shape=name, P=P, grouped=g, per_model=s, won=g["max_ms"] < s["min_ms"], ratio=s["median_ms"] / g["median_ms"])
        out["cases"].append(row)
        print("%-6s P=%-3d grouped %8.3f ms [%.3f, %.3f]  per-model %8.3f ms [%.3f, %.3f]  x%.2f %s" % (
            name, P, g["median_ms"], g["min_ms"], g["max_ms"], s["median_ms"], s["min_ms"], s["max_ms"], row["ratio"],
            "won" if row["won"] else "not won"), flush=True)
    out["smallest_winning_P"] = {}
    for name in ("1x32", "1x500"):
        rows = [r for r in out["cases"] if r["shape"] == name]
        wins = [r["P"] for r in rows if r["won"] and all(q["won"] for q in rows if q["P"] >= r["P"])]
        out["smallest_winning_P"][name] = min(wins) if wins else None
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "steps.json"), "w"), indent=1)
    print(json.dumps(out["smallest_winning_P"]))


def cmd_single(args):
    other = ctypes.CDLL(os.path.abspath(args.other_lib))
    other.ssc_mlp_train_steps.restype = ctypes.c_int
    other.ssc_mlp_train_steps.argtypes = _ffi._SIGNATURES["ssc_mlp_train_steps"][1]
    out = dict(method="this build's ssc_mlp_train_steps against --other-lib's, one process, %d calls of %d steps per window, arms "
                      "alternating, %d windows per arm" % (CALLS, STEPS, WINDOWS), device=torch.cuda.get_device_name(0), cases=[])
    for name, dims in (("1x32", (3, 32, 2)), ("1x500", (3, 500, 2)), ("2x500", (3, 500, 500, 2))):
        m = RawModel(dims, 7)
        this, oth = timed_pair(lambda: m.alone(_ffi.lib()), lambda: m.alone(other))
        inside = oth["min_ms"] <= this["median_ms"] <= oth["max_ms"] or this["median_ms"] <= oth["median_ms"]
        out["cases"].append(dict(shape=name, this=this, other=oth, inside=inside))
        print("%-6s this %8.4f ms [%.4f, %.4f] (%.2f us/step)  other %8.4f ms [%.4f, %.4f] (%.2f us/step)  %s" % (
            name, this["median_ms"], this["min_ms"], this["max_ms"], this["us_per_step"], oth["median_ms"], oth["min_ms"], oth["max_ms"],
            oth["us_per_step"], "inside" if inside else "OUTSIDE"), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "single.json"), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["steps", "single"])
    ap.add_argument("--out", default="profiles/dyn_train_population")
    ap.add_argument("--other-lib", default=None)
    a = ap.parse_args()
    {"steps": cmd_steps, "single": cmd_single}[a.cmd](a)
