"""Forward-simulation dispatch matrix of csrc/dyn_mfma.hip: the case list, each case's inputs, its fp64 reference and
bf16 emulation, the bf16 bound derived from the two, and the emulation mutants that bound must reject.  Shared by the
CPU mutant test (tests/test_oracle_networks.py) and the GPU tests (tests/test_gpu_sim_matrix.py); numpy + oracle only.

The bound.  ``ref`` = O.dyn_forward_sim in fp64, ``emu`` = the same with O.mlp_forward_bf16emu (the kernel's arithmetic
model).  e = max |emu - ref| is what bf16 rounding alone costs AT THIS CASE'S INPUTS; a result X is accepted when

    max |X - emu| <= C_BF16 * e        and        max |X - ref| <= (1 + C_BF16) * e

on three quantities, each with its own e: the whole trajectory S[0..H], the first step S[1] alone (no compounding) and
the per-step increments S[t+1] - S[t] (what the network produces; the states themselves are dominated by s0).
C_BF16 = 1: "the kernel is closer to its arithmetic model than the model is to fp64".  Every mutant of ``mutants()``
moves at least one of the three by more than 2 * C_BF16 * e at every case (asserted on the CPU), so C_BF16 has a
factor of two of room below the smallest wrong kernel the list describes.

Metric.  Both the state metric and the increment metric are asserted; the increment metric is the one that separates
the mutants better at long horizons (a slip in one hidden unit is a per-step error of fixed size, while the state
error e grows with H), the state metric at H = 1 is the same number.
"""
import zlib
from collections import namedtuple

import numpy as np

from oracle import ssc_oracle as O

C_BF16 = 1.0

SEED, PID0, T_STEP = 77, 9, 5            # Philox key of the candidate action sequences (O.mpc_action_samples)
ACT_LOW = [-1.0, -0.5, 0.0, -2.0]
ACT_HIGH = [1.0, 0.5, 3.0, 2.0]


def make_mlp(rng, dims):
    """xavier-normal weights AND biases (feedforward_network.py:8,14-23)."""
    Ws = [rng.normal(size=(dims[i], dims[i + 1])) * np.sqrt(2.0 / (dims[i] + dims[i + 1])) for i in range(len(dims) - 1)]
    bs = [rng.normal(size=dims[i + 1]) * np.sqrt(2.0 / (1 + dims[i + 1])) for i in range(len(dims) - 1)]
    return [w.astype(np.float32) for w in Ws], [b.astype(np.float32) for b in bs]


def make_norm(rng, d, a):
    return dict(mean_x=rng.normal(size=d) * 0.3, std_x=rng.uniform(0.05, 1.0, d), mean_y=rng.normal(size=a) * 0.1,
                std_y=rng.uniform(0.3, 1.2, a), mean_z=rng.normal(size=d) * 0.01, std_z=rng.uniform(0.005, 0.05, d))


def norm32(norm):
    """the kernel receives fp32 statistics; give the oracle the same values"""
    return {k: np.asarray(v, np.float32).astype(np.float64) for k, v in norm.items()}


# name, network dims, horizon, problems x candidates (rows m = P * N), start state per "call" / "problem" / "row", and the
# instantiation dyn_mfma_sim_kernel<UT, NFC, BIASK, KIN, LAG, MODE, WALK> that run_mfma() selects for it (MODE: -1 = run-time
# flags, the LAG kernel has 0 = actions from memory and 1 = in-kernel sampling compiled in: "0|1" is one kernel per mode).
# walk_rows: the launch has P * N rows (more row tiles than CUs) and the oracle runs on a strided subset (walk_subset()).
SimCase = namedtuple("SimCase", "name dims H P N s0_kind inst walk")


def _c(name, dims, H, P, N, s0_kind, inst, walk=False):
    return SimCase(name, tuple(dims), H, P, N, s0_kind, inst, walk)


CASES = [
    # ---- one hidden layer: UT by depth, every KIN --------------------------------------------------------------
    _c("1x32_k4", (3, 32, 2), 20, 4, 250, "problem", "<1,1,false,4,false,-1,false>"),
    _c("1x20_k10", (7, 20, 5), 4, 1, 257, "call", "<1,1,false,10,false,-1,false>"),
    _c("1x32_k12", (12, 32, 8), 4, 5, 51, "row", "<1,1,false,12,false,-1,false>"),
    _c("1x100_k4", (4, 100, 3), 20, 16, 16, "problem", "<4,1,false,4,false,-1,false>"),
    _c("1x100_k10", (10, 100, 7), 4, 5, 51, "problem", "<4,1,false,10,false,-1,false>"),
    _c("1x64_k12", (12, 64, 8), 20, 1, 257, "call", "<4,1,false,12,false,-1,false>"),
    _c("1x500_k4", (4, 500, 3), 20, 4, 250, "row", "<16,1,false,4,false,-1,false>"),
    _c("1x300_k10", (10, 300, 7), 4, 16, 16, "problem", "<16,1,false,10,false,-1,false>"),
    _c("1x500_k12", (12, 500, 8), 4, 1, 255, "call", "<16,1,false,12,false,-1,false>"),
    # ---- two hidden layers, resident W2: UT 1 and 4, b2 in the contraction (BIASK) or not, every KIN -------------
    _c("2x30_k4", (4, 30, 30, 3), 20, 4, 250, "problem", "<1,2,true,4,false,-1,false>"),
    _c("2x31_k4", (3, 31, 31, 2), 4, 1, 255, "row", "<1,2,false,4,false,-1,false>"),
    _c("2x32_k4", (3, 32, 32, 2), 4, 1, 257, "call", "<1,2,false,4,false,-1,false>"),
    _c("2x24_k10", (7, 24, 24, 5), 4, 16, 16, "problem", "<1,2,true,10,false,-1,false>"),
    _c("2x31_k10", (10, 31, 31, 7), 20, 1, 1, "call", "<1,2,false,10,false,-1,false>"),
    _c("2x30_k12", (12, 30, 30, 8), 4, 5, 51, "row", "<1,2,true,12,false,-1,false>"),
    _c("2x32_k12", (12, 32, 32, 8), 4, 1, 256, "call", "<1,2,false,12,false,-1,false>"),
    _c("2x100_k4", (4, 100, 100, 3), 20, 5, 51, "row", "<4,2,true,4,false,-1,false>"),
    _c("2x127_k4", (4, 127, 127, 3), 4, 1, 257, "call", "<4,2,false,4,false,-1,false>"),
    _c("2x128_k4", (3, 128, 128, 2), 4, 16, 16, "problem", "<4,2,false,4,false,-1,false>"),
    _c("2x64_k10", (7, 64, 64, 5), 20, 4, 250, "problem", "<4,2,true,10,false,-1,false>"),
    _c("2x127_k10", (10, 127, 127, 7), 4, 1, 255, "call", "<4,2,false,10,false,-1,false>"),
    _c("2x100_k12", (12, 100, 100, 8), 4, 16, 16, "row", "<4,2,true,12,false,-1,false>"),
    _c("2x128_k12", (12, 128, 128, 8), 20, 1, 257, "call", "<4,2,false,12,false,-1,false>"),
    # ---- two hidden layers, streamed W2 (UT 16), 5..10 inputs: the 3-slot ring kernel ---------------------------------
    _c("2x500_k10", (10, 500, 500, 7), 20, 5, 51, "problem", "<16,2,true,10,false,-1,false>"),
    _c("2x512_k10", (10, 512, 512, 7), 4, 1, 257, "row", "<16,2,false,10,false,-1,false>"),
    # ---- the BASELINE shape: the 4-slot LAG kernel, one block per row tile ------------------------------------------
    _c("2x500_h20", (4, 500, 500, 3), 20, 4, 250, "problem", "<16,2,true,4,true,0|1,false>"),
    _c("2x500_h4", (4, 500, 500, 3), 4, 1, 257, "call", "<16,2,true,4,true,0|1,false>"),
    _c("2x500_h1", (4, 500, 500, 3), 1, 1, 255, "row", "<16,2,true,4,true,0|1,false>"),
    _c("2x500_m1", (3, 500, 500, 2), 4, 1, 1, "call", "<16,2,true,4,true,0|1,false>"),
    _c("2x510_k4", (3, 510, 510, 2), 4, 16, 16, "problem", "<16,2,true,4,true,0|1,false>"),
    _c("2x511_h20", (4, 511, 511, 3), 20, 1, 257, "call", "<16,2,false,4,true,0|1,false>"),
    _c("2x511_3to2", (3, 511, 511, 2), 4, 5, 51, "problem", "<16,2,false,4,true,0|1,false>"),
    _c("2x512_h20", (4, 512, 512, 3), 20, 4, 250, "problem", "<16,2,false,4,true,0|1,false>"),
    _c("2x512_h4", (3, 512, 512, 2), 4, 1, 256, "row", "<16,2,false,4,true,0|1,false>"),
    _c("2x512_h1", (4, 512, 512, 3), 1, 1, 1, "call", "<16,2,false,4,true,0|1,false>"),
    # ---- ... and walking over row tiles (more row tiles than CUs; the oracle runs on walk_subset()) ------------------
    _c("walk500_h20", (4, 500, 500, 3), 20, 9001, 16, "problem", "<16,2,true,4,true,0|1,true>", walk=True),
    _c("walk500_h1", (4, 500, 500, 3), 1, 9001, 16, "problem", "<16,2,true,4,true,0|1,true>", walk=True),
    _c("walk512_h20", (4, 512, 512, 3), 20, 9001, 16, "problem", "<16,2,false,4,true,0|1,true>", walk=True),
    _c("walk512_h1", (4, 512, 512, 3), 1, 9001, 16, "problem", "<16,2,false,4,true,0|1,true>", walk=True),
]
CASE_IDS = [c.name for c in CASES]

TILE_ROWS = 256
WALK_MAX_CUS = 256       # an MI355X has 256 CUs: the launch walks when it has more row tiles than that


def walk_subset(m):
    """Rows of a walking launch that meet the oracle: a stride over everything, the whole first wave of the first tile, the
    last (ragged) tile's first and last rows, and whole waves of tiles handed out by the shared counter (beyond 2 * n_cu)."""
    n_tiles = (m + TILE_ROWS - 1) // TILE_ROWS
    assert n_tiles > 2 * WALK_MAX_CUS + 2 and m % TILE_ROWS not in (0, 1)
    last0 = (n_tiles - 1) * TILE_ROWS
    late = (2 * WALK_MAX_CUS + 1) * TILE_ROWS
    rows = np.concatenate([np.arange(0, m, 149), np.arange(32), np.arange(last0, last0 + 32), np.arange(m - 33, m),
                           np.arange(late + 96, late + 128), np.arange(late + TILE_ROWS - 16, late + TILE_ROWS + 16)])
    return np.unique(rows)


def action_rows(rows, N, H, act_dim, seed=SEED, pid0=PID0, t=T_STEP):
    """O.mpc_action_samples for arbitrary rows of a [P * N] batch (row r = sample r % N of problem pid0 + r // N): the same
    Philox words, keyed per row instead of per problem (the CPU test holds the two to each other)."""
    rows = np.asarray(rows, np.int64)
    per = (H * act_dim + 3) // 4
    out = np.empty((rows.size, H, act_dim), np.float32)
    ids = ((np.uint64(pid0) + (rows // N).astype(np.uint64)) << np.uint64(32)) + (rows % N).astype(np.uint64)
    for c in range(per):
        w = O.rng_words(seed, ids, np.uint64(t) * np.uint64(per) + np.uint64(c), O.TAG_MPC)
        for j in range(4):
            f = c * 4 + j
            if f < H * act_dim:
                h, a = divmod(f, act_dim)
                out[:, h, a] = O.uniform_f32(w[j], np.float32(ACT_LOW[a]), np.float32(ACT_HIGH[a]))
    return out


def hidden_activity(x, Ws, bs):
    """fp64 hidden activations of every hidden layer for network inputs x: list of [rows, depth]"""
    h, acts = np.asarray(x, np.float64), []
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = np.maximum(h @ np.asarray(W, np.float64) + np.asarray(b, np.float64), 0.0)
        acts.append(h)
    return acts


SimInputs = namedtuple("SimInputs", "case Ws bs norm d a low high m rows s0 s0_rows A x0")


def build_inputs(case):
    """Deterministic inputs of a case.  ``s0`` is what the wrapper receives ([d], [P, d] or [m, d]); ``rows`` the rows that
    meet the oracle (all of them unless the case walks), ``s0_rows`` / ``A`` their start states and action sequences."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    dims = case.dims
    d, a = dims[-1], dims[0] - dims[-1]
    Ws, bs = make_mlp(rng, dims)
    norm = make_norm(rng, d, a)
    m = case.P * case.N
    if case.s0_kind == "call":
        s0 = (rng.normal(size=d) * 0.3).astype(np.float32)
    elif case.s0_kind == "problem":
        s0 = (rng.normal(size=(case.P, d)) * 0.3).astype(np.float32)
    else:
        s0 = (rng.normal(size=(m, d)) * 0.3).astype(np.float32)
    rows = walk_subset(m) if case.walk else np.arange(m)
    if case.s0_kind == "call":
        s0_rows = np.broadcast_to(s0, (rows.size, d)).copy()
    elif case.s0_kind == "problem":
        s0_rows = s0[rows // case.N]
    else:
        s0_rows = s0[rows]
    A = action_rows(rows, case.N, case.H, a)
    nm = norm32(norm)
    x0 = np.concatenate([O.normalise(s0_rows, nm["mean_x"], nm["std_x"]), O.normalise(A[:, 0, :], nm["mean_y"], nm["std_y"])], axis=1)
    # unit 0 and the last real unit (the one next to the padding) of every hidden layer are made active on every compared
    # row, by their bias: a mutant that loses one of them must be visible, and a unit that is dead on every row hides it
    h = x0
    for l in range(len(dims) - 2):
        pre = h @ Ws[l].astype(np.float64)
        for u in (0, dims[1] - 1):
            bs[l][u] = np.float32(max(float(bs[l][u]), 0.5 - float(pre[:, u].min())))
        h = np.maximum(pre + bs[l].astype(np.float64), 0.0)
    return SimInputs(case, Ws, bs, norm, d, a, ACT_LOW[:a], ACT_HIGH[:a], m, rows, s0, s0_rows, A, x0)


def simulate(inp, Ws=None, bs=None, norm=None, forward=None):
    """[H+1, rows, d] fp64 trajectories of the compared rows"""
    return O.dyn_forward_sim(inp.s0_rows, inp.A, norm32(norm if norm is not None else inp.norm), Ws if Ws is not None else inp.Ws,
                             bs if bs is not None else inp.bs, forward=forward)


def references(inp):
    """(ref, emu): the fp64 oracle and the bf16 emulation at the case's inputs"""
    return simulate(inp), simulate(inp, forward=O.mlp_forward_bf16emu)


Bf16Error = namedtuple("Bf16Error", "traj t1 inc")


def bf16_error(ref, emu):
    """e_bf16 of the three compared quantities: whole trajectory, first step alone, per-step increments"""
    return Bf16Error(float(np.max(np.abs(emu - ref))), float(np.max(np.abs(emu[1] - ref[1]))),
                     float(np.max(np.abs(np.diff(emu, axis=0) - np.diff(ref, axis=0)))))


def bound_ratios(X, ref, emu, e=None):
    """max |X - emu| / e and max |X - ref| / e for the three quantities: dict of six numbers"""
    e = e or bf16_error(ref, emu)
    X = np.asarray(X, np.float64)
    dX, dr, de = np.diff(X, axis=0), np.diff(ref, axis=0), np.diff(emu, axis=0)
    return dict(emu_traj=np.max(np.abs(X - emu)) / e.traj, ref_traj=np.max(np.abs(X - ref)) / e.traj,
                emu_t1=np.max(np.abs(X[1] - emu[1])) / e.t1, ref_t1=np.max(np.abs(X[1] - ref[1])) / e.t1,
                emu_inc=np.max(np.abs(dX - de)) / e.inc, ref_inc=np.max(np.abs(dX - dr)) / e.inc)


def within_bf16_bound(r, c=C_BF16):
    return all(np.isfinite(v) and v <= (c if k.startswith("emu") else 1.0 + c) for k, v in r.items())


def mutant_separation(r):
    """how far a mutant sits from the emulation, in units of e: the largest of the three emu ratios (it breaks the bound
    as soon as one of them exceeds c)"""
    return max(r["emu_traj"], r["emu_t1"], r["emu_inc"])


def _live_units(act):
    """hidden units active on at least a quarter of the rows, most often active first"""
    frac = (act > 0).mean(axis=0)
    order = np.argsort(-frac, kind="stable")
    return [int(u) for u in order if frac[u] >= 0.25]


def _swap_pair(act, W_out):
    """two live units whose exchange matters: among the 16 most often active ones, the pair with the largest
    mean |h_u - h_v| * max |W_out[u] - W_out[v]| (picked from the data, not by index)"""
    live = _live_units(act)[:16]
    assert len(live) >= 2, "fewer than two live hidden units"
    best, pair = -1.0, None
    for i, u in enumerate(live):
        for v in live[i + 1:]:
            s = np.mean(np.abs(act[:, u] - act[:, v])) * np.max(np.abs(W_out[u] - W_out[v]))
            if s > best:
                best, pair = s, (u, v)
    return pair


def mutants(inp):
    """The ways a kernel goes wrong, as (name, Ws, bs, norm) of an emulation that computes the wrong thing:
    fragment-permutation slips (two live hidden units' outgoing rows swapped, last hidden layer and W2), padding slips (a
    live unit among the last 32 - depth % 32 real ones dropped, and unit 0, in each hidden layer), one network input's
    normalisation skipped, the last action dimension ignored, std_z of one output applied to another."""
    Ws, bs, norm = inp.Ws, inp.bs, inp.norm
    acts = hidden_activity(inp.x0, Ws, bs)
    depth = inp.case.dims[1]
    tail = list(range(depth - (32 - depth % 32), depth))
    out = []

    def with_W(l, edit):
        W2 = [w.copy() for w in Ws]
        edit(W2[l])
        return W2

    def swap(u, v):
        def f(W):
            W[[u, v]] = W[[v, u]]
        return f

    def drop(u):
        def f(W):
            W[u] = 0.0
        return f

    for l, act in enumerate(acts):                    # hidden layer l feeds Ws[l + 1]
        tag = "last" if l == len(acts) - 1 else "w2"
        u, v = _swap_pair(act, np.asarray(Ws[l + 1], np.float64))
        out.append((f"swap_{tag}_{u}_{v}", with_W(l + 1, swap(u, v)), bs, norm))
        live = _live_units(act)
        live_tail = [t for t in live if t in tail]
        assert live_tail and 0 in live, (inp.case.name, l, "the tail units / unit 0 are dead at these inputs")
        # a padding slip loses every unit of the last k-step: the live one that carries most is the one that shows it
        W_out = np.abs(np.asarray(Ws[l + 1], np.float64)).max(axis=1)
        t = max(live_tail, key=lambda q: act[:, q].mean() * W_out[q])
        out.append((f"drop_{tag}_tail_{t}", with_W(l + 1, drop(t)), bs, norm))
        out.append((f"drop_{tag}_unit0", with_W(l + 1, drop(0)), bs, norm))
    # one state input fed raw: the one whose z-score differs most from the raw value
    nm = norm32(norm)
    j = int(np.argmax(np.mean(np.abs(inp.x0[:, :inp.d] - inp.s0_rows), axis=0)))
    n2 = {k: np.array(v, np.float64) for k, v in nm.items()}
    n2["mean_x"][j], n2["std_x"][j] = 0.0, 1.0
    out.append((f"skip_norm_x{j}", Ws, bs, n2))
    out.append(("ignore_last_action", with_W(0, drop(inp.case.dims[0] - 1)), bs, norm))
    n3 = {k: np.array(v, np.float64) for k, v in nm.items()}
    n3["std_z"] = np.roll(n3["std_z"], 1)
    out.append(("std_z_shifted", Ws, bs, n3))
    return out
