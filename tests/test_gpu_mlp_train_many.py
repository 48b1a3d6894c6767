"""ssc_mlp_train_steps_many (csrc/dyn_train.hip: mlp_train_fused_many_kernel<3,2 | 4,3 | 12,8>, fused_begin_many_kernel) and
its wrappers: a population of dynamics models trained with one launch per step ends up, bit for bit, where every model's own
ssc_mlp_train_steps call leaves it -- every layer's W, b and four moment arrays, adam_t, the losses and the whole workspace,
compared as bytes against a twin that was trained alone from the same start.

The populations are built from the small shapes of tests/dyn_train_cases.py: one per kernel instantiation, with surplus
workgroups beside a G = 17 model, partial row tiles, hd < hd_pad, S = 1 and S > 1, more than 64 KB of LDS next to small
models, parameter counts above and below one trip of the Adam loop, unequal step counts and a model without steps.  Every
workspace is exactly as large as ssc_mlp_train_workspace_bytes reports, and it, the losses and every other array lie between
patterned guard bands."""
import ctypes

import numpy as np
import pytest

from tests import dyn_train_cases as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD, PAT, WS_PAT = 256, 0xA5, 0xC3
STATE = [k + str(l) for l in range(2) for k in ("W", "b", "mW", "vW", "mb", "vb")] + ["adam_t", "loss", "ws"]

# (case of tests/dyn_train_cases.py, steps) per model; 0 steps: the model is skipped
POPULATIONS = {
    "<3,2>": [("f32_h32_b512", 3), ("f32_h1_b1", 1), ("f32_h16_b31", 4), ("f32_h17_b33", 2), ("f32_h500_b513", 3), ("f32_h17_b33", 0)],
    "<4,3>": [("f43_h33_b32", 2), ("f43_h100_b544", 3), ("f43_h256_b33", 1), ("f43_h257_b1", 4)],
    "<12,8>": [("f128_h256_b33", 3), ("f128_h16_b513", 2), ("f128_h512_b31", 4), ("f128_h1_b33", 1)],
}


@pytest.fixture(scope="module")
def ffi():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Net:
    """One model's device arrays, each between guard bands; the workspace exactly as large as the library asks for."""

    def __init__(self, ffi, case_name, lr=D.LR, share=None, scale=1.0):
        case = D.CASE_BY_NAME[case_name]
        assert case.path == "fused"
        d = D.case_data(case)
        self.case, self.B, self.raw, self.view = case, case.B, {}, {}
        if share is None:
            self.add("X", d["X"]), self.add("Z", d["Z"]), self.add("idx", d["idx"])
        else:           # the data set and the index stream of another model: only read, so they may coincide
            for k in ("X", "Z", "idx"):
                self.view[k] = share.view[k]
        self.add("loss", np.full(4, -7.0, np.float32)), self.add("adam_t", np.zeros(1, np.int32))
        desc = ffi.MlpTrainDesc()
        desc.n_layers = 2
        for l in range(3):
            desc.dims[l] = case.dims[l]
        for l in range(2):
            self.add("W%d" % l, d["Ws"][l] * np.float32(scale)), self.add("b%d" % l, d["bs"][l] * np.float32(scale))
            for k, like in (("mW", d["Ws"][l]), ("vW", d["Ws"][l]), ("mb", d["bs"][l]), ("vb", d["bs"][l])):
                self.add("%s%d" % (k, l), np.zeros_like(like))
            for k in ("W", "b", "mW", "vW", "mb", "vb"):
                getattr(desc, k)[l] = self.view["%s%d" % (k, l)].data_ptr()
        desc.adam_t = self.view["adam_t"].data_ptr()
        desc.lr, desc.beta1, desc.beta2, desc.epsilon = lr, D.BETA1, D.BETA2, D.EPSILON
        self.desc = desc
        self.need = int(ffi.lib().ssc_mlp_train_workspace_bytes(ctypes.byref(desc), self.B))
        assert self.need > 0 and self.need % 4 == 0
        raw = torch.full((GUARD + self.need + GUARD,), PAT, dtype=torch.uint8, device="cuda")
        raw[GUARD:GUARD + self.need] = WS_PAT
        self.raw["ws"], self.view["ws"] = raw, raw[GUARD:GUARD + self.need]

    def add(self, name, arr):
        arr = np.array(arr, order="C")
        dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}[arr.dtype]
        raw = torch.full((GUARD + arr.nbytes + GUARD,), PAT, dtype=torch.uint8, device="cuda")
        raw[GUARD:GUARD + arr.nbytes].copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1)))
        self.raw[name], self.view[name] = raw, raw[GUARD:GUARD + arr.nbytes].view(dtype).view(arr.shape)

    def guards_intact(self):
        return [k for k, raw in self.raw.items() if not (bool((raw[:GUARD] == PAT).all()) and bool((raw[-GUARD:] == PAT).all()))]

    def state(self):
        return {k: self.view[k].cpu().numpy().tobytes() for k in STATE}

    def reads(self):
        return {k: self.view[k].cpu().numpy().tobytes() for k in ("X", "Z", "idx")}

    def alone(self, ffi, first, n_steps, with_loss=True):
        """the model's own call on rows idx[first : first + n_steps]"""
        ffi.check(ffi.lib().ssc_mlp_train_steps(
            ctypes.byref(self.desc), self.view["X"].data_ptr(), self.view["Z"].data_ptr(),
            self.view["idx"].data_ptr() + 4 * self.B * first, self.B, n_steps,
            self.view["loss"].data_ptr() + 4 * first if with_loss else None, self.view["ws"].data_ptr(), self.need, _stream()))

    def item(self, it, first, n_steps, with_loss=True):
        it.net = self.desc
        it.d_X, it.d_Z = self.view["X"].data_ptr(), self.view["Z"].data_ptr()
        it.d_idx, it.batch, it.n_steps = self.view["idx"].data_ptr() + 4 * self.B * first, self.B, n_steps
        it.d_loss = self.view["loss"].data_ptr() + 4 * first if with_loss else None
        it.d_workspace, it.workspace_bytes = self.view["ws"].data_ptr(), self.need


def together(ffi, nets, firsts, steps, with_loss=None):
    """one ssc_mlp_train_steps_many call over ``nets``"""
    items = (ffi.MlpTrainManyItem * len(nets))()
    for p, net in enumerate(nets):
        net.item(items[p], firsts[p], steps[p], True if with_loss is None else with_loss[p])
    dev = torch.empty(ctypes.sizeof(items), dtype=torch.uint8, device="cuda")
    dev.copy_(torch.from_numpy(np.frombuffer(bytes(items), np.uint8).copy()))
    ffi.check(ffi.lib().ssc_mlp_train_steps_many(ctypes.addressof(items), dev.data_ptr(), len(nets), _stream()))
    torch.cuda.synchronize()


def differing(a, b):
    return [k for k in a if a[k] != b[k]]


_TWINS = {}


def twins(ffi, cls):
    """every model of the class's population trained by its own call: computed once, never modified"""
    if cls not in _TWINS:
        out = []
        for name, n in POPULATIONS[cls]:
            net = Net(ffi, name)
            start = net.state()
            net.alone(ffi, 0, n)
            torch.cuda.synchronize()
            assert net.guards_intact() == []
            out.append((start, net.state()))
        _TWINS[cls] = out
    return _TWINS[cls]


def run_population(ffi, cls):
    nets = [Net(ffi, name) for name, _ in POPULATIONS[cls]]
    reads = [net.reads() for net in nets]
    steps = [n for _, n in POPULATIONS[cls]]
    together(ffi, nets, [0] * len(nets), steps)
    for p, net in enumerate(nets):
        assert net.guards_intact() == [], (cls, p)
        assert differing(reads[p], net.reads()) == [], (cls, p)
    return [net.state() for net in nets]


@pytest.mark.parametrize("cls", list(POPULATIONS))
def test_population_equals_per_model_calls_bit_for_bit(ffi, cls):
    cases = [D.CASE_BY_NAME[name] for name, _ in POPULATIONS[cls]]
    assert {c.kernel for c in cases} == {cls}
    # what the population is there to cover (read off the case table, so a changed table fails here and not silently)
    Gs = [c.G for c in cases]
    assert max(Gs) == 17 and min(Gs) == 1                                  # surplus workgroups beside a G = 17 model
    assert any(c.B % 32 for c in cases) and any(c.dims[1] < c.hd_pad for c in cases)
    assert {c.S == 1 for c in cases} == {True, False} and {c.lds_optin for c in cases} == {True, False}
    assert any(c.P > 2048 for c in cases) and any(c.P < 2048 for c in cases)
    assert len({n for _, n in POPULATIONS[cls]}) > 2
    got, want = run_population(ffi, cls), twins(ffi, cls)
    for p, (state, (start, end)) in enumerate(zip(got, want)):
        assert differing(state, end) == [], (cls, p, POPULATIONS[cls][p])
        if POPULATIONS[cls][p][1] == 0:                                     # a model without steps: nothing of it is touched
            assert differing(state, start) == []
        else:
            assert state["b1"] != start["b1"] and state["adam_t"] == np.int32(POPULATIONS[cls][p][1]).tobytes()


def test_same_start_gives_the_same_bits_twice(ffi):
    first, second = run_population(ffi, "<3,2>"), run_population(ffi, "<3,2>")
    for p, (a, b) in enumerate(zip(first, second)):
        assert differing(a, b) == [], p


def test_two_many_calls_equal_two_single_calls_per_model(ffi):
    """the begin launch recomputes the bias-correction powers from adam_t > 0, like the second single call does"""
    names = [name for name, _ in POPULATIONS["<4,3>"]]
    steps1, steps2 = [2, 1, 2, 1], [2, 3, 1, 2]
    alone, many = [Net(ffi, n) for n in names], [Net(ffi, n) for n in names]
    for net, a, b in zip(alone, steps1, steps2):
        net.alone(ffi, 0, a)
        net.alone(ffi, a, b)
    torch.cuda.synchronize()
    together(ffi, many, [0] * 4, steps1)
    mid = [net.state() for net in many]
    together(ffi, many, steps1, steps2)
    for p, (a, m) in enumerate(zip(alone, many)):
        assert differing(a.state(), m.state()) == [], p
        assert m.state()["adam_t"] == np.int32(steps1[p] + steps2[p]).tobytes() and mid[p]["b1"] != m.state()["b1"]
        assert m.guards_intact() == []
    # ... and one longer single call is NOT the same thing: the powers advance by multiplication inside a call
    # (nothing is asserted about it; the contract is call for call)


def test_shared_reads_and_absent_losses(ffi):
    """X, Z and idx shared by two models with different weights and step sizes; d_loss NULL on some models"""
    def build():
        a = Net(ffi, "f32_h32_b512")
        b = Net(ffi, "f32_h32_b512", lr=3e-3, share=a, scale=0.5)
        c = Net(ffi, "f32_h17_b33")
        return [a, b, c]
    steps, with_loss = [3, 4, 2], [True, False, False]
    alone, many = build(), build()
    for net, n, wl in zip(alone, steps, with_loss):
        net.alone(ffi, 0, n, with_loss=wl)
    torch.cuda.synchronize()
    together(ffi, many, [0] * 3, steps, with_loss)
    states = [net.state() for net in many]
    for p, (a, s) in enumerate(zip(alone, states)):
        assert differing(a.state(), s) == [], p
        assert many[p].guards_intact() == []
    untouched = np.full(4, -7.0, np.float32).tobytes()
    assert states[1]["loss"] == untouched and states[2]["loss"] == untouched and states[0]["loss"] != untouched
    assert states[0]["W0"] != states[1]["W0"] and states[0]["loss"][:12] != alone[1].state()["loss"][:12]


# ---- the wrappers ----------------------------------------------------------------------------------------------------
def _models(nav, seed):
    """a mixed population: two <3,2> models, two <4,3> models and a 2 x 500 model outside the fused kernel"""
    rng = np.random.default_rng(seed)
    out = []
    for dims in ((3, 32, 2), (3, 17, 2), (4, 33, 3), (3, 100, 3), (3, 500, 500, 2)):
        Ws, bs = D.make_mlp(rng, dims)
        d = dims[-1]
        norm = dict(mean_x=np.zeros(d), std_x=np.ones(d), mean_y=np.zeros(dims[0] - d if dims[0] > d else 1),
                    std_y=np.ones(dims[0] - d if dims[0] > d else 1), mean_z=np.zeros(d), std_z=np.ones(d))
        out.append(nav.DynamicsModel(Ws, bs, norm, state_dim=d, act_dim=len(norm["mean_y"])))
    return out


def _model_bits(m):
    arrays = list(m.W) + list(m.b) + m._adam["mW"] + m._adam["vW"] + m._adam["mb"] + m._adam["vb"] + [m._adam["t"]]
    return [a.cpu().numpy().tobytes() for a in arrays]


def test_population_wrappers_equal_each_models_own_training(ffi):
    from smartstartcontinuous_amd import navigator as nav
    alone, grouped = _models(nav, 5), _models(nav, 5)
    pop = nav.DynamicsModelPopulation(grouped)
    assert pop.ways == ["fused<3,2>", "fused<3,2>", "fused<4,3>", "fused<4,3>", "alone"] and not pop.fused
    rng = np.random.default_rng(9)
    rows_old, rows_new = [700, 130, 300, 1200, 200], [90, 0, 40, 10, 64]
    data = []
    for m, n_old, n_new in zip(alone, rows_old, rows_new):
        data.append((rng.normal(size=(n_old, m.in_dim)).astype(np.float32), (0.5 * rng.normal(size=(n_old, m.out_dim))).astype(np.float32),
                     rng.normal(size=(n_new, m.in_dim)).astype(np.float32), (0.5 * rng.normal(size=(n_new, m.out_dim))).astype(np.float32)))
    # train_steps: per-model step counts and batch sizes, one model skipped
    Xs = [torch.as_tensor(d[0], device="cuda") for d in data]
    Zs = [torch.as_tensor(d[1], device="cuda") for d in data]
    shapes = [(3, 64), (2, 33), None, (4, 512), (2, 100)]
    idxs = [None if s is None else torch.as_tensor(rng.integers(0, n, s).astype(np.int32), device="cuda") for s, n in zip(shapes, rows_old)]
    lrs = [1e-3, 2e-3, 1e-3, 5e-4, 1e-3]
    want = [None if i is None else m.train_steps(X, Z, i, lr=lr) for m, X, Z, i, lr in zip(alone, Xs, Zs, idxs, lrs)]
    got = pop.train_steps(Xs, Zs, idxs, lr=lrs)
    assert got[2] is None
    for p in (0, 1, 3, 4):
        assert got[p].cpu().numpy().tobytes() == want[p].cpu().numpy().tobytes(), p
        assert _model_bits(alone[p]) == _model_bits(grouped[p]), p
        assert grouped[p]._image_stale
    # train: per-model epochs, batch sizes and fractions, every model with a generator of its own
    epochs, sizes, fracs = [3, 2, 2, 1, 2], [64, 32, 50, 512, 100], [0.25, 0.5, 0.0, 0.1, 0.3]
    want = [m.train(*d, e, f, batchsize=b, lr=lr, rng=np.random.RandomState(40 + p))
            for p, (m, d, e, f, b, lr) in enumerate(zip(alone, data, epochs, fracs, sizes, lrs))]
    got = pop.train(data, epochs, fracs, batchsize=sizes, lr=lrs, rngs=[np.random.RandomState(40 + p) for p in range(5)])
    assert got == want and all(isinstance(v, float) for v in got) and all(v > 0 for v in got)
    for p in range(5):
        assert _model_bits(alone[p]) == _model_bits(grouped[p]), p
    # the tables are uploaded again only when something in them changed
    uploads = []
    for di in pop._items.values():
        di.upload = (lambda f: lambda: (uploads.append(1), f())[1])(di.upload)
    pop.train_steps(Xs, Zs, idxs, lr=lrs)          # other index tensors than the last epoch's: both groups' tables travel
    assert len(uploads) == 2
    pop.train_steps(Xs, Zs, idxs, lr=lrs)          # the same pointers, shapes and step counts: nothing travels
    assert len(uploads) == 2
    with pytest.raises(ValueError):
        pop.train(data, epochs, fracs, rngs=None)


def test_train_dynamics_models_equals_each_agents_own_call(ffi, golden_dir, tmp_path):
    import smartstartcontinuous_amd as ssc
    from smartstartcontinuous_amd.agents import NND_MB_agent, train_dynamics_models
    g = np.load(f"{golden_dir}/mc_reference_rollouts.npz")
    data = dict(dataX=g["dataX"][:1100], dataY=g["dataY"][:1100], dataZ=g["dataZ"][:1100])
    env = ssc.make("MountainCarContinuous-v0")
    S, A = g["states_val"], g["controls_val"]

    def agents(root):
        out = []
        for seed in (3, 4):
            a = NND_MB_agent(env, None, horizon=4, num_control_samples=100, num_fc_layers=1, depth_fc_layers=32, training_data=data,
                             precision="f32", seed=seed, model_root=str(root), save_dir_name="seed%d" % seed)
            a.save_resulting_dynamics_model = True
            for ep in range(2):
                a.replay_buffer.start_new_episode(a)
                for t in range(40):
                    a.replay_buffer.add(a, S[ep + seed, t], A[ep + seed, t], 0.0, False, S[ep + seed, t + 1])
            out.append(a)
        return out
    own, pop = agents(tmp_path / "own"), agents(tmp_path / "pop")
    want = [a.train_dynamics_model(nEpoch=2, fraction_use_new=0.25, rng=np.random.RandomState(7 + p)) for p, a in enumerate(own)]
    got = train_dynamics_models(pop, [np.random.RandomState(7 + p) for p in range(2)], nEpoch=2, fraction_use_new=0.25)
    assert got == want and all(v > 0 for v in got)
    for a, b in zip(own, pop):
        assert _model_bits(a.dyn_model) == _model_bits(b.dyn_model)
    for seed in (3, 4):                                  # saving stays per agent
        assert (tmp_path / "pop" / ("seed%d" % seed) / "models" / "finalModel.npz").exists()
        assert (tmp_path / "pop" / ("seed%d" % seed) / "models" / "model_numTrain1.npz").exists()
    with pytest.raises(ValueError):
        train_dynamics_models(pop, np.random.RandomState(0))
