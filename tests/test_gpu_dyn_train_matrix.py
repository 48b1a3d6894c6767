"""Every path ssc_mlp_train_steps can launch (csrc/dyn_train.hip: mlp_train_fused_kernel<3,2 | 4,3 | 12,8> over every
hd_pad, the generic gather / forward / backward-data / weight-gradient chain at every depth and every class of its wave
split) held to the fp64 oracle by the bound of tests/dyn_train_cases.py.

Step 1 runs from zero moments, so the device gradient can be read back from the moments (Adam's scale invariance hides
its size from the parameters): |g - g64| <= C_GRAD * 2^-24 * A for every element of every parameter, a bound fixed on
the CPU from a float32 emulation (tests/test_dyn_train_cases_cpu.py), where the older checks of
tests/test_gpu_navigator.py accept a fiftieth of one step.  Steps 2-4 run in one call against the oracle carried along
at the project's existing tolerances.  Every buffer the call is given lies between patterned guard bands, the workspace
is exactly as large as ssc_mlp_train_workspace_bytes reports, and the same start gives the same bits twice.

The generic chain is reached through shapes the fused kernel refuses, never through the process-wide A/B switch."""
import ctypes

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import dyn_train_cases as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 256          # bytes on both sides of every buffer (keeps the 16-byte alignment of the data between them)
PAT, WS_PAT, WS_TAIL = 0xA5, 0xC3, 4096


@pytest.fixture(scope="module")
def ffi():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Buffers:
    """device arrays, each in the middle of a larger tensor whose other bytes hold PAT"""

    def __init__(self):
        self.raw, self.view = {}, {}

    def add(self, name, arr):
        arr = np.array(arr, order="C")          # (a writable copy: the case data is read-only)
        dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}[arr.dtype]
        raw = torch.full((GUARD + arr.nbytes + GUARD,), PAT, dtype=torch.uint8, device="cuda")
        raw[GUARD:GUARD + arr.nbytes].copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1)))
        self.raw[name] = raw
        self.view[name] = raw[GUARD:GUARD + arr.nbytes].view(dtype).view(arr.shape)
        assert self.view[name].data_ptr() % 16 == 0
        return self.view[name]

    def ptr(self, name, byte_offset=0):
        return ctypes.c_void_p(self.view[name].data_ptr() + byte_offset)

    def guards_intact(self):
        return [k for k, raw in self.raw.items() if not (bool((raw[:GUARD] == PAT).all()) and bool((raw[-GUARD:] == PAT).all()))]

    def snapshot(self, names):
        return {k: self.view[k].cpu().numpy().copy() for k in names}


def _state_names(L):
    return [k + str(l) for l in range(L) for k in ("W", "b", "mW", "vW", "mb", "vb")] + ["adam_t"]


def _execute(ffi, case, null_loss):
    """Step 1 from zero moments, then steps 2-4 in one call (d_loss = NULL if ``null_loss``), every buffer guarded.  Returns
    dict(s1, s4 = state after step 1 / step 4, loss [4] (steps 2-4: NaN-pattern untouched if null_loss), need)."""
    lib = ffi.lib()
    d = D.case_data(case)
    L, B = len(d["Ws"]), case.B
    buf = _Buffers()
    buf.add("X", d["X"]), buf.add("Z", d["Z"]), buf.add("idx", d["idx"])
    buf.add("loss", np.full(4, -7.0, np.float32)), buf.add("adam_t", np.zeros(1, np.int32))
    desc = ffi.MlpTrainDesc()
    desc.n_layers = L
    for l in range(L + 1):
        desc.dims[l] = case.dims[l]
    for l in range(L):
        buf.add("W%d" % l, d["Ws"][l]), buf.add("b%d" % l, d["bs"][l])
        for k, like in (("mW", d["Ws"][l]), ("vW", d["Ws"][l]), ("mb", d["bs"][l]), ("vb", d["bs"][l])):
            buf.add("%s%d" % (k, l), np.zeros_like(like))
        desc.W[l], desc.b[l] = buf.view["W%d" % l].data_ptr(), buf.view["b%d" % l].data_ptr()
        desc.mW[l], desc.vW[l] = buf.view["mW%d" % l].data_ptr(), buf.view["vW%d" % l].data_ptr()
        desc.mb[l], desc.vb[l] = buf.view["mb%d" % l].data_ptr(), buf.view["vb%d" % l].data_ptr()
    desc.adam_t = buf.view["adam_t"].data_ptr()
    desc.lr, desc.beta1, desc.beta2, desc.epsilon = D.LR, D.BETA1, D.BETA2, D.EPSILON
    names = _state_names(L)

    need = int(lib.ssc_mlp_train_workspace_bytes(ctypes.byref(desc), B))
    assert need > 0
    ws = torch.full((need + WS_TAIL,), WS_PAT, dtype=torch.uint8, device="cuda")
    wsp = ctypes.c_void_p(ws.data_ptr())

    def steps(first, n, loss_ptr, nbytes):
        return lib.ssc_mlp_train_steps(ctypes.byref(desc), buf.ptr("X"), buf.ptr("Z"), buf.ptr("idx", 4 * B * first), B, n,
                                       loss_ptr, wsp, nbytes, _stream())

    # one byte short of what the size function reports: refused before anything is launched
    start = buf.snapshot(names + ["loss"])
    assert steps(0, 1, buf.ptr("loss"), need - 1) == ffi.SSC_EINVAL
    torch.cuda.synchronize()
    after = buf.snapshot(names + ["loss"])
    assert all(start[k].tobytes() == after[k].tobytes() for k in start) and bool((ws == WS_PAT).all())

    ffi.check(steps(0, 1, buf.ptr("loss"), need))
    torch.cuda.synchronize()
    s1 = buf.snapshot(names)
    ffi.check(steps(1, 3, None if null_loss else buf.ptr("loss", 4), need))
    torch.cuda.synchronize()
    s4 = buf.snapshot(names)
    loss = buf.view["loss"].cpu().numpy().copy()
    # nothing outside the buffers was written, and no input was
    assert buf.guards_intact() == []
    assert bool((ws[need:] == WS_PAT).all()), "the step wrote behind the workspace size it reports"
    for k in ("X", "Z", "idx"):
        assert buf.view[k].cpu().numpy().tobytes() == d[k].tobytes(), k
    return dict(s1=s1, s4=s4, loss=loss, need=need)


_RUNS = {}


def _run(ffi, case):
    """the case's first execution (losses of all four steps written); once per case"""
    if case.name not in _RUNS:
        _RUNS[case.name] = _execute(ffi, case, null_loss=False)
    return _RUNS[case.name]


_ORACLE = {}


def _oracle4(case):
    """O.mlp_train_step carried over the four steps in fp64: (W, b, adam, losses); once per case, never modified"""
    if case.name not in _ORACLE:
        d = D.case_data(case)
        W, b = [w.astype(np.float64) for w in d["Ws"]], [x.astype(np.float64) for x in d["bs"]]
        adam = dict(mW=[np.zeros_like(w) for w in W], vW=[np.zeros_like(w) for w in W], mb=[np.zeros_like(x) for x in b],
                    vb=[np.zeros_like(x) for x in b], t=0)
        losses = []
        for k in range(4):
            W, b, adam, loss = O.mlp_train_step(W, b, adam, d["X"][d["idx"][k]], d["Z"][d["idx"][k]], lr=D.LR)
            losses.append(loss)
        _ORACLE[case.name] = (W, b, adam, losses)
    return _ORACLE[case.name]


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_step1_gradient_moments_and_parameters_within_float32_bound(ffi, case):
    d, ref, run = D.case_data(case), D.reference(case), _run(ffi, case)
    s1 = run["s1"]
    worst = np.zeros(3)
    per = {}
    for l in range(len(d["Ws"])):
        for key, theta0, g64, A in (("W", d["Ws"][l], ref["gW"][l], ref["A_W"][l]), ("b", d["bs"][l], ref["gb"][l], ref["A_b"][l])):
            r = D.step1_ratios(theta0, g64, A, s1["m%s%d" % (key, l)], s1["v%s%d" % (key, l)], s1["%s%d" % (key, l)])
            per["%s%d" % (key, l)] = r
            worst = np.maximum(worst, r)
    rl = D.loss_ratio(ref, run["loss"][0]) / D.C_LOSS
    print("DYN_MATRIX %s %s %s err / allowed: m %.3f v %.3f theta %.3f loss %.3f" % (case.name, case.path, case.kernel, worst[0], worst[1],
                                                                                    worst[2], rl))
    assert int(s1["adam_t"][0]) == 1
    for name, r in per.items():
        assert r[0] <= 1.0 and r[1] <= 1.0 and r[2] <= 1.0, (name, r)
    assert rl <= 1.0, (float(run["loss"][0]), ref["loss"])


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_steps_2_to_4_in_one_call_follow_the_oracle(ffi, case):
    run = _run(ffi, case)
    W, b, adam, losses = _oracle4(case)
    s4 = run["s4"]
    assert int(s4["adam_t"][0]) == 4
    for k in range(4):
        assert abs(float(run["loss"][k]) - losses[k]) <= 2e-4 * max(1.0, losses[k]), (k, float(run["loss"][k]), losses[k])
    for l in range(len(W)):
        assert np.max(np.abs(s4["W%d" % l] - W[l])) <= 2e-5 and np.max(np.abs(s4["b%d" % l] - b[l])) <= 2e-5, l
        for key in ("W", "b"):
            m, v = s4["m%s%d" % (key, l)], s4["v%s%d" % (key, l)]
            rm, rv = adam["m" + key][l], adam["v" + key][l]
            assert np.all(np.abs(m - rm) <= 1e-7 + 1e-3 * np.abs(rm)), (key, l, float(np.max(np.abs(m - rm))))
            assert np.all(np.abs(v - rv) <= 1e-9 + 2e-3 * np.abs(rv)), (key, l, float(np.max(np.abs(v - rv))))


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_same_start_same_bits_with_and_without_loss(ffi, case):
    """a second execution from the same start: the same bits in every parameter, moment and loss; for the rows marked
    null_loss its steps 2-4 run with d_loss = NULL, which changes no parameter or moment bit and writes no loss"""
    first = _run(ffi, case)
    again = _execute(ffi, case, null_loss=case.null_loss)
    assert again["need"] == first["need"]
    for stage in ("s1", "s4"):
        for k, v in first[stage].items():
            assert again[stage][k].tobytes() == v.tobytes(), (stage, k)
    assert again["loss"][0].tobytes() == first["loss"][0].tobytes()
    if case.null_loss:
        assert np.all(again["loss"][1:] == np.float32(-7.0))
    else:
        assert again["loss"].tobytes() == first["loss"].tobytes()


# ------------------------------------------------------------------------------------------------- ssc_mse_batches --
@pytest.mark.parametrize("n_batches", [1, 3])
@pytest.mark.parametrize("batch_elems", [1, 63, 256, 257])
def test_mse_batches_against_fp64_means(ffi, batch_elems, n_batches):
    """Dyn_Model.run_validation's reduction: the per-batch means of (z - pred)^2 and their mean, 1e-5 relative (the
    run_validation tolerance); block sizes below, at and above the 256-thread stride, guarded outputs"""
    rng = np.random.default_rng([batch_elems, n_batches])
    pred = rng.normal(size=n_batches * batch_elems).astype(np.float32)
    z = (pred + 0.5 * rng.normal(size=pred.size)).astype(np.float32)
    buf = _Buffers()
    buf.add("pred", pred), buf.add("z", z), buf.add("batch", np.full(n_batches, -7.0, np.float32)), buf.add("mean", np.full(1, -7.0, np.float32))
    ffi.check(ffi.lib().ssc_mse_batches(buf.ptr("pred"), buf.ptr("z"), n_batches, batch_elems, buf.ptr("batch"), buf.ptr("mean"), _stream()))
    torch.cuda.synchronize()
    ref = ((z.astype(np.float64) - pred.astype(np.float64)) ** 2).reshape(n_batches, batch_elems).mean(axis=1)
    got, mean = buf.view["batch"].cpu().numpy(), float(buf.view["mean"].cpu().numpy()[0])
    assert np.all(np.abs(got - ref) <= 1e-5 * ref), (got, ref)
    assert abs(mean - ref.mean()) <= 1e-5 * ref.mean()
    assert buf.guards_intact() == []
    assert buf.view["pred"].cpu().numpy().tobytes() == pred.tobytes() and buf.view["z"].cpu().numpy().tobytes() == z.tobytes()
