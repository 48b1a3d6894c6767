"""Every fp32 forward-simulation kernel of csrc/dyn_model.hip against the fp64 oracle under the bound derived from the float32
arithmetic (tests/sim32_cases.py: |S - ref| <= C_F32 2^-24 A elementwise at every t, and the per-step increments against
C_F32 2^-24 (A_t + A_t+1); S[0] exact).  tests/test_sim32_cases_cpu.py shows on the CPU that this bound accepts the honest
float32 variants and rejects every listed mutant at every case, and that each case launches the kernels it claims:

    pair_ref_32       (3,32,2)       H=4  m=255  dyn_small_sim_pair_kernel<2,false|true,true>
    pair_lds_30_h9    (3,30,2)       H=9  m=165  dyn_small_sim_pair_kernel<2,false|true,false>
    pair_depth1_m513  (3,1,2)        H=4  m=513  dyn_small_sim_pair_kernel<2,false|true,false>
    pair_d3_128_h20   (4,128,3)      H=20 m=256  dyn_small_sim_pair_kernel<3,false|true,true>
    pair_d3_127       (4,127,3)      H=4  m=259  dyn_small_sim_pair_kernel<3,false|true,false>
    small_*           (2,32,1) (4,64,1) (4,100,2) (3,128,1)              dyn_small_sim_kernel
    chain_*           (7,20,5) (3,129,2) (3,513,513,2) (4,3) (5,40,24,16,3) (12,64,8) (6,32,3)
                      dyn_init, dyn_prepare, mlp_layer_f32<true> .., mlp_layer_f32<false>, dyn_update
    zstd_*            one zero-std state input per family
    mlp_*             ssc_mlp_forward alone: the chain's networks at m = 1, 16, 17, 33

Each case runs once per mode (0: actions from memory, 1: drawn in the kernel); in mode 1 A_out is O.mpc_action_samples bit
for bit, and the two modes give the same bits.  Measured on an MI355X: NOTEBOOK section 26."""
import functools

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import sim_cases as SC
from tests import sim32_cases as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nav():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import navigator
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return navigator


@functools.lru_cache(maxsize=None)
def model_of(nav, name):
    case = S.CASE_BY_NAME.get(name) or S.MLP_BY_NAME[name]
    inp = S.mlp_inputs(case) if isinstance(case, S.MlpCase) else S.build_inputs(case)
    d = case.dims[-1]
    a = case.dims[0] - d if case.dims[0] > d else 1
    norm = inp.norm if hasattr(inp, "norm") else SC.make_norm(np.random.default_rng(0), d, a)
    return inp, nav.DynamicsModel([w.copy() for w in inp.Ws], [b.copy() for b in inp.bs], norm, state_dim=d, act_dim=a,
                                  precision="f32")


def assert_f32_bound(X, ref, A, what):
    assert np.isfinite(X).all(), what
    r = S.bound_ratios(X, ref, A)
    print("SIM32RATIO", *what, "state=%.3f inc=%.3f" % r, "max|X-ref|=%.3e" % np.max(np.abs(X - ref)), flush=True)
    assert max(r) <= 1.0, (what, r)


def sampling(nav, inp, **kw):
    return nav.mpc_sampling(inp.case.N, inp.low, inp.high, SC.SEED, SC.PID0, SC.T_STEP, **kw)


@pytest.mark.parametrize("name", S.CASE_IDS)
def test_sim32_case(nav, name):
    """mode 0 and mode 1 of a case, one launch each, explicit precision="f32", against the fp64 reference under the derived
    bound; A_out of mode 1 is the oracle's candidates; the two modes agree bit for bit"""
    inp, model = model_of(nav, name)
    case = inp.case
    ref, A = S.reference(case)
    s0 = torch.as_tensor(inp.s0.copy(), device="cuda")
    S0 = model.do_forward_sim(s0, inp.A.copy(), precision="f32").cpu().numpy()
    A_out = torch.full((inp.m, case.H, inp.a), -7.0, device="cuda")
    S1 = model.do_forward_sim_sampled(s0, sampling(nav, inp), inp.m, case.H, precision="f32", A_out=A_out).cpu().numpy()
    A_out = A_out.cpu().numpy()
    for p in range(case.P):
        cand = O.mpc_action_samples(SC.SEED, SC.PID0 + p, case.N, case.H, inp.a, SC.T_STEP, inp.low, inp.high)
        assert np.array_equal(A_out[p * case.N:(p + 1) * case.N], cand), (name, p)
    for mode, X in ((0, S0), (1, S1)):
        assert X.shape == (case.H + 1, inp.m, inp.d) and np.array_equal(X[0], inp.s0_rows)
        assert_f32_bound(X, ref, A, (name, f"mode{mode}"))
    assert np.array_equal(S0, S1), name


def test_sim32_small_kernel_masked_and_compact(nav):
    """dyn_small_sim_kernel in mode 1 with a problem mask, then with a compact live list as well: the live rows are the full
    launch's bits (and inside the bound), the rows of masked problems -- S and A_out -- are left alone"""
    name = "small_d1_a3_h7"
    inp, model = model_of(nav, name)
    case = inp.case
    assert S.launched(case.dims, inp.m, case.H, case.N, 1) == (S.SMALL,)
    ref, A = S.reference(case)
    s0 = torch.as_tensor(inp.s0.copy(), device="cuda")
    full = model.do_forward_sim_sampled(s0, sampling(nav, inp), inp.m, case.H, precision="f32").cpu().numpy()
    active = torch.as_tensor((np.arange(case.P) % 2 == 0).astype(np.uint8), device="cuda")
    live = np.repeat(active.cpu().numpy().astype(bool), case.N)
    lst = torch.nonzero(active).flatten().to(torch.int32)
    live_list = torch.zeros(case.P, dtype=torch.int32, device="cuda")
    live_list[:lst.numel()] = lst
    n_live = torch.tensor([lst.numel()], dtype=torch.int32, device="cuda")
    for kw in (dict(active=active), dict(active=active, live_list=live_list, n_live=n_live)):
        out = torch.full((case.H + 1, inp.m, inp.d), 123.0, device="cuda")
        A_out = torch.full((inp.m, case.H, inp.a), -7.0, device="cuda")
        got = model.do_forward_sim_sampled(s0, sampling(nav, inp, **kw), inp.m, case.H, precision="f32", out=out,
                                           A_out=A_out).cpu().numpy()
        A_out = A_out.cpu().numpy()
        assert np.array_equal(got[:, live], full[:, live]) and (got[:, ~live] == 123.0).all(), sorted(kw)
        assert np.array_equal(A_out[live], inp.A[live]) and (A_out[~live] == -7.0).all(), sorted(kw)
        assert_f32_bound(got[:, live], ref[:, live], A[:, live], (name, "masked", "+".join(sorted(kw))))


@pytest.mark.parametrize("name", [c.name for c in S.MLP_CASES])
def test_sim32_mlp_forward(nav, name):
    """ssc_mlp_forward in fp32 alone (the generic chain's layer kernels) against O.mlp_forward under the derived bound"""
    inp, model = model_of(nav, name)
    ref, A = S.reference(inp.case)
    got = model.forward(inp.x.copy(), precision="f32").cpu().numpy()
    assert got.shape == ref.shape
    assert_f32_bound(got, ref, A, (name,))
