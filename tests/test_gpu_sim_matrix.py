"""Every forward-simulation instantiation that run_mfma() (csrc/dyn_mfma.hip) can select, against the fp64 oracle under a
bound that follows the bf16 arithmetic (tests/sim_cases.py: e_bf16 = max |emulation - fp64| at the case's own inputs,
accepted: |S - emu| <= c e_bf16 and |S - ref| <= (1 + c) e_bf16 with c = 1, on the trajectory, on the first step alone and
on the per-step increments).  tests/test_oracle_networks.py shows on the CPU that this bound rejects every listed way a
kernel goes wrong at every case below.

case -> dyn_mfma_sim_kernel<UT, NFC, BIASK, KIN, LAG, MODE, WALK> (MODE -1: decided by run-time flags; "0|1": the LAG kernel
has one instantiation with the actions read from memory and one that draws them, each case runs both):

    1x32_k4      (3,32,2)        H=20 m=1000   <1,1,false,4>          2x127_k10   (10,127,127,7) H=4  m=255  <4,2,false,10>
    1x20_k10     (7,20,5)        H=4  m=257    <1,1,false,10>         2x100_k12   (12,100,100,8) H=4  m=256  <4,2,true,12>
    1x32_k12     (12,32,8)       H=4  m=255    <1,1,false,12>         2x128_k12   (12,128,128,8) H=20 m=257  <4,2,false,12>
    1x100_k4     (4,100,3)       H=20 m=256    <4,1,false,4>          2x500_k10   (10,500,500,7) H=20 m=255  <16,2,true,10>
    1x100_k10    (10,100,7)      H=4  m=255    <4,1,false,10>         2x512_k10   (10,512,512,7) H=4  m=257  <16,2,false,10>
    1x64_k12     (12,64,8)       H=20 m=257    <4,1,false,12>         2x500_h20   (4,500,500,3)  H=20 m=1000 <16,2,true,4,LAG,0|1>
    1x500_k4     (4,500,3)       H=20 m=1000   <16,1,false,4>         2x500_h4    (4,500,500,3)  H=4  m=257  <16,2,true,4,LAG,0|1>
    1x300_k10    (10,300,7)      H=4  m=256    <16,1,false,10>        2x500_h1    (4,500,500,3)  H=1  m=255  <16,2,true,4,LAG,0|1>
    1x500_k12    (12,500,8)      H=4  m=255    <16,1,false,12>        2x500_m1    (3,500,500,2)  H=4  m=1    <16,2,true,4,LAG,0|1>
    2x30_k4      (4,30,30,3)     H=20 m=1000   <1,2,true,4>           2x510_k4    (3,510,510,2)  H=4  m=256  <16,2,true,4,LAG,0|1>
    2x31_k4      (3,31,31,2)     H=4  m=255    <1,2,false,4>          2x511_h20   (4,511,511,3)  H=20 m=257  <16,2,false,4,LAG,0|1>
    2x32_k4      (3,32,32,2)     H=4  m=257    <1,2,false,4>          2x511_3to2  (3,511,511,2)  H=4  m=255  <16,2,false,4,LAG,0|1>
    2x24_k10     (7,24,24,5)     H=4  m=256    <1,2,true,10>          2x512_h20   (4,512,512,3)  H=20 m=1000 <16,2,false,4,LAG,0|1>
    2x31_k10     (10,31,31,7)    H=20 m=1      <1,2,false,10>         2x512_h4    (3,512,512,2)  H=4  m=256  <16,2,false,4,LAG,0|1>
    2x30_k12     (12,30,30,8)    H=4  m=255    <1,2,true,12>          2x512_h1    (4,512,512,3)  H=1  m=1    <16,2,false,4,LAG,0|1>
    2x32_k12     (12,32,32,8)    H=4  m=256    <1,2,false,12>         walk500_h20 (4,500,500,3)  H=20 m=144016 <16,2,true,4,LAG,0|1,WALK>
    2x100_k4     (4,100,100,3)   H=20 m=255    <4,2,true,4>           walk500_h1  (4,500,500,3)  H=1  m=144016 <16,2,true,4,LAG,0|1,WALK>
    2x127_k4     (4,127,127,3)   H=4  m=257    <4,2,false,4>          walk512_h20 (4,512,512,3)  H=20 m=144016 <16,2,false,4,LAG,0|1,WALK>
    2x128_k4     (3,128,128,2)   H=4  m=256    <4,2,false,4>          walk512_h1  (4,512,512,3)  H=1  m=144016 <16,2,false,4,LAG,0|1,WALK>
    2x64_k10     (7,64,64,5)     H=20 m=1000   <4,2,true,10>

31 simulation instantiations: 9 one-layer, 12 resident-W2 (UT 1 and 4), 2 streamed KIN = 10, 8 LAG (BIASK x MODE x WALK).
<16,2,*,4> without LAG is compiled but unreachable (the compact-input shapes all take the LAG kernel), 12 inputs with two
layers deeper than 128 are SSC_EUNSUPPORTED (asserted below).

Measured on an MI355X, max |S - emu| / e_bf16 (per case and quantity: NOTEBOOK section 12): largest 0.82 (2x127_k4, first
step), then 0.79 (1x64_k12), 0.76 (2x32_k12), 0.73 (2x511_3to2); the BASELINE shape 0.12-0.50 at H = 20, 0.47 walking at H = 1;
zero-std cases at most 0.66.  Both modes give the same bits at every case.  c = 1 holds with no kernel or emulation change.
"""
import functools

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import sim_cases as SC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FLAT = [c for c in SC.CASES if not c.walk]
WALK = [c for c in SC.CASES if c.walk]


@pytest.fixture(scope="module")
def nav():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import navigator
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return navigator


@functools.lru_cache(maxsize=None)
def prepared(name):
    case = next(c for c in SC.CASES if c.name == name)
    inp = SC.build_inputs(case)
    ref, emu = SC.references(inp)
    return inp, ref, emu


def assert_bf16_bound(S, ref, emu, what):
    """the existing 3e-2 / 3e-3 assertions and, beside them, the bound that follows the bf16 arithmetic"""
    scale = np.maximum(1.0, np.abs(ref).max())
    assert np.isfinite(S).all(), what
    assert np.max(np.abs(S - ref)) <= 3e-2 * scale, what
    assert np.max(np.abs(S - emu)) <= 3e-3 * scale, what
    r = SC.bound_ratios(S, ref, emu)
    print("SIMRATIO", *what, " ".join(f"{k}={v:.3f}" for k, v in r.items()), flush=True)
    assert SC.within_bf16_bound(r, SC.C_BF16), (what, r)


def run_case(nav, model, inp, mode, precision):
    """mode 0: the actions from memory; mode 1: drawn in the kernel (A_out must come back as the oracle's candidates)"""
    case = inp.case
    assert inp.rows.size == inp.m
    s0 = torch.as_tensor(inp.s0, device="cuda")
    if mode == 0:
        S = model.do_forward_sim(s0, inp.A, precision=precision)
    else:
        sp = nav.mpc_sampling(case.N, inp.low, inp.high, SC.SEED, SC.PID0, SC.T_STEP)
        A_out = torch.full((inp.m, case.H, inp.a), -7.0, device="cuda")
        S = model.do_forward_sim_sampled(s0, sp, inp.m, case.H, precision=precision, A_out=A_out)
        assert np.array_equal(A_out.cpu().numpy(), inp.A), case.name
    S = S.cpu().numpy()
    assert S.shape == (case.H + 1, inp.m, inp.d) and np.array_equal(S[0], inp.s0_rows)
    return S


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", [c.name for c in FLAT])
def test_sim_matrix_mfma_vs_oracle(nav, name, mode):
    """One launch per (case, mode) of the table in the module docstring, an explicit precision="bf16_mfma" (no fp32 fall-back),
    against O.dyn_forward_sim in fp64 and its bf16 emulation.  The candidates are O.mpc_action_samples' in both modes, so the
    two modes of a case have the same reference."""
    inp, ref, emu = prepared(name)
    model = nav.DynamicsModel(inp.Ws, inp.bs, inp.norm, state_dim=inp.d, act_dim=inp.a, precision="bf16_mfma")
    S = run_case(nav, model, inp, mode, "bf16_mfma")
    assert_bf16_bound(S, ref, emu, (name, f"mode{mode}"))


@pytest.mark.parametrize("name", [c.name for c in FLAT])
def test_sim_matrix_f32_vs_oracle(nav, name):
    """The same cases through the fp32 kernels (fused small-network kernels where the shape has them, the generic chain
    elsewhere), both modes, at their existing bound of 1e-4 relative to the largest state."""
    inp, ref, _ = prepared(name)
    model = nav.DynamicsModel(inp.Ws, inp.bs, inp.norm, state_dim=inp.d, act_dim=inp.a, precision="f32")
    for mode in (0, 1):
        S = run_case(nav, model, inp, mode, "f32")
        assert np.max(np.abs(S - ref)) <= 1e-4 * np.maximum(1.0, np.abs(ref).max()), (name, mode)


@pytest.mark.parametrize("name", [c.name for c in WALK])
def test_sim_matrix_walking_vs_oracle(nav, name):
    """More row tiles than CUs: the LAG kernel walks.  Both modes against the oracle on a strided row subset that holds rows
    of the first tile, of the last (ragged) tile and of tiles handed out by the shared counter; the same launch again is
    bit-equal (the counter is back at zero); a one-tile launch on the same model afterwards is still right."""
    inp, ref, emu = prepared(name)
    case = inp.case
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_tiles = (inp.m + SC.TILE_ROWS - 1) // SC.TILE_ROWS
    assert n_cu <= SC.WALK_MAX_CUS and n_tiles > 2 * n_cu + 2
    model = nav.DynamicsModel(inp.Ws, inp.bs, inp.norm, state_dim=inp.d, act_dim=inp.a, precision="bf16_mfma")
    s0 = torch.as_tensor(inp.s0, device="cuda")
    rows = torch.as_tensor(inp.rows, device="cuda")
    sp = nav.mpc_sampling(case.N, inp.low, inp.high, SC.SEED, SC.PID0, SC.T_STEP)
    A_all = torch.full((inp.m, case.H, inp.a), -7.0, device="cuda")
    S1 = model.do_forward_sim_sampled(s0, sp, inp.m, case.H, precision="bf16_mfma", A_out=A_all).clone()
    assert np.array_equal(A_all[rows].cpu().numpy(), inp.A)
    assert torch.equal(S1[0], s0.repeat_interleave(case.N, dim=0))
    assert_bf16_bound(S1[:, rows].cpu().numpy(), ref, emu, (name, "mode1"))
    again = model.do_forward_sim_sampled(s0, sp, inp.m, case.H, precision="bf16_mfma")
    assert torch.equal(again, S1)
    S0 = model.do_forward_sim(s0, A_all, precision="bf16_mfma").clone()
    assert_bf16_bound(S0[:, rows].cpu().numpy(), ref, emu, (name, "mode0"))
    assert torch.equal(S0, S1)
    assert torch.equal(model.do_forward_sim(s0, A_all, precision="bf16_mfma"), S0)
    # one tile, one block, no walk, same model and workspace: the rows of the first tile again
    one = model.do_forward_sim(s0[:SC.TILE_ROWS // case.N].contiguous(), A_all[:SC.TILE_ROWS].contiguous(), precision="bf16_mfma")
    assert torch.equal(one, S0[:, :SC.TILE_ROWS])
    first = inp.rows < 32
    assert first.sum() == 32
    assert_bf16_bound(one[:, :32].cpu().numpy(), ref[:, first], emu[:, first], (name, "one_tile"))
    # ... and the walk once more behind it
    assert torch.equal(model.do_forward_sim_sampled(s0, sp, inp.m, case.H, precision="bf16_mfma"), S1)


@pytest.mark.parametrize("dims", [(3, 32, 2), (4, 100, 100, 3), (4, 500, 500, 3), (4, 512, 512, 3), (10, 500, 500, 7), (12, 64, 8)])
@pytest.mark.parametrize("precision", ["f32", "bf16_mfma"])
def test_sim_horizon_zero(nav, dims, precision):
    """H = 0: ssc_dyn_forward_sim accepts it and S is [1, m, d] == s0 (per call and per row); ssc_mpc_forward_sim (nothing
    to draw) rejects it with SSC_EINVAL."""
    from smartstartcontinuous_amd import _ffi
    rng = np.random.default_rng(sum(dims))
    d, a = dims[-1], dims[0] - dims[-1]
    Ws, bs = SC.make_mlp(rng, dims)
    model = nav.DynamicsModel(Ws, bs, SC.make_norm(rng, d, a), state_dim=d, act_dim=a, precision=precision)
    for m in (1, 257, 700):
        A = torch.empty((m, 0, a), device="cuda")
        for s0 in (rng.normal(size=d).astype(np.float32), rng.normal(size=(m, d)).astype(np.float32)):
            out = torch.full((1, m, d), 123.0, device="cuda")
            S = model.do_forward_sim(s0, A, precision=precision, out=out).cpu().numpy()
            assert S.shape == (1, m, d) and np.array_equal(S[0], np.broadcast_to(s0, (m, d)))
    with pytest.raises(_ffi.SscError) as e:
        model.do_forward_sim_sampled(s0, nav.mpc_sampling(m, SC.ACT_LOW[:a], SC.ACT_HIGH[:a], 1), m, 0, precision=precision,
                                     A_out=torch.empty((m, 0, a), device="cuda"))
    assert e.value.code == _ffi.SSC_EINVAL


def test_sim_twelve_inputs_two_deep_layers_stay_unsupported(nav):
    """12 inputs with two layers deeper than 128: no MFMA kernel (one layer-1 k-step holds 10 inputs) -- an explicit request
    raises SSC_EUNSUPPORTED in every entry point, in both simulation modes."""
    from smartstartcontinuous_amd import _ffi
    rng = np.random.default_rng(12)
    for dims in ((12, 129, 129, 8), (11, 500, 500, 8), (12, 512, 512, 8)):
        d, a = dims[-1], dims[0] - dims[-1]
        Ws, bs = SC.make_mlp(rng, dims)
        model = nav.DynamicsModel(Ws, bs, SC.make_norm(rng, d, a), state_dim=d, act_dim=a, precision="f32")
        A = rng.uniform(-1, 1, size=(64, 3, a)).astype(np.float32)
        s0 = rng.normal(size=d).astype(np.float32)
        calls = [lambda: model.do_forward_sim(s0, A, precision="bf16_mfma"),
                 lambda: model.do_forward_sim_sampled(s0, nav.mpc_sampling(64, SC.ACT_LOW[:a], SC.ACT_HIGH[:a], 1), 64, 3,
                                                      precision="bf16_mfma"),
                 lambda: model.forward(rng.normal(size=(64, dims[0])).astype(np.float32), precision="bf16_mfma")]
        for call in calls:
            with pytest.raises(_ffi.SscError) as e:
                call()
            assert e.value.code == _ffi.SSC_EUNSUPPORTED, dims


# ---------------------------------------------------------------------------------------------- zero std --
FLT_MAX = float(np.finfo(np.float32).max)


def emu_fp32_inputs(x, Ws, bs):
    """O.mlp_forward_bf16emu casts its input to fp32, where the oracle's +-DBL_MAX of x / 0 would be inf and inf * 0 NaN:
    clamp to +-FLT_MAX first, which is what np.nan_to_num gives in fp32 (the kernel's own arithmetic)."""
    return O.mlp_forward_bf16emu(np.clip(x, -FLT_MAX, FLT_MAX), Ws, bs)


# shape -> the input / normalisation code it selects: fp32 (fused pair kernel | generic chain), MFMA (compact KIN = 4 |
# generic KIN = 10 | the LAG kernel, one block per tile and walking)
ZERO_STD_SHAPES = [("pair_or_compact", (3, 32, 2), 1, 300), ("generic_k10", (10, 64, 64, 7), 1, 300),
                   ("lag", (4, 500, 500, 3), 1, 300), ("lag_walk", (4, 500, 500, 3), 9001, 16)]


@pytest.mark.parametrize("quirk", ["zero_over_zero", "x_over_zero", "action_over_zero"])
@pytest.mark.parametrize("shape,precision", [(s[0], p) for s in ZERO_STD_SHAPES for p in ("f32", "bf16_mfma")
                                             if (s[0], p) != ("lag_walk", "f32")])    # walking is an MFMA launch shape
def test_forward_sim_zero_std_every_path(nav, shape, precision, quirk):
    """np.nan_to_num((x - mean) / std) with std == 0 (dynamics_model.py:228-229) on every path that has its own code for it.
    zero_over_zero: the column sits at its mean, 0/0 -> 0 (the existing quirk test's case).  x_over_zero: a zero-std STATE
    column away from its mean, x/0 -> +-max with both signs across rows.  action_over_zero: std_y == 0 under random actions.
    The input's row of W1 is zero, so the huge value must contribute exactly 0 (an inf * 0 = NaN anywhere would poison the
    trajectory): all-finite, and the oracle comparison on every column.  The bf16 emulation gets its inputs clamped to
    +-FLT_MAX (emu_fp32_inputs); with that the MFMA path is held to the bf16 bound here as well."""
    _, dims, P, N = next(s for s in ZERO_STD_SHAPES if s[0] == shape)
    walk = shape == "lag_walk"
    H = 3
    rng = np.random.default_rng(sum(dims) + len(quirk))
    d, a = dims[-1], dims[0] - dims[-1]
    Ws, bs = SC.make_mlp(rng, dims)
    norm = SC.make_norm(rng, d, a)
    m = P * N
    j = d - 1                                               # the zero-std state column
    s0 = (rng.normal(size=(P if walk else m, d)) * 0.3).astype(np.float32)
    if quirk == "action_over_zero":
        Ws[0][dims[0] - 1, :] = 0.0
        norm["std_y"][a - 1] = 0.0
        norm["mean_y"][a - 1] = 0.5 * (SC.ACT_LOW[a - 1] + SC.ACT_HIGH[a - 1]) + 0.125   # inside the range: both signs
    else:
        Ws[0][j, :] = 0.0
        norm["std_x"][j] = 0.0
        norm["mean_z"][j] = norm["std_z"][j] = 0.0          # the column never moves
        norm["mean_x"][j] = 0.25
        s0[:, j] = 0.25 if quirk == "zero_over_zero" else 0.25 + np.where(np.arange(s0.shape[0]) % 2 == 0, 0.5, -0.5)
    model = nav.DynamicsModel(Ws, bs, norm, state_dim=d, act_dim=a, precision=precision)
    rows = SC.walk_subset(m) if walk else np.arange(m)
    A = SC.action_rows(rows, N, H, a)
    s0_rows = s0[rows // N] if walk else s0
    s0_dev = torch.as_tensor(s0, device="cuda")
    if walk:                                                # in-kernel sampling, P problems x 16 candidates
        sp = nav.mpc_sampling(N, SC.ACT_LOW[:a], SC.ACT_HIGH[:a], SC.SEED, SC.PID0, SC.T_STEP)
        S = model.do_forward_sim_sampled(s0_dev, sp, m, H, precision=precision)
        assert bool(torch.isfinite(S).all())
        S = S[:, torch.as_tensor(rows, device="cuda")].cpu().numpy()
    else:
        S = model.do_forward_sim(s0_dev, A, precision=precision).cpu().numpy()
    nm = SC.norm32(norm)
    ref = O.dyn_forward_sim(s0_rows, A, nm, Ws, bs)
    # the case reaches the branch it is named after
    xs = O.normalise(s0_rows, nm["mean_x"], nm["std_x"])
    ys = O.normalise(A[:, 0], nm["mean_y"], nm["std_y"])
    if quirk == "zero_over_zero":
        assert (xs[:, j] == 0).all()
    elif quirk == "x_over_zero":
        assert (xs[:, j] > 1e300).any() and (xs[:, j] < -1e300).any()
    else:
        assert (ys[:, a - 1] > 1e300).any() and (ys[:, a - 1] < -1e300).any()
    assert np.isfinite(S).all() and np.isfinite(ref).all()
    assert np.array_equal(S[0], s0_rows)
    if quirk != "action_over_zero":
        assert np.array_equal(S[:, :, j], np.broadcast_to(s0_rows[:, j], (H + 1, rows.size)))
    scale = np.maximum(1.0, np.abs(ref).max())
    if precision == "f32":
        tol = 1e-5 if shape == "pair_or_compact" else 1e-4  # the fp32 paths' existing bounds
        assert np.max(np.abs(S - ref)) <= tol * scale, (shape, quirk)
    else:
        emu = O.dyn_forward_sim(s0_rows, A, nm, Ws, bs, forward=emu_fp32_inputs)
        assert_bf16_bound(S, ref, emu, (f"zero_std_{shape}", quirk))
