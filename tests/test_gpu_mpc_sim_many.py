"""ssc_mpc_forward_sim_many (csrc/dyn_sim_many.hip: dyn_small_sim_pair_many_kernel<2 | 3>, dyn_small_sim_many_kernel): contiguous
problem ranges of one call simulated with different networks and statistics in ONE launch.  The semantics are the single
call's: after the many-call S and A_out hold, bit for bit (torch.equal on whole sentinel-filled buffers), what one
ssc_mpc_forward_sim(.., f32) per working item leaves there when its problem mask is AND-ed with the item's range.  One item
is also held to the fp64 reference under the derived float32 bound of tests/sim32_cases.py, and the sampled actions to the
oracle's Philox stream.  The models are built from the generators of tests/sim32_cases.py / tests/sim_cases.py."""
import ctypes
import functools
import zlib

import numpy as np
import pytest

from oracle import ssc_oracle as O
from tests import sim_cases as SC
from tests import sim32_cases as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENT_S, SENT_A = 123.0, -7.0


@pytest.fixture(scope="module")
def nav():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    from smartstartcontinuous_amd import navigator
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return navigator


@functools.lru_cache(maxsize=None)
def case_model(nav, name):
    """the network and statistics of a tests/sim32_cases.py case"""
    inp = S.build_inputs(S.CASE_BY_NAME[name])
    return nav.DynamicsModel([w.copy() for w in inp.Ws], [b.copy() for b in inp.bs], inp.norm, state_dim=inp.d, act_dim=inp.a,
                             precision="f32")


@functools.lru_cache(maxsize=None)
def fresh_model(nav, dims, tag):
    """another network of the same generators (sim_cases.make_mlp / make_norm)"""
    rng = np.random.default_rng(zlib.crc32(("many_%s_%s" % (dims, tag)).encode()))
    d, a = dims[-1], dims[0] - dims[-1]
    Ws, bs = SC.make_mlp(rng, dims)
    return nav.DynamicsModel(Ws, bs, SC.make_norm(rng, d, a), state_dim=d, act_dim=a, precision="f32")


def other_norm(nav, model, tag):
    """the same weight tensors (shared pointers) under other statistics"""
    norm = SC.make_norm(np.random.default_rng(zlib.crc32(tag.encode())), model.state_dim, model.act_dim)
    twin = nav.DynamicsModel(model.W, model.b, norm, state_dim=model.state_dim, act_dim=model.act_dim, precision="f32")
    assert [w.data_ptr() for w in twin.W + twin.b] == [w.data_ptr() for w in model.W + model.b]
    assert bytes(twin.norm) != bytes(model.norm)
    return twin


def item_table(ffi, layout):
    """layout: (model, problem0, n_problems) per item -> (host ctypes array, device tensor holding the same bytes)"""
    items = (ffi.MpcSimManyItem * len(layout))()
    for it, (model, p0, n) in zip(items, layout):
        it.mlp, it.norm, it.problem0, it.n_problems = model.desc, model.norm, p0, n
    dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    return items, dev


def many(ffi, layout, sp, m, H, d, a, s0, S_out, A_out):
    items, dev = item_table(ffi, layout)
    s0_rows = 1 if s0.dim() == 1 else s0.shape[0]
    rc = ffi.lib().ssc_mpc_forward_sim_many(ctypes.addressof(items), dev.data_ptr(), len(layout), ctypes.byref(sp), m, H, d, a,
                                            ffi.ptr(s0), s0_rows, ffi.ptr(A_out), ffi.ptr(S_out), ffi.stream())
    torch.cuda.synchronize()
    return rc


def buffers(m, H, d, a):
    return torch.full((H + 1, m, d), SENT_S, device="cuda"), torch.full((m, H, a), SENT_A, device="cuda")


def sequence_of_masked_single_calls(nav, layout, P, N, low, high, pid0, t, t_base, mask, m, H, s0, S_out, A_out):
    """the definition: per working item one single call whose d_problem_active is the caller's mask AND the item's range"""
    for model, p0, n in layout:
        if n == 0:
            continue
        act = np.zeros(P, np.uint8)
        act[p0:p0 + n] = 1
        if mask is not None:
            act &= mask
        sp = nav.mpc_sampling(N, low, high, SC.SEED, pid0, t, t_base=t_base, active=torch.as_tensor(act, device="cuda"))
        model.do_forward_sim_sampled(s0, sp, m, H, precision="f32", out=S_out, A_out=A_out)
    torch.cuda.synchronize()


def check_equal_to_the_sequence(nav, layout, P, N, H, d, a, s0, mask=None, pid0=SC.PID0, t=SC.T_STEP, t_base=None):
    from smartstartcontinuous_amd import _ffi as ffi
    low, high = SC.ACT_LOW[:a], SC.ACT_HIGH[:a]
    m = P * N
    mask_t = None if mask is None else torch.as_tensor(mask, device="cuda")
    want_S, want_A = buffers(m, H, d, a)
    sequence_of_masked_single_calls(nav, layout, P, N, low, high, pid0, t, t_base, mask, m, H, s0, want_S, want_A)
    got_S, got_A = buffers(m, H, d, a)
    sp = nav.mpc_sampling(N, low, high, SC.SEED, pid0, t, t_base=t_base, active=mask_t)
    assert many(ffi, layout, sp, m, H, d, a, s0, got_S, got_A) == ffi.SSC_OK, ffi.lib().ssc_last_error()
    assert torch.equal(got_S, want_S) and torch.equal(got_A, want_A)
    owned = np.zeros(P, bool)
    for _, p0, n in layout:
        owned[p0:p0 + n] = True
    if mask is not None:
        owned &= mask.astype(bool)
    rows = torch.as_tensor(np.repeat(owned, N), device="cuda")
    # the sentinel is where nobody works and nowhere else (so the comparison above compared results, not sentinels)
    assert (got_S[:, ~rows] == SENT_S).all() and (got_A[~rows] == SENT_A).all()
    assert not (got_S[:, rows] == SENT_S).any() and not (got_A[rows] == SENT_A).any()
    # d_A_out NULL: the same states
    only_S, _ = buffers(m, H, d, a)
    assert many(ffi, layout, sp, m, H, d, a, s0, only_S, None) == ffi.SSC_OK
    assert torch.equal(only_S, want_S)
    return got_S, got_A, rows


# ---- 1. two rows per lane, D = 2 ---------------------------------------------------------------------------------------------
N1, GAP = 19, 4                  # problem 4 has no owner
P1 = 34


def layout_d2(nav):
    """depths 32, 30, 1, 128 and 32 again (item 0's weights, other statistics); 1, 3, 27 (513 rows: a second workgroup of one
    row), 0 and 2 problems; the odd row counts 19, 57 and 513 leave a lone last row"""
    m32 = case_model(nav, "pair_ref_32")
    return [(m32, 0, 1), (case_model(nav, "pair_lds_30_h9"), 1, 3), (case_model(nav, "pair_depth1_m513"), 5, 27),
            (fresh_model(nav, (3, 128, 2), "empty"), 17, 0), (other_norm(nav, m32, "item4"), 32, 2)]


def start_states(kind, P, N, d, call=None):
    rng = np.random.default_rng(zlib.crc32(("s0_%s_%d_%d" % (kind, P, N)).encode()))
    if kind == "call":
        return torch.as_tensor(call.copy() if call is not None else (rng.normal(size=d) * 0.3).astype(np.float32), device="cuda")
    return torch.as_tensor((rng.normal(size=(P if kind == "problem" else P * N, d)) * 0.3).astype(np.float32), device="cuda")


@pytest.mark.parametrize("kind", ["problem", "call", "row"])
@pytest.mark.parametrize("H", [4, 9])
def test_pair_family_d2_equals_the_masked_single_calls(nav, H, kind):
    layout = layout_d2(nav)
    assert [S.launched((3, int(mo.desc.dims[1]), 2), P1 * N1, H, N1, 1)[0] for mo, _, _ in layout] == \
        [S.PAIR % (2, "true", w) for w in ("true", "false", "false", "true", "true")]
    mask = np.ones(P1, np.uint8)
    mask[7] = 0                                                   # one problem inside the 27-problem item switched off
    t_base = torch.tensor([3], dtype=torch.int64, device="cuda")  # d_t_base is honoured: t + *d_t_base = T_STEP
    check_equal_to_the_sequence(nav, layout, P1, N1, H, 2, 1, start_states(kind, P1, N1, 2), mask=mask, t=SC.T_STEP - 3,
                                t_base=t_base)


def test_one_item_meets_the_fp64_reference_and_the_oracles_actions(nav):
    """item 2 of the D = 2 layout IS the case pair_depth1_m513 (27 problems x 19, one start state per call, H = 4) once the
    call's problem_id0 puts its first problem at SC.PID0: its rows meet S.reference under the derived bound (C_F32, no new
    constant); every owned problem's actions are O.mpc_action_samples of its GLOBAL problem index"""
    case = S.CASE_BY_NAME["pair_depth1_m513"]
    inp = S.build_inputs(case)
    assert (case.P, case.N, case.H, case.s0_kind) == (27, N1, 4, "call")
    layout = layout_d2(nav)
    pid0 = SC.PID0 - layout[2][1]
    t_base = torch.tensor([2], dtype=torch.int64, device="cuda")
    got_S, got_A, rows = check_equal_to_the_sequence(nav, layout, P1, N1, 4, 2, 1, start_states("call", P1, N1, 2, call=inp.s0),
                                                     pid0=pid0, t=SC.T_STEP - 2, t_base=t_base)
    lo, hi = layout[2][1] * N1, (layout[2][1] + 27) * N1
    X = got_S[:, lo:hi].cpu().numpy()
    ref, A = S.reference(case)
    assert np.array_equal(X[0], inp.s0_rows)
    r = S.bound_ratios(X, ref, A)
    print("SIM32RATIO many pair_depth1_m513 state=%.3f inc=%.3f" % r, flush=True)
    assert np.isfinite(X).all() and max(r) <= 1.0, r
    A_np = got_A.cpu().numpy()
    assert np.array_equal(A_np[lo:hi], inp.A)
    for _, p0, n in layout:
        for p in range(p0, p0 + n):
            cand = O.mpc_action_samples(SC.SEED, pid0 + p, N1, 4, 1, SC.T_STEP, SC.ACT_LOW[:1], SC.ACT_HIGH[:1])
            assert np.array_equal(A_np[p * N1:(p + 1) * N1], cand), p
    assert (A_np[GAP * N1:(GAP + 1) * N1] == SENT_A).all()


# ---- 2. D = 3 -----------------------------------------------------------------------------------------------------------------
def test_pair_family_d3_equals_the_masked_single_calls(nav):
    layout = [(case_model(nav, "pair_d3_128_h20"), 0, 3), (case_model(nav, "pair_d3_127"), 3, 4)]
    check_equal_to_the_sequence(nav, layout, 7, 37, 20, 3, 1, start_states("problem", 7, 37, 3))


# ---- 3. the general kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H,counts", [("small_d1_m257", 4, (2, 0, 15)), ("small_d1_a3_h7", 7, (3, 7)), ("small_d2_a2", 4, (5, 1, 7))])
def test_general_kernel_equals_the_masked_single_calls(nav, name, H, counts):
    """(2,32,1), (4,64,1) with three actions at H = 7, (4,100,2) with two actions: a call each, the case's network and one or two
    others of its shape; 15 x 20 = 300 and 7 x 41 = 287 rows reach a second workgroup"""
    case = S.CASE_BY_NAME[name]
    d, a = case.dims[-1], case.dims[0] - case.dims[-1]
    N = {"small_d1_m257": 20}.get(name, case.N)
    assert S.launched(case.dims, (sum(counts) + 1) * N, H, N, 1) == (S.SMALL,)
    models = [case_model(nav, name)] + [fresh_model(nav, case.dims, "g%d" % k) for k in range(1, len(counts))]
    layout, at = [], 1                                            # problem 0 has no owner
    for mo, n in zip(models, counts):
        layout.append((mo, at, n))
        at += n
    mask = np.ones(at, np.uint8)
    mask[at - 2] = 0
    check_equal_to_the_sequence(nav, layout, at, N, H, d, a, start_states("problem", at, N, d), mask=mask)


# ---- 5. a refused call ----------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_buffers_untouched(nav):
    from smartstartcontinuous_amd import _ffi as ffi
    layout = layout_d2(nav)
    s0 = start_states("problem", P1, N1, 2)
    sp = nav.mpc_sampling(N1, SC.ACT_LOW[:1], SC.ACT_HIGH[:1], SC.SEED, SC.PID0, SC.T_STEP)
    bad = [list(layout), list(layout), list(layout)]
    bad[0][4] = (layout[4][0], 31, 2)                                                       # overlaps the 27-problem item
    bad[1][1] = (fresh_model(nav, (3, 129, 2), "deep"), 1, 3)                               # outside the fused family
    bad[2][0] = (layout[0][0], 33, 2)                                                       # past the last problem
    for lay, code in zip(bad, (ffi.SSC_EINVAL, ffi.SSC_EUNSUPPORTED, ffi.SSC_EINVAL)):
        S_out, A_out = buffers(P1 * N1, 4, 2, 1)
        assert many(ffi, lay, sp, P1 * N1, 4, 2, 1, s0, S_out, A_out) == code
        assert (S_out == SENT_S).all() and (A_out == SENT_A).all()


# ---- the Python layer on the same layout -------------------------------------------------------------------------------------
def test_population_routes_grouped_and_alone_to_the_same_bits(nav, monkeypatch):
    """DynamicsModelPopulation.do_forward_sim_sampled: the many-call for the fused-family models, a scratch and a strided copy
    for the others (a 129-deep fp32 model here), NAV_POPULATION_GROUPED = False for everyone -- all the bits of each model's
    own call on its own problems"""
    models = [case_model(nav, "pair_ref_32"), fresh_model(nav, (3, 129, 2), "deep"), case_model(nav, "pair_lds_30_h9"),
              case_model(nav, "pair_depth1_m513")]
    counts, N, H = [2, 1, 3, 2], 21, 4
    P = sum(counts)
    s0 = start_states("problem", P, N, 2)
    low, high = SC.ACT_LOW[:1], SC.ACT_HIGH[:1]
    want_S, want_A = buffers(P * N, H, 2, 1)
    at = 0
    for mo, n in zip(models, counts):
        sp = nav.mpc_sampling(N, low, high, SC.SEED, SC.PID0 + at, SC.T_STEP)
        A_p = torch.empty((n * N, H, 1), device="cuda")
        want_S[:, at * N:(at + n) * N] = mo.do_forward_sim_sampled(s0[at:at + n], sp, n * N, H, A_out=A_p)
        want_A[at * N:(at + n) * N] = A_p
        at += n
    pop = nav.DynamicsModelPopulation(models)
    for grouped, ways in ((True, ["many", "alone", "many", "many"]), (False, ["alone"] * 4)):
        monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", grouped)
        assert pop.sim_ways == ways
        got_S, got_A = buffers(P * N, H, 2, 1)
        sp = nav.mpc_sampling(N, low, high, SC.SEED, SC.PID0, SC.T_STEP)
        out = pop.do_forward_sim_sampled(s0, sp, counts, H, out=got_S, A_out=got_A)
        assert out is got_S and torch.equal(got_S, want_S) and torch.equal(got_A, want_A), grouped
