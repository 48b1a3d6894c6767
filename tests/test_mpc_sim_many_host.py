"""ssc_mpc_forward_sim_many and navigator.DynamicsModelPopulation.sim_ways: everything they decide on the host, before any
HIP call -- so none of this needs a GPU.  The pointers are made-up addresses: a call that passed validation with work to do
would launch, so every library call here either fails validation or has nothing to launch (m == 0 or every item empty)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ITEMS = 0x7000_0000                                  # the "device copy": never read on the host
D_S0, D_S, D_A = 0x7100_0000, 0x7200_0000, 0x7300_0000
N = 19


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def population(ffi, counts=(1, 3, 2), dims=((3, 32, 2), (3, 30, 2), (3, 128, 2)), first=0):
    """one valid item per count, every array at an address of its own, the ranges back to back from ``first``"""
    items = (ffi.MpcSimManyItem * len(counts))()
    at = first
    for p, (it, n) in enumerate(zip(items, counts)):
        base = 0x1000_0000 * (p + 1)
        dd = dims[p % len(dims)]
        it.mlp.n_layers = len(dd) - 1
        for l, d in enumerate(dd):
            it.mlp.dims[l] = d
        for l in range(len(dd) - 1):
            it.mlp.W[l], it.mlp.b[l] = base + 0x10_0000 * (2 * l + 1), base + 0x10_0000 * (2 * l + 2)
        for k in range(2):
            it.norm.std_x[k] = it.norm.std_z[k] = 1.0
        it.norm.std_y[0] = 1.0
        it.problem0, it.n_problems = at, n
        at += n
    return items


def sampling(ffi, n=N, low=-1.0, high=1.0):
    sp = ffi.MpcSampling()
    sp.n_samples, sp.seed, sp.problem_id0, sp.t = n, 7, 3, 5
    sp.low[0], sp.high[0] = low, high
    return sp


def call(ffi, items, n=None, d_items=D_ITEMS, sp="default", P=None, H=4, d=2, a=1, s0=D_S0, s0_rows=1, A=D_A, S=D_S, m=None):
    sp = sampling(ffi) if sp == "default" else sp
    if m is None:
        P = sum(it.n_problems for it in items) + (items[0].problem0 if len(items) else 0) if P is None else P
        m = P * (sp.n_samples if sp is not None else N)
    rc = ffi.lib().ssc_mpc_forward_sim_many(None if items is None else ctypes.addressof(items), d_items,
                                            len(items) if n is None else n, None if sp is None else ctypes.byref(sp),
                                            m, H, d, a, s0, s0_rows, A, S, None)
    return rc, ffi.lib().ssc_last_error()


def refused(ffi, change, code=None, item=1, word=b"", **kw):
    """the call with one item changed fails with `code`, naming the item -- before any launch"""
    items = population(ffi)
    change(items[item])
    rc, msg = call(ffi, items, P=6, **kw)
    assert rc == (ffi.SSC_EINVAL if code is None else code), msg
    assert b"item %d" % item in msg and word in msg, msg


# ---- the call ------------------------------------------------------------------------------------------------------------
def test_null_arrays_and_item_count(ffi):
    items = population(ffi)
    assert call(ffi, None, n=3, m=6 * N)[0] == ffi.SSC_EINVAL
    assert call(ffi, items, d_items=None)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, n=0)
    assert rc == ffi.SSC_EINVAL and b"n_items" in msg
    assert call(ffi, items, n=-4)[0] == ffi.SSC_EINVAL
    rc, msg = call(ffi, items, n=65536)                  # refused on the count alone: items 3 .. 65535 do not exist
    assert rc == ffi.SSC_EUNSUPPORTED and b"65536" in msg
    assert ffi.lib().ssc_version() == 108                # additive: the ABI version does not move


def test_the_single_calls_checks_on_the_call(ffi):
    E, items = ffi.SSC_EINVAL, population(ffi)
    assert call(ffi, items, sp=None, m=6 * N)[0] == E
    rc, msg = call(ffi, items, m=-N)
    assert rc == E and b"m = " in msg
    assert call(ffi, items, H=0)[0] == E
    for d, a in ((0, 1), (9, 1), (2, 0), (2, 5)):
        rc, msg = call(ffi, items, d=d, a=a)
        assert rc == E and b"out of range" in msg, msg
    rc, msg = call(ffi, items, m=6 * N + 1)
    assert rc == E and b"n_samples" in msg
    assert call(ffi, items, sp=sampling(ffi, n=0), m=6 * N)[0] == E
    rc, msg = call(ffi, items, s0_rows=4)                # 4 does not divide 6 * 19
    assert rc == E and b"s0_rows" in msg
    assert call(ffi, items, s0_rows=0)[0] == E
    rc, msg = call(ffi, items, sp=sampling(ffi, low=0.5, high=0.25))
    assert rc == E and b"low > high" in msg
    for kw in (dict(s0=None), dict(S=None)):
        rc, msg = call(ffi, items, **kw)
        assert rc == E and b"NULL device pointer" in msg, msg


def test_the_compact_live_list_is_refused(ffi):
    for field in ("d_live_list", "d_n_live"):
        sp = sampling(ffi)
        setattr(sp, field, 0x7400_0000)
        rc, msg = call(ffi, population(ffi), sp=sp)
        assert rc == ffi.SSC_EINVAL and b"live" in msg, msg


# ---- the items -----------------------------------------------------------------------------------------------------------
def test_every_working_item_passes_the_single_calls_checks(ffi):
    refused(ffi, lambda it: setattr(it.mlp, "n_layers", 9), word=b"n_layers")
    refused(ffi, lambda it: setattr(it.mlp, "n_layers", 0), item=0, word=b"n_layers")
    refused(ffi, lambda it: it.mlp.dims.__setitem__(1, 0), word=b"dims[1]")
    refused(ffi, lambda it: it.mlp.W.__setitem__(1, None), item=2, word=b"layer 1")
    refused(ffi, lambda it: it.mlp.b.__setitem__(0, None), word=b"layer 0")
    refused(ffi, lambda it: it.mlp.dims.__setitem__(0, 4), word=b"expected 3 -> 2")
    refused(ffi, lambda it: it.mlp.dims.__setitem__(2, 3), item=2, word=b"expected 3 -> 2")
    refused(ffi, lambda it: setattr(it, "n_problems", -1), word=b"n_problems")


def test_an_item_outside_the_fused_family_is_unsupported(ffi):
    U = ffi.SSC_EUNSUPPORTED
    refused(ffi, lambda it: it.mlp.dims.__setitem__(1, 129), code=U, word=b"fused")

    def deeper(it):
        it.mlp.n_layers = 3
        it.mlp.dims[2], it.mlp.dims[3] = 32, 2
        it.mlp.W[2], it.mlp.b[2] = 0x6000_0000, 0x6100_0000
    refused(ffi, deeper, code=U, item=2, word=b"fused")
    # state 4 with one action: in range for the call, outside the family
    items = population(ffi, dims=((5, 32, 4),))
    rc, msg = call(ffi, items, d=4, a=1)
    assert rc == U and b"item 0" in msg, msg
    # the general kernel's shapes are inside
    rc, msg = call(ffi, population(ffi, counts=(1, 2), dims=((4, 64, 1),)), d=1, a=3, S=None)
    assert rc == ffi.SSC_EINVAL and b"NULL device pointer" in msg, msg


def test_ranges_lie_inside_the_calls_problems(ffi):
    refused(ffi, lambda it: setattr(it, "problem0", -1), word=b"outside")
    refused(ffi, lambda it: setattr(it, "problem0", 5), item=2, word=b"outside")            # [5, 7) of 6 problems
    refused(ffi, lambda it: setattr(it, "n_problems", 2 ** 31 - 1), item=2, word=b"outside")   # no 32-bit wrap
    items = population(ffi)
    rc, msg = call(ffi, items, m=0)                        # no problems at all: every working item is outside
    assert rc == ffi.SSC_EINVAL and b"item 0" in msg and b"outside" in msg


@pytest.mark.parametrize("p0,n,other", [(1, 3, 1), (3, 1, 1), (0, 1, 0), (0, 6, 0), (3, 3, 1)])
def test_ranges_are_pairwise_disjoint(ffi, p0, n, other):
    """item 3 takes problems [p0, p0 + n) of the 6 the items 0 (1 problem), 1 (3) and 2 (2) own: it meets `other` first"""
    items = population(ffi, counts=(1, 3, 2, 0))
    items[3].problem0, items[3].n_problems = p0, n
    rc, msg = call(ffi, items, P=6)
    assert rc == ffi.SSC_EINVAL and b"overlap" in msg and b"items %d and 3" % other in msg, msg
    # a skipped item takes no part
    items[3].n_problems = 0
    rc, msg = call(ffi, items, P=6, S=None)                           # (the items pass: the missing buffer is what is named)
    assert rc == ffi.SSC_EINVAL and b"NULL device pointer" in msg, msg


# ---- what is accepted ----------------------------------------------------------------------------------------------------
def test_nothing_to_launch_is_ok(ffi):
    empty = population(ffi, counts=(0, 0, 0))
    assert call(ffi, empty, m=6 * N)[0] == ffi.SSC_OK                       # every item empty
    assert call(ffi, empty, m=0)[0] == ffi.SSC_OK                           # m == 0
    assert call(ffi, empty, m=0, s0=None, S=None, A=None)[0] == ffi.SSC_OK  # ... where the single call wants no buffers either
    assert call(ffi, population(ffi, counts=(0,)), m=N)[0] == ffi.SSC_OK
    # an empty item is not read at all: zeroed, or garbage
    for fill in (0x00, 0xFF):
        items = population(ffi, counts=(0, 0, 0))
        ctypes.memset(ctypes.addressof(items[1]), fill, ctypes.sizeof(ffi.MpcSimManyItem))
        items[1].n_problems = 0
        assert call(ffi, items, m=6 * N)[0] == ffi.SSC_OK


def test_gaps_shared_weights_and_no_action_matrix_pass_validation(ffi):
    """a zeroed empty item, a gap of unowned problems, weights shared between items and d_A_out NULL: all legal -- the one
    thing wrong is what the call reports"""
    items = population(ffi, counts=(1, 3, 0, 2))
    ctypes.memset(ctypes.addressof(items[2]), 0, ctypes.sizeof(ffi.MpcSimManyItem))
    items[3].problem0 = 5                                                    # problem 4 has no owner
    for l in range(2):
        items[3].mlp.W[l], items[3].mlp.b[l] = items[0].mlp.W[l], items[0].mlp.b[l]
    items[3].mlp.dims[1] = items[0].mlp.dims[1]
    rc, msg = call(ffi, items, P=7, A=None, S=None)
    assert rc == ffi.SSC_EINVAL and b"NULL device pointer" in msg and b"item" not in msg, msg


# ---- layout --------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header(ffi, tmp_path):
    """sizeof() and offsetof() of every field as the C compiler sees them == the ctypes mirror, which sits in the
    struct-layout table of _ffi.py; the header's field list holds nothing the mirror lacks."""
    n, M = "ssc_mpc_sim_many_item", ffi.MpcSimManyItem
    assert ffi.STRUCTS[n] is M and "ssc_mpc_forward_sim_many" in ffi._SIGNATURES
    fields = [f for f, _ in M._fields_]
    lines = [f'printf("%zu\\n", sizeof({n}));'] + [f'printf("%zu\\n", offsetof({n}, {f}));' for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssc.h"\nint main(){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(M) and got[1:] == [getattr(M, f).offset for f in fields], got
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssc.h")).read(), flags=re.S)
    body = re.search(r"struct\s+%s\s*\{(.*?)\}\s*;" % n, text, flags=re.S).group(1)
    members = [x for decl in body.split(";") if decl.strip() for x in decl.split(",")]
    assert len(members) == len(fields), members


# ---- the population's routing (stub models: no GPU) ----------------------------------------------------------------------
def stub(*dims, precision="f32", device="cuda:0"):
    return types.SimpleNamespace(W=[np.zeros((dims[l], dims[l + 1]), np.float32) for l in range(len(dims) - 1)], device=device,
                                 precision=precision, state_dim=dims[-1], act_dim=dims[0] - dims[-1])


def test_sim_ways_is_a_function_of_shapes_precisions_group_size_and_the_switches(monkeypatch):
    from smartstartcontinuous_amd import navigator as nav
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "NAV_POPULATION_MIN_GROUP", 2)
    models = [stub(3, 32, 2), stub(3, 128, 2), stub(3, 129, 2), stub(3, 32, 32, 2), stub(3, 32, 2, precision="bf16_mfma"),
              stub(3, 30, 2), stub(3, 32, 2, device="cuda:1")]
    pop = nav.DynamicsModelPopulation(models)
    assert pop.sim_ways == ["many", "many", "alone", "alone", "alone", "many", "alone"]
    # the family is small_sim_shape: state <= 3, state + act <= 4, act <= 3, one hidden layer <= 128
    fam = [stub(4, 64, 1), stub(4, 100, 2), stub(4, 128, 3), stub(5, 32, 4), stub(5, 32, 3), stub(5, 32, 1), stub(2, 1, 1), stub(3, 2)]
    assert [nav.DynamicsModelPopulation.sim_way_of(m) for m in fam] == ["many", "many", "many", "alone", "alone", "alone", "many", "alone"]
    monkeypatch.setattr(nav, "NAV_POPULATION_MIN_GROUP", 4)
    assert pop.sim_ways == ["alone"] * 7                                     # three fused-family models are too few
    monkeypatch.setattr(nav, "NAV_POPULATION_MIN_GROUP", 3)
    assert pop.sim_ways.count("many") == 3
    monkeypatch.setattr(nav, "NAV_POPULATION_MIN_GROUP", 1)
    assert nav.DynamicsModelPopulation([stub(3, 32, 2)]).sim_ways == ["many"]
    monkeypatch.setattr(nav, "NAV_POPULATION_MIN_GROUP", 2)
    assert nav.DynamicsModelPopulation([stub(3, 32, 2)]).sim_ways == ["alone"]
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", False)                # the yardstick: everyone alone
    assert pop.sim_ways == ["alone"] * 7
    # the training switches do not move it
    monkeypatch.setattr(nav, "NAV_POPULATION_GROUPED", True)
    monkeypatch.setattr(nav, "DYN_POPULATION_GROUPED", False)
    assert pop.sim_ways == ["many", "many", "alone", "alone", "alone", "many", "alone"]
