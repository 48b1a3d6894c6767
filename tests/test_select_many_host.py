"""The six population-selection calls over ``ssc_select_many_item``: what they decide on the host, so none of this needs a
GPU.  The struct's size and offsets against the ctypes mirror; every rejection include/ssc.h lists, with its code and the
item's index in ssc_last_error(); SSC_OK without a launch for tables whose every item is empty."""
import ctypes
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ssc_replay_smart_start_indices_many", "ssc_kde_scott_bandwidth_many", "ssc_critic_forward_many", "ssc_kde_evaluate_many",
         "ssc_ucb_topk_many", "ssc_replay_episode_path_many")
N_SS = 5


@pytest.fixture(scope="module")
def ffi():
    from smartstartcontinuous_amd.build import build
    build()
    from smartstartcontinuous_amd import _ffi
    _ffi.lib()
    return _ffi


def test_struct_layout_matches_header(ffi, tmp_path):
    name, M = "ssc_select_many_item", ffi.SelectManyItem
    assert ffi.STRUCTS[name] is M and all(fn in ffi._SIGNATURES for fn in CALLS)
    fields = [f for f, _ in M._fields_]
    lines = [f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {f}));' for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssc.h"\nint main(){' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(M) and got[1:] == [getattr(M, f).offset for f in fields], got
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssc.h")).read(), flags=re.S)
    body = re.search(r"struct\s+%s\s*\{(.*?)\}\s*;" % name, text, flags=re.S).group(1)
    members = [x for decl in body.split(";") if decl.strip() for x in decl.split(",")]
    assert len(members) == len(fields), members
    assert ffi.lib().ssc_version() == 108                # additive: the ABI version does not move


def items(ffi, n):
    """n valid items over made-up device addresses (never read on the host)"""
    arr = (ffi.SelectManyItem * n)()
    for p, x in enumerate(arr):
        b = 0x01000000 + 0x10000 * p
        x.ring.s, x.ring.a, x.ring.r, x.ring.t, x.ring.s2 = b + 0x100, b + 0x200, b + 0x300, b + 0x400, b + 0x500
        x.ring.ep_steps, x.ring.ep_run = b + 0x600, b + 0x700
        x.ring.capacity, x.ring.obs_dim, x.ring.act_dim = 64, 2, 1
        x.count, x.n, x.n_ss, x.n_plans, x.seed, x.counter = 40, 4, N_SS, 3, 7, p
        x.stride, x.n_data, x.scott = 1, 41, 0.29
        c = x.critic
        c.obs_dim, c.act_dim, c.h1, c.h2 = 2, 1, 64, 32
        c.W1, c.b1, c.W2, c.b2, c.W3, c.b3 = (b + 0x1100 + 0x100 * k for k in range(6))
        x.alpha, x.beta, x.volume, x.max_len, x.row0 = 1.0, 2.0, 0.5, 18, N_SS * p
        for k, f in enumerate(("d_idx", "d_n_cand", "d_cand", "d_wh", "d_norm", "d_status", "d_value", "d_pdf", "d_ucb", "d_chosen",
                               "d_path", "d_len")):
            setattr(x, f, b + 0x2100 + 0x100 * k)
        x.d_workspace, x.workspace_bytes = b + 0x4000, ffi.lib().ssc_replay_smart_start_workspace_bytes(N_SS)
    return arr


def call(ffi, fn, arr, n=None, d_items=0x70000000, m=None, d_act=0x72000000):
    lib = ffi.lib()
    n = len(arr) if n is None else n
    h = None if arr is None else ctypes.addressof(arr)
    if fn == "ssc_critic_forward_many":
        rc = lib.ssc_critic_forward_many(h, d_items, n, N_SS * abs(n) if m is None else m, d_act, None)
    else:
        rc = getattr(lib, fn)(h, d_items, n, None)
    return rc, lib.ssc_last_error().decode()


def ln(c, v):
    c.ln1_g = c.ln1_b = c.ln2_g = c.ln2_b = v


def wide_ln(x):
    ln(x.critic, 0x5000)
    x.critic.h1, x.critic.h2 = 400, 300


EVERY = [(lambda x: setattr(x, "n_ss", 4097), "n_ss"), (lambda x: setattr(x, "n_ss", -1), "n_ss"),
         (lambda x: setattr(x, "count", -1), "count"), (lambda x: setattr(x.ring, "capacity", 0), "capacity"),
         (lambda x: setattr(x, "n", 0), "capacity"), (lambda x: setattr(x.ring, "obs_dim", 9), "obs_dim"),
         (lambda x: setattr(x.ring, "obs_dim", 0), "obs_dim"),
         (lambda x: (setattr(x.ring, "capacity", 2 ** 62), setattr(x, "count", 2 ** 62)), "too large")]
E, U = -1, -2       # SSC_EINVAL, SSC_EUNSUPPORTED
PER_CALL = {
    "ssc_replay_smart_start_indices_many": [
        (lambda x: setattr(x.ring, "ep_steps", None), E, "episode index"), (lambda x: setattr(x, "d_idx", None), E, "NULL device pointer"),
        (lambda x: setattr(x, "d_cand", None), E, "NULL device pointer"), (lambda x: setattr(x, "d_n_cand", None), E, "NULL device pointer"),
        (lambda x: setattr(x.ring, "s2", None), E, "NULL device pointer"),
        (lambda x: setattr(x, "workspace_bytes", x.workspace_bytes - 1), E, "workspace"), (lambda x: setattr(x, "d_workspace", None), E, "workspace")],
    "ssc_kde_scott_bandwidth_many": [
        (lambda x: setattr(x, "stride", 0), E, "stride"), (lambda x: setattr(x, "n_data", 40), E, "n_data"),
        (lambda x: (setattr(x, "stride", 3), setattr(x, "n_data", 13)), E, "n_data"),
        (lambda x: setattr(x, "scott", 0.0), E, "scott"), (lambda x: setattr(x, "scott", math.inf), E, "scott"),
        (lambda x: setattr(x, "scott", math.nan), E, "scott"), (lambda x: setattr(x, "d_wh", None), E, "NULL device pointer"),
        (lambda x: setattr(x, "d_norm", None), E, "NULL device pointer"), (lambda x: setattr(x, "d_status", None), E, "NULL device pointer"),
        (lambda x: setattr(x.ring, "s", None), E, "NULL device pointer")],
    "ssc_critic_forward_many": [
        (lambda x: setattr(x.critic, "obs_dim", 9), E, "out of range"), (lambda x: setattr(x.critic, "act_dim", 5), E, "out of range"),
        (lambda x: setattr(x.critic, "obs_dim", 3), E, "ring obs_dim"), (lambda x: setattr(x.critic, "h1", 0), E, "hidden"),
        (lambda x: setattr(x.critic, "h1", 600), E, "hidden"), (lambda x: setattr(x.critic, "b2", None), E, "NULL device pointer"),
        (lambda x: setattr(x.critic, "ln2_g", 0x5000), E, "LayerNorm"), (wide_ln, U, "too wide"),
        (lambda x: setattr(x, "row0", 10 ** 6), E, "outside"), (lambda x: setattr(x, "row0", -1), E, "outside"),
        (lambda x: setattr(x, "row0", 2 ** 63 - 1), E, "outside"), (lambda x: setattr(x, "d_value", None), E, "NULL device pointer"),
        (lambda x: setattr(x, "d_cand", None), E, "NULL device pointer")],
    "ssc_kde_evaluate_many": [
        (lambda x: setattr(x, "n_data", 42), E, "n_data"), (lambda x: setattr(x, "stride", -1), E, "stride"),
        (lambda x: setattr(x, "d_pdf", None), E, "NULL device pointer"), (lambda x: setattr(x, "d_norm", None), E, "NULL device pointer"),
        (lambda x: setattr(x, "d_status", None), E, "NULL device pointer"), (lambda x: setattr(x, "d_cand", None), E, "NULL device pointer")],
    "ssc_ucb_topk_many": [
        (lambda x: setattr(x, "n_plans", 0), E, "n_plans"), (lambda x: setattr(x, "n_plans", 65), E, "n_plans"),
        (lambda x: setattr(x, "volume", 0.0), E, "volume"), (lambda x: setattr(x, "volume", math.nan), E, "volume"),
        (lambda x: setattr(x, "d_chosen", None), E, "NULL device pointer"), (lambda x: setattr(x, "d_ucb", None), E, "NULL device pointer"),
        (lambda x: setattr(x, "d_idx", None), E, "NULL device pointer")],
    "ssc_replay_episode_path_many": [
        (lambda x: setattr(x, "max_len", 0), E, "max_len"), (lambda x: setattr(x, "n_plans", 65), E, "n_plans"),
        (lambda x: setattr(x, "n_plans", 0), E, "n_plans"), (lambda x: setattr(x.ring, "ep_steps", None), E, "episode index"),
        (lambda x: setattr(x, "d_len", None), E, "NULL device pointer"), (lambda x: setattr(x, "d_path", None), E, "NULL device pointer"),
        (lambda x: setattr(x, "d_chosen", None), E, "NULL device pointer")],
}


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("n", [1, 3, 33])
def test_rejections_name_the_item(ffi, fn, n):
    arr = items(ffi, n)
    assert call(ffi, fn, None, n=n)[0] == E and "NULL item array" in call(ffi, fn, None, n=n)[1]
    assert call(ffi, fn, arr, d_items=None)[0] == E
    rc, msg = call(ffi, fn, arr, n=0)
    assert rc == E and "n_items" in msg
    assert call(ffi, fn, arr, n=-n)[0] == E and call(ffi, fn, arr, n=65536)[0] == U            # on the count alone
    for p in sorted({0, n // 2, n - 1}):
        who = "item %d" % p
        for mutate, word in EVERY:
            arr = items(ffi, n)
            mutate(arr[p])
            rc, msg = call(ffi, fn, arr)
            assert rc == E and word in msg and who in msg, (fn, p, word, msg)
        for mutate, code, word in PER_CALL[fn]:
            arr = items(ffi, n)
            mutate(arr[p])
            rc, msg = call(ffi, fn, arr)
            assert rc == code and word in msg and who in msg, (fn, p, word, rc, msg)
    if fn == "ssc_critic_forward_many":
        arr = items(ffi, n)
        assert call(ffi, fn, arr, m=-1)[0] == E
        rc, msg = call(ffi, fn, arr, d_act=None)                                                # after the whole walk
        assert rc == E and "d_act" in msg
    if fn == "ssc_kde_evaluate_many" and n > 1:
        arr = items(ffi, n)
        arr[n - 1].ring.obs_dim = 3
        rc, msg = call(ffi, fn, arr)
        assert rc == U and "items 0 and %d" % (n - 1) in msg and "one obs_dim" in msg


@pytest.mark.parametrize("fn", CALLS)
def test_all_empty_tables_are_ok_without_a_launch(ffi, fn):
    """(a launch would fail here: there is no device) -- and an empty item's other fields are not read"""
    for n in (1, 3):
        for empty in ("count", "n_ss"):
            arr = items(ffi, n)
            for x in arr:
                setattr(x, empty, 0)
            x = arr[n - 1]
            x.ring.capacity, x.ring.obs_dim, x.n_plans, x.d_idx, x.n, x.critic.h1 = -5, 77, 999, None, -3, -1
            x.stride, x.max_len, x.volume, x.row0, x.d_workspace = 0, 0, -1.0, -7, None
            rc, msg = call(ffi, fn, arr)
            assert rc == 0, (fn, n, empty, msg)
