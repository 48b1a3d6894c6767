"""The contract the DDPG learners share (csrc/ddpg_layout.h), compiled for the host and checked without a GPU: the flat
parameter layout against ``agents.views_like`` -- the Python statement of the same layout --, and which learner serves a
descriptor against a table read off the dispatch as it stood before it became a function."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc not available")


@pytest.fixture(scope="module")
def H():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "host_harness"))
    import build as hb
    lib = ctypes.CDLL(hb.build())
    lib.h_ddpg_learner_path.restype = ctypes.c_int
    return lib


def _desc(obs=2, h=(64, 32), act=1, B=64, critic_h=None, **kw):
    from smartstartcontinuous_amd import _ffi
    d = _ffi.DdpgDesc()
    d.obs_dim, d.act_dim, d.batch_size, d.last_layer_tanh = obs, act, B, 1
    d.actor_h1, d.actor_h2 = h
    d.critic_h1, d.critic_h2 = critic_h or h
    for k, v in kw.items():
        setattr(d, k, v)
    return d


C_SEGMENTS = ("W1", "b1", "ln1_b", "ln1_g", "W2", "b2", "ln2_b", "ln2_g", "W3", "b3")   # the order h_ddpg_layout reports


@pytest.mark.parametrize("layer_norm", [False, True], ids=["plain", "layer_norm"])
@pytest.mark.parametrize("net", ["actor", "critic"])
@pytest.mark.parametrize("obs,h,act", [(2, (64, 32), 1), (3, (200, 100), 1), (5, (7, 3), 2)])
def test_cpp_layout_is_views_like(H, obs, h, act, net, layer_norm):
    from smartstartcontinuous_amd import agents as A
    init = A.init_actor_weights if net == "actor" else A.init_critic_weights
    w = init(obs, h[0], h[1], act)
    if layer_norm:
        w = A.with_layer_norm(w)
    flat, views = A.flatten_params(w, "cpu")
    out = np.full(11, -1, np.int32)
    H.h_ddpg_layout(ctypes.byref(_desc(obs, h, act, layer_norm=int(layer_norm))), 0 if net == "actor" else 1,
                    out.ctypes.data_as(ctypes.c_void_p))
    got = dict(zip(C_SEGMENTS, out[:10].tolist()))
    assert set(views) == set(A.param_keys(w)) and set(views) <= set(C_SEGMENTS)
    assert len(views) == (10 if layer_norm else 6)
    for k, v in views.items():
        assert v.data_ptr() == flat.data_ptr() + 4 * got[k], (k, got)
        assert got[k] == v.storage_offset()
    assert int(out[10]) == flat.numel() == sum(v.numel() for v in views.values())
    # every segment ends where the next one begins: the offsets and the shapes agree, not only the starts
    order = sorted(views, key=lambda k: got[k])
    assert order == list(A.param_keys(w))
    for k, nxt in zip(order, order[1:] + [None]):
        assert got[k] + views[k].numel() == (int(out[10]) if nxt is None else got[nxt])


FIXED, FIXED_TILED, INTERPRETER, WIDE, NEEDS_WORKSPACE = range(5)
S = dict(obs=2)                       # the shipped 64-32 networks at batch 64
S3 = dict(obs=3)
B128, B96 = dict(B=128), dict(B=96)
H48 = dict(h=(48, 24))
H64 = dict(h=(64, 64))                # 64-64 / 64-64: narrow enough for one workgroup, but the carve passes the LDS
H200 = dict(h=(200, 100))
LN, L2, CLIP = dict(layer_norm=1), dict(critic_l2_reg=1e-2), dict(clip_norm=0.5)

# (descriptor, have_ws, have_rms, want_interp, want_wide) -> learner, as ddpg_train_any decided before ddpg_learner_path
# existed: no workspace and not narrow (LayerNorm, critic_l2_reg, clip_norm, batch != 64, a layer wider than 64) ->
# refused; workspace, no switch, 64-32 at a multiple of 64 above 64 -> tiled; not narrow, or SSC_DDPG_WIDE with a
# workspace -> wide; the 64-32 shape without SSC_DDPG_INTERPRETER -> fixed; statistics -> wide; carve too large -> wide
# with a workspace, refused without; else the interpreter.
PATHS = [
    (S, True, False, False, False, FIXED), (S, False, False, False, False, FIXED),
    (S3, True, False, False, False, FIXED), (S3, False, False, False, False, FIXED),
    (S, True, True, False, False, FIXED), (S3, True, True, False, False, FIXED),
    (S, True, False, True, False, INTERPRETER), (S, False, False, True, False, INTERPRETER),
    (S3, True, False, True, False, INTERPRETER), (S3, False, False, True, False, INTERPRETER),
    (S, True, True, True, False, WIDE),            # the interpreter has no normalising build
    (S, True, False, False, True, WIDE), (S3, True, False, False, True, WIDE),
    (S, False, False, False, True, FIXED),         # SSC_DDPG_WIDE counts only with a workspace
    (S, False, False, True, True, INTERPRETER),
    (S, True, False, True, True, WIDE),            # both switches: wide
    (S, True, True, False, True, WIDE),
    (B128, True, False, False, False, FIXED_TILED), (B128, False, False, False, False, NEEDS_WORKSPACE),
    (dict(B=128, obs=3), True, False, False, False, FIXED_TILED),
    (B128, True, True, False, False, FIXED_TILED),
    (B128, True, False, False, True, WIDE), (B128, True, False, True, False, WIDE),
    (dict(B=4096), True, False, False, False, FIXED_TILED),
    (dict(B=128, **L2), True, False, False, False, FIXED_TILED),   # the apply pass behind the tiles regularises and clips
    (dict(B=128, **LN), True, False, False, False, WIDE),
    (dict(B=128, **H48), True, False, False, False, WIDE),
    (B96, True, False, False, False, WIDE), (B96, False, False, False, False, NEEDS_WORKSPACE),
    (B96, True, False, True, False, WIDE),
    (H48, True, False, False, False, INTERPRETER), (H48, False, False, False, False, INTERPRETER),
    (H48, True, True, False, False, WIDE),
    (H48, True, False, False, True, WIDE), (H48, False, False, False, True, INTERPRETER),
    (H64, True, False, False, False, WIDE), (H64, False, False, False, False, NEEDS_WORKSPACE),
    (H64, True, False, True, False, WIDE), (H64, False, False, True, False, NEEDS_WORKSPACE),
    (dict(h=(64, 32), critic_h=(64, 64)), True, False, False, False, WIDE),   # 51 040 floats: the critic alone is too much
    (dict(h=(64, 32), critic_h=(64, 64)), False, False, False, False, NEEDS_WORKSPACE),
    (LN, True, False, False, False, WIDE), (LN, False, False, False, False, NEEDS_WORKSPACE),
    (LN, True, False, True, False, WIDE),
    (L2, True, False, False, False, WIDE), (L2, False, False, False, False, NEEDS_WORKSPACE),
    (CLIP, True, False, False, False, WIDE), (CLIP, False, False, False, False, NEEDS_WORKSPACE),
    (H200, True, False, False, False, WIDE), (H200, False, False, False, False, NEEDS_WORKSPACE),
    (dict(h=(65, 32)), True, False, False, False, WIDE), (dict(h=(65, 32)), False, False, False, False, NEEDS_WORKSPACE),
    (dict(act=2), True, False, False, False, INTERPRETER),      # the fixed kernel is a 1-d action
    (dict(obs=4), True, False, False, False, INTERPRETER),      # ... and 2 or 3 observations
]


@pytest.mark.parametrize("row", range(len(PATHS)))
def test_learner_path_table(H, row):
    kw, have_ws, have_rms, want_interp, want_wide, want = PATHS[row]
    got = H.h_ddpg_learner_path(ctypes.byref(_desc(**kw)), int(have_ws), int(have_rms), int(want_interp), int(want_wide))
    assert got == want, (kw, have_ws, have_rms, want_interp, want_wide, got)
