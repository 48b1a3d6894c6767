"""normalize_observations in the DDPG learner, every kernel variant against the fp64 oracle: the eight
ddpg_train_fixed_kernel<O, TANH2, TILED, const double *> instantiations, ddpg_wide_grad_kernel<const double *> with plain
and LayerNorm networks, critic_l2_reg, clip_norm, ragged batches and layer sizes, the shapes that reach the multi-workgroup
kernels only BECAUSE statistics are present (the step interpreter has no normalising build), and statistics that change
between two launches.  The device trains on the RAW replay rows with the statistics block; the oracle on
clip((x - mean) / std, -5, 5) formed in fp64 (tests/test_gpu_agents.py::_ddpg_kernel_vs_oracle: parameters and targets
<= 5e-6 after 6 iterations, losses, all four Adam moment arrays).

Two statistics sets per obs_dim, both with non-zero means that differ in every component:
  floor -- every std on the 0.1 floor; the observations are drawn 0.526 either side of the mean, so that 5 % of the
           components sit on +5 or -5 (asserted on the sampled rows, for s and s2) and most rows stay clear of the clip;
  wide  -- every std above the floor and different in every component (a std or mean taken from a neighbouring component
           cannot cancel); the observations stay within 3 std of the mean: nothing is clipped (asserted)."""
import numpy as np
import pytest

from tests.gpu_util import RMS_EDGE_MEAN, RMS_EDGE_STD, rms_edge_stats
from tests.test_gpu_agents import _ddpg_kernel_vs_oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssc():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no fallback")
    import smartstartcontinuous_amd as pkg
    pkg._ffi.lib()
    return pkg


def _run(ssc, monkeypatch, obs_dim, h, B, llt, kind, env=None, **kw):
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)
    if env is not None:
        monkeypatch.setenv(env, "1")
    rms, obs_range = rms_edge_stats(obs_dim, kind)
    _ddpg_kernel_vs_oracle(ssc, obs_dim, h[0], h[1], B=B, llts=(llt,), cap=5000, obs_rms=rms, obs_range=obs_range,
                           expect_clip=kind == "floor", **kw)


@pytest.mark.parametrize("kind", ["floor", "wide"])
@pytest.mark.parametrize("llt", [True, False])
@pytest.mark.parametrize("obs_dim", [2, 3])
def test_one_workgroup_fixed_rms_vs_oracle(ssc, monkeypatch, obs_dim, llt, kind):
    """64-32 at batch 64: ddpg_train_fixed_kernel<obs_dim, llt, false, const double *> (ddpg_fixed_shape)."""
    _run(ssc, monkeypatch, obs_dim, (64, 32), 64, llt, kind)


@pytest.mark.parametrize("obs_dim,llt,B,kind", [(2, True, 128, "floor"), (2, False, 128, "floor"), (3, True, 128, "floor"),
                                                (3, False, 128, "floor"), (3, False, 128, "wide"), (2, True, 1024, "wide"),
                                                (3, True, 1024, "wide"), (3, True, 4096, "floor")])
def test_tiled_fixed_rms_vs_oracle(ssc, monkeypatch, obs_dim, llt, B, kind):
    """64-32 at a batch of several 64-row tiles: ddpg_train_fixed_kernel<obs_dim, llt, true, const double *> per tile
    (ddpg_fixed_tiled_shape), then the multi-workgroup apply pass."""
    _run(ssc, monkeypatch, obs_dim, (64, 32), B, llt, kind)


@pytest.mark.parametrize("obs_dim,h,ch,B,llt,kind", [
    (2, (128, 64), None, 64, True, "floor"), (2, (128, 64), None, 64, False, "wide"),
    (3, (200, 100), None, 256, True, "wide"), (3, (200, 100), None, 256, False, "floor"),
    (3, (200, 100), None, 1024, True, "floor"),
    (2, (64, 32), None, 50, True, "wide"), (2, (64, 32), None, 50, False, "floor"),         # a ragged last 16-row tile
    (8, (37, 19), None, 77, True, "floor"), (8, (37, 19), None, 77, False, "wide"),        # ragged rows and units, runtime obs_dim
    (2, (128, 64), (200, 100), 128, True, "wide"), (2, (128, 64), (200, 100), 128, False, "floor")])
def test_wide_rms_vs_oracle(ssc, monkeypatch, obs_dim, h, ch, B, llt, kind):
    """Layers wider than 64 or a batch that is no multiple of 64: ddpg_wide_grad_kernel<const double *> (16-row tiles,
    ObsNorm<SSC_MAX_STATE> with the runtime obs_dim) and the apply pass."""
    kw = {} if ch is None else dict(ch1=ch[0], ch2=ch[1])
    _run(ssc, monkeypatch, obs_dim, h, B, llt, kind, **kw)


@pytest.mark.parametrize("obs_dim,h,B,ln,l2,clip,llt,kind", [
    (3, (64, 64), 256, True, 1e-2, 0.05, True, "floor"), (3, (64, 64), 256, True, 1e-2, 0.05, False, "wide"),
    (8, (37, 19), 77, True, 0.3, 0.02, True, "wide"), (8, (37, 19), 77, True, 0.3, 0.02, False, "floor"),
    (3, (200, 100), 1024, False, 1e-2, 0.5, True, "wide"), (3, (200, 100), 1024, False, 1e-2, 0.5, False, "floor"),
    (3, (128, 64), 64, True, 0.0, 5.0, True, "floor"), (3, (128, 64), 64, True, 0.0, 5.0, False, "wide")])
def test_wide_options_rms_vs_oracle(ssc, monkeypatch, obs_dim, h, B, ln, l2, clip, llt, kind):
    """LayerNorm, critic_l2_reg and clip_norm run on ddpg_wide_grad_kernel<const double *> only, with the prepare / apply
    passes (clip thresholds that bind for every variable, for some and for none)."""
    _run(ssc, monkeypatch, obs_dim, h, B, llt, kind, layer_norm=ln, critic_l2_reg=l2, clip_norm=clip)


@pytest.mark.parametrize("obs_dim,h,B,env,llt,kind", [
    (2, (24, 20), 64, None, True, "wide"), (2, (24, 20), 64, None, False, "floor"),
    (8, (64, 32), 64, None, True, "floor"), (8, (64, 32), 64, None, False, "wide"),
    (2, (64, 32), 64, "SSC_DDPG_INTERPRETER", True, "floor"), (2, (64, 32), 64, "SSC_DDPG_INTERPRETER", False, "wide"),
    (2, (64, 32), 1024, "SSC_DDPG_WIDE", True, "wide")])
def test_routed_to_wide_by_statistics_vs_oracle(ssc, monkeypatch, obs_dim, h, B, env, llt, kind):
    """Narrow batch-64 shapes the step interpreter serves without statistics (24-20, obs_dim 8, and 64-32 under
    SSC_DDPG_INTERPRETER=1): the interpreter has no normalising build, ddpg_train_any sends them to
    ddpg_wide_grad_kernel<const double *>; SSC_DDPG_WIDE=1 does the same to the tiled 64-32 shape at batch 1024."""
    _run(ssc, monkeypatch, obs_dim, h, B, llt, kind, env=env)


# what the second launch's statistics are updated with: 400 more rows around a shifted mean, 1.6 times as wide
_SHIFT = np.array([0.6, -0.4, 2.0])


@pytest.mark.parametrize("h,B", [((64, 32), 64), ((64, 32), 128), ((128, 64), 64)])
def test_statistics_move_between_launches(ssc, monkeypatch, h, B):
    """3 iterations, ObsRms.update_rows on the same object (every mean and std moves by more than 1e-2, asserted), 3 more
    on the same agent -- ddpg_train_fixed_kernel<3, true, false, ..>, <3, true, true, ..> and ddpg_wide_grad_kernel<..>;
    the oracle normalises each half with the statistics of its launch.  A mean or std kept across launches fails."""
    monkeypatch.delenv("SSC_DDPG_WIDE", raising=False)
    monkeypatch.delenv("SSC_DDPG_INTERPRETER", raising=False)
    rms, obs_range = rms_edge_stats(3, "wide")
    rows = np.random.default_rng(33).normal(RMS_EDGE_MEAN[:3] + _SHIFT, 1.6 * RMS_EDGE_STD[:3], size=(400, 3)).astype(np.float32)
    _ddpg_kernel_vs_oracle(ssc, 3, h[0], h[1], B=B, llts=(True,), cap=5000, obs_rms=rms, obs_range=obs_range, rms_rows=rows)
