"""Helpers shared by the -m gpu tests."""
import numpy as np


def mc_log(chunk):
    return dict(s_pos=chunk.obs[0].cpu().numpy(), s_vel=chunk.obs[1].cpu().numpy(), act=chunk.act.cpu().numpy(),
                rew=chunk.rew.cpu().numpy(), done=chunk.done.cpu().numpy(),
                s2_pos=chunk.obs2[0].cpu().numpy(), s2_vel=chunk.obs2[1].cpu().numpy())


def assert_replay_clean(res, tol_pos=2.4e-7, tol_vel=1e-8, tol_rew=1e-4):
    assert res["start_mismatch"] == 0, res
    assert res["act_mismatch"] == 0, res
    assert res["done_mismatch"] == 0, res
    assert res["continuity_mismatch"] == 0, res
    assert res["reset_mismatch"] == 0, res
    assert res["max_dpos"] <= tol_pos, res
    assert res["max_dvel"] <= tol_vel, res
    assert res["max_drew"] <= tol_rew, res


def actor_weights(obs_dim=2, h1=64, h2=32, seed=1234, w3_scale=3e-3):
    """glorot-uniform / U(+-3e-3) init like tf.layers.dense in models_editted.py:44-59."""
    rng = np.random.default_rng(seed)

    def glorot(i, o):
        lim = np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, size=(i, o)).astype(np.float32)
    return dict(W1=glorot(obs_dim, h1), b1=(0.1 * rng.normal(size=h1)).astype(np.float32),
                W2=glorot(h1, h2), b2=(0.1 * rng.normal(size=h2)).astype(np.float32),
                W3=rng.uniform(-w3_scale, w3_scale, size=(h2, 1)).astype(np.float32),
                b3=(0.05 * rng.normal(size=1)).astype(np.float32))


def x_hat64(x, obs_rms, obs_clip=5.0):
    """clip((x - mean) / std) in fp64 from the fp32 mean / std the kernels derive (``ObsRms.mean_std``): what the oracle
    is fed where the device normalises the raw observations itself."""
    mean, std = obs_rms.mean_std()
    return np.clip((np.asarray(x, np.float64) - mean.astype(np.float64)) / std.astype(np.float64), -obs_clip, obs_clip)


RMS_EDGE_MEAN = np.array([0.2, -0.1, 0.5, -0.4, 0.3, -0.25, 0.15, -0.35])
RMS_EDGE_STD = np.array([0.5, 0.25, 2.0, 0.4, 0.8, 0.3, 1.2, 0.6])
_FLOOR_HALF_WIDTH = 0.5 / 0.95        # |x - mean| > 0.5 = 5 floor stds is clipped: 5 % of a uniform draw


def rms_edge_stats(obs_dim, kind, seed=21):
    """(ObsRms, (low, high) of the raw observations to draw) of a statistics set that reaches an edge.  Both kinds have
    non-zero means that differ in every component.
      "floor" -- every std on the 0.1 floor; observations drawn 0.526 either side of the mean put 5 % of the components on
                 +clip or -clip and leave most rows clear of it;
      "wide"  -- every std above the floor and different in every component (a std or mean taken from a neighbouring
                 component cannot cancel); observations within 3 std of the mean: nothing is clipped."""
    from smartstartcontinuous_amd.obs_rms import ObsRms
    mean = RMS_EDGE_MEAN[:obs_dim]
    rng = np.random.default_rng(seed + obs_dim)
    if kind == "floor":
        rows, half = rng.normal(mean, 0.02, size=(500, obs_dim)), _FLOOR_HALF_WIDTH
    else:
        assert kind == "wide"
        rows, half = rng.normal(mean, RMS_EDGE_STD[:obs_dim], size=(400, obs_dim)), 3 * RMS_EDGE_STD[:obs_dim]
    rms = ObsRms(obs_dim)
    rms.update_rows(rows.astype(np.float32))
    got_mean, got_std = rms.mean_std()
    assert np.all(np.abs(got_mean) > 0.05)
    if kind == "floor":
        assert np.all(got_std == np.float32(0.1))
    else:
        assert np.all(got_std > 0.2)
    if obs_dim >= 3:     # three different means and stds in the first three components
        assert len(set(got_mean[:3])) == 3
        assert kind == "floor" or len(set(got_std[:3])) == 3
    return rms, (mean - half, mean + half)
