"""What ``ssc_ddpg_eval_rollout`` must report, restated in numpy from a transition trace (CPU only; shared by
tests/test_gpu_ddpg_eval*.py and tests/test_ddpg_eval_host.py).

The running return of an env is the fp32 sum of its rewards in step order -- from 0 (``zero_returns``: the reference zeroes
eval_episode_reward and keeps the episode, training_editted.py:125) or from the env's carried ``ep_ret`` -- and restarts
at 0 behind every done.  An episode's length is the TimeLimit counter at its done (it counts from ``steps0``, the steps the
episode had before the trace).  Means and population stds are numpy's float64 two-pass ones."""
import numpy as np

N_EVAL = 8


def eval_block(rew, done, goal, q, steps0, ep_ret0, zero_returns):
    """rew, q [K, N] fp32; done, goal [K, N] bool; steps0 [N] int; ep_ret0 [N] fp32.
    -> (block [8] float64 in EVAL_NAMES order, final running return [N] fp32, final step counter [N] int64)"""
    rew, q = np.asarray(rew, np.float32), np.asarray(q, np.float32)
    done, goal = np.asarray(done).astype(bool), np.asarray(goal).astype(bool)
    K, N = rew.shape
    run = np.zeros(N, np.float32) if zero_returns else np.asarray(ep_ret0, np.float32).copy()
    el = np.asarray(steps0, np.int64).copy()
    rets, lens, goals = [], [], 0
    for k in range(K):
        run = (run + rew[k]).astype(np.float32)                  # one fp32 addition per step
        el = el + 1
        d = done[k]
        rets.extend(run[d].astype(np.float64).tolist())
        lens.extend(el[d].tolist())
        goals += int(np.sum(goal[k] & d))
        run = np.where(d, np.float32(0), run).astype(np.float32)
        el = np.where(d, 0, el)
    nan = float("nan")
    rets, lens, q64 = np.asarray(rets, np.float64), np.asarray(lens, np.float64), q.astype(np.float64).reshape(-1)
    block = np.array([len(rets), rets.mean() if len(rets) else nan, rets.std() if len(rets) else nan, q64.mean(), q64.std(),
                      K * N, goals, lens.mean() if len(lens) else nan], np.float64)
    return block, run, el


def assert_block(got, want):
    """counts (slots 0, 5, 6) exact; means and stds to 1e-10 * max(1, |value|); NaN where NaN is due"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (N_EVAL,)
    for slot in (0, 5, 6):
        assert got[slot] == want[slot], (slot, got[slot], want[slot])
    for slot in (1, 2, 3, 4, 7):
        if np.isnan(want[slot]):
            assert np.isnan(got[slot]), (slot, got[slot])
        else:
            assert abs(got[slot] - want[slot]) <= 1e-10 * max(1.0, abs(want[slot])), (slot, got[slot], want[slot])
