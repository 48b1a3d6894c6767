#!/usr/bin/env python3
"""The SmartStart navigator on its own, everything resident in HBM:

  1. random-policy rollouts of N envs (one fused launch) -> (s, a, s' - s) training set, statistics, z-scores;
  2. Dyn_Model.train on the device (fused one-launch steps for one hidden layer, fp32-MFMA GEMMs otherwise);
     with --population P the models of P seeds train together, one launch per step for all of them;
  3. P envs each follow a recorded path with MPC as the rollout policy (HIP-graph replay of the 5-launch step);
     with --population P the envs of all seeds sit in ONE VecEnv and one graph steps them (navigator.NavigatorPopulation:
     the forward simulation of every seed's model is one ssc_mpc_forward_sim_many launch when the models are fp32 1 x <=128
     and one ssc_mpc_forward_sim_many_mfma launch when they are bf16 MFMA models of one class -- the default, and any
     --layers / --depth with one hidden layer up to 512 units or two up to 128; the sim_ways line names the way per model).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd import collect_samples as cs, navigator as nav, numerical as num  # noqa: E402
from smartstartcontinuous_amd.agents import init_dynamics_weights  # noqa: E402


def collect(args, seed):
    """random-policy rollouts of one seed -> (collector, z-scored inputs, outputs, statistics)"""
    env1 = ssc.make("MountainCarContinuous-v0", seed=seed)
    t0 = time.perf_counter()
    collector = cs.CollectSamples(env1, cs.Policy_Random(env1), seed=seed)
    ts = collector.collect_dataset(args.rollouts, args.steps_per_rollout)
    (mx, sx), (my, sy), (mz, sz) = (cs.column_stats(v) for v in (ts.dataX, ts.dataY, ts.dataZ))
    inputs = torch.empty((len(ts), 3), device="cuda")
    cs.zscore_into(ts.dataX, mx, sx, inputs, 0)
    cs.zscore_into(ts.dataY, my, sy, inputs, 2)
    outputs = cs.zscore_into(ts.dataZ, mz, sz, torch.empty_like(ts.dataZ))
    torch.cuda.synchronize()
    print("seed %d data set: %d rows from %d rollouts in %.1f ms" % (seed, len(ts), args.rollouts, (time.perf_counter() - t0) * 1e3))
    host = lambda t: t.cpu().numpy()
    norm = dict(mean_x=host(mx), std_x=host(sx), mean_y=host(my), std_y=host(sy), mean_z=host(mz), std_z=host(sz))
    return collector, inputs, outputs, norm


def plans(args, collector):
    """the states of args.problems recorded validation rollouts and the plans (waypoints, distances left, radii) along them"""
    states, _, _, _ = collector.collect_samples(args.problems, 200)
    wps, lefts, radii = [], [], []
    for path in states:
        stds, means = num.path_deltas_stds_and_means_per_dim(path)
        rad = num.radii_calc(means, stds, 1, 1, 1)
        dist = num.elliptical_euclidean_distance_function_generator(rad)
        short = num.path_shortcutter(path, dist, 1)
        wp = np.asarray(num.get_start_waypoints_final_states_steps(short, 1))
        wps.append(wp); radii.append(rad); lefts.append(num.distances_left(wp, dist))
    return states, wps, lefts, radii


def follow(args, seed, model, collector):
    """every problem follows the states of one recorded validation rollout"""
    states, wps, lefts, radii = plans(args, collector)
    P = args.problems
    problems = nav.MpcProblemSet(wps, lefts, radii, [0] * P, theta=1.0, gamma=0.75, horizontal_penalty_factor=0.5)
    batch = nav.NavigatorBatch(model, problems, num_control_samples=args.samples, horizon=args.horizon, seed=seed)
    venv = ssc.VecEnv("MountainCarContinuous-v0", P, seed=seed + 2)
    venv.reset()
    start = torch.as_tensor(np.stack([p[0] for p in states]), dtype=torch.float32, device="cuda")
    venv.s0.copy_(start[:, 0]); venv.s1.copy_(start[:, 1])
    venv.rollout(8, policy=ssc.MpcPolicy(batch))            # warm-up + graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    venv.rollout(args.follow_steps, policy=ssc.MpcPolicy(batch))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    idx = batch.problems.cur_idx.cpu().numpy() if hasattr(batch.problems, "cur_idx") else None
    print("seed %d: %d envs followed their paths for %d MPC steps (%d x %d samples, horizon %d) in %.1f ms = %.3f ms per step"
          % (seed, P, args.follow_steps, P, args.samples, args.horizon, dt * 1e3, dt * 1e3 / args.follow_steps))
    if idx is not None:
        print("waypoint reached per env:", idx.tolist(), "of", [len(w) for w in wps])


def follow_population(args, seeds, pop, collectors):
    """the navigators of ALL seeds in one VecEnv of len(seeds) * args.problems envs: env range p follows seed p's paths with
    seed p's dynamics model, one captured graph steps everybody (navigator.NavigatorPopulation)"""
    states, wps, lefts, radii = [], [], [], []
    for collector in collectors:
        for have, new in zip((states, wps, lefts, radii), plans(args, collector)):
            have.extend(new)
    n = len(states)
    problems = nav.MpcProblemSet(wps, lefts, radii, [0] * n, theta=1.0, gamma=0.75, horizontal_penalty_factor=0.5)
    batch = nav.NavigatorPopulation(pop, problems, args.problems, num_control_samples=args.samples, horizon=args.horizon,
                                    seed=seeds[0])
    venv = ssc.VecEnv("MountainCarContinuous-v0", n, seed=seeds[0] + 2)
    venv.reset()
    start = torch.as_tensor(np.stack([p[0] for p in states]), dtype=torch.float32, device="cuda")
    venv.s0.copy_(start[:, 0]); venv.s1.copy_(start[:, 1])
    venv.rollout(8, policy=ssc.MpcPolicy(batch))            # warm-up + graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    venv.rollout(args.follow_steps, policy=ssc.MpcPolicy(batch))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    idx = problems.cur_idx.cpu().numpy()
    print("seeds %s: %d envs followed their paths for %d MPC steps from ONE graph (%d x %d samples, horizon %d) in %.1f ms = "
          "%.3f ms per step\nsim_ways: %s"
          % (seeds, n, args.follow_steps, n, args.samples, args.horizon, dt * 1e3, dt * 1e3 / args.follow_steps,
             ", ".join(batch.sim_ways)))
    for p, seed in enumerate(seeds):
        sl = slice(p * args.problems, (p + 1) * args.problems)
        print("seed %d waypoint reached per env:" % seed, idx[sl].tolist(), "of", [len(w) for w in wps[sl]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--steps-per-rollout", type=int, default=333)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--problems", type=int, default=16)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--follow-steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--population", type=int, default=1,
                    help="P seeds collect their own data, train their models TOGETHER (one launch per Adam step for all of "
                         "them: navigator.DynamicsModelPopulation) and follow their paths in ONE VecEnv from one graph "
                         "(navigator.NavigatorPopulation)")
    ap.add_argument("--precision", choices=["bf16_mfma", "f32"], default="bf16_mfma",
                    help="forward simulation of the MPC: bf16 MFMA kernel (default) or the fp32 parity path")
    args = ap.parse_args()
    seeds = [args.seed + p for p in range(max(args.population, 1))]
    sets = [collect(args, seed) for seed in seeds]
    models = []
    for seed, (_, _, _, norm) in zip(seeds, sets):
        Ws, bs = init_dynamics_weights(3, 2, args.layers, args.depth, torch.Generator().manual_seed(seed))
        models.append(nav.DynamicsModel(Ws, bs, norm, 2, 1, precision=args.precision))
    none = (np.zeros((0, 3)), np.zeros((0, 2)))
    t0 = time.perf_counter()
    if args.population <= 1:
        losses = [models[0].train(sets[0][1], sets[0][2], *none, args.epochs, 0.0, rng=np.random.RandomState(args.seed))]
        how = "alone"
    else:
        pop = nav.DynamicsModelPopulation(models)
        losses = pop.train([(s[1], s[2]) + none for s in sets], args.epochs, 0.0, rngs=[np.random.RandomState(seed) for seed in seeds])
        how = "ways " + ", ".join(sorted(set(pop.ways)))
    steps = sum(args.epochs * (s[1].shape[0] // 512) for s in sets)
    print("trained %d model(s) %dx%d for %d epochs (%d steps, %s) in %.1f ms, last-epoch losses %s"
          % (len(models), args.layers, args.depth, args.epochs, steps, how, (time.perf_counter() - t0) * 1e3,
             ", ".join("%.4f" % v for v in losses)))
    if args.population <= 1:
        follow(args, seeds[0], models[0], sets[0][0])
    else:
        follow_population(args, seeds, pop, [s[0] for s in sets])


if __name__ == "__main__":
    main()
