#!/usr/bin/env python3
"""DDPG on the edited continuous MountainCar, two ways on one MI355X:

  * ``--mode single``: the reference's own call structure (examples/continuous/DDPG_Baselines_example.py:28-80 --
    make_timed_env -> DDPG_Baselines_agent -> rlTrain -> Summary.save) with the env, the actor/critic and the
    train step running through libssc.so;
  * ``--mode vec``: the vectorised actor-learner loop -- N envs roll out under the current actor in fused
    chunks, the transitions go into a device replay ring, the learner runs on minibatches drawn from it; nothing
    but the loss scalars and the finished-episode records leaves HBM.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import smartstartcontinuous_amd as ssc  # noqa: E402
from smartstartcontinuous_amd.agents import DDPG_Baselines_agent  # noqa: E402


def make_agent(env, seed, normalize_observations=False, param_noise=None, popart=False, hidden=(64, 32)):
    return DDPG_Baselines_agent(env, None, buffer_size=100000, batch_size=64, num_train_iterations=50,
                                num_steps_before_train=200, ou_epsilon=1.0, ou_min_epsilon=0.01,
                                ou_epsilon_decay_factor=.99, ou_mu=0.4, ou_sigma=0.6, ou_theta=.15, actor_lr=0.001,
                                actor_h1=hidden[0], actor_h2=hidden[1], critic_lr=0.001, critic_h1=hidden[0], critic_h2=hidden[1],
                                lastLayerTanh=True, normalize_observations=normalize_observations, seed=seed,
                                param_noise_stddev=param_noise, normalize_returns=popart, enable_popart=popart)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["single", "vec"], default="vec")
    ap.add_argument("--power-scalar", type=float, default=1.0)
    ap.add_argument("--episodes", type=int, default=5, help="single: episodes to run")
    ap.add_argument("--envs", type=int, default=4096, help="vec: parallel envs")
    ap.add_argument("--chunks", type=int, default=20, help="vec: rollout chunks of 250 steps")
    ap.add_argument("--overlap", action="store_true",
                    help="vec: roll chunk i+1 on a second stream while the learner works on chunk i (one chunk stale)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--population", type=int, default=None, metavar="P",
                    help="vec: P agents with seeds SEED .. SEED + P - 1 on envs of their own, trained by one learner launch per chunk "
                         "(rl_train_vec_ddpg_population); prints each seed's late-window return")
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--normalize-observations", action="store_true",
                    help="DDPG normalize_observations: networks see running-statistics-normalised observations")
    ap.add_argument("--param-noise", default=None, metavar="STDDEV[,STDDEV...]",
                    help="adaptive parameter-space noise with this initial (and desired action) stddev, on top of the OU noise; "
                         "with --population a comma list sweeps it: pair p takes entry p modulo the list's length")
    ap.add_argument("--hidden", default=None, metavar="H1-H2[,H1-H2...]",
                    help="hidden layer sizes of actor and critic (default 64-32); with --population a comma list sweeps them, "
                         "e.g. 64-32,128-64,200-100 (the reference's hidden_layer_size_experiment): pair p takes entry p modulo "
                         "the list's length, the 64-32 agents train in the one-workgroup launch and the wider ones in the grouped "
                         "multi-workgroup launches")
    ap.add_argument("--popart", action="store_true",
                    help="DDPG normalize_returns + enable_popart: the critic learns normalised returns, its output layer is "
                         "rescaled with the running return statistics (Pop-Art); with --population the Pop-Art agents, whatever "
                         "their --hidden sizes, train together in grouped launches (ssc_ddpg_train_many_popart)")
    ap.add_argument("--stats-every", type=int, default=None, metavar="K",
                    help="the reference's training diagnostics (get_stats): vec: logged on the device every K chunks and printed "
                         "after the run; single: printed every K episodes")
    ap.add_argument("--eval-every", type=int, default=None, metavar="K",
                    help="vec: the reference's evaluation block (eval/return, eval/Q: the actor without noise on envs of its own) "
                         "every K chunks, logged on the device and printed after the run")
    ap.add_argument("--eval-envs", type=int, default=128, metavar="E", help="vec: evaluation envs")
    ap.add_argument("--eval-steps", type=int, default=None, metavar="S", help="vec: steps per evaluation (default: the time limit)")
    args = ap.parse_args()
    stddevs = None
    if args.param_noise is not None:
        try:
            stddevs = [float(x) for x in args.param_noise.split(",")]
        except ValueError:
            ap.error("--param-noise takes a number or a comma list of numbers")
        if len(stddevs) > 1 and args.population is None:
            ap.error("a list of --param-noise values needs --population")
        args.param_noise = stddevs[0]
    hidden = [(64, 32)]
    if args.hidden is not None:
        try:
            hidden = [tuple(int(x) for x in h.split("-")) for h in args.hidden.split(",")]
        except ValueError:
            hidden = []
        if not hidden or any(len(h) != 2 or min(h) < 1 for h in hidden):
            ap.error("--hidden takes H1-H2 or a comma list of them")
        if len(hidden) > 1 and args.population is None:
            ap.error("a list of --hidden values needs --population")
    np.random.seed(args.seed)
    if args.mode == "single":
        env = ssc.Continuous_MountainCarEnv_Editted.make_timed_env(args.power_scalar, max_episode_steps=1000,
                                                                   seed=args.seed)
        agent = make_agent(env, args.seed, args.normalize_observations, args.param_noise, args.popart, hidden[0])
        if args.stats_every is None:
            summary = ssc.rlTrain(agent, env, print_results=True, print_steps=False, num_episodes=args.episodes,
                                  max_steps=1000)
        else:                                  # one rlTrain call per episode, the diagnostics between them
            summary = None
            for episode in range(args.episodes):
                one = ssc.rlTrain(agent, env, print_results=True, print_steps=False, num_episodes=1, max_steps=1000)
                if summary is None:
                    summary = one
                else:
                    summary.append_record(*one.episodes[0])
                if (episode + 1) % args.stats_every == 0 and len(agent.replay_buffer) >= agent.batch_size:
                    print("  stats:", ", ".join("%s %.6g" % kv for kv in agent.get_stats().items()))
    elif args.population is not None:
        if args.overlap:
            ap.error("--population runs the synchronous loop")
        env_id = "MountainCarContinuousActionX%s-v0" % args.power_scalar
        P = args.population
        seeds = [args.seed + p for p in range(P)]
        envs = [ssc.VecEnv(env_id, args.envs, seed=s, env_id0=p * args.envs) for p, s in enumerate(seeds)]
        noise = [None if stddevs is None else stddevs[p % len(stddevs)] for p in range(P)]
        agents = [make_agent(ssc.SingleEnvView(ssc.VecEnv(env_id, 1, seed=s)), s, args.normalize_observations, sd, args.popart,
                             hidden[p % len(hidden)])
                  for p, (s, sd) in enumerate(zip(seeds, noise))]
        eval_envs = None
        if args.eval_every is not None:        # envs of their own per pair: another seed, ids behind all training envs'
            eval_envs = [ssc.VecEnv(env_id, args.eval_envs, seed=s + P, env_id0=P * args.envs + p * args.eval_envs)
                         for p, s in enumerate(seeds)]
        monitor = ssc.PopulationMonitor(eval_envs=eval_envs, eval_every=args.eval_every, eval_steps=args.eval_steps,
                                        stats_every=args.stats_every)
        runs = ssc.rl_train_vec_ddpg_population(envs, agents, num_chunks=args.chunks, chunk_steps=250, replay_capacity=1 << 20,
                                                train_iters=50, seed=seeds, monitor=monitor,
                                                param_noise_cycle=stddevs is not None)
        last = lambda log, k: next((v for v in log[k][::-1] if not np.isnan(v)), float("nan"))   # the last row that was written
        for s, agent, (summary, losses, replay) in zip(seeds, agents, runs):   # one line per pair
            late = [ret for _steps, ret in summary.episodes[-max(1, len(summary) // 4):]]
            line = ("seed %d (%d-%d): %d finished episodes, late-window return %.2f (last quarter of them), last critic/actor loss %.4g / %.4g"
                    % (s, agent.h1, agent.h2, len(summary), float(np.mean(late)) if late else float("nan"), *losses[-1][-1].tolist()))
            if args.eval_every is not None:
                line += ", eval/return %.2f eval/Q %.4g over %.0f episodes" % (
                    last(summary.eval_stats, "eval/return"), last(summary.eval_stats, "eval/Q"), last(summary.eval_stats, "eval/episodes"))
            if args.stats_every is not None:
                line += ", reference_Q_mean %.4g reference_action_std %.4g" % (
                    last(summary.agent_stats, "reference_Q_mean"), last(summary.agent_stats, "reference_action_std"))
            if agent.param_noise is not None:
                line += ", param_noise_stddev %.4g -> %.4g" % (agent.param_noise.initial_stddev, agent.param_noise.current_stddev)
            print(line)
        if args.save_dir:
            os.makedirs(args.save_dir, exist_ok=True)
            for s, (summary, _l, _r) in zip(seeds, runs):
                print("summary written to", summary.save(args.save_dir, post_fix=s))
        return
    else:
        env = ssc.VecEnv("MountainCarContinuousActionX%s-v0" % args.power_scalar, args.envs, seed=args.seed)
        agent = make_agent(ssc.SingleEnvView(ssc.VecEnv(env.spec.id, 1, seed=args.seed)), args.seed, args.normalize_observations,
                           args.param_noise, args.popart, hidden[0])
        eval_kw = {}
        if args.eval_every is not None:        # envs of their own: another seed, ids behind the training envs'
            eval_kw = dict(eval_env=ssc.VecEnv(env.spec.id, args.eval_envs, seed=args.seed + 1, env_id0=args.envs),
                           eval_every=args.eval_every, eval_steps=args.eval_steps)
        summary, losses, replay = ssc.rl_train_vec_ddpg(env, agent, num_chunks=args.chunks, chunk_steps=250,
                                                        replay_capacity=1 << 20, train_iters=50, overlap=args.overlap,
                                                        stats_every=args.stats_every, **eval_kw)
        goals = sum(1 for steps, ret in summary.episodes if ret > 0)
        print("%d env-steps, %d finished episodes (%d reached the goal), %d records in the replay ring, "
              "last critic/actor loss %.4g / %.4g" % (args.envs * args.chunks * 250, len(summary), goals, len(replay),
                                                      *losses[-1][-1].tolist()))
        if args.stats_every is not None:
            shown = [k for k, v in summary.agent_stats.items() if not np.all(np.isnan(v))]
            print("chunk  " + "  ".join(shown))
            for row, chunk in enumerate(summary.agent_stats_chunks):
                print("%5d  " % chunk + "  ".join("%*.6g" % (len(k), summary.agent_stats[k][row]) for k in shown))
        if args.eval_every is not None:
            names = list(summary.eval_stats)
            print("chunk  " + "  ".join(names))
            for row, chunk in enumerate(summary.eval_chunks):
                print("%5d  " % chunk + "  ".join("%*.6g" % (len(k), summary.eval_stats[k][row]) for k in names))
    if agent.ret_rms is not None:
        print("return statistics: mean %.6g, std %.6g" % tuple(float(x[0]) for x in agent.ret_rms.mean_std()))
    if agent.param_noise is not None:
        print("parameter noise:", agent.param_noise.get_stats())
    if args.save_dir:
        os.makedirs(args.save_dir, exist_ok=True)
        print("summary written to", summary.save(args.save_dir))
    print("episodes: %d, best total reward %.2f" % (len(summary), summary.best_reward))


if __name__ == "__main__":
    main()
