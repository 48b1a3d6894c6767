"""ctypes binding of libssc.so (include/ssc.h).

The HIP library is the product; there is NO CPU fallback.  Importing this module without a
built ``libssc.so`` raises immediately (build it with ``python -m smartstartcontinuous_amd.build``
or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# SSC_LIB_PATH: development override (A/B of variant builds under tools/, e.g. tools/gpu_variant_ab.sh) -- the
# package itself always ships and loads the in-tree libssc.so
LIB_PATH = os.environ.get("SSC_LIB_PATH") or os.path.join(_HERE, "libssc.so")

SSC_OK, SSC_EINVAL, SSC_EUNSUPPORTED, SSC_EHIP = 0, -1, -2, -3
SSC_ENV_MOUNTAINCAR, SSC_ENV_PENDULUM = 0, 1
SSC_POLICY_RANDOM, SSC_POLICY_ACTOR = 0, 1
SSC_PREC_F32, SSC_PREC_BF16_MFMA, SSC_PREC_BF16_MFMA_PREPARED = 0, 1, 2
SSC_MAX_OBS, SSC_MAX_LAYERS, SSC_MAX_STATE, SSC_MAX_ACT = 3, 4, 8, 4
SSC_DDPG_N_STATS = 11
SSC_DDPG_N_EVAL = 8


class SscError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libssc error {code}: {msg}")
        self.code = code


class EnvParams(Structure):
    _fields_ = [("kind", c_int32), ("max_episode_steps", c_int32),
                ("min_action", c_float), ("max_action", c_float),
                ("min_position", c_float), ("max_position", c_float),
                ("max_speed", c_float), ("goal_position", c_float), ("power", c_float),
                ("reset_low", c_float), ("reset_high", c_float),
                ("max_torque", c_float), ("pend_max_speed", c_float), ("dt", c_float),
                ("g", c_float), ("m", c_float), ("l", c_float), ("pend_v1_order", c_int32)]


class ActorDesc(Structure):
    _fields_ = [("obs_dim", c_int32), ("h1", c_int32), ("h2", c_int32), ("act_dim", c_int32),
                ("W1", c_void_p), ("b1", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
                ("W3", c_void_p), ("b3", c_void_p),
                ("last_layer_tanh", c_int32), ("precision", c_int32), ("obs_clip", c_float),
                ("ln1_g", c_void_p), ("ln1_b", c_void_p), ("ln2_g", c_void_p), ("ln2_b", c_void_p)]


class OuDesc(Structure):
    _fields_ = [("mu", c_float), ("sigma", c_float), ("theta", c_float), ("dt", c_float), ("epsilon", c_float),
                ("d_epsilon", c_void_p)]


class PolicyDesc(Structure):
    _fields_ = [("kind", c_int32), ("act_low", c_float), ("act_high", c_float),
                ("actor", ActorDesc), ("ou", OuDesc)]


class RolloutState(Structure):
    _fields_ = [("s0", c_void_p), ("s1", c_void_p), ("steps", c_void_p), ("ep_ret", c_void_p), ("ou_x", c_void_p)]


class TransitionLog(Structure):
    _fields_ = [("obs", c_void_p * SSC_MAX_OBS), ("act", c_void_p), ("rew", c_void_p), ("done", c_void_p),
                ("obs2", c_void_p * SSC_MAX_OBS), ("row_stride", c_int64), ("done_row_stride", c_int64)]


class EpisodeRing(Structure):
    _fields_ = [("env_id", c_void_p), ("length", c_void_p), ("ret", c_void_p), ("cursor", c_void_p),
                ("capacity", c_int32)]


class MlpDesc(Structure):
    _fields_ = [("n_layers", c_int32), ("dims", c_int32 * (SSC_MAX_LAYERS + 1)),
                ("W", c_void_p * SSC_MAX_LAYERS), ("b", c_void_p * SSC_MAX_LAYERS)]


class Norm(Structure):
    _fields_ = [("mean_x", c_float * SSC_MAX_STATE), ("std_x", c_float * SSC_MAX_STATE),
                ("mean_y", c_float * SSC_MAX_ACT), ("std_y", c_float * SSC_MAX_ACT),
                ("mean_z", c_float * SSC_MAX_STATE), ("std_z", c_float * SSC_MAX_STATE)]


class MpcNavState(Structure):
    _fields_ = [("cur_idx", c_void_p), ("start_idx", c_void_p), ("actions_done", c_void_p), ("at_goal", c_void_p),
                ("give_up_after", c_int32), ("final_steps", c_int32)]


class MpcProblems(Structure):
    _fields_ = [("n_problems", c_int32), ("n_samples", c_int32), ("horizon", c_int32), ("state_dim", c_int32),
                ("wp", c_void_p), ("left", c_void_p), ("wp_off", c_void_p), ("cur_idx", c_void_p),
                ("radii", c_void_p), ("theta", c_float), ("gamma", c_float),
                ("horizontal_penalty_factor", c_float), ("per_row_projection", c_int32),
                ("plan_of", c_void_p), ("wp_len", c_void_p), ("active", c_void_p),
                ("live_list", c_void_p), ("n_live", c_void_p)]


class SmartStartStep(Structure):
    _fields_ = [("mode", c_void_p), ("plan_of", c_void_p), ("d_actor_out", c_void_p), ("d_eta", c_void_p),
                ("d_ou_epsilon", c_void_p), ("d_pool", c_void_p), ("ou", OuDesc), ("act_low", c_float), ("act_high", c_float),
                ("d_mode_log", c_void_p), ("mode_log_stride", c_int64), ("d_n_live", c_void_p)]


class MpcSampling(Structure):
    _fields_ = [("n_samples", c_int32), ("low", c_float * SSC_MAX_ACT), ("high", c_float * SSC_MAX_ACT),
                ("seed", c_uint64), ("problem_id0", c_uint64), ("t", c_uint64), ("d_t_base", c_void_p),
                ("d_problem_active", c_void_p), ("d_live_list", c_void_p), ("d_n_live", c_void_p)]


class CriticDesc(Structure):
    _fields_ = [("obs_dim", c_int32), ("act_dim", c_int32), ("h1", c_int32), ("h2", c_int32),
                ("W1", c_void_p), ("b1", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
                ("W3", c_void_p), ("b3", c_void_p), ("last_layer_tanh", c_int32), ("obs_clip", c_float),
                ("ln1_g", c_void_p), ("ln1_b", c_void_p), ("ln2_g", c_void_p), ("ln2_b", c_void_p)]


class MlpTrainDesc(Structure):
    _fields_ = [("n_layers", c_int32), ("dims", c_int32 * (SSC_MAX_LAYERS + 1)),
                ("W", c_void_p * SSC_MAX_LAYERS), ("b", c_void_p * SSC_MAX_LAYERS),
                ("mW", c_void_p * SSC_MAX_LAYERS), ("vW", c_void_p * SSC_MAX_LAYERS),
                ("mb", c_void_p * SSC_MAX_LAYERS), ("vb", c_void_p * SSC_MAX_LAYERS),
                ("adam_t", c_void_p), ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("epsilon", c_float)]


class MlpTrainManyItem(Structure):
    _fields_ = [("net", MlpTrainDesc), ("d_X", c_void_p), ("d_Z", c_void_p), ("d_idx", c_void_p), ("batch", c_int32),
                ("n_steps", c_int32), ("d_loss", c_void_p), ("d_workspace", c_void_p), ("workspace_bytes", c_size_t)]


class MpcSimManyItem(Structure):
    _fields_ = [("mlp", MlpDesc), ("norm", Norm), ("problem0", c_int32), ("n_problems", c_int32)]


class MpcSimManyMfmaItem(Structure):
    _fields_ = [("mlp", MlpDesc), ("d_image", c_void_p), ("image_bytes", c_size_t), ("problem0", c_int32),
                ("n_problems", c_int32)]


class ActorManyItem(Structure):
    _fields_ = [("actor", ActorDesc), ("d_rms", c_void_p), ("row0", c_int64), ("rows", c_int64)]


class SmartStartPair(Structure):
    _fields_ = [("env0", c_int32), ("n_envs", c_int32), ("slot0", c_int32), ("pool_first", c_int32), ("pool_count", c_int32),
                ("pool_slots", c_int32), ("eta", c_float), ("ou_epsilon", c_float), ("ou", OuDesc)]


class DdpgDesc(Structure):
    _fields_ = [("obs_dim", c_int32), ("act_dim", c_int32), ("actor_h1", c_int32), ("actor_h2", c_int32),
                ("critic_h1", c_int32), ("critic_h2", c_int32), ("last_layer_tanh", c_int32), ("batch_size", c_int32),
                ("actor", c_void_p), ("critic", c_void_p), ("target_actor", c_void_p), ("target_critic", c_void_p),
                ("adam_m_actor", c_void_p), ("adam_v_actor", c_void_p), ("adam_m_critic", c_void_p),
                ("adam_v_critic", c_void_p), ("adam_t", c_void_p),
                ("gamma", c_float), ("tau", c_float), ("actor_lr", c_float), ("critic_lr", c_float),
                ("beta1", c_float), ("beta2", c_float), ("epsilon", c_float), ("obs_clip", c_float), ("layer_norm", c_int32),
                ("critic_l2_reg", c_float), ("clip_norm", c_float)]


class ReplayView(Structure):
    _fields_ = [("s", c_void_p), ("a", c_void_p), ("r", c_void_p), ("t", c_void_p), ("s2", c_void_p),
                ("capacity", c_int64)]


class ReplayRing(Structure):
    _fields_ = [("s", c_void_p), ("a", c_void_p), ("r", c_void_p), ("t", c_void_p), ("s2", c_void_p),
                ("capacity", c_int64), ("obs_dim", c_int32), ("act_dim", c_int32),
                ("ep_steps", c_void_p), ("ep_run", c_void_p)]


class SelectManyItem(Structure):
    _fields_ = [("ring", ReplayRing), ("count", c_int64), ("n", c_int64), ("n_ss", c_int32), ("n_plans", c_int32),
                ("seed", c_uint64), ("counter", c_uint64), ("stride", c_int64), ("n_data", c_int64), ("scott", c_double),
                ("actor", ActorDesc), ("critic", CriticDesc), ("d_rms", c_void_p), ("alpha", c_float), ("beta", c_float),
                ("volume", c_double), ("max_len", c_int32), ("pad", c_int32), ("row0", c_int64), ("d_idx", c_void_p),
                ("d_n_cand", c_void_p), ("d_cand", c_void_p), ("d_wh", c_void_p), ("d_norm", c_void_p), ("d_status", c_void_p),
                ("d_value", c_void_p), ("d_pdf", c_void_p), ("d_ucb", c_void_p), ("d_chosen", c_void_p), ("d_path", c_void_p),
                ("d_len", c_void_p), ("d_workspace", c_void_p), ("workspace_bytes", c_size_t)]


class DdpgManyItem(Structure):
    _fields_ = [("ddpg", DdpgDesc), ("replay", ReplayView), ("d_batch_idx", c_void_p), ("d_losses", c_void_p),
                ("d_rms", c_void_p), ("n_iters", c_int32)]


class DdpgManyWideItem(Structure):
    _fields_ = DdpgManyItem._fields_ + [("d_workspace", c_void_p), ("workspace_bytes", c_size_t)]


class DdpgManyPopartItem(Structure):
    _fields_ = DdpgManyWideItem._fields_ + [("d_ret_rms", c_void_p)]


# ssc_ddpg_learner_path's answers
SSC_DDPG_PATH_FIXED, SSC_DDPG_PATH_FIXED_TILED, SSC_DDPG_PATH_INTERPRETER, SSC_DDPG_PATH_WIDE, SSC_DDPG_PATH_NEEDS_WORKSPACE = range(5)


class ReplaySampleKey(Structure):
    _fields_ = [("seed", c_uint64), ("counter0", c_uint64), ("size", c_int64)]


class PairCursor(Structure):
    _fields_ = [("step0", c_uint64), ("replay_start", c_int64)]


class RolloutManyItem(Structure):
    _fields_ = [("params", EnvParams), ("policy", PolicyDesc), ("n", c_int64), ("state", RolloutState), ("log", TransitionLog),
                ("ring", EpisodeRing), ("has_log", c_int32), ("has_ring", c_int32), ("d_stats", c_void_p), ("seed", c_uint64),
                ("env_id0", c_uint64), ("d_rms", c_void_p)]


class ReplayAppendItem(Structure):
    _fields_ = [("ring", ReplayRing), ("log", TransitionLog), ("K", c_int32), ("n", c_int64), ("reward_scale", c_float)]


class DecayItem(Structure):
    _fields_ = [("d_finished", c_void_p), ("finished0", c_double), ("per_generation", c_double), ("n_sched", c_int32),
                ("factor", c_double * 4), ("floor", c_double * 4), ("d_state", c_void_p), ("d_out", c_void_p * 4)]


class ObsRmsItem(Structure):
    _fields_ = [("log", TransitionLog), ("k0", c_int32), ("K", c_int32), ("n", c_int64), ("d_rms", c_void_p),
                ("d_workspace", c_void_p), ("workspace_bytes", c_size_t)]


class DdpgEvalManyItem(Structure):
    _fields_ = [("params", EnvParams), ("actor", ActorDesc), ("critic", CriticDesc), ("act_low", c_float), ("act_high", c_float),
                ("n", c_int64), ("state", RolloutState), ("d_rms", c_void_p), ("d_out", c_void_p), ("d_workspace", c_void_p),
                ("workspace_bytes", c_size_t), ("seed", c_uint64), ("env_id0", c_uint64)]


class DdpgStatsManyItem(Structure):
    _fields_ = [("actor", ActorDesc), ("critic", CriticDesc), ("perturbed", ActorDesc), ("has_perturbed", c_int32), ("m", c_int64),
                ("d_obs", c_void_p), ("d_act", c_void_p), ("d_rms", c_void_p), ("d_param_noise_stddev", c_void_p),
                ("d_out", c_void_p), ("d_workspace", c_void_p), ("workspace_bytes", c_size_t)]


class ParamNoiseManyItem(Structure):
    _fields_ = [("actor", ActorDesc), ("d_obs", c_void_p), ("d_idx", c_void_p), ("d_rms", c_void_p), ("n", c_int64),
                ("d_src", c_void_p), ("skip0_begin", c_int64), ("skip0_end", c_int64), ("skip1_begin", c_int64),
                ("skip1_end", c_int64), ("seed", c_uint64), ("desired", c_float), ("coefficient", c_float),
                ("d_stddev", c_void_p), ("d_distance", c_void_p), ("d_dst", c_void_p)]


class ParamNoiseCursor(Structure):
    _fields_ = [("generation_adaptive", c_uint64), ("generation_acting", c_uint64), ("m", c_int32), ("pad", c_int32)]


# C struct -> its ctypes mirror: the struct-layout table (the tests compare sizeof / offsetof as the C compiler sees them)
STRUCTS = {
    "ssc_env_params": EnvParams, "ssc_actor_desc": ActorDesc, "ssc_ou_desc": OuDesc, "ssc_policy_desc": PolicyDesc,
    "ssc_rollout_state": RolloutState, "ssc_transition_log": TransitionLog, "ssc_episode_ring": EpisodeRing,
    "ssc_mlp_desc": MlpDesc, "ssc_norm": Norm, "ssc_mpc_problems": MpcProblems, "ssc_mpc_sampling": MpcSampling,
    "ssc_mpc_nav_state": MpcNavState, "ssc_smartstart_step": SmartStartStep, "ssc_critic_desc": CriticDesc,
    "ssc_ddpg_desc": DdpgDesc, "ssc_replay_view": ReplayView, "ssc_replay_ring": ReplayRing,
    "ssc_mlp_train_desc": MlpTrainDesc, "ssc_ddpg_many_item": DdpgManyItem,
    "ssc_ddpg_many_wide_item": DdpgManyWideItem, "ssc_ddpg_many_popart_item": DdpgManyPopartItem,
    "ssc_replay_sample_key": ReplaySampleKey,
    "ssc_pair_cursor": PairCursor, "ssc_rollout_many_item": RolloutManyItem, "ssc_replay_append_item": ReplayAppendItem,
    "ssc_decay_item": DecayItem, "ssc_obs_rms_item": ObsRmsItem, "ssc_ddpg_eval_many_item": DdpgEvalManyItem,
    "ssc_ddpg_stats_many_item": DdpgStatsManyItem, "ssc_param_noise_many_item": ParamNoiseManyItem,
    "ssc_param_noise_cursor": ParamNoiseCursor, "ssc_mlp_train_many_item": MlpTrainManyItem,
    "ssc_mpc_sim_many_item": MpcSimManyItem, "ssc_mpc_sim_many_mfma_item": MpcSimManyMfmaItem,
    "ssc_actor_many_item": ActorManyItem, "ssc_smartstart_pair": SmartStartPair, "ssc_select_many_item": SelectManyItem,
}

# symbol -> (restype, argtypes); every function include/ssc.h declares must be listed here
# (tests/test_abi.py cross-checks the header against this table and the built library).
_SIGNATURES = {
    "ssc_version": (c_int, []),
    "ssc_last_error": (c_char_p, []),
    "ssc_env_params_default": (c_int, [c_int, c_float, c_int32, POINTER(EnvParams)]),
    "ssc_mc_step": (c_int, [POINTER(EnvParams), c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p]),
    "ssc_pend_step": (c_int, [POINTER(EnvParams), c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p]),
    "ssc_env_reset": (c_int, [POINTER(EnvParams), c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_uint64, c_uint64, c_uint64, c_void_p]),
    "ssc_env_observe": (c_int, [POINTER(EnvParams), c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ssc_rollout": (c_int, [POINTER(EnvParams), POINTER(PolicyDesc), c_int64, c_int32, POINTER(RolloutState),
                            POINTER(TransitionLog), POINTER(EpisodeRing), c_void_p, c_uint64, c_uint64,
                            c_uint64, c_void_p]),
    "ssc_actor_forward": (c_int, [POINTER(ActorDesc), c_int64, c_void_p, c_void_p, c_void_p]),
    "ssc_pack_bytes": (c_size_t, [c_int32, c_int32, c_int64]),
    "ssc_pack_transitions": (c_int, [POINTER(TransitionLog), c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p,
                                     c_void_p]),
    "ssc_critic_forward": (c_int, [POINTER(CriticDesc), c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ssc_kde_evaluate": (c_int, [c_int32, c_int64, c_void_p, c_int64, c_void_p, POINTER(c_float), c_double, c_void_p,
                                 c_void_p]),
    "ssc_ucb_argmax": (c_int, [c_int64, c_void_p, c_void_p, c_float, c_float, c_double, c_double, c_void_p, c_void_p,
                               c_void_p]),
    "ssc_replay_append": (c_int, [POINTER(ReplayRing), POINTER(TransitionLog), c_int32, c_int64, c_int64, c_float,
                                  c_void_p]),
    "ssc_replay_append_shard": (c_int, [POINTER(ReplayRing), POINTER(TransitionLog), c_int32, c_int64, c_int64, c_int64, c_int64,
                                        c_float, c_void_p]),
    "ssc_decay_schedule": (c_int, [c_void_p, c_double, c_double, c_int32, POINTER(c_double), POINTER(c_double), c_void_p, POINTER(c_void_p),
                                   c_void_p]),
    "ssc_replay_sample": (c_int, [c_uint64, c_uint64, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "ssc_replay_smart_start_workspace_bytes": (c_size_t, [c_int32]),
    "ssc_replay_smart_start_indices": (c_int, [POINTER(ReplayRing), c_int64, c_int64, c_int32, c_uint64, c_uint64,
                                               c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ssc_replay_episode_path": (c_int, [POINTER(ReplayRing), c_int64, c_int64, c_void_p, c_int32, c_void_p, c_void_p,
                                        c_void_p]),
    "ssc_ddpg_train": (c_int, [POINTER(DdpgDesc), POINTER(ReplayView), c_void_p, c_int32, c_void_p, c_void_p]),
    "ssc_ddpg_train_workspace_bytes": (c_size_t, [POINTER(DdpgDesc)]),
    "ssc_ddpg_train_ws": (c_int, [POINTER(DdpgDesc), POINTER(ReplayView), c_void_p, c_int32, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    # normalize_observations: the RunningMeanStd block and the *_rms variants (trailing const double *d_rms)
    "ssc_obs_rms_update_workspace_bytes": (c_size_t, [c_int32]),
    "ssc_obs_rms_update": (c_int, [c_int32, POINTER(TransitionLog), c_int32, c_int32, c_int64, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    "ssc_obs_rms_update_rows": (c_int, [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ssc_actor_forward_rms": (c_int, [POINTER(ActorDesc), c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ssc_critic_forward_rms": (c_int, [POINTER(CriticDesc), c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ssc_rollout_rms": (c_int, [POINTER(EnvParams), POINTER(PolicyDesc), c_int64, c_int32, POINTER(RolloutState),
                                POINTER(TransitionLog), POINTER(EpisodeRing), c_void_p, c_uint64, c_uint64, c_uint64, c_void_p,
                                c_void_p]),
    "ssc_ddpg_train_ws_rms": (c_int, [POINTER(DdpgDesc), POINTER(ReplayView), c_void_p, c_int32, c_void_p, c_void_p, c_size_t,
                                      c_void_p, c_void_p]),
    # normalize_returns + enable_popart: the step with the return statistics (trailing d_rms or NULL, then d_ret_rms)
    "ssc_ddpg_train_popart_workspace_bytes": (c_size_t, [POINTER(DdpgDesc)]),
    "ssc_ddpg_train_ws_popart": (c_int, [POINTER(DdpgDesc), POINTER(ReplayView), c_void_p, c_int32, c_void_p, c_void_p,
                                         c_size_t, c_void_p, c_void_p, c_void_p]),
    # a population of agents in one launch: host items / keys (validated) + the caller's device copy of the same bytes
    "ssc_ddpg_train_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_replay_sample_many": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    # ... of any mix of shapes on the multi-workgroup kernels: host items + the caller's plan (host copy, device copy)
    "ssc_ddpg_train_many_wide_plan_bytes": (c_size_t, [c_int32]),
    "ssc_ddpg_train_many_wide_plan": (c_int, [c_void_p, c_int32, c_void_p, c_size_t]),
    "ssc_ddpg_train_many_wide": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    # ... and of Pop-Art agents (the item carries the agent's ret_rms block; a plan format of its own)
    "ssc_ddpg_train_many_popart_plan_bytes": (c_size_t, [c_int32]),
    "ssc_ddpg_train_many_popart_plan": (c_int, [c_void_p, c_int32, c_void_p, c_size_t]),
    "ssc_ddpg_train_many_popart": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_ddpg_learner_path": (c_int, [POINTER(DdpgDesc), c_int, c_int]),
    # the rest of a population chunk, one launch each: host items / cursors (validated) + the caller's device copies
    "ssc_rollout_many": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "ssc_replay_append_many": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_decay_schedule_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_obs_rms_update_many": (c_int, [c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    # adaptive parameter-space noise: perturb a flat actor, adapt the device stddev
    "ssc_param_noise_perturb": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_uint64,
                                        c_uint64, c_void_p]),
    "ssc_param_noise_adapt": (c_int, [c_int64, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "ssc_param_noise_cycle": (c_int, [POINTER(ActorDesc), c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                      c_int64, c_int64, c_uint64, c_uint64, c_uint64, c_float, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    # ... for a whole population in one launch: host items / cursors (validated) + the caller's device copies
    "ssc_param_noise_cycle_many": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    # training diagnostics (get_stats): one f64 block per call
    "ssc_ddpg_stats_workspace_bytes": (c_size_t, [c_int64]),
    "ssc_ddpg_stats": (c_int, [POINTER(ActorDesc), POINTER(CriticDesc), POINTER(ActorDesc), c_int64, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # evaluation rollouts (eval/return, eval/Q): one fused launch, one f64 block per call
    "ssc_ddpg_eval_workspace_bytes": (c_size_t, [c_int64]),
    "ssc_ddpg_eval_rollout": (c_int, [POINTER(EnvParams), POINTER(ActorDesc), POINTER(CriticDesc), c_float, c_float, c_int64, c_int32,
                                      POINTER(RolloutState), c_void_p, POINTER(TransitionLog), c_void_p, c_int32, c_void_p, c_void_p,
                                      c_size_t, c_uint64, c_uint64, c_uint64, c_void_p]),
    # both for a whole population, one launch per phase: host items / cursors (validated) + the caller's device copies
    "ssc_ddpg_eval_rollout_many": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "ssc_ddpg_stats_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_dataset_scan_workspace_bytes": (c_size_t, [c_int64]),
    "ssc_dataset_scan": (c_int, [POINTER(TransitionLog), c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "ssc_dataset_build": (c_int, [POINTER(TransitionLog), c_int32, c_int32, c_int64, c_void_p, c_void_p, c_int64,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "ssc_column_stats_workspace_bytes": (c_size_t, [c_int32]),
    "ssc_column_stats": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ssc_zscore": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "ssc_path_shortcut": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_double, c_void_p, c_void_p]),
    "ssc_zscore_concat": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p,
                                  c_void_p]),
    "ssc_add_noise": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_double, c_uint64, c_uint64, c_void_p]),
    "ssc_mlp_train_workspace_bytes": (c_size_t, [POINTER(MlpTrainDesc), c_int32]),
    "ssc_mlp_train_steps": (c_int, [POINTER(MlpTrainDesc), c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "ssc_mlp_train_step": (c_int, [POINTER(MlpTrainDesc), c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "ssc_mlp_train_steps_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_mlp_workspace_bytes": (c_size_t, [POINTER(MlpDesc), c_int64, c_int]),
    "ssc_mlp_forward": (c_int, [POINTER(MlpDesc), c_int64, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "ssc_mse_batches": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "ssc_dyn_workspace_bytes": (c_size_t, [POINTER(MlpDesc), c_int64, c_int]),
    "ssc_dyn_prepare": (c_int, [POINTER(MlpDesc), POINTER(Norm), c_void_p, c_size_t, c_void_p]),
    "ssc_dyn_forward_sim": (c_int, [POINTER(MlpDesc), POINTER(Norm), c_int64, c_int32, c_int32, c_int32, c_void_p,
                                    c_int64, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "ssc_mpc_forward_sim": (c_int, [POINTER(MlpDesc), POINTER(Norm), POINTER(MpcSampling), c_int64, c_int32, c_int32, c_int32,
                                    c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "ssc_mpc_forward_sim_many": (c_int, [c_void_p, c_void_p, c_int32, POINTER(MpcSampling), c_int64, c_int32, c_int32, c_int32,
                                         c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "ssc_dyn_mfma_many_class": (c_int, [POINTER(MlpDesc), c_int32, c_int32]),
    "ssc_mpc_forward_sim_many_mfma": (c_int, [c_void_p, c_void_p, c_int32, POINTER(MpcSampling), c_int64, c_int32, c_int32,
                                              c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "ssc_mpc_score_select": (c_int, [POINTER(MpcProblems), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     POINTER(MpcSampling), c_int32, c_float, c_uint64, c_uint64, c_uint64, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "ssc_mpc_sample_actions": (c_int, [c_int32, c_int32, c_int32, c_int32, POINTER(c_float), POINTER(c_float),
                                       c_uint64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p]),
    "ssc_mpc_rollout_step": (c_int, [POINTER(EnvParams), POINTER(MpcProblems), POINTER(MpcNavState), c_void_p, c_void_p,
                                     c_float, c_uint64, c_uint64, POINTER(RolloutState), POINTER(TransitionLog),
                                     POINTER(EpisodeRing), c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "ssc_smartstart_rollout_step": (c_int, [POINTER(EnvParams), POINTER(MpcProblems), POINTER(MpcNavState), POINTER(SmartStartStep),
                                            c_void_p, c_void_p, c_float, c_uint64, c_uint64, POINTER(RolloutState),
                                            POINTER(TransitionLog), POINTER(EpisodeRing), c_void_p, c_uint64, c_uint64, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    # a population of SmartStart pairs: all actors of one class, and the step of all pairs, in one launch each
    "ssc_actor_many_class": (c_int, [POINTER(ActorDesc), c_int]),
    "ssc_actor_forward_many": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_void_p]),
    "ssc_smartstart_rollout_step_many": (c_int, [POINTER(EnvParams), POINTER(MpcProblems), POINTER(MpcNavState),
                                                 POINTER(SmartStartStep), c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_float,
                                                 c_uint64, c_uint64, POINTER(RolloutState), POINTER(TransitionLog),
                                                 POINTER(EpisodeRing), c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_void_p]),
    # the smart-start selection of a population, one launch per stage over ONE item table (host items + device copy)
    "ssc_replay_smart_start_indices_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_kde_scott_bandwidth_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_critic_forward_many": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "ssc_kde_evaluate_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_ucb_topk_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_replay_episode_path_many": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "ssc_nav_compact": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ssc_mpc_score_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "ssc_mpc_score": (c_int, [POINTER(MpcProblems), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                              c_void_p]),
    "ssc_mpc_observe": (c_int, [POINTER(MpcProblems), c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "ssc_mpc_select_action": (c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                      c_float, c_uint64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p]),
}

_lib = None


def lib():
    """Load libssc.so once; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP library is the product and there is no CPU fallback. "
                "Build it with `python -m smartstartcontinuous_amd.build` (needs hipcc).")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != SSC_OK:
        raise SscError(rc, lib().ssc_last_error().decode("utf-8", "replace"))


def default_params(kind, power_scalar=1.0, max_episode_steps=0):
    p = EnvParams()
    check(lib().ssc_env_params_default(kind, power_scalar, max_episode_steps, ctypes.byref(p)))
    return p


def ptr(t):
    """data_ptr() of a tensor (or None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def stream(device=None):
    """The ``hipStream_t`` argument of a launch: torch's current stream on ``device`` (default: the current device)."""
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def set_net_ptrs(desc, w):
    """Point an ActorDesc / CriticDesc at the tensors of the weight dict ``w``: W1 .. b3 and, for a LayerNorm network
    (models_editted.py:45-46, 50-51, 85-86, 91-92), ln1_g .. ln2_b."""
    for k in ("W1", "b1", "W2", "b2", "W3", "b3") + (("ln1_g", "ln1_b", "ln2_g", "ln2_b") if "ln1_g" in w else ()):
        setattr(desc, k, w[k].data_ptr())
