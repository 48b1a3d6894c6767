/* ssc.h -- C ABI of libssc.so, the MI355X (gfx950) rollout engine behind the
 * gym.Env / RLAgent surface of darren-huang/SmartStartContinuous.
 *
 * The reference is pure Python (no FFI of its own); each entry point below names the
 * reference interface it replaces (file:line relative to the reference root).  The
 * Python host layer (smartstartcontinuous_amd/_ffi.py) binds exactly these symbols with
 * ctypes; INTEGRATION.md shows the stubs a reference maintainer would add.
 *
 * Conventions
 *   - Every pointer named d_* / inside the descriptor structs marked "device" is a DEVICE
 *     pointer owned by the caller (a PyTorch-ROCm tensor's data_ptr()).  The library
 *     allocates nothing on the device and keeps no state between calls; all RNG is
 *     counter-based (Philox4x32-10 keyed by seed / global env id / global step).
 *   - All work is enqueued on the given hipStream_t (passed as void*); no call
 *     synchronises, none uses the default stream implicitly.
 *   - Return 0 (SSC_OK) or a negative SSC_E* code; ssc_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI, nothing exits.
 *   - Arrays are structure-of-arrays, fp32 unless stated; "[K][n]" means K rows of n
 *     contiguous elements.
 */
#ifndef SSC_H
#define SSC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSC_VERSION 108 /* 0.1.8: ssc_ddpg_desc.critic_l2_reg / clip_norm, ssc_mse_batches; 0.1.7: LayerNorm (ssc_actor_desc / ssc_critic_desc ln*, ssc_ddpg_desc.layer_norm); 0.1.6: ssc_nav_compact + live lists in ssc_mpc_sampling / ssc_mpc_problems; 0.1.5: ssc_ou_desc.d_epsilon, ssc_decay_schedule, ssc_replay_append_shard; 0.1.4: ssc_path_shortcut; 0.1.3: ssc_zscore_concat (0.1.2: plan pool + active mask in ssc_mpc_problems / ssc_mpc_sampling, ssc_smartstart_rollout_step) */

typedef void *ssc_stream_t; /* hipStream_t */

enum {
    SSC_OK = 0,
    SSC_EINVAL = -1,       /* bad argument (null pointer, negative size, ...) */
    SSC_EUNSUPPORTED = -2, /* shape / option outside what the kernels implement */
    SSC_EHIP = -3          /* a HIP runtime call failed; see ssc_last_error() */
};

enum { SSC_ENV_MOUNTAINCAR = 0, SSC_ENV_PENDULUM = 1 };
enum { SSC_POLICY_RANDOM = 0, SSC_POLICY_ACTOR = 1 };
enum { SSC_PREC_F32 = 0, SSC_PREC_BF16_MFMA = 1, SSC_PREC_BF16_MFMA_PREPARED = 2 };

#define SSC_MAX_OBS 3
#define SSC_MAX_LAYERS 4
#define SSC_MAX_STATE 8
#define SSC_MAX_ACT 4

/* Environment constants.
 * MountainCar: Continuous_MountainCarEnv_Editted.__init__
 *   (smartstart/environments/continuous_mountain_car_editted.py:35-54) + the gym TimeLimit
 *   of make_timed_env (:154-159).
 * Pendulum: gym 0.10.5 PendulumEnv.__init__ [third-party, pinned in Pipfile.lock]. */
typedef struct ssc_env_params {
    int32_t kind;              /* SSC_ENV_* */
    int32_t max_episode_steps; /* TimeLimit; <= 0 means no limit */
    /* MountainCar */
    float min_action, max_action;
    float min_position, max_position;
    float max_speed, goal_position, power;
    float reset_low, reset_high; /* reset(): pos ~ U(reset_low, reset_high), vel = 0 (:84-86) */
    /* Pendulum */
    float max_torque, pend_max_speed, dt, g, m, l;
    int32_t pend_v1_order; /* 0: gym 0.10.5 "v0" update order, 1: modern "v1" order */
} ssc_env_params;

/* DDPG actor (Actor_Editted.__call__, DDPG_Baselines_editted/models_editted.py:38-61).
 * Weights are fp32 device arrays in TensorFlow layout W[in][out]. */
typedef struct ssc_actor_desc {
    int32_t obs_dim, h1, h2, act_dim;
    const float *W1, *b1, *W2, *b2, *W3, *b3; /* device */
    int32_t last_layer_tanh;                  /* models_editted.py:53-56 */
    int32_t precision;                        /* SSC_PREC_*: hidden GEMM in fp32 VALU or bf16 MFMA */
    float obs_clip;                           /* > 0: the observation is clipped to [-obs_clip, obs_clip] before layer 1 --
                                                 DDPG_editted feeds its networks tf.clip_by_value(obs, observation_range)
                                                 (ddpg_editted.py:106-109, observation_range = (-5, 5) in every run);
                                                 0: no clip (bare Actor_Editted.__call__) */
    /* layer_norm=True (models_editted.py:45-46, 50-51; the class default, unused by the shipped runs):
     * tc.layers.layer_norm(center=True, scale=True) [third-party TF 1.5: over the units of a row, variance epsilon 1e-12]
     * behind each hidden dense layer, in front of its activation.  gamma / beta of layer 1 [h1] and layer 2 [h2], device;
     * all four NULL: no LayerNorm.  LayerNorm networks run on the fp32 kernels (`precision` must be SSC_PREC_F32). */
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
} ssc_actor_desc;

/* Exploration noise of DDPG_editted.pi (ddpg_editted.py:266-271):
 * DecayingOrnsteinUhlenbeckActionNoise (smartstart/RLAgents/DDPG_Baselines_agent.py:52-78). */
typedef struct ssc_ou_desc {
    float mu, sigma, theta, dt;
    float epsilon; /* current epsilon (decayed per episode by the host, :77-78); 0 disables noise */
    const float *d_epsilon; /* not NULL: the current epsilon is this DEVICE float, read when the kernel starts (`epsilon` is
                               ignored and the noise path always runs) -- so that a loop whose decay is computed on the
                               device (ssc_decay_schedule) never needs the host between two rollouts */
} ssc_ou_desc;

typedef struct ssc_policy_desc {
    int32_t kind;             /* SSC_POLICY_* */
    float act_low, act_high;  /* action_space bounds (Policy_Random, policy_random.py:9-15;
                                 DDPG_Baselines_agent.scale, DDPG_Baselines_agent.py:236-240) */
    ssc_actor_desc actor;     /* SSC_POLICY_ACTOR */
    ssc_ou_desc ou;           /* SSC_POLICY_ACTOR */
} ssc_policy_desc;

/* Per-env persistent state, each [n] (device).  s0/s1 = (position, velocity) for
 * MountainCar, (theta, theta_dot) for Pendulum. */
typedef struct ssc_rollout_state {
    float *s0, *s1;
    int32_t *steps; /* TimeLimit's elapsed-step counter of the running episode */
    float *ep_ret;  /* running episode return (Episode.total_reward, datacontainers.py:41-49) */
    float *ou_x;    /* OU-noise state x_prev; may be NULL for SSC_POLICY_RANDOM */
} ssc_rollout_state;

/* Transition log of one rollout chunk: the record ReplayBuffer.add stores
 * (smartstart/RLAgents/replay_buffer.py:49-74, tuple (s, a, r, t, s2) :53), as SoA
 * columns of [K][n].  obs/obs2 hold obs_dim columns (2 for MountainCar, 3 for Pendulum);
 * unused entries may be NULL. */
typedef struct ssc_transition_log {
    float *obs[SSC_MAX_OBS];
    float *act;
    float *rew;
    uint8_t *done;
    float *obs2[SSC_MAX_OBS];
    int64_t row_stride;      /* elements between step k and k+1 of one fp32 column; 0 means n (dense [K][n]).
                                A packed chunk puts all fp32 columns of a step side by side:
                                row_stride = (2*obs_dim+2)*n, column c starts at base + c*n. */
    int64_t done_row_stride; /* same for the u8 done column; 0 means n */
} ssc_transition_log;

/* Completed-episode records: what Summary.append keeps per episode
 * (smartstart/utilities/datacontainers.py:173-193: (len(episode), total_reward)). */
typedef struct ssc_episode_ring {
    int64_t *env_id;  /* [capacity] global env id */
    int32_t *length;  /* [capacity] */
    float *ret;       /* [capacity] */
    uint32_t *cursor; /* [1] device counter; records beyond capacity are dropped but counted */
    int32_t capacity;
} ssc_episode_ring;

int ssc_version(void);
const char *ssc_last_error(void);

/* Fill *p with the reference defaults.  kind = SSC_ENV_MOUNTAINCAR: power = 0.0015 *
 * power_scalar (continuous_mountain_car_editted.py:43). */
int ssc_env_params_default(int kind, float power_scalar, int32_t max_episode_steps, ssc_env_params *p);

/* One env.step for n envs -- Continuous_MountainCarEnv_Editted.step
 * (continuous_mountain_car_editted.py:60-82) wrapped by gym TimeLimit.step when d_steps is
 * given (d_steps[i] += 1; done |= d_steps[i] >= max_episode_steps).  pos/vel are updated
 * in place.  d_steps may be NULL (bare env, no time limit). */
int ssc_mc_step(const ssc_env_params *p, int64_t n, float *d_pos, float *d_vel, const float *d_act,
                float *d_rew, uint8_t *d_done, int32_t *d_steps, ssc_stream_t stream);

/* gym 0.10.5 PendulumEnv.step for n envs [third-party]; d_obs is [3][n] =
 * (cos th, sin th, thdot) of the NEW state, may be NULL. */
int ssc_pend_step(const ssc_env_params *p, int64_t n, float *d_th, float *d_thdot, const float *d_act,
                  float *d_obs, float *d_rew, uint8_t *d_done, int32_t *d_steps, ssc_stream_t stream);

/* env.reset for the envs selected by d_mask (NULL = all) --
 * continuous_mountain_car_editted.py:84-86 / gym PendulumEnv.reset.  Draws come from
 * Philox(seed; env_id0 + i, t, TAG_RESET); also zeroes d_steps / d_ep_ret / d_ou_x entries
 * (each may be NULL). */
int ssc_env_reset(const ssc_env_params *p, int64_t n, const uint8_t *d_mask, float *d_s0, float *d_s1,
                  int32_t *d_steps, float *d_ep_ret, float *d_ou_x, uint64_t seed, uint64_t env_id0,
                  uint64_t t, ssc_stream_t stream);

/* Observation of the current state: MountainCar [2][n] = (pos, vel); Pendulum [3][n]. */
int ssc_env_observe(const ssc_env_params *p, int64_t n, const float *d_s0, const float *d_s1,
                    float *d_obs, ssc_stream_t stream);

/* K fused steps of the rlTrain inner loop (smartstart/reinforcementLearningCore/rlTrain.py:75-100)
 * for n independent envs: get_action -> env.step -> record -> auto-reset on done.
 * One thread owns one env; state stays in registers for the K steps.
 *   policy RANDOM = Policy_Random.get_action (NN_Dynamics_Model/policy_random.py:14-15), i.e. the
 *     reference's collect_samples_threaded.py:52-111 rollout;
 *   policy ACTOR  = DDPG_Baselines_agent.get_action (DDPG_Baselines_agent.py:206-234).
 * log, ring, d_stats may each be NULL.  d_stats is double[4] on the device and is
 * ACCUMULATED into: {sum of rewards, goal terminations, env-steps, finished episodes}.
 * Global step index of the first step is step0; env i has global id env_id0 + i, so any
 * sharding of the id space reproduces the same per-env streams. */
int ssc_rollout(const ssc_env_params *p, const ssc_policy_desc *policy, int64_t n, int32_t K,
                const ssc_rollout_state *state, const ssc_transition_log *log,
                const ssc_episode_ring *ring, double *d_stats, uint64_t seed, uint64_t env_id0,
                uint64_t step0, ssc_stream_t stream);

/* The per-episode decay of the exploration schedules, computed where the episode counter lives: the reference decays
 * epsilon (DecayingOrnsteinUhlenbeckActionNoise.reduce_epsilon, DDPG_Baselines_agent.py:77-78, called from end_episode
 * :255-258) and eta (SmartStartContinuous.reduce_eta, smartexplorationcontinuous.py:372-376) once per finished episode; a
 * loop over n parallel envs decays once per GENERATION = `per_generation` finished episodes.  One thread:
 *   g = floor((*d_finished - finished0) / per_generation);  for every schedule i < n_sched, (g - applied) times:
 *   value_i = max(value_i * factor[i], floor[i])   in fp64, exactly the host's Python arithmetic;
 * d_state = double[1 + n_sched]: {generations applied, value_0, ...} (caller-initialised: 0, start values);
 * d_out[i] (device float, may be NULL) receives (float)value_i -- e.g. the ssc_ou_desc.d_epsilon of the next rollout.
 * d_finished: a device double, e.g. d_stats + 3 of ssc_rollout (finished episodes), finished0 its value when the loop
 * started.  n_sched <= 4; factor / floor are HOST arrays. */
int ssc_decay_schedule(const double *d_finished, double finished0, double per_generation, int32_t n_sched, const double *factor,
                       const double *floor, double *d_state, float *const *d_out, ssc_stream_t stream);

/* Packs the LAST g steps of a transition log into one contiguous buffer for the per-chunk exchange
 * (the rollout gather of NN_Dynamics_Model/collect_samples_threaded.py:31-50 as ONE RCCL message):
 *   d_out = [obs (obs_dim x g x n) f32 | act (g x n) | rew (g x n) | obs2 (obs_dim x g x n) | done (g x n) u8]
 * followed, 8-byte aligned, by a snapshot of d_stats (4 doubles) when d_stats != NULL.
 * d_out must hold ssc_pack_bytes(obs_dim, g, n) bytes. */
size_t ssc_pack_bytes(int32_t obs_dim, int32_t g, int64_t n);
int ssc_pack_transitions(const ssc_transition_log *log, int32_t obs_dim, int32_t K, int32_t g, int64_t n,
                         const double *d_stats, void *d_out, ssc_stream_t stream);

/* Batched actor forward, act[m][act_dim] = Actor_Editted(obs[m][obs_dim])
 * (models_editted.py:38-61); row-major in/out.  No noise, no clipping. */
int ssc_actor_forward(const ssc_actor_desc *actor, int64_t m, const float *d_obs, float *d_act,
                      ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * SmartStart navigator: NND_MB dynamics model + MPC (smartstart/RLAgents/NND_MB_agent.py)
 * ------------------------------------------------------------------------------------- */

/* feedforward_network (NN_Dynamics_Model/feedforward_network.py:3-23):
 * h = relu(h @ W_i + b_i) for the num_fc_layers hidden layers, z = h @ W_out + b_out.
 * n_layers = num_fc_layers + 1 weight matrices; dims = {in, depth, ..., out};
 * W[l] is fp32 [dims[l]][dims[l+1]] (TensorFlow layout), device. */
typedef struct ssc_mlp_desc {
    int32_t n_layers;
    int32_t dims[SSC_MAX_LAYERS + 1];
    const float *W[SSC_MAX_LAYERS];
    const float *b[SSC_MAX_LAYERS];
} ssc_mlp_desc;

/* z-score statistics of NND_MB_agent.__init__ (NND_MB_agent.py:302-315), by value. */
typedef struct ssc_norm {
    float mean_x[SSC_MAX_STATE], std_x[SSC_MAX_STATE];
    float mean_y[SSC_MAX_ACT], std_y[SSC_MAX_ACT];
    float mean_z[SSC_MAX_STATE], std_z[SSC_MAX_STATE];
} ssc_norm;

/* y[m][out] = feedforward_network(x[m][in]).  precision SSC_PREC_F32: every layer in fp32
 * (VALU); SSC_PREC_BF16_MFMA: hidden-layer contractions on bf16 MFMA with fp32 accumulation
 * (num_fc_layers 1 or 2, depth <= 512).  d_workspace: ssc_mlp_workspace_bytes() bytes. */
size_t ssc_mlp_workspace_bytes(const ssc_mlp_desc *mlp, int64_t m, int precision);
int ssc_mlp_forward(const ssc_mlp_desc *mlp, int64_t m, const float *d_x, float *d_y, int precision,
                    void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);

/* Dyn_Model.do_forward_sim, batched branch (NN_Dynamics_Model/dynamics_model.py:204-240):
 *   S[0] = s0;  for t < H:  x = nan_to_num((S[t]-mean_x)/std_x) || nan_to_num((A[:,t]-mean_y)/std_y)
 *                           S[t+1] = S[t] + net(x) * std_z + mean_z
 * d_s0 is [s0_rows][state_dim]: s0_rows == 1 (one start state tiled to all rows, :215-217), s0_rows == m,
 * or any divisor P of m (P problems with m/P candidate sequences each: row r starts from state r / (m/P)).
 * d_A is [m][H][act_dim]; d_S is [H+1][m][state_dim]. */
size_t ssc_dyn_workspace_bytes(const ssc_mlp_desc *mlp, int64_t m, int precision);
/* Dyn_Model.run_validation's loss (dynamics_model.py:173-196 with mse_ of :42): d_batch_loss[b] = mean over the
 * `batch_elems` (= batchsize * out_dim) consecutive elements of batch b of (d_z - d_pred)^2, d_mean[0] = their mean in
 * batch order.  d_pred: the network's outputs for the first n_batches * batchsize rows (ssc_mlp_forward). */
int ssc_mse_batches(const float *d_pred, const float *d_z, int64_t n_batches, int64_t batch_elems, float *d_batch_loss,
                    float *d_mean, ssc_stream_t stream);

/* The MFMA path works from a packed bf16 image of the weights (and of the statistics) in the workspace.
 * ssc_dyn_forward_sim / ssc_mlp_forward with SSC_PREC_BF16_MFMA write that image on every call; a caller
 * whose weights stay put between calls -- the navigator between two Dyn_Model.train() rounds
 * (NND_MB_agent.py:421-423), like TF variables that live in the session across sess.run calls
 * (dynamics_model.py:226-233) -- writes it ONCE with ssc_dyn_prepare() and then passes
 * SSC_PREC_BF16_MFMA_PREPARED with the same workspace (which nothing else may touch in between).
 * norm may be NULL for ssc_mlp_forward use.  Workspace size: ssc_dyn_workspace_bytes(.., SSC_PREC_BF16_MFMA). */
int ssc_dyn_prepare(const ssc_mlp_desc *mlp, const ssc_norm *norm, void *d_workspace, size_t workspace_bytes,
                    ssc_stream_t stream);
int ssc_dyn_forward_sim(const ssc_mlp_desc *mlp, const ssc_norm *norm, int64_t m, int32_t H,
                        int32_t state_dim, int32_t act_dim, const float *d_s0, int64_t s0_rows,
                        const float *d_A, float *d_S, int precision, void *d_workspace,
                        size_t workspace_bytes, ssc_stream_t stream);

/* A set of P independent MPC problems (one per real env) with N candidate action sequences
 * each; rows of every [P*N] array are problem-major.  Waypoints / distances_left come from
 * NND_MB_agent.start_new_episode_plan (NND_MB_agent.py:375-423), packed back to back:
 * problem p owns rows wp_off[p] .. wp_off[p+1]-1 (at least 2 waypoints each). */
typedef struct ssc_mpc_problems {
    int32_t n_problems, n_samples, horizon, state_dim;
    const float *wp;        /* device [wp_off[P]][state_dim]  desired_states */
    const float *left;      /* device [wp_off[P]]             distances_left (:411-418) */
    const int32_t *wp_off;  /* device [P+1] */
    const int32_t *cur_idx; /* device [P]  current_desired_state_index */
    const float *radii;     /* device [P][state_dim] (numerical.py:61-62) */
    float theta, gamma, horizontal_penalty_factor; /* :143, :62 */
    int32_t per_row_projection; /* 0 = reference behaviour (batch-global np.sum, numerical.py:89-92);
                                   1 = corrected per-sample projection (NOT the reference) */
    /* Optional plan POOL (the vectorised SmartStart loop: many envs follow one of a few stored plans).  Both NULL:
     * problem p owns plan p, as described above.  Otherwise problem p follows plan q = plan_of[p]: its waypoints are
     * rows wp_off[q] .. wp_off[q] + wp_len[q] - 1 of wp / left and its radii row q of radii; cur_idx stays per problem. */
    const int32_t *plan_of; /* device [P] or NULL */
    const int32_t *wp_len;  /* device [number of plans] or NULL (required with plan_of) */
    /* Optional: device [P] bytes; a problem whose byte is 0 is not scored by the one-launch scorer (n_samples <= 64): its
     * scores / best_idx entries are left untouched.  NULL: every problem is scored. */
    const uint8_t *active;
    /* Optional compact work list (ssc_nav_compact), as in ssc_mpc_sampling: the one-launch scorer serves the *n_live problems
     * live_list[0 .. *n_live) and nothing else; outputs stay indexed by problem. */
    const int32_t *live_list;
    const int32_t *n_live;
} ssc_mpc_problems;

/* all_samples = npr.uniform(low, high, (N, H, act)) (NND_MB_agent.py:500-501) for P problems:
 * d_A [P*N][H][act_dim], Philox(seed; (problem_id0+p) << 32 | n, t, TAG_MPC).  d_t_base (may be NULL) is a
 * device-resident step counter added to t, so that a captured HIP graph can be replayed step after step. */
int ssc_mpc_sample_actions(int32_t n_problems, int32_t n_samples, int32_t horizon, int32_t act_dim,
                           const float *low, const float *high, uint64_t seed, uint64_t problem_id0,
                           uint64_t t, const uint64_t *d_t_base, float *d_A, ssc_stream_t stream);

/* The candidate action sequences of an MPC step as a SPECIFICATION instead of a matrix: all_samples =
 * npr.uniform(low, high, (N, H, act)) (NND_MB_agent.py:500-501) is a pure function of (seed, problem, sample, t) --
 * the Philox stream of ssc_mpc_sample_actions -- so the consumers can draw the numbers where they use them and the
 * [P*N][H][act] matrix need not exist. */
typedef struct ssc_mpc_sampling {
    int32_t n_samples;                       /* N: row r of an [P*N] array is sample r % N of problem r / N */
    float low[SSC_MAX_ACT], high[SSC_MAX_ACT];
    uint64_t seed, problem_id0, t;
    const uint64_t *d_t_base;                /* device step counter added to t (HIP-graph replay); may be NULL */
    /* Optional: device [number of problems] bytes; the rows of a problem whose byte is 0 need not be simulated (their part of
     * d_S / d_A_out is then left untouched).  The kernels with LDS-resident weights (depth <= 128, or one hidden layer) skip
     * a wave whose rows all belong to such problems; the streamed-W2 kernel ignores the mask.  NULL: every problem is live. */
    const uint8_t *d_problem_active;
    /* Optional COMPACT work list (ssc_nav_compact): device int32 list of the live problems and device count.  With both given
     * the fused small-network kernel assigns thread block i * 256 + j to row (list[slot] * N + sample) of the slot-th LIVE
     * problem -- the launch still covers P * N threads (HIP-graph safe), blocks past *d_n_live exit at once -- and every
     * array keeps its problem-major layout.  Other kernels ignore the list (they simulate every row). */
    const int32_t *d_live_list;
    const int32_t *d_n_live;
} ssc_mpc_sampling;

/* ssc_mpc_sample_actions + ssc_dyn_forward_sim in ONE launch (Dyn_Model.do_forward_sim fed by get_best_sim_actions,
 * NND_MB_agent.py:498-512): the forward-simulation kernel draws every row's action sequence itself (bit-identical to
 * ssc_mpc_sample_actions with the same specification), so the sample launch and the [m][H][act] read disappear.
 * d_A_out [m][H][act] (may be NULL) receives the sequences for callers that index them later (ssc_mpc_rollout_step);
 * ssc_mpc_score_select regenerates the winner's first action from the specification and does not need it.
 * precision SSC_PREC_F32 runs the two-launch equivalent and needs d_A_out. */
int ssc_mpc_forward_sim(const ssc_mlp_desc *mlp, const ssc_norm *norm, const ssc_mpc_sampling *sampling, int64_t m,
                        int32_t H, int32_t state_dim, int32_t act_dim, const float *d_s0, int64_t s0_rows,
                        float *d_A_out, float *d_S, int precision, void *d_workspace, size_t workspace_bytes,
                        ssc_stream_t stream);

/* One dynamics model of a population and the problems it simulates.  Declared tag first like the other *_many items;
 * tests/test_mpc_sim_many_host.py holds the struct's size and offsets to the ctypes mirror. */
struct ssc_mpc_sim_many_item {
    ssc_mlp_desc mlp;        /* one hidden layer, depth <= 128: the fused fp32 family (state <= 3, state + act <= 4) */
    ssc_norm     norm;       /* this model's statistics, by value */
    int32_t      problem0;   /* the item's problems: [problem0, problem0 + n_problems) of the call's */
    int32_t      n_problems; /* problem-major arrays; 0: the item is skipped and nothing else of it is read */
};
typedef struct ssc_mpc_sim_many_item ssc_mpc_sim_many_item;

/* ssc_mpc_forward_sim(.., SSC_PREC_F32, ..) for a population of models in ONE launch (the navigators of a sweep's seeds,
 * DESIGN.md section 4.5b): contiguous ranges of the call's m / n_samples problems use different networks and different
 * z-score statistics.  Grid row y runs item y's workgroups (grid x = the largest item's count; surplus workgroups leave at
 * once, before any barrier) through the very kernel bodies of the single call.  Afterwards d_S [H+1][m][state_dim] and
 * d_A_out [m][H][act_dim] (may be NULL) hold, bit for bit, what one ssc_mpc_forward_sim call per item with n_problems > 0
 * leaves in the same buffers when its d_problem_active is AND-ed with "problem in the item's range": rows of problems no
 * item owns, and rows the caller's mask switches off, are left untouched; d_t_base is honoured; the Philox stream is that
 * of (seed, problem_id0 + problem, sample, t) with the call's GLOBAL problem index, so nothing depends on the item split.
 * Conventions of the other *_many calls: the host array is validated completely before any HIP call, the caller's device
 * copy of the same bytes must be complete on `stream`, the library copies nothing, item indices appear in
 * ssc_last_error().  n_items 1..65535.  The single call's checks apply to the call and to every item with n_problems > 0
 * (its codes); an item outside the fused fp32 family is SSC_EUNSUPPORTED naming it; a range outside
 * [0, m / n_samples) or two overlapping ranges are SSC_EINVAL (gaps are legal); sampling->d_live_list / d_n_live must be
 * NULL (SSC_EINVAL: a compact list maps slots to arbitrary problems, a workgroup's weights would not be uniform).
 * Weights may be shared between items.  m == 0, or every item empty: SSC_OK without a launch. */
int ssc_mpc_forward_sim_many(const ssc_mpc_sim_many_item *h_items, const ssc_mpc_sim_many_item *d_items, int32_t n_items,
                             const ssc_mpc_sampling *sampling, int64_t m, int32_t H, int32_t state_dim, int32_t act_dim,
                             const float *d_s0, int64_t s0_rows, float *d_A_out, float *d_S, ssc_stream_t stream);

/* One bf16-MFMA dynamics model of a population and the problems it simulates.  The kernel reads the packed image only (the
 * statistics are inside it, ssc_dyn_prepare); `mlp` serves the host's shape checks and names the class.
 * tests/test_mpc_sim_many_mfma_host.py holds the struct's size and offsets to the ctypes mirror. */
struct ssc_mpc_sim_many_mfma_item {
    ssc_mlp_desc mlp;         /* host side: shape checks and the class; the kernel reads the image only */
    const void  *d_image;     /* written by ssc_dyn_prepare(&mlp, &norm, ...); 16-byte aligned */
    size_t       image_bytes; /* >= ssc_dyn_workspace_bytes(&mlp, m, SSC_PREC_BF16_MFMA) */
    int32_t      problem0;    /* the item's problems: [problem0, problem0 + n_problems) of the call's */
    int32_t      n_problems;  /* 0: the item is skipped and nothing else of it is read */
};
typedef struct ssc_mpc_sim_many_mfma_item ssc_mpc_sim_many_mfma_item;

/* The instantiation class of the MFMA simulation kernel that one many-call can serve this network with (>= 0), or -1:
 * not covered by the MFMA path, streamed W2 (two hidden layers deeper than 128), more than 4 inputs or outputs, or a
 * network that is not state_dim + act_dim -> state_dim.  Classes: 0, 1, 2 = one hidden layer of <= 32, <= 128, <= 512 units;
 * 3 / 4 = two equal hidden layers of <= 32 units with b2 as the accumulator's input / in two spare k slots (depth <= 30);
 * 5 / 6 = the same for <= 128 units (k slots: depth <= 126).  A pure function of the shape. */
int ssc_dyn_mfma_many_class(const ssc_mlp_desc *mlp, int32_t state_dim, int32_t act_dim);

/* ssc_mpc_forward_sim(.., SSC_PREC_BF16_MFMA_PREPARED, ..) -- Dyn_Model.do_forward_sim (dynamics_model.py:204-240) fed by
 * candidates drawn in the kernel -- for a population of models in ONE launch.  Grid row y runs
 * item y; its row tiles of 256 rows are anchored at the item's first row, so the partition into tiles and waves is that of
 * the model's own call on its own rows.  Afterwards the item's rows of d_S [H+1][m][state_dim] and d_A_out [m][H][act_dim]
 * (may be NULL) hold, bit for bit, what the model's own call leaves in a [H+1][rows][state_dim] buffer of its rows alone
 * when it is given problem_id0 + problem0 and the mask from byte problem0 on; a row's start state is the one its row OF THE
 * CALL selects (d_s0[row / (m / s0_rows)]).  Rows of problems no item owns, and waves the mask lets the kernel skip, are left
 * untouched; d_t_base is honoured.  Conventions and checks of ssc_mpc_forward_sim_many; in addition every item with
 * n_problems > 0 must have a class, ALL OF THEM THE SAME ONE (SSC_EUNSUPPORTED naming two items and their classes), a
 * non-NULL 16-byte-aligned image of sufficient size, and at most 2^31 - 1 rows.  The call allocates nothing and makes one
 * launch.  m == 0, or every item empty: SSC_OK without a launch. */
int ssc_mpc_forward_sim_many_mfma(const ssc_mpc_sim_many_mfma_item *h_items, const ssc_mpc_sim_many_mfma_item *d_items,
                                  int32_t n_items, const ssc_mpc_sampling *sampling, int64_t m, int32_t H, int32_t state_dim,
                                  int32_t act_dim, const float *d_s0, int64_t s0_rows, float *d_A_out /* may be NULL */,
                                  float *d_S, ssc_stream_t stream);

/* generate_scores_add_delta (NND_MB_agent.py:566-628) + argmax (:625-626) per problem.
 * d_S [H+1][P*N][state_dim] (output of ssc_dyn_forward_sim); d_scores [P*N]; d_best_idx [P]
 * (index within the problem, lowest index on ties like np.argmax); d_best_score [P]. */
size_t ssc_mpc_score_workspace_bytes(int32_t n_problems, int32_t n_samples, int32_t horizon);
int ssc_mpc_score(const ssc_mpc_problems *prob, const float *d_S, float *d_scores, int32_t *d_best_idx,
                  float *d_best_score, void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);

/* ssc_mpc_score + ssc_mpc_select_action in the same two launches: the block that finishes a problem's argmax also
 * writes action[p] = best_sequence[0] + noise_amount * N(0,1) (no clip, NND_MB_agent.py:353-356; the draws of
 * ssc_mpc_select_action) and the predicted path S[:, best] -> d_best_path [P][H+1][state_dim] (may be NULL).  The
 * first action of the winner comes from d_A [P*N][H][act] when given, otherwise it is regenerated from `sampling`
 * (exactly one of the two must be non-NULL).  noise_seed / problem_id0 / t (+ *d_t_base of `sampling` when given)
 * key the noise like ssc_mpc_select_action. */
int ssc_mpc_score_select(const ssc_mpc_problems *prob, const float *d_S, float *d_scores, int32_t *d_best_idx,
                         float *d_best_score, const float *d_A, const ssc_mpc_sampling *sampling, int32_t act_dim,
                         float noise_amount, uint64_t noise_seed, uint64_t problem_id0, uint64_t t, float *d_action,
                         float *d_best_path, void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);

/* NND_MB_agent.observe (NND_MB_agent.py:360-373) + close_enough_to_goal (:425-432) for P navigators at
 * once: given the state each env reached, advance its waypoint index when the waypoint was reached /
 * overtaken (move_to_next, :491-496) or given up on (d_actions_done > give_up_after), and flag envs that
 * are within theta of their final waypoint (or timed out on it after final_steps actions).
 * d_cur_idx [P] and d_actions_done [P] are updated in place; d_at_goal [P] (u8) may be NULL.
 * d_new_state is [P][state_dim].  (get_action's `actions_done += 1`, :340, is the caller's.) */
int ssc_mpc_observe(const ssc_mpc_problems *prob, const float *d_new_state, int32_t *d_cur_idx,
                    int32_t *d_actions_done, int32_t give_up_after, int32_t final_steps, uint8_t *d_at_goal,
                    ssc_stream_t stream);

/* get_action_with_predicted_states (NND_MB_agent.py:339-358): action[p] = A[best][0] +
 * noise_amount * N(0,1) (no clip, :353-356); also copies the predicted path
 * S[:, best] -> d_best_path [P][H+1][state_dim] (may be NULL). */
int ssc_mpc_select_action(int32_t n_problems, int32_t n_samples, int32_t horizon, int32_t state_dim,
                          int32_t act_dim, const float *d_A, const float *d_S, const int32_t *d_best_idx,
                          float noise_amount, uint64_t seed, uint64_t problem_id0, uint64_t t,
                          float *d_action, float *d_best_path, ssc_stream_t stream);

/* One MPC-policy step of rollout(K, policy = 'mpc') for P envs (one navigation problem each), everything
 * after the scoring in ONE launch: executed action = best_sequence[0] + noise_amount * N(0,1) (NND_MB_agent.py:
 * 353-356, same draws as ssc_mpc_select_action), env.step (+ TimeLimit), transition-log row, chunk statistics,
 * episode record, NND_MB_agent.observe on the new observation (waypoint advance, :360-373), auto-reset of finished
 * envs (state, episode counters, navigator plan position back to d_start_idx) and the planning state of the
 * next step, d_plan_state [P][obs_dim] (the observation after a possible reset).
 * The global step t and the log row k are DEVICE counters (*d_t, *d_k), advanced by the launch itself, so a
 * HIP graph {ssc_mpc_sample_actions(.., 0, d_t, ..), ssc_dyn_forward_sim(d_plan_state, s0_rows = P),
 * ssc_mpc_score, ssc_mpc_rollout_step} is replayed K times per chunk without touching the host.
 * d_ticket: one zero-initialised int32 (election of the block that advances the counters). */
typedef struct ssc_mpc_nav_state {
    int32_t *cur_idx;            /* [P] current waypoint (== ssc_mpc_problems.cur_idx) */
    const int32_t *start_idx;    /* [P] waypoint a fresh episode starts from */
    int32_t *actions_done;       /* [P] actions spent on the current waypoint */
    uint8_t *at_goal;            /* [P] close_enough_to_goal (:425-432); may be NULL */
    int32_t give_up_after, final_steps;
} ssc_mpc_nav_state;

int ssc_mpc_rollout_step(const ssc_env_params *p, const ssc_mpc_problems *problems, const ssc_mpc_nav_state *nav,
                         const float *d_A, const int32_t *d_best_idx, float noise_amount, uint64_t noise_seed,
                         uint64_t problem_id0, const ssc_rollout_state *state, const ssc_transition_log *log,
                         const ssc_episode_ring *ring, double *d_stats, uint64_t env_seed, uint64_t env_id0,
                         uint64_t *d_t, int32_t *d_k, int32_t *d_ticket, float *d_plan_state, ssc_stream_t stream);

/* One step of the VECTORISED SmartStartContinuous loop (smartstart/smartexploration/smartexplorationcontinuous.py:
 * 307-376) for P envs, everything after the scoring in ONE launch -- ssc_mpc_rollout_step with a per-env mode:
 *   mode[p] = 1  "smart_start_pathing": the executed action is the navigator's (best_sequence[0] + noise, as above), the
 *                waypoint bookkeeping runs on the new observation, and close_enough_to_goal hands the env over to
 *                the base agent (mode 0) for the rest of the episode (:333-339);
 *   mode[p] = 0  the base agent acts: d_actor_out[p] (Actor_Editted on the clipped planning state, ssc_actor_forward)
 *                + epsilon * OU noise, clip, scale twice -- DDPG_Baselines_agent.get_action, the OU state advancing
 *                only on these steps, stream and arithmetic of ssc_rollout's ACTOR policy.
 * A finished episode (goal / TimeLimit) resets the env and the OU state and runs start_new_episode (:341-370): with
 * probability *d_eta (uniform draw: word x of Philox(env_seed; env id, t, tag 8); plan: word y) the env takes a plan out of the pool
 * -- slot (pool[0] + word % pool[1]) % pool[2] of the plan arrays behind problems->plan_of, if pool[1] > 0 -- starts it
 * at waypoint 0 and navigates unless the reset state is already close enough to the plan's goal.
 * d_eta, d_ou_epsilon (one float each) and d_pool (int32[3]: first slot, plans on offer, slots) are DEVICE values, so a
 * captured HIP graph of the step keeps following the host's decay schedule and pool refreshes.  d_mode_log (may be
 * NULL) receives the mode each env ACTED in, row *d_k of a [K][P] byte matrix.  problems->plan_of must be writable. */
typedef struct ssc_smartstart_step {
    uint8_t *mode;               /* [P] */
    int32_t *plan_of;            /* [P] == problems->plan_of */
    const float *d_actor_out;    /* [P] */
    const float *d_eta, *d_ou_epsilon;
    const int32_t *d_pool;       /* [3] */
    ssc_ou_desc ou;              /* epsilon field unused (d_ou_epsilon) */
    float act_low, act_high;
    uint8_t *d_mode_log;         /* [K][P] or NULL */
    int64_t mode_log_stride;     /* row stride of d_mode_log (0: P) */
    int32_t *d_n_live;           /* optional: the counter of ssc_nav_compact, zeroed by this launch (the last one of a step) so
                                    that the next step's compaction starts from 0 without a launch of its own */
} ssc_smartstart_step;

/* The envs that are navigating (d_mode[i] != 0) as a compact list: d_list[0 .. *d_count) = their indices (any order),
 * *d_count their number.  *d_count must be 0 on entry (ssc_smartstart_step.d_n_live leaves it so).  One pass: ballot +
 * prefix inside a wave, one atomic per wave for its base. */
int ssc_nav_compact(int64_t n, const uint8_t *d_mode, int32_t *d_list, int32_t *d_count, ssc_stream_t stream);

int ssc_smartstart_rollout_step(const ssc_env_params *p, const ssc_mpc_problems *problems, const ssc_mpc_nav_state *nav,
                                const ssc_smartstart_step *ss, const float *d_A, const int32_t *d_best_idx,
                                float noise_amount, uint64_t noise_seed, uint64_t problem_id0,
                                const ssc_rollout_state *state, const ssc_transition_log *log, const ssc_episode_ring *ring,
                                double *d_stats, uint64_t env_seed, uint64_t env_id0, uint64_t *d_t, int32_t *d_k,
                                int32_t *d_ticket, float *d_plan_state, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * SmartStart selection (smartstart/smartexploration/smartexplorationcontinuous.py:223-305)
 * ------------------------------------------------------------------------------------- */

/* DDPG critic (Critic_Editted.__call__, DDPG_Baselines_editted/models_editted.py:78-100):
 *   x = relu(obs @ W1 + b1); x = concat(x, action); x = tanh|relu(x @ W2 + b2); q = x @ W3 + b3
 * W2 is [h1 + act_dim][h2]; weights fp32, TensorFlow layout, device. */
typedef struct ssc_critic_desc {
    int32_t obs_dim, act_dim, h1, h2;
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    int32_t last_layer_tanh;
    float obs_clip;             /* as in ssc_actor_desc (ddpg_editted.py:106-109); 0: no clip */
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b; /* LayerNorm (models_editted.py:85-86, 91-92) as in ssc_actor_desc; NULL: none */
} ssc_critic_desc;

/* q[m] = Critic(obs[m][obs_dim], act[m][act_dim]) -- the batched get_q_value of
 * ddpg_editted.py:274-279 once act = Actor(obs) (ssc_actor_forward). */
int ssc_critic_forward(const ssc_critic_desc *critic, int64_t m, const float *d_obs, const float *d_act,
                       float *d_q, ssc_stream_t stream);

/* scipy.stats.gaussian_kde(dataset).evaluate(points) [third-party, call site
 * smartexplorationcontinuous.py:260,275] for a bandwidth matrix chosen by the caller:
 *   pdf[i] = norm * sum_j exp(-0.5 * || Wh (points[i] - data[j]) ||^2)
 * Wh is the d x d row-major whitening matrix (chol(inv(covariance))^T, host array), norm =
 * 1 / (n * sqrt(det(2 pi covariance))).  data [n][d], points [m][d], pdf [m]; d <= SSC_MAX_STATE. */
int ssc_kde_evaluate(int32_t d, int64_t n, const float *d_data, int64_t m, const float *d_points,
                     const float *whitening, double norm, float *d_pdf, ssc_stream_t stream);

/* UCB1 over the candidate smart-start states (smartexplorationcontinuous.py:275-280):
 *   ucb[i] = alpha * value[i] + sqrt(beta * ln(D) / (D * pdf[i] * volume));  best = argmax (lowest
 * index on ties).  d_ucb [m] may be NULL; d_best [1]. */
int ssc_ucb_argmax(int64_t m, const float *d_value, const float *d_pdf, float alpha, float beta, double buffer_len,
                   double volume, float *d_ucb, int32_t *d_best, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * DDPG training step
 * ------------------------------------------------------------------------------------- */

/* DDPG_editted.train() + update_target_net() (DDPG_Baselines_editted/ddpg_editted.py:287-339) as
 * driven by DDPG_Baselines_agent.train (smartstart/RLAgents/DDPG_Baselines_agent.py:264-273), in the
 * configuration of every shipped run: no observation/return normalisation, no popart, no l2
 * regularisation, no gradient clipping.  Each network's parameters are ONE flat fp32 device array
 * in TensorFlow trainable_vars order [W1 | b1 | W2 | b2 | W3 | b3] (the order U.flatgrad and
 * MpiAdam use); Adam moments have the same shape.  Critic W2 is [critic_h1 + act_dim][critic_h2]. */
typedef struct ssc_ddpg_desc {
    int32_t obs_dim, act_dim, actor_h1, actor_h2, critic_h1, critic_h2;
    int32_t last_layer_tanh;
    int32_t batch_size;                                   /* 64 in every shipped run; 1..4096 through ssc_ddpg_train_ws */
    float *actor, *critic, *target_actor, *target_critic; /* device, flat */
    float *adam_m_actor, *adam_v_actor, *adam_m_critic, *adam_v_critic; /* device, flat, zero-initialised */
    int32_t *adam_t;                                      /* device [2]: MpiAdam step counters (actor, critic) */
    float gamma, tau, actor_lr, critic_lr;
    float beta1, beta2, epsilon;                          /* MpiAdam: 0.9, 0.999, 1e-8 (ddpg_editted.py:176,198) */
    float obs_clip;                                       /* > 0: obs0 / obs1 clipped to [-obs_clip, obs_clip] before every
                                                             network (ddpg_editted.py:106-109); 0: no clip */
    int32_t layer_norm;                                   /* 1: actor and critic carry LayerNorm (models_editted.py:45-46,50-51,
                                                             85-86,91-92): every flat vector is then
                                                             [W1|b1|beta1|gamma1|W2|b2|beta2|gamma2|W3|b3] (TF trainable_vars order;
                                                             tc.layers.layer_norm creates beta before gamma) and the step runs on
                                                             the multi-workgroup kernels (ssc_ddpg_train_ws) */
    float critic_l2_reg;                                  /* > 0: critic_loss += critic_l2_reg * sum(W^2) / 2 over the critic's
                                                             three dense kernels (ddpg_editted.py:183-191; the name filter keeps
                                                             all of them, models_editted.py names no layer 'output'); 0: none */
    float clip_norm;                                      /* > 0: every variable's gradient, actor and critic, clipped to this
                                                             2-norm (U.flatgrad(..., clip_norm), ddpg_editted.py:175, 197);
                                                             <= 0: none.  Either option runs the multi-workgroup kernels. */
} ssc_ddpg_desc;

/* Replay storage the batches are drawn from: row-major device arrays of `capacity` records
 * (the (s, a, r, t, s2) tuple of replay_buffer.py:53). */
typedef struct ssc_replay_view {
    const float *s, *a, *r;
    const uint8_t *t;
    const float *s2;
    int64_t capacity;
} ssc_replay_view;

/* The same storage, writable: a device-resident replay ring fed straight from rollout chunks.  Record
 * number j (counted since the ring was created) lives at row j % capacity -- the FIFO of the reference's
 * deque (replay_buffer.py:53-72): once full, the oldest record is overwritten.  act_dim must be 1. */
typedef struct ssc_replay_ring {
    float *s, *a, *r;
    uint8_t *t;
    float *s2;
    int64_t capacity;
    int32_t obs_dim, act_dim;
    /* Episode index (both NULL: not kept).  The reference keeps episode_starting_indices beside its deque
     * (replay_buffer.py:33-44, 109-115, 209-213) so that the path to any stored state can be recovered; a chunk of n
     * parallel envs interleaves n episodes, so the device ring keeps, per record, the number of steps of ITS env's
     * running episode up to and including the record (ep_steps [capacity], 1 = the episode's first recorded step).
     * Records of one env lie n record numbers apart (record number = steps * n + env), hence the episode of record j
     * is records j - (ep_steps-1)*n, ..., j - n, j -- valid for path recovery while the first of them is still in the
     * ring.  ep_run [n] carries every env's running step count from one append to the next (zero-initialised; the
     * caller zeroes it when it skips steps between two appends). */
    int32_t *ep_steps;
    int32_t *ep_run;
} ssc_replay_ring;

/* ReplayBuffer.add for a whole rollout chunk (replay_buffer.py:49-74; called per step from
 * DDPG_Baselines_agent.observe, DDPG_Baselines_agent.py:238-240, which scales the reward): appends the
 * K*n records of `log` ([K][n] SoA columns as ssc_rollout wrote them; record order = step-major, then env)
 * after the `start` records appended so far.  The caller keeps the running count (start += K*n); it is
 * deterministic, so no device counter and no host sync is needed. */
int ssc_replay_append(const ssc_replay_ring *ring, const ssc_transition_log *log, int32_t K, int64_t n,
                      int64_t start, float reward_scale, ssc_stream_t stream);

/* The same append for ONE SHARD of a step: the chunk holds envs [env_off, env_off + n) of n_total envs per step, its
 * record (k, e) gets record number start + k * n_total + env_off + e -- the learner of a sharded run appends every
 * rank's gathered records this way and ends up with the ring of the single-GPU run, whatever the world size.  `start`
 * counts whole steps of n_total records; K * n_total <= capacity.  ep_run (if kept) is indexed by env_off + e. */
int ssc_replay_append_shard(const ssc_replay_ring *ring, const ssc_transition_log *log, int32_t K, int64_t n,
                            int64_t start, int64_t n_total, int64_t env_off, float reward_scale, ssc_stream_t stream);

/* ReplayBuffer.sample_batch (replay_buffer.py:79-91: random.sample, i.e. uniform WITHOUT replacement
 * inside a batch) for n_batches batches at once: d_idx [n_batches][batch_size] row indices in
 * [0, size), size = min(records appended, capacity) >= batch_size, batch_size <= 4096.
 * Philox(seed; counter0 + batch, attempt << 8 | slot, TAG_REPLAY) for batch_size <= 64 (one wave per batch),
 * attempt << 16 | slot above (one workgroup per batch); oracle: replay_sample_indices. */
int ssc_replay_sample(uint64_t seed, uint64_t counter0, int64_t size, int32_t n_batches, int32_t batch_size,
                      int32_t *d_idx, ssc_stream_t stream);

/* ReplayBuffer.get_possible_smart_start_indices (replay_buffer.py:136-152: random.sample(range(first, len), n_ss), first =
 * the oldest episode start still in the buffer) on the device ring: up to n_ss DISTINCT buffer indices (0 = oldest
 * record, size-1 = newest; size = min(count, capacity)) drawn uniformly from the records whose whole episode prefix is
 * still in the ring.  Rounds of Philox(seed; counter, round << 20 | slot, TAG_SMART_START) candidates; in a round a slot
 * keeps its candidate unless it is invalid, already taken, or wanted by a lower slot (deterministic; oracle:
 * smart_start_indices).  d_idx [n_ss] int32 (unfilled slots -1), *d_n = number of indices delivered (< n_ss only when
 * fewer valid records exist or after max_rounds = 64).  n_ss <= 4096.  count = records appended so far, n = envs per
 * step of the appended chunks.  Workspace: ssc_replay_smart_start_workspace_bytes(n_ss). */
size_t ssc_replay_smart_start_workspace_bytes(int32_t n_ss);
int ssc_replay_smart_start_indices(const ssc_replay_ring *ring, int64_t count, int64_t n, int32_t n_ss, uint64_t seed,
                                   uint64_t counter, int32_t *d_idx, int32_t *d_n, void *d_workspace,
                                   size_t workspace_bytes, ssc_stream_t stream);

/* ReplayBuffer.get_episodic_path_to_buffer_index (replay_buffer.py:154-176): the states of the episode that contains
 * buffer index *d_buffer_index (device int32; e.g. an entry of d_idx above) up to that record, plus its s2:
 * d_path [max_len + 1][obs_dim], *d_len = number of rows written (episode steps so far + 1; 0 when the record's
 * episode start has left the ring; at most the newest max_len steps of the prefix are kept). */
int ssc_replay_episode_path(const ssc_replay_ring *ring, int64_t count, int64_t n, const int32_t *d_buffer_index,
                            int32_t max_len, float *d_path, int32_t *d_len, ssc_stream_t stream);

/* n_iters sequential training iterations in ONE launch (one workgroup: the iterations are a serial
 * chain through the parameters).  d_batch_idx [n_iters][batch_size] are record indices
 * (ReplayBuffer.sample_batch, replay_buffer.py:79-91, draws them on the host).  d_losses
 * [n_iters][2] = (critic_loss, actor_loss) per iteration, may be NULL.
 * Shapes: batch 64, act_dim 1.  The shipped 64-32 actor / critic with a 2- or 3-d observation runs a kernel compiled
 * for that shape; any other layer sizes <= 64 run a step interpreter as long as the batch's activations plus the four
 * parameter vectors fit the 160 KB of LDS (64-32 with obs_dim <= 8 does; 64-64 does not) -- otherwise SSC_EUNSUPPORTED
 * with the byte count in ssc_last_error(). */
int ssc_ddpg_train(const ssc_ddpg_desc *ddpg, const ssc_replay_view *replay, const int32_t *d_batch_idx,
                   int32_t n_iters, float *d_losses, ssc_stream_t stream);

/* The same training step for ANY layer sizes and batch sizes 1..4096 -- the reference's own grid of actor / critic
 * 64-32, 128-64, 200-100 (DDPG_Baselines_agent.py:86-92, data/ddpg_baselines_summaries/hidden_layer_size_experiment/)
 * and the large batches of a vectorised actor-learner loop.  Shapes the single-workgroup kernels cover (batch 64,
 * layers <= 64) still run there; everything else runs multi-workgroup: the batch is tiled over workgroups of 16 rows
 * (whole forward / backward chain per tile, weights streamed from L2), per-workgroup gradient partials are summed in
 * workgroup order by a second launch that also applies MpiAdam and the soft target update -- two launches per
 * iteration, bitwise reproducible.  d_workspace: ssc_ddpg_train_workspace_bytes(ddpg) bytes of device memory (the
 * gradient partials; caller-owned like every buffer).  SSC_EUNSUPPORTED only when a 16-row tile's activations exceed
 * the 160 KB of LDS (roughly: 2 h1 + 2 h2 of the actor + 2 h1 + 4 h2 of the critic > 2500 units). */
size_t ssc_ddpg_train_workspace_bytes(const ssc_ddpg_desc *ddpg);
int ssc_ddpg_train_ws(const ssc_ddpg_desc *ddpg, const ssc_replay_view *replay, const int32_t *d_batch_idx,
                      int32_t n_iters, float *d_losses, void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * normalize_observations (ddpg_editted.py:14-18, 100-109, 127-132, 281-285)
 * -------------------------------------------------------------------------------------
 * The running statistics of baselines 0.1.5 RunningMeanStd live in ONE device block of 2*obs_dim + 1 doubles,
 *   d_rms = [sum[obs_dim] | sumsq[obs_dim] | count]      (caller-initialised: 0, 1e-2, 1e-2)
 * Every network then sees clip((x - mean) / std, -obs_clip, obs_clip) with, in fp32,
 *   mean = f32(sum / count),  std = sqrtf(max(f32(sumsq / count) - mean * mean, 1e-2f))   (no contraction).
 * Kernels read the block when they start (never a host copy), so HIP graphs stay valid while it changes.
 *
 * ssc_obs_rms_update: adds sum(x), sum(x^2) and the row count (f64) of the obs0 columns of steps [k0, K) of a
 * transition log of n envs (dense or packed row_stride) to d_rms.  ssc_obs_rms_update_rows: the same for a row-major
 * [m][obs_dim] matrix.  Deterministic run to run (fixed-order reduction, no atomics); d_workspace holds
 * ssc_obs_rms_update_workspace_bytes(obs_dim) bytes and may be reused once the call's work is done in stream order.
 *
 * The *_rms variants are the calls above plus a trailing d_rms; d_rms == NULL behaves exactly like the plain call.
 * ssc_rollout_rms reads the block once per launch (the statistics are frozen for the chunk, like the weights); a
 * random policy ignores it. */
size_t ssc_obs_rms_update_workspace_bytes(int32_t obs_dim);
int ssc_obs_rms_update(int32_t obs_dim, const ssc_transition_log *log, int32_t k0, int32_t K, int64_t n, double *d_rms,
                       void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);
int ssc_obs_rms_update_rows(int32_t obs_dim, int64_t m, const float *d_x, double *d_rms, void *d_workspace,
                            size_t workspace_bytes, ssc_stream_t stream);
int ssc_actor_forward_rms(const ssc_actor_desc *actor, int64_t m, const float *d_obs, float *d_act, ssc_stream_t stream,
                          const double *d_rms);
int ssc_critic_forward_rms(const ssc_critic_desc *critic, int64_t m, const float *d_obs, const float *d_act, float *d_q,
                           ssc_stream_t stream, const double *d_rms);
int ssc_rollout_rms(const ssc_env_params *p, const ssc_policy_desc *policy, int64_t n, int32_t K,
                    const ssc_rollout_state *state, const ssc_transition_log *log,
                    const ssc_episode_ring *ring, double *d_stats, uint64_t seed, uint64_t env_id0,
                    uint64_t step0, ssc_stream_t stream, const double *d_rms);
int ssc_ddpg_train_ws_rms(const ssc_ddpg_desc *ddpg, const ssc_replay_view *replay, const int32_t *d_batch_idx,
                          int32_t n_iters, float *d_losses, void *d_workspace, size_t workspace_bytes, ssc_stream_t stream,
                          const double *d_rms);

/* ---------------------------------------------------------------------------------------
 * A population of SmartStart pairs in one captured step
 *
 * The reference fans SmartStart + DDPG over seeds and hyper-parameters
 * (examples/continuous/SmartStart_DDPG_Baselines_experimenter.py); every pair runs SmartStartContinuous.get_action /
 * observe / start_new_episode (smartstart/smartexploration/smartexplorationcontinuous.py:307-376) on envs, an agent, an
 * eta and a plan pool of its own.  The two calls below serve the per-pair state of ALL pairs in one launch each.
 * ------------------------------------------------------------------------------------- */

/* One actor of a population and the rows of the call's observation matrix it acts on.  Declared tag first like the other
 * *_many items; tests/test_smartstart_many_host.py holds the struct's size and offsets to the ctypes mirror. */
struct ssc_actor_many_item {
    ssc_actor_desc actor;
    const double  *d_rms;   /* this actor's RunningMeanStd block; the call's class decides whether it is read */
    int64_t        row0;    /* the item's rows: [row0, row0 + rows) of the call's m */
    int64_t        rows;    /* 0: the item is skipped and nothing else of it is read */
};
typedef struct ssc_actor_many_item ssc_actor_many_item;

/* The kernel class one many-call can serve this actor with (>= 0), or -1: a descriptor ssc_actor_forward refuses.
 * class = 2 * body + (has_rms ? 1 : 0); bodies, by ssc_actor_forward's own rule for m > 32: 0 / 1 the fp32 64-32 kernel
 * with obs_dim 2 / 3; 2 / 3 the bf16 MFMA kernel for h1 <= 64, h2 <= 32; 4 / 5 for h1 <= 128, h2 <= 64; 6 / 7 the
 * LDS-staged one up to 224-128; 8 the generic fp32 kernel (any sizes, LayerNorm included).  A pure function of shape,
 * precision and has_rms. */
int ssc_actor_many_class(const ssc_actor_desc *actor, int has_rms);

/* ssc_actor_forward[_rms] for a population of actors in ONE launch: item y acts on rows [row0, row0 + rows) of d_obs
 * [m][obs_dim] and writes the same rows of d_act [m][act_dim].  Grid row y runs item y; its blocks are anchored at row0, so
 * the partition into blocks and waves is that of the actor's own call on its slice (grid x = the largest item's block
 * count; surplus blocks leave before any barrier or LDS staging).  The kernel runs the device bodies the single call
 * dispatches at m > 32, so every owned row of d_act holds, bit for bit, what ssc_actor_forward[_rms](&actor, rows,
 * d_obs + row0 * obs_dim, d_act + row0 * act_dim, .., d_rms) leaves there -- for an item of <= 32 rows too (the single
 * call's row kernel returns the generic kernel's bits).  Rows no item owns are untouched.
 * One call serves ONE class (ssc_actor_many_class with has_rms = d_rms != NULL); every working item has the obs_dim and
 * act_dim of the first.  Conventions of the other *_many calls: the host array is validated completely before any HIP
 * call, the caller's device copy of the same bytes must be complete on `stream`, the library copies nothing, item indices
 * appear in ssc_last_error().  n_items 1..65535 (more: SSC_EUNSUPPORTED).  The single call's per-descriptor checks apply to
 * every item with rows > 0 (its codes) as they stand at m > 32: an fp32 network too wide for the generic kernel's LDS is
 * SSC_EUNSUPPORTED at any row count (the single call serves <= 32 rows of it through its row kernel); two items of different classes are SSC_EUNSUPPORTED naming both and their classes, an item with
 * no class is SSC_EUNSUPPORTED; a range outside [0, m), two overlapping ranges (gaps are legal) or NULL tables are
 * SSC_EINVAL.  m == 0, or every item empty: SSC_OK without a launch. */
int ssc_actor_forward_many(const ssc_actor_many_item *h_items, const ssc_actor_many_item *d_items, int32_t n_items, int64_t m,
                           const float *d_obs, float *d_act, ssc_stream_t stream);

/* One SmartStart pair of a population step: a row of a DEVICE table the host rewrites between chunks (the kernel reads it
 * when it starts, so a captured graph follows the host's decay schedule and pool refreshes exactly as
 * ssc_smartstart_step.d_eta / d_ou_epsilon / d_pool let a single pair's graph).  tests/test_smartstart_many_host.py holds
 * the struct's size and offsets to the ctypes mirror. */
struct ssc_smartstart_pair {
    int32_t env0, n_envs;                       /* the pair's envs: [env0, env0 + n_envs) of the call's P */
    int32_t slot0;                              /* first slot of its window of the plan arrays */
    int32_t pool_first, pool_count, pool_slots; /* ssc_smartstart_step.d_pool, relative to slot0 */
    float   eta, ou_epsilon;                    /* ssc_smartstart_step.d_eta / d_ou_epsilon */
    ssc_ou_desc ou;                             /* epsilon field unused */
};
typedef struct ssc_smartstart_pair ssc_smartstart_pair;

/* ssc_smartstart_rollout_step for n_pairs SmartStart pairs in ONE launch.  The call's P envs (one VecEnv, RNG streams keyed
 * by the global env / problem id as ever) are split into contiguous ranges, one per pair; grid row y is pair y, its blocks
 * anchored at env0 (grid x = the largest pair's block count).  The step is the single kernel's, arithmetic and order of
 * loads unchanged; eta, the OU epsilon, the OU process and the plan pool come from d_pairs[y]: a fresh plan is slot
 * slot0 + (pool_first + word % pool_count) % pool_slots of the plan arrays.  `ss` keeps mode, plan_of, d_actor_out, the
 * action bounds, d_mode_log and mode_log_stride; its d_eta, d_ou_epsilon, d_pool and ou are not read, and d_n_live must be
 * NULL (the population path has no compact live list).  d_stats is [n_pairs][4] (may be NULL): row y receives pair y's
 * block sums.  The ticket counts all blocks of the 2-D grid and advances *d_t / *d_k once.
 * Host checks before any HIP call: those of the single call; n_pairs 1..65535 (more: SSC_EUNSUPPORTED, as in the other
 * *_many calls); ranges non-empty, in order, disjoint and
 * inside [0, P); pool_slots >= 1, 0 <= pool_first < pool_slots, 0 <= pool_count <= pool_slots; slot0 >= 0 (SSC_EINVAL with
 * the pair index in ssc_last_error()).  The host table is validated; the caller's device copy must be complete on
 * `stream` and hold rows that pass the same checks whenever the launch (or a replay of its graph) runs. */
int ssc_smartstart_rollout_step_many(const ssc_env_params *p, const ssc_mpc_problems *problems, const ssc_mpc_nav_state *nav,
                                     const ssc_smartstart_step *ss, const ssc_smartstart_pair *h_pairs,
                                     const ssc_smartstart_pair *d_pairs, int32_t n_pairs, const float *d_A,
                                     const int32_t *d_best_idx, float noise_amount, uint64_t noise_seed, uint64_t problem_id0,
                                     const ssc_rollout_state *state, const ssc_transition_log *log,
                                     const ssc_episode_ring *ring, double *d_stats, uint64_t env_seed, uint64_t env_id0,
                                     uint64_t *d_t, int32_t *d_k, int32_t *d_ticket, float *d_plan_state, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The smart-start SELECTION of a population of pairs, one launch per stage
 *
 * get_smart_start_path (smartexplorationcontinuous.py:223-305) for every pair at once: candidates, Scott bandwidth,
 * V = Q(s, pi(s)), Gaussian KDE, UCB1 top-k, episodic paths.  ONE item table serves all six calls; grid row y is item y.
 * The actor forward between the candidates and the critic goes through ssc_actor_forward_many on the pooled candidate
 * matrix (d_cand of item y = pool + row0 * obs_dim).
 * ------------------------------------------------------------------------------------- */

/* One pair's selection.  Declared tag first like the other *_many items; tests/test_select_many_host.py holds the struct's
 * size and offsets to the ctypes mirror.  The host keeps count, stride, n_data and scott current; nothing a launch needs
 * depends on a device result.  size = min(count, ring.capacity).  An item with n_ss == 0 or count == 0 is EMPTY: it is
 * skipped and nothing else of it is read. */
struct ssc_select_many_item {
    ssc_replay_ring ring;       /* with the episode index (ep_steps) */
    int64_t  count;             /* records appended so far */
    int64_t  n;                 /* envs per step of the appended chunks */
    int32_t  n_ss;              /* candidate slots, <= 4096 */
    int32_t  n_plans;           /* 1..64, <= n_ss not required */
    uint64_t seed, counter;     /* the Philox key of ssc_replay_smart_start_indices */
    int64_t  stride;            /* KDE data set: logical rows j * stride, j < n_data, of "ring states oldest first, then */
    int64_t  n_data;            /*   the newest record's s2" (size + 1 rows); n_data = ceil((size + 1) / stride) */
    double   scott;             /* (n_data ** (-1.0 / (d + 4))) ** 2, computed by the host */
    ssc_actor_desc  actor;      /* the plain actor; read by the caller's ssc_actor_forward_many table, checked here for obs_dim */
    ssc_critic_desc critic;
    const double *d_rms;        /* the agent's RunningMeanStd block or NULL */
    float    alpha, beta;       /* exploitation / exploration parameter */
    double   volume;
    int32_t  max_len;           /* paths keep at most the newest max_len steps */
    int32_t  pad;
    int64_t  row0;              /* the item's rows [row0, row0 + n_ss) of the call's action matrix (ssc_critic_forward_many) */
    int32_t *d_idx;             /* [n_ss] buffer indices, unfilled slots -1 */
    int32_t *d_n_cand;          /* [1] */
    float   *d_cand;            /* [n_ss][obs_dim]; unfilled slots zero */
    float   *d_wh;              /* [d * d] whitening, row-major */
    double  *d_norm;            /* [1] */
    int32_t *d_status;          /* [1] 0: bandwidth found; 1: n_data < 2 or a non-positive / non-finite pivot */
    float   *d_value;           /* [n_ss] */
    float   *d_pdf;             /* [n_ss] */
    float   *d_ucb;             /* [n_ss]; unfilled slots NaN */
    int32_t *d_chosen;          /* [n_plans] buffer indices, unused places -1 */
    float   *d_path;            /* [n_plans][max_len + 1][obs_dim] */
    int32_t *d_len;             /* [n_plans] rows of each path, 0: none */
    void    *d_workspace;       /* ssc_replay_smart_start_workspace_bytes(n_ss) bytes, this item's own */
    size_t   workspace_bytes;
};
typedef struct ssc_select_many_item ssc_select_many_item;

/* Conventions of all six calls (those of the other *_many calls): the host array is validated completely before any HIP
 * call, the caller's device copy of the same bytes must be complete on `stream`, the library copies and allocates nothing,
 * item indices appear in ssc_last_error().  n_items 1..65535 (more: SSC_EUNSUPPORTED); NULL tables, n_items < 1: SSC_EINVAL.
 * Every call checks of a non-empty item (SSC_EINVAL): ring.capacity > 0, ring.obs_dim in 1..SSC_MAX_STATE, count >= 0,
 * n >= 1, size <= 2^31 - 1, n_ss in 0..4096, and the pointers the call itself reads or writes non-NULL.  Every item
 * empty: SSC_OK without a launch.  Outputs of pair y in a call of P items equal, bit for bit, the call with that item
 * alone. */

/* ssc_replay_smart_start_indices per item (one workgroup each): d_idx and *d_n_cand bit for bit what the single call
 * delivers for that ring and key.  Behind its last barrier the workgroup gathers d_cand[slot] = ring.s2[physical(idx[slot])]
 * (zeros for idx = -1).  Also checks: ep_steps / s2 / d_idx / d_n_cand / d_cand non-NULL, workspace large enough. */
int ssc_replay_smart_start_indices_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items,
                                        ssc_stream_t stream);

/* kde_scott_bandwidth per item on the device, in fp64: the two-pass covariance (ddof = 1) of the data set (read from the
 * ring in place), cov *= scott, wh = chol(inv(cov))^T rounded to float, norm = 1 / (n_data * sqrt(det(2 pi cov))).  One
 * workgroup per item; partial sums merged in a fixed order (wave shuffles, then waves in order): the same bits run to run.
 * *d_status = 1 and nothing else is promised when n_data < 2 or a Cholesky pivot is non-positive or non-finite.
 * Also checks: stride >= 1, n_data == ceil((size + 1) / stride), scott > 0 and finite, ring.s / s2 / d_wh / d_norm /
 * d_status non-NULL. */
int ssc_kde_scott_bandwidth_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items,
                                 ssc_stream_t stream);

/* ssc_critic_forward[_rms] per item: q of rows d_cand [n_ss][obs_dim] with the actions d_act + row0 * act_dim (d_act is
 * [m][act_dim]) into d_value; blocks anchored at the item's first row; every row bit for bit the single call's.  Items with
 * and without d_rms share the launch (each block runs its item's instantiation of the one body).  The single call's
 * per-descriptor checks and codes apply; critic.obs_dim must equal ring.obs_dim; [row0, row0 + n_ss) inside [0, m). */
int ssc_critic_forward_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items, int64_t m,
                            const float *d_act, ssc_stream_t stream);

/* ssc_kde_evaluate per item: d_pdf [n_ss] of the queries d_cand under the KDE of the item's data set, read from the ring in
 * place (the same partition of the data onto threads and loop trips), with wh / norm read from d_wh / d_norm: bit for bit
 * what ssc_kde_evaluate returns on the materialised data set with that whitening and norm.  One call serves ONE obs_dim
 * (SSC_EUNSUPPORTED naming both items otherwise).  An item with *d_status != 0 writes nothing. */
int ssc_kde_evaluate_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items,
                          ssc_stream_t stream);

/* UCB1 and the n_plans best per item (one workgroup each): d_ucb[i] by ssc_ucb_argmax's expression with buffer_len = size for
 * live slots (idx >= 0; NaN for the others), then d_chosen = idx[slot] of the n_plans best live slots, unused places -1.
 * Order: descending ucb, NaN below -inf, lowest slot first on ties -- for n_plans = 1 ssc_ucb_argmax's answer on the live
 * slots.  An item with *d_status != 0 gets d_chosen = -1 throughout.  Also checks: n_plans in 1..64, volume > 0. */
int ssc_ucb_topk_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items, ssc_stream_t stream);

/* ssc_replay_episode_path for every (item, plan): d_path[plan] / d_len[plan] for buffer index d_chosen[plan]; -1, or an
 * episode start that has left the ring, gives len = 0.  Also checks: max_len >= 1, n_plans in 1..64. */
int ssc_replay_episode_path_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items,
                                 ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * normalize_returns + enable_popart (ddpg_editted.py:129-133, 140-149, 201-217, 291-301; arXiv 1602.07714)
 * -------------------------------------------------------------------------------------
 * ret_rms is the same RunningMeanStd as above with one column: d_ret_rms = [sum | sumsq | count] in f64, caller-
 * initialised (0, 1e-2, 1e-2); mean and std in the fp32 arithmetic above.  The critic then outputs NORMALISED values and
 * everything that reads Q denormalises: Q = q * std + mean (:129-131).  One iteration on a batch of B rows:
 *   1. y_i = r_i + (1 - t_i) gamma (q'_i sigma_old + mu_old), q' from the target networks (:132-133, :292-296);
 *   2. sum += sum (double) y_i, sumsq += sum (double) y_i^2, count += B (:297) -> mu_new, sigma_new;
 *   3. critic AND target critic: W3 <- W3 sigma_old / sigma_new, b3 <- (b3 sigma_old + mu_old - mu_new) / sigma_new
 *      (:209-217; Adam moments untouched), so that sigma q + mu is preserved;
 *   4. the usual step with critic loss mean((q - (y - mu_new) / sigma_new)^2) (+ the l2 term over the rescaled W3) and
 *      actor loss -mean(q(s, pi(s)) sigma_new + mu_new); d_losses holds these two (:181-192, :170).
 * With normalize_returns alone ret_rms is never updated (the only call site, :291-297, is under popart): mean 0, std 1,
 * the plain step -- call ssc_ddpg_train_ws[_rms].  This entry point is the conjunction.
 *
 * Every shape and batch 1..4096 runs the multi-workgroup kernels: four launches per iteration (target pass, renormalise,
 * gradient pass, apply), no atomics, fixed summation order: the same bits run to run.  The statistics are read from
 * device memory when a kernel starts (no host read, no synchronisation inside), so a captured graph stays valid.
 * d_workspace: ssc_ddpg_train_popart_workspace_bytes(ddpg) bytes, laid out [the ssc_ddpg_train_workspace_bytes(ddpg) of the
 * plain step | y [batch_size] fp32 | per-workgroup (sum y, sum y^2) [ceil(batch_size / 16)][2] f64 | (mu_old, sigma_old,
 * mu_new, sigma_new) fp32 + padding, 256 bytes], each part rounded up to 256 bytes; after the call the last three hold
 * the last iteration's values.  d_rms: the observation statistics or NULL.
 * d_ret_rms == NULL behaves exactly like ssc_ddpg_train_ws_rms. */
size_t ssc_ddpg_train_popart_workspace_bytes(const ssc_ddpg_desc *ddpg);
int ssc_ddpg_train_ws_popart(const ssc_ddpg_desc *ddpg, const ssc_replay_view *replay, const int32_t *d_batch_idx,
                             int32_t n_iters, float *d_losses, void *d_workspace, size_t workspace_bytes,
                             ssc_stream_t stream, const double *d_rms /* obs statistics or NULL */,
                             double *d_ret_rms /* [sum | sumsq | count], read and written */);

/* ---------------------------------------------------------------------------------------
 * A population of independent DDPG agents in one learner launch
 * -------------------------------------------------------------------------------------
 * The reference fans seeds x hyper-parameter grids out over processes (experimenter.py); the device-side counterpart for
 * the shipped shape: agent p's n_iters iterations run in workgroup p of ONE launch, each exactly as ssc_ddpg_train /
 * ssc_ddpg_train_ws_rms would run them alone -- the same bits.  Workgroups share nothing: no atomics, no workspace.
 * Every agent must have the shipped shape (64-32 actor and critic, batch 64, act_dim 1, obs_dim 2 or 3; no LayerNorm,
 * critic_l2_reg or clip_norm: otherwise SSC_EUNSUPPORTED with the agent's index in ssc_last_error()); obs_dim and
 * last_layer_tanh are the same for the whole population, d_rms is NULL for all agents or for none, and no two agents
 * share any of the nine parameter / optimiser arrays or adam_t (SSC_EINVAL: two workgroups would race on it).  Everything
 * else -- rings, indices, losses, gamma, tau, learning rates, obs_clip, n_iters -- is per agent.
 * The two structs are declared tag first; tests/test_ddpg_many_host.py holds their sizes and offsets to the ctypes mirrors. */
struct ssc_ddpg_many_item {
    ssc_ddpg_desc   ddpg;          /* this agent's arrays and hyper-parameters */
    ssc_replay_view replay;        /* this agent's ring */
    const int32_t  *d_batch_idx;   /* [n_iters][64] */
    float          *d_losses;      /* [n_iters][2] or NULL */
    const double   *d_rms;         /* normalize_observations block or NULL -- all agents or none */
    int32_t         n_iters;       /* >= 0, per agent; 0: the agent is left exactly as it is */
};
typedef struct ssc_ddpg_many_item ssc_ddpg_many_item;

/* h_items: host array [n_agents], validated here before any HIP call.  d_items: the caller's device copy of the same
 * bytes, complete on `stream` before this call (caller-owned like every buffer; the library copies nothing).  All
 * n_iters == 0: SSC_OK without a launch. */
int ssc_ddpg_train_many(const ssc_ddpg_many_item *h_items, const ssc_ddpg_many_item *d_items, int32_t n_agents,
                        ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * A population of ANY mix of shapes on the multi-workgroup learner, in grouped launches
 * -------------------------------------------------------------------------------------
 * What ssc_ddpg_train_many is for the shipped shape, for every descriptor ssc_ddpg_train_ws[_rms] runs on the
 * multi-workgroup kernels: layers wider than 64 (the reference's 128-64 / 200-100 grid), batch sizes 1..4096, LayerNorm,
 * critic_l2_reg, clip_norm, any obs_dim / last_layer_tanh, statistics on some agents and not on others -- all mixed in one
 * call.  Grid row p of every launch is an agent: 2 launches per iteration for the call (3 with critic_l2_reg /
 * clip_norm somewhere) instead of 2 or 3 per agent and iteration, and agent p's result -- the ten arrays, both Adam
 * counters, the losses -- is bit for bit what ssc_ddpg_train_ws / ssc_ddpg_train_ws_rms gives it alone (the kernels share
 * the per-agent arithmetic; nothing is summed across agents).  Pop-Art agents have grouped launches of their own:
 * ssc_ddpg_train_many_popart below.
 *
 * The item is ssc_ddpg_many_item plus the agent's own workspace, sized by ssc_ddpg_train_workspace_bytes and laid out as
 * the single-agent call lays it out.  d_batch_idx is [n_iters][batch_size] of THIS agent's batch size.
 *
 * The kernels read per-agent tables from a device array, the PLAN; the library allocates nothing, so the caller owns it:
 *   1. ssc_ddpg_train_many_wide_plan validates the items and fills h_plan (host memory, pinned if the copy is to be
 *      asynchronous), ssc_ddpg_train_many_wide_plan_bytes(n_agents) bytes; agent p's part depends on item p only;
 *   2. the caller copies h_plan to d_plan (complete on `stream` before the call);
 *   3. ssc_ddpg_train_many_wide validates again -- everything on the host copies, before any HIP call; a plan that no
 *      longer matches the items is SSC_EINVAL -- and launches.
 * Per-iteration quantities (the index rows, the losses row) are derived from the iteration index, a kernel argument: a
 * plan stays valid, call after call, until a pointer, a shape or an iteration count changes.
 *
 * Refused (SSC_EINVAL unless said otherwise): n_agents < 1 (above 65535: SSC_EUNSUPPORTED), a NULL array, an item that
 * fails the single-agent checks, an item with n_iters > 0 that ssc_ddpg_train_ws[_rms] would not run on the
 * multi-workgroup kernels (SSC_EUNSUPPORTED, the agent and its path in ssc_last_error(); ssc_ddpg_learner_path tells
 * beforehand), a workspace below ssc_ddpg_train_workspace_bytes, a tile above the 160 KB of LDS (SSC_EUNSUPPORTED), two
 * agents on one parameter / optimiser array or workspace.  All n_iters == 0: SSC_OK without a launch; such an item may
 * bring NULL arrays and no workspace, and only its shape is checked. */
struct ssc_ddpg_many_wide_item {
    ssc_ddpg_desc   ddpg;            /* this agent's arrays and hyper-parameters */
    ssc_replay_view replay;          /* this agent's ring */
    const int32_t  *d_batch_idx;     /* [n_iters][ddpg.batch_size] */
    float          *d_losses;        /* [n_iters][2] or NULL */
    const double   *d_rms;           /* normalize_observations block or NULL, per agent */
    int32_t         n_iters;         /* >= 0, per agent; 0: the agent is left exactly as it is */
    void           *d_workspace;     /* this agent's own, ssc_ddpg_train_workspace_bytes(&ddpg) bytes */
    size_t          workspace_bytes;
};
typedef struct ssc_ddpg_many_wide_item ssc_ddpg_many_wide_item;

size_t ssc_ddpg_train_many_wide_plan_bytes(int32_t n_agents);   /* linear in n_agents; 0 for n_agents < 1 */
int ssc_ddpg_train_many_wide_plan(const ssc_ddpg_many_wide_item *h_items, int32_t n_agents, void *h_plan, size_t plan_bytes);
int ssc_ddpg_train_many_wide(const ssc_ddpg_many_wide_item *h_items, const void *h_plan, const void *d_plan, int32_t n_agents,
                             ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Pop-Art agents of any mix of shapes in grouped launches
 * -------------------------------------------------------------------------------------
 * What ssc_ddpg_train_many_wide is for ssc_ddpg_train_ws[_rms], for ssc_ddpg_train_ws_popart: every descriptor that call
 * runs (any layer sizes, the shipped 64-32 x 64 included; batch 1..4096; LayerNorm, critic_l2_reg, clip_norm, statistics
 * on some agents and not on others), all mixed in one call.  Grid row p of every launch is an agent: per iteration a
 * target pass, ONE renormalise launch (a workgroup per agent), a gradient pass and the apply pass -- 4 launches for the
 * call, 5 with critic_l2_reg / clip_norm somewhere; one more target and one more gradient launch where agents with and
 * without observation statistics are mixed, one more apply launch where agents with and without critic_l2_reg /
 * clip_norm are -- instead of 4 or 5 per agent and iteration.  Agent p's result -- the ten arrays, both Adam counters,
 * the losses, its ret_rms block and its workspace -- is bit for bit what ssc_ddpg_train_ws_popart gives it alone; no
 * atomics, fixed summation order.
 *
 * The item is ssc_ddpg_many_wide_item plus d_ret_rms.  The workspace is the agent's own, at least
 * ssc_ddpg_train_popart_workspace_bytes(&ddpg) bytes, laid out as the single-agent call lays it out: after the call it
 * holds that agent's last y, partials and (mu_old, sigma_old, mu_new, sigma_new).  The plan protocol is that of
 * ssc_ddpg_train_many_wide (plan on the host, the caller copies it, validate again and launch); the plan's format is its
 * own, ssc_ddpg_train_many_popart_plan_bytes(n_agents) bytes.
 *
 * Refused (SSC_EINVAL unless said otherwise), on the host before any HIP call and with the agent's index in
 * ssc_last_error(): n_agents < 1 (above 65535: SSC_EUNSUPPORTED), a NULL array, an item that fails the single-agent
 * checks, d_ret_rms == NULL on an item with iterations (a plain agent belongs in ssc_ddpg_train_many_wide), a workspace
 * below ssc_ddpg_train_popart_workspace_bytes, a tile above the 160 KB of LDS (SSC_EUNSUPPORTED), two agents on one
 * parameter / optimiser array, one workspace or one ret_rms block, a plan that no longer matches the items.  All
 * n_iters == 0: SSC_OK without a launch; such an item may bring NULL arrays and only its shape is checked. */
struct ssc_ddpg_many_popart_item {
    ssc_ddpg_desc   ddpg;            /* this agent's arrays and hyper-parameters */
    ssc_replay_view replay;          /* this agent's ring */
    const int32_t  *d_batch_idx;     /* [n_iters][ddpg.batch_size] */
    float          *d_losses;        /* [n_iters][2] or NULL */
    const double   *d_rms;           /* normalize_observations block or NULL, per agent */
    int32_t         n_iters;         /* >= 0, per agent; 0: the agent is left exactly as it is */
    void           *d_workspace;     /* this agent's own, ssc_ddpg_train_popart_workspace_bytes(&ddpg) bytes */
    size_t          workspace_bytes;
    double         *d_ret_rms;       /* this agent's own [sum | sumsq | count], read and written */
};
typedef struct ssc_ddpg_many_popart_item ssc_ddpg_many_popart_item;

size_t ssc_ddpg_train_many_popart_plan_bytes(int32_t n_agents);   /* linear in n_agents; 0 for n_agents < 1 */
int ssc_ddpg_train_many_popart_plan(const ssc_ddpg_many_popart_item *h_items, int32_t n_agents, void *h_plan, size_t plan_bytes);
int ssc_ddpg_train_many_popart(const ssc_ddpg_many_popart_item *h_items, const void *h_plan, const void *d_plan, int32_t n_agents,
                               ssc_stream_t stream);

/* Which learner ssc_ddpg_train (have_workspace = 0) / ssc_ddpg_train_ws[_rms] (have_workspace = 1; have_rms: a statistics
 * block comes with the call) runs a descriptor on, the SSC_DDPG_INTERPRETER / SSC_DDPG_WIDE switches of the environment
 * included: one of the values below, or SSC_EINVAL for a NULL or unsized descriptor.  Host only. */
enum {
    SSC_DDPG_PATH_FIXED = 0,            /* the shipped 64-32 shape at batch 64, one workgroup */
    SSC_DDPG_PATH_FIXED_TILED = 1,      /* the shipped networks at batches of several 64-row tiles */
    SSC_DDPG_PATH_INTERPRETER = 2,      /* other layers <= 64 at batch 64, one workgroup */
    SSC_DDPG_PATH_WIDE = 3,             /* the multi-workgroup kernels */
    SSC_DDPG_PATH_NEEDS_WORKSPACE = 4   /* ssc_ddpg_train refuses it: call ssc_ddpg_train_ws */
};
int ssc_ddpg_learner_path(const ssc_ddpg_desc *ddpg, int have_workspace, int have_rms);

struct ssc_replay_sample_key {
    uint64_t seed, counter0;
    int64_t size;
};
typedef struct ssc_replay_sample_key ssc_replay_sample_key;

/* ssc_replay_sample for n_agents rings in one launch: d_idx [n_agents][n_batches][batch_size], agent p's rows drawn with
 * h_keys[p] exactly as ssc_replay_sample(seed, counter0, size, n_batches, batch_size, ..) draws them.  batch_size 1..64
 * (the one-wave kernel; larger: SSC_EUNSUPPORTED), every size >= batch_size.  d_keys: the device copy of h_keys, complete
 * on `stream` before this call. */
int ssc_replay_sample_many(const ssc_replay_sample_key *h_keys, const ssc_replay_sample_key *d_keys, int32_t n_agents,
                           int32_t n_batches, int32_t batch_size, int32_t *d_idx, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The rest of a population chunk in one launch each: rollout, epsilon decay, replay append and
 * observation statistics of P (env set, agent) PAIRS
 * -------------------------------------------------------------------------------------
 * Each entry point below replaces P calls of a single one and writes, bit for bit, what those calls write (one
 * exception: the f64 reward sum d_stats[0] of a pair with more than one workgroup is an atomic sum in both forms, so its
 * last bits depend on arrival order in both).  The conventions are ssc_ddpg_train_many's: a host array that is validated
 * before any HIP call, the caller's device copy of the same bytes, complete on `stream` before the call; the library
 * copies nothing; the pair's index -- or both indices -- is in ssc_last_error().  The structs are declared tag first;
 * tests/test_rollout_many_host.py holds their sizes and offsets to the ctypes mirrors.
 *
 * What changes with every chunk lives in a second, small array used like ssc_replay_sample_key: 16 bytes per pair, so that
 * a steady-state chunk uploads the cursors and nothing else.  ssc_rollout_many reads step0, ssc_replay_append_many
 * replay_start, from the same array. */
struct ssc_pair_cursor {
    uint64_t step0;        /* ssc_rollout's step0 of this chunk */
    int64_t  replay_start; /* ssc_replay_append's start: records appended to the pair's ring so far */
};
typedef struct ssc_pair_cursor ssc_pair_cursor;

/* What one ssc_rollout_rms call takes, except step0 (the pair's cursor) and K (one value for the population). */
struct ssc_rollout_many_item {
    ssc_env_params     params;
    ssc_policy_desc    policy;
    int64_t            n;        /* >= 1, per pair */
    ssc_rollout_state  state;
    ssc_transition_log log;      /* read when has_log */
    ssc_episode_ring   ring;     /* read when has_ring */
    int32_t            has_log;  /* all pairs or none */
    int32_t            has_ring; /* per pair */
    double            *d_stats;  /* [4] or NULL */
    uint64_t           seed, env_id0;
    const double      *d_rms;    /* normalize_observations block or NULL -- all pairs or none */
};
typedef struct ssc_rollout_many_item ssc_rollout_many_item;

/* ssc_rollout_rms for n_pairs pairs in one launch: grid row p runs pair p's workgroups (grid x = the largest pair's
 * workgroup count; the others' surplus workgroups exit at once).  Replaces one ssc_rollout / ssc_rollout_rms per pair.
 * The launch serves ONE kernel instantiation, the ones the population loop's agents select today: SSC_POLICY_ACTOR at
 * SSC_PREC_BF16_MFMA with h1 <= 64, h2 <= 32, act_dim 1, no LayerNorm (anything else, the random policy included:
 * SSC_EUNSUPPORTED naming the pair) -- on MountainCar the straight-line fused policy (unit action bounds, noise on, inert
 * or normalised clip) or the generic MFMA policy, on Pendulum the generic one.  Uniform over the population (SSC_EINVAL
 * naming the first pair that differs from pair 0): the env kind, which of the two policies ssc_rollout would choose,
 * last_layer_tanh for the fused policy, d_rms (all or none), has_log (all or none).  One pair whose log columns are not
 * within 4 GB above obs[0] sends all pairs to the generic log stores (the same values).  Free per pair: n, env
 * constants, OU constants and d_epsilon, action bounds inside the class, obs_clip, seed, env_id0, has_ring.
 * No two pairs share a state column, a log column, an episode ring array or cursor, or a d_stats block (SSC_EINVAL naming
 * both).  K == 0: SSC_OK without a launch. */
int ssc_rollout_many(const ssc_rollout_many_item *h_items, const ssc_rollout_many_item *d_items,
                     const ssc_pair_cursor *h_cursors, const ssc_pair_cursor *d_cursors, int32_t n_pairs, int32_t K,
                     ssc_stream_t stream);

/* What one ssc_replay_append call takes; start is the pair's cursor (replay_start).  K is already reduced to the steps to
 * store and the log pointers advanced past the steps to skip (DeviceReplayBuffer.append_chunk's last_steps). */
struct ssc_replay_append_item {
    ssc_replay_ring    ring;
    ssc_transition_log log;
    int32_t            K;
    int64_t            n;
    float              reward_scale;
};
typedef struct ssc_replay_append_item ssc_replay_append_item;

/* ssc_replay_append for n_pairs rings in one launch (replaces one call per pair): record positions are exactly
 * (start + k * n + e) % capacity.  obs_dim is one value for the population and the episode index (ep_steps / ep_run) is
 * kept for all rings or for none (SSC_EINVAL naming the pair); every item passes ssc_replay_append's checks and no ring
 * array is shared by two pairs (SSC_EINVAL naming both).  Nothing to append anywhere: SSC_OK without a launch. */
int ssc_replay_append_many(const ssc_replay_append_item *h_items, const ssc_replay_append_item *d_items,
                           const ssc_pair_cursor *h_cursors, const ssc_pair_cursor *d_cursors, int32_t n_pairs,
                           ssc_stream_t stream);

/* One ssc_decay_schedule call's arguments by value (factor / floor are part of the item). */
struct ssc_decay_item {
    const double *d_finished;
    double        finished0, per_generation;
    int32_t       n_sched;   /* 0..4 */
    double        factor[4], floor[4];
    double       *d_state;   /* [1 + n_sched] */
    float        *d_out[4];  /* each may be NULL */
};
typedef struct ssc_decay_item ssc_decay_item;

/* ssc_decay_schedule for n_pairs schedule sets in one launch, one thread each (replaces one call per pair).  Nothing in
 * an item changes from chunk to chunk: no cursor.  No d_state shared by two pairs. */
int ssc_decay_schedule_many(const ssc_decay_item *h_items, const ssc_decay_item *d_items, int32_t n_pairs, ssc_stream_t stream);

/* What one ssc_obs_rms_update call takes, with the pair's own workspace. */
struct ssc_obs_rms_item {
    ssc_transition_log log;
    int32_t            k0, K;
    int64_t            n;
    double            *d_rms;
    void              *d_workspace;
    size_t             workspace_bytes; /* >= ssc_obs_rms_update_workspace_bytes(obs_dim) */
};
typedef struct ssc_obs_rms_item ssc_obs_rms_item;

/* ssc_obs_rms_update for n_pairs blocks in two launches (replaces two per pair): every pair's rows are partitioned exactly
 * as its own call partitions them (the partition is derived from (n, K - k0) alone) and summed in the same order, so every
 * bit of every block is that of the single call.  No statistics block or workspace shared by two pairs. */
int ssc_obs_rms_update_many(int32_t obs_dim, const ssc_obs_rms_item *h_items, const ssc_obs_rms_item *d_items, int32_t n_pairs,
                            ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Adaptive parameter-space noise (ddpg_editted.py:47-60, 151-166, 255-259, 360-385)
 * -------------------------------------------------------------------------------------
 * A perturbed actor is a second flat parameter array [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3] that the
 * forward and rollout kernels read through an ordinary ssc_actor_desc.
 *
 * ssc_param_noise_perturb: d_dst[i] = d_src[i] + *d_stddev * g_i for the n elements outside the two skip ranges
 * [skipX_begin, skipX_end) (the LayerNorm beta / gamma segments, models_editted.py:18-19: perturbable_vars; an empty
 * range is begin == end), a bit copy inside them and everywhere when *d_stddev == 0.  The stream depends on the flat
 * index alone: ONE Philox(seed; q, generation, TAG_PARAM_NOISE = 9) evaluation serves elements 4q .. 4q+3 -- words
 * (0, 1) are one Box-Muller pair (cos -> 4q, sin -> 4q+1), words (2, 3) the pair of (4q+2, 4q+3).  generation < 2^56.
 * stddev is read from device memory when the kernel runs; d_src == d_dst is allowed; n == 0 launches nothing.
 *
 * ssc_param_noise_adapt: *d_distance = sqrt(mean((a - b)^2)) over count = batch * act_dim elements (ddpg_editted.py:166;
 * one workgroup, f64 accumulation in a fixed order), then AdaptiveParamNoiseSpec.adapt of baselines 0.1.5 on the device
 * value: *d_stddev /= coefficient if distance > desired, else *d_stddev *= coefficient (fp32; a tie multiplies).
 * 1 <= count <= 4096 * SSC_MAX_ACT, coefficient > 1.  a and b come from two ssc_actor_forward[_rms] calls.
 *
 * ssc_param_noise_cycle: one adaption interval in ONE launch (one workgroup).  Equal to, in this order,
 *   ssc_param_noise_perturb(d_src -> adaptive copy, generation_adaptive)      with the stddev in *d_stddev,
 *   a = actor(obs), b = adaptive_actor(obs)                                   obs [m][obs_dim], 1 <= m <= 4096,
 *   ssc_param_noise_adapt(a, b) -> *d_distance, *d_stddev,
 *   ssc_param_noise_perturb(d_src -> d_dst, generation_acting)                with the NEW stddev,
 * where the adaptive copy lives in LDS only and never reaches HBM.  `actor` describes the PLAIN actor: its parameter
 * pointers must lie inside d_src[0 .. n) (the copy is addressed by the same offsets); both forwards run in fp32 with
 * every unit summed in index order, whatever `precision` says, with or without LayerNorm.  d_rms: as in
 * ssc_actor_forward_rms (NULL: none).  The distance is an f64 sum in a fixed order (no atomics): the same bits run to
 * run.  *d_stddev and d_dst carry the bits of the four-call sequence whenever both agree on which side of `desired` the
 * distance lies; the distance itself agrees to the rounding of the fp32 forwards.  SSC_EINVAL for m, n or coefficient out
 * of range and for d_dst == d_src; SSC_EUNSUPPORTED, with the byte count in ssc_last_error(), when the adaptive copy plus
 * the working space of a 4-row tile exceed the 160 KB of LDS (a 200-100 actor fits, a 400-300 one does not). */
int ssc_param_noise_perturb(int64_t n, const float *d_src, float *d_dst, const float *d_stddev, int64_t skip0_begin,
                            int64_t skip0_end, int64_t skip1_begin, int64_t skip1_end, uint64_t seed, uint64_t generation,
                            ssc_stream_t stream);
int ssc_param_noise_adapt(int64_t count, const float *d_a, const float *d_b, float desired, float coefficient,
                          float *d_stddev, float *d_distance, ssc_stream_t stream);
int ssc_param_noise_cycle(const ssc_actor_desc *actor, int64_t m, const float *d_obs, const double *d_rms, int64_t n,
                          const float *d_src, int64_t skip0_begin, int64_t skip0_end, int64_t skip1_begin, int64_t skip1_end,
                          uint64_t seed, uint64_t generation_adaptive, uint64_t generation_acting, float desired,
                          float coefficient, float *d_stddev, float *d_distance, float *d_dst, ssc_stream_t stream);

/* What one ssc_param_noise_cycle call takes, minus the generations and m (the pair's ssc_param_noise_cursor), with the batch
 * given as row indices into the replay ring's state column.  Declared tag first like the other *_many items;
 * tests/test_param_noise_many_host.py holds both structs' sizes and offsets to the ctypes mirrors. */
struct ssc_param_noise_many_item {
    ssc_actor_desc actor;            /* the PLAIN actor; pointers inside d_src[0..n) */
    const float   *d_obs;            /* the ring's state column base, [rows][obs_dim] */
    const int32_t *d_idx;            /* [m] row indices into d_obs, or NULL: rows 0..m-1 (d_obs holds the batch itself) */
    const double  *d_rms;            /* or NULL, per pair */
    int64_t        n;                /* 0: the pair is skipped */
    const float   *d_src;
    int64_t        skip0_begin, skip0_end, skip1_begin, skip1_end;
    uint64_t       seed;
    float          desired, coefficient;
    float         *d_stddev, *d_distance, *d_dst;
};
typedef struct ssc_param_noise_many_item ssc_param_noise_many_item;

/* What changes with every adaption interval, 24 bytes per pair: the one upload of a steady-state call. */
struct ssc_param_noise_cursor {
    uint64_t generation_adaptive, generation_acting;
    int32_t  m;                      /* 1..4096 batch rows, or 0: perturb only */
    int32_t  pad;
};
typedef struct ssc_param_noise_cursor ssc_param_noise_cursor;

/* ssc_param_noise_cycle for n_pairs agents in ONE launch: workgroup p runs pair p's whole adaption
 * interval exactly as the pair's own launch would -- workgroups share nothing, there are no atomics -- so d_dst, *d_stddev
 * and *d_distance hold, bit for bit, what
 *     ssc_param_noise_cycle(&actor, m, <rows d_idx[0..m) of d_obs>, d_rms, n, d_src, skips, seed, generation_adaptive,
 *                           generation_acting, desired, coefficient, d_stddev, d_distance, d_dst)
 * leaves.  Row r of the batch is d_obs[d_idx[r] * obs_dim + c]: the gather out of the replay ring happens inside the kernel
 * (d_idx == NULL: row r itself).  The caller keeps every d_idx[r] inside the rows of d_obs.
 * m == 0 (the ring holds no batch yet) is the perturb-only interval: d_dst = d_src + *d_stddev * g(generation_acting) with
 * the stddev as it stands -- the bits of ssc_param_noise_perturb(n, d_src, d_dst, d_stddev, skips, seed,
 * generation_acting); *d_stddev and *d_distance are not written, d_obs / d_idx / d_rms not read, generation_adaptive unused.
 * The conventions are ssc_rollout_many's: host arrays (items and cursors) that are validated before any HIP call, the
 * caller's device copies of the same bytes, complete on `stream` before the call; the library copies nothing; the pair's
 * index -- or both indices -- is in ssc_last_error().
 * Per pair, read at run time: layer sizes (64-32, 128-64 and 200-100 agents may share a launch), LayerNorm, last_layer_tanh,
 * obs_clip, d_rms (set or NULL), obs_dim, m, seed, desired, coefficient.  Uniform per launch: the plain parameters are
 * staged in LDS beside the adaptive copy iff EVERY pair with m > 0 fits both copies beside a 128-row tile (the bits do not
 * depend on it: a pair's tile, and with it every summation order, is the same either way); the dynamic LDS size is the
 * largest pair's.
 * Every pair with n > 0 passes ssc_param_noise_cycle's checks with its error codes (m may be 0 as well; SSC_EUNSUPPORTED
 * with the byte count and the pair when the adaptive copy and a 4-row tile exceed LDS, whatever m is).  Across pairs,
 * SSC_EINVAL naming both: no two d_dst ranges [d_dst, d_dst + n) overlap, no d_dst range overlaps any pair's d_src range
 * (its own included), no two pairs share d_stddev or d_distance.  d_src, d_obs, d_idx and d_rms are only read and may be
 * shared.  n_pairs 1..65535 (more: SSC_EUNSUPPORTED).  A pair with n == 0 is skipped, nothing else of its item is read; all
 * n == 0: SSC_OK without a launch. */
int ssc_param_noise_cycle_many(const ssc_param_noise_many_item *h_items, const ssc_param_noise_many_item *d_items,
                               const ssc_param_noise_cursor *h_cursors, const ssc_param_noise_cursor *d_cursors,
                               int32_t n_pairs, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Training diagnostics (ddpg_editted.py:219-253 setup_stats, 341-358 get_stats; printed per epoch by
 * training_editted.py:144)
 * -------------------------------------------------------------------------------------
 * ssc_ddpg_stats: the stats_ops of DDPG_editted on a fixed sample of m transitions (obs [m][obs_dim], act [m][act_dim],
 * 1 <= m <= 4096) into d_out[SSC_DDPG_N_STATS] (f64, device), in the reference's stats_names order:
 *   0 obs_rms_mean   1 obs_rms_std             mean over the dimensions of the fp32 mean / std the networks use (d_rms)
 *   2 reference_Q_mean   3 reference_Q_std                           Q(obs, act)
 *   4 reference_actor_Q_mean   5 reference_actor_Q_std               Q(obs, actor(obs))
 *   6 reference_action_mean   7 reference_action_std                 actor(obs), all m * act_dim elements
 *   8 reference_perturbed_action_mean   9 reference_perturbed_action_std   perturbed(obs), likewise
 *   10 param_noise_stddev                                            *d_param_noise_stddev, read when the kernel runs
 * mean and population std sqrt(mean((x - mean)^2)) (baselines' reduce_std).  Slots that do not apply are NaN: 0-1 with
 * d_rms == NULL, 8-9 with perturbed == NULL, 10 with d_param_noise_stddev == NULL.  Observations enter the networks as in
 * ssc_actor_forward_rms / ssc_critic_forward_rms (each descriptor's own obs_clip; normalised when d_rms is given); all
 * forward passes run in fp32 with every unit summed in index order, whatever `precision` says, with or without LayerNorm.
 * The batch is tiled over workgroups of 16 rows; each leaves (count, mean, M2) per statistic in the workspace -- M2 from a
 * second sweep around the tile mean, never sum(x^2) / n - mean^2 -- and a second small launch merges them in workgroup
 * order with Chan's formula, all in f64, no atomics: the same bits run to run.  No host read; stream-ordered.
 * SSC_EINVAL for NULL descriptors / sample / output, m out of range, actor / critic / perturbed shapes that disagree, or a
 * workspace below ssc_ddpg_stats_workspace_bytes(m) (0 for m out of range) -- all checked before any HIP call;
 * SSC_EUNSUPPORTED, with the byte count in ssc_last_error(), when a 16-row tile's activations exceed the 160 KB of LDS
 * (roughly max(actor h1, critic h1) + max(actor h2, critic h2) > 2500 units). */
#define SSC_DDPG_N_STATS 11
size_t ssc_ddpg_stats_workspace_bytes(int64_t m);
int ssc_ddpg_stats(const ssc_actor_desc *actor, const ssc_critic_desc *critic, const ssc_actor_desc *perturbed, int64_t m,
                   const float *d_obs, const float *d_act, const double *d_rms, const float *d_param_noise_stddev,
                   double *d_out, void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Evaluation rollouts (training_editted.py:122-138, reported :160-164 as eval/return, eval/Q, eval/episodes)
 * -------------------------------------------------------------------------------------
 * ssc_ddpg_eval_rollout: K steps of the reference's evaluation loop for n independent eval envs in ONE fused launch (plus
 * a small merge launch).  Per step, with o the observation of the env's state:
 *   x = clip(o), or clip((o - mean) / std) when d_rms is given -- formed as ssc_actor_forward_rms / ssc_critic_forward_rms
 *       form it, each descriptor's own obs_clip;
 *   a_raw = actor(x);  Q = critic(x, a_raw)          critic_with_actor_tf (ddpg_editted.py:130-131, 262): Q of the RAW output
 *   executed action = scale(scale(clip(a_raw, -1, 1)))   DDPG_Baselines_agent.get_action with the noise off (act_low / act_high)
 *   env.step, TimeLimit, the running episode return in fp32 in step order, auto-reset with
 *   Philox(seed; env_id, step0 + k, TAG_RESET)      as ssc_rollout: chunks compose, the id space shards
 * No noise of any kind: state->ou_x is neither read nor written and may be NULL.  s0, s1, steps and ep_ret are written
 * back.  zero_returns != 0 starts every env's running return at 0 for this launch while the episode itself goes on (the
 * reference zeroes eval_episode_reward and keeps eval_obs, training_editted.py:125); 0 carries state->ep_ret.
 * All forward arithmetic is fp32 with every unit summed in index order by fused multiply-adds -- the arithmetic of
 * ssc_ddpg_stats (critic hidden tanh: tanhf, actor: the fast one); `precision` is ignored, LayerNorm and last_layer_tanh
 * are honoured.  act_dim is 1.
 * d_out[SSC_DDPG_N_EVAL] (f64, device), every slot written by every call:
 *   0 eval/episodes            episodes finished in this launch
 *   1 eval/return   2 its population std    over those episodes; NaN if none (np.mean([]))
 *   3 eval/Q        4 its population std    over all n * K steps
 *   5 env-steps = n * K        6 goal terminations        7 mean length of the finished episodes; NaN if none
 * log (may be NULL): the usual [K][n] transition columns, with the EXECUTED action.  d_q (may be NULL): Q as [K][n], the
 * reference's eval_qs.
 * Reduction: every env keeps (count, mean, M2) of its Q stream, of its finished-episode returns and of their lengths in
 * f64 registers (Welford); a workgroup of 16 envs merges them in env order with Chan's formula into the workspace, and a
 * second small launch merges the workgroups in workgroup order.  No atomics; the grid depends on n alone: the same bits
 * run to run.  The weights are staged in LDS once per launch when both networks and a tile's activations fit its 160 KB
 * (64-32, 128-64), read from global memory otherwise (200-100); the summation order, and the bits, are the same.
 * SSC_EINVAL for NULL params / descriptors / state / output / workspace, n < 1 or K < 1, actor / critic / env obs_dim that
 * disagree, critic->act_dim != actor->act_dim, or a workspace below ssc_ddpg_eval_workspace_bytes(n) -- all checked
 * before any HIP call; SSC_EUNSUPPORTED for act_dim != 1, and, with the byte count in ssc_last_error(), when a tile's
 * activations alone exceed LDS. */
#define SSC_DDPG_N_EVAL 8
size_t ssc_ddpg_eval_workspace_bytes(int64_t n);
int ssc_ddpg_eval_rollout(const ssc_env_params *p, const ssc_actor_desc *actor, const ssc_critic_desc *critic,
                          float act_low, float act_high, int64_t n, int32_t K, const ssc_rollout_state *state,
                          const double *d_rms, const ssc_transition_log *log, float *d_q, int32_t zero_returns,
                          double *d_out, void *d_workspace, size_t workspace_bytes,
                          uint64_t seed, uint64_t env_id0, uint64_t step0, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Evaluation and diagnostics of a whole population, one launch per phase
 * -------------------------------------------------------------------------------------
 * The conventions are ssc_rollout_many's: a host item array that is validated before any HIP call, the caller's device
 * copy of the same bytes (complete on `stream` before the call) that the kernels read, nothing copied by the library, the
 * pair's index -- or both indices -- in ssc_last_error().  Workgroups of different pairs share nothing and there are no
 * atomics: every d_out block, state column and workspace holds, bit for bit, what the pair's own single call leaves.
 * tests/test_ddpg_monitor_many_host.py holds the structs' sizes and offsets to the ctypes mirrors. */

/* What one ssc_ddpg_eval_rollout call takes, minus step0 (the pair's ssc_pair_cursor; replay_start is ignored), K and
 * zero_returns (one value per call), the transition log and d_q (the many-form writes neither: the single call stays for
 * traces). */
struct ssc_ddpg_eval_many_item {
    ssc_env_params    params;
    ssc_actor_desc    actor;
    ssc_critic_desc   critic;
    float             act_low, act_high;
    int64_t           n;               /* >= 1, per pair */
    ssc_rollout_state state;           /* ou_x is not used */
    const double     *d_rms;           /* normalize_observations block or NULL, per pair */
    double           *d_out;           /* [SSC_DDPG_N_EVAL] */
    void             *d_workspace;
    size_t            workspace_bytes; /* >= ssc_ddpg_eval_workspace_bytes(n) */
    uint64_t          seed, env_id0;
};
typedef struct ssc_ddpg_eval_many_item ssc_ddpg_eval_many_item;

/* ssc_ddpg_eval_rollout for n_pairs (eval-env set, agent) pairs in one fused launch plus one merge launch.  Grid row p
 * runs pair p's workgroups (grid x = the largest pair's workgroup count; a smaller pair's surplus workgroups leave at once,
 * before any barrier); the merge launch has one workgroup per pair.
 * Uniform over the population: the env kind (SSC_EINVAL naming the first pair that differs from pair 0).  Per pair, read at
 * run time: the layer sizes of both networks (the kernel is shape-generic: 64-32, 128-64 and 200-100 agents may share a
 * launch), LayerNorm, last_layer_tanh, obs_clip, d_rms (set or NULL), env constants, action bounds, n, seed, env_id0.
 * The weights are staged in LDS iff EVERY pair's networks fit beside its activations (and SSC_DDPG_EVAL_GLOBAL_WEIGHTS is
 * not set); the bits do not depend on it.  The launch's dynamic LDS size is the largest pair's.
 * Every item passes ssc_ddpg_eval_rollout's checks with its error codes (SSC_EUNSUPPORTED for act_dim != 1 or a tile
 * beyond LDS).  No two pairs share a state column, a d_out block or a workspace (SSC_EINVAL naming both); weights may be
 * shared -- they are only read, so one agent evaluated on two env sets is legal.  n_pairs 1..65535.
 * K == 0: SSC_OK without a launch (the validation-only call the wrappers use). */
int ssc_ddpg_eval_rollout_many(const ssc_ddpg_eval_many_item *h_items, const ssc_ddpg_eval_many_item *d_items,
                               const ssc_pair_cursor *h_cursors, const ssc_pair_cursor *d_cursors, int32_t n_pairs, int32_t K,
                               int32_t zero_returns, ssc_stream_t stream);

/* The arguments of one ssc_ddpg_stats call. */
struct ssc_ddpg_stats_many_item {
    ssc_actor_desc  actor;
    ssc_critic_desc critic;
    ssc_actor_desc  perturbed;            /* read when has_perturbed */
    int32_t         has_perturbed;        /* per pair; 0: slots 8-9 are NaN */
    int64_t         m;                    /* 0..4096, per pair; 0: the pair is skipped */
    const float    *d_obs, *d_act;
    const double   *d_rms;                /* or NULL, per pair */
    const float    *d_param_noise_stddev; /* or NULL, per pair */
    double         *d_out;                /* [SSC_DDPG_N_STATS] */
    void           *d_workspace;
    size_t          workspace_bytes;      /* >= ssc_ddpg_stats_workspace_bytes(m) */
};
typedef struct ssc_ddpg_stats_many_item ssc_ddpg_stats_many_item;

/* ssc_ddpg_stats for n_pairs agents in two launches (replaces two per agent): grid row p of the first runs pair p's row
 * tiles, workgroup p of the second merges them.  Everything is per pair: shapes, LayerNorm, d_rms, the perturbed copy, m.
 * A pair with m == 0 is skipped -- no workgroup works for it, its d_out is left untouched and nothing else of its item is
 * read (a pair that has no sample yet); all m == 0: SSC_OK without a launch.  Every other item passes ssc_ddpg_stats's
 * checks with its error codes.  No two pairs with m > 0 share a d_out block or a workspace (SSC_EINVAL naming both). */
int ssc_ddpg_stats_many(const ssc_ddpg_stats_many_item *h_items, const ssc_ddpg_stats_many_item *d_items, int32_t n_pairs,
                        ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Dynamics-model training step
 * ------------------------------------------------------------------------------------- */

/* One iteration of Dyn_Model.train's inner loop (NN_Dynamics_Model/dynamics_model.py:98-101 /
 * :111-113): mse = mean((z - net(x))^2) over the batch (:41), tf.train.AdamOptimizer(lr) step
 * (:44-50) [third-party TF 1.5: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * theta -= lr sqrt(1-b2^t)/(1-b1^t) m / (sqrt(v) + 1e-8)].  The batch is rows d_idx[0..B) of the
 * (already normalised) device data sets d_X [n][in], d_Z [n][out] -- the old/new mixing of :60-96 is
 * index arithmetic done by the caller.  Weights and Adam moments are updated in place. */
typedef struct ssc_mlp_train_desc {
    int32_t n_layers;
    int32_t dims[SSC_MAX_LAYERS + 1];
    float *W[SSC_MAX_LAYERS], *b[SSC_MAX_LAYERS];      /* device, updated in place */
    float *mW[SSC_MAX_LAYERS], *vW[SSC_MAX_LAYERS];    /* device Adam moments, zero-initialised */
    float *mb[SSC_MAX_LAYERS], *vb[SSC_MAX_LAYERS];
    int32_t *adam_t;                                    /* device [1] step counter */
    float lr, beta1, beta2, epsilon;
} ssc_mlp_train_desc;

size_t ssc_mlp_train_workspace_bytes(const ssc_mlp_train_desc *net, int32_t batch);
/* n_steps consecutive iterations enqueued by one call: step k trains on rows d_idx[k*batch .. (k+1)*batch) and
 * writes its batch MSE (before the update) to d_loss[k] (d_loss may be NULL).  One hidden layer of <= 512 units
 * (in <= 12, out <= 8 -- the shapes the reference ships) runs ONE fused launch per step; other shapes run the
 * generic chain of per-layer launches. */
int ssc_mlp_train_steps(const ssc_mlp_train_desc *net, const float *d_X, const float *d_Z, const int32_t *d_idx,
                        int32_t batch, int32_t n_steps, float *d_loss, void *d_workspace, size_t workspace_bytes,
                        ssc_stream_t stream);
/* = ssc_mlp_train_steps with n_steps = 1. */
int ssc_mlp_train_step(const ssc_mlp_train_desc *net, const float *d_X, const float *d_Z, const int32_t *d_idx,
                       int32_t batch, float *d_loss, void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);

/* The arguments of one ssc_mlp_train_steps call.  Declared tag first like the other *_many items;
 * tests/test_mlp_train_many_host.py holds the struct's size and offsets to the ctypes mirror. */
struct ssc_mlp_train_many_item {
    ssc_mlp_train_desc net;
    const float   *d_X, *d_Z;      /* per model; read only, may be shared between models */
    const int32_t *d_idx;          /* [n_steps][batch]; read only, may be shared */
    int32_t        batch, n_steps; /* per model; n_steps == 0: the model is skipped, nothing else of its item is read */
    float         *d_loss;         /* [n_steps] or NULL, per model */
    void          *d_workspace;
    size_t         workspace_bytes;/* >= ssc_mlp_train_workspace_bytes(&net, batch) */
};
typedef struct ssc_mlp_train_many_item ssc_mlp_train_many_item;

/* ssc_mlp_train_steps for n_models independent models (the dynamics models of a sweep's seeds) in one begin launch plus
 * max_p n_steps_p step launches, where per-model calls take sum_p (n_steps_p + 1).  Grid row p of a
 * step launch runs model p's ceil(batch_p / 32) workgroups (grid x = the largest model's count; surplus workgroups, and
 * all workgroups of a model whose steps are done, leave at once, before any barrier); the last workgroup of a model
 * sums that model's partials and applies Adam.  Workgroups of different models share nothing: after the call every
 * model's parameters, moments, adam_t, losses and workspace hold, bit for bit, what its own ssc_mlp_train_steps call with
 * the item's arguments leaves -- ONE call: the bias-correction powers are recomputed at the start of a call and advanced by
 * multiplication inside it, so two many-calls equal two single calls per model, not one longer one.
 * The conventions are ssc_rollout_many's: the host array is validated completely before any HIP call, the caller's device
 * copy of the same bytes must be complete on `stream`, the library copies nothing, model indices appear in
 * ssc_last_error().
 * Uniform over a call: the kernel instantiation the model's own call dispatches (in <= 3 and out <= 2 | in <= 4 and
 * out <= 3 | the rest); SSC_EINVAL names the first model that differs from the first trained one.  Per model, read at run
 * time: hidden width, in, out, batch, n_steps, lr and the Adam constants, d_loss set or NULL.
 * A model the one-launch step does not cover (n_layers != 2, hidden > 512, in > 12, out > 8, or SSC_DYN_TRAIN_GENERIC set)
 * is SSC_EUNSUPPORTED naming it; every other item passes ssc_mlp_train_steps's checks with its codes.
 * What a model's workgroups write -- every layer's W, b, mW, vW, mb, vb, adam_t, d_loss[n_steps], the workspace -- may,
 * among the models with n_steps > 0, overlap no other written range and no model's d_X, d_Z (taken as their first row:
 * the row count is the caller's) or d_idx: SSC_EINVAL naming both models.  What is only read may coincide.
 * n_models 1..65535.  Every n_steps == 0: SSC_OK without a launch (the validation-only call the wrappers use). */
int ssc_mlp_train_steps_many(const ssc_mlp_train_many_item *h_items, const ssc_mlp_train_many_item *d_items,
                             int32_t n_models, ssc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Random-rollout data collection -> dynamics-model training set (SURVEY.md section 8a row A17 and the
 * data format either side of it): CollectSamples.collect_samples / do_rollout
 * (NN_Dynamics_Model/collect_samples_threaded.py:25-111), generate_training_data_inputs / _outputs
 * (NN_Dynamics_Model/data_manipulation.py:58-88), the z-score statistics of NND_MB_agent.py:302-319 and
 * helper_funcs.add_noise (NN_Dynamics_Model/helper_funcs.py:10-17).
 * ------------------------------------------------------------------------------------- */

/* A "rollout" is one env's FIRST episode segment of the chunk `log` ([K][n] SoA columns written by
 * ssc_rollout from freshly reset envs): it stops after its first terminal step like do_rollout (:89-93).
 * d_len [n]  = number of steps of rollout i (first done inclusive, else K);
 * d_off [n+1] = exclusive prefix sum of max(d_len - 1, 0): the first data-set row of rollout i, d_off[n] the
 * total -- every rollout loses its last entry (data_manipulation.py:66-74). */
size_t ssc_dataset_scan_workspace_bytes(int64_t n);
int ssc_dataset_scan(const ssc_transition_log *log, int32_t K, int64_t n, int32_t *d_len, int64_t *d_off,
                     void *d_workspace, size_t workspace_bytes, ssc_stream_t stream);

/* Row-major data set, rollout after rollout like np.concatenate over the list of rollouts (:77-78, :87):
 * d_X [rows][obs_dim] = s_i, d_Y [rows][1] = a_i, d_Z [rows][obs_dim] = s_{i+1} - s_i (fp32 subtraction).
 * Rows >= capacity_rows are not written; n * (K - 1) rows always suffice. */
int ssc_dataset_build(const ssc_transition_log *log, int32_t obs_dim, int32_t K, int64_t n, const int32_t *d_len,
                      const int64_t *d_off, int64_t capacity_rows, float *d_X, float *d_Y, float *d_Z,
                      ssc_stream_t stream);

/* HOST function (no GPU work): path_shortcutter (smartstart/utilities/numerical.py:226-246) with the elliptical distance of
 * :116-124 -- every pair of states (i, j >= i + 2) of path[n][d] within theta of each other is a candidate shortcut, the
 * weighted interval scheduling of :189-222 (weight j - i - 1 per interval after the first, later intervals win ties) picks
 * the non-overlapping set that deletes the most interior states.  keep[i] = 1 for the states that stay, *n_kept their count
 * (may be NULL).  fp64, the reference's expression order: decisions identical to the numpy implementation. */
int ssc_path_shortcut(const double *path, int32_t n, int32_t d, const double *radii, double theta, uint8_t *keep,
                      int32_t *n_kept);

/* mean_c = mean(x[:, c]); std_c = sqrt(mean((x[:, c] - mean_c)^2)) (NND_MB_agent.py:302-304: np.mean, then
 * np.std of the centred column), accumulated in f64 in a fixed order (bit-reproducible).  rows >= 1,
 * cols <= 64. */
size_t ssc_column_stats_workspace_bytes(int32_t cols);
int ssc_column_stats(const float *d_x, int64_t rows, int32_t cols, double *d_mean, double *d_std, void *d_workspace,
                     size_t workspace_bytes, ssc_stream_t stream);

/* d_out[r][out_col0 + c] = np.nan_to_num((x[r][c] - mean_c) / std_c) (NND_MB_agent.py:305,310,315), evaluated
 * in f64 and rounded to fp32; d_out has out_stride columns -- so dataX and dataY land side by side in the
 * network-input matrix of :318 (np.concatenate((dataX, dataY), axis=1)). */
int ssc_zscore(const float *d_x, int64_t rows, int32_t cols, const double *d_mean, const double *d_std, float *d_out,
               int32_t out_stride, int32_t out_col0, ssc_stream_t stream);

/* The same for the whole network-input matrix of :318 in one pass: d_out[r] = [zscore(x[r]) | zscore(y[r])], rows of
 * cols_x + cols_y floats -- np.concatenate((dataX, dataY), axis=1) of the two z-scored matrices (NND_MB_agent.py:303-318).
 * Bit-identical to two ssc_zscore calls into the same matrix; every output line is written whole. */
int ssc_zscore_concat(const float *d_x, int32_t cols_x, const double *d_mean_x, const double *d_std_x, const float *d_y,
                      int32_t cols_y, const double *d_mean_y, const double *d_std_y, int64_t rows, float *d_out,
                      ssc_stream_t stream);

/* helper_funcs.add_noise: x[r][c] += N(0, |mean_c * noise_to_signal|) in the columns where
 * mean_c * noise_to_signal > 0 (only those, :14).  One Philox(seed; r, stream_id << 8 | (c >> 2), TAG_DATA_NOISE = 6)
 * evaluation serves four columns: word pair (x, y) for c & 3 in {0, 1}, (z, w) for {2, 3}; the cos output of the pair's
 * Box-Muller transform for the even column, the sin output for the odd one; oracle: add_noise_keyed. */
int ssc_add_noise(float *d_x, int64_t rows, int32_t cols, const double *d_mean, double noise_to_signal, uint64_t seed,
                  uint64_t stream_id, ssc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SSC_H */
