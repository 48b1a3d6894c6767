// ddpg_eval.hip -- the evaluation rollouts of the reference's training loop (DDPG_Baselines_editted/training_editted.py:
// 122-138: the actor WITHOUT noise on a separate eval_env, the critic asked for Q at every step; reported :160-164 as
// eval/return, eval/Q, eval/episodes) for n independent eval envs, K steps, in ONE fused launch plus a small merge launch:
// no transition log, no Q buffer, no episode ring and no host read are needed to get the numbers.
//
//   * ddpg_eval_kernel: the tiling of ddpg_stats_rows_kernel -- 16 envs per 256-thread workgroup, thread t serves env
//     t & 15 and the units t >> 4, t >> 4 + 16, ... of a layer, activations in LDS as [unit][16 envs], every unit summed in
//     index order by fused multiply-adds (net_rows, ddpg_rows.h: the bits of actor_generic_kernel / critic_kernel).  Lanes
//     0-15 own the env state across the K steps: observe -> clip / normalise -> [all threads: actor, critic on the RAW actor
//     output] -> scale(scale(clip(a))) -> env.step, TimeLimit, fp32 return, auto-reset -- the step of rollout_kernel
//     (rollout.hip) with the noise off.  They also keep (count, mean, M2) of the env's Q stream, of its finished-episode
//     returns and of their lengths in f64 registers (Welford, one update per step / episode).
//     The weights do not change over the K steps: when both networks and the activations fit the 160 KB of LDS they are
//     copied there once per launch (WLDS); otherwise they are read from global memory (L2).  Same code, same summation
//     order: the bits do not depend on which path ran.
//     A workgroup merges its envs in env order with Chan's formula into the workspace.
//   * ddpg_eval_merge_kernel: one wave per stream merges the workgroup partials -- every lane its contiguous share in
//     workgroup order, then a fixed tree over the lanes -- and one thread writes the block.
// No atomics, no ticket; the grid depends on n alone, so the block is the same bits run to run.
#include <stdlib.h>

#include "ddpg_rows.h"
#include "ssc_device.h"
#include "ssc_host.h"

namespace ssc {

int validate_mc_params(const ssc_env_params *p, const char *who);  // env_step.hip

namespace {

constexpr int kEStreams = 3;                   // Q | finished-episode return | finished-episode length
constexpr int kEPart = 3 * kEStreams + 1;      // doubles per env / workgroup record: three (count, mean, M2), the goal count
constexpr size_t kLdsBytes = 160 * 1024;

// the envs as rollout_kernel steps them (rollout.hip: McEnv / PendEnv over the shared device functions of ssc_device.h)
struct McEnv {
    using Const = McConst;
    static constexpr int OBS = 2;
    float pos, vel;
    __device__ void load(float a, float b) { pos = a; vel = b; }
    __device__ void observe(float (&o)[OBS]) const { o[0] = pos; o[1] = vel; }
    __device__ void step(const Const &c, float a, float &rew, bool &goal) { mc_step_one(c, pos, vel, a, rew, goal); }
    __device__ void reset(const Const &c, const u32x4 &w) { mc_reset_one(c, w, pos, vel); }
    __device__ float s0() const { return pos; }
    __device__ float s1() const { return vel; }
};

struct PendEnv {
    using Const = PendConst;
    static constexpr int OBS = 3;
    float th, thdot;
    __device__ void load(float a, float b) { th = a; thdot = b; }
    __device__ void observe(float (&o)[OBS]) const { pend_observe_one(th, thdot, o[0], o[1], o[2]); }
    __device__ void step(const Const &c, float a, float &rew, bool &goal) {
        pend_step_one(c, th, thdot, a, rew);
        goal = false;
    }
    __device__ void reset(const Const &, const u32x4 &w) { pend_reset_one(w, th, thdot); }
    __device__ float s0() const { return th; }
    __device__ float s1() const { return thdot; }
};

struct EvalArgs {
    StatsNet actor, critic;                    // device (global) pointers
    int32_t off_RED, off_XA, off_XC, off_H1, off_H2, off_PI, off_Q, off_AW, off_CW;   // LDS float offsets
    int64_t n;
    int32_t K;
    ssc_rollout_state st;
    ssc_transition_log log;
    int32_t has_log, zero_returns;
    float *q;                                  // [K][n] or null
    const double *rms;                         // null: no normalize_observations
    float act_low, act_high;
    uint64_t seed, env_id0, step0;
    double *part;                              // [n_blocks][kEPart]
};

// floats of a network's LDS image: W1 | b1 | W2 | b2 | W3 | b3 | (gamma1 | beta1 | gamma2 | beta2)
int64_t net_floats(int in_dim, int n_extra, int h1, int h2, int out_dim, bool ln) {
    return (int64_t)in_dim * h1 + h1 + ((int64_t)h1 + n_extra) * h2 + h2 + (int64_t)h2 * out_dim + out_dim + (ln ? 2 * ((int64_t)h1 + h2) : 0);
}

// block-cooperative copy of a network into LDS (layout of net_floats); the caller's next barrier publishes it
__device__ StatsNet stage_net(const StatsNet &g, float *img, int in_dim, int n_extra, int out_dim, int tid) {
    StatsNet l = g;
    float *p = img;
    auto put = [&](const float *src, int count) {
        for (int e = tid; e < count; e += kSThreads) p[e] = src[e];
        const float *at = p;
        p += count;
        return at;
    };
    l.W1 = put(g.W1, in_dim * g.h1);
    l.b1 = put(g.b1, g.h1);
    l.W2 = put(g.W2, (g.h1 + n_extra) * g.h2);
    l.b2 = put(g.b2, g.h2);
    l.W3 = put(g.W3, g.h2 * out_dim);
    l.b3 = put(g.b3, out_dim);
    if (g.ln1_g != nullptr) {
        l.ln1_g = put(g.ln1_g, g.h1);
        l.ln1_b = put(g.ln1_b, g.h1);
        l.ln2_g = put(g.ln2_g, g.h2);
        l.ln2_b = put(g.ln2_b, g.h2);
    }
    return l;
}

// Welford (1962): one more value into (count, mean, M2)
__device__ __forceinline__ void welford(Moments &m, double x) {
    m.n += 1.0;
    const double d = x - m.mean;
    m.mean += d / m.n;
    m.m2 = fma(d, x - m.mean, m.m2);
}

template <class EnvT, bool WLDS>
__global__ __launch_bounds__(kSThreads) void ddpg_eval_kernel(typename EnvT::Const ec, EvalArgs a) {
    constexpr int OBS = EnvT::OBS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    StatsNet actor = a.actor, critic = a.critic;
    if constexpr (WLDS) {   // published by the barrier in front of the first forward pass
        actor = stage_net(a.actor, lds + a.off_AW, OBS, 0, 1, tid);
        critic = stage_net(a.critic, lds + a.off_CW, OBS, 1, 1, tid);
    }
    float *xa = lds + a.off_XA, *xc = lds + a.off_XC, *h1s = lds + a.off_H1, *h2s = lds + a.off_H2;
    float *pi = lds + a.off_PI, *qv = lds + a.off_Q;

    // ---- lanes 0-15: the env of this lane; envs past n shadow env n - 1, write nothing and stay out of the reduction ----
    const int64_t env0 = (int64_t)blockIdx.x * kSR;
    const bool owner = tid < kSR;
    const bool active = owner && env0 + tid < a.n;
    const int64_t i = min(env0 + (tid & (kSR - 1)), a.n - 1);
    const uint64_t env_id = a.env_id0 + (uint64_t)i;
    const bool norm = a.rms != nullptr;
    const bool identity_scale = a.act_low == -1.0f && a.act_high == 1.0f;
    auto scale = [&](float v) {   // DDPG_Baselines_agent.py:236-240, as ActorPolicy::scale (rollout.hip)
        v = fminf(fmaxf(v, -1.0f), 1.0f);
        return identity_scale ? v : fmaf((v + 1.0f) * 0.5f, a.act_high - a.act_low, a.act_low);
    };
    EnvT env;
    ObsNorm<OBS> nrm;
    float obs[OBS];
    int32_t el = 0;
    float ep_ret = 0.0f;
    Moments mq{0.0, 0.0, 0.0}, mr{0.0, 0.0, 0.0}, ml{0.0, 0.0, 0.0};
    double goals = 0.0;
    if (owner) {
        env.load(a.st.s0[i], a.st.s1[i]);
        el = a.st.steps[i];
        ep_ret = a.zero_returns ? 0.0f : a.st.ep_ret[i];   // training_editted.py:125 zeroes the return and keeps eval_obs
        if (norm) nrm.load(a.rms, OBS);
        env.observe(obs);
    }

    for (int32_t k = 0; k < a.K; ++k) {
        if (owner) {   // the network inputs, formed as the *_rms forward kernels form them (each descriptor's own clip)
#pragma unroll
            for (int c = 0; c < OBS; ++c) {
                xa[c * kSR + tid] = norm ? nrm.apply(obs[c], c, actor.obs_clip) : clip_obs(obs[c], actor.obs_clip);
                xc[c * kSR + tid] = norm ? nrm.apply(obs[c], c, critic.obs_clip) : clip_obs(obs[c], critic.obs_clip);
            }
        }
        __syncthreads();
        net_rows<false>(actor, xa, OBS, nullptr, 0, 1, true, h1s, h2s, pi, tid);
        net_rows<true>(critic, xc, OBS, pi, 1, 1, false, h1s, h2s, qv, tid);   // Q of the RAW actor output (ddpg_editted.py:130-131)
        if (owner) {
            const float q = qv[tid];
            // get_action with the noise off: clip (ddpg_editted.py:271), scale twice (DDPG_Baselines_agent.py:232-240)
            const float act = scale(scale(fminf(fmaxf(pi[tid], -1.0f), 1.0f)));
            float rew, obs2[OBS];
            bool goal;
            env.step(ec, act, rew, goal);
            env.observe(obs2);
            el += 1;
            const bool done = goal | ((ec.max_episode_steps > 0) & (el >= ec.max_episode_steps));
            ep_ret += rew;
            if (active) {
                if (a.has_log) {
                    const int64_t lr = (int64_t)k * a.log.row_stride + i, ld = (int64_t)k * a.log.done_row_stride + i;
#pragma unroll
                    for (int c = 0; c < OBS; ++c) {
                        a.log.obs[c][lr] = obs[c];
                        a.log.obs2[c][lr] = obs2[c];
                    }
                    a.log.act[lr] = act;
                    a.log.rew[lr] = rew;
                    a.log.done[ld] = done ? 1 : 0;
                }
                if (a.q != nullptr) a.q[(int64_t)k * a.n + i] = q;
            }
            welford(mq, (double)q);
#pragma unroll
            for (int c = 0; c < OBS; ++c) obs[c] = obs2[c];
            if (done) {
                welford(mr, (double)ep_ret);
                welford(ml, (double)el);
                goals += goal ? 1.0 : 0.0;
                env.reset(ec, rng_words(a.seed, env_id, a.step0 + (uint64_t)k, TAG_RESET));
                el = 0;
                ep_ret = 0.0f;
                env.observe(obs);
            }
        }
    }

    if (active) {
        a.st.s0[i] = env.s0();
        a.st.s1[i] = env.s1();
        a.st.steps[i] = el;
        a.st.ep_ret[i] = ep_ret;
    }
    // ---- the workgroup's envs in env order (Chan) -> its record in the workspace ----
    double *red = reinterpret_cast<double *>(lds + a.off_RED);   // [16 envs][kEPart]
    if (owner) {
        double *r = red + tid * kEPart;
        r[0] = mq.n; r[1] = mq.mean; r[2] = mq.m2;
        r[3] = mr.n; r[4] = mr.mean; r[5] = mr.m2;
        r[6] = ml.n; r[7] = ml.mean; r[8] = ml.m2;
        r[9] = goals;
    }
    __syncthreads();
    const int rows = (int)min((int64_t)kSR, a.n - env0);
    double *out = a.part + (size_t)blockIdx.x * kEPart;
    if (tid < kEStreams) {
        Moments acc{0.0, 0.0, 0.0};
        for (int r = 0; r < rows; ++r) {
            const double *p = red + r * kEPart + 3 * tid;
            acc = chan_merge(acc, Moments{p[0], p[1], p[2]});
        }
        out[3 * tid] = acc.n;
        out[3 * tid + 1] = acc.mean;
        out[3 * tid + 2] = acc.m2;
    } else if (tid == kEStreams) {
        double g = 0.0;
        for (int r = 0; r < rows; ++r) g += red[r * kEPart + 9];   // small integers: exact
        out[9] = g;
    }
}

__global__ __launch_bounds__((kEStreams + 1) * 64) void ddpg_eval_merge_kernel(const double *__restrict__ part, int32_t n_blocks,
                                                                                double *__restrict__ out) {
    const int s = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double nan = __builtin_nan("");
    const int per = (n_blocks + 63) / 64;
    const int b0 = min(lane * per, n_blocks), b1 = min(b0 + per, n_blocks);
    if (s < kEStreams) {   // wave-uniform
        Moments acc{0.0, 0.0, 0.0};
        for (int b = b0; b < b1; ++b) {
            const double *p = part + (size_t)b * kEPart + 3 * s;
            acc = chan_merge(acc, Moments{p[0], p[1], p[2]});
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {   // lane l takes lanes l + off: a fixed tree, lane 0 holds the stream
            const Moments o{__shfl_down(acc.n, off), __shfl_down(acc.mean, off), __shfl_down(acc.m2, off)};
            if (lane + off < 64) acc = chan_merge(acc, o);
        }
        if (lane == 0) {
            const bool any = acc.n > 0.0;
            const double mean = any ? acc.mean : nan, std = any ? sqrt(acc.m2 / acc.n) : nan;   // np.mean([]) is NaN
            if (s == 0) {          // eval/Q over all steps; the step count
                out[3] = mean;
                out[4] = std;
                out[5] = acc.n;
            } else if (s == 1) {   // eval/episodes, eval/return
                out[0] = acc.n;
                out[1] = mean;
                out[2] = std;
            } else {               // mean episode length
                out[7] = mean;
            }
        }
    } else {
        double g = 0.0;
        for (int b = b0; b < b1; ++b) g += part[(size_t)b * kEPart + 9];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) g += __shfl_down(g, off);   // integers: exact in any order
        if (lane == 0) out[6] = g;
    }
}

int eval_blocks(int64_t n) { return (int)((n + kSR - 1) / kSR); }

constexpr int64_t kEMaxEnvs = (int64_t)1 << 30;   // as ssc_rollout

template <class EnvT>
int launch_eval(const typename EnvT::Const &ec, const EvalArgs &a, bool wlds, size_t lds, hipStream_t s) {
    const void *fn = wlds ? reinterpret_cast<const void *>(ddpg_eval_kernel<EnvT, true>)
                          : reinterpret_cast<const void *>(ddpg_eval_kernel<EnvT, false>);
    if (lds > 64 * 1024) {
        int rc = check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute(ddpg_eval_kernel)");
        if (rc) return rc;
    }
    const int nb = eval_blocks(a.n);
    if (wlds)
        hipLaunchKernelGGL((ddpg_eval_kernel<EnvT, true>), dim3(nb), dim3(kSThreads), lds, s, ec, a);
    else
        hipLaunchKernelGGL((ddpg_eval_kernel<EnvT, false>), dim3(nb), dim3(kSThreads), lds, s, ec, a);
    return SSC_OK;
}

}  // namespace

}  // namespace ssc

using namespace ssc;

static_assert(SSC_DDPG_N_EVAL == 8, "episodes, return mean / std, Q mean / std, steps, goals, episode length");

extern "C" {

size_t ssc_ddpg_eval_workspace_bytes(int64_t n) {
    if (n < 1 || n > kEMaxEnvs) return 0;
    return (size_t)eval_blocks(n) * kEPart * sizeof(double);
}

int ssc_ddpg_eval_rollout(const ssc_env_params *p, const ssc_actor_desc *actor, const ssc_critic_desc *critic,
                          float act_low, float act_high, int64_t n, int32_t K, const ssc_rollout_state *state,
                          const double *d_rms, const ssc_transition_log *log, float *d_q, int32_t zero_returns,
                          double *d_out, void *d_workspace, size_t workspace_bytes,
                          uint64_t seed, uint64_t env_id0, uint64_t step0, ssc_stream_t stream) {
    SSC_REQUIRE(p != nullptr && actor != nullptr && critic != nullptr && state != nullptr,
                "ssc_ddpg_eval_rollout: NULL params / actor / critic / state");
    SSC_REQUIRE(d_out != nullptr, "ssc_ddpg_eval_rollout: output block NULL");
    SSC_REQUIRE(n >= 1 && n <= kEMaxEnvs && K >= 1, "ssc_ddpg_eval_rollout: n = %lld (1..2^30), K = %d (>= 1)", (long long)n, K);
    SSC_REQUIRE(p->kind == SSC_ENV_MOUNTAINCAR || p->kind == SSC_ENV_PENDULUM, "ssc_ddpg_eval_rollout: unknown env kind %d", p->kind);
    const int od = p->kind == SSC_ENV_MOUNTAINCAR ? 2 : 3;
    SSC_REQUIRE(actor->obs_dim == od && critic->obs_dim == od,
                "ssc_ddpg_eval_rollout: actor obs_dim %d / critic obs_dim %d, the env observes %d values", actor->obs_dim,
                critic->obs_dim, od);
    SSC_REQUIRE(critic->act_dim == actor->act_dim, "ssc_ddpg_eval_rollout: the critic's act_dim %d differs from the actor's %d",
                critic->act_dim, actor->act_dim);
    if (actor->act_dim != 1) return set_error(SSC_EUNSUPPORTED, "ssc_ddpg_eval_rollout: act_dim %d (only 1)", actor->act_dim);
    SSC_REQUIRE(actor->h1 >= 1 && actor->h2 >= 1 && critic->h1 >= 1 && critic->h2 >= 1, "ssc_ddpg_eval_rollout: bad hidden sizes");
    SSC_REQUIRE(act_low <= act_high, "ssc_ddpg_eval_rollout: act_low > act_high");
    SSC_REQUIRE(state->s0 && state->s1 && state->steps && state->ep_ret, "ssc_ddpg_eval_rollout: NULL state column");
    EvalArgs a{};
    SSC_REQUIRE(fill_net(a.actor, actor->W1, actor->b1, actor->W2, actor->b2, actor->W3, actor->b3, actor->ln1_g, actor->ln1_b,
                         actor->ln2_g, actor->ln2_b, actor->h1, actor->h2, actor->last_layer_tanh, actor->obs_clip),
                "ssc_ddpg_eval_rollout: actor: NULL device pointer, or LayerNorm pointers that do not come together");
    SSC_REQUIRE(fill_net(a.critic, critic->W1, critic->b1, critic->W2, critic->b2, critic->W3, critic->b3, critic->ln1_g,
                         critic->ln1_b, critic->ln2_g, critic->ln2_b, critic->h1, critic->h2, critic->last_layer_tanh,
                         critic->obs_clip),
                "ssc_ddpg_eval_rollout: critic: NULL device pointer, or LayerNorm pointers that do not come together");
    a.n = n; a.K = K; a.st = *state; a.q = d_q; a.rms = d_rms; a.zero_returns = zero_returns != 0;
    a.act_low = act_low; a.act_high = act_high; a.seed = seed; a.env_id0 = env_id0; a.step0 = step0;
    a.has_log = log != nullptr;
    if (log != nullptr) {
        a.log = *log;
        for (int c = 0; c < od; ++c)
            SSC_REQUIRE(log->obs[c] && log->obs2[c], "ssc_ddpg_eval_rollout: NULL log obs column %d", c);
        SSC_REQUIRE(log->act && log->rew && log->done, "ssc_ddpg_eval_rollout: NULL log column");
        SSC_REQUIRE(log->row_stride >= 0 && log->done_row_stride >= 0, "ssc_ddpg_eval_rollout: negative row stride");
        if (a.log.row_stride == 0) a.log.row_stride = n;
        if (a.log.done_row_stride == 0) a.log.done_row_stride = n;
        SSC_REQUIRE(a.log.row_stride >= n && a.log.done_row_stride >= n, "ssc_ddpg_eval_rollout: row stride < n");
    }
    const size_t need = ssc_ddpg_eval_workspace_bytes(n);
    SSC_REQUIRE(d_workspace != nullptr && workspace_bytes >= need,
                "ssc_ddpg_eval_rollout: workspace %zu < %zu bytes (ssc_ddpg_eval_workspace_bytes)", workspace_bytes, need);
    a.part = static_cast<double *>(d_workspace);
    if (p->kind == SSC_ENV_MOUNTAINCAR)
        if (int rc = validate_mc_params(p, "ssc_ddpg_eval_rollout")) return rc;
    // ---- LDS carve: the partial records (f64, at offset 0), rows of 16 floats ([unit][env]), then the weight images ----
    int64_t q = 0;
    auto take = [&](int64_t floats) { const int64_t at = q; q += floats; return (int32_t)at; };
    a.off_RED = take((int64_t)kSR * kEPart * 2);
    a.off_XA = take((int64_t)od * kSR); a.off_XC = take((int64_t)od * kSR);
    a.off_H1 = take((actor->h1 > (int64_t)critic->h1 + 1 ? actor->h1 : (int64_t)critic->h1 + 1) * kSR);
    a.off_H2 = take((int64_t)(actor->h2 > critic->h2 ? actor->h2 : critic->h2) * kSR);
    a.off_PI = take(kSR); a.off_Q = take(kSR);
    const size_t lds_act = (size_t)q * sizeof(float);
    if (lds_act > kLdsBytes)
        return set_error(SSC_EUNSUPPORTED, "ssc_ddpg_eval_rollout: these layer sizes need %zu B of LDS per workgroup (160 KB available)",
                         lds_act);
    const int64_t wa = net_floats(od, 0, actor->h1, actor->h2, 1, actor->ln1_g != nullptr);
    const int64_t wc = net_floats(od, 1, critic->h1, critic->h2, 1, critic->ln1_g != nullptr);
    // SSC_DDPG_EVAL_GLOBAL_WEIGHTS (any value, read per call): A/B switch for the tests and tools -- the weights stay in
    // global memory whatever their size
    const bool wlds = lds_act + (size_t)(wa + wc) * sizeof(float) <= kLdsBytes && getenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS") == nullptr;
    if (wlds) {
        a.off_AW = take(wa);
        a.off_CW = take(wc);
    }
    const size_t lds = (size_t)q * sizeof(float);
    hipStream_t s = as_stream(stream);
    int rc = p->kind == SSC_ENV_MOUNTAINCAR ? launch_eval<McEnv>(make_mc_const(*p), a, wlds, lds, s)
                                            : launch_eval<PendEnv>(make_pend_const(*p), a, wlds, lds, s);
    if (rc) return rc;
    hipLaunchKernelGGL(ddpg_eval_merge_kernel, dim3(1), dim3((kEStreams + 1) * 64), 0, s, a.part, eval_blocks(n), d_out);
    return check_launch("ssc_ddpg_eval_rollout");
}

}  // extern "C"
