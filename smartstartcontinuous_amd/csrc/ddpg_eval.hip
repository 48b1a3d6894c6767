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
//
// A population of (eval-env set, agent) pairs (ssc_ddpg_eval_rollout_many): both kernel bodies are device functions; the
// *_many kernels run them for the pair of their grid row, with the arguments the single call would have put into the
// kernarg formed from the pair's item by the SAME host-and-device functions (fill_net, eval_carve, pack_eval).  Workgroups
// of different pairs share nothing, so every pair's bits are those of its own launch.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

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
    static SSC_HD Const make_const(const ssc_env_params &p) { return make_mc_const(p); }
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
    static SSC_HD Const make_const(const ssc_env_params &p) { return make_pend_const(p); }
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

// LDS carve of one workgroup, in floats: the partial records (f64, at offset 0), rows of 16 floats ([unit][env]), then --
// wlds -- the weight images
struct EvalCarve {
    int32_t off_RED, off_XA, off_XC, off_H1, off_H2, off_PI, off_Q, off_AW, off_CW;
    int64_t act_floats;                        // the activations alone
    int64_t weight_floats;                     // both images
    int64_t floats;                            // what the launch needs: act_floats (+ weight_floats when wlds)
};

struct EvalArgs {
    StatsNet actor, critic;                    // device (global) pointers
    EvalCarve lds;
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
SSC_HD int64_t net_floats(int in_dim, int n_extra, int h1, int h2, int out_dim, bool ln) {
    return (int64_t)in_dim * h1 + h1 + ((int64_t)h1 + n_extra) * h2 + h2 + (int64_t)h2 * out_dim + out_dim + (ln ? 2 * ((int64_t)h1 + h2) : 0);
}

// ONE function of (obs_dim, layer sizes, LayerNorm, wlds) for the host (launch size, the WLDS decision) and for a workgroup
// of the population launch, which carves for its own pair: the two cannot disagree.
SSC_HD EvalCarve eval_carve(int od, int ah1, int ah2, bool aln, int ch1, int ch2, bool cln, bool wlds) {
    EvalCarve c{};
    int64_t q = 0;
    c.off_RED = (int32_t)q; q += (int64_t)kSR * kEPart * 2;
    c.off_XA = (int32_t)q;  q += (int64_t)od * kSR;
    c.off_XC = (int32_t)q;  q += (int64_t)od * kSR;
    c.off_H1 = (int32_t)q;  q += (ah1 > (int64_t)ch1 + 1 ? ah1 : (int64_t)ch1 + 1) * kSR;
    c.off_H2 = (int32_t)q;  q += (int64_t)(ah2 > ch2 ? ah2 : ch2) * kSR;
    c.off_PI = (int32_t)q;  q += kSR;
    c.off_Q = (int32_t)q;   q += kSR;
    c.act_floats = q;
    const int64_t wa = net_floats(od, 0, ah1, ah2, 1, aln), wc = net_floats(od, 1, ch1, ch2, 1, cln);
    c.weight_floats = wa + wc;
    if (wlds) {
        c.off_AW = (int32_t)q; q += wa;
        c.off_CW = (int32_t)q; q += wc;
    }
    c.floats = q;
    return c;
}

SSC_HD int eval_blocks(int64_t n) { return (int)((n + kSR - 1) / kSR); }

// The kernel arguments of one (eval-env set, agent): no log, no Q buffer (ssc_ddpg_eval_rollout adds its own).  The host
// packs them into the kernarg of the single launch, a workgroup of the population launch from its pair's item.
SSC_HD void pack_eval(EvalArgs &a, const ssc_actor_desc &actor, const ssc_critic_desc &critic, float act_low, float act_high,
                      int64_t n, int32_t K, const ssc_rollout_state &st, const double *rms, int32_t zero_returns, double *part,
                      uint64_t seed, uint64_t env_id0, uint64_t step0, bool wlds) {
    fill_net(a.actor, actor.W1, actor.b1, actor.W2, actor.b2, actor.W3, actor.b3, actor.ln1_g, actor.ln1_b, actor.ln2_g, actor.ln2_b,
             actor.h1, actor.h2, actor.last_layer_tanh, actor.obs_clip);
    fill_net(a.critic, critic.W1, critic.b1, critic.W2, critic.b2, critic.W3, critic.b3, critic.ln1_g, critic.ln1_b, critic.ln2_g,
             critic.ln2_b, critic.h1, critic.h2, critic.last_layer_tanh, critic.obs_clip);
    a.lds = eval_carve(actor.obs_dim, actor.h1, actor.h2, actor.ln1_g != nullptr, critic.h1, critic.h2, critic.ln1_g != nullptr, wlds);
    a.n = n; a.K = K; a.st = st; a.has_log = 0; a.zero_returns = zero_returns != 0; a.q = nullptr; a.rms = rms;
    a.act_low = act_low; a.act_high = act_high; a.seed = seed; a.env_id0 = env_id0; a.step0 = step0;
    a.part = part;
}

// block-cooperative copy of a network into LDS (layout of net_floats); the caller's next barrier publishes it
__device__ StatsNet stage_net(const StatsNet &g, float *img, int in_dim, int n_extra, int out_dim, int tid) {
    StatsNet l = g;
    float *p = img;
    auto put = [&](const float *src, int count) {   // (the source is global memory: no FLAT loads out of a population item)
        const SSC_GLOBAL float *gsrc = (const SSC_GLOBAL float *)src;
        for (int e = tid; e < count; e += kSThreads) p[e] = gsrc[e];
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

// The whole launch of one (eval-env set, agent): workgroup blockIdx.x of ITS grid row.  Shared by ddpg_eval_kernel (the
// arguments are its kernarg) and ddpg_eval_many_kernel (the arguments are formed from the pair's item); by value, as
// rollout_body takes its arguments (rollout.hip).
// Without WLDS the weights are read through address-space-1 pointers: out of the kernarg the compiler proves that itself,
// out of a population item it cannot, and every weight load of the K-step loop would be a FLAT instruction.
template <class EnvT, bool WLDS>
__device__ __forceinline__ void eval_body(const typename EnvT::Const ec, const EvalArgs a) {
    constexpr int OBS = EnvT::OBS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    using Net = std::conditional_t<WLDS, StatsNet, GlobalNet>;
    Net actor, critic;
    if constexpr (WLDS) {   // published by the barrier in front of the first forward pass
        actor = stage_net(a.actor, lds + a.lds.off_AW, OBS, 0, 1, tid);
        critic = stage_net(a.critic, lds + a.lds.off_CW, OBS, 1, 1, tid);
    } else {
        actor = global_net(a.actor);
        critic = global_net(a.critic);
    }
    float *xa = lds + a.lds.off_XA, *xc = lds + a.lds.off_XC, *h1s = lds + a.lds.off_H1, *h2s = lds + a.lds.off_H2;
    float *pi = lds + a.lds.off_PI, *qv = lds + a.lds.off_Q;

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
    double *red = reinterpret_cast<double *>(lds + a.lds.off_RED);   // [16 envs][kEPart]
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

template <class EnvT, bool WLDS>
__global__ __launch_bounds__(kSThreads) void ddpg_eval_kernel(typename EnvT::Const ec, EvalArgs a) {
    eval_body<EnvT, WLDS>(ec, a);
}

// A population in one launch (ssc_ddpg_eval_rollout_many): blockIdx.y is the pair.  Its item and cursor sit at
// workgroup-uniform addresses (scalar loads); a workgroup beyond its pair's block count leaves as a whole, before any
// barrier.  WLDS is one value per launch (every pair's weights fit, or none is staged); everything else -- layer sizes,
// LayerNorm, last_layer_tanh, d_rms, the LDS carve -- is the pair's own, read at run time as in the single launch.
// Pointers read out of the item are generic to the compiler: the state loads / stores around the step loop are FLAT
// instructions here; inside the loop nothing but LDS is touched with WLDS, and the weight loads go through global_net
// without it.
template <class EnvT, bool WLDS>
__global__ __launch_bounds__(kSThreads) void ddpg_eval_many_kernel(const ssc_ddpg_eval_many_item *__restrict__ items,
                                                                   const ssc_pair_cursor *__restrict__ cursors, int32_t K,
                                                                   int32_t zero_returns) {
    const ssc_ddpg_eval_many_item &it = items[blockIdx.y];
    if ((int64_t)blockIdx.x * kSR >= it.n) return;
    EvalArgs a;
    pack_eval(a, it.actor, it.critic, it.act_low, it.act_high, it.n, K, it.state, it.d_rms, zero_returns,
              static_cast<double *>(it.d_workspace), it.seed, it.env_id0, cursors[blockIdx.y].step0, WLDS);
    eval_body<EnvT, WLDS>(EnvT::make_const(it.params), a);
}

__device__ __forceinline__ void eval_merge_body(const double *__restrict__ part, int32_t n_blocks, double *__restrict__ out) {
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

__global__ __launch_bounds__((kEStreams + 1) * 64) void ddpg_eval_merge_kernel(const double *__restrict__ part, int32_t n_blocks,
                                                                                double *__restrict__ out) {
    eval_merge_body(part, n_blocks, out);
}

// workgroup p merges pair p's partials exactly as the pair's own merge launch
__global__ __launch_bounds__((kEStreams + 1) * 64) void ddpg_eval_merge_many_kernel(const ssc_ddpg_eval_many_item *__restrict__ items) {
    const ssc_ddpg_eval_many_item &it = items[blockIdx.x];
    eval_merge_body(static_cast<const double *>(it.d_workspace), eval_blocks(it.n), it.d_out);
}

constexpr int64_t kEMaxEnvs = (int64_t)1 << 30;   // as ssc_rollout

int raise_lds(const void *fn, size_t lds, const char *what) {
    if (lds <= 64 * 1024) return SSC_OK;
    return check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), what);
}

template <class EnvT>
int launch_eval(const typename EnvT::Const &ec, const EvalArgs &a, bool wlds, size_t lds, hipStream_t s) {
    const void *fn = wlds ? reinterpret_cast<const void *>(ddpg_eval_kernel<EnvT, true>)
                          : reinterpret_cast<const void *>(ddpg_eval_kernel<EnvT, false>);
    if (int rc = raise_lds(fn, lds, "hipFuncSetAttribute(ddpg_eval_kernel)")) return rc;
    const int nb = eval_blocks(a.n);
    if (wlds)
        hipLaunchKernelGGL((ddpg_eval_kernel<EnvT, true>), dim3(nb), dim3(kSThreads), lds, s, ec, a);
    else
        hipLaunchKernelGGL((ddpg_eval_kernel<EnvT, false>), dim3(nb), dim3(kSThreads), lds, s, ec, a);
    return SSC_OK;
}

template <class EnvT>
int launch_eval_many(const ssc_ddpg_eval_many_item *d_items, const ssc_pair_cursor *d_cursors, int32_t n_pairs, int32_t K,
                     int32_t zero_returns, int64_t n_max, bool wlds, size_t lds, hipStream_t s) {
    const void *fn = wlds ? reinterpret_cast<const void *>(ddpg_eval_many_kernel<EnvT, true>)
                          : reinterpret_cast<const void *>(ddpg_eval_many_kernel<EnvT, false>);
    if (int rc = raise_lds(fn, lds, "hipFuncSetAttribute(ddpg_eval_many_kernel)")) return rc;
    const dim3 grid((unsigned)eval_blocks(n_max), (unsigned)n_pairs);
    if (wlds)
        hipLaunchKernelGGL((ddpg_eval_many_kernel<EnvT, true>), grid, dim3(kSThreads), lds, s, d_items, d_cursors, K, zero_returns);
    else
        hipLaunchKernelGGL((ddpg_eval_many_kernel<EnvT, false>), grid, dim3(kSThreads), lds, s, d_items, d_cursors, K, zero_returns);
    hipLaunchKernelGGL(ddpg_eval_merge_many_kernel, dim3((unsigned)n_pairs), dim3((kEStreams + 1) * 64), 0, s, d_items);
    return check_launch("ssc_ddpg_eval_rollout_many");
}

// The checks of one (eval-env set, agent) -- the single call's, and through `who` an item's of the population call; `log`
// is the single call's.  *carve: the pair's carve without the weight images.
int eval_check(const char *who, const ssc_env_params *p, const ssc_actor_desc *actor, const ssc_critic_desc *critic, float act_low,
               float act_high, int64_t n, int32_t K, int32_t k_min, const ssc_rollout_state *state, const ssc_transition_log *log,
               const double *d_out, const void *d_workspace, size_t workspace_bytes, EvalCarve *carve) {
    SSC_REQUIRE(d_out != nullptr, "%s: output block NULL", who);
    SSC_REQUIRE(n >= 1 && n <= kEMaxEnvs && K >= k_min, "%s: n = %lld (1..2^30), K = %d (>= %d)", who, (long long)n, K, k_min);
    SSC_REQUIRE(p->kind == SSC_ENV_MOUNTAINCAR || p->kind == SSC_ENV_PENDULUM, "%s: unknown env kind %d", who, p->kind);
    const int od = p->kind == SSC_ENV_MOUNTAINCAR ? 2 : 3;
    SSC_REQUIRE(actor->obs_dim == od && critic->obs_dim == od, "%s: actor obs_dim %d / critic obs_dim %d, the env observes %d values", who,
                actor->obs_dim, critic->obs_dim, od);
    SSC_REQUIRE(critic->act_dim == actor->act_dim, "%s: the critic's act_dim %d differs from the actor's %d", who, critic->act_dim,
                actor->act_dim);
    if (actor->act_dim != 1) return set_error(SSC_EUNSUPPORTED, "%s: act_dim %d (only 1)", who, actor->act_dim);
    SSC_REQUIRE(actor->h1 >= 1 && actor->h2 >= 1 && critic->h1 >= 1 && critic->h2 >= 1, "%s: bad hidden sizes", who);
    SSC_REQUIRE(act_low <= act_high, "%s: act_low > act_high", who);
    SSC_REQUIRE(state->s0 && state->s1 && state->steps && state->ep_ret, "%s: NULL state column", who);
    StatsNet net;
    SSC_REQUIRE(fill_net(net, actor->W1, actor->b1, actor->W2, actor->b2, actor->W3, actor->b3, actor->ln1_g, actor->ln1_b,
                         actor->ln2_g, actor->ln2_b, actor->h1, actor->h2, actor->last_layer_tanh, actor->obs_clip),
                "%s: actor: NULL device pointer, or LayerNorm pointers that do not come together", who);
    SSC_REQUIRE(fill_net(net, critic->W1, critic->b1, critic->W2, critic->b2, critic->W3, critic->b3, critic->ln1_g,
                         critic->ln1_b, critic->ln2_g, critic->ln2_b, critic->h1, critic->h2, critic->last_layer_tanh,
                         critic->obs_clip),
                "%s: critic: NULL device pointer, or LayerNorm pointers that do not come together", who);
    if (log != nullptr) {
        for (int c = 0; c < od; ++c) SSC_REQUIRE(log->obs[c] && log->obs2[c], "%s: NULL log obs column %d", who, c);
        SSC_REQUIRE(log->act && log->rew && log->done, "%s: NULL log column", who);
        SSC_REQUIRE(log->row_stride >= 0 && log->done_row_stride >= 0, "%s: negative row stride", who);
        SSC_REQUIRE((log->row_stride == 0 || log->row_stride >= n) && (log->done_row_stride == 0 || log->done_row_stride >= n),
                    "%s: row stride < n", who);
    }
    const size_t need = ssc_ddpg_eval_workspace_bytes(n);
    SSC_REQUIRE(d_workspace != nullptr && workspace_bytes >= need, "%s: workspace %zu < %zu bytes (ssc_ddpg_eval_workspace_bytes)", who,
                workspace_bytes, need);
    if (p->kind == SSC_ENV_MOUNTAINCAR)
        if (int rc = validate_mc_params(p, who)) return rc;
    *carve = eval_carve(od, actor->h1, actor->h2, actor->ln1_g != nullptr, critic->h1, critic->h2, critic->ln1_g != nullptr, false);
    const size_t lds_act = (size_t)carve->act_floats * sizeof(float);
    if (lds_act > kLdsBytes)
        return set_error(SSC_EUNSUPPORTED, "%s: these layer sizes need %zu B of LDS per workgroup (160 KB available)", who, lds_act);
    return SSC_OK;
}

// do both weight images fit beside the activations?
bool weights_fit(const EvalCarve &c) { return (size_t)(c.act_floats + c.weight_floats) * sizeof(float) <= kLdsBytes; }

// SSC_DDPG_EVAL_GLOBAL_WEIGHTS (any value, read per call): A/B switch for the tests and tools -- the weights stay in
// global memory whatever their size
bool global_weights_forced() { return getenv("SSC_DDPG_EVAL_GLOBAL_WEIGHTS") != nullptr; }

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
    EvalCarve carve;
    if (int rc = eval_check("ssc_ddpg_eval_rollout", p, actor, critic, act_low, act_high, n, K, 1, state, log, d_out, d_workspace,
                            workspace_bytes, &carve))
        return rc;
    const bool wlds = weights_fit(carve) && !global_weights_forced();
    EvalArgs a{};
    pack_eval(a, *actor, *critic, act_low, act_high, n, K, *state, d_rms, zero_returns, static_cast<double *>(d_workspace), seed,
              env_id0, step0, wlds);
    a.q = d_q;
    a.has_log = log != nullptr;
    if (log != nullptr) {
        a.log = *log;
        if (a.log.row_stride == 0) a.log.row_stride = n;
        if (a.log.done_row_stride == 0) a.log.done_row_stride = n;
    }
    const size_t lds = (size_t)a.lds.floats * sizeof(float);
    hipStream_t s = as_stream(stream);
    int rc = p->kind == SSC_ENV_MOUNTAINCAR ? launch_eval<McEnv>(make_mc_const(*p), a, wlds, lds, s)
                                            : launch_eval<PendEnv>(make_pend_const(*p), a, wlds, lds, s);
    if (rc) return rc;
    hipLaunchKernelGGL(ddpg_eval_merge_kernel, dim3(1), dim3((kEStreams + 1) * 64), 0, s, a.part, eval_blocks(n), d_out);
    return check_launch("ssc_ddpg_eval_rollout");
}

int ssc_ddpg_eval_rollout_many(const ssc_ddpg_eval_many_item *h_items, const ssc_ddpg_eval_many_item *d_items,
                               const ssc_pair_cursor *h_cursors, const ssc_pair_cursor *d_cursors, int32_t n_pairs, int32_t K,
                               int32_t zero_returns, ssc_stream_t stream) {
    SSC_REQUIRE(n_pairs >= 1, "ssc_ddpg_eval_rollout_many: n_pairs %d < 1", n_pairs);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_ddpg_eval_rollout_many: NULL item array");
    SSC_REQUIRE(h_cursors != nullptr && d_cursors != nullptr, "ssc_ddpg_eval_rollout_many: NULL cursor array");
    if (n_pairs > 65535) return set_error(SSC_EUNSUPPORTED, "ssc_ddpg_eval_rollout_many: %d pairs > 65535 (one grid row each)", n_pairs);
    const int kind0 = h_items[0].params.kind;
    bool wlds = !global_weights_forced();
    int64_t n_max = 0, act_max = 0, all_max = 0;
    std::vector<std::pair<const void *, int>> owned;   // (array, pair) of everything a pair's workgroups write
    owned.reserve((size_t)n_pairs * 6);
    for (int p = 0; p < n_pairs; ++p) {
        const ssc_ddpg_eval_many_item &it = h_items[p];
        char who[56];
        snprintf(who, sizeof who, "ssc_ddpg_eval_rollout_many: pair %d", p);
        EvalCarve carve;
        if (int rc = eval_check(who, &it.params, &it.actor, &it.critic, it.act_low, it.act_high, it.n, K, 0, &it.state, nullptr, it.d_out,
                                it.d_workspace, it.workspace_bytes, &carve))
            return rc;
        SSC_REQUIRE(it.params.kind == kind0, "%s: env kind %d differs from pair 0's %d (one kernel instantiation per launch)", who,
                    it.params.kind, kind0);
        wlds = wlds && weights_fit(carve);
        n_max = std::max(n_max, it.n);
        act_max = std::max(act_max, carve.act_floats);
        all_max = std::max(all_max, carve.act_floats + carve.weight_floats);
        for (const void *q : {(const void *)it.state.s0, (const void *)it.state.s1, (const void *)it.state.steps,
                              (const void *)it.state.ep_ret, (const void *)it.d_out, (const void *)it.d_workspace})
            owned.emplace_back(q, p);
    }
    // two pairs on one array would race without a sign of it; weights are only read and may be shared
    std::sort(owned.begin(), owned.end());
    for (size_t k = 1; k < owned.size(); ++k)
        SSC_REQUIRE(owned[k].first != owned[k - 1].first || owned[k].second == owned[k - 1].second,
                    "ssc_ddpg_eval_rollout_many: pairs %d and %d share a state column, an output block or a workspace",
                    owned[k - 1].second, owned[k].second);
    if (K == 0) return SSC_OK;
    // the launch's dynamic LDS: the largest pair's carve (each workgroup carves for its own pair inside it)
    const size_t lds = (size_t)(wlds ? all_max : act_max) * sizeof(float);
    hipStream_t s = as_stream(stream);
    if (kind0 == SSC_ENV_MOUNTAINCAR) return launch_eval_many<McEnv>(d_items, d_cursors, n_pairs, K, zero_returns, n_max, wlds, lds, s);
    return launch_eval_many<PendEnv>(d_items, d_cursors, n_pairs, K, zero_returns, n_max, wlds, lds, s);
}

}  // extern "C"
