// ddpg_stats.hip -- the training diagnostics of DDPG_editted (setup_stats / get_stats,
// DDPG_Baselines_editted/ddpg_editted.py:219-253, 341-358; printed every epoch by training_editted.py:144) on a fixed
// sample of m transitions: mean and std of Q(s, a), of Q(s, pi(s)), of pi(s), of the perturbed actor's actions, the mean
// over the dimensions of the running observation mean / std, and the parameter-noise stddev -- into ONE f64 device block,
// with no host read anywhere (the vectorised loops log it chunk by chunk and copy the log out once).
//
// Two launches, both in a fixed order (no atomics, no ticket), the discipline of obs_rms.hip:
//   * ddpg_stats_rows_kernel: the batch is tiled over workgroups, 16 rows each (as ddpg_wide_grad_kernel tiles it).  A
//     workgroup runs the three or four forward passes of its rows in fp32 -- thread t serves row t & 15 and the units
//     t >> 4, t >> 4 + 16, ... of a layer, activations in LDS as [unit][16 rows] -- with every unit summed in index order
//     by fused multiply-adds: the arithmetic (and the bits) of actor_generic_kernel / actor_row_kernel (actor.hip) and of
//     critic_kernel (smartstart.hip), through the same clip_obs / ObsNorm / layer_norm_stats / tanh_fast.  It then reduces
//     each of the four value streams of its rows to (count, mean, M2) in f64: the sum in index order, M2 from a SECOND
//     sweep over the values (they sit in LDS) -- never sum(x^2) / n - mean^2, which loses a spread of 1e-3 around Q = 100.
//   * ddpg_stats_merge_kernel: one wave per stream merges the workgroup partials with Chan's formula -- every lane its
//     contiguous share in workgroup order, then a fixed tree over the lanes -- and writes mean and sqrt(M2 / count)
//     (population std, baselines' reduce_std); one thread adds the observation-statistics and parameter-noise slots.
// The grid depends only on m, so the block is the same bits run to run.
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "actor_device.h"
#include "ddpg_rows.h"   // the tile forward (net_rows) and the moments merge, shared with ddpg_eval.hip
#include "ssc_host.h"

namespace ssc {

namespace {

constexpr int kSStreams = 4;                   // Q(s, a) | Q(s, pi(s)) | pi(s) | perturbed pi(s)
constexpr int kSMaxRows = 4096;

// LDS carve of one workgroup, in floats: rows of 16 floats ([unit][row])
struct StatsCarve {
    int32_t off_SA, off_SP, off_SC, off_ACT, off_H1, off_H2, off_PI, off_PP, off_Q, off_QPI;
    int64_t floats;
};

// ONE function of the shapes for the host (launch size) and for a workgroup of the population launch (its own pair)
SSC_HD StatsCarve stats_carve(int od, int ad, int ah1, int ah2, int ch1, int ch2) {
    StatsCarve c{};
    int64_t p = 0;
    c.off_SA = (int32_t)p;  p += (int64_t)od * kSR;
    c.off_SP = (int32_t)p;  p += (int64_t)od * kSR;
    c.off_SC = (int32_t)p;  p += (int64_t)od * kSR;
    c.off_ACT = (int32_t)p; p += (int64_t)ad * kSR;
    c.off_H1 = (int32_t)p;  p += (ah1 > (int64_t)ch1 + ad ? ah1 : (int64_t)ch1 + ad) * kSR;
    c.off_H2 = (int32_t)p;  p += (int64_t)(ah2 > ch2 ? ah2 : ch2) * kSR;
    c.off_PI = (int32_t)p;  p += (int64_t)ad * kSR;
    c.off_PP = (int32_t)p;  p += (int64_t)ad * kSR;
    c.off_Q = (int32_t)p;   p += kSR;
    c.off_QPI = (int32_t)p; p += kSR;
    c.floats = p;
    return c;
}

struct StatsArgs {
    StatsNet actor, pert, critic;
    int32_t has_pert, m, obs_dim, act_dim;
    const float *obs, *act;
    const double *rms;                         // null: no normalize_observations
    StatsCarve lds;
    double *part;                              // [n_blocks][kSStreams][3] = (count, mean, M2)
};

SSC_HD void fill_actor(StatsNet &n, const ssc_actor_desc &d) {
    fill_net(n, d.W1, d.b1, d.W2, d.b2, d.W3, d.b3, d.ln1_g, d.ln1_b, d.ln2_g, d.ln2_b, d.h1, d.h2, d.last_layer_tanh, d.obs_clip);
}

// The kernel arguments of one agent: the host packs them into the kernarg of the single launch, a workgroup of the
// population launch from its pair's item.  perturbed: null for none.
SSC_HD void pack_stats(StatsArgs &a, const ssc_actor_desc &actor, const ssc_critic_desc &critic, const ssc_actor_desc *perturbed,
                       int64_t m, const float *obs, const float *act, const double *rms, double *part) {
    fill_actor(a.actor, actor);
    fill_net(a.critic, critic.W1, critic.b1, critic.W2, critic.b2, critic.W3, critic.b3, critic.ln1_g, critic.ln1_b, critic.ln2_g,
             critic.ln2_b, critic.h1, critic.h2, critic.last_layer_tanh, critic.obs_clip);
    a.pert = a.actor;
    if (perturbed != nullptr) fill_actor(a.pert, *perturbed);
    a.has_pert = perturbed != nullptr;
    a.m = (int32_t)m; a.obs_dim = actor.obs_dim; a.act_dim = actor.act_dim;
    a.obs = obs; a.act = act; a.rms = rms;
    a.part = part;
    a.lds = stats_carve(actor.obs_dim, actor.act_dim, actor.h1, actor.h2, critic.h1, critic.h2);
}

SSC_HD int stats_blocks(int64_t m) { return (int)((m + kSR - 1) / kSR); }

// The whole rows launch of one agent: workgroup blockIdx.x of ITS grid row.  Shared by ddpg_stats_rows_kernel (arguments in
// the kernarg) and ddpg_stats_rows_many_kernel (arguments formed from the pair's item); by value, as rollout_body takes its
// arguments.  The weights are read through address-space-1 pointers (global_net): read out of an item they are generic to
// the compiler, which would load through them with FLAT instructions.
__device__ __forceinline__ void stats_rows_body(const StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kSR;
    const GlobalNet actor = global_net(a.actor), pert = global_net(a.pert), critic = global_net(a.critic);
    // ---- the rows of this workgroup; rows past the batch shadow its last one and stay out of the reduction ----
    if (tid < kSR) {
        const int64_t i = min(row0 + tid, a.m - 1);
        const float clip[3] = {a.actor.obs_clip, a.pert.obs_clip, a.critic.obs_clip};
        const int off[3] = {a.lds.off_SA, a.lds.off_SP, a.lds.off_SC};
        if (a.rms != nullptr) {   // normalize_observations (ddpg_editted.py:100-109), as the *_rms forward kernels
            ObsNorm<SSC_MAX_STATE> nrm;
            nrm.load(a.rms, a.obs_dim);
#pragma unroll
            for (int k = 0; k < SSC_MAX_STATE; ++k)
                if (k < a.obs_dim) {
                    const float x = a.obs[i * a.obs_dim + k];
#pragma unroll
                    for (int q = 0; q < 3; ++q) lds[off[q] + k * kSR + tid] = nrm.apply(x, k, clip[q]);
                }
        } else {
            for (int k = 0; k < a.obs_dim; ++k) {
                const float x = a.obs[i * a.obs_dim + k];
#pragma unroll
                for (int q = 0; q < 3; ++q) lds[off[q] + k * kSR + tid] = clip_obs(x, clip[q]);
            }
        }
        for (int k = 0; k < a.act_dim; ++k) lds[a.lds.off_ACT + k * kSR + tid] = a.act[i * a.act_dim + k];
    }
    __syncthreads();
    const StatsCarve &c = a.lds;
    float *h1s = lds + c.off_H1, *h2s = lds + c.off_H2;
    net_rows<false>(actor, lds + c.off_SA, a.obs_dim, nullptr, 0, a.act_dim, true, h1s, h2s, lds + c.off_PI, tid);
    if (a.has_pert)   // block-uniform
        net_rows<false>(pert, lds + c.off_SP, a.obs_dim, nullptr, 0, a.act_dim, true, h1s, h2s, lds + c.off_PP, tid);
    net_rows<true>(critic, lds + c.off_SC, a.obs_dim, lds + c.off_ACT, a.act_dim, 1, false, h1s, h2s, lds + c.off_Q, tid);
    net_rows<true>(critic, lds + c.off_SC, a.obs_dim, lds + c.off_PI, a.act_dim, 1, false, h1s, h2s, lds + c.off_QPI, tid);
    // ---- (count, mean, M2) of each stream over this workgroup's rows: one thread per stream, the values in index order ----
    if (tid < kSStreams && (tid != 3 || a.has_pert)) {
        const int off[kSStreams] = {c.off_Q, c.off_QPI, c.off_PI, c.off_PP};
        const float *v = lds + off[tid];
        const int rows = min(kSR, a.m - row0), dims = tid < 2 ? 1 : a.act_dim;
        const double cnt = (double)(rows * dims);
        double s = 0.0;
        for (int r = 0; r < rows; ++r)
            for (int d = 0; d < dims; ++d) s += (double)v[d * kSR + r];
        const double mean = s / cnt;
        double m2 = 0.0;
        for (int r = 0; r < rows; ++r)
            for (int d = 0; d < dims; ++d) {
                const double dl = (double)v[d * kSR + r] - mean;
                m2 = fma(dl, dl, m2);
            }
        double *p = a.part + ((size_t)blockIdx.x * kSStreams + tid) * 3;
        p[0] = cnt;
        p[1] = mean;
        p[2] = m2;
    }
}

__global__ __launch_bounds__(kSThreads) void ddpg_stats_rows_kernel(StatsArgs a) { stats_rows_body(a); }

// A population in one launch (ssc_ddpg_stats_many): blockIdx.y is the pair, whose item sits at a workgroup-uniform
// address (scalar loads).  A workgroup beyond its pair's tile count -- every workgroup of a pair with m == 0 -- leaves as a
// whole, before any barrier.  Shapes, LayerNorm, d_rms, the perturbed copy and the LDS carve are the pair's own.
__global__ __launch_bounds__(kSThreads) void ddpg_stats_rows_many_kernel(const ssc_ddpg_stats_many_item *__restrict__ items) {
    const ssc_ddpg_stats_many_item &it = items[blockIdx.y];
    if ((int64_t)blockIdx.x * kSR >= it.m) return;
    StatsArgs a;
    pack_stats(a, it.actor, it.critic, it.has_perturbed ? &it.perturbed : nullptr, it.m, it.d_obs, it.d_act, it.d_rms,
               static_cast<double *>(it.d_workspace));
    stats_rows_body(a);
}

__device__ __forceinline__ void stats_merge_body(const double *__restrict__ part, int32_t n_blocks, int32_t has_pert,
                                                 const double *__restrict__ rms, int32_t obs_dim, const float *__restrict__ stddev,
                                                 double *__restrict__ out) {
    const int s = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double nan = __builtin_nan("");
    if (s < 3 || has_pert) {   // wave-uniform
        const int per = (n_blocks + 63) / 64;
        const int b0 = min(lane * per, n_blocks), b1 = min(b0 + per, n_blocks);
        Moments acc{0.0, 0.0, 0.0};
        for (int b = b0; b < b1; ++b) {
            const double *p = part + ((size_t)b * kSStreams + s) * 3;
            acc = chan_merge(acc, Moments{p[0], p[1], p[2]});
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {   // lane l takes lanes l + off: a fixed tree, lane 0 holds the batch
            const Moments o{__shfl_down(acc.n, off), __shfl_down(acc.mean, off), __shfl_down(acc.m2, off)};
            if (lane + off < 64) acc = chan_merge(acc, o);
        }
        if (lane == 0) {
            out[2 + 2 * s] = acc.mean;
            out[3 + 2 * s] = sqrt(acc.m2 / acc.n);
        }
    } else if (lane == 0) {
        out[2 + 2 * s] = nan;
        out[3 + 2 * s] = nan;
    }
    if (threadIdx.x == 1) {
        // obs_rms_mean / obs_rms_std (ddpg_editted.py:236-238): the mean over the dimensions of the fp32 mean / std the
        // networks use (ObsNorm), summed in f64 in index order
        double sm = nan, ss = nan;
        if (rms != nullptr) {
            ObsNorm<SSC_MAX_STATE> nrm;
            nrm.load(rms, obs_dim);
            sm = 0.0;
            ss = 0.0;
#pragma unroll
            for (int c = 0; c < SSC_MAX_STATE; ++c)
                if (c < obs_dim) {
                    sm += (double)nrm.mean[c];
                    ss += (double)nrm.std[c];
                }
            sm /= (double)obs_dim;
            ss /= (double)obs_dim;
        }
        out[0] = sm;
        out[1] = ss;
        out[10] = stddev != nullptr ? (double)stddev[0] : nan;
    }
}

__global__ __launch_bounds__(kSStreams * 64) void ddpg_stats_merge_kernel(const double *__restrict__ part, int32_t n_blocks,
                                                                           int32_t has_pert, const double *__restrict__ rms,
                                                                           int32_t obs_dim, const float *__restrict__ stddev,
                                                                           double *__restrict__ out) {
    stats_merge_body(part, n_blocks, has_pert, rms, obs_dim, stddev, out);
}

// workgroup p merges pair p's partials exactly as the pair's own merge launch; a skipped pair's block stays untouched
__global__ __launch_bounds__(kSStreams * 64) void ddpg_stats_merge_many_kernel(const ssc_ddpg_stats_many_item *__restrict__ items) {
    const ssc_ddpg_stats_many_item &it = items[blockIdx.x];
    if (it.m == 0) return;
    stats_merge_body(static_cast<const double *>(it.d_workspace), stats_blocks(it.m), it.has_perturbed != 0, it.d_rms, it.actor.obs_dim,
                     it.d_param_noise_stddev, it.d_out);
}

constexpr size_t kLdsBytes = 160 * 1024;

int raise_lds(const void *fn, size_t lds, const char *what) {
    if (lds <= 64 * 1024) return SSC_OK;
    return check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), what);
}

bool net_ok(const ssc_actor_desc &d) {
    StatsNet n;
    return fill_net(n, d.W1, d.b1, d.W2, d.b2, d.W3, d.b3, d.ln1_g, d.ln1_b, d.ln2_g, d.ln2_b, d.h1, d.h2, d.last_layer_tanh, d.obs_clip);
}

// The checks of one agent -- the single call's, and through `who` an item's of the population call.  *lds: the bytes of
// LDS its workgroups need.
int stats_check(const char *who, const ssc_actor_desc *actor, const ssc_critic_desc *critic, const ssc_actor_desc *perturbed, int64_t m,
                const float *d_obs, const float *d_act, const double *d_out, const void *d_workspace, size_t workspace_bytes,
                size_t *lds) {
    SSC_REQUIRE(d_out != nullptr, "%s: output block NULL", who);
    SSC_REQUIRE(m >= 1 && m <= kSMaxRows, "%s: m %lld not in 1..%d", who, (long long)m, kSMaxRows);
    SSC_REQUIRE(actor->obs_dim >= 1 && actor->obs_dim <= SSC_MAX_STATE && actor->act_dim >= 1 && actor->act_dim <= SSC_MAX_ACT,
                "%s: obs_dim %d / act_dim %d out of range", who, actor->obs_dim, actor->act_dim);
    SSC_REQUIRE(critic->obs_dim == actor->obs_dim && critic->act_dim == actor->act_dim,
                "%s: the critic's obs_dim %d / act_dim %d differ from the actor's %d / %d", who, critic->obs_dim, critic->act_dim,
                actor->obs_dim, actor->act_dim);
    SSC_REQUIRE(actor->h1 >= 1 && actor->h2 >= 1 && critic->h1 >= 1 && critic->h2 >= 1, "%s: bad hidden sizes", who);
    if (perturbed != nullptr)
        SSC_REQUIRE(perturbed->obs_dim == actor->obs_dim && perturbed->act_dim == actor->act_dim && perturbed->h1 == actor->h1 &&
                        perturbed->h2 == actor->h2,
                    "%s: the perturbed actor's shape differs from the actor's", who);
    SSC_REQUIRE(d_obs != nullptr && d_act != nullptr, "%s: NULL sample", who);
    SSC_REQUIRE(net_ok(*actor), "%s: actor: NULL device pointer, or LayerNorm pointers that do not come together", who);
    StatsNet cn;
    SSC_REQUIRE(fill_net(cn, critic->W1, critic->b1, critic->W2, critic->b2, critic->W3, critic->b3, critic->ln1_g, critic->ln1_b,
                         critic->ln2_g, critic->ln2_b, critic->h1, critic->h2, critic->last_layer_tanh, critic->obs_clip),
                "%s: critic: NULL device pointer, or LayerNorm pointers that do not come together", who);
    if (perturbed != nullptr)
        SSC_REQUIRE(net_ok(*perturbed), "%s: perturbed actor: NULL device pointer, or LayerNorm pointers that do not come together", who);
    const size_t need = ssc_ddpg_stats_workspace_bytes(m);
    SSC_REQUIRE(d_workspace != nullptr && workspace_bytes >= need, "%s: workspace %zu < %zu bytes (ssc_ddpg_stats_workspace_bytes)", who,
                workspace_bytes, need);
    *lds = (size_t)stats_carve(actor->obs_dim, actor->act_dim, actor->h1, actor->h2, critic->h1, critic->h2).floats * sizeof(float);
    if (*lds > kLdsBytes)
        return set_error(SSC_EUNSUPPORTED, "%s: these layer sizes need %zu B of LDS per workgroup (160 KB available)", who, *lds);
    return SSC_OK;
}

}  // namespace

}  // namespace ssc

using namespace ssc;

static_assert(SSC_DDPG_N_STATS == 3 + 2 * kSStreams, "two observation slots, mean / std per stream, the noise stddev");

extern "C" {

size_t ssc_ddpg_stats_workspace_bytes(int64_t m) {
    if (m < 1 || m > kSMaxRows) return 0;
    return (size_t)stats_blocks(m) * kSStreams * 3 * sizeof(double);
}

int ssc_ddpg_stats(const ssc_actor_desc *actor, const ssc_critic_desc *critic, const ssc_actor_desc *perturbed, int64_t m,
                   const float *d_obs, const float *d_act, const double *d_rms, const float *d_param_noise_stddev,
                   double *d_out, void *d_workspace, size_t workspace_bytes, ssc_stream_t stream) {
    SSC_REQUIRE(actor != nullptr && critic != nullptr, "ssc_ddpg_stats: actor / critic NULL");
    size_t lds = 0;
    if (int rc = stats_check("ssc_ddpg_stats", actor, critic, perturbed, m, d_obs, d_act, d_out, d_workspace, workspace_bytes, &lds))
        return rc;
    StatsArgs a{};
    pack_stats(a, *actor, *critic, perturbed, m, d_obs, d_act, d_rms, static_cast<double *>(d_workspace));
    if (int rc = raise_lds(reinterpret_cast<const void *>(ddpg_stats_rows_kernel), lds, "hipFuncSetAttribute(ddpg_stats_rows_kernel)"))
        return rc;
    hipStream_t s = as_stream(stream);
    const int nb = stats_blocks(m);
    hipLaunchKernelGGL(ddpg_stats_rows_kernel, dim3(nb), dim3(kSThreads), lds, s, a);
    hipLaunchKernelGGL(ddpg_stats_merge_kernel, dim3(1), dim3(kSStreams * 64), 0, s, a.part, nb, a.has_pert, d_rms, a.obs_dim,
                       d_param_noise_stddev, d_out);
    return check_launch("ssc_ddpg_stats");
}

int ssc_ddpg_stats_many(const ssc_ddpg_stats_many_item *h_items, const ssc_ddpg_stats_many_item *d_items, int32_t n_pairs,
                        ssc_stream_t stream) {
    SSC_REQUIRE(n_pairs >= 1, "ssc_ddpg_stats_many: n_pairs %d < 1", n_pairs);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_ddpg_stats_many: NULL item array");
    if (n_pairs > 65535) return set_error(SSC_EUNSUPPORTED, "ssc_ddpg_stats_many: %d pairs > 65535 (one grid row each)", n_pairs);
    int64_t m_max = 0;
    size_t lds_max = 0;
    std::vector<std::pair<const void *, int>> owned;   // (array, pair) of what a pair's workgroups write
    owned.reserve((size_t)n_pairs * 2);
    for (int p = 0; p < n_pairs; ++p) {
        const ssc_ddpg_stats_many_item &it = h_items[p];
        if (it.m == 0) continue;   // skipped: no workgroup works for it, nothing else of the item is read
        char who[48];
        snprintf(who, sizeof who, "ssc_ddpg_stats_many: pair %d", p);
        size_t lds = 0;
        if (int rc = stats_check(who, &it.actor, &it.critic, it.has_perturbed ? &it.perturbed : nullptr, it.m, it.d_obs, it.d_act, it.d_out,
                                 it.d_workspace, it.workspace_bytes, &lds))
            return rc;
        m_max = std::max(m_max, it.m);
        lds_max = std::max(lds_max, lds);
        owned.emplace_back(it.d_out, p);
        owned.emplace_back(it.d_workspace, p);
    }
    std::sort(owned.begin(), owned.end());
    for (size_t k = 1; k < owned.size(); ++k)
        SSC_REQUIRE(owned[k].first != owned[k - 1].first || owned[k].second == owned[k - 1].second, "ssc_ddpg_stats_many: pairs %d and %d share an output block or a workspace",
                    owned[k - 1].second, owned[k].second);
    if (m_max == 0) return SSC_OK;
    if (int rc = raise_lds(reinterpret_cast<const void *>(ddpg_stats_rows_many_kernel), lds_max,
                           "hipFuncSetAttribute(ddpg_stats_rows_many_kernel)"))
        return rc;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ddpg_stats_rows_many_kernel, dim3((unsigned)stats_blocks(m_max), (unsigned)n_pairs), dim3(kSThreads), lds_max, s,
                       d_items);
    hipLaunchKernelGGL(ddpg_stats_merge_many_kernel, dim3((unsigned)n_pairs), dim3(kSStreams * 64), 0, s, d_items);
    return check_launch("ssc_ddpg_stats_many");
}

}  // extern "C"
