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
#include "actor_device.h"
#include "ddpg_rows.h"   // the tile forward (net_rows) and the moments merge, shared with ddpg_eval.hip
#include "ssc_host.h"

namespace ssc {

namespace {

constexpr int kSStreams = 4;                   // Q(s, a) | Q(s, pi(s)) | pi(s) | perturbed pi(s)
constexpr int kSMaxRows = 4096;

struct StatsArgs {
    StatsNet actor, pert, critic;
    int32_t has_pert, m, obs_dim, act_dim;
    const float *obs, *act;
    const double *rms;                         // null: no normalize_observations
    int32_t off_SA, off_SP, off_SC, off_ACT, off_H1, off_H2, off_PI, off_PP, off_Q, off_QPI;   // LDS float offsets
    double *part;                              // [n_blocks][kSStreams][3] = (count, mean, M2)
};

__global__ __launch_bounds__(kSThreads) void ddpg_stats_rows_kernel(StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kSR;
    // ---- the rows of this workgroup; rows past the batch shadow its last one and stay out of the reduction ----
    if (tid < kSR) {
        const int64_t i = min(row0 + tid, a.m - 1);
        const float clip[3] = {a.actor.obs_clip, a.pert.obs_clip, a.critic.obs_clip};
        const int off[3] = {a.off_SA, a.off_SP, a.off_SC};
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
        for (int k = 0; k < a.act_dim; ++k) lds[a.off_ACT + k * kSR + tid] = a.act[i * a.act_dim + k];
    }
    __syncthreads();
    float *h1s = lds + a.off_H1, *h2s = lds + a.off_H2;
    net_rows<false>(a.actor, lds + a.off_SA, a.obs_dim, nullptr, 0, a.act_dim, true, h1s, h2s, lds + a.off_PI, tid);
    if (a.has_pert)   // block-uniform
        net_rows<false>(a.pert, lds + a.off_SP, a.obs_dim, nullptr, 0, a.act_dim, true, h1s, h2s, lds + a.off_PP, tid);
    net_rows<true>(a.critic, lds + a.off_SC, a.obs_dim, lds + a.off_ACT, a.act_dim, 1, false, h1s, h2s, lds + a.off_Q, tid);
    net_rows<true>(a.critic, lds + a.off_SC, a.obs_dim, lds + a.off_PI, a.act_dim, 1, false, h1s, h2s, lds + a.off_QPI, tid);
    // ---- (count, mean, M2) of each stream over this workgroup's rows: one thread per stream, the values in index order ----
    if (tid < kSStreams && (tid != 3 || a.has_pert)) {
        const int off[kSStreams] = {a.off_Q, a.off_QPI, a.off_PI, a.off_PP};
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

__global__ __launch_bounds__(kSStreams * 64) void ddpg_stats_merge_kernel(const double *__restrict__ part, int32_t n_blocks,
                                                                           int32_t has_pert, const double *__restrict__ rms,
                                                                           int32_t obs_dim, const float *__restrict__ stddev,
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

int stats_blocks(int64_t m) { return (int)((m + kSR - 1) / kSR); }

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
    SSC_REQUIRE(d_out != nullptr, "ssc_ddpg_stats: output block NULL");
    SSC_REQUIRE(m >= 1 && m <= kSMaxRows, "ssc_ddpg_stats: m %lld not in 1..%d", (long long)m, kSMaxRows);
    SSC_REQUIRE(actor->obs_dim >= 1 && actor->obs_dim <= SSC_MAX_STATE && actor->act_dim >= 1 && actor->act_dim <= SSC_MAX_ACT,
                "ssc_ddpg_stats: obs_dim %d / act_dim %d out of range", actor->obs_dim, actor->act_dim);
    SSC_REQUIRE(critic->obs_dim == actor->obs_dim && critic->act_dim == actor->act_dim,
                "ssc_ddpg_stats: the critic's obs_dim %d / act_dim %d differ from the actor's %d / %d", critic->obs_dim,
                critic->act_dim, actor->obs_dim, actor->act_dim);
    SSC_REQUIRE(actor->h1 >= 1 && actor->h2 >= 1 && critic->h1 >= 1 && critic->h2 >= 1, "ssc_ddpg_stats: bad hidden sizes");
    if (perturbed != nullptr)
        SSC_REQUIRE(perturbed->obs_dim == actor->obs_dim && perturbed->act_dim == actor->act_dim && perturbed->h1 == actor->h1 &&
                        perturbed->h2 == actor->h2,
                    "ssc_ddpg_stats: the perturbed actor's shape differs from the actor's");
    SSC_REQUIRE(d_obs != nullptr && d_act != nullptr, "ssc_ddpg_stats: NULL sample");
    StatsArgs a{};
    SSC_REQUIRE(fill_net(a.actor, actor->W1, actor->b1, actor->W2, actor->b2, actor->W3, actor->b3, actor->ln1_g, actor->ln1_b,
                         actor->ln2_g, actor->ln2_b, actor->h1, actor->h2, actor->last_layer_tanh, actor->obs_clip),
                "ssc_ddpg_stats: actor: NULL device pointer, or LayerNorm pointers that do not come together");
    SSC_REQUIRE(fill_net(a.critic, critic->W1, critic->b1, critic->W2, critic->b2, critic->W3, critic->b3, critic->ln1_g,
                         critic->ln1_b, critic->ln2_g, critic->ln2_b, critic->h1, critic->h2, critic->last_layer_tanh,
                         critic->obs_clip),
                "ssc_ddpg_stats: critic: NULL device pointer, or LayerNorm pointers that do not come together");
    a.pert = a.actor;
    if (perturbed != nullptr)
        SSC_REQUIRE(fill_net(a.pert, perturbed->W1, perturbed->b1, perturbed->W2, perturbed->b2, perturbed->W3, perturbed->b3,
                             perturbed->ln1_g, perturbed->ln1_b, perturbed->ln2_g, perturbed->ln2_b, perturbed->h1, perturbed->h2,
                             perturbed->last_layer_tanh, perturbed->obs_clip),
                    "ssc_ddpg_stats: perturbed actor: NULL device pointer, or LayerNorm pointers that do not come together");
    const size_t need = ssc_ddpg_stats_workspace_bytes(m);
    SSC_REQUIRE(d_workspace != nullptr && workspace_bytes >= need,
                "ssc_ddpg_stats: workspace %zu < %zu bytes (ssc_ddpg_stats_workspace_bytes)", workspace_bytes, need);
    a.has_pert = perturbed != nullptr;
    a.m = (int32_t)m; a.obs_dim = actor->obs_dim; a.act_dim = actor->act_dim;
    a.obs = d_obs; a.act = d_act; a.rms = d_rms;
    a.part = static_cast<double *>(d_workspace);
    // ---- LDS carve: rows of 16 floats ([unit][row]) ----
    int64_t p = 0;
    auto take = [&](int64_t rows) { const int64_t q = p; p += rows * kSR; return (int32_t)q; };
    const int od = a.obs_dim, ad = a.act_dim;
    a.off_SA = take(od); a.off_SP = take(od); a.off_SC = take(od); a.off_ACT = take(ad);
    a.off_H1 = take(actor->h1 > (int64_t)critic->h1 + ad ? actor->h1 : (int64_t)critic->h1 + ad);
    a.off_H2 = take(actor->h2 > critic->h2 ? actor->h2 : critic->h2);
    a.off_PI = take(ad); a.off_PP = take(ad); a.off_Q = take(1); a.off_QPI = take(1);
    const size_t lds = (size_t)p * sizeof(float);
    if (lds > 160 * 1024)
        return set_error(SSC_EUNSUPPORTED, "ssc_ddpg_stats: these layer sizes need %zu B of LDS per workgroup (160 KB available)", lds);
    if (lds > 64 * 1024) {
        int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(ddpg_stats_rows_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute(ddpg_stats_rows_kernel)");
        if (rc) return rc;
    }
    hipStream_t s = as_stream(stream);
    const int nb = stats_blocks(m);
    hipLaunchKernelGGL(ddpg_stats_rows_kernel, dim3(nb), dim3(kSThreads), lds, s, a);
    hipLaunchKernelGGL(ddpg_stats_merge_kernel, dim3(1), dim3(kSStreams * 64), 0, s, a.part, nb, a.has_pert, d_rms, a.obs_dim,
                       d_param_noise_stddev, d_out);
    return check_launch("ssc_ddpg_stats");
}

}  // extern "C"
