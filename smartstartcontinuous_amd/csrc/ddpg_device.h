// ddpg_device.h -- pieces shared by the DDPG learner kernels (ddpg_train.hip: single-workgroup step interpreter;
// ddpg_train_fixed.hip: the shipped 64-32 shape compiled straight-line; ddpg_train_wide.hip: any shape, multi-workgroup):
// the fp32 MFMA, MpiAdam on one element (moments, the two spellings of the step, the bias-correction clock), and the
// launchers ddpg_train.hip dispatches to.  The flat parameter layout and the dispatch itself are ddpg_layout.h.
#pragma once

#include "ddpg_layout.h"
#include "ssc_device.h"

namespace ssc {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f32x4m __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x4_f32: exact fp32 products and sums.  Lane l of a wave holds A[row l & 15][k = l >> 4],
// B[k = l >> 4][col l & 15], D[row 4 (l >> 4) + r][col l & 15].
__device__ __forceinline__ f32x4m mfma4(float a, float b, const f32x4m &c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// beta^n for an integer step count, by squaring in f64 (ocml's pow() alone is several thousand instructions)
static __device__ __noinline__ double ipow(double base, int n) {
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= base;
        base *= base;
        n >>= 1;
    }
    return r;
}

struct AdamCfg {
    float a, beta1, beta2, eps;   // a = stepsize * sqrt(1 - b2^t) / (1 - b1^t) with t already incremented
};

// MpiAdam.update on one element (baselines common/mpi_adam.py [third-party], ddpg_editted.py:326-327): the moments ...
__device__ __forceinline__ void adam_moments(float &m, float &v, float g, const AdamCfg &c) {
    m = c.beta1 * m + (1.0f - c.beta1) * g;
    v = c.beta2 * v + (1.0f - c.beta2) * (g * g);
}
// ... and the step added to theta, in two spellings ON PURPOSE.  The single-workgroup kernels (step interpreter, fixed
// 64-32) take the 1-ulp sqrt / rcp instructions: a 1e-7 relative wobble of a 1e-3-sized step, and no division sequence
// on their critical path.  The multi-workgroup apply pass (ddpg_wide_apply_kernel, which also finishes the tiled fixed
// kernel and Pop-Art) is one element per thread with nothing to hide and keeps IEEE sqrtf and division.  Each learner is
// bit-for-bit reproducible in its own spelling; do not merge them.
__device__ __forceinline__ float adam_step_fast(float m, float v, const AdamCfg &c) {
    return (-c.a) * m * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) + c.eps);
}
__device__ __forceinline__ float adam_step_ieee(float m, float v, const AdamCfg &c) { return (-c.a) * m / (sqrtf(v) + c.eps); }

// MpiAdam's bias-corrected step size in f64 (1 - 0.999^t loses 5 digits in fp32); b1t, b2t = beta1^t, beta2^t
__device__ __forceinline__ AdamCfg adam_cfg(double lr, double b1t, double b2t, const ssc_ddpg_desc &d) {
    return AdamCfg{(float)(lr * sqrt(1.0 - b2t) / (1.0 - b1t)), d.beta1, d.beta2, d.epsilon};
}

// The step counters of the two optimisers and their running beta powers over a launch of several iterations: one ipow
// per launch, then one multiplication per iteration -- the per-iteration ipow + sqrt + divisions sat on the critical path
// (3.6 k cycles with every other thread waiting at the barrier).  The wide apply pass is one launch per iteration and
// calls ipow + adam_cfg itself.
struct AdamClock {
    int tA, tC;
    double b1a, b2a, b1c, b2c;
    // counters = false: a launch that only produces gradients (the tiled fixed kernel) does not read adam_t
    __device__ __forceinline__ void init(const ssc_ddpg_desc &d, bool counters = true) {
        tA = counters ? d.adam_t[0] : 0; tC = counters ? d.adam_t[1] : 0;
        b1a = ipow((double)d.beta1, tA); b2a = ipow((double)d.beta2, tA);
        b1c = ipow((double)d.beta1, tC); b2c = ipow((double)d.beta2, tC);
    }
    __device__ __forceinline__ void tick(const ssc_ddpg_desc &d) {
        ++tA; ++tC;
        b1a *= (double)d.beta1; b2a *= (double)d.beta2; b1c *= (double)d.beta1; b2c *= (double)d.beta2;
    }
    __device__ __forceinline__ AdamCfg cfg_actor(const ssc_ddpg_desc &d) const { return adam_cfg((double)d.actor_lr, b1a, b2a, d); }
    __device__ __forceinline__ AdamCfg cfg_critic(const ssc_ddpg_desc &d) const { return adam_cfg((double)d.critic_lr, b1c, b2c, d); }
};

// ddpg_train_fixed.hip (ddpg_fixed_shape / ddpg_fixed_tiled_shape: ddpg_layout.h)
int ddpg_train_fixed(const ssc_ddpg_desc *d, const ssc_replay_view *rp, const int32_t *d_batch_idx, int32_t n_iters,
                     float *d_losses, hipStream_t stream, const double *d_rms);

// the shipped shape at batches of 128, 192, ... (multiples of 64): the straight-line kernel on one 64-row tile per workgroup
// (gradients only), then the multi-workgroup apply pass of ddpg_train_wide.hip
int ddpg_train_fixed_tiled(const ssc_ddpg_desc *d, const ssc_replay_view *rp, const int32_t *d_batch_idx, int32_t n_iters,
                           float *d_losses, void *d_workspace, size_t workspace_bytes, hipStream_t stream, const double *d_rms);

// a population of batch-64 agents of the shipped shape, one workgroup each (ssc_ddpg_train_many validated the items)
int ddpg_train_fixed_many(const ssc_ddpg_many_item *d_items, int32_t n_agents, int obs_dim, bool last_layer_tanh, bool rms,
                          hipStream_t stream);

// ddpg_train_wide.hip: any layer sizes / batch sizes, batch tiled over workgroups
size_t ddpg_wide_workspace_bytes(const ssc_ddpg_desc *d);
// The apply pass over `n_blocks` gradient partials laid out [n_blocks][n_params] at the start of the workspace, loss
// partials [n_blocks][2] behind them (ddpg_wide_partials); iteration `it` of the call; `ddpg_wide_finish` moves the
// MpiAdam step counters once, after the last iteration.
struct WidePartials { float *gpart, *lpart; };
WidePartials ddpg_wide_partials(const ssc_ddpg_desc *d, void *d_workspace, int n_blocks);
void ddpg_wide_apply(const ssc_ddpg_desc *d, void *d_workspace, int n_blocks, int it, float *d_losses_it, hipStream_t stream);
void ddpg_wide_finish(const ssc_ddpg_desc *d, int32_t n_iters, hipStream_t stream);
// d_rms (all three): NULL, or the RunningMeanStd block of normalize_observations (actor_device.h)
int ddpg_train_wide(const ssc_ddpg_desc *d, const ssc_replay_view *rp, const int32_t *d_batch_idx, int32_t n_iters,
                    float *d_losses, void *d_workspace, size_t workspace_bytes, hipStream_t stream, const double *d_rms);
// A population on the same kernels, grid row = agent (ssc_ddpg_train_many_wide; the items already through ddpg_check).
// The plan -- [n_agents rows | four lists of row numbers] -- is caller memory: ddpg_wide_plan fills a host buffer of
// ddpg_wide_plan_bytes(n_agents) bytes (pure host code; refuses a short workspace and a tile above the LDS),
// ddpg_train_wide_many launches over the host copy's geometry and the device copy's address.
size_t ddpg_wide_plan_bytes(int32_t n_agents);
int ddpg_wide_plan(const ssc_ddpg_many_wide_item *h_items, int32_t n_agents, void *h_plan);
int ddpg_train_wide_many(const void *h_plan, const void *d_plan, int32_t n_agents, hipStream_t stream);
// ... and the Pop-Art agents' grouped launches (ssc_ddpg_train_many_popart): the same protocol on a plan format of its own,
// [n_agents rows | five lists]
size_t ddpg_pop_plan_bytes(int32_t n_agents);
int ddpg_pop_plan(const ssc_ddpg_many_popart_item *h_items, int32_t n_agents, void *h_plan);
int ddpg_train_pop_many(const void *h_plan, const void *d_plan, int32_t n_agents, hipStream_t stream);
// Pop-Art (normalize_returns + enable_popart): every shape runs the multi-workgroup kernels, four launches per iteration;
// d_ret_rms: the one-column RunningMeanStd block of the returns, read and written
size_t ddpg_popart_workspace_bytes(const ssc_ddpg_desc *d);
int ddpg_train_wide_popart(const ssc_ddpg_desc *d, const ssc_replay_view *rp, const int32_t *d_batch_idx, int32_t n_iters,
                           float *d_losses, void *d_workspace, size_t workspace_bytes, hipStream_t stream, const double *d_rms,
                           double *d_ret_rms);

}  // namespace ssc
