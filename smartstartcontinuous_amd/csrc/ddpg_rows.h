// ddpg_rows.h -- what the kernels that run whole DDPG networks for a tile of 16 rows share (ddpg_stats.hip: the rows of the
// diagnostics sample; ddpg_eval.hip: the envs of an evaluation rollout): the block-cooperative fp32 forward with every unit
// summed in index order, and the (count, mean, M2) merge of Chan, Golub & LeVeque.
#pragma once

#include "actor_device.h"

namespace ssc {

constexpr int kSR = 16;                        // batch rows per workgroup
constexpr int kSThreads = 256;
constexpr int kSParts = kSThreads / kSR;       // threads per batch row

#define SSC_GLOBAL __attribute__((address_space(1)))

// PTR: `const float *` (generic: global memory or an LDS image), or `const SSC_GLOBAL float *` for weights that are known
// to sit in global memory but whose pointers were read out of a population item -- generic to the compiler, which would
// load through them with FLAT instructions
template <class PTR>
struct StatsNetT {
    PTR W1, b1, W2, b2, W3, b3;
    PTR ln1_g, ln1_b, ln2_g, ln2_b;               // LayerNorm (models_editted.py:45-46, 50-51, 85-86, 91-92); null: none
    int32_t h1, h2, last_tanh;
    float obs_clip;
};
using StatsNet = StatsNetT<const float *>;
using GlobalNet = StatsNetT<const SSC_GLOBAL float *>;

__device__ __forceinline__ GlobalNet global_net(const StatsNet &g) {
    using P = const SSC_GLOBAL float *;
    return GlobalNet{(P)g.W1, (P)g.b1, (P)g.W2, (P)g.b2, (P)g.W3, (P)g.b3, (P)g.ln1_g, (P)g.ln1_b, (P)g.ln2_g, (P)g.ln2_b,
                     g.h1, g.h2, g.last_tanh, g.obs_clip};
}

// One network for the workgroup's 16 rows (block-cooperative).  x [in_dim][16]; `extra` [n_extra][16] joins behind the
// first activation (the critic's action, models_editted.py:89; n_extra = 0 for the actor); out [out_dim][16].
// EXACT_TANH: the hidden tanh of critic_kernel is tanhf, the actor kernels' is tanh_fast.  NET: StatsNet or GlobalNet.
template <bool EXACT_TANH, class NET>
static __device__ void net_rows(const NET &n, const float *x, int in_dim, const float *extra, int n_extra, int out_dim,
                                bool out_tanh, float *h1s, float *h2s, float *out, int tid) {
    const int row = tid & (kSR - 1), part = tid >> 4;
    const bool ln = n.ln1_g != nullptr;
    auto act2 = [&](float v) { return n.last_tanh ? (EXACT_TANH ? tanhf(v) : tanh_fast(v)) : fmaxf(v, 0.0f); };
    for (int j = part; j < n.h1; j += kSParts) {
        float acc = n.b1[j];
        for (int c = 0; c < in_dim; ++c) acc = fmaf(x[c * kSR + row], n.W1[c * n.h1 + j], acc);
        h1s[j * kSR + row] = ln ? acc : fmaxf(acc, 0.0f);
    }
    __syncthreads();
    if (ln) {   // every thread forms its row's statistics itself, in index order
        float mean, rstd;
        layer_norm_stats(h1s + row, n.h1, kSR, mean, rstd);
        __syncthreads();
        for (int j = part; j < n.h1; j += kSParts)
            h1s[j * kSR + row] = fmaxf(fmaf((h1s[j * kSR + row] - mean) * rstd, n.ln1_g[j], n.ln1_b[j]), 0.0f);
    }
    for (int a = part; a < n_extra; a += kSParts) h1s[(n.h1 + a) * kSR + row] = extra[a * kSR + row];
    __syncthreads();
    const int in2 = n.h1 + n_extra;
    for (int j = part; j < n.h2; j += kSParts) {
        float acc = n.b2[j];
#pragma unroll 8
        for (int k = 0; k < in2; ++k) acc = fmaf(h1s[k * kSR + row], n.W2[k * n.h2 + j], acc);
        h2s[j * kSR + row] = ln ? acc : act2(acc);
    }
    __syncthreads();
    if (ln) {
        float mean, rstd;
        layer_norm_stats(h2s + row, n.h2, kSR, mean, rstd);
        __syncthreads();
        for (int j = part; j < n.h2; j += kSParts)
            h2s[j * kSR + row] = act2(fmaf((h2s[j * kSR + row] - mean) * rstd, n.ln2_g[j], n.ln2_b[j]));
        __syncthreads();
    }
    for (int a = part; a < out_dim; a += kSParts) {
        // the actor's chain starts from b3 (the actor kernels' bits); a head without an output tanh -- the critic -- adds
        // b3 behind a chain that starts from zero, as critic_kernel does (smartstart.hip has the reason)
        float o = out_tanh ? n.b3[a] : 0.0f;
        for (int j = 0; j < n.h2; ++j) o = fmaf(h2s[j * kSR + row], n.W3[j * out_dim + a], o);
        out[a * kSR + row] = out_tanh ? tanh_fast(o) : o + n.b3[a];
    }
    __syncthreads();
}

struct Moments { double n, mean, m2; };

// Chan, Golub & LeVeque (1979): the moments of the union of two samples
__device__ __forceinline__ Moments chan_merge(const Moments &x, const Moments &y) {
    if (y.n == 0.0) return x;
    if (x.n == 0.0) return y;
    const double n = x.n + y.n, delta = y.mean - x.mean;
    return Moments{n, x.mean + delta * (y.n / n), x.m2 + y.m2 + delta * delta * (x.n * y.n / n)};
}

// false: a NULL device pointer, or LayerNorm pointers that do not come together.  Host and device: the single launches
// fill their kernarg with it, a workgroup of the population launches fills the same struct from its pair's item.
SSC_HD bool fill_net(StatsNet &n, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                     const float *b3, const float *g1, const float *be1, const float *g2, const float *be2, int h1, int h2,
                     int last_tanh, float clip) {
    n = StatsNet{W1, b1, W2, b2, W3, b3, g1, be1, g2, be2, h1, h2, last_tanh, clip};
    const bool ln = g1 != nullptr;
    return W1 && b1 && W2 && b2 && W3 && b3 && ln == (be1 != nullptr) && ln == (g2 != nullptr) && ln == (be2 != nullptr);
}

}  // namespace ssc
