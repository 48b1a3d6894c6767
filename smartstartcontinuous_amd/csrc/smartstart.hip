// smartstart.hip -- SmartStart selection on the GPU (smartexplorationcontinuous.py:223-305):
// batched critic value V(s) = Q(s, pi(s)), Gaussian kernel-density "visitation count" and the
// UCB1 argmax over the candidate smart-start states.
//
// The KDE is the n_ss x |D| pairwise kernel the reference evaluates through
// scipy.stats.gaussian_kde (2000 x 100 000 in the shipped runs): 2e8 exp() per episode start --
// the latency spike the author timed (:354-360).  Here: one block per 8 query points, the data
// set streamed from L2 (0.8 MB at |D| = 1e5, d = 2), fp32 exp on the transcendental pipe, f64
// block reduction.
#include <algorithm>

#include "actor_device.h"
#include "select_many.h"
#include "ssc_host.h"

namespace ssc {

struct CriticW {
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    int32_t obs_dim, act_dim, h1, h2, last_tanh;
    float obs_clip;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;   // LayerNorm (models_editted.py:85-86, 91-92); null: none
};

// one row per lane; layer-1 activations (+ the action, models_editted.py:89) parked in LDS as [unit][lane]
// block bx of the m rows; hs: [(h1 + act_dim)][64] (+ [h2][64] with LayerNorm) of LDS
template <class... Rms>
static __device__ __forceinline__ void critic_body(const CriticW &w, int64_t m, const float *__restrict__ obs,
                                                   const float *__restrict__ act, float *__restrict__ q, float *hs, unsigned bx,
                                                   Rms... rms) {
    const bool ln = w.ln1_g != nullptr;
    const int lane = threadIdx.x;
    const int64_t gi = (int64_t)bx * 64 + lane;
    const bool active = gi < m;
    const int64_t i = active ? gi : m - 1;
    float o[SSC_MAX_STATE];
    if constexpr (kObsNorm<Rms...>) {   // normalize_observations (ddpg_editted.py:100-109; actor_device.h)
        ObsNorm<SSC_MAX_STATE> nrm;
        nrm.load(rms_block(rms...), w.obs_dim);
#pragma unroll
        for (int c = 0; c < SSC_MAX_STATE; ++c) o[c] = (c < w.obs_dim) ? nrm.apply(obs[i * w.obs_dim + c], c, w.obs_clip) : 0.0f;
    } else {
#pragma unroll
        for (int c = 0; c < SSC_MAX_STATE; ++c) {   // ddpg_editted.py:106-109
            const float v = (c < w.obs_dim) ? obs[i * w.obs_dim + c] : 0.0f;
            o[c] = w.obs_clip > 0.0f ? fminf(fmaxf(v, -w.obs_clip), w.obs_clip) : v;
        }
    }
    for (int j = 0; j < w.h1; ++j) {
        float acc = w.b1[j];
#pragma unroll
        for (int c = 0; c < SSC_MAX_STATE; ++c)
            if (c < w.obs_dim) acc = fmaf(o[c], w.W1[c * w.h1 + j], acc);
        hs[j * 64 + lane] = ln ? acc : fmaxf(acc, 0.0f);  // models_editted.py:87
    }
    if (ln) {   // :85-86
        float mean, rstd;
        layer_norm_stats(hs + lane, w.h1, 64, mean, rstd);
        for (int j = 0; j < w.h1; ++j)
            hs[j * 64 + lane] = fmaxf(fmaf((hs[j * 64 + lane] - mean) * rstd, w.ln1_g[j], w.ln1_b[j]), 0.0f);
    }
    for (int a = 0; a < w.act_dim; ++a) hs[(w.h1 + a) * 64 + lane] = act[i * w.act_dim + a];  // :89
    const int in2 = w.h1 + w.act_dim;
    float *h2s = hs + in2 * 64;
    // The output chain starts from zero and b3 is added behind it: b3 follows the mean return (tens), the h2 terms are of
    // order one, and a chain that starts from b3 rounds every partial sum at b3's size -- sqrt(h2) roundings of |b3| where
    // this order has one (tests/forward_cases.py: the bias-first chain misses the derived float32 bound).
    float out = 0.0f;
    for (int j = 0; j < w.h2; ++j) {
        float acc = w.b2[j];
        for (int k = 0; k < in2; ++k) acc = fmaf(hs[k * 64 + lane], w.W2[k * w.h2 + j], acc);
        if (ln) { h2s[j * 64 + lane] = acc; continue; }
        const float h2 = w.last_tanh ? tanhf(acc) : fmaxf(acc, 0.0f);  // :95-98
        out = fmaf(h2, w.W3[j], out);                                    // :100 (no output tanh)
    }
    if (ln) {   // :91-92
        float mean, rstd;
        layer_norm_stats(h2s + lane, w.h2, 64, mean, rstd);
        for (int j = 0; j < w.h2; ++j) {
            const float n2 = fmaf((h2s[j * 64 + lane] - mean) * rstd, w.ln2_g[j], w.ln2_b[j]);
            out = fmaf(w.last_tanh ? tanhf(n2) : fmaxf(n2, 0.0f), w.W3[j], out);
        }
    }
    if (active) q[i] = out + w.b3[0];
}

template <class... Rms>
__global__ __launch_bounds__(64) void critic_kernel(CriticW w, int64_t m, const float *__restrict__ obs,
                                                    const float *__restrict__ act, float *__restrict__ q, Rms... rms) {
    extern __shared__ float hs[];  // [(h1 + act_dim)][64] (+ [h2][64] with LayerNorm)
    critic_body(w, m, obs, act, q, hs, blockIdx.x, rms...);
}

// ssc_critic_forward_many: grid row y = item y on its candidate rows, blocks anchored at the item's first row.  An item with
// statistics runs the body's Rms instantiation, one without the plain one (a workgroup-uniform branch): the single calls' code.
__global__ __launch_bounds__(64) void critic_many_kernel(const ssc_select_many_item *items, const float *__restrict__ act) {
    extern __shared__ float hs[];
    const const_select_item it = (const_select_item)items + blockIdx.y;
    const int64_t rows = it->n_ss;
    if (it->count == 0 || (int64_t)blockIdx.x * 64 >= rows) return;   // an empty item or a surplus block: uniform, no barrier yet
    const CriticW w{it->critic.W1, it->critic.b1, it->critic.W2, it->critic.b2, it->critic.W3, it->critic.b3,
                    it->critic.obs_dim, it->critic.act_dim, it->critic.h1, it->critic.h2, it->critic.last_layer_tanh,
                    it->critic.obs_clip, it->critic.ln1_g, it->critic.ln1_b, it->critic.ln2_g, it->critic.ln2_b};
    const float *a = act + it->row0 * w.act_dim;
    const double *rms = it->d_rms;
    if (rms != nullptr) critic_body(w, rows, it->d_cand, a, it->d_value, hs, blockIdx.x, rms);
    else critic_body(w, rows, it->d_cand, a, it->d_value, hs, blockIdx.x);
}

constexpr int kKdeQ = 8;        // query points per block
constexpr int kKdeThreads = 1024;
constexpr int kKdeU = 4;        // data points per thread and loop trip, loads issued together

struct KdeArgs {
    int32_t d;
    int64_t n, m;
    float wh[SSC_MAX_STATE * SSC_MAX_STATE];
    double norm;
};

// One block = kKdeQ query points against the whole data set.  Round 1 ran this with 256-thread blocks, one data point
// per loop trip and the state dimension as a run-time bound: 2000 / 8 = 250 blocks x 4 waves is ONE wave per SIMD, every
// trip waited for its own L2 round trip, and the d x d whitening plus the per-query distance were 8 x 8 and 8 x 8
// predicated loops for a 2-d state (0.41 ms for 2000 x 100 000, a tenth of the VALU rate).  Now: the dimension is a
// template parameter (D = 0: any d <= SSC_MAX_STATE, guarded), 1024 threads per block (4 waves per SIMD), kKdeU
// independent loads in flight per lane.  fp32 exp on the transcendental pipe, per-thread fp32 sums over <= ~100 terms,
// f64 block reduction in a fixed order (deterministic).
template <int D>
__global__ __launch_bounds__(kKdeThreads) void kde_kernel(KdeArgs a, const float *__restrict__ data,
                                                          const float *__restrict__ points, float *__restrict__ pdf) {
    constexpr int DM = D > 0 ? D : SSC_MAX_STATE;
    __shared__ double red[kKdeThreads / 64][kKdeQ];
    const int d = D > 0 ? D : a.d;
    // whitened query points: y_q = Wh * x_q  (then || Wh (x_q - x_j) || = || y_q - Wh x_j ||).  The whitening matrix is
    // pre-scaled by sqrt(0.5 log2 e), so that exp(-0.5 ||.||^2) = exp2(-||scaled . ||^2): no multiply in front of v_exp_f32
    const float kS = 0.84932180028801904272f;   // sqrt(0.5 * log2(e))
    float yq[kKdeQ][DM];
#pragma unroll
    for (int q = 0; q < kKdeQ; ++q) {
        const int64_t qi = min((int64_t)blockIdx.x * kKdeQ + q, a.m - 1);
#pragma unroll
        for (int r = 0; r < DM; ++r) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < DM; ++c)
                if (r < d && c < d) s = fmaf(a.wh[r * d + c] * kS, points[qi * d + c], s);
            yq[q][r] = s;
        }
    }
    float sum[kKdeQ];
#pragma unroll
    for (int q = 0; q < kKdeQ; ++q) sum[q] = 0.0f;
    for (int64_t j0 = threadIdx.x; j0 < a.n; j0 += (int64_t)kKdeThreads * kKdeU) {
        float x[kKdeU][DM];
#pragma unroll
        for (int u = 0; u < kKdeU; ++u) {
            const int64_t j = j0 + (int64_t)u * kKdeThreads;
#pragma unroll
            for (int c = 0; c < DM; ++c) x[u][c] = (c < d && j < a.n) ? data[j * d + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kKdeU; ++u) {
            const bool live = j0 + (int64_t)u * kKdeThreads < a.n;
            float y[DM];
#pragma unroll
            for (int r = 0; r < DM; ++r) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < DM; ++c)
                    if (r < d && c < d) s = fmaf(a.wh[r * d + c] * kS, x[u][c], s);
                y[r] = s;
            }
            // a data point past the end sits infinitely far away: exp2(-inf) = 0, no select per query
            if (!live) y[0] = INFINITY;
#pragma unroll
            for (int q = 0; q < kKdeQ; ++q) {
                float e = 0.0f;
#pragma unroll
                for (int r = 0; r < DM; ++r)
                    if (r < d) {
                        const float t = yq[q][r] - y[r];
                        e = fmaf(t, t, e);
                    }
                sum[q] += __builtin_amdgcn_exp2f(-e);
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < kKdeQ; ++q) {
        double v = (double)sum[q];
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
        if (lane == 0) red[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kKdeQ) {
        const int64_t qi = (int64_t)blockIdx.x * kKdeQ + threadIdx.x;
        if (qi < a.m) {
            double v = 0.0;
            for (int w = 0; w < kKdeThreads / 64; ++w) v += red[w][threadIdx.x];
            pdf[qi] = (float)(v * a.norm);
        }
    }
}

// kde_kernel's body for ssc_kde_evaluate_many, RESTATED (kde_kernel keeps its text, hence its code: it is the hot launch of a
// selection): the same operations in the same order per query and data point, the same partition of j onto threads and trips
// and the same reduction, with the data row read through `rows` (the ring in place) and the whitening matrix from memory.
struct RingData {
    RingRows r;
    __device__ __forceinline__ float at(int64_t j, int c) const { return r.row(j)[c]; }
};
struct WhOfMemory {
    const float *__restrict__ p;
    __device__ __forceinline__ float operator()(int i) const { return p[i]; }
};

// block bx: kKdeQ query points against the n data rows of `rows`
template <int D, class Rows, class Wh>
static __device__ __forceinline__ void kde_body(int rt_d, int64_t n, int64_t m, const Wh wh, double norm, const Rows rows,
                                                const float *__restrict__ points, float *__restrict__ pdf, unsigned bx) {
    constexpr int DM = D > 0 ? D : SSC_MAX_STATE;
    __shared__ double red[kKdeThreads / 64][kKdeQ];
    const int d = D > 0 ? D : rt_d;
    // whitened query points: y_q = Wh * x_q  (then || Wh (x_q - x_j) || = || y_q - Wh x_j ||).  The whitening matrix is
    // pre-scaled by sqrt(0.5 log2 e), so that exp(-0.5 ||.||^2) = exp2(-||scaled . ||^2): no multiply in front of v_exp_f32
    const float kS = 0.84932180028801904272f;   // sqrt(0.5 * log2(e))
    float yq[kKdeQ][DM];
#pragma unroll
    for (int q = 0; q < kKdeQ; ++q) {
        const int64_t qi = min((int64_t)bx * kKdeQ + q, m - 1);
#pragma unroll
        for (int r = 0; r < DM; ++r) {
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < DM; ++c)
                if (r < d && c < d) s = fmaf(wh(r * d + c) * kS, points[qi * d + c], s);
            yq[q][r] = s;
        }
    }
    float sum[kKdeQ];
#pragma unroll
    for (int q = 0; q < kKdeQ; ++q) sum[q] = 0.0f;
    for (int64_t j0 = threadIdx.x; j0 < n; j0 += (int64_t)kKdeThreads * kKdeU) {
        float x[kKdeU][DM];
#pragma unroll
        for (int u = 0; u < kKdeU; ++u) {
            const int64_t j = j0 + (int64_t)u * kKdeThreads;
#pragma unroll
            for (int c = 0; c < DM; ++c) x[u][c] = (c < d && j < n) ? rows.at(j, c) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kKdeU; ++u) {
            const bool live = j0 + (int64_t)u * kKdeThreads < n;
            float y[DM];
#pragma unroll
            for (int r = 0; r < DM; ++r) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < DM; ++c)
                    if (r < d && c < d) s = fmaf(wh(r * d + c) * kS, x[u][c], s);
                y[r] = s;
            }
            // a data point past the end sits infinitely far away: exp2(-inf) = 0, no select per query
            if (!live) y[0] = INFINITY;
#pragma unroll
            for (int q = 0; q < kKdeQ; ++q) {
                float e = 0.0f;
#pragma unroll
                for (int r = 0; r < DM; ++r)
                    if (r < d) {
                        const float t = yq[q][r] - y[r];
                        e = fmaf(t, t, e);
                    }
                sum[q] += __builtin_amdgcn_exp2f(-e);
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < kKdeQ; ++q) {
        double v = (double)sum[q];
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
        if (lane == 0) red[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kKdeQ) {
        const int64_t qi = (int64_t)bx * kKdeQ + threadIdx.x;
        if (qi < m) {
            double v = 0.0;
            for (int w = 0; w < kKdeThreads / 64; ++w) v += red[w][threadIdx.x];
            pdf[qi] = (float)(v * norm);
        }
    }
}

// ssc_kde_evaluate_many: grid row y = item y; the n_ss candidate slots against the item's data set, read from the ring in place
template <int D>
__global__ __launch_bounds__(kKdeThreads) void kde_many_kernel(const ssc_select_many_item *items) {
    const const_select_item it = (const_select_item)items + blockIdx.y;
    const int64_t m = it->n_ss;
    if (it->count == 0 || (int64_t)blockIdx.x * kKdeQ >= m) return;   // an empty item or a surplus block: uniform, no barrier yet
    if (*it->d_status != 0) return;
    kde_body<D>(it->ring.obs_dim, it->n_data, m, WhOfMemory{it->d_wh}, *it->d_norm, RingData{ring_rows(it)}, it->d_cand, it->d_pdf, blockIdx.x);
}

// :276-279
static __device__ __forceinline__ float ucb_value(float alpha, float value, float pdf, double num, double buffer_len, double volume) {
    const double c_hat = buffer_len * (double)pdf * volume;              // :276
    return alpha * value + (float)sqrt(num / c_hat);                     // :277-279
}

// single block: ucb + argmax (m <= a few thousand candidates)
__global__ __launch_bounds__(256) void ucb_kernel(int64_t m, const float *__restrict__ value,
                                                  const float *__restrict__ pdf, float alpha, float beta,
                                                  double buffer_len, double volume, float *__restrict__ ucb,
                                                  int32_t *__restrict__ best) {
    __shared__ float rs[4];
    __shared__ int ri[4];
    float bs = -INFINITY;
    int bi = 0x7fffffff;
    const double num = (double)beta * log(buffer_len);
    for (int64_t i = threadIdx.x; i < m; i += 256) {
        const float u = ucb_value(alpha, value[i], pdf[i], num, buffer_len, volume);
        if (ucb != nullptr) ucb[i] = u;
        if (u > bs || (u == bs && (int)i < bi)) { bs = u; bi = (int)i; }
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
        const float os = __shfl_xor(bs, msk);
        const int oi = __shfl_xor(bi, msk);
        if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = bs; ri[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (rs[w] > bs || (rs[w] == bs && ri[w] < bi)) { bs = rs[w]; bi = ri[w]; }
        best[0] = (bi == 0x7fffffff) ? 0 : bi;   // :280 np.argmax
    }
}

// ssc_ucb_topk_many: grid row y = item y, one workgroup.  A live slot's rank is one 64-bit word: the float's bits mapped to
// an unsigned that orders like the float (NaN lowest, -0 = +0), plus one, above the complement of the slot -- the largest
// word is the highest ucb, the lowest slot on ties; 0 marks a slot that is masked or already taken.  Integer compares only.
constexpr int kTopkThreads = 256;
__global__ __launch_bounds__(kTopkThreads) void ucb_topk_many_kernel(const ssc_select_many_item *items) {
    __shared__ unsigned long long rank[4096];
    __shared__ unsigned long long wbest[kTopkThreads / 64];
    const const_select_item it = (const_select_item)items + blockIdx.y;
    const int m = it->n_ss;
    const int64_t count = it->count;
    if (m == 0 || count == 0) return;
    const int n_plans = it->n_plans;
    int32_t *chosen = it->d_chosen;
    if (*it->d_status != 0) {       // no bandwidth, hence no pdf: nothing is chosen
        for (int p = threadIdx.x; p < n_plans; p += kTopkThreads) chosen[p] = -1;
        return;
    }
    const int32_t *idx = it->d_idx;
    const float *value = it->d_value, *pdf = it->d_pdf;
    float *ucb = it->d_ucb;
    const float alpha = it->alpha;
    const double buffer_len = (double)(count < it->ring.capacity ? count : it->ring.capacity), volume = it->volume;
    const double num = (double)it->beta * log(buffer_len);
    for (int i = threadIdx.x; i < m; i += kTopkThreads) {
        unsigned long long r = 0ull;
        float u = __uint_as_float(0x7fc00000u);
        if (idx[i] >= 0) {
            u = ucb_value(alpha, value[i], pdf[i], num, buffer_len, volume);
            uint32_t b = __float_as_uint(u);
            if ((b << 1) == 0u) b = 0u;
            const bool nan = (b & 0x7fffffffu) > 0x7f800000u;
            const uint32_t key = nan ? 0u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
            r = ((unsigned long long)(key + 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
        }
        ucb[i] = u;
        rank[i] = r;
    }
    __syncthreads();
    for (int p = 0; p < n_plans; ++p) {
        unsigned long long best = 0ull;
        for (int i = threadIdx.x; i < m; i += kTopkThreads) best = rank[i] > best ? rank[i] : best;
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            const unsigned long long o = __shfl_xor(best, msk);
            best = o > best ? o : best;
        }
        if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kTopkThreads / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
            if (best == 0ull) {
                chosen[p] = -1;
            } else {
                const uint32_t slot = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull);
                chosen[p] = idx[slot];
                rank[slot] = 0ull;
            }
        }
        __syncthreads();
    }
}

// ssc_kde_scott_bandwidth_many: grid row y = item y, one workgroup.  Two passes over the data set in fp64 -- column means,
// then the upper triangle of sum (x - mean)(x - mean)^T -- every per-thread partial merged in a fixed order (xor-shuffle tree
// in the wave, then the waves in order: no atomics, the same bits run to run), then the d x d algebra on thread 0.
constexpr int kBwThreads = 1024;

static __device__ __forceinline__ double bw_block_sum(double v, double *red) {
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
    __syncthreads();                      // the last sum's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kBwThreads / 64; ++w) s += red[w];
    return s;
}

// lower Cholesky factor of the symmetric d x d matrix a (row-major, stride DS) into l; false: a pivot is non-positive or not finite
constexpr int DS = SSC_MAX_STATE;
static __device__ bool bw_cholesky(const double *a, double *l, int d) {
    for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = a[i * DS + j];
            for (int k = 0; k < j; ++k) v -= l[i * DS + k] * l[j * DS + k];
            if (i == j) {
                if (!(v > 0.0) || isinf(v)) return false;
                l[i * DS + i] = sqrt(v);
            } else {
                l[i * DS + j] = v / l[j * DS + j];
            }
        }
    return true;
}

__global__ __launch_bounds__(kBwThreads) void scott_bandwidth_many_kernel(const ssc_select_many_item *items) {
    __shared__ double red[kBwThreads / 64];
    __shared__ double cov[DS * DS], lo[DS * DS], li[DS * DS], pinv[DS * DS];
    const const_select_item it = (const_select_item)items + blockIdx.y;
    if (it->n_ss == 0 || it->count == 0) return;
    const int d = it->ring.obs_dim;
    const int64_t n = it->n_data;
    if (n < 2) {                                   // workgroup-uniform
        if (threadIdx.x == 0) *it->d_status = 1;
        return;
    }
    const RingRows rows = ring_rows(it);
    double acc[DS];
#pragma unroll
    for (int c = 0; c < DS; ++c) acc[c] = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += kBwThreads) {
        const float *x = rows.row(j);
#pragma unroll
        for (int c = 0; c < DS; ++c)
            if (c < d) acc[c] += (double)x[c];
    }
    double mean[DS];
#pragma unroll
    for (int c = 0; c < DS; ++c) mean[c] = c < d ? bw_block_sum(acc[c], red) / (double)n : 0.0;
    double sq[DS * (DS + 1) / 2];
#pragma unroll
    for (int k = 0; k < DS * (DS + 1) / 2; ++k) sq[k] = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += kBwThreads) {
        const float *x = rows.row(j);
        double dx[DS];
#pragma unroll
        for (int c = 0; c < DS; ++c) dx[c] = c < d ? (double)x[c] - mean[c] : 0.0;
#pragma unroll
        for (int r = 0; r < DS; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c)
                if (r < d) sq[r * (r + 1) / 2 + c] = fma(dx[r], dx[c], sq[r * (r + 1) / 2 + c]);
    }
#pragma unroll
    for (int r = 0; r < DS; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c)
            if (r < d) {                                       // (d is workgroup-uniform: every thread takes the same barriers)
                const double v = bw_block_sum(sq[r * (r + 1) / 2 + c], red);
                if (threadIdx.x == 0) cov[r * DS + c] = cov[c * DS + r] = v / (double)(n - 1) * it->scott;
            }
    if (threadIdx.x != 0) return;
    bool ok = bw_cholesky(cov, lo, d);
    double det = 1.0;
    if (ok) {
        // li = lo^-1 (lower), pinv = inv(cov) = li^T li
        for (int i = 0; i < d; ++i) {
            li[i * DS + i] = 1.0 / lo[i * DS + i];
            det *= 2.0 * 3.14159265358979323846 * lo[i * DS + i] * lo[i * DS + i];
            for (int j = 0; j < i; ++j) {
                double v = 0.0;
                for (int k = j; k < i; ++k) v -= lo[i * DS + k] * li[k * DS + j];
                li[i * DS + j] = v / lo[i * DS + i];
            }
        }
        for (int i = 0; i < d; ++i)
            for (int j = 0; j <= i; ++j) {
                double v = 0.0;
                for (int k = i; k < d; ++k) v += li[k * DS + i] * li[k * DS + j];
                pinv[i * DS + j] = pinv[j * DS + i] = v;
            }
        ok = bw_cholesky(pinv, lo, d);          // lo: now the lower factor of inv(cov); the whitening matrix is its transpose
    }
    if (ok) {
        for (int r = 0; r < d; ++r)
            for (int c = 0; c < d; ++c) it->d_wh[r * d + c] = c >= r ? (float)lo[c * DS + r] : 0.0f;
        *it->d_norm = 1.0 / ((double)n * sqrt(det));
    }
    *it->d_status = ok ? 0 : 1;
}

}  // namespace ssc

using namespace ssc;

template <class... Rms>
static int critic_forward(const ssc_critic_desc *c, int64_t m, const float *d_obs, const float *d_act, float *d_q,
                          ssc_stream_t stream, Rms... rms) {
    SSC_REQUIRE(c != nullptr, "ssc_critic_forward: critic NULL");
    SSC_REQUIRE(m >= 0, "ssc_critic_forward: m < 0");
    SSC_REQUIRE(c->obs_dim >= 1 && c->obs_dim <= SSC_MAX_STATE && c->act_dim >= 1 && c->act_dim <= SSC_MAX_ACT,
                "ssc_critic_forward: obs_dim %d / act_dim %d out of range", c->obs_dim, c->act_dim);
    SSC_REQUIRE(c->h1 >= 1 && c->h2 >= 1 && c->h1 + c->act_dim <= 600, "ssc_critic_forward: bad hidden sizes");
    if (m == 0) return SSC_OK;
    SSC_REQUIRE(c->W1 && c->b1 && c->W2 && c->b2 && c->W3 && c->b3 && d_obs && d_act && d_q,
                "ssc_critic_forward: NULL device pointer");
    const CriticW w{c->W1, c->b1, c->W2, c->b2, c->W3, c->b3, c->obs_dim, c->act_dim, c->h1, c->h2, c->last_layer_tanh, c->obs_clip,
                    c->ln1_g, c->ln1_b, c->ln2_g, c->ln2_b};
    const bool ln = c->ln1_g != nullptr;
    SSC_REQUIRE(ln == (c->ln1_b != nullptr) && ln == (c->ln2_g != nullptr) && ln == (c->ln2_b != nullptr),
                "ssc_critic_forward: the four LayerNorm pointers come together");
    const size_t lds = (size_t)(c->h1 + c->act_dim + (ln ? c->h2 : 0)) * 64 * sizeof(float);
    if (lds > 160 * 1024) return set_error(SSC_EUNSUPPORTED, "ssc_critic_forward: h1 %d + h2 %d too wide for the LayerNorm kernel", c->h1, c->h2);
    if (lds > 64 * 1024) {
        int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(critic_kernel<Rms...>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute(critic_kernel)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(critic_kernel<Rms...>, dim3(blocks_for(m, 64)), dim3(64), lds, as_stream(stream), w, m, d_obs, d_act,
                       d_q, rms...);
    return check_launch("ssc_critic_forward");
}

extern "C" {

int ssc_critic_forward(const ssc_critic_desc *c, int64_t m, const float *d_obs, const float *d_act, float *d_q,
                       ssc_stream_t stream) {
    return critic_forward(c, m, d_obs, d_act, d_q, stream);
}

// normalize_observations: Q of clip((obs - mean) / std) with the RunningMeanStd block d_rms (actor_device.h)
int ssc_critic_forward_rms(const ssc_critic_desc *c, int64_t m, const float *d_obs, const float *d_act, float *d_q,
                           ssc_stream_t stream, const double *d_rms) {
    if (d_rms == nullptr) return critic_forward(c, m, d_obs, d_act, d_q, stream);
    return critic_forward(c, m, d_obs, d_act, d_q, stream, d_rms);
}


int ssc_kde_evaluate(int32_t d, int64_t n, const float *d_data, int64_t m, const float *d_points,
                     const float *whitening, double norm, float *d_pdf, ssc_stream_t stream) {
    SSC_REQUIRE(d >= 1 && d <= SSC_MAX_STATE, "ssc_kde_evaluate: d = %d out of range", d);
    SSC_REQUIRE(n >= 1 && m >= 0, "ssc_kde_evaluate: need n >= 1, m >= 0");
    SSC_REQUIRE(whitening != nullptr, "ssc_kde_evaluate: whitening NULL");
    if (m == 0) return SSC_OK;
    SSC_REQUIRE(d_data && d_points && d_pdf, "ssc_kde_evaluate: NULL device pointer");
    KdeArgs a{};
    a.d = d; a.n = n; a.m = m; a.norm = norm;
    for (int i = 0; i < d * d; ++i) a.wh[i] = whitening[i];
    const dim3 grid(blocks_for(m, kKdeQ)), block(kKdeThreads);
    hipStream_t s = as_stream(stream);
    if (d == 1) hipLaunchKernelGGL(kde_kernel<1>, grid, block, 0, s, a, d_data, d_points, d_pdf);
    else if (d == 2) hipLaunchKernelGGL(kde_kernel<2>, grid, block, 0, s, a, d_data, d_points, d_pdf);
    else if (d == 3) hipLaunchKernelGGL(kde_kernel<3>, grid, block, 0, s, a, d_data, d_points, d_pdf);
    else hipLaunchKernelGGL(kde_kernel<0>, grid, block, 0, s, a, d_data, d_points, d_pdf);
    return check_launch("ssc_kde_evaluate");
}

// ssc_critic_forward's per-descriptor checks with its codes, `who` in front
static int check_critic(const char *who, const ssc_critic_desc *c, size_t *lds_out) {
    SSC_REQUIRE(c->obs_dim >= 1 && c->obs_dim <= SSC_MAX_STATE && c->act_dim >= 1 && c->act_dim <= SSC_MAX_ACT,
                "%s: obs_dim %d / act_dim %d out of range", who, c->obs_dim, c->act_dim);
    SSC_REQUIRE(c->h1 >= 1 && c->h2 >= 1 && c->h1 + c->act_dim <= 600, "%s: bad hidden sizes", who);
    SSC_REQUIRE(c->W1 && c->b1 && c->W2 && c->b2 && c->W3 && c->b3, "%s: NULL device pointer", who);
    const bool ln = c->ln1_g != nullptr;
    SSC_REQUIRE(ln == (c->ln1_b != nullptr) && ln == (c->ln2_g != nullptr) && ln == (c->ln2_b != nullptr),
                "%s: the four LayerNorm pointers come together", who);
    const size_t lds = (size_t)(c->h1 + c->act_dim + (ln ? c->h2 : 0)) * 64 * sizeof(float);
    if (lds > 160 * 1024) return set_error(SSC_EUNSUPPORTED, "%s: h1 %d + h2 %d too wide for the LayerNorm kernel", who, c->h1, c->h2);
    *lds_out = lds;
    return SSC_OK;
}

int ssc_critic_forward_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items, int64_t m,
                            const float *d_act, ssc_stream_t stream) {
    const char *fn = "ssc_critic_forward_many";
    if (int rc = select_table_check(fn, h_items, d_items, n_items)) return rc;
    SSC_REQUIRE(m >= 0, "%s: m = %lld < 0", fn, (long long)m);
    size_t lds_max = 0;
    int64_t rows_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const ssc_select_many_item &it = h_items[i];
        char who[72];
        if (int rc = select_item_check(fn, i, it, who)) return rc;
        if (select_item_empty(it)) continue;
        size_t lds = 0;
        if (int rc = check_critic(who, &it.critic, &lds)) return rc;
        SSC_REQUIRE(it.critic.obs_dim == it.ring.obs_dim, "%s: critic obs_dim %d, ring obs_dim %d", who, it.critic.obs_dim,
                    it.ring.obs_dim);
        SSC_REQUIRE(it.row0 >= 0 && it.row0 <= m && it.n_ss <= m - it.row0, "%s: rows [%lld, %lld + %d) outside [0, %lld)", who,
                    (long long)it.row0, (long long)it.row0, it.n_ss, (long long)m);
        SSC_REQUIRE(it.d_cand && it.d_value, "%s: NULL device pointer", who);
        lds_max = std::max(lds_max, lds);
        rows_max = std::max(rows_max, (int64_t)it.n_ss);
    }
    if (rows_max == 0) return SSC_OK;
    SSC_REQUIRE(d_act != nullptr, "%s: d_act NULL", fn);
    if (lds_max > 64 * 1024)
        if (int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(critic_many_kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max),
                               "hipFuncSetAttribute(critic_many_kernel)"))
            return rc;
    hipLaunchKernelGGL(critic_many_kernel, dim3(blocks_for(rows_max, 64), (unsigned)n_items), dim3(64), lds_max, as_stream(stream),
                       d_items, d_act);
    return check_launch(fn);
}

int ssc_kde_scott_bandwidth_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items,
                                 ssc_stream_t stream) {
    const char *fn = "ssc_kde_scott_bandwidth_many";
    if (int rc = select_table_check(fn, h_items, d_items, n_items)) return rc;
    bool work = false;
    for (int i = 0; i < n_items; ++i) {
        const ssc_select_many_item &it = h_items[i];
        char who[72];
        if (int rc = select_item_check(fn, i, it, who)) return rc;
        if (select_item_empty(it)) continue;
        const int64_t size = select_item_size(it);
        SSC_REQUIRE(it.stride >= 1 && it.n_data == (size + it.stride) / it.stride, "%s: stride %lld / n_data %lld for %lld + 1 states",
                    who, (long long)it.stride, (long long)it.n_data, (long long)size);
        SSC_REQUIRE(it.scott > 0.0 && it.scott <= 1.7976931348623157e308, "%s: scott factor %g", who, it.scott);
        SSC_REQUIRE(it.ring.s && it.ring.s2 && it.d_wh && it.d_norm && it.d_status, "%s: NULL device pointer", who);
        work = true;
    }
    if (!work) return SSC_OK;
    hipLaunchKernelGGL(scott_bandwidth_many_kernel, dim3(1, (unsigned)n_items), dim3(kBwThreads), 0, as_stream(stream), d_items);
    return check_launch(fn);
}

int ssc_kde_evaluate_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items,
                          ssc_stream_t stream) {
    const char *fn = "ssc_kde_evaluate_many";
    if (int rc = select_table_check(fn, h_items, d_items, n_items)) return rc;
    int d = 0, d_item = -1;
    int64_t m_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const ssc_select_many_item &it = h_items[i];
        char who[72];
        if (int rc = select_item_check(fn, i, it, who)) return rc;
        if (select_item_empty(it)) continue;
        const int64_t size = select_item_size(it);
        SSC_REQUIRE(it.stride >= 1 && it.n_data == (size + it.stride) / it.stride, "%s: stride %lld / n_data %lld for %lld + 1 states",
                    who, (long long)it.stride, (long long)it.n_data, (long long)size);
        SSC_REQUIRE(it.ring.s && it.ring.s2 && it.d_cand && it.d_wh && it.d_norm && it.d_status && it.d_pdf, "%s: NULL device pointer",
                    who);
        if (d_item < 0) { d = it.ring.obs_dim; d_item = i; }
        if (it.ring.obs_dim != d)
            return set_error(SSC_EUNSUPPORTED, "%s: items %d and %d have obs_dim %d and %d: one call serves one obs_dim", fn, d_item, i, d,
                             it.ring.obs_dim);
        m_max = std::max(m_max, (int64_t)it.n_ss);
    }
    if (m_max == 0) return SSC_OK;
    const dim3 grid(blocks_for(m_max, kKdeQ), (unsigned)n_items), block(kKdeThreads);
    hipStream_t s = as_stream(stream);
    if (d == 1) hipLaunchKernelGGL(kde_many_kernel<1>, grid, block, 0, s, d_items);
    else if (d == 2) hipLaunchKernelGGL(kde_many_kernel<2>, grid, block, 0, s, d_items);
    else if (d == 3) hipLaunchKernelGGL(kde_many_kernel<3>, grid, block, 0, s, d_items);
    else hipLaunchKernelGGL(kde_many_kernel<0>, grid, block, 0, s, d_items);
    return check_launch(fn);
}

int ssc_ucb_topk_many(const ssc_select_many_item *h_items, const ssc_select_many_item *d_items, int32_t n_items, ssc_stream_t stream) {
    const char *fn = "ssc_ucb_topk_many";
    if (int rc = select_table_check(fn, h_items, d_items, n_items)) return rc;
    bool work = false;
    for (int i = 0; i < n_items; ++i) {
        const ssc_select_many_item &it = h_items[i];
        char who[72];
        if (int rc = select_item_check(fn, i, it, who)) return rc;
        if (select_item_empty(it)) continue;
        SSC_REQUIRE(it.n_plans >= 1 && it.n_plans <= 64, "%s: n_plans %d not in 1..64", who, it.n_plans);
        SSC_REQUIRE(it.volume > 0.0, "%s: volume %g", who, it.volume);
        SSC_REQUIRE(it.d_idx && it.d_value && it.d_pdf && it.d_ucb && it.d_chosen && it.d_status, "%s: NULL device pointer", who);
        work = true;
    }
    if (!work) return SSC_OK;
    hipLaunchKernelGGL(ucb_topk_many_kernel, dim3(1, (unsigned)n_items), dim3(kTopkThreads), 0, as_stream(stream), d_items);
    return check_launch(fn);
}

int ssc_ucb_argmax(int64_t m, const float *d_value, const float *d_pdf, float alpha, float beta, double buffer_len,
                   double volume, float *d_ucb, int32_t *d_best, ssc_stream_t stream) {
    SSC_REQUIRE(m >= 1, "ssc_ucb_argmax: m < 1");
    SSC_REQUIRE(buffer_len >= 1.0 && volume > 0.0, "ssc_ucb_argmax: bad buffer_len / volume");
    SSC_REQUIRE(d_value && d_pdf && d_best, "ssc_ucb_argmax: NULL device pointer");
    hipLaunchKernelGGL(ucb_kernel, dim3(1), dim3(256), 0, as_stream(stream), m, d_value, d_pdf, alpha, beta, buffer_len,
                       volume, d_ucb, d_best);
    return check_launch("ssc_ucb_argmax");
}

}  // extern "C"
