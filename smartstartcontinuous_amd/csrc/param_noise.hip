// param_noise.hip -- adaptive parameter-space noise of DDPG (ddpg_editted.py:47-60, 151-166, 360-385) on flat
// parameter arrays [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3]:
//
//   ssc_param_noise_perturb   dst = src + stddev * N(0,1) outside the skip ranges (the LayerNorm segments, which
//                             models_editted.py:18-19 keeps out of perturbable_vars), a bit copy inside them.
//   ssc_param_noise_adapt     distance = sqrt(mean((a - b)^2)) of two action batches, then baselines 0.1.5
//                             AdaptiveParamNoiseSpec.adapt on the device stddev.
//
//   ssc_param_noise_cycle     one adaption interval in ONE launch: perturb the adaptive copy (it lives in LDS only), both
//                             actor forwards on a batch of obs0, adapt, perturb the acting copy with the new stddev.
//   ssc_param_noise_cycle_many  that interval for a population of agents in one launch, workgroup p = pair p, the batch
//                             gathered out of the pair's replay ring by row indices; m == 0: perturb only.
//
// All read stddev from device memory, so a loop adapts and re-perturbs without the host.  A few thousand elements
// each: the cost is the launch.
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "actor_device.h"
#include "ssc_host.h"

namespace ssc {

namespace {

// stream tag of the parameter noise (the oracle's keying: rng_words(seed, q, generation, 9)).  It lives here, next to its
// only user, like TAG_DATA_NOISE in dataset.hip: ssc_device.h is part of the rollout kernel's profiled sources.
enum : uint32_t { TAG_PARAM_NOISE = 9 };

constexpr int kAdaptThreads = 256;

// element i = 4q + j of the stream: src + stddev * g, or the bits of src inside a skip range and when stddev is 0
// (x + 0 * g would turn -0.0 into +0.0)
__device__ __forceinline__ float perturbed(float x, bool skip, float sd, const u32x4 &w, int j) {
    const float g = gaussian_f32(j < 2 ? w.x : w.z, j < 2 ? w.y : w.w, (j & 1) != 0);
    return (skip || sd == 0.0f) ? x : fmaf(sd, g, x);
}

// Thread q serves elements 4q .. 4q+3 with ONE Philox evaluation keyed by the flat index alone (counter q, generation):
// words (x, y) -> Box-Muller pair (cos -> 4q, sin -> 4q+1), words (z, w) -> (4q+2, 4q+3).  No __restrict__: in place
// (src == dst) is allowed, every thread reads and writes only its own four elements.
__global__ __launch_bounds__(kBlock) void param_noise_perturb_kernel(int64_t n, const float *src, float *dst,
                                                                      const float *__restrict__ d_stddev, int64_t s0b,
                                                                      int64_t s0e, int64_t s1b, int64_t s1e, uint64_t seed,
                                                                      uint64_t generation) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i0 = q * 4;
    if (i0 >= n) return;
    const float sd = *d_stddev;
    const u32x4 w = rng_words(seed, (uint64_t)q, generation, TAG_PARAM_NOISE);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) break;
        const float x = src[i];
        const bool skip = (i >= s0b && i < s0e) || (i >= s1b && i < s1e);
        dst[i] = perturbed(x, skip, sd, w, j);
    }
}

// One workgroup, fixed order: every thread sums its strided share in f64, the waves reduce by xor shuffles, thread 0
// adds the wave sums in wave order.  The same bits run to run.
__global__ __launch_bounds__(kAdaptThreads) void param_noise_adapt_kernel(int32_t count, const float *__restrict__ a,
                                                                          const float *__restrict__ b, float desired,
                                                                          float coefficient, float *__restrict__ d_stddev,
                                                                          float *__restrict__ d_distance) {
    __shared__ double red[kAdaptThreads / 64];
    double v = 0.0;
    for (int32_t i = threadIdx.x; i < count; i += kAdaptThreads) {
        const double d = (double)a[i] - (double)b[i];
        v = fma(d, d, v);
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
#pragma unroll
        for (int w = 1; w < kAdaptThreads / 64; ++w) s += red[w];
        const float distance = (float)sqrt(s / (double)count);
        *d_distance = distance;
        // AdaptiveParamNoiseSpec.adapt: a tie multiplies
        const float sd = *d_stddev;
        *d_stddev = distance > desired ? sd / coefficient : sd * coefficient;
    }
}

bool range_ok(int64_t b, int64_t e, int64_t n) { return b >= 0 && b <= e && e <= n; }

// ---------------------------------------------------------------------------------------
// ssc_param_noise_cycle / ssc_param_noise_cycle_many: ONE workgroup of 1024 threads per agent.
//
// LDS (all dynamic, every carve a multiple of 16 B):
//   ad   [n4]                      the adaptive copy: src + stddev * N(0, 1), flat layout of src
//   pl   [n4]                      kStagePlain only: the plain parameters as well (when both copies and a 128-row tile fit,
//                                  e.g. 64-32: the weight reads of the inner loops are then LDS reads for both networks;
//                                  worth 2 us of 89 at 1024 rows -- the loops are bound by LDS read cycles, NOTEBOOK 14)
//   obs  [obs_dim][TR]             the tile's network inputs (normalised / clipped once for both networks)
//   hA   [2][TR/4][h1 + 1][4]      layer-1 activations of the plain (0) and the adaptive (1) network: four rows of one unit
//   hB   [2][TR/4][h2 + 1][4]      side by side (one 16-byte broadcast read feeds four FMAs); the "+ 1" pads a row group by
//                                  four banks so that per-row walks (LayerNorm statistics, layer 3) are conflict-free
//   st   [2][2][TR]                LayerNorm mean / rstd per row
//   red  [16] f64 + the new stddev
// A tile is TR rows (4 .. 128, chosen by cycle_carve: the largest that fits beside the copy).  Work items are
// (row group of 4, output unit) with the unit fastest, so the weight reads of a wave are consecutive floats -- global
// loads for the plain network, LDS reads for the adaptive one -- and BOTH networks run in one item: eight independent FMA
// chains per thread.  Every output unit sums its inputs in index order with fused multiply-adds, like
// actor_generic_kernel / actor_row_kernel.
// ---------------------------------------------------------------------------------------
constexpr int kCycleThreads = 1024;
constexpr int kCycleMaxTile = 128;
constexpr size_t kLdsBytes = 160 * 1024;
constexpr int kCycleMaxRows = 4096;

#define SSC_GLOBAL __attribute__((address_space(1)))

struct CycleNet {                       // offsets into the flat array, in floats
    int32_t W1, b1, W2, b2, W3, b3;
    int32_t g1, be1, g2, be2;           // LayerNorm gamma / beta; g1 < 0: none
    int32_t obs_dim, h1, h2, act_dim, last_tanh;
    float obs_clip;
};

// LDS carve of the workgroup, in floats
struct CycleCarve {
    int32_t copies, tile_rows;          // 2: the plain parameters are staged beside the adaptive copy
    int32_t off_obs, off_hA, off_hB, off_st, off_red;
    int64_t floats;
};

SSC_HD CycleCarve cycle_carve_at(int n4, int copies, int tr, int obs_dim, int h1, int h2) {
    CycleCarve c{};
    c.copies = copies, c.tile_rows = tr;
    int64_t p = (int64_t)copies * n4;
    c.off_obs = (int32_t)p; p += (int64_t)tr * obs_dim;
    c.off_hA = (int32_t)p;  p += 2 * (int64_t)(tr / 4) * (4 * (h1 + 1));
    c.off_hB = (int32_t)p;  p += 2 * (int64_t)(tr / 4) * (4 * (h2 + 1));
    c.off_st = (int32_t)p;  p += 4 * (int64_t)tr;
    c.off_red = (int32_t)p; p += 2 * 16 + 4;
    c.floats = p;
    return c;
}

// ONE function of (parameter count, batch rows, shape) for the host -- launch size, staging decision -- and for a workgroup
// of the population launch (its own pair's offsets).  stage: 1 both copies, 0 the adaptive copy only, < 0: both iff they
// fit beside a 128-row tile.  The tile is the largest that fits beside the copies and no larger than the batch needs
// (4 rows at least: floats * 4 may still exceed LDS, which the host refuses).  A pair that fits both copies gets the same
// tile with one or two, so the tile -- and with it the summation order of the distance -- does not depend on `stage`.
SSC_HD CycleCarve cycle_carve(int n4, int m, int obs_dim, int h1, int h2, int stage) {
    if (stage < 0) stage = (size_t)cycle_carve_at(n4, 2, kCycleMaxTile, obs_dim, h1, h2).floats * sizeof(float) <= kLdsBytes;
    const int copies = stage ? 2 : 1;
    int tr = kCycleMaxTile;
    while (tr > 4 && ((size_t)cycle_carve_at(n4, copies, tr, obs_dim, h1, h2).floats * sizeof(float) > kLdsBytes || tr / 2 >= m)) tr /= 2;
    return cycle_carve_at(n4, copies, tr, obs_dim, h1, h2);
}

struct CycleArgs {
    CycleNet net;
    int32_t m, n, n4;                   // m == 0: perturb only
    CycleCarve lds;
    const float *obs;
    const int32_t *idx;                 // null: rows 0 .. m-1 of obs
    const double *rms;
    const float *src;
    float *dst;
    int64_t s0b, s0e, s1b, s1e;
    uint64_t seed, gen_adaptive, gen_acting;
    float desired, coefficient;
    float *d_stddev, *d_distance;
};

// offset of a parameter segment of `count` floats inside the flat array, or -1 when it does not lie inside it
// (this maps the CALLER's pointers back to offsets, whatever order they come in; the flat layout the learners write --
// [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3] -- is defined in ddpg_layout.h)
SSC_HD int32_t segment(const float *p, int64_t count, const float *src, int64_t n) {
    if (p == nullptr || p < src) return -1;
    const int64_t off = p - src;
    return (off + count <= n) ? (int32_t)off : -1;
}

// The kernel arguments of one agent: the host packs them into the kernarg of the single launch (and checks every pair's
// with it), a workgroup of the population launch forms them from its pair's item and cursor.  false: a parameter segment
// outside d_src[0 .. n), or LayerNorm pointers that do not come together.
SSC_HD bool pack_cycle(CycleArgs &a, const ssc_actor_desc &actor, int32_t m, const float *obs, const int32_t *idx, const double *rms,
                       int64_t n, const float *src, int64_t s0b, int64_t s0e, int64_t s1b, int64_t s1e, uint64_t seed,
                       uint64_t gen_adaptive, uint64_t gen_acting, float desired, float coefficient, float *d_stddev,
                       float *d_distance, float *dst, int stage) {
    CycleNet &nt = a.net;
    const int64_t h1 = actor.h1, h2 = actor.h2;
    nt.W1 = segment(actor.W1, actor.obs_dim * h1, src, n);
    nt.b1 = segment(actor.b1, h1, src, n);
    nt.W2 = segment(actor.W2, h1 * h2, src, n);
    nt.b2 = segment(actor.b2, h2, src, n);
    nt.W3 = segment(actor.W3, h2 * actor.act_dim, src, n);
    nt.b3 = segment(actor.b3, actor.act_dim, src, n);
    bool inside = nt.W1 >= 0 && nt.b1 >= 0 && nt.W2 >= 0 && nt.b2 >= 0 && nt.W3 >= 0 && nt.b3 >= 0;
    const bool ln = actor.ln1_g != nullptr;
    const bool together = ln == (actor.ln1_b != nullptr) && ln == (actor.ln2_g != nullptr) && ln == (actor.ln2_b != nullptr);
    nt.g1 = nt.be1 = nt.g2 = nt.be2 = -1;
    if (ln && together) {
        nt.g1 = segment(actor.ln1_g, h1, src, n);
        nt.be1 = segment(actor.ln1_b, h1, src, n);
        nt.g2 = segment(actor.ln2_g, h2, src, n);
        nt.be2 = segment(actor.ln2_b, h2, src, n);
        inside = inside && nt.g1 >= 0 && nt.be1 >= 0 && nt.g2 >= 0 && nt.be2 >= 0;
    }
    nt.obs_dim = actor.obs_dim, nt.h1 = actor.h1, nt.h2 = actor.h2, nt.act_dim = actor.act_dim;
    nt.last_tanh = actor.last_layer_tanh, nt.obs_clip = actor.obs_clip;
    a.m = m, a.n = (int32_t)n, a.n4 = (int32_t)((n + 3) / 4 * 4);
    a.lds = cycle_carve(a.n4, m, nt.obs_dim, nt.h1, nt.h2, stage);
    a.obs = obs, a.idx = idx, a.rms = rms, a.src = src, a.dst = dst;
    a.s0b = s0b, a.s0e = s0e, a.s1b = s1b, a.s1e = s1e;
    a.seed = seed, a.gen_adaptive = gen_adaptive, a.gen_acting = gen_acting;
    a.desired = desired, a.coefficient = coefficient, a.d_stddev = d_stddev, a.d_distance = d_distance;
    return inside && together;
}

typedef float cyc_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float hidden_act(float x, int last_tanh) { return last_tanh ? tanh_fast(x) : fmaxf(x, 0.0f); }

// out = src + sd * g(generation) for the workgroup, as param_noise_perturb_kernel writes it: thread q of the stream serves
// elements 4q .. 4q+3.  OUT: an LDS array (the adaptive copy) or the destination in global memory.
template <class SRC, class OUT>
__device__ __forceinline__ void cycle_perturb(const CycleArgs &a, SRC src, OUT out, float sd, uint64_t generation) {
    for (int q = threadIdx.x; 4 * q < a.n; q += kCycleThreads) {
        const u32x4 w = rng_words(a.seed, (uint64_t)q, generation, TAG_PARAM_NOISE);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * q + j;
            if (i >= a.n) break;
            const bool skip = (i >= a.s0b && i < a.s0e) || (i >= a.s1b && i < a.s1e);
            out[i] = perturbed(src[i], skip, sd, w, j);
        }
    }
}

// One adaption interval of one agent, by ONE workgroup: the whole of param_noise_cycle_kernel (arguments in the kernarg)
// and of a workgroup of param_noise_cycle_many_kernel (arguments formed from its pair's item and cursor); by value, as
// rollout_body takes its arguments.  kGlobal: src, dst, obs and idx are read through address-space-1 pointers -- read out
// of an item they are generic to the compiler, which would go through them with FLAT instructions.
template <bool kStagePlain, bool kGlobal>
__device__ __forceinline__ void cycle_body(const CycleArgs a) {
    using GF = std::conditional_t<kGlobal, const SSC_GLOBAL float *, const float *>;
    using GW = std::conditional_t<kGlobal, SSC_GLOBAL float *, float *>;
    using GI = std::conditional_t<kGlobal, const SSC_GLOBAL int32_t *, const int32_t *>;
    using PL = std::conditional_t<kStagePlain, const float *, GF>;   // what the plain network reads
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const GF gsrc = (GF)a.src;
    const GW gdst = (GW)a.dst;
    const float sd0 = *a.d_stddev;
    // perturb only (the ring holds no batch yet): ssc_param_noise_perturb with the stddev as it stands; m is
    // workgroup-uniform, the workgroup leaves as a whole before any barrier
    if (a.m == 0) {
        cycle_perturb(a, gsrc, gdst, sd0, a.gen_acting);
        return;
    }
    const GF gobs = (GF)a.obs;
    const GI gidx = (GI)a.idx;
    const CycleNet &nt = a.net;
    const int TR = a.lds.tile_rows, G = TR / 4, od = nt.obs_dim, h1 = nt.h1, h2 = nt.h2, na = nt.act_dim;
    const int sA = 4 * (h1 + 1), sB = 4 * (h2 + 1);   // floats per row group
    float *ad = smem;
    float *obsS = smem + a.lds.off_obs;
    float *hA = smem + a.lds.off_hA;
    float *hB = smem + a.lds.off_hB;
    float *st = smem + a.lds.off_st;
    double *red = reinterpret_cast<double *>(smem + a.lds.off_red);
    float *new_sd = reinterpret_cast<float *>(red + 16);
    const bool ln = nt.g1 >= 0;
    PL src;
    if constexpr (kStagePlain) {
        float *pl = ad + a.n4;
        for (int i = tid; i < a.n; i += kCycleThreads) pl[i] = gsrc[i];
        src = pl;
    } else {
        src = gsrc;
    }

    // 1. the adaptive copy, generation_adaptive, the stddev as it stands
    cycle_perturb(a, gsrc, ad, sd0, a.gen_adaptive);

    // 2. a = actor(obs), b = adaptive_actor(obs), tile by tile; thread t owns element (row t / act_dim, t % act_dim) of
    //    every tile and sums its squared differences in tile order
    double v = 0.0;
    for (int row0 = 0; row0 < a.m; row0 += TR) {
        if (tid < TR) {
            const int rb = min(row0 + tid, a.m - 1);             // rows past m repeat the last one and are not summed
            const int64_t r = gidx != nullptr ? (int64_t)gidx[rb] : (int64_t)rb;   // gathered out of the ring's state column
            if (a.rms != nullptr) {
                ObsNorm<SSC_MAX_STATE> nrm;
                nrm.load(a.rms, od);
#pragma unroll
                for (int c = 0; c < SSC_MAX_STATE; ++c)
                    if (c < od) obsS[c * TR + tid] = nrm.apply(gobs[r * od + c], c, nt.obs_clip);
            } else {
#pragma unroll
                for (int c = 0; c < SSC_MAX_STATE; ++c)
                    if (c < od) obsS[c * TR + tid] = clip_obs(gobs[r * od + c], nt.obs_clip);
            }
        }
        __syncthreads();                                         // (the first one also publishes the adaptive copy)
        for (int it = tid; it < G * h1; it += kCycleThreads) {
            const int rg = it / h1, j = it - rg * h1;
            const float bp = src[nt.b1 + j], ba = ad[nt.b1 + j];
            cyc_f4 p = {bp, bp, bp, bp}, q = {ba, ba, ba, ba};
            for (int c = 0; c < od; ++c) {
                const cyc_f4 o = *reinterpret_cast<const cyc_f4 *>(obsS + c * TR + 4 * rg);
                const float wp = src[nt.W1 + c * h1 + j], wa = ad[nt.W1 + c * h1 + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    p[e] = fmaf(o[e], wp, p[e]);
                    q[e] = fmaf(o[e], wa, q[e]);
                }
            }
            if (!ln) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    p[e] = fmaxf(p[e], 0.0f);
                    q[e] = fmaxf(q[e], 0.0f);
                }
            }
            *reinterpret_cast<cyc_f4 *>(hA + rg * sA + 4 * j) = p;
            *reinterpret_cast<cyc_f4 *>(hA + (G + rg) * sA + 4 * j) = q;
        }
        __syncthreads();
        if (ln) {
            if (tid < 2 * TR) {
                const int net = tid / TR, r = tid - net * TR;
                float mean, rstd;
                layer_norm_stats(hA + (net * G + (r >> 2)) * sA + (r & 3), h1, 4, mean, rstd);
                st[(2 * net) * TR + r] = mean;
                st[(2 * net + 1) * TR + r] = rstd;
            }
            __syncthreads();
            for (int it = tid; it < 2 * G * h1; it += kCycleThreads) {
                const int nrg = it / h1, j = it - nrg * h1, net = nrg / G, rg = nrg - net * G;
                const float g = net ? ad[nt.g1 + j] : src[nt.g1 + j], be = net ? ad[nt.be1 + j] : src[nt.be1 + j];
                cyc_f4 x = *reinterpret_cast<const cyc_f4 *>(hA + nrg * sA + 4 * j);
                const cyc_f4 mean = *reinterpret_cast<const cyc_f4 *>(st + (2 * net) * TR + 4 * rg);
                const cyc_f4 rstd = *reinterpret_cast<const cyc_f4 *>(st + (2 * net + 1) * TR + 4 * rg);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = fmaxf(fmaf((x[e] - mean[e]) * rstd[e], g, be), 0.0f);
                *reinterpret_cast<cyc_f4 *>(hA + nrg * sA + 4 * j) = x;
            }
            __syncthreads();
        }
        for (int it = tid; it < G * h2; it += kCycleThreads) {
            const int rg = it / h2, j = it - rg * h2;
            const float bp = src[nt.b2 + j], ba = ad[nt.b2 + j];
            cyc_f4 p = {bp, bp, bp, bp}, q = {ba, ba, ba, ba};
            const float *xp = hA + rg * sA, *xa = hA + (G + rg) * sA;
            const PL wp = src + nt.W2 + j;
            const float *wa = ad + nt.W2 + j;
#pragma unroll 4
            for (int k = 0; k < h1; ++k) {
                const cyc_f4 hp = *reinterpret_cast<const cyc_f4 *>(xp + 4 * k);
                const cyc_f4 ha = *reinterpret_cast<const cyc_f4 *>(xa + 4 * k);
                const float w0 = wp[k * h2], w1 = wa[k * h2];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    p[e] = fmaf(hp[e], w0, p[e]);
                    q[e] = fmaf(ha[e], w1, q[e]);
                }
            }
            if (!ln) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    p[e] = hidden_act(p[e], nt.last_tanh);
                    q[e] = hidden_act(q[e], nt.last_tanh);
                }
            }
            *reinterpret_cast<cyc_f4 *>(hB + rg * sB + 4 * j) = p;
            *reinterpret_cast<cyc_f4 *>(hB + (G + rg) * sB + 4 * j) = q;
        }
        __syncthreads();
        if (ln) {
            if (tid < 2 * TR) {
                const int net = tid / TR, r = tid - net * TR;
                float mean, rstd;
                layer_norm_stats(hB + (net * G + (r >> 2)) * sB + (r & 3), h2, 4, mean, rstd);
                st[(2 * net) * TR + r] = mean;
                st[(2 * net + 1) * TR + r] = rstd;
            }
            __syncthreads();
            for (int it = tid; it < 2 * G * h2; it += kCycleThreads) {
                const int nrg = it / h2, j = it - nrg * h2, net = nrg / G, rg = nrg - net * G;
                const float g = net ? ad[nt.g2 + j] : src[nt.g2 + j], be = net ? ad[nt.be2 + j] : src[nt.be2 + j];
                cyc_f4 x = *reinterpret_cast<const cyc_f4 *>(hB + nrg * sB + 4 * j);
                const cyc_f4 mean = *reinterpret_cast<const cyc_f4 *>(st + (2 * net) * TR + 4 * rg);
                const cyc_f4 rstd = *reinterpret_cast<const cyc_f4 *>(st + (2 * net + 1) * TR + 4 * rg);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = hidden_act(fmaf((x[e] - mean[e]) * rstd[e], g, be), nt.last_tanh);
                *reinterpret_cast<cyc_f4 *>(hB + nrg * sB + 4 * j) = x;
            }
            __syncthreads();
        }
        if (tid < TR * na) {
            const int r = tid / na, c = tid - r * na;
            const float *xp = hB + (r >> 2) * sB + (r & 3), *xa = hB + (G + (r >> 2)) * sB + (r & 3);
            float op = src[nt.b3 + c], oa = ad[nt.b3 + c];
            for (int j = 0; j < h2; ++j) {
                op = fmaf(xp[4 * j], src[nt.W3 + j * na + c], op);
                oa = fmaf(xa[4 * j], ad[nt.W3 + j * na + c], oa);
            }
            if (row0 + r < a.m) {
                const double d = (double)tanh_fast(op) - (double)tanh_fast(oa);
                v = fma(d, d, v);
            }
        }
        // no barrier here: the next tile's staging writes obs only, and two barriers lie in front of its first write to
        // hA / hB
    }

    // 3. distance and the adapted stddev: the reduction of param_noise_adapt_kernel
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
#pragma unroll
        for (int w = 1; w < kCycleThreads / 64; ++w) s += red[w];
        const float distance = (float)sqrt(s / ((double)a.m * (double)na));
        const float sd = distance > a.desired ? sd0 / a.coefficient : sd0 * a.coefficient;
        *a.d_distance = distance;
        *a.d_stddev = sd;
        *new_sd = sd;
    }
    __syncthreads();

    // 4. the acting copy, generation_acting, the NEW stddev
    cycle_perturb(a, gsrc, gdst, *new_sd, a.gen_acting);
}

template <bool kStagePlain>
__global__ __launch_bounds__(kCycleThreads) void param_noise_cycle_kernel(CycleArgs a) {
    cycle_body<kStagePlain, false>(a);
}

// A population in one launch (ssc_param_noise_cycle_many): workgroup p serves pair p, whose item and cursor sit at
// workgroup-uniform addresses (scalar loads).  Shapes, LayerNorm, d_rms, m, the seed and the LDS carve are the pair's own;
// kStagePlain is the launch's.  A pair with n == 0 leaves at once, as a whole.
template <bool kStagePlain>
__global__ __launch_bounds__(kCycleThreads) void param_noise_cycle_many_kernel(const ssc_param_noise_many_item *__restrict__ items,
                                                                               const ssc_param_noise_cursor *__restrict__ cursors) {
    const ssc_param_noise_many_item &it = items[blockIdx.x];
    const ssc_param_noise_cursor &cu = cursors[blockIdx.x];
    if (it.n == 0) return;
    CycleArgs a;
    pack_cycle(a, it.actor, cu.m, it.d_obs, it.d_idx, it.d_rms, it.n, it.d_src, it.skip0_begin, it.skip0_end, it.skip1_begin,
               it.skip1_end, it.seed, cu.generation_adaptive, cu.generation_acting, it.desired, it.coefficient, it.d_stddev,
               it.d_distance, it.d_dst, kStagePlain ? 1 : 0);
    cycle_body<kStagePlain, true>(a);
}

// The checks of one agent -- the single call's, and through `who` ("ssc_param_noise_cycle_many: pair p") an item's of the
// population call, where m == 0 (perturb only) is a value as well.  Fills `a` (staging as `stage` says) for the launch.
int cycle_check(const char *who, bool many, CycleArgs &a, const ssc_actor_desc *actor, int64_t m, const float *d_obs,
                const int32_t *d_idx, const double *d_rms, int64_t n, const float *d_src, int64_t skip0_begin, int64_t skip0_end,
                int64_t skip1_begin, int64_t skip1_end, uint64_t seed, uint64_t generation_adaptive, uint64_t generation_acting,
                float desired, float coefficient, float *d_stddev, float *d_distance, float *d_dst, int stage) {
    SSC_REQUIRE(m >= (many ? 0 : 1) && m <= kCycleMaxRows, "%s: m %lld not in %d..%d", who, (long long)m, many ? 0 : 1, kCycleMaxRows);
    SSC_REQUIRE(n >= 1 && n < (int64_t)1 << 30, "%s: n %lld out of range", who, (long long)n);
    SSC_REQUIRE(coefficient > 1.0f, "%s: adoption coefficient must be > 1", who);
    SSC_REQUIRE(range_ok(skip0_begin, skip0_end, n) && range_ok(skip1_begin, skip1_end, n),
                "%s: skip ranges need 0 <= begin <= end <= n (n %lld: [%lld, %lld), [%lld, %lld))", who, (long long)n,
                (long long)skip0_begin, (long long)skip0_end, (long long)skip1_begin, (long long)skip1_end);
    const bool empty = skip0_begin == skip0_end || skip1_begin == skip1_end;
    SSC_REQUIRE(empty || skip0_end <= skip1_begin || skip1_end <= skip0_begin, "%s: skip ranges overlap", who);
    SSC_REQUIRE(generation_adaptive < (1ull << 56) && generation_acting < (1ull << 56),
                "%s: generation does not fit the counter (< 2^56)", who);
    SSC_REQUIRE(actor->obs_dim >= 1 && actor->obs_dim <= SSC_MAX_STATE && actor->act_dim >= 1 && actor->act_dim <= SSC_MAX_ACT,
                "%s: obs_dim %d / act_dim %d out of range", who, actor->obs_dim, actor->act_dim);
    SSC_REQUIRE(actor->h1 >= 1 && actor->h2 >= 1, "%s: bad hidden sizes", who);
    SSC_REQUIRE((d_obs != nullptr || m == 0) && d_src != nullptr && d_dst != nullptr, "%s: NULL obs / source / destination", who);
    SSC_REQUIRE(d_dst != d_src, "%s: d_dst == d_src (the actor forward reads the source)", who);
    SSC_REQUIRE(d_stddev != nullptr && d_distance != nullptr, "%s: NULL stddev / distance", who);
    const bool ln = actor->ln1_g != nullptr;
    SSC_REQUIRE(ln == (actor->ln1_b != nullptr) && ln == (actor->ln2_g != nullptr) && ln == (actor->ln2_b != nullptr),
                "%s: the four LayerNorm pointers come together", who);
    SSC_REQUIRE(pack_cycle(a, *actor, (int32_t)m, d_obs, d_idx, d_rms, n, d_src, skip0_begin, skip0_end, skip1_begin, skip1_end, seed,
                           generation_adaptive, generation_acting, desired, coefficient, d_stddev, d_distance, d_dst, stage),
                "%s: the actor's parameters must lie inside d_src[0 .. n)", who);
    const size_t lds = (size_t)a.lds.floats * sizeof(float);
    if (lds > kLdsBytes)
        return set_error(SSC_EUNSUPPORTED, "%s: the adaptive copy (%lld parameters) and a 4-row tile of a %d-%d actor need %zu "
                         "bytes of LDS (limit %zu)", who, (long long)n, a.net.h1, a.net.h2, lds, kLdsBytes);
    return SSC_OK;
}

int raise_cycle_lds(const void *fn, size_t lds) {
    if (lds <= 64 * 1024) return SSC_OK;
    return check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute");
}

struct PairRange {                       // [begin, end) of an array of pair `pair`
    const float *begin, *end;
    int pair;
    bool operator<(const PairRange &o) const { return begin < o.begin || (begin == o.begin && pair < o.pair); }
};

}  // namespace

}  // namespace ssc

using namespace ssc;

extern "C" {

int ssc_param_noise_perturb(int64_t n, const float *d_src, float *d_dst, const float *d_stddev, int64_t skip0_begin,
                            int64_t skip0_end, int64_t skip1_begin, int64_t skip1_end, uint64_t seed, uint64_t generation,
                            ssc_stream_t stream) {
    SSC_REQUIRE(n >= 0, "ssc_param_noise_perturb: n < 0");
    SSC_REQUIRE(range_ok(skip0_begin, skip0_end, n) && range_ok(skip1_begin, skip1_end, n),
                "ssc_param_noise_perturb: skip ranges need 0 <= begin <= end <= n (n %lld: [%lld, %lld), [%lld, %lld))",
                (long long)n, (long long)skip0_begin, (long long)skip0_end, (long long)skip1_begin, (long long)skip1_end);
    const bool empty = skip0_begin == skip0_end || skip1_begin == skip1_end;
    SSC_REQUIRE(empty || skip0_end <= skip1_begin || skip1_end <= skip0_begin, "ssc_param_noise_perturb: skip ranges overlap");
    // the counter keeps 24 bits of the generation's high word beside the stream tag (rng_words)
    SSC_REQUIRE(generation < (1ull << 56), "ssc_param_noise_perturb: generation does not fit the counter (< 2^56)");
    SSC_REQUIRE(d_stddev != nullptr, "ssc_param_noise_perturb: NULL stddev");
    if (n == 0) return SSC_OK;
    SSC_REQUIRE(d_src != nullptr && d_dst != nullptr, "ssc_param_noise_perturb: NULL source / destination");
    const int64_t groups = (n + 3) / 4;
    hipLaunchKernelGGL(param_noise_perturb_kernel, dim3(blocks_for(groups, kBlock)), dim3(kBlock), 0, as_stream(stream), n, d_src,
                       d_dst, d_stddev, skip0_begin, skip0_end, skip1_begin, skip1_end, seed, generation);
    return check_launch("ssc_param_noise_perturb");
}

int ssc_param_noise_adapt(int64_t count, const float *d_a, const float *d_b, float desired, float coefficient,
                          float *d_stddev, float *d_distance, ssc_stream_t stream) {
    SSC_REQUIRE(count >= 1 && count <= (int64_t)4096 * SSC_MAX_ACT, "ssc_param_noise_adapt: count %lld not in 1..%d",
                (long long)count, 4096 * SSC_MAX_ACT);
    SSC_REQUIRE(coefficient > 1.0f, "ssc_param_noise_adapt: adoption coefficient must be > 1");
    SSC_REQUIRE(d_a != nullptr && d_b != nullptr, "ssc_param_noise_adapt: NULL action batch");
    SSC_REQUIRE(d_stddev != nullptr && d_distance != nullptr, "ssc_param_noise_adapt: NULL stddev / distance");
    hipLaunchKernelGGL(param_noise_adapt_kernel, dim3(1), dim3(kAdaptThreads), 0, as_stream(stream), (int32_t)count, d_a, d_b,
                       desired, coefficient, d_stddev, d_distance);
    return check_launch("ssc_param_noise_adapt");
}

int ssc_param_noise_cycle(const ssc_actor_desc *actor, int64_t m, const float *d_obs, const double *d_rms, int64_t n,
                          const float *d_src, int64_t skip0_begin, int64_t skip0_end, int64_t skip1_begin, int64_t skip1_end,
                          uint64_t seed, uint64_t generation_adaptive, uint64_t generation_acting, float desired,
                          float coefficient, float *d_stddev, float *d_distance, float *d_dst, ssc_stream_t stream) {
    SSC_REQUIRE(actor != nullptr, "ssc_param_noise_cycle: actor NULL");
    CycleArgs a{};
    if (int rc = cycle_check("ssc_param_noise_cycle", false, a, actor, m, d_obs, nullptr, d_rms, n, d_src, skip0_begin, skip0_end,
                             skip1_begin, skip1_end, seed, generation_adaptive, generation_acting, desired, coefficient, d_stddev,
                             d_distance, d_dst, -1))
        return rc;
    const size_t lds = (size_t)a.lds.floats * sizeof(float);
    const auto kernel = a.lds.copies == 2 ? param_noise_cycle_kernel<true> : param_noise_cycle_kernel<false>;
    if (int rc = raise_cycle_lds(reinterpret_cast<const void *>(kernel), lds)) return rc;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kCycleThreads), lds, as_stream(stream), a);
    return check_launch("ssc_param_noise_cycle");
}

int ssc_param_noise_cycle_many(const ssc_param_noise_many_item *h_items, const ssc_param_noise_many_item *d_items,
                               const ssc_param_noise_cursor *h_cursors, const ssc_param_noise_cursor *d_cursors, int32_t n_pairs,
                               ssc_stream_t stream) {
    SSC_REQUIRE(n_pairs >= 1, "ssc_param_noise_cycle_many: n_pairs %d < 1", n_pairs);
    if (n_pairs > 65535) return set_error(SSC_EUNSUPPORTED, "ssc_param_noise_cycle_many: %d pairs > 65535", n_pairs);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_param_noise_cycle_many: NULL item array");
    SSC_REQUIRE(h_cursors != nullptr && d_cursors != nullptr, "ssc_param_noise_cycle_many: NULL cursor array");
    std::vector<PairRange> dsts, srcs;
    std::vector<std::pair<const void *, int>> owned;   // (scalar, pair) of what a pair's workgroup writes beside d_dst
    std::vector<CycleArgs> args((size_t)n_pairs);
    bool stage = true, work = false;
    for (int p = 0; p < n_pairs; ++p) {
        const ssc_param_noise_many_item &it = h_items[p];
        const ssc_param_noise_cursor &cu = h_cursors[p];
        char who[56];
        snprintf(who, sizeof who, "ssc_param_noise_cycle_many: pair %d", p);
        SSC_REQUIRE(it.n >= 0, "%s: n %lld out of range", who, (long long)it.n);
        args[p].n = 0;
        if (it.n == 0) continue;   // skipped: its workgroup leaves at once, nothing else of the item is read
        if (int rc = cycle_check(who, true, args[p], &it.actor, cu.m, it.d_obs, it.d_idx, it.d_rms, it.n, it.d_src, it.skip0_begin,
                                 it.skip0_end, it.skip1_begin, it.skip1_end, it.seed, cu.generation_adaptive, cu.generation_acting,
                                 it.desired, it.coefficient, it.d_stddev, it.d_distance, it.d_dst, -1))
            return rc;
        work = true;
        if (cu.m > 0) stage = stage && args[p].lds.copies == 2;
        dsts.push_back(PairRange{it.d_dst, it.d_dst + it.n, p});
        srcs.push_back(PairRange{it.d_src, it.d_src + it.n, p});
        owned.emplace_back(it.d_stddev, p);
        owned.emplace_back(it.d_distance, p);
    }
    // what a workgroup writes, no other workgroup writes or reads
    std::sort(dsts.begin(), dsts.end());
    for (size_t k = 1, top = 0; k < dsts.size(); ++k) {   // top: the range that reaches furthest so far
        SSC_REQUIRE(dsts[top].end <= dsts[k].begin, "ssc_param_noise_cycle_many: pairs %d and %d: the d_dst ranges overlap",
                    std::min(dsts[top].pair, dsts[k].pair), std::max(dsts[top].pair, dsts[k].pair));
        if (dsts[k].end > dsts[top].end) top = k;
    }
    std::sort(srcs.begin(), srcs.end());
    std::vector<size_t> reach(srcs.size());               // reach[k]: the range among srcs[0 .. k] that reaches furthest
    for (size_t k = 0; k < srcs.size(); ++k) reach[k] = (k > 0 && srcs[reach[k - 1]].end >= srcs[k].end) ? reach[k - 1] : k;
    for (const PairRange &d : dsts) {
        // the source ranges that begin below d.end; the one of them that reaches furthest overlaps d if any does
        const size_t cnt = std::lower_bound(srcs.begin(), srcs.end(), d.end, [](const PairRange &s, const float *e) { return s.begin < e; }) -
                           srcs.begin();
        if (cnt == 0) continue;
        const PairRange &s = srcs[reach[cnt - 1]];
        SSC_REQUIRE(s.end <= d.begin, "ssc_param_noise_cycle_many: pairs %d and %d: the d_dst range of pair %d overlaps the d_src range of pair %d",
                    std::min(s.pair, d.pair), std::max(s.pair, d.pair), d.pair, s.pair);
    }
    std::sort(owned.begin(), owned.end());
    for (size_t k = 1; k < owned.size(); ++k)
        SSC_REQUIRE(owned[k].first != owned[k - 1].first || owned[k].second == owned[k - 1].second,
                    "ssc_param_noise_cycle_many: pairs %d and %d share d_stddev / d_distance", std::min(owned[k - 1].second, owned[k].second),
                    std::max(owned[k - 1].second, owned[k].second));
    if (!work) return SSC_OK;
    // staging is the launch's: on iff every adapting pair fits both copies beside a 128-row tile; the LDS size the largest pair's
    size_t lds_max = 0;
    for (int p = 0; p < n_pairs; ++p)
        if (args[p].n > 0 && args[p].m > 0)
            lds_max = std::max(lds_max, (size_t)cycle_carve(args[p].n4, args[p].m, args[p].net.obs_dim, args[p].net.h1, args[p].net.h2,
                                                            stage ? 1 : 0).floats * sizeof(float));
    const auto kernel = stage ? param_noise_cycle_many_kernel<true> : param_noise_cycle_many_kernel<false>;
    if (int rc = raise_cycle_lds(reinterpret_cast<const void *>(kernel), lds_max)) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_pairs), dim3(kCycleThreads), lds_max, as_stream(stream), d_items, d_cursors);
    return check_launch("ssc_param_noise_cycle_many");
}

}  // extern "C"
