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
//
// All read stddev from device memory, so a loop adapts and re-perturbs without the host.  A few thousand elements
// each: the cost is the launch.
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
// ssc_param_noise_cycle: ONE workgroup of 1024 threads.
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
// A tile is TR rows (4 .. 128, chosen by the launcher: the largest that fits beside the copy).  Work items are
// (row group of 4, output unit) with the unit fastest, so the weight reads of a wave are consecutive floats -- global
// loads for the plain network, LDS reads for the adaptive one -- and BOTH networks run in one item: eight independent FMA
// chains per thread.  Every output unit sums its inputs in index order with fused multiply-adds, like
// actor_generic_kernel / actor_row_kernel.
// ---------------------------------------------------------------------------------------
constexpr int kCycleThreads = 1024;
constexpr int kCycleMaxTile = 128;
constexpr size_t kLdsBytes = 160 * 1024;

struct CycleNet {                       // offsets into the flat array, in floats
    int32_t W1, b1, W2, b2, W3, b3;
    int32_t g1, be1, g2, be2;           // LayerNorm gamma / beta; g1 < 0: none
    int32_t obs_dim, h1, h2, act_dim, last_tanh;
    float obs_clip;
};

struct CycleArgs {
    CycleNet net;
    int32_t m, tile_rows, n, n4;
    const float *obs;
    const double *rms;
    const float *src;
    float *dst;
    int64_t s0b, s0e, s1b, s1e;
    uint64_t seed, gen_adaptive, gen_acting;
    float desired, coefficient;
    float *d_stddev, *d_distance;
};

__host__ __device__ inline size_t cycle_lds_floats(int n4, int copies, int tr, int obs_dim, int h1, int h2) {
    return (size_t)copies * n4 + (size_t)tr * obs_dim + 2 * (size_t)(tr / 4) * (4 * (h1 + 1)) + 2 * (size_t)(tr / 4) * (4 * (h2 + 1)) +
           4 * (size_t)tr + 2 * 16 + 4;
}

typedef float cyc_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float hidden_act(float x, int last_tanh) { return last_tanh ? tanh_fast(x) : fmaxf(x, 0.0f); }

template <bool kStagePlain>
__global__ __launch_bounds__(kCycleThreads) void param_noise_cycle_kernel(CycleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const CycleNet &nt = a.net;
    const int TR = a.tile_rows, G = TR / 4, od = nt.obs_dim, h1 = nt.h1, h2 = nt.h2, na = nt.act_dim;
    const int sA = 4 * (h1 + 1), sB = 4 * (h2 + 1);   // floats per row group
    float *ad = smem;
    float *obsS = ad + (kStagePlain ? 2 : 1) * a.n4;
    float *hA = obsS + od * TR;
    float *hB = hA + 2 * G * sA;
    float *st = hB + 2 * G * sB;
    double *red = reinterpret_cast<double *>(st + 4 * TR);
    float *new_sd = reinterpret_cast<float *>(red + 16);
    const bool ln = nt.g1 >= 0;
    const float sd0 = *a.d_stddev;
    const float *src;                                            // what the plain network reads
    if constexpr (kStagePlain) {
        float *pl = ad + a.n4;
        for (int i = tid; i < a.n; i += kCycleThreads) pl[i] = a.src[i];
        src = pl;
    } else {
        src = a.src;
    }

    // 1. the adaptive copy, generation_adaptive, the stddev as it stands
    for (int q = tid; 4 * q < a.n; q += kCycleThreads) {
        const u32x4 w = rng_words(a.seed, (uint64_t)q, a.gen_adaptive, TAG_PARAM_NOISE);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * q + j;
            if (i >= a.n) break;
            const bool skip = (i >= a.s0b && i < a.s0e) || (i >= a.s1b && i < a.s1e);
            ad[i] = perturbed(a.src[i], skip, sd0, w, j);
        }
    }

    // 2. a = actor(obs), b = adaptive_actor(obs), tile by tile; thread t owns element (row t / act_dim, t % act_dim) of
    //    every tile and sums its squared differences in tile order
    double v = 0.0;
    for (int row0 = 0; row0 < a.m; row0 += TR) {
        if (tid < TR) {
            const int r = min(row0 + tid, a.m - 1);              // rows past m repeat the last one and are not summed
            if (a.rms != nullptr) {
                ObsNorm<SSC_MAX_STATE> nrm;
                nrm.load(a.rms, od);
#pragma unroll
                for (int c = 0; c < SSC_MAX_STATE; ++c)
                    if (c < od) obsS[c * TR + tid] = nrm.apply(a.obs[r * od + c], c, nt.obs_clip);
            } else {
#pragma unroll
                for (int c = 0; c < SSC_MAX_STATE; ++c)
                    if (c < od) obsS[c * TR + tid] = clip_obs(a.obs[r * od + c], nt.obs_clip);
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
                const float *wts = net ? ad : src;
                const float g = wts[nt.g1 + j], be = wts[nt.be1 + j];
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
            const float *wp = src + nt.W2 + j, *wa = ad + nt.W2 + j;
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
                const float *wts = net ? ad : src;
                const float g = wts[nt.g2 + j], be = wts[nt.be2 + j];
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
    const float sd1 = *new_sd;
    for (int q = tid; 4 * q < a.n; q += kCycleThreads) {
        const u32x4 w = rng_words(a.seed, (uint64_t)q, a.gen_acting, TAG_PARAM_NOISE);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * q + j;
            if (i >= a.n) break;
            const bool skip = (i >= a.s0b && i < a.s0e) || (i >= a.s1b && i < a.s1e);
            a.dst[i] = perturbed(a.src[i], skip, sd1, w, j);
        }
    }
}

// offset of a parameter segment of `count` floats inside the flat array, or -1 when it does not lie inside it
// (this maps the CALLER's pointers back to offsets, whatever order they come in; the flat layout the learners write --
// [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3] -- is defined in ddpg_layout.h)
int32_t segment(const float *p, int64_t count, const float *src, int64_t n) {
    if (p == nullptr || p < src) return -1;
    const int64_t off = p - src;
    return (off + count <= n) ? (int32_t)off : -1;
}

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
    SSC_REQUIRE(m >= 1 && m <= 4096, "ssc_param_noise_cycle: m %lld not in 1..4096", (long long)m);
    SSC_REQUIRE(n >= 1 && n < (int64_t)1 << 30, "ssc_param_noise_cycle: n %lld out of range", (long long)n);
    SSC_REQUIRE(coefficient > 1.0f, "ssc_param_noise_cycle: adoption coefficient must be > 1");
    SSC_REQUIRE(range_ok(skip0_begin, skip0_end, n) && range_ok(skip1_begin, skip1_end, n),
                "ssc_param_noise_cycle: skip ranges need 0 <= begin <= end <= n (n %lld: [%lld, %lld), [%lld, %lld))",
                (long long)n, (long long)skip0_begin, (long long)skip0_end, (long long)skip1_begin, (long long)skip1_end);
    const bool empty = skip0_begin == skip0_end || skip1_begin == skip1_end;
    SSC_REQUIRE(empty || skip0_end <= skip1_begin || skip1_end <= skip0_begin, "ssc_param_noise_cycle: skip ranges overlap");
    SSC_REQUIRE(generation_adaptive < (1ull << 56) && generation_acting < (1ull << 56),
                "ssc_param_noise_cycle: generation does not fit the counter (< 2^56)");
    SSC_REQUIRE(actor->obs_dim >= 1 && actor->obs_dim <= SSC_MAX_STATE && actor->act_dim >= 1 && actor->act_dim <= SSC_MAX_ACT,
                "ssc_param_noise_cycle: obs_dim %d / act_dim %d out of range", actor->obs_dim, actor->act_dim);
    SSC_REQUIRE(actor->h1 >= 1 && actor->h2 >= 1, "ssc_param_noise_cycle: bad hidden sizes");
    SSC_REQUIRE(d_obs != nullptr && d_src != nullptr && d_dst != nullptr, "ssc_param_noise_cycle: NULL obs / source / destination");
    SSC_REQUIRE(d_dst != d_src, "ssc_param_noise_cycle: d_dst == d_src (the actor forward reads the source)");
    SSC_REQUIRE(d_stddev != nullptr && d_distance != nullptr, "ssc_param_noise_cycle: NULL stddev / distance");
    const bool ln = actor->ln1_g != nullptr;
    SSC_REQUIRE(ln == (actor->ln1_b != nullptr) && ln == (actor->ln2_g != nullptr) && ln == (actor->ln2_b != nullptr),
                "ssc_param_noise_cycle: the four LayerNorm pointers come together");
    const int64_t h1 = actor->h1, h2 = actor->h2;
    CycleArgs a{};
    CycleNet &nt = a.net;
    nt.W1 = segment(actor->W1, actor->obs_dim * h1, d_src, n);
    nt.b1 = segment(actor->b1, h1, d_src, n);
    nt.W2 = segment(actor->W2, h1 * h2, d_src, n);
    nt.b2 = segment(actor->b2, h2, d_src, n);
    nt.W3 = segment(actor->W3, h2 * actor->act_dim, d_src, n);
    nt.b3 = segment(actor->b3, actor->act_dim, d_src, n);
    bool inside = nt.W1 >= 0 && nt.b1 >= 0 && nt.W2 >= 0 && nt.b2 >= 0 && nt.W3 >= 0 && nt.b3 >= 0;
    nt.g1 = nt.be1 = nt.g2 = nt.be2 = -1;
    if (ln) {
        nt.g1 = segment(actor->ln1_g, h1, d_src, n);
        nt.be1 = segment(actor->ln1_b, h1, d_src, n);
        nt.g2 = segment(actor->ln2_g, h2, d_src, n);
        nt.be2 = segment(actor->ln2_b, h2, d_src, n);
        inside = inside && nt.g1 >= 0 && nt.be1 >= 0 && nt.g2 >= 0 && nt.be2 >= 0;
    }
    SSC_REQUIRE(inside, "ssc_param_noise_cycle: the actor's parameters must lie inside d_src[0 .. n)");
    nt.obs_dim = actor->obs_dim, nt.h1 = actor->h1, nt.h2 = actor->h2, nt.act_dim = actor->act_dim;
    nt.last_tanh = actor->last_layer_tanh, nt.obs_clip = actor->obs_clip;
    // the largest tile that fits beside the adaptive copy (and no larger than the batch needs)
    const int n4 = (int)((n + 3) / 4 * 4);
    const bool stage = cycle_lds_floats(n4, 2, kCycleMaxTile, nt.obs_dim, nt.h1, nt.h2) * sizeof(float) <= kLdsBytes;
    const int copies = stage ? 2 : 1;
    int tr = kCycleMaxTile;
    while (tr > 4 && (cycle_lds_floats(n4, copies, tr, nt.obs_dim, nt.h1, nt.h2) * sizeof(float) > kLdsBytes || tr / 2 >= m)) tr /= 2;
    const size_t lds = cycle_lds_floats(n4, copies, tr, nt.obs_dim, nt.h1, nt.h2) * sizeof(float);
    if (lds > kLdsBytes)
        return set_error(SSC_EUNSUPPORTED,
                         "ssc_param_noise_cycle: the adaptive copy (%lld parameters) and a 4-row tile of a %d-%d actor need %zu "
                         "bytes of LDS (limit %zu)", (long long)n, nt.h1, nt.h2, lds, kLdsBytes);
    a.m = (int32_t)m, a.tile_rows = tr, a.n = (int32_t)n, a.n4 = n4;
    a.obs = d_obs, a.rms = d_rms, a.src = d_src, a.dst = d_dst;
    a.s0b = skip0_begin, a.s0e = skip0_end, a.s1b = skip1_begin, a.s1e = skip1_end;
    a.seed = seed, a.gen_adaptive = generation_adaptive, a.gen_acting = generation_acting;
    a.desired = desired, a.coefficient = coefficient, a.d_stddev = d_stddev, a.d_distance = d_distance;
    const auto kernel = stage ? param_noise_cycle_kernel<true> : param_noise_cycle_kernel<false>;
    if (lds > 64 * 1024) {
        int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kCycleThreads), lds, as_stream(stream), a);
    return check_launch("ssc_param_noise_cycle");
}

}  // extern "C"
