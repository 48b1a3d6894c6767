// param_noise.hip -- adaptive parameter-space noise of DDPG (ddpg_editted.py:47-60, 151-166, 360-385) on flat
// parameter arrays [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3]:
//
//   ssc_param_noise_perturb   dst = src + stddev * N(0,1) outside the skip ranges (the LayerNorm segments, which
//                             models_editted.py:18-19 keeps out of perturbable_vars), a bit copy inside them.
//   ssc_param_noise_adapt     distance = sqrt(mean((a - b)^2)) of two action batches, then baselines 0.1.5
//                             AdaptiveParamNoiseSpec.adapt on the device stddev.
//
// Both read stddev from device memory, so a loop adapts and re-perturbs without the host.  A few thousand elements
// each: the cost is the launch.
#include "ssc_device.h"
#include "ssc_host.h"

namespace ssc {

namespace {

// stream tag of the parameter noise (the oracle's keying: rng_words(seed, q, generation, 9)).  It lives here, next to its
// only user, like TAG_DATA_NOISE in dataset.hip: ssc_device.h is part of the rollout kernel's profiled sources.
enum : uint32_t { TAG_PARAM_NOISE = 9 };

constexpr int kAdaptThreads = 256;

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
        const float g = gaussian_f32(j < 2 ? w.x : w.z, j < 2 ? w.y : w.w, (j & 1) != 0);
        // stddev 0 is a bit copy as well (x + 0 * g would turn -0.0 into +0.0)
        dst[i] = (skip || sd == 0.0f) ? x : fmaf(sd, g, x);
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

}  // extern "C"
