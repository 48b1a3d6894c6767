// obs_rms.hip -- the running observation statistics of DDPG's normalize_observations (ddpg_editted.py:14-18, 100-109):
// baselines 0.1.5 RunningMeanStd.update (common/mpi_running_mean_std.py, restated in DESIGN section 5) adds sum(x),
// sum(x^2) and the row count, all in f64, to the block [sum[D] | sumsq[D] | count].  store_transition feeds it the obs0
// of every stored transition (ddpg_editted.py:281-285).
//
// Two launches, both in a fixed order (no atomics, no ticket): every block reduces its share of the rows into one f64
// partial per component in the workspace; one block sums the partials in block order and adds them to the block.  The
// grid depends only on the shape, so the result is the same bits run to run.  HBM-bound: 4 B read per element.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "actor_device.h"
#include "ssc_host.h"

namespace ssc {

namespace {

constexpr int kRmsThreads = 256;
constexpr int kRmsMaxBlocks = 1024;

// element (r, i) of component c: base[c][r * row_stride + i * elem_stride], r < R, i < n
struct RmsArgs {
    const float *base[SSC_MAX_STATE];
    int64_t row_stride, elem_stride, n;
    int32_t R, rows_per_y;
    double *part;   // [gridDim.x * gridDim.y][2 * D]
};

template <int D>
__device__ __forceinline__ void block_reduce_store(double (&v)[2 * D], double *out) {
    __shared__ double red[kRmsThreads / 64][2 * D];
#pragma unroll
    for (int j = 0; j < 2 * D; ++j)
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) v[j] += __shfl_xor(v[j], msk);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < 2 * D; ++j) red[wave][j] = v[j];
    __syncthreads();
    if ((int)threadIdx.x < 2 * D) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kRmsThreads / 64; ++w) s += red[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// block (bx, by) of a partial grid that is gx blocks wide
template <int D>
__device__ __forceinline__ void obs_rms_partial_body(const RmsArgs &a, unsigned bx, unsigned by, unsigned gx) {
    double v[2 * D];
#pragma unroll
    for (int j = 0; j < 2 * D; ++j) v[j] = 0.0;
    const int32_t r0 = by * a.rows_per_y, r1 = min(a.R, r0 + a.rows_per_y);
    const int64_t istep = (int64_t)gx * kRmsThreads;
    for (int64_t i = (int64_t)bx * kRmsThreads + threadIdx.x; i < a.n; i += istep) {
        const int64_t off = i * a.elem_stride;
#pragma unroll 4
        for (int32_t r = r0; r < r1; ++r) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const double x = (double)a.base[c][(int64_t)r * a.row_stride + off];
                v[c] += x;
                v[D + c] = fma(x, x, v[D + c]);   // exact square in f64 for an fp32 x: the fma changes nothing
            }
        }
    }
    block_reduce_store<D>(v, a.part + (size_t)(by * gx + bx) * 2 * D);
}

template <int D>
__global__ __launch_bounds__(kRmsThreads) void obs_rms_partial_kernel(RmsArgs a) {
    obs_rms_partial_body<D>(a, blockIdx.x, blockIdx.y, gridDim.x);
}

template <int D>
__device__ __forceinline__ void obs_rms_final_body(const double *__restrict__ part, int32_t n_blocks, double rows, double *__restrict__ rms) {
    double v[2 * D];
#pragma unroll
    for (int j = 0; j < 2 * D; ++j) v[j] = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += kRmsThreads)
#pragma unroll
        for (int j = 0; j < 2 * D; ++j) v[j] += part[(size_t)b * 2 * D + j];
    __shared__ double tot[2 * D];
    block_reduce_store<D>(v, tot);
    __syncthreads();
    if ((int)threadIdx.x < 2 * D) rms[threadIdx.x] += tot[threadIdx.x];
    if (threadIdx.x == 0) rms[2 * D] += rows;
}

template <int D>
__global__ __launch_bounds__(kRmsThreads) void obs_rms_final_kernel(const double *__restrict__ part, int32_t n_blocks, double rows,
                                                                    double *__restrict__ rms) {
    obs_rms_final_body<D>(part, n_blocks, rows, rms);
}

// the partial grid of n elements x R rows: a function of the shape alone, so that the bits are the same run to run -- and
// the same whether the host computes it for one launch or a workgroup of ssc_obs_rms_update_many for its pair
struct RmsGrid { int gx, gy, rows_per_y; };
__host__ __device__ __forceinline__ RmsGrid rms_grid(int64_t n, int32_t R) {
    RmsGrid g;
    const int64_t gx64 = (n + kRmsThreads - 1) / kRmsThreads;
    g.gx = (int)(gx64 < kRmsMaxBlocks ? gx64 : kRmsMaxBlocks);
    g.gy = kRmsMaxBlocks / g.gx;
    if (g.gy > R) g.gy = R;
    g.rows_per_y = (R + g.gy - 1) / g.gy;
    g.gy = (R + g.rows_per_y - 1) / g.rows_per_y;
    return g;
}

// ssc_obs_rms_update's arguments as the kernels take them (a chunk log: elem_stride 1)
__host__ __device__ __forceinline__ void pack_rms(const ssc_transition_log &log, int obs_dim, int32_t k0, int32_t K, int64_t n,
                                                  void *workspace, RmsArgs &a) {
    a.row_stride = log.row_stride ? log.row_stride : n;
    for (int c = 0; c < SSC_MAX_STATE; ++c) a.base[c] = c < obs_dim ? log.obs[c < SSC_MAX_OBS ? c : 0] + (int64_t)k0 * a.row_stride : nullptr;
    a.elem_stride = 1;
    a.n = n;
    a.R = K - k0;
    a.rows_per_y = 0;
    a.part = static_cast<double *>(workspace);
}

// P updates in two launches (ssc_obs_rms_update_many): blockIdx.z is the pair; its blocks are those of ITS OWN partial grid
// (gx x gy inside the launch's max gx x max gy; the others leave), its gx takes gridDim.x's place in the stride and in
// the partial index, and one workgroup per pair sums its gx * gy partials in block order.
template <int D>
__global__ __launch_bounds__(kRmsThreads) void obs_rms_partial_many_kernel(const ssc_obs_rms_item *__restrict__ items) {
    const ssc_obs_rms_item &it = items[blockIdx.z];
    const RmsGrid g = rms_grid(it.n, it.K - it.k0);
    if ((int)blockIdx.x >= g.gx || (int)blockIdx.y >= g.gy) return;
    RmsArgs a;
    pack_rms(it.log, D, it.k0, it.K, it.n, it.d_workspace, a);
    a.rows_per_y = g.rows_per_y;
    obs_rms_partial_body<D>(a, blockIdx.x, blockIdx.y, (unsigned)g.gx);
}

template <int D>
__global__ __launch_bounds__(kRmsThreads) void obs_rms_final_many_kernel(const ssc_obs_rms_item *__restrict__ items) {
    const ssc_obs_rms_item &it = items[blockIdx.x];
    const RmsGrid g = rms_grid(it.n, it.K - it.k0);
    obs_rms_final_body<D>(static_cast<const double *>(it.d_workspace), g.gx * g.gy, (double)(it.K - it.k0) * (double)it.n, it.d_rms);
}

template <int D>
int launch_rms(RmsArgs a, double *rms, hipStream_t s) {
    const RmsGrid g = rms_grid(a.n, a.R);
    a.rows_per_y = g.rows_per_y;
    hipLaunchKernelGGL(obs_rms_partial_kernel<D>, dim3(g.gx, g.gy), dim3(kRmsThreads), 0, s, a);
    hipLaunchKernelGGL(obs_rms_final_kernel<D>, dim3(1), dim3(kRmsThreads), 0, s, a.part, g.gx * g.gy, (double)a.R * (double)a.n, rms);
    return check_launch("ssc_obs_rms_update");
}

template <int D>
int launch_rms_many(const ssc_obs_rms_item *d_items, int32_t n_pairs, int gx, int gy, hipStream_t s) {
    hipLaunchKernelGGL(obs_rms_partial_many_kernel<D>, dim3(gx, gy, n_pairs), dim3(kRmsThreads), 0, s, d_items);
    hipLaunchKernelGGL(obs_rms_final_many_kernel<D>, dim3(n_pairs), dim3(kRmsThreads), 0, s, d_items);
    return check_launch("ssc_obs_rms_update_many");
}

int dispatch_rms(int obs_dim, const RmsArgs &a, double *rms, hipStream_t s) {
    switch (obs_dim) {
    case 1: return launch_rms<1>(a, rms, s);
    case 2: return launch_rms<2>(a, rms, s);
    case 3: return launch_rms<3>(a, rms, s);
    case 4: return launch_rms<4>(a, rms, s);
    case 5: return launch_rms<5>(a, rms, s);
    case 6: return launch_rms<6>(a, rms, s);
    case 7: return launch_rms<7>(a, rms, s);
    default: return launch_rms<8>(a, rms, s);
    }
}

}  // namespace

}  // namespace ssc

using namespace ssc;

extern "C" {

size_t ssc_obs_rms_update_workspace_bytes(int32_t obs_dim) {
    if (obs_dim < 1 || obs_dim > SSC_MAX_STATE) return 0;
    return (size_t)kRmsMaxBlocks * 2 * (size_t)obs_dim * sizeof(double);
}

int ssc_obs_rms_update(int32_t obs_dim, const ssc_transition_log *log, int32_t k0, int32_t K, int64_t n, double *d_rms,
                       void *d_workspace, size_t workspace_bytes, ssc_stream_t stream) {
    SSC_REQUIRE(obs_dim >= 1 && obs_dim <= SSC_MAX_OBS, "ssc_obs_rms_update: obs_dim %d out of range", obs_dim);
    SSC_REQUIRE(log != nullptr && d_rms != nullptr, "ssc_obs_rms_update: NULL log / statistics block");
    SSC_REQUIRE(k0 >= 0 && K > k0, "ssc_obs_rms_update: need 0 <= k0 < K (k0 %d, K %d)", k0, K);
    SSC_REQUIRE(n >= 1, "ssc_obs_rms_update: n < 1");
    SSC_REQUIRE(log->row_stride == 0 || log->row_stride >= n, "ssc_obs_rms_update: row stride < n");
    const size_t need = ssc_obs_rms_update_workspace_bytes(obs_dim);
    SSC_REQUIRE(d_workspace != nullptr && workspace_bytes >= need,
                "ssc_obs_rms_update: workspace %zu < %zu bytes (ssc_obs_rms_update_workspace_bytes)", workspace_bytes, need);
    for (int c = 0; c < obs_dim; ++c) SSC_REQUIRE(log->obs[c] != nullptr, "ssc_obs_rms_update: NULL log obs column %d", c);
    RmsArgs a{};
    pack_rms(*log, obs_dim, k0, K, n, d_workspace, a);
    return dispatch_rms(obs_dim, a, d_rms, as_stream(stream));
}

int ssc_obs_rms_update_many(int32_t obs_dim, const ssc_obs_rms_item *h_items, const ssc_obs_rms_item *d_items, int32_t n_pairs,
                            ssc_stream_t stream) {
    SSC_REQUIRE(obs_dim >= 1 && obs_dim <= SSC_MAX_OBS, "ssc_obs_rms_update_many: obs_dim %d out of range", obs_dim);
    SSC_REQUIRE(n_pairs >= 1, "ssc_obs_rms_update_many: n_pairs %d < 1", n_pairs);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_obs_rms_update_many: NULL item array");
    if (n_pairs > 65535) return set_error(SSC_EUNSUPPORTED, "ssc_obs_rms_update_many: %d pairs > 65535 (one grid layer each)", n_pairs);
    const size_t need = ssc_obs_rms_update_workspace_bytes(obs_dim);
    int gx = 0, gy = 0;
    std::vector<std::pair<const void *, int>> owned;   // (statistics block / workspace, pair)
    owned.reserve((size_t)n_pairs * 2);
    for (int p = 0; p < n_pairs; ++p) {
        const ssc_obs_rms_item &it = h_items[p];
        SSC_REQUIRE(it.d_rms != nullptr, "ssc_obs_rms_update_many: pair %d: NULL statistics block", p);
        SSC_REQUIRE(it.k0 >= 0 && it.K > it.k0, "ssc_obs_rms_update_many: pair %d: need 0 <= k0 < K (k0 %d, K %d)", p, it.k0, it.K);
        SSC_REQUIRE(it.n >= 1, "ssc_obs_rms_update_many: pair %d: n < 1", p);
        SSC_REQUIRE(it.log.row_stride == 0 || it.log.row_stride >= it.n, "ssc_obs_rms_update_many: pair %d: row stride < n", p);
        SSC_REQUIRE(it.d_workspace != nullptr && it.workspace_bytes >= need,
                    "ssc_obs_rms_update_many: pair %d: workspace %zu < %zu bytes (ssc_obs_rms_update_workspace_bytes)", p, it.workspace_bytes, need);
        for (int c = 0; c < obs_dim; ++c)
            SSC_REQUIRE(it.log.obs[c] != nullptr, "ssc_obs_rms_update_many: pair %d: NULL log obs column %d", p, c);
        const RmsGrid g = rms_grid(it.n, it.K - it.k0);
        if (g.gx > gx) gx = g.gx;
        if (g.gy > gy) gy = g.gy;
        owned.emplace_back(it.d_rms, p);
        owned.emplace_back(it.d_workspace, p);
    }
    std::sort(owned.begin(), owned.end());
    for (size_t k = 1; k < owned.size(); ++k)
        SSC_REQUIRE(owned[k].first != owned[k - 1].first, "ssc_obs_rms_update_many: pairs %d and %d share a statistics block or a workspace",
                    owned[k - 1].second, owned[k].second);
    hipStream_t s = as_stream(stream);
    if (obs_dim == 1) return launch_rms_many<1>(d_items, n_pairs, gx, gy, s);
    if (obs_dim == 2) return launch_rms_many<2>(d_items, n_pairs, gx, gy, s);
    return launch_rms_many<3>(d_items, n_pairs, gx, gy, s);
}

int ssc_obs_rms_update_rows(int32_t obs_dim, int64_t m, const float *d_x, double *d_rms, void *d_workspace,
                            size_t workspace_bytes, ssc_stream_t stream) {
    SSC_REQUIRE(obs_dim >= 1 && obs_dim <= SSC_MAX_STATE, "ssc_obs_rms_update_rows: obs_dim %d out of range", obs_dim);
    SSC_REQUIRE(m >= 0, "ssc_obs_rms_update_rows: m < 0");
    SSC_REQUIRE(d_rms != nullptr, "ssc_obs_rms_update_rows: NULL statistics block");
    const size_t need = ssc_obs_rms_update_workspace_bytes(obs_dim);
    SSC_REQUIRE(d_workspace != nullptr && workspace_bytes >= need,
                "ssc_obs_rms_update_rows: workspace %zu < %zu bytes (ssc_obs_rms_update_workspace_bytes)", workspace_bytes, need);
    if (m == 0) return SSC_OK;
    SSC_REQUIRE(d_x != nullptr, "ssc_obs_rms_update_rows: NULL rows");
    RmsArgs a{};
    for (int c = 0; c < obs_dim; ++c) a.base[c] = d_x + c;
    a.row_stride = 0;
    a.elem_stride = obs_dim;
    a.n = m;
    a.R = 1;
    a.part = static_cast<double *>(d_workspace);
    return dispatch_rms(obs_dim, a, d_rms, as_stream(stream));
}

}  // extern "C"
