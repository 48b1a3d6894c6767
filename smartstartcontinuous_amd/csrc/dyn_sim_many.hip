// dyn_sim_many.hip -- ssc_mpc_forward_sim_many: the fused fp32 forward simulation (dyn_small_sim.h) for a POPULATION of
// dynamics models in one launch.  Grid row y = item y: a contiguous range of the call's problems with a network and
// z-score statistics of its own.  A workgroup reads its item at a workgroup-uniform address (scalar loads), fills the
// single-model kernels' SmallSimArgs from the call-level kernel arguments plus the item and runs the same __device__ body
// over the item's row range -- so every row gets, bit for bit, what the model's own ssc_mpc_forward_sim call gives it.
//
// NOTE: compiled WITHOUT -fno-honor-nans, like dyn_model.hip -- np.nan_to_num semantics need real NaN/Inf tests.
#include <algorithm>
#include <stdio.h>
#include <vector>

#include "dyn_small_sim.h"

namespace ssc {

typedef const __attribute__((address_space(4))) ssc_mpc_sim_many_item *const_item;   // uniform reads: scalar loads

// The item's part of the arguments.  The weight pointers land in SGPRs (the SW variant reads through them with scalar
// loads); g.S / g.A_out stay the kernel arguments, so the buffer descriptors are uniform without a waterfall loop.
__device__ __forceinline__ void small_sim_item_args(SmallSimArgs &g, const_item it) {
    g.depth = it->mlp.dims[1];
    g.W1 = it->mlp.W[0]; g.b1 = it->mlp.b[0]; g.W2 = it->mlp.W[1]; g.b2 = it->mlp.b[1];
#pragma unroll
    for (int k = 0; k < SSC_MAX_STATE; ++k) {
        g.nm.mean_x[k] = it->norm.mean_x[k]; g.nm.std_x[k] = it->norm.std_x[k];
        g.nm.mean_z[k] = it->norm.mean_z[k]; g.nm.std_z[k] = it->norm.std_z[k];
    }
#pragma unroll
    for (int k = 0; k < SSC_MAX_ACT; ++k) { g.nm.mean_y[k] = it->norm.mean_y[k]; g.nm.std_y[k] = it->norm.std_y[k]; }
    g.live_list = nullptr; g.n_live = nullptr;       // (refused by the launcher: the compact-list code folds away)
}

// one row per lane: any state / action split of the fused family
__global__ __launch_bounds__(256) void dyn_small_sim_many_kernel(SmallSimArgs g, const ssc_mpc_sim_many_item *items) {
    __shared__ __attribute__((aligned(16))) float rec[kSmallSimMaxDepth][8];
    const const_item it = (const_item)items + blockIdx.y;
    const int64_t rows = (int64_t)it->n_problems * g.N;
    if ((int64_t)blockIdx.x * 256 >= rows) return;       // a surplus workgroup, or an empty item: workgroup-uniform, no barrier yet
    small_sim_item_args(g, it);
    const int64_t lo = (int64_t)it->problem0 * g.N;
    small_sim_body(g, rec, blockIdx.x, lo, lo + rows);
}

// two rows per lane (state D = 2 or 3, one action, every byte offset below 2^31).  The variant is the one the item's own
// call runs -- weights by scalar loads when depth % 4 == 0, else the LDS image -- chosen per workgroup.
template <int D>
__global__ __launch_bounds__(256) void dyn_small_sim_pair_many_kernel(SmallSimArgs g, const ssc_mpc_sim_many_item *items) {
    __shared__ __attribute__((aligned(16))) float rec[kSmallSimMaxDepth][8];
    const const_item it = (const_item)items + blockIdx.y;
    const uint32_t rows = (uint32_t)it->n_problems * (uint32_t)g.N;
    if (blockIdx.x * 512u >= rows) return;               // a surplus workgroup, or an empty item: workgroup-uniform, no barrier yet
    small_sim_item_args(g, it);
    const uint32_t lo = (uint32_t)it->problem0 * (uint32_t)g.N;
    if (g.depth % 4 == 0) small_sim_pair_body<D, true, true>(g, rec, blockIdx.x, lo, lo + rows);
    else small_sim_pair_body<D, true, false>(g, rec, blockIdx.x, lo, lo + rows);
}

struct ItemRange {
    int64_t begin, end;
    int item;
    bool operator<(const ItemRange &o) const { return begin != o.begin ? begin < o.begin : item < o.item; }
};

}  // namespace ssc

using namespace ssc;

extern "C" {

int ssc_mpc_forward_sim_many(const ssc_mpc_sim_many_item *h_items, const ssc_mpc_sim_many_item *d_items, int32_t n_items,
                             const ssc_mpc_sampling *sp, int64_t m, int32_t H, int32_t state_dim, int32_t act_dim,
                             const float *d_s0, int64_t s0_rows, float *d_A_out, float *d_S, ssc_stream_t stream) {
    SSC_REQUIRE(n_items >= 1, "ssc_mpc_forward_sim_many: n_items %d < 1", n_items);
    if (n_items > 65535)
        return set_error(SSC_EUNSUPPORTED, "ssc_mpc_forward_sim_many: %d items > 65535 (one grid row each)", n_items);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_mpc_forward_sim_many: NULL item array");
    SSC_REQUIRE(sp != nullptr, "ssc_mpc_forward_sim_many: NULL descriptor");
    SSC_REQUIRE(m >= 0 && H >= 1, "ssc_mpc_forward_sim_many: m = %lld, H = %d", (long long)m, H);
    SSC_REQUIRE(state_dim >= 1 && state_dim <= SSC_MAX_STATE && act_dim >= 1 && act_dim <= SSC_MAX_ACT,
                "ssc_mpc_forward_sim_many: state_dim %d / act_dim %d out of range", state_dim, act_dim);
    SSC_REQUIRE(sp->n_samples >= 1 && m % sp->n_samples == 0, "ssc_mpc_forward_sim_many: n_samples %d must divide m = %lld",
                sp->n_samples, (long long)m);
    SSC_REQUIRE(s0_rows >= 1 && (m == 0 || m % s0_rows == 0), "ssc_mpc_forward_sim_many: s0_rows must divide m");
    for (int a = 0; a < act_dim; ++a)
        SSC_REQUIRE(sp->low[a] <= sp->high[a], "ssc_mpc_forward_sim_many: low > high for action component %d", a);
    SSC_REQUIRE(sp->d_live_list == nullptr && sp->d_n_live == nullptr,
                "ssc_mpc_forward_sim_many: a compact live list maps slots to arbitrary problems (a workgroup's weights would "
                "not be uniform): d_live_list / d_n_live must be NULL");
    const int64_t P = m / sp->n_samples;
    std::vector<ItemRange> ranges;
    int64_t rows_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const ssc_mpc_sim_many_item &it = h_items[i];
        char who[56];
        snprintf(who, sizeof who, "ssc_mpc_forward_sim_many: item %d", i);
        SSC_REQUIRE(it.n_problems >= 0, "%s: n_problems %d < 0", who, it.n_problems);
        if (it.n_problems == 0) continue;      // skipped: its workgroups leave at once, nothing else of the item is read
        if (int rc = validate_mlp(&it.mlp, who)) return rc;
        SSC_REQUIRE(it.mlp.dims[0] == state_dim + act_dim && it.mlp.dims[it.mlp.n_layers] == state_dim,
                    "%s: network is %d -> %d, expected %d -> %d", who, it.mlp.dims[0], it.mlp.dims[it.mlp.n_layers],
                    state_dim + act_dim, state_dim);
        if (!small_sim_shape(&it.mlp, state_dim, act_dim))
            return set_error(SSC_EUNSUPPORTED, "%s: outside the fused fp32 family (one hidden layer <= %d, state <= 3, "
                             "state + act <= 4); simulate it with ssc_mpc_forward_sim", who, kSmallSimMaxDepth);
        SSC_REQUIRE(it.problem0 >= 0 && (int64_t)it.problem0 + it.n_problems <= P,
                    "%s: problems [%d, %lld) outside [0, %lld)", who, it.problem0, (long long)it.problem0 + it.n_problems,
                    (long long)P);
        ranges.push_back(ItemRange{it.problem0, (int64_t)it.problem0 + it.n_problems, i});
        rows_max = std::max(rows_max, (int64_t)it.n_problems * sp->n_samples);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1, top = 0; k < ranges.size(); ++k) {      // top: the range before this one that reaches furthest
        const ItemRange &r = ranges[k], &o = ranges[top];
        SSC_REQUIRE(o.end <= r.begin, "ssc_mpc_forward_sim_many: items %d and %d: problems [%lld, %lld) and [%lld, %lld) overlap",
                    std::min(o.item, r.item), std::max(o.item, r.item), (long long)o.begin, (long long)o.end,
                    (long long)r.begin, (long long)r.end);
        if (r.end > o.end) top = k;
    }
    if (m == 0) return SSC_OK;
    SSC_REQUIRE(d_s0 && d_S, "ssc_mpc_forward_sim_many: NULL device pointer");
    if (ranges.empty()) return SSC_OK;
    SmallSimArgs g{};
    small_sim_call_args(g, sp, m, H, state_dim, act_dim, d_s0, s0_rows, nullptr, d_A_out, d_S);
    hipStream_t s = as_stream(stream);
    // launch_small_sim's rule on the call's m (the byte offsets are those of the whole buffers)
    if (small_sim_pair_shape(sp, m, H, state_dim, act_dim)) {
        const dim3 grid((unsigned)((rows_max + 511) / 512), (unsigned)n_items);
        if (state_dim == 2) hipLaunchKernelGGL(dyn_small_sim_pair_many_kernel<2>, grid, dim3(256), 0, s, g, d_items);
        else hipLaunchKernelGGL(dyn_small_sim_pair_many_kernel<3>, grid, dim3(256), 0, s, g, d_items);
        return check_launch("dyn_small_sim_pair_many_kernel");
    }
    hipLaunchKernelGGL(dyn_small_sim_many_kernel, dim3(blocks_for(rows_max), (unsigned)n_items), dim3(256), 0, s, g, d_items);
    return check_launch("dyn_small_sim_many_kernel");
}

}  // extern "C"
