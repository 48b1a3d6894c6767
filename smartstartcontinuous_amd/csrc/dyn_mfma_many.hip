// dyn_mfma_many.hip -- ssc_mpc_forward_sim_many_mfma: the bf16-MFMA forward simulation (dyn_mfma_sim.h) for a POPULATION
// of dynamics models in one launch.  Grid row y = item y: a contiguous range of the call's problems with a packed weight
// image of its own (ssc_dyn_prepare); grid x = the item's row tiles of 256 rows, ANCHORED AT THE ITEM'S FIRST ROW, so the
// partition into tiles, waves and 16-row column tiles is that of the model's own call on its own rows -- and with it which
// waves the problem mask lets skip.  A workgroup reads its item at a workgroup-uniform address (scalar loads), moves the
// call-level arguments to the item's first row and problem and runs the single-model kernel's body: every row gets, bit for
// bit, what the model's own ssc_mpc_forward_sim(.., SSC_PREC_BF16_MFMA_PREPARED) call on the item's rows gives it.
//
// Served: the seven instantiation classes with <= 4 inputs and outputs whose weights are resident in LDS (one hidden layer
// up to 512 units; two equal hidden layers up to 128).  The streamed-W2 kernels (two layers deeper than 128) re-read their
// own kernarg segment at tile boundaries and have no register to spare: they stay single-model.
//
// NOTE: compiled with the flags of dyn_mfma.hip (no -fno-honor-nans, MFMA results in AGPRs) -- the bits must match.
#include <algorithm>
#include <stdio.h>
#include <vector>

#include "dyn_mfma_sim.h"

namespace ssc {

int validate_mlp(const ssc_mlp_desc *mlp, const char *who);                        // dyn_model.hip
bool dyn_mfma_supported(const ssc_mlp_desc *mlp, int state_dim, int act_dim);      // dyn_mfma.hip
size_t dyn_mfma_workspace_bytes(const ssc_mlp_desc *mlp);

typedef const __attribute__((address_space(4))) ssc_mpc_sim_many_mfma_item *const_mfma_item;   // uniform reads: scalar loads

// The offsets inside a packed image depend on the class only (make_pack), so an item is its image's base address and its
// problem range; the z-score statistics are inside the image.
template <int UT, int NFC, bool BIASK>
__global__ __launch_bounds__(kDynThreads, 2) void dyn_mfma_sim_many_kernel(DynSimArgs g, const ssc_mpc_sim_many_mfma_item *items) {
    const const_mfma_item it = (const_mfma_item)items + blockIdx.y;
    const int64_t rows = (int64_t)it->n_problems * g.N;
    if ((int64_t)blockIdx.x * kDynRows >= rows) return;   // a surplus workgroup, or an empty item: workgroup-uniform, no barrier yet
    constexpr DynPack pk = make_pack(UT, NFC);
    const unsigned char *img = static_cast<const unsigned char *>(it->d_image);
    const int64_t p0 = it->problem0, lo = p0 * g.N;
    g.a1 = img + pk.a1; g.a2 = img + pk.a2; g.a3 = img + pk.a3;
    g.b2 = reinterpret_cast<const float *>(img + pk.b2); g.b3 = reinterpret_cast<const float *>(img + pk.b3);
    g.nm = reinterpret_cast<const float *>(img + pk.nm);
    // relative to its item a row is what it is in the model's own call: Philox problem id, mask byte, rows of S and A_out
    g.pid0 += (uint64_t)p0;
    if (g.active != nullptr) g.active += p0;
    g.S += lo * g.d;
    if (g.A_out != nullptr) g.A_out += lo * g.H * g.a;
    dyn_mfma_sim_body<UT, NFC, BIASK, 4, false, 1, false, true>(g, DynManyRows{lo, rows});
}

// id of the instantiation class that serves the network, -1: none
static int many_class(const ssc_mlp_desc *mlp, int state_dim, int act_dim) {
    if (mlp == nullptr || (mlp->n_layers != 2 && mlp->n_layers != 3)) return -1;
    const int nfc = mlp->n_layers - 1, in = mlp->dims[0], depth = mlp->dims[1], out = mlp->dims[mlp->n_layers];
    if (in < 1 || depth < 1 || out < 1 || !dyn_mfma_supported(mlp, state_dim, act_dim)) return -1;
    if (state_dim < 1 || act_dim < 1 || in != state_dim + act_dim || out != state_dim) return -1;
    if (in > 4 || out > 4) return -1;              // the KIN = 4 kernels (compact layer 1)
    const int UT = tiles_for(depth);
    if (nfc == 2 && UT > 4) return -1;             // streamed W2
    const int ut = UT == 1 ? 0 : (UT == 4 ? 1 : 2);
    if (nfc == 1) return ut;                       // 0, 1, 2: <1,1>, <4,1>, <16,1>
    const bool biask = depth + 2 <= 32 * UT;       // make_net's rule
    return 3 + 2 * ut + (biask ? 1 : 0);           // 3, 4: <1,2>, <1,2,biask>; 5, 6: <4,2>, <4,2,biask>
}

template <int UT, int NFC, bool BIASK>
static int launch_many(const DynSimArgs &g, const ssc_mpc_sim_many_mfma_item *d_items, int64_t rows_max, int n_items, hipStream_t s) {
    const size_t lds = (size_t)dyn_a2_bufs<UT, NFC>() * UT * 2048 + (size_t)UT * 1024 + (size_t)UT * 512 + (size_t)UT * 128 + 64;
    const void *kern = reinterpret_cast<const void *>(dyn_mfma_sim_many_kernel<UT, NFC, BIASK>);
    if (lds > 64 * 1024) {
        int rc = check_hip(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute(dyn_mfma_sim_many_kernel)");
        if (rc) return rc;
    }
    DynSimArgs ga = g;
    void *params[] = {&ga, &d_items};
    const dim3 grid((unsigned)((rows_max + kDynRows - 1) / kDynRows), (unsigned)n_items);
    if (int rc = check_hip(hipLaunchKernel(kern, grid, dim3(kDynThreads), params, lds, s), "hipLaunchKernel(dyn_mfma_sim_many_kernel)"))
        return rc;
    return check_launch("dyn_mfma_sim_many_kernel");
}

struct MfmaItemRange {
    int64_t begin, end;
    int item;
    bool operator<(const MfmaItemRange &o) const { return begin != o.begin ? begin < o.begin : item < o.item; }
};

}  // namespace ssc

using namespace ssc;

extern "C" {

int ssc_dyn_mfma_many_class(const ssc_mlp_desc *mlp, int32_t state_dim, int32_t act_dim) { return many_class(mlp, state_dim, act_dim); }

int ssc_mpc_forward_sim_many_mfma(const ssc_mpc_sim_many_mfma_item *h_items, const ssc_mpc_sim_many_mfma_item *d_items,
                                  int32_t n_items, const ssc_mpc_sampling *sp, int64_t m, int32_t H, int32_t state_dim,
                                  int32_t act_dim, const float *d_s0, int64_t s0_rows, float *d_A_out, float *d_S,
                                  ssc_stream_t stream) {
    SSC_REQUIRE(n_items >= 1, "ssc_mpc_forward_sim_many_mfma: n_items %d < 1", n_items);
    if (n_items > 65535)
        return set_error(SSC_EUNSUPPORTED, "ssc_mpc_forward_sim_many_mfma: %d items > 65535 (one grid row each)", n_items);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_mpc_forward_sim_many_mfma: NULL item array");
    SSC_REQUIRE(sp != nullptr, "ssc_mpc_forward_sim_many_mfma: NULL descriptor");
    SSC_REQUIRE(m >= 0 && H >= 1, "ssc_mpc_forward_sim_many_mfma: m = %lld, H = %d", (long long)m, H);
    SSC_REQUIRE(state_dim >= 1 && state_dim <= SSC_MAX_STATE && act_dim >= 1 && act_dim <= SSC_MAX_ACT,
                "ssc_mpc_forward_sim_many_mfma: state_dim %d / act_dim %d out of range", state_dim, act_dim);
    SSC_REQUIRE(sp->n_samples >= 1 && m % sp->n_samples == 0, "ssc_mpc_forward_sim_many_mfma: n_samples %d must divide m = %lld",
                sp->n_samples, (long long)m);
    SSC_REQUIRE(s0_rows >= 1 && (m == 0 || m % s0_rows == 0), "ssc_mpc_forward_sim_many_mfma: s0_rows must divide m");
    for (int a = 0; a < act_dim; ++a)
        SSC_REQUIRE(sp->low[a] <= sp->high[a], "ssc_mpc_forward_sim_many_mfma: low > high for action component %d", a);
    SSC_REQUIRE(sp->d_live_list == nullptr && sp->d_n_live == nullptr,
                "ssc_mpc_forward_sim_many_mfma: a compact live list maps slots to arbitrary problems (a workgroup's weights "
                "would not be uniform): d_live_list / d_n_live must be NULL");
    const int64_t P = m / sp->n_samples;
    std::vector<MfmaItemRange> ranges;
    int64_t rows_max = 0;
    int cls = -1, cls_item = -1;
    for (int i = 0; i < n_items; ++i) {
        const ssc_mpc_sim_many_mfma_item &it = h_items[i];
        char who[64];
        snprintf(who, sizeof who, "ssc_mpc_forward_sim_many_mfma: item %d", i);
        SSC_REQUIRE(it.n_problems >= 0, "%s: n_problems %d < 0", who, it.n_problems);
        if (it.n_problems == 0) continue;      // skipped: its workgroups leave at once, nothing else of the item is read
        if (int rc = validate_mlp(&it.mlp, who)) return rc;
        SSC_REQUIRE(it.mlp.dims[0] == state_dim + act_dim && it.mlp.dims[it.mlp.n_layers] == state_dim,
                    "%s: network is %d -> %d, expected %d -> %d", who, it.mlp.dims[0], it.mlp.dims[it.mlp.n_layers],
                    state_dim + act_dim, state_dim);
        const int c = many_class(&it.mlp, state_dim, act_dim);
        if (c < 0)
            return set_error(SSC_EUNSUPPORTED, "%s: no many-call class (one hidden layer <= 512 or two equal ones <= 128, inputs "
                             "and outputs <= 4); simulate it with ssc_mpc_forward_sim", who);
        if (cls < 0) { cls = c; cls_item = i; }
        if (c != cls)
            return set_error(SSC_EUNSUPPORTED, "ssc_mpc_forward_sim_many_mfma: items %d and %d are of classes %d and %d: one "
                             "call serves one class", cls_item, i, cls, c);
        SSC_REQUIRE(it.d_image != nullptr, "%s: NULL d_image", who);
        SSC_REQUIRE((reinterpret_cast<uintptr_t>(it.d_image) & 15) == 0, "%s: d_image must be 16-byte aligned", who);
        const size_t need = dyn_mfma_workspace_bytes(&it.mlp);
        SSC_REQUIRE(it.image_bytes >= need, "%s: image %zu < %zu bytes", who, it.image_bytes, need);
        SSC_REQUIRE(it.problem0 >= 0 && (int64_t)it.problem0 + it.n_problems <= P,
                    "%s: problems [%d, %lld) outside [0, %lld)", who, it.problem0, (long long)it.problem0 + it.n_problems,
                    (long long)P);
        const int64_t rows = (int64_t)it.n_problems * sp->n_samples;
        SSC_REQUIRE(rows <= 0x7fffffffLL, "%s: %lld rows (the kernel indexes an item's rows with 32 bits)", who, (long long)rows);
        ranges.push_back(MfmaItemRange{it.problem0, (int64_t)it.problem0 + it.n_problems, i});
        rows_max = std::max(rows_max, rows);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1, top = 0; k < ranges.size(); ++k) {      // top: the range before this one that reaches furthest
        const MfmaItemRange &r = ranges[k], &o = ranges[top];
        SSC_REQUIRE(o.end <= r.begin, "ssc_mpc_forward_sim_many_mfma: items %d and %d: problems [%lld, %lld) and [%lld, %lld) overlap",
                    std::min(o.item, r.item), std::max(o.item, r.item), (long long)o.begin, (long long)o.end,
                    (long long)r.begin, (long long)r.end);
        if (r.end > o.end) top = k;
    }
    if (m == 0) return SSC_OK;
    SSC_REQUIRE(d_s0 && d_S, "ssc_mpc_forward_sim_many_mfma: NULL device pointer");
    if (ranges.empty()) return SSC_OK;
    DynSimArgs g{};          // dyn_mfma_forward_sim_sampled's arguments; the image pointers are filled per workgroup
    g.m = m; g.H = H; g.d = state_dim; g.a = act_dim; g.in = state_dim + act_dim; g.out = state_dim; g.fwd_mode = 0;
    g.s0 = d_s0; g.s0_rows = m / s0_rows; g.A = nullptr; g.S = d_S;
    g.sample = 1; g.N = sp->n_samples; g.seed = sp->seed; g.pid0 = sp->problem_id0; g.t = sp->t; g.t_base = sp->d_t_base;
    for (int a = 0; a < SSC_MAX_ACT; ++a) {
        g.low[a] = a < act_dim ? sp->low[a] : 0.0f;
        g.span[a] = a < act_dim ? sp->high[a] - sp->low[a] : 0.0f;
    }
    g.A_out = d_A_out;
    g.active = sp->d_problem_active;
    hipStream_t s = as_stream(stream);
    switch (cls) {
    case 0: return launch_many<1, 1, false>(g, d_items, rows_max, n_items, s);
    case 1: return launch_many<4, 1, false>(g, d_items, rows_max, n_items, s);
    case 2: return launch_many<16, 1, false>(g, d_items, rows_max, n_items, s);
    case 3: return launch_many<1, 2, false>(g, d_items, rows_max, n_items, s);
    case 4: return launch_many<1, 2, true>(g, d_items, rows_max, n_items, s);
    case 5: return launch_many<4, 2, false>(g, d_items, rows_max, n_items, s);
    default: return launch_many<4, 2, true>(g, d_items, rows_max, n_items, s);
    }
}

}  // extern "C"
