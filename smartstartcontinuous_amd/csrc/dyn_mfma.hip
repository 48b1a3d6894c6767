// dyn_mfma.hip -- bf16-MFMA path of the NND_MB dynamics model: the H-step forward simulation
// Dyn_Model.do_forward_sim (NN_Dynamics_Model/dynamics_model.py:204-240) over
// feedforward_network (feedforward_network.py:3-23) as ONE persistent kernel.
//
// Shape of the work (BASELINE config 4: in 4, 2x500 hidden, out 3): 507 kflop per row-step, of
// which 500 k are the [rows,500]x[500,500] hidden contraction -> MFMA-bound (bf16 dense peak
// ~2.5 PFLOP/s).  The state feeds back every step, so the H loop lives inside the kernel and
// NOTHING but the [H+1][m][d] trajectory (the result) and the per-step actions touch HBM.
//
// Mapping to CDNA4:
//   * a block = 512 threads = 8 waves x 32 rows; waves w and w+4 share a SIMD (2 waves per SIMD, 256
//     VGPRs each).  A wave holds the first hidden layer of its 32 rows as bf16 MFMA fragments in
//     registers (128 VGPRs at depth 512); the waves of a block share the weight fragments through LDS.
//   * every layer is computed TRANSPOSED: D[unit][row] = W^T[unit][k] * H[k][row], i.e. the weights
//     are the MFMA A operand and the activations the B operand.  All contractions run on
//     v_mfma_f32_16x16x32_bf16 (on this chip the 16x16x32 shape holds a ~6.5 % higher clock than
//     32x32x16 at equal cycles: tools/exp_dyn_clock.py).  Two 16x16 accumulator tiles of a layer (units
//     32p..32p+15 and 32p+16..32p+31 of 16 rows) are -- after ReLU + v_cvt_pk_bf16_f32 in registers --
//     exactly ONE B fragment (32 k x 16 rows) of the next layer under a fixed permutation of k that is
//     folded into the packed weights: activations never touch LDS and no lane moves
//     (cdna_hip_programming.md section 3, "An accumulator tile as the next MFMA's operand").
//   * layer 1 (K = state+action <= 12) also runs on the bf16 MFMA at fp32-level accuracy by splitting
//     x and W1 into bf16 head + bf16 residual (3 products per input, bias in two more k slots).
//   * layer-2 output tiles (32 units) are consumed immediately by the output layer (one more MFMA per
//     16 rows), so the second hidden activation is never materialised.
//   * W2 is packed once per call into fragment order (bf16) and streamed L2 -> LDS by LDS-DMA one
//     32-unit output tile (32 KiB at depth 512) at a time through a ring of 3 slots, one barrier per
//     tile, the two waves of a SIMD half a tile out of phase (details at tile_body below).
#include "dyn_mfma_sim.h"

namespace ssc {

struct DynNet {
    const float *W1, *b1, *W2, *b2, *W3, *b3;  // W3/b3 = output layer; W2/b2 unused when nfc == 1
    int in, depth, out, nfc;
    bool biask;  // b2 in the spare k slots depth, depth+1 of the hidden contraction (needs depth + 2 <= 32*UT)
    bool compact1;  // layer-1 fragments in the compact lane-group layout of the KIN = 4 kernels (see l1_compact below)
};

// Compact layer-1 layout (networks with <= 4 inputs and outputs, i.e. every kernel compiled with KIN = 4): k group g = lane >> 4 of the MFMA carries
// INPUT g alone -- slots 8g + {0, 1, 2} = {xh * wh, xl * wh, xh * wl}, slot 8g + 3 = 1 * (bf16 head of b1 in group 0, its
// residual in group 1), slots 8g + 4..7 unused.  A lane then splits ONE input per step instead of selecting its eight
// slots out of all of them (the per-step input code drops from ~120 to ~16 VALU ops per 16 rows), and a weight fragment
// is 8 bytes per lane instead of 16: the layer-1 image is 16 KB instead of 32 KB, which is what buys the W2 ring its
// fourth 32 KB slot.
__host__ __device__ __forceinline__ bool l1_compact(int in, int out) { return in <= 4 && out <= 4; }   // == the KIN = 4 kernels

__device__ __forceinline__ __bf16 bf16_head(float v) { return (__bf16)v; }
__device__ __forceinline__ __bf16 bf16_resid(float v) { return (__bf16)(v - (float)(__bf16)v); }

__global__ __launch_bounds__(256) void dyn_pack_kernel(DynNet n, int UT, DynPack pk, ssc_norm nm,
                                                       unsigned char *__restrict__ ws) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < 48) {
        const int q = (int)gid >> 3, k = (int)gid & 7;
        float v = 0.0f;
        // 1/std (std == 0 -> inf) so that the z-score is one multiply in the kernel (zscore())
        if (q == 0) v = nm.mean_x[k]; else if (q == 1) v = 1.0f / nm.std_x[k];
        else if (q == 2) v = nm.mean_y[k & 3]; else if (q == 3) v = 1.0f / nm.std_y[k & 3];
        else if (q == 4) v = nm.mean_z[k]; else v = nm.std_z[k];
        reinterpret_cast<float *>(ws + pk.nm)[gid] = v;
        if (gid < 2) reinterpret_cast<int32_t *>(ws + pk.ctr)[gid] = 0;
    }
    const int64_t n_a2 = (n.nfc == 2) ? (int64_t)UT * UT * 2 * 64 * 8 : 0;
    const int64_t n_a3 = (int64_t)UT * 4 * 8 * 8;
    const int64_t n_a1 = (int64_t)kMaxKS1 * 2 * UT * 64 * 8;
    const int64_t n_b = (int64_t)UT * 32;
    int64_t e = gid;
    if (e < n_a2) {
        const int j = e & 7, lane = (e >> 3) & 63;
        const int f = (int)((e >> 9) % (2 * UT)), jt = (int)((e >> 9) / (2 * UT));
        const int u = frag_unit(f >> 1, lane >> 4, j), col = jt * 32 + 16 * (f & 1) + (lane & 15);
        __bf16 v = (__bf16)0.0f;
        if (col < n.depth) {
            if (u < n.depth) v = (__bf16)n.W2[(int64_t)u * n.depth + col];
            else if (n.biask && u == n.depth) v = bf16_head(n.b2[col]);
            else if (n.biask && u == n.depth + 1) v = bf16_resid(n.b2[col]);
        }
        reinterpret_cast<__bf16 *>(ws + pk.a2)[e] = v;
        return;
    }
    e -= n_a2;
    if (e < n_a3) {
        // MFMA row m = 0..15 of the output layer computes output (m & omask): with <= 4 outputs every k-group lane
        // of a batch row then ends up holding ALL outputs in its 4 accumulator registers (no lane exchange)
        const int j = e & 7, o8 = (e >> 3) & 7, g = (e >> 6) & 3, p = (int)(e >> 8);
        const int u = frag_unit(p, g, j), o = o8 & (n.out <= 4 ? 3 : 7);
        const float v = (u < n.depth && o < n.out) ? n.W3[(int64_t)u * n.out + o] : 0.0f;
        reinterpret_cast<__bf16 *>(ws + pk.a3)[e] = (__bf16)v;
        return;
    }
    e -= n_a3;
    if (e < n_a1 && n.compact1) {   // [mt][64 lane][4]: slots 0..3 of the lane's k group (l1_compact)
        if (e >= (int64_t)2 * UT * 64 * 4) return;
        const int j = e & 3, lane = (e >> 2) & 63, mt = (int)(e >> 8);
        const int i = lane >> 4, unit = mt * 16 + (lane & 15);
        __bf16 v = (__bf16)0.0f;
        if (unit < n.depth) {
            if (j == 3) v = (i == 0) ? bf16_head(n.b1[unit]) : (i == 1 ? bf16_resid(n.b1[unit]) : (__bf16)0.0f);
            else if (i < n.in) {
                const float w = n.W1[(int64_t)i * n.depth + unit];
                v = (j == 2) ? bf16_resid(w) : bf16_head(w);
            }
        } else if (n.biask && unit < n.depth + 2 && i == 0 && j == 3) {
            v = (__bf16)1.0f;  // the carriers of b2 (see below)
        }
        reinterpret_cast<__bf16 *>(ws + pk.a1)[e] = v;
        return;
    }
    if (e < n_a1) {
        const int j = e & 7, lane = (e >> 3) & 63, mt = (int)((e >> 9) % (2 * UT)), ks = (int)((e >> 9) / (2 * UT));
        const int q = 32 * ks + 8 * (lane >> 4) + j, unit = mt * 16 + (lane & 15);
        __bf16 v = (__bf16)0.0f;
        if (unit < n.depth) {
            if (q == 0) v = bf16_head(n.b1[unit]);
            else if (q == 1) v = bf16_resid(n.b1[unit]);
            else {
                const int i = (q - 2) / 3, c = (q - 2) % 3;
                if (i < n.in) {
                    const float w = n.W1[(int64_t)i * n.depth + unit];
                    v = (c == 2) ? bf16_resid(w) : bf16_head(w);
                }
            }
        } else if (n.biask && unit < n.depth + 2 && q == 0) {
            v = (__bf16)1.0f;  // hidden units depth, depth+1 == ReLU(1 * 1) == 1: the carriers of b2
        }
        reinterpret_cast<__bf16 *>(ws + pk.a1)[e] = v;
        return;
    }
    e -= n_a1;
    if (e < n_b) {  // b2: [jt][mh][g][r]
        const int r = e & 3, g = (e >> 2) & 3, mh = (e >> 4) & 1, jt = (int)(e >> 5);
        const int u = jt * 32 + 16 * mh + 4 * g + r;
        reinterpret_cast<float *>(ws + pk.b2)[e] = (n.nfc == 2 && !n.biask && u < n.depth) ? n.b2[u] : 0.0f;
        return;
    }
    e -= n_b;
    if (e < 16) {  // b3: [g][r], MFMA row 4g + r computes output (4g + r) & omask
        const int o = (int)e & (n.out <= 4 ? 3 : 7);
        reinterpret_cast<float *>(ws + pk.b3)[e] = (o < n.out) ? n.b3[o] : 0.0f;
    }
}

template <int UT, int NFC, bool BIASK, int KIN, bool LAG = false, int MODE = -1, bool WALK = false>
__global__ __launch_bounds__(kDynThreads, 2) void dyn_mfma_sim_kernel(DynSimArgs g) {
    dyn_mfma_sim_body<UT, NFC, BIASK, KIN, LAG, MODE, WALK>(g, DynManyRows{});
}

bool dyn_mfma_supported(const ssc_mlp_desc *mlp, int state_dim, int act_dim) {
    (void)state_dim; (void)act_dim;
    const int nfc = mlp->n_layers - 1;
    if (nfc != 1 && nfc != 2) return false;
    const int depth = mlp->dims[1];
    if (depth > 512 || (nfc == 2 && mlp->dims[2] != depth)) return false;
    if (mlp->dims[0] > kMaxIn || mlp->dims[mlp->n_layers] > SSC_MAX_STATE) return false;
    // streamed W2 (depth > 128) leaves LDS room for one layer-1 k-step only: 2 + 3*in <= 32
    if (nfc == 2 && tiles_for(depth) > 4 && l1_ksteps(mlp->dims[0]) > 1) return false;
    return true;
}

size_t dyn_mfma_workspace_bytes(const ssc_mlp_desc *mlp) {
    const int nfc = mlp->n_layers - 1;
    if (nfc != 1 && nfc != 2) return 256;
    return make_pack(tiles_for(mlp->dims[1]), nfc).total;
}

template <int UT, int NFC, bool BIASK, int KIN, bool LAG = false, int MODE = -1>
static int launch_sim(DynSimArgs g, hipStream_t s) {
    constexpr bool STREAM = (NFC == 2) && (UT > 4);
    size_t lds = (size_t)(LAG ? 4 : dyn_a2_bufs<UT, NFC>()) * UT * 2048 +
                 (KIN == 4 ? (size_t)UT * 1024 : (size_t)l1_ksteps(KIN) * UT * 2048) + (size_t)UT * 512 + (size_t)UT * 128 + 64;
    const int64_t tiles = (g.m + kDynRows - 1) / kDynRows;
    unsigned grid = (unsigned)tiles;
    g.walk = 0;
    const void *kern = reinterpret_cast<const void *>(dyn_mfma_sim_kernel<UT, NFC, BIASK, KIN, LAG, MODE>);
    // Only the 4-slot LAG kernel of the BASELINE shape walks (the other streamed shapes keep a block per tile).
    if constexpr (STREAM && LAG && MODE != 2) {
        // Streamed W2 (one block per CU: 8 waves x 256 VGPRs, ~158 KB of LDS): with more row tiles than CUs a block WALKS
        // over row tiles -- the W2 ring, its barriers and the two wave groups' 1.5-tile lag run on across the row tiles
        // as if the next tile's first step were the next step of the same rows, so the prologue (weight images + the
        // first two W2 tiles: ~4.5 us of a ~92 us tile at H = 4) is paid once per block instead of once per 256 rows.
        // The next tile's start states come in by LDS-DMA under the current tile's last step (stage_next_tile), the
        // tiles beyond a block's first two are handed out by a shared counter (next_tile in the kernel).
        static int n_cu = 0;
        if (n_cu == 0) {
            int dev = 0, v = 0;
            if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
                n_cu = v;
            else
                n_cu = 256;
        }
        const int64_t n_s0 = g.s0_rows > 0 ? (g.m + g.s0_rows - 1) / g.s0_rows : 0;
        const bool can_walk = !g.fwd_mode && g.H > 0 && g.d <= 4 && g.m <= 0x7fffffffLL && n_s0 * g.d * 4 <= 0x7fffffffLL;
        if (can_walk && tiles > n_cu && g.tile_ctr != nullptr) {
            grid = (unsigned)n_cu;
            g.walk = 1;
            lds += (size_t)kNW * 2 * 64 * 4 + 64;   // the start-state staging area and the next-tile slots
            kern = reinterpret_cast<const void *>(dyn_mfma_sim_kernel<UT, NFC, BIASK, KIN, LAG, MODE, true>);
        }
    }
    if (lds > 64 * 1024) {
        int rc = check_hip(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                           "hipFuncSetAttribute(dyn_mfma_sim_kernel)");
        if (rc) return rc;
    }
    void *params[] = {&g};
    if (int rc = check_hip(hipLaunchKernel(kern, dim3(grid), dim3(kDynThreads), params, lds, s), "hipLaunchKernel(dyn_mfma_sim_kernel)"))
        return rc;
    return check_launch("dyn_mfma_sim_kernel");
}

static DynNet make_net(const ssc_mlp_desc *mlp, int UT) {
    const int nfc = mlp->n_layers - 1;
    DynNet n;
    n.in = mlp->dims[0]; n.depth = mlp->dims[1]; n.out = mlp->dims[mlp->n_layers]; n.nfc = nfc;
    n.biask = (nfc == 2) && (n.depth + 2 <= 32 * UT);
    n.compact1 = l1_compact(n.in, n.out);
    n.W1 = mlp->W[0]; n.b1 = mlp->b[0];
    n.W2 = (nfc == 2) ? mlp->W[1] : nullptr; n.b2 = (nfc == 2) ? mlp->b[1] : nullptr;
    n.W3 = mlp->W[nfc]; n.b3 = mlp->b[nfc];
    return n;
}

// write the packed weight image (ssc_dyn_prepare, or the first half of an unprepared call)
int dyn_mfma_prepare(const ssc_mlp_desc *mlp, const ssc_norm *norm, void *wsv, hipStream_t s) {
    const int nfc = mlp->n_layers - 1;
    const int UT = tiles_for(mlp->dims[1]);
    const DynPack pk = make_pack(UT, nfc);
    const DynNet n = make_net(mlp, UT);
    const int64_t n_pack = (nfc == 2 ? (int64_t)UT * UT * 1024 : 0) + (int64_t)UT * 256 + (int64_t)kMaxKS1 * UT * 1024 +
                           (int64_t)UT * 32 + 16;
    ssc_norm nm{};
    if (norm) nm = *norm;
    hipLaunchKernelGGL(dyn_pack_kernel, dim3(blocks_for(n_pack)), dim3(256), 0, s, n, UT, pk, nm,
                       static_cast<unsigned char *>(wsv));
    return check_launch("dyn_pack_kernel");
}

static int run_mfma(const ssc_mlp_desc *mlp, DynSimArgs &g, void *wsv, hipStream_t s) {
    const int nfc = mlp->n_layers - 1;
    const int UT = tiles_for(mlp->dims[1]);
    const DynPack pk = make_pack(UT, nfc);
    const DynNet n = make_net(mlp, UT);
    unsigned char *ws = static_cast<unsigned char *>(wsv);
    SSC_REQUIRE(g.m <= 0x7fffffffLL, "dyn_mfma: m = %lld rows per launch (the kernel indexes rows with 32 bits)", (long long)g.m);
    g.in = n.in; g.out = n.out;
    g.a1 = ws + pk.a1; g.a2 = ws + pk.a2; g.a3 = ws + pk.a3;
    g.b2 = reinterpret_cast<const float *>(ws + pk.b2); g.b3 = reinterpret_cast<const float *>(ws + pk.b3);
    g.nm = reinterpret_cast<const float *>(ws + pk.nm);
    g.tile_ctr = reinterpret_cast<int32_t *>(ws + pk.ctr);
    const int kin = (n.in <= 4 && n.out <= 4) ? 4 : (n.in <= 10 ? 10 : kMaxIn);
#define SSC_DYN_CASE(U, F, B)                                                                 \
    if (UT == U && nfc == F && n.biask == B)                                                  \
        return kin == 4 ? launch_sim<U, F, B, 4>(g, s) : kin == 10 ? launch_sim<U, F, B, 10>(g, s) : launch_sim<U, F, B, kMaxIn>(g, s)
    if (n.compact1 && UT == 16 && nfc == 2) {   // streamed W2, <= 4 inputs and outputs (the BASELINE shape): the 4-slot, 1.5-tile-lag kernel
        const int mode = g.fwd_mode ? 2 : (g.sample ? 1 : 0);
        if (n.biask)
            return mode == 2 ? launch_sim<16, 2, true, 4, true, 2>(g, s) : mode == 1 ? launch_sim<16, 2, true, 4, true, 1>(g, s)
                                                                                     : launch_sim<16, 2, true, 4, true, 0>(g, s);
        return mode == 2 ? launch_sim<16, 2, false, 4, true, 2>(g, s) : mode == 1 ? launch_sim<16, 2, false, 4, true, 1>(g, s)
                                                                                  : launch_sim<16, 2, false, 4, true, 0>(g, s);
    }
    SSC_DYN_CASE(1, 1, false); SSC_DYN_CASE(4, 1, false); SSC_DYN_CASE(16, 1, false);
    SSC_DYN_CASE(1, 2, false); SSC_DYN_CASE(4, 2, false); SSC_DYN_CASE(16, 2, false);
    SSC_DYN_CASE(1, 2, true); SSC_DYN_CASE(4, 2, true); SSC_DYN_CASE(16, 2, true);
#undef SSC_DYN_CASE
    return set_error(SSC_EUNSUPPORTED, "dyn_mfma: no kernel for UT=%d nfc=%d", UT, nfc);
}

int dyn_mfma_forward_sim(const ssc_mlp_desc *mlp, const ssc_norm *norm, int64_t m, int32_t H, int32_t state_dim,
                         int32_t act_dim, const float *d_s0, int64_t s0_rows, const float *d_A, float *d_S,
                         void *ws, bool prepared, hipStream_t s) {
    if (!prepared)
        if (int rc = dyn_mfma_prepare(mlp, norm, ws, s)) return rc;
    DynSimArgs g{};
    g.m = m; g.H = H; g.d = state_dim; g.a = act_dim; g.fwd_mode = 0;
    g.s0 = d_s0; g.s0_rows = m / s0_rows; g.A = d_A; g.S = d_S;
    return run_mfma(mlp, g, ws, s);
}

// the same simulation with the candidate actions drawn inside the kernel (ssc_mpc_forward_sim)
int dyn_mfma_forward_sim_sampled(const ssc_mlp_desc *mlp, const ssc_norm *norm, const ssc_mpc_sampling *sp, int64_t m,
                                 int32_t H, int32_t state_dim, int32_t act_dim, const float *d_s0, int64_t s0_rows,
                                 float *d_A_out, float *d_S, void *ws, bool prepared, hipStream_t s) {
    if (!prepared)
        if (int rc = dyn_mfma_prepare(mlp, norm, ws, s)) return rc;
    DynSimArgs g{};
    g.m = m; g.H = H; g.d = state_dim; g.a = act_dim; g.fwd_mode = 0;
    g.s0 = d_s0; g.s0_rows = m / s0_rows; g.A = nullptr; g.S = d_S;
    g.sample = 1; g.N = sp->n_samples; g.seed = sp->seed; g.pid0 = sp->problem_id0; g.t = sp->t; g.t_base = sp->d_t_base;
    for (int a = 0; a < SSC_MAX_ACT; ++a) {
        g.low[a] = a < act_dim ? sp->low[a] : 0.0f;
        g.span[a] = a < act_dim ? sp->high[a] - sp->low[a] : 0.0f;
    }
    g.A_out = d_A_out;
    g.active = sp->d_problem_active;
    return run_mfma(mlp, g, ws, s);
}

int dyn_mfma_mlp_forward(const ssc_mlp_desc *mlp, int64_t m, const float *d_x, float *d_y, void *ws, bool prepared,
                         hipStream_t s) {
    if (!prepared)
        if (int rc = dyn_mfma_prepare(mlp, nullptr, ws, s)) return rc;
    DynSimArgs g{};
    g.m = m; g.H = 1; g.d = 0; g.a = 0; g.fwd_mode = 1;
    g.s0 = nullptr; g.s0_rows = 1; g.A = d_x; g.S = d_y;
    return run_mfma(mlp, g, ws, s);
}

}  // namespace ssc
