// actor_many.hip -- ssc_actor_forward_many: the batched DDPG actor forward (actor.hip) for a POPULATION of actors in one
// launch.  Grid row y = item y: a contiguous range of the call's rows with a network of its own; grid x = the item's blocks,
// ANCHORED AT THE ITEM'S FIRST ROW, so the partition into blocks and waves is that of the actor's own call on its slice.  A
// block reads its item at a block-uniform address (scalar loads), moves the observation / action pointers to the item's
// first row and runs the body the single call dispatches for the descriptor at m > 32 (actor_device.h): every owned row
// gets, bit for bit, what ssc_actor_forward[_rms] on the slice gives it.
//
// NOTE: compiled with the flags of actor.hip (-fno-honor-nans, MFMA results in VGPRs) -- the bits must match.
#include <algorithm>
#include <stdio.h>
#include <vector>

#include "actor_device.h"
#include "ssc_host.h"

namespace ssc {

typedef const __attribute__((address_space(4))) ssc_actor_many_item *const_actor_item;   // uniform reads: scalar loads

// bodies (ssc_actor_many_class = 2 * body + has_rms)
enum { kBodyF32 = 0, kBodyMfmaSmall = 2, kBodyMfmaMid = 4, kBodyMfmaLds = 6, kBodyGeneric = 8 };

static __device__ __forceinline__ ActorWeights item_weights(const_actor_item it) {
    return ActorWeights{it->actor.W1, it->actor.b1, it->actor.W2, it->actor.b2, it->actor.W3, it->actor.b3,
                        it->actor.obs_dim, it->actor.h1, it->actor.h2, it->actor.last_layer_tanh, it->actor.obs_clip,
                        it->actor.ln1_g, it->actor.ln1_b, it->actor.ln2_g, it->actor.ln2_b};
}

// the fixed-shape bodies: 256-thread blocks, one row per lane
template <class Net, int OBS, bool RMS>
__global__ __launch_bounds__(kBlock) void actor_many_kernel(const ssc_actor_many_item *items, const float *__restrict__ obs,
                                                            float *__restrict__ act) {
    const const_actor_item it = (const_actor_item)items + blockIdx.y;
    const int64_t rows = it->rows;
    if ((int64_t)blockIdx.x * kBlock >= rows) return;   // a surplus block, or an empty item: block-uniform, no barrier yet
    const ActorWeights w = item_weights(it);
    const int64_t row0 = it->row0;
    if constexpr (RMS) actor_net_body<Net, OBS>(w, rows, obs + row0 * OBS, act + row0, it->d_rms);
    else actor_net_body<Net, OBS>(w, rows, obs + row0 * OBS, act + row0);
}

// the generic body: 64-thread blocks, dynamic LDS sized by the widest item of the call
template <bool RMS>
__global__ __launch_bounds__(64) void actor_many_generic_kernel(const ssc_actor_many_item *items, const float *__restrict__ obs,
                                                                float *__restrict__ act) {
    extern __shared__ float h1s[];
    const const_actor_item it = (const_actor_item)items + blockIdx.y;
    const int64_t rows = it->rows;
    if ((int64_t)blockIdx.x * 64 >= rows) return;
    const ActorWeights w = item_weights(it);
    const int act_dim = it->actor.act_dim;
    const int64_t row0 = it->row0;
    if constexpr (RMS) actor_generic_body(w, act_dim, rows, obs + row0 * w.obs_dim, act + row0 * act_dim, h1s, it->d_rms);
    else actor_generic_body(w, act_dim, rows, obs + row0 * w.obs_dim, act + row0 * act_dim, h1s);
}

static size_t generic_lds(const ssc_actor_desc *a) {
    return (size_t)(a->h1 + (a->ln1_g != nullptr ? a->h2 : 0)) * 64 * sizeof(float);
}

// ssc_actor_forward's per-descriptor checks with its codes, `who` in front; SSC_OK: the descriptor has a body
static int check_actor(const char *who, const ssc_actor_desc *a) {
    SSC_REQUIRE(a->obs_dim >= 1 && a->obs_dim <= SSC_MAX_STATE && a->act_dim >= 1 && a->act_dim <= SSC_MAX_ACT,
                "%s: obs_dim %d / act_dim %d out of range", who, a->obs_dim, a->act_dim);
    SSC_REQUIRE(a->h1 >= 1 && a->h2 >= 1, "%s: bad hidden sizes", who);
    SSC_REQUIRE(a->W1 && a->b1 && a->W2 && a->b2 && a->W3 && a->b3, "%s: NULL device pointer", who);
    const bool ln = a->ln1_g != nullptr;
    SSC_REQUIRE(ln == (a->ln1_b != nullptr) && ln == (a->ln2_g != nullptr) && ln == (a->ln2_b != nullptr),
                "%s: the four LayerNorm pointers come together", who);
    if (ln && a->precision != SSC_PREC_F32)
        return set_error(SSC_EUNSUPPORTED, "%s: LayerNorm networks run on the fp32 kernels (precision SSC_PREC_F32)", who);
    if (a->precision == SSC_PREC_BF16_MFMA) {
        if (a->act_dim != 1 || (a->obs_dim != 2 && a->obs_dim != 3) || a->h1 > 224 || a->h2 > 128)
            return set_error(SSC_EUNSUPPORTED, "%s: MFMA path needs obs_dim 2|3, act_dim 1, h1 <= 224, h2 <= 128", who);
        return SSC_OK;
    }
    if (a->precision != SSC_PREC_F32) return set_error(SSC_EINVAL, "%s: unknown precision", who);
    if (!ln && a->act_dim == 1 && a->h1 == 64 && a->h2 == 32 && (a->obs_dim == 2 || a->obs_dim == 3)) return SSC_OK;
    if (a->h1 > 512) return set_error(SSC_EUNSUPPORTED, "%s: h1 %d > 512", who, a->h1);
    if (generic_lds(a) > 160 * 1024)
        return set_error(SSC_EUNSUPPORTED, "%s: h1 %d + h2 %d too wide for the LayerNorm kernel", who, a->h1, a->h2);
    return SSC_OK;
}

// ssc_actor_forward's dispatch at m > 32, as a body id; -1: refused
static int many_body(const ssc_actor_desc *a) {
    if (a == nullptr || a->obs_dim < 1 || a->obs_dim > SSC_MAX_STATE || a->act_dim < 1 || a->act_dim > SSC_MAX_ACT || a->h1 < 1 ||
        a->h2 < 1)
        return -1;
    const bool ln = a->ln1_g != nullptr;
    if (a->precision == SSC_PREC_BF16_MFMA) {
        if (ln || a->act_dim != 1 || (a->obs_dim != 2 && a->obs_dim != 3) || a->h1 > 224 || a->h2 > 128) return -1;
        const int o = a->obs_dim - 2;
        if (a->h1 > 128 || a->h2 > 64) return kBodyMfmaLds + o;
        return (a->h1 <= 64 && a->h2 <= 32 ? kBodyMfmaSmall : kBodyMfmaMid) + o;
    }
    if (a->precision != SSC_PREC_F32) return -1;
    if (!ln && a->act_dim == 1 && a->h1 == 64 && a->h2 == 32 && (a->obs_dim == 2 || a->obs_dim == 3)) return kBodyF32 + a->obs_dim - 2;
    if (a->h1 > 512 || generic_lds(a) > 160 * 1024) return -1;
    return kBodyGeneric;
}

template <class Net, int OBS>
static int launch_fixed(bool rms, const ssc_actor_many_item *d_items, int64_t rows_max, int n_items, const float *d_obs, float *d_act,
                        hipStream_t s) {
    const dim3 grid(blocks_for(rows_max), (unsigned)n_items), block(kBlock);
    if (rms) hipLaunchKernelGGL((actor_many_kernel<Net, OBS, true>), grid, block, 0, s, d_items, d_obs, d_act);
    else hipLaunchKernelGGL((actor_many_kernel<Net, OBS, false>), grid, block, 0, s, d_items, d_obs, d_act);
    return check_launch("ssc_actor_forward_many");
}

struct ActorItemRange {
    int64_t begin, end;
    int item;
    bool operator<(const ActorItemRange &o) const { return begin != o.begin ? begin < o.begin : item < o.item; }
};

}  // namespace ssc

using namespace ssc;

extern "C" {

int ssc_actor_many_class(const ssc_actor_desc *a, int has_rms) {
    const int b = many_body(a);
    return b < 0 ? -1 : 2 * b + (has_rms ? 1 : 0);
}

int ssc_actor_forward_many(const ssc_actor_many_item *h_items, const ssc_actor_many_item *d_items, int32_t n_items, int64_t m,
                           const float *d_obs, float *d_act, ssc_stream_t stream) {
    SSC_REQUIRE(n_items >= 1, "ssc_actor_forward_many: n_items %d < 1", n_items);
    if (n_items > 65535) return set_error(SSC_EUNSUPPORTED, "ssc_actor_forward_many: %d items > 65535 (one grid row each)", n_items);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_actor_forward_many: NULL item array");
    SSC_REQUIRE(m >= 0, "ssc_actor_forward_many: m = %lld < 0", (long long)m);
    std::vector<ActorItemRange> ranges;
    int64_t rows_max = 0;
    size_t lds_max = 0;
    int cls = -1, cls_item = -1, obs_dim = 0, act_dim = 0;
    for (int i = 0; i < n_items; ++i) {
        const ssc_actor_many_item &it = h_items[i];
        char who[64];
        snprintf(who, sizeof who, "ssc_actor_forward_many: item %d", i);
        SSC_REQUIRE(it.rows >= 0, "%s: rows %lld < 0", who, (long long)it.rows);
        if (it.rows == 0) continue;            // skipped: its blocks leave at once, nothing else of the item is read
        if (int rc = check_actor(who, &it.actor)) return rc;
        const int c = ssc_actor_many_class(&it.actor, it.d_rms != nullptr);
        if (c < 0) return set_error(SSC_EUNSUPPORTED, "%s: no many-call class", who);
        if (cls < 0) { cls = c; cls_item = i; obs_dim = it.actor.obs_dim; act_dim = it.actor.act_dim; }
        if (c != cls)
            return set_error(SSC_EUNSUPPORTED, "ssc_actor_forward_many: items %d and %d are of classes %d and %d: one call serves "
                             "one class", cls_item, i, cls, c);
        if (it.actor.obs_dim != obs_dim || it.actor.act_dim != act_dim)
            return set_error(SSC_EUNSUPPORTED, "ssc_actor_forward_many: items %d and %d differ in obs_dim / act_dim (%d / %d and "
                             "%d / %d): one call serves one row layout", cls_item, i, obs_dim, act_dim, it.actor.obs_dim,
                             it.actor.act_dim);
        SSC_REQUIRE(it.row0 >= 0 && it.row0 <= m && it.rows <= m - it.row0, "%s: rows [%lld, %lld + %lld) outside [0, %lld)", who,
                    (long long)it.row0, (long long)it.row0, (long long)it.rows, (long long)m);
        ranges.push_back(ActorItemRange{it.row0, it.row0 + it.rows, i});
        rows_max = std::max(rows_max, it.rows);
        if (cls / 2 == kBodyGeneric) lds_max = std::max(lds_max, generic_lds(&it.actor));
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1, top = 0; k < ranges.size(); ++k) {      // top: the range before this one that reaches furthest
        const ActorItemRange &r = ranges[k], &o = ranges[top];
        SSC_REQUIRE(o.end <= r.begin, "ssc_actor_forward_many: items %d and %d: rows [%lld, %lld) and [%lld, %lld) overlap",
                    std::min(o.item, r.item), std::max(o.item, r.item), (long long)o.begin, (long long)o.end, (long long)r.begin,
                    (long long)r.end);
        if (r.end > o.end) top = k;
    }
    if (m == 0 || ranges.empty()) return SSC_OK;
    SSC_REQUIRE(d_obs && d_act, "ssc_actor_forward_many: NULL device pointer");
    hipStream_t s = as_stream(stream);
    const bool rms = cls & 1;
    switch (cls / 2) {
    case kBodyF32: return launch_fixed<ActorF32<2, 64, 32>, 2>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    case kBodyF32 + 1: return launch_fixed<ActorF32<3, 64, 32>, 3>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    case kBodyMfmaSmall: return launch_fixed<ActorMfma<2, 2, 1>, 2>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    case kBodyMfmaSmall + 1: return launch_fixed<ActorMfma<3, 2, 1>, 3>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    case kBodyMfmaMid: return launch_fixed<ActorMfma<2, 4, 2>, 2>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    case kBodyMfmaMid + 1: return launch_fixed<ActorMfma<3, 4, 2>, 3>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    case kBodyMfmaLds: return launch_fixed<ActorMfmaLds<2, 7, 4>, 2>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    case kBodyMfmaLds + 1: return launch_fixed<ActorMfmaLds<3, 7, 4>, 3>(rms, d_items, rows_max, n_items, d_obs, d_act, s);
    default: break;
    }
    const void *kern = rms ? reinterpret_cast<const void *>(actor_many_generic_kernel<true>)
                           : reinterpret_cast<const void *>(actor_many_generic_kernel<false>);
    if (lds_max > 64 * 1024)
        if (int rc = check_hip(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max), "hipFuncSetAttribute"))
            return rc;
    const dim3 grid(blocks_for(rows_max, 64), (unsigned)n_items), block(64);
    if (rms) hipLaunchKernelGGL(actor_many_generic_kernel<true>, grid, block, lds_max, s, d_items, d_obs, d_act);
    else hipLaunchKernelGGL(actor_many_generic_kernel<false>, grid, block, lds_max, s, d_items, d_obs, d_act);
    return check_launch("ssc_actor_forward_many(generic)");
}

}  // extern "C"
