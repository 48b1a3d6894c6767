// ddpg_layout.h -- what every DDPG learner must agree on, stated once: the flat parameter layout of a network, and which
// learner serves a descriptor.  Host and device; nothing here needs a GPU (tests/host_harness compiles it for the CPU and
// tests/test_ddpg_layout_host.py holds it to agents.views_like, the Python statement of the same layout).
#pragma once

#include <stddef.h>

#include "ssc.h"

namespace ssc {

constexpr int kB = 64;       // batch size = lanes of a wave
constexpr int kP = kB + 4;   // padded LDS row: 16-B aligned rows (float4 access over 4 samples); a stride of
                             // 68 dwords keeps both ds_read_b128 column gathers and ds_write_b128 conflict-free

// ---- the flat parameter vector of one network: [W1|b1|(beta1|gamma1)|W2|b2|(beta2|gamma2)|W3|b3] --------------------
// (TensorFlow's trainable_vars order; W row-major [in][out]).  The moments of MpiAdam use the same offsets.
struct DdpgNet {
    int in, h1, h2, out;     // actor: obs -> h1 -> h2 -> act ; critic: obs -> h1 (+act) -> h2 -> 1
    int extra;               // rows concatenated to the first hidden layer (critic: act_dim, actor: 0)
    int ln;                  // 1: LayerNorm beta, then gamma behind both hidden layers (ssc_ddpg_desc::layer_norm)
    constexpr int oW1() const { return 0; }
    constexpr int ob1() const { return in * h1; }
    constexpr int obe1() const { return ob1() + h1; }           // ln only
    constexpr int og1() const { return obe1() + h1; }
    constexpr int oW2() const { return ob1() + h1 + (ln ? 2 * h1 : 0); }
    constexpr int ob2() const { return oW2() + (h1 + extra) * h2; }
    constexpr int obe2() const { return ob2() + h2; }           // ln only
    constexpr int og2() const { return obe2() + h2; }
    constexpr int oW3() const { return ob2() + h2 + (ln ? 2 * h2 : 0); }
    constexpr int ob3() const { return oW3() + h2 * out; }
    constexpr int total() const { return ob3() + out; }
};

struct DdpgNets { DdpgNet A, C; };   // actor, critic (their targets share the layouts)

inline DdpgNets ddpg_nets(const ssc_ddpg_desc *d) {
    const int ln = d->layer_norm ? 1 : 0;
    return DdpgNets{DdpgNet{d->obs_dim, d->actor_h1, d->actor_h2, d->act_dim, 0, ln},
                    DdpgNet{d->obs_dim, d->critic_h1, d->critic_h2, 1, d->act_dim, ln}};
}

// ---- which learner serves a descriptor ------------------------------------------------------------------------------
// The shipped 64-32 / batch-64 shape has a kernel of its own (ddpg_train_fixed.hip), which also runs batches of several
// 64-row tiles in front of the multi-workgroup apply pass; other nets <= 64 wide at batch 64 run the single-workgroup
// step interpreter (ddpg_train.hip) while its LDS carve fits; everything else -- wider layers (the reference's 128-64
// and 200-100 grid), other batch sizes, LayerNorm, critic_l2_reg, clip_norm -- the multi-workgroup kernels of
// ddpg_train_wide.hip, which need a workspace.
constexpr int kFixedH1 = 64, kFixedH2 = 32;

inline bool ddpg_fixed_nets(const ssc_ddpg_desc *d) {
    return (d->obs_dim == 2 || d->obs_dim == 3) && d->act_dim == 1 && d->actor_h1 == kFixedH1 && d->actor_h2 == kFixedH2 &&
           d->critic_h1 == kFixedH1 && d->critic_h2 == kFixedH2;
}
inline bool ddpg_fixed_shape(const ssc_ddpg_desc *d) { return d->batch_size == kB && ddpg_fixed_nets(d); }
inline bool ddpg_fixed_tiled_shape(const ssc_ddpg_desc *d) {
    return ddpg_fixed_nets(d) && !d->layer_norm && d->batch_size > kB && d->batch_size % kB == 0 && d->batch_size <= 4096;
}

// what the single-workgroup kernels can run at all
inline bool ddpg_narrow(const ssc_ddpg_desc *d) {
    return !d->layer_norm && d->critic_l2_reg == 0.0f && !(d->clip_norm > 0.0f) && d->batch_size == kB && d->actor_h1 <= 64 &&
           d->actor_h2 <= 64 && d->critic_h1 <= 64 && d->critic_h2 <= 64;
}

// The interpreter's LDS carve, offsets in floats: activation / delta rows of kP floats, then the four parameter vectors.
struct InterpCarve {
    int S, RT;            // state rows; r, terminal, y (target Q), -Q(s, pi(s))
    int X2;               // critic: relu(layer 1) rows, then the action rows
    int CA2, S2;          // critic layer 2; before that the next-state rows (read by the target pass's first two steps only)
    int DQ, DZ2;
    int DZ1, X2B;         // critic layer-1 deltas; before that the target pass's X2B
    int U1, U2, PI, DZ3A, DZ1A;
    int CB2, DZB2;        // also target-pass scratch
    int DZ2A;             // actor layer-2 deltas = CB2: written (bwd a3) after the last read of CB2, and in the target pass
                          // (target actor layer 2) read for the last time before CB2 is written
    int TA, TC, TTA, TTC; // actor, critic, target actor, target critic
    int floats;           // the whole carve; what is left of the LDS takes Adam moments of small layers
};
constexpr int kInterpLdsFloats = (160 * 1024 - 128) / 4;   // 64 B of static LDS (loss partials, Adam step sizes)

inline InterpCarve ddpg_interp_carve(const ssc_ddpg_desc *d) {
    const DdpgNets n = ddpg_nets(d);
    const DdpgNet &A = n.A, &C = n.C;
    InterpCarve c{};
    int p = 0;
    auto take = [&](int rows) { const int q = p; p += rows * kP; return q; };
    c.S = take(d->obs_dim); c.RT = take(4);
    c.X2 = take(C.h1 + d->act_dim);
    c.CA2 = c.S2 = take(C.h2 > d->obs_dim ? C.h2 : d->obs_dim);
    c.DQ = take(1); c.DZ2 = take(C.h2);
    c.DZ1 = c.X2B = take(C.h1 + d->act_dim);
    c.U1 = take(A.h1); c.U2 = take(A.h2); c.PI = take(d->act_dim);
    c.DZ3A = take(d->act_dim); c.DZ1A = take(A.h1);
    c.CB2 = c.DZ2A = take(C.h2 > A.h2 ? C.h2 : A.h2); c.DZB2 = take(C.h2);
    // every parameter vector starts on a 16-byte boundary: the dense passes read weights as float4 (a
    // misaligned ds_read_b128 was measured 6x slower)
    auto al4 = [](int x) { return (x + 3) & ~3; };
    c.TA = al4(p); c.TC = al4(c.TA + A.total()); c.TTA = al4(c.TC + C.total()); c.TTC = al4(c.TTA + A.total());
    c.floats = c.TTC + C.total();
    return c;
}

enum DdpgPath { DDPG_FIXED, DDPG_FIXED_TILED, DDPG_INTERPRETER, DDPG_WIDE, DDPG_NEEDS_WORKSPACE };

// have_ws: the call brought a workspace (ssc_ddpg_train does not); have_rms: normalize_observations statistics;
// want_interp / want_wide: SSC_DDPG_INTERPRETER=1 / SSC_DDPG_WIDE=1 (A/B measurements, and the tests that check every
// path against the oracle on the shipped shape); the latter counts only with a workspace.
inline DdpgPath ddpg_learner_path(const ssc_ddpg_desc *d, bool have_ws, bool have_rms, bool want_interp, bool want_wide) {
    want_wide = want_wide && have_ws;
    const bool narrow = ddpg_narrow(d);
    if (!have_ws && !narrow) return DDPG_NEEDS_WORKSPACE;
    // the shipped 64-32 networks at a batch of several 64-row tiles: the straight-line kernel per tile, then the apply pass
    if (have_ws && !want_wide && !want_interp && ddpg_fixed_tiled_shape(d)) return DDPG_FIXED_TILED;
    if (!narrow || want_wide) return DDPG_WIDE;
    if (ddpg_fixed_shape(d) && !want_interp) return DDPG_FIXED;
    // the step interpreter has no normalising build: with statistics its shapes run on the multi-workgroup kernels
    // (statistics come only through ssc_ddpg_train_ws_rms, which has a workspace)
    if (have_rms) return DDPG_WIDE;
    // 64-wide layers in both networks: the activation rows alone pass the LDS
    if (ddpg_interp_carve(d).floats > kInterpLdsFloats) return have_ws ? DDPG_WIDE : DDPG_NEEDS_WORKSPACE;
    return DDPG_INTERPRETER;
}

}  // namespace ssc
