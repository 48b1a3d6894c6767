// rollout.hip -- the fused K-step rollout kernel: the rlTrain inner loop
// (smartstart/reinforcementLearningCore/rlTrain.py:75-100) for n independent envs.
//
//   for k in range(K):  action = agent.get_action(obs)        (:81)
//                       obs2, r, done = env.step(action)      (:84)  [+ gym TimeLimit]
//                       record (obs, a, r, done, obs2)        (:91-94, replay_buffer.py:53)
//                       if done: Summary.append((len, ret)); env.reset()   (:97-114)
//
// MI355X mapping: one thread owns one env; pos/vel/elapsed/return (and the OU state) live
// in VGPRs for all K steps, so the only HBM traffic is the transition log itself --
// [K][n] SoA columns, each wave-instruction storing 256 contiguous bytes (1 dword/lane).
// 25 B per MountainCar env-step, 33 B per Pendulum env-step: the
// kernel is HBM-write-bound by construction.  Episode records go to a ring through a
// wave-aggregated atomic cursor; chunk statistics are reduced wave -> block -> one f64
// atomic per block.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "actor_device.h"
#ifndef SSC_WIDE_ACTOR_ET
#define SSC_WIDE_ACTOR_ET 2   // env tiles per wave of the LDS-staged wide actor (1: two waves per SIMD at 65 536 envs)
#endif
#include "mpc_device.h"
#include "ssc_device.h"
#include "ssc_host.h"


namespace ssc {

struct RolloutArgs {
    int64_t n;
    int32_t K;
    ssc_rollout_state st;
    ssc_transition_log log;
    ssc_episode_ring ring;
    double *stats;
    uint64_t seed, env_id0, step0;
    int32_t has_log, has_ring;
    // one_base: every fp32 column of the log starts within 4 GB above obs[0] (a packed chunk: column c at + c * n floats),
    // so a step's stores share ONE running row pointer and differ in a 32-bit per-lane offset (col_off[c] + 4 * env)
    // computed once -- instead of seven 64-bit row pointers rebuilt from k * row_stride in every step (35 of the ~100
    // instructions of a random-policy step were that scalar address arithmetic)
    int32_t one_base;
    uint32_t col_off[2 * SSC_MAX_OBS + 2];   // bytes: obs[0..OBS), act, rew, obs2[0..OBS)
};

struct PolicyArgs {
    float act_low, act_span, act_high;
    ActorWeights actor;
    float ou_mu, ou_sigma, ou_theta, ou_dt, ou_eps;
    const float *d_eps;  // ssc_ou_desc::d_epsilon: the device value wins over ou_eps and the noise path always runs
};

// ------------------------------------------------------------------------------- envs --
struct McEnv {
    using Const = McConst;
    static constexpr int OBS = 2;
    float pos, vel;
    static SSC_HD Const make_const(const ssc_env_params &p) { return make_mc_const(p); }
    __device__ void load(float a, float b) { pos = a; vel = b; }
    __device__ void observe(float (&o)[OBS]) const { o[0] = pos; o[1] = vel; }
    __device__ void step(const Const &c, float a, float &rew, bool &goal) { mc_step_one(c, pos, vel, a, rew, goal); }
    __device__ void reset(const Const &c, const u32x4 &w) { mc_reset_one(c, w, pos, vel); }
    __device__ float s0() const { return pos; }
    __device__ float s1() const { return vel; }
};

struct PendEnv {
    using Const = PendConst;
    static constexpr int OBS = 3;
    float th, thdot;
    static SSC_HD Const make_const(const ssc_env_params &p) { return make_pend_const(p); }
    __device__ void load(float a, float b) { th = a; thdot = b; }
    __device__ void observe(float (&o)[OBS]) const { pend_observe_one(th, thdot, o[0], o[1], o[2]); }
    __device__ void step(const Const &c, float a, float &rew, bool &goal) {
        pend_step_one(c, th, thdot, a, rew);
        goal = false;
    }
    __device__ void reset(const Const &, const u32x4 &w) { pend_reset_one(w, th, thdot); }
    __device__ float s0() const { return th; }
    __device__ float s1() const { return thdot; }
};

// --------------------------------------------------------------------------- policies --
// A Philox4x32-10 evaluation that can be advanced a few rounds at a time, so that the
// (independent) RNG chain of the NEXT 4-step group is interleaved with the serial dynamics
// chain of the current steps: at 65 536 envs there is one wave per SIMD and instruction-level
// parallelism is the only latency hiding available (DESIGN.md "rollout kernel").
struct PhiloxPipe {
    uint32_t c0, c1, c2, c3, k0, k1;
    __device__ __forceinline__ void start(uint64_t seed, uint64_t env_id, uint64_t t, uint32_t tag) {
        c0 = (uint32_t)env_id; c1 = (uint32_t)(env_id >> 32);
        c2 = (uint32_t)t; c3 = (uint32_t)(((t >> 32) << 8) | tag);
        k0 = (uint32_t)seed; k1 = (uint32_t)(seed >> 32);
    }
    template <int R>
    __device__ __forceinline__ void rounds() {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
            const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
            const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
            c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
    }
    // Keeps the rounds issued so far in the basic block where they were written (the optimiser
    // would otherwise sink the whole evaluation to its single use at the end of the group).
    __device__ __forceinline__ void pin() { asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3)); }
    __device__ __forceinline__ u32x4 get() const { return u32x4{c0, c1, c2, c3}; }
};

// Policy_Random.get_action = U(low, high)  (NN_Dynamics_Model/policy_random.py:14-15).
// One Philox call serves 4 consecutive steps: counter t>>2, word t&3.
template <int OBS>
struct RandomPolicy {
    static constexpr bool kPipelined = true;
    static constexpr bool kFusedActor = false;
    static constexpr int kLanesPerEnv = 1;
    u32x4 cache;
    float low, span;
    __device__ void init(const PolicyArgs &pa, const RolloutArgs &, int64_t) { low = pa.act_low; span = pa.act_span; }
    __device__ float act(const float (&)[OBS], uint64_t seed, uint64_t env_id, uint64_t t, bool first) {
        if (first || (t & 3) == 0) cache = rng_words(seed, env_id, t >> 2, TAG_ACTION);  // wave-uniform branch
        return uniform_f32(pick(cache, (uint32_t)(t & 3)), low, span);
    }
    __device__ float from_word(uint32_t w) const { return uniform_f32(w, low, span); }
    __device__ void on_reset() {}
    __device__ void store(const RolloutArgs &, int64_t) const {}
};

// DDPG_Baselines_agent.get_action (smartstart/RLAgents/DDPG_Baselines_agent.py:206-234):
//   a = actor(obs) + epsilon * OU();  a = clip(a, -1, 1)      (ddpg_editted.py:262-271)
//   a = scale(scale(a))                                        (DDPG_Baselines_agent.py:236-240)
// OU [third-party baselines 0.1.5 ddpg/noise.py]: x += theta*(mu-x)*dt + sigma*sqrt(dt)*N(0,1).
// One Philox call serves the gaussians of 4 consecutive steps (counter t >> 2, both Box-Muller outputs of both
// word pairs: ou_gaussian_from_words).
// the statistics of a NORM policy; an empty base otherwise, so that the plain policy's layout (and code) stays as it was
template <int OBS, bool NORM> struct PolicyNorm {};
template <int OBS> struct PolicyNorm<OBS, true> { ObsNorm<OBS> nrm; };

template <class Net, int OBS, bool NORM = false>
struct ActorPolicy : PolicyNorm<OBS, NORM> {
    static constexpr bool kPipelined = false;
    static constexpr bool kFusedActor = false;
    static constexpr int kLanesPerEnv = Net::kLanesPerEnv;
    Net net;
    u32x4 cache;
    float ou_x, mu, sig_sqrt_dt, theta_dt, eps;
    float low, high, obs_clip;
    bool identity_scale, noisy;

    __device__ void init(const PolicyArgs &pa, const RolloutArgs &ra, int64_t i) {
        net.init(pa.actor);
        mu = pa.ou_mu;
        sig_sqrt_dt = pa.ou_sigma * sqrtf(pa.ou_dt);
        theta_dt = pa.ou_theta * pa.ou_dt;
        eps = fmaxf(pa.d_eps != nullptr ? *pa.d_eps : pa.ou_eps, 0.0f);  // DDPG_Baselines_agent.py:74
        noisy = pa.d_eps != nullptr || eps > 0.0f;
        ou_x = (ra.st.ou_x != nullptr) ? ra.st.ou_x[i] : 0.0f;
        low = pa.act_low;
        high = pa.act_high;
        obs_clip = pa.actor.obs_clip;
        identity_scale = (low == -1.0f && high == 1.0f);
    }
    __device__ float scale(float a) const {  // DDPG_Baselines_agent.py:236-240
        a = fminf(fmaxf(a, -1.0f), 1.0f);
        return identity_scale ? a : fmaf((a + 1.0f) * 0.5f, high - low, low);
    }
    __device__ float act(const float (&obs)[OBS], uint64_t seed, uint64_t env_id, uint64_t t, bool first) {
        float oc[OBS];   // the network sees the clipped observation (ddpg_editted.py:106-109); the log keeps the raw one
#pragma unroll
        for (int c = 0; c < OBS; ++c) {
            if constexpr (NORM) oc[c] = this->nrm.apply(obs[c], c, obs_clip);   // the statistics of this launch
            else oc[c] = clip_obs(obs[c], obs_clip);
        }
        float a = net.forward(oc);
        if (noisy) {  // wave-uniform
            if (first || (t & 3) == 0) cache = rng_words(seed, env_id, t >> 2, TAG_OU);
            const float g = ou_gaussian_from_words(cache, t);
            ou_x = fmaf(sig_sqrt_dt, g, fmaf(theta_dt, mu - ou_x, ou_x));
            a = fmaf(ou_x, eps, a);  // ddpg_editted.py:267-270
        }
        a = fminf(fmaxf(a, -1.0f), 1.0f);  // ddpg_editted.py:271 (action_range = (-1, 1))
        return scale(scale(a));
    }
    __device__ float from_word(uint32_t) const { return 0.0f; }
    __device__ void on_reset() { ou_x = 0.0f; }  // DDPG_Baselines_agent.end_episode -> noise reset (:255-258)
    __device__ void store(const RolloutArgs &ra, int64_t i) const {
        if (ra.st.ou_x != nullptr) ra.st.ou_x[i] = ou_x;
    }
    __device__ void init_norm(const double *rms) { this->nrm.load(rms, OBS); }
};

// The same policy for the shape BASELINE config 3 runs (MountainCar: 2 observations, actor h1 <= 64 / h2 <= 32 on the
// bf16 MFMA, action bounds [-1, 1], epsilon > 0), written so that one env-step is ONE basic block: every
// wave-uniform choice of ActorPolicy (last_layer_tanh, epsilon > 0, the identity scale, the even/odd Philox word
// pair) is a template parameter or resolved by the caller's two-step loop.  With one wave per SIMD the only thing
// that can run under the MFMAs and in the bubbles of the dependent action -> env.step chain is independent work of
// the same wave, and the scheduler only moves code inside a basic block: the noise generation (half a Philox
// evaluation + Box-Muller per step) is that work.
//
// NORM (normalize_observations): the network input is clip((obs - mean) / std); the statistics are read once per launch,
// and the division is a multiply by 1 / std plus one residual correction (q = d r; q += (d - q std) r) -- the step body
// is VALU-issue-bound, and the correctly rounded division is ~10 instructions more per component.  The corrected
// quotient can differ from the correctly rounded one in the last bit.
template <bool LAST_TANH, bool NORM = false>
struct ActorPolicyFused {
    static constexpr bool kPipelined = false;
    static constexpr bool kFusedActor = true;
    static constexpr int kLanesPerEnv = 1;
    ActorMfma2<LAST_TANH> net;
    float ou_x, mu, sig_sqrt_dt, theta_dt, eps;
    float n_mean[2], n_std[2], n_rstd[2], n_clip;   // NORM only

    __device__ void init(const PolicyArgs &pa, const RolloutArgs &ra, int64_t i) {
        net.init(pa.actor);
        mu = pa.ou_mu;
        sig_sqrt_dt = pa.ou_sigma * sqrtf(pa.ou_dt);
        theta_dt = pa.ou_theta * pa.ou_dt;
        eps = pa.d_eps != nullptr ? fmaxf(*pa.d_eps, 0.0f) : pa.ou_eps;  // host value: > 0 (dispatch)
        ou_x = ra.st.ou_x[i];
        if constexpr (NORM) n_clip = pa.actor.obs_clip;
    }
    // Box-Muller like gaussian_f32 in three pieces, so that the radius and the sin output of a word pair computed in
    // the even step are reused by the odd one.  -2 ln(u1) = (-2 ln 2) log2(u1) on the bare v_log_f32: u1 >= 2^-24 is
    // never denormal, so the range handling logf() wraps around the instruction (10 more VALU ops) is dead weight.
    static __device__ __forceinline__ float bm_radius(uint32_t x0) {
        const float u1 = ((float)(x0 >> 8) + 1.0f) * (1.0f / 16777216.0f);
        return __builtin_amdgcn_sqrtf(-1.38629436111989061883f * __builtin_amdgcn_logf(u1));
    }
    static __device__ __forceinline__ float bm_cos(uint32_t x1) { return __builtin_amdgcn_cosf((float)(x1 >> 8) * (1.0f / 16777216.0f)); }
    static __device__ __forceinline__ float bm_sin(uint32_t x1) { return __builtin_amdgcn_sinf((float)(x1 >> 8) * (1.0f / 16777216.0f)); }
    static __device__ __forceinline__ float gaussian(const u32x4 &w, uint64_t t) {  // = ou_gaussian_from_words
        const bool hi = (t & 2) != 0;
        const uint32_t x0 = hi ? w.z : w.x, x1 = hi ? w.w : w.y;
        return bm_radius(x0) * ((t & 1) ? bm_sin(x1) : bm_cos(x1));
    }
    // DDPG_Baselines_agent.get_action for this lane's env; g = the step's N(0,1) draw.  Every multiply-add is
    // spelled out: the step body exists in several copies (head, the four bodies of the main loop, tail) and
    // hipcc decides contraction per copy -- a rollout must not depend on how it was cut into chunks.
    __device__ __forceinline__ float act(const float (&obs)[2], float g) {
        float pre;
        if constexpr (NORM) {
            float o[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float d = obs[c] - n_mean[c];
                const float q = d * n_rstd[c];
                o[c] = clip_obs(fmaf(fmaf(-q, n_std[c], d), n_rstd[c], q), n_clip);
            }
            pre = net.forward_pre(o[0], o[1]);
        } else {
            pre = net.forward_pre(obs[0], obs[1]);
        }
        ou_x = fmaf(sig_sqrt_dt, g, fmaf(theta_dt, mu - ou_x, ou_x));
        const float a = fmaf(ou_x, eps, tanh_fast(pre));  // ddpg_editted.py:267-270
        // clip (:271); scale(scale(.)) (DDPG_Baselines_agent.py:236-240) is the identity on a clipped action for
        // bounds [-1, 1]
        return fminf(fmaxf(a, -1.0f), 1.0f);
    }
    __device__ float from_word(uint32_t) const { return 0.0f; }
    __device__ void on_reset() { ou_x = 0.0f; }
    __device__ void store(const RolloutArgs &ra, int64_t i) const { ra.st.ou_x[i] = ou_x; }
    __device__ void init_norm(const double *rms) {
        ObsNorm<2> nrm;
        nrm.load(rms, 2);
#pragma unroll
        for (int c = 0; c < 2; ++c) { n_mean[c] = nrm.mean[c]; n_std[c] = nrm.std[c]; n_rstd[c] = 1.0f / nrm.std[c]; }
    }
};

// (wave-uniform row pointer) + (32-bit per-lane byte offset) as the SGPR-base form of global_store: the row pointer
// is pinned to SGPRs with readfirstlane (free for a value that already is uniform; otherwise the optimiser
// re-associates base + (row + lane) and every store pays a 64-bit VALU add), and the result is an explicit
// global-address-space pointer (the integer round trip hides the kernel-argument provenance, and a generic
// pointer would turn the stores into flat_store).
#define SSC_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ SSC_GLOBAL T *lane_ptr(T *row_uniform, uint32_t lane_byte_off) {
    const uint64_t v = reinterpret_cast<uint64_t>(row_uniform);
    // (the builtin returns a SIGNED int: without the casts the low half is sign-extended into the high one)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    const uint64_t u = ((uint64_t)hi << 32) | (uint64_t)lo;
    return (SSC_GLOBAL T *)((SSC_GLOBAL char *)u + lane_byte_off);
}

// ----------------------------------------------------------------------------- kernel --
// Per-thread rollout state + the one-step body shared by the generic and the pipelined loop.
template <class EnvT, class PolT, bool LOG, bool ONEBASE = false>
struct Rollout {
    static constexpr int OBS = EnvT::OBS;
    const float *rowp;          // ONEBASE: obs[0] row of the current step (wave-uniform, advanced by the step)
    uint8_t *donep;             // ... and the done row
    uint32_t coff[2 * OBS + 2]; // ... per-lane byte offsets of the fp32 columns: col_off[c] + 4 * env
    const typename EnvT::Const &ec;
    const RolloutArgs &ra;
    EnvT env;
    PolT pol;
    float obs[OBS];
    int32_t el;
    float ep_ret, sum_r;
    int32_t n_goal, n_eps;
    uint64_t env_id;
    uint32_t voff;  // byte offset of this env inside a log row (fp32 columns); row bases are wave-uniform
    bool active;    // this lane's env exists (ragged last wave) ...
    bool owner;     // ... and this lane is the one that reports it (kLanesPerEnv == 2: lanes 0-31 only)

    __device__ __forceinline__ Rollout(const typename EnvT::Const &ec_, const RolloutArgs &ra_) : ec(ec_), ra(ra_) {}

    // Everything after the action is chosen: env.step, bookkeeping, log row k, rare reset path.
    // Inactive lanes of a ragged last wave shadow env n-1 and store the same values to the same
    // addresses as its owner -- benign, and it keeps the hot loop free of exec-mask branches.
    __device__ __forceinline__ void step(float a, int32_t k) {
        float rew;
        bool goal;
        float obs2[OBS];
        env.step(ec, a, rew, goal);
        env.observe(obs2);
        el += 1;
        // bitwise, not short-circuit: no exec-mask region in the hot loop
        const bool done = goal | ((ec.max_episode_steps > 0) & (el >= ec.max_episode_steps));
        ep_ret += rew;
        sum_r += rew;
        n_goal += goal ? 1 : 0;
        if constexpr (LOG && ONEBASE) {
            if (PolT::kLanesPerEnv == 1 || owner) {
                float *rp = const_cast<float *>(rowp);
                uint32_t vo[2 * OBS + 2];
#pragma unroll
                for (int c = 0; c < 2 * OBS + 2; ++c) { vo[c] = coff[c]; asm volatile("" : "+v"(vo[c])); }   // (32-bit offsets: see below)
#pragma unroll
                for (int c = 0; c < OBS; ++c) __builtin_nontemporal_store(obs[c], lane_ptr(rp, vo[c]));
                __builtin_nontemporal_store(a, lane_ptr(rp, vo[OBS]));
                __builtin_nontemporal_store(rew, lane_ptr(rp, vo[OBS + 1]));
                uint32_t vd = voff >> 2;
                asm volatile("" : "+v"(vd));
                *lane_ptr(donep, vd) = (uint8_t)(done ? 1 : 0);            // plain store: see the generic branch
#pragma unroll
                for (int c = 0; c < OBS; ++c) __builtin_nontemporal_store(obs2[c], lane_ptr(rp, vo[OBS + 2 + c]));
            }
            rowp += ra.log.row_stride;          // scalar: one 64-bit add per pointer and step
            donep += ra.log.done_row_stride;
        } else if (LOG && (PolT::kLanesPerEnv == 1 || owner)) {
            const int64_t row = (int64_t)k * ra.log.row_stride;  // wave-uniform
            const int64_t drow = (int64_t)k * ra.log.done_row_stride;
            // The lane offset is re-materialised as a 32-bit value in every step: hoisted out of the loop it becomes a
            // 64-bit VGPR pair and every store then pays a v_lshl_add_u64 (2 passes) for base + offset; a 32-bit
            // VGPR offset against the wave-uniform row base is the SGPR-base form of global_store (no VALU op).
            uint32_t vo = voff;
            asm volatile("" : "+v"(vo));
#define SSC_STORE_F32(val, ptr) __builtin_nontemporal_store((val), (ptr))
#pragma unroll
            for (int c = 0; c < OBS; ++c) SSC_STORE_F32(obs[c], lane_ptr(ra.log.obs[c] + row, vo));
            SSC_STORE_F32(a, lane_ptr(ra.log.act + row, vo));
            SSC_STORE_F32(rew, lane_ptr(ra.log.rew + row, vo));
            // a PLAIN store for the byte column: a wave writes 64 B of it, half a 128-byte line; as a non-temporal
            // store that half line goes to memory on its own, as a plain one the L2 merges it with the neighbour
            // wave's half first.  tools/membw.hip `series .. rows` (profiles/r02/membw_rows.txt): fp32 columns nt +
            // byte column plain 6.0 TB/s, all nt 5.6, all plain 5.4
            *lane_ptr(ra.log.done + drow, vo >> 2) = (uint8_t)(done ? 1 : 0);
#pragma unroll
            for (int c = 0; c < OBS; ++c) SSC_STORE_F32(obs2[c], lane_ptr(ra.log.obs2[c] + row, vo));
        }
#pragma unroll
        for (int c = 0; c < OBS; ++c) obs[c] = obs2[c];
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(done) != 0, 0)) reset_path(done, k);  // wave-uniform, rare
    }

    __device__ __forceinline__ void reset_path(bool done, int32_t k) {
        {
            if (done) {
                if (ra.has_ring && active && owner) {
                    // explicit global-address-space pointers: read out of a population item (rollout_many_kernel) the ring
                    // pointers are generic, and the record would be the one FLAT access inside the step loop
                    // (atomicAdd is this relaxed agent-scope add)
                    const uint32_t slot = __hip_atomic_fetch_add((SSC_GLOBAL uint32_t *)ra.ring.cursor, 1u, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT);
                    if (slot < (uint32_t)ra.ring.capacity) {
                        ((SSC_GLOBAL int64_t *)ra.ring.env_id)[slot] = (int64_t)env_id;
                        ((SSC_GLOBAL int32_t *)ra.ring.length)[slot] = el;
                        ((SSC_GLOBAL float *)ra.ring.ret)[slot] = ep_ret;
                    }
                }
                n_eps += 1;
                env.reset(ec, rng_words(ra.seed, env_id, ra.step0 + (uint64_t)k, TAG_RESET));
                el = 0;
                ep_ret = 0.0f;
                pol.on_reset();
                env.observe(obs);
            }
        }
    }
};

// The whole launch of one (env set, policy): workgroup blockIdx.x of ITS grid row.  Shared by rollout_kernel (arguments in
// the kernarg) and rollout_many_kernel (arguments derived from the pair's item).  The arguments come BY VALUE: by const
// reference hipcc schedules the random policy's step loop differently than it did when this was the kernel itself (same
// instructions, another order); by value the single kernels compile to what they were.
template <class EnvT, class PolT, bool LOG, bool ONEBASE, class... Rms>
__device__ __forceinline__ void rollout_body(const typename EnvT::Const ec, const PolicyArgs pa, const RolloutArgs ra, Rms... rms) {
    constexpr int LPE = PolT::kLanesPerEnv;
    constexpr int kEnvsPerBlock = kBlock / LPE;
    // LPE == 2: a wave covers 32 envs, env j of the wave lives on lanes j and j+32
    const int in_block = (LPE == 1) ? (int)threadIdx.x : (int)((threadIdx.x >> 6) * 32 + (threadIdx.x & 31));
    const int64_t gi = (int64_t)blockIdx.x * kEnvsPerBlock + in_block;
    Rollout<EnvT, PolT, LOG, ONEBASE> r(ec, ra);
    r.active = gi < ra.n;
    r.owner = (LPE == 1) || ((threadIdx.x & 63) < 32);
    const int64_t i = r.active ? gi : ra.n - 1;
    r.env_id = ra.env_id0 + (uint64_t)i;
    r.voff = (uint32_t)i * 4u;
    if constexpr (LOG && ONEBASE) {
        r.rowp = ra.log.obs[0];
        r.donep = ra.log.done;
#pragma unroll
        for (int c = 0; c < 2 * EnvT::OBS + 2; ++c) r.coff[c] = ra.col_off[c] + r.voff;
    }

    r.env.load(ra.st.s0[i], ra.st.s1[i]);
    r.el = ra.st.steps[i];
    r.ep_ret = ra.st.ep_ret[i];
    r.pol.init(pa, ra, i);
    if constexpr (kObsNorm<Rms...>) r.pol.init_norm(rms_block(rms...));
    r.env.observe(r.obs);
    r.sum_r = 0.0f;
    r.n_goal = 0;
    r.n_eps = 0;

    // Retire the state loads HERE.  Otherwise hipcc places their s_waitcnt vmcnt(N) inside the
    // loop, where vmcnt also counts the log stores: every iteration would then wait for the
    // previous iteration's stores to land (0x0F70 = vmcnt(0), expcnt/lgkmcnt untouched).
    __builtin_amdgcn_s_waitcnt(0x0F70);

    int32_t k = 0;
    if constexpr (PolT::kPipelined) {
        // head: single steps until the global step index is a multiple of 4
        for (; k < ra.K && ((ra.step0 + (uint64_t)k) & 3) != 0; ++k)
            r.step(r.pol.act(r.obs, ra.seed, r.env_id, ra.step0 + (uint64_t)k, k == 0), k);
        if (k + 4 <= ra.K) {
            u32x4 cur = rng_words(ra.seed, r.env_id, (ra.step0 + (uint64_t)k) >> 2, TAG_ACTION);
            for (; k + 4 <= ra.K; k += 4) {
                PhiloxPipe nx;
                nx.start(ra.seed, r.env_id, ((ra.step0 + (uint64_t)k) >> 2) + 1, TAG_ACTION);
                nx.rounds<3>(); nx.pin();
                r.step(r.pol.from_word(cur.x), k);
                nx.rounds<3>(); nx.pin();
                r.step(r.pol.from_word(cur.y), k + 1);
                nx.rounds<2>(); nx.pin();
                r.step(r.pol.from_word(cur.z), k + 2);
                nx.rounds<2>(); nx.pin();
                r.step(r.pol.from_word(cur.w), k + 3);
                cur = nx.get();
            }
        }
        // tail (< 4 steps)
        const int32_t k_tail = k;
        for (; k < ra.K; ++k)
            r.step(r.pol.act(r.obs, ra.seed, r.env_id, ra.step0 + (uint64_t)k, k == k_tail), k);
    } else if constexpr (PolT::kFusedActor) {
        // Four steps per iteration: one Philox evaluation (counter t >> 2) serves them (ou_gaussian_from_words),
        // and the evaluation for the NEXT four is split 3 + 3 + 2 + 2 rounds over the four step bodies.
        uint64_t t = ra.step0;
        u32x4 cur = rng_words(ra.seed, r.env_id, t >> 2, TAG_OU);
        for (; k < ra.K && (t & 3) != 0; ++k, ++t) r.step(r.pol.act(r.obs, PolT::gaussian(cur, t)), k);  // head
        if (k + 4 <= ra.K) {
            if (k != 0) cur = rng_words(ra.seed, r.env_id, t >> 2, TAG_OU);
            for (; k + 4 <= ra.K; k += 4, t += 4) {
                PhiloxPipe nx;
                nx.start(ra.seed, r.env_id, (t >> 2) + 1, TAG_OU);
                nx.rounds<3>(); nx.pin();
                const float r0 = PolT::bm_radius(cur.x), s0 = PolT::bm_sin(cur.y);
                r.step(r.pol.act(r.obs, r0 * PolT::bm_cos(cur.y)), k);
                nx.rounds<3>(); nx.pin();
                r.step(r.pol.act(r.obs, r0 * s0), k + 1);
                nx.rounds<2>(); nx.pin();
                const float r1 = PolT::bm_radius(cur.z), s1 = PolT::bm_sin(cur.w);
                r.step(r.pol.act(r.obs, r1 * PolT::bm_cos(cur.w)), k + 2);
                nx.rounds<2>(); nx.pin();
                r.step(r.pol.act(r.obs, r1 * s1), k + 3);
                cur = nx.get();
            }
        } else if (k < ra.K && k != 0) {
            cur = rng_words(ra.seed, r.env_id, t >> 2, TAG_OU);
        }
        for (; k < ra.K; ++k, ++t) r.step(r.pol.act(r.obs, PolT::gaussian(cur, t)), k);  // tail (< 4 steps, t & 3 == 0 at its start)
    } else {
        for (; k < ra.K; ++k)
            r.step(r.pol.act(r.obs, ra.seed, r.env_id, ra.step0 + (uint64_t)k, k == 0), k);
    }

    if (r.active && r.owner) {
        ra.st.s0[i] = r.env.s0();
        ra.st.s1[i] = r.env.s1();
        ra.st.steps[i] = r.el;
        ra.st.ep_ret[i] = r.ep_ret;
        r.pol.store(ra, i);
    }

    if (ra.stats != nullptr) {
        const bool cnt = r.active && r.owner;
        double v[4] = {cnt ? (double)r.sum_r : 0.0, cnt ? (double)r.n_goal : 0.0, cnt ? (double)ra.K : 0.0,
                       cnt ? (double)r.n_eps : 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v[q] += __shfl_xor(v[q], m);
        __shared__ double red[kBlock / 64][4];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[wave][q] = v[q];
        __syncthreads();
        if (threadIdx.x < 4) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
            atomicAdd(ra.stats + threadIdx.x, s);
        }
    }
}

template <class EnvT, class PolT, bool LOG, bool ONEBASE = false, class... Rms>
__global__ __launch_bounds__(kBlock) void rollout_kernel(typename EnvT::Const ec, PolicyArgs pa, RolloutArgs ra, Rms... rms) {
    rollout_body<EnvT, PolT, LOG, ONEBASE, Rms...>(ec, pa, ra, rms...);
}

// Can the fp32 columns of the log be addressed from obs[0] with 32-bit offsets?  (always for a packed chunk)
static SSC_HD void set_one_base(RolloutArgs &ra, int obs_dim) {
    const float *cols[2 * SSC_MAX_OBS + 2];
    int nc = 0;
    for (int c = 0; c < obs_dim; ++c) cols[nc++] = ra.log.obs[c];
    cols[nc++] = ra.log.act;
    cols[nc++] = ra.log.rew;
    for (int c = 0; c < obs_dim; ++c) cols[nc++] = ra.log.obs2[c];
    ra.one_base = 1;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(cols[0]);
    for (int c = 0; c < nc; ++c) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(cols[c]);
        if (p < b0 || (p - b0) + (uint64_t)ra.n * 4u > 0xFFFFFFFFull) { ra.one_base = 0; break; }
        ra.col_off[c] = (uint32_t)(p - b0);
    }
}

// One call's arguments as the kernels take them: what rollout() packs on the host for the single launch and what
// rollout_many_kernel packs from its pair's item -- the same assignments, and the one rounding among them (act_span) is
// one IEEE subtraction on either side, so a pair's workgroups see the bits its own launch would hand them.  No checks:
// those are the host's (rollout_check).
static SSC_HD void pack_args(const ssc_policy_desc &pol, int64_t n, int32_t K, const ssc_rollout_state &st,
                             const ssc_transition_log *log, const ssc_episode_ring *ring, double *stats, uint64_t seed,
                             uint64_t env_id0, uint64_t step0, int obs_dim, PolicyArgs &pa, RolloutArgs &ra) {
    ra.n = n;
    ra.K = K;
    ra.st = st;
    ra.has_log = log != nullptr;
    ra.has_ring = ring != nullptr;
    ra.one_base = 0;
    if (log) {
        ra.log = *log;
        if (ra.log.row_stride == 0) ra.log.row_stride = n;
        if (ra.log.done_row_stride == 0) ra.log.done_row_stride = n;
        set_one_base(ra, obs_dim);
    } else {
        ra.log = ssc_transition_log{};
    }
    if (ring) ra.ring = *ring;
    else ra.ring = ssc_episode_ring{};
    ra.stats = stats;
    ra.seed = seed;
    ra.env_id0 = env_id0;
    ra.step0 = step0;

    pa = PolicyArgs{};
    pa.act_low = pol.act_low;
    pa.act_high = pol.act_high;
    pa.act_span = pol.act_high - pol.act_low;
    if (pol.kind == SSC_POLICY_ACTOR) {
        const ssc_actor_desc &a = pol.actor;
        pa.actor = ActorWeights{a.W1, a.b1, a.W2, a.b2, a.W3, a.b3, a.obs_dim, a.h1, a.h2, a.last_layer_tanh, a.obs_clip,
                                a.ln1_g, a.ln1_b, a.ln2_g, a.ln2_b};
        pa.ou_mu = pol.ou.mu;
        pa.ou_sigma = pol.ou.sigma;
        pa.ou_theta = pol.ou.theta;
        pa.ou_dt = pol.ou.dt;
        pa.ou_eps = pol.ou.epsilon;
        pa.d_eps = pol.ou.d_epsilon;
    }
}

// A population of (env set, policy) pairs in one launch (ssc_rollout_many): blockIdx.y is the pair, whose workgroups run
// rollout_body exactly as the pair's own launch would.  The item and the cursor sit at workgroup-uniform addresses and are
// read before anything is written: scalar loads into SGPRs, where the kernarg of the single launch lives too.  Grid x is
// the LARGEST pair's block count: the workgroups a smaller pair does not have leave at once.  Pairs share nothing (the
// host refuses two pairs on one array); a pair's atomics on its own d_stats and ring cursor are those of its own launch.
// Pointers read out of the item are generic to the compiler: the state loads / stores around the step loop are FLAT
// instructions here, the log stores inside it go through lane_ptr and stay global_store.
template <class EnvT, class PolT, bool LOG, bool ONEBASE, class... Rms>
__global__ __launch_bounds__(kBlock) void rollout_many_kernel(const ssc_rollout_many_item *__restrict__ items,
                                                              const ssc_pair_cursor *__restrict__ cursors, int32_t K) {
    const ssc_rollout_many_item &it = items[blockIdx.y];
    if ((int64_t)blockIdx.x * (kBlock / PolT::kLanesPerEnv) >= it.n) return;
    PolicyArgs pa;
    RolloutArgs ra;
    pack_args(it.policy, it.n, K, it.state, LOG ? &it.log : nullptr, it.has_ring ? &it.ring : nullptr, it.d_stats, it.seed,
              it.env_id0, cursors[blockIdx.y].step0, EnvT::OBS, pa, ra);
    const typename EnvT::Const ec = EnvT::make_const(it.params);
    rollout_body<EnvT, PolT, LOG, ONEBASE, Rms...>(ec, pa, ra, static_cast<Rms>(it.d_rms)...);
}

template <class EnvT, class PolT, class... Rms>
static int launch_rollout(const typename EnvT::Const &ec, const PolicyArgs &pa, const RolloutArgs &ra,
                          hipStream_t stream, Rms... rms) {
    const dim3 grid(blocks_for(ra.n, kBlock / PolT::kLanesPerEnv));
    // One running row pointer + per-column lane offsets (ONEBASE) takes ~30 scalar address instructions out of every
    // step: 12 % faster for the actor policies, whose step is instruction-bound (0.254 -> 0.224 ms per 65 536 x 256).
    // The random policy is HBM-bound and gets SLOWER with it (0.242 -> 0.27-0.28 ms per 65 536 x 1024, median; the minimum
    // stays at 0.237): with the stores in one burst AND with the stores spread over the step by scheduling fences -- so
    // it is not the burst.  The launch-time distribution widens, as if the 1024 waves, freed of ~30 scalar instructions
    // of per-step jitter, fell into step with each other.  It keeps the per-column pointers.
    constexpr bool kOneBase = !PolT::kPipelined;
    if (ra.has_log && ra.one_base && kOneBase)
        hipLaunchKernelGGL((rollout_kernel<EnvT, PolT, true, kOneBase, Rms...>), grid, dim3(kBlock), 0, stream, ec, pa, ra, rms...);
    else if (ra.has_log)
        hipLaunchKernelGGL((rollout_kernel<EnvT, PolT, true, false, Rms...>), grid, dim3(kBlock), 0, stream, ec, pa, ra, rms...);
    else
        hipLaunchKernelGGL((rollout_kernel<EnvT, PolT, false, false, Rms...>), grid, dim3(kBlock), 0, stream, ec, pa, ra, rms...);
    return check_launch("ssc_rollout");
}

int validate_mc_params(const ssc_env_params *p, const char *who);  // env_step.hip

// Does a MountainCar bf16-MFMA actor run the straight-line fused policy?  (dispatch_policy, and ssc_rollout_many for its pairs)
static bool mc_fused_policy(const McConst &ec, const ssc_actor_desc &a, const PolicyArgs &pa, bool norm) {
    const float obs_bound = fmaxf(fmaxf(fabsf(ec.min_position), fabsf(ec.max_position)), fabsf(ec.max_speed));
    const bool clip_inert = !(a.obs_clip > 0.0f) || a.obs_clip >= obs_bound;
    return a.h1 <= 64 && a.h2 <= 32 && pa.act_low == -1.0f && pa.act_high == 1.0f && (pa.ou_eps > 0.0f || pa.d_eps != nullptr) &&
           (clip_inert || norm);
}

// Rms: empty, or the RunningMeanStd block of normalize_observations (every actor policy then has a NORM instantiation)
template <class EnvT, class... Rms>
static int dispatch_policy(const typename EnvT::Const &ec, const ssc_policy_desc *pol, const PolicyArgs &pa,
                           const RolloutArgs &ra, hipStream_t stream, Rms... rms) {
    constexpr int OBS = EnvT::OBS;
    constexpr bool N = kObsNorm<Rms...>;
    if (pol->kind == SSC_POLICY_RANDOM) return launch_rollout<EnvT, RandomPolicy<OBS>>(ec, pa, ra, stream);   // (no network: no statistics)
    const ssc_actor_desc &a = pol->actor;
    if (a.obs_dim != OBS)
        return set_error(SSC_EINVAL, "ssc_rollout: actor obs_dim %d != env obs_dim %d", a.obs_dim, OBS);
    if (a.act_dim != 1) return set_error(SSC_EUNSUPPORTED, "ssc_rollout: act_dim %d (only 1)", a.act_dim);
    if (a.precision == SSC_PREC_F32) {
        if (a.h1 == 64 && a.h2 == 32)
            return launch_rollout<EnvT, ActorPolicy<ActorF32<OBS, 64, 32>, OBS, N>>(ec, pa, ra, stream, rms...);
        if (a.h1 == 64 && a.h2 == 64)      // Actor_Editted's own default sizes (models_editted.py:23)
            return launch_rollout<EnvT, ActorPolicy<ActorF32<OBS, 64, 64>, OBS, N>>(ec, pa, ra, stream, rms...);
        return set_error(SSC_EUNSUPPORTED,
                         "ssc_rollout: fused fp32 actor supports h1-h2 = 64-32 and 64-64 (got %d-%d); use the bf16 MFMA "
                         "path or step the env with ssc_actor_forward + ssc_*_step",
                         a.h1, a.h2);
    }
    if (a.precision == SSC_PREC_BF16_MFMA) {
        if constexpr (OBS == 2) {
            // the shipped shape on unit action bounds with exploration noise on: the straight-line fused policy
            // (MountainCar observations are bounded by the env's own clamps: an observation clip at or beyond them
            // -- DDPG's (-5, 5) against |pos| <= 1.2, |vel| <= 0.07 -- never acts, so the fused policy skips it; a normalised
            // observation has no such bound, and the NORM instantiation clips)
            if (mc_fused_policy(ec, a, pa, N)) {
                if (a.last_layer_tanh) return launch_rollout<EnvT, ActorPolicyFused<true, N>>(ec, pa, ra, stream, rms...);
                return launch_rollout<EnvT, ActorPolicyFused<false, N>>(ec, pa, ra, stream, rms...);
            }
        }
        if (a.h1 <= 64 && a.h2 <= 32)
            return launch_rollout<EnvT, ActorPolicy<ActorMfma<OBS, 2, 1, 2>, OBS, N>>(ec, pa, ra, stream, rms...);
        if (a.h1 <= 128 && a.h2 <= 64)
            return launch_rollout<EnvT, ActorPolicy<ActorMfma<OBS, 4, 2, 2>, OBS, N>>(ec, pa, ra, stream, rms...);
        // the wide shapes of the reference's grid (200-100): W2 fragments staged in LDS (ActorMfmaLds)
        if (a.h1 <= 224 && a.h2 <= 128)
            return launch_rollout<EnvT, ActorPolicy<ActorMfmaLds<OBS, 7, 4, SSC_WIDE_ACTOR_ET>, OBS, N>>(ec, pa, ra, stream, rms...);
        return set_error(SSC_EUNSUPPORTED, "ssc_rollout: MFMA actor supports h1 <= 224, h2 <= 128 (got %d-%d)",
                         a.h1, a.h2);
    }
    return set_error(SSC_EINVAL, "ssc_rollout: unknown precision %d", a.precision);
}


// ---------------------------------------------------------------- MPC-policy rollout step --
// Everything of one rollout(K, 'mpc') step that follows the scoring, for P envs (one navigation problem each)
// in one launch: executed action, env.step, log row, statistics, episode record, navigator bookkeeping,
// auto-reset, planning state of the next step.  The step index t and the log row k come from device counters
// that the launch advances itself (the block that finishes last), so the whole step is HIP-graph replayable.
struct MpcStepArgs {
    MpcArgs nav;
    int32_t *cur_idx;
    const int32_t *start_idx;
    int32_t *actions_done;
    uint8_t *at_goal;
    int32_t give_up, final_steps;
    const float *A;
    const int32_t *best_idx;
    float noise;
    uint64_t noise_seed, problem_id0;
    uint64_t *d_t;
    int32_t *d_k, *ticket;
    float *plan_state;
};

// the vectorised SmartStartContinuous step (ssc_smartstart_rollout_step): per-env mode on top of the MPC step
struct SsStepArgs {
    uint8_t *mode;
    int32_t *plan_of;
    const float *actor_out, *d_eta, *d_eps;
    const int32_t *d_pool;
    float ou_mu, ou_sig_sqrt_dt, ou_theta_dt, act_low, act_high;
    uint8_t *mode_log;
    int64_t mode_log_stride;
    int32_t *n_live;   // ssc_smartstart_step::d_n_live: zeroed here for the next step's ssc_nav_compact
};

// The population form (ssc_smartstart_rollout_step_many) is an instantiation of its own: ONE extra trailing argument, the
// device table of ssc_smartstart_pair rows, spelled as a parameter pack like the kernels' statistics block -- with an empty
// pack the kernel keeps its parameter list and code.  Grid row y is pair y: its envs are [env0, env0 + n_envs) of the call's,
// its blocks anchored at env0, and what the single step reads through sa.d_eta / d_eps / d_pool and the OU scalars comes from
// row y of the table (block-uniform address: scalar loads).
typedef const __attribute__((address_space(4))) ssc_smartstart_pair *const_ss_pair;
template <class... Many> inline constexpr bool kSsMany = sizeof...(Many) > 0;
template <class... Many> __device__ __forceinline__ const_ss_pair ss_pair_row(Many... many) {
    if constexpr (sizeof...(Many) > 0) return (const_ss_pair)(many, ...) + blockIdx.y;
    else return nullptr;
}

template <class EnvT, bool SS = false, class... Many>
__global__ __launch_bounds__(kBlock) void mpc_rollout_step_kernel(typename EnvT::Const ec, RolloutArgs ra, MpcStepArgs ma, SsStepArgs sa,
                                                                  Many... many) {
    constexpr int OBS = EnvT::OBS;
    constexpr bool MANY = kSsMany<Many...>;
    static_assert(!MANY || SS, "the pair table belongs to the SmartStart step");
    [[maybe_unused]] const const_ss_pair pair = ss_pair_row(many...);
    // the navigator plans in observation space (checked on the host): with the dimension a constant the waypoint / radii loads of
    // the bookkeeping below are straight-line and go out together -- as a run-time bound every one of them was a branch with a
    // load and a full wait behind it, a dozen dependent round trips in a kernel that is one wave per SIMD
    ma.nav.d = OBS;
    int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (MANY) {   // the pair's envs; a surplus block (a smaller pair than the grid's widest) is inactive throughout
        gi += pair->env0;
        ra.n = (int64_t)pair->env0 + pair->n_envs;
        if (ra.stats != nullptr) ra.stats += 4 * blockIdx.y;
    }
    if (!MANY && SS && gi == 0 && sa.n_live != nullptr) *sa.n_live = 0;   // simulation and scoring of this step are behind us in the stream
    const bool active = gi < ra.n;
    const int64_t i = active ? gi : ra.n - 1;
    const uint64_t t = *ma.d_t;
    const int32_t k = *ma.d_k;
    float rew = 0.0f;
    bool goal = false, done = false;
    if (active) {
        EnvT env;
        env.load(ra.st.s0[i], ra.st.s1[i]);
        int32_t el = ra.st.steps[i];
        float ep_ret = ra.st.ep_ret[i];
        float obs[OBS], obs2[OBS];
        env.observe(obs);
        // the navigator's bookkeeping state and plan: requested here, with the env's state, not behind the log stores below
        // (which the compiler cannot move loads across)
        int idx = ma.cur_idx[i];
        int done_act = ma.actions_done[i];
        const NavPlan plan = nav_plan_load(ma.nav, (int)i);
        // SmartStartContinuous.get_action (smartexplorationcontinuous.py:307-317): the navigator while smart_start_pathing,
        // the base agent otherwise
        bool navigating = true;
        float ou_x = 0.0f;
        if (SS) {
            navigating = sa.mode[i] != 0;
            ou_x = ra.st.ou_x[i];
            if (sa.mode_log != nullptr) sa.mode_log[(int64_t)k * sa.mode_log_stride + i] = navigating ? 1 : 0;
        }
        float a;
        if (navigating) {
            // action = best_sequence[0] + noise * N(0,1), no clip (NND_MB_agent.py:353-356; ssc_mpc_select_action's draw)
            const int64_t row = i * ma.nav.N + ma.best_idx[i];
            a = ma.A[row * ma.nav.H];   // act_dim == 1 (the envs of this engine)
            if (ma.noise != 0.0f) {
                const u32x4 w = rng_words(ma.noise_seed, ma.problem_id0 + (uint64_t)i, t, TAG_MPC_NOISE);
                a += ma.noise * gaussian_f32(w.x, w.y);
            }
        } else {
            // DDPG_Baselines_agent.get_action (:206-240): actor + epsilon * OU, clip, scale twice -- ActorPolicy::act's
            // arithmetic and noise stream; the OU state moves on these steps only (the agent is not asked while navigating)
            a = sa.actor_out[i];
            if constexpr (MANY) {   // the products the single call's host code forms, as the same floats (correctly rounded sqrtf)
                sa.ou_mu = pair->ou.mu;
                sa.ou_sig_sqrt_dt = pair->ou.sigma * sqrtf(pair->ou.dt);
                sa.ou_theta_dt = pair->ou.theta * pair->ou.dt;
            }
            const float eps = fmaxf(MANY ? pair->ou_epsilon : *sa.d_eps, 0.0f);
            if (eps > 0.0f) {
                const u32x4 w = rng_words(ra.seed, ra.env_id0 + (uint64_t)i, t >> 2, TAG_OU);
                const float g = ou_gaussian_from_words(w, t);
                ou_x = fmaf(sa.ou_sig_sqrt_dt, g, fmaf(sa.ou_theta_dt, sa.ou_mu - ou_x, ou_x));
                a = fmaf(ou_x, eps, a);
            }
            a = fminf(fmaxf(a, -1.0f), 1.0f);
            const bool identity = sa.act_low == -1.0f && sa.act_high == 1.0f;
#pragma unroll
            for (int rep = 0; rep < 2; ++rep) {
                a = fminf(fmaxf(a, -1.0f), 1.0f);
                a = identity ? a : fmaf((a + 1.0f) * 0.5f, sa.act_high - sa.act_low, sa.act_low);
            }
        }
        env.step(ec, a, rew, goal);
        env.observe(obs2);
        el += 1;
        done = goal || (ec.max_episode_steps > 0 && el >= ec.max_episode_steps);
        ep_ret += rew;
        if (ra.has_log) {
            const int64_t lr = (int64_t)k * ra.log.row_stride + i, ld = (int64_t)k * ra.log.done_row_stride + i;
#pragma unroll
            for (int c = 0; c < OBS; ++c) {
                ra.log.obs[c][lr] = obs[c];
                ra.log.obs2[c][lr] = obs2[c];
            }
            ra.log.act[lr] = a;
            ra.log.rew[lr] = rew;
            ra.log.done[ld] = done ? 1 : 0;
        }
        // NND_MB_agent.get_action counts the action (:340), observe advances the waypoint (:360-373)
        float x[SSC_MAX_STATE];
#pragma unroll
        for (int c = 0; c < SSC_MAX_STATE; ++c) x[c] = (c < OBS) ? obs2[c < OBS ? c : 0] : 0.0f;
        bool at_goal = false;
        if (navigating) {
            done_act += 1;
            at_goal = nav_observe_plan(ma.nav, plan, x, idx, done_act, ma.give_up, ma.final_steps);
        }
        if (ma.at_goal != nullptr) ma.at_goal[i] = at_goal ? 1 : 0;
        if (SS && navigating && at_goal) navigating = false;     // :336-339: the base agent takes over
        if (done) {
            if (ra.has_ring) {
                const uint32_t slot = atomicAdd(ra.ring.cursor, 1u);
                if (slot < (uint32_t)ra.ring.capacity) {
                    ra.ring.env_id[slot] = (int64_t)(ra.env_id0 + (uint64_t)i);
                    ra.ring.length[slot] = el;
                    ra.ring.ret[slot] = ep_ret;
                }
            }
            env.reset(ec, rng_words(ra.seed, ra.env_id0 + (uint64_t)i, t, TAG_RESET));
            el = 0;
            ep_ret = 0.0f;
            idx = ma.start_idx[i];    // start_new_episode_plan (:383-384)
            done_act = 0;
            if (!SS && ra.st.ou_x != nullptr) ra.st.ou_x[i] = 0.0f;
            if (SS) {
                ou_x = 0.0f;              // DDPG_Baselines_agent.end_episode: noise reset (:255-258)
                // SmartStartContinuous.start_new_episode (:341-370) on the reset state
                navigating = false;
                const u32x4 w = rng_words(ra.seed, ra.env_id0 + (uint64_t)i, t, TAG_SS_EPISODE);
                const int first = MANY ? pair->pool_first : sa.d_pool[0], count = MANY ? pair->pool_count : sa.d_pool[1],
                          slots = MANY ? pair->pool_slots : sa.d_pool[2];
                if (count > 0 && (float)(w.x >> 8) * (1.0f / 16777216.0f) <= (MANY ? pair->eta : *sa.d_eta)) {   // np.random.rand() <= eta (:350)
                    const int q = (MANY ? pair->slot0 : 0) + (first + (int)(w.y % (uint32_t)count)) % slots;
                    sa.plan_of[i] = q;    // read by the scorer of the next step (same stream)
                    idx = 0;
                    // close_enough_to_goal(state) with a fresh plan (:425-432): the goal test alone
                    float xr[SSC_MAX_STATE], obs_r[OBS];
                    env.observe(obs_r);
#pragma unroll
                    for (int c = 0; c < SSC_MAX_STATE; ++c) xr[c] = (c < OBS) ? obs_r[c < OBS ? c : 0] : 0.0f;
                    const int W = ma.nav.wp_len[q], d = ma.nav.d;
                    float inv_r[SSC_MAX_STATE];
#pragma unroll
                    for (int c = 0; c < SSC_MAX_STATE; ++c) inv_r[c] = (c < d) ? 1.0f / ma.nav.radii[q * d + c] : 0.0f;
                    const float *goal_wp = ma.nav.wp + ((int64_t)ma.nav.wp_off[q] + W - 1) * d;
                    navigating = !(ell_dist(xr, goal_wp, inv_r, d) <= ma.nav.theta);
                }
            }
        }
        if (SS) {
            sa.mode[i] = navigating ? 1 : 0;
            ra.st.ou_x[i] = ou_x;
        }
        ra.st.s0[i] = env.s0();
        ra.st.s1[i] = env.s1();
        ra.st.steps[i] = el;
        ra.st.ep_ret[i] = ep_ret;
        ma.cur_idx[i] = idx;
        ma.actions_done[i] = done_act;
        env.observe(obs);
#pragma unroll
        for (int c = 0; c < OBS; ++c) ma.plan_state[i * OBS + c] = obs[c];
    }
    __shared__ double red[kBlock / 64][4];
    if (ra.stats != nullptr) {
        double v[4] = {active ? (double)rew : 0.0, (active && goal) ? 1.0 : 0.0, active ? 1.0 : 0.0, (active && done) ? 1.0 : 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v[q] += __shfl_xor(v[q], m);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[wave][q] = v[q];
    }
    __syncthreads();
    if (ra.stats != nullptr && threadIdx.x < 4) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
        atomicAdd(ra.stats + threadIdx.x, s);
    }
    // every block has read *d_t / *d_k before it gets here; the last one to arrive advances them.  The ticket orders
    // nothing but those two READS (this lane's have returned after the wait; the other lanes consumed theirs before the
    // barrier), so it is a relaxed agent-scope add: a __threadfence() here is an L2 write-back + invalidate per block --
    // it was 15 of this kernel's 37 us at 65 536 envs.  What the step wrote is published by the kernel boundary.
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(ma.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)(gridDim.x * (MANY ? gridDim.y : 1u)) - 1) {
            *ma.ticket = 0;
            *ma.d_t = t + 1;
            *ma.d_k = k + 1;
        }
    }
}

}  // namespace ssc

using namespace ssc;

// the checks of one rollout call, in two parts: rollout() returns SSC_OK between them when there is nothing to run
static int rollout_check_sizes(const char *who, const ssc_env_params *p, const ssc_policy_desc *policy, int64_t n, int32_t K,
                               const ssc_rollout_state *state) {
    SSC_REQUIRE(p && policy && state, "%s: NULL descriptor", who);
    SSC_REQUIRE(n >= 0 && K >= 0, "%s: n = %lld, K = %d", who, (long long)n, K);
    SSC_REQUIRE(n <= ((int64_t)1 << 30), "%s: n = %lld > 2^30 envs per launch", who, (long long)n);
    SSC_REQUIRE(policy->kind == SSC_POLICY_RANDOM || policy->kind == SSC_POLICY_ACTOR,
                "%s: unknown policy kind %d", who, policy->kind);
    return SSC_OK;
}

static int rollout_check_arrays(const char *who, const ssc_env_params *p, const ssc_policy_desc *policy, int64_t n,
                                const ssc_rollout_state *state, const ssc_transition_log *log, const ssc_episode_ring *ring) {
    SSC_REQUIRE(state->s0 && state->s1 && state->steps && state->ep_ret, "%s: NULL state column", who);
    SSC_REQUIRE(policy->act_low <= policy->act_high, "%s: act_low > act_high", who);
    const int obs_dim = (p->kind == SSC_ENV_MOUNTAINCAR) ? 2 : 3;
    if (log) {
        for (int c = 0; c < obs_dim; ++c)
            SSC_REQUIRE(log->obs[c] && log->obs2[c], "%s: NULL log obs column %d", who, c);
        SSC_REQUIRE(log->act && log->rew && log->done, "%s: NULL log column", who);
        SSC_REQUIRE(log->row_stride >= 0 && log->done_row_stride >= 0, "%s: negative row stride", who);
        SSC_REQUIRE((log->row_stride == 0 || log->row_stride >= n) && (log->done_row_stride == 0 || log->done_row_stride >= n),
                    "%s: row stride < n", who);
    }
    if (ring)
        SSC_REQUIRE(ring->env_id && ring->length && ring->ret && ring->cursor && ring->capacity >= 0,
                    "%s: bad episode ring", who);
    if (policy->kind == SSC_POLICY_ACTOR) {
        const ssc_actor_desc &a = policy->actor;
        SSC_REQUIRE(a.W1 && a.b1 && a.W2 && a.b2 && a.W3 && a.b3, "%s: NULL actor weight pointer", who);
        SSC_REQUIRE(a.h1 > 0 && a.h2 > 0, "%s: bad actor sizes", who);
        const bool ln = a.ln1_g != nullptr;
        SSC_REQUIRE(ln == (a.ln1_b != nullptr) && ln == (a.ln2_g != nullptr) && ln == (a.ln2_b != nullptr),
                    "%s: the four LayerNorm pointers come together", who);
        if (ln && a.precision != SSC_PREC_F32)
            return set_error(SSC_EUNSUPPORTED, "%s: LayerNorm actors run on the fp32 policy (precision SSC_PREC_F32)", who);
        SSC_REQUIRE(!(policy->ou.epsilon > 0.0f || policy->ou.d_epsilon != nullptr) || state->ou_x != nullptr,
                    "%s: OU noise needs state->ou_x", who);
    }
    return SSC_OK;
}

template <class... Rms>
static int rollout(const ssc_env_params *p, const ssc_policy_desc *policy, int64_t n, int32_t K,
                   const ssc_rollout_state *state, const ssc_transition_log *log,
                   const ssc_episode_ring *ring, double *d_stats, uint64_t seed, uint64_t env_id0,
                   uint64_t step0, ssc_stream_t stream, Rms... rms) {
    if (int rc = rollout_check_sizes("ssc_rollout", p, policy, n, K, state)) return rc;
    if (n == 0 || K == 0) return SSC_OK;
    if (int rc = rollout_check_arrays("ssc_rollout", p, policy, n, state, log, ring)) return rc;
    RolloutArgs ra;
    PolicyArgs pa;
    pack_args(*policy, n, K, *state, log, ring, d_stats, seed, env_id0, step0, (p->kind == SSC_ENV_MOUNTAINCAR) ? 2 : 3, pa, ra);
    if (p->kind == SSC_ENV_MOUNTAINCAR) {
        if (int rc = validate_mc_params(p, "ssc_rollout")) return rc;
        return dispatch_policy<McEnv>(make_mc_const(*p), policy, pa, ra, as_stream(stream), rms...);
    }
    if (p->kind == SSC_ENV_PENDULUM)
        return dispatch_policy<PendEnv>(make_pend_const(*p), policy, pa, ra, as_stream(stream), rms...);
    return set_error(SSC_EINVAL, "ssc_rollout: unknown env kind %d", p->kind);
}

extern "C" int ssc_rollout(const ssc_env_params *p, const ssc_policy_desc *policy, int64_t n, int32_t K,
                           const ssc_rollout_state *state, const ssc_transition_log *log,
                           const ssc_episode_ring *ring, double *d_stats, uint64_t seed, uint64_t env_id0,
                           uint64_t step0, ssc_stream_t stream) {
    return rollout(p, policy, n, K, state, log, ring, d_stats, seed, env_id0, step0, stream);
}

// normalize_observations: the actor sees clip((obs - mean) / std) of the RunningMeanStd block d_rms, read once per
// launch (frozen for the chunk, like the weights); a random policy ignores it
extern "C" int ssc_rollout_rms(const ssc_env_params *p, const ssc_policy_desc *policy, int64_t n, int32_t K,
                               const ssc_rollout_state *state, const ssc_transition_log *log,
                               const ssc_episode_ring *ring, double *d_stats, uint64_t seed, uint64_t env_id0,
                               uint64_t step0, ssc_stream_t stream, const double *d_rms) {
    if (d_rms == nullptr) return rollout(p, policy, n, K, state, log, ring, d_stats, seed, env_id0, step0, stream);
    return rollout(p, policy, n, K, state, log, ring, d_stats, seed, env_id0, step0, stream, d_rms);
}

// ---- a population of pairs in one launch ----------------------------------------------------------------------
namespace {

template <class EnvT, class PolT, class... Rms>
int launch_rollout_many(const ssc_rollout_many_item *d_items, const ssc_pair_cursor *d_cursors, int32_t n_pairs, int32_t K,
                        int64_t n_max, bool has_log, bool one_base, hipStream_t stream) {
    const dim3 grid(blocks_for(n_max, kBlock / PolT::kLanesPerEnv), (unsigned)n_pairs);
    if (has_log && one_base)   // (the actor policies: launch_rollout's kOneBase)
        hipLaunchKernelGGL((rollout_many_kernel<EnvT, PolT, true, true, Rms...>), grid, dim3(kBlock), 0, stream, d_items, d_cursors, K);
    else if (has_log)
        hipLaunchKernelGGL((rollout_many_kernel<EnvT, PolT, true, false, Rms...>), grid, dim3(kBlock), 0, stream, d_items, d_cursors, K);
    else
        hipLaunchKernelGGL((rollout_many_kernel<EnvT, PolT, false, false, Rms...>), grid, dim3(kBlock), 0, stream, d_items, d_cursors, K);
    return check_launch("ssc_rollout_many");
}

// the policy class dispatch_policy chooses for a served pair
enum ManyClass { MANY_FUSED = 0, MANY_MFMA = 1 };

template <class EnvT, class... Rms>
int dispatch_rollout_many(ManyClass cls, bool last_tanh, const ssc_rollout_many_item *d_items, const ssc_pair_cursor *d_cursors,
                          int32_t n_pairs, int32_t K, int64_t n_max, bool has_log, bool one_base, hipStream_t stream) {
    constexpr int OBS = EnvT::OBS;
    constexpr bool N = sizeof...(Rms) > 0;
    if constexpr (OBS == 2) {
        if (cls == MANY_FUSED) {
            if (last_tanh)
                return launch_rollout_many<EnvT, ActorPolicyFused<true, N>, Rms...>(d_items, d_cursors, n_pairs, K, n_max, has_log, one_base, stream);
            return launch_rollout_many<EnvT, ActorPolicyFused<false, N>, Rms...>(d_items, d_cursors, n_pairs, K, n_max, has_log, one_base, stream);
        }
    }
    return launch_rollout_many<EnvT, ActorPolicy<ActorMfma<OBS, 2, 1, 2>, OBS, N>, Rms...>(d_items, d_cursors, n_pairs, K, n_max, has_log, one_base,
                                                                                       stream);
}

}  // namespace

extern "C" int ssc_rollout_many(const ssc_rollout_many_item *h_items, const ssc_rollout_many_item *d_items,
                                const ssc_pair_cursor *h_cursors, const ssc_pair_cursor *d_cursors, int32_t n_pairs, int32_t K,
                                ssc_stream_t stream) {
    SSC_REQUIRE(n_pairs >= 1, "ssc_rollout_many: n_pairs %d < 1", n_pairs);
    SSC_REQUIRE(h_items != nullptr && d_items != nullptr, "ssc_rollout_many: NULL item array");
    SSC_REQUIRE(h_cursors != nullptr && d_cursors != nullptr, "ssc_rollout_many: NULL cursor array");
    SSC_REQUIRE(K >= 0, "ssc_rollout_many: K = %d", K);
    if (n_pairs > 65535) return set_error(SSC_EUNSUPPORTED, "ssc_rollout_many: %d pairs > 65535 (one grid row each)", n_pairs);
    const ssc_rollout_many_item &i0 = h_items[0];
    ManyClass cls0 = MANY_MFMA;
    bool tanh0 = false, one_base = true;
    int64_t n_max = 0;
    std::vector<std::pair<const void *, int>> owned;   // (array, pair) of everything a pair's workgroups write
    owned.reserve((size_t)n_pairs * 20);
    for (int p = 0; p < n_pairs; ++p) {
        const ssc_rollout_many_item &it = h_items[p];
        char who[48];
        snprintf(who, sizeof who, "ssc_rollout_many: pair %d", p);
        const ssc_transition_log *log = it.has_log ? &it.log : nullptr;
        const ssc_episode_ring *ring = it.has_ring ? &it.ring : nullptr;
        // the single call's checks
        if (int rc = rollout_check_sizes(who, &it.params, &it.policy, it.n, K, &it.state)) return rc;
        SSC_REQUIRE(it.n >= 1, "%s: n = %lld < 1", who, (long long)it.n);
        SSC_REQUIRE(it.params.kind == SSC_ENV_MOUNTAINCAR || it.params.kind == SSC_ENV_PENDULUM, "%s: unknown env kind %d", who,
                    it.params.kind);
        if (int rc = rollout_check_arrays(who, &it.params, &it.policy, it.n, &it.state, log, ring)) return rc;
        if (it.params.kind == SSC_ENV_MOUNTAINCAR)
            if (int rc = validate_mc_params(&it.params, who)) return rc;
        // one instantiation per launch: env kind first (the obs_dim every other check reads)
        SSC_REQUIRE(it.params.kind == i0.params.kind, "%s: env kind %d differs from pair 0's %d (one kernel instantiation per launch)", who,
                    it.params.kind, i0.params.kind);
        const int obs_dim = it.params.kind == SSC_ENV_MOUNTAINCAR ? 2 : 3;
        const ssc_actor_desc &a = it.policy.actor;
        if (it.policy.kind != SSC_POLICY_ACTOR)
            return set_error(SSC_EUNSUPPORTED, "%s: the random policy does not roll out as a population; call ssc_rollout", who);
        SSC_REQUIRE(a.obs_dim == obs_dim, "%s: actor obs_dim %d != env obs_dim %d", who, a.obs_dim, obs_dim);
        if (a.act_dim != 1) return set_error(SSC_EUNSUPPORTED, "%s: act_dim %d (only 1)", who, a.act_dim);
        if (a.precision != SSC_PREC_BF16_MFMA || a.h1 > 64 || a.h2 > 32 || a.ln1_g != nullptr)
            return set_error(SSC_EUNSUPPORTED, "%s: only bf16-MFMA actors with h1 <= 64, h2 <= 32 and no LayerNorm roll out as a population "
                                               "(precision %d, %d-%d); call ssc_rollout_rms", who, a.precision, a.h1, a.h2);
        PolicyArgs pa;
        RolloutArgs ra;
        pack_args(it.policy, it.n, K, it.state, log, ring, it.d_stats, it.seed, it.env_id0, h_cursors[p].step0, obs_dim, pa, ra);
        const ManyClass cls = (obs_dim == 2 && mc_fused_policy(make_mc_const(it.params), a, pa, it.d_rms != nullptr)) ? MANY_FUSED : MANY_MFMA;
        const bool t2 = a.last_layer_tanh != 0;
        if (p == 0) { cls0 = cls; tanh0 = t2; }
        SSC_REQUIRE(cls == cls0, "%s: runs the %s actor policy, pair 0 the %s one (action bounds / epsilon / obs_clip select it; one kernel "
                                 "instantiation per launch)", who, cls == MANY_FUSED ? "fused" : "generic", cls0 == MANY_FUSED ? "fused" : "generic");
        SSC_REQUIRE(cls != MANY_FUSED || t2 == tanh0, "%s: last_layer_tanh %d differs from pair 0's %d (one kernel instantiation per launch)",
                    who, a.last_layer_tanh, i0.policy.actor.last_layer_tanh);
        SSC_REQUIRE((it.d_rms != nullptr) == (i0.d_rms != nullptr), "%s: d_rms is %s, pair 0's is not (statistics for all pairs or for none)",
                    who, it.d_rms ? "set" : "NULL");
        SSC_REQUIRE((it.has_log != 0) == (i0.has_log != 0), "%s: has_log %d differs from pair 0's %d (a log for all pairs or for none)", who,
                    it.has_log, i0.has_log);
        one_base = one_base && (!log || ra.one_base);
        if (it.n > n_max) n_max = it.n;
        for (const void *q : {(const void *)it.state.s0, (const void *)it.state.s1, (const void *)it.state.steps, (const void *)it.state.ep_ret,
                              (const void *)it.state.ou_x, (const void *)it.d_stats})
            if (q != nullptr) owned.emplace_back(q, p);
        if (log) {
            for (int c = 0; c < obs_dim; ++c) {
                owned.emplace_back(log->obs[c], p);
                owned.emplace_back(log->obs2[c], p);
            }
            for (const void *q : {(const void *)log->act, (const void *)log->rew, (const void *)log->done}) owned.emplace_back(q, p);
        }
        if (ring)
            for (const void *q : {(const void *)ring->env_id, (const void *)ring->length, (const void *)ring->ret, (const void *)ring->cursor})
                owned.emplace_back(q, p);
    }
    // two pairs on one array would race without a sign of it
    std::sort(owned.begin(), owned.end());
    for (size_t k = 1; k < owned.size(); ++k)
        SSC_REQUIRE(owned[k].first != owned[k - 1].first || owned[k].second == owned[k - 1].second,
                    "ssc_rollout_many: pairs %d and %d share a state, log, episode-ring or statistics array", owned[k - 1].second,
                    owned[k].second);
    if (K == 0) return SSC_OK;
    const bool has_log = i0.has_log != 0;
    hipStream_t s = as_stream(stream);
    if (i0.params.kind == SSC_ENV_MOUNTAINCAR) {
        if (i0.d_rms != nullptr)
            return dispatch_rollout_many<McEnv, const double *>(cls0, tanh0, d_items, d_cursors, n_pairs, K, n_max, has_log, one_base, s);
        return dispatch_rollout_many<McEnv>(cls0, tanh0, d_items, d_cursors, n_pairs, K, n_max, has_log, one_base, s);
    }
    if (i0.d_rms != nullptr)
        return dispatch_rollout_many<PendEnv, const double *>(cls0, tanh0, d_items, d_cursors, n_pairs, K, n_max, has_log, one_base, s);
    return dispatch_rollout_many<PendEnv>(cls0, tanh0, d_items, d_cursors, n_pairs, K, n_max, has_log, one_base, s);
}

// argument checks and packing shared by ssc_mpc_rollout_step and ssc_smartstart_rollout_step
static int build_mpc_step_args(const char *fn, const ssc_env_params *p, const ssc_mpc_problems *pr, const ssc_mpc_nav_state *nav,
                               const float *d_A, const int32_t *d_best_idx, float noise_amount, uint64_t noise_seed,
                               uint64_t problem_id0, const ssc_rollout_state *state, const ssc_transition_log *log,
                               const ssc_episode_ring *ring, double *d_stats, uint64_t env_seed, uint64_t env_id0,
                               uint64_t *d_t, int32_t *d_k, int32_t *d_ticket, float *d_plan_state, RolloutArgs &ra, MpcStepArgs &ma) {
    SSC_REQUIRE(p && pr && nav && state, "%s: NULL descriptor", fn);
    const int64_t n = pr->n_problems;
    SSC_REQUIRE(n >= 0 && pr->n_samples >= 1 && pr->horizon >= 1, "%s: bad problem sizes", fn);
    const int obs_dim = (p->kind == SSC_ENV_MOUNTAINCAR) ? 2 : 3;
    SSC_REQUIRE(pr->state_dim == obs_dim, "%s: the navigator plans in observation space (%d dims), "
                                          "problems have %d", fn, obs_dim, pr->state_dim);
    SSC_REQUIRE(pr->wp && pr->wp_off && pr->radii && nav->cur_idx && nav->start_idx && nav->actions_done,
                "%s: NULL navigator pointer", fn);
    SSC_REQUIRE((pr->plan_of == nullptr) == (pr->wp_len == nullptr), "%s: plan_of and wp_len go together", fn);
    SSC_REQUIRE(state->s0 && state->s1 && state->steps && state->ep_ret, "%s: NULL state column", fn);
    SSC_REQUIRE(d_A && d_best_idx && d_t && d_k && d_ticket && d_plan_state, "%s: NULL device pointer", fn);
    ra.n = n;
    ra.K = 1;
    ra.st = *state;
    ra.has_log = log != nullptr;
    ra.has_ring = ring != nullptr;
    ra.one_base = 0;
    if (log) {
        ra.log = *log;
        for (int c = 0; c < obs_dim; ++c)
            SSC_REQUIRE(log->obs[c] && log->obs2[c], "%s: NULL log obs column %d", fn, c);
        SSC_REQUIRE(log->act && log->rew && log->done, "%s: NULL log column", fn);
        if (ra.log.row_stride == 0) ra.log.row_stride = n;
        if (ra.log.done_row_stride == 0) ra.log.done_row_stride = n;
        SSC_REQUIRE(ra.log.row_stride >= n && ra.log.done_row_stride >= n, "%s: row stride < n", fn);
    } else {
        ra.log = ssc_transition_log{};
    }
    if (ring) {
        ra.ring = *ring;
        SSC_REQUIRE(ring->env_id && ring->length && ring->ret && ring->cursor && ring->capacity >= 0,
                    "%s: bad episode ring", fn);
    } else {
        ra.ring = ssc_episode_ring{};
    }
    ra.stats = d_stats;
    ra.seed = env_seed;
    ra.env_id0 = env_id0;
    ra.step0 = 0;
    ma = MpcStepArgs{};
    ma.nav.P = pr->n_problems; ma.nav.N = pr->n_samples; ma.nav.H = pr->horizon; ma.nav.d = pr->state_dim;
    ma.nav.wp = pr->wp; ma.nav.left = pr->left; ma.nav.radii = pr->radii; ma.nav.wp_off = pr->wp_off;
    ma.nav.cur_idx = pr->cur_idx; ma.nav.theta = pr->theta; ma.nav.plan_of = pr->plan_of; ma.nav.wp_len = pr->wp_len;
    ma.cur_idx = nav->cur_idx; ma.start_idx = nav->start_idx; ma.actions_done = nav->actions_done; ma.at_goal = nav->at_goal;
    ma.give_up = nav->give_up_after; ma.final_steps = nav->final_steps;
    ma.A = d_A; ma.best_idx = d_best_idx; ma.noise = noise_amount; ma.noise_seed = noise_seed; ma.problem_id0 = problem_id0;
    ma.d_t = d_t; ma.d_k = d_k; ma.ticket = d_ticket; ma.plan_state = d_plan_state;
    return SSC_OK;
}

extern "C" int ssc_mpc_rollout_step(const ssc_env_params *p, const ssc_mpc_problems *pr, const ssc_mpc_nav_state *nav,
                                    const float *d_A, const int32_t *d_best_idx, float noise_amount, uint64_t noise_seed,
                                    uint64_t problem_id0, const ssc_rollout_state *state, const ssc_transition_log *log,
                                    const ssc_episode_ring *ring, double *d_stats, uint64_t env_seed, uint64_t env_id0,
                                    uint64_t *d_t, int32_t *d_k, int32_t *d_ticket, float *d_plan_state,
                                    ssc_stream_t stream) {
    RolloutArgs ra;
    MpcStepArgs ma;
    if (int rc = build_mpc_step_args("ssc_mpc_rollout_step", p, pr, nav, d_A, d_best_idx, noise_amount, noise_seed, problem_id0, state,
                                     log, ring, d_stats, env_seed, env_id0, d_t, d_k, d_ticket, d_plan_state, ra, ma))
        return rc;
    const int64_t n = ra.n;
    if (n == 0) return SSC_OK;
    hipStream_t s = as_stream(stream);
    if (p->kind == SSC_ENV_MOUNTAINCAR) {
        if (int rc = validate_mc_params(p, "ssc_mpc_rollout_step")) return rc;
        hipLaunchKernelGGL(mpc_rollout_step_kernel<McEnv>, dim3(blocks_for(n)), dim3(kBlock), 0, s, make_mc_const(*p), ra, ma, SsStepArgs{});
    } else if (p->kind == SSC_ENV_PENDULUM) {
        hipLaunchKernelGGL(mpc_rollout_step_kernel<PendEnv>, dim3(blocks_for(n)), dim3(kBlock), 0, s, make_pend_const(*p), ra, ma, SsStepArgs{});
    } else {
        return set_error(SSC_EINVAL, "ssc_mpc_rollout_step: unknown env kind %d", p->kind);
    }
    return check_launch("ssc_mpc_rollout_step");
}

extern "C" int ssc_smartstart_rollout_step(const ssc_env_params *p, const ssc_mpc_problems *pr, const ssc_mpc_nav_state *nav,
                                           const ssc_smartstart_step *ss, const float *d_A, const int32_t *d_best_idx,
                                           float noise_amount, uint64_t noise_seed, uint64_t problem_id0,
                                           const ssc_rollout_state *state, const ssc_transition_log *log,
                                           const ssc_episode_ring *ring, double *d_stats, uint64_t env_seed, uint64_t env_id0,
                                           uint64_t *d_t, int32_t *d_k, int32_t *d_ticket, float *d_plan_state,
                                           ssc_stream_t stream) {
    RolloutArgs ra;
    MpcStepArgs ma;
    if (int rc = build_mpc_step_args("ssc_smartstart_rollout_step", p, pr, nav, d_A, d_best_idx, noise_amount, noise_seed, problem_id0,
                                     state, log, ring, d_stats, env_seed, env_id0, d_t, d_k, d_ticket, d_plan_state, ra, ma))
        return rc;
    SSC_REQUIRE(ss != nullptr, "ssc_smartstart_rollout_step: NULL step descriptor");
    SSC_REQUIRE(ss->mode && ss->plan_of && ss->d_actor_out && ss->d_eta && ss->d_ou_epsilon && ss->d_pool,
                "ssc_smartstart_rollout_step: NULL device pointer in the step descriptor");
    SSC_REQUIRE(pr->plan_of != nullptr && pr->plan_of == ss->plan_of && pr->wp_len != nullptr,
                "ssc_smartstart_rollout_step: the problem set must use the plan pool (plan_of == ss->plan_of, wp_len)");
    SSC_REQUIRE(state->ou_x != nullptr, "ssc_smartstart_rollout_step: the base agent's OU noise needs state->ou_x");
    SSC_REQUIRE(ss->act_low <= ss->act_high && ss->mode_log_stride >= 0, "ssc_smartstart_rollout_step: bad action bounds / stride");
    const int64_t n = ra.n;
    if (n == 0) return SSC_OK;
    SsStepArgs sa{};
    sa.mode = ss->mode; sa.plan_of = ss->plan_of; sa.actor_out = ss->d_actor_out; sa.d_eta = ss->d_eta; sa.d_eps = ss->d_ou_epsilon;
    sa.d_pool = ss->d_pool;
    sa.ou_mu = ss->ou.mu; sa.ou_sig_sqrt_dt = ss->ou.sigma * sqrtf(ss->ou.dt); sa.ou_theta_dt = ss->ou.theta * ss->ou.dt;
    sa.act_low = ss->act_low; sa.act_high = ss->act_high;
    sa.mode_log = ss->d_mode_log; sa.mode_log_stride = ss->mode_log_stride ? ss->mode_log_stride : n;
    sa.n_live = ss->d_n_live;
    SSC_REQUIRE(sa.mode_log_stride >= n, "ssc_smartstart_rollout_step: mode log stride < n");
    hipStream_t s = as_stream(stream);
    if (p->kind == SSC_ENV_MOUNTAINCAR) {
        if (int rc = validate_mc_params(p, "ssc_smartstart_rollout_step")) return rc;
        hipLaunchKernelGGL((mpc_rollout_step_kernel<McEnv, true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, make_mc_const(*p), ra, ma, sa);
    } else if (p->kind == SSC_ENV_PENDULUM) {
        hipLaunchKernelGGL((mpc_rollout_step_kernel<PendEnv, true>), dim3(blocks_for(n)), dim3(kBlock), 0, s, make_pend_const(*p), ra, ma, sa);
    } else {
        return set_error(SSC_EINVAL, "ssc_smartstart_rollout_step: unknown env kind %d", p->kind);
    }
    return check_launch("ssc_smartstart_rollout_step");
}

// the step for a population of SmartStart pairs: grid row y = pair y of the device table (read by the kernel at launch)
extern "C" int ssc_smartstart_rollout_step_many(const ssc_env_params *p, const ssc_mpc_problems *pr, const ssc_mpc_nav_state *nav,
                                                const ssc_smartstart_step *ss, const ssc_smartstart_pair *h_pairs,
                                                const ssc_smartstart_pair *d_pairs, int32_t n_pairs, const float *d_A,
                                                const int32_t *d_best_idx, float noise_amount, uint64_t noise_seed,
                                                uint64_t problem_id0, const ssc_rollout_state *state, const ssc_transition_log *log,
                                                const ssc_episode_ring *ring, double *d_stats, uint64_t env_seed, uint64_t env_id0,
                                                uint64_t *d_t, int32_t *d_k, int32_t *d_ticket, float *d_plan_state,
                                                ssc_stream_t stream) {
    const char *fn = "ssc_smartstart_rollout_step_many";
    RolloutArgs ra;
    MpcStepArgs ma;
    if (int rc = build_mpc_step_args(fn, p, pr, nav, d_A, d_best_idx, noise_amount, noise_seed, problem_id0, state, log, ring, d_stats,
                                     env_seed, env_id0, d_t, d_k, d_ticket, d_plan_state, ra, ma))
        return rc;
    SSC_REQUIRE(ss != nullptr, "%s: NULL step descriptor", fn);
    SSC_REQUIRE(ss->mode && ss->plan_of && ss->d_actor_out, "%s: NULL device pointer in the step descriptor", fn);
    SSC_REQUIRE(pr->plan_of != nullptr && pr->plan_of == ss->plan_of && pr->wp_len != nullptr,
                "%s: the problem set must use the plan pool (plan_of == ss->plan_of, wp_len)", fn);
    SSC_REQUIRE(state->ou_x != nullptr, "%s: the base agent's OU noise needs state->ou_x", fn);
    SSC_REQUIRE(ss->act_low <= ss->act_high && ss->mode_log_stride >= 0, "%s: bad action bounds / stride", fn);
    SSC_REQUIRE(ss->d_n_live == nullptr, "%s: the population step has no compact live list: d_n_live must be NULL", fn);
    SSC_REQUIRE(n_pairs >= 1, "%s: n_pairs %d < 1", fn, n_pairs);
    if (n_pairs > 65535) return set_error(SSC_EUNSUPPORTED, "%s: n_pairs %d > 65535 (one grid row each)", fn, n_pairs);
    SSC_REQUIRE(h_pairs != nullptr && d_pairs != nullptr, "%s: NULL pair table", fn);
    const int64_t n = ra.n;
    int64_t at = 0;          // the end of the range before
    int32_t n_max = 0;
    for (int y = 0; y < n_pairs; ++y) {
        const ssc_smartstart_pair &q = h_pairs[y];
        SSC_REQUIRE(q.n_envs >= 1, "%s: pair %d: n_envs %d < 1", fn, y, q.n_envs);
        SSC_REQUIRE(q.env0 >= 0 && (int64_t)q.env0 + q.n_envs <= n, "%s: pair %d: envs [%d, %lld) outside [0, %lld)", fn, y, q.env0,
                    (long long)q.env0 + q.n_envs, (long long)n);
        SSC_REQUIRE(q.env0 >= at, "%s: pair %d: envs [%d, %lld) overlap pair %d's or are out of order", fn, y, q.env0,
                    (long long)q.env0 + q.n_envs, y - 1);
        SSC_REQUIRE(q.pool_slots >= 1 && q.pool_first >= 0 && q.pool_first < q.pool_slots && q.pool_count >= 0 &&
                    q.pool_count <= q.pool_slots, "%s: pair %d: bad pool (first %d, count %d, slots %d)", fn, y, q.pool_first,
                    q.pool_count, q.pool_slots);
        SSC_REQUIRE(q.slot0 >= 0, "%s: pair %d: slot0 %d < 0", fn, y, q.slot0);
        at = (int64_t)q.env0 + q.n_envs;
        n_max = std::max(n_max, q.n_envs);
    }
    SsStepArgs sa{};
    sa.mode = ss->mode; sa.plan_of = ss->plan_of; sa.actor_out = ss->d_actor_out;
    sa.act_low = ss->act_low; sa.act_high = ss->act_high;
    sa.mode_log = ss->d_mode_log; sa.mode_log_stride = ss->mode_log_stride ? ss->mode_log_stride : n;
    SSC_REQUIRE(sa.mode_log_stride >= n, "%s: mode log stride < n", fn);
    hipStream_t s = as_stream(stream);
    const dim3 grid(blocks_for(n_max), (unsigned)n_pairs), block(kBlock);
    if (p->kind == SSC_ENV_MOUNTAINCAR) {
        if (int rc = validate_mc_params(p, fn)) return rc;
        hipLaunchKernelGGL((mpc_rollout_step_kernel<McEnv, true, const ssc_smartstart_pair *>), grid, block, 0, s, make_mc_const(*p), ra, ma,
                           sa, d_pairs);
    } else if (p->kind == SSC_ENV_PENDULUM) {
        hipLaunchKernelGGL((mpc_rollout_step_kernel<PendEnv, true, const ssc_smartstart_pair *>), grid, block, 0, s, make_pend_const(*p), ra,
                           ma, sa, d_pairs);
    } else {
        return set_error(SSC_EINVAL, "%s: unknown env kind %d", fn, p->kind);
    }
    return check_launch(fn);
}
