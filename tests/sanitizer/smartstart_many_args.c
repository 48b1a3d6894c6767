/* Host-side sanitizer job for the SmartStart population entry points: ssc_actor_forward_many walks n_items caller structs,
 * runs every working item through the single call's descriptor checks and sorts a table of the row ranges to find an
 * overlap; ssc_smartstart_rollout_step_many walks n_pairs rows of the pair table.  Built against the ASan + UBSan host
 * build of libssc (tests/sanitizer/build.py builds the library; tests/test_smartstart_many_sanitizer_host.py this driver)
 * and driven with exactly-sized heap arrays, so a read past element n - 1 is a report.  Every call here fails validation or
 * has nothing to launch: no GPU.  Exit code 0 and no sanitizer report = pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssc.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, ssc_last_error()); ++failures; } } while (0)
#define ERR(word) (strstr(ssc_last_error(), word) != NULL)
#define FAKE(T, a) ((T)(uintptr_t)(a))          /* made-up device addresses: never read on the host */

static const ssc_actor_many_item *const D_ITEMS = FAKE(const ssc_actor_many_item *, 0x70000000u);
static const float *const D_OBS = FAKE(const float *, 0x71000000u);
static float *const D_ACT = FAKE(float *, 0x72000000u);

/* n valid fp32 64-32 items, item p owning rows [3 p, 3 p + per): per = 3 leaves no gaps */
static ssc_actor_many_item *actors(int n, int per) {
    ssc_actor_many_item *it = (ssc_actor_many_item *)malloc((size_t)n * sizeof *it);
    memset(it, 0, (size_t)n * sizeof *it);
    for (int p = 0; p < n; ++p) {
        ssc_actor_desc *a = &it[p].actor;
        uintptr_t base = (uintptr_t)0x01000000u + 0x1000u * (uintptr_t)p;
        a->obs_dim = 2; a->h1 = 64; a->h2 = 32; a->act_dim = 1; a->precision = SSC_PREC_F32;
        a->W1 = FAKE(const float *, base + 0x100); a->b1 = FAKE(const float *, base + 0x200); a->W2 = FAKE(const float *, base + 0x300);
        a->b2 = FAKE(const float *, base + 0x400); a->W3 = FAKE(const float *, base + 0x500); a->b3 = FAKE(const float *, base + 0x600);
        it[p].row0 = 3 * (int64_t)p; it[p].rows = per;
    }
    return it;
}

static int fwd(const ssc_actor_many_item *it, int n, int64_t m) { return ssc_actor_forward_many(it, D_ITEMS, n, m, D_OBS, D_ACT, NULL); }

static void actor_many(void) {
    char want[64];
    const int sizes[3] = {1, 2, 33};
    for (int k = 0; k < 3; ++k) {
        const int n = sizes[k];
        const int64_t m = 3 * (int64_t)n;
        ssc_actor_many_item *it = actors(n, 3);
        EXPECT(ssc_actor_forward_many(NULL, D_ITEMS, n, m, D_OBS, D_ACT, NULL) == SSC_EINVAL);
        EXPECT(ssc_actor_forward_many(it, NULL, n, m, D_OBS, D_ACT, NULL) == SSC_EINVAL);
        EXPECT(fwd(it, 0, m) == SSC_EINVAL && ERR("n_items"));
        EXPECT(fwd(it, -n, m) == SSC_EINVAL);
        EXPECT(fwd(it, 65536, m) == SSC_EUNSUPPORTED);                                     /* on the count alone */
        EXPECT(fwd(it, n, -1) == SSC_EINVAL);
        /* every item passes, the ranges tile [0, m): what is refused is the missing buffer, after the whole walk */
        EXPECT(ssc_actor_forward_many(it, D_ITEMS, n, m, NULL, D_ACT, NULL) == SSC_EINVAL && ERR("NULL device pointer"));
        EXPECT(ssc_actor_forward_many(it, D_ITEMS, n, m, D_OBS, NULL, NULL) == SSC_EINVAL && ERR("NULL device pointer"));
        snprintf(want, sizeof want, "item %d", n - 1);
        ssc_actor_many_item *last = &it[n - 1];
        /* the single call's per-descriptor checks, with its codes, on the LAST item */
        last->actor.obs_dim = 9;  EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("out of range") && ERR(want)); last->actor.obs_dim = 2;
        last->actor.act_dim = 0;  EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("out of range")); last->actor.act_dim = 1;
        last->actor.h2 = 0;       EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("hidden")); last->actor.h2 = 32;
        last->actor.b2 = NULL;    EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("NULL device pointer") && ERR(want));
        last->actor.b2 = it[0].actor.W2;                                                   /* shared arrays are legal */
        last->actor.ln1_g = D_OBS; EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("LayerNorm")); last->actor.ln1_g = NULL;
        last->actor.precision = 5; EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("precision") && ERR(want));
        last->actor.precision = SSC_PREC_BF16_MFMA; last->actor.h1 = 225;                  /* no class */
        EXPECT(fwd(it, n, m) == SSC_EUNSUPPORTED && ERR(want));
        last->actor.precision = SSC_PREC_F32; last->actor.h1 = 513;
        EXPECT(fwd(it, n, m) == SSC_EUNSUPPORTED && ERR("512") && ERR(want));
        last->actor.h1 = 64;
        last->actor.ln1_g = last->actor.ln1_b = last->actor.ln2_g = last->actor.ln2_b = D_OBS; last->actor.precision = SSC_PREC_BF16_MFMA;
        EXPECT(fwd(it, n, m) == SSC_EUNSUPPORTED && ERR("LayerNorm"));
        last->actor.ln1_g = last->actor.ln1_b = last->actor.ln2_g = last->actor.ln2_b = NULL; last->actor.precision = SSC_PREC_F32;
        /* ranges */
        last->rows = -1;          EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("rows") && ERR(want));
        last->rows = 4;           EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("outside") && ERR(want));      /* one row past the end */
        last->rows = INT64_MAX;   EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("outside"));                   /* no signed overflow */
        last->rows = 3; last->row0 = -1; EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("outside"));
        last->row0 = INT64_MAX;   EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("outside"));
        free(it);
        if (n > 1) {
            it = actors(n, 3);
            it[n - 1].actor.precision = SSC_PREC_BF16_MFMA;                                /* two classes in one call */
            snprintf(want, sizeof want, "items 0 and %d", n - 1);
            EXPECT(fwd(it, n, m) == SSC_EUNSUPPORTED && ERR(want) && ERR("classes 0 and 4"));
            it[n - 1].actor.precision = SSC_PREC_F32;
            it[n - 1].d_rms = FAKE(const double *, 0x73000000u);                           /* has-rms is part of the class */
            EXPECT(fwd(it, n, m) == SSC_EUNSUPPORTED && ERR(want) && ERR("classes 0 and 1"));
            it[n - 1].d_rms = NULL;
            it[n - 1].row0 = 1;                                                            /* last item over the first */
            EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR(want) && ERR("overlap"));
            free(it);
            it = actors(n, 1);                                                             /* gaps everywhere: legal; */
            it[n - 1].row0 = 3 * (int64_t)(n - 2); it[n - 1].rows = 2;                     /* one pair collides       */
            snprintf(want, sizeof want, "items %d and %d", n - 2, n - 1);
            EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR(want));
            it[n - 1].row0 = 3 * (int64_t)(n - 2) + 1;                                     /* ... and just behind it */
            EXPECT(ssc_actor_forward_many(it, D_ITEMS, n, m, NULL, D_ACT, NULL) == SSC_EINVAL && ERR("NULL device pointer"));
            free(it);
            it = actors(n, 3);                                                             /* one range swallows all */
            it[0].rows = m;
            EXPECT(fwd(it, n, m) == SSC_EINVAL && ERR("items 0 and 1"));
            free(it);
        }
        /* nothing to do anywhere, one item garbage: "launched" without a launch; and m == 0 */
        it = actors(n, 0);
        memset(&it[n / 2], 0xFF, sizeof it[0]);
        it[n / 2].rows = 0;
        EXPECT(fwd(it, n, m) == SSC_OK);
        EXPECT(ssc_actor_forward_many(it, D_ITEMS, n, 0, NULL, NULL, NULL) == SSC_OK);
        free(it);
    }
    /* the largest table: 65535 items are walked to the end (the last one is wrong), and all of them empty is SSC_OK */
    ssc_actor_many_item *it = actors(65535, 3);
    it[65534].actor.W3 = NULL;
    EXPECT(fwd(it, 65535, 3 * 65535) == SSC_EINVAL && ERR("item 65534"));
    it[65534].actor.W3 = it[0].actor.W3;
    EXPECT(ssc_actor_forward_many(it, D_ITEMS, 65535, 3 * 65535, D_OBS, NULL, NULL) == SSC_EINVAL && ERR("NULL device pointer"));
    for (int p = 0; p < 65535; ++p) it[p].rows = 0;
    EXPECT(fwd(it, 65535, 3 * 65535) == SSC_OK);
    free(it);
}

/* ---- ssc_smartstart_rollout_step_many --------------------------------------------------------------------------------- */
#define PER 5
static ssc_smartstart_pair *pairs(int n) {
    ssc_smartstart_pair *q = (ssc_smartstart_pair *)malloc((size_t)n * sizeof *q);
    memset(q, 0, (size_t)n * sizeof *q);
    for (int y = 0; y < n; ++y) {
        q[y].env0 = PER * y; q[y].n_envs = PER; q[y].slot0 = 3 * y;
        q[y].pool_first = 1; q[y].pool_count = 2; q[y].pool_slots = 3; q[y].eta = 0.5f; q[y].ou_epsilon = 0.3f;
        q[y].ou.mu = 0.4f; q[y].ou.sigma = 0.2f; q[y].ou.theta = 0.15f; q[y].ou.dt = 0.01f;
    }
    return q;
}

struct step_call {
    ssc_env_params p; ssc_mpc_problems pr; ssc_mpc_nav_state nav; ssc_smartstart_step ss; ssc_rollout_state st;
    uint64_t *d_t; int32_t *d_k, *d_ticket; float *d_plan;
};

static void step_defaults(struct step_call *c, int n_pairs) {
    memset(c, 0, sizeof *c);
    ssc_env_params_default(SSC_ENV_MOUNTAINCAR, 1.0f, 17, &c->p);
    c->pr.n_problems = PER * n_pairs; c->pr.n_samples = 16; c->pr.horizon = 3; c->pr.state_dim = 2;
    c->pr.wp = FAKE(const float *, 0x10000); c->pr.left = FAKE(const float *, 0x11000); c->pr.wp_off = FAKE(const int32_t *, 0x12000);
    c->pr.cur_idx = FAKE(int32_t *, 0x13000); c->pr.radii = FAKE(const float *, 0x14000); c->pr.theta = 1.0f; c->pr.gamma = 0.75f;
    c->pr.plan_of = FAKE(int32_t *, 0x15000); c->pr.wp_len = FAKE(const int32_t *, 0x16000);
    c->nav.cur_idx = FAKE(int32_t *, 0x13000); c->nav.start_idx = FAKE(const int32_t *, 0x17000); c->nav.actions_done = FAKE(int32_t *, 0x18000);
    c->nav.give_up_after = 2; c->nav.final_steps = 4;
    c->ss.mode = FAKE(uint8_t *, 0x19000); c->ss.plan_of = FAKE(int32_t *, 0x15000); c->ss.d_actor_out = FAKE(const float *, 0x1a000);
    c->ss.act_low = -1.0f; c->ss.act_high = 1.0f;
    c->st.s0 = FAKE(float *, 0x1b000); c->st.s1 = FAKE(float *, 0x1c000); c->st.steps = FAKE(int32_t *, 0x1d000);
    c->st.ep_ret = FAKE(float *, 0x1e000); c->st.ou_x = FAKE(float *, 0x1f000);
    c->d_t = FAKE(uint64_t *, 0x20000); c->d_k = FAKE(int32_t *, 0x21000); c->d_ticket = FAKE(int32_t *, 0x22000); c->d_plan = FAKE(float *, 0x23000);
}

static int step(const struct step_call *c, const ssc_smartstart_pair *h, const ssc_smartstart_pair *d, int n) {
    return ssc_smartstart_rollout_step_many(&c->p, &c->pr, &c->nav, &c->ss, h, d, n, FAKE(const float *, 0x24000), FAKE(const int32_t *, 0x25000),
                                            0.005f, 7, 40, &c->st, NULL, NULL, NULL, 9, 40, c->d_t, c->d_k, c->d_ticket, c->d_plan, NULL);
}

static void step_many(void) {
    const ssc_smartstart_pair *const D_PAIRS = FAKE(const ssc_smartstart_pair *, 0x74000000u);
    char want[32];
    const int sizes[3] = {1, 2, 33};
    for (int k = 0; k < 3; ++k) {
        const int n = sizes[k];
        struct step_call c;
        step_defaults(&c, n);
        ssc_smartstart_pair *q = pairs(n), *last = &q[n - 1];
        snprintf(want, sizeof want, "pair %d", n - 1);
        /* the table; every case below leaves exactly one thing wrong, so nothing launches */
        EXPECT(step(&c, NULL, D_PAIRS, n) == SSC_EINVAL && ERR("pair table"));
        EXPECT(step(&c, q, NULL, n) == SSC_EINVAL && ERR("pair table"));
        EXPECT(step(&c, q, D_PAIRS, 0) == SSC_EINVAL && ERR("n_pairs"));
        EXPECT(step(&c, q, D_PAIRS, -1) == SSC_EINVAL && ERR("n_pairs"));
        EXPECT(step(&c, q, D_PAIRS, 65536) == SSC_EUNSUPPORTED && ERR("n_pairs"));              /* on the count alone */
        /* the single call's checks */
        c.ss.d_n_live = FAKE(int32_t *, 0x26000); EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("d_n_live")); c.ss.d_n_live = NULL;
        c.ss.mode = NULL;   EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("step descriptor")); c.ss.mode = FAKE(uint8_t *, 0x19000);
        c.st.ou_x = NULL;   EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("ou_x")); c.st.ou_x = FAKE(float *, 0x1f000);
        c.ss.plan_of = FAKE(int32_t *, 0x99000); EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("plan pool")); c.ss.plan_of = FAKE(int32_t *, 0x15000);
        c.ss.act_low = 2.0f; EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("action bounds")); c.ss.act_low = -1.0f;
        c.pr.state_dim = 3; EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("observation space")); c.pr.state_dim = 2;
        c.d_plan = NULL;    EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("NULL device pointer")); c.d_plan = FAKE(float *, 0x23000);
        EXPECT(ssc_smartstart_rollout_step_many(&c.p, &c.pr, &c.nav, NULL, q, D_PAIRS, n, FAKE(const float *, 0x24000), FAKE(const int32_t *, 0x25000),
                                                0.0f, 7, 40, &c.st, NULL, NULL, NULL, 9, 40, c.d_t, c.d_k, c.d_ticket, c.d_plan, NULL) == SSC_EINVAL);
        /* the rows, the LAST one wrong */
        last->n_envs = 0;          EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("n_envs") && ERR(want)); last->n_envs = PER;
        last->n_envs = PER + 1;    EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("outside") && ERR(want));
        last->n_envs = INT32_MAX;  EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("outside")); last->n_envs = PER;   /* no overflow */
        last->env0 = -1;           EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR(want)); last->env0 = PER * (n - 1);
        last->pool_slots = 0;      EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("pool") && ERR(want)); last->pool_slots = 3;
        last->pool_first = 3;      EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("pool")); last->pool_first = -1;
        EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("pool")); last->pool_first = 1;
        last->pool_count = 4;      EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("pool")); last->pool_count = -1;
        EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("pool") && ERR(want)); last->pool_count = 0;                  /* 0 is legal */
        last->slot0 = -1;          EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("slot0") && ERR(want)); last->slot0 = 0;
        if (n > 1) {
            last->env0 -= 1;       EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("overlap") && ERR(want)); last->env0 += 1;   /* overlap */
            const ssc_smartstart_pair t = q[0]; q[0] = *last; *last = t;                                                     /* out of order */
            EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("out of order"));
            *last = q[0]; q[0] = t;
        }
        /* a legal table: gaps between the ranges pass; what is left is the unknown env kind, behind the whole walk */
        c.pr.n_problems += 4; last->env0 += 4;
        c.p.kind = 7; c.pr.state_dim = 3;                    /* (an unknown kind plans in three dimensions) */
        EXPECT(step(&c, q, D_PAIRS, n) == SSC_EINVAL && ERR("env kind"));
        free(q);
    }
    struct step_call c;                                      /* 65535 rows are walked to the end */
    step_defaults(&c, 65535);
    ssc_smartstart_pair *q = pairs(65535);
    q[65534].pool_slots = 0;
    EXPECT(step(&c, q, D_PAIRS, 65535) == SSC_EINVAL && ERR("pair 65534"));
    free(q);
}

int main(void) {
    actor_many();
    step_many();
    if (failures == 0) printf("all expectations hold\n");
    return failures == 0 ? 0 : 1;
}
