/* Host-side sanitizer job for the six population-selection entry points over ssc_select_many_item
 * (ssc_replay_smart_start_indices_many, ssc_kde_scott_bandwidth_many, ssc_critic_forward_many, ssc_kde_evaluate_many,
 * ssc_ucb_topk_many, ssc_replay_episode_path_many): each walks n_items caller structs and validates them completely before
 * any HIP call.  Built against the ASan + UBSan host build of libssc (tests/sanitizer/build.py builds the library;
 * tests/test_select_many_sanitizer_host.py this driver) and driven with exactly-sized heap arrays, so a read past element
 * n - 1 is a report.  Every call here fails validation or has nothing to launch: no GPU.  Exit code 0 and no sanitizer
 * report = pass. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssc.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, ssc_last_error()); ++failures; } } while (0)
#define ERR(word) (strstr(ssc_last_error(), word) != NULL)
#define FAKE(T, a) ((T)(uintptr_t)(a))          /* made-up device addresses: never read on the host */

static const ssc_select_many_item *const D_ITEMS = FAKE(const ssc_select_many_item *, 0x70000000u);
static const float *const D_ACT = FAKE(const float *, 0x72000000u);

enum { N_SS = 5, CALLS = 6 };

/* n valid items: a ring of 64 records holding 40, a 64-32 critic, rows [5 p, 5 p + 5) of the action matrix */
static ssc_select_many_item *items(int n) {
    ssc_select_many_item *it = (ssc_select_many_item *)malloc((size_t)n * sizeof *it);
    memset(it, 0, (size_t)n * sizeof *it);
    for (int p = 0; p < n; ++p) {
        ssc_select_many_item *x = &it[p];
        uintptr_t b = (uintptr_t)0x01000000u + 0x10000u * (uintptr_t)p;
        x->ring.s = FAKE(float *, b + 0x100); x->ring.a = FAKE(float *, b + 0x200); x->ring.r = FAKE(float *, b + 0x300);
        x->ring.t = FAKE(uint8_t *, b + 0x400); x->ring.s2 = FAKE(float *, b + 0x500);
        x->ring.ep_steps = FAKE(int32_t *, b + 0x600); x->ring.ep_run = FAKE(int32_t *, b + 0x700);
        x->ring.capacity = 64; x->ring.obs_dim = 2; x->ring.act_dim = 1;
        x->count = 40; x->n = 4; x->n_ss = N_SS; x->n_plans = 3; x->seed = 7; x->counter = (uint64_t)p;
        x->stride = 1; x->n_data = 41; x->scott = 0.29;
        ssc_critic_desc *c = &x->critic;
        c->obs_dim = 2; c->act_dim = 1; c->h1 = 64; c->h2 = 32;
        c->W1 = FAKE(const float *, b + 0x1100); c->b1 = FAKE(const float *, b + 0x1200); c->W2 = FAKE(const float *, b + 0x1300);
        c->b2 = FAKE(const float *, b + 0x1400); c->W3 = FAKE(const float *, b + 0x1500); c->b3 = FAKE(const float *, b + 0x1600);
        x->alpha = 1.0f; x->beta = 2.0f; x->volume = 0.5; x->max_len = 18; x->row0 = (int64_t)N_SS * p;
        x->d_idx = FAKE(int32_t *, b + 0x2100); x->d_n_cand = FAKE(int32_t *, b + 0x2200); x->d_cand = FAKE(float *, b + 0x2300);
        x->d_wh = FAKE(float *, b + 0x2400); x->d_norm = FAKE(double *, b + 0x2500); x->d_status = FAKE(int32_t *, b + 0x2600);
        x->d_value = FAKE(float *, b + 0x2700); x->d_pdf = FAKE(float *, b + 0x2800); x->d_ucb = FAKE(float *, b + 0x2900);
        x->d_chosen = FAKE(int32_t *, b + 0x2a00); x->d_path = FAKE(float *, b + 0x2b00); x->d_len = FAKE(int32_t *, b + 0x2c00);
        x->d_workspace = FAKE(void *, b + 0x4000); x->workspace_bytes = ssc_replay_smart_start_workspace_bytes(N_SS);
    }
    return it;
}

static int call(int which, const ssc_select_many_item *h, const ssc_select_many_item *d, int n, int64_t m) {
    switch (which) {
    case 0: return ssc_replay_smart_start_indices_many(h, d, n, NULL);
    case 1: return ssc_kde_scott_bandwidth_many(h, d, n, NULL);
    case 2: return ssc_critic_forward_many(h, d, n, m, D_ACT, NULL);
    case 3: return ssc_kde_evaluate_many(h, d, n, NULL);
    case 4: return ssc_ucb_topk_many(h, d, n, NULL);
    default: return ssc_replay_episode_path_many(h, d, n, NULL);
    }
}

static void empty(ssc_select_many_item *it, int n) {
    for (int p = 0; p < n; ++p) it[p].count = 0;
}

int main(void) {
    char want[64];
    const int sizes[3] = {1, 3, 33};
    for (int k = 0; k < 3; ++k) {
        const int n = sizes[k];
        const int64_t m = (int64_t)N_SS * n;
        snprintf(want, sizeof want, "item %d", n - 1);
        for (int w = 0; w < CALLS; ++w) {
            ssc_select_many_item *it = items(n);
            ssc_select_many_item *last = &it[n - 1];
            EXPECT(call(w, NULL, D_ITEMS, n, m) == SSC_EINVAL && ERR("NULL item array"));
            EXPECT(call(w, it, NULL, n, m) == SSC_EINVAL && ERR("NULL item array"));
            EXPECT(call(w, it, D_ITEMS, 0, m) == SSC_EINVAL && ERR("n_items"));
            EXPECT(call(w, it, D_ITEMS, -n, m) == SSC_EINVAL);
            EXPECT(call(w, it, D_ITEMS, 65536, m) == SSC_EUNSUPPORTED);                    /* on the count alone */
            /* the checks every call makes, on the LAST item */
            last->n_ss = 4097;      EXPECT(call(w, it, D_ITEMS, n, m) == SSC_EINVAL && ERR("n_ss") && ERR(want)); last->n_ss = N_SS;
            last->n_ss = -1;        EXPECT(call(w, it, D_ITEMS, n, m) == SSC_EINVAL && ERR("n_ss")); last->n_ss = N_SS;
            last->count = -1;       EXPECT(call(w, it, D_ITEMS, n, m) == SSC_EINVAL && ERR("count") && ERR(want)); last->count = 40;
            last->ring.capacity = 0; EXPECT(call(w, it, D_ITEMS, n, m) == SSC_EINVAL && ERR("capacity") && ERR(want)); last->ring.capacity = 64;
            last->n = 0;            EXPECT(call(w, it, D_ITEMS, n, m) == SSC_EINVAL && ERR(want)); last->n = 4;
            last->ring.obs_dim = 9; EXPECT(call(w, it, D_ITEMS, n, m) == SSC_EINVAL && ERR("obs_dim") && ERR(want)); last->ring.obs_dim = 2;
            last->ring.capacity = INT64_MAX; last->count = INT64_MAX;
            EXPECT(call(w, it, D_ITEMS, n, m) == SSC_EINVAL && ERR("too large") && ERR(want));
            last->ring.capacity = 64; last->count = 40;
            /* an empty item is skipped and nothing else of it is read: garbage passes; every item empty: SSC_OK, nothing
             * launched (a launch would fail here: there is no device) */
            empty(it, n);
            last->ring.capacity = -5; last->ring.obs_dim = 77; last->n_plans = 999; last->d_idx = NULL; last->n = -3;
            last->critic.h1 = -1; last->stride = 0; last->max_len = 0; last->volume = -1.0; last->row0 = -7;
            EXPECT(call(w, it, D_ITEMS, n, m) == SSC_OK);
            free(it);
            it = items(n);
            for (int p = 0; p < n; ++p) { it[p].count = 40; it[p].n_ss = 0; }
            EXPECT(call(w, it, D_ITEMS, n, m) == SSC_OK);
            free(it);
        }
        /* per call, on the last item */
        ssc_select_many_item *it = items(n);
        ssc_select_many_item *last = &it[n - 1];
        ssc_select_many_item *ok = items(n);                      /* untouched: what a mutated field is put back from */
#define BAD(w, set, code, word, reset) do { set; EXPECT(call(w, it, D_ITEMS, n, m) == code && ERR(word) && ERR(want)); reset; } while (0)
        /* indices */
        BAD(0, last->ring.ep_steps = NULL, SSC_EINVAL, "episode index", last->ring.ep_steps = ok[n - 1].ring.ep_steps);
        BAD(0, last->d_idx = NULL, SSC_EINVAL, "NULL device pointer", last->d_idx = ok[n - 1].d_idx);
        BAD(0, last->d_cand = NULL, SSC_EINVAL, "NULL device pointer", last->d_cand = ok[n - 1].d_cand);
        BAD(0, last->d_n_cand = NULL, SSC_EINVAL, "NULL device pointer", last->d_n_cand = ok[n - 1].d_n_cand);
        BAD(0, last->workspace_bytes -= 1, SSC_EINVAL, "workspace", last->workspace_bytes += 1);
        BAD(0, last->d_workspace = NULL, SSC_EINVAL, "workspace", last->d_workspace = ok[n - 1].d_workspace);
        /* bandwidth */
        BAD(1, last->stride = 0, SSC_EINVAL, "stride", last->stride = 1);
        BAD(1, last->n_data = 40, SSC_EINVAL, "n_data", last->n_data = 41);
        BAD(1, (last->stride = 3, last->n_data = 13), SSC_EINVAL, "n_data", (last->stride = 1, last->n_data = 41));   /* ceil(41 / 3) = 14 */
        BAD(1, last->scott = 0.0, SSC_EINVAL, "scott", last->scott = 0.29);
        BAD(1, last->scott = INFINITY, SSC_EINVAL, "scott", last->scott = 0.29);
        BAD(1, last->scott = NAN, SSC_EINVAL, "scott", last->scott = 0.29);
        BAD(1, last->d_wh = NULL, SSC_EINVAL, "NULL device pointer", last->d_wh = ok[n - 1].d_wh);
        BAD(1, last->d_status = NULL, SSC_EINVAL, "NULL device pointer", last->d_status = ok[n - 1].d_status);
        /* critic: the single call's checks and codes, the row range */
        BAD(2, last->critic.obs_dim = 9, SSC_EINVAL, "out of range", last->critic.obs_dim = 2);
        BAD(2, last->critic.obs_dim = 3, SSC_EINVAL, "ring obs_dim", last->critic.obs_dim = 2);
        BAD(2, last->critic.h1 = 0, SSC_EINVAL, "hidden", last->critic.h1 = 64);
        BAD(2, last->critic.h1 = 600, SSC_EINVAL, "hidden", last->critic.h1 = 64);
        BAD(2, last->critic.b2 = NULL, SSC_EINVAL, "NULL device pointer", last->critic.b2 = ok[n - 1].critic.b2);
        BAD(2, last->critic.ln2_g = D_ACT, SSC_EINVAL, "LayerNorm", last->critic.ln2_g = NULL);
        BAD(2, (last->critic.ln1_g = last->critic.ln1_b = last->critic.ln2_g = last->critic.ln2_b = D_ACT, last->critic.h1 = 400, last->critic.h2 = 300),
            SSC_EUNSUPPORTED, "too wide", (last->critic.ln1_g = last->critic.ln1_b = last->critic.ln2_g = last->critic.ln2_b = NULL, last->critic.h1 = 64, last->critic.h2 = 32));
        BAD(2, last->row0 += 1, SSC_EINVAL, "outside", last->row0 -= 1);
        BAD(2, last->row0 = -1, SSC_EINVAL, "outside", last->row0 = (int64_t)N_SS * (n - 1));
        BAD(2, last->row0 = INT64_MAX, SSC_EINVAL, "outside", last->row0 = (int64_t)N_SS * (n - 1));          /* no signed overflow */
        BAD(2, last->d_value = NULL, SSC_EINVAL, "NULL device pointer", last->d_value = ok[n - 1].d_value);
        EXPECT(ssc_critic_forward_many(it, D_ITEMS, n, -1, D_ACT, NULL) == SSC_EINVAL);
        EXPECT(ssc_critic_forward_many(it, D_ITEMS, n, m, NULL, NULL) == SSC_EINVAL && ERR("d_act"));         /* after the whole walk */
        /* kde */
        BAD(3, last->n_data = 42, SSC_EINVAL, "n_data", last->n_data = 41);
        BAD(3, last->d_pdf = NULL, SSC_EINVAL, "NULL device pointer", last->d_pdf = ok[n - 1].d_pdf);
        BAD(3, last->d_norm = NULL, SSC_EINVAL, "NULL device pointer", last->d_norm = ok[n - 1].d_norm);
        if (n > 1) { last->ring.obs_dim = 3; EXPECT(call(3, it, D_ITEMS, n, m) == SSC_EUNSUPPORTED && ERR("items 0 and") && ERR("one obs_dim")); last->ring.obs_dim = 2; }
        /* top-k */
        BAD(4, last->n_plans = 0, SSC_EINVAL, "n_plans", last->n_plans = 3);
        BAD(4, last->n_plans = 65, SSC_EINVAL, "n_plans", last->n_plans = 3);
        BAD(4, last->volume = 0.0, SSC_EINVAL, "volume", last->volume = 0.5);
        BAD(4, last->volume = NAN, SSC_EINVAL, "volume", last->volume = 0.5);
        BAD(4, last->d_chosen = NULL, SSC_EINVAL, "NULL device pointer", last->d_chosen = ok[n - 1].d_chosen);
        /* paths */
        BAD(5, last->max_len = 0, SSC_EINVAL, "max_len", last->max_len = 18);
        BAD(5, last->n_plans = 65, SSC_EINVAL, "n_plans", last->n_plans = 3);
        BAD(5, last->ring.ep_steps = NULL, SSC_EINVAL, "episode index", last->ring.ep_steps = ok[n - 1].ring.ep_steps);
        BAD(5, last->d_len = NULL, SSC_EINVAL, "NULL device pointer", last->d_len = ok[n - 1].d_len);
        free(it);
        free(ok);
    }
    if (failures) { printf("%d expectation(s) failed\n", failures); return 1; }
    printf("all expectations hold\n");
    return 0;
}
