/* Host-side sanitizer job for the population forward simulation: ssc_mpc_forward_sim_many walks n_items caller structs, runs
 * every working item through the single call's checks and sorts a table of the problem ranges to find an overlap.  Built
 * against the ASan + UBSan host build of libssc (tests/sanitizer/build.py builds the library;
 * tests/test_mpc_sim_many_sanitizer_host.py this driver) and driven with exactly-sized heap arrays, so a read past item
 * n_items - 1 is a report.  Every call here fails validation or has nothing to launch: no GPU.  Exit code 0 and no
 * sanitizer report = pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssc.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, ssc_last_error()); ++failures; } } while (0)

static const ssc_mpc_sim_many_item *const D_ITEMS = (const ssc_mpc_sim_many_item *)(uintptr_t)0x70000000u;   /* never read on the host */
static const float *const D_S0 = (const float *)(uintptr_t)0x71000000u;
static float *const D_S = (float *)(uintptr_t)0x72000000u;
#define NSAMP 19

/* n valid items (3 -> depth -> 2, depth 1 + p % 128), item p owning problems [2 p, 2 p + per): per = 2 leaves no gaps */
static ssc_mpc_sim_many_item *population(int n, int per) {
    ssc_mpc_sim_many_item *it = (ssc_mpc_sim_many_item *)malloc((size_t)n * sizeof *it);
    memset(it, 0, (size_t)n * sizeof *it);
    for (int p = 0; p < n; ++p) {
        ssc_mlp_desc *d = &it[p].mlp;
        uintptr_t base = (uintptr_t)0x01000000u * (uintptr_t)(p + 1);
        d->n_layers = 2; d->dims[0] = 3; d->dims[1] = 1 + p % 128; d->dims[2] = 2;
        for (int l = 0; l < 2; ++l) {
            d->W[l] = (const float *)(base + 0x100000u * (uintptr_t)(2 * l + 1));
            d->b[l] = (const float *)(base + 0x100000u * (uintptr_t)(2 * l + 2));
        }
        for (int k = 0; k < 2; ++k) it[p].norm.std_x[k] = it[p].norm.std_z[k] = 1.0f;
        it[p].norm.std_y[0] = 1.0f;
        it[p].problem0 = 2 * p; it[p].n_problems = per;
    }
    return it;
}

static int run(const ssc_mpc_sim_many_item *it, int n, const ssc_mpc_sampling *sp, int64_t problems, float *d_S) {
    return ssc_mpc_forward_sim_many(it, D_ITEMS, n, sp, problems * NSAMP, 4, 2, 1, D_S0, 1, NULL, d_S, NULL);
}

int main(void) {
    ssc_mpc_sim_many_item *it;
    char want[48];
    ssc_mpc_sampling sp;
    memset(&sp, 0, sizeof sp);
    sp.n_samples = NSAMP; sp.low[0] = -1.0f; sp.high[0] = 1.0f; sp.seed = 7; sp.problem_id0 = 3; sp.t = 5;

    const int sizes[3] = {1, 2, 33};
    for (int k = 0; k < 3; ++k) {
        const int n = sizes[k];
        it = population(n, 2);
        EXPECT(ssc_mpc_forward_sim_many(NULL, D_ITEMS, n, &sp, 2 * n * NSAMP, 4, 2, 1, D_S0, 1, NULL, D_S, NULL) == SSC_EINVAL);
        EXPECT(ssc_mpc_forward_sim_many(it, NULL, n, &sp, 2 * n * NSAMP, 4, 2, 1, D_S0, 1, NULL, D_S, NULL) == SSC_EINVAL);
        EXPECT(run(it, 0, &sp, 2 * n, D_S) == SSC_EINVAL);
        EXPECT(run(it, -n, &sp, 2 * n, D_S) == SSC_EINVAL);
        EXPECT(run(it, 65536, &sp, 2 * n, D_S) == SSC_EUNSUPPORTED);                             /* on the count alone */
        EXPECT(run(it, n, NULL, 2 * n, D_S) == SSC_EINVAL);
        /* every item passes, the ranges tile [0, 2 n): what is refused is the missing output buffer, after the whole walk */
        EXPECT(run(it, n, &sp, 2 * n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "NULL device pointer") != NULL);
        snprintf(want, sizeof want, "item %d", n - 1);
        it[n - 1].mlp.dims[1] = 129;                                                              /* the LAST item is read */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EUNSUPPORTED && strstr(ssc_last_error(), want) != NULL);
        it[n - 1].mlp.dims[1] = 16;
        it[n - 1].mlp.n_layers = SSC_MAX_LAYERS + 1;                                              /* dims[] must not be walked */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "n_layers") != NULL &&
               strstr(ssc_last_error(), want) != NULL);
        it[n - 1].mlp.n_layers = 2;
        it[n - 1].mlp.b[1] = NULL;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "layer 1") != NULL);
        it[n - 1].mlp.b[1] = it[0].mlp.W[1];                                                      /* shared weights are legal */
        it[n - 1].n_problems = -1;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL);
        it[n - 1].n_problems = 3;                                                                 /* one problem past the end */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "outside") != NULL &&
               strstr(ssc_last_error(), want) != NULL);
        it[n - 1].n_problems = INT32_MAX;                                                         /* no signed overflow */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "outside") != NULL);
        free(it);
        if (n > 1) {
            it = population(n, 2);
            it[n - 1].problem0 = 1;                                                               /* last item over the first */
            snprintf(want, sizeof want, "items 0 and %d", n - 1);
            EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL);
            free(it);
            it = population(n, 1);                                                                /* gaps everywhere: legal; */
            it[n - 1].problem0 = 2 * (n - 2); it[n - 1].n_problems = 2;                           /* one pair collides       */
            snprintf(want, sizeof want, "items %d and %d", n - 2, n - 1);
            EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL);
            it[n - 1].problem0 = 2 * (n - 2) + 1;                                                 /* ... and just behind it */
            EXPECT(run(it, n, &sp, 2 * n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "NULL device pointer") != NULL);
            free(it);
            it = population(n, 2);                                                                /* one range swallows all */
            it[0].n_problems = 2 * n;
            EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "items 0 and 1") != NULL);
            free(it);
        }
        /* the compact list is refused whatever the items hold */
        it = population(n, 2);
        sp.d_live_list = (const int32_t *)(uintptr_t)0x74000000u;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "live") != NULL);
        sp.d_live_list = NULL;
        free(it);
        /* nothing to do anywhere, one item garbage: "launched" without a launch; and m == 0 */
        it = population(n, 0);
        memset(&it[n / 2], 0xFF, sizeof it[0]);
        it[n / 2].n_problems = 0;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_OK);
        EXPECT(run(it, n, &sp, 0, NULL) == SSC_OK);
        free(it);
    }

    if (failures == 0) printf("all expectations hold\n");
    return failures == 0 ? 0 : 1;
}
