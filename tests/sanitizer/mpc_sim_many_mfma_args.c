/* Host-side sanitizer job for the population forward simulation of bf16-MFMA models: ssc_mpc_forward_sim_many_mfma walks
 * n_items caller structs, runs every working item through the single call's checks, the class check and the image checks,
 * and sorts a table of the problem ranges to find an overlap.  Built against the ASan + UBSan host build of libssc
 * (tests/sanitizer/build.py builds the library; tests/test_mpc_sim_many_mfma_sanitizer_host.py this driver) and driven with
 * exactly-sized heap arrays, so a read past item n_items - 1 is a report.  Every call here fails validation or has nothing
 * to launch: no GPU.  Exit code 0 and no sanitizer report = pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssc.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, ssc_last_error()); ++failures; } } while (0)

static const ssc_mpc_sim_many_mfma_item *const D_ITEMS = (const ssc_mpc_sim_many_mfma_item *)(uintptr_t)0x70000000u;   /* never read on the host */
static const float *const D_S0 = (const float *)(uintptr_t)0x71000000u;
static float *const D_S = (float *)(uintptr_t)0x72000000u;
#define NSAMP 19

static void shape(ssc_mlp_desc *d, int hidden_layers, int depth, uintptr_t base) {
    d->n_layers = hidden_layers + 1;
    d->dims[0] = 3;
    for (int l = 1; l <= hidden_layers; ++l) d->dims[l] = depth;
    d->dims[hidden_layers + 1] = 2;
    for (int l = 0; l <= hidden_layers; ++l) {
        d->W[l] = (const float *)(base + 0x100000u * (uintptr_t)(2 * l + 1));
        d->b[l] = (const float *)(base + 0x100000u * (uintptr_t)(2 * l + 2));
    }
}

/* n valid items of class <16,1> (3 -> depth -> 2, depth 129 + p % 384), item p owning problems [2 p, 2 p + per) */
static ssc_mpc_sim_many_mfma_item *population(int n, int per) {
    ssc_mpc_sim_many_mfma_item *it = (ssc_mpc_sim_many_mfma_item *)malloc((size_t)n * sizeof *it);
    memset(it, 0, (size_t)n * sizeof *it);
    for (int p = 0; p < n; ++p) {
        shape(&it[p].mlp, 1, 129 + p % 384, (uintptr_t)0x01000000u * (uintptr_t)(p + 1));
        it[p].d_image = (const void *)((uintptr_t)0x60000000u + 0x100000u * (uintptr_t)p);
        it[p].image_bytes = ssc_dyn_workspace_bytes(&it[p].mlp, 1, SSC_PREC_BF16_MFMA);
        it[p].problem0 = 2 * p; it[p].n_problems = per;
    }
    return it;
}

static int run(const ssc_mpc_sim_many_mfma_item *it, int n, const ssc_mpc_sampling *sp, int64_t problems, float *d_S) {
    return ssc_mpc_forward_sim_many_mfma(it, D_ITEMS, n, sp, problems * NSAMP, 4, 2, 1, D_S0, 1, NULL, d_S, NULL);
}

int main(void) {
    ssc_mpc_sim_many_mfma_item *it;
    char want[64];
    ssc_mpc_sampling sp;
    memset(&sp, 0, sizeof sp);
    sp.n_samples = NSAMP; sp.low[0] = -1.0f; sp.high[0] = 1.0f; sp.seed = 7; sp.problem_id0 = 3; sp.t = 5;

    /* the class function reads dims[] only as far as n_layers says */
    {
        ssc_mlp_desc *d = (ssc_mlp_desc *)malloc(sizeof *d);
        memset(d, 0, sizeof *d);
        EXPECT(ssc_dyn_mfma_many_class(NULL, 2, 1) == -1);
        shape(d, 1, 500, 0x01000000u);
        EXPECT(ssc_dyn_mfma_many_class(d, 2, 1) == 2);
        shape(d, 2, 126, 0x01000000u);
        EXPECT(ssc_dyn_mfma_many_class(d, 2, 1) == 6);
        shape(d, 2, 500, 0x01000000u);
        EXPECT(ssc_dyn_mfma_many_class(d, 2, 1) == -1);
        d->n_layers = SSC_MAX_LAYERS + 1;
        EXPECT(ssc_dyn_mfma_many_class(d, 2, 1) == -1);
        d->n_layers = -3;
        EXPECT(ssc_dyn_mfma_many_class(d, 2, 1) == -1);
        d->n_layers = INT32_MAX;
        EXPECT(ssc_dyn_mfma_many_class(d, 2, 1) == -1);
        free(d);
    }

    const int sizes[3] = {1, 2, 33};
    for (int k = 0; k < 3; ++k) {
        const int n = sizes[k];
        it = population(n, 2);
        EXPECT(ssc_mpc_forward_sim_many_mfma(NULL, D_ITEMS, n, &sp, 2 * n * NSAMP, 4, 2, 1, D_S0, 1, NULL, D_S, NULL) == SSC_EINVAL);
        EXPECT(ssc_mpc_forward_sim_many_mfma(it, NULL, n, &sp, 2 * n * NSAMP, 4, 2, 1, D_S0, 1, NULL, D_S, NULL) == SSC_EINVAL);
        EXPECT(run(it, 0, &sp, 2 * n, D_S) == SSC_EINVAL);
        EXPECT(run(it, -n, &sp, 2 * n, D_S) == SSC_EINVAL);
        EXPECT(run(it, 65536, &sp, 2 * n, D_S) == SSC_EUNSUPPORTED);                             /* on the count alone */
        EXPECT(run(it, n, NULL, 2 * n, D_S) == SSC_EINVAL);
        /* every item passes, the ranges tile [0, 2 n): what is refused is the missing output buffer, after the whole walk */
        EXPECT(run(it, n, &sp, 2 * n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "NULL device pointer") != NULL);
        snprintf(want, sizeof want, "item %d", n - 1);
        it[n - 1].mlp.dims[1] = 513;                                                              /* the LAST item is read */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EUNSUPPORTED && strstr(ssc_last_error(), want) != NULL);
        it[n - 1].mlp.dims[1] = 200;
        it[n - 1].mlp.n_layers = SSC_MAX_LAYERS + 1;                                              /* dims[] must not be walked */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "n_layers") != NULL &&
               strstr(ssc_last_error(), want) != NULL);
        it[n - 1].mlp.n_layers = 2;
        it[n - 1].mlp.b[1] = NULL;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "layer 1") != NULL);
        it[n - 1].mlp.b[1] = it[0].mlp.W[1];
        it[n - 1].d_image = NULL;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "d_image") != NULL && strstr(ssc_last_error(), want) != NULL);
        it[n - 1].d_image = (const void *)((uintptr_t)0x60000000u + 4);                           /* misaligned */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "aligned") != NULL);
        it[n - 1].d_image = (const void *)(uintptr_t)0x60000000u;                                 /* item 0's: a shared image is legal */
        it[n - 1].image_bytes -= 1;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "image") != NULL && strstr(ssc_last_error(), want) != NULL);
        it[n - 1].image_bytes = SIZE_MAX;
        it[n - 1].n_problems = -1;
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL);
        it[n - 1].n_problems = 3;                                                                 /* one problem past the end */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "outside") != NULL &&
               strstr(ssc_last_error(), want) != NULL);
        it[n - 1].n_problems = INT32_MAX;                                                         /* no signed overflow */
        EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EINVAL && strstr(ssc_last_error(), "outside") != NULL);
        free(it);
        /* rows of one item past 32 bits: n_samples 2^11, 2^20 problems */
        it = population(n, 2);
        {
            ssc_mpc_sampling big = sp;
            big.n_samples = 1 << 11;
            it[n - 1].n_problems = 1 << 20;
            EXPECT(ssc_mpc_forward_sim_many_mfma(it, D_ITEMS, n, &big, ((int64_t)2 * (n - 1) + (1 << 20)) * (1 << 11), 4, 2, 1, D_S0, 1,
                                                 NULL, D_S, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "32 bits") != NULL);
        }
        free(it);
        if (n > 1) {
            /* the class check: the last item differs from the first; an empty one is not looked at */
            it = population(n, 2);
            shape(&it[n - 1].mlp, 1, 128, 0x05000000u);
            snprintf(want, sizeof want, "items 0 and %d are of classes 2 and 1", n - 1);
            EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EUNSUPPORTED && strstr(ssc_last_error(), want) != NULL);
            shape(&it[n - 1].mlp, 2, 100, 0x05000000u);
            snprintf(want, sizeof want, "items 0 and %d are of classes 2 and 6", n - 1);
            EXPECT(run(it, n, &sp, 2 * n, D_S) == SSC_EUNSUPPORTED && strstr(ssc_last_error(), want) != NULL);
            it[n - 1].n_problems = 0;
            EXPECT(run(it, n, &sp, 2 * n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "NULL device pointer") != NULL);
            free(it);
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
