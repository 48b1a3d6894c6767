/* Host-side sanitizer job for the grouped dynamics-model step: ssc_mlp_train_steps_many walks n_models caller structs, runs
 * every trained model through the single call's checks and sorts a table of the byte ranges the launches would write and
 * read.  Built against the ASan + UBSan host build of libssc (tests/sanitizer/build.py builds the library;
 * tests/test_mlp_train_many_sanitizer_host.py this driver) and driven with exactly-sized heap arrays, so a read past item
 * n_models - 1 is a report.  Every call here fails validation or has nothing to launch: no GPU.  Exit code 0 and no
 * sanitizer report = pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssc.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, ssc_last_error()); ++failures; } } while (0)

static const ssc_mlp_train_many_item *const D_ITEMS = (const ssc_mlp_train_many_item *)(uintptr_t)0x70000000u;   /* never read on the host */

/* n valid <3,2> models (hidden width 16 + p % 40, batch 33 + p), every array and workspace at a made-up address of its own */
static ssc_mlp_train_many_item *population(int n, int n_steps) {
    ssc_mlp_train_many_item *it = (ssc_mlp_train_many_item *)malloc((size_t)n * sizeof *it);
    memset(it, 0, (size_t)n * sizeof *it);
    for (int p = 0; p < n; ++p) {
        ssc_mlp_train_desc *d = &it[p].net;
        uintptr_t base = (uintptr_t)0x10000000u * (uintptr_t)(p + 1);
        d->n_layers = 2; d->dims[0] = 3; d->dims[1] = 16 + p % 40; d->dims[2] = 2;
        for (int l = 0; l < 2; ++l) {
            uintptr_t a = base + (uintptr_t)0x600000u * (uintptr_t)l;
            d->W[l] = (float *)(a + 0x100000); d->b[l] = (float *)(a + 0x200000);
            d->mW[l] = (float *)(a + 0x300000); d->vW[l] = (float *)(a + 0x400000);
            d->mb[l] = (float *)(a + 0x500000); d->vb[l] = (float *)(a + 0x600000);
        }
        d->adam_t = (int32_t *)(base + 0xD00000);
        d->lr = 1e-3f; d->beta1 = 0.9f; d->beta2 = 0.999f; d->epsilon = 1e-8f;
        it[p].d_X = (const float *)(base + 0x1000000); it[p].d_Z = (const float *)(base + 0x2000000);
        it[p].d_idx = (const int32_t *)(base + 0x3000000);
        it[p].batch = 33 + p; it[p].n_steps = n_steps;
        it[p].d_loss = p % 2 ? NULL : (float *)(base + 0x4000000);
        it[p].d_workspace = (void *)(base + 0x5000000);
        it[p].workspace_bytes = ssc_mlp_train_workspace_bytes(d, it[p].batch);
    }
    return it;
}

int main(void) {
    ssc_mlp_train_many_item *it;
    char want[48];
    unsetenv("SSC_DYN_TRAIN_GENERIC");

    const int sizes[2] = {1, 33};
    for (int k = 0; k < 2; ++k) {
        const int n = sizes[k];
        it = population(n, 3);
        EXPECT(ssc_mlp_train_steps_many(NULL, D_ITEMS, n, NULL) == SSC_EINVAL);
        EXPECT(ssc_mlp_train_steps_many(it, NULL, n, NULL) == SSC_EINVAL);
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, 0, NULL) == SSC_EINVAL);
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, -n, NULL) == SSC_EINVAL);
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, 65536, NULL) == SSC_EUNSUPPORTED);          /* on the count alone */
        snprintf(want, sizeof want, "model %d", n - 1);
        it[n - 1].workspace_bytes -= 1;                                                           /* the LAST item is read */
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "workspace") != NULL &&
               strstr(ssc_last_error(), want) != NULL);
        it[n - 1].workspace_bytes += 1;
        it[n - 1].net.dims[1] = 513;                                                              /* outside the fused kernel */
        it[n - 1].workspace_bytes = ssc_mlp_train_workspace_bytes(&it[n - 1].net, it[n - 1].batch);
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EUNSUPPORTED && strstr(ssc_last_error(), want) != NULL);
        it[n - 1].net.dims[1] = 16;
        it[n - 1].net.n_layers = SSC_MAX_LAYERS + 1;                                              /* dims[] must not be walked */
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "n_layers") != NULL);
        it[n - 1].net.n_layers = 2;
        it[n - 1].n_steps = -1;
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL);
        free(it);
        if (n > 1) {
            it = population(n, 3);
            it[n - 1].net.dims[0] = 4; it[n - 1].net.dims[2] = 3;                                 /* another instantiation */
            it[n - 1].workspace_bytes = ssc_mlp_train_workspace_bytes(&it[n - 1].net, it[n - 1].batch);
            EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "<4,3>") != NULL &&
                   strstr(ssc_last_error(), "model 0") != NULL && strstr(ssc_last_error(), want) != NULL);
            free(it);
            snprintf(want, sizeof want, "models 0 and %d", n - 1);
            it = population(n, 3);
            it[n - 1].net.vb[1] = it[0].net.W[0];                                                 /* first and last on one array */
            EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL);
            free(it);
            it = population(n, 3);
            it[n - 1].d_idx = (const int32_t *)((uintptr_t)it[0].d_workspace + it[0].workspace_bytes - 4);   /* a read over a tail */
            EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL &&
                   strstr(ssc_last_error(), "read") != NULL);
            it[n - 1].d_idx = (const int32_t *)((uintptr_t)it[0].d_workspace + it[0].workspace_bytes);       /* ... and just behind it */
            it[n - 1].d_loss = it[0].d_loss;
            EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "written") != NULL);
            free(it);
            it = population(n, 3);                                                                /* shared reads are legal: the   */
            for (int p = 1; p < n; ++p) {                                                         /* one conflict is what is named */
                it[p].d_X = it[0].d_X; it[p].d_Z = it[0].d_Z; it[p].d_idx = it[0].d_idx; it[p].batch = it[0].batch;
            }
            it[n - 1].net.adam_t = it[n - 2].net.adam_t;
            snprintf(want, sizeof want, "models %d and %d", n - 2, n - 1);
            EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), want) != NULL);
            free(it);
        }
        /* nothing to do anywhere, one item garbage: "launched" without a launch */
        it = population(n, 0);
        memset(&it[n / 2], 0xFF, sizeof it[0]);
        it[n / 2].n_steps = 0;
        EXPECT(ssc_mlp_train_steps_many(it, D_ITEMS, n, NULL) == SSC_OK);
        free(it);
    }

    if (failures == 0) printf("all expectations hold\n");
    return failures == 0 ? 0 : 1;
}
