/* Host-side sanitizer job for the population entry points: ssc_ddpg_train_many and ssc_replay_sample_many walk caller
 * arrays of n_agents structs and sort a vector of their pointers before any HIP call.  Built against the ASan + UBSan
 * host build of libssc (tests/sanitizer/build.py builds the library; tests/test_ddpg_many_sanitizer_host.py this driver)
 * and driven with exactly-sized heap arrays, so a read past item n_agents - 1 is a report.  Every call here fails
 * validation or has nothing to launch: no GPU.  Exit code 0 and no sanitizer report = pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssc.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, ssc_last_error()); ++failures; } } while (0)

static const ssc_ddpg_many_item *const D_ITEMS = (const ssc_ddpg_many_item *)(uintptr_t)0x70000000u;   /* never read on the host */

/* n valid items of the shipped shape, every array at a made-up address of its own */
static ssc_ddpg_many_item *population(int n, int n_iters) {
    ssc_ddpg_many_item *it = (ssc_ddpg_many_item *)malloc((size_t)n * sizeof *it);
    memset(it, 0, (size_t)n * sizeof *it);
    for (int p = 0; p < n; ++p) {
        ssc_ddpg_desc *d = &it[p].ddpg;
        uintptr_t base = (uintptr_t)0x100000u * (uintptr_t)(p + 1);
        d->obs_dim = 2; d->act_dim = 1; d->actor_h1 = d->critic_h1 = 64; d->actor_h2 = d->critic_h2 = 32;
        d->last_layer_tanh = 1; d->batch_size = 64;
        d->actor = (float *)(base + 0x1000); d->critic = (float *)(base + 0x2000);
        d->target_actor = (float *)(base + 0x3000); d->target_critic = (float *)(base + 0x4000);
        d->adam_m_actor = (float *)(base + 0x5000); d->adam_v_actor = (float *)(base + 0x6000);
        d->adam_m_critic = (float *)(base + 0x7000); d->adam_v_critic = (float *)(base + 0x8000);
        d->adam_t = (int32_t *)(base + 0x9000);
        d->gamma = 0.99f; d->tau = 0.001f; d->actor_lr = 1e-4f; d->critic_lr = 1e-3f;
        d->beta1 = 0.9f; d->beta2 = 0.999f; d->epsilon = 1e-8f; d->obs_clip = 5.0f;
        it[p].replay.s = (const float *)(base + 0xA000); it[p].replay.a = (const float *)(base + 0xB000);
        it[p].replay.r = (const float *)(base + 0xC000); it[p].replay.t = (const uint8_t *)(base + 0xD000);
        it[p].replay.s2 = (const float *)(base + 0xE000); it[p].replay.capacity = 256;
        it[p].d_batch_idx = (const int32_t *)(base + 0xF000);
        it[p].n_iters = n_iters;
    }
    return it;
}

int main(void) {
    ssc_ddpg_many_item *it;

    EXPECT(ssc_ddpg_train_many(NULL, D_ITEMS, 3, NULL) == SSC_EINVAL);
    it = population(3, 0);
    EXPECT(ssc_ddpg_train_many(it, NULL, 3, NULL) == SSC_EINVAL);
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 0, NULL) == SSC_EINVAL);
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, -1, NULL) == SSC_EINVAL);
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 3, NULL) == SSC_OK);                       /* nothing to launch */
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 1, NULL) == SSC_OK);
    free(it);

    for (int n = 1; n <= 600; n = 3 * n + 1) {                                            /* 1, 4, 13, 40, 121, 364 */
        it = population(n, 0);
        EXPECT(ssc_ddpg_train_many(it, D_ITEMS, n, NULL) == SSC_OK);
        it[n - 1].ddpg.actor_h1 = 128;                                                    /* the LAST item is read */
        EXPECT(ssc_ddpg_train_many(it, D_ITEMS, n, NULL) == SSC_EUNSUPPORTED);
        char want[32];
        snprintf(want, sizeof want, "agent %d", n - 1);
        EXPECT(strstr(ssc_last_error(), want) != NULL);
        it[n - 1].ddpg.actor_h1 = 64;
        if (n > 1) {
            it[n - 1].ddpg.critic = it[0].ddpg.critic;                                    /* first and last on one array */
            EXPECT(ssc_ddpg_train_many(it, D_ITEMS, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "share") != NULL);
            it[n - 1].ddpg.critic = (float *)it[n - 1].ddpg.adam_t;                       /* two arrays of ONE agent */
            EXPECT(ssc_ddpg_train_many(it, D_ITEMS, n, NULL) == SSC_EINVAL);
        }
        free(it);
    }

    it = population(5, 0);
    it[3].ddpg.obs_dim = 3;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EINVAL);
    it[3].ddpg.obs_dim = 2; it[4].ddpg.last_layer_tanh = 0;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EINVAL);
    it[4].ddpg.last_layer_tanh = 7;                                                       /* any non-zero value is "tanh" */
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_OK);
    it[2].d_rms = (const double *)(uintptr_t)0x5000;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EINVAL);
    it[2].d_rms = NULL; it[1].n_iters = -2;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EINVAL);
    it[1].n_iters = 3; it[1].ddpg.adam_t = NULL;                                          /* work to do, an array missing */
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EINVAL);
    it[1].n_iters = 0;                                                                    /* nothing to do: may be missing */
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_OK);
    it[0].ddpg.batch_size = 128;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EUNSUPPORTED);
    it[0].ddpg.batch_size = 64; it[0].ddpg.layer_norm = 1;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EUNSUPPORTED);
    it[0].ddpg.layer_norm = 0; it[0].ddpg.clip_norm = 0.5f;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EUNSUPPORTED);
    it[0].ddpg.clip_norm = 0.0f; it[0].ddpg.critic_l2_reg = 0.01f;
    EXPECT(ssc_ddpg_train_many(it, D_ITEMS, 5, NULL) == SSC_EUNSUPPORTED);
    free(it);

    /* the sampler's keys */
    const ssc_replay_sample_key *const D_KEYS = (const ssc_replay_sample_key *)(uintptr_t)0x70000000u;
    int32_t *const D_IDX = (int32_t *)(uintptr_t)0x60000000u;
    for (int n = 1; n <= 600; n = 3 * n + 1) {
        ssc_replay_sample_key *k = (ssc_replay_sample_key *)malloc((size_t)n * sizeof *k);
        for (int p = 0; p < n; ++p) { k[p].seed = 11u + (uint64_t)p; k[p].counter0 = 100u * (uint64_t)p; k[p].size = 64 + p; }
        EXPECT(ssc_replay_sample_many(k, D_KEYS, n, 0, 64, NULL, NULL) == SSC_OK);        /* nothing to draw */
        EXPECT(ssc_replay_sample_many(k, D_KEYS, n, 3, 64, NULL, NULL) == SSC_EINVAL);    /* d_idx NULL */
        EXPECT(ssc_replay_sample_many(k, D_KEYS, n, 3, 65, D_IDX, NULL) == SSC_EUNSUPPORTED);
        EXPECT(ssc_replay_sample_many(k, D_KEYS, n, 3, 0, D_IDX, NULL) == SSC_EINVAL);
        EXPECT(ssc_replay_sample_many(k, D_KEYS, n, -1, 64, D_IDX, NULL) == SSC_EINVAL);
        k[n - 1].size = 63;                                                               /* the LAST key is read */
        EXPECT(ssc_replay_sample_many(k, D_KEYS, n, 3, 64, D_IDX, NULL) == SSC_EINVAL);
        k[n - 1].size = (int64_t)1 << 31;
        EXPECT(ssc_replay_sample_many(k, D_KEYS, n, 3, 64, D_IDX, NULL) == SSC_EINVAL);
        EXPECT(ssc_replay_sample_many(NULL, D_KEYS, n, 3, 64, D_IDX, NULL) == SSC_EINVAL);
        EXPECT(ssc_replay_sample_many(k, NULL, n, 3, 64, D_IDX, NULL) == SSC_EINVAL);
        EXPECT(ssc_replay_sample_many(k, D_KEYS, 0, 3, 64, D_IDX, NULL) == SSC_EINVAL);
        free(k);
    }

    if (failures == 0) printf("all expectations hold\n");
    return failures == 0 ? 0 : 1;
}
