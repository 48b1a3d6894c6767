/* Host-side sanitizer job for the grouped launches of Pop-Art agents: ssc_ddpg_train_many_popart_plan walks n_agents
 * caller structs, sorts a table of their pointers and fills a caller buffer of ssc_ddpg_train_many_popart_plan_bytes(n_agents)
 * bytes; ssc_ddpg_train_many_popart walks the same structs and reads that buffer back.  Built against the ASan + UBSan host
 * build of libssc (tests/sanitizer/build.py builds the library; tests/test_ddpg_many_popart_sanitizer_host.py this driver) and
 * driven with exactly-sized heap arrays, so a read past item n_agents - 1 or a write past the plan's last byte is a report.
 * Every call of the launching entry point here fails validation or has nothing to launch: no GPU.  Exit code 0 and no
 * sanitizer report = pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ssc.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #cond, ssc_last_error()); ++failures; } } while (0)

static const void *const D_PLAN = (const void *)(uintptr_t)0x70000000u;   /* never read on the host */

/* n valid Pop-Art items (128-64 actor, 200-100 critic, batch 17), every array, workspace and ret_rms block at a made-up
 * address of its own */
static ssc_ddpg_many_popart_item *population(int n, int n_iters) {
    ssc_ddpg_many_popart_item *it = (ssc_ddpg_many_popart_item *)malloc((size_t)n * sizeof *it);
    memset(it, 0, (size_t)n * sizeof *it);
    for (int p = 0; p < n; ++p) {
        ssc_ddpg_desc *d = &it[p].ddpg;
        uintptr_t base = (uintptr_t)0x10000000u * (uintptr_t)(p + 1);
        d->obs_dim = 2; d->act_dim = 1; d->actor_h1 = 128; d->actor_h2 = 64; d->critic_h1 = 200; d->critic_h2 = 100;
        d->last_layer_tanh = 1; d->batch_size = 17;
        d->actor = (float *)(base + 0x100000); d->critic = (float *)(base + 0x200000);
        d->target_actor = (float *)(base + 0x300000); d->target_critic = (float *)(base + 0x400000);
        d->adam_m_actor = (float *)(base + 0x500000); d->adam_v_actor = (float *)(base + 0x600000);
        d->adam_m_critic = (float *)(base + 0x700000); d->adam_v_critic = (float *)(base + 0x800000);
        d->adam_t = (int32_t *)(base + 0x900000);
        d->gamma = 0.99f; d->tau = 0.001f; d->actor_lr = 1e-4f; d->critic_lr = 1e-3f;
        d->beta1 = 0.9f; d->beta2 = 0.999f; d->epsilon = 1e-8f; d->obs_clip = 5.0f;
        if (p % 3 == 1) d->clip_norm = 0.5f;                                              /* the prepared apply group */
        it[p].replay.s = (const float *)(base + 0xA00000); it[p].replay.a = (const float *)(base + 0xA10000);
        it[p].replay.r = (const float *)(base + 0xA20000); it[p].replay.t = (const uint8_t *)(base + 0xA30000);
        it[p].replay.s2 = (const float *)(base + 0xA40000); it[p].replay.capacity = 256;
        it[p].d_batch_idx = (const int32_t *)(base + 0xA50000);
        it[p].d_losses = (float *)(base + 0xA60000);
        if (p % 2 == 1) it[p].d_rms = (const double *)(base + 0xA70000);                  /* the statistics gradient group */
        it[p].n_iters = n_iters;
        it[p].d_workspace = (void *)(base + 0x1000000);
        it[p].workspace_bytes = ssc_ddpg_train_popart_workspace_bytes(d);
        it[p].d_ret_rms = (double *)(base + 0xA80000);
    }
    return it;
}

int main(void) {
    ssc_ddpg_many_popart_item *it;
    unsetenv("SSC_DDPG_WIDE");
    unsetenv("SSC_DDPG_INTERPRETER");

    EXPECT(ssc_ddpg_train_many_popart_plan_bytes(0) == 0 && ssc_ddpg_train_many_popart_plan_bytes(-5) == 0);
    EXPECT(ssc_ddpg_train_many_popart_plan_bytes(33) == 33 * ssc_ddpg_train_many_popart_plan_bytes(1));

    const int sizes[2] = {1, 33};
    for (int k = 0; k < 2; ++k) {
        const int n = sizes[k];
        const size_t bytes = ssc_ddpg_train_many_popart_plan_bytes(n);
        char *plan = (char *)malloc(bytes), *shorter = (char *)malloc(bytes - 1);         /* exact size; one byte short */
        it = population(n, 2);
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, shorter, bytes - 1) == SSC_EINVAL);   /* refused before a byte is written */
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_OK);              /* fills exactly `bytes` */
        EXPECT(ssc_ddpg_train_many_popart_plan(NULL, n, plan, bytes) == SSC_EINVAL);
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, NULL, bytes) == SSC_EINVAL);
        EXPECT(ssc_ddpg_train_many_popart_plan(it, 0, plan, bytes) == SSC_EINVAL);
        EXPECT(ssc_ddpg_train_many_popart(it, plan, NULL, n, NULL) == SSC_EINVAL);
        EXPECT(ssc_ddpg_train_many_popart(it, NULL, D_PLAN, n, NULL) == SSC_EINVAL);
        EXPECT(ssc_ddpg_train_many_popart(NULL, plan, D_PLAN, n, NULL) == SSC_EINVAL);
        it[n - 1].n_iters = 3;                                                            /* the LAST item is read: a stale plan */
        EXPECT(ssc_ddpg_train_many_popart(it, plan, D_PLAN, n, NULL) == SSC_EINVAL && strstr(ssc_last_error(), "plan") != NULL);
        it[n - 1].n_iters = 2;
        it[n - 1].workspace_bytes -= 1;
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_EINVAL && strstr(ssc_last_error(), "workspace") != NULL);
        EXPECT(ssc_ddpg_train_many_popart(it, plan, D_PLAN, n, NULL) == SSC_EINVAL);
        it[n - 1].workspace_bytes += 1;
        it[n - 1].workspace_bytes = ssc_ddpg_train_workspace_bytes(&it[n - 1].ddpg);     /* big enough for the plain step only */
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_EINVAL && strstr(ssc_last_error(), "workspace") != NULL);
        it[n - 1].workspace_bytes = ssc_ddpg_train_popart_workspace_bytes(&it[n - 1].ddpg);
        it[n - 1].d_ret_rms = NULL;                                                       /* a plain agent belongs elsewhere */
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_EINVAL && strstr(ssc_last_error(), "d_ret_rms") != NULL);
        char want[32];
        snprintf(want, sizeof want, "agent %d", n - 1);
        EXPECT(strstr(ssc_last_error(), want) != NULL);
        it[n - 1].d_ret_rms = (double *)(uintptr_t)0x7F000000u;
        it[n - 1].ddpg.actor_h1 = 64; it[n - 1].ddpg.actor_h2 = 32; it[n - 1].ddpg.critic_h1 = 64; it[n - 1].ddpg.critic_h2 = 32;
        it[n - 1].ddpg.batch_size = 64; it[n - 1].ddpg.clip_norm = 0.0f;                  /* the shipped shape is served too */
        it[n - 1].workspace_bytes = ssc_ddpg_train_popart_workspace_bytes(&it[n - 1].ddpg);
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_OK);
        free(it);
        if (n > 1) {
            it = population(n, 2);
            it[n - 1].ddpg.critic = it[0].ddpg.critic;                                    /* first and last on one array */
            EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_EINVAL && strstr(ssc_last_error(), "share") != NULL);
            it[n - 1].ddpg.critic = (float *)it[n - 1].d_workspace;                       /* an array inside ONE agent's workspace slot */
            EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_EINVAL);
            free(it);
            it = population(n, 2);
            it[n - 1].d_ret_rms = it[0].d_ret_rms;                                        /* first and last on one ret_rms block */
            EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_EINVAL && strstr(ssc_last_error(), "ret_rms") != NULL);
            EXPECT(ssc_ddpg_train_many_popart(it, plan, D_PLAN, n, NULL) == SSC_EINVAL);
            free(it);
        }
        /* nothing to do anywhere, one item with every array NULL: planned, and "launched" without a launch */
        it = population(n, 0);
        ssc_ddpg_desc *d = &it[n / 2].ddpg;
        d->actor = d->critic = d->target_actor = d->target_critic = NULL;
        d->adam_m_actor = d->adam_v_actor = d->adam_m_critic = d->adam_v_critic = NULL;
        d->adam_t = NULL;
        it[n / 2].d_batch_idx = NULL; it[n / 2].d_losses = NULL; it[n / 2].d_rms = NULL;
        it[n / 2].d_workspace = NULL; it[n / 2].workspace_bytes = 0; it[n / 2].d_ret_rms = NULL;
        memset(&it[n / 2].replay, 0, sizeof it[n / 2].replay);
        EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_OK);
        EXPECT(ssc_ddpg_train_many_popart(it, plan, D_PLAN, n, NULL) == SSC_OK);
        if (n > 1) {                                                                      /* ... and beside agents that have work */
            for (int p = 0; p < n; ++p) it[p].n_iters = p == n / 2 ? 0 : 1 + p % 4;
            EXPECT(ssc_ddpg_train_many_popart_plan(it, n, plan, bytes) == SSC_OK);
            it[0].n_iters = -1;
            EXPECT(ssc_ddpg_train_many_popart(it, plan, D_PLAN, n, NULL) == SSC_EINVAL);
        }
        free(it);
        free(plan);
        free(shorter);
    }

    if (failures == 0) printf("all expectations hold\n");
    return failures == 0 ? 0 : 1;
}
