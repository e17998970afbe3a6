/* Host-side checks of the grouped optimizer entry points (purely added under ABI 18) that need no GPU: the version,
 * the size of vit_opt_group, and the argument validation of vit_adamw_groups, vit_lamb_moments_groups,
 * vit_lamb_trust_groups and vit_lamb_update_groups, which refuse bad input through VIT_REQUIRE before any launch.
 * Built by tests/test_lr_schedule_cpu.py against the shipped library with gcc, as tests/host_abi_lamb_check.c is.
 * Exit status 0 = every check passed; a failed check prints its line. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      fprintf(stderr, "host_abi_groups_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                                \
    }                                                                         \
  } while (0)

/* an entry point refused its arguments: VIT_ERR_INVALID and a non-empty message naming it */
static int refused(int rc, const char* name) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, name) != NULL;
}

/* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
static vit_tensor_chunk tab[1];
static double partial[2];
static int32_t first[2] = {0, 1}, owner[1], of_chunk[1], of_tensor[1];
static float trust[1] = {1.f};

static int adamw(const vit_tensor_chunk* t, const int32_t* goc, int64_t n, const vit_opt_group* g, int32_t ng) {
  return vit_adamw_groups(t, NULL, goc, n, g, ng, 1.f, VIT_BF16, 0.f, NULL, NULL);
}
static int moments(const vit_tensor_chunk* t, const int32_t* goc, double* part, int64_t n, const vit_opt_group* g,
                   int32_t ng) {
  return vit_lamb_moments_groups(t, goc, n, g, ng, 1.f, NULL, part, NULL);
}
static int trustp(const double* part, const int32_t* fi, const int32_t* got, float* tr, int64_t n,
                  const vit_opt_group* g, int32_t ng) {
  return vit_lamb_trust_groups(part, fi, got, n, g, ng, tr, NULL, NULL);
}
static int update(const vit_tensor_chunk* t, const int32_t* ow, const float* tr, const int32_t* goc, int64_t n,
                  const vit_opt_group* g, int32_t ng) {
  return vit_lamb_update_groups(t, NULL, ow, tr, goc, n, g, ng, VIT_BF16, 0.f, NULL, NULL);
}

/* the groups `g` are refused by the AdamW entry point and, with `lamb_too`, by the three LAMB ones as well */
static void all_refuse(const vit_opt_group* g, int32_t ng, int lamb_too) {
  CHECK(refused(adamw(tab, of_chunk, 1, g, ng), "vit_adamw_groups"));
  if (!lamb_too) return;
  CHECK(refused(moments(tab, of_chunk, partial, 1, g, ng), "vit_lamb_moments_groups"));
  CHECK(refused(trustp(partial, first, of_tensor, trust, 1, g, ng), "vit_lamb_trust_groups"));
  CHECK(refused(update(tab, owner, trust, of_chunk, 1, g, ng), "vit_lamb_update_groups"));
}

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(sizeof(vit_opt_group) == 32);
  CHECK(VIT_OPT_MAX_GROUPS == 64 && VIT_OPT_ADAPT == 1 && VIT_OPT_TRUST_CLIP == 2);

  vit_opt_group good[VIT_OPT_MAX_GROUPS + 1], g[3];
  float* ema[1] = {NULL};
  const float nan_f = (float)NAN, inf_f = (float)INFINITY;
  memset(tab, 0, sizeof(tab));
  for (int i = 0; i <= VIT_OPT_MAX_GROUPS; ++i) {
    const vit_opt_group one = {1e-3f, 0.9f, 0.999f, 1e-6f, 0.01f, 0.1f, 0.001f, 0};
    good[i] = one;
  }

  /* NULL pointers */
  CHECK(refused(adamw(NULL, of_chunk, 1, good, 2), "vit_adamw_groups"));
  CHECK(refused(adamw(tab, NULL, 1, good, 2), "vit_adamw_groups"));
  CHECK(refused(adamw(tab, of_chunk, 1, NULL, 2), "vit_adamw_groups"));
  CHECK(refused(moments(NULL, of_chunk, partial, 1, good, 2), "vit_lamb_moments_groups"));
  CHECK(refused(moments(tab, NULL, partial, 1, good, 2), "vit_lamb_moments_groups"));
  CHECK(refused(moments(tab, of_chunk, NULL, 1, good, 2), "vit_lamb_moments_groups"));
  CHECK(refused(moments(tab, of_chunk, partial, 1, NULL, 2), "vit_lamb_moments_groups"));
  CHECK(refused(trustp(NULL, first, of_tensor, trust, 1, good, 2), "vit_lamb_trust_groups"));
  CHECK(refused(trustp(partial, NULL, of_tensor, trust, 1, good, 2), "vit_lamb_trust_groups"));
  CHECK(refused(trustp(partial, first, NULL, trust, 1, good, 2), "vit_lamb_trust_groups"));
  CHECK(refused(trustp(partial, first, of_tensor, NULL, 1, good, 2), "vit_lamb_trust_groups"));
  CHECK(refused(trustp(partial, first, of_tensor, trust, 1, NULL, 2), "vit_lamb_trust_groups"));
  CHECK(refused(update(NULL, owner, trust, of_chunk, 1, good, 2), "vit_lamb_update_groups"));
  CHECK(refused(update(tab, NULL, trust, of_chunk, 1, good, 2), "vit_lamb_update_groups"));
  CHECK(refused(update(tab, owner, NULL, of_chunk, 1, good, 2), "vit_lamb_update_groups"));
  CHECK(refused(update(tab, owner, trust, NULL, 1, good, 2), "vit_lamb_update_groups"));
  CHECK(refused(update(tab, owner, trust, of_chunk, 1, NULL, 2), "vit_lamb_update_groups"));

  /* counts <= 0 */
  CHECK(refused(adamw(tab, of_chunk, 0, good, 2), "vit_adamw_groups"));
  CHECK(refused(adamw(tab, of_chunk, -2, good, 2), "vit_adamw_groups"));
  CHECK(refused(moments(tab, of_chunk, partial, 0, good, 2), "vit_lamb_moments_groups"));
  CHECK(refused(trustp(partial, first, of_tensor, trust, 0, good, 2), "vit_lamb_trust_groups"));
  CHECK(refused(update(tab, owner, trust, of_chunk, -1, good, 2), "vit_lamb_update_groups"));

  /* ngroups outside 1..64 */
  all_refuse(good, 0, 1);
  CHECK(strstr(vit_last_error(), "ngroups") != NULL);
  all_refuse(good, VIT_OPT_MAX_GROUPS + 1, 1);
  all_refuse(good, -1, 1);

  /* one bad group behind two good ones: bias corrections outside (0, 1], negative eps, an lr that is not finite */
  const float bad_bc[] = {0.f, -0.1f, 1.001f, nan_f};
  for (unsigned k = 0; k < sizeof(bad_bc) / sizeof(bad_bc[0]); ++k) {
    g[0] = g[1] = g[2] = good[0];
    g[2].bias_corr1 = bad_bc[k];
    all_refuse(g, 3, 1);
    CHECK(strstr(vit_last_error(), "bias corrections") != NULL);
    g[2] = good[0];
    g[1].bias_corr2 = bad_bc[k];
    all_refuse(g, 3, 1);
  }
  g[0] = g[1] = g[2] = good[0];
  g[2].eps = -1e-8f;
  all_refuse(g, 3, 1);
  CHECK(strstr(vit_last_error(), "eps") != NULL);
  g[2].eps = nan_f;
  all_refuse(g, 3, 1);
  g[2] = good[0];
  g[0].lr = inf_f;
  all_refuse(g, 3, 1);
  CHECK(strstr(vit_last_error(), "lr") != NULL);
  g[0].lr = nan_f;
  all_refuse(g, 3, 1);
  g[0] = good[0];

  /* flags: none for AdamW, only the two known ones for LAMB */
  g[1].flags = VIT_OPT_ADAPT;
  all_refuse(g, 3, 0);
  CHECK(strstr(vit_last_error(), "flags") != NULL);
  g[1].flags = VIT_OPT_TRUST_CLIP;
  all_refuse(g, 3, 0);
  g[1].flags = 4;
  all_refuse(g, 3, 1);
  g[1].flags = 0;

  /* with an EMA array the weight must lie in (0, 1) */
  CHECK(refused(vit_adamw_groups(tab, ema, of_chunk, 1, good, 2, 1.f, VIT_BF16, 0.f, NULL, NULL), "vit_adamw_groups"));
  CHECK(strstr(vit_last_error(), "ema_weight") != NULL);
  CHECK(refused(vit_adamw_groups(tab, ema, of_chunk, 1, good, 2, 1.f, VIT_BF16, 1.f, NULL, NULL), "vit_adamw_groups"));
  CHECK(refused(vit_lamb_update_groups(tab, ema, owner, trust, of_chunk, 1, good, 2, VIT_BF16, 0.f, NULL, NULL),
                "vit_lamb_update_groups"));

  if (fails == 0) printf("host_abi_groups_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
