/* Host-side checks of the LAMB entry points (purely added under ABI 18) that need no GPU: the version, and the
 * argument validation of vit_lamb_moments, vit_lamb_trust and vit_lamb_update, which refuse bad input through
 * VIT_REQUIRE before any launch.  Built by tests/test_lamb_cpu.py against the shipped library with gcc, as
 * tests/host_abi_ema_check.c is.  Exit status 0 = every check passed; a failed check prints its line. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "host_abi_lamb_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                              \
    }                                                                       \
  } while (0)

/* an entry point refused its arguments: VIT_ERR_INVALID and a non-empty message naming it */
static int refused(int rc, const char* name) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, name) != NULL;
}

/* valid LAMB scalars: only the pointers, the count and the bias corrections vary */
static int moments(const vit_tensor_chunk* tab, double* partial, int64_t n, float bc1, float bc2) {
  return vit_lamb_moments(tab, n, 0.9f, 0.999f, 1e-6f, 0.01f, bc1, bc2, 1.f, NULL, partial, NULL);
}

static int update(const vit_tensor_chunk* tab, const int32_t* owner, const float* trust, int64_t n, float bc1,
                  float bc2) {
  return vit_lamb_update(tab, NULL, owner, trust, n, 1e-3f, 1e-6f, 0.01f, bc1, bc2, VIT_BF16, 0.f, NULL, NULL);
}

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);

  /* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
  vit_tensor_chunk tab[1];
  double partial[2] = {0.0, 0.0};
  int32_t first[2] = {0, 1}, owner[1] = {0};
  float trust[1] = {1.f};
  float* ema[1] = {NULL};
  const float nan_f = (float)NAN;
  memset(tab, 0, sizeof(tab));

  CHECK(refused(moments(NULL, partial, 1, 0.1f, 0.001f), "vit_lamb_moments"));      /* NULL table */
  CHECK(refused(moments(tab, NULL, 1, 0.1f, 0.001f), "vit_lamb_moments"));          /* NULL partials */
  CHECK(refused(moments(tab, partial, 0, 0.1f, 0.001f), "vit_lamb_moments"));       /* nchunks <= 0 */
  CHECK(refused(moments(tab, partial, -3, 0.1f, 0.001f), "vit_lamb_moments"));
  CHECK(refused(moments(tab, partial, 1, 0.f, 0.001f), "vit_lamb_moments"));        /* bias corrections outside (0, 1] */
  CHECK(strstr(vit_last_error(), "bias corrections") != NULL);
  CHECK(refused(moments(tab, partial, 1, 1.5f, 0.001f), "vit_lamb_moments"));
  CHECK(refused(moments(tab, partial, 1, -0.1f, 0.001f), "vit_lamb_moments"));
  CHECK(refused(moments(tab, partial, 1, nan_f, 0.001f), "vit_lamb_moments"));
  CHECK(refused(moments(tab, partial, 1, 0.1f, 0.f), "vit_lamb_moments"));
  CHECK(refused(moments(tab, partial, 1, 0.1f, 1.001f), "vit_lamb_moments"));
  CHECK(refused(moments(tab, partial, 1, 0.1f, nan_f), "vit_lamb_moments"));

  CHECK(refused(vit_lamb_trust(NULL, first, 1, 1, 0, trust, NULL, NULL), "vit_lamb_trust"));    /* NULL partials */
  CHECK(refused(vit_lamb_trust(partial, NULL, 1, 1, 0, trust, NULL, NULL), "vit_lamb_trust"));  /* NULL tensor index */
  CHECK(refused(vit_lamb_trust(partial, first, 1, 1, 0, NULL, NULL, NULL), "vit_lamb_trust"));  /* NULL trust */
  CHECK(refused(vit_lamb_trust(partial, first, 0, 1, 0, trust, NULL, NULL), "vit_lamb_trust")); /* ntensors <= 0 */
  CHECK(refused(vit_lamb_trust(partial, first, -1, 1, 0, trust, NULL, NULL), "vit_lamb_trust"));

  CHECK(refused(update(NULL, owner, trust, 1, 0.1f, 0.001f), "vit_lamb_update"));   /* NULL table */
  CHECK(refused(update(tab, NULL, trust, 1, 0.1f, 0.001f), "vit_lamb_update"));     /* NULL chunk-to-tensor map */
  CHECK(refused(update(tab, owner, NULL, 1, 0.1f, 0.001f), "vit_lamb_update"));     /* NULL trust */
  CHECK(refused(update(tab, owner, trust, 0, 0.1f, 0.001f), "vit_lamb_update"));    /* nchunks <= 0 */
  CHECK(refused(update(tab, owner, trust, -1, 0.1f, 0.001f), "vit_lamb_update"));
  CHECK(refused(update(tab, owner, trust, 1, 0.f, 0.001f), "vit_lamb_update"));     /* bias corrections */
  CHECK(refused(update(tab, owner, trust, 1, 2.f, 0.001f), "vit_lamb_update"));
  CHECK(refused(update(tab, owner, trust, 1, 0.1f, 0.f), "vit_lamb_update"));
  CHECK(refused(update(tab, owner, trust, 1, 0.1f, nan_f), "vit_lamb_update"));
  /* with an EMA array the weight must lie in (0, 1) */
  CHECK(refused(vit_lamb_update(tab, ema, owner, trust, 1, 1e-3f, 1e-6f, 0.01f, 0.1f, 0.001f, VIT_BF16, 0.f, NULL, NULL),
                "vit_lamb_update"));
  CHECK(strstr(vit_last_error(), "ema_weight") != NULL);
  CHECK(refused(vit_lamb_update(tab, ema, owner, trust, 1, 1e-3f, 1e-6f, 0.01f, 0.1f, 0.001f, VIT_BF16, 1.f, NULL, NULL),
                "vit_lamb_update"));

  if (fails == 0) printf("host_abi_lamb_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
