/* Host-side checks of the weight-EMA entry points (ABI 18) that need no GPU: the version, and the argument
 * validation of vit_adamw_ema and vit_ema_swap, which refuse bad input through VIT_REQUIRE before any launch.  Built by
 * tests/test_ema_cpu.py against the shipped library with gcc, as tests/host_abi_check.c is.
 * Exit status 0 = every check passed; a failed check prints its line. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                           \
  do {                                                                     \
    if (!(c)) {                                                            \
      fprintf(stderr, "host_abi_ema_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                             \
    }                                                                      \
  } while (0)

/* an entry point refused its arguments: VIT_ERR_INVALID and a non-empty message naming it */
static int refused(int rc, const char* name) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, name) != NULL;
}

/* vit_adamw_ema with valid AdamW scalars: only the table, the EMA array, the count and the weight vary */
static int adamw_ema(const vit_tensor_chunk* tab, float* const* ema, int64_t n, float w) {
  return vit_adamw_ema(tab, ema, n, 1e-3f, 0.9f, 0.999f, 1e-8f, 1e-4f, 0.1f, 0.001f, 1.f, VIT_BF16, w, NULL, NULL);
}

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);

  /* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
  vit_tensor_chunk tab[1];
  float* ema[1] = {NULL};
  memset(tab, 0, sizeof(tab));

  CHECK(refused(adamw_ema(NULL, ema, 1, 0.1f), "vit_adamw_ema"));      /* NULL table */
  CHECK(refused(adamw_ema(tab, NULL, 1, 0.1f), "vit_adamw_ema"));      /* NULL EMA array */
  CHECK(refused(adamw_ema(tab, ema, 0, 0.1f), "vit_adamw_ema"));       /* nchunks = 0 */
  CHECK(refused(adamw_ema(tab, ema, -2, 0.1f), "vit_adamw_ema"));
  CHECK(refused(adamw_ema(tab, ema, 1, 0.f), "vit_adamw_ema"));        /* ema_weight outside (0, 1) */
  CHECK(refused(adamw_ema(tab, ema, 1, 1.f), "vit_adamw_ema"));
  CHECK(refused(adamw_ema(tab, ema, 1, -0.5f), "vit_adamw_ema"));
  CHECK(refused(adamw_ema(tab, ema, 1, (float)NAN), "vit_adamw_ema"));  /* NaN */
  CHECK(strstr(vit_last_error(), "ema_weight") != NULL);

  CHECK(refused(vit_ema_swap(NULL, ema, 1, VIT_BF16, NULL), "vit_ema_swap"));
  CHECK(refused(vit_ema_swap(tab, NULL, 1, VIT_BF16, NULL), "vit_ema_swap"));
  CHECK(refused(vit_ema_swap(tab, ema, 0, VIT_F32, NULL), "vit_ema_swap"));
  CHECK(refused(vit_ema_swap(tab, ema, -1, VIT_F32, NULL), "vit_ema_swap"));

  if (fails == 0) printf("host_abi_ema_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
