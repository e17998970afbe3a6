/* Host-side checks of the label-smoothing / batch-mix entry points that need no GPU: vit_softmax_xent_mixed and
 * vit_mix_batch refuse bad input through VIT_REQUIRE before any launch, with an error string that names the entry
 * point, and adding them left the ABI version at 18 (purely added entry points do not change it, vit_hip.h).  Built by
 * tests/test_batch_mix_cpu.py against the shipped library with gcc, as tests/host_abi_ema_check.c is.
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
      fprintf(stderr, "host_abi_mix_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                             \
    }                                                                      \
  } while (0)

/* an entry point refused its arguments: VIT_ERR_INVALID and a non-empty message naming it */
static int refused(int rc, const char* name) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, name) != NULL;
}

#define XENT "vit_softmax_xent_mixed"
#define MIX "vit_mix_batch"

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(sizeof(vit_mix_item) == 24);

  /* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
  static float buf[64];
  static int64_t lab[4];
  float* f = buf;
  const float eps = 0.1f;

  /* ---- vit_softmax_xent_mixed(logits, labels_a, labels_b, lam, smoothing, rows, classes, loss, dlogits, ws, s) */
  CHECK(refused(vit_softmax_xent_mixed(NULL, lab, lab, f, eps, 4, 4, f, f, f, NULL), XENT));  /* NULL logits */
  CHECK(refused(vit_softmax_xent_mixed(f, NULL, lab, f, eps, 4, 4, f, f, f, NULL), XENT));    /* NULL labels_a */
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, eps, 4, 4, NULL, f, f, NULL), XENT));  /* NULL loss */
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, eps, 4, 4, f, NULL, f, NULL), XENT));  /* NULL dlogits */
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, eps, 4, 4, f, f, NULL, NULL), XENT));  /* NULL workspace */
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, eps, 0, 4, f, f, f, NULL), XENT));     /* rows <= 0 */
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, eps, -3, 4, f, f, f, NULL), XENT));
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, eps, 4, 0, f, f, f, NULL), XENT));     /* classes <= 0 */
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, eps, 4, -1, f, f, f, NULL), XENT));
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, 1.f, 4, 4, f, f, f, NULL), XENT));     /* smoothing */
  CHECK(strstr(vit_last_error(), "smoothing") != NULL);
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, 1.5f, 4, 4, f, f, f, NULL), XENT));
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, -0.1f, 4, 4, f, f, f, NULL), XENT));
  CHECK(refused(vit_softmax_xent_mixed(f, lab, lab, f, (float)NAN, 4, 4, f, f, f, NULL), XENT));
  CHECK(refused(vit_softmax_xent_mixed(f, lab, NULL, f, eps, 4, 4, f, f, f, NULL), XENT));    /* lam, no labels_b */
  CHECK(strstr(vit_last_error(), "labels_b") != NULL);

  /* ---- vit_mix_batch(x, out, dtype, B, C, H, W, items, stream) */
  static char x[4096], out[4096];
  static vit_mix_item items[2];
  CHECK(refused(vit_mix_batch(NULL, out, VIT_F32, 2, 3, 4, 4, items, NULL), MIX));            /* NULL pointers */
  CHECK(refused(vit_mix_batch(x, NULL, VIT_F32, 2, 3, 4, 4, items, NULL), MIX));
  CHECK(refused(vit_mix_batch(x, out, VIT_F32, 2, 3, 4, 4, NULL, NULL), MIX));
  CHECK(refused(vit_mix_batch(x, out, VIT_F32, 0, 3, 4, 4, items, NULL), MIX));               /* dimensions */
  CHECK(refused(vit_mix_batch(x, out, VIT_F32, 2, 0, 4, 4, items, NULL), MIX));
  CHECK(refused(vit_mix_batch(x, out, VIT_F32, 2, 3, -4, 4, items, NULL), MIX));
  CHECK(refused(vit_mix_batch(x, out, VIT_BF16, 2, 3, 4, 0, items, NULL), MIX));
  CHECK(strstr(vit_last_error(), "dimension") != NULL);
  CHECK(refused(vit_mix_batch(x, out, VIT_MASK4, 2, 3, 4, 4, items, NULL), MIX));             /* dtype */
  CHECK(refused(vit_mix_batch(x, out, 7, 2, 3, 4, 4, items, NULL), MIX));
  CHECK(strstr(vit_last_error(), "dtype") != NULL);
  /* out overlapping x: in place, out inside x (one element in, last byte), x inside out */
  CHECK(refused(vit_mix_batch(x, x, VIT_F32, 2, 3, 4, 4, items, NULL), MIX));
  CHECK(strstr(vit_last_error(), "overlap") != NULL);
  CHECK(refused(vit_mix_batch(x, x + 4, VIT_F32, 2, 3, 4, 4, items, NULL), MIX));
  CHECK(refused(vit_mix_batch(x, x + 2 * 3 * 4 * 4 * 4 - 1, VIT_F32, 2, 3, 4, 4, items, NULL), MIX));
  CHECK(refused(vit_mix_batch(x + 2, x, VIT_BF16, 2, 3, 4, 4, items, NULL), MIX));
  CHECK(refused(vit_mix_batch(x + 2 * 3 * 4 * 4 * 2 - 2, x, VIT_BF16, 2, 3, 4, 4, items, NULL), MIX));

  if (fails == 0) printf("host_abi_mix_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
