/* Host-side checks of the knowledge-distillation entry point that need no GPU: vit_softmax_xent_distill has the
 * prototype of vit_hip.h, the two kinds are 0 and 1, every bad argument is refused through VIT_REQUIRE before any
 * launch with an error string that names the entry point, and adding it left the ABI version at 18 (purely added
 * entry points do not change it, vit_hip.h).  Built by tests/test_distill_cpu.py against the shipped library with
 * gcc, as tests/host_abi_mix_check.c is.  Exit status 0 = every check passed; a failed check prints its line. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "host_abi_distill_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                                 \
    }                                                                          \
  } while (0)

/* the entry point refused its arguments: VIT_ERR_INVALID and a message naming it and, where given, the argument */
static int refused(int rc, const char* word) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, "vit_softmax_xent_distill") != NULL &&
         (word == NULL || strstr(e, word) != NULL);
}

/* the prototype, as a function pointer type: a mismatch with the header is a compile error under -Werror or a warning */
typedef int (*distill_fn)(const float*, const float*, const int64_t*, const int64_t*, const float*, float, int32_t,
                          float, float, int64_t, int64_t, float*, float*, float*, void*);

int main(void) {
  distill_fn fn = vit_softmax_xent_distill;
  CHECK(fn != NULL);
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(VIT_DISTILL_SOFT == 0 && VIT_DISTILL_HARD == 1);

  /* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
  static float buf[64];
  static int64_t lab[4];
  float* f = buf;
  const float eps = 0.1f, al = 0.5f, tau = 2.0f;
  const int32_t S = VIT_DISTILL_SOFT, H = VIT_DISTILL_HARD;

  /* (logits, teacher, labels_a, labels_b, lam, smoothing, kind, alpha, tau, rows, classes, loss, dlogits, ws, s) */
  CHECK(refused(fn(NULL, f, lab, lab, f, eps, S, al, tau, 4, 4, f, f, f, NULL), "null"));   /* NULL logits */
  CHECK(refused(fn(f, NULL, lab, lab, f, eps, S, al, tau, 4, 4, f, f, f, NULL), "null"));   /* NULL teacher */
  CHECK(refused(fn(f, f, NULL, lab, f, eps, H, al, tau, 4, 4, f, f, f, NULL), "null"));     /* NULL labels_a */
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, tau, 4, 4, NULL, f, f, NULL), "null"));   /* NULL loss */
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, tau, 4, 4, f, NULL, f, NULL), "null"));   /* NULL dlogits */
  CHECK(refused(fn(f, f, lab, lab, f, eps, H, al, tau, 4, 4, f, f, NULL, NULL), "null"));   /* NULL workspace */
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, tau, 0, 4, f, f, f, NULL), "rows"));      /* rows <= 0 */
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, tau, -3, 4, f, f, f, NULL), "rows"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, tau, 4, 0, f, f, f, NULL), "classes"));   /* classes <= 0 */
  CHECK(refused(fn(f, f, lab, lab, f, eps, H, al, tau, 4, -1, f, f, f, NULL), "classes"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, tau, (int64_t)1 << 31, 4, f, f, f, NULL), "too many rows"));
  CHECK(refused(fn(f, f, lab, lab, f, 1.f, S, al, tau, 4, 4, f, f, f, NULL), "smoothing"));  /* smoothing */
  CHECK(refused(fn(f, f, lab, lab, f, 1.5f, S, al, tau, 4, 4, f, f, f, NULL), "smoothing"));
  CHECK(refused(fn(f, f, lab, lab, f, -0.1f, H, al, tau, 4, 4, f, f, f, NULL), "smoothing"));
  CHECK(refused(fn(f, f, lab, lab, f, (float)NAN, S, al, tau, 4, 4, f, f, f, NULL), "smoothing"));
  CHECK(refused(fn(f, f, lab, NULL, f, eps, S, al, tau, 4, 4, f, f, f, NULL), "labels_b"));  /* lam, no labels_b */
  CHECK(refused(fn(f, f, lab, lab, f, eps, 2, al, tau, 4, 4, f, f, f, NULL), "kind"));       /* kind */
  CHECK(refused(fn(f, f, lab, lab, f, eps, -1, al, tau, 4, 4, f, f, f, NULL), "kind"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, -0.01f, tau, 4, 4, f, f, f, NULL), "alpha"));  /* alpha */
  CHECK(refused(fn(f, f, lab, lab, f, eps, H, 1.01f, tau, 4, 4, f, f, f, NULL), "alpha"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, (float)NAN, tau, 4, 4, f, f, f, NULL), "alpha"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, 0.f, 4, 4, f, f, f, NULL), "tau"));        /* tau */
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, -1.f, 4, 4, f, f, f, NULL), "tau"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, (float)INFINITY, 4, 4, f, f, f, NULL), "tau"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, S, al, (float)NAN, 4, 4, f, f, f, NULL), "tau"));
  CHECK(refused(fn(f, f, lab, lab, f, eps, H, al, 0.f, 4, 4, f, f, f, NULL), "tau"));        /* checked for hard too */

  if (fails == 0) printf("host_abi_distill_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
