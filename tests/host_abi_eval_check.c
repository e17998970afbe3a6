/* Host-side checks of vit_eval_update (purely added under ABI 18) that need no GPU: the version, and the argument
 * validation, which refuses bad input through VIT_REQUIRE before any launch.  Built by tests/test_eval_metrics_cpu.py
 * against the shipped library with gcc, as tests/host_abi_lamb_check.c is.  Exit status 0 = every check passed; a
 * failed check prints its line. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "host_abi_eval_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                              \
    }                                                                       \
  } while (0)

/* the entry point refused its arguments: VIT_ERR_INVALID and a message naming it */
static int refused(int rc) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, "vit_eval_update") != NULL;
}

/* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
static float logits[16];
static int64_t labels[4], pred[4], counts[2 + VIT_EVAL_MAXK], confusion[16];
static int32_t rank[4];
static float row_loss[4];
static double loss_sum[1];

/* a valid call of 4 rows x 4 classes but for the sizes given */
static int sized(int64_t ld, int64_t rows, int64_t classes, int32_t maxk) {
  return vit_eval_update(logits, ld, labels, rows, classes, maxk, pred, rank, row_loss, counts, loss_sum, confusion,
                         NULL);
}

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(VIT_EVAL_MAXK == 16);

  /* a NULL among the seven required pointers (confusion may be NULL, which a refusal cannot show without a launch) */
  CHECK(refused(vit_eval_update(NULL, 4, labels, 4, 4, 1, pred, rank, row_loss, counts, loss_sum, confusion, NULL)));
  CHECK(refused(vit_eval_update(logits, 4, NULL, 4, 4, 1, pred, rank, row_loss, counts, loss_sum, confusion, NULL)));
  CHECK(refused(vit_eval_update(logits, 4, labels, 4, 4, 1, NULL, rank, row_loss, counts, loss_sum, confusion, NULL)));
  CHECK(refused(vit_eval_update(logits, 4, labels, 4, 4, 1, pred, NULL, row_loss, counts, loss_sum, confusion, NULL)));
  CHECK(refused(vit_eval_update(logits, 4, labels, 4, 4, 1, pred, rank, NULL, counts, loss_sum, confusion, NULL)));
  CHECK(refused(vit_eval_update(logits, 4, labels, 4, 4, 1, pred, rank, row_loss, NULL, loss_sum, confusion, NULL)));
  CHECK(refused(vit_eval_update(logits, 4, labels, 4, 4, 1, pred, rank, row_loss, counts, NULL, confusion, NULL)));
  CHECK(refused(vit_eval_update(logits, 4, labels, 4, 4, 1, pred, rank, row_loss, counts, NULL, NULL, NULL)));

  CHECK(refused(sized(4, 0, 4, 1)));                     /* rows <= 0 */
  CHECK(refused(sized(4, -2, 4, 1)));
  CHECK(refused(sized(4, 4, 0, 1)));                     /* classes <= 0 */
  CHECK(refused(sized(4, 4, -1, 1)));
  CHECK(refused(sized(3, 4, 4, 1)));                     /* ld < classes */
  CHECK(refused(sized(0, 4, 4, 1)));
  CHECK(refused(sized(-4, 4, 4, 1)));
  CHECK(refused(sized(4, 4, 4, 0)));                     /* maxk outside [1, min(classes, VIT_EVAL_MAXK)] */
  CHECK(refused(sized(4, 4, 4, -1)));
  CHECK(refused(sized(4, 4, 4, 5)));                     /* above classes */
  CHECK(refused(sized(64, 4, 64, VIT_EVAL_MAXK + 1)));   /* above VIT_EVAL_MAXK */
  CHECK(refused(sized(1, 4, 1, 2)));
  CHECK(refused(sized(4, (int64_t)INT32_MAX + 1, 4, 1)));                       /* rows above INT32_MAX */
  CHECK(refused(sized((int64_t)INT32_MAX + 1, 4, (int64_t)INT32_MAX + 1, 1)));  /* classes above INT32_MAX */
  CHECK(refused(sized((int64_t)1 << 40, 4, (int64_t)1 << 40, 16)));

  if (fails == 0) printf("host_abi_eval_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
