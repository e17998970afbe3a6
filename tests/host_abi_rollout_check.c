/* Host-side checks of the attention-rollout entry points (purely added under ABI 18) that need no GPU: the version,
 * the constants, the workspace size, and the argument validation, which refuses bad input through VIT_REQUIRE before
 * any launch.  Built by tests/test_attention_rollout_cpu.py against the shipped library with gcc, as
 * tests/host_abi_eval_check.c is.  Exit status 0 = every check passed; a failed check prints its line. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "host_abi_rollout_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                                 \
    }                                                                          \
  } while (0)

/* the entry point refused its arguments: VIT_ERR_INVALID and a message naming it */
static int refused(int rc) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, "vit_attn_rollout_step") != NULL;
}

/* non-null, 16-B aligned host addresses: a refused call never reads them, let alone hands them to a kernel */
static _Alignas(16) float qkv[64], r_in[64], r_out[64], ws[64];

/* a valid call but for the arguments given */
static int sized(int64_t B, int64_t T, int64_t H, int64_t hd, int32_t dtype, int32_t fuse) {
  return vit_attn_rollout_step(qkv, r_in, r_out, B, T, H, hd, 1.0f, dtype, fuse, ws, NULL);
}

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(VIT_ROLLOUT_MEAN == 0 && VIT_ROLLOUT_MAX == 1 && VIT_ROLLOUT_MIN == 2);

  /* the workspace grows with B and with T, and is 0 for a shape that the step refuses */
  const int64_t w = vit_attn_rollout_workspace_bytes(2, 197, 12, 64, VIT_BF16, VIT_ROLLOUT_MEAN);
  CHECK(w > 0);
  CHECK(vit_attn_rollout_workspace_bytes(4, 197, 12, 64, VIT_BF16, VIT_ROLLOUT_MEAN) > w);
  CHECK(vit_attn_rollout_workspace_bytes(2, 577, 12, 64, VIT_BF16, VIT_ROLLOUT_MEAN) > w);
  CHECK(vit_attn_rollout_workspace_bytes(2, 198, 12, 64, VIT_BF16, VIT_ROLLOUT_MEAN) > w);
  CHECK(vit_attn_rollout_workspace_bytes(1, 1, 1, 4, VIT_F32, VIT_ROLLOUT_MIN) > 0);
  CHECK(vit_attn_rollout_workspace_bytes(2, 1025, 12, 64, VIT_BF16, VIT_ROLLOUT_MEAN) == 0);
  CHECK(vit_attn_rollout_workspace_bytes(2, 197, 12, 64, VIT_BF16, 3) == 0);
  CHECK(vit_attn_rollout_workspace_bytes(0, 197, 12, 64, VIT_BF16, 0) == 0);

  CHECK(refused(sized(2, 4, 2, 0, VIT_BF16, 0)));        /* hd out of range */
  CHECK(refused(sized(2, 4, 2, 132, VIT_BF16, 0)));
  CHECK(refused(sized(2, 4, 2, 132, VIT_F32, 0)));
  CHECK(refused(sized(2, 4, 2, 66, VIT_BF16, 0)));       /* hd % 4 != 0 */
  CHECK(refused(sized(2, 4, 2, -64, VIT_BF16, 0)));
  CHECK(refused(sized(2, 1025, 2, 64, VIT_BF16, 0)));    /* T beyond the limit */
  CHECK(refused(sized(2, 0, 2, 64, VIT_BF16, 0)));
  CHECK(refused(sized(2, (int64_t)1 << 33, 2, 64, VIT_F32, 0)));
  CHECK(refused(sized(2, 4, 2, 64, VIT_BF16, 3)));       /* fuse out of range */
  CHECK(refused(sized(2, 4, 2, 64, VIT_BF16, -1)));
  CHECK(refused(sized(2, 4, 2, 64, VIT_MASK4, 0)));      /* dtype */
  CHECK(refused(sized(0, 4, 2, 64, VIT_BF16, 0)));       /* B, H <= 0 */
  CHECK(refused(sized(2, 4, 0, 64, VIT_BF16, 0)));
  CHECK(refused(sized((int64_t)1 << 40, 1024, 2, 64, VIT_BF16, 0)));   /* the grid does not fit */

  /* r_in == r_out, or overlapping */
  CHECK(refused(vit_attn_rollout_step(qkv, r_in, r_in, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, ws, NULL)));
  CHECK(refused(vit_attn_rollout_step(qkv, r_in, r_in + 4, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, ws, NULL)));
  /* a NULL among the required pointers */
  CHECK(refused(vit_attn_rollout_step(NULL, r_in, r_out, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, ws, NULL)));
  CHECK(refused(vit_attn_rollout_step(qkv, NULL, r_out, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, ws, NULL)));
  CHECK(refused(vit_attn_rollout_step(qkv, r_in, NULL, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, ws, NULL)));
  CHECK(refused(vit_attn_rollout_step(qkv, r_in, r_out, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, NULL, NULL)));
  /* qkv not 16-B aligned */
  CHECK(refused(vit_attn_rollout_step(qkv + 1, r_in, r_out, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, ws, NULL)));
  /* the form: outside 0..2, or the MFMA form where it does not apply */
  CHECK(refused(vit_attn_rollout_step_form(qkv, r_in, r_out, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, 3, ws, NULL)));
  CHECK(refused(vit_attn_rollout_step_form(qkv, r_in, r_out, 2, 4, 2, 64, 1.0f, VIT_BF16, 0, -1, ws, NULL)));
  CHECK(refused(vit_attn_rollout_step_form(qkv, r_in, r_out, 2, 4, 2, 32, 1.0f, VIT_BF16, 0, 2, ws, NULL)));
  CHECK(refused(vit_attn_rollout_step_form(qkv, r_in, r_out, 2, 4, 2, 64, 1.0f, VIT_F32, 0, 2, ws, NULL)));

  if (fails == 0) printf("host_abi_rollout_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
