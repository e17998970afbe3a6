/* Host-side checks of the patch-dropout entry points that need no GPU: vit_patch_keep, vit_im2col_gather,
 * vit_gather_pos, vit_pos_grad_gather and vit_col2im_scatter link, refuse bad input through VIT_REQUIRE before any
 * launch, with an error string that names the entry point, and adding them left the ABI version at 18 (purely added
 * entry points do not change it, vit_hip.h).  Built by tests/test_patch_drop_cpu.py against the shipped library with
 * gcc, as tests/host_abi_drop_path_check.c is.
 * Exit status 0 = every check passed; a failed check prints its line. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "host_abi_patch_drop_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                                          \
    }                                                                                   \
  } while (0)

/* an entry point refused its arguments: VIT_ERR_INVALID and a non-empty message naming it */
static int refused(int rc, const char* name) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, name) != NULL;
}

#define KEEP "vit_patch_keep"
#define I2C "vit_im2col_gather"
#define POS "vit_gather_pos"
#define PGR "vit_pos_grad_gather"
#define C2I "vit_col2im_scatter"

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(VIT_PATCH_KEEP_MAX_N == 4096);

  /* non-null, aligned host addresses: a refused call never reads them, let alone hands them to a kernel */
  static _Alignas(16) int32_t idx[64], inv[64];
  static _Alignas(16) float f[64], g[64];

  /* ---- vit_patch_keep(seed, L, B, N, K, idx, inv, stream) */
  CHECK(refused(vit_patch_keep(1u, 2, 2, 4, 2, NULL, inv, NULL), KEEP));                       /* NULL pointers */
  CHECK(refused(vit_patch_keep(1u, 2, 2, 4, 2, idx, NULL, NULL), KEEP));
  CHECK(strstr(vit_last_error(), "null pointer") != NULL);
  CHECK(refused(vit_patch_keep(1u, 2, 2, 4, 5, idx, inv, NULL), KEEP));                        /* K > N */
  CHECK(strstr(vit_last_error(), "1 <= K <= N <= 4096") != NULL);
  CHECK(refused(vit_patch_keep(1u, 2, 2, 4, 0, idx, inv, NULL), KEEP));                        /* K < 1 */
  CHECK(strstr(vit_last_error(), "1 <= K <= N <= 4096") != NULL);
  CHECK(refused(vit_patch_keep(1u, 2, 2, 4, -1, idx, inv, NULL), KEEP));
  CHECK(refused(vit_patch_keep(1u, 2, 2, 4097, 8, idx, inv, NULL), KEEP));                     /* N > 4096 */
  CHECK(strstr(vit_last_error(), "N=4097") != NULL);
  CHECK(refused(vit_patch_keep(1u, 2, 2, 0, 0, idx, inv, NULL), KEEP));                        /* N < 1 */
  CHECK(refused(vit_patch_keep(1u, 2, 0, 4, 2, idx, inv, NULL), KEEP));                        /* B <= 0 */
  CHECK(refused(vit_patch_keep(1u, 2, -3, 4, 2, idx, inv, NULL), KEEP));
  CHECK(refused(vit_patch_keep(1u, -1, 2, 4, 2, idx, inv, NULL), KEEP));                       /* L < 0 */
  CHECK(refused(vit_patch_keep(1u, 2, (int64_t)1 << 19, 4096, 2, idx, inv, NULL), KEEP));      /* B * N = 2^31 */

  /* ---- vit_im2col_gather(x, x_dtype, cols, dtype, idx, B, C, H, W, P, K, stream): 8 x 8 image, P 4 -> N = 4 */
  CHECK(refused(vit_im2col_gather(NULL, VIT_F32, g, VIT_F32, idx, 1, 1, 8, 8, 4, 2, NULL), I2C));
  CHECK(refused(vit_im2col_gather(f, VIT_F32, NULL, VIT_F32, idx, 1, 1, 8, 8, 4, 2, NULL), I2C));
  CHECK(refused(vit_im2col_gather(f, VIT_F32, g, VIT_F32, NULL, 1, 1, 8, 8, 4, 2, NULL), I2C));
  CHECK(refused(vit_im2col_gather(f, VIT_F32, g, VIT_F32, idx, 1, 1, 8, 8, 4, 5, NULL), I2C));            /* K > N */
  CHECK(refused(vit_im2col_gather(f, VIT_F32, g, VIT_F32, idx, 1, 1, 8, 8, 4, 0, NULL), I2C));            /* K < 1 */
  CHECK(refused(vit_im2col_gather(f, VIT_F32, g, VIT_F32, idx, 1, 1, 260, 260, 4, 8, NULL), I2C));        /* N = 4225 */
  CHECK(refused(vit_im2col_gather(f, VIT_F32, g, VIT_F32, idx, 1, 1, 8, 9, 4, 2, NULL), I2C));            /* W % P */
  CHECK(refused(vit_im2col_gather(f, VIT_F32, g, VIT_F32, idx, 1, 1, 6, 6, 2, 2, NULL), I2C));            /* P % 4 */
  CHECK(refused(vit_im2col_gather(f, VIT_BF16, g, VIT_F32, idx, 1, 1, 8, 8, 4, 2, NULL), I2C));           /* dtype pair */
  CHECK(refused(vit_im2col_gather(f, VIT_F32, g, VIT_F32, idx, 0, 1, 8, 8, 4, 2, NULL), I2C));            /* B <= 0 */

  /* ---- vit_gather_pos(pos, idx, posg, B, N, K, D, stream) */
  CHECK(refused(vit_gather_pos(NULL, idx, g, 2, 4, 2, 8, NULL), POS));
  CHECK(refused(vit_gather_pos(f, NULL, g, 2, 4, 2, 8, NULL), POS));
  CHECK(refused(vit_gather_pos(f, idx, NULL, 2, 4, 2, 8, NULL), POS));
  CHECK(refused(vit_gather_pos(f, idx, g, 2, 4, 5, 8, NULL), POS));                            /* K > N */
  CHECK(refused(vit_gather_pos(f, idx, g, 2, 4, 0, 8, NULL), POS));                            /* K < 1 */
  CHECK(refused(vit_gather_pos(f, idx, g, 2, 4097, 2, 8, NULL), POS));                         /* N > 4096 */
  CHECK(refused(vit_gather_pos(f, idx, g, 2, 4, 2, 6, NULL), POS));                            /* D % 4 */
  CHECK(refused(vit_gather_pos(f, idx, g, 2, 4, 2, 0, NULL), POS));
  CHECK(refused(vit_gather_pos(f + 1, idx, g, 2, 4, 2, 8, NULL), POS));                        /* misaligned rows */

  /* ---- vit_pos_grad_gather(dx, dtype, inv, gpos, B, N, K, D, beta, stream) */
  CHECK(refused(vit_pos_grad_gather(NULL, VIT_F32, inv, g, 2, 4, 2, 8, 0.f, NULL), PGR));
  CHECK(refused(vit_pos_grad_gather(f, VIT_F32, NULL, g, 2, 4, 2, 8, 0.f, NULL), PGR));
  CHECK(refused(vit_pos_grad_gather(f, VIT_F32, inv, NULL, 2, 4, 2, 8, 0.f, NULL), PGR));
  CHECK(refused(vit_pos_grad_gather(f, VIT_F32, inv, g, 2, 4, 5, 8, 0.f, NULL), PGR));         /* K > N */
  CHECK(refused(vit_pos_grad_gather(f, VIT_F32, inv, g, 2, 4, 0, 8, 0.f, NULL), PGR));         /* K < 1 */
  CHECK(refused(vit_pos_grad_gather(f, VIT_F32, inv, g, 2, 4097, 2, 8, 0.f, NULL), PGR));      /* N > 4096 */
  CHECK(refused(vit_pos_grad_gather(f, VIT_F32, inv, g, 2, 4, 2, 7, 0.f, NULL), PGR));         /* D % 4 */
  CHECK(refused(vit_pos_grad_gather(f, VIT_F32, inv, g + 1, 2, 4, 2, 8, 1.f, NULL), PGR));     /* misaligned gpos */
  CHECK(refused(vit_pos_grad_gather(f, VIT_MASK4, inv, g, 2, 4, 2, 8, 0.f, NULL), PGR));       /* dtype */

  /* ---- vit_col2im_scatter(cols, dtype, inv, x, x_dtype, B, C, H, W, P, K, stream) */
  CHECK(refused(vit_col2im_scatter(NULL, VIT_F32, inv, g, VIT_F32, 1, 1, 8, 8, 4, 2, NULL), C2I));
  CHECK(refused(vit_col2im_scatter(f, VIT_F32, NULL, g, VIT_F32, 1, 1, 8, 8, 4, 2, NULL), C2I));
  CHECK(refused(vit_col2im_scatter(f, VIT_F32, inv, NULL, VIT_F32, 1, 1, 8, 8, 4, 2, NULL), C2I));
  CHECK(refused(vit_col2im_scatter(f, VIT_F32, inv, g, VIT_F32, 1, 1, 8, 8, 4, 5, NULL), C2I));           /* K > N */
  CHECK(refused(vit_col2im_scatter(f, VIT_F32, inv, g, VIT_F32, 1, 1, 8, 8, 4, 0, NULL), C2I));           /* K < 1 */
  CHECK(refused(vit_col2im_scatter(f, VIT_F32, inv, g, VIT_F32, 1, 1, 260, 260, 4, 8, NULL), C2I));       /* N = 4225 */
  CHECK(refused(vit_col2im_scatter(f, VIT_F32, inv, g, VIT_F32, 1, 1, 8, 10, 4, 2, NULL), C2I));          /* W % P */
  CHECK(refused(vit_col2im_scatter(f, VIT_F32, inv, g, VIT_BF16, 1, 1, 8, 8, 4, 2, NULL), C2I));          /* dtype pair */

  if (fails == 0) printf("host_abi_patch_drop_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
