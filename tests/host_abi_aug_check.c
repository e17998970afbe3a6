/* Host-side checks of the training-augmentation entry points that need no GPU: vit_augment_to_tensor refuses bad
 * input through VIT_REQUIRE before any launch, with an error string that names it; vit_augment_workspace_bytes is
 * monotone; sizeof(vit_aug_item) is what the header states; and adding them left the ABI version at 18.  Built by
 * tests/test_augment_cpu.py against the shipped library with gcc, as tests/host_abi_mix_check.c is.
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
      fprintf(stderr, "host_abi_aug_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                             \
    }                                                                      \
  } while (0)

#define AUG "vit_augment_to_tensor"

/* an entry point refused its arguments: VIT_ERR_INVALID and a message naming it */
static int refused(int rc) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, AUG) != NULL;
}

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(sizeof(vit_aug_item) == 36);
  CHECK(VIT_AUG_TILE_ROWS == 16 && VIT_AUG_TILE_COLS == 64 && VIT_AUG_TILE_MAX_SPAN == 80);

  /* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
  static char src[64], out[64], ws[64];
  static int64_t meta[8];
  static vit_aug_item items[2];
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  const int64_t B = 2, S = 8, KS = 3;
  const int64_t big = vit_augment_workspace_bytes(B, S, S, KS);

  /* ---- vit_augment_workspace_bytes: the tables of vit_resize_to_tensor, monotone in every argument */
  CHECK(big == vit_resize_workspace_bytes(B, S, S, KS) && big > 0);
  CHECK(vit_augment_workspace_bytes(B + 1, S, S, KS) > big);
  CHECK(vit_augment_workspace_bytes(B, S + 1, S, KS) > big);
  CHECK(vit_augment_workspace_bytes(B, S, S + 1, KS) > big);
  CHECK(vit_augment_workspace_bytes(B, S, S, KS + 2) > big);

  /* ---- vit_augment_to_tensor(src, meta, items, B, oh, ow, ks, mean3, std3, erase, out, dtype, ws, ws_bytes, s):
   * every call below is refused before any launch, so the workspace size given never matters but in its own check */
  CHECK(refused(vit_augment_to_tensor(NULL, meta, items, B, S, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, NULL, items, B, S, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, NULL, B, S, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, NULL, NULL, 0.f, NULL, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, NULL, NULL, 0.f, out, VIT_F32, NULL, big, NULL)));
  /* only one of mean3 / std3 */
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, mean, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, NULL, sd, 0.f, out, VIT_F32, ws, big, NULL)));
  /* a zero or non-finite std, a non-finite mean */
  for (int c = 0; c < 3; ++c) {
    const float bad[3] = {0.f, (float)INFINITY, (float)NAN};
    for (int k = 0; k < 3; ++k) {
      float s2[3] = {sd[0], sd[1], sd[2]};
      s2[c] = bad[k];
      CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, mean, s2, 0.f, out, VIT_F32, ws, big, NULL)));
      CHECK(strstr(vit_last_error(), "std") != NULL);
    }
    float m2[3] = {mean[0], mean[1], mean[2]};
    m2[c] = (float)NAN;
    CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, m2, sd, 0.f, out, VIT_F32, ws, big, NULL)));
    m2[c] = -(float)INFINITY;
    CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, m2, sd, 0.f, out, VIT_F32, ws, big, NULL)));
  }
  /* a non-finite erase_value */
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, mean, sd, (float)NAN, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, NULL, NULL, (float)INFINITY, out, VIT_BF16, ws, big,
                                      NULL)));
  CHECK(strstr(vit_last_error(), "erase_value") != NULL);
  /* a bad dtype */
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, NULL, NULL, 0.f, out, VIT_MASK4, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, NULL, NULL, 0.f, out, 7, ws, big, NULL)));
  CHECK(strstr(vit_last_error(), "dtype") != NULL);
  /* the size limits of vit_resize_to_tensor */
  CHECK(refused(vit_augment_to_tensor(src, meta, items, 0, S, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, 0, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, -1, KS, NULL, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, 2, NULL, NULL, 0.f, out, VIT_F32, ws, big, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, 65536, S, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws,
                                      INT64_MAX, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, 65536, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws,
                                      INT64_MAX, NULL)));
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, 4097, NULL, NULL, 0.f, out, VIT_F32, ws,
                                      INT64_MAX, NULL)));
  CHECK(strstr(vit_last_error(), "range") != NULL);
  /* a workspace that is too small */
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS, NULL, NULL, 0.f, out, VIT_F32, ws, big - 1, NULL)));
  CHECK(strstr(vit_last_error(), "workspace") != NULL);
  CHECK(refused(vit_augment_to_tensor(src, meta, items, B, S, S, KS + 2, mean, sd, 0.f, out, VIT_F32, ws, big, NULL)));

  /* the option that chooses between the two forms: 0 by default, set and restored */
  CHECK(vit_get_option("augment_path") == 0);
  CHECK(vit_set_option("augment_path", 2) == 0 && vit_get_option("augment_path") == 2);
  CHECK(vit_set_option("augment_path", 0) == 0 && vit_get_option("augment_path") == 0);

  if (fails == 0) printf("host_abi_aug_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
