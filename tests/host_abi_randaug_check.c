/* Host-side checks of the RandAugment entry points that need no GPU: the layout of vit_ra_layer / vit_ra_item is what
 * the header states; vit_augment_to_u8 and vit_randaug_to_tensor refuse bad input through VIT_REQUIRE before any
 * launch, with an error string that names them; vit_randaug_workspace_bytes holds two pictures and one layer's tables
 * and is monotone; and adding them left the ABI version at 18.  Built by tests/test_randaug_cpu.py against the shipped
 * library with gcc, as tests/host_abi_aug_check.c is.
 * Exit status 0 = every check passed; a failed check prints its line. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "host_abi_randaug_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                                 \
    }                                                                          \
  } while (0)

/* an entry point refused its arguments: VIT_ERR_INVALID and a message naming it */
static int refused(int rc, const char* who) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, who) != NULL;
}
#define U8 "vit_augment_to_u8"
#define RA "vit_randaug_to_tensor"

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);

  /* ---- layout */
  CHECK(VIT_RA_MAX_LAYERS == 4);
  CHECK(sizeof(vit_ra_layer) == 72 && sizeof(vit_ra_item) == 288);
  CHECK(offsetof(vit_ra_layer, coef) == 0 && offsetof(vit_ra_layer, kind) == 48);
  CHECK(offsetof(vit_ra_layer, iarg0) == 52 && offsetof(vit_ra_layer, iarg1) == 56);
  CHECK(offsetof(vit_ra_layer, farg) == 60 && offsetof(vit_ra_layer, fill) == 64);
  CHECK(offsetof(vit_ra_item, layer) == 0);
  CHECK(VIT_RA_NONE == 0 && VIT_RA_AUTOCONTRAST == 1 && VIT_RA_EQUALIZE == 2 && VIT_RA_INVERT == 3);
  CHECK(VIT_RA_POSTERIZE == 4 && VIT_RA_SOLARIZE == 5 && VIT_RA_SOLARIZE_ADD == 6 && VIT_RA_COLOR == 7);
  CHECK(VIT_RA_CONTRAST == 8 && VIT_RA_BRIGHTNESS == 9 && VIT_RA_SHARPNESS == 10 && VIT_RA_AFFINE == 11);
  CHECK(VIT_RA_KINDS == 12);

  /* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
  static char src[64], ws[64];
  static char u8[4096], out[4096];
  static int64_t meta[8];
  static vit_aug_item items[2];
  static vit_ra_item ra[2];
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  const int64_t B = 2, S = 8, KS = 3;

  /* ---- vit_augment_to_u8(src, meta, items, B, oh, ow, ks, out_u8, ws, ws_bytes, stream): vit_augment_to_tensor's
   * tables, workspace and limits */
  const int64_t big = vit_augment_workspace_bytes(B, S, S, KS);
  CHECK(refused(vit_augment_to_u8(NULL, meta, items, B, S, S, KS, u8, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, NULL, items, B, S, S, KS, u8, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, NULL, B, S, S, KS, u8, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, S, S, KS, NULL, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, S, S, KS, u8, NULL, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, 0, S, S, KS, u8, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, 0, S, KS, u8, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, S, -1, KS, u8, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, S, S, 2, u8, ws, big, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, 65536, S, S, KS, u8, ws, INT64_MAX, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, 65536, S, KS, u8, ws, INT64_MAX, NULL), U8));
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, S, S, 4097, u8, ws, INT64_MAX, NULL), U8));
  CHECK(strstr(vit_last_error(), "range") != NULL);
  CHECK(refused(vit_augment_to_u8(src, meta, items, B, S, S, KS, u8, ws, big - 1, NULL), U8));
  CHECK(strstr(vit_last_error(), "workspace") != NULL);

  /* ---- vit_randaug_workspace_bytes: two pictures of the batch and one layer's [B][3][256] tables; monotone */
  const int64_t need = vit_randaug_workspace_bytes(B, S, S);
  CHECK(need >= 2 * B * S * S * 3 + B * 768);
  CHECK(vit_randaug_workspace_bytes(B + 1, S, S) > need);
  CHECK(vit_randaug_workspace_bytes(B, S + 9, S) > need);
  CHECK(vit_randaug_workspace_bytes(B, S, S + 9) > need);
  CHECK(vit_randaug_workspace_bytes(0, S, S) < 0 && vit_randaug_workspace_bytes(B, 0, S) < 0);
  CHECK(vit_randaug_workspace_bytes(B, S, -1) < 0);

  /* ---- vit_randaug_to_tensor(u8, ra, B, S_h, S_w, nlayers, stats_layers, mean3, std3, erase_items, erase_value, out,
   * dtype, ws, ws_bytes, stream): every call below is refused before any launch.  A pretended workspace address far
   * from the other buffers keeps the overlap check out of the way of the other checks. */
  char* far_ws = (char*)(uintptr_t)0x10000000000ull;
#define CALL(u8_, ra_, B_, H_, W_, nl, st, m_, s_, it_, ev, out_, dt, ws_, wsb)                                         \
  vit_randaug_to_tensor(u8_, ra_, B_, H_, W_, nl, st, m_, s_, it_, ev, out_, dt, ws_, wsb, NULL)
  CHECK(refused(CALL(NULL, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, NULL, B, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, NULL, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, NULL, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, NULL, need), RA));
  /* sizes */
  CHECK(refused(CALL(u8, ra, 0, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, 0, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, -3, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, 65536, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, INT64_MAX), RA));
  CHECK(refused(CALL(u8, ra, B, 65536, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, INT64_MAX), RA));
  CHECK(refused(CALL(u8, ra, 1, 32768, 32768, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, INT64_MAX), RA));
  CHECK(strstr(vit_last_error(), "range") != NULL);
  /* layers */
  CHECK(refused(CALL(u8, ra, B, S, S, 0, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, VIT_RA_MAX_LAYERS + 1, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(strstr(vit_last_error(), "nlayers") != NULL);
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 4, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, 2, -1, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(strstr(vit_last_error(), "stats_layers") != NULL);
  /* mean / std / erase_value / dtype, as for vit_augment_to_tensor */
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, mean, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, sd, items, 0.f, out, VIT_F32, far_ws, need), RA));
  for (int c = 0; c < 3; ++c) {
    const float bad[3] = {0.f, (float)INFINITY, (float)NAN};
    for (int k = 0; k < 3; ++k) {
      float s2[3] = {sd[0], sd[1], sd[2]};
      s2[c] = bad[k];
      CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, mean, s2, items, 0.f, out, VIT_F32, far_ws, need), RA));
      CHECK(strstr(vit_last_error(), "std") != NULL);
    }
    float m2[3] = {mean[0], mean[1], mean[2]};
    m2[c] = (float)NAN;
    CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, m2, sd, items, 0.f, out, VIT_F32, far_ws, need), RA));
  }
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, mean, sd, items, (float)NAN, out, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, (float)INFINITY, out, VIT_BF16, far_ws, need), RA));
  CHECK(strstr(vit_last_error(), "erase_value") != NULL);
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_MASK4, far_ws, need), RA));
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, out, 7, far_ws, need), RA));
  CHECK(strstr(vit_last_error(), "dtype") != NULL);
  /* a workspace that is too small */
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need - 1), RA));
  CHECK(strstr(vit_last_error(), "workspace") != NULL);
  /* overlaps: out with u8_in, out with the workspace, u8_in with the workspace */
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, u8 + 16, VIT_F32, far_ws, need), RA));
  CHECK(strstr(vit_last_error(), "overlap") != NULL);
  CHECK(refused(CALL(u8, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, far_ws + need - 4, VIT_F32, far_ws, need), RA));
  CHECK(refused(CALL(far_ws + 64, ra, B, S, S, 2, 0, NULL, NULL, items, 0.f, out, VIT_F32, far_ws, need), RA));
  CHECK(strstr(vit_last_error(), "overlap") != NULL);

  if (fails == 0) printf("host_abi_randaug_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
