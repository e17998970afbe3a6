/* Host-side checks of the stochastic-depth entry points that need no GPU: vit_drop_path_rows and vit_gemm_rowscale
 * link, refuse bad input through VIT_REQUIRE before any launch, with an error string that names the entry point (or,
 * for a descriptor vit_gemm itself refuses, vit_gemm), and adding them left the ABI version at 18 (purely added entry
 * points do not change it, vit_hip.h).  Built by tests/test_drop_path_cpu.py against the shipped library with gcc, as
 * tests/host_abi_mix_check.c is.
 * Exit status 0 = every check passed; a failed check prints its line. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vit_hip.h"

static int fails = 0;
#define CHECK(c)                                                                       \
  do {                                                                                 \
    if (!(c)) {                                                                        \
      fprintf(stderr, "host_abi_drop_path_check: FAILED line %d: %s\n", __LINE__, #c); \
      ++fails;                                                                         \
    }                                                                                  \
  } while (0)

/* an entry point refused its arguments: VIT_ERR_INVALID and a non-empty message naming it */
static int refused(int rc, const char* name) {
  const char* e = vit_last_error();
  return rc == VIT_ERR_INVALID && e != NULL && strstr(e, name) != NULL;
}

#define ROWS "vit_drop_path_rows"
#define RSC "vit_gemm_rowscale"

int main(void) {
  CHECK(vit_abi_version() == 18);
  CHECK(VIT_ABI_VERSION == 18);
  CHECK(VIT_DROP_PATH_MAX_LAYERS == 64);

  /* non-null host addresses: a refused call never reads them, let alone hands them to a kernel */
  static float out[64];
  static float many[VIT_DROP_PATH_MAX_LAYERS + 1];
  float rates[3] = {0.f, 0.25f, 0.5f};

  /* ---- vit_drop_path_rows(out, seed, L, B, T, rates, stream) */
  CHECK(refused(vit_drop_path_rows(NULL, 1u, 3, 2, 2, rates, NULL), ROWS));                   /* NULL pointers */
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, 2, NULL, NULL), ROWS));
  CHECK(refused(vit_drop_path_rows(out, 1u, 0, 2, 2, rates, NULL), ROWS));                    /* sizes <= 0 */
  CHECK(refused(vit_drop_path_rows(out, 1u, -1, 2, 2, rates, NULL), ROWS));
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 0, 2, rates, NULL), ROWS));
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, 0, rates, NULL), ROWS));
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, -5, rates, NULL), ROWS));
  CHECK(refused(vit_drop_path_rows(out, 1u, VIT_DROP_PATH_MAX_LAYERS + 1, 2, 2, many, NULL), ROWS));   /* the cap on L */
  CHECK(strstr(vit_last_error(), "VIT_DROP_PATH_MAX_LAYERS") != NULL);
  CHECK(refused(vit_drop_path_rows(out, 1u, 1, (int64_t)1 << 20, (int64_t)1 << 11, rates, NULL), ROWS));   /* B*T = 2^31 */
  rates[1] = 1.0f;                                                                            /* rates outside [0, 1) */
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, 2, rates, NULL), ROWS));
  CHECK(strstr(vit_last_error(), "rate") != NULL);
  rates[1] = -0.01f;
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, 2, rates, NULL), ROWS));
  rates[1] = 1.5f;
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, 2, rates, NULL), ROWS));
  rates[1] = (float)NAN;
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, 2, rates, NULL), ROWS));
  rates[1] = 0.25f;
  rates[2] = 1.0f;                                                                            /* ... in the last entry */
  CHECK(refused(vit_drop_path_rows(out, 1u, 3, 2, 2, rates, NULL), ROWS));
  CHECK(vit_drop_path_rows(out, 1u, 2, 2, 2, NULL, NULL) == VIT_ERR_INVALID);

  /* ---- vit_gemm_rowscale(d, row_scale, stream): vit_gemm's own refusals, and the table's alignment */
  CHECK(refused(vit_gemm_rowscale(NULL, out, NULL), "vit_gemm"));                              /* NULL descriptor */
  static float a[16], b[16], c[16];
  vit_gemm_desc d;
  memset(&d, 0, sizeof d);
  d.a = a; d.b = b; d.c = c;
  d.lda = d.ldb = d.ldc = 4;
  d.m = d.n = d.k = 4;
  d.a_kcontig = d.b_kcontig = 1;
  d.in_dtype = d.out_dtype = VIT_F32;
  d.alpha = 1.f;
  CHECK(refused(vit_gemm_rowscale(&d, (const float*)((const char*)out + 2), NULL), RSC));      /* misaligned table */
  d.m = 0;
  CHECK(refused(vit_gemm_rowscale(&d, out, NULL), "vit_gemm"));                                /* bad shape */
  d.m = 4;
  d.dropout_p = 1.0f;
  CHECK(refused(vit_gemm_rowscale(&d, out, NULL), "vit_gemm"));                                /* dropout_p */
  d.dropout_p = 0.f;
  d.c = NULL;
  CHECK(refused(vit_gemm_rowscale(&d, out, NULL), "vit_gemm"));                                /* NULL operand */

  /* ---- vit_gemm_kernel_choice(d, row_scale, &impl, &kind): the launcher's plan, nothing launched or read */
  int32_t impl = -1, kind = -1;
  d.c = c;
  CHECK(vit_gemm_kernel_choice(&d, NULL, &impl, &kind) == VIT_OK && impl == 0 && kind == VIT_EPI_GENERAL);  /* fp32 */
  CHECK(refused(vit_gemm_kernel_choice(&d, NULL, NULL, &kind), "vit_gemm_kernel_choice"));
  CHECK(refused(vit_gemm_kernel_choice(&d, NULL, &impl, NULL), "vit_gemm_kernel_choice"));
  CHECK(refused(vit_gemm_kernel_choice(NULL, NULL, &impl, &kind), "vit_gemm"));
  /* the forward's proj GEMM: bf16, both operands k-contiguous, bias, dropout, bf16 residual, keep bits */
  static _Alignas(16) char big[16];
  memset(&d, 0, sizeof d);
  d.a = big; d.b = big; d.c = big; d.res = big; d.mask_out = big;
  d.bias = (const float*)big;
  d.m = 272; d.n = 256; d.k = 128;
  d.lda = d.ldb = 128; d.ldc = d.ldres = 256;
  d.a_kcontig = d.b_kcontig = 1;
  d.in_dtype = d.out_dtype = d.res_dtype = VIT_BF16;
  d.alpha = 1.f;
  d.dropout_p = 0.2f;
  CHECK(vit_gemm_kernel_choice(&d, NULL, &impl, &kind) == VIT_OK && impl == 4 && kind == VIT_EPI_BDR);
  CHECK(vit_gemm_kernel_choice(&d, out, &impl, &kind) == VIT_OK && impl == 4 && kind == VIT_EPI_BDRS);
  d.dropout_p = 0.f;                       /* no dropout, no residual: still the kind that applies the factor */
  d.res = NULL;
  CHECK(vit_gemm_kernel_choice(&d, out, &impl, &kind) == VIT_OK && impl == 4 && kind == VIT_EPI_BDRS);
  d.act = VIT_ACT_RELU;                    /* what the fast kind does not compute goes to the general epilogue */
  CHECK(vit_gemm_kernel_choice(&d, out, &impl, &kind) == VIT_OK && impl == 4 && kind == VIT_EPI_GENERAL);
  d.act = VIT_ACT_NONE;
  d.m = 136;                               /* a half-batch chain of 8 x 17 rows: the 128x128 kernel */
  CHECK(vit_gemm_kernel_choice(&d, out, &impl, &kind) == VIT_OK && impl == 2 && kind == VIT_EPI_GENERAL);
  d.m = 272;
  d.split_k = 2;                           /* a K split: slabs, then the reduce's general epilogue */
  CHECK(vit_gemm_kernel_choice(&d, out, &impl, &kind) == VIT_OK && impl == 4 && kind == VIT_EPI_SLAB);

  if (fails == 0) printf("host_abi_drop_path_check: all checks passed (ABI %d)\n", vit_abi_version());
  return fails == 0 ? 0 : 1;
}
