// Patch dropout (timm's patch_drop_rate, the FLIP / MAE-style token subset): the keep table of a training forward, and
// the gathering / scattering forms of the embedding's memory-bound kernels.  All small and memory-bound; none is on the
// MFMA path.  Layout of the kept tokens (vit_hip.h "Patch dropout"): K of the N patches per image in ascending patch
// order, patch 0 always among them, then the CLS token — T' = K + 1 rows per image.
#include "vit_common.h"

namespace {

inline unsigned pd_grid(int64_t work, int64_t per_block, int64_t cap = 16384) {
  int64_t b = (work + per_block - 1) / per_block;
  return (unsigned)std::min<int64_t>(std::max<int64_t>(b, 1), cap);
}

// A table entry as the row it may address: tables can come from a caller (Engine.forward(keep=...)), and an entry
// outside its range must not become an address outside the tensor.
VIT_DEV int64_t pd_patch(int32_t n, int64_t N) { return n < 0 ? 0 : (n >= N ? N - 1 : n); }

// ---------------------------------------------------------------------------------------------------------------
// vit_patch_keep: one workgroup per image.  The N keys go into LDS; thread t owns the contiguous patches
// [t * per, (t + 1) * per) and ranks each among patches 1 .. N-1 by counting the smaller (key, n) pairs — every lane
// reads the same LDS word at the same time (a broadcast) — then the kept patches' rows come from a prefix sum over
// the per-thread keep counts.  No atomics: the same seed gives the same bytes.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PK_THREADS = 256;
constexpr int PK_MAX_N = 4096;
constexpr int PK_PER = PK_MAX_N / PK_THREADS;      // most patches one thread owns

__global__ __launch_bounds__(PK_THREADS) void patch_keep_kernel(uint32_t pseed, int N, int K, int32_t* __restrict__ idx,
                                                                int32_t* __restrict__ inv) {
  __shared__ uint32_t keys[PK_MAX_N];
  __shared__ int cnt[PK_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  for (int n = t; n < N; n += PK_THREADS) keys[n] = vit_hash_u32(pseed, (uint32_t)b * (uint32_t)N + (uint32_t)n);
  __syncthreads();
  const int per = (N + PK_THREADS - 1) / PK_THREADS;
  const int n0 = min(t * per, N), n1 = min(n0 + per, N);
  uint32_t keep = 0;                                // bit i: patch n0 + i is kept (per <= 16)
  int mine = 0;
  for (int n = n0; n < n1; ++n) {
    bool k = n == 0;
    if (n > 0) {
      const uint32_t kn = keys[n];
      int rank = 0;
      for (int m = 1; m < N; ++m) {
        const uint32_t km = keys[m];
        rank += (km < kn || (km == kn && m < n)) ? 1 : 0;
      }
      k = rank < K - 1;
    }
    keep |= (k ? 1u : 0u) << (n - n0);
    mine += k ? 1 : 0;
  }
  cnt[t] = mine;
  __syncthreads();
  int j = 0;
  for (int u = 0; u < t; ++u) j += cnt[u];
  for (int n = n0; n < n1; ++n) {
    const bool k = (keep >> (n - n0)) & 1u;
    inv[(int64_t)b * N + n] = k ? j : -1;
    if (k) {
      if (j < K) idx[(int64_t)b * K + j] = n;       // (j < K always: exactly K bits are set per image)
      ++j;
    }
  }
}

// im2col_kernel (vit_misc.hip) where row b * K + j is patch idx[b, j] of image b: same thread shape (row, 4 columns),
// same 4-column store; the patches outside the table are never read.
template <class TI, class TO>
__global__ __launch_bounds__(256) void im2col_gather_kernel(const TI* __restrict__ x, TO* __restrict__ cols,
                                                            const int32_t* __restrict__ idx, int64_t B, int64_t C,
                                                            int64_t H, int64_t W, int64_t P, int64_t K) {
  const int64_t nw = W / P, nh = H / P, N = nh * nw, KC = C * P * P;
  const int64_t q4 = KC / 4, total = B * K * q4;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = t / q4, col = (t % q4) * 4;
    const int64_t b = m / K, n = pd_patch(idx[m], N), ph = n / nw, pw = n % nw;
    const int64_t c = col / (P * P), rem = col % (P * P), kh = rem / P, kw = rem % P;
    const TI* src = x + ((b * C + c) * H + ph * P + kh) * W + pw * P + kw;
    float v[4];
    v[0] = ld1<TI>(src); v[1] = ld1<TI>(src + 1); v[2] = ld1<TI>(src + 2); v[3] = ld1<TI>(src + 3);
    st4<TO>(cols + m * KC + col, v);
  }
}

// posg[b * K + j] = pos[idx[b, j]]: the fp32 residual rows of the gathered embedding GEMM, 4 columns per thread.
__global__ __launch_bounds__(256) void gather_pos_kernel(const float* __restrict__ pos, const int32_t* __restrict__ idx,
                                                         float* __restrict__ posg, int64_t rows, int64_t N, int64_t D) {
  const int64_t q4 = D / 4, total = rows * q4;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = t / q4, col = (t % q4) * 4;
    *reinterpret_cast<f32x4*>(posg + m * D + col) =
        *reinterpret_cast<const f32x4*>(pos + pd_patch(idx[m], N) * D + col);
  }
}

// gpos[n] = beta * gpos[n] + sum over the images that kept position n of their row of dx, images in ascending order
// in one thread per (position, 4 columns): a fixed order, bitwise repeatable.  Position N is the CLS row K of every
// image.
template <class T>
__global__ __launch_bounds__(256) void pos_grad_gather_kernel(const T* __restrict__ dx, const int32_t* __restrict__ inv,
                                                              float* __restrict__ gpos, int64_t B, int64_t N, int64_t K,
                                                              int64_t D, float beta) {
  const int64_t q4 = D / 4, total = (N + 1) * q4, Tk = K + 1;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = t / q4, col = (t % q4) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t b = 0; b < B; ++b) {
      const int64_t j = n < N ? (int64_t)inv[b * N + n] : K;
      if (j >= 0 && j <= K) {
        float v[4];
        ld4<T>(dx + (b * Tk + j) * D + col, v);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += v[r];
      }
    }
    float* o = gpos + n * D + col;
    if (beta != 0.f) {
      float old[4];
      ld4<float>(o, old);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] += beta * old[r];
    }
    st4<float>(o, acc);
  }
}

// col2im_kernel (vit_misc.hip) reading row inv[b, n] of the gathered cols; zero where the patch was dropped.
template <class TI, class TO>
__global__ __launch_bounds__(256) void col2im_scatter_kernel(const TI* __restrict__ cols, const int32_t* __restrict__ inv,
                                                             TO* __restrict__ x, int64_t B, int64_t C, int64_t H,
                                                             int64_t W, int64_t P, int64_t K) {
  const int64_t nw = W / P, N = (H / P) * nw, KC = C * P * P, total = B * C * H * W;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t w = t % W, h = (t / W) % H, c = (t / (W * H)) % C, b = t / (W * H * C);
    const int64_t n = (h / P) * nw + w / P, col = (c * P + h % P) * P + w % P;
    const int64_t j = inv[b * N + n];
    st1<TO>(x + t, j >= 0 && j < K ? ld1<TI>(cols + (b * K + j) * KC + col) : 0.f);
  }
}

// the shape checks the table's users share
#define PD_REQUIRE_TABLE(name, B, N, K)                                                                                 \
  VIT_REQUIRE((B) > 0 && (N) >= 1 && (N) <= VIT_PATCH_KEEP_MAX_N && (K) >= 1 && (K) <= (N),                              \
              name ": need B > 0 and 1 <= K <= N <= %d, got B=%lld N=%lld K=%lld", VIT_PATCH_KEEP_MAX_N, (long long)(B), \
              (long long)(N), (long long)(K))

}  // namespace

static_assert(PK_MAX_N == VIT_PATCH_KEEP_MAX_N, "the kernel's LDS key array is the header's cap");
static_assert(PK_PER <= 32, "a thread's keep bits are one 32-bit word");

extern "C" int vit_patch_keep(uint32_t seed, int64_t L, int64_t B, int64_t N, int64_t K, int32_t* idx, int32_t* inv,
                              void* stream) {
  VIT_REQUIRE(idx && inv, "vit_patch_keep: null pointer");
  PD_REQUIRE_TABLE("vit_patch_keep", B, N, K);
  VIT_REQUIRE(L >= 0 && L < (1LL << 29), "vit_patch_keep: bad layer count L=%lld", (long long)L);
  VIT_REQUIRE(B * N < (1LL << 31), "vit_patch_keep: B * N must be below 2^31");
  // site_seed(seed, 2L, 0) of the host package: the element dropout's streams are layers 0 .. L-1, the drop path's
  // L .. 2L-1
  const uint32_t mixed = seed * 0x632BE5ABu + 0x1234567u, site = (uint32_t)(2 * L) * 2u;
  uint32_t h = site * 0x9E3779B1u + mixed;          // vit_hash_u32(mixed, site) on the host
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  h ^= h >> 16;
  patch_keep_kernel<<<(unsigned)B, PK_THREADS, 0, VIT_STREAM(stream)>>>(h, (int)N, (int)K, idx, inv);
  return vit::check_launch("vit_patch_keep");
}

extern "C" int vit_im2col_gather(const void* x, int32_t x_dtype, void* cols, int32_t dtype, const int32_t* idx, int64_t B,
                                 int64_t C, int64_t H, int64_t W, int64_t P, int64_t K, void* stream) {
  VIT_REQUIRE(x && cols && idx, "vit_im2col_gather: null pointer");
  VIT_REQUIRE(B > 0 && C > 0 && P > 0 && H > 0 && W > 0 && H % P == 0 && W % P == 0,
              "vit_im2col_gather: image %lldx%lld not divisible by P=%lld", (long long)H, (long long)W, (long long)P);
  VIT_REQUIRE(P % 4 == 0, "vit_im2col_gather: patch size must be a multiple of 4");
  PD_REQUIRE_TABLE("vit_im2col_gather", B, (H / P) * (W / P), K);
  const unsigned grid = pd_grid(B * K * C * P * P / 4, 256);
  hipStream_t s = VIT_STREAM(stream);
  if (x_dtype == VIT_F32 && dtype == VIT_BF16)
    im2col_gather_kernel<float, bf16_t><<<grid, 256, 0, s>>>((const float*)x, (bf16_t*)cols, idx, B, C, H, W, P, K);
  else if (x_dtype == VIT_F32 && dtype == VIT_F32)
    im2col_gather_kernel<float, float><<<grid, 256, 0, s>>>((const float*)x, (float*)cols, idx, B, C, H, W, P, K);
  else if (x_dtype == VIT_BF16 && dtype == VIT_BF16)
    im2col_gather_kernel<bf16_t, bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)x, (bf16_t*)cols, idx, B, C, H, W, P, K);
  else {
    vit::set_error("vit_im2col_gather: unsupported dtype pair %d->%d", x_dtype, dtype);
    return VIT_ERR_INVALID;
  }
  return vit::check_launch("vit_im2col_gather");
}

extern "C" int vit_gather_pos(const float* pos, const int32_t* idx, float* posg, int64_t B, int64_t N, int64_t K,
                              int64_t D, void* stream) {
  VIT_REQUIRE(pos && idx && posg, "vit_gather_pos: null pointer");
  PD_REQUIRE_TABLE("vit_gather_pos", B, N, K);
  VIT_REQUIRE(D > 0 && D % 4 == 0, "vit_gather_pos: D=%lld must be a positive multiple of 4", (long long)D);
  VIT_REQUIRE(((uintptr_t)pos | (uintptr_t)posg) % 16 == 0, "vit_gather_pos: pos and posg must be 16-byte aligned");
  gather_pos_kernel<<<pd_grid(B * K * D / 4, 256), 256, 0, VIT_STREAM(stream)>>>(pos, idx, posg, B * K, N, D);
  return vit::check_launch("vit_gather_pos");
}

extern "C" int vit_pos_grad_gather(const void* dx, int32_t dtype, const int32_t* inv, float* gpos, int64_t B, int64_t N,
                                   int64_t K, int64_t D, float beta, void* stream) {
  VIT_REQUIRE(dx && inv && gpos, "vit_pos_grad_gather: null pointer");
  PD_REQUIRE_TABLE("vit_pos_grad_gather", B, N, K);
  VIT_REQUIRE(D > 0 && D % 4 == 0, "vit_pos_grad_gather: D=%lld must be a positive multiple of 4", (long long)D);
  VIT_REQUIRE((uintptr_t)gpos % 16 == 0 && (uintptr_t)dx % (dtype == VIT_BF16 ? 8 : 16) == 0,
              "vit_pos_grad_gather: dx and gpos must be aligned for 4-column accesses");
  const unsigned grid = pd_grid((N + 1) * D / 4, 256);
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_BF16)
    pos_grad_gather_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)dx, inv, gpos, B, N, K, D, beta);
  else if (dtype == VIT_F32)
    pos_grad_gather_kernel<float><<<grid, 256, 0, s>>>((const float*)dx, inv, gpos, B, N, K, D, beta);
  else {
    vit::set_error("vit_pos_grad_gather: unsupported dtype %d", dtype);
    return VIT_ERR_INVALID;
  }
  return vit::check_launch("vit_pos_grad_gather");
}

extern "C" int vit_col2im_scatter(const void* cols, int32_t dtype, const int32_t* inv, void* x, int32_t x_dtype, int64_t B,
                                  int64_t C, int64_t H, int64_t W, int64_t P, int64_t K, void* stream) {
  VIT_REQUIRE(x && cols && inv, "vit_col2im_scatter: null pointer");
  VIT_REQUIRE(B > 0 && C > 0 && P > 0 && H > 0 && W > 0 && H % P == 0 && W % P == 0,
              "vit_col2im_scatter: image %lldx%lld not divisible by P=%lld", (long long)H, (long long)W, (long long)P);
  PD_REQUIRE_TABLE("vit_col2im_scatter", B, (H / P) * (W / P), K);
  const unsigned grid = pd_grid(B * C * H * W, 256);
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_BF16 && x_dtype == VIT_F32)
    col2im_scatter_kernel<bf16_t, float><<<grid, 256, 0, s>>>((const bf16_t*)cols, inv, (float*)x, B, C, H, W, P, K);
  else if (dtype == VIT_F32 && x_dtype == VIT_F32)
    col2im_scatter_kernel<float, float><<<grid, 256, 0, s>>>((const float*)cols, inv, (float*)x, B, C, H, W, P, K);
  else if (dtype == VIT_BF16 && x_dtype == VIT_BF16)
    col2im_scatter_kernel<bf16_t, bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)cols, inv, (bf16_t*)x, B, C, H, W, P, K);
  else {
    vit::set_error("vit_col2im_scatter: unsupported dtype pair %d->%d", dtype, x_dtype);
    return VIT_ERR_INVALID;
  }
  return vit::check_launch("vit_col2im_scatter");
}
