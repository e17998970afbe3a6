// Memory-bound kernels of the ViT step: patch im2col, CLS rows, column sums, strided copies, dropout backward,
// GELU, softmax cross-entropy, the multi-tensor AdamW / shadow-weight pack, the gradient norm of its clipped
// form and the weight EMA kept inside it.  All vectorised where the shape allows (8-16 B per lane), grid-stride,
// fixed reduction order (bitwise reproducible).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>

#include "vit_common.h"

namespace vit {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return VIT_ERR_LAUNCH;
  }
  return VIT_OK;
}
}  // namespace vit

extern "C" int vit_abi_version(void) { return VIT_ABI_VERSION; }
extern "C" const char* vit_last_error(void) { return vit::g_err; }

// ---------------------------------------------------------------------------------------------------------------
// Launch options (vit_hip.h vit_set_option): names, shipped defaults, current values.
// ---------------------------------------------------------------------------------------------------------------
namespace {
struct OptDef {
  const char* name;
  int64_t def;
};
#define X(ENUM, NAME, DEF) {NAME, DEF},
constexpr OptDef kOpts[vit::OPT_COUNT] = {VIT_OPTIONS(X)};
#undef X
#define X(ENUM, NAME, DEF) {DEF},
std::atomic<int64_t> g_opt[vit::OPT_COUNT] = {VIT_OPTIONS(X)};
#undef X

int opt_index(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < vit::OPT_COUNT; ++i)
    if (strcmp(name, kOpts[i].name) == 0) return i;
  return -1;
}
}  // namespace

int64_t vit::opt(vit::Opt o) { return g_opt[o].load(std::memory_order_relaxed); }

extern "C" int vit_set_option(const char* name, int64_t value) {
  const int i = opt_index(name);
  VIT_REQUIRE(i >= 0, "vit_set_option: unknown option '%s'", name ? name : "(null)");
  g_opt[i].store(value, std::memory_order_relaxed);
  return VIT_OK;
}

extern "C" int64_t vit_get_option(const char* name) {
  const int i = opt_index(name);
  return i >= 0 ? g_opt[i].load(std::memory_order_relaxed) : INT64_MIN;
}

namespace {

inline unsigned grid_for(int64_t work, int64_t per_block, int64_t cap = 8192) {
  int64_t b = (work + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

// ---------------------------------------------------------------------------------------------------------------
// im2col: one thread per (row m = b*N + n, 4 consecutive columns); column (c, kh, kw) with kw fastest.
// ---------------------------------------------------------------------------------------------------------------
template <class TI, class TO>
__global__ __launch_bounds__(256) void im2col_kernel(const TI* __restrict__ x, TO* __restrict__ cols, int64_t B,
                                                     int64_t C, int64_t H, int64_t W, int64_t P) {
  const int64_t nw = W / P, nh = H / P, N = nh * nw, KC = C * P * P;
  const int64_t q4 = KC / 4, total = B * N * q4;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = t / q4, col = (t % q4) * 4;
    const int64_t b = m / N, n = m % N, ph = n / nw, pw = n % nw;
    const int64_t c = col / (P * P), rem = col % (P * P), kh = rem / P, kw = rem % P;
    const TI* src = x + ((b * C + c) * H + ph * P + kh) * W + pw * P + kw;
    float v[4];
    v[0] = ld1<TI>(src); v[1] = ld1<TI>(src + 1); v[2] = ld1<TI>(src + 2); v[3] = ld1<TI>(src + 3);
    st4<TO>(cols + m * KC + col, v);
  }
}

// col2im for k = s = P: one thread per image element (b, c, h, w), coalesced on the image write.
template <class TI, class TO>
__global__ __launch_bounds__(256) void col2im_kernel(const TI* __restrict__ cols, TO* __restrict__ x, int64_t B,
                                                     int64_t C, int64_t H, int64_t W, int64_t P) {
  const int64_t nw = W / P, N = (H / P) * nw, KC = C * P * P, total = B * C * H * W;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t w = t % W, h = (t / W) % H, c = (t / (W * H)) % C, b = t / (W * H * C);
    const int64_t n = (h / P) * nw + w / P, col = (c * P + h % P) * P + w % P;
    st1<TO>(x + t, ld1<TI>(cols + (b * N + n) * KC + col));
  }
}

template <class T>
__global__ __launch_bounds__(256) void embed_cls_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                        T* __restrict__ x0, int64_t B, int64_t T_, int64_t D) {
  const int64_t N = T_ - 1;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < B * D; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / D, d = t % D;
    st1<T>(x0 + (b * T_ + N) * D + d, cls[b * D + d] + pos[N * D + d]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Column sums, two deterministic stages.  Stage 1: block (64 x 4 threads) owns 256 columns (4 per lane) and a chunk
// of rows; writes partial[chunk][cols].  Stage 2: one thread per column sums the chunks in order.
// ---------------------------------------------------------------------------------------------------------------
constexpr int CS_CHUNKS_MAX = 256;

template <class T>
__global__ __launch_bounds__(256) void colsum_stage1(const T* __restrict__ x, int64_t ldx, int64_t rows,
                                                     int64_t cols, int64_t rows_per_chunk, float* __restrict__ part,
                                                     int vec, float alpha = 1.f) {
  __shared__ float red[4][256];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 256 + tx * 4;
  const int64_t chunk = blockIdx.y;
  const int64_t r0 = chunk * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0 + ty; r < r1; r += 4) {
    const T* p = x + r * ldx + c0;
    if (vec && c0 + 3 < cols) {
      float v[4];
      ld4<T>(p, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += v[k];
    } else {
      for (int k = 0; k < 4; ++k)
        if (c0 + k < cols) acc[k] += ld1<T>(p + k);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[ty][tx * 4 + k] = acc[k];
  __syncthreads();
  if (ty == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cc = tx * 4 + k;
      const float s = red[0][cc] + red[1][cc] + red[2][cc] + red[3][cc];
      if (c0 + k < cols) part[chunk * cols + c0 + k] = s * alpha;
    }
  }
}

// Stage 2: 64 columns per block; 16 waves stride over the chunk partials (wave w sums chunks w, w+16, ...), then the
// 16 wave sums are added in wave order through LDS -> deterministic for a given (rows, cols).
// blockIdx.y selects one of up to 3 independent sets: part + set*nchunks*cols -> outs.p[set] (vit_colsum_finish).
constexpr int CS2_WAVES = 16;
struct OutSet {
  float* p[3];
};
// One 64-column block of one set: the chunk partials summed by 16 waves (8 independent chains per lane), then the wave
// sums in wave order through LDS.
VIT_DEV void colsum_block(const float* __restrict__ part, int64_t nchunks, int64_t cols, float* __restrict__ out,
                          float beta, int64_t cblock, float (*red)[64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c = cblock * 64 + lane;
  // 8 independent chains per lane (chunk k goes to chain (k / CS2_WAVES) % 8): 8 loads in flight per lane, order fixed
  constexpr int CH = 8;
  float sc[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) sc[i] = 0.f;
  if (c < cols) {
    int64_t k = w;
    for (; k + (CH - 1) * CS2_WAVES < nchunks; k += CH * CS2_WAVES) {
#pragma unroll
      for (int i = 0; i < CH; ++i) sc[i] += part[(k + i * CS2_WAVES) * cols + c];
    }
#pragma unroll
    for (int i = 0; i < CH; ++i)
      if (k + i * CS2_WAVES < nchunks) sc[i] += part[(k + i * CS2_WAVES) * cols + c];
  }
  red[w][lane] = ((sc[0] + sc[1]) + (sc[2] + sc[3])) + ((sc[4] + sc[5]) + (sc[6] + sc[7]));
  __syncthreads();
  if (w == 0 && c < cols) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CS2_WAVES; ++i) s += red[i][lane];
    out[c] = beta != 0.f ? beta * out[c] + s : s;
  }
}

__global__ __launch_bounds__(64 * CS2_WAVES) void colsum_stage2(const float* __restrict__ part, int64_t nchunks,
                                                                int64_t cols, OutSet outs, float beta) {
  __shared__ float red[CS2_WAVES][64];
  float* out = blockIdx.y == 0 ? outs.p[0] : (blockIdx.y == 1 ? outs.p[1] : outs.p[2]);
  colsum_block(part + (int64_t)blockIdx.y * nchunks * cols, nchunks, cols, out, beta, blockIdx.x, red);
}

// vit_colsum_finish_batch: several finishes in one launch; block b belongs to the job whose [first, first + nsets *
// colblocks) range holds it.  Each (job, set, column block) is the same computation as colsum_stage2's.
constexpr int CS_BATCH_MAX = 8;
struct CsBatch {
  vit_colsum_job job[CS_BATCH_MAX];
  int64_t first[CS_BATCH_MAX + 1];
  int n;
};
__global__ __launch_bounds__(64 * CS2_WAVES) void colsum_stage2_batch(CsBatch tab) {
  __shared__ float red[CS2_WAVES][64];
  const int64_t b = blockIdx.x;
  int j = 0;
  while (j + 1 < tab.n && b >= tab.first[j + 1]) ++j;
  const vit_colsum_job& jb = tab.job[j];
  const int64_t cbs = (jb.cols + 63) / 64, local = b - tab.first[j], set = local / cbs;
  float* out = set == 0 ? jb.out[0] : (set == 1 ? jb.out[1] : jb.out[2]);
  colsum_block(jb.part + set * jb.nparts * jb.cols, jb.nparts, jb.cols, out, jb.beta, local % cbs, red);
}

int64_t colsum_chunks(int64_t rows, int64_t cols) {
  // aim for ~2048 blocks total, each with >= 32 rows
  const int64_t cblocks = (cols + 255) / 256;
  int64_t ch = 2048 / (cblocks > 0 ? cblocks : 1);
  if (ch < 1) ch = 1;
  if (ch > CS_CHUNKS_MAX) ch = CS_CHUNKS_MAX;
  const int64_t maxch = (rows + 31) / 32;
  if (ch > maxch) ch = maxch;
  if (ch < 1) ch = 1;
  return ch;
}

// ---------------------------------------------------------------------------------------------------------------
template <class TS, class TD>
__global__ __launch_bounds__(256) void copy2d_kernel(const TS* __restrict__ src, int64_t lds, TD* __restrict__ dst,
                                                     int64_t ldd, int64_t rows, int64_t cols, int64_t grp,
                                                     int64_t grp_stride, float beta) {
  const int64_t total = rows * cols;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / cols, j = t % cols;
    const int64_t si = grp ? (i / grp) * grp_stride + (i % grp) : i;
    float v = ld1<TS>(src + si * lds + j);
    TD* d = dst + i * ldd + j;
    if (beta != 0.f) v += beta * ld1<TD>(d);
    st1<TD>(d, v);
  }
}

// Same-dtype copy without beta as 16-B chunks (bit-exact; rows and leading dimensions 16-B aligned)
__global__ __launch_bounds__(256) void copy2d_raw16_kernel(const uint8_t* __restrict__ src, int64_t lds,
                                                           uint8_t* __restrict__ dst, int64_t ldd, int64_t rows,
                                                           int64_t cpr, int64_t grp, int64_t grp_stride) {
  const int64_t total = rows * cpr;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / cpr, j = (t - i * cpr) * 16;
    const int64_t si = grp ? (i / grp) * grp_stride + (i % grp) : i;
    *reinterpret_cast<uint4*>(dst + i * ldd + j) = *reinterpret_cast<const uint4*>(src + si * lds + j);
  }
}

template <class T>
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n,
                                                          uint32_t thr, float scale, uint32_t seed) {  // y = keep*x*scale
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const float v = ld1<T>(x + t);
    st1<T>(y + t, vit_hash_u32(seed, (uint32_t)t) >= thr ? v * scale : 0.f);
  }
}

// y[i][j] = x[i][j] * mask4 bit (i, j) * scale, x any dtype -> y any dtype (4 columns per thread; cols % 4 == 0)
template <class TI, class TO>
__global__ __launch_bounds__(256) void mask4_apply_kernel(const TI* __restrict__ x, int64_t ldx, TO* __restrict__ y,
                                                          int64_t ldy, const uint8_t* __restrict__ mask, int64_t rows,
                                                          int64_t cols, float scale) {
  const int64_t nq = cols / 4, total = rows * nq;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / nq, j = (t % nq) * 4;
    float v[4];
    ld4<TI>(x + i * ldx + j, v);
    const uint32_t b = mask[mask4_byte(i, j, cols)];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (b >> r) & 1u ? v[r] * scale : 0.f;
    st4<TO>(y + i * ldy + j, v);
  }
}

// Drop path: the per-row factor table of vit_drop_path_rows.  blockIdx.y = l * 2 + site, so the layer's threshold and
// scale are uniform reads of the kernel arguments; one draw per image, written to its T token rows.
struct DropPathTab {
  uint32_t thr[VIT_DROP_PATH_MAX_LAYERS];
  float scale[VIT_DROP_PATH_MAX_LAYERS];
};
__global__ __launch_bounds__(256) void drop_path_rows_kernel(float* __restrict__ out, uint32_t seed, uint32_t L,
                                                             uint32_t BT, uint32_t T, DropPathTab tab) {
  const uint32_t ls = blockIdx.y, l = ls >> 1;
  // site_seed(seed, L + l, site) of the host package: the element-dropout streams use layers 0 .. L-1
  const uint32_t sseed = vit_hash_u32(seed * 0x632BE5ABu + 0x1234567u, (L + l) * 2u + (ls & 1u));
  const uint32_t thr = tab.thr[l];
  const float scale = tab.scale[l];
  float* o = out + (int64_t)ls * BT;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < BT; t += gridDim.x * blockDim.x)
    o[t] = vit_hash_u32(sseed, t / T) >= thr ? scale : 0.f;
}

template <class T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                                       T* __restrict__ dx, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    st1<T>(dx + t, ld1<T>(y + t) > 0.f ? ld1<T>(dy + t) : 0.f);
}

__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    y[t] = gelu_erf(x[t]);
}
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ dx, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    dx[t] = dy[t] * gelu_erf_grad(x[t]);
}

// one workgroup per row: max, sum-exp, loss term, gradient row
__global__ __launch_bounds__(256) void xent_rows_kernel(const float* __restrict__ logits,
                                                        const int64_t* __restrict__ labels, int64_t classes,
                                                        float inv_rows, float* __restrict__ dlogits,
                                                        float* __restrict__ row_loss) {
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  const float* x = logits + r * classes;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float mx = -INFINITY;
  for (int64_t c = tid; c < classes; c += 256) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f;
  for (int64_t c = tid; c < classes; c += 256) s += __expf(x[c] - mx);
  s = wave_sum(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  s = red[0] + red[1] + red[2] + red[3];
  const float lse = mx + __logf(s);
  const int64_t y = labels[r];
  for (int64_t c = tid; c < classes; c += 256) {
    const float p = __expf(x[c] - lse);
    dlogits[r * classes + c] = (p - (c == y ? 1.f : 0.f)) * inv_rows;
  }
  if (tid == 0) row_loss[r] = lse - x[y];
}

// xent_rows_kernel against the two-label smoothed target t = (1 - eps) * (lam * onehot(a) + (1 - lam) * onehot(b)) +
// eps / C, which is never stored (vit_hip.h "vit_softmax_xent_mixed").  Everything is relative to the row maximum, the
// sum over the classes included: t sums to 1, so the maximum cancels and x - 16 gives the same loss to rounding.
// labels_b == NULL: b = a; lam == NULL: lam = 1.  A label outside [0, classes) gives a NaN loss, not a stray read.
__global__ __launch_bounds__(256) void xent_mixed_rows_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ labels_a,
                                                              const int64_t* __restrict__ labels_b,
                                                              const float* __restrict__ lam, float smoothing,
                                                              int64_t classes, float inv_rows,
                                                              float* __restrict__ dlogits,
                                                              float* __restrict__ row_loss) {
  __shared__ float red[4];
  __shared__ float red2[4];
  const int64_t r = blockIdx.x;
  const float* x = logits + r * classes;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float mx = -INFINITY;
  for (int64_t c = tid; c < classes; c += 256) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f, z = 0.f;                               // sum exp(x - mx), sum (x - mx)
  for (int64_t c = tid; c < classes; c += 256) {
    const float d = x[c] - mx;
    s += __expf(d);
    z += d;
  }
  s = wave_sum(s);
  z = wave_sum(z);
  if (lane == 0) {
    red[w] = s;
    red2[w] = z;
  }
  __syncthreads();
  s = red[0] + red[1] + red[2] + red[3];
  z = red2[0] + red2[1] + red2[2] + red2[3];
  const float lse = mx + __logf(s);
  const int64_t ya = labels_a[r];
  const int64_t yb = labels_b ? labels_b[r] : ya;
  const float l = (lam && labels_b) ? lam[r] : 1.f;
  const float keep = 1.f - smoothing;
  const float ta = keep * l, tb = keep * (1.f - l), tu = smoothing / (float)classes;
  for (int64_t c = tid; c < classes; c += 256) {
    const float p = __expf(x[c] - lse);
    const float t = (c == ya ? ta : 0.f) + (c == yb ? tb : 0.f) + tu;
    dlogits[r * classes + c] = (p - t) * inv_rows;
  }
  if (tid == 0) {
    const float za = (ya >= 0 && ya < classes) ? x[ya] - mx : NAN;
    const float zb = (yb >= 0 && yb < classes) ? x[yb] - mx : NAN;
    // a label of weight 0 contributes nothing, whatever its logit holds (lam in {0, 1}, or no partner at all)
    float v = __logf(s) - ((ta != 0.f ? ta * za : 0.f) + (tb != 0.f ? tb * zb : 0.f));
    if (smoothing != 0.f) v -= tu * z;                  // eps = 0: a -inf logit must not turn 0 * -inf into NaN
    row_loss[r] = v;
  }
}

__global__ __launch_bounds__(256) void xent_reduce_kernel(const float* __restrict__ row_loss, int64_t rows,
                                                          float inv_rows, float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += 256) s += row_loss[r];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (red[0] + red[1] + red[2] + red[3]) * inv_rows;
}

// ---------------------------------------------------------------------------------------------------------------
// Multi-tensor AdamW: one workgroup per table chunk (the host sets its size: 8 Ki elements, _ops.CHUNK), one element
// per lane per step (16-B accesses measured no faster: the update runs at ~5.8 TB/s over 30 B per element).
// ---------------------------------------------------------------------------------------------------------------
// EMA: also e += ema_w * (p_new - e) on the chunk's EMA slice `ema` (vit_hip.h "Weight EMA"), its load issued with the
// other four ahead of the dependent math.  One body for both forms, so that p / m / v / shadow agree bit for bit.
template <class TS, bool EMA = false>
VIT_DEV void adamw_chunk(const vit_tensor_chunk ch, float lr, float b1, float b2, float eps, float wd,
                         float step_size, float inv_sqrt_bc2, float gscale, float* ema = nullptr,
                         float ema_w = 0.f) {
  const float decay = 1.0f - lr * wd;
  for (int64_t t = threadIdx.x; t < ch.n; t += 256) {
    float g = ch.g[t] * gscale;
    float m = ch.m[t], v = ch.v[t], p = ch.p[t];
    float e = 0.f;
    if constexpr (EMA) e = ema[t];
    // p *= decay; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g; p -= step_size * m / (sqrt(v) inv_sqrt_bc2 + eps),
    // with the fused multiply-adds spelled out as the compiler had chosen them: left to it, the EMA form's extra
    // stream changed which products it fused, and with that the bits of m, v and p.  The plain form's last line is
    // left to the compiler, which keeps that kernel's code what it was; there it fuses exactly the fma written here.
    m = __builtin_fmaf(b1, m, (1.0f - b1) * g);
    v = __builtin_fmaf(b2, v, (1.0f - b2) * g * g);
    const float denom = __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
    if constexpr (EMA) p = __builtin_fmaf(p, decay, -(step_size * (m / denom)));
    else p = p * decay - step_size * (m / denom);
    ch.m[t] = m;
    ch.v[t] = v;
    ch.p[t] = p;
    if constexpr (EMA) ema[t] = __builtin_fmaf(ema_w, p - e, e);
    if (ch.shadow) st1<TS>((TS*)ch.shadow + t, p);
  }
}

template <class TS>
__global__ __launch_bounds__(256) void adamw_kernel(const vit_tensor_chunk* __restrict__ tab, float lr, float b1,
                                                    float b2, float eps, float wd, float step_size,
                                                    float inv_sqrt_bc2, float gscale) {
  adamw_chunk<TS>(tab[blockIdx.x], lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, gscale);
}

template <class TS>
__global__ __launch_bounds__(256) void pack_kernel(const vit_tensor_chunk* __restrict__ tab) {
  const vit_tensor_chunk ch = tab[blockIdx.x];
  if (!ch.shadow) return;
  for (int64_t t = threadIdx.x; t < ch.n; t += 256) st1<TS>((TS*)ch.shadow + t, ch.p[t]);
}

// ---------------------------------------------------------------------------------------------------------------
// Global-norm gradient clipping (vit_hip.h "Gradient clipping"): a norm pass over the AdamW chunk table, a one-
// workgroup finish that turns the per-chunk sums into (norm, coef, skip), and the AdamW update reading coef / skip
// from device memory.  Everything accumulates in fp64 in a fixed order: no atomics, bitwise reproducible.
// ---------------------------------------------------------------------------------------------------------------
VIT_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over the 256 threads of a workgroup, valid in thread 0: wave butterflies, then the 4 wave sums in wave order.
VIT_DEV double block_sum_f64(double v, double* red /* LDS [4] */) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

VIT_DEV double sq_f64(float g, float gs) {
  const double d = (double)(g * gs);      // the fp32 product the update itself forms
  return d * d;
}

// partial[chunk] = sum over the chunk of (gs * g[t])^2.  A pure read stream: where the chunk's gradient pointer is
// 16-B aligned each lane issues GS_UNROLL 16-B loads before it consumes the first (all of a lane's loads for the 8 Ki
// chunk in one batch), unconditionally, so none is branched around; any other base (views of a flat buffer are only
// 4-B aligned) and the last n % 4 elements go by dword.  A lane adds its elements in index order.  The table hands
// the pointer over through memory, so it is cast to the global address space here: global_load, not flat_load.
constexpr int GS_UNROLL = 8;
typedef const float __attribute__((address_space(1))) * gs_gptr;
typedef const f32x4 __attribute__((address_space(1))) * gs_gptr4;

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const vit_tensor_chunk* __restrict__ tab, float gs,
                                                         double* __restrict__ partial) {
  __shared__ double red[4];
  const vit_tensor_chunk ch = tab[blockIdx.x];
  const gs_gptr g = (gs_gptr)ch.g;
  double acc = 0.0;
  int64_t done = 0;                       // elements [0, done) are covered by the 16-B loop
  if ((reinterpret_cast<uintptr_t>(ch.g) & 15) == 0) {
    const gs_gptr4 g4 = (gs_gptr4)ch.g;
    const int64_t n4 = ch.n >> 2;
    int64_t i = threadIdx.x;
    for (; i + (GS_UNROLL - 1) * 256 < n4; i += GS_UNROLL * 256) {
      f32x4 x[GS_UNROLL];
#pragma unroll
      for (int u = 0; u < GS_UNROLL; ++u) x[u] = g4[i + u * 256];
#pragma unroll
      for (int u = 0; u < GS_UNROLL; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += sq_f64(x[u][j], gs);
    }
    for (; i < n4; i += 256) {
      const f32x4 x = g4[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += sq_f64(x[j], gs);
    }
    done = n4 << 2;
  }
  for (int64_t t = done + threadIdx.x; t < ch.n; t += 256) acc += sq_f64(g[t], gs);
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// clip[0] = norm, clip[1] = coef, clip[2] = skip, clip[3] += skip.  Thread t adds partial[t], partial[t + 256], ...
// in that order, then the fixed tree: the order depends on n only through how many terms each thread has.
// max_norm < 0 selects torch's behaviour for a non-finite norm (|max_norm| is the bound): no skip, and the
// coefficient (0 for an infinite norm, NaN for a NaN one) reaches the update.
__global__ __launch_bounds__(256) void grad_clip_finish_kernel(const double* __restrict__ partial, int64_t n,
                                                               float max_norm, float* __restrict__ clip) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i];
  acc = block_sum_f64(acc, red);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(acc);
  const bool finite = fabsf(norm) <= 3.402823466e+38f;      // false for inf and for NaN
  const bool skip = !finite && max_norm > 0.f;
  float coef = fabsf(max_norm) / (norm + 1e-6f);
  if (coef > 1.f) coef = 1.f;                               // a NaN stays NaN, as torch.clamp(max=1) leaves it
  if (skip) coef = 0.f;
  clip[0] = norm;
  clip[1] = coef;
  clip[2] = skip ? 1.f : 0.f;
  clip[3] += skip ? 1.f : 0.f;
}

// How every kernel of a clipped step begins: false when clip[2] (skip) is set, and the kernel then returns before it
// touches anything; else the gradient scale, where the kernel has one, takes clip[1] (coef).  clip == NULL is the
// unclipped step.
VIT_DEV bool clip_enter(const float* __restrict__ clip, float* gscale = nullptr) {
  if (!clip) return true;
  if (clip[2] != 0.f) return false;
  if (gscale) *gscale = *gscale * clip[1];
  return true;
}

// The AdamW update of a clipped step.  A kernel of its own, so adamw_kernel keeps its arguments and its code.  Its
// clip is never NULL (vit_adamw_clipped refuses one), so clip_enter's first exit is dead code here.
template <class TS>
__global__ __launch_bounds__(256) void adamw_clipped_kernel(const vit_tensor_chunk* __restrict__ tab, float lr,
                                                            float b1, float b2, float eps, float wd, float step_size,
                                                            float inv_sqrt_bc2, float gscale,
                                                            const float* __restrict__ clip) {
  if (!clip_enter(clip, &gscale)) return;
  adamw_chunk<TS>(tab[blockIdx.x], lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, gscale);
}

// ---------------------------------------------------------------------------------------------------------------
// Weight EMA inside the AdamW step (vit_hip.h "Weight EMA"): the update above, then e += w * (p_new - e) while p_new
// is still in a register — a sixth stream (8 B per element more: 38 instead of 30), no second pass over p.  ema[i] is
// chunk i's slice of the EMA tensor (only 4-B aligned: it may be a view), NULL for a chunk that keeps none, which then
// runs adamw_chunk as it is.  clip as in adamw_clipped_kernel, or NULL for the unclipped step.  One element per lane
// per iteration: adamw_chunk's EMA form.
// ---------------------------------------------------------------------------------------------------------------
template <class TS>
__global__ __launch_bounds__(256) void adamw_ema_kernel(const vit_tensor_chunk* __restrict__ tab,
                                                        float* const* __restrict__ ema, float lr, float b1, float b2,
                                                        float eps, float wd, float step_size, float inv_sqrt_bc2,
                                                        float gscale, float ema_w, const float* __restrict__ clip) {
  if (!clip_enter(clip, &gscale)) return;
  const vit_tensor_chunk ch = tab[blockIdx.x];
  float* const ema_p = ema[blockIdx.x];
  if (!ema_p) {
    adamw_chunk<TS>(ch, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, gscale);
    return;
  }
  adamw_chunk<TS, true>(ch, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, gscale, ema_p, ema_w);
}

// p <-> e element by element, shadow = (dtype) new p.  Reads only the p / shadow / n fields of the table.
template <class TS>
__global__ __launch_bounds__(256) void ema_swap_kernel(const vit_tensor_chunk* __restrict__ tab,
                                                       float* const* __restrict__ ema) {
  const vit_tensor_chunk ch = tab[blockIdx.x];
  float* const ema_p = ema[blockIdx.x];
  if (!ema_p) return;
  for (int64_t t = threadIdx.x; t < ch.n; t += 256) {
    const float p = ch.p[t], e = ema_p[t];
    ch.p[t] = e;
    ema_p[t] = p;
    if (ch.shadow) st1<TS>((TS*)ch.shadow + t, e);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// LAMB (vit_hip.h "LAMB"): Adam's moments, the update u = m_hat / (sqrt(v_hat) + eps) + wd * p, one trust ratio
// |p| / |u| per tensor, then p -= lr * ratio * u.  The ratio needs the whole tensor's norms before any element of it
// moves, so the step is two passes over the chunk table with a per-tensor finish between them.  u is not stored:
// pass 2 forms it again from the m and v pass 1 wrote and the p it left alone (42 B per element over both passes;
// storing u would cost 46 B and a parameter-sized buffer).
// ---------------------------------------------------------------------------------------------------------------
// u as both passes form it.  The host folds the bias corrections into c1 = bc1 / sqrt(bc2) and c2 = bc1 * eps, so
// that (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) = m / (sqrt(v) * c1 + c2): five roundings (sqrt, c1, the fma, the
// quotient, the last fma).  Both fused multiply-adds are spelled out, as in adamw_chunk and for its reason: left to
// the compiler, what it fuses depends on the code around the call, and the two passes must form the same bits.
VIT_DEV float lamb_u(float m, float v, float p, float c1, float c2, float wd) {
  const float denom = __builtin_fmaf(sqrtf(v), c1, c2);
  return __builtin_fmaf(wd, p, m / denom);
}

// Pass 1, one workgroup per chunk: m and v as adamw_chunk forms them, written back; partial[2i] = sum p^2 and
// partial[2i + 1] = sum u^2 over chunk i = blockIdx.x, each fp32 value squared and added in fp64, a lane's elements in
// index order, then block_sum_f64's fixed tree.  p is only read.
VIT_DEV void lamb_moments_chunk(const vit_tensor_chunk ch, float b1, float b2, float c1, float c2, float wd,
                                float gscale, double* __restrict__ partial) {
  __shared__ double red_p[4], red_u[4];
  double sp = 0.0, su = 0.0;
  for (int64_t t = threadIdx.x; t < ch.n; t += 256) {
    const float g = ch.g[t] * gscale;
    float m = ch.m[t], v = ch.v[t];
    const float p = ch.p[t];
    m = __builtin_fmaf(b1, m, (1.0f - b1) * g);
    v = __builtin_fmaf(b2, v, (1.0f - b2) * g * g);
    const float u = lamb_u(m, v, p, c1, c2, wd);
    ch.m[t] = m;
    ch.v[t] = v;
    sp += (double)p * (double)p;
    su += (double)u * (double)u;
  }
  sp = block_sum_f64(sp, red_p);
  su = block_sum_f64(su, red_u);
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = sp;
    partial[2 * (int64_t)blockIdx.x + 1] = su;
  }
}

// clip as in adamw_ema_kernel.
__global__ __launch_bounds__(256) void lamb_moments_kernel(const vit_tensor_chunk* __restrict__ tab, float b1, float b2,
                                                           float c1, float c2, float wd, float gscale,
                                                           const float* __restrict__ clip,
                                                           double* __restrict__ partial) {
  if (!clip_enter(clip, &gscale)) return;
  lamb_moments_chunk(tab[blockIdx.x], b1, b2, c1, c2, wd, gscale, partial);
}

// One workgroup per tensor: its chunks are first[b] .. first[b + 1] - 1 of pass 1's table.  Thread i adds partials
// first + i, first + i + 256, ... in that order, then the fixed tree, as grad_clip_finish_kernel does, so a tensor
// of more than 256 chunks takes the same path.  trust[b] = |p| / |u| where `adapt` is set and both norms are positive,
// else 1; at most 1 with `trust_clip`.  The quotient is formed in fp64 and rounded to fp32 once.
VIT_DEV void lamb_trust_tensor(const double* __restrict__ partial, const int32_t* __restrict__ first, int adapt,
                               int trust_clip, float* __restrict__ trust) {
  __shared__ double red_p[4], red_u[4];
  const int64_t lo = first[blockIdx.x], hi = first[blockIdx.x + 1];
  double sp = 0.0, su = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    sp += partial[2 * i];
    su += partial[2 * i + 1];
  }
  sp = block_sum_f64(sp, red_p);
  su = block_sum_f64(su, red_u);
  if (threadIdx.x != 0) return;
  float r = 1.f;
  if (adapt && sp > 0.0 && su > 0.0) r = (float)(sqrt(sp) / sqrt(su));      // a NaN sum compares false: r stays 1
  if (trust_clip && r > 1.f) r = 1.f;
  trust[blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void lamb_trust_kernel(const double* __restrict__ partial,
                                                         const int32_t* __restrict__ first, int adapt, int trust_clip,
                                                         float* __restrict__ trust, const float* __restrict__ clip) {
  if (!clip_enter(clip)) return;
  lamb_trust_tensor(partial, first, adapt, trust_clip, trust);
}

// Pass 2, one workgroup per chunk: p -= (lr * trust[tensor of the chunk]) * u with u formed again by lamb_u, the
// shadow, and with EMA the recurrence of adamw_chunk's EMA form on the chunk's EMA slice.
template <class TS, bool EMA>
VIT_DEV void lamb_update_chunk(const vit_tensor_chunk ch, float step, float c1, float c2, float wd,
                               float* ema = nullptr, float ema_w = 0.f) {
  for (int64_t t = threadIdx.x; t < ch.n; t += 256) {
    const float m = ch.m[t], v = ch.v[t];
    float p = ch.p[t];
    float e = 0.f;
    if constexpr (EMA) e = ema[t];
    p = __builtin_fmaf(-step, lamb_u(m, v, p, c1, c2, wd), p);
    ch.p[t] = p;
    if constexpr (EMA) ema[t] = __builtin_fmaf(ema_w, p - e, e);
    if (ch.shadow) st1<TS>((TS*)ch.shadow + t, p);
  }
}

template <class TS>
__global__ __launch_bounds__(256) void lamb_update_kernel(const vit_tensor_chunk* __restrict__ tab,
                                                          float* const* __restrict__ ema,
                                                          const int32_t* __restrict__ tensor_of_chunk,
                                                          const float* __restrict__ trust, float lr, float c1,
                                                          float c2, float wd, float ema_w,
                                                          const float* __restrict__ clip) {
  if (!clip_enter(clip)) return;
  const vit_tensor_chunk ch = tab[blockIdx.x];
  const float step = lr * trust[tensor_of_chunk[blockIdx.x]];
  float* const ema_p = ema ? ema[blockIdx.x] : nullptr;
  if (ema_p) lamb_update_chunk<TS, true>(ch, step, c1, c2, wd, ema_p, ema_w);
  else lamb_update_chunk<TS, false>(ch, step, c1, c2, wd);
}

// ---------------------------------------------------------------------------------------------------------------
// Grouped steps (vit_hip.h "Grouped optimizer steps"): the kernels above with the launch scalars of up to
// VIT_OPT_MAX_GROUPS param groups in ONE launch.  The per-group factors, formed on the host by adamw_factors and
// lamb_factors as for a single group, travel by value in the kernel-argument segment (CsBatch above is the
// precedent), so a learning rate that changes every step costs no copy.  group_of_chunk[blockIdx.x] is made
// wave-uniform with readfirstlane before it indexes the struct: the factors then come by scalar loads from the kernel
// arguments, and the struct is never copied to private memory.  A chunk (or tensor) whose group index is not below
// `n` returns without touching anything.  The element arithmetic is the device functions above, called as the
// single-group kernels call them, so every chunk comes out bit for bit as from its group's own launch.
// ---------------------------------------------------------------------------------------------------------------
struct AdamwGroup {      // 32 bytes: one 8-dword scalar load
  float lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, pad;
};
struct AdamwGroups {
  AdamwGroup g[VIT_OPT_MAX_GROUPS];
  int n;
};
struct LambGroup {       // 32 bytes
  float lr, b1, b2, c1, c2, wd;
  int adapt, trust_clip;
};
struct LambGroups {
  LambGroup g[VIT_OPT_MAX_GROUPS];
  int n;
};

// adamw_kernel / adamw_clipped_kernel / adamw_ema_kernel in one: clip and ema may each be NULL.
template <class TS>
__global__ __launch_bounds__(256) void adamw_groups_kernel(const vit_tensor_chunk* __restrict__ tab,
                                                           float* const* __restrict__ ema,
                                                           const int32_t* __restrict__ group_of_chunk,
                                                           const AdamwGroups gs, float gscale, float ema_w,
                                                           const float* __restrict__ clip) {
  if (!clip_enter(clip, &gscale)) return;
  const unsigned gi = (unsigned)__builtin_amdgcn_readfirstlane(group_of_chunk[blockIdx.x]);
  if (gi >= (unsigned)gs.n) return;
  const AdamwGroup& h = gs.g[gi];
  const vit_tensor_chunk ch = tab[blockIdx.x];
  float* const ema_p = ema ? ema[blockIdx.x] : nullptr;
  if (!ema_p) {
    adamw_chunk<TS>(ch, h.lr, h.b1, h.b2, h.eps, h.wd, h.step_size, h.inv_sqrt_bc2, gscale);
    return;
  }
  adamw_chunk<TS, true>(ch, h.lr, h.b1, h.b2, h.eps, h.wd, h.step_size, h.inv_sqrt_bc2, gscale, ema_p, ema_w);
}

// lamb_moments_kernel with the group's factors.
__global__ __launch_bounds__(256) void lamb_moments_groups_kernel(const vit_tensor_chunk* __restrict__ tab,
                                                                  const int32_t* __restrict__ group_of_chunk,
                                                                  const LambGroups gs, float gscale,
                                                                  const float* __restrict__ clip,
                                                                  double* __restrict__ partial) {
  if (!clip_enter(clip, &gscale)) return;
  const unsigned gi = (unsigned)__builtin_amdgcn_readfirstlane(group_of_chunk[blockIdx.x]);
  if (gi >= (unsigned)gs.n) return;
  const LambGroup& h = gs.g[gi];
  lamb_moments_chunk(tab[blockIdx.x], h.b1, h.b2, h.c1, h.c2, h.wd, gscale, partial);
}

// lamb_trust_kernel with the flags of the tensor's group.
__global__ __launch_bounds__(256) void lamb_trust_groups_kernel(const double* __restrict__ partial,
                                                                const int32_t* __restrict__ first,
                                                                const int32_t* __restrict__ group_of_tensor,
                                                                const LambGroups gs, float* __restrict__ trust,
                                                                const float* __restrict__ clip) {
  if (!clip_enter(clip)) return;
  const unsigned gi = (unsigned)__builtin_amdgcn_readfirstlane(group_of_tensor[blockIdx.x]);
  if (gi >= (unsigned)gs.n) return;
  lamb_trust_tensor(partial, first, gs.g[gi].adapt, gs.g[gi].trust_clip, trust);
}

template <class TS>
__global__ __launch_bounds__(256) void lamb_update_groups_kernel(const vit_tensor_chunk* __restrict__ tab,
                                                                 float* const* __restrict__ ema,
                                                                 const int32_t* __restrict__ tensor_of_chunk,
                                                                 const float* __restrict__ trust,
                                                                 const int32_t* __restrict__ group_of_chunk,
                                                                 const LambGroups gs, float ema_w,
                                                                 const float* __restrict__ clip) {
  if (!clip_enter(clip)) return;
  const unsigned gi = (unsigned)__builtin_amdgcn_readfirstlane(group_of_chunk[blockIdx.x]);
  if (gi >= (unsigned)gs.n) return;
  const LambGroup& h = gs.g[gi];
  const vit_tensor_chunk ch = tab[blockIdx.x];
  const float step = h.lr * trust[tensor_of_chunk[blockIdx.x]];
  float* const ema_p = ema ? ema[blockIdx.x] : nullptr;
  if (ema_p) lamb_update_chunk<TS, true>(ch, step, h.c1, h.c2, h.wd, ema_p, ema_w);
  else lamb_update_chunk<TS, false>(ch, step, h.c1, h.c2, h.wd);
}

}  // namespace

// ===============================================================================================================
extern "C" int vit_im2col(const void* x, int32_t x_dtype, void* cols, int32_t dtype, int64_t B, int64_t C, int64_t H,
                          int64_t W, int64_t P, void* stream) {
  VIT_REQUIRE(x && cols, "vit_im2col: null pointer");
  VIT_REQUIRE(B > 0 && C > 0 && P > 0 && H % P == 0 && W % P == 0, "vit_im2col: image %lldx%lld not divisible by P=%lld",
              (long long)H, (long long)W, (long long)P);
  VIT_REQUIRE(P % 4 == 0, "vit_im2col: patch size must be a multiple of 4");
  const int64_t work = B * (H / P) * (W / P) * C * P * P / 4;
  const unsigned grid = grid_for(work, 256, 16384);
  hipStream_t s = VIT_STREAM(stream);
  if (x_dtype == VIT_F32 && dtype == VIT_BF16)
    im2col_kernel<float, bf16_t><<<grid, 256, 0, s>>>((const float*)x, (bf16_t*)cols, B, C, H, W, P);
  else if (x_dtype == VIT_F32 && dtype == VIT_F32)
    im2col_kernel<float, float><<<grid, 256, 0, s>>>((const float*)x, (float*)cols, B, C, H, W, P);
  else if (x_dtype == VIT_BF16 && dtype == VIT_BF16)
    im2col_kernel<bf16_t, bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)x, (bf16_t*)cols, B, C, H, W, P);
  else {
    vit::set_error("vit_im2col: unsupported dtype pair %d->%d", x_dtype, dtype);
    return VIT_ERR_INVALID;
  }
  return vit::check_launch("vit_im2col");
}

extern "C" int vit_col2im(const void* cols, int32_t dtype, void* x, int32_t x_dtype, int64_t B, int64_t C,
                          int64_t H, int64_t W, int64_t P, void* stream) {
  VIT_REQUIRE(x && cols, "vit_col2im: null pointer");
  VIT_REQUIRE(B > 0 && C > 0 && P > 0 && H % P == 0 && W % P == 0, "vit_col2im: image %lldx%lld not divisible by P=%lld",
              (long long)H, (long long)W, (long long)P);
  const unsigned grid = grid_for(B * C * H * W, 256, 16384);
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_BF16 && x_dtype == VIT_F32)
    col2im_kernel<bf16_t, float><<<grid, 256, 0, s>>>((const bf16_t*)cols, (float*)x, B, C, H, W, P);
  else if (dtype == VIT_F32 && x_dtype == VIT_F32)
    col2im_kernel<float, float><<<grid, 256, 0, s>>>((const float*)cols, (float*)x, B, C, H, W, P);
  else if (dtype == VIT_BF16 && x_dtype == VIT_BF16)
    col2im_kernel<bf16_t, bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)cols, (bf16_t*)x, B, C, H, W, P);
  else {
    vit::set_error("vit_col2im: unsupported dtype pair %d->%d", dtype, x_dtype);
    return VIT_ERR_INVALID;
  }
  return vit::check_launch("vit_col2im");
}

extern "C" int vit_embed_cls(const float* cls, const float* pos, void* x0, int32_t dtype, int64_t B, int64_t T,
                             int64_t D, void* stream) {
  VIT_REQUIRE(cls && pos && x0 && B > 0 && T > 0 && D > 0, "vit_embed_cls: bad arguments");
  const unsigned grid = grid_for(B * D, 256);
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_BF16) embed_cls_kernel<bf16_t><<<grid, 256, 0, s>>>(cls, pos, (bf16_t*)x0, B, T, D);
  else embed_cls_kernel<float><<<grid, 256, 0, s>>>(cls, pos, (float*)x0, B, T, D);
  return vit::check_launch("vit_embed_cls");
}

namespace vit {
void colsum_parts_launch(const void* x, int64_t ldx, int dtype, int64_t rows, int64_t cols, int64_t rows_per_chunk,
                         float* part, hipStream_t s) {
  const int64_t ch = (rows + rows_per_chunk - 1) / rows_per_chunk;
  const int vec = (cols % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)x) % 16 == 0);
  dim3 g1((unsigned)((cols + 255) / 256), (unsigned)ch);
  if (dtype == VIT_BF16)
    colsum_stage1<bf16_t><<<g1, 256, 0, s>>>((const bf16_t*)x, ldx, rows, cols, rows_per_chunk, part, vec);
  else
    colsum_stage1<float><<<g1, 256, 0, s>>>((const float*)x, ldx, rows, cols, rows_per_chunk, part, vec);
}
}  // namespace vit

extern "C" int64_t vit_colsum_workspace_bytes(int64_t rows, int64_t cols) {
  return colsum_chunks(rows, cols) * cols * (int64_t)sizeof(float);
}

extern "C" int vit_colsum(const void* x, int64_t ldx, int32_t dtype, int64_t rows, int64_t cols, float* out,
                          float alpha, float beta, void* workspace, void* stream) {
  VIT_REQUIRE(x && out && workspace && rows > 0 && cols > 0, "vit_colsum: bad arguments");
  const int64_t ch = colsum_chunks(rows, cols);
  const int64_t rpc = (rows + ch - 1) / ch;
  const int vec = (cols % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)x) % 16 == 0);
  dim3 g1((unsigned)((cols + 255) / 256), (unsigned)ch);
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_BF16)
    colsum_stage1<bf16_t><<<g1, 256, 0, s>>>((const bf16_t*)x, ldx, rows, cols, rpc, (float*)workspace, vec, alpha);
  else
    colsum_stage1<float><<<g1, 256, 0, s>>>((const float*)x, ldx, rows, cols, rpc, (float*)workspace, vec, alpha);
  OutSet outs{{out, nullptr, nullptr}};
  colsum_stage2<<<(unsigned)((cols + 63) / 64), 64 * CS2_WAVES, 0, s>>>((const float*)workspace, ch, cols, outs, beta);
  return vit::check_launch("vit_colsum");
}

extern "C" int vit_colsum_finish(const float* part, int64_t nparts, int64_t cols, int32_t nsets, float* out0,
                                 float* out1, float* out2, float beta, void* stream) {
  VIT_REQUIRE(part && nparts > 0 && cols > 0 && nsets >= 1 && nsets <= 3, "vit_colsum_finish: bad arguments");
  OutSet outs{{out0, out1, out2}};
  for (int i = 0; i < nsets; ++i) VIT_REQUIRE(outs.p[i] != nullptr, "vit_colsum_finish: output %d is NULL", i);
  dim3 grid((unsigned)((cols + 63) / 64), (unsigned)nsets);
  colsum_stage2<<<grid, 64 * CS2_WAVES, 0, VIT_STREAM(stream)>>>(part, nparts, cols, outs, beta);
  return vit::check_launch("vit_colsum_finish");
}

extern "C" int vit_colsum_finish_batch(const vit_colsum_job* jobs, int32_t njobs, void* stream) {
  VIT_REQUIRE(jobs && njobs >= 1 && njobs <= CS_BATCH_MAX, "vit_colsum_finish_batch: 1..%d jobs", CS_BATCH_MAX);
  CsBatch tab{};
  tab.n = njobs;
  tab.first[0] = 0;
  for (int j = 0; j < njobs; ++j) {
    const vit_colsum_job& jb = jobs[j];
    VIT_REQUIRE(jb.part && jb.nparts > 0 && jb.cols > 0 && jb.nsets >= 1 && jb.nsets <= 3,
                "vit_colsum_finish_batch: bad job %d", j);
    for (int i = 0; i < jb.nsets; ++i)
      VIT_REQUIRE(jb.out[i] != nullptr, "vit_colsum_finish_batch: job %d output %d is NULL", j, i);
    tab.job[j] = jb;
    tab.first[j + 1] = tab.first[j] + jb.nsets * ((jb.cols + 63) / 64);
  }
  colsum_stage2_batch<<<(unsigned)tab.first[njobs], 64 * CS2_WAVES, 0, VIT_STREAM(stream)>>>(tab);
  return vit::check_launch("vit_colsum_finish_batch");
}

extern "C" int vit_copy2d(const void* src, int64_t lds, int32_t src_dtype, void* dst, int64_t ldd, int32_t dst_dtype,
                          int64_t rows, int64_t cols, int64_t src_group_rows, int64_t src_group_stride, float beta,
                          void* stream) {
  VIT_REQUIRE(src && dst && rows > 0 && cols > 0, "vit_copy2d: bad arguments");
  hipStream_t s = VIT_STREAM(stream);
  const int64_t es = src_dtype == VIT_F32 ? 4 : 2;
  if (src_dtype == dst_dtype && beta == 0.f && (cols * es) % 16 == 0 && (lds * es) % 16 == 0 && (ldd * es) % 16 == 0 &&
      ((uintptr_t)src | (uintptr_t)dst) % 16 == 0) {
    const int64_t cpr = cols * es / 16;
    copy2d_raw16_kernel<<<grid_for(rows * cpr, 256, 16384), 256, 0, s>>>(
        (const uint8_t*)src, lds * es, (uint8_t*)dst, ldd * es, rows, cpr, src_group_rows, src_group_stride);
    return vit::check_launch("vit_copy2d");
  }
  const unsigned grid = grid_for(rows * cols, 256, 16384);
#define CP(TS, TD)                                                                                            \
  copy2d_kernel<TS, TD><<<grid, 256, 0, s>>>((const TS*)src, lds, (TD*)dst, ldd, rows, cols, src_group_rows, \
                                             src_group_stride, beta)
  if (src_dtype == VIT_F32 && dst_dtype == VIT_F32) CP(float, float);
  else if (src_dtype == VIT_F32) CP(float, bf16_t);
  else if (dst_dtype == VIT_F32) CP(bf16_t, float);
  else CP(bf16_t, bf16_t);
#undef CP
  return vit::check_launch("vit_copy2d");
}

extern "C" int vit_dropout_bwd(const void* x, void* y, int32_t dtype, int64_t n, float p, uint32_t seed, float scale,
                               void* stream) {
  VIT_REQUIRE(x && y && n > 0 && p >= 0.f && p < 1.f, "vit_dropout_bwd: bad arguments");
  const uint32_t thr = vit_drop_threshold(p);
  const unsigned grid = grid_for(n, 256, 16384);
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_BF16) dropout_bwd_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)x, (bf16_t*)y, n, thr, scale, seed);
  else dropout_bwd_kernel<float><<<grid, 256, 0, s>>>((const float*)x, (float*)y, n, thr, scale, seed);
  return vit::check_launch("vit_dropout_bwd");
}

extern "C" int vit_mask4_apply(const void* x, int64_t ldx, int32_t x_dtype, void* y, int64_t ldy, int32_t y_dtype,
                               const void* mask, int64_t rows, int64_t cols, float scale, void* stream) {
  VIT_REQUIRE(x && y && mask && rows > 0 && cols > 0, "vit_mask4_apply: bad arguments");
  VIT_REQUIRE(cols % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0, "vit_mask4_apply: cols/ld must be multiples of 4");
  const unsigned grid = grid_for(rows * (cols / 4), 256, 16384);
  hipStream_t s = VIT_STREAM(stream);
  const uint8_t* m = (const uint8_t*)mask;
#define MA(TI, TO) mask4_apply_kernel<TI, TO><<<grid, 256, 0, s>>>((const TI*)x, ldx, (TO*)y, ldy, m, rows, cols, scale)
  if (x_dtype == VIT_BF16 && y_dtype == VIT_BF16) MA(bf16_t, bf16_t);
  else if (x_dtype == VIT_BF16) MA(bf16_t, float);
  else if (y_dtype == VIT_BF16) MA(float, bf16_t);
  else MA(float, float);
#undef MA
  return vit::check_launch("vit_mask4_apply");
}

extern "C" int vit_drop_path_rows(float* out, uint32_t seed, int64_t L, int64_t B, int64_t T, const float* rates,
                                  void* stream) {
  VIT_REQUIRE(out && rates, "vit_drop_path_rows: null pointer");
  VIT_REQUIRE(L > 0 && B > 0 && T > 0, "vit_drop_path_rows: bad sizes L=%lld B=%lld T=%lld", (long long)L, (long long)B,
              (long long)T);
  VIT_REQUIRE(L <= VIT_DROP_PATH_MAX_LAYERS, "vit_drop_path_rows: L=%lld exceeds VIT_DROP_PATH_MAX_LAYERS=%d",
              (long long)L, VIT_DROP_PATH_MAX_LAYERS);
  VIT_REQUIRE(B < (1LL << 31) && T < (1LL << 31) && B * T < (1LL << 31), "vit_drop_path_rows: B * T must be below 2^31");
  DropPathTab tab{};
  for (int64_t l = 0; l < L; ++l) {
    const float p = rates[l];
    VIT_REQUIRE(p >= 0.f && p < 1.f, "vit_drop_path_rows: rate %g of layer %lld outside [0, 1)", (double)p, (long long)l);
    tab.thr[l] = vit_drop_threshold(p);
    tab.scale[l] = 1.0f / (1.0f - p);
  }
  const dim3 grid(grid_for(B * T, 256, 1024), (unsigned)(2 * L));
  drop_path_rows_kernel<<<grid, 256, 0, VIT_STREAM(stream)>>>(out, seed, (uint32_t)L, (uint32_t)(B * T), (uint32_t)T, tab);
  return vit::check_launch("vit_drop_path_rows");
}

extern "C" int vit_relu_bwd(const void* dy, const void* y, void* dx, int32_t dtype, int64_t n, void* stream) {
  VIT_REQUIRE(dy && y && dx && n > 0, "vit_relu_bwd: bad arguments");
  const unsigned grid = grid_for(n, 256, 16384);
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_BF16) relu_bwd_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)dy, (const bf16_t*)y, (bf16_t*)dx, n);
  else relu_bwd_kernel<float><<<grid, 256, 0, s>>>((const float*)dy, (const float*)y, (float*)dx, n);
  return vit::check_launch("vit_relu_bwd");
}

extern "C" int vit_gelu_fwd(const float* x, float* y, int64_t n, void* stream) {
  VIT_REQUIRE(x && y && n > 0, "vit_gelu_fwd: bad arguments");
  gelu_fwd_kernel<<<grid_for(n, 256), 256, 0, VIT_STREAM(stream)>>>(x, y, n);
  return vit::check_launch("vit_gelu_fwd");
}

extern "C" int vit_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) {
  VIT_REQUIRE(x && dy && dx && n > 0, "vit_gelu_bwd: bad arguments");
  gelu_bwd_kernel<<<grid_for(n, 256), 256, 0, VIT_STREAM(stream)>>>(x, dy, dx, n);
  return vit::check_launch("vit_gelu_bwd");
}

extern "C" int vit_softmax_xent(const float* logits, const int64_t* labels, int64_t rows, int64_t classes, float* loss,
                                float* dlogits, float* workspace, void* stream) {
  VIT_REQUIRE(logits && labels && loss && dlogits && workspace && rows > 0 && classes > 0,
              "vit_softmax_xent: bad arguments");
  hipStream_t s = VIT_STREAM(stream);
  const float inv = 1.0f / (float)rows;
  xent_rows_kernel<<<(unsigned)rows, 256, 0, s>>>(logits, labels, classes, inv, dlogits, workspace);
  xent_reduce_kernel<<<1, 256, 0, s>>>(workspace, rows, inv, loss);
  return vit::check_launch("vit_softmax_xent");
}

extern "C" int vit_softmax_xent_mixed(const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                                      const float* lam, float smoothing, int64_t rows, int64_t classes, float* loss,
                                      float* dlogits, float* workspace, void* stream) {
  VIT_REQUIRE(logits && labels_a && loss && dlogits && workspace, "vit_softmax_xent_mixed: null pointer");
  VIT_REQUIRE(rows > 0 && classes > 0, "vit_softmax_xent_mixed: rows and classes must be positive (got %lld, %lld)",
              (long long)rows, (long long)classes);
  VIT_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "vit_softmax_xent_mixed: smoothing must lie in [0, 1) (got %g)",
              (double)smoothing);
  VIT_REQUIRE(!lam || labels_b, "vit_softmax_xent_mixed: lam given without labels_b");
  VIT_REQUIRE(rows <= 0x7fffffff, "vit_softmax_xent_mixed: too many rows for one grid (%lld)", (long long)rows);
  hipStream_t s = VIT_STREAM(stream);
  const float inv = 1.0f / (float)rows;
  xent_mixed_rows_kernel<<<(unsigned)rows, 256, 0, s>>>(logits, labels_a, labels_b, lam, smoothing, classes, inv,
                                                        dlogits, workspace);
  xent_reduce_kernel<<<1, 256, 0, s>>>(workspace, rows, inv, loss);
  return vit::check_launch("vit_softmax_xent_mixed");
}

// Host side of the chunk-table launchers.  The two factors the AdamW kernels take in place of the bias corrections:
// the one place that forms them, for the single-group entry points and for each group of vit_adamw_groups.
static void adamw_factors(float lr, float bias_corr1, float bias_corr2, float* step_size, float* inv_sqrt_bc2) {
  *step_size = lr / bias_corr1;
  *inv_sqrt_bc2 = 1.0f / sqrtf(bias_corr2);
}

// What the three single-group AdamW entry points check alike, reported under the name `who` of the one that was called
// (`ptrs`: every pointer it cannot do without is set), then adamw_factors.
static int adamw_args(const char* who, bool ptrs, int64_t nchunks, float lr, float bias_corr1, float bias_corr2,
                      float* step_size, float* inv_sqrt_bc2) {
  VIT_REQUIRE(ptrs && nchunks > 0 && bias_corr1 > 0.f && bias_corr2 > 0.f, "%s: bad arguments", who);
  adamw_factors(lr, bias_corr1, bias_corr2, step_size, inv_sqrt_bc2);
  return VIT_OK;
}

// The EMA weight of the entry point `who`, where it keeps an EMA at all (`used`).
static int check_ema_weight(const char* who, bool used, float ema_weight) {
  VIT_REQUIRE(!used || (ema_weight > 0.f && ema_weight < 1.f), "%s: ema_weight must lie in (0, 1) (got %g)", who,
              (double)ema_weight);
  return VIT_OK;
}

// KERNEL<shadow dtype>, one 256-thread workgroup per chunk of the table: bf16 shadows, or fp32 for any other code.
// Reads the entry point's own `shadow_dtype`, `nchunks` and `stream`.
#define TABLE_LAUNCH(KERNEL, ...)                                                                                \
  if (shadow_dtype == VIT_BF16) KERNEL<bf16_t><<<(unsigned)nchunks, 256, 0, VIT_STREAM(stream)>>>(__VA_ARGS__); \
  else KERNEL<float><<<(unsigned)nchunks, 256, 0, VIT_STREAM(stream)>>>(__VA_ARGS__)

extern "C" int vit_adamw(const vit_tensor_chunk* table_dev, int64_t nchunks, float lr, float beta1, float beta2,
                         float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                         int32_t shadow_dtype, void* stream) {
  float step_size, inv_sqrt_bc2;
  if (int rc = adamw_args("vit_adamw", table_dev, nchunks, lr, bias_corr1, bias_corr2, &step_size, &inv_sqrt_bc2))
    return rc;
  TABLE_LAUNCH(adamw_kernel, table_dev, lr, beta1, beta2, eps, weight_decay, step_size, inv_sqrt_bc2, grad_scale);
  return vit::check_launch("vit_adamw");
}

extern "C" int vit_grad_sumsq(const vit_tensor_chunk* table_dev, int64_t nchunks, float grad_scale, double* partial,
                              void* stream) {
  VIT_REQUIRE(table_dev && partial && nchunks > 0, "vit_grad_sumsq: bad arguments");
  grad_sumsq_kernel<<<(unsigned)nchunks, 256, 0, VIT_STREAM(stream)>>>(table_dev, grad_scale, partial);
  return vit::check_launch("vit_grad_sumsq");
}

extern "C" int vit_grad_clip_finish(const double* partial, int64_t nparts, float max_norm, float* clip,
                                    void* stream) {
  VIT_REQUIRE(partial && clip && nparts > 0, "vit_grad_clip_finish: bad arguments");
  VIT_REQUIRE(max_norm < 0.f || max_norm > 0.f, "vit_grad_clip_finish: max_norm must be nonzero (got %g)",
              (double)max_norm);
  grad_clip_finish_kernel<<<1, 256, 0, VIT_STREAM(stream)>>>(partial, nparts, max_norm, clip);
  return vit::check_launch("vit_grad_clip_finish");
}

extern "C" int vit_adamw_clipped(const vit_tensor_chunk* table_dev, int64_t nchunks, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                                 float grad_scale, int32_t shadow_dtype, const float* clip, void* stream) {
  float step_size, inv_sqrt_bc2;
  if (int rc = adamw_args("vit_adamw_clipped", table_dev && clip, nchunks, lr, bias_corr1, bias_corr2, &step_size,
                          &inv_sqrt_bc2))
    return rc;
  TABLE_LAUNCH(adamw_clipped_kernel, table_dev, lr, beta1, beta2, eps, weight_decay, step_size, inv_sqrt_bc2,
               grad_scale, clip);
  return vit::check_launch("vit_adamw_clipped");
}

extern "C" int vit_adamw_ema(const vit_tensor_chunk* table_dev, float* const* ema_dev, int64_t nchunks, float lr,
                             float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                             float bias_corr2, float grad_scale, int32_t shadow_dtype, float ema_weight,
                             const float* clip, void* stream) {
  float step_size, inv_sqrt_bc2;
  if (int rc = adamw_args("vit_adamw_ema", table_dev && ema_dev, nchunks, lr, bias_corr1, bias_corr2, &step_size,
                          &inv_sqrt_bc2))
    return rc;
  if (int rc = check_ema_weight("vit_adamw_ema", true, ema_weight)) return rc;
  TABLE_LAUNCH(adamw_ema_kernel, table_dev, ema_dev, lr, beta1, beta2, eps, weight_decay, step_size, inv_sqrt_bc2,
               grad_scale, ema_weight, clip);
  return vit::check_launch("vit_adamw_ema");
}

extern "C" int vit_ema_swap(const vit_tensor_chunk* table_dev, float* const* ema_dev, int64_t nchunks,
                            int32_t shadow_dtype, void* stream) {
  VIT_REQUIRE(table_dev && ema_dev && nchunks > 0, "vit_ema_swap: bad arguments");
  TABLE_LAUNCH(ema_swap_kernel, table_dev, ema_dev);
  return vit::check_launch("vit_ema_swap");
}

// The two constants lamb_u takes in place of the bias corrections, formed in double and rounded once each: the one
// place that forms them, for vit_lamb_moments / vit_lamb_update and for each group of their grouped forms.
static void lamb_factors(float eps, float bias_corr1, float bias_corr2, float* c1, float* c2) {
  *c1 = (float)((double)bias_corr1 / sqrt((double)bias_corr2));
  *c2 = (float)((double)bias_corr1 * (double)eps);
}

// What vit_lamb_moments and vit_lamb_update check alike, then lamb_factors.
static int lamb_args(const char* who, bool ptrs, int64_t nchunks, float eps, float bias_corr1, float bias_corr2,
                     float* c1, float* c2) {
  VIT_REQUIRE(ptrs, "%s: null pointer", who);
  VIT_REQUIRE(nchunks > 0 && nchunks <= 0x3fffffff, "%s: nchunks must be positive (got %lld)", who,
              (long long)nchunks);
  VIT_REQUIRE(bias_corr1 > 0.f && bias_corr1 <= 1.f && bias_corr2 > 0.f && bias_corr2 <= 1.f,
              "%s: bias corrections must lie in (0, 1] (got %g, %g)", who, (double)bias_corr1, (double)bias_corr2);
  VIT_REQUIRE(eps >= 0.f, "%s: eps must not be negative (got %g)", who, (double)eps);
  lamb_factors(eps, bias_corr1, bias_corr2, c1, c2);
  return VIT_OK;
}

extern "C" int vit_lamb_moments(const vit_tensor_chunk* table_dev, int64_t nchunks, float beta1, float beta2,
                                float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                                const float* clip, double* partial, void* stream) {
  float c1, c2;
  if (int rc = lamb_args("vit_lamb_moments", table_dev && partial, nchunks, eps, bias_corr1, bias_corr2, &c1, &c2))
    return rc;
  lamb_moments_kernel<<<(unsigned)nchunks, 256, 0, VIT_STREAM(stream)>>>(table_dev, beta1, beta2, c1, c2, weight_decay,
                                                                         grad_scale, clip, partial);
  return vit::check_launch("vit_lamb_moments");
}

extern "C" int vit_lamb_trust(const double* partial, const int32_t* tensor_first, int64_t ntensors, int32_t adapt,
                              int32_t trust_clip, float* trust, const float* clip, void* stream) {
  VIT_REQUIRE(partial && tensor_first && trust, "vit_lamb_trust: null pointer");
  VIT_REQUIRE(ntensors > 0 && ntensors <= 0x3fffffff, "vit_lamb_trust: ntensors must be positive (got %lld)",
              (long long)ntensors);
  lamb_trust_kernel<<<(unsigned)ntensors, 256, 0, VIT_STREAM(stream)>>>(partial, tensor_first, adapt != 0,
                                                                        trust_clip != 0, trust, clip);
  return vit::check_launch("vit_lamb_trust");
}

extern "C" int vit_lamb_update(const vit_tensor_chunk* table_dev, float* const* ema_dev,
                               const int32_t* tensor_of_chunk, const float* trust, int64_t nchunks, float lr,
                               float eps, float weight_decay, float bias_corr1, float bias_corr2,
                               int32_t shadow_dtype, float ema_weight, const float* clip, void* stream) {
  float c1, c2;
  if (int rc = lamb_args("vit_lamb_update", table_dev && tensor_of_chunk && trust, nchunks, eps, bias_corr1,
                         bias_corr2, &c1, &c2))
    return rc;
  if (int rc = check_ema_weight("vit_lamb_update", ema_dev, ema_weight)) return rc;
  TABLE_LAUNCH(lamb_update_kernel, table_dev, ema_dev, tensor_of_chunk, trust, lr, c1, c2, weight_decay, ema_weight,
               clip);
  return vit::check_launch("vit_lamb_update");
}

extern "C" int vit_pack(const vit_tensor_chunk* table_dev, int64_t nchunks, int32_t shadow_dtype, void* stream) {
  VIT_REQUIRE(table_dev && nchunks > 0, "vit_pack: bad arguments");
  TABLE_LAUNCH(pack_kernel, table_dev);
  return vit::check_launch("vit_pack");
}

// What the four grouped entry points check alike, under the name `who` of the one that was called (`lamb`: the LAMB
// flags are allowed).  `count` is nchunks, or ntensors for the trust pass.
static int check_opt_groups(const char* who, bool ptrs, int64_t count, const vit_opt_group* groups, int32_t ngroups,
                            bool lamb) {
  VIT_REQUIRE(ptrs && groups, "%s: null pointer", who);
  VIT_REQUIRE(count > 0 && count <= 0x3fffffff, "%s: the chunk / tensor count must be positive (got %lld)", who,
              (long long)count);
  VIT_REQUIRE(ngroups >= 1 && ngroups <= VIT_OPT_MAX_GROUPS, "%s: ngroups must lie in 1..%d (got %d)", who,
              VIT_OPT_MAX_GROUPS, (int)ngroups);
  for (int32_t i = 0; i < ngroups; ++i) {
    const vit_opt_group& g = groups[i];
    VIT_REQUIRE(g.bias_corr1 > 0.f && g.bias_corr1 <= 1.f && g.bias_corr2 > 0.f && g.bias_corr2 <= 1.f,
                "%s: group %d: bias corrections must lie in (0, 1] (got %g, %g)", who, (int)i, (double)g.bias_corr1,
                (double)g.bias_corr2);
    VIT_REQUIRE(g.eps >= 0.f, "%s: group %d: eps must not be negative (got %g)", who, (int)i, (double)g.eps);
    VIT_REQUIRE(fabsf(g.lr) <= 3.402823466e+38f, "%s: group %d: lr must be finite (got %g)", who, (int)i,
                (double)g.lr);
    if (lamb)
      VIT_REQUIRE((g.flags & ~(VIT_OPT_ADAPT | VIT_OPT_TRUST_CLIP)) == 0, "%s: group %d: unknown flags 0x%x", who,
                  (int)i, (unsigned)g.flags);
    else
      VIT_REQUIRE(g.flags == 0, "%s: group %d: flags must be 0 for AdamW (got 0x%x)", who, (int)i,
                  (unsigned)g.flags);
  }
  return VIT_OK;
}

// The kernel-argument struct of the LAMB passes, c1 and c2 per group by lamb_factors.
static int lamb_group_args(const char* who, bool ptrs, int64_t count, const vit_opt_group* groups, int32_t ngroups,
                           LambGroups* out) {
  if (int rc = check_opt_groups(who, ptrs, count, groups, ngroups, true)) return rc;
  memset(out, 0, sizeof(*out));
  out->n = ngroups;
  for (int32_t i = 0; i < ngroups; ++i) {
    const vit_opt_group& g = groups[i];
    LambGroup& h = out->g[i];
    h.lr = g.lr, h.b1 = g.beta1, h.b2 = g.beta2, h.wd = g.weight_decay;
    lamb_factors(g.eps, g.bias_corr1, g.bias_corr2, &h.c1, &h.c2);
    h.adapt = (g.flags & VIT_OPT_ADAPT) != 0, h.trust_clip = (g.flags & VIT_OPT_TRUST_CLIP) != 0;
  }
  return VIT_OK;
}

extern "C" int vit_adamw_groups(const vit_tensor_chunk* table_dev, float* const* ema_dev,
                                const int32_t* group_of_chunk, int64_t nchunks, const vit_opt_group* groups,
                                int32_t ngroups, float grad_scale, int32_t shadow_dtype, float ema_weight,
                                const float* clip, void* stream) {
  if (int rc = check_opt_groups("vit_adamw_groups", table_dev && group_of_chunk, nchunks, groups, ngroups, false))
    return rc;
  if (int rc = check_ema_weight("vit_adamw_groups", ema_dev, ema_weight)) return rc;
  AdamwGroups gs;
  memset(&gs, 0, sizeof(gs));
  gs.n = ngroups;
  for (int32_t i = 0; i < ngroups; ++i) {
    const vit_opt_group& g = groups[i];
    AdamwGroup& h = gs.g[i];
    h.lr = g.lr, h.b1 = g.beta1, h.b2 = g.beta2, h.eps = g.eps, h.wd = g.weight_decay;
    adamw_factors(g.lr, g.bias_corr1, g.bias_corr2, &h.step_size, &h.inv_sqrt_bc2);
  }
  TABLE_LAUNCH(adamw_groups_kernel, table_dev, ema_dev, group_of_chunk, gs, grad_scale, ema_weight, clip);
  return vit::check_launch("vit_adamw_groups");
}

extern "C" int vit_lamb_moments_groups(const vit_tensor_chunk* table_dev, const int32_t* group_of_chunk,
                                       int64_t nchunks, const vit_opt_group* groups, int32_t ngroups,
                                       float grad_scale, const float* clip, double* partial, void* stream) {
  LambGroups gs;
  if (int rc = lamb_group_args("vit_lamb_moments_groups", table_dev && group_of_chunk && partial, nchunks, groups,
                               ngroups, &gs))
    return rc;
  lamb_moments_groups_kernel<<<(unsigned)nchunks, 256, 0, VIT_STREAM(stream)>>>(table_dev, group_of_chunk, gs,
                                                                                grad_scale, clip, partial);
  return vit::check_launch("vit_lamb_moments_groups");
}

extern "C" int vit_lamb_trust_groups(const double* partial, const int32_t* tensor_first,
                                     const int32_t* group_of_tensor, int64_t ntensors, const vit_opt_group* groups,
                                     int32_t ngroups, float* trust, const float* clip, void* stream) {
  LambGroups gs;
  if (int rc = lamb_group_args("vit_lamb_trust_groups", partial && tensor_first && group_of_tensor && trust, ntensors,
                               groups, ngroups, &gs))
    return rc;
  lamb_trust_groups_kernel<<<(unsigned)ntensors, 256, 0, VIT_STREAM(stream)>>>(partial, tensor_first, group_of_tensor,
                                                                               gs, trust, clip);
  return vit::check_launch("vit_lamb_trust_groups");
}

extern "C" int vit_lamb_update_groups(const vit_tensor_chunk* table_dev, float* const* ema_dev,
                                      const int32_t* tensor_of_chunk, const float* trust,
                                      const int32_t* group_of_chunk, int64_t nchunks, const vit_opt_group* groups,
                                      int32_t ngroups, int32_t shadow_dtype, float ema_weight, const float* clip,
                                      void* stream) {
  LambGroups gs;
  if (int rc = lamb_group_args("vit_lamb_update_groups", table_dev && tensor_of_chunk && trust && group_of_chunk,
                               nchunks, groups, ngroups, &gs))
    return rc;
  if (int rc = check_ema_weight("vit_lamb_update_groups", ema_dev, ema_weight)) return rc;
  TABLE_LAUNCH(lamb_update_groups_kernel, table_dev, ema_dev, tensor_of_chunk, trust, group_of_chunk, gs, ema_weight,
               clip);
  return vit::check_launch("vit_lamb_update_groups");
}
#undef TABLE_LAUNCH
