// Knowledge distillation loss (vit_hip.h "vit_softmax_xent_distill"): the smoothed two-label cross entropy of
// vit_softmax_xent_mixed and a teacher term, soft (Hinton: tau^2 * KL(softmax(z / tau) || softmax(x / tau))) or hard
// (cross entropy against the teacher's arg max), blended by alpha, with the gradient row written in the same pass:
//   loss = mean_r((1 - alpha) * base_r + alpha * d_r),   dlogits_r = ((1 - alpha) * (p - t) + alpha * g_r) / rows.
// The reduction over the rows is "batchmean": F.kl_div(log_softmax(x / tau), log_softmax(z / tau),
// reduction="batchmean", log_target=True) * tau^2.  DeiT's own script calls F.kl_div with reduction="sum" and divides
// by rows * classes instead, which weighs the teacher term 1 / classes as much; a caller who wants that weighting
// scales alpha.
//
// One 256-thread workgroup per row, as xent_rows_kernel / xent_mixed_rows_kernel (vit_misc.hip): a pass for the two
// row maxima, one for the sums, one for the gradient row; the row loss goes to the workspace and a fixed-order
// reduce forms the scalar.  No atomics: bitwise repeatable.  Nothing of shape [rows, classes] but dlogits is written.
// The base term keeps the mixed kernel's expressions for p, t and the row loss (same __expf / __logf, same order), so
// alpha = 0 reproduces that kernel bit for bit.
#include <math.h>

#include "vit_common.h"

namespace {

// sum over the workgroup of up to N values per thread, in the order of the sibling kernels: wave_sum, then
// ((w0 + w1) + w2) + w3.  One barrier pair for all N.
template <int N>
VIT_DEV void block_sums(float (&v)[N], float (*red)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float s = wave_sum(v[k]);
    if (lane == 0) red[k][w] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
  __syncthreads();
}

VIT_DEV float block_max(float v, float (*red)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_max(v);
  if (lane == 0) red[0][w] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  __syncthreads();
  return v;
}

// (value, index) arg max over the workgroup, the lower index winning ties.  NaN values never win (every comparison
// with one is false); the caller flags them separately.
VIT_DEV void argmax_take(float& v, long long& i, float ov, long long oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}
VIT_DEV long long block_argmax(float v, long long i, float (*red)[4], long long* redi) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const long long oi = __shfl_xor(i, o, 64);
    argmax_take(v, i, ov, oi);
  }
  if (lane == 0) {
    red[0][w] = v;
    redi[w] = i;
  }
  __syncthreads();
  v = red[0][0];
  i = redi[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) argmax_take(v, i, red[0][k], redi[k]);
  __syncthreads();
  return i;
}

// KIND: VIT_DISTILL_SOFT / VIT_DISTILL_HARD.  x: the student's row, z: the teacher's.
template <int KIND>
__global__ __launch_bounds__(256) void xent_distill_rows_kernel(
    const float* __restrict__ logits, const float* __restrict__ teacher, const int64_t* __restrict__ labels_a,
    const int64_t* __restrict__ labels_b, const float* __restrict__ lam, float smoothing, float alpha, float tau,
    float inv_tau, int64_t classes, float inv_rows, float* __restrict__ dlogits, float* __restrict__ row_loss) {
  __shared__ float red[5][4];
  __shared__ long long redi[4];
  const int64_t r = blockIdx.x;
  const float* x = logits + r * classes;
  const float* z = teacher + r * classes;
  const int tid = threadIdx.x;

  // pass 1: the student's maximum; the teacher's maximum (soft) or its lowest arg max (hard)
  float mx = -INFINITY, mz = -INFINITY;
  long long yhat = -1;
  bool znan = false;
  {
    float bad = 0.f;
    long long iz = classes;
    for (int64_t c = tid; c < classes; c += 256) {
      mx = fmaxf(mx, x[c]);
      const float zc = z[c];
      if constexpr (KIND == VIT_DISTILL_HARD) {
        if (zc > mz) {            // strict: ascending c keeps the thread's lowest index
          mz = zc;
          iz = c;
        }
        if (zc != zc) bad = NAN;
      } else {
        mz = fmaxf(mz, zc);
      }
    }
    mx = block_max(mx, red);
    if constexpr (KIND == VIT_DISTILL_HARD) {
      yhat = block_argmax(mz, iz, red, redi);
      float b[1] = {bad};
      block_sums<1>(b, red);
      znan = b[0] != b[0];
      if (znan || yhat >= classes) yhat = -1;             // no arg max: NaN row below, and no read through yhat
    } else {
      mz = block_max(mz, red);
    }
  }

  // pass 2: the sums.  s, zs: the mixed kernel's sum exp(x - mx) and sum (x - mx).  Soft: sx = sum e^{dx / tau},
  // sz = sum e^{dz / tau}, a = sum e^{dz / tau} * (dz - dx), with dx = x - mx and dz = z - mz: both maxima cancel in
  // KL = a / (tau * sz) - log sz + log sx.
  float s = 0.f, zs = 0.f, sx = 0.f, sz = 0.f, a = 0.f;
  for (int64_t c = tid; c < classes; c += 256) {
    const float d = x[c] - mx;
    s += __expf(d);
    zs += d;
    if constexpr (KIND == VIT_DISTILL_SOFT) {
      const float dz = z[c] - mz;
      const float ez = __expf(dz * inv_tau);
      sx += __expf(d * inv_tau);
      sz += ez;
      a += ez * (dz - d);
    }
  }
  if constexpr (KIND == VIT_DISTILL_SOFT) {
    float v[5] = {s, zs, sx, sz, a};
    block_sums<5>(v, red);
    s = v[0], zs = v[1], sx = v[2], sz = v[3], a = v[4];
  } else {
    float v[2] = {s, zs};
    block_sums<2>(v, red);
    s = v[0], zs = v[1];
  }

  // pass 3: the gradient row
  const float lse = mx + __logf(s);
  const int64_t ya = labels_a[r];
  const int64_t yb = labels_b ? labels_b[r] : ya;
  const float l = (lam && labels_b) ? lam[r] : 1.f;
  const float keep = 1.f - smoothing;
  const float ta = keep * l, tb = keep * (1.f - l), tu = smoothing / (float)classes;
  const float wb = 1.f - alpha;
  const float inv_sx = 1.f / sx, inv_sz = 1.f / sz;
  for (int64_t c = tid; c < classes; c += 256) {
    const float p = __expf(x[c] - lse);
    const float t = (c == ya ? ta : 0.f) + (c == yb ? tb : 0.f) + tu;
    float g;
    if constexpr (KIND == VIT_DISTILL_SOFT) {
      const float pt = __expf((x[c] - mx) * inv_tau) * inv_sx;
      const float qt = __expf((z[c] - mz) * inv_tau) * inv_sz;
      g = tau * (pt - qt);
    } else {
      g = znan ? NAN : p - (c == yhat ? 1.f : 0.f);
    }
    dlogits[r * classes + c] = (wb * (p - t) + alpha * g) * inv_rows;
  }

  if (tid == 0) {
    const float za = (ya >= 0 && ya < classes) ? x[ya] - mx : NAN;
    const float zb = (yb >= 0 && yb < classes) ? x[yb] - mx : NAN;
    // the mixed kernel's row term, expression for expression
    float v = __logf(s) - ((ta != 0.f ? ta * za : 0.f) + (tb != 0.f ? tb * zb : 0.f));
    if (smoothing != 0.f) v -= tu * zs;
    float d;
    if constexpr (KIND == VIT_DISTILL_SOFT) {
      // log sx - log sz as one logarithm of a ratio near 1: its absolute error is that of the ratio, not of two
      // logarithms of size log(classes), which tau^2 would scale
      d = tau * tau * (a * inv_tau * inv_sz + logf(sx * inv_sz));
    } else {
      d = yhat >= 0 ? __logf(s) - (x[yhat] - mx) : NAN;
    }
    row_loss[r] = wb * v + alpha * d;
  }
}

// xent_reduce_kernel of vit_misc.hip: the same order, so the same bits
__global__ __launch_bounds__(256) void distill_reduce_kernel(const float* __restrict__ row_loss, int64_t rows,
                                                             float inv_rows, float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += 256) s += row_loss[r];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (red[0] + red[1] + red[2] + red[3]) * inv_rows;
}

}  // namespace

extern "C" int vit_softmax_xent_distill(const float* logits, const float* teacher_logits, const int64_t* labels_a,
                                        const int64_t* labels_b, const float* lam, float smoothing, int32_t kind,
                                        float alpha, float tau, int64_t rows, int64_t classes, float* loss,
                                        float* dlogits, float* workspace, void* stream) {
  VIT_REQUIRE(logits && teacher_logits && labels_a && loss && dlogits && workspace,
              "vit_softmax_xent_distill: null pointer");
  VIT_REQUIRE(rows > 0 && classes > 0, "vit_softmax_xent_distill: rows and classes must be positive (got %lld, %lld)",
              (long long)rows, (long long)classes);
  VIT_REQUIRE(rows <= 0x7fffffff, "vit_softmax_xent_distill: too many rows for one grid (%lld)", (long long)rows);
  VIT_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "vit_softmax_xent_distill: smoothing must lie in [0, 1) (got %g)",
              (double)smoothing);
  VIT_REQUIRE(!lam || labels_b, "vit_softmax_xent_distill: lam given without labels_b");
  VIT_REQUIRE(kind == VIT_DISTILL_SOFT || kind == VIT_DISTILL_HARD,
              "vit_softmax_xent_distill: kind must be VIT_DISTILL_SOFT (0) or VIT_DISTILL_HARD (1) (got %d)", (int)kind);
  VIT_REQUIRE(alpha >= 0.f && alpha <= 1.f, "vit_softmax_xent_distill: alpha must lie in [0, 1] (got %g)",
              (double)alpha);
  VIT_REQUIRE(isfinite(tau) && tau > 0.f, "vit_softmax_xent_distill: tau must be finite and positive (got %g)",
              (double)tau);
  hipStream_t s = VIT_STREAM(stream);
  const float inv = 1.0f / (float)rows, inv_tau = 1.0f / tau;
  if (kind == VIT_DISTILL_SOFT)
    xent_distill_rows_kernel<VIT_DISTILL_SOFT><<<(unsigned)rows, 256, 0, s>>>(
        logits, teacher_logits, labels_a, labels_b, lam, smoothing, alpha, tau, inv_tau, classes, inv, dlogits,
        workspace);
  else
    xent_distill_rows_kernel<VIT_DISTILL_HARD><<<(unsigned)rows, 256, 0, s>>>(
        logits, teacher_logits, labels_a, labels_b, lam, smoothing, alpha, tau, inv_tau, classes, inv, dlogits,
        workspace);
  distill_reduce_kernel<<<1, 256, 0, s>>>(workspace, rows, inv, loss);
  return vit::check_launch("vit_softmax_xent_distill");
}
