// Validation metrics on the device (vit_hip.h "vit_eval_update"): per row of logits the prediction, the rank of the
// label and the loss term, then one workgroup that folds them into state that stays on the device until the epoch ends.
#include "vit_common.h"

namespace {

// The order of a row's entries (vit_hip.h): (a, ia) precedes (b, ib) when a > b, or when they compare equal and ia < ib.
// A NaN is greater than every number and equal to another NaN; -0.0 == +0.0 as in IEEE.
VIT_DEV bool eval_precedes(float a, int ia, float b, int ib) {
  const bool an = a != a, bn = b != b;
  const bool gt = an ? !bn : (!bn && a > b);
  const bool eq = an ? bn : a == b;                    // bn alone makes a == b false
  return gt || (eq && ia < ib);
}

constexpr int kEvalNoEntry = 0x7fffffff;               // index of "no entry yet": every real entry precedes (-inf, this)

// One wave per row, four rows per workgroup.  Rows of 10 classes (the loaders') and of 1000 (the benchmark's) both
// occur: a wave covers the first in one step and the second in 16, and no LDS or barrier is needed for either.
// Pass 1 finds the first entry of the order (the prediction; its value is the row maximum); pass 2 sums exp(x - max)
// and counts the entries that precede the label.  The second read of the row comes from the cache.
__global__ __launch_bounds__(256) void eval_rows_kernel(const float* __restrict__ logits, int64_t ld,
                                                        const int64_t* __restrict__ labels, int rows, int classes,
                                                        int64_t* __restrict__ pred, int32_t* __restrict__ rank,
                                                        float* __restrict__ row_loss) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                               // whole waves leave: no barrier follows
  const float* x = logits + r * ld;
  float bv = -INFINITY;
  int bi = kEvalNoEntry;
  for (int c = lane; c < classes; c += 64) {
    const float v = x[c];
    if (eval_precedes(v, c, bv, bi)) {
      bv = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                   // a total order: every lane ends with the same entry
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (eval_precedes(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  const int64_t y = labels[r];
  const bool scored = y >= 0 && y < classes;
  const int yi = scored ? (int)y : 0;
  const float xy = scored ? x[yi] : 0.f;               // an ignored label indexes nothing
  const float mx = bv;
  float s = 0.f;
  int before = 0;
  for (int c = lane; c < classes; c += 64) {
    const float v = x[c];
    s += __expf(v - mx);
    before += eval_precedes(v, c, xy, yi) ? 1 : 0;
  }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  if (lane == 0) {
    pred[r] = bi;
    rank[r] = scored ? before : -1;
    row_loss[r] = scored ? (mx + __logf(s)) - xy : 0.f;
  }
}

// One workgroup reads the rows back and updates the state.  The integers are exact in any order (LDS counters, and
// 64-bit vector atomics for the confusion matrix); the loss is an fp64 sum in a fixed order: lane t adds rows t,
// t + 256, ... in row order, then a fixed tree over the 256 partial sums.  Launches on one stream follow each other,
// so the plain read-modify-write of counts[] and loss_sum accumulates across them.
__global__ __launch_bounds__(256) void eval_finish_kernel(const int64_t* __restrict__ labels,
                                                          const int64_t* __restrict__ pred,
                                                          const int32_t* __restrict__ rank,
                                                          const float* __restrict__ row_loss, int rows, int classes,
                                                          int maxk, int64_t* __restrict__ counts,
                                                          double* __restrict__ loss_sum,
                                                          int64_t* __restrict__ confusion) {
  __shared__ unsigned int cnt[2 + VIT_EVAL_MAXK];      // rows <= INT32_MAX: no counter overflows
  __shared__ double red[256];
  const int tid = threadIdx.x;
  if (tid < 2 + VIT_EVAL_MAXK) cnt[tid] = 0;
  __syncthreads();
  double s = 0.0;
  unsigned int scored = 0, ignored = 0;
  for (int64_t r = tid; r < rows; r += 256) {
    const int32_t k = rank[r];
    if (k < 0) {
      ++ignored;
      continue;
    }
    ++scored;
    s += (double)row_loss[r];
    if (k < maxk) atomicAdd(&cnt[2 + k], 1u);
    if (confusion) {
      const int64_t y = labels[r];                     // in [0, classes): the rows kernel gave it a rank
      atomicAdd(reinterpret_cast<unsigned long long*>(confusion + y * (int64_t)classes + pred[r]), 1ull);
    }
  }
  if (scored) atomicAdd(&cnt[0], scored);
  if (ignored) atomicAdd(&cnt[1], ignored);
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid < 2 + maxk && cnt[tid] != 0) counts[tid] += (int64_t)cnt[tid];
  if (tid == 0) *loss_sum += red[0];
}

}  // namespace

extern "C" int vit_eval_update(const float* logits, int64_t ld, const int64_t* labels, int64_t rows, int64_t classes,
                               int32_t maxk, int64_t* pred, int32_t* rank, float* row_loss, int64_t* counts,
                               double* loss_sum, int64_t* confusion, void* stream) {
  VIT_REQUIRE(logits && labels && pred && rank && row_loss && counts && loss_sum, "vit_eval_update: null pointer");
  VIT_REQUIRE(rows > 0 && classes > 0, "vit_eval_update: rows and classes must be positive (got %lld, %lld)",
              (long long)rows, (long long)classes);
  VIT_REQUIRE(rows <= 0x7fffffff && classes <= 0x7fffffff,
              "vit_eval_update: rows and classes must fit 32 bits (got %lld, %lld)", (long long)rows,
              (long long)classes);
  VIT_REQUIRE(ld >= classes, "vit_eval_update: row stride %lld is shorter than a row of %lld classes", (long long)ld,
              (long long)classes);
  VIT_REQUIRE(maxk >= 1 && maxk <= VIT_EVAL_MAXK && maxk <= classes,
              "vit_eval_update: maxk must lie in [1, min(classes, %d)] (got %d for %lld classes)", VIT_EVAL_MAXK,
              (int)maxk, (long long)classes);
  hipStream_t s = VIT_STREAM(stream);
  eval_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(logits, ld, labels, (int)rows, (int)classes, pred, rank,
                                                              row_loss);
  eval_finish_kernel<<<1, 256, 0, s>>>(labels, pred, rank, row_loss, (int)rows, (int)classes, (int)maxk, counts,
                                       loss_sum, confusion);
  return vit::check_launch("vit_eval_update");
}
