// Attention rollout (Abnar & Zuidema 2020) of one token, one step per encoder block, formed from the block's qkv
// without a [B][H][T][T] probability tensor in memory (vit_hip.h "Attention rollout").
//
// One step, per image:  F[i][j] = fuse_h softmax_j(scale * q_i(h) . k_j(h)),  w_i = r_in[i] / (1 + sum_j F[i][j]),
//                       r_out[j] = sum_i w_i F[i][j] + w_j.
//
// rollout_mfma / rollout_valu: a workgroup owns (image, 32 query rows) and loops over the heads.  Per head it makes
//   two sweeps over the keys: the first for each row's maximum and sum (online), the second forms P and fuses it into
//   the workgroup's 32 x T block of F, which stays in LDS.  Every F entry is touched by one lane only over all heads,
//   so the head loop needs no barrier for F.  Then the row sums, w, and the w-weighted column sums of the block go to
//   part[image][row block][T] of the workspace, and w to wvec[image][T].
// rollout_finish: r_out[j] = sum over row blocks of part (ascending order) + wvec[j].  No atomics: same bits each run.
//
// bf16, hd == 64: S^T = K Q^T with v_mfma_f32_32x32x16_bf16, queries on the lanes as in vit_attention.hip's forward
//   (row statistics are per-lane scalars); the 4 waves split the 32-key blocks, each staging its K tile through a
//   wave-private LDS image, and exchange their (max, sum) through LDS once per head.
// Otherwise: VALU dot products, keys on the lanes, 8 query rows per wave sharing each K load.
// All arithmetic after the bf16 x bf16 products (exact in fp32) is fp32.
#include "vit_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int RB = 32;              // query rows per workgroup
constexpr int RO_TMAX = 1024;
constexpr int RO_HDMAX = 128;
constexpr int RO_HD = 64;           // head size of the MFMA form

// exp(d) for d <= 0 (or -inf): hardware exp2 of the difference taken in the natural-log domain first, so the
// rounding of a large logit is not multiplied by log2(e) before the subtraction
VIT_DEV float ex(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }

template <int FUSE> VIT_DEV float fuse2(float a, float p) {
  if (FUSE == VIT_ROLLOUT_MEAN) return a + p;
  if (FUSE == VIT_ROLLOUT_MAX) return fmaxf(a, p);
  return fminf(a, p);
}

// The end of a workgroup's step.  F[i * TS + j] holds rows i < nrows (i0 + i < Tn) of the fused matrix (for mean: the
// sum over the heads, divided here); every thread of the workgroup calls this after the barrier that publishes F.
template <int FUSE>
VIT_DEV void rollout_tail(float* F, float* wrow, int TS, int Tn, int H, int nrows, const float* __restrict__ r_in_b,
                          int i0, float* __restrict__ wvec_b, float* __restrict__ part, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const float fh = (float)H;
  for (int i = wave; i < nrows; i += 4) {
    float s = 0.f;
    for (int j = lane; j < Tn; j += 64) {
      float f = F[i * TS + j];
      if (FUSE == VIT_ROLLOUT_MEAN) {
        f = f / fh;
        F[i * TS + j] = f;
      }
      s += f;
    }
    s = wave_sum(s);
    if (lane == 0) {
      const float w = r_in_b[i0 + i] / (1.0f + s);
      wrow[i] = w;
      wvec_b[i0 + i] = w;
    }
  }
  __syncthreads();
  for (int j = tid; j < Tn; j += 256) {
    float acc = 0.f;
    for (int i = 0; i < nrows; ++i) acc += wrow[i] * F[i * TS + j];
    part[j] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// bf16, hd = 64: MFMA form.  The operand helpers restate vit_attention.hip's (its kernels are file-local).
// ---------------------------------------------------------------------------------------------------------------
VIT_DEV int aswz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }

// row index (within a 32-row MFMA tile) of accumulator register r for lane half h
VIT_DEV int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// S^T[key][query] of keys k0 .. k0 + 31 (rows past Tn - 1 read row Tn - 1; the caller masks them) against the 32
// queries of qf.  The K tile goes through the wave's own [32][64] LDS image, 16-B chunk c of row r at chunk
// c ^ aswz(r) (conflict-free ds_read_b128 row reads); LDS accesses of one wave execute in order, so the image needs no
// workgroup barrier.
VIT_DEV f32x16 score_tile(const bf16_t* __restrict__ kbase, int64_t ld, int k0, int Tn, bf16_t* t,
                          const bf16x8_t (&qf)[4], int lane) {
  s16x8 v[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int c = it * 64 + lane, rl = c >> 3, cc = c & 7;
    v[it] = *reinterpret_cast<const s16x8*>(kbase + (int64_t)min(k0 + rl, Tn - 1) * ld + cc * 8);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the previous tile's reads are done
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int c = it * 64 + lane, rl = c >> 3, cc = c & 7;
    *reinterpret_cast<s16x8*>(t + rl * RO_HD + ((cc ^ aswz(rl)) << 3)) = v[it];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  f32x16 acc = {};
  const int r = lane & 31;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = 2 * s + (lane >> 5);
    const s16x8 kf = *reinterpret_cast<const s16x8*>(t + r * RO_HD + ((c ^ aswz(r)) << 3));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, kf), qf[s], acc, 0, 0, 0);
  }
  return acc;
}

template <int FUSE, int TMAX>
__global__ __launch_bounds__(256) void rollout_mfma(const bf16_t* __restrict__ qkv, const float* __restrict__ r_in,
                                                    float* __restrict__ wvec, float* __restrict__ part, int Tn, int H,
                                                    float scale) {
  __shared__ __attribute__((aligned(16))) bf16_t kt[4][32 * RO_HD];   // one K tile per wave
  __shared__ float F[RB * (TMAX + 1)];
  __shared__ float stat[2][4][2][32];                                 // [head parity][wave][max, sum][query]
  __shared__ float wrow[RB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, ql = lane & 31;
  const int nrb = (Tn + RB - 1) / RB;
  const int64_t b = blockIdx.x / nrb;
  const int rb = (int)(blockIdx.x - b * nrb), i0 = rb * RB;
  const int TS = Tn | 1;                                              // odd row stride: conflict-free column writes
  const int64_t D = (int64_t)H * RO_HD, ld = 3 * D;
  const bf16_t* base = qkv + b * Tn * ld;

  for (int h = 0; h < H; ++h) {
    bf16x8_t qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {   // lane holds Q[i0 + ql][16 s + 8 hf + 0..7], zero past Tn
      s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (i0 + ql < Tn)
        v = *reinterpret_cast<const s16x8*>(base + (int64_t)(i0 + ql) * ld + h * RO_HD + 16 * s + 8 * hf);
      qf[s] = __builtin_bit_cast(bf16x8_t, v);
    }
    const bf16_t* kbase = base + D + h * RO_HD;

    // sweep 1: this wave's keys, online (max, sum) of query ql over the keys of lane half hf
    float m_run = -INFINITY, l_run = 0.f;
    for (int kb = wave; kb < nrb; kb += 4) {
      const f32x16 sacc = score_tile(kbase, ld, kb * 32, Tn, kt[wave], qf, lane);
      float x[16], mloc = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        x[r] = kb * 32 + acc_row(r, hf) < Tn ? sacc[r] * scale : -INFINITY;
        mloc = fmaxf(mloc, x[r]);
      }
      const float m_new = fmaxf(m_run, mloc);
      const float ms = m_new == -INFINITY ? 0.f : m_new;   // a half with no valid key yet: every term below is 0
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) psum += ex(x[r] - ms);
      l_run = l_run * ex(m_run - ms) + psum;
      m_run = m_new;
    }
    {
      const float mo = __shfl_xor(m_run, 32, 64), lo = __shfl_xor(l_run, 32, 64);
      const float mm = fmaxf(m_run, mo), ms = mm == -INFINITY ? 0.f : mm;
      l_run = l_run * ex(m_run - ms) + lo * ex(mo - ms);
      m_run = mm;
    }
    float(&st)[4][2][32] = stat[h & 1];
    if (hf == 0) {
      st[wave][0][ql] = m_run;
      st[wave][1][ql] = l_run;
    }
    __syncthreads();   // one barrier per head: stat[] alternates, and a wave is past this one before it rewrites
    float M = st[0][0][ql];   // wave 0 holds key 0: finite
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, st[w][0][ql]);
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) L += st[w][1][ql] * ex(st[w][0][ql] - M);
    const float inv = 1.0f / L;

    // sweep 2: P, fused into F[query][key]
    for (int kb = wave; kb < nrb; kb += 4) {
      const f32x16 sacc = score_tile(kbase, ld, kb * 32, Tn, kt[wave], qf, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb * 32 + acc_row(r, hf);
        if (key < Tn) {
          const float p = ex(sacc[r] * scale - M) * inv;
          float* f = F + ql * TS + key;
          *f = h == 0 ? p : fuse2<FUSE>(*f, p);
        }
      }
    }
  }
  __syncthreads();
  rollout_tail<FUSE>(F, wrow, TS, Tn, H, min(RB, Tn - i0), r_in + b * Tn, i0, wvec + b * Tn,
                     part + ((int64_t)blockIdx.x) * Tn, tid);
}

// ---------------------------------------------------------------------------------------------------------------
// VALU form: any dtype, hd <= 128, hd % 4 == 0
// ---------------------------------------------------------------------------------------------------------------
// s[a] = q[a] . k for the wave's 8 query rows (LDS, broadcast reads) and this lane's key row
template <class T>
VIT_DEV void dots8(const T* __restrict__ krow, const float (*q)[RO_HDMAX], int hd, float s[8]) {
#pragma unroll
  for (int a = 0; a < 8; ++a) s[a] = 0.f;
  for (int d = 0; d < hd; d += 4) {
    float k[4];
    ld4<T>(krow + d, k);
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const f32x4 qv = *reinterpret_cast<const f32x4*>(&q[a][d]);
      s[a] += qv[0] * k[0];
      s[a] += qv[1] * k[1];
      s[a] += qv[2] * k[2];
      s[a] += qv[3] * k[3];
    }
  }
}

template <class T, int FUSE, int TMAX>
__global__ __launch_bounds__(256) void rollout_valu(const T* __restrict__ qkv, const float* __restrict__ r_in,
                                                    float* __restrict__ wvec, float* __restrict__ part, int Tn, int H,
                                                    int hd, float scale) {
  __shared__ __attribute__((aligned(16))) float qs[RB][RO_HDMAX];
  __shared__ float F[RB * (TMAX + 1)];
  __shared__ float wrow[RB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nrb = (Tn + RB - 1) / RB;
  const int64_t b = blockIdx.x / nrb;
  const int rb = (int)(blockIdx.x - b * nrb), i0 = rb * RB;
  const int TS = Tn | 1;
  const int nrows = min(RB, Tn - i0);
  const int64_t D = (int64_t)H * hd, ld = 3 * D;
  const T* base = qkv + b * Tn * ld;
  const int r0 = wave * 8;

  for (int h = 0; h < H; ++h) {
    __syncthreads();   // the previous head's reads of qs
    for (int e = tid; e < RB * hd; e += 256) {
      const int i = e / hd, d = e - i * hd;
      qs[i][d] = i < nrows ? ld1<T>(base + (int64_t)(i0 + i) * ld + h * hd + d) : 0.f;
    }
    __syncthreads();
    if (r0 >= nrows) continue;   // wave-uniform; the barriers above are reached by every wave in every head
    const T* kbase = base + D + h * hd;
    float m[8], l[8], s[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      m[a] = -INFINITY;
      l[a] = 0.f;
    }
    for (int j = lane; j < Tn; j += 64) {
      dots8<T>(kbase + (int64_t)j * ld, qs + r0, hd, s);
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const float x = s[a] * scale, mn = fmaxf(m[a], x);
        l[a] = l[a] * ex(m[a] - mn) + ex(x - mn);
        m[a] = mn;
      }
    }
    float inv[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const float M = wave_max(m[a]);          // lane 0 holds key 0: finite
      inv[a] = 1.0f / wave_sum(l[a] * ex(m[a] - M));
      m[a] = M;
    }
    for (int j = lane; j < Tn; j += 64) {
      dots8<T>(kbase + (int64_t)j * ld, qs + r0, hd, s);
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        if (r0 + a < nrows) {
          const float p = ex(s[a] * scale - m[a]) * inv[a];
          float* f = F + (r0 + a) * TS + j;
          *f = h == 0 ? p : fuse2<FUSE>(*f, p);
        }
      }
    }
  }
  __syncthreads();
  rollout_tail<FUSE>(F, wrow, TS, Tn, H, nrows, r_in + b * Tn, i0, wvec + b * Tn, part + ((int64_t)blockIdx.x) * Tn,
                     tid);
}

__global__ __launch_bounds__(256) void rollout_finish(const float* __restrict__ wvec, const float* __restrict__ part,
                                                      float* __restrict__ r_out, int64_t n, int Tn, int nrb) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;   // = b * Tn + j
  if (e >= n) return;
  const int64_t b = e / Tn, j = e - b * Tn;
  float acc = 0.f;
  for (int rb = 0; rb < nrb; ++rb) acc += part[(b * nrb + rb) * Tn + j];
  r_out[e] = acc + wvec[e];
}

bool rollout_mfma_ok(int64_t hd, int32_t dtype) { return dtype == VIT_BF16 && hd == RO_HD; }

template <int FUSE, int TMAX>
void rollout_launch(const void* qkv, const float* r_in, float* wvec, float* part, int64_t B, int64_t T, int64_t H,
                    int64_t hd, float scale, int32_t dtype, bool mfma, hipStream_t s) {
  const unsigned grid = (unsigned)(B * ((T + RB - 1) / RB));
  if (mfma)
    rollout_mfma<FUSE, TMAX><<<grid, 256, 0, s>>>((const bf16_t*)qkv, r_in, wvec, part, (int)T, (int)H, scale);
  else if (dtype == VIT_BF16)
    rollout_valu<bf16_t, FUSE, TMAX><<<grid, 256, 0, s>>>((const bf16_t*)qkv, r_in, wvec, part, (int)T, (int)H,
                                                         (int)hd, scale);
  else
    rollout_valu<float, FUSE, TMAX><<<grid, 256, 0, s>>>((const float*)qkv, r_in, wvec, part, (int)T, (int)H, (int)hd,
                                                        scale);
}

// the F block's LDS size follows T in three steps, so that the common T <= 256 keeps several workgroups on a CU
template <int FUSE>
void rollout_launch_t(const void* qkv, const float* r_in, float* wvec, float* part, int64_t B, int64_t T, int64_t H,
                      int64_t hd, float scale, int32_t dtype, bool mfma, hipStream_t s) {
  if (T <= 256)
    rollout_launch<FUSE, 256>(qkv, r_in, wvec, part, B, T, H, hd, scale, dtype, mfma, s);
  else if (T <= 640)
    rollout_launch<FUSE, 640>(qkv, r_in, wvec, part, B, T, H, hd, scale, dtype, mfma, s);
  else
    rollout_launch<FUSE, RO_TMAX>(qkv, r_in, wvec, part, B, T, H, hd, scale, dtype, mfma, s);
}

bool rollout_shape_ok(int64_t B, int64_t T, int64_t H, int64_t hd, int32_t dtype, int32_t fuse) {
  return B > 0 && T > 0 && H > 0 && hd > 0 && T <= RO_TMAX && hd <= RO_HDMAX && hd % 4 == 0 &&
         (dtype == VIT_F32 || dtype == VIT_BF16) && fuse >= VIT_ROLLOUT_MEAN && fuse <= VIT_ROLLOUT_MIN &&
         B * ((T + RB - 1) / RB) <= 0x7fffffffLL && B * T <= (1LL << 38) && 3 * H * hd <= 0x7fffffffLL;
}

}  // namespace

extern "C" int64_t vit_attn_rollout_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t hd, int32_t dtype,
                                                    int32_t fuse) {
  if (!rollout_shape_ok(B, T, H, hd, dtype, fuse)) return 0;
  return B * T * ((T + RB - 1) / RB + 1) * (int64_t)sizeof(float);   // wvec[B][T], part[B][row blocks][T]
}

extern "C" int vit_attn_rollout_step_form(const void* qkv, const float* r_in, float* r_out, int64_t B, int64_t T,
                                          int64_t H, int64_t hd, float scale, int32_t dtype, int32_t fuse,
                                          int32_t form, void* workspace, void* stream) {
  VIT_REQUIRE(qkv && r_in && r_out && workspace, "vit_attn_rollout_step: NULL pointer");
  VIT_REQUIRE(B > 0 && T > 0 && H > 0 && hd > 0, "vit_attn_rollout_step: bad sizes");
  VIT_REQUIRE(dtype == VIT_F32 || dtype == VIT_BF16, "vit_attn_rollout_step: dtype must be VIT_F32 or VIT_BF16");
  VIT_REQUIRE(fuse >= VIT_ROLLOUT_MEAN && fuse <= VIT_ROLLOUT_MIN,
              "vit_attn_rollout_step: fuse must be 0 (mean), 1 (max) or 2 (min)");
  VIT_REQUIRE(T <= RO_TMAX && hd <= RO_HDMAX && hd % 4 == 0, "vit_attn_rollout_step: T <= %d, hd <= %d, hd %% 4 == 0",
              RO_TMAX, RO_HDMAX);
  VIT_REQUIRE(rollout_shape_ok(B, T, H, hd, dtype, fuse),
              "vit_attn_rollout_step: B * ceil(T / 32) and 3 * H * hd must fit 31 bits");
  VIT_REQUIRE(form >= 0 && form <= 2 && (form != 2 || rollout_mfma_ok(hd, dtype)),
              "vit_attn_rollout_step: form must be 0 (automatic), 1 (VALU) or 2 (MFMA: bf16, hd == 64)");
  VIT_REQUIRE(r_in + B * T <= r_out || r_out + B * T <= r_in,
              "vit_attn_rollout_step: r_in and r_out must not overlap");
  VIT_REQUIRE(((uintptr_t)qkv) % 16 == 0 && ((uintptr_t)workspace) % 4 == 0 && ((uintptr_t)r_in) % 4 == 0 &&
                  ((uintptr_t)r_out) % 4 == 0,
              "vit_attn_rollout_step: qkv must be 16-B aligned, the fp32 buffers 4-B aligned");
  const bool mfma = form == 2 || (form == 0 && rollout_mfma_ok(hd, dtype));
  hipStream_t s = VIT_STREAM(stream);
  float* wvec = (float*)workspace;
  float* part = wvec + B * T;
  switch (fuse) {
    case VIT_ROLLOUT_MEAN:
      rollout_launch_t<VIT_ROLLOUT_MEAN>(qkv, r_in, wvec, part, B, T, H, hd, scale, dtype, mfma, s);
      break;
    case VIT_ROLLOUT_MAX:
      rollout_launch_t<VIT_ROLLOUT_MAX>(qkv, r_in, wvec, part, B, T, H, hd, scale, dtype, mfma, s);
      break;
    default:
      rollout_launch_t<VIT_ROLLOUT_MIN>(qkv, r_in, wvec, part, B, T, H, hd, scale, dtype, mfma, s);
      break;
  }
  if (int rc = vit::check_launch("vit_attn_rollout_step")) return rc;
  const int nrb = (int)((T + RB - 1) / RB);
  rollout_finish<<<(unsigned)((B * T + 255) / 256), 256, 0, s>>>(wvec, part, r_out, B * T, (int)T, nrb);
  return vit::check_launch("vit_attn_rollout_step");
}

extern "C" int vit_attn_rollout_step(const void* qkv, const float* r_in, float* r_out, int64_t B, int64_t T, int64_t H,
                                     int64_t hd, float scale, int32_t dtype, int32_t fuse, void* workspace,
                                     void* stream) {
  return vit_attn_rollout_step_form(qkv, r_in, r_out, B, T, H, hd, scale, dtype, fuse, 0, workspace, stream);
}
