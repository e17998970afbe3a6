// GPU image pipeline of the training loader (reference src/train.py:151-155, BrainTumorDataset.py:35-39):
// convert('RGB') -> Resize((S, S)) (PIL bilinear) -> ToTensor, for a batch of raw uint8 HWC images of any sizes
// (ragged batches allowed) packed into one byte buffer.  Bit-exact with Pillow's 8-bit resampler:
//   * per-axis coefficients are Pillow's (triangle filter, support scaled by the reduction factor, normalised in
//     double, 22-bit fixed point) and are computed on the device in double with FP contraction OFF, so every
//     intermediate rounds exactly as the host C code does;
//   * the horizontal pass rounds to 8 bits (clip8) before the vertical pass, exactly like Pillow's two-pass resize
//     (which runs the horizontal pass first); a pass whose size does not change is an identity in this arithmetic.
// Kernel 1 writes per-image coefficient tables to the caller's workspace; kernel 2 computes one output pixel (all 3
// channels) per thread, coalesced along output rows of each channel plane.
#include <math.h>

#include "vit_common.h"

namespace {

constexpr int PREC = 22;

struct ImgMeta {        // device view of the caller's int64 meta[B][4]
  int64_t off, h, w, c;
};

// Pillow precompute_coeffs + normalize_coeffs_8bpc for output index i of one axis.
__device__ __noinline__ void axis_coeffs(int i, int in_size, int out_size, int ksize, int* bound, int* k) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double ss = 1.0 / filterscale;
  const double center = 0.0 + ((double)i + 0.5) * scale;
  int lo = (int)(center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + support + 0.5);
  if (hi > in_size) hi = in_size;
  const int n = hi - lo;
  double ww = 0.0;
  for (int j = 0; j < n; ++j) {
    double t = ((double)(j + lo) - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    ww += t < 1.0 ? 1.0 - t : 0.0;
  }
  for (int j = 0; j < ksize; ++j) {
    int kv = 0;
    if (j < n) {
      double t = ((double)(j + lo) - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      double w = t < 1.0 ? 1.0 - t : 0.0;
      if (ww != 0.0) w = w / ww;
      kv = w < 0.0 ? (int)(-0.5 + w * (double)(1 << PREC)) : (int)(0.5 + w * (double)(1 << PREC));
    }
    k[j] = kv;
  }
  bound[0] = lo;
  bound[1] = n < ksize ? n : ksize;      // never read past this row's taps (the host passes ksize >= every n)
}

// Table layout per image (ints): bounds_w[ow][2], bounds_h[oh][2], k_w[ow][ks], k_h[oh][ks].
__global__ __launch_bounds__(256) void resize_coeffs_kernel(const int64_t* __restrict__ meta, int oh, int ow, int ks,
                                                            int* __restrict__ tab) {
  const int b = blockIdx.y;
  const ImgMeta m = reinterpret_cast<const ImgMeta*>(meta)[b];
  const int64_t per = (int64_t)(ow + oh) * (2 + ks);
  int* t = tab + b * per;
  int* bw = t;
  int* bh = bw + 2 * ow;
  int* kw = bh + 2 * oh;
  int* kh = kw + (int64_t)ow * ks;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ow + oh; i += gridDim.x * blockDim.x) {
    if (i < ow) axis_coeffs(i, (int)m.w, ow, ks, bw + 2 * i, kw + (int64_t)i * ks);
    else axis_coeffs(i - ow, (int)m.h, oh, ks, bh + 2 * (i - ow), kh + (int64_t)(i - ow) * ks);
  }
}

VIT_DEV int clip8(int v) {
  v >>= PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <class TO>
__global__ __launch_bounds__(256) void resize_apply_kernel(const uint8_t* __restrict__ src,
                                                           const int64_t* __restrict__ meta, int oh, int ow, int ks,
                                                           const int* __restrict__ tab, TO* __restrict__ out) {
  const int b = blockIdx.z;
  const int y = blockIdx.y;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= ow) return;
  const ImgMeta m = reinterpret_cast<const ImgMeta*>(meta)[b];
  const int64_t per = (int64_t)(ow + oh) * (2 + ks);
  const int* t = tab + b * per;
  const int* bw = t;
  const int* bh = bw + 2 * ow;
  const int* kw = bh + 2 * oh + (int64_t)x * ks;
  const int* kh = bh + 2 * oh + (int64_t)ow * ks + (int64_t)y * ks;
  const int xlo = bw[2 * x], xn = bw[2 * x + 1];
  const int ylo = bh[2 * y], yn = bh[2 * y + 1];
  const int C = (int)m.c, W = (int)m.w;
  // convert('RGB'): L / LA replicate channel 0, RGB / RGBA take channels 0..2
  const int c1 = C >= 3 ? 1 : 0, c2 = C >= 3 ? 2 : 0;
  const uint8_t* img = src + m.off;
  int acc0 = 1 << (PREC - 1), acc1 = acc0, acc2 = acc0;
  for (int j = 0; j < yn; ++j) {
    const uint8_t* row = img + (int64_t)(ylo + j) * W * C;
    int h0 = 1 << (PREC - 1), h1 = h0, h2 = h0;
    for (int i = 0; i < xn; ++i) {
      const uint8_t* px = row + (int64_t)(xlo + i) * C;
      const int kk = kw[i];
      h0 += (int)px[0] * kk;
      h1 += (int)px[c1] * kk;
      h2 += (int)px[c2] * kk;
    }
    const int kv = kh[j];
    acc0 += clip8(h0) * kv;
    acc1 += clip8(h1) * kv;
    acc2 += clip8(h2) * kv;
  }
  const int64_t plane = (int64_t)oh * ow;
  TO* o = out + (int64_t)b * 3 * plane + (int64_t)y * ow + x;
  st1<TO>(o, (float)clip8(acc0) / 255.0f);           // ToTensor: uint8 / 255, IEEE division
  st1<TO>(o + plane, (float)clip8(acc1) / 255.0f);
  st1<TO>(o + 2 * plane, (float)clip8(acc2) / 255.0f);
}

// ---------------------------------------------------------------------------------------------------------------
// Training augmentation in the resize launch (vit_hip.h "Training augmentation"): the crop is another source window
// per image (the coefficient tables are those of the crop's size, their bounds offset by the crop's origin), the flip
// a mirrored store column, the normalize another final scale, the erase a pixel that reads no tap.  The tables have
// vit_resize_to_tensor's layout.  Two apply kernels give the same bits: the direct one is resize_apply_kernel's
// schedule; the tiled one runs the horizontal pass once per source row of a tile's row span into LDS (one dword per
// pixel: the three clip8'd channels) and the vertical pass out of it.  Both are also instantiated with a uint8 store
// (vit_augment_to_u8, vit_hip.h "RandAugment"): the resized, flipped crop itself as HWC bytes, no value, no erase.
// ---------------------------------------------------------------------------------------------------------------
// Automatic dispatch: the tiled form up to this ksize (scale <= 4, where every tile's row span fits: 16 x 4 + 2 x 4
// rows), the range it was measured in and won (ksize 3 and 7); the direct form above it.
constexpr int AUG_TILED_MAX_KS = 9;

// one axis of a crop box, clamped to its image: the origin into [0, size-1], the extent into [1, size-origin]
VIT_DEV void clamp_box(int& o, int& n, int size) {
  o = o < 0 ? 0 : (o > size - 1 ? size - 1 : o);
  n = n < 1 ? 1 : (n > size - o ? size - o : n);
}

__global__ __launch_bounds__(256) void augment_coeffs_kernel(const int64_t* __restrict__ meta,
                                                             const vit_aug_item* __restrict__ items, int oh, int ow,
                                                             int ks, int* __restrict__ tab) {
  const int b = blockIdx.y;
  const ImgMeta m = reinterpret_cast<const ImgMeta*>(meta)[b];
  const vit_aug_item it = items[b];
  int x0 = it.x0, cw = it.cw, y0 = it.y0, ch = it.ch;
  clamp_box(x0, cw, (int)m.w);
  clamp_box(y0, ch, (int)m.h);
  const int64_t per = (int64_t)(ow + oh) * (2 + ks);
  int* t = tab + b * per;
  int* bw = t;
  int* bh = bw + 2 * ow;
  int* kw = bh + 2 * oh;
  int* kh = kw + (int64_t)ow * ks;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ow + oh; i += gridDim.x * blockDim.x) {
    if (i < ow) {
      axis_coeffs(i, cw, ow, ks, bw + 2 * i, kw + (int64_t)i * ks);
      bw[2 * i] += x0;                     // taps stay inside the crop: [x0 + lo, x0 + lo + n) with lo + n <= cw
    } else {
      axis_coeffs(i - ow, ch, oh, ks, bh + 2 * (i - ow), kh + (int64_t)(i - ow) * ks);
      bh[2 * (i - ow)] += y0;
    }
  }
}

// Pixel (x, y) of the resized crop in resize_apply_kernel's arithmetic; kwt / kht: the image's k_w / k_h tables.
VIT_DEV void resize_pixel(const uint8_t* __restrict__ img, int W, int C, const int* __restrict__ bw,
                          const int* __restrict__ bh, const int* __restrict__ kwt, const int* __restrict__ kht, int ks,
                          int x, int y, int& r0, int& r1, int& r2) {
  const int* kw = kwt + (int64_t)x * ks;
  const int* kh = kht + (int64_t)y * ks;
  const int xlo = bw[2 * x], xn = bw[2 * x + 1];
  const int ylo = bh[2 * y], yn = bh[2 * y + 1];
  const int c1 = C >= 3 ? 1 : 0, c2 = C >= 3 ? 2 : 0;
  int acc0 = 1 << (PREC - 1), acc1 = acc0, acc2 = acc0;
  for (int j = 0; j < yn; ++j) {
    const uint8_t* row = img + (int64_t)(ylo + j) * W * C;
    int h0 = 1 << (PREC - 1), h1 = h0, h2 = h0;
    for (int i = 0; i < xn; ++i) {
      const uint8_t* px = row + (int64_t)(xlo + i) * C;
      const int kk = kw[i];
      h0 += (int)px[0] * kk;
      h1 += (int)px[c1] * kk;
      h2 += (int)px[c2] * kk;
    }
    const int kv = kh[j];
    acc0 += clip8(h0) * kv;
    acc1 += clip8(h1) * kv;
    acc2 += clip8(h2) * kv;
  }
  r0 = clip8(acc0);
  r1 = clip8(acc1);
  r2 = clip8(acc2);
}

// TO = uint8_t (vit_augment_to_u8) stores the resized, flipped crop itself as HWC bytes: no value table, no erase.
template <class TO> constexpr bool AUG_BYTES = false;
template <> constexpr bool AUG_BYTES<uint8_t> = true;

VIT_DEV void aug_store_bytes(uint8_t* out, int b, int oh, int ow, int y, int xs, int v0, int v1, int v2) {
  uint8_t* o = out + (((int64_t)b * oh + y) * ow + xs) * 3;
  o[0] = (uint8_t)v0;
  o[1] = (uint8_t)v1;
  o[2] = (uint8_t)v2;
}

template <class TO>
__global__ __launch_bounds__(256) void augment_apply_kernel(const uint8_t* __restrict__ src,
                                                            const int64_t* __restrict__ meta,
                                                            const vit_aug_item* __restrict__ items, int oh, int ow,
                                                            int ks, const int* __restrict__ tab, AugNorm nm, float ev,
                                                            TO* __restrict__ out) {
  const int b = blockIdx.z;
  const int y = blockIdx.y;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;       // column of the resized crop
  if (x >= ow) return;
  const vit_aug_item it = items[b];
  const int xs = it.flip ? ow - 1 - x : x;                   // column it is stored at
  const int64_t plane = (int64_t)oh * ow;
  TO* o = out + (int64_t)b * 3 * plane + (int64_t)y * ow + xs;
  if constexpr (!AUG_BYTES<TO>) {
    if (aug_erased(it, y, xs)) {
      st1<TO>(o, ev);
      st1<TO>(o + plane, ev);
      st1<TO>(o + 2 * plane, ev);
      return;
    }
  }
  const ImgMeta m = reinterpret_cast<const ImgMeta*>(meta)[b];
  const int* bw = tab + b * ((int64_t)(ow + oh) * (2 + ks));
  const int* bh = bw + 2 * ow;
  const int* kwt = bh + 2 * oh;
  int v0, v1, v2;
  resize_pixel(src + m.off, (int)m.w, (int)m.c, bw, bh, kwt, kwt + (int64_t)ow * ks, ks, x, y, v0, v1, v2);
  if constexpr (AUG_BYTES<TO>) {
    aug_store_bytes(out, b, oh, ow, y, xs, v0, v1, v2);
  } else {
    st1<TO>(o, aug_value(v0, nm.mean[0], nm.sd[0], nm.on));
    st1<TO>(o + plane, aug_value(v1, nm.mean[1], nm.sd[1], nm.on));
    st1<TO>(o + 2 * plane, aug_value(v2, nm.mean[2], nm.sd[2], nm.on));
  }
}

// One workgroup per tile of TR output rows x TC output columns of one image; lane (lx, ly) owns column lx of the tile
// and its rows ly, ly + 4, ...  The item, the meta and the tile's row span [r0, r1) are workgroup-uniform.  Only
// 256 x 3 distinct output values exist: they are formed once per workgroup, with aug_value's arithmetic, in LDS.
template <class TO>
__global__ __launch_bounds__(256) void augment_tiled_kernel(const uint8_t* __restrict__ src,
                                                            const int64_t* __restrict__ meta,
                                                            const vit_aug_item* __restrict__ items, int oh, int ow,
                                                            int ks, const int* __restrict__ tab, AugNorm nm, float ev,
                                                            TO* __restrict__ out) {
  constexpr int TR = VIT_AUG_TILE_ROWS, TC = VIT_AUG_TILE_COLS, SPAN = VIT_AUG_TILE_MAX_SPAN;
  static_assert(TC == 64 && TR % 4 == 0, "a wave owns one row of the tile, a workgroup four");
  __shared__ uint32_t hp[SPAN * TC];       // horizontal pass: [source row - r0][column], channels in bytes 0..2
  __shared__ float val[3 * 256];           // output value of byte v in channel c
  const int b = blockIdx.z;
  const int ty0 = blockIdx.y * TR;
  const int tyn = oh - ty0 < TR ? oh - ty0 : TR;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = blockIdx.x * TC + lx;
  const vit_aug_item it = items[b];
  const ImgMeta m = reinterpret_cast<const ImgMeta*>(meta)[b];
  const int xs = it.flip ? ow - 1 - x : x;
  const int* bw = tab + b * ((int64_t)(ow + oh) * (2 + ks));
  const int* bh = bw + 2 * ow;
  const int* kwt = bh + 2 * oh;
  const int* kht = kwt + (int64_t)ow * ks;
  const uint8_t* img = src + m.off;
  const int C = (int)m.c, W = (int)m.w;
  if constexpr (!AUG_BYTES<TO>) {
#pragma unroll
    for (int c = 0; c < 3; ++c) val[c * 256 + threadIdx.x] = aug_value((int)threadIdx.x, nm.mean[c], nm.sd[c], nm.on);
  }
  int r0 = 0x7fffffff, r1 = 0;
  for (int r = 0; r < tyn; ++r) {
    const int lo = bh[2 * (ty0 + r)], n = bh[2 * (ty0 + r) + 1];
    r0 = lo < r0 ? lo : r0;
    r1 = lo + n > r1 ? lo + n : r1;
  }
  const bool fits = r1 - r0 <= SPAN;       // else this tile takes the direct form below
  if (fits) {
    // a column whose every pixel in this tile is erased reads nothing
    const bool dead = !AUG_BYTES<TO> && xs >= it.ex0 && xs < it.ex1 && ty0 >= it.ey0 && ty0 + tyn <= it.ey1;
    if (x < ow && !dead) {
      const int xlo = bw[2 * x], xn = bw[2 * x + 1];
      const int* kw = kwt + (int64_t)x * ks;
      const int c1 = C >= 3 ? 1 : 0, c2 = C >= 3 ? 2 : 0;
      for (int r = r0 + ly; r < r1; r += 4) {
        const uint8_t* row = img + (int64_t)r * W * C;
        int h0 = 1 << (PREC - 1), h1 = h0, h2 = h0;
        for (int i = 0; i < xn; ++i) {
          const uint8_t* px = row + (int64_t)(xlo + i) * C;
          const int kk = kw[i];
          h0 += (int)px[0] * kk;
          h1 += (int)px[c1] * kk;
          h2 += (int)px[c2] * kk;
        }
        hp[(r - r0) * TC + lx] = (uint32_t)clip8(h0) | ((uint32_t)clip8(h1) << 8) | ((uint32_t)clip8(h2) << 16);
      }
    }
  }
  __syncthreads();
  if (x >= ow) return;
  const int64_t plane = (int64_t)oh * ow;
  for (int y = ty0 + ly; y < ty0 + tyn; y += 4) {
    TO* o = out + (int64_t)b * 3 * plane + (int64_t)y * ow + xs;
    if constexpr (!AUG_BYTES<TO>) {
      if (aug_erased(it, y, xs)) {
        st1<TO>(o, ev);
        st1<TO>(o + plane, ev);
        st1<TO>(o + 2 * plane, ev);
        continue;
      }
    }
    int v0, v1, v2;
    if (fits) {
      const int ylo = bh[2 * y], yn = bh[2 * y + 1];
      const int* kh = kht + (int64_t)y * ks;
      const uint32_t* col = hp + (ylo - r0) * TC + lx;
      int acc0 = 1 << (PREC - 1), acc1 = acc0, acc2 = acc0;
      for (int j = 0; j < yn; ++j) {
        const uint32_t p = col[j * TC];
        const int kv = kh[j];
        acc0 += (int)(p & 255u) * kv;
        acc1 += (int)((p >> 8) & 255u) * kv;
        acc2 += (int)(p >> 16) * kv;
      }
      v0 = clip8(acc0);
      v1 = clip8(acc1);
      v2 = clip8(acc2);
    } else {
      resize_pixel(img, W, C, bw, bh, kwt, kht, ks, x, y, v0, v1, v2);
    }
    if constexpr (AUG_BYTES<TO>) {
      aug_store_bytes(out, b, oh, ow, y, xs, v0, v1, v2);
    } else {
      st1<TO>(o, val[v0]);
      st1<TO>(o + plane, val[256 + v1]);
      st1<TO>(o + 2 * plane, val[512 + v2]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Batch mix (vit_hip.h "Batch mix"): out[i] = x[src_i] inside image i's box, w_i * x[i] + (1 - w_i) * x[src_i] outside
// it — mixup (empty box), CutMix (w = 1) and the unmixed image (w = 1, empty box) in one streaming kernel.
// One lane owns U units of one image, a unit being 16 bytes of one row (VEC = 4 fp32 / 8 bf16 elements) or, where the
// pointers or the row length do not allow that, one element (VEC = 1).  The image's table entry is workgroup-uniform.
// All loads of a lane's units are issued before the math; a unit outside the box of a w = 1 image never reads x[src],
// a unit inside the box never reads x[i], and a 16-byte unit that a box edge cuts is done element by element, each
// element read from the one image it needs.
// ---------------------------------------------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <class T, int VEC> struct MixUnit { typedef u32x4 type; };
template <class T> struct MixUnit<T, 1> { typedef T type; };

// the one blend both forms use, so that they agree bit for bit: w1 = 1 - w formed once per image
VIT_DEV float mix1(float a, float b, float w, float w1) { return fmaf(w, a, w1 * b); }

VIT_DEV float mix_unit(float a, float b, float w, float w1) { return mix1(a, b, w, w1); }
VIT_DEV bf16_t mix_unit(bf16_t a, bf16_t b, float w, float w1) { return f2bf(mix1(bf2f(a), bf2f(b), w, w1)); }
template <class T> VIT_DEV u32x4 mix_unit16(u32x4 a, u32x4 b, float w, float w1);
template <> VIT_DEV u32x4 mix_unit16<float>(u32x4 a, u32x4 b, float w, float w1) {
  u32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = __float_as_uint(mix1(__uint_as_float(a[k]), __uint_as_float(b[k]), w, w1));
  return r;
}
template <> VIT_DEV u32x4 mix_unit16<bf16_t>(u32x4 a, u32x4 b, float w, float w1) {
  u32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float lo = mix1(__uint_as_float(a[k] << 16), __uint_as_float(b[k] << 16), w, w1);
    const float hi = mix1(__uint_as_float(a[k] & 0xffff0000u), __uint_as_float(b[k] & 0xffff0000u), w, w1);
    r[k] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
  }
  return r;
}
template <class T, int VEC> VIT_DEV typename MixUnit<T, VEC>::type mix_blend(typename MixUnit<T, VEC>::type a,
                                                                             typename MixUnit<T, VEC>::type b,
                                                                             float w, float w1) {
  if constexpr (VEC == 1) return mix_unit(a, b, w, w1);
  else return mix_unit16<T>(a, b, w, w1);
}

// one element as the 32 bits it waits in
VIT_DEV uint32_t mix_raw(float v) { return __float_as_uint(v); }
VIT_DEV uint32_t mix_raw(bf16_t v) { return v; }
template <class T> VIT_DEV T mix_unraw(uint32_t r);
template <> VIT_DEV float mix_unraw<float>(uint32_t r) { return __uint_as_float(r); }
template <> VIT_DEV bf16_t mix_unraw<bf16_t>(uint32_t r) { return (bf16_t)r; }

enum { MIX_SKIP = 0, MIX_OUTSIDE = 1, MIX_INSIDE = 2, MIX_CUT = 3 };

// nu: units per image, upr: units per row (W / VEC), bpi: workgroups per image, n: elements per image
template <class T, int VEC, int U>
__global__ __launch_bounds__(256) void mix_batch_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                        const vit_mix_item* __restrict__ items, uint32_t nu,
                                                        uint32_t upr, uint32_t H, uint32_t bpi, int64_t n) {
  typedef typename MixUnit<T, VEC>::type R;
  const uint32_t img = blockIdx.x / bpi;
  const uint32_t chunk = blockIdx.x - img * bpi;
  const vit_mix_item it = items[img];
  const bool keep = it.w == 1.0f;                 // outside the box the image is its own, bitwise
  const float w = it.w, w1 = 1.0f - it.w;
  const T* xi = x + (int64_t)img * n;
  const T* xs = x + (int64_t)it.src * n;
  T* o = out + (int64_t)img * n;
  uint32_t e[U];                                  // first element of the unit within the image
  int xv[U], mode[U];
  R a[U], b[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t v = chunk * (256u * U) + (uint32_t)u * 256u + threadIdx.x;
    mode[u] = MIX_SKIP;
    e[u] = 0;
    xv[u] = 0;
    if (v < nu) {
      const uint32_t row = v / upr;
      const int y = (int)(row % H);
      xv[u] = (int)(v - row * upr) * VEC;
      e[u] = v * VEC;
      const bool rowin = y >= it.y0 && y < it.y1;
      if (!rowin || xv[u] + VEC <= it.x0 || xv[u] >= it.x1) mode[u] = MIX_OUTSIDE;
      else if (xv[u] >= it.x0 && xv[u] + VEC <= it.x1) mode[u] = MIX_INSIDE;
      else mode[u] = MIX_CUT;
    }
    if (mode[u] == MIX_OUTSIDE) a[u] = *reinterpret_cast<const R*>(xi + e[u]);
    if (mode[u] == MIX_INSIDE || (mode[u] == MIX_OUTSIDE && !keep)) b[u] = *reinterpret_cast<const R*>(xs + e[u]);
    if constexpr (VEC > 1) {
      // A unit with a box edge inside it (its row is inside the box's rows; a random box gives most box rows two):
      // element by element, every element from the one image it needs — x[src] inside the box, x[i] outside —, issued
      // here with the other loads.  Element j waits, unconverted, in the unit's a / b registers (j < 4 / j >= 4).
      if (mode[u] == MIX_CUT) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int xx = xv[u] + j;
          const uint32_t raw = mix_raw(((xx >= it.x0 && xx < it.x1) ? xs : xi)[e[u] + j]);
          if (j < 4) a[u][j] = raw;
          else b[u][j - 4] = raw;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (mode[u] == MIX_OUTSIDE) {
      *reinterpret_cast<R*>(o + e[u]) = keep ? a[u] : mix_blend<T, VEC>(a[u], b[u], w, w1);
    } else if (mode[u] == MIX_INSIDE) {
      *reinterpret_cast<R*>(o + e[u]) = b[u];
    }
    if constexpr (VEC > 1) {
      if (mode[u] == MIX_CUT) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int xx = xv[u] + j;
          T r = mix_unraw<T>(j < 4 ? a[u][j] : b[u][j - 4]);
          // only a blended image with a box (w < 1 and a box, which BatchMix never draws) needs a second element
          if (!keep && !(xx >= it.x0 && xx < it.x1)) r = mix_unit(r, xs[e[u] + j], w, w1);
          o[e[u] + j] = r;
        }
      }
    }
  }
}

template <class T>
static void mix_batch_launch(const void* x, void* out, int64_t B, int64_t n, int64_t H, int64_t W, bool vec,
                             int64_t bpi, const vit_mix_item* items, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T), U = 4;
  const unsigned grid = (unsigned)(bpi * B);
  if (vec)
    mix_batch_kernel<T, VEC, U><<<grid, 256, 0, s>>>((const T*)x, (T*)out, items, (uint32_t)(n / VEC),
                                                     (uint32_t)(W / VEC), (uint32_t)H, (uint32_t)bpi, n);
  else
    mix_batch_kernel<T, 1, U><<<grid, 256, 0, s>>>((const T*)x, (T*)out, items, (uint32_t)n, (uint32_t)W,
                                                   (uint32_t)H, (uint32_t)bpi, n);
}

// The coefficient launch and the apply launch (the form chosen as vit_hip.h states) of one augmented batch.
template <class TO>
static void augment_launch(const void* src, const int64_t* meta, const vit_aug_item* items_dev, int64_t B,
                           int64_t out_h, int64_t out_w, int64_t ksize, const AugNorm& nm, float erase_value, TO* out,
                           void* workspace, hipStream_t s) {
  int* tab = (int*)workspace;
  const int oh = (int)out_h, ow = (int)out_w, ks = (int)ksize;
  const uint8_t* sp = (const uint8_t*)src;
  dim3 g1((unsigned)((ow + oh + 255) / 256), (unsigned)B);
  augment_coeffs_kernel<<<g1, 256, 0, s>>>(meta, items_dev, oh, ow, ks, tab);
  const int64_t path = vit::opt(vit::OPT_AUGMENT_PATH);
  const bool tiled = path == 2 || (path != 1 && ks <= AUG_TILED_MAX_KS);
  if (tiled) {
    dim3 g2((unsigned)((ow + VIT_AUG_TILE_COLS - 1) / VIT_AUG_TILE_COLS),
            (unsigned)((oh + VIT_AUG_TILE_ROWS - 1) / VIT_AUG_TILE_ROWS), (unsigned)B);
    augment_tiled_kernel<TO><<<g2, 256, 0, s>>>(sp, meta, items_dev, oh, ow, ks, tab, nm, erase_value, out);
  } else {
    dim3 g2((unsigned)((ow + 255) / 256), (unsigned)oh, (unsigned)B);
    augment_apply_kernel<TO><<<g2, 256, 0, s>>>(sp, meta, items_dev, oh, ow, ks, tab, nm, erase_value, out);
  }
}

}  // namespace

extern "C" int vit_resize_ksize(int64_t in_size, int64_t out_size) {
  if (in_size <= 0 || out_size <= 0) return -1;
  const double scale = (double)in_size / (double)out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(support) * 2 + 1;
}

extern "C" int64_t vit_resize_workspace_bytes(int64_t B, int64_t out_h, int64_t out_w, int64_t ksize) {
  return B * (out_h + out_w) * (2 + ksize) * (int64_t)sizeof(int);
}

extern "C" int vit_resize_to_tensor(const void* src, const int64_t* meta, int64_t B, int64_t out_h, int64_t out_w,
                                    int64_t ksize, void* out, int32_t out_dtype, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  VIT_REQUIRE(src && meta && out && workspace && B > 0 && out_h > 0 && out_w > 0 && ksize >= 3,
              "vit_resize_to_tensor: bad arguments");
  VIT_REQUIRE(out_h <= 65535 && B <= 65535 && ksize <= 4096, "vit_resize_to_tensor: size out of range");
  VIT_REQUIRE(workspace_bytes >= vit_resize_workspace_bytes(B, out_h, out_w, ksize),
              "vit_resize_to_tensor: workspace too small");
  VIT_REQUIRE(out_dtype == VIT_F32 || out_dtype == VIT_BF16, "vit_resize_to_tensor: bad out dtype");
  hipStream_t s = VIT_STREAM(stream);
  int* tab = (int*)workspace;
  const int oh = (int)out_h, ow = (int)out_w, ks = (int)ksize;
  dim3 g1((unsigned)((ow + oh + 255) / 256), (unsigned)B);
  resize_coeffs_kernel<<<g1, 256, 0, s>>>(meta, oh, ow, ks, tab);
  dim3 g2((unsigned)((ow + 255) / 256), (unsigned)oh, (unsigned)B);
  if (out_dtype == VIT_F32)
    resize_apply_kernel<float><<<g2, 256, 0, s>>>((const uint8_t*)src, meta, oh, ow, ks, tab, (float*)out);
  else
    resize_apply_kernel<bf16_t><<<g2, 256, 0, s>>>((const uint8_t*)src, meta, oh, ow, ks, tab, (bf16_t*)out);
  return vit::check_launch("vit_resize_to_tensor");
}

extern "C" int64_t vit_augment_workspace_bytes(int64_t B, int64_t out_h, int64_t out_w, int64_t ksize) {
  return vit_resize_workspace_bytes(B, out_h, out_w, ksize);       // the same tables, of the crops
}

extern "C" int vit_augment_to_tensor(const void* src, const int64_t* meta, const vit_aug_item* items_dev, int64_t B,
                                     int64_t out_h, int64_t out_w, int64_t ksize, const float* mean3,
                                     const float* std3, float erase_value, void* out, int32_t out_dtype,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  VIT_REQUIRE(src && meta && items_dev && out && workspace, "vit_augment_to_tensor: null pointer");
  VIT_REQUIRE(B > 0 && out_h > 0 && out_w > 0 && ksize >= 3, "vit_augment_to_tensor: bad arguments");
  VIT_REQUIRE(out_h <= 65535 && B <= 65535 && ksize <= 4096, "vit_augment_to_tensor: size out of range");
  VIT_REQUIRE((mean3 == nullptr) == (std3 == nullptr), "vit_augment_to_tensor: mean3 and std3 go together");
  AugNorm nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, 0};
  if (mean3) {
    for (int c = 0; c < 3; ++c) {
      VIT_REQUIRE(isfinite(mean3[c]) && isfinite(std3[c]) && std3[c] != 0.f,
                  "vit_augment_to_tensor: mean must be finite and std finite and non-zero (channel %d: %g, %g)", c,
                  (double)mean3[c], (double)std3[c]);
      nm.mean[c] = mean3[c];
      nm.sd[c] = std3[c];
    }
    nm.on = 1;
  }
  VIT_REQUIRE(isfinite(erase_value), "vit_augment_to_tensor: erase_value is not finite");
  VIT_REQUIRE(out_dtype == VIT_F32 || out_dtype == VIT_BF16, "vit_augment_to_tensor: bad out dtype");
  VIT_REQUIRE(workspace_bytes >= vit_augment_workspace_bytes(B, out_h, out_w, ksize),
              "vit_augment_to_tensor: workspace too small");
  hipStream_t s = VIT_STREAM(stream);
  if (out_dtype == VIT_F32)
    augment_launch<float>(src, meta, items_dev, B, out_h, out_w, ksize, nm, erase_value, (float*)out, workspace, s);
  else
    augment_launch<bf16_t>(src, meta, items_dev, B, out_h, out_w, ksize, nm, erase_value, (bf16_t*)out, workspace, s);
  return vit::check_launch("vit_augment_to_tensor");
}

extern "C" int vit_augment_to_u8(const void* src, const int64_t* meta, const vit_aug_item* items_dev, int64_t B,
                                 int64_t out_h, int64_t out_w, int64_t ksize, void* out_u8, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  VIT_REQUIRE(src && meta && items_dev && out_u8 && workspace, "vit_augment_to_u8: null pointer");
  VIT_REQUIRE(B > 0 && out_h > 0 && out_w > 0 && ksize >= 3, "vit_augment_to_u8: bad arguments");
  VIT_REQUIRE(out_h <= 65535 && B <= 65535 && ksize <= 4096, "vit_augment_to_u8: size out of range");
  VIT_REQUIRE(workspace_bytes >= vit_augment_workspace_bytes(B, out_h, out_w, ksize),
              "vit_augment_to_u8: workspace too small");
  const AugNorm nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, 0};
  augment_launch<uint8_t>(src, meta, items_dev, B, out_h, out_w, ksize, nm, 0.f, (uint8_t*)out_u8, workspace,
                          VIT_STREAM(stream));
  return vit::check_launch("vit_augment_to_u8");
}

extern "C" int vit_mix_batch(const void* x, void* out, int32_t dtype, int64_t B, int64_t C, int64_t H, int64_t W,
                             const vit_mix_item* items_dev, void* stream) {
  VIT_REQUIRE(x && out && items_dev, "vit_mix_batch: null pointer");
  VIT_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "vit_mix_batch: non-positive dimension (B %lld, C %lld, H %lld, W %lld)",
              (long long)B, (long long)C, (long long)H, (long long)W);
  VIT_REQUIRE(dtype == VIT_F32 || dtype == VIT_BF16, "vit_mix_batch: bad dtype %d", (int)dtype);
  const int64_t lim = 0x7fffffff, esize = dtype == VIT_F32 ? 4 : 2;
  // one image is indexed in 32 bits, the batch in 64
  VIT_REQUIRE(C <= lim && H <= lim && W <= lim && C * H <= lim / W, "vit_mix_batch: an image of 2^31 elements or more");
  const int64_t n = C * H * W;
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  const bool vec = ((xa | oa) & 15) == 0 && (W * esize) % 16 == 0;
  const int64_t nu = vec ? n / (16 / esize) : n;
  const int64_t bpi = (nu + 1023) / 1024;         // 256 lanes x 4 units per workgroup
  VIT_REQUIRE(B <= lim / bpi, "vit_mix_batch: batch too large (%lld workgroups)", (long long)B * (long long)bpi);
  const uint64_t bytes = (uint64_t)B * (uint64_t)n * (uint64_t)esize;
  // the mix reads image src after writing image i: in place (or any overlap) cannot be right
  VIT_REQUIRE(xa + bytes <= oa || oa + bytes <= xa, "vit_mix_batch: out overlaps x");
  hipStream_t s = VIT_STREAM(stream);
  if (dtype == VIT_F32) mix_batch_launch<float>(x, out, B, n, H, W, vec, bpi, items_dev, s);
  else mix_batch_launch<bf16_t>(x, out, B, n, H, W, vec, bpi, items_dev, s);
  return vit::check_launch("vit_mix_batch");
}
