// RandAugment chains on the GPU (vit_hip.h "RandAugment"): up to VIT_RA_MAX_LAYERS image operations per image on the
// uint8 HWC RGB picture that vit_augment_to_u8 stored, every one bit-exact with the Pillow call it stands for, then
// the tensor store of vit_augment_to_tensor (value, erase).  Per layer:
//   * ra_stats_kernel, only when the caller names the layer in stats_layers: one workgroup per image whose kind needs
//     the picture's histograms (AUTOCONTRAST, EQUALIZE, CONTRAST) builds them in LDS and writes the image's
//     [3][256] lookup table;
//   * ra_apply_kernel: the image's kind is workgroup-uniform and selects one of three bodies — a lookup table (built
//     in LDS from the layer's arguments, or fetched from the statistics launch), a blend with a degenerate picture
//     (COLOR: the pixel's gray; SHARPNESS: the 3x3 smooth), or the affine bilinear gather.
// The arithmetic Pillow does in C float / double (the blend, the smooth filter, the affine gather) and in Python float
// (the autocontrast table) is done here in fp32 / fp64 with FP contraction OFF: Pillow's x86-64 build has no FMA, and a
// fused form differs exactly where a result sits on an integer.  Those functions are host-callable too, so a CPU
// program can run the very same code against Pillow.
#include <math.h>

#include "vit_common.h"

namespace {

#define VIT_HD __host__ __device__ __forceinline__

VIT_HD int ra_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Image.blend(degenerate, image, f) of one channel: d + f * (v - d) in fp32, product and sum rounded separately;
// truncated for 0 <= f <= 1 (the value is in [0, 255] there), clipped and truncated otherwise.
VIT_HD int ra_blend(int d, int v, float f) {
#pragma clang fp contract(off)
  const float t = (float)d + f * (float)(v - d);
  if (!(t > 0.0f)) return 0;          // also a NaN factor: a wrong picture, not an undefined conversion
  if (t >= 255.0f) return 255;
  return (int)t;
}

// convert('L'): ITU-R 601-2 luma in 16-bit fixed point
VIT_HD int ra_gray(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// The lookup tables that need no statistics, entry i.
VIT_HD int ra_point(int kind, int iarg0, int iarg1, float farg, int i) {
  switch (kind) {
    case VIT_RA_INVERT:
      return 255 - i;
    case VIT_RA_POSTERIZE:
      return i & ~((1 << (8 - ra_clamp(iarg0, 0, 8))) - 1);
    case VIT_RA_SOLARIZE:
      return i < ra_clamp(iarg0, 0, 256) ? i : 255 - i;
    case VIT_RA_SOLARIZE_ADD: {
      const int s = i + ra_clamp(iarg0, 0, 255);
      return i < ra_clamp(iarg1, 0, 256) ? (s > 255 ? 255 : s) : i;
    }
    case VIT_RA_BRIGHTNESS:
      return ra_blend(0, i, farg);
    default:
      return i;
  }
}

// ImageOps.autocontrast's table of one channel whose lowest / highest value present is lo / hi, entry i: Python floats.
VIT_HD int ra_autocontrast_entry(int i, int lo, int hi) {
#pragma clang fp contract(off)
  if (hi <= lo) return i;
  const double scale = 255.0 / (double)(hi - lo);
  const double offset = (double)(-lo) * scale;
  const double v = (double)i * scale + offset;
  return v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v);
}

// ImageOps.equalize's table of one channel, entry i: `below` pixels have a value under i, `nz` values are present,
// step = (pixels - count of the highest value present) / 255.  Image.point clips an entry above 255.
VIT_HD int ra_equalize_entry(int i, uint32_t below, uint32_t step, int nz) {
  if (nz <= 1 || step == 0) return i;
  const uint32_t v = (step / 2 + below) / step;
  return v > 255u ? 255 : (int)v;
}

// ImageStat.Stat(gray).mean -> Contrast's degenerate level: the exact sum over the count in fp64, plus 0.5, truncated
VIT_HD int ra_contrast_level(uint64_t graysum, uint32_t pixels) {
#pragma clang fp contract(off)
  const double mean = (double)graysum / (double)pixels;
  return ra_clamp((int)(mean + 0.5), 0, 255);
}

// ImageFilter.SMOOTH of channel c at an INTERIOR pixel (1 <= x <= W-2, 1 <= y <= H-2): Pillow's float 3x3 filter — the
// weights are the fp32 quotients by 13, the sum starts at 0.5 and takes one row's three products at a time, the row
// below first.
VIT_HD int ra_smooth(const uint8_t* __restrict__ img, int W, int x, int y, int c) {
#pragma clang fp contract(off)
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  const uint8_t* p = img + ((int64_t)y * W + x) * 3 + c;
  const int64_t row = (int64_t)W * 3;
  float ss = 0.5f;
  ss += (float)p[row - 3] * k1 + (float)p[row] * k1 + (float)p[row + 3] * k1;
  ss += (float)p[-3] * k1 + (float)p[0] * k5 + (float)p[3] * k1;
  ss += (float)p[-row - 3] * k1 + (float)p[-row] * k1 + (float)p[-row + 3] * k1;
  if (!(ss > 0.0f)) return 0;
  if (ss >= 255.0f) return 255;
  return (int)ss;
}

// Image.transform(size, AFFINE, a, BILINEAR, fillcolor) at output pixel (x, y) of an H x W picture: see vit_hip.h.
// Every tap is clamped into the picture whatever the coefficients are; NaN fails the window test and gives the fill.
VIT_HD void ra_affine_pixel(const uint8_t* __restrict__ img, int H, int W, const double* a, const uint8_t* fill, int x,
                            int y, int px[3]) {
#pragma clang fp contract(off)
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  double xin = a[0] * xc + a[1] * yc + a[2];
  double yin = a[3] * xc + a[4] * yc + a[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
    px[0] = fill[0];
    px[1] = fill[1];
    px[2] = fill[2];
    return;
  }
  xin -= 0.5;
  yin -= 0.5;
  const int x0 = (int)floor(xin), y0 = (int)floor(yin);       // in [-1, W-1] x [-1, H-1]
  const double dx = xin - (double)x0, dy = yin - (double)y0;
  const int xa = ra_clamp(x0, 0, W - 1), xb = ra_clamp(x0 + 1, 0, W - 1);
  const bool below = y0 + 1 >= 0 && y0 + 1 < H;
  const uint8_t* r0 = img + (int64_t)ra_clamp(y0, 0, H - 1) * W * 3;
  const uint8_t* r1 = img + (int64_t)ra_clamp(y0 + 1, 0, H - 1) * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double p00 = (double)r0[xa * 3 + c], p01 = (double)r0[xb * 3 + c];
    const double v1 = p00 + (p01 - p00) * dx;
    double v2 = v1;
    if (below) {
      const double p10 = (double)r1[xa * 3 + c], p11 = (double)r1[xb * 3 + c];
      v2 = p10 + (p11 - p10) * dx;
    }
    const double v = v1 + (v2 - v1) * dy;
    px[c] = ra_clamp((int)v, 0, 255);
  }
}

VIT_HD bool ra_needs_stats(int kind) {
  return kind == VIT_RA_AUTOCONTRAST || kind == VIT_RA_EQUALIZE || kind == VIT_RA_CONTRAST;
}

VIT_HD bool ra_is_table(int kind) {
  return ra_needs_stats(kind) || kind == VIT_RA_INVERT || kind == VIT_RA_POSTERIZE || kind == VIT_RA_SOLARIZE ||
         kind == VIT_RA_SOLARIZE_ADD || kind == VIT_RA_BRIGHTNESS;
}

// One workgroup per image.  An image whose kind in this layer needs no histogram leaves at once.  Histograms 0..2:
// the channels (AUTOCONTRAST, EQUALIZE); histogram 3: the gray picture (CONTRAST).  Lanes 0..2 then walk their
// channel's histogram once (lowest / highest value present, values present, pixels below each value) and lane 3 sums
// the gray one; every lane writes entry threadIdx.x of the three tables.  All integer: the order of the LDS atomics
// does not show.
__global__ __launch_bounds__(256) void ra_stats_kernel(const uint8_t* __restrict__ in,
                                                       const vit_ra_item* __restrict__ items, int layer, int H, int W,
                                                       uint8_t* __restrict__ lut) {
  const int b = blockIdx.x;
  const vit_ra_layer& ly = items[b].layer[layer];
  const int kind = ly.kind;
  if (!ra_needs_stats(kind)) return;
  __shared__ uint32_t hist[4][256];
  __shared__ uint32_t below[3][256];
  __shared__ int lo[3], hi[3], nz[3];
  __shared__ uint32_t step[3];
  __shared__ int level;
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) hist[k][t] = 0;
  __syncthreads();
  const uint32_t npix = (uint32_t)H * (uint32_t)W;
  const uint8_t* img = in + (int64_t)b * npix * 3;
  for (uint32_t p = t; p < npix; p += 256) {
    const int r = img[(int64_t)p * 3], g = img[(int64_t)p * 3 + 1], bl = img[(int64_t)p * 3 + 2];
    if (kind == VIT_RA_CONTRAST) {
      atomicAdd(&hist[3][ra_gray(r, g, bl)], 1u);
    } else {
      atomicAdd(&hist[0][r], 1u);
      atomicAdd(&hist[1][g], 1u);
      atomicAdd(&hist[2][bl], 1u);
    }
  }
  __syncthreads();
  if (t < 3) {
    int l = 256, h = -1, n = 0;
    uint32_t run = 0, last = 0;
    for (int i = 0; i < 256; ++i) {
      const uint32_t c = hist[t][i];
      below[t][i] = run;
      run += c;
      if (c) {
        if (l == 256) l = i;
        h = i;
        ++n;
        last = c;
      }
    }
    lo[t] = l;
    hi[t] = h;
    nz[t] = n;
    step[t] = (npix - last) / 255u;
  } else if (t == 3) {
    uint64_t sum = 0;
    for (int i = 0; i < 256; ++i) sum += (uint64_t)i * hist[3][i];
    level = ra_contrast_level(sum, npix);
  }
  __syncthreads();
  uint8_t* o = lut + (int64_t)b * 768;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int v;
    if (kind == VIT_RA_AUTOCONTRAST) v = ra_autocontrast_entry(t, lo[c], hi[c]);
    else if (kind == VIT_RA_EQUALIZE) v = ra_equalize_entry(t, below[c][t], step[c], nz[c]);
    else v = ra_blend(level, t, ly.farg);
    o[c * 256 + t] = (uint8_t)v;
  }
}

typedef uint32_t ra_u32x4 __attribute__((ext_vector_type(4)));

// PX pixels per lane: 16 (48 bytes, three 16-byte accesses; the host chooses it where the picture's bytes and the
// buffers allow) or 1.  upi: units of PX pixels per image.  The kind, hence the body, is workgroup-uniform.
template <int PX>
__global__ __launch_bounds__(256) void ra_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                       const vit_ra_item* __restrict__ items, int layer, int H, int W,
                                                       const uint8_t* __restrict__ lut_g, uint32_t upi) {
  constexpr int NB = PX * 3, NW = (NB + 3) / 4;
  __shared__ uint8_t lut[768];
  const int b = blockIdx.y;
  const vit_ra_layer& ly = items[b].layer[layer];
  const int kind = ly.kind;
  const int64_t n = (int64_t)H * W * 3;
  const uint8_t* img = in + b * n;
  const bool table = ra_is_table(kind);
  if (table) {
    const int i0 = ly.iarg0, i1 = ly.iarg1;
    const float f = ly.farg;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      lut[c * 256 + threadIdx.x] = ra_needs_stats(kind) ? lut_g[(int64_t)b * 768 + c * 256 + threadIdx.x]
                                                        : (uint8_t)ra_point(kind, i0, i1, f, (int)threadIdx.x);
    __syncthreads();
  }
  const uint32_t u = blockIdx.x * 256u + threadIdx.x;
  if (u >= upi) return;
  const uint32_t p0 = u * PX;                 // first pixel of the unit
  uint32_t w[NW];                             // the unit's bytes: read (elementwise kinds), then written
  const bool gather = kind == VIT_RA_SHARPNESS || kind == VIT_RA_AFFINE;
  if (!gather) {
    if constexpr (PX == 16) {
      const ra_u32x4* p = reinterpret_cast<const ra_u32x4*>(img + (int64_t)p0 * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const ra_u32x4 v = p[k];
        w[4 * k] = v[0], w[4 * k + 1] = v[1], w[4 * k + 2] = v[2], w[4 * k + 3] = v[3];
      }
    } else {
      const uint8_t* p = img + (int64_t)p0 * 3;
      w[0] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
  }
  uint32_t o[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) o[k] = 0;
  if (kind == VIT_RA_AFFINE) {
    double a[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = ly.coef[k];
    const uint8_t fill[3] = {ly.fill[0], ly.fill[1], ly.fill[2]};
    int y = (int)(p0 / (uint32_t)W), x = (int)(p0 - (uint32_t)y * (uint32_t)W);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      int px[3];
      ra_affine_pixel(img, H, W, a, fill, x, y, px);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[(3 * j + c) >> 2] |= (uint32_t)px[c] << (((3 * j + c) & 3) * 8);
      if (++x == W) x = 0, ++y;
    }
  } else if (kind == VIT_RA_SHARPNESS) {
    const float f = ly.farg;
    int y = (int)(p0 / (uint32_t)W), x = (int)(p0 - (uint32_t)y * (uint32_t)W);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const bool inner = x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2;
      const uint8_t* p = img + ((int64_t)y * W + x) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v = p[c];
        const int r = ra_blend(inner ? ra_smooth(img, W, x, y, c) : v, v, f);
        o[(3 * j + c) >> 2] |= (uint32_t)r << (((3 * j + c) & 3) * 8);
      }
      if (++x == W) x = 0, ++y;
    }
  } else if (kind == VIT_RA_COLOR) {
    const float f = ly.farg;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      int v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (int)((w[(3 * j + c) >> 2] >> (((3 * j + c) & 3) * 8)) & 255u);
      const int g = ra_gray(v[0], v[1], v[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[(3 * j + c) >> 2] |= (uint32_t)ra_blend(g, v[c], f) << (((3 * j + c) & 3) * 8);
    }
  } else if (table) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
      o[j >> 2] |= (uint32_t)lut[(j % 3) * 256 + ((w[j >> 2] >> ((j & 3) * 8)) & 255u)] << ((j & 3) * 8);
  } else {                                    // VIT_RA_NONE and every unknown kind: a copy
#pragma unroll
    for (int k = 0; k < NW; ++k) o[k] = w[k];
  }
  uint8_t* q = out + b * n + (int64_t)p0 * 3;
  if constexpr (PX == 16) {
    ra_u32x4* qv = reinterpret_cast<ra_u32x4*>(q);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ra_u32x4 v = {o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
      qv[k] = v;
    }
  } else {
    q[0] = (uint8_t)o[0];
    q[1] = (uint8_t)(o[0] >> 8);
    q[2] = (uint8_t)(o[0] >> 16);
  }
}

// The tensor store of vit_augment_to_tensor from the finished uint8 picture: one lane per pixel, CHW planes.
template <class TO>
__global__ __launch_bounds__(256) void ra_finish_kernel(const uint8_t* __restrict__ in,
                                                        const vit_aug_item* __restrict__ items, int H, int W,
                                                        AugNorm nm, float ev, TO* __restrict__ out) {
  const int b = blockIdx.z;
  const int y = blockIdx.y;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= W) return;
  const vit_aug_item it = items[b];
  const int64_t plane = (int64_t)H * W;
  TO* o = out + (int64_t)b * 3 * plane + (int64_t)y * W + x;
  if (aug_erased(it, y, x)) {
    st1<TO>(o, ev);
    st1<TO>(o + plane, ev);
    st1<TO>(o + 2 * plane, ev);
    return;
  }
  const uint8_t* p = in + ((int64_t)b * plane + (int64_t)y * W + x) * 3;
  st1<TO>(o, aug_value(p[0], nm.mean[0], nm.sd[0], nm.on));
  st1<TO>(o + plane, aug_value(p[1], nm.mean[1], nm.sd[1], nm.on));
  st1<TO>(o + 2 * plane, aug_value(p[2], nm.mean[2], nm.sd[2], nm.on));
}

constexpr int64_t RA_ALIGN = 256;
int64_t ra_picture_bytes(int64_t B, int64_t H, int64_t W) { return (B * H * W * 3 + RA_ALIGN - 1) / RA_ALIGN * RA_ALIGN; }

}  // namespace

// Workspace: two uint8 pictures of the batch, which take turns, and the [B][3][256] tables of one layer.
extern "C" int64_t vit_randaug_workspace_bytes(int64_t B, int64_t S_h, int64_t S_w) {
  if (B <= 0 || S_h <= 0 || S_w <= 0) return -1;
  return 2 * ra_picture_bytes(B, S_h, S_w) + B * 768;
}

extern "C" int vit_randaug_to_tensor(const void* u8_in, const vit_ra_item* items_dev, int64_t B, int64_t S_h,
                                     int64_t S_w, int32_t nlayers, int32_t stats_layers, const float* mean3,
                                     const float* std3, const vit_aug_item* erase_items_dev, float erase_value,
                                     void* out, int32_t out_dtype, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  VIT_REQUIRE(u8_in && items_dev && erase_items_dev && out && workspace, "vit_randaug_to_tensor: null pointer");
  VIT_REQUIRE(B > 0 && S_h > 0 && S_w > 0, "vit_randaug_to_tensor: bad arguments");
  VIT_REQUIRE(S_h <= 65535 && B <= 65535 && S_w <= 0x7fffffff / 3 / S_h,
              "vit_randaug_to_tensor: size out of range (an image of 2^31 bytes or more, or more than 65535 rows or "
              "images)");
  VIT_REQUIRE(nlayers >= 1 && nlayers <= VIT_RA_MAX_LAYERS, "vit_randaug_to_tensor: nlayers %d outside [1, %d]",
              (int)nlayers, VIT_RA_MAX_LAYERS);
  VIT_REQUIRE(stats_layers >= 0 && (stats_layers >> nlayers) == 0,
              "vit_randaug_to_tensor: stats_layers %d names a layer at or above nlayers %d", (int)stats_layers,
              (int)nlayers);
  VIT_REQUIRE((mean3 == nullptr) == (std3 == nullptr), "vit_randaug_to_tensor: mean3 and std3 go together");
  AugNorm nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, 0};
  if (mean3) {
    for (int c = 0; c < 3; ++c) {
      VIT_REQUIRE(isfinite(mean3[c]) && isfinite(std3[c]) && std3[c] != 0.f,
                  "vit_randaug_to_tensor: mean must be finite and std finite and non-zero (channel %d: %g, %g)", c,
                  (double)mean3[c], (double)std3[c]);
      nm.mean[c] = mean3[c];
      nm.sd[c] = std3[c];
    }
    nm.on = 1;
  }
  VIT_REQUIRE(isfinite(erase_value), "vit_randaug_to_tensor: erase_value is not finite");
  VIT_REQUIRE(out_dtype == VIT_F32 || out_dtype == VIT_BF16, "vit_randaug_to_tensor: bad out dtype");
  VIT_REQUIRE(workspace_bytes >= vit_randaug_workspace_bytes(B, S_h, S_w), "vit_randaug_to_tensor: workspace too small");
  const int H = (int)S_h, W = (int)S_w;
  const int64_t npix = S_h * S_w, pic = ra_picture_bytes(B, S_h, S_w);
  const uintptr_t oa = (uintptr_t)out, ob = (uint64_t)B * npix * 3 * (out_dtype == VIT_F32 ? 4 : 2);
  const uintptr_t wa = (uintptr_t)workspace, ia = (uintptr_t)u8_in;
  const uintptr_t wb = (uint64_t)workspace_bytes, ib = (uint64_t)B * npix * 3;
  VIT_REQUIRE((oa + ob <= wa || wa + wb <= oa) && (oa + ob <= ia || ia + ib <= oa) && (ia + ib <= wa || wa + wb <= ia),
              "vit_randaug_to_tensor: out, the workspace and u8_in must not overlap");
  hipStream_t s = VIT_STREAM(stream);
  uint8_t* buf[2] = {(uint8_t*)workspace, (uint8_t*)workspace + pic};
  uint8_t* lut = (uint8_t*)workspace + 2 * pic;
  // 16 pixels (48 bytes) per lane where every image starts on a 16-byte boundary in all three pictures
  const bool vec = npix % 16 == 0 && ((ia | wa) & 15) == 0;
  const int64_t upi = vec ? npix / 16 : npix;
  dim3 ga((unsigned)((upi + 255) / 256), (unsigned)B);
  const uint8_t* cur = (const uint8_t*)u8_in;
  for (int l = 0; l < nlayers; ++l) {
    if ((stats_layers >> l) & 1) ra_stats_kernel<<<(unsigned)B, 256, 0, s>>>(cur, items_dev, l, H, W, lut);
    uint8_t* nxt = buf[l & 1];
    if (vec) ra_apply_kernel<16><<<ga, 256, 0, s>>>(cur, nxt, items_dev, l, H, W, lut, (uint32_t)upi);
    else ra_apply_kernel<1><<<ga, 256, 0, s>>>(cur, nxt, items_dev, l, H, W, lut, (uint32_t)upi);
    cur = nxt;
  }
  dim3 gf((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)B);
  if (out_dtype == VIT_F32)
    ra_finish_kernel<float><<<gf, 256, 0, s>>>(cur, erase_items_dev, H, W, nm, erase_value, (float*)out);
  else
    ra_finish_kernel<bf16_t><<<gf, 256, 0, s>>>(cur, erase_items_dev, H, W, nm, erase_value, (bf16_t*)out);
  return vit::check_launch("vit_randaug_to_tensor");
}
