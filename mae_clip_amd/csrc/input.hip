// Input pipeline on the device.
//
// Replaces the per-image host transform of dataset.py:44-58: the decoded RGB
// uint8 HWC image (cv2.imread + cvtColor, dataset.py:30-33) goes through
// albumentations Normalize(max_pixel_value=255) (dataset.py:49) and
// torch.tensor(image).permute(2, 0, 1).float() (dataset.py:34). The batch is
// uploaded as uint8 (a quarter of the fp32 bytes over PCIe) and normalised
// here, in HBM, straight into the model's NCHW fp32 input.
//
// maeclip_image_preprocess_u8 adds the resize in the same pass: images of any
// size (one descriptor each) -> A.Resize(S, S) = cv2.resize INTER_LINEAR
// (dataset.py:48; OpenCV's fixed-point uint8 algorithm, see oracle/input_ref.py)
// -> Normalize -> NCHW fp32 [B, 3, S, S]: the whole get_transforms() pipeline.
//
// Arithmetic is albumentations' normalize(): mean32 = f32(mean) * max_pixel,
// den32 = 1 / (f32(std) * max_pixel) (both fp32, computed on the host with
// IEEE division), out = (f32(x) - mean32) * den32 -- two roundings, no FMA.
// HBM-bound: 3 B read + 12 B written per pixel.
#include "common.h"
#include "../../include/maeclip.h"

namespace {
constexpr int NTH = 256;

// 4 consecutive pixels of one row per thread: three 4-B loads of interleaved
// RGB, one 16-B store per plane (W % 4 == 0)
__global__ void __launch_bounds__(NTH) normalize_u8_x4_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                               int64_t npix4, int64_t HW, NormConst k) {
  const int64_t q = (int64_t)blockIdx.x * NTH + threadIdx.x;
  if (q >= npix4) return;
  const int64_t pix = q * 4;              // global pixel index b*HW + y*W + x
  const int64_t b = pix / HW, off = pix % HW;
  const uint32_t* s = (const uint32_t*)(src + pix * 3);
  const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
  const uint8_t v[12] = {(uint8_t)w0, (uint8_t)(w0 >> 8), (uint8_t)(w0 >> 16), (uint8_t)(w0 >> 24),
                         (uint8_t)w1, (uint8_t)(w1 >> 8), (uint8_t)(w1 >> 16), (uint8_t)(w1 >> 24),
                         (uint8_t)w2, (uint8_t)(w2 >> 8), (uint8_t)(w2 >> 16), (uint8_t)(w2 >> 24)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v4f o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = mc_norm_px(v[3 * j + c], k, c);
    }
    *(v4f*)(dst + (b * 3 + c) * HW + off) = o;
  }
}

__global__ void __launch_bounds__(NTH) normalize_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                            int64_t npix, int64_t HW, NormConst k) {
  const int64_t pix = (int64_t)blockIdx.x * NTH + threadIdx.x;
  if (pix >= npix) return;
  const int64_t b = pix / HW, off = pix % HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dst[(b * 3 + c) * HW + off] = mc_norm_px(src[pix * 3 + c], k, c);
  }
}
// OpenCV INTER_LINEAR source index / fixed-point weights of output coordinate d
// (resize.cpp, CV_8U: float f from double arithmetic, weights
// saturate_cast<short>(w * 2048) = rint, borders clamp with weight 0)
struct Lin {
  int s0, s1, a0, a1;
};
__device__ __forceinline__ double lin_scale(int n_src, int n_dst) { return 1.0 / ((double)n_dst / (double)n_src); }
__device__ __forceinline__ Lin lin_coef_at(int d, int n_src, double scale) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  bool hi = false;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= n_src - 1) { s = n_src - 1; f = 0.f; hi = true; }
  Lin r;
  r.s0 = s;
  r.s1 = min(s + 1, n_src - 1);
  r.a0 = (int)rintf((1.f - f) * 2048.f);
  r.a1 = hi ? 0 : (int)rintf(f * 2048.f);
  return r;
}
__device__ __forceinline__ Lin lin_coef(int d, int n_src, int n_dst) { return lin_coef_at(d, n_src, lin_scale(n_src, n_dst)); }

// one output pixel (3 channels) per thread; grid (pixel blocks, image)
__global__ void __launch_bounds__(NTH) preprocess_u8_kernel(const maeclip_image_src* __restrict__ imgs, float* __restrict__ dst,
                                                             int S, NormConst k) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * NTH + threadIdx.x;
  if (p >= S * S) return;
  const int dy = p / S, dx = p % S;
  const maeclip_image_src im = imgs[b];
  const uint8_t* src = im.src;
  const int H = im.H, W = im.W;
  const int64_t rs = im.row_stride;
  int v[3];
  if (H == S && W == S) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = src[dy * rs + dx * 3 + c];
  } else if (H == 2 * S && W == 2 * S) {   // cv2: exact 2x -> INTER_AREA fast path
    const uint8_t* r0 = src + (int64_t)(2 * dy) * rs + 2 * dx * 3;
    const uint8_t* r1 = r0 + rs;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (r0[c] + r0[3 + c] + r1[c] + r1[3 + c] + 2) >> 2;
  } else {
    const Lin x = lin_coef(dx, W, S), y = lin_coef(dy, H, S);
    const uint8_t* r0 = src + (int64_t)y.s0 * rs;
    const uint8_t* r1 = src + (int64_t)y.s1 * rs;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int h0 = r0[x.s0 * 3 + c] * x.a0 + r0[x.s1 * 3 + c] * x.a1;
      const int h1 = r1[x.s0 * 3 + c] * x.a0 + r1[x.s1 * 3 + c] * x.a1;
      // VResizeLinearVec_32s8u: mul_hi of (h >> 4) by the int16 weight, round by 2 bits
      const int t = (((h0 >> 4) * y.a0) >> 16) + (((h1 >> 4) * y.a1) >> 16);
      v[c] = min(max((t + 2) >> 2, 0), 255);
    }
  }
  const int64_t plane = (int64_t)S * S;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[((int64_t)b * 3 + c) * plane + p] = mc_norm_px(v[c], k, c);
}

// ------------------------------------------------- RandomResizedCrop + flip
// The box of one sample, torchvision / albumentations get_params in double;
// the order of operations is the one written out at maeclip_crop_params in
// maeclip.h, and tests/augment_ref.py follows it line by line. Host and
// device evaluate this one function (no contraction into fma on either).
__host__ __device__ inline void mc_crop_draw(uint64_t step_seed, uint64_t gb, int H, int W, double s0, double s1,
                                             double r0, double r1, double flip_p, int32_t* box) {
#pragma clang fp contract(off)
  const double inv24 = 1.0 / 16777216.0;
  const double lr0 = log(r0), lr1 = log(r1);
  const double hw = (double)H * (double)W;
  int w = 0, h = 0, x0 = 0, y0 = 0;
  bool found = false;
  for (int k = 0; k < 10 && !found; ++k) {
    const double ua = (double)(mc_hash4(step_seed, gb, (uint64_t)k, 0) >> 8) * inv24;
    const double ur = (double)(mc_hash4(step_seed, gb, (uint64_t)k, 1) >> 8) * inv24;
    const double area = hw * (s0 + ua * (s1 - s0));
    const double ar = exp(lr0 + ur * (lr1 - lr0));
    const double wd = rint(sqrt(area * ar)), hd = rint(sqrt(area / ar));
    if (wd > 0.0 && wd <= (double)W && hd > 0.0 && hd <= (double)H) {
      w = (int)wd;
      h = (int)hd;
      const double uy = (double)(mc_hash4(step_seed, gb, (uint64_t)k, 2) >> 8) * inv24;
      const double ux = (double)(mc_hash4(step_seed, gb, (uint64_t)k, 3) >> 8) * inv24;
      y0 = (int)floor(uy * (double)(H - h + 1));
      x0 = (int)floor(ux * (double)(W - w + 1));
      found = true;
    }
  }
  if (!found) {
    const double in_ratio = (double)W / (double)H;
    w = W;
    h = H;
    if (in_ratio < r0) {
      h = (int)fmin(fmax(rint((double)W / r0), 1.0), (double)H);
    } else if (in_ratio > r1) {
      w = (int)fmin(fmax(rint((double)H * r1), 1.0), (double)W);
    }
    y0 = (H - h) / 2;
    x0 = (W - w) / 2;
  }
  const double uf = (double)(mc_hash4(step_seed, gb, 10, 4) >> 8) * inv24;
  box[0] = x0;
  box[1] = y0;
  box[2] = w;
  box[3] = h;
  box[4] = uf < flip_p ? 1 : 0;
}
__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// sample b of a draw (step_ptr and every array of `a` readable from the caller's side)
__host__ __device__ inline void crop_params_sample(const maeclip_crop_params_args& a, int b) {
  int H = a.H, W = a.W;
  if (a.images) {
    H = a.images[b].H;
    W = a.images[b].W;
  } else if (a.sizes) {
    H = clampi(a.sizes[2 * b], 1, a.H);
    W = clampi(a.sizes[2 * b + 1], 1, a.W);
  }
  if (H < 1) H = 1;
  if (W < 1) W = 1;
  mc_crop_draw(mc_step_seed(a.seed, a.step_ptr), a.sample_offset + (uint64_t)b, H, W, (double)a.scale[0],
               (double)a.scale[1], (double)a.ratio[0], (double)a.ratio[1], (double)a.flip_p, a.boxes + 5 * (int64_t)b);
}
__global__ void __launch_bounds__(NTH) crop_params_kernel(const maeclip_crop_params_args a) {
  const int b = blockIdx.x * NTH + threadIdx.x;
  if (b < a.B) crop_params_sample(a, b);
}

// PX consecutive pixels of one output row per thread (PX = 4: S % 4 == 0, the
// store shapes of normalize_u8_x4_kernel -- one 16-B store per fp32 plane,
// three 4-B stores of interleaved uint8; PX = 1: any S). grid (pixel blocks,
// image), so the path taken (copy / area / linear) is uniform in a block. The
// flip mirrors the resized column a thread READS (S-1-x); its stores stay in
// ascending x, consecutive lanes on consecutive addresses.
template <int PX>
__global__ void __launch_bounds__(NTH) augment_u8_kernel(const maeclip_augment_args a, NormConst k) {
  const int b = blockIdx.y, S = (int)a.S;
  const int q = blockIdx.x * NTH + threadIdx.x;
  if (q >= S * S / PX) return;
  const int p = q * PX, dy = p / S, dx = p % S;
  const uint8_t* src;
  int H, W;
  int64_t rs;
  if (a.images) {
    const maeclip_image_src im = a.images[b];
    src = im.src, H = im.H, W = im.W, rs = im.row_stride;
  } else {
    src = a.batch + (int64_t)b * a.Hmax * a.Wmax * 3;
    rs = (int64_t)a.Wmax * 3;
    H = a.sizes ? clampi(a.sizes[2 * b], 1, a.Hmax) : a.Hmax;
    W = a.sizes ? clampi(a.sizes[2 * b + 1], 1, a.Wmax) : a.Wmax;
  }
  if (H < 1 || W < 1) return;
  const int32_t* bx = a.boxes + 5 * (int64_t)b;
  const int x0 = clampi(bx[0], 0, W - 1), y0 = clampi(bx[1], 0, H - 1);
  const int w = clampi(bx[2], 1, W - x0), h = clampi(bx[3], 1, H - y0);
  const bool flip = bx[4] != 0;
  src += (int64_t)y0 * rs + (int64_t)x0 * 3;
  int v[PX][3];
  if (h == S && w == S) {
    const uint8_t* r = src + (int64_t)dy * rs;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const int sx = flip ? S - 1 - (dx + j) : dx + j;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[j][c] = r[sx * 3 + c];
    }
  } else if (h == 2 * S && w == 2 * S) {   // cv2: exact 2x -> INTER_AREA fast path
    const uint8_t* r0 = src + (int64_t)(2 * dy) * rs;
    const uint8_t* r1 = r0 + rs;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const int sx = 2 * (flip ? S - 1 - (dx + j) : dx + j) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[j][c] = (r0[sx + c] + r0[sx + 3 + c] + r1[sx + c] + r1[sx + 3 + c] + 2) >> 2;
    }
  } else {
    const double xscale = lin_scale(w, S);
    const Lin y = lin_coef(dy, h, S);
    const uint8_t* r0 = src + (int64_t)y.s0 * rs;
    const uint8_t* r1 = src + (int64_t)y.s1 * rs;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const Lin x = lin_coef_at(flip ? S - 1 - (dx + j) : dx + j, w, xscale);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int h0 = r0[x.s0 * 3 + c] * x.a0 + r0[x.s1 * 3 + c] * x.a1;
        const int h1 = r1[x.s0 * 3 + c] * x.a0 + r1[x.s1 * 3 + c] * x.a1;
        const int t = (((h0 >> 4) * y.a0) >> 16) + (((h1 >> 4) * y.a1) >> 16);   // as preprocess_u8_kernel
        v[j][c] = min(max((t + 2) >> 2, 0), 255);
      }
    }
  }
  const int64_t plane = (int64_t)S * S;
  if (a.dst_f32) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* d = a.dst_f32 + ((int64_t)b * 3 + c) * plane + p;
      if constexpr (PX == 4) {
        v4f o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = mc_norm_px(v[j][c], k, c);
        *(v4f*)d = o;
      } else {
        d[0] = mc_norm_px(v[0][c], k, c);
      }
    }
  }
  if (a.dst_u8) {
    uint8_t* d = a.dst_u8 + ((int64_t)b * plane + p) * 3;
    if constexpr (PX == 4) {
      uint32_t o[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        o[i] = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n) o[i] |= (uint32_t)v[(4 * i + n) / 3][(4 * i + n) % 3] << (8 * n);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) ((uint32_t*)d)[i] = o[i];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c] = (uint8_t)v[0][c];
    }
  }
}
}  // namespace

static int32_t crop_params_check(const maeclip_crop_params_args* a, const char* who) {
  MC_CHECK_ARG(a && a->boxes, "%s: null pointer", who);
  MC_CHECK_ARG(a->B >= 0, "%s: B must be >= 0", who);
  MC_CHECK_ARG(a->images || (a->H > 0 && a->W > 0), "%s: needs image descriptors or H, W > 0", who);
  MC_CHECK_ARG(a->scale[0] > 0.f && a->scale[0] <= a->scale[1] && a->scale[1] <= 1.f,
               "%s: scale must satisfy 0 < s0 <= s1 <= 1", who);
  MC_CHECK_ARG(a->ratio[0] > 0.f && a->ratio[0] <= a->ratio[1] && a->ratio[1] < INFINITY,
               "%s: ratio must satisfy 0 < r0 <= r1", who);
  MC_CHECK_ARG(a->flip_p >= 0.f && a->flip_p <= 1.f, "%s: flip_p must be in [0, 1]", who);
  return 0;
}

extern "C" int32_t maeclip_crop_params(const maeclip_crop_params_args* a, void* stream) {
  if (int32_t rc = crop_params_check(a, "maeclip_crop_params")) return rc;
  if (a->B == 0) return 0;
  hipLaunchKernelGGL(crop_params_kernel, dim3((unsigned)((a->B + NTH - 1) / NTH)), dim3(NTH), 0, (hipStream_t)stream,
                     *a);
  MC_CHECK_LAUNCH("maeclip_crop_params");
  return 0;
}

extern "C" int32_t maeclip_crop_params_host(const maeclip_crop_params_args* a) {
  if (int32_t rc = crop_params_check(a, "maeclip_crop_params_host")) return rc;
  for (int b = 0; b < a->B; ++b) crop_params_sample(*a, b);
  return 0;
}

extern "C" int32_t maeclip_image_augment_u8(const maeclip_augment_args* a, void* stream) {
  MC_CHECK_ARG(a && a->boxes, "maeclip_image_augment_u8: null pointer");
  MC_CHECK_ARG(a->B >= 0 && a->S > 0 && a->S <= 8192 && a->B <= 65535, "maeclip_image_augment_u8: bad sizes");
  MC_CHECK_ARG((a->images != nullptr) != (a->batch != nullptr),
               "maeclip_image_augment_u8: exactly one source (images or batch)");
  MC_CHECK_ARG(a->images || (a->Hmax > 0 && a->Wmax > 0), "maeclip_image_augment_u8: bad batch slot size");
  MC_CHECK_ARG(a->dst_f32 || a->dst_u8, "maeclip_image_augment_u8: no destination");
  NormConst k;
  MC_CHECK_ARG(mc_norm_const(a->mean, a->std, a->max_pixel, k),
               "maeclip_image_augment_u8: std and max_pixel must be > 0");
  if (a->B == 0) return 0;
  const int S = (int)a->S;
  const bool vec = S % 4 == 0 && ((uintptr_t)a->dst_f32 & 15) == 0 && ((uintptr_t)a->dst_u8 & 3) == 0;
  const int n = vec ? S * S / 4 : S * S;
  const dim3 grid((unsigned)((n + NTH - 1) / NTH), (unsigned)a->B);
  if (vec) {
    hipLaunchKernelGGL(augment_u8_kernel<4>, grid, dim3(NTH), 0, (hipStream_t)stream, *a, k);
  } else {
    hipLaunchKernelGGL(augment_u8_kernel<1>, grid, dim3(NTH), 0, (hipStream_t)stream, *a, k);
  }
  MC_CHECK_LAUNCH("maeclip_image_augment_u8");
  return 0;
}

extern "C" int32_t maeclip_image_preprocess_u8(const maeclip_preprocess_args* a, void* stream) {
  MC_CHECK_ARG(a && a->images && a->dst, "maeclip_image_preprocess_u8: null pointer");
  MC_CHECK_ARG(a->B >= 0 && a->S > 0 && a->S <= 8192 && a->B <= 65535, "maeclip_image_preprocess_u8: bad sizes");
  NormConst k;
  MC_CHECK_ARG(mc_norm_const(a->mean, a->std, a->max_pixel, k),
               "maeclip_image_preprocess_u8: std and max_pixel must be > 0");
  if (a->B == 0) return 0;
  const int S = (int)a->S;
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3((unsigned)((S * S + NTH - 1) / NTH), (unsigned)a->B), dim3(NTH), 0,
                     (hipStream_t)stream, a->images, a->dst, S, k);
  MC_CHECK_LAUNCH("maeclip_image_preprocess_u8");
  return 0;
}

extern "C" int32_t maeclip_image_normalize_u8(const maeclip_image_u8_args* a, void* stream) {
  MC_CHECK_ARG(a && a->src && a->dst, "maeclip_image_normalize_u8: null pointer");
  MC_CHECK_ARG(a->B >= 0 && a->H > 0 && a->W > 0, "maeclip_image_normalize_u8: bad sizes");
  NormConst k;
  MC_CHECK_ARG(mc_norm_const(a->mean, a->std, a->max_pixel, k),
               "maeclip_image_normalize_u8: std and max_pixel must be > 0");
  const int64_t HW = a->H * a->W, npix = a->B * HW;
  if (npix == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = a->W % 4 == 0 && ((uintptr_t)a->src & 3) == 0 && ((uintptr_t)a->dst & 15) == 0;
  if (vec) {
    const int64_t n4 = npix / 4;
    hipLaunchKernelGGL(normalize_u8_x4_kernel, dim3((unsigned)((n4 + NTH - 1) / NTH)), dim3(NTH), 0, s, a->src, a->dst,
                       n4, HW, k);
  } else {
    hipLaunchKernelGGL(normalize_u8_kernel, dim3((unsigned)((npix + NTH - 1) / NTH)), dim3(NTH), 0, s, a->src, a->dst,
                       npix, HW, k);
  }
  MC_CHECK_LAUNCH("maeclip_image_normalize_u8");
  return 0;
}
