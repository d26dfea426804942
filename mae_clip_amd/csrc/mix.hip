// Mixup / CutMix on the device (include/maeclip.h "Mixup / CutMix"): timm's
// Mixup (correct_lam, partner = x.flip(0)) as three entry points, so that a
// fine-tuning step replayed as one HIP graph mixes anew on every replay:
//   maeclip_mix_params   the draw, one record per sample, keyed by the device
//                        step (and its host twin: one __host__ __device__ function)
//   maeclip_mix_images   the pixels, uint8 HWC or fp32 CHW, out of place
//   maeclip_mix_targets  the class-probability targets for maeclip_xent_fwd
// None of them allocates, synchronises, reads on the host or uses atomics.
//
// The pixel kernel is HBM-bound (2 reads + 1 write per element at most). A
// workgroup covers NTH * U consecutive 16-byte pieces of ONE sample (its
// record is uniform over the workgroup); thread t takes pieces t, t + NTH, ...,
// so consecutive lanes go to consecutive addresses. Where 16-byte accesses are
// not possible (extent or alignment) a piece is one element: the same code
// per element, so the same bits.
#include "common.h"
#include "../../include/maeclip.h"

#include <math.h>

namespace {
constexpr int NTH = 256;
constexpr int U = 4;              // pieces per thread (pixel kernel)
constexpr int MIX_TRIES = 16;     // Marsaglia-Tsang attempts per gamma variate

enum : uint64_t { F_MIX = 16, F_SWITCH = 17, F_N1 = 18, F_N2 = 19, F_ACC = 20, F_BOOST = 21, F_CY = 22, F_CX = 23 };

__host__ __device__ inline int mix_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The draw of one key; the order of operations is the one written out at
// maeclip_mix_params in maeclip.h, and tests/mix_ref.py follows it line by
// line. Host and device evaluate this one function (no contraction into fma
// on either).
struct MixDraw {
  uint64_t sseed, key;
  __host__ __device__ inline double u(uint64_t k, uint64_t f) const {
    return (double)(mc_hash4(sseed, key, k, f) >> 8) * (1.0 / 16777216.0);
  }
  __host__ __device__ inline double uo(uint64_t k, uint64_t f) const {
    return (double)((mc_hash4(sseed, key, k, f) >> 8) + 1u) * (1.0 / 16777216.0);
  }
  __host__ __device__ inline double gamma(double a, int g) const {
#pragma clang fp contract(off)
    const double a1 = a < 1.0 ? a + 1.0 : a;
    const double d = a1 - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    double G = d;                                   // all MIX_TRIES attempts rejected (p < 1.5e-21): v = 1
    for (int t = 0; t < MIX_TRIES; ++t) {
      const uint64_t k = (uint64_t)(MIX_TRIES * g + t);
      const double x = sqrt(-2.0 * log(uo(k, F_N1))) * cos(6.283185307179586 * u(k, F_N2));
      const double t1 = 1.0 + c * x;
      if (t1 <= 0.0) continue;
      const double v = (t1 * t1) * t1;
      const double rhs = (((0.5 * x) * x + d) - d * v) + d * log(v);
      if (log(uo(k, F_ACC)) < rhs) {
        G = d * v;
        break;
      }
    }
    if (a < 1.0) G = G * exp(log(uo((uint64_t)(MIX_TRIES * g), F_BOOST)) / a);
    return G;
  }
};

__host__ __device__ inline void mc_mix_draw(uint64_t step_seed, uint64_t key, int H, int W, double mixup_alpha,
                                            double cutmix_alpha, double prob, double switch_prob, int partner,
                                            maeclip_mix_record* out) {
#pragma clang fp contract(off)
  const MixDraw r = {step_seed, key};
  maeclip_mix_record rec = {MAECLIP_MIX_NONE, partner, 0, 0, 0, 0, 1.f, 1.f};
  bool cutmix = false;
  double alpha = 0.0;
  if (r.u(0, F_MIX) < prob) {
    if (mixup_alpha > 0.0 && cutmix_alpha > 0.0) {
      cutmix = r.u(0, F_SWITCH) < switch_prob;
      alpha = cutmix ? cutmix_alpha : mixup_alpha;
    } else if (mixup_alpha > 0.0) {
      alpha = mixup_alpha;
    } else if (cutmix_alpha > 0.0) {
      cutmix = true;
      alpha = cutmix_alpha;
    }
  }
  if (alpha > 0.0) {
    double lam;
    if (alpha == 1.0) {
      lam = r.u(0, F_N1);
    } else {
      const double X = r.gamma(alpha, 0), Y = r.gamma(alpha, 1);
      lam = X / (X + Y);
    }
    if (!cutmix) {
      rec.kind = MAECLIP_MIX_MIXUP;
      rec.lam_pixel = rec.lam_target = (float)lam;
    } else {
      const double rt = sqrt(1.0 - lam);
      const int ch = (int)((double)H * rt), cw = (int)((double)W * rt);
      const int cy = (int)floor(r.u(0, F_CY) * (double)H), cx = (int)floor(r.u(0, F_CX) * (double)W);
      rec.kind = MAECLIP_MIX_CUTMIX;
      rec.y0 = mix_clampi(cy - ch / 2, 0, H);
      rec.y1 = mix_clampi(cy + ch / 2, 0, H);
      rec.x0 = mix_clampi(cx - cw / 2, 0, W);
      rec.x1 = mix_clampi(cx + cw / 2, 0, W);
      const double area = (double)((int64_t)(rec.x1 - rec.x0) * (int64_t)(rec.y1 - rec.y0));
      rec.lam_target = (float)(1.0 - area / ((double)H * (double)W));
    }
  }
  *out = rec;
}

// sample b of a draw (step_ptr and params readable from the caller's side)
__host__ __device__ inline void mix_params_sample(const maeclip_mix_params_args& a, int b) {
  const uint64_t key = a.mode == MAECLIP_MIX_BATCH ? (uint64_t)MAECLIP_MIX_BATCH_KEY : a.sample_offset + (uint64_t)b;
  mc_mix_draw(mc_step_seed(a.seed, a.step_ptr), key, a.H, a.W, (double)a.mixup_alpha, (double)a.cutmix_alpha,
              (double)a.prob, (double)a.switch_prob, a.B - 1 - b, a.params + b);
}
__global__ void __launch_bounds__(NTH) mix_params_kernel(const maeclip_mix_params_args a) {
  const int b = blockIdx.x * NTH + threadIdx.x;
  if (b < a.B) mix_params_sample(a, b);
}

// ------------------------------------------------------------------ pixels
// (x, y) of element g of a sample, stepped one element at a time.
// uint8 [S][S][3]: pixel g / 3; fp32 [3][S][S]: g % (S S) within its plane.
template <typename T> struct Pos;
template <> struct Pos<uint8_t> {
  int x, y, c, S;
  __device__ __forceinline__ Pos(unsigned g, int S_) : S(S_) {
    const unsigned pix = g / 3u;
    c = (int)(g - pix * 3u);
    y = (int)(pix / (unsigned)S);
    x = (int)(pix - (unsigned)y * (unsigned)S);
  }
  __device__ __forceinline__ void next() {
    if (++c == 3) {
      c = 0;
      if (++x == S) {
        x = 0;
        ++y;
      }
    }
  }
};
template <> struct Pos<float> {
  int x, y, S;
  __device__ __forceinline__ Pos(unsigned g, int S_) : S(S_) {
    const unsigned plane = (unsigned)S * (unsigned)S;
    const unsigned r = g % plane;
    y = (int)(r / (unsigned)S);
    x = (int)(r - (unsigned)y * (unsigned)S);
  }
  __device__ __forceinline__ void next() {
    if (++x == S) {
      x = 0;
      if (++y == S) y = 0;
    }
  }
};

// fl(fl(lam a) + fl(oml p)): three roundings (HIP's __fmul_rn / __fadd_rn are plain
// operators that the compiler may fuse; the pragma is what keeps them apart)
__device__ __forceinline__ float mix_val(float a, float p, float lam, float oml) {
#pragma clang fp contract(off)
  const float la = lam * a;
  const float op = oml * p;
  return la + op;
}
__device__ __forceinline__ uint8_t mix_one(uint8_t a, uint8_t p, float lam, float oml) {
  const float v = rintf(mix_val((float)a, (float)p, lam, oml));
  return (uint8_t)fminf(fmaxf(v, 0.f), 255.f);      // fmaxf(NaN, 0) = 0
}
__device__ __forceinline__ float mix_one(float a, float p, float lam, float oml) { return mix_val(a, p, lam, oml); }

// a piece of N elements of T: 16 bytes (N = 16 / sizeof(T)) or one element
// (kept as four dwords, elements taken out by constant shifts: registers, no scratch)
template <typename T, int N> struct Piece {
  v4u w = {0u, 0u, 0u, 0u};
  __device__ __forceinline__ void load(const T* p) { w = *(const v4u*)p; }
  __device__ __forceinline__ void store(T* p) const { *(v4u*)p = w; }
  __device__ __forceinline__ T get(int i) const {
    if constexpr (sizeof(T) == 4) {
      return __uint_as_float(w[i]);
    } else {
      return (T)(w[i >> 2] >> ((i & 3) * 8));
    }
  }
  // into a piece that starts as zeros
  __device__ __forceinline__ void set(int i, T x) {
    if constexpr (sizeof(T) == 4) {
      w[i] = __float_as_uint(x);
    } else {
      w[i >> 2] |= (unsigned)x << ((i & 3) * 8);
    }
  }
};
template <typename T> struct Piece<T, 1> {
  T v = 0;
  __device__ __forceinline__ void load(const T* p) { v = *p; }
  __device__ __forceinline__ void store(T* p) const { *p = v; }
  __device__ __forceinline__ T get(int) const { return v; }
  __device__ __forceinline__ void set(int, T x) { v = x; }
};

struct MixK {
  const void* src;
  void* dst;
  const maeclip_mix_record* params;
  int B, S;
  unsigned E;        // elements per sample
  unsigned nblk;     // workgroups per sample
};

template <typename T, int N>
__global__ void __launch_bounds__(NTH) mix_images_kernel(const MixK k) {
  const unsigned b = blockIdx.x / k.nblk, blk = blockIdx.x - b * k.nblk;
  const maeclip_mix_record rec = k.params[b];
  const int S = k.S;
  const int kind = rec.kind;
  const int pb = mix_clampi(rec.partner, 0, k.B - 1);
  const T* sa = (const T*)k.src + (int64_t)b * k.E;
  const T* sp = (const T*)k.src + (int64_t)pb * k.E;
  T* d = (T*)k.dst + (int64_t)b * k.E;
  const int x0 = mix_clampi(rec.x0, 0, S), x1 = mix_clampi(rec.x1, 0, S);
  const int y0 = mix_clampi(rec.y0, 0, S), y1 = mix_clampi(rec.y1, 0, S);
  const float lam = rec.lam_pixel, oml = __fsub_rn(1.f, lam);
  const unsigned npiece = k.E / N;                    // N divides E (host)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned q = (blk * U + u) * NTH + threadIdx.x;
    if (q >= npiece) continue;
    const unsigned g = q * N;
    Piece<T, N> a, p, o;
    if (kind == MAECLIP_MIX_MIXUP) {
      a.load(sa + g);
      p.load(sp + g);
#pragma unroll
      for (int i = 0; i < N; ++i) o.set(i, mix_one(a.get(i), p.get(i), lam, oml));
    } else if (kind == MAECLIP_MIX_CUTMIX) {
      unsigned in = 0;                                // bit i: element i lies in the box
      Pos<T> pos(g, S);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        in |= (pos.x >= x0 && pos.x < x1 && pos.y >= y0 && pos.y < y1 ? 1u : 0u) << i;
        pos.next();
      }
      constexpr unsigned ALL = (1u << N) - 1u;
      if (in != ALL) a.load(sa + g);
      if (in != 0) p.load(sp + g);
#pragma unroll
      for (int i = 0; i < N; ++i) o.set(i, (in >> i) & 1u ? p.get(i) : a.get(i));
    } else {
      o.load(sa + g);
    }
    o.store(d + g);
  }
}

template <typename T, int N>
void launch_mix_images(const MixK& k, hipStream_t s) {
  hipLaunchKernelGGL((mix_images_kernel<T, N>), dim3(k.nblk * (unsigned)k.B), dim3(NTH), 0, s, k);
}

// ----------------------------------------------------------------- targets
struct TgtK {
  const void* labels;
  int lab64;
  const maeclip_mix_record* params;
  float* t;
  int64_t ld;
  int B;
  int64_t C;
  unsigned nblk;     // workgroups per row
};
__device__ __forceinline__ int64_t tgt_label(const TgtK& k, int i) {
  return k.lab64 ? ((const int64_t*)k.labels)[i] : (int64_t)((const int32_t*)k.labels)[i];
}
// thread: 4 consecutive columns of one row
template <bool VEC>
__global__ void __launch_bounds__(NTH) mix_targets_kernel(const TgtK k) {
  const unsigned b = blockIdx.x / k.nblk, blk = blockIdx.x - b * k.nblk;
  const int64_t col = ((int64_t)blk * NTH + threadIdx.x) * 4;
  if (col >= k.ld) return;
  const maeclip_mix_record rec = k.params[b];
  const int pb = mix_clampi(rec.partner, 0, k.B - 1);
  const int64_t ya = tgt_label(k, (int)b), yp = tgt_label(k, pb);
  const float lam = rec.lam_target, oml = __fsub_rn(1.f, lam);
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t j = col + r;
    float t = 0.f;
    if (j < k.C) {
      if (j == ya && j == yp) {
        t = 1.f;
      } else if (j == ya) {
        t = lam;
      } else if (j == yp) {
        t = oml;
      }
    }
    v[r] = t;
  }
  float* row = k.t + (int64_t)b * k.ld;
  if (VEC) {                                          // ld % 4 == 0: the four columns exist
    *(v4f*)(row + col) = (v4f){v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (col + r < k.ld) row[col + r] = v[r];
  }
}
}  // namespace

static int32_t mix_params_check(const maeclip_mix_params_args* a, const char* who) {
  MC_CHECK_ARG(a && a->params, "%s: null pointer", who);
  MC_CHECK_ARG(((uintptr_t)a->params & 3) == 0 && ((uintptr_t)a->step_ptr & 7) == 0,
               "%s: params must be 4-byte aligned, step_ptr 8-byte aligned", who);
  MC_CHECK_ARG(a->B >= 0, "%s: B must be >= 0", who);
  MC_CHECK_ARG(a->H >= 1 && a->H <= 32768 && a->W >= 1 && a->W <= 32768, "%s: H and W must be in [1, 32768]", who);
  MC_CHECK_ARG(a->mixup_alpha >= 0.f && a->mixup_alpha < INFINITY && a->cutmix_alpha >= 0.f && a->cutmix_alpha < INFINITY,
               "%s: alphas must be finite and >= 0", who);
  MC_CHECK_ARG(a->prob >= 0.f && a->prob <= 1.f, "%s: prob must be in [0, 1]", who);
  MC_CHECK_ARG(a->switch_prob >= 0.f && a->switch_prob <= 1.f, "%s: switch_prob must be in [0, 1]", who);
  MC_CHECK_ARG(a->mode == MAECLIP_MIX_BATCH || a->mode == MAECLIP_MIX_ELEM, "%s: mode must be 0 (batch) or 1 (elem)", who);
  return 0;
}

extern "C" int32_t maeclip_mix_params(const maeclip_mix_params_args* a, void* stream) {
  if (int32_t rc = mix_params_check(a, "maeclip_mix_params")) return rc;
  if (a->B == 0) return 0;
  hipLaunchKernelGGL(mix_params_kernel, dim3((unsigned)((a->B + NTH - 1) / NTH)), dim3(NTH), 0, (hipStream_t)stream, *a);
  MC_CHECK_LAUNCH("maeclip_mix_params");
  return 0;
}

extern "C" int32_t maeclip_mix_params_host(const maeclip_mix_params_args* a) {
  if (int32_t rc = mix_params_check(a, "maeclip_mix_params_host")) return rc;
  for (int b = 0; b < a->B; ++b) mix_params_sample(*a, b);
  return 0;
}

extern "C" int32_t maeclip_mix_images(const maeclip_mix_images_args* a, void* stream) {
  MC_CHECK_ARG(a && a->src && a->dst && a->params, "maeclip_mix_images: null pointer");
  MC_CHECK_ARG(a->dtype == MAECLIP_MIX_U8 || a->dtype == MAECLIP_MIX_F32,
               "maeclip_mix_images: dtype must be 0 (uint8 HWC) or 1 (fp32 CHW) (got %d)", a->dtype);
  MC_CHECK_ARG(a->B >= 0 && a->B <= 0x7fffffffLL && a->S >= 1 && a->S <= 8192, "maeclip_mix_images: bad sizes");
  const bool f32 = a->dtype == MAECLIP_MIX_F32;
  const size_t esz = f32 ? 4 : 1;
  MC_CHECK_ARG(((uintptr_t)a->params & 3) == 0 && ((uintptr_t)a->src & (esz - 1)) == 0 && ((uintptr_t)a->dst & (esz - 1)) == 0,
               "maeclip_mix_images: params and fp32 images must be 4-byte aligned");
  const int64_t E = a->S * a->S * 3;                      // elements per sample, <= 2^27.6
  const uintptr_t s0 = (uintptr_t)a->src, d0 = (uintptr_t)a->dst, bytes = (uintptr_t)(a->B * E) * esz;
  MC_CHECK_ARG(bytes == 0 || s0 + bytes <= d0 || d0 + bytes <= s0,
               "maeclip_mix_images: dst overlaps src (the kernel is out of place)");
  if (a->B == 0) return 0;
  const bool vec = ((s0 | d0) & 15) == 0 && (E * (int64_t)esz) % 16 == 0;
  const int64_t n = vec ? 16 / (int64_t)esz : 1;
  const int64_t npiece = E / n;
  const int64_t nblk = (npiece + NTH * U - 1) / (NTH * U);
  MC_CHECK_ARG(nblk * a->B <= 0x7fffffffLL, "maeclip_mix_images: B x S x S too large for one launch");
  MixK k = {a->src, a->dst, a->params, (int)a->B, (int)a->S, (unsigned)E, (unsigned)nblk};
  hipStream_t s = (hipStream_t)stream;
  if (f32) {
    if (vec) {
      launch_mix_images<float, 4>(k, s);
    } else {
      launch_mix_images<float, 1>(k, s);
    }
  } else if (vec) {
    launch_mix_images<uint8_t, 16>(k, s);
  } else {
    launch_mix_images<uint8_t, 1>(k, s);
  }
  MC_CHECK_LAUNCH("maeclip_mix_images");
  return 0;
}

extern "C" int32_t maeclip_mix_targets(const maeclip_mix_targets_args* a, void* stream) {
  MC_CHECK_ARG(a && a->labels && a->params && a->targets, "maeclip_mix_targets: null pointer");
  MC_CHECK_ARG(a->label_dtype == 0 || a->label_dtype == 1, "maeclip_mix_targets: label_dtype must be 0 (int32) or 1 (int64)");
  MC_CHECK_ARG(a->B >= 0 && a->B <= 0x7fffffffLL, "maeclip_mix_targets: B must be in [0, 2^31) (got %lld)", (long long)a->B);
  MC_CHECK_ARG(a->C >= 1 && a->C <= 0x7fffffffLL, "maeclip_mix_targets: C must be in [1, 2^31) (got %lld)", (long long)a->C);
  MC_CHECK_ARG(a->ld_t >= a->C && a->ld_t <= 0x7fffffffLL, "maeclip_mix_targets: ld_t must be >= C (got %lld < %lld)",
               (long long)a->ld_t, (long long)a->C);
  MC_CHECK_ARG(((uintptr_t)a->params & 3) == 0 && ((uintptr_t)a->targets & 3) == 0 &&
                   ((uintptr_t)a->labels & (a->label_dtype ? 7 : 3)) == 0,
               "maeclip_mix_targets: float / int32 pointers must be 4-byte aligned, int64 labels 8-byte aligned");
  if (a->B == 0) return 0;
  const int64_t nblk = ((a->ld_t + 3) / 4 + NTH - 1) / NTH;
  MC_CHECK_ARG(nblk * a->B <= 0x7fffffffLL, "maeclip_mix_targets: B x ld_t too large for one launch");
  TgtK k = {a->labels, a->label_dtype, a->params, a->targets, a->ld_t, (int)a->B, a->C, (unsigned)nblk};
  const bool vec = ((uintptr_t)a->targets & 15) == 0 && a->ld_t % 4 == 0;
  const dim3 grid((unsigned)(nblk * a->B));
  if (vec) {
    hipLaunchKernelGGL(mix_targets_kernel<true>, grid, dim3(NTH), 0, (hipStream_t)stream, k);
  } else {
    hipLaunchKernelGGL(mix_targets_kernel<false>, grid, dim3(NTH), 0, (hipStream_t)stream, k);
  }
  MC_CHECK_LAUNCH("maeclip_mix_targets");
  return 0;
}
