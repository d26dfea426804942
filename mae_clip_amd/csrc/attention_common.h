// What the attention files share, stated once (attention.hip: the route, the
// dispatcher, the entry points, the resident forward and the two-phase
// backward; attention_diag.hip: the diagonal backward; attention_rows.hip: the
// fp32 rows kernels; attention_stream.h: the streamed bf16 kernels): the
// constants, the LDS image layout and its fillers, the MFMA fragment helpers,
// the forward's chunk body, the fused fp8-blocks store, the LDS footprints the
// route and the launches both use, the route itself (maeclip::AttnRoute) and
// the declarations of what one file calls in another. Internal: included by
// those files only.
#pragma once
#include "common.h"
#include "../../include/maeclip.h"
#include <type_traits>

constexpr int MAXW = 8;          // max waves per workgroup (sized per launch to the tile count)
constexpr size_t LDS_MAX = 163840;   // 160 KiB of LDS per CU (and per workgroup)
constexpr size_t LDS_FREE = 65536;   // dynamic LDS a launch may ask for without maeclip::allow_lds
// forward waves per SIMD the register allocator must keep: the bf16 HD 32
// body with the MFMA row sum fits 80 VGPRs (6 waves per SIMD, 3 workgroups of
// 7 waves per CU at n = 197); the others are left to the compiler
template <typename T, int HD, bool DROP> constexpr int fwd_wpe() {
  return (sizeof(T) == 2 && HD == 32 && !DROP) ? 6 : 1;
}

// Q / K / V / O / dO are read once per (sample, head): non-temporal loads, so
// they do not evict what the next kernels reuse
#define ANT(p) __builtin_nontemporal_load(p)
#define NW ((int)(blockDim.x >> 6))
#define NTH ((int)blockDim.x)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1.0e30f;
constexpr int SB = 64;   // streamed bf16 kernels: rows per streamed block = rows of a ring slot

#ifdef ATTN_STAMPS
// diagnostic build only: s_memtime per wave of the first 4096 backward
// workgroups at start / prologue done / phase 1 done / phase 2 start / phase 2
// done / exit. The two translation units that stamp (attention.hip,
// attention_diag.hip) define a buffer each; maeclip_debug_attn_stamps merges them.
#define ATTN_STAMPS_BUFFER static __device__ uint64_t g_attn_stamps[4096 * MAXW * 8];
namespace maeclip { int attn_diag_stamps(uint64_t* host, int n); }   // attention_diag.hip
#define ASTAMP(k) do { if (lane == 0 && blockIdx.x < 4096) g_attn_stamps[((int64_t)blockIdx.x * MAXW + wave) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ATTN_STAMPS_BUFFER
#define ASTAMP(k) do {} while (0)
#endif

template <typename T, int HD> struct Img {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr int ROWB = BF ? HD * 2 : HD * 4 + 16;
  __device__ static __forceinline__ int f(int row) { return HD == 64 ? (row & 6) : ((row >> 1) & 2); }
  // byte offset of 16-byte chunk c of a row
  __device__ static __forceinline__ int chunk(int row, int c) {
    return BF ? row * ROWB + ((c ^ f(row)) << 4) : row * ROWB + (c << 4);
  }
  static constexpr int CPR = BF ? HD / 8 : HD / 4;  // 16-B chunks per row
};

// NI head slices of the same token rows (global [n rows, stride ld]) -> NI
// LDS images, zero rows >= n up to npad. Every thread keeps 2*NI 16-B loads in
// flight before it writes LDS (the loop is latency-, not bandwidth-bound).
template <typename T, int HD, int NI>
__device__ __forceinline__ void load_imgs(char* const (&lds)[NI], const T* const (&g)[NI], int64_t ld, int n,
                                          int npad) {
  using I = Img<T, HD>;
  const int total = npad * I::CPR;
  for (int id0 = threadIdx.x; id0 < total; id0 += 2 * NTH) {
    v4u v[2][NI];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int id = id0 + u * NTH;
      const int row = id / I::CPR, c = id % I::CPR;
      const bool ok = id < total && row < n;
#pragma unroll
      for (int i = 0; i < NI; ++i)
        v[u][i] = ok ? ANT((const v4u*)(g[i] + (int64_t)row * ld + c * (16 / sizeof(T)))) : v4u{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int id = id0 + u * NTH;
      const int row = id / I::CPR, c = id % I::CPR;
      if (id < total) {
#pragma unroll
        for (int i = 0; i < NI; ++i) *(v4u*)(lds[i] + I::chunk(row, c)) = v[u][i];
      }
    }
  }
}

// bf16 K / V images by LDS-DMA (buffer_load_dwordx4 ... lds): one
// wave-instruction fills 1 KiB of an image, lane L the 16-B slot L of it, so
// the XOR swizzle goes into the SOURCE address (slot s of row r holds chunk
// s ^ f(r)); rows >= n read as zero through the descriptor's range check (its
// extent ends with row n - 1's slice). No VGPR round trip and no per-chunk
// address VALU beyond one row / chunk split per instruction; the wave waits for
// its own DMA, the caller's barrier for everyone's. Non-temporal (aux bit 1)
// like the register path's loads. (The register path for the bf16 K / V images
// and Q fragments from global per tile were build switches until round 18: the
// DMA and the Q image measured faster where fwd_qimg takes them; removed.)
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __amdgpu_buffer_rsrc_t rsrc_t;
// forward: Q as a third LDS image (bf16 DMA path) only while two workgroups
// per CU still fit with it: with one, the longer prologue has nothing to
// overlap (C1 encoder n = 197 at hd 64: 95.6 -> 116.2 us; C4 decoder n = 577:
// 233 -> 249 us), with two it saves a global round trip per query tile (C2
// decoder 74.2 -> 67.6 us, C4 encoder 49.9 -> 47.3; profiles/r06/attn_fwd_qimg_ab_r6aa.txt)
template <typename T, int HD> __host__ __device__ __forceinline__ bool fwd_qimg(int npad) {
  return std::is_same<T, bf16_t>::value && 2 * (3 * npad * Img<T, HD>::ROWB + npad * 4) <= (int)LDS_MAX;
}

template <int HD, int NI>
__device__ __forceinline__ void dma_imgs(char* const (&dst)[NI], const bf16_t* const (&src)[NI], int64_t ld, int n,
                                         int npad) {
  using I = Img<bf16_t, HD>;
  const int64_t span = ((int64_t)(n - 1) * ld + HD) * 2;
  const int nrec = (int)(span < 0x7fffffff ? span : 0x7fffffff);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = (int)(blockDim.x >> 6);
  const int ninst = npad * I::CPR / 64;   // npad is a multiple of 64
  for (int k = wave; k < ninst; k += nw) {
    const int id = k * 64 + lane;
    const int row = id / I::CPR, sl = id % I::CPR;
    const int voff = row * (int)ld * 2 + ((sl ^ I::f(row)) << 4);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src[i], (short)0, nrec, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(dst[i] + k * 1024), 16, voff, 0, 0, 2);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// dot product of two 16-B chunks in f32
template <typename T> __device__ __forceinline__ float chunk_dot(v4u a, v4u b);
template <> __device__ __forceinline__ float chunk_dot<bf16_t>(v4u a, v4u b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s = fmaf(__uint_as_float(a[j] << 16), __uint_as_float(b[j] << 16), s);
    s = fmaf(__uint_as_float(a[j] & 0xffff0000u), __uint_as_float(b[j] & 0xffff0000u), s);
  }
  return s;
}
template <> __device__ __forceinline__ float chunk_dot<float>(v4u a, v4u b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s = fmaf(__uint_as_float(a[j]), __uint_as_float(b[j]), s);
  return s;
}

// ---- row fragment: 8 consecutive d (d = 32ks + 8g + j) of LDS row r0 + (lane&15)
template <typename T, int HD> struct RowFrag;
template <int HD> struct RowFrag<bf16_t, HD> {
  v8s v;
  __device__ __forceinline__ void lds(const char* img, int r0, int ks, int lane) {
    const int row = r0 + (lane & 15);
    v = *(const v8s*)(img + Img<bf16_t, HD>::chunk(row, 4 * ks + (lane >> 4)));
  }
  __device__ __forceinline__ void glob(const bf16_t* p, int ks, int lane, bool ok) {
    v = ok ? ANT((const v8s*)(p + 32 * ks + 8 * (lane >> 4))) : v8s{0, 0, 0, 0, 0, 0, 0, 0};
  }
};
template <int HD> struct RowFrag<float, HD> {
  float v[8];
  __device__ __forceinline__ void lds(const char* img, int r0, int ks, int lane) {
    const int row = r0 + (lane & 15);
    const int c0 = 8 * ks + 2 * (lane >> 4);
    v4f a = *(const v4f*)(img + Img<float, HD>::chunk(row, c0));
    v4f b = *(const v4f*)(img + Img<float, HD>::chunk(row, c0 + 1));
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
  __device__ __forceinline__ void glob(const float* p, int ks, int lane, bool ok) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ok ? p[32 * ks + 8 * (lane >> 4) + j] : 0.f;
  }
};

// D += X Y over a 32-deep k-step; X, Y row fragments (X rows on lane for A operand).
__device__ __forceinline__ v4f mma32(const RowFrag<bf16_t, 64>& x, const RowFrag<bf16_t, 64>& y, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x.v, y.v, c, 0, 0, 0);
}
__device__ __forceinline__ v4f mma32(const RowFrag<bf16_t, 32>& x, const RowFrag<bf16_t, 32>& y, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x.v, y.v, c, 0, 0, 0);
}
template <int HD>
__device__ __forceinline__ v4f mma32(const RowFrag<float, HD>& x, const RowFrag<float, HD>& y, v4f c) {
#pragma unroll
  for (int s = 0; s < 8; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(x.v[s], y.v[s], c, 0, 0, 0);
  return c;
}

// bf16 transposed fragment: element j <-> row rb + 16*(j>>2) + 4*g + (j&3),
// column c0 + (lane&15): the A operand "X^T" of a product that sums over rows.
template <int HD>
__device__ __forceinline__ v8s tr_frag(const char* img, int rb, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int unit = (c0 >> 2) + p;  // 8-byte unit within the row
  v8s r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = rb + 16 * h + 4 * g + q;
    const char* a = img + Img<bf16_t, HD>::chunk(row, unit >> 1) + ((unit & 1) << 3);
    v4s t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, a));
#pragma unroll
    for (int e = 0; e < 4; ++e) r[4 * h + e] = t[e];
  }
  return r;
}
__device__ __forceinline__ v8s pack_p(const v4f& a, const v4f& b) {
  // four v_cvt_pk_bf16_f32 (RNE), one per pair
  const v4u u = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
  return __builtin_bit_cast(v8s, u);
}

// D[c][col] += sum over 32 rows (rb..rb+31) of X[row][c] * P[row][col], where
// P is held as two accumulator tiles (rows rb+4g+i and rb+16+4g+i on lane col).
template <typename T, int HD>
__device__ __forceinline__ v4f mma_rowsum(const char* img, int rb, int c0, const v4f& p0, const v4f& p1,
                                          v4f acc, int lane) {
  if constexpr (std::is_same<T, bf16_t>::value) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(img, rb, c0, lane), pack_p(p0, p1), acc, 0, 0, 0);
  } else {
    const int g = lane >> 4, col = c0 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x0 = *(const float*)(img + (rb + 4 * g + i) * Img<float, HD>::ROWB + col * 4);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, p0[i], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x1 = *(const float*)(img + (rb + 16 + 4 * g + i) * Img<float, HD>::ROWB + col * 4);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, p1[i], acc, 0, 0, 0);
    }
    return acc;
  }
}

__device__ __forceinline__ bool dropout_keep(uint64_t seed, uint64_t bh, int q, int k, uint32_t thr) {
  return mc_hash4(seed, bh, (uint64_t)q, (uint64_t)k) >= thr;
}

// ============================================================== forward
// max over the four 16-lane rows (the lanes l, l^16, l^32, l^48 of a query):
// two permlane swaps (VALU) instead of two ds_bpermute round trips
// (a plain v_max_f32 in inline asm, which skips fmaxf's canonicalising of each
// permlane result, pinned the schedule: C4 decoder fwd 255 -> 280 us; removed)
__device__ __forceinline__ float max4rows(float x) {
  const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float sum4rows(float x) {
  const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = __uint_as_float(p[0]) + __uint_as_float(p[1]);
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

struct FwdDrop {
  uint64_t seed, bh;
  uint32_t thr;
  float scale;
};

// One 64-key chunk of a 16-query tile with its shape fixed at compile time, so
// the body is straight-line code the scheduler can interleave (the runtime
// per-32-key / mask / dropout branches of a generic body split it into ~30
// basic blocks with an MFMA or a few VALU ops each). NT: 16-key S tiles that
// hold real keys (4 for a whole chunk; the tail chunk of n = 197, keys
// 192..196, runs one tile instead of two -- its PV product takes a zero
// second half); MASKED: add the key bias (padding keys, DistilBERT's key mask)
// -- the scale c > 0 then rides in the bias fma, otherwise in the exponent's
// fma and the running max is taken on the raw scores.
// bf16 without dropout: the row sum of P comes out of the MFMA as a
// 17th..32nd "V column" of ones (lsum accumulator `ol`, every element the
// lane's query's sum of the bf16 P the PV product uses) instead of 16 VALU
// adds per chunk -- the kernel is VALU-bound at HD 32, the MFMA pipe is not;
// lsum is then the exact weight sum of O = sum P V (both over bf16(P)).
// With dropout the normalisation needs the sum BEFORE the mask: VALU adds.
// (A lazy rescale -- moving the running max only when a wave-uniform ballot
// saw a chunk max 8 log2 units above it -- measured slower: the branch splits
// the chunk body. The exponent arguments of a value pair in one v_pk_fma_f32
// measured neutral to -3 %, decoder 75 -> 77-80 us. Both removed.)
template <typename T, int HD, int NT, bool MASKED, bool DROP>
__device__ __forceinline__ void fwd_chunk(const char* Kimg, const char* Vimg, const float* kmask, int kc,
                                          const RowFrag<T, HD> (&qf)[HD / 32], float c, float& m, float& lsum,
                                          v4f (&o)[HD / 16], v4f& ol, int lane, const FwdDrop& dr, int q) {
  constexpr bool BF = std::is_same<T, bf16_t>::value;
  constexpr bool MSUM = BF && !DROP;
  constexpr int NP = (NT + 1) / 2;   // 32-key halves of the PV product
  const int g = lane >> 4;
  v4f s[2 * NP];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    s[t] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
      RowFrag<T, HD> kf;
      kf.lds(Kimg, kc + 16 * t, ks, lane);
      s[t] = mma32(kf, qf[ks], s[t]);
    }
  }
  float mloc = NEG_BIG;
  if (MASKED) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const v4f km = *(const v4f*)(kmask + kc + 16 * t + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[t][i] = fmaf(s[t][i], c, km[i]);
        mloc = fmaxf(mloc, s[t][i]);
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) mloc = fmaxf(mloc, s[t][i]);
    mloc *= c;
  }
  mloc = max4rows(mloc);
  const float mnew = fmaxf(m, mloc);
  const float lsc = __builtin_amdgcn_exp2f(m - mnew);
  if (MSUM) ol[0] *= lsc;   // only element 0 is read back
#pragma unroll
  for (int dt = 0; dt < HD / 16; ++dt) o[dt] *= lsc;
  m = mnew;
  const float cc = MASKED ? 1.f : c, nm = -m;
  float lp = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float p = __builtin_amdgcn_exp2f(fmaf(s[t][i], cc, nm));
      if (!MSUM) lp += p;
      s[t][i] = p;
    }
  }
  if (NT & 1) s[NT] = v4f{0.f, 0.f, 0.f, 0.f};
  if (!MSUM) lsum = fmaf(lsum, lsc, lp);
  if (DROP) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kc + 16 * t + 4 * g + i;
        s[t][i] = dropout_keep(dr.seed, dr.bh, q, key, dr.thr) ? s[t][i] * dr.scale : 0.f;
      }
  }
#pragma unroll
  for (int s2 = 0; s2 < NP; ++s2) {
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt)
      o[dt] = mma_rowsum<T, HD>(Vimg, kc + 32 * s2, 16 * dt, s[2 * s2], s[2 * s2 + 1], o[dt], lane);
    if constexpr (MSUM) {
      const v8s ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};   // bf16 1.0
      ol = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pack_p(s[2 * s2], s[2 * s2 + 1]), ol, 0, 0, 0);
    }
  }
}

// fp8-blocks copy (maeclip_attn_args q8) of the HD columns [col0, col0 + HD)
// of output row `row` this lane's 16-row tile stores: lane (row, g = lane / 16)
// holds v[dt] = columns 16 dt + 4 g .. +3 as stored in bf16, so the 32-column
// block j is dt = 2j, 2j + 1 of the four lanes l % 16 + 16 g: its amax is two
// permlane swaps (every lane of the wave takes part; `ok` gates the stores).
template <int HD>
__device__ __forceinline__ void q8_store(const maeclip_attn_args& a, int64_t row, bool ok, int col0, int rowlen,
                                         const v4f (&v)[HD / 16], int lane) {
  const int g = lane >> 4;
  const bool e5 = a.q8_fmt == MAECLIP_FP8_E5M2;
#pragma unroll
  for (int j = 0; j < HD / 32; ++j) {
    float x[8], am = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[i] = bf2f(f2bf(v[2 * j][i]));
      x[4 + i] = bf2f(f2bf(v[2 * j + 1][i]));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(x[i]));
    auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(am), __float_as_uint(am), false, false);
    am = fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
    p = __builtin_amdgcn_permlane32_swap(__float_as_uint(am), __float_as_uint(am), false, false);
    am = fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
    const unsigned ex = mc_e8m0(am, e5);
    const float inv = mc_e8m0_inv(ex);
    if (ok) {
      uint8_t* q = (uint8_t*)a.q8 + row * a.ldq8 + col0 + 32 * j + 4 * g;
      unsigned w0, w1;
      if (e5) {
        w0 = mc_cvt4_fp8<true>(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv);
        w1 = mc_cvt4_fp8<true>(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv);
      } else {
        w0 = mc_cvt4_fp8<false>(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv);
        w1 = mc_cvt4_fp8<false>(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv);
      }
      *(unsigned*)q = w0;
      *(unsigned*)(q + 16) = w1;
      if (g == 0) a.q8_scale[mc_fp8b_off(row, (col0 >> 5) + j, rowlen >> 7)] = (uint8_t)ex;
    }
  }
}

// ------------------------------------------------------- LDS footprints
template <int HD> size_t bwd_diag_lds(int n) {
  const int npad = (n + 31) & ~31, nw = npad / 32;
  return (size_t)2 * npad * Img<bf16_t, HD>::ROWB + (size_t)2 * npad * 4 + (size_t)npad * 4 * HD +
         (size_t)nw * 2048 + (size_t)8 * nw * HD * 4 + (size_t)nw * 4;
}

template <typename T, int HD> size_t fwd_lds(int n) {
  const int npad = (n + 63) & ~63;
  const int nimg = fwd_qimg<T, HD>(npad) ? 3 : 2;   // K, V (+ Q; the 16-wave launches ignore the third)
  return (size_t)nimg * npad * Img<T, HD>::ROWB + (size_t)npad * 4;
}
template <typename T, int HD> size_t bwd_lds(int n, int nw, bool two = false, bool masked = false) {
  const int npad = (n + 31) & ~31;
  const int nimg = (std::is_same<T, bf16_t>::value && !two) ? 4 : 2;
  return (size_t)nimg * npad * Img<T, HD>::ROWB + (size_t)(masked ? 3 : 2) * npad * 4 + (size_t)nw * 3 * HD * 4;
}

// largest n the resident bf16 kernels hold (fwd_lds / the two-image bwd_lds <= 160 KiB)
template <int HD> constexpr int resident_max_n(bool bwd) { return HD == 64 ? 576 : bwd ? 1152 : 1216; }

// ----------------------------------------------------------------- the route
namespace maeclip {
// the kernel an attention call runs on (the value maeclip_attn_impl returns)
enum class AttnPath : int32_t {
  REJECTED = -1,
  FWD = 0,         // resident forward (attn_fwd_kernel, up to 8 waves)
  FWD16 = 1,       // resident forward, up to 16 waves
  BWD_FOUR = 2,    // two-phase backward, four LDS images (fp32: the same instantiation, which holds two)
  BWD_TWO = 3,     // two-phase backward, two LDS images
  BWD_TWO3 = 4,    // two images at the 3-workgroups-per-CU register budget (head_dim 32)
  BWD_MASKED = 5,  // two-phase backward with key_mask and / or dropout
  BWD_DIAG = 6,    // one-pass diagonal backward (attention_diag.hip)
  BWD_16 = 7,      // two images, up to 16 waves
  ROWS = 8,        // fp32 rows kernels (attention_rows.hip)
  STREAM = 9,      // streamed bf16 kernels (attention_stream.hip)
  BWD_OCC = 10,    // BWD_FOUR, BWD_TWO or BWD_TWO3, whichever keeps most workgroups per CU: the one
                   // choice that asks the device, settled at the launch (bwd_two in attention.hip)
};
// Everything a launch needs, decided from the arguments and the options alone.
struct AttnRoute {
  AttnPath path;
  bool bwd;        // the backward (ROWS and STREAM serve both directions)
  int nw;         // waves per workgroup (ROWS: one, 64 threads)
  size_t lds;      // dynamic LDS bytes (ROWS: none; STREAM: per kernel, attention_stream.hip)
  bool qimg;       // forward: Q is a third LDS image
  bool q8_fused;   // the kernel writes the fp8-blocks copy itself (else: the standalone pass)
  char err[320];   // REJECTED: the message
};
// after the entry points' argument checks; no HIP call
AttnRoute attn_route(const maeclip_attn_args& a, bool bwd);                            // attention.hip
int attn_diag(const maeclip_attn_args& a, const AttnRoute& r, hipStream_t s);         // attention_diag.hip
int attn_rows(const maeclip_attn_args& a, const AttnRoute& r, hipStream_t s);         // attention_rows.hip
int attn_stream(const maeclip_attn_args& a, const AttnRoute& r, hipStream_t s);       // attention_stream.hip
}  // namespace maeclip

// one workgroup per (sample, head) of 64 r.nw threads: the LDS allowance above
// 64 KiB, the launch and its check
template <typename K>
int attn_launch(K kern, const char* what, const maeclip_attn_args& a, const maeclip::AttnRoute& r, hipStream_t s) {
  if (r.lds > LDS_FREE) maeclip::allow_lds((const void*)kern, (int)r.lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.B * a.H)), dim3(64 * r.nw), r.lds, s, a);
  MC_CHECK_LAUNCH(what);
  return 0;
}
