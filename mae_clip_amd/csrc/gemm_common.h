// What the GEMM files (gemm.hip v1, gemm2.hip v2, gemm4*.hip v4 / fp8 / grouped
// weight gradients, gemm_small.hip) share, stated once: the layout and epilogue values of
// maeclip_gemm_args, the host dispatch from those runtime values to template
// arguments, the declarations of what one file calls in another, and the
// fragment reader and fragment epilogue of the two 16x16-fragment kernels that
// keep one output row x 4 columns per lane (v1 and v2). Internal: included by
// those files only.
#pragma once
#include "common.h"
#include "../../include/maeclip.h"
#include <type_traits>

enum { LAY_KC = 0, LAY_RC = 1 };
enum { EPI_NONE = 0, EPI_GELU = 1, EPI_RESID = 2, EPI_DGELU = 3, EPI_GELU_D = 4, EPI_MUL_AUX = 5 };
// the numbers maeclip.h documents for maeclip_gemm_args.a_layout / b_layout / epilogue
static_assert(LAY_KC == 0 && LAY_RC == 1, "maeclip.h: layouts 0 = K-contiguous, 1 = row-contiguous");
static_assert(EPI_NONE == 0 && EPI_GELU == 1 && EPI_RESID == 2 && EPI_DGELU == 3 && EPI_GELU_D == 4 && EPI_MUL_AUX == 5,
              "maeclip.h: epilogues 0 none, 1 GELU, 2 residual, 3 dGELU, 4 GELU', 5 mul-aux");

typedef __attribute__((address_space(3))) void lds_void;

// XOR swizzle (in 8-B units) of k-row k of a bf16 RC tile
__device__ __forceinline__ int swz_rc(int k) { return ((k & 3) | (((k >> 3) & 1) << 2)) << 2; }

namespace maeclip {
// the kernel family maeclip_gemm runs a call on (the value maeclip_gemm_impl returns)
enum class GemmRoute : int32_t { V1 = 0, SMALL = 1, V2 = 2, V4 = 4 };
GemmRoute gemm_route(const maeclip_gemm_args& a);                    // gemm.hip
int gemm_v2(const maeclip_gemm_args& a, hipStream_t s, int variant);  // gemm2.hip
int gemm_v4(const maeclip_gemm_args& a, hipStream_t s);               // gemm4.hip
bool gemm_v4_ok(const maeclip_gemm_args& a);
int64_t gemm_v4_workspace(const maeclip_gemm_args& a);
int check_q8(const maeclip_gemm_args& a, const char* who);        // gemm4_fp8.hip
int gemm_small(const maeclip_gemm_args& a, hipStream_t s);            // gemm_small.hip
bool gemm_small_ok(const maeclip_gemm_args& a);
int64_t gemm_small_workspace(const maeclip_gemm_args& a);
}  // namespace maeclip

// ------------------------------------------------------------ host dispatch
// f(la, lb) with the two operand layouts as std::integral_constant values
// (la.value / decltype(la)::value is a template argument inside a generic lambda)
template <typename F>
int dispatch_layouts(const maeclip_gemm_args& a, F&& f) {
  using KC = std::integral_constant<int, LAY_KC>;
  using RC = std::integral_constant<int, LAY_RC>;
  if (a.a_layout == LAY_KC && a.b_layout == LAY_KC) return f(KC{}, KC{});
  if (a.a_layout == LAY_KC && a.b_layout == LAY_RC) return f(KC{}, RC{});
  if (a.a_layout == LAY_RC && a.b_layout == LAY_KC) return f(RC{}, KC{});
  return f(RC{}, RC{});
}

// f(epi) with the epilogue as a std::integral_constant value. The public entry
// points reject an unknown value before they get here; no path runs another
// epilogue's kernel for one. (The cases stand in the order in which v2 and v4
// have always instantiated their kernels, which is the order of the kernels
// in the code object: it keeps v4's object as it was.)
template <typename F>
int dispatch_epilogue(const maeclip_gemm_args& a, const char* who, F&& f) {
  switch (a.epilogue) {
    case EPI_NONE: return f(std::integral_constant<int, EPI_NONE>{});
    case EPI_GELU: return f(std::integral_constant<int, EPI_GELU>{});
    case EPI_RESID: return f(std::integral_constant<int, EPI_RESID>{});
    case EPI_GELU_D: return f(std::integral_constant<int, EPI_GELU_D>{});
    case EPI_MUL_AUX: return f(std::integral_constant<int, EPI_MUL_AUX>{});
    case EPI_DGELU: return f(std::integral_constant<int, EPI_DGELU>{});
  }
  maeclip::set_error("%s: bad epilogue %d", who, a.epilogue);
  return -1;
}

// ------------------------------------------- bf16 fragment reader (v1, v2)
// 8 consecutive k (k = 32 ks + 8 g + j, g = lane >> 4) of tile row rs + (lane & 15).
// KC tile: [rows][128 B], 16-B chunks XOR-swizzled by (row >> 1) & 7.
// RC tile: [64 k][PITCH B], 8-B units XOR-swizzled by swz_rc(k), read with the
// hardware transpose.
template <int LAY, int PITCH>
__device__ __forceinline__ v8s load_frag_bf16(const char* lds, int rs, int ks, int lane) {
  if (LAY == LAY_KC) {
    const int row = rs + (lane & 15);
    const int chunk = 4 * ks + (lane >> 4);
    return *(const v8s*)(lds + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4));
  } else {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int unit = (rs >> 2) + p;
    v8s v;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int krow = 32 * ks + 8 * g + 4 * h + q;
      const char* a = lds + krow * PITCH + ((unit ^ swz_rc(krow)) << 3);
      v4s t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, a));
      v[4 * h + 0] = t[0];
      v[4 * h + 1] = t[1];
      v[4 * h + 2] = t[2];
      v[4 * h + 3] = t[3];
    }
    return v;
  }
}

// ---------------------------------------------- fragment epilogue (v1, v2)
// The FM x FN accumulator fragments of wave (wm, wn) of the tile at (m0, n0) to
// memory; a lane owns C[m0 + 16 FM wm + 16 i + (lane & 15)][n0 + 16 FN wn + 16 j +
// 4 (lane >> 4) .. + 3]. (m0 and wm are passed apart and summed as the kernels
// always summed them: handing over their sum changes the address code.)
// S > 1: the raw alpha-scaled partial tile goes to this K slice's slab of the
// workspace (the host reduces the slabs). Otherwise bias, epilogue
// EPI (aux / aux_out of type AuxT), beta, the store, and one column-sum partial
// row per 64-row group, reduced over the group's rows in a fixed order
// (deterministic bias gradients).
// BIAS_ONCE: the wave's FN bias vectors are loaded once before the rows (from a
// clamped address, null bias = zeros) and added in the expression of the alpha
// product (v2); otherwise they are loaded per fragment and added in a statement
// of their own, only when there is a bias (v1). The two forms round differently
// where the compiler contracts the first into an fma, so each kernel keeps its own.
// args by value: by reference the compiler keeps alpha / beta / bias of the
// kernel's argument copy in scratch memory.
template <typename AuxT, typename OutT, int EPI, int FM, int FN, bool BIAS_ONCE>
__device__ __forceinline__ void frag_epilogue(const maeclip_gemm_args args, const v4f (&acc)[FM][FN], int S, int m0, int n0,
                                              int wm, int wn, int lane) {
  constexpr int TM = 16 * FM, TN = 16 * FN;  // the wave's rows and columns
  const int M = (int)args.M, N = (int)args.N;
  const int64_t z = blockIdx.z;
  const int g = lane >> 4;
  if (S > 1) {
    float* slab = args.workspace + ((int64_t)z * S + blockIdx.y) * (int64_t)M * N;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int m = m0 + wm * TM + 16 * i + (lane & 15);
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * TN + 16 * j + 4 * g;
        if (m < M && n < N) *(v4f*)(slab + (int64_t)m * N + n) = acc[i][j] * args.alpha;
      }
    }
    return;
  }
  OutT* __restrict__ C = (OutT*)args.C + z * args.strideC;
  const float alpha = args.alpha, beta = args.beta;
  const float* __restrict__ bias = args.bias;
  static_assert(FM % 4 == 0, "a wave owns whole 64-row groups");
  constexpr int NH = FM / 4;  // 64-row groups per wave (column-sum partial rows)
  float csum[NH][FN][4];
#pragma unroll
  for (int hh = 0; hh < NH; ++hh)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) csum[hh][j][r] = 0.f;
  v4f bias4[FN];
  if (BIAS_ONCE) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = min(n0 + wn * TN + 16 * j + 4 * g, N - 4);
      bias4[j] = bias ? *(const v4f*)(bias + n) : v4f{0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * TM + 16 * i + (lane & 15);
    const bool mok = m < M;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + wn * TN + 16 * j + 4 * g;
      if (!mok || n >= N) continue;
      v4f v;
      if (BIAS_ONCE) {
        v = acc[i][j] * alpha + bias4[j];
      } else {
        v = acc[i][j] * alpha;
        if (bias) {
          const v4f bb = *(const v4f*)(bias + n);
          v += bb;
        }
      }
      if (EPI == EPI_GELU) {
        if (args.aux_out) st4<AuxT>((AuxT*)args.aux_out + z * args.strideC + (int64_t)m * args.ldaux + n, v);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_f(v[r]);
      } else if (EPI == EPI_RESID) {
        v += *(const v4f*)(args.resid + z * args.strideC + (int64_t)m * args.ldr + n);
      } else if (EPI == EPI_DGELU) {
        const v4f pre = ld4<AuxT>((const AuxT*)args.aux + z * args.strideC + (int64_t)m * args.ldaux + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= gelu_grad_f(pre[r]);
        if (args.resid) v += *(const v4f*)(args.resid + z * args.strideC + (int64_t)m * args.ldr + n);
      } else if (EPI == EPI_GELU_D) {
        const v4f d = gelu4_inplace(v);
        if (args.aux_out) st4<AuxT>((AuxT*)args.aux_out + z * args.strideC + (int64_t)m * args.ldaux + n, d);
      } else if (EPI == EPI_MUL_AUX) {
        v *= ld4<AuxT>((const AuxT*)args.aux + z * args.strideC + (int64_t)m * args.ldaux + n);
        if (args.resid) v += *(const v4f*)(args.resid + z * args.strideC + (int64_t)m * args.ldr + n);
      }
      OutT* cp = C + (int64_t)m * args.ldc + n;
      if (beta != 0.f) v += beta * ld4<OutT>(cp);
#pragma unroll
      for (int r = 0; r < 4; ++r) csum[i / 4][j][r] += v[r];
      st4<OutT>(cp, v);
    }
  }
  if (args.colsum_partial) {
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = csum[hh][j][r];
          s += __shfl_xor(s, 1, 64);
          s += __shfl_xor(s, 2, 64);
          s += __shfl_xor(s, 4, 64);
          s += __shfl_xor(s, 8, 64);
          csum[hh][j][r] = s;
        }
      const int mrow = m0 + wm * TM + 64 * hh;
      if ((lane & 15) == 0 && mrow < M) {
        float* prow = args.colsum_partial + ((int64_t)z * ((M + 63) / 64) + mrow / 64) * N;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int n = n0 + wn * TN + 16 * j + 4 * g;
          if (n < N) *(v4f*)(prow + n) = v4f{csum[hh][j][0], csum[hh][j][1], csum[hh][j][2], csum[hh][j][3]};
        }
      }
    }
  }
}
