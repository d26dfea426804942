// The device idiom shared by the similarity kernels (clip_loss.hip,
// contrastive.hip, retrieval_eval.hip, and the row sums of retrieval.hip), and
// the argument checks shared by the two loss entry points. One definition of
// each piece: the bitwise-reproducibility claims of those files (the same
// score bits in every pass and every workgroup, the same tau in every kernel of
// a call, sums in one fixed order) rest on all of them running this code.
#pragma once
#include "common.h"

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr float NEG = -1.0e30f;   // "no value yet" of an online max

// one step of the exact-f32 MFMA (v_mfma_f32_16x16x4_f32), bitwise an f32 fma chain in k order
__device__ __forceinline__ v4f mma4(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the lane's 16-byte fragment of k-group b, from its row at + 4(lane>>4) (LDS
// or global) or from registers loaded that way
__device__ __forceinline__ v4f kfrag(const float* row, int b) { return *(const v4f*)(row + 16 * b); }
__device__ __forceinline__ v4f kfrag(const v4f* r, int b) { return r[b]; }

// 16x16 dot tile over NB k-groups of 16: D[4(lane>>4) + r][lane&15], a the
// fragments of the lane's row (of the first operand), b of its column.
// MFMA k mapping: in sub-step s of k-group b, hardware k = lane>>4 carries real
// k = 16b + 4(lane>>4) + s, so each lane reads its operands as 16-byte vectors.
// Two accumulator chains (sub-steps 0, 2 and 1, 3) in one order, added at the
// end: every pass and every kernel that forms a score this way gets the same
// bits. nb < NB (run time) leaves the k-groups from nb on out, fragments included.
template <int NB, class FA, class FB>
__device__ __forceinline__ v4f dot_tile(FA a, FB b, int nb = NB) {
  v4f c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < NB; ++g)
    if (g < nb) {
      const v4f x = kfrag(a, g), y = kfrag(b, g);
      c0 = mma4(x[0], y[0], c0);
      c1 = mma4(x[1], y[1], c1);
      c0 = mma4(x[2], y[2], c0);
      c1 = mma4(x[3], y[3], c1);
    }
  return c0 + c1;
}

// online (max, sumexp): (m, s) <- (m, s) merged with (m2, s2)
__device__ __forceinline__ void merge_ms(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  s = s * __expf(m - M) + s2 * __expf(m2 - M);
  m = M;
}
// x - lse from the parts (max M, log sumexp lz) kept apart: lse = M + log z
// rounded to f32 is off by up to ulp(|M|) / 2 (1e-6 at |x| ~ 30), which nearly
// cancelling gradient terms then amplify; (x - M) - log z has both differences
// exact or small where it matters.
__device__ __forceinline__ float lsub(float x, float M, float lz) { return (x - M) - lz; }

// a per-lane float that is the same in every lane, back in a scalar register
__device__ __forceinline__ float wave_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
// tau of the call: the by-value field, or exp(theta) of the device theta = ln tau.
// The one expression every kernel takes it from, so that every pass of a call
// uses the same value bit for bit (exp(0) = 1 exactly: theta = 0 is the
// by-value tau = 1). a: the kernel's argument struct, with the fields tau and ltau.
template <class K> __device__ __forceinline__ float call_tau(const K& a) {
  if (!a.ltau) return a.tau;
  return wave_uniform(expf(*a.ltau));
}
// an optional device scalar (0 when absent)
__device__ __forceinline__ float call_scalar(const float* p) {
  if (!p) return 0.f;
  return wave_uniform(*p);
}

// K dot products of the wave's row x with the rows y[k], P floats each, in one
// fixed order: lane l the fma chain over columns l, l + 64, ..., then the xor
// butterfly; every lane gets the sums. y[k] = x gives ||x||^2: the L2
// normalisation's forward and backward take it from here, so both see the
// same norm and take the same side of the eps clamp.
template <int K>
__device__ __forceinline__ void row_dots(const float* x, const float* const (&y)[K], int64_t P, int lane, float (&s)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.f;
  for (int64_t c = lane; c < P; c += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = fmaf(x[c], y[k][c], s[k]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += __shfl_xor(s[k], o, 64);
  }
}

// Host: the checks maeclip_clip_loss and maeclip_contrastive_loss share, on the
// fields their args structs have in common, in two groups because the
// contrastive entry has checks of its own between them. fn: the entry point's
// name for the messages.
// Shape and temperature; max_n: the entry point's cap on N.
template <class Args>
int pair_check_shape(const Args* a, const char* fn, int64_t max_n) {
  MC_CHECK_ARG(a->N > 0 && a->N <= max_n, "%s: N must be in [1, %lld] (got %lld)", fn, (long long)max_n, (long long)a->N);
  MC_CHECK_ARG(a->P == 64 || a->P == 128 || a->P == 256 || a->P == 512, "%s: P must be 64, 128, 256 or 512 (got %lld)", fn,
               (long long)a->P);
  MC_CHECK_ARG(a->log_temperature || a->temperature > 0.f, "%s: temperature must be > 0", fn);
  return 0;
}
// Row alignment of I/T, the gradient-row range and the alignment of dI/dT
// (checked when both are given); *gr: the resolved gradient row count, 0
// without gradients. full_rows: dI/dT rows must also hold P floats.
template <class Args>
int pair_check_rows(const Args* a, const char* fn, bool full_rows, int64_t* gr) {
  const int64_t ldi = a->ld_I ? a->ld_I : a->P, ldt = a->ld_T ? a->ld_T : a->P;
  MC_CHECK_ARG(ldi >= a->P && ldt >= a->P && ldi % 4 == 0 && ldt % 4 == 0 && ((uintptr_t)a->I & 15) == 0 &&
                   ((uintptr_t)a->T & 15) == 0,
               "%s: I/T rows must be 16-byte aligned", fn);
  *gr = 0;
  if (a->dI && a->dT) {
    MC_CHECK_ARG(a->grad_row0 >= 0 && a->grad_row0 < a->N && a->grad_rows >= 0 && a->grad_row0 + a->grad_rows <= a->N,
                 "%s: gradient rows out of range", fn);
    *gr = a->grad_rows > 0 ? a->grad_rows : a->N - a->grad_row0;
    const int64_t lddi = a->ld_dI ? a->ld_dI : a->P, lddt = a->ld_dT ? a->ld_dT : a->P;
    MC_CHECK_ARG((!full_rows || (lddi >= a->P && lddt >= a->P)) && lddi % 4 == 0 && lddt % 4 == 0 &&
                     ((uintptr_t)a->dI & 15) == 0 && ((uintptr_t)a->dT & 15) == 0,
                 "%s: dI/dT rows must be 16-byte aligned", fn);
  }
  return 0;
}
