// Stochastic depth (include/maeclip.h "Stochastic depth"): timm's DropPath with
// scale_by_keep on the two residual branches of a pre-LN block, as two
// row-wise kernels beside the GEMMs (whose residual epilogue a dropping block
// does not use):
//   maeclip_droppath_fwd  out = resid + s * branch          (in place on branch)
//   maeclip_droppath_bwd  gs = s * g in the compute dtype + its column partials
// s is one value per (sample, branch key), re-formed from the hash of the
// device step by every wave for the row it owns (one __host__ __device__
// function, also behind maeclip_droppath_scales_host); nothing is stored, no
// launch allocates, synchronises or uses atomics.
//
// Both kernels are HBM-bound. A wave owns whole rows, lane l the 16-byte
// pieces l, l + 64, ... of the row, so consecutive lanes go to consecutive
// addresses; the loads of several pieces (forward) or of two rows (backward)
// are issued before the first is used. Forward: <= 2048 workgroups that stride
// over the rows. Backward: one workgroup per 64-row group, wave w the rows
// w, w + 4, ... of it, column sums kept in registers and combined through LDS
// in a fixed order (the partial of a group is the same whichever launch
// computes it).
#include "common.h"
#include "../../include/maeclip.h"

namespace {
constexpr int NTH = 256;
constexpr int NW = NTH / 64;
constexpr int FW_U = 4;            // 16-byte pieces per lane in flight per stream (forward)
constexpr int FW_GRID_CAP = 2048;  // 256 CUs x 8 workgroups
constexpr int GROUP = 64;          // rows per partial row (backward)
constexpr int BW_MAXC = 8;         // D <= 2048 (backward: the column sums live in registers)

__host__ __device__ inline float dp_scale(uint64_t step_seed, uint64_t sample, uint64_t key, float p, float inv) {
  const float u = (float)(mc_hash4(step_seed, sample, key, (uint64_t)MAECLIP_DROPPATH_FIELD) >> 8) * (1.0f / 16777216.0f);
  return u >= p ? inv : 0.0f;
}

struct DpK {
  const float* resid;
  const float* branch;
  float* out;
  const float* g;
  void* gs;
  float* partial;
  int64_t ld_resid, ld_branch, ld_out, ld_g, ld_gs;
  unsigned M, n;
  int D;
  float p, inv;      // inv = 1 / (1 - p), divided on the host
  uint64_t seed, sample_offset, key;
  const int64_t* step_ptr;
};

// fl(s b) and fl(a + b) as two roundings, i.e. what __fadd_rn(a, __fmul_rn(s, b))
// is meant to say. HIP's _rn intrinsics cannot say it here: the headers define
// them as `return x * y;` / `return x + y;`, compiled under the header's own
// contraction mode, and written with them the forward below came out as
// v_pk_fma_f32 (one rounding). The operators have to stand inside the pragma's
// scope themselves: an fmul / fadd made there carries no contract flag, so no
// pass may fuse it after inlining, whatever -ffp-contract says (as mix.hip's
// mix_val). tests/test_droppath_gpu.py compares every element bit for bit.
__device__ __forceinline__ float dp_mul(float s, float b) {
#pragma clang fp contract(off)
  return s * b;
}
__device__ __forceinline__ float dp_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

__global__ void __launch_bounds__(NTH) droppath_fwd_kernel(const DpK k) {
  const int lane = threadIdx.x & 63;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t sseed = mc_step_seed(k.seed, k.step_ptr);
  const int D = k.D;
  for (unsigned r = blockIdx.x * NW + wave; r < k.M; r += gridDim.x * NW) {
    const float s = dp_scale(sseed, k.sample_offset + (uint64_t)(r / k.n), k.key, k.p, k.inv);
    const float* rr = k.resid + (int64_t)r * k.ld_resid;
    const float* br = k.branch + (int64_t)r * k.ld_branch;
    float* orow = k.out + (int64_t)r * k.ld_out;
    for (int e0 = lane * 4; e0 < D; e0 += 256 * FW_U) {
      v4f a[FW_U], b[FW_U];
#pragma unroll
      for (int u = 0; u < FW_U; ++u) {
        const int e = e0 + u * 256;
        if (e < D) {
          a[u] = ld4<float>(rr + e);
          if (s != 0.f) b[u] = ld4<float>(br + e);   // a dropped sample's branch is not read
        }
      }
#pragma unroll
      for (int u = 0; u < FW_U; ++u) {
        const int e = e0 + u * 256;
        if (e < D) {
          v4f o = a[u];
          if (s != 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = dp_add(a[u][j], dp_mul(s, b[u][j]));
          }
          st4<float>(orow + e, o);
        }
      }
    }
  }
}

template <typename T, int NC>
__global__ void __launch_bounds__(NTH) droppath_bwd_kernel(const DpK k) {
  __shared__ float red[NW][NC * 256];
  const int lane = threadIdx.x & 63;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t sseed = mc_step_seed(k.seed, k.step_ptr);
  const int D = k.D;
  float acc[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.f;
  const unsigned r0 = blockIdx.x * GROUP + wave;
#pragma unroll 1
  for (int i = 0; i < GROUP / NW; i += 2) {
    unsigned r[2];
    float s[2];
    v4f v[2][NC];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      r[h] = r0 + (unsigned)(NW * (i + h));
      s[h] = r[h] < k.M ? dp_scale(sseed, k.sample_offset + (uint64_t)(r[h] / k.n), k.key, k.p, k.inv) : 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int e = c * 256 + lane * 4;
        v[h][c] = (v4f){0.f, 0.f, 0.f, 0.f};
        if (s[h] != 0.f && e < D) v[h][c] = ld4<float>(k.g + (int64_t)r[h] * k.ld_g + e);   // dropped: g is not read
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (r[h] >= k.M) continue;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int e = c * 256 + lane * 4;
        if (e < D) {
          v4f q;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            q[j] = dp_mul(s[h], v[h][c][j]);
            acc[c][j] = dp_add(acc[c][j], q[j]);
          }
          st4<T>((T*)k.gs + (int64_t)r[h] * k.ld_gs + e, q);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = c * 256 + lane * 4 + j;
      if (e < D) red[wave][e] = acc[c][j];
    }
  __syncthreads();
  for (int e = threadIdx.x; e < D; e += NTH) {
    float t = red[0][e];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += red[w][e];
    k.partial[(int64_t)blockIdx.x * D + e] = t;
  }
}

// [p, p + bytes of M rows of D floats at stride ld)
struct Span {
  uintptr_t lo, hi;
};
Span span_of(const void* p, int64_t M, int64_t D, int64_t ld, size_t esz) {
  const uintptr_t lo = (uintptr_t)p;
  return {lo, lo + (uintptr_t)((M - 1) * ld + D) * esz};
}
bool overlaps(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }
}  // namespace

// the checks both entry points share; fills the kernels' argument block
static int32_t droppath_check(const maeclip_droppath_args* a, const char* who, DpK& k) {
  MC_CHECK_ARG(a, "%s: null pointer", who);
  MC_CHECK_ARG(a->p >= 0.f && a->p < 1.f, "%s: p must be in [0, 1) (got %g)", who, (double)a->p);
  MC_CHECK_ARG(a->n >= 1 && a->n <= 0x7fffffffLL, "%s: n must be in [1, 2^31) (got %lld)", who, (long long)a->n);
  MC_CHECK_ARG(a->M >= 0 && a->M <= 0x7fffffffLL - 256, "%s: M must be in [0, 2^31 - 256) (got %lld)", who, (long long)a->M);
  MC_CHECK_ARG(a->M % a->n == 0, "%s: M (%lld) must be a multiple of n (%lld)", who, (long long)a->M, (long long)a->n);
  MC_CHECK_ARG(a->D >= 4 && a->D <= 0x3fffffffLL && a->D % 4 == 0, "%s: D must be a positive multiple of 4 below 2^30 (got %lld)", who,
               (long long)a->D);
  MC_CHECK_ARG(a->k >= 0, "%s: k must be >= 0 (got %d)", who, a->k);
  MC_CHECK_ARG(((uintptr_t)a->step_ptr & 7) == 0, "%s: step_ptr must be 8-byte aligned", who);
  k = DpK{};
  k.M = (unsigned)a->M;
  k.n = (unsigned)a->n;
  k.D = (int)a->D;
  k.p = a->p;
  const volatile float keep = 1.0f - a->p;
  k.inv = 1.0f / keep;
  k.seed = a->seed;
  k.sample_offset = a->sample_offset;
  k.key = (uint64_t)a->k;
  k.step_ptr = a->step_ptr;
  return 0;
}

#define DP_CHECK_ROWS(ptr, ld, align, who, name)                                                                    \
  MC_CHECK_ARG(((uintptr_t)(ptr) & ((align)-1)) == 0 && (ld) >= a->D && (ld) % 4 == 0,                              \
               "%s: %s must be %d-byte aligned with a row stride >= D that is a multiple of 4", who, name, (int)(align))

extern "C" int32_t maeclip_droppath_fwd(const maeclip_droppath_args* a, void* stream) {
  const char* who = "maeclip_droppath_fwd";
  DpK k;
  if (int32_t rc = droppath_check(a, who, k)) return rc;
  MC_CHECK_ARG(a->resid && a->branch && a->out, "%s: null pointer", who);
  DP_CHECK_ROWS(a->resid, a->ld_resid, 16, who, "resid");
  DP_CHECK_ROWS(a->branch, a->ld_branch, 16, who, "branch");
  DP_CHECK_ROWS(a->out, a->ld_out, 16, who, "out");
  if (a->M == 0) return 0;
  const Span so = span_of(a->out, a->M, a->D, a->ld_out, 4);
  MC_CHECK_ARG(!overlaps(so, span_of(a->resid, a->M, a->D, a->ld_resid, 4)), "%s: out overlaps resid", who);
  MC_CHECK_ARG((a->out == a->branch && a->ld_out == a->ld_branch) || !overlaps(so, span_of(a->branch, a->M, a->D, a->ld_branch, 4)),
               "%s: out overlaps branch without being branch (in place needs out == branch and equal strides)", who);
  k.resid = a->resid;
  k.branch = a->branch;
  k.out = a->out;
  k.ld_resid = a->ld_resid;
  k.ld_branch = a->ld_branch;
  k.ld_out = a->ld_out;
  const int64_t blocks = (a->M + NW - 1) / NW;
  const dim3 grid((unsigned)(blocks < FW_GRID_CAP ? blocks : FW_GRID_CAP));
  hipLaunchKernelGGL(droppath_fwd_kernel, grid, dim3(NTH), 0, (hipStream_t)stream, k);
  MC_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int64_t maeclip_droppath_partial_rows(int64_t M) { return M <= 0 ? 0 : (M + GROUP - 1) / GROUP; }

template <typename T>
static void launch_droppath_bwd(const DpK& k, hipStream_t s) {
  const dim3 grid((k.M + GROUP - 1) / GROUP);
  switch ((k.D + 255) / 256) {
#define DP_BW(NC) \
  case NC: hipLaunchKernelGGL((droppath_bwd_kernel<T, NC>), grid, dim3(NTH), 0, s, k); break;
    DP_BW(1) DP_BW(2) DP_BW(3) DP_BW(4) DP_BW(5) DP_BW(6) DP_BW(7) DP_BW(8)
#undef DP_BW
  }
}

extern "C" int32_t maeclip_droppath_bwd(const maeclip_droppath_args* a, void* stream) {
  const char* who = "maeclip_droppath_bwd";
  DpK k;
  if (int32_t rc = droppath_check(a, who, k)) return rc;
  MC_CHECK_ARG(a->g && a->gs && a->partial, "%s: null pointer", who);
  MC_CHECK_ARG(a->gs_dtype == MAECLIP_F32 || a->gs_dtype == MAECLIP_BF16, "%s: gs_dtype must be 0 (fp32) or 1 (bf16) (got %d)",
               who, a->gs_dtype);
  MC_CHECK_ARG(a->D <= BW_MAXC * 256, "%s: D must be <= %d (got %lld)", who, BW_MAXC * 256, (long long)a->D);
  const bool bf = a->gs_dtype == MAECLIP_BF16;
  DP_CHECK_ROWS(a->g, a->ld_g, 16, who, "g");
  DP_CHECK_ROWS(a->gs, a->ld_gs, bf ? 8 : 16, who, "gs");
  MC_CHECK_ARG(((uintptr_t)a->partial & 3) == 0, "%s: partial must be 4-byte aligned", who);
  if (a->M == 0) return 0;
  const Span sg = span_of(a->g, a->M, a->D, a->ld_g, 4), ss = span_of(a->gs, a->M, a->D, a->ld_gs, bf ? 2 : 4);
  const Span sp = span_of(a->partial, maeclip_droppath_partial_rows(a->M), a->D, a->D, 4);
  MC_CHECK_ARG(!overlaps(ss, sg) && !overlaps(sp, sg) && !overlaps(sp, ss), "%s: g, gs and partial must not overlap", who);
  k.g = a->g;
  k.gs = a->gs;
  k.partial = a->partial;
  k.ld_g = a->ld_g;
  k.ld_gs = a->ld_gs;
  if (bf) {
    launch_droppath_bwd<bf16_t>(k, (hipStream_t)stream);
  } else {
    launch_droppath_bwd<float>(k, (hipStream_t)stream);
  }
  MC_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int32_t maeclip_droppath_scales_host(float* scales, int64_t B, const int32_t* keys, int32_t nk, float p,
                                                uint64_t seed, uint64_t sample_offset, const int64_t* host_step) {
  const char* who = "maeclip_droppath_scales_host";
  MC_CHECK_ARG(scales && keys, "%s: null pointer", who);
  MC_CHECK_ARG(B >= 0 && nk >= 0, "%s: B and nk must be >= 0", who);
  maeclip_droppath_args a = {};
  a.p = p;
  a.n = 1;
  a.D = 4;
  a.seed = seed;
  a.sample_offset = sample_offset;
  a.step_ptr = host_step;
  DpK k;
  if (int32_t rc = droppath_check(&a, who, k)) return rc;      // p and the step pointer, whatever nk is
  for (int32_t i = 0; i < nk; ++i) MC_CHECK_ARG(keys[i] >= 0, "%s: k must be >= 0 (got %d)", who, keys[i]);
  const uint64_t sseed = mc_step_seed(seed, host_step);
  for (int32_t i = 0; i < nk; ++i)
    for (int64_t b = 0; b < B; ++b)
      scales[(int64_t)i * B + b] = dp_scale(sseed, sample_offset + (uint64_t)b, (uint64_t)keys[i], k.p, k.inv);
  return 0;
}
