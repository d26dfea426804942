// Softmax cross-entropy over class logits, forward and backward, fp32 always:
// torch.nn.functional.cross_entropy with label_smoothing, class-index or
// class-probability targets (include/maeclip.h "softmax cross-entropy").
//
// Per row i of logits [M, C] (row stride ld >= C, columns >= C never read):
//   m = max_j x_j ; lz = log sum_j exp(x_j - m) ; lse = m + lz ; p_j = exp(x_j - lse)
//   t_j = (1 - eps) [j == y_i] + eps / C          (hard)
//   t_j = (1 - eps) Y_ij + eps / C                (soft)
//   r_i = (sum_j t_j) lse - sum_j t_j x_j = (sum_j t_j) lz - sum_j t_j (x_j - m)
//   loss = s sum_i r_i,  s = loss_scale / M
//   dlogits_ij = g s ((sum_j t_j) p_ij - t_ij)
//   rank_i = #{ j : x_j > x_y, or x_j == x_y and j < y }
// The row loss is taken in the shifted form on the right: every term is a
// difference to the row maximum, so a row at |x| ~ 1e4 loses nothing to the
// cancellation of lse against x_y. For hard targets sum_j t_j (x_j - m) is
// (1 - eps) (x_y - m) + (eps / C) sum_j (x_j - m): no pass over the targets.
//
// lse leaves the forward as two floats: lse[i] = fl(m + lz) and lse_lo[i] = the
// rounding error of that sum (TwoSum). fl(m + lz) alone is off by ulp(|m|) / 2,
// 5e-4 at |m| ~ 1e4, and the backward's p = exp(x - lse) would carry that as a
// relative error of every p of the row; (x - lse) - lse_lo has it back.
//
// Forward launches (fixed-order sums everywhere, no atomics, no allocation, no
// sync): the row pass, then a one-workgroup reduce of the M row terms in double.
//   row pass, C <= XENT_WAVE_COLS:  one wave per row, four rows per workgroup;
//             C <= XENT_REG_COLS:   one workgroup per row (so M = 256 rows are
//                                   256 workgroups, not 64);
//             both hold the row in registers (NV 16-byte pieces per thread,
//             thread t of TPR the columns 4 (c TPR + t) .. + 3 of piece c): one
//             read of the logits, the maximum first, then every sum;
//             C > XENT_REG_COLS:    one workgroup per row streams the row once,
//             16 columns per thread and step, with an online (max, sums) state
//             per thread: a new maximum m' rescales sum exp by exp(m - m') and
//             shifts the sums of (x - m) by (count or sum of Y) (m - m').
//   The 16-byte loads need a 16-byte aligned base and ld % 4 == 0 (of the
//   logits and of Y); otherwise the same threads read the same columns with
//   4-byte loads (the VEC template argument), so both give the same bits. The
//   last piece of a row, where it reaches past C, is read element by element.
// Backward: one launch, elementwise given lse: workgroup (row group, chunk of
// 16 TPR columns); thread t reads its four pieces of the logits, then writes
// them, so dlogits == logits is safe; columns C .. ld_d - 1 get zeros. Soft
// targets need sum_j Y_ij first: every workgroup of the row sums the row of Y in
// one fixed order (a second read of Y, from L2 for all but the first).
#include "common.h"
#include "../../include/maeclip.h"

namespace {
constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int XENT_WAVE_COLS = 256;    // rows up to here: one wave per row
constexpr int XENT_REG_COLS = 8192;    // the register bound: longer rows are streamed
constexpr int U = 4;                   // 16-byte pieces per thread and step (streamed forward, backward)
constexpr float NEG = -3.0e38f;        // "no value yet" of a maximum

struct XentK {
  const float* x;
  int64_t ld;
  const void* labels;
  int lab64;
  const float* Y;
  int64_t ldy;
  int64_t M;
  int C;
  float eps, ome, epsC, s;   // eps, 1 - eps, eps / C, loss_scale / M
  float* rowterm;
  float* lse;
  float* lse_lo;
  int* rank;
  const float* lse_in;
  const float* lse_lo_in;
  const float* gout;
  float* dx;
  int64_t ldd;
  int64_t nch;               // backward: column chunks per row
};

// columns col .. col + 3 of a row of C columns; nothing at or past C is read
template <bool VEC>
__device__ __forceinline__ v4f load4(const float* row, int64_t col, int C, float fill) {
  const int64_t left = (int64_t)C - col;
  if (VEC && left >= 4) return *(const v4f*)(row + col);
  v4f v = {fill, fill, fill, fill};
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r < left) v[r] = row[col + r];
  return v;
}

// columns col .. col + 3 of a row of n columns
template <bool VEC>
__device__ __forceinline__ void store4(float* row, int64_t col, int64_t n, v4f v) {
  const int64_t left = n - col;
  if (VEC && left >= 4) {
    *(v4f*)(row + col) = v;
    return;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r < left) row[col + r] = v[r];
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sums / maximum over the TPR threads of a row: the wave's, then (TPR = NT) the
// four waves' in wave order through LDS. Every thread of the row gets the result.
template <int TPR>
__device__ __forceinline__ float row_max(float v, float* red) {
  v = wave_max(v);
  if (TPR == 64) return v;
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
template <int TPR, int K>
__device__ __forceinline__ void row_sum(float (&v)[K], float* red) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (TPR == 64) return;
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[w * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
}
template <int TPR>
__device__ __forceinline__ int row_sum_int(int v, int* red) {
  v = wave_sum_int(v);
  if (TPR == 64) return v;
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ int64_t label_of(const XentK& a, int64_t i) {
  if (!a.labels) return -1;
  return a.lab64 ? ((const int64_t*)a.labels)[i] : (int64_t)((const int32_t*)a.labels)[i];
}

// what the thread adds for the element x of column col: sums relative to m
struct Acc {
  float se = 0.f, sd = 0.f, sy = 0.f, syd = 0.f;
  int rk = 0;
  __device__ __forceinline__ void add(float x, float yv, float m, bool soft, float xy, int64_t col, int64_t y) {
    const float d = x - m;
    se += __expf(d);
    sd += d;
    if (soft) {
      sy += yv;
      syd = fmaf(yv, d, syd);
    }
    rk += (x > xy || (x == xy && col < y)) ? 1 : 0;
  }
};

// the row's sums (relative to its maximum m) -> row term, lse, rank
template <int TPR>
__device__ __forceinline__ void finish(const XentK& a, bool live, int64_t i, float m, Acc acc, float xy, bool yok,
                                       float* red, int* redi) {
  float v[4] = {acc.se, acc.sd, acc.sy, acc.syd};
  row_sum<TPR, 4>(v, red);
  const int rk = row_sum_int<TPR>(acc.rk, redi);
  if (threadIdx.x % TPR != 0 || !live) return;
  const bool soft = a.Y != nullptr;
  const float lz = logf(v[0]);
  float st = 0.f, td = 0.f;   // sum_j t_j, sum_j t_j (x_j - m)
  const bool any = soft || yok;
  if (soft) {
    st = fmaf(a.ome, v[2], a.eps);
    td = a.ome * v[3];
  } else if (yok) {
    st = fmaf(a.ome, 1.f, a.eps);
    td = a.ome * (xy - m);
  }
  if (any && a.eps > 0.f) td = fmaf(a.epsC, v[1], td);
  a.rowterm[i] = any ? a.s * (st * lz - td) : 0.f;
  // TwoSum of m + lz
  const float hi = m + lz, bb = hi - m;
  a.lse[i] = hi;
  if (a.lse_lo) a.lse_lo[i] = (m - (hi - bb)) + (lz - bb);
  if (a.rank) a.rank[i] = yok ? rk : a.C;
}

// ------------------------------------------------------------ forward, row in registers
// TPR threads per row, NT / TPR rows per workgroup; rows past M repeat row M - 1
// (every wave runs the same code, nothing of them is stored)
template <int TPR, int NV, bool VEC>
__global__ void __launch_bounds__(NT) xent_fwd_reg_kernel(const XentK a) {
  __shared__ float red[NW * 4];
  __shared__ int redi[NW];
  const int t = threadIdx.x % TPR;
  const int64_t i = (int64_t)blockIdx.x * (NT / TPR) + threadIdx.x / TPR;
  const bool live = i < a.M;
  const int64_t ir = live ? i : a.M - 1;
  const int C = a.C;
  const float* row = a.x + ir * a.ld;
  const bool soft = a.Y != nullptr;
  const float* yrow = soft ? a.Y + ir * a.ldy : nullptr;
  const int64_t y = label_of(a, ir);
  const bool yok = y >= 0 && y < C;
  const float xy = yok ? row[y] : 0.f;
  v4f x[NV], yv[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) x[c] = load4<VEC>(row, 4 * (c * TPR + t), C, NEG);
#pragma unroll
  for (int c = 0; c < NV; ++c) yv[c] = soft ? load4<VEC>(yrow, 4 * (c * TPR + t), C, 0.f) : v4f{0.f, 0.f, 0.f, 0.f};
  float m = NEG;
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, x[c][r]);
  m = row_max<TPR>(m, red);
  Acc acc;
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = 4 * (c * TPR + t) + r;
      if (col < C) acc.add(x[c][r], yv[c][r], m, soft, xy, col, y);
    }
  finish<TPR>(a, live, i, m, acc, xy, yok, red, redi);
}

// ------------------------------------------------------------ forward, streamed
// one workgroup per row
template <bool VEC>
__global__ void __launch_bounds__(NT) xent_fwd_stream_kernel(const XentK a) {
  __shared__ float red[NW * 4];
  __shared__ int redi[NW];
  const int t = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int C = a.C;
  const float* row = a.x + i * a.ld;
  const bool soft = a.Y != nullptr;
  const float* yrow = soft ? a.Y + i * a.ldy : nullptr;
  const int64_t y = label_of(a, i);
  const bool yok = y >= 0 && y < C;
  const float xy = yok ? row[y] : 0.f;
  float m = NEG, cnt = 0.f;
  Acc acc;
  for (int64_t base = 0; base < C; base += NT * 4 * U) {
    v4f x[U], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = load4<VEC>(row, base + 4 * (u * NT + t), C, NEG);
#pragma unroll
    for (int u = 0; u < U; ++u) yv[u] = soft ? load4<VEC>(yrow, base + 4 * (u * NT + t), C, 0.f) : v4f{0.f, 0.f, 0.f, 0.f};
    float bm = NEG;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) bm = fmaxf(bm, x[u][r]);
    if (bm > m) {
      if (cnt > 0.f) {
        const float dm = m - bm;
        acc.se *= __expf(dm);
        acc.sd = fmaf(cnt, dm, acc.sd);
        acc.syd = fmaf(acc.sy, dm, acc.syd);
      }
      m = bm;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t col = base + 4 * (u * NT + t) + r;
        if (col < C) {
          acc.add(x[u][r], yv[u][r], m, soft, xy, col, y);
          cnt += 1.f;
        }
      }
  }
  const float mr = row_max<NT>(m, red);
  if (cnt > 0.f) {
    const float dm = m - mr;
    acc.se *= __expf(dm);
    acc.sd = fmaf(cnt, dm, acc.sd);
    acc.syd = fmaf(acc.sy, dm, acc.syd);
  }
  finish<NT>(a, true, i, mr, acc, xy, yok, red, redi);
}

// ------------------------------------------------------------ reduce
// loss = sum of the M row terms (and their copy to row_loss): one workgroup, in
// double and in a fixed order (strided per-thread sums, then a binary tree)
__global__ void __launch_bounds__(NT) xent_reduce_kernel(const float* __restrict__ rowterm, int64_t n,
                                                         float* __restrict__ loss, float* __restrict__ row_loss) {
  __shared__ double red[NT];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += NT) {
    s += (double)rowterm[i];
    if (row_loss) row_loss[i] = rowterm[i];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)red[0];
}

// ------------------------------------------------------------ backward
// workgroup = (row group, column chunk of 16 TPR columns), flattened into
// blockIdx.x; the chunks run to ld_d, past C they write zeros
template <int TPR, bool VEC>
__global__ void __launch_bounds__(NT) xent_bwd_kernel(const XentK a) {
  __shared__ float red[NW];
  const int t = threadIdx.x % TPR;
  const int64_t rg = blockIdx.x / a.nch, ch = blockIdx.x % a.nch;
  const int64_t i = rg * (NT / TPR) + threadIdx.x / TPR;
  const bool live = i < a.M;
  const int64_t ir = live ? i : a.M - 1;
  const int C = a.C;
  const float* row = a.x + ir * a.ld;
  const bool soft = a.Y != nullptr;
  const float* yrow = soft ? a.Y + ir * a.ldy : nullptr;
  const int64_t y = label_of(a, ir);
  const bool yok = y >= 0 && y < C;
  const float gs = (a.gout ? *a.gout : 1.f) * a.s;
  const float hi = a.lse_in[ir], lo = a.lse_lo_in ? a.lse_lo_in[ir] : 0.f;
  float st = yok ? fmaf(a.ome, 1.f, a.eps) : 0.f;
  if (soft) {
    float sy[1] = {0.f};
    for (int64_t base = 0; base < C; base += TPR * 4 * U) {
      v4f yv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) yv[u] = load4<VEC>(yrow, base + 4 * (u * TPR + t), C, 0.f);
#pragma unroll
      for (int u = 0; u < U; ++u) sy[0] += (yv[u][0] + yv[u][1]) + (yv[u][2] + yv[u][3]);
    }
    row_sum<TPR, 1>(sy, red);
    st = fmaf(a.ome, sy[0], a.eps);
  }
  const bool zero = !soft && !yok;   // an invalid hard label: a zero gradient row
  const int64_t base = ch * (TPR * 4 * U);
  v4f x[U], yv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) x[u] = load4<VEC>(row, base + 4 * (u * TPR + t), C, 0.f);
#pragma unroll
  for (int u = 0; u < U; ++u) yv[u] = soft ? load4<VEC>(yrow, base + 4 * (u * TPR + t), C, 0.f) : v4f{0.f, 0.f, 0.f, 0.f};
  float* drow = a.dx + ir * a.ldd;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t col = base + 4 * (u * TPR + t);
    v4f g;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t cc = col + r;
      const float p = __expf((x[u][r] - hi) - lo);
      const float tj = fmaf(a.ome, soft ? yv[u][r] : (cc == y ? 1.f : 0.f), a.epsC);
      g[r] = (cc < C && !zero) ? gs * (st * p - tj) : 0.f;
    }
    if (live) store4<VEC>(drow, col, a.ldd, g);
  }
}

// ------------------------------------------------------------ host
bool vec_ok(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

int check_common(const maeclip_xent_args* a, const char* who) {
  MC_CHECK_ARG(a && a->logits, "%s: null pointer (args / logits)", who);
  MC_CHECK_ARG(a->M >= 1 && a->M <= 0x7fffffffLL, "%s: M must be in [1, 2^31) (got %lld)", who, (long long)a->M);
  MC_CHECK_ARG(a->C >= 1 && a->C <= 0x7fffffffLL, "%s: C must be in [1, 2^31) (got %lld)", who, (long long)a->C);
  MC_CHECK_ARG(a->ld >= a->C, "%s: ld must be >= C (got %lld < %lld)", who, (long long)a->ld, (long long)a->C);
  MC_CHECK_ARG(a->label_smoothing >= 0.f && a->label_smoothing < 1.f, "%s: label_smoothing must be in [0, 1) (got %g)",
               who, (double)a->label_smoothing);
  MC_CHECK_ARG(a->soft_targets == 0 || a->soft_targets == 1, "%s: soft_targets must be 0 or 1", who);
  MC_CHECK_ARG(a->label_dtype == 0 || a->label_dtype == 1, "%s: label_dtype must be 0 (int32) or 1 (int64)", who);
  if (a->soft_targets) {
    MC_CHECK_ARG(a->targets, "%s: exactly one of labels / targets defines the loss: soft_targets without targets", who);
    MC_CHECK_ARG(a->ld_t >= a->C, "%s: ld_t must be >= C (got %lld < %lld)", who, (long long)a->ld_t, (long long)a->C);
  } else {
    MC_CHECK_ARG(a->labels && !a->targets,
                 "%s: exactly one of labels / targets defines the loss: hard targets take labels and no targets", who);
  }
  MC_CHECK_ARG(((uintptr_t)a->logits & 3) == 0 && ((uintptr_t)a->targets & 3) == 0 &&
                   ((uintptr_t)a->labels & (a->label_dtype ? 7 : 3)) == 0 && ((uintptr_t)a->loss & 3) == 0 &&
                   ((uintptr_t)a->row_loss & 3) == 0 && ((uintptr_t)a->lse & 3) == 0 && ((uintptr_t)a->lse_lo & 3) == 0 &&
                   ((uintptr_t)a->rank & 3) == 0 && ((uintptr_t)a->dlogits & 3) == 0,
               "%s: float / int32 pointers must be 4-byte aligned, int64 labels 8-byte aligned", who);
  return 0;
}

XentK make_k(const maeclip_xent_args& a) {
  XentK k = {};
  k.x = a.logits;
  k.ld = a.ld;
  k.labels = a.labels;
  k.lab64 = a.label_dtype;
  k.Y = a.soft_targets ? a.targets : nullptr;
  k.ldy = a.ld_t;
  k.M = a.M;
  k.C = (int)a.C;
  k.eps = a.label_smoothing;
  k.ome = 1.f - a.label_smoothing;
  k.epsC = a.label_smoothing / (float)a.C;
  k.s = a.loss_scale / (float)a.M;
  return k;
}

template <int TPR, int NV>
void launch_fwd_reg(const XentK& k, bool vec, hipStream_t s) {
  const unsigned grid = (unsigned)((k.M + NT / TPR - 1) / (NT / TPR));
  if (vec) {
    hipLaunchKernelGGL((xent_fwd_reg_kernel<TPR, NV, true>), dim3(grid), dim3(NT), 0, s, k);
  } else {
    hipLaunchKernelGGL((xent_fwd_reg_kernel<TPR, NV, false>), dim3(grid), dim3(NT), 0, s, k);
  }
}

}  // namespace

extern "C" size_t maeclip_xent_workspace(int64_t M) {
  if (M < 1) M = 1;
  return ((size_t)M * sizeof(float) + 15) / 16 * 16;
}

extern "C" int32_t maeclip_xent_fwd(const maeclip_xent_args* a, void* stream) {
  if (check_common(a, "maeclip_xent_fwd")) return -1;
  MC_CHECK_ARG(a->loss && a->lse, "maeclip_xent_fwd: null pointer (loss / lse)");
  MC_CHECK_ARG(!a->rank || a->labels, "maeclip_xent_fwd: rank needs labels");
  MC_CHECK_ARG(a->workspace && a->ws_bytes >= maeclip_xent_workspace(a->M) && ((uintptr_t)a->workspace & 15) == 0,
               "maeclip_xent_fwd: workspace too small or misaligned");
  hipStream_t s = (hipStream_t)stream;
  XentK k = make_k(*a);
  k.rowterm = (float*)a->workspace;
  k.lse = a->lse;
  k.lse_lo = a->lse_lo;
  k.rank = a->rank;
  const bool vec = vec_ok(a->logits, a->ld) && (!k.Y || vec_ok(k.Y, a->ld_t));
  const int64_t C = a->C;
  if (C <= XENT_WAVE_COLS) {
    launch_fwd_reg<64, 1>(k, vec, s);
  } else if (C <= 1024) {
    launch_fwd_reg<NT, 1>(k, vec, s);
  } else if (C <= 2048) {
    launch_fwd_reg<NT, 2>(k, vec, s);
  } else if (C <= 4096) {
    launch_fwd_reg<NT, 4>(k, vec, s);
  } else if (C <= XENT_REG_COLS) {
    launch_fwd_reg<NT, 8>(k, vec, s);
  } else if (vec) {
    hipLaunchKernelGGL(xent_fwd_stream_kernel<true>, dim3((unsigned)k.M), dim3(NT), 0, s, k);
  } else {
    hipLaunchKernelGGL(xent_fwd_stream_kernel<false>, dim3((unsigned)k.M), dim3(NT), 0, s, k);
  }
  MC_CHECK_LAUNCH("maeclip_xent_fwd(rows)");
  hipLaunchKernelGGL(xent_reduce_kernel, dim3(1), dim3(NT), 0, s, k.rowterm, k.M, a->loss, a->row_loss);
  MC_CHECK_LAUNCH("maeclip_xent_fwd(reduce)");
  return 0;
}

extern "C" int32_t maeclip_xent_bwd(const maeclip_xent_args* a, const float* grad_output, void* stream) {
  if (check_common(a, "maeclip_xent_bwd")) return -1;
  MC_CHECK_ARG(a->dlogits && a->lse, "maeclip_xent_bwd: null pointer (dlogits / lse)");
  MC_CHECK_ARG(a->ld_d >= a->C, "maeclip_xent_bwd: ld_d must be >= C (got %lld < %lld)", (long long)a->ld_d,
               (long long)a->C);
  MC_CHECK_ARG(a->dlogits != a->logits || a->ld_d == a->ld, "maeclip_xent_bwd: in place needs ld_d == ld");
  MC_CHECK_ARG(((uintptr_t)grad_output & 3) == 0, "maeclip_xent_bwd: grad_output must be 4-byte aligned");
  const bool wave = a->C <= XENT_WAVE_COLS;
  const int tpr = wave ? 64 : NT;
  const int64_t nch = (a->ld_d + tpr * 4 * U - 1) / (tpr * 4 * U);
  const int64_t nrg = (a->M + NT / tpr - 1) / (NT / tpr);
  MC_CHECK_ARG(nch <= 0x7fffffffLL / nrg, "maeclip_xent_bwd: M x ld_d too large for one launch");
  hipStream_t s = (hipStream_t)stream;
  XentK k = make_k(*a);
  k.lse_in = a->lse;
  k.lse_lo_in = a->lse_lo;
  k.gout = grad_output;
  k.dx = a->dlogits;
  k.ldd = a->ld_d;
  k.nch = nch;
  const bool vec = vec_ok(a->logits, a->ld) && vec_ok(a->dlogits, a->ld_d) && (!k.Y || vec_ok(k.Y, a->ld_t));
  const dim3 grid((unsigned)(nch * nrg));
  if (wave) {
    if (vec) {
      hipLaunchKernelGGL((xent_bwd_kernel<64, true>), grid, dim3(NT), 0, s, k);
    } else {
      hipLaunchKernelGGL((xent_bwd_kernel<64, false>), grid, dim3(NT), 0, s, k);
    }
  } else if (vec) {
    hipLaunchKernelGGL((xent_bwd_kernel<NT, true>), grid, dim3(NT), 0, s, k);
  } else {
    hipLaunchKernelGGL((xent_bwd_kernel<NT, false>), grid, dim3(NT), 0, s, k);
  }
  MC_CHECK_LAUNCH("maeclip_xent_bwd");
  return 0;
}
