// Hard-target contrastive losses on L2-normalised (or any) embeddings, forward +
// closed-form backward, fp32 always, and no N x N matrix in memory.
//
//   l_ij = (I_i . T_j) / tau + b            (b = 0 for InfoNCE)
// InfoNCE (the OpenAI-CLIP loss: identity targets, symmetric cross-entropy)
//   loss  = (1/2N) sum_i [lse_j(l_ij) + lse_j(l_ji) - 2 l_ii]
//   dl_ij = (exp(l_ij - lse_row_i) + exp(l_ij - lse_col_j) - 2 delta_ij) / 2N
// SigLIP (pairwise sigmoid, z_ij = 2 delta_ij - 1)
//   loss  = -(1/N) sum_ij log sigma(z_ij l_ij),  log sigma(x) = min(x, 0) - log1p(exp(-|x|))
//   dl_ij = -z_ij sigma(-z_ij l_ij) / N
// Both: dI_i = (1/tau) sum_j dl_ij T_j, dT_i = (1/tau) sum_j dl_ji I_j for the
// rows [grad_row0, +grad_rows) only; d loss / d theta = -sum dl_ij (l_ij - b) and
// d loss / d b = sum dl_ij over the image rows i of that slice.
//
// The two gradients are one problem stated twice. Role 0 owns X = I and meets
// Y = T, role 1 owns X = T and meets Y = I; with m_ij = (X_i . Y_j) / tau + b
// (role 1: m_ij = l_ji) both are  G_i = (1/tau) sum_j w_ij Y_j,  w_ij the dl of
// (row statistics of role, column statistics = row statistics of the other
// role). So every kernel below is written for "a role", selected by blockIdx.z.
//
// Launches (fixed-order sums everywhere, no atomics, no allocation, no sync):
//   stats   (InfoNCE) workgroup (16 rows i of X, one j-split, role): the 16x16
//           tiles m[j][i] on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32, bitwise
//           an f32 fma chain), wave w the j-tiles w, w + 4, ... of the split;
//           online (max, sumexp) of the row -> part; role 0 also keeps l_ii.
//   combine (InfoNCE) per row: (max M, log z) of both roles (kept apart: x - lse
//           is taken as (x - M) - log z) and the row's loss term.
//   grad    workgroup (16 gradient rows, a chunk of PC columns of P, role): wave
//           w recomputes the tiles m[j][i] of its j-tiles with the SAME fma chain
//           as the stats pass (so l - lse is consistent), forms w_ij in
//           registers and adds Y_j^T (.) w on the MFMA into PC / 4 accumulator
//           registers; the four waves are added in a fixed tree and row i gets
//           16-B stores. PC = min(P, 256) (128 at P = 512), or 64 when the wide chunk would leave
//           most CUs without a workgroup (the tile products are then recomputed
//           per chunk: 5/8 of the MFMA work per workgroup for 4x the workgroups).
//           Role 0, chunk 0 also sums the per-row terms of d theta and d b.
//           SigLIP has no statistics, so its loss comes from the same launch:
//           extra "loss" workgroups (one per 16 rows of the full N, role 0) run
//           the products alone and write the row's loss term.
//   reduce  one workgroup: loss = sum of the row terms, d theta, d b (double,
//           fixed order).
// The dot tile and its MFMA k mapping, the online (max, sumexp) merge and tau
// and b of the call are simtile.h's, shared with clip_loss.hip and
// retrieval_eval.hip. The workgroup's own 16 rows X_i sit in LDS (row stride
// P + 4), the Y_j rows are read from global memory.
#include "simtile.h"
#include "../../include/maeclip.h"

namespace {
constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int64_t MAX_N = 262144;

struct ConK {
  const float* X[2];   // [0] = I, [1] = T
  int64_t ld[2];
  int N, P, kind;
  float tau;
  const float* ltau;   // device theta = ln tau, or null: tau by value
  const float* bias;   // device b (SigLIP), or null: 0
  int nrep, Js;        // stats: j-tiles per workgroup, number of j-splits
  float* part;         // [2][Js][N] (max, sumexp)
  float* stat;         // [2][N] (max, log sumexp): role 0 rows of l, role 1 columns of l
  float* diag;         // [N] l_ii
  float* rowterm;      // [N] per-row loss terms
  float* dtrow;        // [16 * gradient row blocks] per-row terms of d loss / d theta
  float* dbrow;        // [16 * gradient row blocks] per-row terms of d loss / d b
  int g0, Ng, ngb;     // gradient rows, gradient row blocks
};

// the workgroup's 16 rows of X from row i0 -> LDS [16][P + 4] (zero rows past N)
template <int NB>
__device__ __forceinline__ void stage_rows(const float* X, int64_t ld, int i0, int N, float* Xi) {
  constexpr int P = 64 * NB, RS = P + 4;
  for (int v = threadIdx.x; v < 16 * P / 4; v += NT) {
    const int r = v / (P / 4), c = (v % (P / 4)) * 4;
    const int i = i0 + r;
    *(v4f*)(Xi + r * RS + c) = i < N ? *(const v4f*)(X + (int64_t)i * ld + c) : v4f{0.f, 0.f, 0.f, 0.f};
  }
}

// 16x16 dot tile D[j = 4(lane>>4) + reg][i = lane&15] = Y_j . X_i; yrow: the
// lane's row j = jb + (lane&15) of Y (clamped by the caller) + 4(lane>>4); xi:
// the lane's row of the LDS image + 4(lane>>4). Every global load of the Y row
// is issued before the first MFMA. The statistics pass and the gradient pass
// call this, so both get the same bits.
template <int NB>
__device__ __forceinline__ v4f yx_tile(const float* yrow, const float* xi) {
  v4f y[4 * NB];
#pragma unroll
  for (int b = 0; b < 4 * NB; ++b) y[b] = *(const v4f*)(yrow + 16 * b);
  return dot_tile<4 * NB>(y, xi);
}

// ------------------------------------------------------------------ stats
// grid (16-row blocks of N, Js, 2 roles)
template <int NB>
__global__ void __launch_bounds__(NT) con_stats_kernel(const ConK a) {
  constexpr int P = 64 * NB, RS = P + 4;
  __shared__ __attribute__((aligned(16))) float Xi[16 * RS];
  __shared__ float ms[NW][16][2];
  const int lane = threadIdx.x & 63, g = lane >> 4, il = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int role = blockIdx.z, N = a.N;
  const int i0 = 16 * (int)blockIdx.x;
  const float* Y = a.X[1 - role];
  const int64_t ldY = a.ld[1 - role];
  stage_rows<NB>(a.X[role], a.ld[role], i0, N, Xi);
  __syncthreads();
  const float itau = 1.f / call_tau(a);
  const int njt = (N + 15) / 16;
  const int jt0 = (int)blockIdx.y * a.nrep, jt1 = min(jt0 + a.nrep, njt);
  const int i = i0 + il;
  float m0 = NEG, s0 = 0.f;
  for (int jt = jt0 + w; jt < jt1; jt += NW) {
    const int jb = 16 * jt;
    const v4f d = yx_tile<NB>(Y + (int64_t)min(jb + il, N - 1) * ldY + 4 * g, Xi + il * RS + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = jb + 4 * g + r;
      const float l = fmaf(d[r], itau, 0.f);
      if (j < N) merge_ms(m0, s0, l, 1.f);
      if (role == 0 && j == i && i < N) a.diag[i] = l;
    }
  }
  float m2 = __shfl_xor(m0, 16, 64), s2 = __shfl_xor(s0, 16, 64);
  merge_ms(m0, s0, m2, s2);
  m2 = __shfl_xor(m0, 32, 64);
  s2 = __shfl_xor(s0, 32, 64);
  merge_ms(m0, s0, m2, s2);
  if (g == 0) {
    ms[w][il][0] = m0;
    ms[w][il][1] = s0;
  }
  __syncthreads();
  if (threadIdx.x < 16 && i < N) {
    float m = ms[0][il][0], s = ms[0][il][1];
#pragma unroll
    for (int k = 1; k < NW; ++k) merge_ms(m, s, ms[k][il][0], ms[k][il][1]);
    *(v2f*)(a.part + (((int64_t)role * a.Js + blockIdx.y) * N + i) * 2) = v2f{m, s};
  }
}

// ------------------------------------------------------------------ combine
// one thread per row: (M, log z) of both roles from the j-split partials in
// split order, and the row's loss term ((lse_row - l_ii) + (lse_col - l_ii)) / 2N
__global__ void __launch_bounds__(NT) con_combine_kernel(const ConK a) {
  const int i = blockIdx.x * NT + threadIdx.x, N = a.N;
  if (i >= N) return;
  float M[2], lz[2];
#pragma unroll
  for (int role = 0; role < 2; ++role) {
    float m = NEG, z = 0.f;
    for (int js = 0; js < a.Js; ++js) {
      const v2f v = *(const v2f*)(a.part + (((int64_t)role * a.Js + js) * N + i) * 2);
      merge_ms(m, z, v[0], v[1]);
    }
    M[role] = m;
    lz[role] = logf(z);
    *(v2f*)(a.stat + ((int64_t)role * N + i) * 2) = v2f{m, lz[role]};
  }
  const float d = a.diag[i];
  a.rowterm[i] = (((M[0] - d) + lz[0]) + ((M[1] - d) + lz[1])) * (0.5f / (float)N);
}

// ------------------------------------------------------------------ grad
// grid (gradient row blocks + loss row blocks, P / PC, 2 roles); NC = PC / 16.
// Loss workgroups (SigLIP only) are those past the a.ngb gradient blocks; they
// exist for chunk 0, role 0.
template <int NB, int NC>
__global__ void __launch_bounds__(NT) con_grad_kernel(const ConK a, float* G0, int64_t ldg0, float* G1, int64_t ldg1) {
  constexpr int P = 64 * NB, RS = P + 4;
  __shared__ __attribute__((aligned(16))) float Xi[16 * RS];
  __shared__ __attribute__((aligned(16))) v4f accs[NW / 2][NC][64];
  __shared__ float red[3][NW][16];
  const int lane = threadIdx.x & 63, g = lane >> 4, il = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = a.N, role = blockIdx.z;
  const bool lossWG = (int)blockIdx.x >= a.ngb;   // workgroup-uniform
  if (lossWG && (blockIdx.y != 0 || blockIdx.z != 0)) return;
  const int i0 = lossWG ? 16 * ((int)blockIdx.x - a.ngb) : a.g0 + 16 * (int)blockIdx.x;
  const int iend = lossWG ? N : a.g0 + a.Ng;      // <= N
  const float* Y = a.X[1 - role];
  const int64_t ldY = a.ld[1 - role];
  stage_rows<NB>(a.X[role], a.ld[role], i0, N, Xi);
  __syncthreads();
  const float itau = 1.f / call_tau(a), b = call_scalar(a.bias);
  const bool sig = a.kind == 1;
  const int i = i0 + il;
  const bool iok = i < iend;
  const int irow = min(i, N - 1);
  float Am = 0.f, Alz = 0.f;
  if (!sig) {
    const v2f s = *(const v2f*)(a.stat + ((int64_t)role * N + irow) * 2);
    Am = s[0];
    Alz = s[1];
  }
  const float* Bst = a.stat + (int64_t)(1 - role) * N * 2;
  const float invn = (sig ? 1.f : 0.5f) / (float)N;
  const int pc = 16 * NC * (int)blockIdx.y;
  const int njt = (N + 15) / 16;
  v4f acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = v4f{0.f, 0.f, 0.f, 0.f};
  float lsum = 0.f, tsum = 0.f, usum = 0.f;
  for (int jt = w; jt < njt; jt += NW) {
    const int jb = 16 * jt;
    const v4f d = yx_tile<NB>(Y + (int64_t)min(jb + il, N - 1) * ldY + 4 * g, Xi + il * RS + 4 * g);
    float wv[4];
    const float* yc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = jb + 4 * g + r, jrow = min(j, N - 1);
      yc[r] = Y + (int64_t)jrow * ldY + pc + il;
      const float l = fmaf(d[r], itau, b);
      float dl;
      if (sig) {
        // x = z l; sigma(-x) and log sigma(x) from e = exp(-|x|) <= 1: no overflow
        const float x = j == i ? l : -l;
        const float e = expf(-fabsf(x));
        const float sg = (x >= 0.f ? e : 1.f) / (1.f + e);
        if (j < N && iok) lsum += log1pf(e) - fminf(x, 0.f);
        dl = (j == i ? -sg : sg) * invn;
      } else {
        const v2f bs = *(const v2f*)(Bst + (int64_t)jrow * 2);
        dl = (expf(lsub(l, Am, Alz)) + expf(lsub(l, bs[0], bs[1])) - (j == i ? 2.f : 0.f)) * invn;
      }
      dl = (j < N && iok) ? dl : 0.f;
      tsum = fmaf(dl, d[r] * itau, tsum);
      usum += dl;
      wv[r] = dl * itau;
    }
    if (!lossWG) {
      // G^T[p][i] += Y_j[p] w[j][i]: lane (il, g) carries Y[j = 4g + r][pc + 16c + il]
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float ya[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ya[r] = yc[r][16 * c];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[c] = mma4(ya[r], wv[r], acc[c]);
      }
    }
  }
  // per-row sums: the four 4-j groups of a row, then the waves in wave order
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  tsum += __shfl_xor(tsum, 16, 64);
  tsum += __shfl_xor(tsum, 32, 64);
  usum += __shfl_xor(usum, 16, 64);
  usum += __shfl_xor(usum, 32, 64);
  if (g == 0) {
    red[0][w][il] = lsum;
    red[1][w][il] = tsum;
    red[2][w][il] = usum;
  }
  if (!lossWG && w >= NW / 2) {
#pragma unroll
    for (int c = 0; c < NC; ++c) accs[w - NW / 2][c][lane] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const float ls = (red[0][0][il] + red[0][1][il]) + (red[0][2][il] + red[0][3][il]);
    const float ts = (red[1][0][il] + red[1][1][il]) + (red[1][2][il] + red[1][3][il]);
    const float us = (red[2][0][il] + red[2][1][il]) + (red[2][2][il] + red[2][3][il]);
    if (lossWG) {
      if (i < N) a.rowterm[i] = ls * invn;
    } else if (role == 0 && blockIdx.y == 0) {
      // the last block of a slice runs past it: those rows are no part of the sum
      a.dtrow[16 * (int)blockIdx.x + il] = iok ? -ts : 0.f;
      a.dbrow[16 * (int)blockIdx.x + il] = iok ? us : 0.f;
    }
  }
  if (lossWG) return;
  // (w0 + w2) + (w1 + w3)
  if (w < NW / 2) {
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += accs[w][c][lane];
  }
  __syncthreads();
  if (w == 1) {
#pragma unroll
    for (int c = 0; c < NC; ++c) accs[0][c][lane] = acc[c];
  }
  __syncthreads();
  if (w == 0 && iok) {
    // lane holds G^T[p = pc + 16c + 4g + r][i = il] -> row i, 4 consecutive p
    float* dst = (role == 0 ? G0 + (int64_t)(i - a.g0) * ldg0 : G1 + (int64_t)(i - a.g0) * ldg1) + pc + 4 * g;
#pragma unroll
    for (int c = 0; c < NC; ++c) *(v4f*)(dst + 16 * c) = acc[c] + accs[0][c][lane];
  }
}

// ------------------------------------------------------------------ reduce
// loss = sum of the N row terms (and their copy to row_loss), d theta and d b
// = sums of the per-row terms: one workgroup, in double and in a fixed order
// (strided per-lane sums, then a binary tree through LDS)
__global__ void __launch_bounds__(NT) con_reduce_kernel(const float* __restrict__ rowterm, int n, float* __restrict__ loss,
                                                        float* __restrict__ row_loss, const float* __restrict__ dtrow,
                                                        const float* __restrict__ dbrow, int nrows,
                                                        float* __restrict__ dth, float* __restrict__ db) {
  __shared__ double red[NT];
  for (int job = 0; job < 3; ++job) {
    const float* src = job == 0 ? rowterm : job == 1 ? dtrow : dbrow;
    float* out = job == 0 ? loss : job == 1 ? dth : db;
    const int cnt = job == 0 ? n : nrows;
    if (!out) continue;   // workgroup-uniform
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += NT) {
      s += (double)src[i];
      if (job == 0 && row_loss) row_loss[i] = src[i];
    }
    __syncthreads();
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)red[0];
  }
}

// ------------------------------------------------------------ geometry
int64_t up4(int64_t n) { return (n + 3) / 4 * 4; }

// stats: ~2048 workgroups over (16-row blocks) x (j-splits) x (2 roles), at
// least one j-tile per wave
void stats_geometry(int64_t N, int& nrep, int& Js) {
  const int64_t nb = (N + 15) / 16;
  int64_t want = (1024 + nb - 1) / nb;
  const int64_t most = (nb + NW - 1) / NW;
  if (want > most) want = most;
  if (want < 1) want = 1;
  nrep = (int)((nb + want - 1) / want);
  Js = (int)((nb + nrep - 1) / nrep);
}

struct Layout {
  size_t part, stat, diag, rowterm, dtrow, dbrow, total;   // in floats
};
Layout ws_layout(int64_t N, int64_t grad_rows, int kind) {
  int nrep = 0, Js = 0;
  if (kind == 0) stats_geometry(N, nrep, Js);
  const int64_t gb = 16 * ((grad_rows + 15) / 16);
  Layout l;
  l.part = 0;
  l.stat = l.part + (size_t)up4(2 * (int64_t)Js * N * 2);
  l.diag = l.stat + (size_t)(kind == 0 ? up4(4 * N) : 0);
  l.rowterm = l.diag + (size_t)(kind == 0 ? up4(N) : 0);
  l.dtrow = l.rowterm + (size_t)up4(N);
  l.dbrow = l.dtrow + (size_t)gb;
  l.total = l.dbrow + (size_t)gb + 4;
  return l;
}

template <int NB, int NC>
void launch_grad(const ConK& k, dim3 grid, hipStream_t s, const maeclip_contrastive_args& a) {
  const int64_t lddI = a.ld_dI ? a.ld_dI : a.P, lddT = a.ld_dT ? a.ld_dT : a.P;
  hipLaunchKernelGGL((con_grad_kernel<NB, NC>), grid, dim3(NT), 0, s, k, a.dI, lddI, a.dT, lddT);
}

template <int NB>
int run(const maeclip_contrastive_args& a, int64_t Ng, hipStream_t s) {
  const int64_t N = a.N;
  float* ws = (float*)a.workspace;
  const Layout l = ws_layout(N, Ng, a.kind);
  ConK k = {};
  k.X[0] = a.I;
  k.X[1] = a.T;
  k.ld[0] = a.ld_I ? a.ld_I : a.P;
  k.ld[1] = a.ld_T ? a.ld_T : a.P;
  k.N = (int)N;
  k.P = (int)a.P;
  k.kind = a.kind;
  k.tau = a.temperature;
  k.ltau = a.log_temperature;
  k.bias = a.logit_bias;
  k.part = ws + l.part;
  k.stat = ws + l.stat;
  k.diag = ws + l.diag;
  k.rowterm = ws + l.rowterm;
  k.dtrow = ws + l.dtrow;
  k.dbrow = ws + l.dbrow;
  k.g0 = Ng > 0 ? (int)a.grad_row0 : 0;
  k.Ng = (int)Ng;
  k.ngb = (int)((Ng + 15) / 16);
  const unsigned nb = (unsigned)((N + 15) / 16);
  if (a.kind == 0) {
    stats_geometry(N, k.nrep, k.Js);
    hipLaunchKernelGGL((con_stats_kernel<NB>), dim3(nb, k.Js, 2), dim3(NT), 0, s, k);
    MC_CHECK_LAUNCH("maeclip_contrastive_loss(stats)");
    hipLaunchKernelGGL(con_combine_kernel, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, s, k);
    MC_CHECK_LAUNCH("maeclip_contrastive_loss(combine)");
  }
  const unsigned gx = (unsigned)k.ngb + (a.kind == 1 ? nb : 0u);
  if (gx) {
    // wide chunks (the whole of P up to 256 columns; 128 at P = 512, whose X_i
    // image and wave sums would not fit 64 KB of LDS otherwise) unless they
    // leave most of the 256 CUs without a gradient workgroup; then 64-column chunks
    constexpr int WIDE = NB < 4 ? 4 * NB : NB == 4 ? 16 : 8;
    const bool narrow = WIDE > 4 && 2 * (int64_t)k.ngb * (4 * NB / WIDE) < 256;
    if (narrow) {
      launch_grad<NB, 4>(k, dim3(gx, NB, 2), s, a);
    } else {
      launch_grad<NB, WIDE>(k, dim3(gx, 4 * NB / WIDE, 2), s, a);
    }
    MC_CHECK_LAUNCH("maeclip_contrastive_loss(grad)");
  }
  hipLaunchKernelGGL(con_reduce_kernel, dim3(1), dim3(NT), 0, s, k.rowterm, (int)N, a.loss, a.row_loss_out, k.dtrow, k.dbrow,
                     16 * k.ngb, a.d_log_temperature, a.d_logit_bias);
  MC_CHECK_LAUNCH("maeclip_contrastive_loss(reduce)");
  return 0;
}

}  // namespace

extern "C" size_t maeclip_contrastive_workspace(int64_t N, int64_t P, int64_t grad_rows, int32_t kind) {
  (void)P;
  if (N <= 0 || N > MAX_N || grad_rows < 0 || grad_rows > N || (kind != 0 && kind != 1)) return 64 * sizeof(float);
  return ws_layout(N, grad_rows, kind).total * sizeof(float);
}

extern "C" int32_t maeclip_contrastive_loss(const maeclip_contrastive_args* a, void* stream) {
  MC_CHECK_ARG(a && a->I && a->T && a->loss && a->workspace, "maeclip_contrastive_loss: null pointer");
  MC_CHECK_ARG(a->kind == 0 || a->kind == 1, "maeclip_contrastive_loss: kind must be 0 (InfoNCE) or 1 (SigLIP) (got %d)",
               (int)a->kind);
  if (pair_check_shape(a, "maeclip_contrastive_loss", MAX_N)) return -1;
  MC_CHECK_ARG(a->kind == 1 || (!a->logit_bias && !a->d_logit_bias),
               "maeclip_contrastive_loss: logit_bias / d_logit_bias are SigLIP's (kind 1) only");
  MC_CHECK_ARG(((uintptr_t)a->log_temperature & 3) == 0 && ((uintptr_t)a->d_log_temperature & 3) == 0 &&
                   ((uintptr_t)a->logit_bias & 3) == 0 && ((uintptr_t)a->d_logit_bias & 3) == 0,
               "maeclip_contrastive_loss: log_temperature / logit_bias and their gradients must be 4-byte aligned");
  MC_CHECK_ARG(!a->d_log_temperature || (a->log_temperature && a->dI && a->dT),
               "maeclip_contrastive_loss: d_log_temperature needs log_temperature, dI and dT");
  MC_CHECK_ARG(!a->d_logit_bias || (a->dI && a->dT), "maeclip_contrastive_loss: d_logit_bias needs dI and dT");
  MC_CHECK_ARG(!a->dI == !a->dT, "maeclip_contrastive_loss: dI and dT come together");
  int64_t gr;
  if (pair_check_rows(a, "maeclip_contrastive_loss", true, &gr)) return -1;
  MC_CHECK_ARG(a->ws_bytes >= maeclip_contrastive_workspace(a->N, a->P, gr, a->kind) && ((uintptr_t)a->workspace & 15) == 0,
               "maeclip_contrastive_loss: workspace too small or misaligned");
  hipStream_t s = (hipStream_t)stream;
  switch (a->P) {
    case 64: return run<1>(*a, gr, s);
    case 128: return run<2>(*a, gr, s);
    case 256: return run<4>(*a, gr, s);
    default: return run<8>(*a, gr, s);
  }
}
