// Grouped weight gradients on the v4 body (maeclip_wgrad_grouped): the
// persistent RC x RC kernel, its two reduce kernels, the shape conditions and
// the entry points. Device code: gemm4_body.h; the launch plan of a chunk of
// problems: wgrad_plan (gemm4_plan.h).
#include "gemm4_body.h"

namespace {

// grouped weight gradients: RC x RC, fp32 out, no epilogue (beta only)
template <bool SPLIT>
__global__ void __launch_bounds__(512) wgrad4_kernel(const WgGroup grp) {
  maeclip_gemm_args a = {};
  a.alpha = 1.f;
  gemm4_body<LAY_RC, LAY_RC, float, EPI_NONE, SPLIT, true>(a, &grp);
}

// S slabs of every problem -> dW (fixed summation order)
__global__ void __launch_bounds__(256) wgrad4_reduce_kernel(const WgGroup grp) {
  const WgProb& q = grp.p[blockIdx.y];
  const int64_t NK = (int64_t)q.N * q.K;
  const float* ws = grp.ws + q.slab_off;
  for (int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; e < NK; e += (int64_t)gridDim.x * 1024) {
    v4f v = *(const v4f*)(ws + e);
    for (int s = 1; s < grp.S; ++s) v += *(const v4f*)(ws + s * NK + e);
    float* d = q.dw + e;
    if (grp.beta != 0.f) v += grp.beta * *(const v4f*)d;
    *(v4f*)d = v;
  }
}

// stream-K remainder tile blockIdx.x, element chunk blockIdx.y (of SKR_CHUNKS):
// the partial slots of the blocks that shared its K range, in block-position
// order (fixed summation order), + beta dW. Chunking the tile over SKR_CHUNKS
// workgroups keeps the reduce at HBM rate when only a few tiles are cut (the
// encoder's 16 remainder tiles each carry ~17 slots).
__global__ void __launch_bounds__(256) wgrad4_sk_reduce_kernel(const WgGroup grp) {
  const int r = blockIdx.x, NT = grp.NT, w = grp.skw;
  const int p0 = r * NT / w, p1 = ((r + 1) * NT - 1) / w;
  if (p0 == p1) return;   // one block ran the whole tile and wrote dW itself
  const int tile = grp.Tdp + r;
  int p = 0;
  while (p + 1 < grp.np && grp.p[p + 1].tile_begin <= tile) ++p;
  const WgProb& q = grp.p[p];
  const int local = tile - q.tile_begin, gnp = (q.K + 255) / 256;
  const int m0 = (local / gnp) * 256, n0 = (local % gnp) * 256;
  constexpr int CH = 65536 / SKR_CHUNKS;
  for (int e = blockIdx.y * CH + threadIdx.x * 4; e < (int)(blockIdx.y + 1) * CH; e += 1024) {
    const int m = m0 + (e >> 8), n = n0 + (e & 255);
    if (m >= q.N || n >= q.K) continue;   // K % 8 == 0: a 4-group is all in or all out
    v4f v = {0.f, 0.f, 0.f, 0.f};
    for (int c = p0; c <= p1; ++c) {
      const int slot = 2 * c + ((c * w) / NT == r ? 0 : 1);
      v += *(const v4f*)(grp.ws + (int64_t)slot * 65536 + e);
    }
    float* d = q.dw + (int64_t)m * q.K + n;
    if (grp.beta != 0.f) v += grp.beta * *(const v4f*)d;
    *(v4f*)d = v;
  }
}

bool wg_v4_ok(const maeclip_wgrad_problem* pr, int n, int64_t M, int32_t dtype) {
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (dtype != MAECLIP_BF16 || M <= 0 || M % 64 != 0 || M >= (1ll << 31)) return false;
  for (int i = 0; i < n; ++i) {
    const maeclip_wgrad_problem& q = pr[i];
    if (q.N < 256 || q.K < 256 || q.N % 8 || q.K % 8 || q.ldy % 8 || q.ldx % 8) return false;
    if (q.ldy < q.N || q.ldx < q.K) return false;
    if (!al16(q.dy) || !al16(q.x) || !al16(q.dw)) return false;
    if (M * q.ldy * 2 >= 0x7fffffffLL || M * q.ldx * 2 >= 0x7fffffffLL) return false;
  }
  return true;
}

}  // namespace

extern "C" int64_t maeclip_wgrad_grouped_workspace(const maeclip_wgrad_problem* probs, int32_t nprob, int64_t M,
                                                   int32_t dtype) {
  if (!probs || nprob <= 0 || !wg_v4_ok(probs, nprob, M, dtype)) return 0;
  const int ncu = maeclip::gemm4_device_ncu();
  int64_t ws = 0;
  for (int c = 0; c < nprob; c += WG_MAX)
    ws = std::max(ws, maeclip::wgrad_plan(probs + c, std::min(WG_MAX, nprob - c), M, ncu).workspace_bytes);
  return ws;
}

// The plan of the first chunk (at most WG_MAX problems) of a maeclip_wgrad_grouped
// call on ncu CUs (ncu <= 0: this device's, the only case that touches HIP).
// Returns 1 and fills out[10] = {T, S, skw, Tdp, NT, main grid, reduce kernel
// (0 none, 1 slabs, 2 stream-K remainder), its grid x, y, workspace bytes} when
// the grouped kernel takes the list, 0 when the call falls back to one
// maeclip_gemm per problem, -1 for a bad list.
extern "C" int32_t maeclip_wgrad_grouped_plan(const maeclip_wgrad_problem* probs, int32_t nprob, int64_t M,
                                              int32_t dtype, int32_t ncu, int64_t out[10]) {
  MC_CHECK_ARG(probs != nullptr && nprob > 0 && out != nullptr, "maeclip_wgrad_grouped_plan: bad problem list");
  if (!wg_v4_ok(probs, nprob, M, dtype)) return 0;
  if (ncu <= 0) ncu = maeclip::gemm4_device_ncu();
  const maeclip::WgradPlan p = maeclip::wgrad_plan(probs, std::min(WG_MAX, nprob), M, ncu);
  const int64_t v[10] = {p.T, p.S, p.skw, p.Tdp, p.NT, p.grid, p.reduce, p.rgx, p.rgy, p.workspace_bytes};
  std::copy(v, v + 10, out);
  return 1;
}

extern "C" int32_t maeclip_wgrad_grouped(const maeclip_wgrad_problem* probs, int32_t nprob, int64_t M, int32_t dtype,
                                         float beta, void* workspace, int64_t ws_bytes, void* stream) {
  MC_CHECK_ARG(probs != nullptr && nprob >= 0, "maeclip_wgrad_grouped: bad problem list");
  MC_CHECK_ARG(M >= 0, "maeclip_wgrad_grouped: bad token count");
  if (nprob == 0 || M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (!wg_v4_ok(probs, nprob, M, dtype)) {
    // shapes / dtypes outside the grouped kernel: one maeclip_gemm per problem
    for (int i = 0; i < nprob; ++i) {
      const maeclip_wgrad_problem& q = probs[i];
      maeclip_gemm_args a = {};
      a.A = q.dy;
      a.B = q.x;
      a.C = q.dw;
      a.M = q.N;
      a.N = q.K;
      a.K = M;
      a.lda = q.ldy;
      a.ldb = q.ldx;
      a.ldc = q.K;
      a.batch = 1;
      a.dtype = dtype;
      a.out_dtype = MAECLIP_F32;
      a.a_layout = LAY_RC;
      a.b_layout = LAY_RC;
      a.alpha = 1.f;
      a.beta = beta;
      a.splitk = 1;
      const int rc = maeclip_gemm(&a, stream);
      if (rc != 0) return rc;
    }
    return 0;
  }
  MC_CHECK_ARG(ws_bytes >= maeclip_wgrad_grouped_workspace(probs, nprob, M, dtype) &&
                   (ws_bytes == 0 || ((uintptr_t)workspace & 15) == 0),
               "maeclip_wgrad_grouped: workspace too small or misaligned");
  const int ncu = maeclip::gemm4_device_ncu();
  for (int c = 0; c < nprob; c += WG_MAX) {
    const int n = std::min(WG_MAX, nprob - c);
    const maeclip::WgradPlan p = maeclip::wgrad_plan(probs + c, n, M, ncu);
    WgGroup g = {};
    g.np = n;
    g.Mtok = (int)M;
    g.beta = beta;
    g.ws = (float*)workspace;
    g.T = p.T;
    g.S = p.S;
    g.skw = p.skw;
    g.Tdp = p.Tdp;
    g.NT = p.NT;
    for (int i = 0; i < n; ++i) {
      const maeclip_wgrad_problem& q = probs[c + i];
      WgProb& w = g.p[i];
      w.dy = (const bf16_t*)q.dy;
      w.x = (const bf16_t*)q.x;
      w.dw = q.dw;
      w.N = (int)q.N;
      w.K = (int)q.K;
      w.ldy = (int)q.ldy;
      w.ldx = (int)q.ldx;
      w.tile_begin = p.tile_begin[i];
      MC_CHECK_ARG(p.slab_off[i] < (1ll << 31), "maeclip_wgrad_grouped: workspace offsets exceed 2^31 floats");
      w.slab_off = (int)p.slab_off[i];
    }
    auto kern = p.S > 1 ? wgrad4_kernel<true> : wgrad4_kernel<false>;
    maeclip::allow_lds((const void*)kern, TileM<256>::LDS_ALL);
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(512), TileM<256>::LDS_ALL, s, g);
    MC_CHECK_LAUNCH(p.skw > 0 ? "maeclip_wgrad_grouped(stream-k)" : "maeclip_wgrad_grouped");
    if (p.reduce == maeclip::WG_REDUCE_STREAMK) {
      hipLaunchKernelGGL(wgrad4_sk_reduce_kernel, dim3(p.rgx, p.rgy), dim3(256), 0, s, g);
      MC_CHECK_LAUNCH("maeclip_wgrad_grouped(stream-k reduce)");
    } else if (p.reduce == maeclip::WG_REDUCE_SLABS) {
      hipLaunchKernelGGL(wgrad4_reduce_kernel, dim3(p.rgx, p.rgy), dim3(256), 0, s, g);
      MC_CHECK_LAUNCH("maeclip_wgrad_grouped(reduce)");
    }
  }
  return 0;
}
