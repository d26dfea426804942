// Retrieval evaluation: fused similarity + top-k (+ first label hit), the
// similarity matrix never written.
//   s_ij = sum_p q_ip g_jp   (fp32 in, exact-f32 MFMA: bitwise an f32 fma chain
//                             in a fixed k order, so a score's bits do not
//                             depend on the workgroup that computed it)
//   per query row: the k best (value descending, index ascending: the order of
//   maeclip_topk_rows), k <= 64.
// sim_topk_kernel: workgroup = 64 query rows (16 per wave, the query fragment
//   in registers: P / 4 VGPRs per lane) x one contiguous slice of the gallery.
//   Gallery rows arrive in 16-row tiles through LDS (loaded into registers one
//   tile ahead), shared by the four waves. A 16 x 16 score tile leaves lane
//   (i = lane & 15, g = lane >> 4) with the scores of query row i against
//   gallery rows 4g .. 4g + 3 of the tile. Each query row keeps an UNSORTED
//   candidate list of k (value, index) pairs in LDS and its worst pair (the
//   threshold) beside it; a score enters only if it ranks before the threshold,
//   replacing the worst pair, and the new worst is found by one scan of the
//   list. The four lanes of a row insert in lane order, one after the other
//   (wave-synchronous: a row's list belongs to one wave), so there are no
//   atomics; (value desc, index asc) is a total order, so the k best are
//   unique whatever the insertion order. Gallery rows past the slice are
//   masked by index. At the end each row's list is ranked by counting and
//   written in order: to vals / idx (one slice), or to the workspace.
// sim_topk_merge_kernel (slices > 1): workgroup = one query row. A wave merges
//   up to 63 sorted slice lists with its running list: lane l is the cursor of
//   list l, k rounds of a wave arg-best over the 64 heads. Chunks of 63 lists
//   are dealt to the four waves and wave 0 merges the four results. The same
//   total order, so the result does not depend on the slice count.
// first_hit (labels given): smallest t with g_label[idx[q][t]] == q_label[q],
//   else k; written by whichever kernel writes the final list.
// The dot tile and its MFMA k mapping are simtile.h's, shared with
// clip_loss.hip and contrastive.hip.
#include "simtile.h"
#include "../../include/maeclip.h"

namespace {
constexpr int NT = 256;
constexpr int QB = 64;          // query rows per workgroup
constexpr int GT = 16;          // gallery rows per tile
constexpr int KMAX = 64;
constexpr int ML = 64;          // lists a wave merges at once (its running list included)
constexpr int CUS = 256;        // workgroups that fill the chip (MI355X)
constexpr int SENT = 0x7fffffff;   // index of an empty list slot: ranks after every real pair

typedef float v4fu __attribute__((ext_vector_type(4), aligned(4)));   // rows at any float offset / stride

struct SimK {
  const float* q;
  const float* g;
  int64_t ldq, ldg, Q, N;
  int P, k, ks;          // ks: row stride of a list in LDS (odd: the rows of a wave on distinct banks)
  int S, T;              // slices, 16-row gallery tiles; slice s = tiles [s T / S, (s + 1) T / S)
  float* vals;
  int64_t* idx;
  float* wv;             // workspace [S][Q][k]
  int64_t* wi;
  const int64_t* ql;
  const int64_t* gl;
  int32_t* fh;
};

// is (v, i) ranked before (bv, bi)?  value descending, index ascending
__device__ __forceinline__ bool before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__host__ __device__ __forceinline__ int slice_tile0(int s, int S, int T) { return (int)((int64_t)s * T / S); }
// candidates slice s leaves: min(k, its rows)
__device__ __forceinline__ int slice_count(const SimK& a, int s) {
  const int64_t j0 = (int64_t)GT * slice_tile0(s, a.S, a.T);
  const int64_t j1 = min((int64_t)GT * slice_tile0(s + 1, a.S, a.T), a.N);
  return (int)min((int64_t)a.k, j1 - j0);
}

// the LDS writes of the lanes before this point are seen by the lanes after it
// (one wave; LDS operations of a wave complete in order)
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int CTRL> __device__ __forceinline__ int dpp_movi(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ void best_step(float& v, int& i) {
  const float ov = dpp_mov<CTRL>(v);
  const int oi = dpp_movi<CTRL>(i);
  if (before(ov, oi, v, i)) {
    v = ov;
    i = oi;
  }
}
// the best pair of the wave, in every lane (DPP within the 16-lane rows, then
// the four row results through v_readlane)
__device__ __forceinline__ void wave_best(float& v, int& i) {
  best_step<0xB1>(v, i);
  best_step<0x4E>(v, i);
  best_step<0x141>(v, i);
  best_step<0x140>(v, i);
  float bv = lane_f(v, 0);
  int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int l = 16; l < 64; l += 16) {
    const float ov = lane_f(v, l);
    const int oi = __builtin_amdgcn_readlane(i, l);
    if (before(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  v = bv;
  i = bi;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// the thread's 16-B pieces of a 16-row gallery tile (zero for rows at or past jend)
template <int NV> struct GStage {
  static constexpr int U = NV / 4;   // GT * (16 NV / 4) vectors over NT threads
  v4f val[U];
  __device__ __forceinline__ void load(const SimK& a, int64_t jb, int64_t jend) {
    const int pv = a.P / 4;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = threadIdx.x + u * NT;
      const int r = v / pv, c = (v - r * pv) * 4;
      const int64_t j = jb + r;
      val[u] = (r < GT && j < jend) ? (v4f) * (const v4fu*)(a.g + j * a.ldg + c) : v4f{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void store(const SimK& a, float* Gt) const {
    const int pv = a.P / 4, RS = a.P + 4;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = threadIdx.x + u * NT;
      const int r = v / pv, c = (v - r * pv) * 4;
      if (r < GT) *(v4f*)(Gt + r * RS + c) = val[u];
    }
  }
};

// (v, j) replaces the worst pair (slot wp) of the row's list; the new worst
// (wv, wi, wp) by one scan (8 independent reads at a time; slots past k - 1
// re-read k - 1). The caller writes the threshold back.
__device__ __forceinline__ void list_insert(float* rv, int* ri, int k, float v, int j, float& wv, int& wi, int& wp) {
  rv[wp] = v;
  ri[wp] = j;
  wv = v;
  wi = j;
  for (int t0 = 0; t0 < k; t0 += 8) {
    float ev[8];
    int ei[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = min(t0 + u, k - 1);
      ev[u] = rv[t];
      ei[u] = ri[t];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (before(wv, wi, ev[u], ei[u])) {
        wv = ev[u];
        wi = ei[u];
        wp = min(t0 + u, k - 1);
      }
  }
}

// NV: 16-float k-groups held per lane (P <= 16 NV)
template <int NV>
__global__ void __launch_bounds__(NT) sim_topk_kernel(const SimK a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int P = a.P, RS = P + 4, k = a.k, ks = a.ks, nv = P / 16;
  float* Gt = smem;                    // [16][P + 4]
  float* lv = Gt + GT * RS;            // [64][ks]
  int* li = (int*)(lv + QB * ks);      // [64][ks]
  float* tv = (float*)(li + QB * ks);  // [64] threshold value, index, slot
  int* ti = (int*)(tv + QB);
  int* tp = ti + QB;
  const int lane = threadIdx.x & 63, g = lane >> 4, il = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q0 = (int64_t)QB * blockIdx.x;
  const int s = blockIdx.y;
  const int jt0 = slice_tile0(s, a.S, a.T), jt1 = slice_tile0(s + 1, a.S, a.T);
  const int64_t jend = min((int64_t)GT * jt1, a.N);
  const int rowl = 16 * w + il;
  const bool rowok = q0 + rowl < a.Q;
  const bool wave_on = q0 + 16 * w < a.Q;   // waves with no query row only move tiles

  // query fragment: row i = lane & 15, 16-B vector b at k = 16 b + 4 (lane >> 4)
  v4f qr[NV];
  {
    const float* row = a.q + (rowok ? q0 + rowl : 0) * a.ldq + 4 * g;
#pragma unroll
    for (int b = 0; b < NV; ++b)
      qr[b] = (rowok && b < nv) ? (v4f) * (const v4fu*)(row + 16 * b) : v4f{0.f, 0.f, 0.f, 0.f};
  }
  // empty lists: every slot (-inf, SENT), the worst is slot 0
  for (int t = lane; t < 16 * ks; t += 64) {
    lv[16 * w * ks + t] = -INFINITY;
    li[16 * w * ks + t] = SENT;
  }
  if (lane < 16) {
    tv[16 * w + lane] = -INFINITY;
    ti[16 * w + lane] = SENT;
    tp[16 * w + lane] = 0;
  }

  GStage<NV> st;
  st.load(a, (int64_t)GT * jt0, jend);
  for (int jt = jt0; jt < jt1; ++jt) {
    __syncthreads();   // the previous tile's LDS reads are done
    st.store(a, Gt);
    __syncthreads();
    if (jt + 1 < jt1) st.load(a, (int64_t)GT * (jt + 1), jend);
    if (!wave_on) continue;
    // 16 x 16 scores of the tile: D[j = 4 g + reg][i = lane & 15]; P < 16 NV
    // takes the k-groups below nv alone
    const float* rowp = Gt + il * RS + 4 * g;
    const v4f d = nv == NV ? dot_tile<NV>(rowp, qr) : dot_tile<NV>(rowp, qr, nv);
    const int64_t jb = (int64_t)GT * jt + 4 * g;
    float thv = tv[rowl];
    int thi = ti[rowl];
    bool any = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) any |= rowok && jb + r < jend && before(d[r], (int)(jb + r), thv, thi);
    if (__ballot(any) == 0) continue;   // wave-uniform
    // the four lanes of a row, in lane order
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      if (__ballot(any && g == gg) != 0) {
        if (any && g == gg) {
          float wv = tv[rowl];
          int wi = ti[rowl], wp = tp[rowl];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = (int)(jb + r);
            if (jb + r < jend && before(d[r], j, wv, wi))
              list_insert(lv + rowl * ks, li + rowl * ks, k, d[r], j, wv, wi, wp);
          }
          tv[rowl] = wv;
          ti[rowl] = wi;
          tp[rowl] = wp;
        }
        wave_sync_lds();
      }
    }
  }
  if (!wave_on) return;
  wave_sync_lds();
  // rank each row's list by counting (lane t: slot t) and write it in order
  const int cnt = (int)min((int64_t)k, jend - (int64_t)GT * jt0);
  for (int rr = 0; rr < 16; ++rr) {
    const int64_t qrow = q0 + 16 * w + rr;
    if (qrow >= a.Q) break;
    const float* rv = lv + (16 * w + rr) * ks;
    const int* ri = li + (16 * w + rr) * ks;
    const bool have = lane < k;
    const float ev = have ? rv[lane] : -INFINITY;
    const int ei = have ? ri[lane] : SENT;
    int rank = 0;
    for (int u = 0; u < k; ++u) rank += before(rv[u], ri[u], ev, ei) ? 1 : 0;
    const bool real = ei != SENT && rank < cnt;
    if (a.S == 1) {
      if (real) {
        a.vals[qrow * k + rank] = ev;
        a.idx[qrow * k + rank] = ei;
      }
      if (a.fh) {
        const bool hit = real && a.gl[ei] == a.ql[qrow];
        const int f = wave_min_i(hit ? rank : k);
        if (lane == 0) a.fh[qrow] = f;
      }
    } else if (real) {
      const int64_t o = ((int64_t)s * a.Q + qrow) * k + rank;
      a.wv[o] = ev;
      a.wi[o] = ei;
    }
  }
}

// One merge of up to 64 sorted lists, lane l the cursor of the list at (mv, mi)
// with n entries: the first min(k, total) pairs in order, pair t in lane t.
__device__ __forceinline__ int merge_lists(const float* mv, const int* mi, int n, int k, int lane, float& rv, int& ri) {
  int ptr = 0;
  float hv = n > 0 ? mv[0] : -INFINITY;
  int hi = n > 0 ? mi[0] : SENT;
  int rc = 0;
  rv = -INFINITY;
  ri = SENT;
  for (int t = 0; t < k; ++t) {
    float bv = hv;
    int bi = hi;
    wave_best(bv, bi);
    if (bi == SENT) break;   // every list is used up (wave-uniform)
    if (lane == t) {
      rv = bv;
      ri = bi;
    }
    ++rc;
    if (hi == bi) {   // indices are distinct: one winner
      ++ptr;
      hv = ptr < n ? mv[ptr] : -INFINITY;
      hi = ptr < n ? mi[ptr] : SENT;
    }
  }
  return rc;
}

__global__ void __launch_bounds__(NT) sim_topk_merge_kernel(const SimK a, int lw) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int wcnt[4];
  const int k = a.k, ks = a.ks;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = blockIdx.x;
  float* mv = smem + (size_t)w * lw * ks * 2;   // [lw][ks] values, then [lw][ks] indices
  int* mi = (int*)(mv + lw * ks);
  const int ch = lw - 1;   // slice lists per chunk; list 0 is the running list
  float rv = -INFINITY;
  int ri = SENT, rc = 0;
  for (int c = w; c * ch < a.S; c += 4) {
    const int s0 = c * ch, ns = min(ch, a.S - s0);
    wave_sync_lds();   // the previous chunk's reads are done
    if (lane < rc) {
      mv[lane] = rv;
      mi[lane] = ri;
    }
    for (int l = 0; l < ns; ++l) {
      if (lane < slice_count(a, s0 + l)) {
        const int64_t o = ((int64_t)(s0 + l) * a.Q + q) * k + lane;
        mv[(1 + l) * ks + lane] = a.wv[o];
        mi[(1 + l) * ks + lane] = (int)a.wi[o];
      }
    }
    wave_sync_lds();
    const int n = lane == 0 ? rc : (lane <= ns ? slice_count(a, s0 + lane - 1) : 0);
    const int l = lane <= ns ? lane : 0;
    rc = merge_lists(mv + l * ks, mi + l * ks, n, k, lane, rv, ri);
  }
  // the four waves' lists -> wave 0
  wave_sync_lds();
  if (lane < rc) {
    mv[lane] = rv;
    mi[lane] = ri;
  }
  if (lane == 0) wcnt[w] = rc;
  __syncthreads();
  if (w != 0) return;
  {
    const int l = lane < 4 ? lane : 0;
    const int n = lane < 4 ? wcnt[l] : 0;
    const float* ov = smem + (size_t)l * lw * ks * 2;
    rc = merge_lists(ov, (const int*)(ov + lw * ks), n, k, lane, rv, ri);
  }
  const bool have = lane < rc;   // rc == k: the slices cover N >= k rows
  if (have) {
    a.vals[q * k + lane] = rv;
    a.idx[q * k + lane] = ri;
  }
  if (a.fh) {
    const bool hit = have && a.gl[ri] == a.ql[q];
    const unsigned long long m = __ballot(hit);
    if (lane == 0) a.fh[q] = m ? __builtin_ctzll(m) : k;
  }
}

// shape checks shared by the three entry points; the slice count on success
int plan_splits(const char* who, int64_t Q, int64_t N, int64_t P, int32_t k, int32_t splits) {
  MC_CHECK_ARG(Q >= 0 && N >= 1 && N <= 0x7fffff00LL, "%s: need Q >= 0 and 1 <= N < 2^31 - 256, got Q=%lld N=%lld", who,
               (long long)Q, (long long)N);
  MC_CHECK_ARG(P >= 16 && P <= 512 && P % 16 == 0, "%s: need P %% 16 == 0, 16 <= P <= 512, got P=%lld", who,
               (long long)P);
  MC_CHECK_ARG(k >= 1 && k <= KMAX && k <= N, "%s: need 1 <= k <= min(N, 64), got k=%d (N=%lld)", who, k,
               (long long)N);
  MC_CHECK_ARG(splits >= 0, "%s: splits must be >= 0, got %d", who, splits);
  const int64_t T = (N + GT - 1) / GT;
  int64_t want = splits;
  if (splits == 0) {
    // enough workgroups to fill the chip, slices of at least 4 tiles
    const int64_t nq = Q > 0 ? (Q + QB - 1) / QB : 1;
    want = nq >= CUS ? 1 : (CUS + nq - 1) / nq;
    if (want > T / 4) want = T / 4 > 0 ? T / 4 : 1;
  }
  return (int)(want < T ? want : T);
}

size_t main_lds(int P, int ks) { return ((size_t)GT * (P + 4) + (size_t)QB * ks * 2 + QB * 3) * 4; }

template <int NV> void launch_main(const SimK& a, dim3 grid, size_t lds, hipStream_t s) {
  maeclip::allow_lds((const void*)sim_topk_kernel<NV>, (int)lds);
  hipLaunchKernelGGL(sim_topk_kernel<NV>, grid, dim3(NT), lds, s, a);
}
}  // namespace

extern "C" int32_t maeclip_sim_topk_splits(int64_t Q, int64_t N, int64_t P, int32_t k, int32_t splits) {
  return plan_splits("maeclip_sim_topk_splits", Q, N, P, k, splits);
}

extern "C" int64_t maeclip_sim_topk_workspace(int64_t Q, int64_t N, int64_t P, int32_t k, int32_t splits) {
  const int S = plan_splits("maeclip_sim_topk_workspace", Q, N, P, k, splits);
  if (S < 0) return S;
  return S == 1 ? 0 : (int64_t)S * Q * k * 12;
}

extern "C" int32_t maeclip_sim_topk(const float* q, const float* g, int64_t Q, int64_t N, int64_t P, int64_t ldq,
                                    int64_t ldg, int32_t k, int32_t splits, float* vals, int64_t* idx,
                                    const int64_t* q_label, const int64_t* g_label, int32_t* first_hit, void* ws,
                                    int64_t ws_bytes, void* stream) {
  const int S = plan_splits("maeclip_sim_topk", Q, N, P, k, splits);
  if (S < 0) return S;
  MC_CHECK_ARG(q && g && vals && idx, "maeclip_sim_topk: null q, g, vals or idx");
  MC_CHECK_ARG(ldq >= P && ldg >= P, "maeclip_sim_topk: need ldq, ldg >= P, got ldq=%lld ldg=%lld P=%lld",
               (long long)ldq, (long long)ldg, (long long)P);
  MC_CHECK_ARG((q_label != nullptr) == (g_label != nullptr),
               "maeclip_sim_topk: q_label and g_label must be given together");
  MC_CHECK_ARG((q_label != nullptr) == (first_hit != nullptr),
               "maeclip_sim_topk: labels and first_hit must be given together");
  MC_CHECK_ARG(Q <= (int64_t)0x7fffffff * QB, "maeclip_sim_topk: Q=%lld too large", (long long)Q);
  const int64_t need = S == 1 ? 0 : (int64_t)S * Q * k * 12;
  MC_CHECK_ARG(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0),
               "maeclip_sim_topk: workspace of %lld bytes (8-byte aligned) needed for %d splits, got %lld",
               (long long)need, S, (long long)ws_bytes);
  if (Q == 0) return 0;
  SimK a;
  a.q = q;
  a.g = g;
  a.ldq = ldq;
  a.ldg = ldg;
  a.Q = Q;
  a.N = N;
  a.P = (int)P;
  a.k = k;
  a.ks = k | 1;
  a.S = S;
  a.T = (int)((N + GT - 1) / GT);
  a.vals = vals;
  a.idx = idx;
  a.wi = (int64_t*)ws;   // [S][Q][k] indices, then the values
  a.wv = S == 1 ? nullptr : (float*)((int64_t*)ws + (int64_t)S * Q * k);
  a.ql = q_label;
  a.gl = g_label;
  a.fh = first_hit;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((Q + QB - 1) / QB), (unsigned)S);
  const size_t lds = main_lds(a.P, a.ks);
  if (P <= 64)
    launch_main<4>(a, grid, lds, s);
  else if (P <= 128)
    launch_main<8>(a, grid, lds, s);
  else if (P <= 256)
    launch_main<16>(a, grid, lds, s);
  else
    launch_main<32>(a, grid, lds, s);
  MC_CHECK_LAUNCH("maeclip_sim_topk");
  if (S > 1) {
    const int lw = S + 1 < ML ? S + 1 : ML;
    const size_t mlds = (size_t)4 * lw * a.ks * 2 * 4;
    maeclip::allow_lds((const void*)sim_topk_merge_kernel, (int)mlds);
    hipLaunchKernelGGL(sim_topk_merge_kernel, dim3((unsigned)Q), dim3(NT), mlds, s, a, lw);
    MC_CHECK_LAUNCH("maeclip_sim_topk(merge)");
  }
  return 0;
}
