// Attention backward, one-pass diagonal schedule (bf16): maeclip::attn_diag,
// the route maeclip::AttnPath::BWD_DIAG of attention.hip.
#include "attention_common.h"

ATTN_STAMPS_BUFFER

namespace {

// ======================================================= backward, diagonal
// bf16, HD = 32 with npad <= 256 (the C2/C3 MAE decoder: n = 197) and HD = 64
// with npad <= 224 (the ViT encoders: C1 n = 197, C2 n = 50, C4 n = 145): one pass
// instead of two. Wave w owns key chunk w (32 keys, K/V fragments in
// registers) and in round r works query chunk c = (w + r) % NC, so in every
// round each query chunk is touched by exactly one wave. Per (key chunk, query
// chunk) block it computes S, dP, P, dS once, accumulates dK/dV in registers,
// transposes dS through a 2 KB per-wave LDS tile (ds_read_b64_tr_b16) and adds
// dQ^T = K^T dS^T into an fp32 dQ image in LDS (read-modify-write by the one
// wave that owns the chunk this round; a barrier ends the round). The order
// in which the waves add to a query chunk is fixed by the schedule, so the
// result is deterministic, and S / dP / exp are not recomputed for dQ.
// LDS: Q, dO images, L2 / Dv, dQ f32 [npad][HD] (16-B chunks XOR-swizzled by
// the row), NW dS tiles, bias partials: ~78 KB at n = 197, HD = 32 (two
// workgroups per CU); ~142 KB at HD = 64 (one).
// dQ image: HD f32 per row, 16-B chunk ^ (row & 7) (128-B rows) / (row & 15)
// (256-B rows): conflict-free b128 reads and writes of the (16 rows x 4
// chunks) tiles of one MFMA output
template <int HD> __device__ __forceinline__ int dq_off(int row, int c16) {
  return row * (4 * HD) + ((c16 ^ (row & (HD / 4 - 1))) << 4);
}
// dS tile [32 keys][32 q] bf16, 64-B rows, 8-B unit ^ F(row) with F linear in
// row bits 1..3 (found by tools/lds_bank_sim.py): conflict-free for both the
// ds_write_b64 of the MFMA output (row = key, unit = 4u + g) and the
// ds_read_b64_tr_b16 of the dQ B operand
__device__ __forceinline__ int dst_off(int row, int unit) {
  const int f = ((row >> 1) & 1) ^ (((row >> 2) & 1) << 2) ^ (((row >> 3) & 1) << 1);
  return row * 64 + ((unit ^ f) << 3);
}
// B operand dS^T[key][q] for keys 0..31 (permuted order of pack_p), q = c0 + (lane & 15)
__device__ __forceinline__ v8s dst_frag(const char* t, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  v8s r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    v4s x = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, t + dst_off(16 * h + 4 * g + q, (c0 >> 2) + p)));
#pragma unroll
    for (int e = 0; e < 4; ++e) r[4 * h + e] = x[e];
  }
  return r;
}

// 8 f32 -> the v8s bf16 operand (elements 0-3 from a, 4-7 from b), one
// v_cvt_pk_bf16_f32 per pair and no lane shuffles
__device__ __forceinline__ v8s pack8(const v4f& a, const v4f& b) {
  const v4u u = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
  return __builtin_bit_cast(v8s, u);
}

template <int HD>
__global__ void __launch_bounds__(MAXW * 64) __attribute__((amdgpu_waves_per_eu(HD == 32 ? 4 : 2)))
attn_bwd_diag_kernel(const maeclip_attn_args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KS = HD / 32, DT = HD / 16, CPR = HD / 8, ROWB = Img<bf16_t, HD>::ROWB, DQB = 4 * HD;
  using I = Img<bf16_t, HD>;
  const int n = a.n, H = a.H;
  const int bid = xcd_chunk_id(blockIdx.x, gridDim.x);
  const int b = bid / H, h = bid % H;
  const int npad = (n + 31) & ~31, NC = npad >> 5;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, l15 = lane & 15;
  const int img = npad * I::ROWB;
  char* Qi = smem;
  char* Di = smem + img;
  float* L2 = (float*)(smem + 2 * img);
  float* Dv = L2 + npad;
  char* dQi = (char*)(Dv + npad);                 // f32 [npad][HD]
  char* dst = dQi + npad * DQB;                   // NW x [32 keys][32 q] bf16
  float* csv = (float*)(dst + NW * 2048);         // [4 NW][HD] v-bias partials (one row per 16-lane row)
  float* csq = csv + 4 * NW * HD;                 // [4 NW][HD] q-bias partials
  char* myds = dst + wave * 2048;
  // rflag[w]: r + 2 once wave w's round-r dQ add is in. (HD 32 also had a
  // variant in which each wave filled and published its own 32-row chunk of the
  // images instead of the prologue barrier: decoder bwd 186.4 -> 191.8 us,
  // bitwise-identical; removed)
  int* rflag = (int*)(csq + 4 * NW * HD);
  if (threadIdx.x < NW) rflag[threadIdx.x] = 0;   // stale LDS of an earlier workgroup
  ASTAMP(0);

  const int HH = H * HD;
  const float c = a.scale * LOG2E;
  const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)b * n * a.ld_qkv;
  const bf16_t* O = (const bf16_t*)a.o + (int64_t)b * n * a.ld_o + h * HD;
  const bf16_t* dO = (const bf16_t*)a.dout + (int64_t)b * n * a.ld_o + h * HD;
  const float* lse = a.lse + ((int64_t)b * H + h) * n;

  // ---- prologue: every global load of the workgroup issued before the first
  // use (row indices clamped, out-of-range values selected to zero afterwards)
  // this wave's key chunk: K (scaled by c: S comes out in log2 units), V as
  // B-operand row fragments, K^T as the A operand of dQ^T in the permuted key
  // order of pack8 / dst_frag
  const int kbase = 32 * wave;
  v8s kf[2][KS], vf[2][KS], kT[DT];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = min(kbase + 16 * kt + l15, n - 1);
    const bf16_t* kr = qkv + (int64_t)key * a.ld_qkv + HH + h * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      kf[kt][ks] = ANT((const v8s*)(kr + 32 * ks));
      vf[kt][ks] = ANT((const v8s*)(kr + HH + 32 * ks));
    }
  }
  // Q, dO, O chunks: thread -> chunk slots tid + u NTH (CPR per row)
  constexpr int U = CPR / 2;   // npad CPR chunks over NTH = 2 npad threads
  auto prow = [&](int u) { return (int)(threadIdx.x + u * NTH) / CPR; };
  v4u vq[U], vd[U], vo[U];
  float ls[U];
  const int cc = threadIdx.x % CPR;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int row = prow(u), rc = min(row, n - 1);
    vq[u] = ANT((const v4u*)(qkv + (int64_t)rc * a.ld_qkv + h * HD + 8 * cc));
    vd[u] = ANT((const v4u*)(dO + (int64_t)rc * a.ld_o + 8 * cc));
    vo[u] = ANT((const v4u*)(O + (int64_t)rc * a.ld_o + 8 * cc));
    ls[u] = lse[rc];
  }
  if (HD == 32) {   // (HD = 64: the region first holds the K images for K^T, below)
    for (int i = threadIdx.x * 4; i < npad * HD; i += 4 * NTH) *(v4f*)(dQi + i * 4) = v4f{0.f, 0.f, 0.f, 0.f};
  }
  ASTAMP(6);
  float vs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // v-bias: column sums of dO
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int row = prow(u);
    const bool ok = row < n;
    const v4u z = {0, 0, 0, 0};
    const v4u q = ok ? vq[u] : z, d = ok ? vd[u] : z;
    *(v4u*)(Qi + I::chunk(row, cc)) = q;
    *(v4u*)(Di + I::chunk(row, cc)) = d;
    float dd = chunk_dot<bf16_t>(d, ok ? vo[u] : z);
    dd += dpp_mov<0xB1>(dd);   // the row's CPR chunks are one lane quad (HD 32) or two
    dd += dpp_mov<0x4E>(dd);
    if (CPR == 8) dd += dpp_mov<0x141>(dd);   // row_half_mirror: the other quad
    if (cc == 0) {
      Dv[row] = -dd;
      L2[row] = ok ? -ls[u] : -1.0e30f;   // S' = c S: the exponent is S' - lse2
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vs[2 * j] += __uint_as_float(d[j] << 16);
      vs[2 * j + 1] += __uint_as_float(d[j] & 0xffff0000u);
    }
  }
  // lanes cc, cc + CPR, ... of each 16-lane row: row_shr 4, 8 (DPP) leave the
  // row's sum for chunk cc in lane 16 - CPR + cc
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (CPR == 4) vs[j] += dpp_mov<0x114>(vs[j]);
    vs[j] += dpp_mov<0x118>(vs[j]);
  }
  // K^T (the A operand of dQ^T) through LDS: the wave's 32 K rows as a
  // [32][HD] image (padding keys zero), read back transposed -- instead of
  // 16 DT two-byte global loads per lane. HD 32: this wave's dS tile, free
  // until the first round; HD 64 (4 KB): the wave's slice of the dQ image,
  // zeroed afterwards
  char* kimg = HD == 32 ? myds : dQi + wave * 4096;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const bool kok = kbase + 16 * kt + l15 < n;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      *(v8s*)(kimg + I::chunk(16 * kt + l15, 4 * ks + g)) = kok ? kf[kt][ks] : v8s{0, 0, 0, 0, 0, 0, 0, 0};
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) kT[dt] = tr_frag<HD>(kimg, 0, 16 * dt, lane);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const bool kok = kbase + 16 * kt + l15 < n;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      v8s t;
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = kok ? (short)f2bf(c * bf2f((bf16_t)kf[kt][ks][j])) : (short)0;
      kf[kt][ks] = t;
      vf[kt][ks] = kok ? vf[kt][ks] : v8s{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  if (HD != 32) {
    __syncthreads();   // every wave has read its K^T back
    for (int i = threadIdx.x * 4; i < npad * HD; i += 4 * NTH) *(v4f*)(dQi + i * 4) = v4f{0.f, 0.f, 0.f, 0.f};
  }
  ASTAMP(7);
  __syncthreads();
  if (a.colsum_partial && (lane & 15) >= 16 - CPR)
#pragma unroll
    for (int j = 0; j < 8; ++j) csv[(4 * wave + (lane >> 4)) * HD + 8 * cc + j] = vs[j];
  ASTAMP(1);

  // per-lane LDS offsets; a round adds its query-chunk base (q0 is a multiple
  // of 32, so every swizzle below depends on the lane only)
  const int p_ = lane & 3;
  const int qq_ = (lane >> 2) & 3;
  int o_rf[KS];                                          // Q / dO row fragment, + 16 ROWB for u = 1
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) o_rf[ks] = I::chunk(l15, 4 * ks + g);
  int o_tr[DT];                                          // Q / dO transposed, + 16 ROWB for h = 1
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int unit = 4 * dt + p_;
    o_tr[dt] = I::chunk(4 * g + qq_, unit >> 1) + ((unit & 1) << 3);
  }
  int o_dq[DT];                                          // dQ f32, + 16 DQB for u = 1
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o_dq[dt] = dq_off<HD>(l15, 4 * dt + g);
  int o_sw[2], o_sr[2];                                  // dS tile write (+ 1024 kt = 1) / read (+ 1024 h = 1)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    o_sw[u] = dst_off(l15, 4 * u + g);
    o_sr[u] = dst_off(4 * g + qq_, 4 * u + p_);
  }

  v4f dv[2][DT], dk[2][DT];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dv[kt][dt] = v4f{0, 0, 0, 0}; dk[kt][dt] = v4f{0, 0, 0, 0}; }

  for (int r = 0; r < NC; ++r) {
    int qc = wave + r;
    qc = qc >= NC ? qc - NC : qc;
    const int q0 = qc * 32;
    const char* Qr = Qi + q0 * ROWB;
    const char* Dr = Di + q0 * ROWB;
    v8s qf[2][KS], df[2][KS];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qf[u][ks] = *(const v8s*)(Qr + o_rf[ks] + 16 * ROWB * u);
        df[u][ks] = *(const v8s*)(Dr + o_rf[ks] + 16 * ROWB * u);
      }
    // transposed Q / dO fragments (A operands of dK^T / dV^T): rows q0..q0+31
    v8s qT[DT], dT[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      v4s x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, Qr + o_tr[dt]));
      v4s x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, Qr + o_tr[dt] + 16 * ROWB));
      v4s y0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, Dr + o_tr[dt]));
      v4s y1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, Dr + o_tr[dt] + 16 * ROWB));
      qT[dt] = __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
      dT[dt] = __builtin_shufflevector(y0, y1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    v4f l2[2], dvr[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      l2[u] = *(const v4f*)(L2 + q0 + 16 * u + 4 * g);
      dvr[u] = *(const v4f*)(Dv + q0 + 16 * u + 4 * g);
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      v4f P[2], dS[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // S' - lse2 [q = 4g+i][key = lane&15] and dP - Dv, row constants as the
        // initial accumulators
        v4f s = l2[u], dp = dvr[u];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[u][ks], kf[kt][ks], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[u][ks], vf[kt][ks], dp, 0, 0, 0);
        }
        // P clamped to [0, 1] by the exp's output modifier (free): softmax
        // probabilities never exceed 1, and a padding key (zero K row: S' = 0,
        // P = 2^-lse2) can then never overflow into 0 * inf = NaN in dQ
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          P[u][i] = fminf(fmaxf(__builtin_amdgcn_exp2f(s[i]), 0.f), 1.f);
          dS[u][i] = P[u][i] * dp[i];
        }
        const v2u pk = {pack2bf(dS[u][0], dS[u][1]), pack2bf(dS[u][2], dS[u][3])};
        *(v2u*)(myds + o_sw[u] + 1024 * kt) = pk;
      }
      const v8s pp = pack8(P[0], P[1]), ps = pack8(dS[0], dS[1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dv[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dT[dt], pp, dv[kt][dt], 0, 0, 0);
        dk[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT[dt], ps, dk[kt][dt], 0, 0, 0);
      }
    }
    // dQ^T[d][q] += K^T[d][keys] dS^T[keys][q] for this wave's 32 keys.
    // Instead of a workgroup barrier per round, wave w waits
    // only for the wave that added into this query chunk in the round before
    // ((w + 1) mod NC, one LDS flag); every other phase of the round depends on
    // no other wave, so the waves drift apart by at most a round each and their
    // exp / MFMA / LDS phases interleave. The order of the adds per chunk (and
    // so the result) is the barrier schedule's. (The barrier per round was a
    // build switch: slower everywhere at HD 64, profiles/r03/attn_diag64_ab.txt; removed)
    if (r > 0) {
      const int src = wave + 1 == NW ? 0 : wave + 1;
      while (__hip_atomic_load(&rflag[src], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < r + 1)
        __builtin_amdgcn_s_sleep(1);
    }
    char* dQr = dQi + q0 * DQB;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      v4s x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, myds + o_sr[u]));
      v4s x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, myds + o_sr[u] + 1024));
      const v8s bds = __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        v4f* pq = (v4f*)(dQr + o_dq[dt] + 16 * DQB * u);
        *pq = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT[dt], bds, *pq, 0, 0, 0);
      }
    }
    __hip_atomic_store(&rflag[wave], r + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  ASTAMP(2);

  bf16_t* dqkv = (bf16_t*)a.dqkv + (int64_t)b * a.n * a.ld_dqkv;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = kbase + 16 * kt + l15;
    if (key < n) {
      bf16_t* rowp = dqkv + (int64_t)key * a.ld_dqkv + h * HD;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        st4<bf16_t>(rowp + HH + 16 * dt + 4 * g, dk[kt][dt] * a.scale);
        st4<bf16_t>(rowp + 2 * HH + 16 * dt + 4 * g, dv[kt][dt]);
      }
    }
  }
  ASTAMP(3);
  __syncthreads();   // every wave's last dQ update is in
  // dQ rows: thread -> (row, 4 columns); q-bias partial per (row group, column)
  float cq[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int C4N = HD / 4;   // 16-B chunks per dQ row
  const int c4 = threadIdx.x % C4N, rg = threadIdx.x / C4N, nrg = NTH / C4N;
  for (int row = rg; row < n; row += nrg) {
    const v4f v = *(const v4f*)(dQi + dq_off<HD>(row, c4)) * a.scale;
    st4<bf16_t>(dqkv + (int64_t)row * a.ld_dqkv + h * HD + 4 * c4, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) cq[i] += v[i];
  }
  ASTAMP(4);
  if (a.colsum_partial) {
    // reduce the row groups of a wave (lanes with equal c4) by shuffles, then
    // one partial row per wave in cs
    // HD 32: lanes c4 and c4 + 8 of each 16-lane row (row_shr 8): the row's
    // sum in lane 8 + c4; HD 64: a 16-lane row is one dQ row already
    if (HD == 32)
#pragma unroll
      for (int i = 0; i < 4; ++i) cq[i] += dpp_mov<0x118>(cq[i]);
    if ((lane & 15) >= (HD == 32 ? 8 : 0))
#pragma unroll
      for (int i = 0; i < 4; ++i) csq[(4 * wave + (lane >> 4)) * HD + 4 * c4 + i] = cq[i];
    __syncthreads();
    // q | k | v bias partials of this (sample, head); k is identically zero
    for (int i = threadIdx.x; i < 3 * HD; i += NTH) {
      const int part = i / HD, d = i % HD;
      float sum = 0.f;
      if (part != 1) {
        const float* src = part == 0 ? csq : csv;
        for (int w = 0; w < 4 * NW; ++w) sum += src[w * HD + d];
      }
      a.colsum_partial[(int64_t)b * 3 * HH + part * HH + h * HD + d] = sum;
    }
  }
  ASTAMP(5);
}

}  // namespace

namespace maeclip {
int attn_diag(const maeclip_attn_args& a, const AttnRoute& r, hipStream_t s) {
  const char* what = "maeclip_attn_bwd(diag)";
  return a.head_dim == 64 ? attn_launch(attn_bwd_diag_kernel<64>, what, a, r, s)
                          : attn_launch(attn_bwd_diag_kernel<32>, what, a, r, s);
}
#ifdef ATTN_STAMPS
int attn_diag_stamps(uint64_t* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_attn_stamps), sizeof(uint64_t) * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif
}  // namespace maeclip
