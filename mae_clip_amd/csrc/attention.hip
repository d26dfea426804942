// Multi-head attention forward/backward (gfx950 MFMA).
//
// Replaces F.scaled_dot_product_attention inside timm's Attention (ViT encoder
// blocks, timm 0.9.12), HF ViTMAE decoder layers (modeling_vit_mae.py:455-580)
// and DistilBERT's self-attention with additive key-padding mask
// (modeling_distilbert.py:125-145, 174-205).
//
// Input is the fused qkv activation [B*n, ld_qkv] (token rows; q at column
// h*HD, k at H*HD + h*HD, v at 2*H*HD + h*HD) exactly as the qkv GEMM wrote
// it, so no permute/copy kernels sit between the GEMM and attention.
//
// Resident kernels: one workgroup (8 waves) owns one (sample, head): the whole
// K/V (and for the backward Q/dO) slice of that head lives in LDS. That holds
// n <= 576 at HD=64 and n <= 1216 (forward) / 1152 (backward) at HD=32: ViT-B
// 197/50, decoder 197/577 at HD=32, text 25. Beyond it (ViT-L/14@336 unmasked,
// n = 577 at HD=64) the bf16 streamed kernels take the call.
// Which file holds what:
//   attention_common.h   constants, LDS images and their fillers, MFMA fragment
//                        helpers, fwd_chunk, q8_store, the LDS footprints, the
//                        route types and the cross-file declarations
//   attention.hip        the argument checks, maeclip::attn_route (the whole
//                        choice of kernel, before any HIP call), the dispatcher,
//                        the entry points; the resident forward and the
//                        two-phase backward kernels
//   attention_diag.hip   the one-pass diagonal backward (maeclip::attn_diag)
//   attention_rows.hip   the fp32 rows kernels (maeclip::attn_rows)
//   attention_stream.h   the streamed bf16 kernels and their ring (maeclip::attn_stream);
//                        included at the end of this file: one translation unit
//                        with the resident kernels (see its header for why)
// The resident kernels:
//   forward : waves take 16-query tiles; S^T = K Q^T on MFMA (key on the
//             register axis, query on the lane) -> online softmax entirely
//             lane-local, P stays in registers and feeds P.V as the B operand;
//             V^T fragments come from ds_read_b64_tr_b16.
//   backward: phase 1 -- waves own 16-key tiles, sweep queries: S, dP, then
//             dV^T += dO^T P, dK^T += Q^T dS (accumulator-as-operand, no LDS
//             round trip). phase 2 -- waves own 16-query tiles, sweep keys:
//             S^T, dP^T, dQ^T += K^T dS^T. No atomics, deterministic.
// LDS images (bf16): [rows][HD] with 16-B chunk index XOR-swizzled by f(row)
// = row&6 (HD=64) or (row>>1)&2 (HD=32): conflict-free for both the
// ds_read_b128 row reads and the ds_read_b64_tr_b16 transposed reads
// (checked with tools/lds_bank_sim.py). fp32 parity mode uses padded rows and
// exact-f32 MFMA (v_mfma_f32_16x16x4_f32).
// Softmax statistics are kept in log2 units: lse2 = log2(sum 2^(s*scale*log2e)).
#include "attention_common.h"
#include <stdlib.h>

ATTN_STAMPS_BUFFER

namespace {

// Backward prologue: Q, K, V, dO images + Dv[q] = -rowsum(dO * O) (f32) +
// L2[q] = -lse / c (-1e30 on padding rows), all rows in one pass with every load of an iteration in flight.
// A row's CPR chunks sit on CPR consecutive lanes of one wave (CPR | 64, NTH a
// multiple of 64, total a multiple of 64), so the row sum is an xor-shuffle.
template <typename T, int HD, bool KV>
__device__ __forceinline__ void bwd_prologue(char* Qi, char* Ki, char* Vi, char* Di, float* L2, float* Dv,
                                             const T* q, const T* k, const T* v, int64_t ld_qkv, const T* O,
                                             const T* dO, int64_t ld_o, const float* lse, float inv_c, int n,
                                             int npad) {
  using I = Img<T, HD>;
  constexpr int CPR = I::CPR, EPC = 16 / (int)sizeof(T);
  const int total = npad * CPR;
  for (int id0 = threadIdx.x; id0 < total; id0 += 2 * NTH) {
    v4u vq[2], vk[2], vv[2], vd[2], vo[2];
    float ls[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int id = id0 + u * NTH;
      const int row = id / CPR, c = id % CPR;
      const bool ok = id < total && row < n;
      const int64_t oq = (int64_t)row * ld_qkv + c * EPC, oo = (int64_t)row * ld_o + c * EPC;
      const v4u z = {0, 0, 0, 0};
      vq[u] = ok ? ANT((const v4u*)(q + oq)) : z;
      if (KV) {
        vk[u] = ok ? ANT((const v4u*)(k + oq)) : z;
        vv[u] = ok ? ANT((const v4u*)(v + oq)) : z;
      }
      vd[u] = ok ? ANT((const v4u*)(dO + oo)) : z;
      vo[u] = ok ? ANT((const v4u*)(O + oo)) : z;
      ls[u] = (ok && c == 0) ? -lse[row] * inv_c : -1.0e30f;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int id = id0 + u * NTH;
      if (id >= total) break;  // wave-uniform
      const int row = id / CPR, c = id % CPR;
      *(v4u*)(Qi + I::chunk(row, c)) = vq[u];
      if (KV) {
        *(v4u*)(Ki + I::chunk(row, c)) = vk[u];
        *(v4u*)(Vi + I::chunk(row, c)) = vv[u];
      }
      *(v4u*)(Di + I::chunk(row, c)) = vd[u];
      float d = chunk_dot<T>(vd[u], vo[u]);
#pragma unroll
      for (int o = 1; o < CPR; o <<= 1) d += __shfl_xor(d, o, 64);
      if (c == 0) {
        Dv[row] = -d;
        L2[row] = ls[u];
      }
    }
  }
}

// WG = 16: up to 16 waves when the K / V images leave room for one workgroup
// per CU only (the C4 decoder, n = 577: 37 query tiles in 3 rounds of 13
// waves instead of 5 rounds of 8)
template <int A, int B> constexpr int cmax() { return A > B ? A : B; }
// Q8: the fp8-blocks copy of o (maeclip_attn_args q8) from the kernel's own
// stores -- its own instantiation, so the plain kernels keep their registers
// QI: Q as a third LDS image (fwd_qimg; bf16, 8-wave launches only)
template <typename T, int HD, bool DROP, int WG = MAXW, bool Q8 = false, bool QI = false>
__global__ void __launch_bounds__(WG * 64)
__attribute__((amdgpu_waves_per_eu(WG > MAXW ? cmax<fwd_wpe<T, HD, DROP>(), 4>() : fwd_wpe<T, HD, DROP>())))
attn_fwd_kernel(const maeclip_attn_args a) {
  static_assert(!QI || (std::is_same<T, bf16_t>::value && WG == MAXW), "QI: bf16, 8-wave launches");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using I = Img<T, HD>;
  const int n = a.n, H = a.H;
  const int bid = xcd_chunk_id(blockIdx.x, gridDim.x);
  const int b = bid / H, h = bid % H;
  const int npad = (n + 63) & ~63;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  ASTAMP(0);
  char* Kimg = smem;
  char* Vimg = smem + npad * I::ROWB;
  float* kmask = (float*)(smem + 2 * npad * I::ROWB);

  const T* qkv = (const T*)a.qkv + (int64_t)b * n * a.ld_qkv;
  const int HH = H * HD;
  // bf16: the Q rows come as a third LDS image with K and V when two
  // workgroups per CU still fit (fwd_qimg), so a query tile reads its Q
  // fragments from LDS instead of a global round trip per tile
  constexpr bool qimg = QI;
  char* Qimg = smem + 2 * npad * I::ROWB + npad * 4;
  if constexpr (qimg) {
    char* const dst[3] = {Kimg, Vimg, Qimg};
    const bf16_t* const src[3] = {(const bf16_t*)qkv + HH + h * HD, (const bf16_t*)qkv + 2 * HH + h * HD,
                                  (const bf16_t*)qkv + h * HD};
    dma_imgs<HD, 3>(dst, src, a.ld_qkv, n, npad);
  } else if constexpr (std::is_same<T, bf16_t>::value) {
    char* const dst[2] = {Kimg, Vimg};
    const bf16_t* const src[2] = {qkv + HH + h * HD, qkv + 2 * HH + h * HD};
    dma_imgs<HD, 2>(dst, src, a.ld_qkv, n, npad);
  } else {
    char* const dst[2] = {Kimg, Vimg};
    const T* const src[2] = {qkv + HH + h * HD, qkv + 2 * HH + h * HD};
    load_imgs<T, HD, 2>(dst, src, a.ld_qkv, n, npad);
  }
  for (int k = threadIdx.x; k < npad; k += NTH) {
    float mk = (k < n) ? 0.f : NEG_BIG;
    if (k < n && a.key_mask && a.key_mask[(int64_t)b * n + k] == 0.f) mk = NEG_BIG;
    kmask[k] = mk;
  }
  __syncthreads();
  ASTAMP(1);

  const float c = a.scale * LOG2E;
  FwdDrop dr{};
  if (DROP) {
    dr.seed = mc_step_seed(a.seed, a.step_ptr);
    dr.bh = (uint64_t)b * H + h;
    dr.thr = (uint32_t)((double)a.dropout_p * 4294967296.0);
    dr.scale = 1.f / (1.f - a.dropout_p);
  }
  // chunks whose 64 keys are all real and unmasked run the bias-free body
  const int nfull = a.key_mask ? 0 : n >> 6;

  const int nqt = (n + 15) >> 4;
  for (int qt = wave; qt < nqt; qt += NW) {
    const int q = qt * 16 + (lane & 15);
    const bool qok = q < n;
    RowFrag<T, HD> qf[HD / 32];
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
      if constexpr (qimg) qf[ks].lds(Qimg, qt * 16, ks, lane);
      else qf[ks].glob(qkv + (int64_t)q * a.ld_qkv + h * HD, ks, lane, qok);
    }

    float m = NEG_BIG, lsum = 0.f;
    v4f o[HD / 16], ol = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) o[dt] = v4f{0.f, 0.f, 0.f, 0.f};

    int kc = 0;
    for (; kc < 64 * nfull; kc += 64)
      fwd_chunk<T, HD, 4, false, DROP>(Kimg, Vimg, kmask, kc, qf, c, m, lsum, o, ol, lane, dr, q);
    for (; kc < npad; kc += 64) {
      // 16-key tiles of this chunk that hold real keys (wave-uniform; n > kc)
      const int rem = n - kc;
      if (rem > 48) fwd_chunk<T, HD, 4, true, DROP>(Kimg, Vimg, kmask, kc, qf, c, m, lsum, o, ol, lane, dr, q);
      else if (rem > 32) fwd_chunk<T, HD, 3, true, DROP>(Kimg, Vimg, kmask, kc, qf, c, m, lsum, o, ol, lane, dr, q);
      else if (rem > 16) fwd_chunk<T, HD, 2, true, DROP>(Kimg, Vimg, kmask, kc, qf, c, m, lsum, o, ol, lane, dr, q);
      else fwd_chunk<T, HD, 1, true, DROP>(Kimg, Vimg, kmask, kc, qf, c, m, lsum, o, ol, lane, dr, q);
    }
    // the MFMA row sum (bf16, no dropout) is whole in every lane of the query
    if (std::is_same<T, bf16_t>::value && !DROP) lsum = ol[0];
    else lsum = sum4rows(lsum);
    const float inv = 1.f / lsum;
    if constexpr (Q8 && std::is_same<T, bf16_t>::value) {
      {
        v4f ov[HD / 16];
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt) ov[dt] = o[dt] * inv;
        q8_store<HD>(a, (int64_t)b * n + q, qok, h * HD, HH, ov, lane);
      }
    }
    if (qok) {
      T* orow = (T*)a.o + ((int64_t)b * n + q) * a.ld_o + h * HD;
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt) st4<T>(orow + 16 * dt + 4 * g, o[dt] * inv);
      if (g == 0 && a.lse) a.lse[((int64_t)b * H + h) * n + q] = m + log2f(lsum);
    }
    if (qt == wave) ASTAMP(2);
  }
  ASTAMP(3);
}

// ============================================================== backward
// TWO_ (bf16; always on for fp32): two [npad][HD] images in LDS instead of four --
// phase 1 keeps Q, dO and reads each wave's K/V tile from HBM, phase 2 reloads
// the slots with K, V. Chosen when it fits more workgroups per CU (C4: decoder
// n = 577, encoder n = 145 at HD = 64).
// OCC > 1 asks the compiler for that many resident 8-wave workgroups per CU
// (register budget 512 / (2 OCC)); used with TWO_ at HD = 32, where the
// two-image LDS footprint would allow three.
// WG = 16: up to 16 waves in the one workgroup a CU holds (the C4 decoder,
// n = 577: 37 tiles, at most 3 per wave instead of 5; register budget 128).
// MASKED / DROP (the trainable DistilBERT tower; instantiations of their own,
// so the plain kernels keep their code and registers): key_mask zeroes P of
// masked and padding keys in both phases (kvm[] in LDS: 1 = valid key); DROP
// redraws the forward's keep mask M(q, k): dV = (M P sc)^T dO and
// dS = P (M sc dP - rowsum(dO O)), so the dP accumulator starts at 0 instead
// of -rowsum and the v-bias partial is the column sum of the dV tiles (rows
// of M P sc do not sum to 1); the k-bias partial stays identically zero.
template <typename T, int HD, bool TWO_ = false, int OCC = 1, int WG = MAXW, bool Q8 = false, bool MASKED = false,
          bool DROP = false>
__global__ void __launch_bounds__(WG * 64) __attribute__((amdgpu_waves_per_eu(WG > MAXW ? 4 : 2 * OCC)))
attn_bwd_kernel(const maeclip_attn_args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using I = Img<T, HD>;
  const int n = a.n, H = a.H;
  const int bid = xcd_chunk_id(blockIdx.x, gridDim.x);
  const int b = bid / H, h = bid % H;
  const int npad = (n + 31) & ~31;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  ASTAMP(0);
  // bf16: Q, K, V, dO images resident together. fp32 parity mode (rows twice
  // as wide) holds two at a time so that n = 197 at HD = 64 fits: phase 1
  // keeps Q, dO in LDS and reads each wave's K/V tile from HBM, phase 2
  // reloads the two slots with K, V and reads Q/dO tiles from HBM.
  constexpr bool TWO = TWO_ || !std::is_same<T, bf16_t>::value;
  const int img = npad * I::ROWB;
  char* Qi = smem;
  char* Di = smem + (TWO ? 1 : 3) * img;
  char* Ki = TWO ? smem : smem + img;
  char* Vi = TWO ? smem + img : smem + 2 * img;
  float* L2 = (float*)(smem + (TWO ? 2 : 4) * img);
  float* Dv = L2 + npad;
  float* cs = Dv + npad;  // [NW][3*HD] bias-grad partials
  float* kvm = cs + NW * 3 * HD;  // MASKED: [npad] 1 = valid key, 0 = masked / padding
  if constexpr (MASKED) {
    for (int k = threadIdx.x; k < npad; k += NTH)
      kvm[k] = (k < n && a.key_mask[(int64_t)b * n + k] != 0.f) ? 1.f : 0.f;
  }
  uint64_t dseed = 0, dbh = 0;
  uint32_t dthr = 0;
  float dsc = 1.f;
  if constexpr (DROP) {
    dseed = mc_step_seed(a.seed, a.step_ptr);
    dbh = (uint64_t)b * H + h;
    dthr = (uint32_t)((double)a.dropout_p * 4294967296.0);
    dsc = 1.f / (1.f - a.dropout_p);
  }

  const int HH = H * HD;
  const T* qkv = (const T*)a.qkv + (int64_t)b * n * a.ld_qkv;
  const T* O = (const T*)a.o + (int64_t)b * n * a.ld_o + h * HD;
  const T* dO = (const T*)a.dout + (int64_t)b * n * a.ld_o + h * HD;
  bwd_prologue<T, HD, !TWO>(Qi, Ki, Vi, Di, L2, Dv, qkv + h * HD, qkv + HH + h * HD, qkv + 2 * HH + h * HD, a.ld_qkv,
                            O, dO, a.ld_o, a.lse + ((int64_t)b * H + h) * n, 1.f / (a.scale * LOG2E), n, npad);
  for (int i = threadIdx.x; i < NW * 3 * HD; i += NTH) cs[i] = 0.f;
  const int nkt = (n + 15) >> 4;
  __syncthreads();
  ASTAMP(1);
  if (!DROP && a.colsum_partial && threadIdx.x < NW * HD) {
    // v-bias gradient: sum over keys of dV = sum over queries of dO (softmax
    // rows sum to 1, over the valid keys under a key mask; with dropout the
    // partial comes from the dV tiles of phase 1 instead). Row group
    // r0 of column d -> cs[r0][2 HD + d]; the k-bias gradient is identically
    // zero (softmax is invariant to a per-query constant) and stays 0.
    constexpr int EPC = 16 / (int)sizeof(T);
    const int d = threadIdx.x % HD, r0 = threadIdx.x / HD;
    float sv = 0.f;
    for (int r = r0; r < n; r += NW)
      sv += ld_as_f<T>((const T*)(Di + I::chunk(r, d / EPC) + (d % EPC) * (int)sizeof(T)));
    cs[r0 * 3 * HD + 2 * HD + d] = sv;
  }

  const float c = a.scale * LOG2E;
  T* dqkv = (T*)a.dqkv + (int64_t)b * n * a.ld_dqkv;

  // ---------------- phase 1: dK, dV (wave owns 16-key tiles)
  float cv[HD / 16][4];  // DROP: per-lane running sum of this wave's dV rows (v-bias gradient)
#pragma unroll
  for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) cv[dt][i] = 0.f;
  for (int kt = wave; kt < nkt; kt += NW) {
    const int k0 = kt * 16;
    const int key = k0 + (lane & 15);
    const bool kok = key < n;
    bool kvalid = true;
    if constexpr (MASKED) kvalid = kvm[key] != 0.f;
    RowFrag<T, HD> kf[HD / 32], vf[HD / 32];
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
      if (TWO) {
        const T* kr = qkv + (int64_t)(kok ? key : 0) * a.ld_qkv + HH + h * HD;
        kf[ks].glob(kr, ks, lane, kok);
        vf[ks].glob(kr + HH, ks, lane, kok);
      } else {
        kf[ks].lds(Ki, k0, ks, lane);
        vf[ks].lds(Vi, k0, ks, lane);
      }
    }
    v4f dv[HD / 16], dk[HD / 16];
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) { dv[dt] = v4f{0, 0, 0, 0}; dk[dt] = v4f{0, 0, 0, 0}; }

    for (int qc = 0; qc < npad; qc += 32) {
      v4f P[2], dS[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q0 = qc + 16 * u;
        // row constants as the initial accumulators: s' = S - lse/c, dp' = dP - Dv
        const v4f dvq = *(const v4f*)(Dv + q0 + 4 * g);
        v4f s = *(const v4f*)(L2 + q0 + 4 * g), dp = DROP ? v4f{0.f, 0.f, 0.f, 0.f} : dvq;
#pragma unroll
        for (int ks = 0; ks < HD / 32; ++ks) {
          RowFrag<T, HD> qf, df;
          qf.lds(Qi, q0, ks, lane);
          df.lds(Di, q0, ks, lane);
          s = mma32(qf, kf[ks], s);    // S[q=4g+i][key=lane&15]
          dp = mma32(df, vf[ks], dp);  // dP[q][key]
        }
        // padding keys (lane >= n) only pollute their own dK/dV columns, which
        // are never stored; padding queries have p = 0 (L2 = -1e30)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float p = __builtin_amdgcn_exp2f(s[i] * c);
          if constexpr (MASKED) p = kvalid ? p : 0.f;   // a select: exp2 of a masked key's score may overflow
          if constexpr (DROP) {
            const bool keep = dropout_keep(dseed, dbh, q0 + 4 * g + i, key, dthr);
            P[u][i] = keep ? p * dsc : 0.f;
            dS[u][i] = p * ((keep ? dp[i] * dsc : 0.f) + dvq[i]);
          } else {
            P[u][i] = p;
            dS[u][i] = p * dp[i];
          }
        }
      }
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt) {
        dv[dt] = mma_rowsum<T, HD>(Di, qc, 16 * dt, P[0], P[1], dv[dt], lane);
        dk[dt] = mma_rowsum<T, HD>(Qi, qc, 16 * dt, dS[0], dS[1], dk[dt], lane);
      }
    }
    // lane holds dV[key][16dt+4g+i], dK likewise
    if constexpr (Q8 && std::is_same<T, bf16_t>::value) {
      {
        v4f kv[HD / 16];
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt) kv[dt] = dk[dt] * a.scale;
        q8_store<HD>(a, (int64_t)b * n + key, kok, HH + h * HD, 3 * HH, kv, lane);
        q8_store<HD>(a, (int64_t)b * n + key, kok, 2 * HH + h * HD, 3 * HH, dv, lane);
      }
    }
    if (kok) {
      T* rowp = dqkv + (int64_t)key * a.ld_dqkv + h * HD;
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt) {
        st4<T>(rowp + HH + 16 * dt + 4 * g, dk[dt] * a.scale);
        st4<T>(rowp + 2 * HH + 16 * dt + 4 * g, dv[dt]);
      }
      if constexpr (DROP) {
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
          for (int i = 0; i < 4; ++i) cv[dt][i] += dv[dt][i];
      }
    }
  }
  if constexpr (DROP) {
    if (a.colsum_partial) {
      // v-bias gradient from the dV rows this wave computed (fixed order: the
      // wave's tiles, then the 16 key lanes, then the waves below)
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float sv = cv[dt][i];
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) sv += __shfl_xor(sv, o, 64);
          if ((lane & 15) == 0) cs[wave * 3 * HD + 2 * HD + 16 * dt + 4 * g + i] = sv;
        }
    }
  }

  ASTAMP(2);
  if (TWO) {
    // phase-1 reads of the Q / dO images are done: K, V take their slots
    __syncthreads();
    char* const dst[2] = {Ki, Vi};
    const T* const src[2] = {qkv + HH + h * HD, qkv + 2 * HH + h * HD};
    load_imgs<T, HD, 2>(dst, src, a.ld_qkv, n, npad);
    __syncthreads();
  }
  // ---------------- phase 2: dQ (wave owns 16-query tiles)
  ASTAMP(3);
  float cq[HD / 16][4];  // per-lane running sum of this wave's dQ rows (q-bias gradient)
#pragma unroll
  for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) cq[dt][i] = 0.f;
  for (int qt = wave; qt < nkt; qt += NW) {
    const int q0 = qt * 16;
    const int q = q0 + (lane & 15);
    const bool qok = q < n;
    v4f dq[HD / 16];
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) dq[dt] = v4f{0, 0, 0, 0};
    RowFrag<T, HD> qf[HD / 32], df[HD / 32];
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
      if (TWO) {
        qf[ks].glob(qkv + (int64_t)(qok ? q : 0) * a.ld_qkv + h * HD, ks, lane, qok);
        df[ks].glob(dO + (int64_t)(qok ? q : 0) * a.ld_o, ks, lane, qok);
      } else {
        qf[ks].lds(Qi, q0, ks, lane);
        df[ks].lds(Di, q0, ks, lane);
      }
    }
    const float lq = L2[q], dq_ = Dv[q];
    for (int kc = 0; kc < npad; kc += 32) {
      v4f dST[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kb = kc + 16 * u;
        v4f s = {lq, lq, lq, lq}, dp = {dq_, dq_, dq_, dq_};
        if constexpr (DROP) dp = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < HD / 32; ++ks) {
          RowFrag<T, HD> kf, vf;
          kf.lds(Ki, kb, ks, lane);
          vf.lds(Vi, kb, ks, lane);
          s = mma32(kf, qf[ks], s);    // S^T[key=4g+i][q=lane&15]
          dp = mma32(vf, df[ks], dp);  // dP^T
        }
        if constexpr (DROP) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool keep = dropout_keep(dseed, dbh, q, kb + 4 * g + i, dthr);
            dp[i] = (keep ? dp[i] * dsc : 0.f) + dq_;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) dST[u][i] = __builtin_amdgcn_exp2f(s[i] * c) * dp[i];
        if constexpr (MASKED) {
          // masked and padding keys: P = 0 (a select, as below)
          const v4f kq = *(const v4f*)(kvm + kb + 4 * g);
#pragma unroll
          for (int i = 0; i < 4; ++i) dST[u][i] = kq[i] != 0.f ? dST[u][i] : 0.f;
        }
        // padding keys (last chunk only): K rows are zero, but an overflowing
        // exp2(-lse) would turn 0 * inf into NaN in dQ, so zero them explicitly
        if (kb + 16 > n) {
#pragma unroll
          for (int i = 0; i < 4; ++i) dST[u][i] = (kb + 4 * g + i < n) ? dST[u][i] : 0.f;
        }
      }
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt) dq[dt] = mma_rowsum<T, HD>(Ki, kc, 16 * dt, dST[0], dST[1], dq[dt], lane);
    }
    if constexpr (Q8 && std::is_same<T, bf16_t>::value) {
      {
        v4f qv[HD / 16];
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt) qv[dt] = dq[dt] * a.scale;
        q8_store<HD>(a, (int64_t)b * n + q, qok, h * HD, 3 * HH, qv, lane);
      }
    }
    if (qok) {
      T* rowp = dqkv + (int64_t)q * a.ld_dqkv + h * HD;
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt) st4<T>(rowp + 16 * dt + 4 * g, dq[dt] * a.scale);
#pragma unroll
      for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) cq[dt][i] += dq[dt][i];
    }
  }
  if (a.colsum_partial) {
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float sq = cq[dt][i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sq += __shfl_xor(sq, o, 64);
        if ((lane & 15) == 0) cs[wave * 3 * HD + 16 * dt + 4 * g + i] = sq * a.scale;
      }
  }
  ASTAMP(4);
  if (a.colsum_partial) {
    __syncthreads();
    // colsum_partial row b: [3*H*HD], this head's q/k/v column slices
    for (int i = threadIdx.x; i < 3 * HD; i += NTH) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += cs[w * 3 * HD + i];
      const int part = i / HD, d = i % HD;
      a.colsum_partial[(int64_t)b * 3 * HH + part * HH + h * HD + d] = s;
    }
  }
  ASTAMP(5);
}

// ================================================================ the route
using maeclip::AttnPath;
using maeclip::AttnRoute;

AttnRoute rejected(AttnRoute r, const char* fmt, ...) {
  r.path = AttnPath::REJECTED;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(r.err, sizeof(r.err), fmt, ap);
  va_end(ap);
  return r;
}

// option ATTN_STREAM: 1 forces the streamed kernels, 0 turns them off, unset
// (-1) takes them exactly where the resident kernels' LDS images do not fit.
template <int HD> bool stream_wanted(const maeclip_attn_args& a, bool bwd) {
  const int os = maeclip::option(MAECLIP_OPT_ATTN_STREAM, -1);
  if (os >= 0) return os == 1;
  if (!bwd) return fwd_lds<bf16_t, HD>(a.n) > LDS_MAX;
  const int tiles = (a.n + 15) / 16, nw = tiles < MAXW ? tiles : MAXW;
  // the two-image layout is the smallest; ATTN_TWO = 0 pins the four-image one
  if (bwd_lds<bf16_t, HD>(a.n, nw, true) > LDS_MAX) return true;
  return maeclip::option(MAECLIP_OPT_ATTN_TWO, -1) == 0 && bwd_lds<bf16_t, HD>(a.n, nw) > LDS_MAX;
}

// The whole choice of kernel for a checked call, in the order the conditions
// take precedence. No HIP call: a rejected launch can be told from a failed
// one on any host, and tests/test_attention_route_cpu.py reads the answer
// through maeclip_attn_impl without a device.
template <typename T, int HD>
AttnRoute route(const maeclip_attn_args& a, bool bwd) {
  constexpr bool BF = std::is_same<T, bf16_t>::value;
  AttnRoute r{};
  r.bwd = bwd;
  const int tiles = (a.n + 15) / 16;
  if constexpr (BF) {
    // beyond the LDS-resident limit (or forced): the streamed kernels
    if (stream_wanted<HD>(a, bwd)) {
      if (a.key_mask || a.dropout_p != 0.f)
        return rejected(r, "maeclip_attn_%s: the streamed path (option ATTN_STREAM; bf16 beyond the LDS-resident limit, "
                           "n > %d at head_dim %d) takes no key_mask and no dropout (got n %d)",
                        bwd ? "bwd" : "fwd", resident_max_n<HD>(bwd), HD, a.n);
      r.nw = tiles < MAXW ? tiles : MAXW;
      const int64_t ldm = a.ld_qkv > a.ld_o ? a.ld_qkv : a.ld_o;
      const int64_t nwg = (int64_t)a.B * a.H * ((tiles + r.nw - 1) / r.nw);
      if (!(((int64_t)a.n + 2 * SB) * ldm * 2 < 0x7fffffff && nwg < 0x7fffffff))
        return rejected(r, "maeclip_attn(streamed): a sample's rows must span less than 2 GiB (n %d, row stride %lld)",
                        a.n, (long long)ldm);
      r.path = AttnPath::STREAM;
      return r;
    }
  }
  // one wave per 16-row tile (no idle waves), at most MAXW; the forward
  // spreads its tiles evenly over the rounds it needs (n = 197: 13 tiles on 7
  // waves, not 8 waves of which 3 idle for the second round)
  const int rounds = (tiles + MAXW - 1) / MAXW;
  r.nw = bwd ? (tiles < MAXW ? tiles : MAXW) : (tiles + rounds - 1) / rounds;
  r.lds = bwd ? bwd_lds<T, HD>(a.n, r.nw) : fwd_lds<T, HD>(a.n);
  // bf16 backward, four LDS images or two: option ATTN_TWO = 0 / 1 / 3 pins the
  // layout (3: two images at 3 workgroups per CU, head_dim 32 only -- at 64 it
  // is the two-image kernel); unset (-1), the occupancy decides at the launch.
  // Only while the two-image layout fits: otherwise four images, and the
  // rejection below reports their size.
  int layout = 0;
  if constexpr (BF) {
    if (bwd) {
      const size_t lds2 = bwd_lds<T, HD>(a.n, r.nw, true);
      if (lds2 <= LDS_MAX) {
        const int forced = maeclip::option(MAECLIP_OPT_ATTN_TWO, -1);
        layout = forced < 0 ? -1 : forced == 0 ? 0 : forced == 3 && HD == 32 ? 3 : 1;
      }
      if (layout > 0) r.lds = lds2;
    }
  } else {
    // fp32 beyond the LDS images (option ATTN_ROWS = 1 forces it: tests)
    if (r.lds > LDS_MAX || maeclip::option(MAECLIP_OPT_ATTN_ROWS, 0) != 0) {
      if (a.dropout_p != 0.f) return rejected(r, "maeclip_attn: the fp32 long-sequence path has no attention dropout");
      r.path = AttnPath::ROWS;
      r.nw = 1;
      r.lds = 0;
      return r;
    }
  }
  if (bwd && (a.key_mask || a.dropout_p > 0.f)) {
    // the trainable text tower's backward: its own instantiations of the
    // two-phase kernel (npad <= 256 at head_dim 64: 137 KiB of LDS in bf16,
    // 145 KiB in fp32)
    if (!(HD == 64 && a.n <= 256))
      return rejected(r, "maeclip_attn_bwd: key_mask / dropout need head_dim 64 and n <= 256 (got head_dim %d, n %d); "
                         "past that only the fp32 rows path takes a key_mask", HD, a.n);
    if (!(a.dropout_p < 1.f)) return rejected(r, "maeclip_attn_bwd: dropout_p must be < 1");
    r.lds = bwd_lds<T, HD>(a.n, r.nw, !BF, true);
    if (r.lds > LDS_MAX) return rejected(r, "maeclip_attn_bwd: n=%d needs %zu B of LDS (> 160 KiB)", a.n, r.lds);
    r.path = AttnPath::BWD_MASKED;
    return r;
  }
  // (by occupancy: the two-image layout fits, so one of the layouts does)
  if (layout >= 0 && r.lds > LDS_MAX)
    return rejected(r, "maeclip_attn: n=%d needs %zu B of LDS (> 160 KiB)", a.n, r.lds);
  if constexpr (BF) {
    if (bwd) {
      // one-pass diagonal backward: the default at HD 32 up to npad 256
      // (MAECLIP_ATTN_DIAG=0 turns it off). HD 64 (LDS fits up to npad 224): the
      // 56 KB f32 dQ image leaves one workgroup per CU, whose ~140 KB prologue
      // has nothing to overlap with -- slower everywhere with a barrier per
      // round (profiles/r03/attn_diag64_ab.txt); with the per-wave round flags
      // it wins at the long rows only (C1 encoder n = 197: 299 -> 289 us; C2
      // encoder n = 50: 52 -> 55; C4 n = 145 even; profiles/r05/attn_diag64_ab_r5ag.txt),
      // so it is the default for npad >= 192 (option ATTN_DIAG = 1 / 0 forces it on / off).
      // (A key_mask or dropout call never gets here.)
      const int od = maeclip::option(MAECLIP_OPT_ATTN_DIAG, -1);
      const int npad = (a.n + 31) & ~31;
      const size_t ld = bwd_diag_lds<HD>(a.n);
      const bool want = HD == 32 ? od != 0 : (od >= 0 ? od == 1 : npad >= 192);
      if (npad <= 256 && ld <= LDS_MAX && want) {
        r.path = AttnPath::BWD_DIAG;
        r.nw = npad / 32;
        r.lds = ld;
        return r;
      }
      // bf16 rows beyond the diagonal kernel with more 16-row tiles than MAXW
      // waves: the two-image layout with up to 16 waves, default at HD 32 (C4
      // decoder n = 577: 604 -> 555 us; at HD 64 the C4 encoder, n = 145, loses:
      // 147 -> 168; profiles/r05/attn_bw16_ab_r5ah.txt). Option ATTN_BW16 = 1 / 0
      // forces it on / off. Where its LDS does not fit, the 8-wave kernels below.
      const int o16 = maeclip::option(MAECLIP_OPT_ATTN_BW16, -1);
      if (tiles > MAXW && (o16 >= 0 ? o16 != 0 : HD == 32)) {
        const int nw16 = tiles < 16 ? tiles : 16;
        const size_t lds16 = bwd_lds<T, HD>(a.n, nw16, true);
        if (lds16 <= LDS_MAX) {
          r.path = AttnPath::BWD_16;
          r.nw = nw16;
          r.lds = lds16;
          r.q8_fused = a.q8 != nullptr;
          return r;
        }
      }
    }
  }
  if (bwd) {
    // (round 2 also had a bf16 variant that kept dS in LDS between the two
    // phases instead of recomputing S / dP for dQ: 355 vs 224 us at the
    // decoder shape, the n x n image halving the workgroups per CU; removed)
    r.path = layout < 0 ? AttnPath::BWD_OCC : layout == 3 ? AttnPath::BWD_TWO3 : layout == 1 ? AttnPath::BWD_TWO
                                                                                           : AttnPath::BWD_FOUR;
    // BWD_TWO3 has no fused-copy instantiation (BWD_OCC: bwd_two settles it with the layout)
    r.q8_fused = BF && a.q8 != nullptr && r.path != AttnPath::BWD_TWO3;
    return r;
  }
  // the fused fp8 copy: bf16 without dropout (the fp8 stacks' case)
  r.q8_fused = BF && a.q8 != nullptr && a.dropout_p == 0.f;
  // (n <= 48: at most three query tiles, one per wave -- the DMA'd Q saves no
  // round trip and lengthens the prologue: text n = 25 13.5 -> 15.5 us)
  r.qimg = a.n > 48 && fwd_qimg<T, HD>((a.n + 63) & ~63);
  r.path = AttnPath::FWD;
  // one workgroup per CU by LDS and more tiles than MAXW waves: up to 16
  // waves (option ATTN_FW16 = 0 turns it off); Q from global there
  if (tiles > MAXW && 2 * r.lds > LDS_MAX && maeclip::option(MAECLIP_OPT_ATTN_FW16, 1) != 0) {
    const int r16 = (tiles + 15) / 16;
    r.nw = (tiles + r16 - 1) / r16;
    r.qimg = false;
    r.path = AttnPath::FWD16;
  }
  return r;
}

// =============================================================== the launch
typedef void (*attn_kernel_t)(const maeclip_attn_args);

// the forward instantiation of a route: dropout x fused fp8 copy x Q image x 16 waves
template <typename T, int HD>
attn_kernel_t fwd_kernel_for(const maeclip_attn_args& a, const AttnRoute& r) {
  const bool drop = a.dropout_p > 0.f, q8 = r.q8_fused;
  if (r.path == AttnPath::FWD16)
    return drop ? attn_fwd_kernel<T, HD, true, 16>
                : (q8 ? attn_fwd_kernel<T, HD, false, 16, true> : attn_fwd_kernel<T, HD, false, 16>);
  if constexpr (std::is_same<T, bf16_t>::value) {
    if (r.qimg)
      return drop ? attn_fwd_kernel<T, HD, true, MAXW, false, true>
                  : (q8 ? attn_fwd_kernel<T, HD, false, MAXW, true, true> : attn_fwd_kernel<T, HD, false, MAXW, false, true>);
  }
  return drop ? attn_fwd_kernel<T, HD, true>
              : (q8 ? attn_fwd_kernel<T, HD, false, MAXW, true> : attn_fwd_kernel<T, HD, false>);
}

// the two-phase backward instantiation of a route (BWD_OCC settled before)
template <typename T, int HD>
attn_kernel_t bwd_kernel_for(const maeclip_attn_args& a, const AttnRoute& r) {
  if (r.path == AttnPath::BWD_MASKED) {
    if constexpr (HD == 64) {   // (four images in bf16, two in fp32; 8 waves)
      const bool drop = a.dropout_p > 0.f;
      return a.key_mask && drop ? attn_bwd_kernel<T, HD, false, 1, MAXW, false, true, true>
             : a.key_mask       ? attn_bwd_kernel<T, HD, false, 1, MAXW, false, true, false>
                                : attn_bwd_kernel<T, HD, false, 1, MAXW, false, false, true>;
    }
  }
  if constexpr (std::is_same<T, bf16_t>::value) {
    const bool q8 = r.q8_fused;
    switch (r.path) {
      case AttnPath::BWD_16:
        return q8 ? attn_bwd_kernel<T, HD, true, 1, 16, true> : attn_bwd_kernel<T, HD, true, 1, 16>;
      case AttnPath::BWD_TWO3: return attn_bwd_kernel<T, HD, true, HD == 32 ? 3 : 1>;
      case AttnPath::BWD_TWO: return q8 ? attn_bwd_kernel<T, HD, true, 1, MAXW, true> : attn_bwd_kernel<T, HD, true>;
      default: if (q8) return attn_bwd_kernel<T, HD, false, 1, MAXW, true>;
    }
  }
  return attn_bwd_kernel<T, HD, false>;
}

// resident workgroups per CU of a bwd variant (registers, waves and LDS)
template <typename T, int HD, bool TWO, int OCC = 1>
int bwd_occupancy(int nthreads, size_t lds) {
  if (lds > LDS_FREE)
    maeclip::allow_lds((const void*)attn_bwd_kernel<T, HD, TWO, OCC>, (int)lds);
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)attn_bwd_kernel<T, HD, TWO, OCC>,
                                                   nthreads, lds) != hipSuccess)
    return 0;
  return nb;
}

// BWD_OCC -> BWD_FOUR, BWD_TWO or BWD_TWO3 (bf16): the two-image backward when
// it keeps more workgroups per CU resident; cached per shape. The one place
// attention asks the device, and only for routes that come back "by occupancy".
template <int HD>
void bwd_two(const maeclip_attn_args& a, AttnRoute& r) {
  const size_t lds4 = r.lds, lds2 = bwd_lds<bf16_t, HD>(a.n, r.nw, true);
  static int cache[2][64][MAXW + 1] = {};   // (npad / 32) x nw -> variant + 1
  const int key = ((a.n + 31) >> 5) & 63;
  int& c = cache[HD == 64][key][r.nw];
  if (c == 0) {
    const int occ4 = lds4 <= LDS_MAX ? bwd_occupancy<bf16_t, HD, false>(64 * r.nw, lds4) : 0;
    const int occ2 = bwd_occupancy<bf16_t, HD, true>(64 * r.nw, lds2);
    const int occ3 = HD == 32 ? bwd_occupancy<bf16_t, HD, true, 3>(64 * r.nw, lds2) : 0;
    c = occ3 > occ2 && occ3 > occ4 ? 4 : occ2 > occ4 ? 2 : 1;
  }
  r.path = c == 4 ? AttnPath::BWD_TWO3 : c == 2 ? AttnPath::BWD_TWO : AttnPath::BWD_FOUR;
  if (c != 1) r.lds = lds2;
  r.q8_fused = a.q8 != nullptr && c != 4;
}

// r: BWD_OCC is settled in place, so the caller sees q8_fused of what ran
template <typename T, int HD>
int run(const maeclip_attn_args& a, AttnRoute& r, hipStream_t s) {
  if constexpr (std::is_same<T, bf16_t>::value) {
    if (r.path == AttnPath::BWD_OCC) {
      bwd_two<HD>(a, r);
      // four images chosen although they do not fit: only if the device reported no occupancy for either layout
      MC_CHECK_ARG(r.lds <= LDS_MAX, "maeclip_attn: n=%d needs %zu B of LDS (> 160 KiB)", a.n, r.lds);
    }
  }
  switch (r.path) {
    case AttnPath::STREAM: return maeclip::attn_stream(a, r, s);
    case AttnPath::ROWS: return maeclip::attn_rows(a, r, s);
    case AttnPath::BWD_DIAG: return maeclip::attn_diag(a, r, s);
    case AttnPath::FWD:
    case AttnPath::FWD16: return attn_launch(fwd_kernel_for<T, HD>(a, r), "maeclip_attn_fwd", a, r, s);
    case AttnPath::BWD_MASKED:
      return attn_launch(bwd_kernel_for<T, HD>(a, r), "maeclip_attn_bwd(mask / dropout)", a, r, s);
    case AttnPath::BWD_16: return attn_launch(bwd_kernel_for<T, HD>(a, r), "maeclip_attn_bwd(16 waves)", a, r, s);
    default: return attn_launch(bwd_kernel_for<T, HD>(a, r), "maeclip_attn_bwd", a, r, s);
  }
}

int check(const maeclip_attn_args* a, bool bwd) {
  MC_CHECK_ARG(a && a->qkv && a->o, "maeclip_attn: null pointer");
  MC_CHECK_ARG(a->head_dim == 32 || a->head_dim == 64, "maeclip_attn: head_dim must be 32 or 64 (got %d)", a->head_dim);
  MC_CHECK_ARG(a->B > 0 && a->n > 0 && a->H > 0, "maeclip_attn: bad sizes");
  MC_CHECK_ARG(a->dtype == MAECLIP_F32 || a->dtype == MAECLIP_BF16, "maeclip_attn: bad dtype");
  const int epc = a->dtype == MAECLIP_BF16 ? 8 : 4;
  MC_CHECK_ARG(a->ld_qkv % epc == 0 && a->ld_o % epc == 0, "maeclip_attn: row strides must be 16-byte multiples");
  if (bwd) {
    MC_CHECK_ARG(a->dout && a->dqkv && a->lse, "maeclip_attn_bwd: null pointer");
    MC_CHECK_ARG(a->ld_dqkv % epc == 0, "maeclip_attn_bwd: ld_dqkv");
  }
  if (a->q8) {
    const int64_t len = (int64_t)a->H * a->head_dim * (bwd ? 3 : 1);
    MC_CHECK_ARG(len % 128 == 0 && a->ldq8 >= len && a->ldq8 % 16 == 0 && ((uintptr_t)a->q8 & 15) == 0 &&
                     a->q8_scale && (a->q8_fmt == MAECLIP_FP8_E4M3 || a->q8_fmt == MAECLIP_FP8_E5M2),
                 "maeclip_attn: fp8-blocks output needs a row length %% 128, ldq8 %% 16, a scale buffer and a format");
  }
  return 0;
}

}  // namespace

namespace maeclip {
AttnRoute attn_route(const maeclip_attn_args& a, bool bwd) {
  if (a.dtype == MAECLIP_BF16) return a.head_dim == 64 ? route<bf16_t, 64>(a, bwd) : route<bf16_t, 32>(a, bwd);
  return a.head_dim == 64 ? route<float, 64>(a, bwd) : route<float, 32>(a, bwd);
}
}  // namespace maeclip

namespace {

int dispatch(const maeclip_attn_args* a, bool bwd, void* stream) {
  if (int e = check(a, bwd)) return e;
  AttnRoute r = maeclip::attn_route(*a, bwd);
  MC_CHECK_ARG(r.path != AttnPath::REJECTED, "%s", r.err);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (a->dtype == MAECLIP_BF16) rc = a->head_dim == 64 ? run<bf16_t, 64>(*a, r, s) : run<bf16_t, 32>(*a, r, s);
  else rc = a->head_dim == 64 ? run<float, 64>(*a, r, s) : run<float, 32>(*a, r, s);
  if (rc != 0 || !a->q8 || r.q8_fused) return rc;
  // routes without the fused copy: the standalone pass over the output
  const int64_t HH = (int64_t)a->H * a->head_dim;
  return bwd ? maeclip_quant_blocks_fp8(a->dqkv, a->dtype, (int64_t)a->B * a->n, 3 * HH, a->ld_dqkv, a->q8, a->ldq8,
                                        a->q8_scale, a->q8_fmt, stream)
             : maeclip_quant_blocks_fp8(a->o, a->dtype, (int64_t)a->B * a->n, HH, a->ld_o, a->q8, a->ldq8,
                                        a->q8_scale, a->q8_fmt, stream);
}

}  // namespace

#ifdef ATTN_STAMPS
// the later stamp of the two translation units that keep stamps (a slot's
// counter only grows, and a run stamps one of them)
extern "C" int maeclip_debug_attn_stamps(uint64_t* host, int n) {
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_attn_stamps), sizeof(uint64_t) * (size_t)n) != hipSuccess) return -1;
  uint64_t* diag = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)n);
  const int rc = diag ? maeclip::attn_diag_stamps(diag, n) : -1;
  for (int i = 0; rc == 0 && i < n; ++i) host[i] = diag[i] > host[i] ? diag[i] : host[i];
  free(diag);
  return rc;
}
#endif

// The route of *args as a number (maeclip::AttnPath) after the argument checks
// of maeclip_attn_fwd (bwd = 0) / maeclip_attn_bwd: nothing is launched and no
// device is needed. -1 and the message for a call those would reject.
extern "C" int32_t maeclip_attn_impl(const maeclip_attn_args* a, int32_t bwd) {
  if (int e = check(a, bwd != 0)) return e;
  const AttnRoute r = maeclip::attn_route(*a, bwd != 0);
  MC_CHECK_ARG(r.path != AttnPath::REJECTED, "%s", r.err);
  return (int32_t)r.path;
}

extern "C" int32_t maeclip_attn_fwd(const maeclip_attn_args* a, void* stream) { return dispatch(a, false, stream); }
extern "C" int32_t maeclip_attn_bwd(const maeclip_attn_args* a, void* stream) { return dispatch(a, true, stream); }

#include "attention_stream.h"

