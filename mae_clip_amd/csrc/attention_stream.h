// Attention in bf16 beyond the LDS-resident limit: maeclip::attn_stream, the
// route maeclip::AttnPath::STREAM of attention.hip. A file of its own, but
// compiled in attention.hip's translation unit (included at its end): these
// kernels and the resident ones call the same helpers (fwd_chunk, RowFrag,
// mma_rowsum), which the compiler's interprocedural passes shape by all their
// callers before they are inlined. Compiled apart, both sides come out with
// other code (profiles/r18: the text forward 13.8 -> 15.4 us); together they
// are the kernels they were.
#pragma once
#include "attention_common.h"

namespace {

// ===================================== bf16 beyond the LDS-resident limit
// Streamed kernels: the LDS footprint does not grow with n. A workgroup owns
// a block of 16 NW query (forward, dQ) or key (dK / dV) rows, one 16-row tile
// per wave with its operand fragments in registers, and the other side of the
// product arrives in SB = 64 row blocks through a ring of two LDS slots. A
// slot is an Img<bf16_t, HD> image of 64 rows filled by LDS-DMA exactly as
// dma_imgs fills a whole sequence (swizzle in the source address, rows >= n
// zero through the descriptor range), so fwd_chunk and the MFMA bodies of the
// two-phase backward run on it unchanged with a block-local row index.
// Ring protocol, one iteration per block j: the DMA of block j + 1 is issued
// into the other slot, block j is consumed, then the wave waits for its own
// DMA (vmcnt) and a workgroup barrier hands the slot over -- it also says that
// every wave is done reading slot j, which block j + 2 overwrites.
// K / V (Q / dO / O) are re-read once per row block of the owning side, from
// L2 after the first (no non-temporal hint here). No key_mask, no dropout.
// (SB = 64 rows per streamed block = rows of a ring slot: attention_common.h)

// rows row0 .. row0 + 63 of NI head slices -> NI ring slots; the caller waits
template <int HD, int NI>
__device__ __forceinline__ void dma_block(char* const (&dst)[NI], const bf16_t* const (&src)[NI],
                                          const int64_t (&ld)[NI], int row0, int n) {
  using I = Img<bf16_t, HD>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nw = (int)(blockDim.x >> 6);
  for (int k = wave; k < I::CPR; k += nw) {   // SB * CPR / 64 wave-instructions of 1 KiB per image
    const int id = k * 64 + lane;
    const int r = id / I::CPR, sl = id % I::CPR;   // f(row0 + r) = f(r): row0 is a multiple of 64
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int64_t span = ((int64_t)(n - 1) * ld[i] + HD) * 2;
      const int nrec = (int)(span < 0x7fffffff ? span : 0x7fffffff);
      const int voff = (row0 + r) * (int)ld[i] * 2 + ((sl ^ I::f(r)) << 4);
      const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src[i], (short)0, nrec, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(dst[i] + k * 1024), 16, voff, 0, 0, 0);
    }
  }
}
// the wave's own DMA has landed, then the workgroup's: the slot hand-over
__device__ __forceinline__ void ring_handover() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
// barrier for plain LDS traffic that leaves the LDS-DMA in flight (a
// __syncthreads() would wait for it: it counts as a pending LDS write)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// (sample, head, row block) of a streamed workgroup: the row blocks of one
// head are consecutive ids, so they share their XCD's L2 copy of the stream
struct StreamId { int b, h, rb; };
__device__ __forceinline__ StreamId stream_id(int H, int nrb) {
  const int bid = xcd_chunk_id(blockIdx.x, gridDim.x);
  const int bh = bid / nrb;
  return {bh / H, bh % H, bid % nrb};
}

template <int HD>
__global__ void __launch_bounds__(MAXW * 64) attn_fwd_stream_kernel(const maeclip_attn_args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using I = Img<bf16_t, HD>;
  constexpr int SLOT = SB * I::ROWB;
  const int n = a.n, H = a.H, HH = H * HD;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = lane >> 4;
  const StreamId id = stream_id(H, (n + 16 * NW - 1) / (16 * NW));
  const int b = id.b, h = id.h;
  // ring: slot s = K image, V image; then the tail block's key bias
  float* kmask = (float*)(smem + 4 * SLOT);
  const int nblk = (n + SB - 1) / SB, nfull = n / SB;
  if (threadIdx.x < SB) kmask[threadIdx.x] = nfull * SB + (int)threadIdx.x < n ? 0.f : NEG_BIG;

  const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)b * n * a.ld_qkv;
  const bf16_t* const src[2] = {qkv + HH + h * HD, qkv + 2 * HH + h * HD};
  const int64_t ld[2] = {a.ld_qkv, a.ld_qkv};
  const int q0 = (id.rb * NW + wave) * 16;
  const int q = q0 + (lane & 15);
  const bool qok = q < n, active = q0 < n;   // a wave without query rows still feeds the ring
  RowFrag<bf16_t, HD> qf[HD / 32];
#pragma unroll
  for (int ks = 0; ks < HD / 32; ++ks) qf[ks].glob(qkv + (int64_t)(qok ? q : 0) * a.ld_qkv + h * HD, ks, lane, qok);
  {
    char* const dst[2] = {smem, smem + SLOT};
    dma_block<HD, 2>(dst, src, ld, 0, n);
  }
  ring_handover();

  const float c = a.scale * LOG2E;
  const FwdDrop dr{};
  float m = NEG_BIG, lsum = 0.f;
  v4f o[HD / 16], ol = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dt = 0; dt < HD / 16; ++dt) o[dt] = v4f{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < nblk; ++j) {
    const char* Kimg = smem + (j & 1) * 2 * SLOT;
    const char* Vimg = Kimg + SLOT;
    if (j + 1 < nblk) {
      char* const dst[2] = {smem + ((j + 1) & 1) * 2 * SLOT, smem + ((j + 1) & 1) * 2 * SLOT + SLOT};
      dma_block<HD, 2>(dst, src, ld, (j + 1) * SB, n);
    }
    if (active) {
      if (j < nfull) {
        fwd_chunk<bf16_t, HD, 4, false, false>(Kimg, Vimg, kmask, 0, qf, c, m, lsum, o, ol, lane, dr, q);
      } else {
        // the 16-key tiles of the tail block that hold real keys (wave-uniform)
        const int rem = n - j * SB;
        if (rem > 48) fwd_chunk<bf16_t, HD, 4, true, false>(Kimg, Vimg, kmask, 0, qf, c, m, lsum, o, ol, lane, dr, q);
        else if (rem > 32) fwd_chunk<bf16_t, HD, 3, true, false>(Kimg, Vimg, kmask, 0, qf, c, m, lsum, o, ol, lane, dr, q);
        else if (rem > 16) fwd_chunk<bf16_t, HD, 2, true, false>(Kimg, Vimg, kmask, 0, qf, c, m, lsum, o, ol, lane, dr, q);
        else fwd_chunk<bf16_t, HD, 1, true, false>(Kimg, Vimg, kmask, 0, qf, c, m, lsum, o, ol, lane, dr, q);
      }
    }
    ring_handover();
  }
  if (qok) {
    lsum = ol[0];   // the MFMA row sum, whole in every lane of the query
    const float inv = 1.f / lsum;
    bf16_t* orow = (bf16_t*)a.o + ((int64_t)b * n + q) * a.ld_o + h * HD;
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) st4<bf16_t>(orow + 16 * dt + 4 * g, o[dt] * inv);
    if (g == 0 && a.lse) a.lse[((int64_t)b * H + h) * n + q] = m + log2f(lsum);
  }
}

// dQ: the workgroup's query tiles keep Q, dO, -lse / c and Dv = -rowsum(dO O)
// in registers; K / V blocks stream. The body is phase 2 of attn_bwd_kernel.
template <int HD>
__global__ void __launch_bounds__(MAXW * 64) attn_bwd_stream_dq_kernel(const maeclip_attn_args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using I = Img<bf16_t, HD>;
  constexpr int SLOT = SB * I::ROWB;
  const int n = a.n, H = a.H, HH = H * HD;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = lane >> 4;
  const StreamId id = stream_id(H, (n + 16 * NW - 1) / (16 * NW));
  const int b = id.b, h = id.h;
  const int nblk = (n + SB - 1) / SB;

  const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)b * n * a.ld_qkv;
  const bf16_t* O = (const bf16_t*)a.o + (int64_t)b * n * a.ld_o + h * HD;
  const bf16_t* dO = (const bf16_t*)a.dout + (int64_t)b * n * a.ld_o + h * HD;
  const bf16_t* const src[2] = {qkv + HH + h * HD, qkv + 2 * HH + h * HD};
  const int64_t ld[2] = {a.ld_qkv, a.ld_qkv};
  const int q0 = (id.rb * NW + wave) * 16;
  const int q = q0 + (lane & 15);
  const bool qok = q < n, active = q0 < n;
  const int qr = qok ? q : 0;
  RowFrag<bf16_t, HD> qf[HD / 32], df[HD / 32];
  float dd = 0.f;
#pragma unroll
  for (int ks = 0; ks < HD / 32; ++ks) {
    RowFrag<bf16_t, HD> of;
    qf[ks].glob(qkv + (int64_t)qr * a.ld_qkv + h * HD, ks, lane, qok);
    df[ks].glob(dO + (int64_t)qr * a.ld_o, ks, lane, qok);
    of.glob(O + (int64_t)qr * a.ld_o, ks, lane, qok);
    dd += chunk_dot<bf16_t>(__builtin_bit_cast(v4u, df[ks].v), __builtin_bit_cast(v4u, of.v));
  }
  // the row's chunks sit on lanes l, l ^ 16, l ^ 32, l ^ 48
  const float dq_ = -sum4rows(dd);
  const float lq = qok ? -a.lse[((int64_t)b * H + h) * n + q] * (1.f / (a.scale * LOG2E)) : -1.0e30f;
  {
    char* const dst[2] = {smem, smem + SLOT};
    dma_block<HD, 2>(dst, src, ld, 0, n);
  }
  ring_handover();

  const float c = a.scale * LOG2E;
  v4f dq[HD / 16];
#pragma unroll
  for (int dt = 0; dt < HD / 16; ++dt) dq[dt] = v4f{0, 0, 0, 0};
  for (int j = 0; j < nblk; ++j) {
    const char* Ki = smem + (j & 1) * 2 * SLOT;
    const char* Vi = Ki + SLOT;
    if (j + 1 < nblk) {
      char* const dst[2] = {smem + ((j + 1) & 1) * 2 * SLOT, smem + ((j + 1) & 1) * 2 * SLOT + SLOT};
      dma_block<HD, 2>(dst, src, ld, (j + 1) * SB, n);
    }
    if (active) {
      const int k0 = j * SB;
      for (int kc = 0; kc < SB && k0 + kc < n; kc += 32) {
        v4f dST[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int kb = kc + 16 * u;
          v4f s = {lq, lq, lq, lq}, dp = {dq_, dq_, dq_, dq_};
#pragma unroll
          for (int ks = 0; ks < HD / 32; ++ks) {
            RowFrag<bf16_t, HD> kf, vf;
            kf.lds(Ki, kb, ks, lane);
            vf.lds(Vi, kb, ks, lane);
            s = mma32(kf, qf[ks], s);    // S^T[key=4g+i][q=lane&15]
            dp = mma32(vf, df[ks], dp);  // dP^T
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) dST[u][i] = __builtin_amdgcn_exp2f(s[i] * c) * dp[i];
          // padding keys (zero K rows): an overflowing exp2(-lse) would turn
          // 0 * inf into NaN in dQ, so zero them explicitly
          if (k0 + kb + 16 > n) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dST[u][i] = (k0 + kb + 4 * g + i < n) ? dST[u][i] : 0.f;
          }
        }
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt)
          dq[dt] = mma_rowsum<bf16_t, HD>(Ki, kc, 16 * dt, dST[0], dST[1], dq[dt], lane);
      }
    }
    ring_handover();
  }
  if (qok) {
    bf16_t* rowp = (bf16_t*)a.dqkv + ((int64_t)b * n + q) * a.ld_dqkv + h * HD;
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) st4<bf16_t>(rowp + 16 * dt + 4 * g, dq[dt] * a.scale);
  }
}

// dK, dV: the workgroup's key tiles keep K, V in registers (as the two-image
// variant's phase 1); Q, dO and O blocks stream, and lse with them (a 4-byte
// DMA per row). maeclip_attn_args has nowhere to keep Dv between the passes,
// so every block's Dv = -rowsum(dO O) is formed from the dO / O images by the
// whole workgroup (a chunk pair per thread) before the block is consumed.
template <int HD>
__global__ void __launch_bounds__(MAXW * 64) attn_bwd_stream_dkv_kernel(const maeclip_attn_args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using I = Img<bf16_t, HD>;
  constexpr int SLOT = SB * I::ROWB, CPR = I::CPR;
  const int n = a.n, H = a.H, HH = H * HD;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = lane >> 4;
  const StreamId id = stream_id(H, (n + 16 * NW - 1) / (16 * NW));
  const int b = id.b, h = id.h;
  const int nblk = (n + SB - 1) / SB;
  // ring: slot s = Q, dO, O images; then lse of both slots, then L2 / Dv of the current block
  float* lraw = (float*)(smem + 6 * SLOT);   // [2][SB]
  float* L2 = lraw + 2 * SB;                 // [SB] -lse / c, -1e30 on padding rows
  float* Dv = L2 + SB;                       // [SB]

  const bf16_t* qkv = (const bf16_t*)a.qkv + (int64_t)b * n * a.ld_qkv;
  const bf16_t* const src[3] = {qkv + h * HD, (const bf16_t*)a.dout + (int64_t)b * n * a.ld_o + h * HD,
                                (const bf16_t*)a.o + (int64_t)b * n * a.ld_o + h * HD};
  const int64_t ld[3] = {a.ld_qkv, a.ld_o, a.ld_o};
  const float* lse = a.lse + ((int64_t)b * H + h) * n;
  auto stage = [&](int j) {
    char* base = smem + (j & 1) * 3 * SLOT;
    char* const dst[3] = {base, base + SLOT, base + 2 * SLOT};
    dma_block<HD, 3>(dst, src, ld, j * SB, n);
    if (wave == 0) {   // rows >= n read as zero
      const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)lse, (short)0, n * 4, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(lraw + (j & 1) * SB), 4, (j * SB + lane) * 4, 0, 0, 0);
    }
  };
  const int k0 = (id.rb * NW + wave) * 16;
  const int key = k0 + (lane & 15);
  const bool kok = key < n, active = k0 < n;
  RowFrag<bf16_t, HD> kf[HD / 32], vf[HD / 32];
#pragma unroll
  for (int ks = 0; ks < HD / 32; ++ks) {
    const bf16_t* kr = qkv + (int64_t)(kok ? key : 0) * a.ld_qkv + HH + h * HD;
    kf[ks].glob(kr, ks, lane, kok);
    vf[ks].glob(kr + HH, ks, lane, kok);
  }
  stage(0);
  ring_handover();

  const float c = a.scale * LOG2E, inv_c = 1.f / c;
  v4f dv[HD / 16], dk[HD / 16];
#pragma unroll
  for (int dt = 0; dt < HD / 16; ++dt) { dv[dt] = v4f{0, 0, 0, 0}; dk[dt] = v4f{0, 0, 0, 0}; }
  for (int j = 0; j < nblk; ++j) {
    const char* Qi = smem + (j & 1) * 3 * SLOT;
    const char* Di = Qi + SLOT;
    const char* Oi = Di + SLOT;
    const float* lr = lraw + (j & 1) * SB;
    if (j + 1 < nblk) stage(j + 1);
    // a row's CPR chunks sit on CPR consecutive lanes (NTH and SB CPR are
    // multiples of 64): the row sum is an xor-shuffle, as in bwd_prologue
    for (int t = threadIdx.x; t < SB * CPR; t += NTH) {
      const int row = t / CPR, cc = t % CPR;
      float d = chunk_dot<bf16_t>(*(const v4u*)(Di + I::chunk(row, cc)), *(const v4u*)(Oi + I::chunk(row, cc)));
#pragma unroll
      for (int o = 1; o < CPR; o <<= 1) d += __shfl_xor(d, o, 64);
      if (cc == 0) {
        Dv[row] = -d;
        L2[row] = j * SB + row < n ? -lr[row] * inv_c : -1.0e30f;
      }
    }
    lds_barrier();
    if (active) {
      for (int qc = 0; qc < SB && j * SB + qc < n; qc += 32) {
        v4f P[2], dS[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int q0 = qc + 16 * u;
          // row constants as the initial accumulators: s' = S - lse/c, dp' = dP - Dv
          v4f s = *(const v4f*)(L2 + q0 + 4 * g), dp = *(const v4f*)(Dv + q0 + 4 * g);
#pragma unroll
          for (int ks = 0; ks < HD / 32; ++ks) {
            RowFrag<bf16_t, HD> qf, df;
            qf.lds(Qi, q0, ks, lane);
            df.lds(Di, q0, ks, lane);
            s = mma32(qf, kf[ks], s);    // S[q=4g+i][key=lane&15]
            dp = mma32(df, vf[ks], dp);  // dP[q][key]
          }
          // padding keys only pollute their own dK/dV columns, which are never
          // stored; padding queries have p = 0 (L2 = -1e30)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            P[u][i] = __builtin_amdgcn_exp2f(s[i] * c);
            dS[u][i] = P[u][i] * dp[i];
          }
        }
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt) {
          dv[dt] = mma_rowsum<bf16_t, HD>(Di, qc, 16 * dt, P[0], P[1], dv[dt], lane);
          dk[dt] = mma_rowsum<bf16_t, HD>(Qi, qc, 16 * dt, dS[0], dS[1], dk[dt], lane);
        }
      }
    }
    ring_handover();   // also: every read of L2 / Dv is done before the next block's are written
  }
  if (kok) {
    bf16_t* rowp = (bf16_t*)a.dqkv + ((int64_t)b * n + key) * a.ld_dqkv + h * HD;
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) {
      st4<bf16_t>(rowp + HH + 16 * dt + 4 * g, dk[dt] * a.scale);
      st4<bf16_t>(rowp + 2 * HH + 16 * dt + 4 * g, dv[dt]);
    }
  }
}

// bias partials of the streamed backward (several workgroups per sample and
// head, so no in-kernel partial): the q slice is the column sum of the stored
// dqkv rows, the k slice identically zero, the v slice the column sum of dO
// (sum over keys of dV = sum over queries of dO: softmax rows sum to 1).
// One thread per column, rows in order: deterministic.
__global__ void __launch_bounds__(256) attn_stream_colsum_kernel(const maeclip_attn_args a, int HH) {
  const int b = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
  if (col >= 3 * HH) return;
  float s = 0.f;
  if (col < HH) {
    const bf16_t* p = (const bf16_t*)a.dqkv + (int64_t)b * a.n * a.ld_dqkv + col;
    for (int r = 0; r < a.n; ++r) s += bf2f(p[(int64_t)r * a.ld_dqkv]);
  } else if (col >= 2 * HH) {
    const bf16_t* p = (const bf16_t*)a.dout + (int64_t)b * a.n * a.ld_o + (col - 2 * HH);
    for (int r = 0; r < a.n; ++r) s += bf2f(p[(int64_t)r * a.ld_o]);
  }
  a.colsum_partial[(int64_t)b * 3 * HH + col] = s;
}

// the route has checked the mask / dropout and 2 GiB span rejections
template <int HD>
int run_stream(const maeclip_attn_args& a, bool bwd, int nw, hipStream_t s) {
  const int tiles = (a.n + 15) / 16;
  const int64_t nwg = (int64_t)a.B * a.H * ((tiles + nw - 1) / nw);
  const dim3 grid((unsigned)nwg), block(64 * nw);
  constexpr size_t slot = (size_t)SB * Img<bf16_t, HD>::ROWB;
  if (!bwd) {
    hipLaunchKernelGGL(attn_fwd_stream_kernel<HD>, grid, block, 4 * slot + SB * 4, s, a);
    MC_CHECK_LAUNCH("maeclip_attn_fwd(streamed)");
    return 0;
  }
  hipLaunchKernelGGL(attn_bwd_stream_dq_kernel<HD>, grid, block, 4 * slot, s, a);
  hipLaunchKernelGGL(attn_bwd_stream_dkv_kernel<HD>, grid, block, 6 * slot + 4 * SB * 4, s, a);
  if (a.colsum_partial) {
    const int HH = a.H * HD;
    hipLaunchKernelGGL(attn_stream_colsum_kernel, dim3((unsigned)((3 * HH + 255) / 256), (unsigned)a.B), dim3(256), 0,
                       s, a, HH);
  }
  MC_CHECK_LAUNCH("maeclip_attn_bwd(streamed)");
  return 0;
}
}  // namespace

namespace maeclip {
int attn_stream(const maeclip_attn_args& a, const AttnRoute& r, hipStream_t s) {
  return a.head_dim == 64 ? run_stream<64>(a, r.bwd, r.nw, s) : run_stream<32>(a, r.bwd, r.nw, s);
}
}  // namespace maeclip
