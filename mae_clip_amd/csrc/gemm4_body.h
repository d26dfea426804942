// GEMM v4: 256x256x64 bf16 tile, 8 waves in two ping-pong groups, LDS-DMA
// prefetch kept in flight across raw barriers (the 256² 8-phase structure of
// cdna_hip_programming.md §5, restated for this library's operand layouts and
// epilogues).
//
// Geometry: waves (wm, wn) = 2 x 4, each wave owns a 128 x 64 output block as
// 8 x 4 fragments of 16x16 (acc = 128 VGPRs). A K-tile is split into four
// 16-KiB "halves" so that each half's last LDS read lands at a different phase:
//   Am0 = A rows {0-63, 128-191}  (mi = 0 sub-rows of both wave rows)
//   Am1 = A rows {64-127, 192-255}
//   Bn0 = B cols {0-31, 64-95, 128-159, 192-223} (ni = 0 sub-cols of all wn)
//   Bn1 = the other 128 columns
// Per K-tile every wave runs four phases, each one 64x32 output quadrant x K 64
// = 16 MFMA 16x16x32:
//   p0 (mi0,ni0): read A-sub0 + B-sub0     p1 (mi0,ni1): read B-sub1
//   p2 (mi1,ni1): read A-sub1              p3 (mi1,ni0): B-sub0 still in VGPRs
// so the last LDS reads are Am0,Bn0 @p0, Bn1 @p1, Am1 @p2.
// DMA schedule (2 glds per wave per phase = one half):
//   p0 of tile t issues half Am1 of tile t+1;  p1,p2,p3 issue Am0,Bn0,Bn1 of
//   tile t+2 into the buffer tile t is still being read -- each one phase after
//   that half's last read (the reads are retired by lgkmcnt(0) before the
//   barrier that ends the reading segment).
//   p3 waits vmcnt(6): everything but the three youngest halves (tile t+2's)
//   has landed, i.e. all of tile t+1, before the barrier that precedes its
//   first read.
// Ping-pong: group 1 (wm == 1) executes one extra barrier up front, so in every
// barrier-delimited segment one group issues its ds_reads/DMA while the other
// group's 16 MFMAs run (one wave of each group per SIMD).
//
// The layout / epilogue values, their host dispatch and the RC swizzle come
// from gemm_common.h; the epilogue (epilogue4: LDS-transposed 16-row chunks
// with prefetch rings) is this file's own.
//
// This header is the device code of the family: tile geometry, fragment
// readers, quad_mma, epilogue4, the split fix-up, the grouped problem list and
// gemm4_body. Three translation units instantiate it: gemm4.hip (dense bf16),
// gemm4_fp8.hip (fp8 rows / fp8 blocks) and gemm4_wgrad.hip (grouped weight
// gradients); their launch plans come from gemm4_plan.h.
//
// Compile-time switches (both off in the library that ships):
//   GEMM4_STAMPS   diagnostic build: s_memtime stamps per tile of the dense
//                  bf16 kernels, read back by maeclip_debug_gemm4_stamps
//                  (gemm4.hip; tools/gemm4_variant.sh, tools/stamp_run.py)
//   GEMM4_DEV_SUBSET / GEMM4_DEV_EPI   one epilogue (GEMM4_DEV_EPI, default
//                  none) instead of all six, for the register / ISA inspection
//                  build of tools/isa_gemm4.sh
#pragma once
#include "gemm4_plan.h"

namespace {

#ifdef GEMM4_STAMPS
__device__ uint64_t g_stamps[256 * 8 * 2 * 4];
#endif

constexpr int HALF = 16384;          // bytes per half image (128 rows/cols x 64 k x bf16)
// BM = 192 (plain launches, KC A operand): 96-row A halves (12 KiB), waves own
// 96 x 64 output blocks (3 x 4 fragments per quadrant row), 6 row fragments;
// chosen when it needs fewer full-tile rounds of the grid (encoder N = 768
// shapes: 201 tiles of 192 x 256 instead of 150 of 256 x 256 on 256 CUs)
template <int BM> struct TileM {
  static constexpr int MI = BM / 64;                 // A fragments per wave per half
  static constexpr int HALF_A = BM / 2 * 128;        // bytes per A half image
  static constexpr int BUF_T = 2 * HALF_A + 2 * HALF;
  static constexpr int LDS_T = 2 * BUF_T;                      // operand stages
  // BM = 192: fp8-blocks A scales, one 1 KiB image per K-tile stage (the 3
  // 64-row groups of the tile + a dummy slot, 256 B each)
  static constexpr int SC_T = BM == 192 ? 2048 : 0;
  static constexpr int SCR_OFF = LDS_T + SC_T;
  static constexpr int LDS_ALL = SCR_OFF + 8 * 4096;             // + epilogue scratch (8 waves x 4 KiB)
  __device__ static __forceinline__ int hoff(int h) { return h < 2 ? h * HALF_A : 2 * HALF_A + (h - 2) * HALF; }
};
static_assert(TileM<256>::LDS_ALL == maeclip::gemm4_lds_bytes(256) && TileM<192>::LDS_ALL == maeclip::gemm4_lds_bytes(192) &&
                  TileM<128>::LDS_ALL == maeclip::gemm4_lds_bytes(128),
              "gemm4_plan.h states the LDS bytes of a tile height");

// local index l (0..127) of a half -> offset inside the 256-wide block tile
// (BM = 192: local row l of a 96-row half; BM = 128: of a 64-row half; the
// wave row group wm owns rows [BM/2 wm, BM/2 (wm + 1)), half `sub` its
// sub-rows BM/4 sub .. +BM/4)
template <int BM = 256>
__device__ __forceinline__ int amap(int l, int sub) {
  if constexpr (BM == 256) return (l & 63) + ((l >> 6) << 7) + (sub << 6);
  else return (l % (BM / 4)) + (l / (BM / 4)) * (BM / 2) + sub * (BM / 4);
}
__device__ __forceinline__ int bmap(int l, int sub) { return (l & 31) + ((l >> 5) << 6) + (sub << 5); }

// Operand DMA through buffer descriptors (buffer_load_dwordx4 ... lds): the
// tile base and extent live in SGPRs, the per-lane byte offsets of the two
// wave-instructions this wave issues per half are loop invariants (8 VGPRs for
// both operands), and the K-tile advance is the scalar soffset. Rows (KC) past
// the operand's end read as zero through the descriptor's range check, so no
// clamping is needed; RC columns past N read neighbouring (finite) data whose
// results are never stored.
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ rsrc_t make_rsrc(const char* base, int64_t bytes) {
  const int nrec = (int)(bytes < 0x7fffffff ? (bytes > 0 ? bytes : 0) : 0x7fffffff);
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, nrec, 0x00020000);
}

// per-lane byte offset of wave-instruction i (0, 1) of half `sub` (0, 1) of an operand
template <int LAY, bool ISA, int ESZ = 2, int BM = 256>
__device__ __forceinline__ int half_voffset(int64_t ld, int sub, int i, int wave, int lane) {
  const int q = i * 8 + wave;
  if (LAY == LAY_KC) {
    const int r = q * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int g = ISA ? amap<BM>(r, sub) : bmap(r, sub);
    return (int)(g * ld * ESZ) + c * 16;
  } else {
    const int kr = q * 4 + (lane >> 4);
    const int c = (lane & 15) ^ (swz_rc(kr) >> 1);
    const int g = ISA ? amap(c * 8, sub) : bmap(c * 8, sub);
    return (int)(kr * ld * 2) + g * 2;
  }
}

// One half = 16 wave-instructions of 1 KiB; this wave issues 2 of them.
__device__ __forceinline__ void issue_half(rsrc_t rs, int v0, int v1, int soff, char* lds, int wave) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(lds + wave * 1024), 16, v0, soff, 0, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(lds + (8 + wave) * 1024), 16, v1, soff, 0, 0);
}

template <int LAY>
__device__ __forceinline__ v8s frag(const char* lds, int rs, int ks, int lane) {
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
      const char* a = lds + krow * 256 + ((unit ^ swz_rc(krow)) << 3);
      v4s t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(v4s, a));
      v[4 * h + 0] = t[0];
      v[4 * h + 1] = t[1];
      v[4 * h + 2] = t[2];
      v[4 * h + 3] = t[3];
    }
    return v;
  }
}

// p1 / p2 reads (Bn1, Am1) are restaged two phases after they are read, so
// they need not be retired before the barrier that ends their segment
// (cdna_hip_programming.md §5, 256^2 template, WAR rule). Leaving their wait
// to the compiler's, right before the first MFMA that uses them, was tried and
// not kept (within 1 % on every shape, profiles/r05/gemm_latelgkm_ab_r5m.txt):
// all three reading phases wait with lgkmcnt(0) before their barrier.

#define SEG_BARRIER()                       \
  do {                                       \
    asm volatile("" ::: "memory");           \
    __builtin_amdgcn_sched_barrier(0);       \
    __builtin_amdgcn_s_barrier();            \
    __builtin_amdgcn_sched_barrier(0);       \
    asm volatile("" ::: "memory");           \
  } while (0)

// The 16 MFMAs of one quadrant: rows i0.. of acc (4 A fragments), columns j0..
// (2 B fragments). Each operand fragment is two 16-B LDS chunks of a row (k
// chunks g and 4 + g of the 128-byte K-tile row). bf16: two 16x16x32 MFMAs
// (ks = 0, 1). fp8 (F8 = 1: A e4m3, F8 = 2: A e5m2; B e4m3): the same 32 bytes
// are one 16x16x128 block-scaled MFMA operand (all block scales 2^0; the
// per-row / per-column dequantisation scales are applied in the epilogue). A
// and B fragments put identical k's at identical lane/byte positions, so the
// hardware's k order inside the 128 need not be known.
__device__ __forceinline__ v8i cat_frag(v8s a, v8s b) {
  const v4i x = __builtin_bit_cast(v4i, a), y = __builtin_bit_cast(v4i, b);
  return __builtin_shufflevector(x, y, 0, 1, 2, 3, 4, 5, 6, 7);
}
// Keep a quadrant's MFMAs inside their segment: an empty asm that reads and
// writes the quadrant's accumulators cannot be reordered with the asm barrier
// that follows, so every MFMA of the cluster is emitted before it. Without
// it hipcc (ROCm 7.2) moved 10 of the 16 MFMAs of p0 and of p1 past the
// segment's closing s_barrier into the next read segment (tools/isa_gemm4.sh
// + the per-segment MFMA count), undoing the ping-pong. Pinning was measured
// against that schedule (profiles/r05/gemm_pin_ab_r5n.txt): every plain shape
// 1.02-1.17x (4096^3 1109 -> 1292 TF/s), the C2 step 9963 -> 10221 img/s. The
// grouped weight-gradient body pins p0 and p1 only: all four phases made its
// RC x RC fragment addresses spill inside the K loop (2790 instead of 2450 us
// per launch); p0 + p1 (the two clusters the compiler split) alone kept every
// cluster whole with the unpinned body's spills (one scratch reload per
// K-tile): step 10150 -> 10254 img/s on one box
// (profiles/r05/step_pinmask_ab_r5p.txt).
template <int MI>
__device__ __forceinline__ void pin_quad(v4f (&acc)[2 * MI][4], int i0, int j0) {
#pragma unroll
  for (int i = 0; i < MI; ++i) asm volatile("" : "+v"(acc[i0 + i][j0]), "+v"(acc[i0 + i][j0 + 1]));
}

// F8 = 3 / 4 (fp8-blocks A, e4m3 / e5m2): the A fragment i of the half takes
// its e8m0 block scale from byte i of `sc` (the MFMA's scale byte select), B's
// scale is 2^0 (its per-column scale is applied in the epilogue). Measured
// operand layout of the 16x16x128 form (tools/mfma_scale_probe.py,
// profiles/r06/mfma_scale_probe.json): lane group g holds K [16 g, 16 g + 16)
// in its first four VGPRs and K [64 + 16 g, ...) in the last four -- the two
// 16-B chunks g and 4 + g of the K-tile row that frag() reads -- and the scale
// of lane l applies to row l % 16 and K-block l / 16 = K [32 (l / 16), +32):
// a K-block's 32 elements sit in two lane groups, its scale in a third lane's
// VGPR, which is what the scale tensor's layout hands each lane.
template <int AF, int I>
__device__ __forceinline__ v4f mfma_blk(v8i b, v8i a, v4f c, unsigned sc) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, c, 0, AF, 0, 127, I, (int)sc);
}
template <int F8, int MI>
__device__ __forceinline__ void quad_mma(v4f (&acc)[2 * MI][4], int i0, int j0, const v8s (&fbq)[2][2],
                                         const v8s (&fa)[MI][2], unsigned sc = 0) {
  if constexpr (F8 >= 3) {
    constexpr int AF = F8 == 4 ? 1 : 0;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const v8i a8 = cat_frag(fa[i][0], fa[i][1]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const v8i b8 = cat_frag(fbq[j][0], fbq[j][1]);
        v4f& c = acc[i0 + i][j0 + j];
        switch (i) {
          case 0: c = mfma_blk<AF, 0>(b8, a8, c, sc); break;
          case 1: c = mfma_blk<AF, 1>(b8, a8, c, sc); break;
          case 2: c = mfma_blk<AF, 2>(b8, a8, c, sc); break;
          default: c = mfma_blk<AF, 3>(b8, a8, c, sc); break;
        }
      }
    }
  } else if constexpr (F8 == 0) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i0 + i][j0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fbq[j][ks], fa[i][ks], acc[i0 + i][j0 + j], 0, 0, 0);
  } else {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const v8i a8 = cat_frag(fa[i][0], fa[i][1]);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i0 + i][j0 + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            cat_frag(fbq[j][0], fbq[j][1]), a8, acc[i0 + i][j0 + j], 0, F8 == 2 ? 1 : 0, 0, 127, 0, 127);
    }
  }
}

// Epilogue. Fragment (i, j) of the wave covers rows m0 + 128 wm + 64 (i>>2) +
// 16 (i&3) and columns n0 + 64 wn + 32 (j>>1) + 16 (j&1); the MFMA leaves lane
// l with C[row l&15][4 (l>>4) .. +3] of each fragment. A permlane16 swap of the
// column pair (2 ni, 2 ni + 1) hands every lane 8 CONSECUTIVE columns of one
// fragment (lane group g: fragment g&1, columns 8 (g>>1) .. +7), so a row
// segment is one 16-B access per lane (bf16) instead of two 8-B ones
// (cdna_hip_programming.md T21).
//
// vmcnt is in-order on CDNA: a load issued after a store can only be waited
// for together with that store. So every load (bias, aux, resid) of a chunk of
// two row fragments is issued BEFORE the stores of the previous chunk, and the
// stores themselves are never waited for here (they drain behind the next
// tile's main loop, see the counted wait at the tile start).
template <int NI8 = 8>
__device__ __forceinline__ void swap_pairs(v4f (&acc)[NI8][4]) {
#pragma unroll
  for (int i = 0; i < NI8; ++i)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i][2 * ni][r]),
                                                  __float_as_uint(acc[i][2 * ni + 1][r]), false, false);
        acc[i][2 * ni][r] = __uint_as_float(p[0]);
        acc[i][2 * ni + 1][r] = __uint_as_float(p[1]);
      }
}

// split-K slab: fp32 partial of this K slice (dense [M, N]), no epilogue
__device__ __forceinline__ void epilogue4_slab(float* __restrict__ slab, int M, int N, float alpha, v4f (&acc)[8][4],
                                               int m0, int n0, int wm, int wn, int lane) {
  const int g = lane >> 4;
  swap_pairs(acc);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + 128 * wm + 64 * (i >> 2) + 16 * (i & 3) + (lane & 15);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int n = n0 + 64 * wn + 32 * ni + 16 * (g & 1) + 8 * (g >> 1);
      if (m < M && n < N) {
        float* d = slab + (int64_t)m * N + n;
        *(v4f*)d = acc[i][2 * ni] * alpha;
        *(v4f*)(d + 4) = acc[i][2 * ni + 1] * alpha;
      }
    }
  }
}

// whole 256x256 fp32 tile (stream-K partial) into a dense slot [256][256]
__device__ __forceinline__ void epilogue4_tile(float* __restrict__ t, v4f (&acc)[8][4], int wm, int wn, int lane) {
  const int g = lane >> 4;
  swap_pairs(acc);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ml = 128 * wm + 64 * (i >> 2) + 16 * (i & 3) + (lane & 15);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      float* d = t + ml * 256 + 64 * wn + 32 * ni + 16 * (g & 1) + 8 * (g >> 1);
      *(v4f*)d = acc[i][2 * ni];
      *(v4f*)(d + 4) = acc[i][2 * ni + 1];
    }
  }
}

// Epilogue in full-line row layout. The MFMA fragments (16 rows x 16 columns,
// 4 consecutive columns per lane) would be stored / loaded as 16 rows x 64 B
// per wave-instruction; tools/micro/store_layout.hip measured 2.3x the
// per-CU rate for whole 128-B lines (8 rows x 128 B per instruction: 12.4 vs
// 28.8 us for the same bytes on 64 CUs, loads alike), and the epilogue of
// this kernel is bound by its CU's memory-instruction rate
// (tools/gemm_grid_scan.py). So each 16-row chunk of the wave's 64-column
// block goes through a 4 KiB per-wave LDS scratch (beside the operand stages:
// the next tile's DMA is in flight in those) and comes back row-major:
//   bf16 output (L8): lane -> row lane / 8 (+ 8 q), columns 8 (lane % 8) .. +7
//                     = 16 B per lane, 8 rows x 128 B per instruction
//   f32 output  (L4): lane -> row lane / 16 (+ 4 q), columns 4 (lane % 16) .. +3
//                     = 16 B per lane, 4 rows x 256 B per instruction
// and every epilogue operand (bias, aux, residual, C for beta, aux_out) is
// read / written in that layout. Scratch: 16 rows x 256 B, 16-B unit u of
// row r at unit u ^ r (conflict-free for the fragment writes and both read
// layouts). The wave reads back only what it wrote (LDS is in order per wave).
//
// vmcnt is in-order on CDNA: a load issued after a store can only be waited
// for together with that store. So every load (aux, resid) of a chunk is
// issued BEFORE the stores of the previous chunk, and the stores themselves
// are never waited for here (they drain behind the next tile's main loop, see
// the counted wait at the tile start: 2 bf16 / 4 f32 store instructions per
// chunk, as many more for the GELU epilogues' aux_out).
//
// sa / sb (fp8 only): per-row dequantisation scale of A [M] and per-column
// scale of B [N]; the product scales the accumulator before alpha / bias.
constexpr int EPI_SCR = 4096;   // bytes of epilogue scratch per wave
// epilogue streams (aux / residual reads, C / aux_out writes) touch each byte
// once: non-temporal loads and stores, so they do not evict the A / B panels
// the XCD's tiles share (whole-step A/B against stores only and neither:
// profiles/r04/gemm_epi_nontemporal_step_ab_r4al.txt)
__device__ __forceinline__ int scr_off(int r, int u) { return r * 256 + ((u ^ r) << 4); }

template <typename OutT, int EPI, bool F8 = false, int BM = 256>
__device__ __forceinline__ void epilogue4(const maeclip_gemm_args& args, v4f (&acc)[BM / 32][4], int64_t z, int m0,
                                          int n0, int wm, int wn, int lane, char* __restrict__ scr,
                                          const float* __restrict__ sa = nullptr,
                                          const float* __restrict__ sb = nullptr) {
  constexpr int NCH = BM / 32;               // 16-row chunks per wave: 8 (BM 256) or 6 (BM 192)
  constexpr bool L8 = sizeof(OutT) == 2;
  constexpr int RPI = L8 ? 8 : 4;            // rows per instruction
  constexpr int NQ = 16 / RPI;               // instructions per chunk
  constexpr int VPL = L8 ? 8 : 4;            // values per lane per instruction
  constexpr bool LOAD_AUX = EPI == EPI_DGELU || EPI == EPI_MUL_AUX;
  constexpr bool LOAD_RES = EPI == EPI_RESID || EPI == EPI_DGELU || EPI == EPI_MUL_AUX;
  const int M = (int)args.M, N = (int)args.N;
  const int g = lane >> 4;
  swap_pairs(acc);
  const int64_t off = z * args.strideC;
  OutT* __restrict__ C = (OutT*)args.C + off;
  const float alpha = args.alpha, beta = args.beta;
  const bool has_res = LOAD_RES && args.resid != nullptr;
  const int lr = L8 ? lane >> 3 : lane >> 4;                    // row of the lane within an instruction
  const int n = n0 + 64 * wn + (L8 ? 8 * (lane & 7) : 4 * (lane & 15));
  const bool nok = n < N;                                        // N % 8 == 0 on this path
  const int nc = nok ? n : N - VPL;
  const int rbase = m0 + (BM / 2) * wm + lr;                     // + 16 c + RPI q
  float bias[VPL], csc[VPL];
#pragma unroll
  for (int v = 0; v < VPL; v += 4) {
    const v4f bv = args.bias ? *(const v4f*)(args.bias + nc + v) : v4f{0.f, 0.f, 0.f, 0.f};
    const v4f sv = F8 ? *(const v4f*)(sb + nc + v) : v4f{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bias[v + r] = bv[r];
      csc[v + r] = sv[r] * alpha;
    }
  }
  // aux / residual of chunk c + PF - 1 issued before chunk c is finished;
  // both rings are two chunks deep (a deeper aux ring, 8 VGPRs a chunk, was
  // measured and not kept: profiles/r05/aux_ring_step_ab_r5aa.txt)
  constexpr int PF = 2;
  constexpr int PFA = LOAD_AUX ? 2 : 1;
  typedef unsigned int auxv_t __attribute__((ext_vector_type(L8 ? 4 : 2)));
  auxv_t ax[PFA][NQ];
  v4f rs[PF][NQ][VPL / 4];
  auto load_aux = [&](int c) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int m = min(rbase + 16 * c + RPI * q, M - 1);
      ax[c % PFA][q] = __builtin_nontemporal_load((const auxv_t*)((const bf16_t*)args.aux + off + (int64_t)m * args.ldaux + nc));
    }
  };
  auto load_res = [&](int c) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int m = min(rbase + 16 * c + RPI * q, M - 1);
      const float* rp = args.resid + off + (int64_t)m * args.ldr + nc;
#pragma unroll
      for (int v = 0; v < VPL / 4; ++v) rs[c % PF][q][v] = __builtin_nontemporal_load((const v4f*)(rp + 4 * v));
    }
  };
  float csum[VPL];
#pragma unroll
  for (int v = 0; v < VPL; ++v) csum[v] = 0.f;
  if constexpr (LOAD_AUX) {
#pragma unroll
    for (int c = 0; c < PFA - 1; ++c) load_aux(c);
  }
  if (LOAD_RES && has_res) {
#pragma unroll
    for (int c = 0; c < PF - 1; ++c) load_res(c);
  }
  // fragment -> scratch offsets of this lane (row lane & 15; units 8 ni + 4 (g & 1) + 2 (g >> 1) + e)
  int wo[4];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int e = 0; e < 2; ++e) wo[2 * ni + e] = scr_off(lane & 15, 8 * ni + 4 * (g & 1) + 2 * (g >> 1) + e);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (LOAD_AUX && c + PFA - 1 < NCH) load_aux(c + PFA - 1);
    if (LOAD_RES && has_res && c + PF - 1 < NCH) load_res(c + PF - 1);
    __builtin_amdgcn_sched_barrier(0);   // keep chunk c+1's loads ahead of chunk c's stores
#pragma unroll
    for (int j = 0; j < 4; ++j) *(v4f*)(scr + wo[j]) = acc[c][j];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int R = lr + RPI * q;           // row within the chunk
      const int m = rbase + 16 * c + RPI * q;
      float x[VPL];
#pragma unroll
      for (int v = 0; v < VPL / 4; ++v) {
        const v4f t = *(const v4f*)(scr + scr_off(R, L8 ? 2 * (lane & 7) + v : (lane & 15)));
#pragma unroll
        for (int r = 0; r < 4; ++r) x[4 * v + r] = t[r];
      }
      const float rsc = (F8 && sa) ? sa[min(m, M - 1)] : 1.f;   // fp8-blocks A: scaled in the MFMA
#pragma unroll
      for (int v = 0; v < VPL; ++v) x[v] = F8 ? fmaf(x[v] * rsc, csc[v], bias[v]) : fmaf(x[v], alpha, bias[v]);
      const bool ok = m < M && nok;
      if (EPI == EPI_GELU || EPI == EPI_GELU_D) {
        float d[VPL];   // GELU: aux_out <- pre-activation; GELU_D: aux_out <- gelu'(pre)
        mc_f32x2 xv[VPL / 2], yv[VPL / 2], dv[VPL / 2];   // value pairs: packed f32 math
#pragma unroll
        for (int v = 0; v < VPL; v += 2) xv[v / 2] = mc_f32x2{x[v], x[v + 1]};
        gelu_pairs<VPL / 2>(xv, yv, dv);
#pragma unroll
        for (int v = 0; v < VPL; v += 2) {
          d[v] = EPI == EPI_GELU_D ? dv[v / 2][0] : x[v];
          d[v + 1] = EPI == EPI_GELU_D ? dv[v / 2][1] : x[v + 1];
          x[v] = yv[v / 2][0];
          x[v + 1] = yv[v / 2][1];
        }
        if (args.aux_out && ok) {
          bf16_t* ap = (bf16_t*)args.aux_out + off + (int64_t)m * args.ldaux + n;
          if (L8) {
            const v4u pk = {pack2bf(d[0], d[1]), pack2bf(d[2], d[3]), pack2bf(d[4 % VPL], d[5 % VPL]),
                            pack2bf(d[6 % VPL], d[7 % VPL])};
            __builtin_nontemporal_store(pk, (v4u*)ap);
          } else {
            const v2u pk = {pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
            __builtin_nontemporal_store(pk, (v2u*)ap);
          }
        }
      }
      if (LOAD_AUX) {
        const auxv_t pk = ax[c % PFA][q];
#pragma unroll
        for (int r = 0; r < VPL / 2; ++r) {
          const float a0 = __uint_as_float(pk[r] << 16), a1 = __uint_as_float(pk[r] & 0xffff0000u);
          if (EPI == EPI_MUL_AUX) {
            x[2 * r] *= a0;
            x[2 * r + 1] *= a1;
          } else {
            x[2 * r] *= gelu_grad_f(a0);
            x[2 * r + 1] *= gelu_grad_f(a1);
          }
        }
      }
      if (LOAD_RES && has_res) {
#pragma unroll
        for (int v = 0; v < VPL; ++v) x[v] += rs[c % PF][q][v / 4][v % 4];
      }
      if (L8 && args.q8) {
        // fp8-blocks copy of the bf16 row segment as stored (maeclip.h q8):
        // a 32-column block is the lane quad 4k .. 4k + 3 (8 columns each)
        float xs[VPL], am = 0.f;
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
          xs[v] = bf2f(f2bf(x[v]));
          am = fmaxf(am, fabsf(xs[v]));
        }
        am = fmaxf(am, dpp_mov<0xB1>(am));
        am = fmaxf(am, dpp_mov<0x4E>(am));
        const bool e5 = args.q8_fmt == MAECLIP_FP8_E5M2;
        const unsigned ex = mc_e8m0(am, e5);
        const float inv = mc_e8m0_inv(ex);
#pragma unroll
        for (int v = 0; v < VPL; ++v) xs[v] *= inv;
        if (ok) {
          v2u o;
          if (e5) {
            o[0] = mc_cvt4_fp8<true>(xs[0], xs[1], xs[2], xs[3]);
            o[1] = mc_cvt4_fp8<true>(xs[4 % VPL], xs[5 % VPL], xs[6 % VPL], xs[7 % VPL]);
          } else {
            o[0] = mc_cvt4_fp8<false>(xs[0], xs[1], xs[2], xs[3]);
            o[1] = mc_cvt4_fp8<false>(xs[4 % VPL], xs[5 % VPL], xs[6 % VPL], xs[7 % VPL]);
          }
          __builtin_nontemporal_store(o, (v2u*)((uint8_t*)args.q8 + (int64_t)m * args.ldq8 + n));
          if ((lane & 3) == 0) args.q8_scale[mc_fp8b_off(m, n >> 5, N >> 7)] = (uint8_t)ex;
        }
      }
      if (ok) {
        OutT* cp = C + (int64_t)m * args.ldc + n;
        if (beta != 0.f) {
#pragma unroll
          for (int v = 0; v < VPL; v += 4) {
            const v4f cv = ld4<OutT>(cp + v);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[v + r] += beta * cv[r];
          }
        }
#pragma unroll
        for (int v = 0; v < VPL; ++v) csum[v] += x[v];
        if (L8) {
          const v4u pk = {pack2bf(x[0], x[1]), pack2bf(x[2], x[3]), pack2bf(x[4 % VPL], x[5 % VPL]),
                          pack2bf(x[6 % VPL], x[7 % VPL])};
          __builtin_nontemporal_store(pk, (v4u*)cp);
        } else {
          __builtin_nontemporal_store((v4f{x[0], x[1], x[2], x[3]}), (v4f*)cp);
        }
      }
    }
    if (BM == 256 && (c & 3) == 3 && args.colsum_partial) {   // one partial row per 64-row group
      // the lanes holding the same columns: L8 lanes k + 8 j (row_ror 8 inside
      // each 16-lane row, then the four rows), L4 lanes u + 16 j (the four rows)
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        float t = csum[v];
        if (L8) t += dpp_mov<0x128>(t);
        const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(t), __float_as_uint(t), false, false);
        t = __uint_as_float(p[0]) + __uint_as_float(p[1]);
        const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t), __float_as_uint(t), false, false);
        csum[v] = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
      }
      const int mrow = m0 + 128 * wm + 64 * (c >> 2);
      if (lane < (L8 ? 8 : 16) && mrow < M && nok) {
        float* prow = args.colsum_partial + ((int64_t)z * ((M + 63) / 64) + mrow / 64) * N + n;
#pragma unroll
        for (int v = 0; v < VPL; v += 4) *(v4f*)(prow + v) = v4f{csum[v], csum[v + 1], csum[v + 2], csum[v + 3]};
      }
#pragma unroll
      for (int v = 0; v < VPL; ++v) csum[v] = 0.f;
    }
  }
}

// One unit of work of the persistent loop: a 256x256 output tile of one
// problem and its K range (a split-K slice or the whole K).
struct Unit4 {
  const char* A;
  const char* B;
  int64_t lda, ldb;
  int M, N, K;        // problem sizes (K = full reduction length)
  int m0, n0;
  int kbeg, nt;       // first k and number of 64-wide K-tiles of this unit
  int slice, prob;
  int slot;           // stream-K partial tile: workspace slot; -1 = final result
  int tl;             // stream-K: remainder tile index
};

// Split plan of a plain launch (maeclip_gemm with a workspace): every tile's
// K range is cut into S slices, one unit per (tile, slice), units tile-major
// and dealt out in XCD-contiguous chunks of the persistent grid, so a launch
// with fewer tiles than CUs still fills the chip (the micro-batch's 6400-row
// encoder shapes: 75 tiles of 256 x 256 for 256 CUs) and the blocks on one XCD
// work the same K-range of neighbouring tiles at the same time, sharing A rows
// / B columns in its L2. (Stream-K ranges -- every block an equal run of
// K-tiles across tile boundaries -- start every block at a different K and
// lose that reuse: 2.5x the K-tile time, profiles/r05/stream_k_diag_r5c.jsonl;
// removed.) The slices of a tile are summed IN THE SAME LAUNCH by the block
// that arrives last (sk_fixup): no second launch, no waiting, a fixed
// summation order. Slice 0 is the longest, by `lead` K-tiles per other slice
// (L0 = ceil((NT + (S - 1) lead) / S), the rest split evenly): the other
// slices finish first and publish while slice 0 still computes, so slice 0
// usually finds them all published and sums without publishing its own.
// Workspace: [SK_CNT_BYTES] arrival counters (zero before the first launch,
// left zero by every completed launch), then one SK_SLOT partial per unit
// (slot t * S + s), at most 2 per CU (the constants: gemm4_plan.h).
struct SkPlan {
  int NT;             // K-tiles of the whole K
  int S;              // slices per tile (0: no split)
  int L0;             // K-tiles of slice 0 (the others share NT - L0)
  int nsl;            // fp32 256x256 slots in the workspace
  unsigned* cnt;
  float* slots;
};
struct Gemm4Args {
  maeclip_gemm_args a;
  SkPlan sk;
  const float* sa;    // fp8 only: per-row A / per-column B dequantisation scales
  const float* sb;
  const uint8_t* sab; // fp8-blocks A: e8m0 block scales (common.h mc_fp8b_off layout)
};

// Fix-up of one split tile (slice u.slot of S = 2): returns true in the block
// that arrives last, whose acc then holds the whole tile's sum and which runs
// the epilogue. Hand-off (MI355X_MICROARCH.md, publish-large / handoff-payload):
// every slice but the last to arrive is stored write-through (16-B sc1
// stores), each storing wave drains with vmcnt(0), a workgroup barrier, then
// ONE lane adds to the tile's agent-scope counter; the block whose add returns
// S - 1 (or whose poll already reads S - 1 and so skips its own store: slice
// 0, by its lead) reads the other slices with sc1 loads only. The summation
// order is fixed by slice index whichever block reduces: ((p0 + p1) + p2),
// the reducer's own partial entering at its position, so the output bits do
// not depend on arrival order (p0 + p1 == p1 + p0). Slot layout is fragment-native (the accumulator
// registers as they stand, 1 KiB per wave-instruction): [wave][row
// fragment][col fragment][lane] x 16 B.
template <int NF>
__device__ __forceinline__ bool sk_fixup(v4f (&acc)[NF][4], const SkPlan& sk, const Unit4& u, int* flag, int tid,
                                         int wave, int lane) {
  const int np = sk.S, r = u.slot;
  unsigned* cnt = sk.cnt + u.tl * SK_CNT_STRIDE;
  const unsigned last_count = (unsigned)(np - 1);
  const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)sk.slots, (short)0, (int)((int64_t)sk.nsl * SK_SLOT),
                                                      0x00020000);
  const int vo = lane * 16 + wave * NF * 4 * 1024;
  const int sbase = u.tl * np * (int)SK_SLOT;
  if (tid == 0) *flag = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == last_count ? 1 : 0;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  SEG_BARRIER();
  bool last = *flag == 1;
  if (!last) {
    const int so = sbase + r * (int)SK_SLOT;
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, acc[i][j]), rs, vo, so + (i * 4 + j) * 1024, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SEG_BARRIER();
    if (tid == 0)
      *flag = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == last_count ? 1 : 2;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    SEG_BARRIER();
    last = *flag == 1;
  }
  if (!last) return false;
  auto ld4 = [&](int p, int i, v4f (&L)[4]) {
    const int so = sbase + p * (int)SK_SLOT;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      L[j] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so + (i * 4 + j) * 1024, 16));
  };
  // (the per-fragment offset rides in the scalar soffset: as a per-lane
  // voffset it would take one VGPR per fragment, past the immediate's range)
  // S = 2: the other slice's two row fragments at a time, 8 16-B loads per
  // lane in flight (the hand-off read is latency-bound below that)
  const int o = 1 - r;
#pragma unroll
  for (int i = 0; i < NF; i += 2) {
    v4f L[2][4];
    ld4(o, i, L[0]);
    ld4(o, i + 1, L[1]);
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i + ii][j] += L[ii][j];   // p0 + p1 == p1 + p0
    // keep the next fragments' loads below this sum: hoisted, they would
    // hold the whole partial beside acc
    __builtin_amdgcn_sched_barrier(0);
  }
  if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// Grouped weight gradients (maeclip_wgrad_grouped): dW_p[N_p, K_p] (+)=
// dy_p[Mtok, N_p]^T x_p[Mtok, K_p] for up to WG_MAX problems in one persistent
// launch, so the 4 x layers weight-gradient GEMMs of a transformer stack share
// one grid instead of each needing an fp32 split-K slab round trip to fill the
// chip. In GEMM terms M = N_p, N = K_p, K = Mtok, both operands RC.
struct WgProb {
  const bf16_t* dy;
  const bf16_t* x;
  float* dw;
  int N, K, ldy, ldx;
  int tile_begin;     // prefix sum of tiles
  int slab_off;       // floats, S > 1 only
};
struct WgGroup {
  int np, S, T, Mtok;
  // stream-K remainder (skw > 0): tiles [0, Tdp) run whole (Tdp a multiple of
  // the grid), the K-tiles of tiles [Tdp, T) are dealt out evenly, skw per
  // block in block-position order; a tile cut between blocks leaves fp32
  // partials in 256x256 slots (2 per block) summed by wgrad4_sk_reduce_kernel
  int Tdp, skw, NT;
  float beta;
  float* ws;
  WgProb p[WG_MAX];
};

// F8: 0 = bf16 operands (K-tile 64); 1 / 2 = fp8 operands, A e4m3 / e5m2 and
// B e4m3 (K-tile 128 = the same 128 bytes per row), per-row A scales sa[M] and
// per-column B scales sb[N] applied in the epilogue.
template <int LA, int LB, typename OutT, int EPI, bool SPLIT, bool GRP, int F8 = 0, int BM = 256, bool SK = false>
__device__ __forceinline__ void gemm4_body(const maeclip_gemm_args& args, const WgGroup* __restrict__ gp,
                                           const float* __restrict__ sa = nullptr,
                                           const float* __restrict__ sb = nullptr, const SkPlan* skp_ = nullptr,
                                           const uint8_t* __restrict__ sab = nullptr) {
  static_assert(F8 == 0 || (LA == LAY_KC && LB == LAY_KC && !SPLIT && !GRP), "fp8: KC x KC plain launches only");
  // fp8-blocks A (F8 3 / 4): 192-row tiles, no split plan. The three 64-row
  // scale groups of a K-tile ride with its Bn1 half: waves 4-6 issue one
  // 256-B LDS-DMA each (wave 7 a dummy copy), so every wave keeps 6 DMA
  // instructions in the three youngest halves (waves 0-3: 2 + 2 + 2, waves
  // 4-7: 1 + 2 + 3) and one counted wait serves all.
  constexpr bool F8B = F8 >= 3;
  static_assert(!F8B || (BM == 192 && !SK), "fp8-blocks A: 192-row tiles without a split plan");
  static_assert(BM == 256 || ((BM == 192 || BM == 128) && LA == LAY_KC && !SPLIT && !GRP),
                "BM 192 / 128: KC A, plain launches only");
  static_assert(!SK || (!SPLIT && !GRP), "stream-K: plain launches only");
  using TM = TileM<BM>;
  constexpr int MI = TM::MI;
  constexpr int ESZ = F8 ? 1 : 2;      // operand bytes per element
  constexpr int KT = 128 / ESZ;        // elements per K-tile (128 bytes per row)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  char* const scr = smem + TM::SCR_OFF + wave * EPI_SCR;   // this wave's epilogue scratch
  const int64_t z = GRP ? 0 : blockIdx.z;

  // units: standard = output tiles (this block's slice is blockIdx.y);
  // grouped = slice-major (slice, tile) pairs, so neighbouring units share operands
  int T, gn = 1, klen = 0;
  if (GRP) {
    T = gp->skw > 0 ? gp->Tdp : gp->T * gp->S;
    klen = ((gp->Mtok + gp->S - 1) / gp->S + KT - 1) / KT * KT;
  } else {
    const int gm = ((int)args.M + BM - 1) / BM;
    gn = ((int)args.N + 255) / 256;
    T = gm * gn;
    const int S = SPLIT ? args.splitk : 1;
    klen = (((int)args.K + S - 1) / S + KT - 1) / KT * KT;
  }
  // stream-K remainder (grouped launches: gp): tiles [Tdp, Ttot) are dealt out
  // by K-tiles, skw per block
  int Ttot = T, Tdp = T, skw = 0, NTr = 1;
  if (GRP && gp->skw > 0) {
    Ttot = gp->T;
    Tdp = gp->Tdp;
    skw = gp->skw;
    NTr = gp->NT;
  }
  int skS = 0;   // aligned split: units = (tile, slice)
  if (SK) {
    skS = skp_->S;
    Ttot = Tdp = T = T * skS;
  }
  auto unit = [&](int u) {
    Unit4 w;
    if (GRP) {
      const int tile = u % gp->T, sl = u / gp->T;
      int p = 0;
      while (p + 1 < gp->np && gp->p[p + 1].tile_begin <= tile) ++p;
      const WgProb& q = gp->p[p];
      const int local = tile - q.tile_begin, gnp = (q.K + 255) / 256;
      w.A = (const char*)q.dy;
      w.B = (const char*)q.x;
      w.lda = q.ldy;
      w.ldb = q.ldx;
      w.M = q.N;
      w.N = q.K;
      w.K = gp->Mtok;
      w.m0 = (local / gnp) * 256;
      w.n0 = (local % gnp) * 256;
      w.slice = sl;
      w.prob = p;
    } else {
      w.A = (const char*)args.A + z * args.strideA * ESZ;
      w.B = (const char*)args.B + z * args.strideB * ESZ;
      w.lda = args.lda;
      w.ldb = args.ldb;
      w.M = (int)args.M;
      w.N = (int)args.N;
      w.K = (int)args.K;
      const int tile = skS > 0 ? u / skS : u;
      w.m0 = (tile / gn) * BM;
      w.n0 = (tile % gn) * 256;
      w.slice = skS > 0 ? u - tile * skS : (int)blockIdx.y;
      w.prob = 0;
    }
    if (SK && skS > 0) {
      // slice 0: K-tiles [0, L0); slice s >= 1: its share of the rest
      const int L0 = skp_->L0, rem = skp_->NT - L0, q = rem / (skS - 1), rr = rem % (skS - 1);
      const int s1 = w.slice - 1;
      const int kb = w.slice == 0 ? 0 : L0 + s1 * q + min(s1, rr);
      w.nt = w.slice == 0 ? L0 : q + (s1 < rr ? 1 : 0);
      w.kbeg = kb * KT;
    } else {
      w.kbeg = w.slice * klen;
      const int kend = min(w.K, w.kbeg + klen);
      w.nt = kend > w.kbeg ? (kend - w.kbeg) / KT : 0;
    }
    w.slot = skS > 0 ? w.slice : -1;   // aligned split: every unit is a piece
    w.tl = skS > 0 ? u / skS : 0;
    return w;
  };

  // Persistent over units: the units are cut into 8 contiguous chunks, chunk
  // x worked by the blocks with blockIdx.x % 8 == x (round-robin dispatch puts
  // them on one XCD, so concurrently running tiles share A rows in that XCD's
  // L2; placement is a speed assumption only).
  const int G = gridDim.x, x8 = blockIdx.x % 8, li = blockIdx.x / 8;
  const int nbx = (G - x8 + 7) / 8;
  const int cq = T / 8, cr = T % 8;
  const int cbeg = x8 < cr ? x8 * (cq + 1) : cr * (cq + 1) + (x8 - cr) * cq;
  const int cend = cbeg + cq + (x8 < cr ? 1 : 0);
  // this block's jobs: its whole tiles, then (grouped stream-K) its K range of
  // the remainder tiles
  const int ndp = cbeg + li < cend ? (cend - (cbeg + li) + nbx - 1) / nbx : 0;
  // this block's stream-K range [ska, skb) of (remainder tile, K-tile)
  // iterations: tiles t0 (from K-tile k0) .. t1 (up to K-tile k1); the
  // divisions stay out of the K loop, where job() is also called
  int nsk = 0, skp = 0, sk_t0 = 0, sk_k0 = 0, sk_t1 = 0, sk_k1 = 0;
  if (skw > 0) {
    skp = G % 8 == 0 ? x8 * (G / 8) + li : (int)blockIdx.x;   // XCD-contiguous positions
    const int tot = (Ttot - Tdp) * NTr;
    const int ska = min(skp * skw, tot), skb = min(ska + skw, tot);
    if (skb > ska) {
      sk_t0 = ska / NTr;
      sk_k0 = ska - sk_t0 * NTr;
      sk_t1 = (skb - 1) / NTr;
      sk_k1 = skb - sk_t1 * NTr;
      nsk = sk_t1 - sk_t0 + 1;
    }
  }
  auto job = [&](int j) -> Unit4 {
    if (j < ndp) return unit(cbeg + li + j * nbx);
    const int s = j - ndp, NT = NTr;
    const int tl = sk_t0 + s;
    const int k0 = s == 0 ? sk_k0 : 0;
    const int k1 = tl == sk_t1 ? sk_k1 : NT;
    Unit4 w = unit(Tdp + tl);
    w.kbeg = k0 * KT;
    w.nt = k1 - k0;
    w.slot = (k0 == 0 && k1 == NT) ? -1 : 2 * skp + (s == 0 ? 0 : 1);
    w.tl = tl;
    return w;
  };
  const int njobs = ndp + nsk;

  // per-lane DMA byte offsets of a unit's operands (loop invariants of its K loop)
  auto offsets = [&](const Unit4& w, int (&vA)[2][2], int (&vB)[2][2]) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        vA[sub][i] = half_voffset<LA, true, ESZ, BM>(w.lda, sub, i, wave, lane);
        vB[sub][i] = half_voffset<LB, false, ESZ>(w.ldb, sub, i, wave, lane);
      }
  };
  // half h of K-tile t of unit w: 0 = Am0, 1 = Am1, 2 = Bn0, 3 = Bn1. The
  // K-tile advance is along the row (KC) or down the k-rows (RC).
  auto issue = [&](const Unit4& w, const int (&vA)[2][2], const int (&vB)[2][2], int t, int h) {
    char* dst = smem + (t & 1) * TM::BUF_T + TM::hoff(h);
    const int k0 = w.kbeg + t * KT;
    if (h < 2) {
      const rsrc_t rs = LA == LAY_KC ? make_rsrc(w.A + (int64_t)w.m0 * w.lda * ESZ, ((int64_t)w.M - w.m0) * w.lda * ESZ)
                                     : make_rsrc(w.A + (int64_t)w.m0 * ESZ, ((int64_t)w.K * w.lda - w.m0) * ESZ);
      if constexpr (BM == 256) {
        issue_half(rs, vA[h][0], vA[h][1], k0 * (LA == LAY_KC ? ESZ : (int)(w.lda * ESZ)), dst, wave);
      } else {
        // a 96-row A half is 12 wave-instructions (waves 0-3 issue two, 4-7
        // one), a 64-row half 8 (one per wave)
        const int soff = k0 * ESZ;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(dst + wave * 1024), 16, vA[h][0], soff, 0, 0);
        if (BM == 192 && wave < 4)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(dst + (8 + wave) * 1024), 16, vA[h][1], soff, 0, 0);
      }
    } else {
      const rsrc_t rs = LB == LAY_KC ? make_rsrc(w.B + (int64_t)w.n0 * w.ldb * ESZ, ((int64_t)w.N - w.n0) * w.ldb * ESZ)
                                     : make_rsrc(w.B + (int64_t)w.n0 * ESZ, ((int64_t)w.K * w.ldb - w.n0) * ESZ);
      issue_half(rs, vB[h - 2][0], vB[h - 2][1], k0 * (LB == LAY_KC ? ESZ : (int)(w.ldb * ESZ)), dst, wave);
      if constexpr (F8B) {
        if (h == 3 && wave >= 4) {
          const int T8 = w.K / KT;
          const int G = w.m0 / 64 + min(wave - 4, 2);
          const rsrc_t rsc = make_rsrc((const char*)sab, mc_fp8b_bytes(w.M, w.K));
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsc, (lds_void*)(smem + TM::LDS_T + (t & 1) * 1024 + (wave - 4) * 256),
                                                   4, lane * 4, (G * T8 + w.kbeg / KT + t) * 256, 0, 0);
        }
      }
    }
  };
  // K-tile 0 whole + three halves of K-tile 1 (its Am1 follows in p0)
  auto prologue = [&](const Unit4& w) {
    int vA[2][2], vB[2][2];
    offsets(w, vA, vB);
    issue(w, vA, vB, 0, 0);
    issue(w, vA, vB, 0, 2);
    issue(w, vA, vB, 0, 3);
    issue(w, vA, vB, 0, 1);
    if (w.nt > 1) {
      issue(w, vA, vB, 1, 0);
      issue(w, vA, vB, 1, 2);
      issue(w, vA, vB, 1, 3);
    }
  };

  bool primed = false, first = true, prev_full = false;
  // everything but the three youngest halves (Am0, Bn0, Bn1 of one K-tile):
  // 2 + 2 + 2 wave-instructions, or 1 + 2 + 2 for waves 4-7 at BM 192 and
  // every wave at BM 128
  auto wait_halves = [&]() {
    if (BM == 256 || (BM == 192 && (wave < 4 || F8B))) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  };
#ifdef GEMM4_STAMPS
  // diagnostic build only: s_memtime at tile start / after the DMA wait /
  // after the K-loop / after the epilogue, waves 0 and 4 of every block
  int ntile = 0;
  const bool stamp = blockIdx.y == 0 && blockIdx.z == 0 && (wave == 0 || wave == 4) && lane == 0 && blockIdx.x < 256;
  uint64_t* sp = g_stamps + ((int64_t)blockIdx.x * 8 * 2 + (wave >> 2)) * 4;
#define STAMP(k) do { if (stamp && ntile < 8) sp[ntile * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STAMP(k) do {} while (0)
#endif
  for (int jb = 0; jb < njobs; ++jb) {
    STAMP(0);
    const Unit4 u = job(jb);
    const int m0 = u.m0, n0 = u.n0, nt = u.nt;
    int voA[2][2], voB[2][2];
    offsets(u, voA, voB);
    if (nt > 0 && !primed) prologue(u);
    if (first && nt > 1) {
      wait_halves();
    } else if (prev_full) {
      // This tile's DMA was issued before the previous tile's epilogue, whose
      // C stores (at least NST per wave for a full tile: 8 row fragments x 2
      // x 16-B, twice that for fp32) are the youngest vector-memory ops: wait
      // for everything older and let the stores drain behind this tile's
      // MFMAs instead of stalling every CU on HBM writes at once.
      // GELU epilogues with aux_out also store a bf16 pre-activation / GELU'
      // per chunk: twice the bf16 stores, all younger than this tile's DMA
      const bool two_out = (EPI == EPI_GELU || EPI == EPI_GELU_D) && args.aux_out != nullptr && !GRP;
      // an fp8-blocks copy (q8) adds two stores per bf16 store instruction
      // (the fp8 bytes, the quad's scale byte)
      const bool q8 = sizeof(OutT) == 2 && args.q8 != nullptr && !GRP;
      if (q8) {
        if (BM == 256) {
          if (two_out) asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
        } else if (BM == 128) {
          if (two_out) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
        } else {
          if (two_out) asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(36)" ::: "memory");
        }
      } else if (BM == 256) {
        if (sizeof(OutT) == 2 && two_out) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
        else if (sizeof(OutT) == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
      } else if (BM == 128) {   // 4 row fragments x 2 (bf16) or x 4 (fp32) stores
        if (sizeof(OutT) == 2 && two_out) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else if (sizeof(OutT) == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      } else if (sizeof(OutT) == 2 && two_out) {
        asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
      } else {   // 6 row fragments x 2 (bf16) or x 4 (fp32) stores
        if (sizeof(OutT) == 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
      }
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    first = false;
    prev_full = !SPLIT && m0 + BM <= u.M && n0 + 256 <= u.N;
    primed = false;
    SEG_BARRIER();
    if (wm == 1) SEG_BARRIER();
    STAMP(1);

    v4f acc[2 * MI][4];
#pragma unroll
    for (int i = 0; i < 2 * MI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

    v8s fa[MI][2], fb[2][2][2];
    // fp8-blocks: the A scale dword of half `sub` for this lane (row lane % 16,
    // block lane / 16): the 16-row groups 6 wm + 3 sub .. +2 of the tile, byte i
    // = fragment i after the byte align
    auto read_sc = [&](const char* img, int sub) -> unsigned {
      const int g16 = 6 * wm + 3 * sub;
      const int o = (lane >> 4) * 64 + (lane & 15) * 4;
      const unsigned lo = *(const unsigned*)(img + (g16 >> 2) * 256 + o);
      const unsigned hi = *(const unsigned*)(img + ((g16 + 2) >> 2) * 256 + o);
      return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)(g16 & 3));
    };
    unsigned sc0 = 0, sc1 = 0;
    for (int t = 0; t < nt; ++t) {
      const char* buf = smem + (t & 1) * TM::BUF_T;
      const char* scimg = smem + TM::LDS_T + (t & 1) * 1024;
      const char* hA0 = buf;
      const char* hA1 = buf + TM::HALF_A;
      const char* hB0 = buf + 2 * TM::HALF_A;
      const char* hB1 = hB0 + HALF;
      const bool more1 = t + 1 < nt, more2 = t + 2 < nt;
      // ---- p0: quadrant (0,0)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fb[0][j][ks] = frag<LB>(hB0, 32 * wn + 16 * j, ks, lane);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fa[i][ks] = frag<LA>(hA0, (BM / 4) * wm + 16 * i, ks, lane);
      if constexpr (F8B) sc0 = read_sc(scimg, 0);
      if (more1) issue(u, voA, voB, t + 1, 1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      SEG_BARRIER();
      __builtin_amdgcn_s_setprio(1);
      quad_mma<F8, MI>(acc, 0, 0, fb[0], fa, sc0);
      pin_quad<MI>(acc, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      SEG_BARRIER();
      // ---- p1: quadrant (0,1)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fb[1][j][ks] = frag<LB>(hB1, 32 * wn + 16 * j, ks, lane);
      if (more2) issue(u, voA, voB, t + 2, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      SEG_BARRIER();
      __builtin_amdgcn_s_setprio(1);
      quad_mma<F8, MI>(acc, 0, 2, fb[1], fa, sc0);
      pin_quad<MI>(acc, 0, 2);
      __builtin_amdgcn_s_setprio(0);
      SEG_BARRIER();
      // ---- p2: quadrant (1,1)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) fa[i][ks] = frag<LA>(hA1, (BM / 4) * wm + 16 * i, ks, lane);
      if constexpr (F8B) sc1 = read_sc(scimg, 1);
      if (more2) issue(u, voA, voB, t + 2, 2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      SEG_BARRIER();
      __builtin_amdgcn_s_setprio(1);
      quad_mma<F8, MI>(acc, MI, 2, fb[1], fa, sc1);
      if constexpr (!GRP) pin_quad<MI>(acc, MI, 2);   // grouped: p0 + p1 only (pin_quad)
      __builtin_amdgcn_s_setprio(0);
      SEG_BARRIER();
      // ---- p3: quadrant (1,0), operands already in VGPRs. Every LDS read of
      // this tile has been retired behind an earlier barrier, so the last
      // K-tile starts the next unit's DMA here.
      if (more2) {
        issue(u, voA, voB, t + 2, 3);
        wait_halves();
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (!more1 && jb + 1 < njobs) {
          const Unit4 un = job(jb + 1);
          if (un.nt > 0) {
            prologue(un);
            primed = true;
          }
        }
      }
      SEG_BARRIER();
      __builtin_amdgcn_s_setprio(1);
      quad_mma<F8, MI>(acc, MI, 0, fb[0], fa, sc1);
      if constexpr (!GRP) pin_quad<MI>(acc, MI, 0);
      __builtin_amdgcn_s_setprio(0);
      if (wm == 0 || more1) SEG_BARRIER();   // group 1 skips its very last one (it took one extra up front)
    }
    if (nt == 0 && wm == 0) SEG_BARRIER();
    STAMP(2);
    // cut tile (stream-K): the epilogue runs once, in the block that sums the
    // pieces (one epilogue call site either way). Flag word: the Am1 half of
    // LDS buffer 1, which no DMA writes before the next unit's first K-tile
    // (the prologue fills buffer 0 and the other three halves of buffer 1)
    bool run_epi = true;
    if (SK && u.slot >= 0)
      run_epi = sk_fixup<2 * MI>(acc, *skp_, u, (int*)(smem + TM::BUF_T + TM::HALF_A), tid, wave, lane);
    if (!run_epi) {
    } else if constexpr (BM != 256) {
      epilogue4<OutT, EPI, F8 != 0, BM>(args, acc, z, m0, n0, wm, wn, lane, scr, sa, sb);
    } else if (GRP) {
      const WgProb& q = gp->p[u.prob];
      if (u.slot >= 0) {
        epilogue4_tile(gp->ws + (int64_t)u.slot * 65536, acc, wm, wn, lane);
      } else if (SPLIT) {
        epilogue4_slab(gp->ws + q.slab_off + (int64_t)u.slice * q.N * q.K, q.N, q.K, 1.f, acc, m0, n0, wm, wn, lane);
      } else {
        maeclip_gemm_args ea = args;
        ea.M = q.N;
        ea.N = q.K;
        ea.C = q.dw;
        ea.ldc = q.K;
        ea.alpha = 1.f;
        ea.beta = gp->beta;
        epilogue4<OutT, EPI>(ea, acc, 0, m0, n0, wm, wn, lane, scr);
      }
    } else if (SPLIT) {
      epilogue4_slab(args.workspace + ((int64_t)z * args.splitk + blockIdx.y) * args.M * args.N, (int)args.M,
                     (int)args.N, args.alpha, acc, m0, n0, wm, wn, lane);
    } else {
      epilogue4<OutT, EPI, F8 != 0>(args, acc, z, m0, n0, wm, wn, lane, scr, sa, sb);
    }
    STAMP(3);
#ifdef GEMM4_STAMPS
    ++ntile;
#endif
  }
}

// The one launch of a planned dense / fp8 GEMM: every kernel of the two
// families takes a Gemm4Args; `kern` is the instantiation the caller picked
// for the plan's (tile height, split), `who` names it in a launch failure.
typedef void (*Gemm4Kern)(const Gemm4Args);
inline int launch_plan(const maeclip::Gemm4Plan& p, Gemm4Kern kern, const char* who, const maeclip_gemm_args& a,
                       const float* sa, const float* sb, const uint8_t* sab, hipStream_t s) {
  Gemm4Args g = {};
  g.a = a;
  g.sa = sa;
  g.sb = sb;
  g.sab = sab;
  if (p.S > 0) g.sk = {p.NT, p.S, p.L0, p.nsl, (unsigned*)a.workspace, (float*)((char*)a.workspace + SK_CNT_BYTES)};
  maeclip::allow_lds((const void*)kern, p.lds_bytes);
  hipLaunchKernelGGL(kern, dim3(p.gx, p.gy, p.gz), dim3(512), p.lds_bytes, s, g);
  MC_CHECK_LAUNCH(who);
  return 0;
}

}  // namespace
