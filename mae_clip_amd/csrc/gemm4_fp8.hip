// GEMM v4 on fp8 operands: maeclip_gemm_fp8 (per-row A scales) and
// maeclip_gemm_fp8_blocks (e8m0 block scales of A inside the MFMA), KC x KC,
// their argument checks and the device-free query maeclip_gemm_fp8_plan.
// Device code: gemm4_body.h; the launch plan: gemm4_plan.h.
#include "gemm4_body.h"

namespace {

// fp8 operands (maeclip_gemm_fp8): KC x KC, per-row / per-column scales
template <typename OutT, int EPI, int F8, int BM = 256, bool SK = false>
__global__ void __launch_bounds__(512) gemm4_f8_kernel(const Gemm4Args g) {
  gemm4_body<LAY_KC, LAY_KC, OutT, EPI, false, false, F8, BM, SK>(g.a, nullptr, g.sa, g.sb, &g.sk, g.sab);
}

template <typename OutT, int EPI, int F8>
int launch_f8(const maeclip_gemm_args& a, const float* sa, const float* sb, hipStream_t s) {
  const maeclip::Gemm4Plan p = maeclip::gemm4_plan(a, maeclip::G4_FP8_ROWS, maeclip::gemm4_device_ncu(), a.workspace != nullptr);
  Gemm4Kern kern = gemm4_f8_kernel<OutT, EPI, F8>;
  const char* who = "maeclip_gemm_fp8";
  if (p.bm == 192) {
    kern = p.S > 0 ? gemm4_f8_kernel<OutT, EPI, F8, 192, true> : gemm4_f8_kernel<OutT, EPI, F8, 192>;
    who = "maeclip_gemm_fp8(192-row tiles)";
  }
  return launch_plan(p, kern, who, a, sa, sb, nullptr, s);
}

template <typename OutT, int F8>
int epi_f8(const maeclip_gemm_args& a, const float* sa, const float* sb, hipStream_t s) {
#ifdef GEMM4_DEV_SUBSET
  return launch_f8<OutT, EPI_NONE, F8>(a, sa, sb, s);
#else
  return dispatch_epilogue(a, "maeclip_gemm_fp8",
                           [&](auto epi) { return launch_f8<OutT, decltype(epi)::value, F8>(a, sa, sb, s); });
#endif
}

// fp8-blocks A (maeclip_gemm_fp8_blocks): the plan is always 192-row tiles
// without a split
template <typename OutT, int EPI, int F8>
int launch_f8b(const maeclip_gemm_args& a, const uint8_t* sab, const float* sb, hipStream_t s) {
  const maeclip::Gemm4Plan p = maeclip::gemm4_plan(a, maeclip::G4_FP8_BLOCKS, maeclip::gemm4_device_ncu(), false);
  return launch_plan(p, gemm4_f8_kernel<OutT, EPI, F8, 192>, "maeclip_gemm_fp8_blocks", a, nullptr, sb, sab, s);
}

template <typename OutT, int F8>
int epi_f8b(const maeclip_gemm_args& a, const uint8_t* sab, const float* sb, hipStream_t s) {
  return dispatch_epilogue(a, "maeclip_gemm_fp8_blocks", [&](auto epi) -> int {
    constexpr int EPI = decltype(epi)::value;
    if constexpr (EPI == EPI_GELU || EPI == EPI_DGELU)
      MC_CHECK_ARG(false, "maeclip_gemm_fp8_blocks: epilogue %d not built (0, 2, 4, 5)", a.epilogue);
    else
      return launch_f8b<OutT, EPI, F8>(a, sab, sb, s);
  });
}

// argument checks shared by the two fp8 entries
int check_f8(const maeclip_gemm_args* a, const char* who) {
  MC_CHECK_ARG(a->dtype == MAECLIP_FP8_E4M3 || a->dtype == MAECLIP_FP8_E5M2,
               "%s: dtype (A format) must be MAECLIP_FP8_E4M3 or MAECLIP_FP8_E5M2", who);
  MC_CHECK_ARG(a->a_layout == LAY_KC && a->b_layout == LAY_KC, "%s: KC x KC operands only", who);
  MC_CHECK_ARG(a->K > 0 && a->K % 128 == 0, "%s: K=%lld must be a positive multiple of 128", who, (long long)a->K);
  MC_CHECK_ARG(a->M >= 256 && a->N >= 256 && a->N % 8 == 0, "%s: M, N >= 256 and N %% 8 == 0", who);
  MC_CHECK_ARG(a->splitk <= 1, "%s: no split-K", who);
  MC_CHECK_ARG(a->batch >= 1, "%s: batch >= 1", who);
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  MC_CHECK_ARG(al16(a->A) && al16(a->B) && a->lda % 16 == 0 && a->ldb % 16 == 0 && a->lda >= a->K && a->ldb >= a->K,
               "%s: operands need 16-B aligned rows (lda, ldb %% 16 == 0, >= K)", who);
  MC_CHECK_ARG(al16(a->C) && (a->out_dtype == MAECLIP_BF16 ? a->ldc % 8 : a->ldc % 4) == 0, "%s: C alignment", who);
  const bool wa = a->epilogue == EPI_GELU || a->epilogue == EPI_GELU_D;
  const bool ra = a->epilogue == EPI_DGELU || a->epilogue == EPI_MUL_AUX;
  MC_CHECK_ARG(!(wa && a->aux_out && (!al16(a->aux_out) || a->ldaux % 8)) && !(ra && (!al16(a->aux) || a->ldaux % 8)),
               "%s: aux alignment", who);
  MC_CHECK_ARG(!a->resid || (al16(a->resid) && a->ldr % 4 == 0), "%s: resid alignment", who);
  MC_CHECK_ARG(!a->bias || al16(a->bias), "%s: bias alignment", who);
  const int64_t lim = 0x7fffffffLL;
  MC_CHECK_ARG(a->M * a->lda < lim && a->N * a->ldb < lim, "%s: operand exceeds 2^31 bytes", who);
  return maeclip::check_q8(*a, who);
}

}  // namespace

namespace maeclip {
// the optional fp8-blocks output of a GEMM (maeclip_gemm_args q8)
int check_q8(const maeclip_gemm_args& a, const char* who) {
  if (!a.q8) return 0;
  MC_CHECK_ARG(a.out_dtype == MAECLIP_BF16 && a.batch == 1 && a.beta == 0.f && a.splitk <= 1 && a.N % 128 == 0 &&
                   a.ldq8 >= a.N && a.ldq8 % 8 == 0 && ((uintptr_t)a.q8 & 7) == 0 && a.q8_scale &&
                   (a.q8_fmt == MAECLIP_FP8_E4M3 || a.q8_fmt == MAECLIP_FP8_E5M2),
               "%s: fp8-blocks output (q8) needs bf16 C, batch 1, beta 0, N %% 128 == 0, ldq8 %% 8, a scale buffer "
               "and an fp8 format", who);
  return 0;
}
}  // namespace maeclip

extern "C" int32_t maeclip_gemm_fp8_blocks(const maeclip_gemm_args* a, const uint8_t* scale_a, const float* scale_b,
                                           void* stream) {
  MC_CHECK_ARG(a != nullptr && scale_a != nullptr && scale_b != nullptr, "maeclip_gemm_fp8_blocks: null argument");
  if (int e = check_f8(a, "maeclip_gemm_fp8_blocks")) return e;
  MC_CHECK_ARG(a->batch == 1 && ((uintptr_t)scale_b & 15) == 0, "maeclip_gemm_fp8_blocks: batch 1, 16-B aligned scale_b");
  hipStream_t s = (hipStream_t)stream;
  const bool e5 = a->dtype == MAECLIP_FP8_E5M2;
  if (a->out_dtype == MAECLIP_BF16)
    return e5 ? epi_f8b<bf16_t, 4>(*a, scale_a, scale_b, s) : epi_f8b<bf16_t, 3>(*a, scale_a, scale_b, s);
  return e5 ? epi_f8b<float, 4>(*a, scale_a, scale_b, s) : epi_f8b<float, 3>(*a, scale_a, scale_b, s);
}

extern "C" int32_t maeclip_gemm_fp8(const maeclip_gemm_args* a, const float* scale_a, const float* scale_b,
                                    void* stream) {
  MC_CHECK_ARG(a != nullptr && scale_a != nullptr && scale_b != nullptr, "maeclip_gemm_fp8: null argument");
  if (int e = check_f8(a, "maeclip_gemm_fp8")) return e;
  MC_CHECK_ARG(((uintptr_t)scale_b & 15) == 0, "maeclip_gemm_fp8: 16-B aligned scale_b");
  hipStream_t s = (hipStream_t)stream;
  const bool e5 = a->dtype == MAECLIP_FP8_E5M2;
  if (a->out_dtype == MAECLIP_BF16)
    return e5 ? epi_f8<bf16_t, 2>(*a, scale_a, scale_b, s) : epi_f8<bf16_t, 1>(*a, scale_a, scale_b, s);
  return e5 ? epi_f8<float, 2>(*a, scale_a, scale_b, s) : epi_f8<float, 1>(*a, scale_a, scale_b, s);
}

// The plan of maeclip_gemm_fp8 (blocks = 0) / maeclip_gemm_fp8_blocks (blocks
// != 0) for *a on ncu CUs (ncu <= 0: this device's, the only case that
// touches HIP) after their argument checks; out as maeclip_gemm_plan.
extern "C" int32_t maeclip_gemm_fp8_plan(const maeclip_gemm_args* a, int32_t blocks, int32_t ncu, int32_t out[8],
                                         int64_t* workspace_bytes) {
  const char* who = "maeclip_gemm_fp8_plan";
  MC_CHECK_ARG(a != nullptr && out != nullptr, "%s: null argument", who);
  if (int e = check_f8(a, who)) return e;
  MC_CHECK_ARG(!blocks || a->batch == 1, "%s: fp8 blocks: batch 1", who);
  if (ncu <= 0) ncu = maeclip::gemm4_device_ncu();
  const int family = blocks ? maeclip::G4_FP8_BLOCKS : maeclip::G4_FP8_ROWS;
  maeclip::gemm4_plan_out(maeclip::gemm4_plan(*a, family, ncu, !blocks && a->workspace != nullptr), out);
  if (workspace_bytes) *workspace_bytes = maeclip::gemm4_plan(*a, family, ncu, !blocks).workspace_bytes;
  return (int32_t)maeclip::GemmRoute::V4;
}
