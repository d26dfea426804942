// GEMM v4, dense bf16 operands: the kernels of maeclip_gemm's v4 route, their
// launch from a plan (gemm4_plan.h), the shape conditions of the route and its
// workspace query, the device's CU count and the diagnostic stamps export.
// Device code: gemm4_body.h.
#include "gemm4_body.h"

namespace {

template <int LA, int LB, typename OutT, int EPI, bool SPLIT, int BM = 256, bool SK = false>
__global__ void __launch_bounds__(512) gemm4_kernel(const Gemm4Args g) {
  gemm4_body<LA, LB, OutT, EPI, SPLIT, false, 0, BM, SK>(g.a, nullptr, nullptr, nullptr, &g.sk);
}

template <int LA, int LB, typename OutT, int EPI>
int launch4(const maeclip_gemm_args& a, hipStream_t s) {
  const maeclip::Gemm4Plan p = maeclip::gemm4_plan(a, maeclip::G4_BF16, maeclip::gemm4_device_ncu(), a.workspace != nullptr);
  // 256-row tiles: the caller's split-K slices (grid y) write fp32 slabs
  Gemm4Kern kern = p.gy > 1 ? gemm4_kernel<LA, LB, OutT, EPI, true> : gemm4_kernel<LA, LB, OutT, EPI, false>;
  const char* who = "maeclip_gemm(v4)";
  if constexpr (LA == LAY_KC) {
    if (p.bm == 192) {
      kern = p.S > 0 ? gemm4_kernel<LA, LB, OutT, EPI, false, 192, true> : gemm4_kernel<LA, LB, OutT, EPI, false, 192>;
      who = "maeclip_gemm(v4, 192-row tiles)";
    } else if (p.bm == 128) {
      kern = gemm4_kernel<LA, LB, OutT, EPI, false, 128>;
      who = "maeclip_gemm(v4, 128-row tiles)";
    }
  }
  return launch_plan(p, kern, who, a, nullptr, nullptr, nullptr, s);
}

template <int LA, int LB, typename OutT>
int epi4(const maeclip_gemm_args& a, hipStream_t s) {
#ifdef GEMM4_DEV_SUBSET   // register / ISA inspection builds only: one epilogue
#ifndef GEMM4_DEV_EPI
#define GEMM4_DEV_EPI EPI_NONE
#endif
  return launch4<LA, LB, OutT, GEMM4_DEV_EPI>(a, s);
#else
  return dispatch_epilogue(a, "maeclip_gemm(v4)",
                           [&](auto epi) { return launch4<LA, LB, OutT, decltype(epi)::value>(a, s); });
#endif
}

template <int LA, int LB>
int out4(const maeclip_gemm_args& a, hipStream_t s) {
  return a.out_dtype == MAECLIP_BF16 ? epi4<LA, LB, bf16_t>(a, s) : epi4<LA, LB, float>(a, s);
}

}  // namespace

#ifdef GEMM4_STAMPS
extern "C" int maeclip_debug_gemm4_stamps(uint64_t* host, int n) {
  // n < 0: zero the stamp buffer (host unused)
  if (n < 0) {
    static uint64_t zero[256 * 8 * 2 * 4] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
  }
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), sizeof(uint64_t) * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif

namespace maeclip {
// Shapes the v4 epilogue supports: 8 consecutive output columns per lane with
// 16-B accesses on C / aux / resid.
bool gemm_v4_ok(const maeclip_gemm_args& a) {
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (a.dtype != MAECLIP_BF16 || a.K % 64 != 0 || a.K <= 0 || a.lda % 8 || a.ldb % 8) return false;
  if (a.M < 256 || a.N < 256 || a.N % 8) return false;
  // buffer-descriptor DMA: every operand byte offset must fit 31 bits
  const int64_t lim = 0x7fffffffLL;
  if ((a.a_layout == LAY_KC ? a.M * a.lda : a.K * a.lda) * 2 >= lim) return false;
  if ((a.b_layout == LAY_KC ? a.N * a.ldb : a.K * a.ldb) * 2 >= lim) return false;
  if (a.splitk > 1) return al16(a.workspace);
  if (!al16(a.C) || (a.out_dtype == MAECLIP_BF16 ? a.ldc % 8 : a.ldc % 4)) return false;
  const bool wa = a.epilogue == EPI_GELU || a.epilogue == EPI_GELU_D;
  const bool ra = a.epilogue == EPI_DGELU || a.epilogue == EPI_MUL_AUX;
  if ((wa && a.aux_out && (!al16(a.aux_out) || a.ldaux % 8)) || (ra && (!al16(a.aux) || a.ldaux % 8))) return false;
  if (a.resid && (!al16(a.resid) || a.ldr % 4)) return false;
  if (a.bias && !al16(a.bias)) return false;
  return true;
}

// scratch bytes of the in-launch split a launch of this shape would take when
// a workspace is offered (0: none chosen)
int64_t gemm_v4_workspace(const maeclip_gemm_args& a) {
  const bool f8 = a.dtype == MAECLIP_FP8_E4M3 || a.dtype == MAECLIP_FP8_E5M2;
  if (f8 ? (a.K % 128 != 0 || a.M < 256 || a.N < 256) : !gemm_v4_ok(a)) return 0;
  return gemm4_plan(a, f8 ? G4_FP8_ROWS : G4_BF16, gemm4_device_ncu(), true).workspace_bytes;
}

int gemm4_device_ncu() {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
  }
  return ncu;
}

int gemm_v4(const maeclip_gemm_args& a, hipStream_t s) {
  return dispatch_layouts(a, [&](auto la, auto lb) { return out4<decltype(la)::value, decltype(lb)::value>(a, s); });
}
}  // namespace maeclip
