// WDFLUXES (wdfluxes.F90:156-306) and SETICE (setice.F90:67-86) for OUTSTEP0 (outstep0.F90:106-221: the output before the first time step and
// after a restart).  WDFLUXES is the flux-only mode of k_implsch4 (implsch_v4.h, PART = 3: the source terms evaluated once, nothing advanced)
// on the common builds (flag sets A and B) and the alternate ones (IPHYS = 0, ISNONLIN = 1 on flag set A), single and double precision (24 directions: single only), at
// the shapes of implsch_v4_shapes.h.  A translation unit of its own: the builds of the time step are not recompiled
// with it, nor it with them.
#include "implsch_v4_launch.h"
#include "launch.h"

// 24 directions: single precision only.  The double precision build (four points per wavefront) gave a wrong PHIWA and Stokes drift on the
// device while every other instantiation is right; the cause is not found (DESIGN.md section 1 says what is known and what is not): not
// shipped, ecwam_hip_wdfluxes refuses the configuration (wdfluxes_built).
// (A developer looking for the cause adds the plain -DECWAM_HIP_WDF_DP24=1 to the flags of this unit.)
#ifndef ECWAM_HIP_WDF_DP24
#define ECWAM_HIP_WDF_DP24 0
#endif
template <typename T, typename S>
constexpr bool v4_wdf_built = sizeof(T) == 4 || S::NANG != 24 || ECWAM_HIP_WDF_DP24;

// v: A, B (EXT), iphys0 (JAN) or isnonlin1 (ENHMC).  Returns 0 when launched, -1 when no instantiation covers the configuration.
template <typename T>
int launch_wdfluxes(const void* tab, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* ff, void* intf, int* mij, void* xllws,
                    void* fin, double* w2n, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s) {
  if (kijl - kijs <= 0) return 0;
  if (NFRE != V4_NFRE) return -1;
  // (the kernel's pointer types are those of the time step; this mode stores through neither fl1 nor ff)
#define V4_ARGS tab, kijs, kijl, const_cast<void*>(fl1), wvprpt, const_cast<void*>(ff), intf, mij, xllws, fin, w2n, nullptr, 0, nullptr, V4Adv<T>{}, s
  return v4_for_shape(NANG, r1, r2, nh, [&](auto sh) {
    using S = decltype(sh);
    if constexpr (v4_wdf_built<T, S>) {
      switch (v) {
        case Implsch4Variant::A: return launch4<T, S, false, false, false, false, V4_WDF>(V4_ARGS);
        case Implsch4Variant::B: return launch4<T, S, true, false, false, false, V4_WDF>(V4_ARGS);
        case Implsch4Variant::iphys0: return launch4<T, S, false, true, false, false, V4_WDF>(V4_ARGS);
        case Implsch4Variant::isnonlin1: return launch4<T, S, false, false, true, false, V4_WDF>(V4_ARGS);
        default: break;
      }
    }
    return -1;
  });
#undef V4_ARGS
}
template int launch_wdfluxes<float>(const void*, int, int, const void*, const void*, const void*, void*, int*, void*, void*, double*, int, int, int, int, int, Implsch4Variant, hipStream_t);
template int launch_wdfluxes<double>(const void*, int, int, const void*, const void*, const void*, void*, int*, void*, void*, double*, int, int, int, int, int, Implsch4Variant, hipStream_t);
// whether WDFLUXES is built at NANG directions in the precision of real_bytes
bool wdfluxes_built(int NANG, int real_bytes) {
  return v4_for_nang(NANG, [&](auto sh) { return int(real_bytes == 4 ? v4_wdf_built<float, decltype(sh)> : v4_wdf_built<double, decltype(sh)>); }) == 1;
}

// SETICE, element-wise: a thread owns the 16 bytes (direction K, frequencies M .. M + VEC - 1) of one sea point.  Where CICOVER > CITHRSH the
// spectrum becomes MAX(EPSMIN, 1 - CICOVER) FLMIN MAX(0, COS(TH(K) - WDWAVE))**2 (the reference's F * 0 + that: the same value); elsewhere it
// is F * 1 + 0, F itself: those threads touch nothing.
template <typename T>
__global__ void __launch_bounds__(256) k_setice(const DevTab<T>* __restrict__ tp, int kijs, int kijl, T* __restrict__ fl1, const T* __restrict__ ffa) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  const DevTab<T>& tb = *tp;
  const int NC = tb.NFRE / VEC, per = tb.NANG * NC;      // chunks per direction, per point
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= (size_t)(kijl - kijs) * per) return;
  const int ij = kijs + (int)(w / per);
  const int r = (int)(w - (size_t)(ij - kijs) * per);
  const T* ff = ffa + (size_t)ij * ECWAM_HIP_NFF;
  const T WDWAVE = ff[1], CICOVER = ff[2];
  if (!(CICOVER > tb.CITHRSH)) return;
  const T cd = m_max(T(0), m_cos(tb.TH[r / NC] - WDWAVE));
  const T v = (m_max(tb.EPSMIN, T(1) - CICOVER) * tb.FLMIN) * (cd * cd);
  VT o;
#pragma unroll
  for (int i = 0; i < VEC; i++) o[i] = v;
  *reinterpret_cast<VT*>(fl1 + (size_t)ij * tb.NANG * tb.NFRE + (size_t)r * VEC) = o;
}
// returns 0 when launched, -1 when a direction's frequencies are no whole number of 16-byte chunks
template <typename T>
int launch_setice(const void* tab, int kijs, int kijl, void* fl1, const void* ff, int NANG, int NFRE, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  if (kijl - kijs <= 0) return 0;
  const size_t total = (size_t)(kijl - kijs) * NANG * (NFRE / VEC);
  hipLaunchKernelGGL((k_setice<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, (T*)fl1, (const T*)ff);
  return 0;
}
template int launch_setice<float>(const void*, int, int, void*, const void*, int, int, hipStream_t);
template int launch_setice<double>(const void*, int, int, void*, const void*, int, int, hipStream_t);
