// The per-point arithmetic of the integrated output parameters (FEMEAN femean.F90:84-121, STHQ sthq.F90:75-120, DOMINANT_PERIOD
// dominant_period.F90:76-112; outblock.F90:204,223-263) on a spectrum that sits in an LDS tile: shared by k_outbs (csrc/outbs.hip, the
// tile is FL1) and k_outbs_absolute (csrc/outbs_fl2nd.hip, the tile is FL2ND), so that both give the same bits on the same spectrum.
#pragma once
#include "dev.h"

// FEMEAN's sums over frequency and its tail (femean.F90:105-120) from t2 = the sum over K of MAX(F(K,M),EPSMIN) that lane M holds: shared by
// outbs_point below and by k_outbs_integrals (csrc/outbs_int.hip: FEMEAN of the wind half plane, halphap.F90:89).
template <typename T>
__device__ __forceinline__ void femean_of_rowsums(const DevTab<T>& tb, T t2, int lane, T& EM, T& FM) {
  const int NFRE = tb.NFRE;
  const bool actm = lane < NFRE;
  usum2(actm ? t2 * tb.DFIM[lane] : T(0), actm ? tb.DFIMOFR[lane] * t2 : T(0), EM, FM);
  const T tl = lane_get(t2, NFRE - 1);
  EM = EM + tb.WETAIL * tb.FR[NFRE - 1] * tb.DELTH * tl;
  FM = FM + tb.FRTAIL * tb.DELTH * tl;
  FM = EM / FM;
  FM = m_max(FM, tb.FR[0]);
}

// One wavefront per point; sF = the tile [M][NANG|1], complete and visible to the wave.  lane = M sums MAX(F,EPSMIN) over K in the
// reference's order (FEMEAN), lane = K sums F*DFIM over M in the reference's order (STHQ): EM, FM and THQ [radians, 0 .. 2 PI] in every lane.
// Shared by outbs_point below and by k_outbc (csrc/nest.hip: the mean parameters of the boundary file's records, outbc.F90:83-84).
template <typename T>
__device__ __forceinline__ void femean_sthq_point(const DevTab<T>& tb, const T* sF, int lane, T& EM, T& FM, T& THQ) {
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1;
  const bool actm = lane < NFRE, actk = lane < NANG;
  // FEMEAN
  T t2 = T(0);
  if (actm) {
    const T* p = sF + lane * NAP;
    t2 = m_max(p[0], tb.EPSMIN);
    for (int kk = 1; kk < NANG; kk++) t2 = t2 + m_max(p[kk], tb.EPSMIN);
  }
  femean_of_rowsums(tb, t2, lane, EM, FM);
  // STHQ
  T temp = T(0);
  if (actk)
    for (int m = 0; m < NFRE; m++) temp = temp + sF[m * NAP + lane] * tb.DFIM[m];
  T SI, CI;
  usum2(actk ? tb.SINTH[lane] * temp : T(0), actk ? tb.COSTH[lane] * temp : T(0), SI, CI);
  if (CI == T(0)) CI = tb.EPSMIN;
  THQ = m_atan2(SI, CI);
  if (THQ < T(0)) THQ = THQ + tb.ZPI;
}

// The same wave and tile.  Lane 0 writes o[0..4] = significant wave height, mean direction [degrees], mean period or zmiss, EM, peak
// period or zmiss.
template <typename T>
__device__ __forceinline__ void outbs_point(const DevTab<T>& tb, const T* sF, int lane, T zmiss, T* __restrict__ o) {
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1;
  const bool actm = lane < NFRE, actk = lane < NANG;
  T EM, FM, THQ;
  femean_sthq_point(tb, sF, lane, EM, FM, THQ);
  // DOMINANT_PERIOD: lane = K finds its maximum, lane = M sums the cropped directions in the reference's order
  T fmx = T(0);
  if (actk)
    for (int m = 0; m < NFRE; m++) fmx = m_max(fmx, sF[m * NAP + lane]);
  const T FCROP = T(0.1) * umax(actk ? fmx : T(0));
  T f1d = T(0);
  if (actm) {
    const T* p = sF + lane * NAP;
    for (int kk = 0; kk < NANG; kk++)
      if (p[kk] > FCROP) f1d = f1d + p[kk] * tb.DELTH;
    f1d = (f1d * f1d) * (f1d * f1d);
  }
  T EM4, DP;
  usum2(actm ? tb.DFIM[lane] * f1d : T(0), actm ? tb.DFIMFR[lane] * f1d : T(0), EM4, DP);
  DP = (EM4 > T(0) && DP > tb.EPSMIN) ? EM4 / DP : T(0);
  if (lane == 0) {
    const T DEG = T(180.0) / tb.PI;
    o[0] = T(4) * m_sqrt(m_max(EM, T(0)));
    T d = DEG * THQ + T(180.0);
    d = d - T(360.0) * T((int)(d / T(360.0)));  // MOD(.,360) for d >= 0
    o[1] = d;
    o[2] = (FM > T(0)) ? T(1) / FM : zmiss;
    o[3] = EM;
    o[4] = (DP > T(0)) ? DP : zmiss;
  }
}
