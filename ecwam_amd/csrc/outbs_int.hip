// OUTBLOCK's remaining spectral integrals on the device, one pass over the spectrum (outblock.F90:266-287, 451-462, 500-523, 597-604):
// OUTBETA's drag coefficient and TAUW / MAX(UFRIC**2, EPSUS) (point-wise, FF only); MEANSQS at the two cut-offs (HALPHAP with MEANSQS_LF and
// FEMEAN of the wind half plane, MEANSQS_GC with OMEGAGC, MEANSQS_LF, the logarithmic tail); CIMSSTRN with AKI_ICE; WEFLUX; CTCOR -- all of
// FL1 -- and SEBTMEAN of the output spectrum FL2ND for up to 8 period bands (SE10MEAN is one of them).  Reads FL1 once and a separate FL2ND
// once; writes out[ij][8 + NBAND] in the column order of ecwam_hip.h.  Then OUTSETWMASK (outsetwmask.F90) for any output buffer.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "implsch_point.h"
#include "outbs_int.h"
#include "outbs_point.h"
#include "launch.h"

__device__ __forceinline__ float mi_fmod(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double mi_fmod(double a, double b) { return fmod(a, b); }

// Per-wave LDS: the spectrum tile [M][NANG|1]; NSUM arrays [NFRE|1] of per-frequency terms, each summed over M by one lane; F1D of the
// FL2ND row [NFRE]; the interpolated F1D at the bands' cut frequencies [2 NBAND]; WD [NANG]
constexpr int INT_NSUM = 9;
struct IntLds {
  size_t terms, f1d, cut, wd, bytes;
  __host__ __device__ IntLds(int NANG, int NFRE, size_t tsz) {
    terms = ((size_t)NFRE * (NANG | 1) * tsz + 7) & ~(size_t)7;
    f1d = terms + (size_t)INT_NSUM * (NFRE | 1) * tsz;
    cut = f1d + (size_t)NFRE * tsz;
    wd = cut + (size_t)2 * ECWAM_HIP_MAXBAND * tsz;
    bytes = (wd + (size_t)NANG * tsz + 15) & ~(size_t)15;
  }
};

// One wavefront per point, wpb points per workgroup.  Phase A, lane = M: the sums over K, in the reference's order of K.  Phase B: lane = M
// forms the term of every sum over M and leaves it in LDS; lane = q then adds the terms of sum q from M = 1 upwards, so every sum over M is
// added in the reference's order (FEMEAN of the half-plane spectrum is the exception: it is outbs_point.h's, reduced across the wavefront).
// The scalars that follow are computed by every lane alike.  Contraction is off: every product and sum is rounded where the reference
// rounds it.  No atomics; nothing depends on scheduling.
template <typename T, int NANG>
__global__ void __launch_bounds__(256) k_outbs_integrals(const DevTab<T>* __restrict__ tp, const IntTab<T>* __restrict__ ip, int kijs, int kijl, int wpb,
                                                         const T* __restrict__ fl1, const T* __restrict__ fl2nd, const T* __restrict__ wvprpt,
                                                         const T* __restrict__ ff, int flags, T zmiss, T* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char int_smem[];
  const DevTab<T>& tb = *tp;
  const IntTab<T>& it = *ip;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ij = kijs + blockIdx.x * wpb + wave;
  if (ij >= kijl) return;  // wave-uniform, no block barrier below
  const int NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE, SP = NFRE | 1, NBAND = it.NBAND;
  const IntLds L(NANG, NFRE, sizeof(T));
  unsigned char* base = int_smem + (size_t)wave * L.bytes;
  T* sF = reinterpret_cast<T*>(base);
  T* sS = reinterpret_cast<T*>(base + L.terms);
  T* sD = reinterpret_cast<T*>(base + L.f1d);
  T* sI = reinterpret_cast<T*>(base + L.cut);
  T* sW = reinterpret_cast<T*>(base + L.wd);
  const bool actm = lane < NFRE;
  const T EPS = tb.EPSMIN, DELTH = tb.DELTH;
  const T* f = ff + (size_t)ij * ECWAM_HIP_NFF;
  const T* wp = wvprpt + (size_t)ij * (ECWAM_HIP_NWPR * NFRE);
  const int ncol = 8 + NBAND;
  T* o = out + (size_t)ij * ncol;
  const bool want_fl1 = flags & (INT_SLOPES | INT_STRAIN | INT_FLUX | INT_CTCOR);
  const bool want_bands = flags & INT_BANDS;
  const bool same = fl2nd == fl1;

  // the row [K][M] -> the tile [M][K]; INT_U rounds of 64 bins are in flight at once
  auto load_tile = [&](const T* __restrict__ src) {
    constexpr int INT_U = 8;
    const size_t row = (size_t)ij * N;
    for (int c0 = 0; c0 < N; c0 += 64 * INT_U) {
      T fv[INT_U];
#pragma unroll
      for (int u = 0; u < INT_U; u++) fv[u] = src[row + min(c0 + 64 * u + lane, N - 1)];  // in the row: no branch around the loads
#pragma unroll
      for (int u = 0; u < INT_U; u++) {
        const int e = c0 + 64 * u + lane;
        if (e < N) {
          const int kk = e / NFRE, mm = e - kk * NFRE;
          sF[mm * NAP + kk] = fv[u];
        }
      }
    }
  };
  // F1D of the tile (sebtmean.F90:133-144) per lane = M, and per band the interpolated F1D at its two cut frequencies, formed per K
  // (sebtmean.F90:117-131, 146-160): lane 2 b the lower one, lane 2 b + 1 the upper one
  auto band_sums = [&]() {
    if (lane < 2 * NBAND) {
      const int b = lane >> 1, top = lane & 1;
      const int r1 = top ? it.MCUTT[b] : it.MCUTB[b] - 1;  // 0-based row of the right-hand neighbour
      T acc = T(0);
      if (r1 >= 1 && r1 < NFRE) {
        const T wl = top ? it.WLT[b] : it.WLB[b], wr = top ? it.WRT[b] : it.WRB[b];
        const T *p0 = sF + (r1 - 1) * NAP, *p1 = sF + r1 * NAP;
        acc = (wl * p0[0] + wr * p1[0]) * DELTH;
        for (int kk = 1; kk < NANG; kk++) acc = acc + (wl * p0[kk] + wr * p1[kk]) * DELTH;
      }
      sI[lane] = acc;
    }
  };

  T sA = T(0), sWD = T(0), sFE = T(0), sWDd = T(0), tcg = T(0), tx = T(0), ty = T(0), px = T(0), py = T(0), d2 = T(0);
  if (want_fl1 || (want_bands && same)) {
    load_tile(fl1);
    // the wind half plane WD (halphap.F90:73) with COSWDIF of outblock.F90:200
    if (want_fl1 && lane < NANG) sW[lane] = T(0.5) + T(0.5) * m_sign(T(1), m_cos(tb.TH[lane] - f[1]));
    WSYNC();
  }
  if (want_fl1 && actm) {
    const T cg = wp[NFRE + lane];
    const T* p = sF + lane * NAP;
#pragma unroll 4
    for (int kk = 0; kk < NANG; kk++) {
      const T v = p[kk];
      const T fw = v * sW[kk];
      sA = sA + v;
      sWD = sWD + fw;
      sFE = sFE + m_max(fw, EPS);
      sWDd = sWDd + fw * DELTH;
      const T fcg = v * cg;  // weflux.F90:113-123
      tcg = tcg + fcg;
      tx = tx + fcg * tb.SINTH[kk];
      ty = ty + fcg * tb.COSTH[kk];
      px = px + v * tb.SINTH[kk];  // weflux.F90:139-149 (used at M = NFRE)
      py = py + v * tb.COSTH[kk];
      d2 = d2 + v * DELTH;
    }
  } else if (want_bands && same && actm) {
    const T* p = sF + lane * NAP;
    for (int kk = 0; kk < NANG; kk++) d2 = d2 + p[kk] * DELTH;
  }
  if (want_bands && same) band_sums();
  if (want_bands && !same) {
    WSYNC();  // the tile's readers above are done
    load_tile(fl2nd);
    WSYNC();
    d2 = T(0);
    if (actm) {
      const T* p = sF + lane * NAP;
      for (int kk = 0; kk < NANG; kk++) d2 = d2 + p[kk] * DELTH;
    }
    band_sums();
  }

  // ---- the bands: lane = b adds the trapezoid from M0 to M1, then the front tail, then the f**-5 extension (sebtmean.F90:107-109, 163-198)
  if (want_bands) {
    if (actm) sD[lane] = d2;
    WSYNC();
    if (lane < NBAND) {
      const int b = lane, cb = it.MCUTB[b], ct = it.MCUTT[b];
      auto f1d = [&](int M) {  // 1-based
        if (ct < NFRE && M == ct + 1) return sI[2 * b + 1];
        if (cb > 1 && M == cb - 1) return sI[2 * b];
        return sD[M - 1];
      };
      T E = EPS;
      for (int M = it.M0[b]; M <= it.M1[b]; M++) E = E + it.DF[b][M - 1] * (f1d(M + 1) + f1d(M));
      if (it.FRONT[b]) E = E + it.DFT[b] * f1d(1);
      if (it.TAIL[b]) E = E + it.ZW[b] * sD[NFRE - 1];
      o[8 + b] = T(4) * m_sqrt(m_max(E, T(0)));
    }
  }

  // ---- the readers of FL1
  if (want_fl1) {
    const T ufric = f[7];
    const T wn = actm ? wp[lane] : T(1);
    const T dfim = actm ? tb.DFIM[lane] : T(0);
    const T temp1 = dfim * (wn * wn);  // meansqs_lf.F90:89
    T strn = T(0);
    if ((flags & INT_STRAIN) && actm) {  // cimsstrn.F90:89-118
      const T cith = f[13], depth = f[15];
      const T xki = aki_ice_d(tb.G, wn, depth, tb.ROWATER, cith);
      const T e = T(0.5) * cith * (xki * xki * xki) / wn;
      if (sA > tb.FLMIN / DELTH) strn = e * e * sA * dfim;
    }
    if (actm) {
      sS[0 * SP + lane] = temp1 * sWD;
      sS[1 * SP + lane] = temp1 * sA;
      sS[3 * SP + lane] = strn;
      sS[4 * SP + lane] = dfim * sA;                // ctcor.F90:85
      sS[5 * SP + lane] = tb.DFIMFR[lane] * sA;     // ctcor.F90:86
      sS[6 * SP + lane] = dfim * tcg;               // weflux.F90:127-129
      sS[7 * SP + lane] = dfim * tx;
      sS[8 * SP + lane] = dfim * ty;
    }
    WSYNC();
    T acc = T(0);
    if (lane < INT_NSUM) {  // lane 1 / 2: MEANSQS_LF up to NFRE_EFF of cut-off 0 / 1 (meansqs.F90:101-103)
      const int arr = lane == 2 ? 1 : lane;
      const int hi = lane == 1 ? it.NFRE_EFF[0] : lane == 2 ? it.NFRE_EFF[1] : NFRE;
      for (int m = 0; m < hi; m++) acc = acc + sS[arr * SP + m];
    }
    const T XMSSWD = lane_get(acc, 0), XLF0 = lane_get(acc, 1), XLF1 = lane_get(acc, 2), STRN = lane_get(acc, 3), EMC = lane_get(acc, 4);
    T ZT1 = lane_get(acc, 5), WEFMAG = lane_get(acc, 6), WEFX = lane_get(acc, 7), WEFY = lane_get(acc, 8);

    if (flags & INT_SLOPES) {
      // HALPHAP (halphap.F90:86-112)
      T EM, FM;
      femean_of_rowsums(tb, sFE, lane, EM, FM);
      const T tail = tb.ZPI4GM2 * tb.FR5[NFRE - 1] * lane_get(sWDd, NFRE - 1);
      T ALPHAP = tail;
      if (EM > T(0) && FM < tb.FR[NFRE - 3]) {
        ALPHAP = XMSSWD / (m_log(tb.FR[NFRE - 1]) - m_log(FM));
        if (ALPHAP > tb.ALPHAPMAX) ALPHAP = tail;
      }
      const T HALP = T(0.5) * m_min(ALPHAP, tb.ALPHAPMAX);
      // OMEGAGC (omegagc.F90:51-55)
      const int NS0 = ns_gc_d(tb, ufric);
      const T XKS = tb.XK_GC[NS0], FRGC = tb.OMEGA_GC[NS0] / tb.ZPI;
#pragma unroll
      for (int c = 0; c < 2; c++) {  // meansqs_gc.F90:59-82, meansqs.F90:99-112
        int NS = NS0;
        const int NE = it.NE[c];
        T X;
        if (XKS > it.XKMSS[c]) { NS = NE; X = T(0); }
        else X = tb.DELKCC_GC_NS[NS] * tb.XKM_GC[NS];
        for (int i = NS + 1; i <= NE; i++) X = X + it.DELKCC_GC[i] * tb.XKM_GC[i];
        const T COEF = tb.C2OSQRTVG_GC[NS] * HALP;
        X = X * COEF;
        X = X + (c ? XLF1 : XLF0);
        const T XLOGFS = m_log(tb.FR[it.NFRE_EFF[c] - 1]);
        X = X + T(2) * HALP * m_max(m_log(m_min(FRGC, it.FCUT[c])) - XLOGFS, T(0));
        if (lane == 0) o[c ? 7 : 2] = X;
      }
    }
    if ((flags & INT_STRAIN) && lane == 0) o[3] = STRN;
    if (flags & INT_FLUX) {  // weflux.F90:104-105, 153-177; outblock.F90:507-512
      const T ROG = tb.ROWATER * tb.G;
      const T DELT = tb.FRTAIL * DELTH * tb.G / (T(2) * tb.ZPI);
      WEFMAG = WEFMAG + DELT * lane_get(sA, NFRE - 1);
      WEFX = WEFX + DELT * lane_get(px, NFRE - 1);
      WEFY = WEFY + DELT * lane_get(py, NFRE - 1);
      WEFMAG = ROG * WEFMAG;
      if (WEFY == T(0)) WEFY = EPS;
      T d = m_atan2(WEFX, WEFY);
      if (d < T(0)) d = d + tb.ZPI;
      if (lane == 0) {
        const T DEG = T(57.295778667);  // yowpcons.F90:31
        o[4] = WEFMAG;
        o[5] = mi_fmod(DEG * d + T(180), T(360));
      }
    }
    if (flags & INT_CTCOR) {  // ctcor.F90:91-120
      if (ZT1 > T(0)) ZT1 = m_min(EMC / ZT1, T(1) / tb.FR[0]);
      else ZT1 = T(0);
      WSYNC();  // the sums above have read their terms
      if (actm) {
        const T zarg = tb.PI * tb.FR[lane] * ZT1, zamp = dfim * sA;
        sS[0 * SP + lane] = zamp * m_cos(zarg);
        sS[1 * SP + lane] = zamp * m_sin(zarg);
      }
      WSYNC();
      T a2 = T(0);
      if (lane < 2)
        for (int m = 0; m < NFRE; m++) a2 = a2 + sS[lane * SP + m];
      const T ZRHO = lane_get(a2, 0), ZLAM = lane_get(a2, 1);
      if (lane == 0) o[6] = EMC > T(0) ? m_sqrt(ZRHO * ZRHO + ZLAM * ZLAM) / EMC : zmiss;
    }
  }

  // ---- point-wise: OUTBETA's CD (outbeta.F90:113-133, outblock.F90:277) and TAUW / MAX(UFRIC**2, EPSUS) (outblock.F90:281)
  if ((flags & INT_POINT) && lane == 0) {
    const T u10 = f[3], ustar = f[7], tauw = f[8], chrnck = f[12];
    const T amax = tb.LLGCBZ0 ? tb.ALPHAMAX : m_min(tb.ALPHAMAX, T(0.02) + T(0.01) * u10);
    const T usm = T(1) / m_max(ustar, tb.EPSUS);
    const T betam = m_max(m_min(chrnck, amax), tb.ALPHAMIN);
    const T z0atm = tb.RNUM * usm + tb.GM1 * betam * (ustar * ustar);
    const T q = tb.XKAPPA / m_log(T(1) + tb.XNLEV / z0atm);
    o[0] = m_min(q * q, T(0.01));
    o[1] = tauw / m_max(ustar * ustar, tb.EPSUS);
  }
}

template <typename T, int NANG>
static void launch_int_n(const void* tab, const void* itab, int kijs, int kijl, const void* fl1, const void* fl2nd, const void* wvprpt, const void* ff,
                         int flags, double zmiss, void* out, int NFRE, hipStream_t s) {
  const int n = kijl - kijs;
  const IntLds L(NANG, NFRE, sizeof(T));
  const int wpb = (int)std::min<size_t>(4, (size_t)64 * 1024 / L.bytes);
  hipLaunchKernelGGL((k_outbs_integrals<T, NANG>), dim3((n + wpb - 1) / wpb), dim3(64 * wpb), wpb * L.bytes, s, (const DevTab<T>*)tab,
                     (const IntTab<T>*)itab, kijs, kijl, wpb, (const T*)fl1, (const T*)fl2nd, (const T*)wvprpt, (const T*)ff, flags, (T)zmiss, (T*)out);
}

// 0 = launched (or nothing to do), 1 = unsupported spectral size, 2 = no build for NANG
template <typename T>
int launch_outbs_integrals(const void* tab, const void* itab, int kijs, int kijl, const void* fl1, const void* fl2nd, const void* wvprpt, const void* ff,
                           int flags, double zmiss, void* out, int NANG, int NFRE, hipStream_t s) {
  if (kijl - kijs <= 0 || !flags) return 0;
  if (!outbs_size_ok(NANG, NFRE, sizeof(T))) return 1;
  switch (NANG) {
    case 48: launch_int_n<T, 48>(tab, itab, kijs, kijl, fl1, fl2nd, wvprpt, ff, flags, zmiss, out, NFRE, s); return 0;
    case 36: launch_int_n<T, 36>(tab, itab, kijs, kijl, fl1, fl2nd, wvprpt, ff, flags, zmiss, out, NFRE, s); return 0;
    case 24: launch_int_n<T, 24>(tab, itab, kijs, kijl, fl1, fl2nd, wvprpt, ff, flags, zmiss, out, NFRE, s); return 0;
    case 12: launch_int_n<T, 12>(tab, itab, kijs, kijl, fl1, fl2nd, wvprpt, ff, flags, zmiss, out, NFRE, s); return 0;
  }
  return 2;
}
template int launch_outbs_integrals<float>(const void*, const void*, int, int, const void*, const void*, const void*, const void*, int, double, void*, int, int, hipStream_t);
template int launch_outbs_integrals<double>(const void*, const void*, int, int, const void*, const void*, const void*, const void*, int, double, void*, int, int, hipStream_t);

// ---- the constants of IntTab, on the host, in the working precision and in the reference's order of operations
template <typename T>
static const char* int_tab_fill(const DevTab<T>& tb, double xkmss_cutoff, int nband, const double* tbnd, const double* ttop, const void* delkcc_gc, IntTab<T>& h) {
  memset(&h, 0, sizeof(h));
  const int NFRE = tb.NFRE, NG = tb.NWAV_GC;
  const T* FR = tb.FR;  // 0-based here
  for (int i = 0; i < NG; i++) h.DELKCC_GC[i + 1] = ((const T*)delkcc_gc)[i];
  // userin.F90:1214; outblock.F90:602
  h.XKMSS[0] = xkmss_cutoff > 0.0 ? (T)xkmss_cutoff : tb.XK_GC[NG];
  const T zf = tb.ZPI * FR[NFRE - 1];
  h.XKMSS[1] = zf * zf / tb.G;
  for (int c = 0; c < 2; c++) {
    h.FCUT[c] = std::sqrt(tb.G * h.XKMSS[c]) / tb.ZPI;  // meansqs.F90:99-101
    const int mss = (int)(std::log((double)h.FCUT[c] / (double)FR[0]) / std::log((double)tb.FRATIO)) + 1;
    h.NFRE_EFF[c] = std::min(NFRE, mss);
    if (h.NFRE_EFF[c] < 1) return "the mean-square-slope cut-off lies below FR(1)";
    const long ne = std::lround(std::log((double)h.XKMSS[c] * (double)tb.XKM_GC[1]) * (double)tb.XLOGKRATIOM1_GC);  // meansqs_gc.F90:59
    h.NE[c] = (int)std::min<long>(std::max<long>(ne, 1), NG);
  }
  h.NBAND = nband;
  const T EPS = tb.EPSMIN, one = T(1), half = T(0.5);
  for (int b = 0; b < nband; b++) {  // sebtmean.F90:81-102
    const T TB = (T)tbnd[b], TT = (T)ttop[b];
    if (!(TB <= TT)) return "a band needs TB <= TT (the shorter period first)";
    T FBOT = one / std::max(TT, EPS);
    const T FCUTB_FT = std::min(FBOT, FR[NFRE - 1]);
    const T FCUTB = std::max(FR[0], FCUTB_FT);
    FBOT = std::max(FBOT, FR[NFRE - 1]);
    int MCUTB = 1;
    while (FR[MCUTB - 1] < FCUTB && MCUTB < NFRE) MCUTB++;
    T FTOP = one / std::max(TB, EPS);
    const T FCUTT = std::max(FR[0], std::min(FTOP, FR[NFRE - 1]));
    FTOP = std::max(FTOP, FR[NFRE - 1]);
    int MCUTT = NFRE;
    while (FR[MCUTT - 1] > FCUTT && MCUTT > 1) MCUTT--;
    if (FCUTB == FCUTT) MCUTT = MCUTB - 1;
    if (MCUTT < 1) return "a band lies wholly below FR(1) (SEBTMEAN would read FR(0))";
    T FRLOC[MAXF + 2];
    for (int m = 1; m <= NFRE; m++) FRLOC[m] = FR[m - 1];
    h.WLB[b] = h.WLT[b] = T(0); h.WRB[b] = h.WRT[b] = one;
    if (MCUTB > 1) {  // :117-120
      FRLOC[MCUTB - 1] = FCUTB;
      h.WLB[b] = (FR[MCUTB - 1] - FCUTB) / (FR[MCUTB - 1] - FR[MCUTB - 2]);
      h.WRB[b] = one - h.WLB[b];
    }
    if (MCUTT < NFRE) {  // :146-149
      FRLOC[MCUTT + 1] = FCUTT;
      h.WLT[b] = (FR[MCUTT] - FCUTT) / (FR[MCUTT] - FR[MCUTT - 1]);
      h.WRT[b] = one - h.WLT[b];
    }
    h.MCUTB[b] = MCUTB; h.MCUTT[b] = MCUTT;
    h.M0[b] = std::max(MCUTB - 1, 1); h.M1[b] = std::min(MCUTT, NFRE - 1);
    for (int M = h.M0[b]; M <= h.M1[b]; M++) h.DF[b][M - 1] = half * (FRLOC[M + 1] - FRLOC[M]);  // :165
    if (FCUTB_FT < FCUTB && FCUTB == FR[0]) {  // :172-175
      const T WL = (FR[0] - FCUTB_FT) / FR[0], WR = one - WL;
      h.FRONT[b] = 1;
      h.DFT[b] = half * (FR[0] - FCUTB_FT) * (one + WR);
    }
    if (FBOT < FTOP) {  // :182-184
      const T b2 = FBOT * FBOT, t2 = FTOP * FTOP;
      h.TAIL[b] = 1;
      h.ZW[b] = T(0.25) * tb.FR5[NFRE - 1] * (one / (b2 * b2) - one / (t2 * t2));
    }
  }
  return nullptr;
}

const char* outbs_int_tab_build(const void* devtab_host, int real_bytes, double xkmss_cutoff, int nband, const double* tbnd, const double* ttop,
                                const void* delkcc_gc, std::vector<unsigned char>& host) {
  if (real_bytes == 4) {
    host.resize(sizeof(IntTab<float>));
    return int_tab_fill<float>(*(const DevTab<float>*)devtab_host, xkmss_cutoff, nband, tbnd, ttop, delkcc_gc, *(IntTab<float>*)host.data());
  }
  host.resize(sizeof(IntTab<double>));
  return int_tab_fill<double>(*(const DevTab<double>*)devtab_host, xkmss_cutoff, nband, tbnd, ttop, delkcc_gc, *(IntTab<double>*)host.data());
}
size_t outbs_devtab_bytes(int real_bytes) { return real_bytes == 4 ? sizeof(DevTab<float>) : sizeof(DevTab<double>); }

// ---- OUTSETWMASK (outsetwmask.F90:57-75) on out[ij][ncol]: one thread per value; the sea-ice mask first, then the sea mask as written there
template <typename T>
__global__ void __launch_bounds__(256) k_outsetwmask(int kijs, int kijl, T* __restrict__ out, int ncol, OutMaskCols cols, const T* __restrict__ ff,
                                                     const int* __restrict__ iodp, int ice, T cithrsh, T zmiss) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nv = (size_t)(kijl - kijs) * ncol;
  if (i >= nv) return;
  const size_t r = i / ncol;
  const int c = (int)(i - r * ncol), cf = cols.f[c];
  const size_t ij = (size_t)kijs + r;
  if (!cf) return;
  T v = out[ij * ncol + c];
  if (ice && (cf & 1) && ff[ij * ECWAM_HIP_NFF + 2] > cithrsh) v = zmiss;
  if (cf & 2) {
    const int io = iodp[ij];
    v = v * T(io) + T(1 - io) * zmiss;
  }
  out[ij * ncol + c] = v;
}

template <typename T>
void launch_outsetwmask(int kijs, int kijl, void* out, int ncol, const OutMaskCols& cols, const void* ff, const int* iodp, int ice, double cithrsh,
                        double zmiss, hipStream_t s) {
  const size_t nv = (size_t)(kijl - kijs) * ncol;
  if (!nv) return;
  hipLaunchKernelGGL(k_outsetwmask<T>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, kijs, kijl, (T*)out, ncol, cols, (const T*)ff, iodp, ice,
                     (T)cithrsh, (T)zmiss);
}
template void launch_outsetwmask<float>(int, int, void*, int, const OutMaskCols&, const void*, const int*, int, double, double, hipStream_t);
template void launch_outsetwmask<double>(int, int, void*, int, const OutMaskCols&, const void*, const int*, int, double, double, hipStream_t);
