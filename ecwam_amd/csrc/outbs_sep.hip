// Wind-sea / swell separation and the mean-period / spread parameters of OUTBLOCK on the device (outblock.F90:214-382 with
// FL2ND = FL1, LLPARTITION = F): SEPWISW (sepwisw.F90) -- the wind-sea mask, the swell part MAX(FL1,EPSMIN)*SWM and the sea part --
// with FEMEAN, STHQ, MWP1, MWP2 and WDIRSPREAD (LLPEAKF = T: PEAKFRI + SCOSFL at the peak) of each part, and MWP1, MWP2 and
// WDIRSPREAD (LLPEAKF = F: SCOSFL at every frequency) of the total spectrum.  Reads FL1, XLLWS, CINV (WVPRPT[ij][2][:]), WDWAVE and
// UFRIC (FF[ij][1], FF[ij][7]); writes out[ij][15] in the column order of ecwam_hip.h.  Swell trains (SEP3TR) are not computed.
#include <algorithm>

#include "dev.h"
#include "launch.h"

__device__ __forceinline__ float m_fmod(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double m_fmod(double a, double b) { return fmod(a, b); }

// Per-wave LDS: the spectrum tile [M][NANG|1]; COSWDIF[K]; XINVWVAGE[M] = UFRIC*CINV(M); the final mask as one word per direction
// (bit M = SWM(K,M)); the first mask as a flat bit string over the row's [K][M] order (one ballot per 64 loaded bins, + 1 zero word).
struct SepLds {
  size_t cw, xi, msk, bits, bytes;
  __host__ __device__ SepLds(int NANG, int NFRE, size_t tsz) {
    const size_t nw = (size_t)(NANG * NFRE + 63) / 64 + 1;
    cw = ((size_t)NFRE * (NANG | 1) * tsz + 7) & ~(size_t)7;
    xi = cw + (size_t)NANG * tsz;
    msk = (xi + (size_t)NFRE * tsz + 7) & ~(size_t)7;
    bits = msk + (size_t)NANG * 8;
    bytes = (bits + nw * 8 + 15) & ~(size_t)15;
  }
};

// One wavefront per point, wpb points per workgroup.  lane = M sums over K in the reference's order (FEMEAN, MWP1/MWP2, PEAKFRI, the
// total spectrum's SCOSFL per frequency), lane = K sums over M (STHQ) and walks its mask word from NFRE down to 2.  The swell and sea
// parts are formed from the tile and the mask bits where they are summed; they never go to memory.  Contraction is off so that every
// product and sum is rounded where the reference rounds it (the reductions across lanes still add in wavefront order).
template <typename T>
__global__ void __launch_bounds__(256) k_outbs_sepwisw(const DevTab<T>* __restrict__ tp, int kijs, int kijl, int wpb, const T* __restrict__ fl1,
                                                       const T* __restrict__ xllws, const T* __restrict__ wvprpt, const T* __restrict__ ff, int flags,
                                                       T zmiss, T* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char sep_smem[];
  const DevTab<T>& tb = *tp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ij = kijs + blockIdx.x * wpb + wave;
  if (ij >= kijl) return;  // wave-uniform, no block barrier below
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE, NW = (N + 63) >> 6;
  const SepLds L(NANG, NFRE, sizeof(T));
  unsigned char* base = sep_smem + (size_t)wave * L.bytes;
  T* sF = reinterpret_cast<T*>(base);
  T* sCw = reinterpret_cast<T*>(base + L.cw);
  T* sXi = reinterpret_cast<T*>(base + L.xi);
  unsigned long long* sW = reinterpret_cast<unsigned long long*>(base + L.msk);
  unsigned long long* sB = reinterpret_cast<unsigned long long*>(base + L.bits);
  auto wsync = [] {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  const bool actm = lane < NFRE, actk = lane < NANG;
  const T EPS = tb.EPSMIN, DELTH = tb.DELTH;
  const T COEF = T(1.2) * tb.FRIC;  // OLDWSFC*FRIC, yowfred.F90:82, sepwisw.F90:146
  const T wdwave = ff[(size_t)ij * ECWAM_HIP_NFF + 1], ufric = ff[(size_t)ij * ECWAM_HIP_NFF + 7];
  const T* cinv = wvprpt + (size_t)ij * (ECWAM_HIP_NWPR * NFRE) + 2 * NFRE;
  // COSWDIF (outblock.F90:197-201) and XINVWVAGE (sepwisw.F90:148-152)
  const T cw = actk ? m_cos(tb.TH[lane] - wdwave) : T(0);
  if (actk) sCw[lane] = cw;
  if (actm) sXi[lane] = ufric * cinv[lane];
  wsync();
  // tile load; the first mask (sepwisw.F90:159-175) as the ballot of every 64 consecutive bins of the row.  The loads of SEP_U rounds of
  // 64 bins are issued before any of them is used: one memory latency per SEP_U rounds instead of one per round.
  constexpr int SEP_U = 8;
  const size_t row = (size_t)ij * N;
  for (int c0 = 0; c0 < N; c0 += 64 * SEP_U) {
    T fv[SEP_U], xv[SEP_U];
#pragma unroll
    for (int u = 0; u < SEP_U; u++) {
      const int e = min(c0 + 64 * u + lane, N - 1);  // in the row: no branch around the loads
      fv[u] = fl1[row + e];
      xv[u] = xllws[row + e];
    }
#pragma unroll
    for (int u = 0; u < SEP_U; u++) {
      const int b0 = c0 + 64 * u, e = b0 + lane;
      if (b0 >= N) break;  // wave-uniform
      bool keep = false;
      if (e < N) {
        const int kk = e / NFRE, mm = e - kk * NFRE;
        sF[mm * NAP + kk] = fv[u];
        keep = xv[u] == T(0) && !(sXi[mm] * (COEF * sCw[kk]) >= T(1));
      }
      const unsigned long long b = __ballot(keep);
      if (lane == 0) sB[b0 >> 6] = b;
    }
  }
  if (lane == 0) sB[NW] = 0;
  wsync();
  const unsigned long long fmask = (1ull << NFRE) - 1;
  unsigned long long w = 0;  // lane K: SWM(K, :)
  if (actk) {
    const int b = lane * NFRE, q = b >> 6, sh = b & 63;
    w = sB[q] >> sh;
    if (sh) w |= sB[q + 1] << (64 - sh);
    w &= fmask;
  }
  const int DF = NFRE / 2 - 1;  // 0-based first frequency of M >= NFRE/2 (sepwisw.F90:250)
  // the two parts of one bin: swell MAX(FL1,EPSMIN)*SWM (sepwisw.F90:223-229), sea MAX(FL1-F1 [+EPSMIN*COSWDIF**4], 0) (:246-256)
  auto parts = [&](T f, bool s, T c, int m, T& x1, T& x2) {
    x1 = s ? m_max(f, EPS) : T(0);
    T d = f - x1;
    if (c > T(0.8) && m >= DF) d = d + EPS * m_pow4(c);
    x2 = m_max(d, T(0));
  };
  auto femean_tail = [&](T em, T fm, T tl, T& E, T& F) {  // femean.F90:115-120
    E = em + tb.WETAIL * tb.FR[NFRE - 1] * DELTH * tl;
    F = fm + tb.FRTAIL * DELTH * tl;
    F = E / F;
    F = m_max(F, tb.FR[0]);
  };
  if (!(flags & 1)) {  // IF (.NOT. CLDOMAIN == 's'), sepwisw.F90:177-221
    T a = T(0), c = T(0);
    if (actm) {
      const T* p = sF + lane * NAP;
      for (int kk = 0; kk < NANG; kk++) {
        const int bi = kk * NFRE + lane;
        const bool s = (sB[bi >> 6] >> (bi & 63)) & 1ull;
        const T f = p[kk];
        const T f1 = s ? f : T(0);
        a = a + m_max(f1, EPS);
        c = c + m_max(m_max(f - f1, T(0)), EPS);
      }
    }
    T EMs, FMs, EMe, FMe, ESW, FSW, ESE, FSE;
    usum4(actm ? a * tb.DFIM[lane] : T(0), actm ? tb.DFIMOFR[lane] * a : T(0), actm ? c * tb.DFIM[lane] : T(0),
          actm ? tb.DFIMOFR[lane] * c : T(0), EMs, FMs, EMe, FMe);
    femean_tail(EMs, FMs, lane_get(a, NFRE - 1), ESW, FSW);
    femean_tail(EMe, FMe, lane_get(c, NFRE - 1), ESE, FSE);
    const bool R = FSW > T(0.96) * FSE;
    if (actk) {
      if (R) {  // the second mask; with R = 0 every CHECKTA is 0
        const T dc = COEF * m_sign(T(1), T(0.4) + cw);
        for (int m = 0; m < NFRE; m++)
          if (sXi[m] * dc >= T(1)) w &= ~(1ull << m);
      }
      // the walk from NFRE down to 2 (sepwisw.F90:208-219)
      for (int m = NFRE - 1; m >= 1; m--) {
        const bool s0 = (w >> m) & 1ull, s1 = (w >> (m - 1)) & 1ull;
        if (s0 && s1) break;
        if (!s0 && s1 && sF[m * NAP + lane] >= sF[(m - 1) * NAP + lane]) w &= ~(1ull << (m - 1));
      }
    }
  }
  if (actk) sW[lane] = w;
  wsync();
  // lane = M: FEMEAN / MWP / PEAKFRI sums of the swell (s), sea (e) and total (t) spectra, and SCOSFL of the total spectrum at M
  T s_fe = T(0), s_w = T(0), s_d = T(0), e_fe = T(0), e_w = T(0), e_d = T(0), t_fe = T(0), t_w = T(0), t_sc = T(0);
  if (actm) {
    const T* p = sF + lane * NAP;
    T si = T(0), ci = T(0);
    for (int kk = 0; kk < NANG; kk++) {
      const T f = p[kk];
      T x1, x2;
      parts(f, (sW[kk] >> lane) & 1ull, sCw[kk], lane, x1, x2);
      s_fe = s_fe + m_max(x1, EPS); s_w = s_w + x1; s_d = s_d + x1 * DELTH;
      e_fe = e_fe + m_max(x2, EPS); e_w = e_w + x2; e_d = e_d + x2 * DELTH;
      t_fe = t_fe + m_max(f, EPS); t_w = t_w + f;
      si = si + tb.SINTH[kk] * f;
      ci = ci + tb.COSTH[kk] * f;
    }
    const T md = (ci == T(0) && si == T(0)) ? T(0) : m_atan2(si, ci);  // scosfl.F90:77-83
    T mc = T(0);
    for (int kk = 0; kk < NANG; kk++) mc = mc + m_cos(tb.TH[kk] - md) * p[kk];
    t_sc = DELTH * mc;
  }
  const int MO = tb.NFRE_ODD;
  const bool acts = lane < MO;  // MWP1 / MWP2 sum M = 1 .. NFRE_ODD
  const T wsim = acts ? tb.DFIM_SIM[lane] : T(0);
  const T w1 = acts ? tb.DFIM_SIM[lane] * tb.FR[lane] : T(0);                    // DFIMFR_SIM
  const T w2 = acts ? tb.DFIM_SIM[lane] * (tb.FR[lane] * tb.FR[lane]) : T(0);    // DFIMFR2_SIM
  const T dfim = actm ? tb.DFIM[lane] : T(0), dfimofr = actm ? tb.DFIMOFR[lane] : T(0);
  T EMs, FMs, EMe, FMe, Es, M1s, M2s, Ee, M1e, M2e, Et, M1t, M2t, EMt, Wt, unused;
  usum4(s_fe * dfim, dfimofr * s_fe, e_fe * dfim, dfimofr * e_fe, EMs, FMs, EMe, FMe);
  usum4(wsim * s_w, w1 * s_w, w2 * s_w, wsim * e_w, Es, M1s, M2s, Ee);
  usum4(w1 * e_w, w2 * e_w, wsim * t_w, w1 * t_w, M1e, M2e, Et, M1t);
  usum4(w2 * t_w, t_fe * dfim, t_sc * dfim, T(0), M2t, EMt, Wt, unused);
  T PKs, PKe;
  umax2(actm ? s_d : T(0), actm ? e_d : T(0), PKs, PKe);
  // MWP1 / MWP2 (mwp1.F90:101-115, mwp2.F90:101-115): the tail from TEMP at NFRE_ODD
  const T fro = tb.FR[MO - 1], FR1M1 = T(1) / tb.FR[0];
  auto mwp = [&](T E, T M1, T M2, T tl, T& P1, T& P2) {
    E = E + tb.WETAIL * fro * DELTH * tl;
    M1 = M1 + tb.WP1TAIL * DELTH * (fro * fro) * tl;
    M2 = M2 + T(0.5) * DELTH * (fro * fro * fro) * tl;  // WP2TAIL = 0.5, yowfred.F90:54
    P1 = (E > T(0) && M1 > EPS) ? m_min(E / M1, FR1M1) : T(0);
    P2 = (E > T(0) && M2 > EPS) ? m_min(m_sqrt(E / M2), FR1M1) : T(0);
  };
  T P1s, P2s, P1e, P2e, P1t, P2t;
  mwp(Es, M1s, M2s, lane_get(s_w, MO - 1), P1s, P2s);
  mwp(Ee, M1e, M2e, lane_get(e_w, MO - 1), P1e, P2e);
  mwp(Et, M1t, M2t, lane_get(t_w, MO - 1), P1t, P2t);
  T ESW, FSW, ESE, FSE;
  femean_tail(EMs, FMs, lane_get(s_fe, NFRE - 1), ESW, FSW);
  femean_tail(EMe, FMe, lane_get(e_fe, NFRE - 1), ESE, FSE);
  // WDIRSPREAD of the total spectrum, LLPEAKF = F (wdirspread.F90:95-115) with EMEAN = EM of FEMEAN
  const T EMEAN = EMt + tb.WETAIL * tb.FR[NFRE - 1] * DELTH * lane_get(t_fe, NFRE - 1);
  T wdt = Wt / DELTH + lane_get(t_sc, NFRE - 1) * (tb.WETAIL * tb.FR[NFRE - 1]);
  wdt = EMEAN > EPS ? m_min(wdt / EMEAN, T(1)) : T(1);
  wdt = m_sqrt(T(2) * (T(1) - wdt));
  // PEAKFRI of the parts: the first frequency of the largest F1D, NFRE if all are 0 (peakfri.F90:64-86)
  const unsigned long long bs = __ballot(actm && PKs > T(0) && s_d == PKs), be = __ballot(actm && PKe > T(0) && e_d == PKe);
  const int ips = bs ? __ffsll((long long)bs) - 1 : NFRE - 1, ipe = be ? __ffsll((long long)be) - 1 : NFRE - 1;
  // lane = K: STHQ sums of the parts (sthq.F90:76-90) and the parts at the peak frequencies
  T ts = T(0), te = T(0), ks = T(0), ke = T(0);
  if (actk) {
    for (int m = 0; m < NFRE; m++) {
      T x1, x2;
      parts(sF[m * NAP + lane], (w >> m) & 1ull, cw, m, x1, x2);
      ts = ts + x1 * tb.DFIM[m];
      te = te + x2 * tb.DFIM[m];
    }
    T x1, x2;
    parts(sF[ips * NAP + lane], (w >> ips) & 1ull, cw, ips, x1, x2);
    ks = x1;
    parts(sF[ipe * NAP + lane], (w >> ipe) & 1ull, cw, ipe, x1, x2);
    ke = x2;
  }
  const T sth = actk ? tb.SINTH[lane] : T(0), cth = actk ? tb.COSTH[lane] : T(0);
  T SIs, CIs, SIe, CIe, SKs, CKs, SKe, CKe;
  usum4(sth * ts, cth * ts, sth * te, cth * te, SIs, CIs, SIe, CIe);
  usum4(sth * ks, cth * ks, sth * ke, cth * ke, SKs, CKs, SKe, CKe);
  auto sthq = [&](T si, T ci) {
    if (ci == T(0)) ci = EPS;
    T th = m_atan2(si, ci);
    if (th < T(0)) th = th + tb.ZPI;
    return th;
  };
  const T THSW = sthq(SIs, CIs);
  const T THSE = ESE <= T(1.0e-9) ? wdwave : sthq(SIe, CIe);  // sepwisw.F90:260-264
  // SCOSFL at the peak (scosfl.F90:71-92) and WDIRSPREAD with LLPEAKF = T (wdirspread.F90:86-94)
  const T mds = (CKs == T(0) && SKs == T(0)) ? T(0) : m_atan2(SKs, CKs);
  const T mde = (CKe == T(0) && SKe == T(0)) ? T(0) : m_atan2(SKe, CKe);
  T MCs, MCe;
  usum2(actk ? m_cos(tb.TH[lane] - mds) * ks : T(0), actk ? m_cos(tb.TH[lane] - mde) * ke : T(0), MCs, MCe);
  auto spread = [&](T mc, T pk) {
    T s = DELTH * mc;
    s = pk > T(0) ? m_min(s / pk, T(1)) : T(1);
    return m_sqrt(T(2) * (T(1) - s));
  };
  const T SPs = spread(MCs, PKs), SPe = spread(MCe, PKe);
  if (lane == 0) {
    T* o = out + (size_t)ij * 15;
    const T DEG = T(57.295778667);  // yowpcons.F90:31
    o[0] = P1t;
    o[1] = P2t;
    o[2] = wdt;
    o[3] = T(4) * m_sqrt(m_max(ESE, T(0)));
    o[4] = T(4) * m_sqrt(m_max(ESW, T(0)));
    o[5] = m_fmod(DEG * THSE + T(180), T(360));  // Fortran MOD: the sign of the dividend
    o[6] = m_fmod(DEG * THSW + T(180), T(360));
    o[7] = FSE > T(0) ? T(1) / FSE : zmiss;
    o[8] = FSW > T(0) ? T(1) / FSW : zmiss;
    o[9] = P1e;
    o[10] = P1s;
    o[11] = P2e;
    o[12] = P2s;
    o[13] = SPe;
    o[14] = SPs;
  }
}

// The same spectral sizes as launch_outbs (four tiles <= 64 KiB); as many waves per workgroup as fit in 64 KiB with the masks.
template <typename T>
int launch_outbs_sepwisw(const void* tab, int kijs, int kijl, const void* fl1, const void* xllws, const void* wvprpt, const void* ff, int flags,
                         double zmiss, void* out, int NANG, int NFRE, hipStream_t s) {
  const int n = kijl - kijs;
  if (n <= 0) return 0;
  if (!outbs_size_ok(NANG, NFRE, sizeof(T))) return 1;
  const SepLds L(NANG, NFRE, sizeof(T));
  const int wpb = (int)std::min<size_t>(4, (size_t)64 * 1024 / L.bytes);
  hipLaunchKernelGGL(k_outbs_sepwisw<T>, dim3((n + wpb - 1) / wpb), dim3(64 * wpb), wpb * L.bytes, s, (const DevTab<T>*)tab, kijs, kijl, wpb,
                     (const T*)fl1, (const T*)xllws, (const T*)wvprpt, (const T*)ff, flags, (T)zmiss, (T*)out);
  return 0;
}
template int launch_outbs_sepwisw<float>(const void*, int, int, const void*, const void*, const void*, const void*, int, double, void*, int, int, hipStream_t);
template int launch_outbs_sepwisw<double>(const void*, int, int, const void*, const void*, const void*, const void*, int, double, void*, int, int, hipStream_t);
