// SEPWISW (sepwisw.F90) of OUTBLOCK on the device (outblock.F90:214-382 and 436-449 with FL2ND = FL1), one kernel template built twice per
// precision:
//   TRAINS = false  LLPARTITION = F (ecwam_hip_outbs_sepwisw): the wind-sea mask, the swell part MAX(FL1,EPSMIN)*SWM and the sea part, with
//                   FEMEAN, STHQ, MWP1, MWP2 and WDIRSPREAD (LLPEAKF = T: PEAKFRI + SCOSFL at the peak) of each part, and MWP1, MWP2 and
//                   WDIRSPREAD (LLPEAKF = F: SCOSFL at every frequency) of the total spectrum.  Reads FL1, XLLWS, CINV (WVPRPT[ij][2][:]),
//                   WDWAVE and UFRIC (FF[ij][1], FF[ij][7]); writes out[ij][15] in the column order of ecwam_hip.h.
//   TRAINS = true   LLPARTITION = T (ecwam_hip_outbs_partition): the same with SEP3TR (sep3tr.F90), FNDPRT (fndprt.F90) and PARMEAN
//                   (parmean.F90).  Reads MIJ as well; writes out[ij][24]: those 15 columns, then height, direction and period of swell
//                   trains 1..3 (parameters 42-50).  CLDOMAIN = 's' is refused before the launch: SEP3TR would read an FSEA that SEPWISW
//                   has not computed.
//
// SEP3TR leaves the swell mask as it was.  FNDPRT multiplies SWM by MAX(W1,1), but W1 never exceeds 1: a bin starts at W1 = 0 or 1 and
// each peak adds its W2 once; W2 = 1 needs W1 < 0.5 (the seed's centre W1 < 0.25, step 2.b W1 < 0.5) and W2 = 0.5 needs W1 <= 0.5 (the
// seed) or W1 < 1 (step 2.c), so W1 + W2 <= 1 for every peak and for the extra partition (W1 <= 0 -> 1).  MAX(W1,1) = 1, FLSW after
// FNDPRT is the swell spectrum before it, and SEPWISW 2.2 and 3 give what they give with LLPARTITION = F.  The first 15 columns are
// therefore the same code in both builds (CLDOMAIN /= 's'); W1 is held as the classes 0, 0.5 and >= 1.
//
// Layout: one wavefront per point.  The spectrum tile [M][NANG|1] and, with TRAINS, SEP3TR's smoothed swell spectrum FL [M][NANG|1] sit in
// LDS.  FNDPRT runs with lane = M on 64-bit direction words (bit K): W2 as two bit planes (0.5, 1), W1 as two (= 0, = 0.5), LLW3, and one
// "the neighbour (K+dk, M+dm) is larger" word per neighbour offset, built once per point.  Within a sweep neither step depends on the order
// in which the reference visits the bins, so a sweep is two whole-plane updates (2.b, then 2.c): 2.b only turns W2 = 0.5 into 1 and reads
// W2 = 0.5 of the bin and W2 = 0 of its neighbours, which that change leaves alone; 2.c only turns W2 = 0 into 0.5 and reads W2 = 0 of the
// bin itself and W2 = 1 of its neighbours, which that change leaves alone.  The words of M +- 1 come from the neighbouring lanes.  PARMEAN
// sums each partition with lane = M (over K, in the reference's order) and lane = K (over M: the W2 planes go through LDS).  The peaks'
// ENE / DIR / PER live in lane IP of three registers.
//
// LDS per wave (SepLds) with TRAINS: two tiles NFRE x (NANG|1) reals, COSWDIF[NANG] and XINVWVAGE[NFRE], the mask words [NANG], the first
// mask's bits and three words per frequency.  At 36 x 36: 12.3 KB (sp) / 23.2 KB (dp).  As many waves per workgroup as fit in 64 KB (sp 4,
// dp 2), so the 160 KB of a CU hold 3 workgroups: 12 waves (3 per SIMD) in sp, 6 (1.5 per SIMD) in dp.  Registers would allow 4 (sp, 126
// VGPRs) and 2 (dp, 188 VGPRs) waves per SIMD.  At 48 x 36 dp (29.6 KB): 2-wave workgroups, 2 per CU.  Without TRAINS: one tile and no
// words per frequency.
#include <algorithm>

#include "dev.h"
#include "launch.h"

namespace {

__device__ __forceinline__ float m_fmod(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double m_fmod(double a, double b) { return fmod(a, b); }
__device__ __forceinline__ unsigned long long p_shfl(unsigned long long v, int src) {
  const int lo = __shfl((int)(unsigned)(v & 0xffffffffull), src), hi = __shfl((int)(unsigned)(v >> 32), src);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// Per-wave LDS: the spectrum tile [M][NANG|1]; with trains, SEP3TR's FL tile; COSWDIF[K]; XINVWVAGE[M] = UFRIC*CINV(M); the final mask as
// one word per direction (bit M = SWM(K,M)); the first mask as a flat bit string over the row's [K][M] order (one ballot per 64 loaded
// bins, + 1 zero word); with trains, three words per frequency: W2 = 0.5, W2 = 1 (or the assigned bins), the peaks.
struct SepLds {
  size_t fs, cw, xi, msk, bits, pw, bytes;
  __host__ __device__ SepLds(int NANG, int NFRE, size_t tsz, bool trains) {
    const size_t nw = (size_t)(NANG * NFRE + 63) / 64 + 1;
    const size_t tile = ((size_t)NFRE * (NANG | 1) * tsz + 7) & ~(size_t)7;
    fs = tile;
    cw = trains ? 2 * tile : tile;
    xi = cw + (size_t)NANG * tsz;
    msk = (xi + (size_t)NFRE * tsz + 7) & ~(size_t)7;
    bits = msk + (size_t)NANG * 8;
    pw = bits + nw * 8;
    bytes = ((trains ? pw + (size_t)3 * NFRE * 8 : pw) + 15) & ~(size_t)15;
  }
};

constexpr int NPMAX = 20, NTRAIN = 3;

}  // namespace

// One wavefront per point, wpb points per workgroup.  lane = M sums over K in the reference's order (FEMEAN, MWP1/MWP2, PEAKFRI, the
// total spectrum's SCOSFL per frequency), lane = K sums over M (STHQ) and walks its mask word from NFRE down to 2.  The swell and sea
// parts are formed from the tile and the mask bits where they are summed; they never go to memory.  Contraction is off so that every
// product and sum is rounded where the reference rounds it (the reductions across lanes still add in wavefront order).
template <typename T, bool TRAINS>
__global__ void __launch_bounds__(256) k_outbs_sepwisw(const DevTab<T>* __restrict__ tp, int kijs, int kijl, int wpb, const T* __restrict__ fl1,
                                                       const T* __restrict__ xllws, const int* __restrict__ mijp, const T* __restrict__ wvprpt,
                                                       const T* __restrict__ ff, int flags, T zmiss, T* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char sep_smem[];
  const DevTab<T>& tb = *tp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ij = kijs + blockIdx.x * wpb + wave;
  if (ij >= kijl) return;  // wave-uniform, no block barrier below
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE, NW = (N + 63) >> 6;
  const SepLds L(NANG, NFRE, sizeof(T), TRAINS);
  unsigned char* base = sep_smem + (size_t)wave * L.bytes;
  T* sF = reinterpret_cast<T*>(base);
  T* sS = reinterpret_cast<T*>(base + L.fs);  // trains only, like sH, sO and sP
  T* sCw = reinterpret_cast<T*>(base + L.cw);
  T* sXi = reinterpret_cast<T*>(base + L.xi);
  unsigned long long* sW = reinterpret_cast<unsigned long long*>(base + L.msk);
  unsigned long long* sB = reinterpret_cast<unsigned long long*>(base + L.bits);
  unsigned long long* sH = reinterpret_cast<unsigned long long*>(base + L.pw);
  unsigned long long* sO = sH + NFRE;
  unsigned long long* sP = sO + NFRE;
  auto wsync = [] {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  const bool actm = lane < NFRE, actk = lane < NANG;
  const T EPS = tb.EPSMIN, DELTH = tb.DELTH;
  const T COEF = T(1.2) * tb.FRIC;  // OLDWSFC*FRIC, yowfred.F90:82, sepwisw.F90:146
  const T wdwave = ff[(size_t)ij * ECWAM_HIP_NFF + 1], ufric = ff[(size_t)ij * ECWAM_HIP_NFF + 7];
  const T* cinv = wvprpt + (size_t)ij * (ECWAM_HIP_NWPR * NFRE) + 2 * NFRE;
  const int MIJ = TRAINS ? min(max(mijp[ij], 1), NFRE) : NFRE;  // 1-based; clamped so that no table is read outside its row
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
  T FSEA1 = T(0);                             // FSEA of sepwisw.F90:184, which SEP3TR's fall-back reads
  if (!(!TRAINS && (flags & 1))) {            // IF (.NOT. CLDOMAIN == 's'), sepwisw.F90:177-221; never 's' with trains
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
    T EMs, FMs, EMe, FMe, ESW, FSW, ESE;
    usum4(actm ? a * tb.DFIM[lane] : T(0), actm ? tb.DFIMOFR[lane] * a : T(0), actm ? c * tb.DFIM[lane] : T(0),
          actm ? tb.DFIMOFR[lane] * c : T(0), EMs, FMs, EMe, FMe);
    femean_tail(EMs, FMs, lane_get(a, NFRE - 1), ESW, FSW);
    femean_tail(EMe, FMe, lane_get(c, NFRE - 1), ESE, FSEA1);
    const bool R = FSW > T(0.96) * FSEA1;
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
  // SEPWISW 2.2 and 3 (with trains the swell mask is still the one above, see the header).  lane = M: FEMEAN / MWP / PEAKFRI sums of the
  // swell (s), sea (e) and total (t) spectra, and SCOSFL of the total spectrum at M
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
  T EMs, FMs, EMe, FMe, Es, M1s, M2s, Ee, M1e, M2e, Et, M1t, M2t, EMt, Wt, ETTs;
  usum4(s_fe * dfim, dfimofr * s_fe, e_fe * dfim, dfimofr * e_fe, EMs, FMs, EMe, FMe);
  usum4(wsim * s_w, w1 * s_w, w2 * s_w, wsim * e_w, Es, M1s, M2s, Ee);
  usum4(w1 * e_w, w2 * e_w, wsim * t_w, w1 * t_w, M1e, M2e, Et, M1t);
  usum4(w2 * t_w, t_fe * dfim, t_sc * dfim, TRAINS ? dfim * s_w : T(0), M2t, EMt, Wt, ETTs);
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
  // ETT = SEMEAN of FLSW without EPSMIN (sep3tr.F90, semean.F90): sum_K of the swell part per frequency = s_w
  const T DELT25 = tb.WETAIL * tb.FR[NFRE - 1] * DELTH;
  const T ETT = TRAINS ? ETTs + DELT25 * lane_get(s_w, NFRE - 1) : T(0);
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
  const T DEG = T(57.295778667);  // yowpcons.F90:31
  T* o = out + (size_t)ij * (TRAINS ? 24 : 15);
  if (lane == 0) {
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

  if constexpr (TRAINS) {
    // ---- SEP3TR set-up, lane = M: the swell spectrum FLSW = MAX(FL1,EPSMIN)*SWM smoothed over directions into FL (sS) -----------------
    const unsigned long long kmask = NANG == 64 ? ~0ull : (1ull << NANG) - 1;
    const int M0 = lane;  // 0-based frequency of this lane
    T enmax = T(0);
    unsigned long long pos = 0, w3 = 0;  // FL > 0, FL > FLLOW (LLW3)
    if (actm) {
      const T* p = sF + M0 * NAP;
      auto flsw = [&](int k) { return ((sW[k] >> M0) & 1ull) ? m_max(p[k], EPS) : T(0); };
      T prv = flsw(NANG - 1), cur = flsw(0);
      for (int k = 0; k < NANG; k++) {
        const T nxt = flsw(k + 1 < NANG ? k + 1 : 0);
        T v = T(0);
        if (cur > T(0)) {
          v = T(0.10) * (prv + nxt) + T(0.80) * cur;
          enmax = m_max(enmax, v);
        }
        sS[M0 * NAP + k] = v;
        pos |= (unsigned long long)(v > T(0)) << k;
        w3 |= (unsigned long long)(v > tb.FLMIN) << k;
        prv = cur;
        cur = nxt;
      }
    }
    const T FLNOISE = T(0.005) * umax(enmax);  // XNOISELEVEL * ENMAX
    const T LOWEST = m_max(tb.FLMIN, FLNOISE);
    wsync();
    // the neighbour words: gt[j] bit K = FL(K+dk, M+dm) > FL(K, M) where that neighbour exists, j over the 8 offsets (dk, dm) != (0, 0);
    // the peaks (sep3tr.F90): FL > MAX(FLLOW, FLNOISE), all 8 neighbours > 0 and <= FL, M = 2 .. MIJ-1; and FL > FLNOISE (the extra partition)
    unsigned long long gt[8], pk = 0, abn = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) gt[j] = 0;
    if (actm) {
      const bool hasl = M0 > 0, hash = M0 + 1 < NFRE;
      bool inr = M0 >= 1 && M0 <= MIJ - 2;
      for (int k = 0; k < NANG; k++) {
        const int kl = k == 0 ? NANG - 1 : k - 1, kh = k + 1 == NANG ? 0 : k + 1;
        const T c = sS[M0 * NAP + k];
        T v[8];
        bool ex[8];
        const int kn[3] = {kl, k, kh};
        int j = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
          for (int dm = -1; dm <= 1; dm++) {
            if (a == 1 && dm == 0) continue;
            const bool e = dm < 0 ? hasl : (dm > 0 ? hash : true);
            ex[j] = e;
            v[j] = e ? sS[(M0 + dm) * NAP + kn[a]] : T(0);
            j++;
          }
        }
        bool peak = inr && c > LOWEST;
#pragma unroll
        for (int q = 0; q < 8; q++) {
          if (ex[q] && v[q] > c) gt[q] |= 1ull << k;
          peak = peak && v[q] > T(0) && c >= v[q];
        }
        pk |= (unsigned long long)peak << k;
        abn |= (unsigned long long)(c > FLNOISE) << k;
      }
      sP[M0] = pk;
    }
    // gt[] order: (dk,dm) = (-1,-1) (-1,0) (-1,+1) (0,-1) (0,+1) (+1,-1) (+1,0) (+1,+1)
    auto rotm = [&](unsigned long long x) {  // bit K <- bit K-1 (the neighbour K-1 seen from K)
      return ((x << 1) & kmask) | ((x >> (NANG - 1)) & 1ull);
    };
    auto rotp = [&](unsigned long long x) {  // bit K <- bit K+1
      return (x >> 1) | ((x & 1ull) << (NANG - 1));
    };
    // the words of M-1 and M+1 (0 where that frequency does not exist); every lane takes part in the shuffles
    auto from_lo = [&](unsigned long long x) {
      const unsigned long long y = p_shfl(x, lane > 0 ? lane - 1 : 0);
      return M0 > 0 ? y : 0ull;
    };
    auto from_hi = [&](unsigned long long x) {
      const unsigned long long y = p_shfl(x, lane < 63 ? lane + 1 : 63);
      return M0 + 1 < NFRE ? y : 0ull;
    };
    // OR over the 8 neighbours of a plane, or of a plane masked by gt[]
    auto nbr_or = [&](unsigned long long x, bool withgt) {
      const unsigned long long lo = from_lo(x), hi = from_hi(x);
      const unsigned long long s[8] = {rotm(lo), rotm(x), rotm(hi), lo, hi, rotp(lo), rotp(x), rotp(hi)};
      unsigned long long r = 0;
#pragma unroll
      for (int q = 0; q < 8; q++) r |= withgt ? (s[q] & gt[q]) : s[q];
      return r;
    };
    wsync();
    // ---- the peaks in discovery order (M-major, then K), at most NPMAX ----------------------------------------------------------------------
    const int nfound = (int)usum(actm ? T(__popcll(pk)) : T(0));  // at most 63 x 64: exact in either precision
    int npeak = min(nfound, NPMAX);
    // ---- FNDPRT -------------------------------------------------------------------------------------------------------------------------
    const int NANGH = m_nint((T(75.0) / T(360.0)) * T(NANG)) + 1;  // NINT: half away from zero
    unsigned long long z1 = w3, h1 = 0, asg = 0;                       // W1 = 0, W1 = 0.5 (W1 = 1 elsewhere); assigned bins
    const unsigned long long bw3 = __ballot(w3 != 0);
    int mmin = bw3 ? __ffsll((long long)bw3) - 1 : NFRE - 1;
    int mmax = bw3 ? 63 - __clzll((long long)bw3) : -1;
    T r_ene = T(0), r_dir = T(0), r_per = T(0);  // lane IP (1-based): ENE, DIR, PER of partition IP
    // PARMEAN of the partition W2 = h2 (0.5) | o2 (1) into lane ip
    auto parmean = [&](unsigned long long h2, unsigned long long o2, int ip) {
      if (actm) {
        sH[M0] = h2;
        sO[M0] = o2;
      }
      wsync();
      T f1d = T(0);
      if (actm) {
        const T* p = sS + M0 * NAP;
        for (int k = 0; k < NANG; k++) {
          const T wt = ((o2 >> k) & 1ull) ? T(1) : (((h2 >> k) & 1ull) ? T(0.5) : T(0));
          f1d = f1d + p[k] * wt;
        }
      }
      T tmp = T(0);
      if (actk) {
        for (int m = 0; m < NFRE; m++) {
          const T wt = ((sO[m] >> lane) & 1ull) ? T(1) : (((sH[m] >> lane) & 1ull) ? T(0.5) : T(0));
          tmp = tmp + (sS[m * NAP + lane] * wt) * tb.DFIM[m];
        }
      }
      // the sums across lanes add in wavefront order, and CI = 0 -> EPSMIN is tested on the total, not after every K: the reference's
      // mid-sum test only matters where a partial sum of CI is exactly 0, and then moves CI by EPSMIN (1e-33)
      T em, fm, si, ci;
      usum4(f1d * dfim, f1d * dfimofr, sth * tmp, cth * tmp, em, fm, si, ci);
      em = EPS + em;
      fm = EPS + fm;
      if (ci == T(0)) ci = EPS;
      T th = m_atan2(si, ci);
      if (th < T(0)) th = th + tb.ZPI;
      if (lane == ip && em > EPS) {
        r_ene = em;
        r_per = fm / em;
        r_dir = th;
      }
      wsync();
    };
    int cm = -1;
    unsigned long long cur = 0;
    for (int ip = 1; ip <= npeak; ip++) {
      while (cur == 0) cur = sP[++cm];  // wave-uniform: the next peak
      const int kc = __ffsll((long long)cur) - 1, mc = cm;
      cur &= cur - 1;
      unsigned long long sec = 0;
      for (int d = -NANGH; d <= NANGH; d++) sec |= 1ull << (((kc + d) % NANG + NANG) % NANG);
      const unsigned long long kc3 = (1ull << kc) | (1ull << (kc == 0 ? NANG - 1 : kc - 1)) | (1ull << (kc + 1 == NANG ? 0 : kc + 1));
      unsigned long long h2 = 0, o2 = 0;
      if (M0 >= mc - 1 && M0 <= mc + 1) h2 = kc3 & (z1 | h1);  // the 3 x 3 seed: W1 <= 0.5
      if (M0 == mc && ((z1 >> kc) & 1ull)) {                   // the centre: W1 < 0.25
        o2 = 1ull << kc;
        h2 &= ~o2;
      }
      // MMAX: the highest M in MMIN .. MMAX with a sector bin at W1 < 1
      const unsigned long long bm = __ballot(actm && M0 >= mmin && M0 <= mmax && ((z1 | h1) & sec) != 0);
      if (bm) mmax = 63 - __clzll((long long)bm);
      const bool actb = actm && M0 >= mmin && M0 <= min(MIJ - 1, mmax), actc = actm && M0 >= mmin && M0 <= mmax;
      for (int nitt = 1; nitt <= 25; nitt++) {
        const unsigned long long zero2 = kmask & ~(h2 | o2);
        // 2.b: W2 = 0.5 -> 1 where W1 = 0 and no neighbour at W2 = 0 is larger
        const unsigned long long blk = nbr_or(zero2, true);
        const unsigned long long addb = actb ? (w3 & sec & h2 & z1 & ~blk) : 0ull;
        o2 |= addb;
        h2 &= ~addb;
        // 2.c: W2 = 0 -> 0.5 where W1 < 1 and a neighbour has W2 = 1
        const unsigned long long one = nbr_or(o2, false);
        const unsigned long long addc = actc ? (w3 & (z1 | h1) & sec & zero2 & one) : 0ull;
        h2 |= addc;
        if (!__ballot((addb | addc) != 0)) break;
      }
      // W1 = W1 + W2 (it stays <= 1: see the header)
      const unsigned long long w2 = h2 | o2;
      h1 = (h1 & ~w2) | (z1 & h2);
      z1 &= ~w2;
      parmean(h2, o2, ip);
      asg |= w2 & pos;
    }
    // the extra partition in the wind sector against the wind (COSWDIF < -0.4), while NPEAK < NPMAX
    if (npeak < NPMAX) {
      const unsigned long long llc = __ballot(actk && cw < T(-0.4));
      const unsigned long long o2 = actm ? (llc & z1 & abn) : 0ull;
      if (__ballot(o2 != 0)) {
        z1 &= ~o2;
        npeak++;
        parmean(0ull, o2, npeak);
        asg |= o2 & pos;
      }
    }
    // ---- SEP3TR tail ----------------------------------------------------------------------------------------------------------------------
    T sumene = T(0);
    for (int ip = 1; ip <= npeak; ip++) sumene = sumene + lane_get(r_ene, ip);
    // the unassigned part SUNASGN = FL outside the partitions: FEMEAN, then SEMEAN overwriting E, then STHQ
    if (actm) sO[M0] = asg;
    wsync();
    T ua = T(0), ub = T(0), uk = T(0);
    if (actm) {
      const T* p = sS + M0 * NAP;
      for (int k = 0; k < NANG; k++) {
        const T f = ((asg >> k) & 1ull) ? T(0) : p[k];
        ua = ua + m_max(f, EPS);
        ub = ub + f;
      }
    }
    if (actk) {
      for (int m = 0; m < NFRE; m++) uk = uk + (((sO[m] >> lane) & 1ull) ? T(0) : sS[m * NAP + lane]) * tb.DFIM[m];
    }
    T UEM, UFM, UE, USI, UCI, unused;
    usum4(ua * dfim, dfimofr * ua, dfim * ub, sth * uk, UEM, UFM, UE, USI);
    usum2(cth * uk, T(0), UCI, unused);
    T EUN0, FUN;
    femean_tail(UEM, UFM, lane_get(ua, NFRE - 1), EUN0, FUN);
    const T EUN = UE + DELT25 * lane_get(ub, NFRE - 1);
    const T THUN = sthq(USI, UCI);
    const int NPKNA = EUN > sumene ? NTRAIN : NTRAIN - 1;
    if (npeak < NPKNA && EUN > T(0)) {
      npeak++;
      if (lane == npeak) {
        r_ene = EUN;
        r_dir = THUN;
        r_per = T(1) / FUN;
      }
    }
    // the HSMIN / period removal: FRINVMIJ is an INTEGER in sep3tr.F90, 1/FR(MIJ) truncated
    const int FRINVMIJ = (int)(T(1) / tb.FR[MIJ - 1]);
    {
      const T hsmin = T(0.05) + T(-0.0017) * r_per;
      const T thrs = T(0.0625) * (hsmin * hsmin);
      const bool drop = lane >= 1 && lane <= npeak && (r_ene < thrs || r_per < T(FRINVMIJ));
      if (drop) r_ene = r_dir = r_per = T(0);
      const int npk = npeak - __popcll(__ballot(drop));
      if (npk <= 0 && ESW > T(0) && FSW < FSEA1) {  // the total swell instead
        npeak = 1;
        if (lane == 1) {
          r_ene = ESW;
          r_dir = THSW;
          r_per = T(1) / FSW;
        }
      }
    }
    if (lane == 0 || lane > NPMAX) r_ene = r_dir = r_per = T(0);  // entry 0 of the reference's 0:NPMAX arrays
    // the first energy sort: the first of the largest ENE > 0, then that entry set to 0
    T em[NTRAIN], th[NTRAIN], pm[NTRAIN];
    int ien[NTRAIN];
    for (int s = 0; s < NTRAIN; s++) {
      const T mx = umax(r_ene);
      const unsigned long long b = __ballot(mx > T(0) && r_ene == mx);
      const int ipn = mx > T(0) && b ? __ffsll((long long)b) - 1 : 0;
      em[s] = lane_get(r_ene, ipn);
      th[s] = lane_get(r_dir, ipn);
      pm[s] = lane_get(r_per, ipn);
      if (lane == ipn) r_ene = T(0);
      ien[s] = min(ipn, 1);
    }
    T sumet = m_max(em[0], EPS);
    for (int s = 1; s < NTRAIN; s++) sumet = sumet + em[s];
    const T enex = npeak >= NPKNA ? m_max(ETT - sumet, T(0)) / sumet : T(0);
    for (int s = 0; s < NTRAIN; s++) em[s] = em[s] + enex * em[s];
    // the second sort over the three trains
    T xe[NTRAIN] = {em[0], em[1], em[2]}, xd[NTRAIN] = {th[0], th[1], th[2]}, xq[NTRAIN] = {pm[0], pm[1], pm[2]};
    for (int s = 0; s < NTRAIN; s++) {
      int ipn = -1;
      T mx = T(0);
      for (int q = 0; q < NTRAIN; q++)
        if (xe[q] > mx) {
          ipn = q;
          mx = xe[q];
        }
      const int ipl = max(ipn, 0);
      em[s] = xe[ipl];
      th[s] = xd[ipl];
      pm[s] = xq[ipl];
      xe[ipl] = T(0);
    }
    if (lane == 0) {
      for (int s = 0; s < NTRAIN; s++) {
        const bool z = ien[s] == 0;
        const T e = z ? T(0) : em[s], d = z ? wdwave : th[s], p = z ? T(0) : pm[s];
        o[15 + 3 * s] = T(4) * m_sqrt(m_max(e, T(0)));
        o[16 + 3 * s] = m_fmod(DEG * d + T(180), T(360));
        o[17 + 3 * s] = p;
      }
    }
  }
}

namespace {

// As many waves per workgroup (up to 4) as fit in 64 KiB with the masks (and, with trains, the second tile and the word planes).
template <typename T, bool TRAINS>
void launch_sepwisw(const SepLds& L, const void* tab, int kijs, int kijl, const void* fl1, const void* xllws, const int* mij, const void* wvprpt,
                    const void* ff, int flags, double zmiss, void* out, hipStream_t s) {
  const int n = kijl - kijs, wpb = (int)std::min<size_t>(4, (size_t)64 * 1024 / L.bytes);
  hipLaunchKernelGGL((k_outbs_sepwisw<T, TRAINS>), dim3((n + wpb - 1) / wpb), dim3(64 * wpb), wpb * L.bytes, s, (const DevTab<T>*)tab, kijs, kijl,
                     wpb, (const T*)fl1, (const T*)xllws, mij, (const T*)wvprpt, (const T*)ff, flags, (T)zmiss, (T*)out);
}

}  // namespace

// The same spectral sizes as launch_outbs (four tiles <= 64 KiB).
template <typename T>
int launch_outbs_sepwisw(const void* tab, int kijs, int kijl, const void* fl1, const void* xllws, const void* wvprpt, const void* ff, int flags,
                         double zmiss, void* out, int NANG, int NFRE, hipStream_t s) {
  if (kijl <= kijs) return 0;
  if (!outbs_size_ok(NANG, NFRE, sizeof(T))) return 1;
  launch_sepwisw<T, false>(SepLds(NANG, NFRE, sizeof(T), false), tab, kijs, kijl, fl1, xllws, nullptr, wvprpt, ff, flags, zmiss, out, s);
  return 0;
}
template int launch_outbs_sepwisw<float>(const void*, int, int, const void*, const void*, const void*, const void*, int, double, void*, int, int, hipStream_t);
template int launch_outbs_sepwisw<double>(const void*, int, int, const void*, const void*, const void*, const void*, int, double, void*, int, int, hipStream_t);

// The spectral sizes of launch_outbs_sepwisw whose two tiles and word planes fit in 64 KiB.
template <typename T>
int launch_outbs_partition(const void* tab, int kijs, int kijl, const void* fl1, const void* xllws, const int* mij, const void* wvprpt,
                           const void* ff, double zmiss, void* out, int NANG, int NFRE, hipStream_t s) {
  if (!outbs_size_ok(NANG, NFRE, sizeof(T))) return 1;
  if (kijl <= kijs) return 0;
  const SepLds L(NANG, NFRE, sizeof(T), true);
  if (L.bytes > 64 * 1024) return 1;
  launch_sepwisw<T, true>(L, tab, kijs, kijl, fl1, xllws, mij, wvprpt, ff, 0, zmiss, out, s);
  return 0;
}
template int launch_outbs_partition<float>(const void*, int, int, const void*, const void*, const int*, const void*, const void*, double, void*, int,
                                           int, hipStream_t);
template int launch_outbs_partition<double>(const void*, int, int, const void*, const void*, const int*, const void*, const void*, double, void*,
                                            int, int, hipStream_t);
