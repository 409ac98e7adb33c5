// The stages of the output spectrum FL2ND of OUTBLOCK (outblock.F90:159-194) on a spectrum tile in LDS, one wavefront per sea point: shared
// by k_outbs_absolute (csrc/outbs_fl2nd.hip) and the second-order pipeline (csrc/outbs_2nd.hip), so that both give the same bits:
//   fl2nd_load_intpol  the tile load and, with IREFRA = 2 / 3, INTPOL with IRA = 1 (intpol.F90:98-271)
//   fl2nd_ice          the noise level under sea ice reshaped bin by bin (outblock.F90:175-194)
//   fl2nd_store        FL2ND to memory
//   fl2nd_params       the eight output columns: outbs_point, then MWP1, MWP2 and WDIRSPREAD of the total spectrum
#pragma once
#include "outbs_point.h"

#define INTPOL_MAXM 64  // one lane per source frequency; NFRE_MAX = 64 at NFRE = MAXF = 48 with the reference's FR(1), FRATIO

// The loop of INTPOL over the source frequencies M = 1 .. NFRE_MAX (intpol.F90:98-115, 153-169) as tables, built once on the host in the
// working precision: FREQ, DFREQTH = FREQ*CDF (= DFTH(M) for M <= NFRE) and, beyond NFRE, the deep-water WAVN and FR5(NFRE)/FREQ**5.
template <typename T>
struct IntpolTab {
  int NFRE_MAX;
  T COEF, FRE0, FR1OFRATIO, FRATIOFRN;  // IRA/ZPI, FRATIO-1, FR(1)/FRATIO, FRATIO*FR(NFRE)
  T FREQ[INTPOL_MAXM], DFQ[INTPOL_MAXM], WAVD[INTPOL_MAXM], R5[INTPOL_MAXM];
};

// Per-wave LDS: the FL2ND tile [M][NANG|1]; with INTPOL the FL1 tile of the same shape, FR and DFTH [NFRE] (read at the bin a source
// lands in); with the ice reshaping ZRDUC [NFRE].
struct AbsLds {
  size_t src, fr, dfth, zr, bytes;
  __host__ __device__ AbsLds(int NANG, int NFRE, size_t tsz, bool intpol) {
    const size_t tile = ((size_t)NFRE * (NANG | 1) * tsz + 15) & ~(size_t)15;
    src = tile;
    fr = src + (intpol ? tile : 0);
    dfth = fr + (size_t)NFRE * tsz;
    zr = dfth + (size_t)NFRE * tsz;
    bytes = (zr + (size_t)NFRE * tsz + 15) & ~(size_t)15;
  }
};

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef float4 type; static constexpr int N = 4; };
template <> struct Vec16<double> { typedef double2 type; static constexpr int N = 2; };


__device__ __forceinline__ void fl2nd_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The pointers of one wave's slice of LDS (AbsLds): the FL2ND tile [M][NANG|1], the INTPOL source tile, FR, DFTH, ZRDUC.
template <typename T>
struct AbsTile {
  T *sF, *sS, *sFr, *sDf, *sZr;
  __device__ AbsTile(unsigned char* base, const AbsLds& L)
      : sF(reinterpret_cast<T*>(base)), sS(reinterpret_cast<T*>(base + L.src)), sFr(reinterpret_cast<T*>(base + L.fr)),
        sDf(reinterpret_cast<T*>(base + L.dfth)), sZr(reinterpret_cast<T*>(base + L.zr)) {}
};

// INTPOL's scatter without atomics: lane K evaluates source direction K at every M (new frequency, bin, the two weights); a source whose
// shifted frequency is positive stays in direction K, the others land in MOD(K+NANG/2-1,NANG)+1.  Lane KH therefore adds its own source
// and pulls (ds_bpermute) the one of lane KH - NANG/2 when that one flipped -- in ascending K, M outer, which is the reference's order of
// additions into FLA(KH,:).  Only lane KH writes column KH of the tile.  Contraction is off: products and sums round where the
// reference's do (the consumers in outbs_point keep the contraction of k_outbs, whose bits they reproduce).
// On return the tile t.sF holds FL1 (intpol = false) or FLA, visible to the whole wave.
template <typename T>
__device__ __forceinline__ void fl2nd_load_intpol(const DevTab<T>& tb, const IntpolTab<T>* __restrict__ ip, const AbsTile<T>& t, int ij, int lane,
                                                  bool intpol, const T* __restrict__ fl1, const T* __restrict__ wvprpt,
                                                  const T* __restrict__ ucur, const T* __restrict__ vcur) {
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE;
  const bool actm = lane < NFRE, actk = lane < NANG;
  const T EPS = tb.EPSMIN;
  T *sF = t.sF, *sS = t.sS, *sFr = t.sFr, *sDf = t.sDf;
  auto wsync = [] { fl2nd_wsync(); };
  const size_t row = (size_t)ij * N;
  {
#pragma clang fp contract(off)
    // tile load: FL1 is the INTPOL source, or FL2ND itself
    T* dst = intpol ? sS : sF;
    bool above = false;
    for (int e = lane; e < N; e += 64) {
      const int kk = e / NFRE, mm = e - kk * NFRE;
      const T f = fl1[row + e];
      above = above || f > EPS;
      dst[mm * NAP + kk] = f;
    }
    if (intpol) {
      const IntpolTab<T>& it = *ip;
      const bool lice2sea = __ballot(above) == 0ull;  // no bin above EPSMIN: OLDFL = 0 everywhere (intpol.F90:129-139)
      // lane M holds the constants of source frequency M (NFRE_MAX <= 64): the loop below reads them with v_readlane, not from memory.
      // Up to NFRE the wave number is the point's and the f**-5 factor is 1 (OLDFL = FLR(K,M) exactly)
      const int nmax = it.NFRE_MAX;
      const int ml = min(lane, nmax - 1);
      const T freq_l = it.FREQ[ml], dfq_l = it.DFQ[ml];
      const T wavn_l = actm ? wvprpt[(size_t)ij * (ECWAM_HIP_NWPR * NFRE) + lane] : it.WAVD[ml];
      const T r5_l = actm ? T(1) : it.R5[ml];
      if (actm) {
        sFr[lane] = freq_l;
        sDf[lane] = dfq_l;
      }
      for (int e = lane; e < NFRE * NAP; e += 64) sF[e] = T(0);
      wsync();
      if (!lice2sea) {
        const int k = actk ? lane : NANG - 1;                 // idle lanes repeat a valid direction and write nothing
        const int k2 = (k + NANG - NANG / 2) % NANG;          // the direction that lands in k when it flips
        const T u = ucur[ij], v = vcur[ij];
        const T proj = tb.COSTH[k] * v + tb.SINTH[k] * u;
        const T* col = sS + k;
        T* acc = sF + k;
        const T FRE0 = it.FRE0, FR1 = sFr[0], FRN = sFr[NFRE - 1], DF1 = sDf[0], DFN = sDf[NFRE - 1];
        const T COEF = it.COEF, FR1OFRATIO = it.FR1OFRATIO, FRATIOFRN = it.FRATIOFRN, FRATIO = tb.FRATIO, FLOGSPRDM1 = tb.FLOGSPRDM1;
        for (int m = 0; m < nmax; m++) {
          const T freq = lane_get(freq_l, m), dfq = lane_get(dfq_l, m), wavn = lane_get(wavn_l, m);
          const T old = col[min(m, NFRE - 1) * NAP] * lane_get(r5_l, m);
          T fnef = freq + COEF * wavn * proj;
          const bool flip = !(fnef > T(0));
          if (flip) fnef = -fnef;
          int newm = -1;  // 1-based NEWF
          if (!(fnef <= FR1OFRATIO)) newm = (int)m_floor(m_log10(fnef / FR1) * FLOGSPRDM1) + 1;
          int im = -1, ipl = -1;  // 0-based bins that receive GWM / GWP
          T gwm = T(0), gwp = T(0);
          if (newm >= 1 && newm < NFRE) {
            const T f0 = sFr[newm - 1], f1 = sFr[newm];
            const T gwh = dfq / (f1 - f0) * old;
            gwm = gwh * (f1 - fnef) / sDf[newm - 1];
            gwp = gwh * (fnef - f0) / sDf[newm];
            im = newm - 1; ipl = newm;
          } else if (newm == 0) {
            const T gwh = FRATIO * dfq / (FRE0 * FR1) * old;
            gwp = gwh * (fnef - FR1OFRATIO) / DF1;
            ipl = 0;
          } else if (newm == NFRE) {
            const T gwh = dfq / (FRE0 * FRN) * old;
            gwm = gwh * (FRATIOFRN - fnef) / DFN;
            im = NFRE - 1;
          }
          const bool anyflip = __ballot(flip && actk) != 0ull;  // wave-uniform; rare (needs K.U/ZPI > FREQ)
          bool pf = false;
          int pim = -1, pip = -1;
          T pgm = T(0), pgp = T(0);
          if (anyflip) {
            pf = __builtin_amdgcn_ds_bpermute(k2 << 2, flip ? 1 : 0) != 0;
            pim = __builtin_amdgcn_ds_bpermute(k2 << 2, im);
            pip = __builtin_amdgcn_ds_bpermute(k2 << 2, ipl);
            pgm = lane_pull(gwm, k2);
            pgp = lane_pull(gwp, k2);
          }
          if (actk) {
            if (pf && k2 < k) {
              if (pim >= 0) acc[pim * NAP] = acc[pim * NAP] + pgm;
              if (pip >= 0) acc[pip * NAP] = acc[pip * NAP] + pgp;
            }
            if (!flip) {
              if (im >= 0) acc[im * NAP] = acc[im * NAP] + gwm;
              if (ipl >= 0) acc[ipl * NAP] = acc[ipl * NAP] + gwp;
            }
            if (pf && k2 > k) {
              if (pim >= 0) acc[pim * NAP] = acc[pim * NAP] + pgm;
              if (pip >= 0) acc[pip * NAP] = acc[pip * NAP] + pgp;
            }
          }
        }
      }
      if (actk)
        for (int m = 0; m < NFRE; m++) sF[m * NAP + lane] = m_max(sF[m * NAP + lane], EPS);
    }
    wsync();
  }
}

// outblock.F90:175-194 on the tile
template <typename T>
__device__ __forceinline__ void fl2nd_ice(const DevTab<T>& tb, const AbsTile<T>& t, int ij, int lane, const T* __restrict__ ff) {
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1;
  const bool actm = lane < NFRE, actk = lane < NANG;
  T *sF = t.sF, *sZr = t.sZr;
  {
#pragma clang fp contract(off)
    const T cicover = ff[(size_t)ij * ECWAM_HIP_NFF + 2], wswave = ff[(size_t)ij * ECWAM_HIP_NFF + 3];
    const T zthrs = (T(1) - T(0.9) * m_min(cicover, T(0.99))) * tb.FLMIN;
    if (actm) sZr[lane] = m_exp(T(-10) * (tb.FR[lane] * tb.FR[lane]) / m_sqrt(m_max(wswave, T(1))));
    fl2nd_wsync();
    if (actk)
      for (int m = 0; m < NFRE; m++) {
        const T f = sF[m * NAP + lane], zr = sZr[m];
        if (f <= zthrs) sF[m * NAP + lane] = m_max(zr * f, zthrs * (zr * zr));
      }
    fl2nd_wsync();
  }
}

// the tile to fl2nd[ij][K][M]; vec: the rows take 16-byte stores (NFRE a multiple of the vector, fl2nd on 16 bytes)
template <typename T>
__device__ __forceinline__ void fl2nd_store(const DevTab<T>& tb, const AbsTile<T>& t, int ij, int lane, bool vec, T* __restrict__ fl2nd) {
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE;
  const T* sF = t.sF;
  const size_t row = (size_t)ij * N;
  if (vec) {
    typedef typename Vec16<T>::type V;
    constexpr int VN = Vec16<T>::N;
    V* g = reinterpret_cast<V*>(fl2nd + row);
    for (int q = lane; q < N / VN; q += 64) {
      const int e = q * VN, kk = e / NFRE, mm = e - kk * NFRE;  // NFRE % VN == 0: the VN bins share the direction
      V w;
      T* wp = reinterpret_cast<T*>(&w);
#pragma unroll
      for (int j = 0; j < VN; j++) wp[j] = sF[(mm + j) * NAP + kk];
      g[q] = w;
    }
  } else {
    for (int e = lane; e < N; e += 64) {
      const int kk = e / NFRE, mm = e - kk * NFRE;
      fl2nd[row + e] = sF[mm * NAP + kk];
    }
  }
}

// o[0..7]: the five columns of k_outbs, then MWP1, MWP2 and WDIRSPREAD (LLPEAKF = F) of the total spectrum
template <typename T>
__device__ __forceinline__ void fl2nd_params(const DevTab<T>& tb, const AbsTile<T>& t, int lane, T zmiss, T* __restrict__ o) {
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1;
  const bool actm = lane < NFRE;
  const T EPS = tb.EPSMIN;
  const T* sF = t.sF;
  outbs_point(tb, sF, lane, zmiss, o);
  {
#pragma clang fp contract(off)
    // MWP1, MWP2 and WDIRSPREAD (LLPEAKF = F) of the total spectrum as k_outbs_sepwisw computes them (csrc/outbs_sep.hip; mwp1.F90:101-115,
    // mwp2.F90:101-115, wdirspread.F90:95-115, scosfl.F90:71-92): the same operations and the same wave reductions, hence the same bits
    const T DELTH = tb.DELTH;
    T t_fe = T(0), t_w = T(0), t_sc = T(0);
    if (actm) {
      const T* p = sF + lane * NAP;
      T si = T(0), ci = T(0);
      for (int kk = 0; kk < NANG; kk++) {
        const T f = p[kk];
        t_fe = t_fe + m_max(f, EPS); t_w = t_w + f;
        si = si + tb.SINTH[kk] * f;
        ci = ci + tb.COSTH[kk] * f;
      }
      const T md = (ci == T(0) && si == T(0)) ? T(0) : m_atan2(si, ci);
      T mc = T(0);
      for (int kk = 0; kk < NANG; kk++) mc = mc + m_cos(tb.TH[kk] - md) * p[kk];
      t_sc = DELTH * mc;
    }
    const int MO = tb.NFRE_ODD;
    const bool acts = lane < MO;
    const T wsim = acts ? tb.DFIM_SIM[lane] : T(0);
    const T w1 = acts ? tb.DFIM_SIM[lane] * tb.FR[lane] : T(0);
    const T w2 = acts ? tb.DFIM_SIM[lane] * (tb.FR[lane] * tb.FR[lane]) : T(0);
    const T dfim = actm ? tb.DFIM[lane] : T(0);
    T Et, M1t, M2t, EMt, Wt, un1, un2, un3;
    usum4(wsim * t_w, w1 * t_w, w2 * t_w, t_fe * dfim, Et, M1t, M2t, EMt);
    usum4(t_sc * dfim, T(0), T(0), T(0), Wt, un1, un2, un3);
    const T fro = tb.FR[MO - 1], FR1M1 = T(1) / tb.FR[0];
    const T tl = lane_get(t_w, MO - 1);
    T E = Et + tb.WETAIL * fro * DELTH * tl;
    T M1 = M1t + tb.WP1TAIL * DELTH * (fro * fro) * tl;
    T M2 = M2t + T(0.5) * DELTH * (fro * fro * fro) * tl;  // WP2TAIL = 0.5, yowfred.F90:54
    const T P1 = (E > T(0) && M1 > EPS) ? m_min(E / M1, FR1M1) : T(0);
    const T P2 = (E > T(0) && M2 > EPS) ? m_min(m_sqrt(E / M2), FR1M1) : T(0);
    const T EMEAN = EMt + tb.WETAIL * tb.FR[NFRE - 1] * DELTH * lane_get(t_fe, NFRE - 1);
    T wdt = Wt / DELTH + lane_get(t_sc, NFRE - 1) * (tb.WETAIL * tb.FR[NFRE - 1]);
    wdt = EMEAN > EPS ? m_min(wdt / EMEAN, T(1)) : T(1);
    wdt = m_sqrt(T(2) * (T(1) - wdt));
    if (lane == 0) {
      o[5] = P1;
      o[6] = P2;
      o[7] = wdt;
    }
  }
}
