// The output spectrum FL2ND of OUTBLOCK (outblock.F90:159-194) built per sea point in LDS, and the parameters that read it:
//   1. IREFRA = 2 / 3: INTPOL with IRA = 1 (intpol.F90:98-271), the Doppler transform of FL1 from the frame moving with the current to the
//      absolute frame -- the f**-5 tail beyond FR(NFRE) folded back in, energy of negative shifted frequency moved to the opposite direction;
//      IREFRA = 0 / 1: FL2ND = FL1;
//   2. LICERUN and not LMASKICE: the noise level under sea ice reshaped bin by bin (outblock.F90:175-194);
//   3. FEMEAN, STHQ, DOMINANT_PERIOD (the five columns of k_outbs, csrc/outbs_point.h) and MWP1, MWP2, WDIRSPREAD with LLPEAKF = F (columns
//      0-2 of k_outbs_sepwisw, restated here operation for operation) of FL2ND; optionally FL2ND itself goes to memory.
// LSECONDORDER (CAL_SECOND_ORDER_SPEC) is not served.
#include <algorithm>
#include <cmath>
#include <vector>

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

template <typename T>
static T host_powi(T x, int n) {  // X**N as compilers expand it (binary powering), n >= 1
  T y = (n & 1) ? x : T(1);
  while (n > 1) {
    n >>= 1;
    x = x * x;
    if (n & 1) y = y * x;
  }
  return y;
}

// 0 on success; 1 when NFRE_MAX does not fit.  CURRENT_MAX = 1.5 (yowcurr.F90:18).
template <typename T>
static int build_intpol_tab(const ecwam_hip_params* p, const ecwam_hip_tables* t, IntpolTab<T>* d) {
  const int NFRE = p->nfre;
  const T* FR = (const T*)t->fr;
  const T* FR5 = (const T*)t->fr5;
  const T FRATIO = (T)p->fratio, ZPI = (T)p->zpi, G = (T)p->g, DELTH = (T)p->delth, FLOGSPRDM1 = (T)p->flogsprdm1;
  const T CURRENT_MAX = T(1.5);
  volatile T fmax = FR[NFRE - 1] + (ZPI / G) * (FR[NFRE - 1] * FR[NFRE - 1]) * CURRENT_MAX;
  volatile T q = fmax / FR[0];
  volatile T lg = std::log10((T)q) * FLOGSPRDM1;
  const int nmax = (int)std::floor((T)lg) + 1;
  if (nmax < NFRE || nmax > INTPOL_MAXM) return 1;
  d->NFRE_MAX = nmax;
  d->COEF = T(1) / ZPI;
  d->FRE0 = FRATIO - T(1);
  d->FR1OFRATIO = FR[0] / FRATIO;
  d->FRATIOFRN = FRATIO * FR[NFRE - 1];
  const T CDF = T(0.5) * (FRATIO - T(1) / FRATIO) * DELTH;
  const T ZPI2GM = (ZPI * ZPI) / G;
  for (int m = 0; m < INTPOL_MAXM; m++) d->FREQ[m] = d->DFQ[m] = d->WAVD[m] = d->R5[m] = T(0);
  for (int m = 0; m < nmax; m++) {
    volatile T f = m < NFRE ? FR[m] : FR[NFRE - 1] * host_powi<T>(FRATIO, m + 1 - NFRE);
    volatile T dq = (T)f * CDF;
    volatile T w = ZPI2GM * ((T)f * (T)f);
    volatile T r = FR5[NFRE - 1] / host_powi<T>((T)f, 5);
    d->FREQ[m] = f; d->DFQ[m] = dq; d->WAVD[m] = w; d->R5[m] = r;
  }
  return 0;
}

// bytes of the table in `host` (resized); 0 when NFRE_MAX does not fit
size_t intpol_tab_build(const ecwam_hip_params* p, const ecwam_hip_tables* t, int real_bytes, std::vector<unsigned char>& host) {
  if (real_bytes == 4) {
    host.assign(sizeof(IntpolTab<float>), 0);
    if (build_intpol_tab<float>(p, t, reinterpret_cast<IntpolTab<float>*>(host.data()))) return 0;
  } else {
    host.assign(sizeof(IntpolTab<double>), 0);
    if (build_intpol_tab<double>(p, t, reinterpret_cast<IntpolTab<double>*>(host.data()))) return 0;
  }
  return host.size();
}

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

// One wavefront per point, wpb points per workgroup.  mode bit 0: INTPOL, bit 1: ice reshaping, bit 2: fl2nd rows take 16-byte stores.
// INTPOL's scatter without atomics: lane K evaluates source direction K at every M (new frequency, bin, the two weights); a source whose
// shifted frequency is positive stays in direction K, the others land in MOD(K+NANG/2-1,NANG)+1.  Lane KH therefore adds its own source
// and pulls (ds_bpermute) the one of lane KH - NANG/2 when that one flipped -- in ascending K, M outer, which is the reference's order of
// additions into FLA(KH,:).  Only lane KH writes column KH of the tile.  Contraction is off: products and sums round where the
// reference's do (the consumers in outbs_point keep the contraction of k_outbs, whose bits they reproduce).
template <typename T>
__global__ void __launch_bounds__(256) k_outbs_absolute(const DevTab<T>* __restrict__ tp, const IntpolTab<T>* __restrict__ ip, int kijs, int kijl,
                                                        int wpb, int mode, const T* __restrict__ fl1, const T* __restrict__ wvprpt,
                                                        const T* __restrict__ ucur, const T* __restrict__ vcur, const T* __restrict__ ff, T zmiss,
                                                        T* __restrict__ out, T* __restrict__ fl2nd) {
  extern __shared__ __align__(16) unsigned char abs_smem[];
  const DevTab<T>& tb = *tp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ij = kijs + blockIdx.x * wpb + wave;
  if (ij >= kijl) return;  // wave-uniform, no block barrier below
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE;
  const bool intpol = mode & 1;
  const AbsLds L(NANG, NFRE, sizeof(T), intpol);
  unsigned char* base = abs_smem + (size_t)wave * L.bytes;
  T* sF = reinterpret_cast<T*>(base);
  T* sS = reinterpret_cast<T*>(base + L.src);
  T* sFr = reinterpret_cast<T*>(base + L.fr);
  T* sDf = reinterpret_cast<T*>(base + L.dfth);
  T* sZr = reinterpret_cast<T*>(base + L.zr);
  auto wsync = [] {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  const bool actm = lane < NFRE, actk = lane < NANG;
  const T EPS = tb.EPSMIN;
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
    if (mode & 2) {  // outblock.F90:175-194
      const T cicover = ff[(size_t)ij * ECWAM_HIP_NFF + 2], wswave = ff[(size_t)ij * ECWAM_HIP_NFF + 3];
      const T zthrs = (T(1) - T(0.9) * m_min(cicover, T(0.99))) * tb.FLMIN;
      if (actm) sZr[lane] = m_exp(T(-10) * (tb.FR[lane] * tb.FR[lane]) / m_sqrt(m_max(wswave, T(1))));
      wsync();
      if (actk)
        for (int m = 0; m < NFRE; m++) {
          const T f = sF[m * NAP + lane], zr = sZr[m];
          if (f <= zthrs) sF[m * NAP + lane] = m_max(zr * f, zthrs * (zr * zr));
        }
      wsync();
    }
    if (fl2nd) {
      if (mode & 4) {
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
  }
  T* o = out + (size_t)ij * 8;
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

// The spectral sizes of launch_outbs_sepwisw; as many waves per workgroup (up to 4) as fit in 64 KiB.
template <typename T>
int launch_outbs_absolute(const void* tab, const void* itab, int kijs, int kijl, int mode, const void* fl1, const void* wvprpt, const void* ucur,
                          const void* vcur, const void* ff, double zmiss, void* out, void* fl2nd, int NANG, int NFRE, hipStream_t s) {
  const int n = kijl - kijs;
  if (n <= 0) return 0;
  if ((size_t)4 * NFRE * (NANG | 1) * sizeof(T) > 64 * 1024 || NANG > 64 || NFRE > 63) return 1;
  const AbsLds L(NANG, NFRE, sizeof(T), mode & 1);
  if (L.bytes > 64 * 1024) return 1;
  const int wpb = (int)std::min<size_t>(4, (size_t)64 * 1024 / L.bytes);
  mode &= 3;
  if (fl2nd && NFRE % Vec16<T>::N == 0 && ((size_t)fl2nd & 15) == 0) mode |= 4;  // every row then starts on 16 bytes
  hipLaunchKernelGGL(k_outbs_absolute<T>, dim3((n + wpb - 1) / wpb), dim3(64 * wpb), wpb * L.bytes, s, (const DevTab<T>*)tab,
                     (const IntpolTab<T>*)itab, kijs, kijl, wpb, mode, (const T*)fl1, (const T*)wvprpt, (const T*)ucur, (const T*)vcur, (const T*)ff,
                     (T)zmiss, (T*)out, (T*)fl2nd);
  return 0;
}
template int launch_outbs_absolute<float>(const void*, const void*, int, int, int, const void*, const void*, const void*, const void*, const void*,
                                          double, void*, void*, int, int, hipStream_t);
template int launch_outbs_absolute<double>(const void*, const void*, int, int, int, const void*, const void*, const void*, const void*, const void*,
                                           double, void*, void*, int, int, hipStream_t);
