// Start spectra on the device: what the reference runs where a model does not begin from a restart file.
//   ST_MSTART    MSTART for IOPTI 0, 1, 2 (mstart.F90:104-136): PEAK's fetch law (peak.F90:88-102) and SPECTRA (spectra.F90:95-120) = JONSWAP
//                (jonswap.F90:70-91) times SPR's cos**2 spread (spr.F90:69-81)
//   ST_UNSETICE  UNSETICE (unsetice.F90:79-171): a fetch-law JONSWAP spectrum where a point holds nothing above the noise level and is no
//                longer ice, the ice noise floor everywhere, then SDEPTHLIM (sdepthlim.F90:64-78 with semean.F90:82-120) when LBIWBK
//   ST_TAIL      the end of a GRIB read (getspec.F90:648-659): the frequencies above NFRE_RED from the last one read, then SDEPTHLIM
//   k_getspec_noise   FL1 = EPSMIN (getspec.F90:174-188, LNSESTART)
// All of them are bound by memory.  A wavefront owns whole sea points: lane l holds the 16-byte chunks l, l + 64, ... of the point's
// [NANG][NFRE] reals in registers between ONE load and ONE store (MSTART only stores).  The NFRE values of ET come from the lanes that own a
// frequency, the NANG values of the spread from the lanes that own a direction, once per point, and reach the chunks through LDS.  UNSETICE's
// OR over every bin is a ballot.  SEMEAN is summed in the reference's own order -- the directions of a frequency in sequence on the lane
// of that frequency, from a copy of the rewritten spectrum in LDS, then the frequencies in sequence -- so that SDEPTHLIM's scale has the
// reference's bits wherever the spectrum has.  The arithmetic of a bin keeps the reference's order, without contraction.
#include "dev.h"
#include "launch.h"

enum { ST_MSTART = 0, ST_UNSETICE = 1, ST_TAIL = 2 };

template <typename T>
struct StartPar {
  int iopti, cimask, lim, nfre_red;      // cimask: LICERUN .AND. LMASKICE; lim: SDEPTHLIM runs
  T fetch, frmax, thetaq, fm, alfa, zgamma, sa, sb, delphi;
};

// PEAK (peak.F90:88-102) = unsetice.F90:133-143: the same lines.  A calm point gets FP = 0 and keeps the ALPHAJ it came with.
template <typename T>
__device__ __forceinline__ void start_peak(T G, T fetch, T fpmax, T u10, T& fp, T& alphaj) {
#pragma clang fp contract(off)
  const T AJONS = T(2.84), BJONS = T(0.033), DJONS = T(-3.0) / T(10.0), EJONS = T(2.0) / T(3.0);      // yowjons.F90:18-21
  if (u10 > T(0.1e-08)) {
    const T gx = G * fetch;
    const T gxu = gx / (u10 * u10);
    const T ug = G / u10;
    T f = AJONS * m_pow(gxu, DJONS);
    f = m_max(T(0.13), f);
    f = m_min(f, fpmax / ug);
    T al = BJONS * m_pow(f, EJONS);
    alphaj = m_max(al, T(0.0081));
    fp = f * ug;
  } else {
    fp = T(0);
  }
}

// JONSWAP (jonswap.F90:70-91) at one frequency: g2 = 1 / (FR**5 ZPI4GM2)
template <typename T>
__device__ __forceinline__ T start_jonswap(T frh, T g2, T alphaj, T zgamma, T sa, T sb, T fp) {
#pragma clang fp contract(off)
  if (!(alphaj != T(0) && fp != T(0))) return T(0);
  const T sigma = frh > fp ? sb : sa;
  const T x = (frh - fp) / (sigma * fp);
  T earg = T(0.5) * (x * x);
  earg = m_min(earg, T(50));
  const T fjon = m_pow(zgamma, m_exp(-earg));
  const T r = fp / frh, r2 = r * r;
  T fmpf = T(1.25) * (r2 * r2);
  fmpf = m_min(fmpf, T(50));
  const T fjonh = m_exp(-fmpf);
  return alphaj * g2 * fjonh * fjon;
}

// writes of this wavefront to its LDS rows before, reads of them after (a wavefront's LDS operations complete in order)
__device__ __forceinline__ void start_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// waves per SIMD the register budget is set for: the double precision POW alone takes about 100 VGPRs
constexpr int start_waves(size_t real_bytes, int nch) { return real_bytes == 8 && nch > 4 ? 2 : 4; }

// NCH: the 16-byte chunks a lane holds, >= ceil(NANG NFRE / VEC / 64).  Chunk c of a point is its reals c VEC .. c VEC + VEC - 1:
// direction c / NC, frequencies (c % NC) VEC ..., NC = NFRE / VEC.  Several waves per SIMD (start_waves): while one wave works on the bins of
// its point, the loads and stores of the others are in flight.
template <typename T, int OP, int NCH>
__global__ void __launch_bounds__(256, start_waves(sizeof(T), NCH)) k_start(const DevTab<T>* __restrict__ tp, int kijs, int kijl, T* __restrict__ fl1, const T* __restrict__ ffa,
                                               const StartPar<T> a) {
#pragma clang fp contract(off)
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  extern __shared__ __align__(16) unsigned char start_smem[];
  const DevTab<T>& tb = *tp;
  const int NANG = tb.NANG, NFRE = tb.NFRE, N = NANG * NFRE, NC = NFRE / VEC, per = NANG * NC;
  const int wpb = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool LIM = OP == ST_TAIL || (OP == ST_UNSETICE && a.lim);
  const int wstride = 3 * 64 + (LIM ? N : 0);
  T* sET = reinterpret_cast<T*>(start_smem) + (size_t)wave * wstride;      // [64] ET of the point
  T* sSP = sET + 64;                                                       // [64] the spread per direction
  T* sC2 = sSP + 64;                                                       // [64] UNSETICE's COS2NOISE
  T* sF = sC2 + 64;                                                        // [NANG][NFRE] the rewritten spectrum, for SEMEAN
  const int dk = 64 / NC, dc = 64 - dk * NC;      // from chunk c to chunk c + 64: directions and chunks of a direction
  const int ml = lane < NFRE ? lane : NFRE - 1, kl = lane < NANG ? lane : NANG - 1;
  const T frh = tb.FR[ml], g2 = T(1) / (tb.FR5[ml] * tb.ZPI4GM2), dfim = tb.DFIM[ml], th = tb.TH[kl];
  const T zdp = T(2) / tb.PI;
  const T delt25 = tb.WETAIL * tb.FR[NFRE - 1] * tb.DELTH;
  const T EPSMIN = tb.EPSMIN;
  if constexpr (OP == ST_TAIL) {      // FRM5 = 1 / FR5 is not on the device: formed as initmdl.F90:466 does, once per wavefront
    sET[lane] = T(1) / tb.FR5[ml];
    start_wave_sync();
  }
  for (int ijv = kijs + (int)blockIdx.x * wpb + wave; ijv < kijl; ijv += (int)gridDim.x * wpb) {
    const int ij = __builtin_amdgcn_readfirstlane(ijv);
    T* __restrict__ row = fl1 + (size_t)ij * N;
    const T* __restrict__ ff = ffa + (size_t)ij * ECWAM_HIP_NFF;
    // The lane number as a value the compiler cannot see through: what depends on it -- the addresses, the direction and the frequencies of every
    // chunk -- is formed again at each point (a division and a few additions), not kept in registers across the loop beside the spectrum.
    int ln = lane;
    asm volatile("" : "+v"(ln));
    // ---- the point's scalars, ET on the lanes of the frequencies, the spread on the lanes of the directions: before the spectrum is loaded,
    //      so that the registers POW and EXP need are not needed beside it
    T flcoef = T(0), EMAXDPT = T(0);
    if constexpr (OP == ST_MSTART) {
      const T WDWAVE = ff[1], WSWAVE = ff[3];
      T fp, alphaj, thes;
      if (a.iopti == 1) {
        fp = T(0); alphaj = T(0); thes = WDWAVE;
      } else if (a.iopti == 0) {
        fp = a.fm; alphaj = a.alfa; thes = a.thetaq;
      } else {
        fp = a.fm; alphaj = a.alfa; thes = WSWAVE > T(0.1e-08) ? WDWAVE : T(0);
      }
      if (a.iopti != 0) start_peak(tb.G, a.fetch, a.frmax, WSWAVE, fp, alphaj);
      sET[lane] = start_jonswap(frh, g2, alphaj, a.zgamma, a.sa, a.sb, fp);
      const T the = m_cos(th - thes);      // SPR: the cut below 0.1E-08 is its own
      T st = T(0);
      if (the > T(0)) {
        st = zdp * (the * the);
        if (st < T(0.1e-08)) st = T(0);
      }
      sSP[lane] = st;
    } else if constexpr (OP == ST_UNSETICE) {
      const T WDWAVE = ff[1], CICOVER = ff[2], WSWAVE = ff[3], DEPTH = ff[15];
      EMAXDPT = ff[14];
      const T CILIMIT = a.cimask ? tb.CITHRSH : T(0);
      const T FPMAX = tb.FR[NFRE - 2];
      // ET as it is if the point turns out to hold nothing above the noise level (LICE2SEA, known once the spectrum is here); otherwise
      // ALPHAV = 0 and ET = 0 whatever FPK is
      T fpk = FPMAX, alphav = T(0);
      if (CICOVER <= CILIMIT) {
        T FETCH;
        if (DEPTH <= T(10)) FETCH = m_min(T(0.5) * a.delphi, T(10000));
        else if (DEPTH <= T(50)) FETCH = m_min(a.delphi, T(50000));
        else if (DEPTH <= T(150)) FETCH = m_min(T(2) * a.delphi, T(100000));
        else if (DEPTH <= T(250)) FETCH = m_min(T(3) * a.delphi, T(200000));
        else FETCH = m_min(T(5) * a.delphi, T(250000));
        start_peak(tb.G, FETCH, FPMAX, WSWAVE, fpk, alphav);
      }
      sET[lane] = start_jonswap(frh, g2, alphav, T(3.0), T(7.0e-02), T(9.0e-02), fpk);
      const T cd = m_max(T(0), m_cos(th - WDWAVE));
      const T c2 = cd * cd;
      sC2[lane] = c2;
      sSP[lane] = zdp * c2;
      flcoef = (T(1) - T(0.9) * m_min(CICOVER, T(0.99))) * tb.FLMIN;      // still noise under full ice cover, ten percent of it
    } else {
      EMAXDPT = ff[14];
    }
    if constexpr (OP != ST_TAIL) start_wave_sync();
    __builtin_amdgcn_sched_barrier(0);
    // ---- the spectrum: one load
    VT f[NCH];
    bool LICE2SEA = true;
    if constexpr (OP != ST_MSTART) {
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int c = ln + 64 * j;
#pragma unroll
        for (int v = 0; v < VEC; v++) f[j][v] = T(0);
        if (c < per) f[j] = *reinterpret_cast<const VT*>(row + (size_t)c * VEC);
      }
      if constexpr (OP == ST_UNSETICE) {
        bool above = false;
#pragma unroll
        for (int j = 0; j < NCH; j++) {
#pragma unroll
          for (int v = 0; v < VEC; v++) above = above || (f[j][v] > EPSMIN);      // (the chunks past the point hold zeros)
        }
        LICE2SEA = __ballot(above) == 0ull;
      }
    }
    if constexpr (OP == ST_TAIL) {      // the copy for SEMEAN goes to LDS now: the fill takes the last frequency read from it, not from memory again
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int c = ln + 64 * j;
        if (c < per) *reinterpret_cast<VT*>(sF + (size_t)c * VEC) = f[j];
      }
      start_wave_sync();
    }
    // ---- the bins
    {
      const int k0 = ln / NC;
      int k = k0, cc = ln - k0 * NC;
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        if (ln + 64 * j < per) {
          const int m0 = cc * VEC;
          if constexpr (OP == ST_TAIL) {
            if (m0 + VEC > a.nfre_red) {
              const T last = sF[k * NFRE + a.nfre_red - 1], fr5r = tb.FR5[a.nfre_red - 1];      // (a bin below NFRE_RED: no fill writes it)
              const VT frm5 = *reinterpret_cast<const VT*>(sET + m0);
#pragma unroll
              for (int v = 0; v < VEC; v++)
                if (m0 + v >= a.nfre_red) f[j][v] = last * fr5r * frm5[v];
              *reinterpret_cast<VT*>(sF + (size_t)(ln + 64 * j) * VEC) = f[j];
            }
          } else {
            const VT et = *reinterpret_cast<const VT*>(sET + m0);
            const T sp = sSP[k];
            if constexpr (OP == ST_MSTART) {
#pragma unroll
              for (int v = 0; v < VEC; v++) f[j][v] = et[v] * sp;
            } else {
              const T fllowest = flcoef * sC2[k];
#pragma unroll
              for (int v = 0; v < VEC; v++) f[j][v] = m_max(m_max(f[j][v], (LICE2SEA ? et[v] : T(0)) * sp), fllowest);
            }
          }
        }
        k += dk; cc += dc;
        if (cc >= NC) { cc -= NC; k++; }
      }
    }
    // ---- SDEPTHLIM
    if (LIM) {
      if constexpr (OP != ST_TAIL) {
#pragma unroll
        for (int j = 0; j < NCH; j++) {
          const int c = ln + 64 * j;
          if (c < per) *reinterpret_cast<VT*>(sF + (size_t)c * VEC) = f[j];
        }
      }
      start_wave_sync();
      T temp = sF[ml];
      for (int k = 1; k < NANG; k++) temp = temp + sF[k * NFRE + ml];
      const T p = dfim * temp;
      T em = EPSMIN;
      for (int m = 0; m < NFRE; m++) em = em + lane_get(p, m);
      em = em + delt25 * lane_get(temp, NFRE - 1);
      const T sc = m_min(EMAXDPT / em, T(1));
#pragma unroll
      for (int j = 0; j < NCH; j++) {
#pragma unroll
        for (int v = 0; v < VEC; v++) f[j][v] = m_max(f[j][v] * sc, EPSMIN);
      }
    }
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int c = ln + 64 * j;
      if (c < per) *reinterpret_cast<VT*>(row + (size_t)c * VEC) = f[j];
    }
    start_wave_sync();      // the next point's ET and spectrum copy go to the same LDS rows
  }
}

// FL1 = EPSMIN on rows [kijs, kijl): one contiguous range, 16 bytes per thread
template <typename T>
__global__ void __launch_bounds__(256) k_getspec_noise(const DevTab<T>* __restrict__ tp, T* __restrict__ p, size_t nchunk) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= nchunk) return;
  const T e = tp->EPSMIN;
  VT o;
#pragma unroll
  for (int i = 0; i < VEC; i++) o[i] = e;
  reinterpret_cast<VT*>(p)[w] = o;
}

// 0 = launched (or nothing to do), -1 = a direction's frequencies are no whole number of 16-byte chunks, 1 = unsupported spectral size
template <typename T, int OP>
static int start_launch(const void* tab, int kijs, int kijl, void* fl1, const void* ff, const StartPar<T>& a, int NANG, int NFRE, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  if (NANG > 64 || NFRE > 64 || NANG < 1 || NFRE < 2) return 1;
  const int n = kijl - kijs;
  const bool lim = OP == ST_TAIL || (OP == ST_UNSETICE && a.lim);
  const size_t wbytes = (size_t)(3 * 64 + (lim ? NANG * NFRE : 0)) * sizeof(T);
  int wpb = 4;
  while (wpb > 1 && wbytes * wpb > 64 * 1024) wpb >>= 1;
  if (wbytes * wpb > 64 * 1024) return 1;
  // At most 48 x 36 reals a point, in whole rows of 64 chunks: 7 chunks a lane in single, 14 in double precision.  Every instantiation below
  // is one that a spectral size of the model (12, 24, 36, 48 directions of 36 frequencies) takes.
  const int need = (NANG * (NFRE / VEC) + 63) / 64;
  if (need * VEC > 28) return 1;
  if (n <= 0) return 0;
  const long long want = ((long long)n + wpb - 1) / wpb;
  const dim3 grid((unsigned)(want < 4096 ? want : 4096)), block(64 * wpb);
#define START_GO(NCH_)                                                                                                                          \
  hipLaunchKernelGGL((k_start<T, OP, NCH_>), grid, block, wbytes * wpb, s, (const DevTab<T>*)tab, kijs, kijl, (T*)fl1, (const T*)ff, a)
  if constexpr (VEC == 4) {
    if (need <= 2) START_GO(2);
    else if (need <= 4) START_GO(4);
    else START_GO(7);
  } else {
    if (need <= 4) START_GO(4);
    else if (need <= 7) START_GO(7);
    else if (need <= 11) START_GO(11);
    else START_GO(14);
  }
#undef START_GO
  return 0;
}

template <typename T>
int launch_mstart(const void* tab, int kijs, int kijl, void* fl1, const void* ff, int iopti, const double* par, int NANG, int NFRE, hipStream_t s) {
  StartPar<T> a = {};
  a.iopti = iopti;
  a.fetch = T(par[0]); a.frmax = T(par[1]); a.thetaq = T(par[2]); a.fm = T(par[3]);
  a.alfa = T(par[4]); a.zgamma = T(par[5]); a.sa = T(par[6]); a.sb = T(par[7]);
  return start_launch<T, ST_MSTART>(tab, kijs, kijl, fl1, ff, a, NANG, NFRE, s);
}
template <typename T>
int launch_unsetice(const void* tab, int kijs, int kijl, void* fl1, const void* ff, double delphi, int cimask, int lim, int NANG, int NFRE, hipStream_t s) {
  StartPar<T> a = {};
  a.cimask = cimask; a.lim = lim; a.delphi = T(delphi);
  return start_launch<T, ST_UNSETICE>(tab, kijs, kijl, fl1, ff, a, NANG, NFRE, s);
}
template <typename T>
int launch_getspec_tail(const void* tab, int kijs, int kijl, void* fl1, const void* ff, int nfre_red, int NANG, int NFRE, hipStream_t s) {
  StartPar<T> a = {};
  a.lim = 1; a.nfre_red = nfre_red;
  return start_launch<T, ST_TAIL>(tab, kijs, kijl, fl1, ff, a, NANG, NFRE, s);
}
template <typename T>
int launch_getspec_noise(const void* tab, int kijs, int kijl, void* fl1, int NANG, int NFRE, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  if (kijl - kijs <= 0) return 0;
  const size_t N = (size_t)NANG * NFRE, nchunk = (size_t)(kijl - kijs) * N / VEC;
  hipLaunchKernelGGL((k_getspec_noise<T>), dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, s, (const DevTab<T>*)tab, (T*)fl1 + (size_t)kijs * N, nchunk);
  return 0;
}
template int launch_mstart<float>(const void*, int, int, void*, const void*, int, const double*, int, int, hipStream_t);
template int launch_mstart<double>(const void*, int, int, void*, const void*, int, const double*, int, int, hipStream_t);
template int launch_unsetice<float>(const void*, int, int, void*, const void*, double, int, int, int, int, hipStream_t);
template int launch_unsetice<double>(const void*, int, int, void*, const void*, double, int, int, int, int, hipStream_t);
template int launch_getspec_tail<float>(const void*, int, int, void*, const void*, int, int, int, hipStream_t);
template int launch_getspec_tail<double>(const void*, int, int, void*, const void*, int, int, int, hipStream_t);
template int launch_getspec_noise<float>(const void*, int, int, void*, int, int, hipStream_t);
template int launch_getspec_noise<double>(const void*, int, int, void*, int, int, hipStream_t);
