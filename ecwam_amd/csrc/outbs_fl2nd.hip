// The output spectrum FL2ND of OUTBLOCK (outblock.F90:159-194) built per sea point in LDS, and the parameters that read it:
//   1. IREFRA = 2 / 3: INTPOL with IRA = 1 (intpol.F90:98-271), the Doppler transform of FL1 from the frame moving with the current to the
//      absolute frame -- the f**-5 tail beyond FR(NFRE) folded back in, energy of negative shifted frequency moved to the opposite direction;
//      IREFRA = 0 / 1: FL2ND = FL1;
//   2. LICERUN and not LMASKICE: the noise level under sea ice reshaped bin by bin (outblock.F90:175-194);
//   3. FEMEAN, STHQ, DOMINANT_PERIOD (the five columns of k_outbs, csrc/outbs_point.h) and MWP1, MWP2, WDIRSPREAD with LLPEAKF = F (columns
//      0-2 of k_outbs_sepwisw, restated here operation for operation) of FL2ND; optionally FL2ND itself goes to memory.
// CAL_SECOND_ORDER_SPEC (LSECONDORDER) is served by ecwam_hip_outbs_second_order (csrc/outbs_2nd.hip), which runs the stages of
// csrc/outbs_fl2nd.h with the correction between them.
#include <algorithm>
#include <cmath>
#include <vector>

#include "outbs_fl2nd.h"
#include "launch.h"

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
// One wavefront per point, wpb points per workgroup.  mode bit 0: INTPOL, bit 1: ice reshaping, bit 2: fl2nd rows take 16-byte stores.
// The stages are those of csrc/outbs_fl2nd.h.
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
  const AbsTile<T> t(abs_smem + (size_t)wave * L.bytes, L);
  fl2nd_load_intpol(tb, ip, t, ij, lane, intpol, fl1, wvprpt, ucur, vcur);
  if (mode & 2) fl2nd_ice(tb, t, ij, lane, ff);
  if (fl2nd) fl2nd_store(tb, t, ij, lane, (mode & 4) != 0, fl2nd);
  fl2nd_params(tb, t, lane, zmiss, out + (size_t)ij * 8);
}

// The spectral sizes of launch_outbs_sepwisw; as many waves per workgroup (up to 4) as fit in 64 KiB.
template <typename T>
int launch_outbs_absolute(const void* tab, const void* itab, int kijs, int kijl, int mode, const void* fl1, const void* wvprpt, const void* ucur,
                          const void* vcur, const void* ff, double zmiss, void* out, void* fl2nd, int NANG, int NFRE, hipStream_t s) {
  const int n = kijl - kijs;
  if (n <= 0) return 0;
  if (!outbs_size_ok(NANG, NFRE, sizeof(T))) return 1;
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
