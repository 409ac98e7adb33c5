// The output spectrum FL2ND of OUTBLOCK with LSECONDORDER = T (outblock.F90:168-194): INTPOL, CAL_SECOND_ORDER_SPEC
// (cal_second_order_spec.F90:91-193, the thinning path MR = MA = 2 that SECONDHH_GEN always selects), the ice noise reshaping, and the eight
// columns of ecwam_hip_outbs_absolute.  Three kernels on one stream:
//   k_so_pre   one wavefront per point: the stages of csrc/outbs_fl2nd.h up to INTPOL; FKMEAN (EMEAN, AKMEAN) of the result, the depth index
//              JD (secspom.F90:127-135), the EMAXL switch, and the thinned spectrum extended by its f**-5 tail to NMAX frequencies, written
//              point-minor: PF1[K + NANGH M][point]
//   k_so_sum   SECSPOM's double sum (secspom.F90:179-288), lane = point, workgroup = 64 points x one output frequency M.  The NANGH
//              accumulators of the output directions and the rows F2(:,M1), F2(:,M2_M), F2(:,M2_P) sit in registers; the lanes of one
//              depth index share every coefficient, so the five tables are read through the scalar data path (one load per 64 points)
//              and the vector work is multiply-adds only.  A wavefront that mixes depth indices runs the sum once per distinct index
//              with the other lanes masked.  Every bin adds its terms in the reference's order (M1 outer, K1 inner, the TA term before the
//              XINCR term); there are no atomics, so the result does not depend on scheduling.
//   k_so_post  one wavefront per point: INTPOL again (cheaper than a round trip of the full spectrum through memory), the energy
//              conserving interpolation of PF3 back to NANG x NFRE with the EMAXL switch and the clamp, the ice reshaping, the store and the
//              parameters -- the stages of csrc/outbs_fl2nd.h again.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "outbs_fl2nd.h"
#include "launch.h"

#define SO_MAXNH 24  // NFREH at NFRE = MAXF = 48
#define SO_MAXNX 32  // NMAX (28 at NFRE = 48)

template <typename T>
struct SoTab {
  int NH, AH, NMAX, NDEPTH;
  T DEPTHA, XLOGD, ZFAC, SMALL;
  T OMRT[SO_MAXNX];                                   // OMEGA(NFREH)**5 / OMEGA_EXT(M)**5 beyond NFREH, 0 below
  T DELM1[SO_MAXNH];                                  // 1 / (OMEGA_EXT(MP) - OMEGA(MM))
  int MP[SO_MAXNH], MM[SO_MAXNH];                     // 0-based
  int IMP[SO_MAXNH * SO_MAXNH], IMM[SO_MAXNH * SO_MAXNH];  // [M][M1], 0-based frequency of F2
  int M0[MAXF], MPI[MAXF];                            // the interpolation back to the full grid, per M: thinned rows (0-based) and D1
  T D1[MAXF];
};

template <typename T>
static T so_powi(T x, int n) {  // X**N as compilers expand it (binary powering), n >= 1
  T y = (n & 1) ? x : T(1);
  while (n > 1) {
    n >>= 1;
    x = x * x;
    if (n & 1) y = y * x;
  }
  return y;
}

// 0 on success; otherwise the reason
template <typename T>
static const char* build_so_tab(const ecwam_hip_params* p, const void* fr, int ndepth, double deptha, double depthd, int nmax,
                                const int* im_p, const int* im_m, SoTab<T>* d) {
  const int NANG = p->nang, NFRE = p->nfre;
  if ((NANG & 1) || (NFRE & 1)) return "NANG and NFRE must be even (SECONDHH_GEN thins with MR = MA = 2)";
  const int NH = NFRE / 2, AH = NANG / 2;
  if (NH > SO_MAXNH || nmax > SO_MAXNX || nmax < NH + 1) return "NFREH or NMAX outside the library's tables";
  if (ndepth < 1 || !(deptha > 0) || !(depthd > 1)) return "bad depth table (NDEPTH >= 1, DEPTHA > 0, DEPTHD > 1)";
  const T* FR = (const T*)fr;
  const T ZPI = (T)p->zpi, FRATIO = (T)p->fratio;
  d->NH = NH; d->AH = AH; d->NMAX = nmax; d->NDEPTH = ndepth;
  d->DEPTHA = (T)deptha;
  d->XLOGD = std::log((T)depthd);
  d->ZFAC = T(0.6) * T(0.6) / T(16);
  d->SMALL = T(0.000001);
  volatile T frac = FRATIO - T(1), omstart = ZPI * FR[0];
  T ome[SO_MAXNX];
  for (int m = 0; m < NH; m++) { volatile T o = ZPI * FR[2 * m + 1]; ome[m] = o; d->OMRT[m] = T(0); }
  const T omg5 = so_powi<T>(ome[NH - 1], 5);
  for (int m = NH; m < nmax; m++) {
    volatile T o = (T)omstart * so_powi<T>(T(1) + (T)frac, 2 * (m + 1) - 1);
    volatile T r = omg5 / so_powi<T>((T)o, 5);
    ome[m] = o; d->OMRT[m] = r;
  }
  for (int m = nmax; m < SO_MAXNX; m++) d->OMRT[m] = T(0);
  for (int m = 0; m < NH; m++) {
    const int mp = std::min(m + 1, nmax - 1), mm = std::max(m - 1, 0);
    volatile T dl = ome[mp] - ome[mm];
    d->MP[m] = mp; d->MM[m] = mm; d->DELM1[m] = T(1) / (T)dl;
    for (int m1 = 0; m1 < NH; m1++) {
      const int ip = im_p[m * NH + m1], im = im_m[m * NH + m1];   // IM_P(M1,M) in the reference's storage order
      if (ip < 1 || ip > nmax || im < 1 || im > nmax) return "IM_P / IM_M outside 1 .. NMAX";
      d->IMP[m * SO_MAXNH + m1] = ip - 1; d->IMM[m * SO_MAXNH + m1] = im - 1;
    }
  }
  for (int M = 1; M <= NFRE; M++) {
    int m0 = M / 2, mp;
    T d1;
    if (m0 < 1) { m0 = 1; mp = 2; d1 = T(1); }
    else if (m0 < NH) {
      mp = m0 + 1;
      volatile T a = FR[M - 1] - FR[2 * m0 - 1], b = FR[2 * mp - 1] - FR[2 * m0 - 1];
      d1 = (T)a / (T)b;
    } else { m0 = NH; mp = NH; d1 = T(0); }
    d->M0[M - 1] = m0 - 1; d->MPI[M - 1] = mp - 1; d->D1[M - 1] = d1;
  }
  return nullptr;
}

const char* so_tab_build(const ecwam_hip_params* p, const void* t, int real_bytes, int ndepth, double deptha, double depthd, int nmax,
                         const int* im_p, const int* im_m, std::vector<unsigned char>& host) {
  if (real_bytes == 4) {
    host.assign(sizeof(SoTab<float>), 0);
    return build_so_tab<float>(p, t, ndepth, deptha, depthd, nmax, im_p, im_m, reinterpret_cast<SoTab<float>*>(host.data()));
  }
  host.assign(sizeof(SoTab<double>), 0);
  return build_so_tab<double>(p, t, ndepth, deptha, depthd, nmax, im_p, im_m, reinterpret_cast<SoTab<double>*>(host.data()));
}

// The five coefficient tables from the reference's storage order TA(JD,L,M1,M) (JD fastest) to the device's [JD][M][M1][table][L0], L0 = the
// direction difference (K - K1) MOD NANGH (the reference's L = NANGH is L0 = 0): one depth index is one contiguous slice, and the NANGH
// coefficients of one table and frequency pair are consecutive words for the scalar loads of k_so_sum.
void so_coef_layout(int real_bytes, int ND, int AH, int NH, const void* const src[5], std::vector<unsigned char>& host) {
  const size_t tsz = real_bytes, n = (size_t)ND * NH * NH * 5 * AH;
  host.assign(n * tsz, 0);
  for (int c = 0; c < 5; c++)
    for (int m = 0; m < NH; m++)
      for (int m1 = 0; m1 < NH; m1++)
        for (int l = 0; l < AH; l++)
          for (int jd = 0; jd < ND; jd++) {
            const size_t from = (((size_t)m * NH + m1) * AH + l) * ND + jd;
            const size_t to = ((((size_t)jd * NH + m) * NH + m1) * 5 + c) * AH + (l + 1) % AH;
            memcpy(host.data() + to * tsz, (const unsigned char*)src[c] + from * tsz, tsz);
          }
}

// bytes of the work space of n points: PF1 [NANGH NMAX][npad], PF3 [NANGH NFREH][npad], JD and EMAXL [npad] ints
size_t so_work_bytes(int real_bytes, int n, int AH, int NH, int NMAX) {
  const size_t npad = ((size_t)n + 63) & ~(size_t)63;
  return npad * ((size_t)AH * (NMAX + NH) * real_bytes + sizeof(int));
}

template <typename T>
__global__ void __launch_bounds__(256) k_so_pre(const DevTab<T>* __restrict__ tp, const IntpolTab<T>* __restrict__ ip, const SoTab<T>* __restrict__ sp,
                                                int kijs, int kijl, int wpb, int mode, size_t npad, const T* __restrict__ fl1,
                                                const T* __restrict__ wvprpt, const T* __restrict__ depth, const T* __restrict__ ucur,
                                                const T* __restrict__ vcur, T* __restrict__ pf1, int* __restrict__ jdv) {
  extern __shared__ __align__(16) unsigned char so_smem[];
  const DevTab<T>& tb = *tp;
  const SoTab<T>& so = *sp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ij = kijs + blockIdx.x * wpb + wave;
  if (ij >= kijl) return;  // wave-uniform, no block barrier below
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1;
  const bool intpol = mode & 1;
  const AbsLds L(NANG, NFRE, sizeof(T), intpol);
  const AbsTile<T> t(so_smem + (size_t)wave * L.bytes, L);
  fl2nd_load_intpol(tb, ip, t, ij, lane, intpol, fl1, wvprpt, ucur, vcur);
  const T* sF = t.sF;
  const size_t p = (size_t)(ij - kijs);
  {
#pragma clang fp contract(off)
    // FKMEAN (fkmean.F90:100-150): lane M sums its directions in ascending K; the sums over M run one after the other on every lane
    T temp2 = T(0), tempa = T(0);
    if (lane < NFRE) {
      const T* r = sF + lane * NAP;
      temp2 = r[0];
      for (int kk = 1; kk < NANG; kk++) temp2 = temp2 + r[kk];
      tempa = tb.DFIM[lane] / m_sqrt(wvprpt[(size_t)ij * (ECWAM_HIP_NWPR * NFRE) + lane]);
    }
    T em = tb.EPSMIN, ak = tb.EPSMIN;
    for (int m = 0; m < NFRE; m++) {
      const T t2 = lane_get(temp2, m);
      em = em + tb.DFIM[m] * t2;
      ak = ak + lane_get(tempa, m) * t2;
    }
    const T tl = lane_get(temp2, NFRE - 1);
    em = em + tb.WETAIL * tb.FR[NFRE - 1] * tb.DELTH * tl;
    ak = ak + tb.FRTAIL * tb.DELTH * m_sqrt(tb.G) / tb.ZPI * tl;
    const T q = em / ak;
    ak = q * q;
    const T dep = depth[ij];
    T xd = m_max(T(1) / ak, dep);
    xd = m_log(xd / so.DEPTHA) / so.XLOGD + T(1);
    int id = m_nint(xd);
    id = min(max(id, 1), so.NDEPTH) - 1;
    const int emaxl = (em <= so.ZFAC * (dep * dep)) ? 1 : 0;
    if (lane == 0) jdv[p] = id | (emaxl << 16);
    // thinning to PF1 (K0 = MA K + 1, M0 = MR M) and the f**-5 extension to NMAX
    const int AH = so.AH, NH = so.NH, NX = so.NMAX;
    for (int e = lane; e < AH * NX; e += 64) {
      const int m = e / AH, k = e - m * AH;
      const int k0 = (2 * k + 2) % NANG;
      const T v = m < NH ? sF[(2 * m + 1) * NAP + k0] : so.OMRT[m] * sF[(2 * NH - 1) * NAP + k0];
      pf1[(size_t)e * npad + p] = v;
    }
  }
}

// PF3(K,M) of 64 points for one M.  grid (npad / 64, NFREH), 64 threads.
template <typename T, int AH>
__global__ void __launch_bounds__(64) k_so_sum(const SoTab<T>* __restrict__ sp, const T* __restrict__ coef, int n, size_t npad,
                                              const T* __restrict__ pf1, const int* __restrict__ jdv, T* __restrict__ pf3) {
  const SoTab<T>& so = *sp;
  const int lane = threadIdx.x, m = blockIdx.y;
  const size_t p = (size_t)blockIdx.x * 64 + lane;
  const bool valid = p < (size_t)n;
  const int NH = so.NH;
  const int jd = valid ? (jdv[p] & 0xffff) : -1;
  const T* f2 = pf1 + p;  // F2(K,M) = f2[(M AH + K) npad]; p < npad always
  T acc[AH], f0[AH], dkp[AH], dkm[AH];
  {
    const T delm1 = so.DELM1[m];
    const int mp = so.MP[m], mm = so.MM[m];
#pragma unroll
    for (int k = 0; k < AH; k++) {
      acc[k] = T(0);
      f0[k] = valid ? f2[(size_t)(m * AH + k) * npad] : T(0);
      dkp[k] = valid ? f2[(size_t)(mp * AH + k) * npad] * delm1 : T(0);
      dkm[k] = valid ? f2[(size_t)(mm * AH + k) * npad] * delm1 : T(0);
    }
  }
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const int jdu = __builtin_amdgcn_readlane(jd, leader);  // wave-uniform: the coefficient loads below are scalar
    const bool mine = valid && jd == jdu;
    todo &= ~__ballot(mine);
    if (mine) {
      // (the constant address space makes the uniform loads scalar ones: the tables are never written while a kernel runs)
      typedef const __attribute__((address_space(4))) T* CPtr;
      const unsigned long long ca = (unsigned long long)(coef + ((size_t)jdu * NH + m) * NH * (5 * AH));
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)ca), hi = __builtin_amdgcn_readfirstlane((unsigned)(ca >> 32));
      const CPtr cm = (CPtr)(((unsigned long long)hi << 32) | lo);
      for (int m1 = 0; m1 < NH; m1++) {
        const int mmi = so.IMM[m * SO_MAXNH + m1], mpi = so.IMP[m * SO_MAXNH + m1];
        const CPtr cf = cm + (size_t)m1 * (5 * AH);
        T r1[AH], rm[AH], rp[AH];
#pragma unroll
        for (int k = 0; k < AH; k++) {
          r1[k] = f2[(size_t)(m1 * AH + k) * npad];
          rm[k] = f2[(size_t)(mmi * AH + k) * npad];
          rp[k] = f2[(size_t)(mpi * AH + k) * npad];
        }
        // TA is zero where OM1 >= OM0 / 2 (tables_2nd.F90:145-155): adding the zero term leaves the sum as the reference's skipped one
#pragma unroll
        for (int k = 0; k < AH; k++) {
#pragma unroll
          for (int k1 = 0; k1 < AH; k1++) {
            const int l = (k - k1 + AH) % AH;
            acc[k] = acc[k] + cf[l] * (r1[k1] * rm[k] + r1[k] * rm[k1]);
            T xincr = T(2) * cf[AH + l] * rp[k];
            xincr = xincr + cf[2 * AH + l] * f0[k];
            xincr = xincr - (dkp[k] * cf[4 * AH + l] - dkm[k] * cf[3 * AH + l]);
            acc[k] = acc[k] + r1[k1] * xincr;
          }
        }
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < AH; k++) pf3[(size_t)(m * AH + k) * npad + p] = acc[k];
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_so_post(const DevTab<T>* __restrict__ tp, const IntpolTab<T>* __restrict__ ip, const SoTab<T>* __restrict__ sp,
                                                 int kijs, int kijl, int wpb, int mode, size_t npad, size_t wbytes, T sig,
                                                 const T* __restrict__ fl1, const T* __restrict__ wvprpt, const T* __restrict__ ucur,
                                                 const T* __restrict__ vcur, const T* __restrict__ ff, const T* __restrict__ pf3,
                                                 const int* __restrict__ jdv, T zmiss, T* __restrict__ out, T* __restrict__ fl2nd) {
  extern __shared__ __align__(16) unsigned char so_smem[];
  const DevTab<T>& tb = *tp;
  const SoTab<T>& so = *sp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ij = kijs + blockIdx.x * wpb + wave;
  if (ij >= kijl) return;  // wave-uniform, no block barrier below
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE;
  const bool intpol = mode & 1;
  const AbsLds L(NANG, NFRE, sizeof(T), intpol);
  unsigned char* base = so_smem + (size_t)wave * wbytes;
  const AbsTile<T> t(base, L);
  T* sP = reinterpret_cast<T*>(base + L.bytes);  // PF3 [M][K] of the point
  const size_t p = (size_t)(ij - kijs);
  const int AH = so.AH, NH = so.NH;
  for (int e = lane; e < AH * NH; e += 64) sP[e] = pf3[(size_t)e * npad + p];
  fl2nd_load_intpol(tb, ip, t, ij, lane, intpol, fl1, wvprpt, ucur, vcur);  // ends with a wave barrier: sP is visible too
  {
#pragma clang fp contract(off)
    // the energy conserving interpolation back to NANG x NFRE (cal_second_order_spec.F90:148-192)
    const T es = ((jdv[p] >> 16) & 1) ? sig : T(0);  // EMAXL SIG
    T* sF = t.sF;
    for (int e = lane; e < N; e += 64) {
      const int kk = e / NFRE, mm = e - kk * NFRE;
      const int m0 = so.M0[mm], mp = so.MPI[mm];
      const T d1 = so.D1[mm], d2 = T(1) - d1;
      int k0 = kk / 2;
      const T d3 = T(kk) / T(2) - T(k0), d4 = T(1) - d3;
      if (k0 < 1) k0 += AH;
      int kp = k0 + 1;
      if (kp > AH) kp -= AH;
      k0 -= 1; kp -= 1;
      const T c1 = sP[m0 * AH + k0] * d4 + sP[m0 * AH + kp] * d3;
      const T c2 = sP[mp * AH + kp] * d3 + sP[mp * AH + k0] * d4;
      const T delf = c1 * d2 + c2 * d1;
      const T f = sF[mm * NAP + kk];
      sF[mm * NAP + kk] = m_max(m_min(so.SMALL, f), f + es * delf);
    }
    fl2nd_wsync();
  }
  if (mode & 2) fl2nd_ice(tb, t, ij, lane, ff);
  if (fl2nd) fl2nd_store(tb, t, ij, lane, (mode & 4) != 0, fl2nd);
  fl2nd_params(tb, t, lane, zmiss, out + (size_t)ij * 8);
}

template <typename T, int AH>
static void launch_sum(const SoTab<T>* so, const T* coef, int n, size_t npad, const T* pf1, const int* jdv, T* pf3, int NH, hipStream_t s) {
  hipLaunchKernelGGL((k_so_sum<T, AH>), dim3((unsigned)(npad / 64), NH), dim3(64), 0, s, so, coef, n, npad, pf1, jdv, pf3);
}

// 0 on success, 1: unsupported spectral size
template <typename T>
int launch_outbs_second_order(const void* tab, const void* itab, const void* sotab, const void* coef, void* work, int nmax, int kijs, int kijl, int mode,
                              const void* fl1, const void* wvprpt, const void* depth, const void* ucur, const void* vcur, const void* ff, double sig,
                              double zmiss, void* out, void* fl2nd, int NANG, int NFRE, hipStream_t s) {
  const int n = kijl - kijs;
  if (n <= 0) return 0;
  if (!outbs_size_ok(NANG, NFRE, sizeof(T))) return 1;
  const int AH = NANG / 2, NH = NFRE / 2;
  if (AH != 24 && AH != 18 && AH != 12 && AH != 6) return 1;
  const AbsLds L(NANG, NFRE, sizeof(T), mode & 1);
  const size_t wbytes = L.bytes + (((size_t)AH * NH * sizeof(T) + 15) & ~(size_t)15);
  if (wbytes > 64 * 1024) return 1;
  const size_t npad = ((size_t)n + 63) & ~(size_t)63;
  T* pf1 = (T*)work;
  T* pf3 = pf1 + (size_t)AH * nmax * npad;
  int* jdv = (int*)(pf3 + (size_t)AH * NH * npad);
  const SoTab<T>* so = (const SoTab<T>*)sotab;
  mode &= 3;
  if (fl2nd && NFRE % Vec16<T>::N == 0 && ((size_t)fl2nd & 15) == 0) mode |= 4;
  {
    const int wpb = (int)std::min<size_t>(4, (size_t)64 * 1024 / L.bytes);
    hipLaunchKernelGGL(k_so_pre<T>, dim3((n + wpb - 1) / wpb), dim3(64 * wpb), wpb * L.bytes, s, (const DevTab<T>*)tab, (const IntpolTab<T>*)itab, so,
                       kijs, kijl, wpb, mode, npad, (const T*)fl1, (const T*)wvprpt, (const T*)depth, (const T*)ucur, (const T*)vcur, pf1, jdv);
  }
  switch (AH) {
    case 24: launch_sum<T, 24>(so, (const T*)coef, n, npad, pf1, jdv, pf3, NH, s); break;
    case 18: launch_sum<T, 18>(so, (const T*)coef, n, npad, pf1, jdv, pf3, NH, s); break;
    case 12: launch_sum<T, 12>(so, (const T*)coef, n, npad, pf1, jdv, pf3, NH, s); break;
    default: launch_sum<T, 6>(so, (const T*)coef, n, npad, pf1, jdv, pf3, NH, s); break;
  }
  {
    const int wpb = (int)std::min<size_t>(4, (size_t)64 * 1024 / wbytes);
    hipLaunchKernelGGL(k_so_post<T>, dim3((n + wpb - 1) / wpb), dim3(64 * wpb), wpb * wbytes, s, (const DevTab<T>*)tab, (const IntpolTab<T>*)itab, so,
                       kijs, kijl, wpb, mode, npad, wbytes, (T)sig, (const T*)fl1, (const T*)wvprpt, (const T*)ucur, (const T*)vcur, (const T*)ff,
                       pf3, jdv, (T)zmiss, (T*)out, (T*)fl2nd);
  }
  return 0;
}
template int launch_outbs_second_order<float>(const void*, const void*, const void*, const void*, void*, int, int, int, int, const void*, const void*,
                                              const void*, const void*, const void*, const void*, double, double, void*, void*, int, int, hipStream_t);
template int launch_outbs_second_order<double>(const void*, const void*, const void*, const void*, void*, int, int, int, int, const void*, const void*,
                                               const void*, const void*, const void*, const void*, double, double, void*, void*, int, int, hipStream_t);
