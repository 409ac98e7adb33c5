// The start and the end of a run on the device (include/ecwam_hip_restart.h).
//   k_depthprpt      INITDPTHFLDS (initdpthflds.F90:54-88): EMAXDPT, then DEPTHPRPT (depthprpt.F90:60-82) on AKI's wave number (aki.F90:71-91)
//   k_buildstress    BUILDSTRESS 1.2 to 1.5 (buildstress.F90:231-318, readwgrib.F90:165-175) and GETSTRESS's statements around it (getstress.F90:95-97, 294-303)
//   k_stress_fields  the sixteen restart fields of SAVSTRESS (savstress.F90:112-127) and GETSTRESS (getstress.F90:150-165)
//   k_savspec_tile   WRITEFL's record (writefl.F90:113, 117): the transposition of csrc/gribout.hip for the whole spectrum
// k_depthprpt: one thread owns one 16-byte piece (4 single or 2 double precision frequencies) of a point's row of frequencies.  AKI is a Newton
// iteration whose number of steps differs from element to element: a thread iterates its elements in lockstep under a per-element mask, and the
// wave leaves the loop when a ballot shows no lane with an element left.  Every requested plane is written in whole 16-byte stores; no LDS, no
// atomics.  The thread of a point's first piece also writes EMAXDPT and DEPTH.
// k_buildstress and k_stress_fields: one thread per point with the row of ff in registers (FfRow: whole 16-byte pieces, only those the call reads
// or writes); the sixteen field vectors are read or written column by column, lanes along consecutive rows.  The positions of a relabelled
// vector come from the inverse of the map that ecwam_hip_set_restart_map validated on the host.
// k_savspec_tile: a block takes a tile of 64 points and ONE 16-byte piece of each direction: 64 x NANG pieces through an LDS tile
// [64][NANG VEC | 1] (the odd pitch of csrc/gribout.hip: the transposed read, lanes along the points, hits different banks), and NANG VEC field
// columns out, lanes along consecutive rows or scattered through the map.  The blocks that take the other pieces of a tile run on the same XCD.
// The arithmetic keeps the reference's order, without contraction.
#include "../../include/ecwam_hip_restart.h"
#include "dev.h"
#include "ff_row.h"
#include "launch.h"
#include "dd_math.h"      // after the HIP runtime: its <cmath> is the one the device overloads extend

namespace {

__device__ __forceinline__ float m_cosh(float x) { return coshf(x); }
__device__ __forceinline__ double m_cosh(double x) { return cosh(x); }

constexpr int AKI_MAXIT = 4096;      // where the reference would not return

template <typename T>
struct DepthPar {
  T dkmax, gam_b_j;
};

template <typename T>
__global__ void __launch_bounds__(256) k_depthprpt(const DevTab<T>* __restrict__ tp, int kijs, int kijl, int NFRE, const T* __restrict__ depth, const DepthPar<T> a,
                                                   T* __restrict__ wvprpt, T* __restrict__ wavnum, T* __restrict__ cgroup, T* __restrict__ omosnh2kd, T* __restrict__ ffa) {
#pragma clang fp contract(off)
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  const int np = NFRE / VEC;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long npts = (long long)(kijl - kijs);
  const bool valid = t < npts * np;
  const int ij = valid ? kijs + (int)(t / np) : kijs;
  const int p = valid ? (int)(t % np) : 0;
  const DevTab<T>& tb = *tp;
  const T G = tb.G, EBS = T(0.0001);
  const T beta = depth[ij];
  // ---- AKI per element
  T om[VEC], ao[VEC], ak[VEC];
  unsigned act = valid ? (1u << VEC) - 1u : 0u;
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    om[i] = tb.ZPIFR[p * VEC + i];
    const T akm1 = om[i] * om[i] / (T(4) * G);
    const T akm2 = om[i] / (T(2) * m_sqrt(G * beta));
    ao[i] = m_max(akm1, akm2);
    ak[i] = ao[i];
  }
  for (int it = 0; it < AKI_MAXIT; it++) {
    if (__ballot(act != 0u) == 0ull) break;
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      if (act & (1u << i)) {
        const T akp = ao[i];
        const T bo = beta * ao[i];
        if (bo > a.dkmax) {
          ak[i] = om[i] * om[i] / G;
          act &= ~(1u << i);
        } else {
          const T th = G * ao[i] * m_tanh(bo);
          const T sth = m_sqrt(th);
          const T ch = m_cosh(bo);
          ao[i] = ao[i] + (om[i] - sth) * sth * T(2) / (th / ao[i] + G * bo / (ch * ch));
          ak[i] = ao[i];
          if (!(m_abs(akp - ao[i]) > EBS * ao[i])) act &= ~(1u << i);
        }
      }
    }
  }
  if (!valid) return;
  // ---- DEPTHPRPT
  const T GH = G / (T(4) * tb.PI);
  VT wn, cg, ci, xk, sf, os;
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    const T AK = ak[i], OM = om[i];
    const T AKD = AK * beta;
    T CG, OS, SF;
    if (AKD <= T(10)) {
      CG = T(0.5) * m_sqrt(G * m_tanh(AKD) / AK) * (T(1) + T(2) * AKD / m_sinh(T(2) * AKD));
      OS = OM / m_sinh(T(2) * AKD);
      SF = T(2) * G * (AK * AK) / (OM * m_tanh(T(2) * AKD));
    } else {
      CG = GH / tb.FR[p * VEC + i];
      OS = T(0);
      SF = T(2) / G * (OM * OM * OM);
    }
    wn[i] = AK;
    cg[i] = CG;
    os[i] = OS;
    sf[i] = SF;
    ci[i] = AK / OM;
    xk[i] = AK * AK * CG;
  }
  const size_t o = (size_t)ij * NFRE + (size_t)p * VEC;
  if (wvprpt) {
    T* __restrict__ w = wvprpt + (size_t)ij * 5 * NFRE + (size_t)p * VEC;
    *reinterpret_cast<VT*>(w) = wn;
    *reinterpret_cast<VT*>(w + NFRE) = cg;
    *reinterpret_cast<VT*>(w + 2 * NFRE) = ci;
    *reinterpret_cast<VT*>(w + 3 * NFRE) = xk;
    *reinterpret_cast<VT*>(w + 4 * NFRE) = sf;
  }
  if (wavnum) *reinterpret_cast<VT*>(wavnum + o) = wn;
  if (cgroup) *reinterpret_cast<VT*>(cgroup + o) = cg;
  if (omosnh2kd) *reinterpret_cast<VT*>(omosnh2kd + o) = os;
  // ---- EMAXDPT and DEPTH: the last 16-byte piece of the row of ff
  if (ffa && p == 0) {
    const T GAM = beta < T(4) ? a.gam_b_j * beta / T(4) : a.gam_b_j;
    const T gd = GAM * beta;
    T* __restrict__ q = ffa + (size_t)ij * ECWAM_HIP_NFF + (ECWAM_HIP_NFF - VEC);
    VT x = {};
    if constexpr (VEC > 2) x = *reinterpret_cast<const VT*>(q);      // single precision: CHRNCK and CITHICK share the piece
    x[VEC - 2] = T(0.0625) * (gd * gd);
    x[VEC - 1] = beta;
    *reinterpret_cast<VT*>(q) = x;
  }
}

// CDUSTARZ0 (cdustarz0.F90:66-71) for one point; POW and EXP as csrc/forcing.hip::k_cdustarz0 takes them
template <typename T>
__device__ __forceinline__ void cdustarz0_point(const DevTab<T>& tb, T u10, T zref, T& cd, T& ustar, T& z0) {
#pragma clang fp contract(off)
  const T C1CD = T(1.03e-3), C2CD = T(0.04e-3), P1CD = T(1.48), P2CD = T(-0.21), Z0MIN = T(0.000001);      // yowpcons.F90:61-64, cdustarz0.F90:57
  const T u10p = m_max(u10, tb.WSPMIN);
  cd = m_min((C1CD + C2CD * ref_pow(u10p, P1CD)) * ref_pow(u10p, P2CD), tb.CDMAX);
  ustar = m_max(m_sqrt(cd) * u10p, tb.EPSUS);
  z0 = m_max(zref / (ref_exp(tb.XKAPPA * m_min(u10p / ustar, T(100))) - T(1)), Z0MIN);
}

template <typename T>
struct StressPar {
  T zref, prchar, zmiss;
  int nsestart;
};

// MODE: bit 0 Z0B = 0, bit 1 a plane of wind speeds, bit 2 CHRNCK is written (a plane of drag coefficients, or the noise start)
template <typename T, int MODE>
__global__ void __launch_bounds__(256) k_buildstress(const DevTab<T>* __restrict__ tp, int kijs, int kijl, const int* __restrict__ map, const T* __restrict__ uwave,
                                                     const T* __restrict__ cdin, const StressPar<T> a, T* __restrict__ ffa) {
#pragma clang fp contract(off)
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const DevTab<T>& tb = *tp;
  constexpr unsigned W = col(F_UFRIC) | col(F_TAUW) | col(F_TAUWDIR) | col(F_Z0M) | ((MODE & 1) ? col(F_Z0B) : 0u) | ((MODE & 2) ? col(F_WSWAVE) : 0u) |
                         ((MODE & 4) ? col(F_CHRNCK) : 0u);
  T* __restrict__ frow = ffa + (size_t)ij * ECWAM_HIP_NFF;
  FfRow<T> r;
  r.template load_for<col(F_WSWAVE) | col(F_WDWAVE), W>(frow);
  if constexpr ((MODE & 1) != 0) r.v[F_Z0B] = T(0);
  if constexpr ((MODE & 2) != 0) {
    const T w = uwave[map[ij]];
    if (w != a.zmiss && w > T(0)) r.v[F_WSWAVE] = w;
  }
  const T ws = r.v[F_WSWAVE];
  T CD, USTAR, Z0;
  cdustarz0_point(tb, ws, a.zref, CD, USTAR, Z0);
  r.v[F_UFRIC] = USTAR;
  r.v[F_Z0M] = Z0;
  r.v[F_TAUW] = T(0.1) * (USTAR * USTAR);
  r.v[F_TAUWDIR] = r.v[F_WDWAVE];
  if constexpr ((MODE & 4) != 0) {
    if (cdin) {
      const T c = cdin[map[ij]];
      if (c != a.zmiss && c > T(0)) CD = c;
      // CHNKMIN (chnkmin.F90:60)
      const T alphaog = tb.LLCAPCHNK ? (tb.ALPHAMIN + (tb.ALPHA - tb.ALPHAMIN) * T(0.5) * (T(1) - m_tanh(ws - tb.CHNKMIN_U))) * tb.GM1 : tb.ALPHA * tb.GM1;
      T uf = CD * m_max(ws * ws, tb.EPSU10 * tb.EPSU10);
      uf = m_max(uf, tb.EPSUS);
      const T ustar = m_sqrt(uf);
      const T cdsqrtinv = m_min(T(1) / m_sqrt(CD), T(50));
      const T z0tot = a.zref * ref_exp(-tb.XKAPPA * cdsqrtinv);
      const T z0m = m_max(z0tot - tb.RNUM / ustar, alphaog * uf);
      T ch = z0m / uf;
      ch = m_max(ch, alphaog);
      const T q = alphaog / ch;
      r.v[F_Z0M] = z0m;
      r.v[F_TAUW] = m_max(uf * (T(1) - q * q), T(0));
      r.v[F_TAUWDIR] = r.v[F_WDWAVE];
      r.v[F_CHRNCK] = tb.G * ch;
      r.v[F_UFRIC] = ustar;
    }
    if (a.nsestart) {
      r.v[F_CHRNCK] = a.prchar;
      r.v[F_TAUW] = T(0);
    }
  }
  r.template store<W>(frow);
}

// the columns of ff in the order of the restart fields (savstress.F90:112-125)
struct StressCols { unsigned char c[14]; };
constexpr unsigned STRESS_COLS = (1u << 14) - 1u;      // columns 0 .. 13

template <typename T, bool PACK>
__global__ void __launch_bounds__(256) k_stress_fields(int kijs, int kijl, const int* __restrict__ inv, T* __restrict__ ffa, T* __restrict__ ucur, T* __restrict__ vcur,
                                                       T* __restrict__ rfield, size_t ld) {
  constexpr StressCols sc = {{F_WSWAVE, F_WDWAVE, F_UFRIC, F_TAUW, F_TAUWDIR, F_Z0M, F_Z0B, F_CHRNCK, F_AIRD, F_WSTAR, F_CICOVER, F_CITHICK, F_USTRA, F_VSTRA}};
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const size_t pos = inv ? (size_t)inv[ij] : (size_t)ij;
  T* __restrict__ frow = ffa + (size_t)ij * ECWAM_HIP_NFF;
  FfRow<T> r;
  if constexpr (PACK) {
    r.template load<STRESS_COLS>(frow);
#pragma unroll
    for (int f = 0; f < 14; f++) rfield[ld * f + pos] = r.v[sc.c[f]];
    rfield[ld * 14 + pos] = ucur[ij];
    rfield[ld * 15 + pos] = vcur[ij];
  } else {
    r.template load_for<0u, STRESS_COLS>(frow);      // single precision: EMAXDPT and DEPTH share a piece with CHRNCK and CITHICK
#pragma unroll
    for (int f = 0; f < 14; f++) r.v[sc.c[f]] = rfield[ld * f + pos];
    r.template store<STRESS_COLS>(frow);
    ucur[ij] = rfield[ld * 14 + pos];
    vcur[ij] = rfield[ld * 15 + pos];
  }
}

constexpr int TILE = 64, NTHR = 256, NWAVE = NTHR / 64, NXCD = 8;

template <typename T>
__global__ void __launch_bounds__(NTHR) k_savspec_tile(const T* __restrict__ fl1, int kijs, int kijl, int ifld0, int ifld1, int NANG, int NFRE, int p_lo, int ny, int ntiles,
                                                       const int* __restrict__ inv, T* __restrict__ blk, size_t ld) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ncol = NANG * VEC, P = ncol | 1;
  T* __restrict__ tile = reinterpret_cast<T*>(smem);      // [TILE][P]
  // blocks b, b + 8, b + 16 ... run on one XCD: they take the ny pieces of one tile, then those of the tile 8 further on
  const int b = (int)blockIdx.x, j = b / NXCD, t = (j / ny) * NXCD + b % NXCD, p = p_lo + j % ny;
  if (t >= ntiles) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ij0 = kijs + t * TILE, npt = kijl - ij0 < TILE ? kijl - ij0 : TILE;
  for (int idx = tid; idx < npt * NANG; idx += NTHR) {
    const int pt = idx / NANG, k = idx - pt * NANG;
    const VT x = *reinterpret_cast<const VT*>(fl1 + ((size_t)(ij0 + pt) * NANG + k) * NFRE + p * VEC);
#pragma unroll
    for (int i = 0; i < VEC; i++) tile[pt * P + k * VEC + i] = x[i];
  }
  __syncthreads();
  if (lane >= npt) return;
  const int ij = ij0 + lane;
  const size_t pos = inv ? (size_t)inv[ij] : (size_t)ij;
  for (int c = wave; c < ncol; c += NWAVE) {
    const int k = c / VEC, m = p * VEC + c % VEC, f = m * NANG + k;
    if (f < ifld0 || f >= ifld1) continue;      // the same for the whole wave
    blk[(size_t)(f - ifld0) * ld + pos] = tile[lane * P + c];
  }
}

}  // namespace

template <typename T>
int launch_depthprpt(const void* tab, int kijs, int kijl, const void* depth, double dkmax, double gam_b_j, void* wvprpt, void* wavnum, void* cgroup, void* omosnh2kd, void* ff,
                     int NFRE, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  if (kijl <= kijs) return 0;
  const DepthPar<T> a = {T(dkmax), T(gam_b_j)};
  const long long nthr = (long long)(kijl - kijs) * (NFRE / VEC);
  hipLaunchKernelGGL((k_depthprpt<T>), dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, NFRE, (const T*)depth, a, (T*)wvprpt,
                     (T*)wavnum, (T*)cgroup, (T*)omosnh2kd, (T*)ff);
  return 0;
}

template <typename T, int MODE>
static void buildstress_go(const void* tab, int kijs, int kijl, const int* map, const void* uwave, const void* cd, const StressPar<T>& a, void* ff, hipStream_t s) {
  hipLaunchKernelGGL((k_buildstress<T, MODE>), dim3((unsigned)((kijl - kijs + 255) / 256)), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, map, (const T*)uwave,
                     (const T*)cd, a, (T*)ff);
}

template <typename T>
void launch_buildstress(const void* tab, int kijs, int kijl, const int* map, const void* uwave, const void* cd, double zref, int flags, double prchar, double zmiss, void* ff,
                        hipStream_t s) {
  if (kijl <= kijs) return;
  const StressPar<T> a = {T(zref), T(prchar), T(zmiss), (flags & ECWAM_HIP_BST_NSESTART) != 0};
  const int mode = ((flags & ECWAM_HIP_BST_Z0B_ZERO) ? 1 : 0) | (uwave ? 2 : 0) | ((cd || a.nsestart) ? 4 : 0);
  switch (mode) {
    case 0: buildstress_go<T, 0>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
    case 1: buildstress_go<T, 1>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
    case 2: buildstress_go<T, 2>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
    case 3: buildstress_go<T, 3>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
    case 4: buildstress_go<T, 4>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
    case 5: buildstress_go<T, 5>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
    case 6: buildstress_go<T, 6>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
    default: buildstress_go<T, 7>(tab, kijs, kijl, map, uwave, cd, a, ff, s); break;
  }
}

template <typename T>
void launch_stress_fields(int pack, int kijs, int kijl, const int* inv, void* ff, void* ucur, void* vcur, void* rfield, size_t ld, hipStream_t s) {
  if (kijl <= kijs) return;
  const dim3 grid((unsigned)((kijl - kijs + 255) / 256));
  if (pack)
    hipLaunchKernelGGL((k_stress_fields<T, true>), grid, dim3(256), 0, s, kijs, kijl, inv, (T*)ff, (T*)ucur, (T*)vcur, (T*)rfield, ld);
  else
    hipLaunchKernelGGL((k_stress_fields<T, false>), grid, dim3(256), 0, s, kijs, kijl, inv, (T*)ff, (T*)ucur, (T*)vcur, (T*)rfield, ld);
}

template <typename T>
int launch_savspec_pack(int kijs, int kijl, const void* fl1, int ifld0, int nfld, const int* inv, void* blk, size_t ld, int NANG, int NFRE, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  const size_t lds = (size_t)TILE * ((NANG * VEC) | 1) * sizeof(T);
  if (lds > 64 * 1024) return 1;
  if (kijl <= kijs) return 0;
  const int m_lo = ifld0 / NANG, m_hi = (ifld0 + nfld - 1) / NANG + 1;      // the frequencies of the field range
  const int p_lo = m_lo / VEC, ny = (m_hi + VEC - 1) / VEC - p_lo;
  const int ntiles = (kijl - kijs + TILE - 1) / TILE;
  const unsigned nblk = (unsigned)((ntiles + NXCD - 1) / NXCD) * NXCD * (unsigned)ny;
  hipLaunchKernelGGL((k_savspec_tile<T>), dim3(nblk), dim3(NTHR), lds, s, (const T*)fl1, kijs, kijl, ifld0, ifld0 + nfld, NANG, NFRE, p_lo, ny, ntiles, inv, (T*)blk, ld);
  return 0;
}

#define RESTART_INSTANTIATE(T)                                                                                                                                   \
  template int launch_depthprpt<T>(const void*, int, int, const void*, double, double, void*, void*, void*, void*, void*, int, hipStream_t);                     \
  template void launch_buildstress<T>(const void*, int, int, const int*, const void*, const void*, double, int, double, double, void*, hipStream_t);             \
  template void launch_stress_fields<T>(int, int, int, const int*, void*, void*, void*, void*, size_t, hipStream_t);                                            \
  template int launch_savspec_pack<T>(int, int, const void*, int, int, const int*, void*, size_t, int, int, hipStream_t);
RESTART_INSTANTIATE(float)
RESTART_INSTANTIATE(double)
#undef RESTART_INSTANTIATE
