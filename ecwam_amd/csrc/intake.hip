// The forcing intake on the device (include/ecwam_hip_intake.h): what PREWIND runs in front of GETWND, and what WAMODEL hands to NEMO at its end.
//   k_fldinter        FLDINTER (fldinter.F90:176-374): the bilinear interpolation of IFSTOWAM through the per-point table of ecwam_hip_set_fldinter
//   k_init_fieldg     the LLINIALL branch of INIT_FIELDG (init_fieldg.F90:92-116)
//   k_recvnemofields  the point-wise branches of RECVNEMOFIELDS (recvnemofields.F90:101-110, 176-250)
//   k_updnemo         UPDNEMOFIELDS (updnemofields.F90:92-98) and UPDNEMOSTRESS (updnemostress.F90:84-132)
// One thread per sea point (k_init_fieldg: per 16-byte piece).  k_fldinter is a gather: a point's table is one 16-byte load of its four source
// positions and the weights padded to whole pieces, and its 4 x (up to 10) field values are independent loads, all issued before the first is used;
// the positions were validated on the host, the atmosphere's fields are small enough to be served by the caches.  The stores go through the inbound
// map of ecwam_hip_set_forcing_map, whose cells ecwam_hip_set_fldinter found distinct.  The arithmetic keeps the reference's order, without
// contraction; the division of the sea-ice rule is the compiler's correctly rounded one.
#include "../../include/ecwam_hip_intake.h"
#include "dev.h"
#include "launch.h"

template <typename T> struct FliWeights;      // DJ1, DII1, DIIP1 and padding: one (single) or two (double precision) pieces of 16 bytes
template <> struct alignas(16) FliWeights<float> { float dj1, dii1, diip1, pad; };
template <> struct alignas(16) FliWeights<double> { double dj1, dii1, diip1, pad; };

template <typename T>
struct FliPar {
  T roair, wstar0, pmiss;
  int laden, lgust, llkc;
};

// USE: the fields beyond U10, V10, the sea ice fraction and the stresses that the interpolation reads -- bit 0 the air density (LADEN), 1 w* (LGUST),
// 2 the lake fraction (LLKC), 3 the currents (NEWCURR and LWCUR); CUR: NEWCURR, the current planes are written (as 0 without bit 3 of USE).
// Without INTERPOL (LLINTERPOL = F) a point reads one position of each field, and the reference's expressions with ZLADEN, ZLGUST and ZLLKC are kept
// as they stand: all eight fields are read.
template <typename T, bool INTERPOL, int USE, bool CUR>
__global__ void __launch_bounds__(256) k_fldinter(int kijs, int kijl, const int4* __restrict__ idx, const FliWeights<T>* __restrict__ wgt, const int* __restrict__ map,
                                                  const T* __restrict__ fields, size_t ngptotg, T* __restrict__ fieldg, size_t ncell, int* __restrict__ mask_in,
                                                  const FliPar<T> a) {
#pragma clang fp contract(off)
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const int4 p = idx[ij];
  T* __restrict__ o = fieldg + map[ij];
  if constexpr (!INTERPOL) {
    T f[10];
#pragma unroll
    for (int k = 0; k < ((USE & 8) ? 10 : 8); k++) f[k] = fields[ngptotg * k + p.x];
    if (mask_in) mask_in[p.x] = 1;
    const T zladen = a.laden ? T(1) : T(0), zlgust = a.lgust ? T(1) : T(0), zllkc = a.llkc ? T(1) : T(0);
    o[ECWAM_HIP_FG_UWND * ncell] = f[0];
    o[ECWAM_HIP_FG_VWND * ncell] = f[1];
    o[ECWAM_HIP_FG_AIRD * ncell] = zladen * f[2] + (T(1) - zladen) * a.roair;
    o[ECWAM_HIP_FG_WSTAR * ncell] = zlgust * f[3] + (T(1) - zlgust) * a.wstar0;
    o[ECWAM_HIP_FG_CICOVER * ncell] = f[4];
    o[ECWAM_HIP_FG_LKFR * ncell] = zllkc * f[5];
    o[ECWAM_HIP_FG_USTRA * ncell] = f[6];
    o[ECWAM_HIP_FG_VSTRA * ncell] = f[7];
    o[ECWAM_HIP_FG_CITHICK * ncell] = T(0);
    if constexpr (CUR) {
      o[ECWAM_HIP_FG_UCUR * ncell] = (USE & 8) ? f[8] : T(0);
      o[ECWAM_HIP_FG_VCUR * ncell] = (USE & 8) ? f[9] : T(0);
    }
  } else {
    // the fields read: 0, 1, 4, 6, 7 always
    constexpr unsigned READ = 0xD3u | ((USE & 1) ? 4u : 0u) | ((USE & 2) ? 8u : 0u) | ((USE & 4) ? 32u : 0u) | ((USE & 8) ? 0x300u : 0u);
    const FliWeights<T> w = wgt[ij];
    T f00[10], f10[10], f01[10], f11[10];
#pragma unroll
    for (int k = 0; k < 10; k++)
      if (READ & (1u << k)) {
        const T* __restrict__ fk = fields + ngptotg * k;
        f00[k] = fk[p.x];
        f10[k] = fk[p.y];
        f01[k] = fk[p.z];
        f11[k] = fk[p.w];
      }
    if (mask_in) {
      mask_in[p.x] = 1;
      mask_in[p.y] = 1;
      mask_in[p.z] = 1;
      mask_in[p.w] = 1;
    }
    const T dj1 = w.dj1, dj2 = T(1) - dj1, dii1 = w.dii1, dii2 = T(1) - dii1, diip1 = w.diip1, diip2 = T(1) - diip1;
    T r[10];
#pragma unroll
    for (int k = 0; k < 10; k++)
      if (READ & (1u << k)) r[k] = dj2 * (dii2 * f00[k] + dii1 * f10[k]) + dj1 * (diip2 * f01[k] + diip1 * f11[k]);
    // the sea ice fraction: with a missing corner the nearest corner's value if it is there, else the mean of the corners that are (fldinter.F90:276-330)
    const T pm = a.pmiss;
    const bool m00 = f00[4] == pm, m10 = f10[4] == pm, m01 = f01[4] == pm, m11 = f11[4] == pm;
    const bool top = dj1 <= T(0.5);
    const bool first = top ? dii1 <= T(0.5) : diip1 <= T(0.5);
    const T nearest = top ? (first ? f00[4] : f10[4]) : (first ? f01[4] : f11[4]);
    T sum = T(0);
    sum = m00 ? sum : sum + f00[4];
    sum = m10 ? sum : sum + f10[4];
    sum = m01 ? sum : sum + f01[4];
    sum = m11 ? sum : sum + f11[4];
    const int ncount = 4 - (int)m00 - (int)m10 - (int)m01 - (int)m11;
    const T mean = ncount > 0 ? sum / T(ncount > 0 ? ncount : 1) : pm;
    const T ci = (m00 || m10 || m01 || m11) ? (nearest == pm ? mean : nearest) : r[4];
    o[ECWAM_HIP_FG_UWND * ncell] = r[0];
    o[ECWAM_HIP_FG_VWND * ncell] = r[1];
    o[ECWAM_HIP_FG_AIRD * ncell] = (USE & 1) ? r[2] : a.roair;
    o[ECWAM_HIP_FG_WSTAR * ncell] = (USE & 2) ? r[3] : a.wstar0;
    o[ECWAM_HIP_FG_CICOVER * ncell] = ci;
    o[ECWAM_HIP_FG_CITHICK * ncell] = T(0);
    o[ECWAM_HIP_FG_LKFR * ncell] = (USE & 4) ? r[5] : T(0);
    o[ECWAM_HIP_FG_USTRA * ncell] = r[6];
    o[ECWAM_HIP_FG_VSTRA * ncell] = r[7];
    if constexpr (CUR) {
      o[ECWAM_HIP_FG_UCUR * ncell] = (USE & 8) ? r[8] : T(0);
      o[ECWAM_HIP_FG_VCUR * ncell] = (USE & 8) ? r[9] : T(0);
    }
  }
}

// one thread per 16-byte piece of the 13 planes; a piece may lie across two planes.  The elements behind the last whole piece are stored one by one.
template <typename T>
__global__ void __launch_bounds__(256) k_init_fieldg(const DevTab<T>* __restrict__ tp, T* __restrict__ fieldg, size_t ncell, T roair, T wstar0) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  const size_t total = ncell * ECWAM_HIP_NFIELDG, whole = total / VEC;
  const T wspmin = tp->WSPMIN;
  auto value = [&](size_t g) {
    const int plane = (int)(g / ncell);
    return plane == ECWAM_HIP_FG_WSWAVE ? wspmin : plane == ECWAM_HIP_FG_AIRD ? roair : plane == ECWAM_HIP_FG_WSTAR ? wstar0 : T(0);
  };
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < whole; v += (size_t)gridDim.x * 256) {
    VT x;
#pragma unroll
    for (int i = 0; i < VEC; i++) x[i] = value(v * VEC + i);
    *reinterpret_cast<VT*>(fieldg + v * VEC) = x;
  }
  if (blockIdx.x == 0 && threadIdx.x < total - whole * VEC) fieldg[whole * VEC + threadIdx.x] = value(whole * VEC + threadIdx.x);
}

// SIGN(MIN(ABS(x), CURRENT_MAX), x) in NEMO's kind
__device__ __forceinline__ double nemo_clip(double x) { return copysign(fmin(fabs(x), 1.5), x); }

// the 16-byte piece of a row of 16 reals that holds column C
template <typename T, int C>
struct RowPiece {
  static constexpr int VEC = 16 / (int)sizeof(T), AT = (C / VEC) * VEC, IN = C % VEC;
  typedef T VT __attribute__((ext_vector_type(VEC)));
  VT x;
  __device__ __forceinline__ void load(const T* __restrict__ row) { x = *reinterpret_cast<const VT*>(row + AT); }
  __device__ __forceinline__ void store(T* __restrict__ row) const { *reinterpret_cast<VT*>(row + AT) = x; }
  __device__ __forceinline__ T get() const { return x[IN]; }
  __device__ __forceinline__ void set(T v) { x[IN] = v; }
};

// flags: ECWAM_HIP_RNF_*, uniform over the launch
template <typename T>
__global__ void __launch_bounds__(256) k_recvnemofields(int kijs, int kijl, int flags, const int* __restrict__ map, const T* __restrict__ fieldg, size_t ncell,
                                                        double* __restrict__ nemo, double* __restrict__ nemoibr, T* __restrict__ ffa, T* __restrict__ ucur,
                                                        T* __restrict__ vcur, T* __restrict__ intfa) {
#pragma clang fp contract(off)
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const bool rest = flags & ECWAM_HIP_RNF_LREST, init = flags & ECWAM_HIP_RNF_LINIT, cou = flags & ECWAM_HIP_RNF_LWCOU;
  const bool cic = flags & ECWAM_HIP_RNF_LWNEMOCOUCIC, cit = flags & ECWAM_HIP_RNF_LWNEMOCOUCIT, cur = flags & ECWAM_HIP_RNF_LWNEMOCOUCUR;
  const bool ibr = flags & ECWAM_HIP_RNF_LWNEMOCOUIBR;
  T* __restrict__ frow = ffa + (size_t)ij * ECWAM_HIP_NFF;
  T* __restrict__ irow = intfa + (size_t)ij * ECWAM_HIP_NINTF;
  const size_t n = (size_t)kijl;
  // the pieces a branch reads or gives back beside the column it writes: CICOVER [2], CITHICK [13] of ff, IBRMEM [15] of intf
  const bool w_ci = init && (cic || (cit && cou)), w_ct = init && cit, w_ib = init && ibr;
  RowPiece<T, 2> pci;
  RowPiece<T, 13> pct;
  RowPiece<T, 15> pib;
  if (rest || w_ci) pci.load(frow);
  if (rest || w_ct) pct.load(frow);
  if (ibr && (rest || w_ib)) pib.load(irow);
  double ncic = 0, ncit = 0, nu = 0, nv = 0, nib = 0;
  if (rest) {      // the restart file's values become NEMO's
    ncic = (double)pci.get();
    ncit = (double)pct.get();
    nu = (double)ucur[ij];
    nv = (double)vcur[ij];
    nemo[ij] = ncic;
    nemo[n + ij] = ncit;
    nemo[2 * n + ij] = nu;
    nemo[3 * n + ij] = nv;
    if (ibr) {
      nib = (double)pib.get();
      nemoibr[ij] = nib;
    }
  } else {
    if (cic || cit) ncic = nemo[ij];
    if (cit) ncit = nemo[n + ij];
    if (cur) {
      nu = nemo[2 * n + ij];
      nv = nemo[3 * n + ij];
    }
    if (ibr) nib = nemoibr[ij];
  }
  if (!init) return;
  if (cou) {
    // no lake cover: an open ocean point takes NEMO's values.  Only the cover, the thickness and the currents ask: without them neither the map
    // nor fieldg is read (ecwam_hip_recvnemofields lets fieldg be NULL then)
    const bool asks = cic || cit || cur;
    const size_t cell = asks ? (size_t)map[ij] : 0;
    const bool ocean = asks ? fieldg[ECWAM_HIP_FG_LKFR * ncell + cell] <= T(0) : true;
    if (cic) pci.set(ocean ? T(ncic) : fieldg[ECWAM_HIP_FG_CICOVER * ncell + cell]);
    if (cit) {
      if (ocean) pct.set(T(ncic * ncit));
      else pci.set(T(0.5 * ncic));      // recvnemofields.F90:201 as it stands: the cover, not the thickness
    }
    if (cur) {
      ucur[ij] = ocean ? T(nemo_clip(nu)) : T(0);
      vcur[ij] = ocean ? T(nemo_clip(nv)) : T(0);
    }
  } else {
    if (cic) pci.set(T(ncic));
    if (cit) pct.set(T(ncic * ncit));
    if (cur) {
      ucur[ij] = T(nu);
      vcur[ij] = T(nv);
    }
  }
  if (ibr) pib.set(T(nib));
  if (w_ci) pci.store(frow);
  if (w_ct) pct.store(frow);
  if (w_ib) pib.store(irow);
}

__global__ void __launch_bounds__(256) k_updnemo(int kijs, int kijl, double* __restrict__ wam2nemo, int scale, double znemontaum1, double* __restrict__ fields7,
                                                 double* __restrict__ stress6, size_t ld) {
#pragma clang fp contract(off)
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  // the columns of wam2nemo (ecwam_hip_implsch) in the order of the outputs
  constexpr int UPD_FIELDS[7] = {5, 6, 3, 4, 2, 0, 1};      // NSWH, NMWP, NPHIEPS, NTAUOC, NEMOSTRN, NEMOUSTOKES, NEMOVSTOKES
  constexpr int UPD_STRESS[6] = {7, 8, 11, 12, 9, 10};      // NEMOTAUX, NEMOTAUY, NEMOWSWAVE, NEMOPHIF, NEMOTAUICX, NEMOTAUICY
  double* __restrict__ row = wam2nemo + (size_t)ij * 13;
  if (fields7) {
#pragma unroll
    for (int f = 0; f < 7; f++) fields7[ld * f + ij] = row[UPD_FIELDS[f]];
  }
  if (stress6) {
#pragma unroll
    for (int f = 0; f < 6; f++) {
      stress6[ld * f + ij] = scale ? row[UPD_STRESS[f]] * znemontaum1 : 0.0;
      row[UPD_STRESS[f]] = 0.0;      // the accumulation starts again
    }
  }
}

static inline dim3 rows_grid(int kijs, int kijl) { return dim3((unsigned)((kijl - kijs + 255) / 256)); }

template <typename T, bool INTERPOL, bool CUR>
static void fldinter_go(int use, int kijs, int kijl, const void* idx, const void* wgt, const int* map, const void* fields, size_t ngptotg, void* fieldg, size_t ncell,
                        int* mask_in, const FliPar<T>& a, hipStream_t s) {
  switch (use) {
#define FLI_CASE(U_)                                                                                                                                             \
  case U_:                                                                                                                                                       \
    hipLaunchKernelGGL((k_fldinter<T, INTERPOL, U_, CUR>), rows_grid(kijs, kijl), dim3(256), 0, s, kijs, kijl, (const int4*)idx, (const FliWeights<T>*)wgt, map, \
                       (const T*)fields, ngptotg, (T*)fieldg, ncell, mask_in, a);                                                                                \
    break
    FLI_CASE(0); FLI_CASE(1); FLI_CASE(2); FLI_CASE(3); FLI_CASE(4); FLI_CASE(5); FLI_CASE(6); FLI_CASE(7);
    FLI_CASE(8); FLI_CASE(9); FLI_CASE(10); FLI_CASE(11); FLI_CASE(12); FLI_CASE(13); FLI_CASE(14); FLI_CASE(15);
#undef FLI_CASE
  }
}
template <typename T>
void launch_fldinter(int kijs, int kijl, const void* idx, const void* wgt, int interpol, const int* map, const void* fields, size_t ngptotg, int flags, double roair,
                     double wstar0, double pmiss, void* fieldg, size_t ncell, int* mask_in, hipStream_t s) {
  if (kijl <= kijs) return;
  FliPar<T> a = {T(roair), T(wstar0), T(pmiss), (flags & ECWAM_HIP_FLI_LADEN) != 0, (flags & ECWAM_HIP_FLI_LGUST) != 0, (flags & ECWAM_HIP_FLI_LLKC) != 0};
  const bool cur = (flags & ECWAM_HIP_FLI_NEWCURR) != 0;
  const int curf = cur && (flags & ECWAM_HIP_FLI_LWCUR) ? 8 : 0;
  if (!interpol) {      // every field is read whatever the switches: only the currents make another kernel
#define FLI_PLAIN(U_, C_)                                                                                                                                   \
  hipLaunchKernelGGL((k_fldinter<T, false, U_, C_>), rows_grid(kijs, kijl), dim3(256), 0, s, kijs, kijl, (const int4*)idx, (const FliWeights<T>*)wgt, map, \
                     (const T*)fields, ngptotg, (T*)fieldg, ncell, mask_in, a)
    if (curf) FLI_PLAIN(8, true);
    else if (cur) FLI_PLAIN(0, true);
    else FLI_PLAIN(0, false);
#undef FLI_PLAIN
    return;
  }
  const int use = (flags & (ECWAM_HIP_FLI_LADEN | ECWAM_HIP_FLI_LGUST | ECWAM_HIP_FLI_LLKC)) | curf;
  if (cur) fldinter_go<T, true, true>(use, kijs, kijl, idx, wgt, map, fields, ngptotg, fieldg, ncell, mask_in, a, s);
  else fldinter_go<T, true, false>(use, kijs, kijl, idx, wgt, map, fields, ngptotg, fieldg, ncell, mask_in, a, s);
}
template <typename T>
void launch_init_fieldg(const void* tab, void* fieldg, size_t ncell, double roair, double wstar0, hipStream_t s) {
  if (ncell == 0) return;
  const size_t want = (ncell * ECWAM_HIP_NFIELDG / (16 / sizeof(T)) + 255) / 256 + 1;
  hipLaunchKernelGGL((k_init_fieldg<T>), dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s, (const DevTab<T>*)tab, (T*)fieldg, ncell, T(roair), T(wstar0));
}
template <typename T>
void launch_recvnemofields(int kijs, int kijl, int flags, const int* map, const void* fieldg, size_t ncell, double* nemo, double* nemoibr, void* ff, void* ucur,
                           void* vcur, void* intf, hipStream_t s) {
  if (kijl <= kijs) return;
  hipLaunchKernelGGL((k_recvnemofields<T>), rows_grid(kijs, kijl), dim3(256), 0, s, kijs, kijl, flags, map, (const T*)fieldg, ncell, nemo, nemoibr, (T*)ff, (T*)ucur,
                     (T*)vcur, (T*)intf);
}
void launch_updnemo(int kijs, int kijl, double* wam2nemo, int scale, double znemontaum1, double* fields7, double* stress6, int ld, hipStream_t s) {
  if (kijl <= kijs || (!fields7 && !stress6)) return;
  hipLaunchKernelGGL(k_updnemo, rows_grid(kijs, kijl), dim3(256), 0, s, kijs, kijl, wam2nemo, scale, znemontaum1, fields7, stress6, (size_t)ld);
}

#define INTAKE_INSTANTIATE(T)                                                                                                                                        \
  template void launch_fldinter<T>(int, int, const void*, const void*, int, const int*, const void*, size_t, int, double, double, double, void*, size_t, int*,     \
                                   hipStream_t);                                                                                                                     \
  template void launch_init_fieldg<T>(const void*, void*, size_t, double, double, hipStream_t);                                                                      \
  template void launch_recvnemofields<T>(int, int, int, const int*, const void*, size_t, double*, double*, void*, void*, void*, void*, hipStream_t);
INTAKE_INSTANTIATE(float)
INTAKE_INSTANTIATE(double)
#undef INTAKE_INSTANTIATE
