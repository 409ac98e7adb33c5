// Dual rotated-quadrant propagation, IPROPAGS = 1 (include/ecwam_hipx_propags1.h): section 3 of PROPAGS1 (propags1.F90:537-925), the spherical grid with
// IREFRA 0 or 1, with CHECKCFL's arguments as :867-878 forms them at M = 1.  Sections 1, 2 and 4 of PROPAGS1 are those of PROPAGS and run k_propags
// (propags.hip; section 4 in its build with the product form of DP1 / DP2).
// k_propags1 has the shape of k_propags: the layout FL[row][K][NFRE]; a block takes a tile of PG1_TP points.  What depends on the point only is formed once
// per point and goes to LDS: the neighbour indices and the point's scalars; the rows of frequencies CGKLON(M,1:2) and CGKLAT(M,1:2) with their land cases
// (:602-654), the products OBSLON CGKLON and OBSLAT CGKLAT of the first call (:656-668), CGROUP and OMOSNH2KD of the point, and CGROUP of the 2 x 2 x 2
// rotated neighbours, a land neighbour replaced by the point itself (:766-785); the rows of directions CDR and SDR of the point and of those eight.
// Then a thread owns one 16-byte piece of consecutive frequencies of one (point, direction): it reads SDR(IJ,K) and CDR(IJ,K), selects the upwind side of
// each rotated axis by index (:701-712; no branch), issues the ten gathers of spectra, then rebuilds ACGKRLAT / ACGKRLON (:786-793) and forms the weights of
// its frequencies.  The piece the end of the advected range NFRE_RED cuts is computed and stored element by element.
// The arithmetic is the reference's, expression by expression in its order, without contraction and with correctly rounded divisions (the unit is not among
// the IMPLSCH sources of build.py): PROPAGS1 holds only + - * / and ABS, so the results are its bits.
#include "dev.h"
#include "launch.h"

namespace {

constexpr int PG1_TP = 4;          // points of a tile
constexpr int PG1_NI = 16;         // ints per point in LDS
constexpr int PG1_NS = 24;         // reals per point in LDS
constexpr int PG1_NPL = 18;        // rows of frequencies per point
constexpr int PG1_NDR = 18;        // rows of directions per point: CDR, then SDR, of the point and its eight rotated neighbours
// KLON(IJ,1:2), KLAT(IJ,1,1:2), KLAT(IJ,2,1:2), KRLAT(IJ,1,1:2), KRLAT(IJ,2,1:2), KRLON(IJ,1,1:2), KRLON(IJ,2,1:2): as the tables hold them (the gathers)
enum { QI_IJ = 0, QI_LON1, QI_LON2, QI_LAT11, QI_LAT12, QI_LAT21, QI_LAT22, QI_RLAT, QI_RLON = QI_RLAT + 4 };
enum { QS_DCO = 0, QS_WL1, QS_WL2, QS_WM1, QS_WM2, QS_TANPH, QS_DLADCO, QS_PRQRT, QS_DELPH0R, QS_WRLAT1, QS_WRLAT2, QS_WRLATM1, QS_WRLATM2, QS_WRLON1, QS_WRLON2,
       QS_WRLONM1, QS_WRLONM2 };
// rows of frequencies
enum { QR_CGKLON = 0, QR_CGKLAT = 2, QR_CG0 = 4, QR_OM = 5, QR_OBSLON = 6, QR_OBSLAT = 8, QR_CGR = 10 };

template <typename T, int VW>
struct Piece1 {
  typedef T V __attribute__((ext_vector_type(VW)));
  static __device__ __forceinline__ void ld(const T* p, T* o) {
    const V v = *reinterpret_cast<const V*>(p);
#pragma unroll
    for (int c = 0; c < VW; c++) o[c] = v[c];
  }
  static __device__ __forceinline__ void st(T* p, const T* o) {
    V v;
#pragma unroll
    for (int c = 0; c < VW; c++) v[c] = o[c];
    *reinterpret_cast<V*>(p) = v;
  }
};

template <typename T>
struct Propags1Args {
  const T *f1;
  T* f3;
  int nland, irefra;
  T delpro, delphi, sqrt2;
  const int* kxlt;
  const T *cosph, *sinph, *dellam1, *cosphm1;
  const int *klon, *klat, *krlat, *krlon;
  const T *wlat, *wrlat, *wrlon, *cdr, *sdr, *prqrt, *cg, *om, *dot, *obs;
  int kijs, kijl, copy_rest;
  T* cfl;
  int* cflfail;
};

#define PG1_ROW(t, p) (sR + ((size_t)(t) * PG1_NPL + (p)) * NFRE)
#define PG1_DIR(t, p) (sD + ((size_t)(t) * PG1_NDR + (p)) * NANG)

template <typename T, int VW>
__global__ void __launch_bounds__(256) k_propags1(const DevTab<T>* __restrict__ tab, const Propags1Args<T> a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char pg1_smem[];
  typedef Piece1<T, VW> IO;
  const int NANG = tab->NANG, NFRE = tab->NFRE, NR = tab->NFRE_RED;
  const int N = NANG * NFRE, FV = NFRE / VW, NV = NANG * FV;
  const int IREFRA = a.irefra, nland = a.nland;
  int* sI = reinterpret_cast<int*>(pg1_smem);                       // [TP][PG1_NI]
  T* sS = reinterpret_cast<T*>(sI + PG1_TP * PG1_NI);               // [TP][PG1_NS]
  T* sR = sS + PG1_TP * PG1_NS;                                     // [TP][PG1_NPL][NFRE]
  T* sD = sR + (size_t)PG1_TP * PG1_NPL * NFRE;                     // [TP][PG1_NDR][NANG]
  const T DELPRO = a.delpro, DELPHI = a.delphi;
  const T DELTH0 = T(0.25) * DELPRO / tab->DELTH;
  const T DELPH0 = T(0.5) * DELPRO / DELPHI;
  const T COFDELPH0R = T(0.5) * DELPRO / (a.sqrt2 * DELPHI);      // :572
  const int p0 = a.kijs + (int)blockIdx.x * PG1_TP;
  const int np = min(PG1_TP, a.kijl - p0);
  // ---- the point: indices and scalars (:198-222, 574-593)
  if ((int)threadIdx.x < np) {
    const int t = threadIdx.x, ij = p0 + t;
    int* q = sI + t * PG1_NI;
    q[QI_IJ] = ij;
    q[QI_LON1] = a.klon[ij * 2 + 0]; q[QI_LON2] = a.klon[ij * 2 + 1];
    q[QI_LAT11] = a.klat[ij * 4 + 0]; q[QI_LAT12] = a.klat[ij * 4 + 1]; q[QI_LAT21] = a.klat[ij * 4 + 2]; q[QI_LAT22] = a.klat[ij * 4 + 3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      q[QI_RLAT + i] = a.krlat[ij * 4 + i];
      q[QI_RLON + i] = a.krlon[ij * 4 + i];
    }
    q[15] = 0;
    T* s = sS + t * PG1_NS;
    const T DELLA0 = DELPRO * a.dellam1[ij];
    const T DCO = a.cosphm1[ij];
    const T PRQRT = a.prqrt[ij];
    s[QS_DCO] = DCO;
    const T w1 = a.wlat[ij * 2 + 0], w2 = a.wlat[ij * 2 + 1];
    s[QS_WL1] = w1; s[QS_WL2] = w2;
    s[QS_WM1] = T(1) - w1; s[QS_WM2] = T(1) - w2;
    const int JH = a.kxlt[ij];
    s[QS_TANPH] = a.sinph[JH] / a.cosph[JH];
    s[QS_DLADCO] = (T(1) - PRQRT) * (DCO * DELLA0);      // :581
    s[QS_PRQRT] = PRQRT;
    s[QS_DELPH0R] = PRQRT * COFDELPH0R;                  // :575; DELLA0R is the same number (:577)
    const T r1 = a.wrlat[ij * 2 + 0], r2 = a.wrlat[ij * 2 + 1], o1 = a.wrlon[ij * 2 + 0], o2 = a.wrlon[ij * 2 + 1];
    s[QS_WRLAT1] = r1; s[QS_WRLAT2] = r2; s[QS_WRLATM1] = T(1) - r1; s[QS_WRLATM2] = T(1) - r2;
    s[QS_WRLON1] = o1; s[QS_WRLON2] = o2; s[QS_WRLONM1] = T(1) - o1; s[QS_WRLONM2] = T(1) - o2;
  }
  __syncthreads();
  // ---- the rows of frequencies that all directions of a point share
  for (int it = threadIdx.x; it < np * NFRE; it += blockDim.x) {
    const int t = it / NFRE, m = it - t * NFRE;
    if (m >= NR) continue;
    const int* q = sI + t * PG1_NI;
    const T* s = sS + t * PG1_NS;
    const int ij = q[QI_IJ];
    const T cg0 = a.cg[(size_t)ij * NFRE + m];
    const T DCO = s[QS_DCO];
    const T* ob = a.obs ? a.obs + (size_t)ij * 8 * NFRE : nullptr;
#pragma unroll
    for (int ic = 0; ic < 2; ic++) {
      const int jl = q[QI_LON1 + ic];
      const T cgklon = jl != nland ? a.cg[(size_t)jl * NFRE + m] + cg0 : T(2) * cg0;      // :605-609
      PG1_ROW(t, QR_CGKLON + ic)[m] = cgklon;
      PG1_ROW(t, QR_OBSLON + ic)[m] = ob ? ob[(2 + ic) * NFRE + m] * cgklon : cgklon;      // :663
      const int j1 = q[QI_LAT11 + 2 * ic], j2 = q[QI_LAT12 + 2 * ic];
      const T DP = j1 == nland ? T(1) : DCO * (T(1) / a.cosphm1[j1]);                      // :204, 212-222
      const T W = s[QS_WL1 + ic], WM = s[QS_WM1 + ic];
      T cgklat;                                                                            // :616-652
      if (j1 == nland && j2 == nland) {
        cgklat = cg0 * (DP + T(1));
      } else if (j1 == nland) {
        const T c2 = a.cg[(size_t)j2 * NFRE + m];
        cgklat = cg0 + DP * (W * c2 + WM * c2);
      } else if (j2 == nland) {
        const T c1 = a.cg[(size_t)j1 * NFRE + m];
        cgklat = cg0 + DP * (W * c1 + WM * c1);
      } else {
        cgklat = cg0 + DP * (W * a.cg[(size_t)j1 * NFRE + m] + WM * a.cg[(size_t)j2 * NFRE + m]);
      }
      PG1_ROW(t, QR_CGKLAT + ic)[m] = cgklat;
      PG1_ROW(t, QR_OBSLAT + ic)[m] = ob ? ob[ic * NFRE + m] * cgklat : cgklat;            // :664
    }
    PG1_ROW(t, QR_CG0)[m] = cg0;
    PG1_ROW(t, QR_OM)[m] = IREFRA == 1 ? a.om[(size_t)ij * NFRE + m] : T(0);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int j = q[QI_RLAT + i];
      PG1_ROW(t, QR_CGR + i)[m] = j != nland ? a.cg[(size_t)j * NFRE + m] : cg0;
    }
  }
  // ---- the rows of directions: CDR, SDR of the point and of its rotated neighbours (land: the point itself)
  for (int it = threadIdx.x; it < np * NANG; it += blockDim.x) {
    const int t = it / NANG, k = it - t * NANG;
    const int* q = sI + t * PG1_NI;
    const int ij = q[QI_IJ];
    PG1_DIR(t, 0)[k] = a.cdr[(size_t)ij * NANG + k];
    PG1_DIR(t, 9)[k] = a.sdr[(size_t)ij * NANG + k];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      int j = q[QI_RLAT + i];
      j = j != nland ? j : ij;
      PG1_DIR(t, 1 + i)[k] = a.cdr[(size_t)j * NANG + k];
      PG1_DIR(t, 10 + i)[k] = a.sdr[(size_t)j * NANG + k];
    }
  }
  __syncthreads();
  // ---- the stencil: piece e of the tile is (point t, direction k, piece mv) with e = (t NANG + k) FV + mv
  for (int e = threadIdx.x; e < np * NV; e += blockDim.x) {
    const int t = e / NV, r = e - t * NV, k = r / FV, m = (r - k * FV) * VW;
    const int* q = sI + t * PG1_NI;
    const T* s = sS + t * PG1_NS;
    const int ij = q[QI_IJ];
    const size_t own = (size_t)ij * N + (size_t)k * NFRE + m;
    if (m >= NR) {      // no frequency of the piece is advected
      if (a.copy_rest && a.f3) {
        T v[VW];
        IO::ld(a.f1 + own, v);
        IO::st(a.f3 + own, v);
      }
      continue;
    }
    const bool check = m == 0;      // CHECKCFL at M = 1 (:867)
    const bool spectra = a.f3 != nullptr;
    if (!spectra && !check) continue;
    const int KP1 = k + 1 >= NANG ? 0 : k + 1, KM1 = k - 1 < 0 ? NANG - 1 : k - 1;
    const T SD = tab->SINTH[k], CD = tab->COSTH[k];
    const int ila = SD < T(0) ? 1 : 0, iph = CD < T(0) ? 1 : 0;      // IJLA - 1, IJPH - 1 (:682-691)
    // the speeds along the rotated axes, per unit group velocity: [0] the point, [1 + 2 ic + j] its neighbours
    T cdr[9], sdr[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      cdr[i] = PG1_DIR(t, i)[k];
      sdr[i] = PG1_DIR(t, 9 + i)[k];
    }
    const int irla = sdr[0] < T(0) ? 1 : 0, irph = cdr[0] < T(0) ? 1 : 0;      // IJRLA - 1, IJRPH - 1 (:701-712), per point and direction
    // ---- every gather of spectra, before its first use
    T fo[VW], fkp[VW], fkm[VW], g0[VW], g1[VW], g4[VW], r0[VW], r1[VW], r2[VW], r3[VW];
#pragma unroll
    for (int c = 0; c < VW; c++) fo[c] = fkp[c] = fkm[c] = g0[c] = g1[c] = g4[c] = r0[c] = r1[c] = r2[c] = r3[c] = T(0);
    if (spectra) {
      const size_t el = (size_t)k * NFRE + m;
      IO::ld(a.f1 + own, fo);
      IO::ld(a.f1 + (size_t)q[QI_LAT11 + 2 * iph] * N + el, g0);
      IO::ld(a.f1 + (size_t)q[QI_LAT12 + 2 * iph] * N + el, g1);
      IO::ld(a.f1 + (size_t)q[QI_LON1 + ila] * N + el, g4);
      IO::ld(a.f1 + (size_t)q[QI_RLAT + 2 * irph] * N + el, r0);
      IO::ld(a.f1 + (size_t)q[QI_RLAT + 2 * irph + 1] * N + el, r1);
      IO::ld(a.f1 + (size_t)q[QI_RLON + 2 * irla] * N + el, r2);
      IO::ld(a.f1 + (size_t)q[QI_RLON + 2 * irla + 1] * N + el, r3);
      IO::ld(a.f1 + (size_t)ij * N + (size_t)KP1 * NFRE + m, fkp);
      IO::ld(a.f1 + (size_t)ij * N + (size_t)KM1 * NFRE + m, fkm);
    }
    // ---- what depends on the direction and not on the frequency
    const T* dt = a.dot ? a.dot + (size_t)ij * ECWAM_HIP_PROPAGS_DOT_W(NANG) : nullptr;
    T DRDP = T(0), DRDM = T(0);
    if (IREFRA != 0) {
      DRDP = (dt[k] + dt[KP1]) * DELTH0;
      DRDM = (dt[k] + dt[KM1]) * DELTH0;
    }
    const T SP = DELTH0 * (SD + tab->SINTH[KP1]) / tab->R;
    const T SM = DELTH0 * (SD + tab->SINTH[KM1]) / tab->R;
    const T DRGP = s[QS_TANPH] * SP, DRGM = s[QS_TANPH] * SM;
    const T PRQRT = s[QS_PRQRT];
    const T SDA2 = T(0.5) * m_abs(SD);
    const T DELPH0_CDA = (T(1) - PRQRT) * DELPH0 * m_abs(CD);      // :697
    const T SDDL = SDA2 * s[QS_DLADCO];                              // :698
    const T XXR = s[QS_DCO] * s[QS_DELPH0R];                         // :800, :812: DCO DELLA0R = DCO DELPH0R
    const T* ob = a.obs ? a.obs + (size_t)ij * 8 * NFRE : nullptr;      // planes 4-5 OBSRLAT(:,:,1:2), 6-7 OBSRLON(:,:,1:2), applied as they are
    T res[VW], cf[11];
#pragma unroll
    for (int c = 0; c < VW; c++) {
      const int M = m + c;
      if (M >= NR) { res[c] = fo[c]; continue; }
      if (!spectra && c > 0) { res[c] = T(0); continue; }
      // :745-759
      T CFLEA = SDDL * PG1_ROW(t, QR_CGKLON + 1 - ila)[M];
      T DTC = CFLEA;
      const T DLE = SDDL * PG1_ROW(t, QR_OBSLON + ila)[M];
      T CFLNO = DELPH0_CDA * PG1_ROW(t, QR_CGKLAT + 1 - iph)[M];
      DTC = DTC + CFLNO;
      T XX = DELPH0_CDA * PG1_ROW(t, QR_OBSLAT + iph)[M];
      const T DPN = s[QS_WL1 + iph] * XX;
      const T DPN2 = s[QS_WM1 + iph] * XX;
      // :764-795
      const T cg0 = PG1_ROW(t, QR_CG0)[M];
      T ACGKRLAT[2], ACGKRLON[2];
#pragma unroll
      for (int ic = 0; ic < 2; ic++) {
        const T ca1 = PG1_ROW(t, QR_CGR + 2 * ic)[M], ca2 = PG1_ROW(t, QR_CGR + 2 * ic + 1)[M];
        const T co1 = PG1_ROW(t, QR_CGR + 4 + 2 * ic)[M], co2 = PG1_ROW(t, QR_CGR + 4 + 2 * ic + 1)[M];
        const T la = cg0 * cdr[0] + s[QS_WRLAT1 + ic] * ca1 * cdr[1 + 2 * ic] + s[QS_WRLATM1 + ic] * ca2 * cdr[2 + 2 * ic];
        const T lo = cg0 * sdr[0] + s[QS_WRLON1 + ic] * co1 * sdr[5 + 2 * ic] + s[QS_WRLONM1 + ic] * co2 * sdr[6 + 2 * ic];
        ACGKRLAT[ic] = m_abs(la);
        ACGKRLON[ic] = m_abs(lo);
      }
      // :797-819
      const T CFLEAR = XXR * (irla ? ACGKRLON[0] : ACGKRLON[1]);
      DTC = DTC + CFLEAR;
      T FF = XXR * (irla ? ACGKRLON[1] : ACGKRLON[0]);
      FF = FF * (ob ? ob[(6 + irla) * NFRE + M] : T(1));
      const T RLE = s[QS_WRLON1 + irla] * FF;
      const T RLE2 = s[QS_WRLONM1 + irla] * FF;
      const T CFLNOR = XXR * (irph ? ACGKRLAT[0] : ACGKRLAT[1]);
      DTC = DTC + CFLNOR;
      FF = XXR * (irph ? ACGKRLAT[1] : ACGKRLAT[0]);
      FF = FF * (ob ? ob[(4 + irph) * NFRE + M] : T(1));
      const T RPN = s[QS_WRLAT1 + irph] * FF;
      const T RPN2 = s[QS_WRLATM1 + irph] * FF;
      // :824-844
      T DTHP, DTHM;
      if (IREFRA == 0) {
        DTHP = DRGP * cg0;
        DTHM = DRGM * cg0;
      } else {
        const T OM = PG1_ROW(t, QR_OM)[M];
        DTHP = DRGP * cg0 + OM * DRDP;
        DTHM = DRGM * cg0 + OM * DRDM;
      }
      const T CFLTP = DTHP + m_abs(DTHP);
      const T CFLTM = -DTHM + m_abs(DTHM);
      DTC = DTC + CFLTP + CFLTM;
      const T DTP = -DTHP + m_abs(DTHP);
      const T DTM = DTHM + m_abs(DTHM);
      // :850-863
      res[c] = (T(1) - DTC) * fo[c] + DPN * g0[c] + DPN2 * g1[c] + DLE * g4[c] + RPN * r0[c] + RPN2 * r1[c] + RLE * r2[c] + RLE2 * r3[c] + DTP * fkp[c]
               + DTM * fkm[c];
      if (M == 0) {      // :867-878: the unrotated numbers rescaled, a DTC of them alone
        const T CGOMFULL = T(1) / (T(1) - PRQRT);
        CFLEA = CFLEA * CGOMFULL;
        CFLNO = CFLNO * CGOMFULL;
        DTC = CFLEA + CFLNO + CFLTP + CFLTM;
        cf[0] = DTC; cf[1] = CFLEA; cf[2] = CFLEA; cf[3] = CFLNO; cf[4] = CFLNO; cf[5] = CFLNO; cf[6] = CFLNO; cf[7] = CFLTP; cf[8] = CFLTM;
        cf[9] = CFLTP; cf[10] = CFLTM;
      }
    }
    if (check) {
      bool bad = false;
#pragma unroll
      for (int i = 0; i < 11; i++) bad = bad || cf[i] > T(1);
      if (bad && a.cflfail) a.cflfail[ij] = 1;
      if (a.cfl) {
        T* o = a.cfl + ((size_t)ij * NANG + k) * 11;
#pragma unroll
        for (int i = 0; i < 11; i++) o[i] = cf[i];
      }
    }
    if (spectra) {
      if (m + VW <= NR) {
        IO::st(a.f3 + own, res);
      } else {      // the piece the end of the range cuts: element by element
#pragma unroll
        for (int c = 0; c < VW; c++)
          if (m + c < NR || a.copy_rest) a.f3[own + c] = res[c];
      }
    }
  }
}
#undef PG1_ROW
#undef PG1_DIR

template <typename T>
size_t propags1_lds(int NANG, int NFRE) {
  return (size_t)PG1_TP * PG1_NI * sizeof(int) + (size_t)PG1_TP * (PG1_NS + (size_t)PG1_NPL * NFRE + (size_t)PG1_NDR * NANG) * sizeof(T);
}

}  // namespace

template <typename T>
int launch_propags1(const void* tab, const PropagsCall& c, const RotatedTables& r, int NANG, int NFRE, hipStream_t s) {
  constexpr int VW = 16 / (int)sizeof(T);
  if (c.kijl <= c.kijs) return 0;
  const size_t lds = propags1_lds<T>(NANG, NFRE);
  if (lds > 64 * 1024) return 1;
  Propags1Args<T> a;
  a.f1 = (const T*)c.f1; a.f3 = (T*)c.f3;
  a.nland = c.nland; a.irefra = c.irefra;
  a.delpro = (T)c.delpro; a.delphi = (T)c.delphi; a.sqrt2 = (T)r.sqrt2;
  a.kxlt = c.kxlt;
  a.cosph = (const T*)c.cosph; a.sinph = (const T*)c.sinph; a.dellam1 = (const T*)c.dellam1; a.cosphm1 = (const T*)c.cosphm1;
  a.klon = c.klon; a.klat = c.klat; a.krlat = r.krlat; a.krlon = r.krlon;
  a.wlat = (const T*)c.wlat; a.wrlat = (const T*)r.wrlat; a.wrlon = (const T*)r.wrlon; a.cdr = (const T*)r.cdr; a.sdr = (const T*)r.sdr;
  a.prqrt = (const T*)r.prqrt; a.cg = (const T*)c.cg; a.om = (const T*)c.om; a.dot = (const T*)c.dot; a.obs = (const T*)c.obs;
  a.kijs = c.kijs; a.kijl = c.kijl; a.copy_rest = c.copy_rest;
  a.cfl = (T*)c.cfl; a.cflfail = c.cflfail;
  const dim3 grid((c.kijl - c.kijs + PG1_TP - 1) / PG1_TP), block(256);
  hipLaunchKernelGGL((k_propags1<T, VW>), grid, block, lds, s, (const DevTab<T>*)tab, a);
  return 0;
}

template int launch_propags1<float>(const void*, const PropagsCall&, const RotatedTables&, int, int, hipStream_t);
template int launch_propags1<double>(const void*, const PropagsCall&, const RotatedTables&, int, int, hipStream_t);
