// First-order upwind propagation, IPROPAGS = 0 (include/ecwam_hip_propags.h).
//   k_propags_dot   GRADI + PROPDOT (gradi.F90:113-232, propdot.F90:109-198) statement by statement, ICASE 1 and 2: one thread per point writes the row
//                   DOT[ij][3 NANG + 4] = THDD(K), THDC(K), S0(K) (the SDOT(IJ,K,NFRE_RED) of propdot.F90:178 before the frequency loop), OMDD, three reals of padding
//   k_propags       PROPAGS (propags.F90:10-998), one build per section: 1 Cartesian IREFRA 0/1, 2 Cartesian IREFRA 2/3, 3 spherical IREFRA 0/1, 4 spherical
//                   IREFRA 2/3 (IRGG 0 and 1), with CHECKCFL (checkcfl.F90:74-247) as the spherical sections call it at M = 1
// k_propags: the layout FL[row][K][NFRE] and the access pattern of k_propags2_otf (propag.hip).  A block takes a tile of PG_TP points.  What does not depend on
// the direction is formed once per point and goes to LDS: the neighbour indices and the point's scalars; in section 3 the midpoint velocities CGKLON(M,1:2) and
// CGKLAT(M,1:2); in sections 2 and 4 the CGROUP rows and U, V of the point and of its 2 + 4 space neighbours; in every section that reads them the point's
// OMOSNH2KD and WAVNUM rows.  Then a thread owns one 16-byte piece of consecutive frequencies of one (point, direction): it issues every gather of neighbour
// spectra, then forms the weights of its frequencies and applies the stencil.  The piece the end of the advected range NFRE_RED cuts is computed and stored
// element by element; MP1 = MIN(NFRE_RED, M+1) and MM1 = MAX(1, M-1) clamp inside it.
// The arithmetic is the reference's, expression by expression in its order, without contraction and with correctly rounded divisions (the unit is not among
// the IMPLSCH sources of build.py): the reference holds only + - * / and ABS here, so the results are its bits.  SDOT(IJ,K,M) is not stored: it is rebuilt as
// (S0(K) CGROUP(M) + OMDD OMOSNH2KD(M)) WAVNUM(M), the expression of propdot.F90:190-191.
#include "../../include/ecwam_hip_propags.h"
#include "dev.h"
#include "launch.h"

namespace {

constexpr int PG_TP = 8;          // points of a tile
constexpr int PG_NS = 12;         // reals per point in LDS
enum { PS_DELLA0 = 0, PS_DCO, PS_DP1, PS_DP2, PS_WL1, PS_WL2, PS_WM1, PS_WM2, PS_TANPH, PS_DLADCO, PS_DELLA0_NINF };
enum { PI_IJ = 0, PI_LON1, PI_LON2, PI_LAT11, PI_LAT12, PI_LAT21, PI_LAT22, PI_N };      // KLON(IJ,1:2), KLAT(IJ,1,1:2), KLAT(IJ,2,1:2)

template <typename T, int VW>
struct Piece {
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

// gradi.F90:113-232 + propdot.F90:109-198, one thread per point
template <typename T>
__global__ void __launch_bounds__(256) k_propags_dot(const DevTab<T>* __restrict__ tab, int n, int nland, int IREFRA, int ICASE, const int* __restrict__ kxlt,
                                                     const T* __restrict__ zdello, T xdella, const T* __restrict__ cosph, const int* __restrict__ klon,
                                                     const int* __restrict__ klat, const T* __restrict__ wlat, const T* __restrict__ cosphm1,
                                                     const T* __restrict__ depth, const T* __restrict__ ue, const T* __restrict__ ve, T* __restrict__ dot) {
#pragma clang fp contract(off)
  const int ij = blockIdx.x * blockDim.x + threadIdx.x;
  if (ij >= n) return;
  const int NANG = tab->NANG;
  const T CGM = T(0.00001);      // CURRENT_GRADIENT_MAX, yowcurr.F90:19
  const T DELPHI = xdella * tab->CIRC / T(360.0);      // readmdlconf.F90:136
  const T ONEO2DELPHI = T(0.5) / DELPHI;
  const int KX = kxlt[ij];
  const T DELLAM = zdello[KX] * tab->CIRC / T(360.0);      // readmdlconf.F90:145
  T DDPHI = T(0), DDLAM = T(0), DUPHI = T(0), DULAM = T(0), DVPHI = T(0), DVLAM = T(0);
  const T wl1 = wlat[ij * 2 + 0], wl2 = wlat[ij * 2 + 1];
  if (IREFRA == 1 || IREFRA == 3) {
    const int IPP = klat[ij * 4 + 2], IPM = klat[ij * 4 + 0], IPP2 = klat[ij * 4 + 3], IPM2 = klat[ij * 4 + 1];
    if (IPP != nland && IPM != nland && IPP2 != nland && IPM2 != nland) {
      const T DPTP = wl2 * depth[IPP] + (T(1) - wl2) * depth[IPP2];
      const T DPTM = wl1 * depth[IPM] + (T(1) - wl1) * depth[IPM2];
      DDPHI = (DPTP - DPTM) * ONEO2DELPHI;
    } else if (IPP != nland && IPM != nland) {
      DDPHI = (depth[IPP] - depth[IPM]) * ONEO2DELPHI;
    } else if (IPP2 != nland && IPM2 != nland) {
      DDPHI = (depth[IPP2] - depth[IPM2]) * ONEO2DELPHI;
    }
    const int ILP = klon[ij * 2 + 1], ILM = klon[ij * 2 + 0];
    if (ILP != nland && ILM != nland) DDLAM = (depth[ILP] - depth[ILM]) / (T(2) * DELLAM);
  }
  if (IREFRA == 2 || IREFRA == 3) {
    int IPP = klat[ij * 4 + 2], IPM = klat[ij * 4 + 0], IPP2 = klat[ij * 4 + 3], IPM2 = klat[ij * 4 + 1];
    // an exact zero means "current not defined there": no gradient is extrapolated (gradi.F90:170-180)
    if (ue[IPP] == T(0) && ve[IPP] == T(0)) IPP = nland;
    if (ue[IPM] == T(0) && ve[IPM] == T(0)) IPM = nland;
    if (ue[IPP2] == T(0) && ve[IPP2] == T(0)) IPP2 = nland;
    if (ue[IPM2] == T(0) && ve[IPM2] == T(0)) IPM2 = nland;
    if (IPP != nland && IPM != nland && IPP2 != nland && IPM2 != nland) {
      const T UP = wl2 * ue[IPP] + (T(1) - wl2) * ue[IPP2];
      const T VP = wl2 * ve[IPP] + (T(1) - wl2) * ve[IPP2];
      const T UM = wl1 * ue[IPM] + (T(1) - wl1) * ue[IPM2];
      const T VM = wl1 * ve[IPM] + (T(1) - wl1) * ve[IPM2];
      DUPHI = (UP - UM) * ONEO2DELPHI;
      DVPHI = (VP - VM) * ONEO2DELPHI;
    } else if (IPP != nland && IPM != nland) {
      DUPHI = (ue[IPP] - ue[IPM]) * ONEO2DELPHI;
      DVPHI = (ve[IPP] - ve[IPM]) * ONEO2DELPHI;
    }
    int ILP = klon[ij * 2 + 1], ILM = klon[ij * 2 + 0];
    if (ue[ILP] == T(0) && ve[ILP] == T(0)) ILP = nland;
    if (ue[ILM] == T(0) && ve[ILM] == T(0)) ILM = nland;
    if (ILP != nland && ILM != nland) {
      DULAM = (ue[ILP] - ue[ILM]) / (T(2) * DELLAM);
      DVLAM = (ve[ILP] - ve[ILM]) / (T(2) * DELLAM);
    }
    const T CGMAX = CGM * cosph[KX];
    DUPHI = m_sign(m_min(m_abs(DUPHI), CGMAX), DUPHI);
    DVPHI = m_sign(m_min(m_abs(DVPHI), CGMAX), DVPHI);
    DULAM = m_sign(m_min(m_abs(DULAM), CGMAX), DULAM);
    DVLAM = m_sign(m_min(m_abs(DVLAM), CGMAX), DVLAM);
  }
  const T DCO = ICASE == 1 ? cosphm1[ij] : T(1);
  T* o = dot + (size_t)ij * ECWAM_HIP_PROPAGS_DOT_W(NANG);
  o[3 * NANG] = IREFRA == 3 ? ve[ij] * DDPHI + ue[ij] * DDLAM * DCO : T(0);
  o[3 * NANG + 1] = T(0);
  o[3 * NANG + 2] = T(0);
  o[3 * NANG + 3] = T(0);
  for (int k = 0; k < NANG; k++) {
    const T SD = tab->SINTH[k], CD = tab->COSTH[k];
    T thdd = T(0), thdc = T(0), s0 = T(0);
    if (IREFRA == 1 || IREFRA == 3) thdd = SD * DDPHI - CD * DDLAM * DCO;
    if (IREFRA == 2 || IREFRA == 3) {
      const T SS = SD * SD, SC = SD * CD, CC = CD * CD;
      s0 = -SC * DUPHI - CC * DVPHI - (SS * DULAM + SC * DVLAM) * DCO;
      thdc = SS * DUPHI + SC * DVPHI - (SC * DULAM + CC * DVLAM) * DCO;
    }
    o[k] = thdd;
    o[NANG + k] = thdc;
    o[2 * NANG + k] = s0;
  }
}

template <typename T>
struct PropagsArgs {
  const T *f1;
  T* f3;
  int nland, irefra, irgg;
  T delpro, delphi;
  const int* kxlt;
  const T *cosph, *sinph, *dellam1, *cosphm1;
  const int *klon, *klat;
  const T *wlat, *cg, *om, *wn, *u, *v, *dot, *obs;
  int kijs, kijl, copy_rest;
  T* cfl;
  int* cflfail;
};

// the plane p of point t in the tile's LDS table of rows of frequencies
#define PG_ROW(t, p) (sR + ((size_t)(t) * NPL + (p)) * NFRE)

// DPP (section 4 alone): DP1, DP2 as the product DCO(IJ) * (1 / DCO(JH)) of propags1.F90:203-222; the default is the quotient of propags.F90:217-224
template <typename T, int VW, int SEC, bool DPP = false>
__global__ void __launch_bounds__(256) k_propags(const DevTab<T>* __restrict__ tab, const PropagsArgs<T> a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char pg_smem[];
  typedef Piece<T, VW> IO;
  constexpr bool SPH = SEC >= 3, CUR = SEC == 2 || SEC == 4;
  // planes of rows of frequencies per point.  Section 3: CGKLON(:,1:2), CGKLAT(:,1:2), CGROUP, OMOSNH2KD.  Section 1: CGROUP of the point and of KLON(1:2),
  // KLAT(1:2,1), OMOSNH2KD.  Sections 2, 4: CGROUP of the point, KLON(1:2), KLAT(1,1:2), KLAT(2,1:2), then OMOSNH2KD, WAVNUM.
  constexpr int NPL = CUR ? 9 : 6;
  const int NANG = tab->NANG, NFRE = tab->NFRE, NR = tab->NFRE_RED;
  const int N = NANG * NFRE, FV = NFRE / VW, NV = NANG * FV;
  const int IREFRA = a.irefra, nland = a.nland;
  int* sI = reinterpret_cast<int*>(pg_smem);                        // [TP][8]
  T* sS = reinterpret_cast<T*>(sI + PG_TP * 8);                     // [TP][PG_NS]
  T* sU = sS + PG_TP * PG_NS;                                       // [TP][7][2]: U, V of the point and its neighbours in the order of PI_*
  T* sR = sU + PG_TP * 14;                                          // [TP][NPL][NFRE]
  const T DELPRO = a.delpro, DELPHI = a.delphi, FRATIO = tab->FRATIO;
  const T DELTH0 = T(0.25) * DELPRO / tab->DELTH;
  const T DELPH0 = SEC == 1 ? DELPRO / DELPHI : SEC == 3 ? T(0.5) * DELPRO / DELPHI : T(0.25) * DELPRO / DELPHI;
  const T DELFR0 = T(0.25) * DELPRO / ((FRATIO - T(1)) * tab->ZPI);
  const int p0 = a.kijs + (int)blockIdx.x * PG_TP;
  const int np = min(PG_TP, a.kijl - p0);
  // ---- the point: indices and scalars (propags.F90:164-226, 528-533, 577-579, 601-606)
  if ((int)threadIdx.x < np) {
    const int t = threadIdx.x, ij = p0 + t;
    int* q = sI + t * 8;
    q[PI_IJ] = ij;
    q[PI_LON1] = a.klon[ij * 2 + 0]; q[PI_LON2] = a.klon[ij * 2 + 1];
    q[PI_LAT11] = a.klat[ij * 4 + 0]; q[PI_LAT12] = a.klat[ij * 4 + 1]; q[PI_LAT21] = a.klat[ij * 4 + 2]; q[PI_LAT22] = a.klat[ij * 4 + 3];
    T* s = sS + t * PG_NS;
    T DELLA0 = DELPRO * a.dellam1[ij];
    T DELLA0_NINF = DELPRO * a.dellam1[0];
    if (SPH) {
      const T DCO = a.cosphm1[ij];
      const int j1 = q[PI_LAT11], j2 = q[PI_LAT21];
      s[PS_DCO] = DCO;
      if (DPP) {
        s[PS_DP1] = j1 == nland ? T(1) : DCO * (T(1) / a.cosphm1[j1]);
        s[PS_DP2] = j2 == nland ? T(1) : DCO * (T(1) / a.cosphm1[j2]);
      } else {
        s[PS_DP1] = j1 == nland ? T(1) : DCO / a.cosphm1[j1];
        s[PS_DP2] = j2 == nland ? T(1) : DCO / a.cosphm1[j2];
      }
      const T w1 = a.wlat[ij * 2 + 0], w2 = a.wlat[ij * 2 + 1];
      s[PS_WL1] = w1; s[PS_WL2] = w2;
      s[PS_WM1] = T(1) - w1; s[PS_WM2] = T(1) - w2;
      const int JH = a.kxlt[ij];
      s[PS_TANPH] = a.sinph[JH] / a.cosph[JH];
      s[PS_DLADCO] = DCO * DELLA0;      // section 3, with the DELLA0 of :178
    }
    if (CUR) {      // DELLA0 = 0.25 DELLA0 (:386, :793)
      DELLA0 = T(0.25) * DELLA0;
      DELLA0_NINF = T(0.25) * DELLA0_NINF;
    }
    s[PS_DELLA0] = DELLA0;
    s[PS_DELLA0_NINF] = DELLA0_NINF;
    if (CUR) {
#pragma unroll
      for (int i = 0; i < PI_N; i++) {
        sU[(t * 7 + i) * 2] = a.u[q[i]];
        sU[(t * 7 + i) * 2 + 1] = a.v[q[i]];
      }
    }
  }
  __syncthreads();
  // ---- the rows of frequencies that all directions of a point share
  for (int it = threadIdx.x; it < np * NFRE; it += blockDim.x) {
    const int t = it / NFRE, m = it - t * NFRE;
    if (m >= NR) continue;
    const int* q = sI + t * 8;
    const T* s = sS + t * PG_NS;
    const T cg0 = a.cg[(size_t)q[PI_IJ] * NFRE + m];
    if (SEC == 3) {
      const T c1 = a.cg[(size_t)q[PI_LON1] * NFRE + m], c2 = a.cg[(size_t)q[PI_LON2] * NFRE + m];
      const T a11 = a.cg[(size_t)q[PI_LAT11] * NFRE + m], a12 = a.cg[(size_t)q[PI_LAT12] * NFRE + m];
      const T a21 = a.cg[(size_t)q[PI_LAT21] * NFRE + m], a22 = a.cg[(size_t)q[PI_LAT22] * NFRE + m];
      PG_ROW(t, 0)[m] = c1 + cg0;                                                         // CGKLON(IJ,M,1), :541
      PG_ROW(t, 1)[m] = c2 + cg0;
      PG_ROW(t, 2)[m] = cg0 + s[PS_DP1] * (s[PS_WL1] * a11 + s[PS_WM1] * a12);            // CGKLAT(IJ,M,1), :548-550
      PG_ROW(t, 3)[m] = cg0 + s[PS_DP2] * (s[PS_WL2] * a21 + s[PS_WM2] * a22);            // CGKLAT(IJ,M,2), :556-558
      PG_ROW(t, 4)[m] = cg0;
      PG_ROW(t, 5)[m] = IREFRA == 1 ? a.om[(size_t)q[PI_IJ] * NFRE + m] : T(0);
    } else if (SEC == 1) {
      PG_ROW(t, 0)[m] = cg0;
      PG_ROW(t, 1)[m] = a.cg[(size_t)q[PI_LON1] * NFRE + m];
      PG_ROW(t, 2)[m] = a.cg[(size_t)q[PI_LON2] * NFRE + m];
      PG_ROW(t, 3)[m] = a.cg[(size_t)q[PI_LAT11] * NFRE + m];
      PG_ROW(t, 4)[m] = a.cg[(size_t)q[PI_LAT21] * NFRE + m];
      PG_ROW(t, 5)[m] = IREFRA == 1 ? a.om[(size_t)q[PI_IJ] * NFRE + m] : T(0);
    } else {
#pragma unroll
      for (int i = 0; i < PI_N; i++) PG_ROW(t, i)[m] = a.cg[(size_t)q[i] * NFRE + m];
      PG_ROW(t, 7)[m] = a.om[(size_t)q[PI_IJ] * NFRE + m];
      PG_ROW(t, 8)[m] = a.wn[(size_t)q[PI_IJ] * NFRE + m];
    }
  }
  __syncthreads();
  // ---- the stencil: piece e of the tile is (point t, direction k, piece mv) with e = (t NANG + k) FV + mv
  for (int e = threadIdx.x; e < np * NV; e += blockDim.x) {
    const int t = e / NV, r = e - t * NV, k = r / FV, m = (r - k * FV) * VW;
    const int* q = sI + t * 8;
    const T* s = sS + t * PG_NS;
    const int ij = q[PI_IJ];
    const size_t own = (size_t)ij * N + (size_t)k * NFRE + m;
    if (m >= NR) {      // no frequency of the piece is advected
      if (a.copy_rest && a.f3) {
        T v[VW];
        IO::ld(a.f1 + own, v);
        IO::st(a.f3 + own, v);
      }
      continue;
    }
    const bool check = SPH && m == 0;      // CHECKCFL at M = 1 (:718, :924)
    const bool spectra = a.f3 != nullptr;
    if (!spectra && !check) continue;
    const int KP1 = k + 1 >= NANG ? 0 : k + 1, KM1 = k - 1 < 0 ? NANG - 1 : k - 1;
    const T SD = tab->SINTH[k], CD = tab->COSTH[k];
    // the neighbours of the direction's quadrant (:252-261, :611-620)
    const int IJLA = SD < T(0) ? 2 : 1, IJPH = CD < T(0) ? 2 : 1;
    // ---- every gather of spectra, before its first use
    T fo[VW], fkp[VW], fkm[VW], g0[VW], g1[VW], g2[VW], g3[VW], g4[VW], g5[VW];
    T fmm = T(0), fmp = T(0);      // F1(IJ,K,m-1) and F1(IJ,K,m+VW), clamped to the advected range
#pragma unroll
    for (int c = 0; c < VW; c++) fo[c] = fkp[c] = fkm[c] = g0[c] = g1[c] = g2[c] = g3[c] = g4[c] = g5[c] = T(0);
    if (spectra) {
      const size_t el = (size_t)k * NFRE + m;
      IO::ld(a.f1 + own, fo);
      if (CUR) {
        IO::ld(a.f1 + (size_t)q[PI_LAT21] * N + el, g0);
        IO::ld(a.f1 + (size_t)q[PI_LAT11] * N + el, g2);
        IO::ld(a.f1 + (size_t)q[PI_LON2] * N + el, g4);
        IO::ld(a.f1 + (size_t)q[PI_LON1] * N + el, g5);
        if (SEC == 4 && a.irgg == 1) {
          IO::ld(a.f1 + (size_t)q[PI_LAT22] * N + el, g1);
          IO::ld(a.f1 + (size_t)q[PI_LAT12] * N + el, g3);
        }
        fmm = a.f1[own - (m > 0 ? 1 : 0)];
        fmp = a.f1[(size_t)ij * N + (size_t)k * NFRE + min(NR - 1, m + VW)];
      } else {
        IO::ld(a.f1 + (size_t)q[IJPH == 1 ? PI_LAT11 : PI_LAT21] * N + el, g0);
        if (SEC == 3) IO::ld(a.f1 + (size_t)q[IJPH == 1 ? PI_LAT12 : PI_LAT22] * N + el, g1);
        IO::ld(a.f1 + (size_t)q[IJLA == 1 ? PI_LON1 : PI_LON2] * N + el, g4);
      }
      if (SPH || IREFRA != 0) {
        IO::ld(a.f1 + (size_t)ij * N + (size_t)KP1 * NFRE + m, fkp);
        IO::ld(a.f1 + (size_t)ij * N + (size_t)KM1 * NFRE + m, fkm);
      }
    }
    // ---- what depends on the direction and not on the frequency
    const T* dt = a.dot ? a.dot + (size_t)ij * ECWAM_HIP_PROPAGS_DOT_W(NANG) : nullptr;
    T DRDP = T(0), DRDM = T(0), DRCP = T(0), DRCM = T(0), DRGP = T(0), DRGM = T(0), S0 = T(0), OMDD = T(0);
    if (IREFRA != 0) {
      DRDP = (dt[k] + dt[KP1]) * DELTH0;
      DRDM = (dt[k] + dt[KM1]) * DELTH0;
    }
    if (CUR) {
      DRCP = (dt[NANG + k] + dt[NANG + KP1]) * DELTH0;
      DRCM = (dt[NANG + k] + dt[NANG + KM1]) * DELTH0;
      S0 = dt[2 * NANG + k];
      OMDD = dt[3 * NANG];
    }
    if (SPH) {
      const T SP = DELTH0 * (SD + tab->SINTH[KP1]) / tab->R;
      const T SM = DELTH0 * (SD + tab->SINTH[KM1]) / tab->R;
      DRGP = s[PS_TANPH] * SP;
      DRGM = s[PS_TANPH] * SM;
    }
    const T* ob = a.obs ? a.obs + (size_t)ij * 8 * NFRE : nullptr;      // OBS[ij][8][NFRE]: OBSLAT(:,:,1:2), OBSLON(:,:,1:2), then the corners
    T res[VW], cf[11];
#pragma unroll
    for (int c = 0; c < VW; c++) {
      const int M = m + c;
      if (M >= NR) { res[c] = fo[c]; continue; }
      if (!spectra && c > 0) { res[c] = T(0); continue; }
      T F3;
      if (SEC == 1) {
        const T sd = T(0.5) * SD, cd = T(0.5) * CD;
        const T cg0 = PG_ROW(t, 0)[M];
        const T SDD = sd * s[PS_DELLA0];
        T DLA, DTC;
        if (sd >= T(0)) {
          DLA = SDD * (PG_ROW(t, 1)[M] + cg0);
          DTC = SDD * (PG_ROW(t, 2)[M] + cg0);
        } else {
          DLA = -SDD * (PG_ROW(t, 2)[M] + cg0);
          DTC = -SDD * (PG_ROW(t, 1)[M] + cg0);
        }
        const T CDD = cd * DELPH0;
        T DPH;
        if (cd >= T(0)) {
          DPH = CDD * (PG_ROW(t, 3)[M] + cg0);
          DTC = DTC + CDD * (PG_ROW(t, 4)[M] + cg0);
        } else {
          DPH = -CDD * (PG_ROW(t, 4)[M] + cg0);
          DTC = DTC - CDD * (PG_ROW(t, 3)[M] + cg0);
        }
        T DTP = T(0), DTM = T(0);
        if (IREFRA == 1) {
          const T OM = PG_ROW(t, 5)[M];
          const T DTHP = OM * DRDP, DTHM = OM * DRDM;
          DTC = DTC + DTHP + m_abs(DTHP) - DTHM + m_abs(DTHM);
          DTP = -DTHP + m_abs(DTHP);
          DTM = DTHM + m_abs(DTHM);
        }
        F3 = (T(1) - DTC) * fo[c] + DPH * g0[c] + DLA * g4[c];
        if (IREFRA == 1) F3 = F3 + DTP * fkp[c] + DTM * fkm[c];
      } else if (SEC == 3) {
        const T SDA2 = T(0.5) * m_abs(SD), DELPH0_CDA = DELPH0 * m_abs(CD);
        const T cgk_e = PG_ROW(t, SD > T(0) ? 1 : 0)[M], cgk_o = PG_ROW(t, SD > T(0) ? 0 : 1)[M];      // CGKLON(IJ,M,2 | 1), the one OBSLON goes with
        T XX = SDA2 * s[PS_DLADCO];
        const T CFLEA = XX * cgk_e;
        T DTC = CFLEA;
        // OBSLON(IJ,M,IC) holds OBSLON CGKLON after the first call (:570): the product first, then XX (...)
        const T oblon = ob ? ob[(SD > T(0) ? 2 : 3) * NFRE + M] * cgk_o : cgk_o;
        const T DLE = XX * oblon;
        const T cgl_n = PG_ROW(t, CD > T(0) ? 3 : 2)[M], cgl_o = PG_ROW(t, CD > T(0) ? 2 : 3)[M];
        const T CFLNO = DELPH0_CDA * cgl_n;
        DTC = DTC + CFLNO;
        const T oblat = ob ? ob[(CD > T(0) ? 0 : 1) * NFRE + M] * cgl_o : cgl_o;
        XX = DELPH0_CDA * oblat;
        const T DPN = (CD > T(0) ? s[PS_WL1] : s[PS_WL2]) * XX;
        const T DPN2 = (CD > T(0) ? s[PS_WM1] : s[PS_WM2]) * XX;
        const T cg0 = PG_ROW(t, 4)[M];
        T DTHP, DTHM;
        if (IREFRA == 0) {
          DTHP = DRGP * cg0;
          DTHM = DRGM * cg0;
        } else {
          const T OM = PG_ROW(t, 5)[M];
          DTHP = DRGP * cg0 + OM * DRDP;
          DTHM = DRGM * cg0 + OM * DRDM;
        }
        const T CFLTP = DTHP + m_abs(DTHP);
        const T CFLTM = -DTHM + m_abs(DTHM);
        DTC = DTC + CFLTP + CFLTM;
        const T DTP = -DTHP + m_abs(DTHP);
        const T DTM = DTHM + m_abs(DTHM);
        F3 = (T(1) - DTC) * fo[c] + DPN * g0[c] + DPN2 * g1[c] + DLE * g4[c] + DTP * fkp[c] + DTM * fkm[c];
        if (M == 0) {      // the arguments of :719-721
          cf[0] = DTC; cf[1] = CFLEA; cf[2] = CFLEA; cf[3] = CFLNO; cf[4] = CFLNO; cf[5] = CFLNO; cf[6] = CFLNO; cf[7] = CFLTP; cf[8] = CFLTM;
          cf[9] = CFLTP; cf[10] = CFLTM;
        }
      } else {      // sections 2 and 4
        const int MP1 = min(NR - 1, M + 1), MM1 = max(0, M - 1);
        const T DFP = DELFR0 / tab->FR[M];
        const T DFM = DELFR0 / tab->FR[MM1];
        // DLA and DPH of the point and its neighbours (:430-435, :857-862); the land row has no current
        T DLA[PI_N], DPH[PI_N];
#pragma unroll
        for (int i = 0; i < PI_N; i++) {
          const T cgi = PG_ROW(t, i)[M];
          if (q[i] == nland) {
            DLA[i] = SEC == 2 ? SD * cgi * s[PS_DELLA0_NINF] : SD * cgi;
            DPH[i] = CD * cgi * DELPH0;
          } else {
            const T ui = sU[(t * 7 + i) * 2], vi = sU[(t * 7 + i) * 2 + 1];
            if (SEC == 2) DLA[i] = (ui + SD * cgi) * (i == 0 ? s[PS_DELLA0] : T(0.25) * (DELPRO * a.dellam1[q[i]]));
            else DLA[i] = ui + SD * cgi;
            DPH[i] = (vi + CD * cgi) * DELPH0;
          }
        }
        T DLWE, DLEA;
        if (SEC == 2) {
          DLWE = DLA[PI_IJ] + DLA[PI_LON1];
          DLEA = DLA[PI_IJ] + DLA[PI_LON2];
        } else {
          DLWE = (DLA[PI_IJ] + DLA[PI_LON1]) * s[PS_DELLA0] * s[PS_DCO];
          DLEA = (DLA[PI_IJ] + DLA[PI_LON2]) * s[PS_DELLA0] * s[PS_DCO];
        }
        T DLE = -DLEA + m_abs(DLEA);
        T DLW = DLWE + m_abs(DLWE);
        const T CFLEA = DLEA + m_abs(DLEA);
        const T CFLWE = -DLWE + m_abs(DLWE);
        T DTC, DPN, DPS, DPN2 = T(0), DPS2 = T(0), CFLNO, CFLSO, CFLNO2 = T(0), CFLSO2 = T(0);
        if (SEC == 2) {
          DTC = DLEA + m_abs(DLEA) - DLWE + m_abs(DLWE);
          const T DPSO = DPH[PI_IJ] + DPH[PI_LAT11];
          const T DPNO = DPH[PI_IJ] + DPH[PI_LAT21];
          DPN = -DPNO + m_abs(DPNO);
          DPS = DPSO + m_abs(DPSO);
          DTC = DTC + DPNO + m_abs(DPNO) - DPSO + m_abs(DPSO);
          CFLNO = CFLSO = T(0);
        } else {
          const T o_lon1 = ob ? ob[2 * NFRE + M] : T(1), o_lon2 = ob ? ob[3 * NFRE + M] : T(1);
          const T o_lat1 = ob ? ob[0 * NFRE + M] : T(1), o_lat2 = ob ? ob[1 * NFRE + M] : T(1);
          DLE = DLE * o_lon2;
          DLW = DLW * o_lon1;
          DTC = CFLEA + CFLWE;
          if (a.irgg == 1) {
            const T DPNO = (DPH[PI_IJ] + DPH[PI_LAT21] * s[PS_DP2]) * s[PS_WL2];
            DPN = (-DPNO + m_abs(DPNO)) * o_lat2;
            const T DPNO2 = (DPH[PI_IJ] + DPH[PI_LAT22] * s[PS_DP2]) * s[PS_WM2];
            DPN2 = (-DPNO2 + m_abs(DPNO2)) * o_lat2;
            const T DPSO = (DPH[PI_IJ] + DPH[PI_LAT11] * s[PS_DP1]) * s[PS_WL1];
            DPS = (DPSO + m_abs(DPSO)) * o_lat1;
            const T DPSO2 = (DPH[PI_IJ] + DPH[PI_LAT12] * s[PS_DP1]) * s[PS_WM1];
            DPS2 = (DPSO2 + m_abs(DPSO2)) * o_lat1;
            CFLNO = DPNO + m_abs(DPNO);
            CFLSO = -DPSO + m_abs(DPSO);
            CFLNO2 = DPNO2 + m_abs(DPNO2);
            CFLSO2 = -DPSO2 + m_abs(DPSO2);
            DTC = DTC + CFLNO + CFLSO + CFLNO2 + CFLSO2;
          } else {
            const T DPNO = DPH[PI_IJ] + DPH[PI_LAT21] * s[PS_DP2];
            DPN = (-DPNO + m_abs(DPNO)) * o_lat2;
            const T DPSO = DPH[PI_IJ] + DPH[PI_LAT11] * s[PS_DP1];
            DPS = (DPSO + m_abs(DPSO)) * o_lat1;
            CFLNO = DPNO + m_abs(DPNO);
            CFLSO = -DPSO + m_abs(DPSO);
            DTC = DTC + CFLNO + CFLSO;
          }
        }
        const T cg0 = PG_ROW(t, 0)[M], OM = PG_ROW(t, 7)[M];
        T DTHP, DTHM;
        if (SEC == 2) {
          DTHP = OM * DRDP + DRCP;
          DTHM = OM * DRDM + DRCM;
        } else {
          DTHP = DRGP * cg0 + OM * DRDP + DRCP;
          DTHM = DRGM * cg0 + OM * DRDM + DRCM;
        }
        const T CFLTP = DTHP + m_abs(DTHP);
        const T CFLTM = -DTHM + m_abs(DTHM);
        if (SEC == 2) DTC = DTC + DTHP + m_abs(DTHP) - DTHM + m_abs(DTHM);
        else DTC = DTC + CFLTP + CFLTM;
        const T DTP = -DTHP + m_abs(DTHP);
        const T DTM = DTHM + m_abs(DTHM);
        // SDOT(IJ,K,M), SDOT(IJ,K,MP1), SDOT(IJ,K,MM1): propdot.F90:190-191
        const T sd_m = (S0 * cg0 + OMDD * OM) * PG_ROW(t, 8)[M];
        const T sd_p = (S0 * PG_ROW(t, 0)[MP1] + OMDD * PG_ROW(t, 7)[MP1]) * PG_ROW(t, 8)[MP1];
        const T sd_q = (S0 * PG_ROW(t, 0)[MM1] + OMDD * PG_ROW(t, 7)[MM1]) * PG_ROW(t, 8)[MM1];
        DTHP = (sd_m + sd_p) * DFP;
        DTHM = (sd_m + sd_q) * DFM;
        const T CFLOP = DTHP + m_abs(DTHP);
        const T CFLOM = -DTHM + m_abs(DTHM);
        if (SEC == 2) DTC = DTC + DTHP + m_abs(DTHP) - DTHM + m_abs(DTHM);
        else DTC = DTC + CFLOP + CFLOM;
        const T DOP = (-DTHP + m_abs(DTHP)) / FRATIO;
        const T DOM = (DTHM + m_abs(DTHM)) * FRATIO;
        // F1(IJ,K,MP1), F1(IJ,K,MM1): inside the piece, beside it, or the clamped element itself
        const T f_mp = MP1 == M ? fo[c] : (c + 1 < VW ? fo[(c + 1) % VW] : fmp);
        const T f_mm = MM1 == M ? fo[c] : (c > 0 ? fo[(c + VW - 1) % VW] : fmm);
        F3 = (T(1) - DTC) * fo[c] + DPN * g0[c];
        if (SEC == 4 && a.irgg == 1) F3 = F3 + DPN2 * g1[c] + DPS * g2[c] + DPS2 * g3[c];
        else F3 = F3 + DPS * g2[c];
        F3 = F3 + DLE * g4[c] + DLW * g5[c] + DTP * fkp[c] + DTM * fkm[c] + DOP * f_mp + DOM * f_mm;
        if (M == 0) {      // the arguments of :925-927
          cf[0] = DTC; cf[1] = CFLEA; cf[2] = CFLWE; cf[3] = CFLNO; cf[4] = CFLSO; cf[5] = CFLNO2; cf[6] = CFLSO2; cf[7] = CFLTP; cf[8] = CFLTM;
          cf[9] = CFLOP; cf[10] = CFLOM;
        }
      }
      res[c] = F3;
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
#undef PG_ROW

template <typename T>
size_t propags_lds(int sec, int NFRE) {
  const int npl = (sec == 2 || sec == 4) ? 9 : 6;
  return (size_t)PG_TP * 8 * sizeof(int) + (size_t)PG_TP * (PG_NS + 14 + (size_t)npl * NFRE) * sizeof(T);
}

}  // namespace

template <typename T>
void launch_propags_dot(const void* tab, int n, int nland, int irefra, int icase, const AdvGeom& g, const void* depth, const void* ue, const void* ve, void* dot,
                        hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_propags_dot<T>, dim3((n + 255) / 256), dim3(256), 0, s, (const DevTab<T>*)tab, n, nland, irefra, icase, g.kxlt, (const T*)g.zdello,
                     (T)g.xdella, (const T*)g.cosph, g.klon, g.klat, (const T*)g.wlat, (const T*)g.cosphm1_ext, (const T*)depth, (const T*)ue, (const T*)ve,
                     (T*)dot);
}

template <typename T>
int launch_propags(const void* tab, const PropagsCall& c, int NFRE, hipStream_t s) {
  constexpr int VW = 16 / (int)sizeof(T);
  if (c.kijl <= c.kijs) return 0;
  const bool cur = c.irefra == 2 || c.irefra == 3;
  const int sec = c.icase == 1 ? (cur ? 4 : 3) : (cur ? 2 : 1);
  const size_t lds = propags_lds<T>(sec, NFRE);
  if (lds > 64 * 1024) return 1;
  PropagsArgs<T> a;
  a.f1 = (const T*)c.f1; a.f3 = (T*)c.f3;
  a.nland = c.nland; a.irefra = c.irefra; a.irgg = c.irgg;
  a.delpro = (T)c.delpro; a.delphi = (T)c.delphi;
  a.kxlt = c.kxlt;
  a.cosph = (const T*)c.cosph; a.sinph = (const T*)c.sinph; a.dellam1 = (const T*)c.dellam1; a.cosphm1 = (const T*)c.cosphm1;
  a.klon = c.klon; a.klat = c.klat;
  a.wlat = (const T*)c.wlat; a.cg = (const T*)c.cg; a.om = (const T*)c.om; a.wn = (const T*)c.wn; a.u = (const T*)c.u; a.v = (const T*)c.v;
  a.dot = (const T*)c.dot; a.obs = (const T*)c.obs;
  a.kijs = c.kijs; a.kijl = c.kijl; a.copy_rest = c.copy_rest;
  a.cfl = (T*)c.cfl; a.cflfail = c.cflfail;
  const dim3 grid((c.kijl - c.kijs + PG_TP - 1) / PG_TP), block(256);
  const DevTab<T>* tp = (const DevTab<T>*)tab;
  switch (sec) {
    case 1: hipLaunchKernelGGL((k_propags<T, VW, 1>), grid, block, lds, s, tp, a); break;
    case 2: hipLaunchKernelGGL((k_propags<T, VW, 2>), grid, block, lds, s, tp, a); break;
    case 3: hipLaunchKernelGGL((k_propags<T, VW, 3>), grid, block, lds, s, tp, a); break;
    default:
      if (c.dp_product) hipLaunchKernelGGL((k_propags<T, VW, 4, true>), grid, block, lds, s, tp, a);
      else hipLaunchKernelGGL((k_propags<T, VW, 4>), grid, block, lds, s, tp, a);
      break;
  }
  return 0;
}

template void launch_propags_dot<float>(const void*, int, int, int, int, const AdvGeom&, const void*, const void*, const void*, void*, hipStream_t);
template void launch_propags_dot<double>(const void*, int, int, int, int, const AdvGeom&, const void*, const void*, const void*, void*, hipStream_t);
template int launch_propags<float>(const void*, const PropagsCall&, int, hipStream_t);
template int launch_propags<double>(const void*, const PropagsCall&, int, hipStream_t);
