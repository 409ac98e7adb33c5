// The forcing and coupling seam on the device (include/ecwam_hip_forcing.h): what WAVEMDL runs around WAMODEL.
//   k_getwnd       GETWND per chunk (getwnd.F90:211-229): WAMWND (wamwnd.F90:126-294), then MICEP (micep.F90:116-254)
//   k_cdustarz0    CDUSTARZ0 with ZREF = XNLEV (cdustarz0.F90:66-71 as getfrstwnd.F90:125-126 calls it); its POW and EXP are those of dd_math.h
//   k_wamadswstar  WAMADSWSTAR (wamadswstar.F90:60-69)
//   k_getcurr      WAMCUR (wamcur.F90:78-85), the NEMO currents and the zero currents of getcurr.F90:135-198, with KUPDATE (getcurr.F90:268-278)
//   k_wvblock      OUTBETA (outbeta.F90:113-125) and the WVBLOCK fill (wavemdl.F90:757-802)
//   k_fld_init, k_fld_scatter   MPFLDTOIFS on one task (mpfldtoifs.F90:105-118, 346-352)
// All of them are point-wise and bound by the bytes they move (and, at the sizes of a model, by the launch).  One thread per sea point.  A row
// of ff / intf is 16 reals = 4 (single) or 8 (double precision) pieces of 16 bytes: FfRow loads and stores whole pieces, and only those that
// hold a column the routine reads or writes -- a piece whose every column is written is not loaded.  The gathers from the gridded planes go
// through the map that ecwam_hip_set_forcing_map validated on the host.  The arithmetic keeps the reference's order, without contraction.
#include "../../include/ecwam_hip_forcing.h"
#include "dev.h"
#include "ff_row.h"
#include "launch.h"
#include "dd_math.h"      // after the HIP runtime: its <cmath> is the one the device overloads extend

template <typename T>
struct GetwndPar {
  int icode, llwswave, llwdwave, lcorrel, iparamci, lwcou, cic, cit, icerest, liceth, swamp;
  T rwfac, swampcith, zmiss;
};

// ICODE3: the wind at 10 m goes to WSWAVE and UFRIC is kept; otherwise the friction velocity goes to UFRIC and WSWAVE is kept
template <typename T, bool ICODE3>
__global__ void __launch_bounds__(256) k_getwnd(const DevTab<T>* __restrict__ tp, int kijs, int kijl, const int* __restrict__ map, const T* __restrict__ fieldg, size_t ncell,
                                                const T* __restrict__ ucur, const T* __restrict__ vcur, const double* __restrict__ nemo, T* __restrict__ ffa,
                                                const GetwndPar<T> a) {
#pragma clang fp contract(off)
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const DevTab<T>& tb = *tp;
  constexpr unsigned W = col(F_AIRD) | col(F_WDWAVE) | col(F_CICOVER) | col(F_WSTAR) | col(F_USTRA) | col(F_VSTRA) | col(F_CITHICK) |
                         (ICODE3 ? col(F_WSWAVE) : col(F_UFRIC));
  const T* __restrict__ fg = fieldg + map[ij];
  T* __restrict__ frow = ffa + (size_t)ij * ECWAM_HIP_NFF;
  FfRow<T> r;
  r.template load_for<0u, W>(frow);
  // ---- WAMWND
  T UU = fg[ECWAM_HIP_FG_UWND * ncell], VV = fg[ECWAM_HIP_FG_VWND * ncell];
  const T ADS = fg[ECWAM_HIP_FG_AIRD * ncell];
  T CITH = fg[ECWAM_HIP_FG_CITHICK * ncell];
  r.v[F_AIRD] = ADS;
  r.v[F_WSTAR] = fg[ECWAM_HIP_FG_WSTAR * ncell];
  r.v[F_USTRA] = fg[ECWAM_HIP_FG_USTRA * ncell];
  r.v[F_VSTRA] = fg[ECWAM_HIP_FG_VSTRA * ncell];
  T THW;
  if constexpr (ICODE3) {
    T U10;
    if (a.llwswave && a.llwdwave) {
      U10 = fg[ECWAM_HIP_FG_WSWAVE * ncell];
      THW = fg[ECWAM_HIP_FG_WDWAVE * ncell];
      if (U10 <= T(0)) {      // no value of the wave model: U and V of the atmosphere instead
        const T ws = m_sqrt(UU * UU + VV * VV);
        if (ws > T(0)) { U10 = ws; THW = m_atan2(UU, VV); }
        else { U10 = T(0); THW = T(0); }
      }
      if (a.lcorrel) {
        UU = U10 * m_sin(THW);
        VV = U10 * m_cos(THW);
        UU = UU - a.rwfac * ucur[ij];
        VV = VV - a.rwfac * vcur[ij];
        const T ws = m_sqrt(UU * UU + VV * VV);
        if (ws > T(0)) { U10 = ws; THW = m_atan2(UU, VV); }
        else { U10 = T(0); THW = T(0); }
      }
    } else {
      if (a.llwswave) {
        const T w = fg[ECWAM_HIP_FG_WSWAVE * ncell];
        if (w != a.zmiss && w > T(0)) {
          const T ws = m_sqrt(UU * UU + VV * VV);
          if (ws > T(0)) {
            const T rescale = w / ws;
            UU = UU * rescale;
            VV = VV * rescale;
          }
        }
      }
      if (a.lcorrel) {
        UU = UU + a.rwfac * ucur[ij];
        VV = VV + a.rwfac * vcur[ij];
      }
      U10 = m_sqrt(UU * UU + VV * VV);
      THW = U10 != T(0) ? m_atan2(UU, VV) : T(0);
    }
    r.v[F_WSWAVE] = m_max(U10, tb.WSPMIN);
  } else {
    T US = m_sqrt(UU * UU + VV * VV);
    THW = US != T(0) ? m_atan2(UU, VV) : T(0);
    if (a.icode == 2) US = m_sqrt(m_max(US, T(0)) / m_max(ADS, T(1)));      // the input is a surface stress
    r.v[F_UFRIC] = m_max(US, tb.EPSUS);
  }
  if (THW < T(0)) THW = THW + tb.ZPI;
  r.v[F_WDWAVE] = THW;
  // ---- MICEP
  const T C1 = T(0.2), C2 = T(0.4);
  const bool lake = (a.cic || a.cit) && a.lwcou && !(fg[ECWAM_HIP_FG_LKFR * ncell] <= T(0));
  T CICVR;
  if (a.cic && !lake) {
    CICVR = T(nemo[ij]);      // NEMOCICOVER
  } else if (a.cic || a.iparamci == 31) {
    const T ci = fg[ECWAM_HIP_FG_CICOVER * ncell];
    if (ci == a.zmiss || ci < T(0.01) || ci > T(1.01)) CICVR = T(0);
    else if (ci > T(0.95)) CICVR = T(1);
    else CICVR = ci;
  } else {
    CICVR = fg[ECWAM_HIP_FG_CICOVER * ncell] < T(271.5) ? T(1) : T(0);      // IPARAM 139: the plane holds the sea surface temperature
  }
  const bool check = tb.LICERUN && !tb.LMASKICE && !a.swamp && (a.cit || a.liceth);
  if (!tb.LICERUN || tb.LMASKICE) {
    CITH = T(0);
  } else if (a.swamp) {
    CITH = CICVR > T(0) ? a.swampcith : T(0);
  } else if ((!a.liceth && !a.cit) || (a.cit && lake)) {      // parameterised from the cover
    CITH = CICVR > T(0) ? m_max(C1 + C2 * CICVR, T(0)) : T(0);
  } else if (a.cit) {
    const double th = nemo[(size_t)kijl + ij];      // NEMOCITHICK (JWRO): the product is formed in its kind
    CITH = a.icerest ? T(th) : T((double)CICVR * th);
  } else {
    CITH = CICVR * CITH;
  }
  if (check && CICVR > T(0) && CITH < T(0.5) * tb.HICMIN) {      // no ice if it is thinner than 0.5 HICMIN
    CICVR = T(0);
    CITH = T(0);
  }
  r.v[F_CICOVER] = CICVR;
  r.v[F_CITHICK] = CITH;
  r.template store<W>(frow);
}

template <typename T>
__global__ void __launch_bounds__(256) k_cdustarz0(const DevTab<T>* __restrict__ tp, int kijs, int kijl, T* __restrict__ ffa) {
#pragma clang fp contract(off)
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const DevTab<T>& tb = *tp;
  constexpr unsigned W = col(F_UFRIC) | col(F_Z0M);
  const T C1CD = T(1.03e-3), C2CD = T(0.04e-3), P1CD = T(1.48), P2CD = T(-0.21), Z0MIN = T(0.000001);      // yowpcons.F90:61-64, cdustarz0.F90:57
  T* __restrict__ frow = ffa + (size_t)ij * ECWAM_HIP_NFF;
  FfRow<T> r;
  r.template load_for<col(F_WSWAVE), W>(frow);
  const T u10p = m_max(r.v[F_WSWAVE], tb.WSPMIN);
  // Z0 moves by about XKAPPA U10 / USTAR = 8 .. 12 roundings when a power below moves by one: POW and EXP rounded once (dd_math.h)
  const T cd = m_min((C1CD + C2CD * ref_pow(u10p, P1CD)) * ref_pow(u10p, P2CD), tb.CDMAX);
  const T ustar = m_max(m_sqrt(cd) * u10p, tb.EPSUS);
  r.v[F_UFRIC] = ustar;
  r.v[F_Z0M] = m_max(tb.XNLEV / (ref_exp(tb.XKAPPA * m_min(u10p / ustar, T(100))) - T(1)), Z0MIN);
  r.template store<W>(frow);
}

template <typename T>
__global__ void __launch_bounds__(256) k_wamadswstar(int kijs, int kijl, const int* __restrict__ map, const T* __restrict__ fieldg, size_t ncell, T* __restrict__ ffa) {
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  constexpr unsigned W = col(F_AIRD) | col(F_WSTAR) | col(F_USTRA) | col(F_VSTRA);
  const T* __restrict__ fg = fieldg + map[ij];
  T* __restrict__ frow = ffa + (size_t)ij * ECWAM_HIP_NFF;
  FfRow<T> r;
  r.template load_for<0u, W>(frow);
  r.v[F_AIRD] = fg[ECWAM_HIP_FG_AIRD * ncell];
  r.v[F_WSTAR] = fg[ECWAM_HIP_FG_WSTAR * ncell];
  r.v[F_USTRA] = fg[ECWAM_HIP_FG_USTRA * ncell];
  r.v[F_VSTRA] = fg[ECWAM_HIP_FG_VSTRA * ncell];
  r.template store<W>(frow);
}

// SIGN(MIN(ABS(x), CURRENT_MAX), x)
__device__ __forceinline__ float cur_clip(float x) { return copysignf(fminf(fabsf(x), 1.5f), x); }
__device__ __forceinline__ double cur_clip(double x) { return copysign(fmin(fabs(x), 1.5), x); }

template <typename T>
__global__ void __launch_bounds__(256) k_getcurr(int kijs, int kijl, int mode, const int* __restrict__ map, const T* __restrict__ fieldg, size_t ncell,
                                                 const double* __restrict__ nemo, T* __restrict__ ucur, T* __restrict__ vcur, int* __restrict__ changed) {
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  T u = T(0), v = T(0);
  if (mode == 0) {
    const T* __restrict__ fg = fieldg + map[ij];
    u = cur_clip(fg[ECWAM_HIP_FG_UCUR * ncell]);
    v = cur_clip(fg[ECWAM_HIP_FG_VCUR * ncell]);
  } else if (mode == 1) {
    if (fieldg[ECWAM_HIP_FG_LKFR * ncell + map[ij]] <= T(0)) {      // an open ocean point: the clip is formed in NEMO's kind (JWRO)
      u = T(cur_clip(nemo[(size_t)2 * kijl + ij]));
      v = T(cur_clip(nemo[(size_t)3 * kijl + ij]));
    }
  }
  // KUPDATE: every lane that sees a change stores the same 1 (an ordinary store: no atomic, no reduction)
  if (changed && (u != ucur[ij] || v != vcur[ij])) *changed = 1;
  ucur[ij] = u;
  vcur[ij] = v;
}

// FLAGS: the ECWAM_HIP_WVB_* bits; LLGCBZ0 of the context decides whether OUTBETA reads WSWAVE
template <typename T, int FLAGS, bool LLGCBZ0>
__global__ void __launch_bounds__(256) k_wvblock(const DevTab<T>* __restrict__ tp, int kijs, int kijl, const T* __restrict__ ffa, const T* __restrict__ intfa, int nwvfields,
                                                 T prchar, T* __restrict__ wvblock, size_t ld) {
#pragma clang fp contract(off)
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  T* __restrict__ o = wvblock + ij;
  int f = 0;
  T betam = prchar;
  if constexpr ((FLAGS & ECWAM_HIP_WVB_LWCOU2W) != 0) {
    const DevTab<T>& tb = *tp;
    const T AMAX = T(0.02), BMAX = T(0.01), BETAHQ_REDUCE = T(0.25);      // outbeta.F90:90-96
    constexpr unsigned R = col(F_UFRIC) | col(F_Z0B) | col(F_CHRNCK) | (LLGCBZ0 ? 0u : col(F_WSWAVE));
    FfRow<T> r;
    r.template load<R>(ffa + (size_t)ij * ECWAM_HIP_NFF);
    const T amaxu10 = LLGCBZ0 ? tb.ALPHAMAX : m_min(tb.ALPHAMAX, AMAX + BMAX * r.v[F_WSWAVE]);
    const T usm = T(1) / m_max(r.v[F_UFRIC], tb.EPSUS);
    const T gusm2 = tb.G * (usm * usm);
    betam = m_max(m_min(r.v[F_CHRNCK], amaxu10), tb.ALPHAMIN);
    const T betahq = m_max(BETAHQ_REDUCE * (betam - m_max(r.v[F_Z0B] * gusm2, tb.ALPHA)), tb.ALPHAMIN);
    o[ld * f++] = betam;
    if constexpr ((FLAGS & ECWAM_HIP_WVB_LWCOUHMF) != 0) o[ld * f++] = betahq;
  } else {
    o[ld * f++] = betam;
  }
  if constexpr ((FLAGS & (ECWAM_HIP_WVB_LWSTOKES | ECWAM_HIP_WVB_LWFLUX)) != 0) {
    constexpr unsigned RS = col(I_USTOKES) | col(I_VSTOKES);
    constexpr unsigned RF = col(I_PHIOCD) | col(I_TAUOCXD) | col(I_TAUOCYD) | col(I_TAUICX) | col(I_TAUICY) | col(I_WSEMEAN) | col(I_WSFMEAN);
    constexpr unsigned R = ((FLAGS & ECWAM_HIP_WVB_LWSTOKES) ? RS : 0u) | ((FLAGS & ECWAM_HIP_WVB_LWFLUX) ? RF : 0u);
    FfRow<T> r;
    r.template load<R>(intfa + (size_t)ij * ECWAM_HIP_NINTF);
    if constexpr ((FLAGS & ECWAM_HIP_WVB_LWSTOKES) != 0) {
      o[ld * f++] = r.v[I_USTOKES];
      o[ld * f++] = r.v[I_VSTOKES];
    }
    if constexpr ((FLAGS & ECWAM_HIP_WVB_LWFLUX) != 0) {
      o[ld * f++] = r.v[I_PHIOCD];
      o[ld * f++] = r.v[I_TAUOCXD];
      o[ld * f++] = r.v[I_TAUOCYD];
      o[ld * f++] = r.v[I_TAUICX];
      o[ld * f++] = r.v[I_TAUICY];
      o[ld * f++] = r.v[I_WSEMEAN];
      o[ld * f++] = r.v[I_WSFMEAN];
    }
  }
  for (; f < nwvfields; f++) o[ld * f] = T(0);
}

template <typename T>
struct FldDefaults { T v[ECWAM_HIP_MAXWVFIELDS]; };

// LLINIT_GRID: GRID(:,:,IFLD) = DEFVAL(IFLD)
template <typename T>
__global__ void __launch_bounds__(256) k_fld_init(T* __restrict__ grid, size_t ncell, int nwvfields, const FldDefaults<T> d) {
  const size_t total = ncell * (size_t)nwvfields;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) grid[g] = d.v[g / ncell];
}
// GRID(IX,IY,IFLD) = BLOCK(IJ,IFLD): the cells of the map are distinct (ecwam_hip_set_forcing_map)
template <typename T>
__global__ void __launch_bounds__(256) k_fld_scatter(int kijs, int kijl, const int* __restrict__ map, const T* __restrict__ wvblock, size_t ld, int nwvfields, T* __restrict__ grid,
                                                     size_t ncell) {
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const size_t c = (size_t)map[ij];
  for (int f = 0; f < nwvfields; f++) grid[ncell * f + c] = wvblock[ld * f + ij];
}

static inline dim3 rows_grid(int kijs, int kijl) { return dim3((unsigned)((kijl - kijs + 255) / 256)); }

template <typename T>
void launch_getwnd(const void* tab, int kijs, int kijl, const int* map, const void* fieldg, size_t ncell, const void* ucur, const void* vcur, const double* nemo, void* ff,
                   const ecwam_hip_forcing_opts& o, hipStream_t s) {
  if (kijl <= kijs) return;
  GetwndPar<T> a = {};
  a.icode = o.icode_wnd; a.llwswave = o.llwswave != 0; a.llwdwave = o.llwdwave != 0; a.lcorrel = o.lcorrel != 0; a.iparamci = o.iparamci;
  a.lwcou = o.lwcou != 0; a.cic = o.lwnemocoucic != 0; a.cit = o.lwnemocoucit != 0; a.icerest = o.lnemoicerest != 0; a.liceth = o.liceth != 0;
  a.swamp = o.swamp != 0;
  a.rwfac = T(o.rwfac); a.swampcith = T(o.swampcith); a.zmiss = T(o.zmiss);
  if (o.icode_wnd == 3)
    hipLaunchKernelGGL((k_getwnd<T, true>), rows_grid(kijs, kijl), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, map, (const T*)fieldg, ncell, (const T*)ucur,
                       (const T*)vcur, nemo, (T*)ff, a);
  else
    hipLaunchKernelGGL((k_getwnd<T, false>), rows_grid(kijs, kijl), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, map, (const T*)fieldg, ncell, (const T*)ucur,
                       (const T*)vcur, nemo, (T*)ff, a);
}
template <typename T>
void launch_cdustarz0(const void* tab, int kijs, int kijl, void* ff, hipStream_t s) {
  if (kijl <= kijs) return;
  hipLaunchKernelGGL((k_cdustarz0<T>), rows_grid(kijs, kijl), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, (T*)ff);
}
template <typename T>
void launch_wamadswstar(int kijs, int kijl, const int* map, const void* fieldg, size_t ncell, void* ff, hipStream_t s) {
  if (kijl <= kijs) return;
  hipLaunchKernelGGL((k_wamadswstar<T>), rows_grid(kijs, kijl), dim3(256), 0, s, kijs, kijl, map, (const T*)fieldg, ncell, (T*)ff);
}
template <typename T>
void launch_getcurr(int kijs, int kijl, int mode, const int* map, const void* fieldg, size_t ncell, const double* nemo, void* ucur, void* vcur, int* changed, hipStream_t s) {
  if (kijl <= kijs) return;
  hipLaunchKernelGGL((k_getcurr<T>), rows_grid(kijs, kijl), dim3(256), 0, s, kijs, kijl, mode, map, (const T*)fieldg, ncell, nemo, (T*)ucur, (T*)vcur, changed);
}

template <typename T, int FLAGS>
static void wvblock_go(const void* tab, int llgcbz0, int kijs, int kijl, const void* ff, const void* intf, int nwvfields, double prchar, void* wvblock, int ld, hipStream_t s) {
  if (llgcbz0)
    hipLaunchKernelGGL((k_wvblock<T, FLAGS, true>), rows_grid(kijs, kijl), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, (const T*)ff, (const T*)intf, nwvfields, T(prchar),
                       (T*)wvblock, (size_t)ld);
  else
    hipLaunchKernelGGL((k_wvblock<T, FLAGS, false>), rows_grid(kijs, kijl), dim3(256), 0, s, (const DevTab<T>*)tab, kijs, kijl, (const T*)ff, (const T*)intf, nwvfields, T(prchar),
                       (T*)wvblock, (size_t)ld);
}
// flags: LWCOUHMF only beside LWCOU2W (ecwam_hip_wvblock refuses the rest)
template <typename T>
void launch_wvblock(const void* tab, int llgcbz0, int kijs, int kijl, const void* ff, const void* intf, int flags, int nwvfields, double prchar, void* wvblock, int ld,
                    hipStream_t s) {
  if (kijl <= kijs) return;
  switch (flags) {
#define WVB_CASE(F_) case F_: wvblock_go<T, F_>(tab, llgcbz0, kijs, kijl, ff, intf, nwvfields, prchar, wvblock, ld, s); break
    WVB_CASE(0); WVB_CASE(1); WVB_CASE(3); WVB_CASE(4); WVB_CASE(5); WVB_CASE(7); WVB_CASE(8); WVB_CASE(9); WVB_CASE(11); WVB_CASE(12); WVB_CASE(13); WVB_CASE(15);
#undef WVB_CASE
  }
}
template <typename T>
void launch_fldtoifs(int kijs, int kijl, const int* map, const void* wvblock, int ld, int nwvfields, const double* defval, void* grid, size_t ncell, hipStream_t s) {
  if (defval) {
    FldDefaults<T> d = {};
    for (int f = 0; f < nwvfields; f++) d.v[f] = T(defval[f]);
    const size_t total = ncell * (size_t)nwvfields, want = (total + 255) / 256;
    hipLaunchKernelGGL((k_fld_init<T>), dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s, (T*)grid, ncell, nwvfields, d);
  }
  if (kijl <= kijs) return;
  hipLaunchKernelGGL((k_fld_scatter<T>), rows_grid(kijs, kijl), dim3(256), 0, s, kijs, kijl, map, (const T*)wvblock, (size_t)ld, nwvfields, (T*)grid, ncell);
}

#define FORCING_INSTANTIATE(T)                                                                                                                                     \
  template void launch_getwnd<T>(const void*, int, int, const int*, const void*, size_t, const void*, const void*, const double*, void*, const ecwam_hip_forcing_opts&, \
                                 hipStream_t);                                                                                                                     \
  template void launch_cdustarz0<T>(const void*, int, int, void*, hipStream_t);                                                                                    \
  template void launch_wamadswstar<T>(int, int, const int*, const void*, size_t, void*, hipStream_t);                                                              \
  template void launch_getcurr<T>(int, int, int, const int*, const void*, size_t, const double*, void*, void*, int*, hipStream_t);                                 \
  template void launch_wvblock<T>(const void*, int, int, int, const void*, const void*, int, int, double, void*, int, hipStream_t);                                \
  template void launch_fldtoifs<T>(int, int, const int*, const void*, int, int, const double*, void*, size_t, hipStream_t);
FORCING_INSTANTIATE(float)
FORCING_INSTANTIATE(double)
#undef FORCING_INSTANTIATE
