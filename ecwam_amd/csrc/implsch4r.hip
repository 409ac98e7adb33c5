// Launcher of the RARE builds of k_implsch4 (implsch_v4.h): what no registered test configuration of the reference selects -- ISNONLIN = 2
// (TRANSF_SNL + PEAK_ANG), LCIWA2 (sdice2.F90), the NEMO ice stress and strain LWNEMOCOUWRS / LWNEMOCOUSTRN (wnfluxes.F90:178-196,
// cimsstrn.F90), friction-velocity forcing ICODE = 1, 2 (airsea.F90:100-117), LWVFLX_SNL = F, and ISNONLIN = 1 beside LLGCBZ0 / LLNORMAGAM or
// IPHYS = 0 -- decided at run time inside two builds per shape (implsch_v4_shapes.h), the variants rare (EXT + ENHMC) and rare_iphys0 (EXT + JAN +
// ENHMC) of launch.h.  A translation unit of its own: the builds compile beside those of implsch4.hip / implsch4x.hip.
#include "implsch_v4_launch.h"
#include "launch.h"

// v: rare or rare_iphys0 (JAN).  Returns 0 when launched, -1 when no instantiation covers the configuration (ecwam_hip_create refuses those).
// V4R_PREC selects the precision this object instantiates: 1 = single (implsch4r.o), 2 = double (implsch4rd.o).
// Double precision runs as the two-kernel split (launch4 V4_SPLIT; + 12 % time, the context owns wind-input rows for it).  As ONE function the
// double precision builds ended in a memory access fault or in wrong numbers at -O3 on their first launch, a code generation problem of one
// 280 KB function with > 256 VGPRs + AGPR copies + > 100 SGPR spills + a call; the split does not depend on the optimisation level
// (the history: profiles/r05_rare_dp_rootcause.txt, profiles/r06_rare_dp_note.txt).
#ifndef V4R_PREC
#define V4R_PREC 3
#endif
template <typename T>
int launch_implsch4r(const void* tab, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws,
                     void* fin, double* w2n, void* gfast, int gk, void* wi, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s) {
  if (kijl - kijs <= 0) return 0;
  if (NFRE != V4_NFRE || (v != Implsch4Variant::rare && v != Implsch4Variant::rare_iphys0)) return -1;
  constexpr int MODE = sizeof(T) == 4 ? V4_STEP : V4_SPLIT;      // double precision: the two-kernel split
#define V4_ARGS tab, kijs, kijl, fl1, wvprpt, ff, intf, mij, xllws, fin, w2n, gfast, gk, wi, V4Adv<T>{}, s
  // (the IPHYS = 0 build carries LLGCBZ0 / LLNORMAGAM too: EXT and JAN)
  return v4_for_shape(NANG, r1, r2, nh, [&](auto sh) {
    using S = decltype(sh);
    return v == Implsch4Variant::rare_iphys0 ? launch4<T, S, true, true, true, true, MODE>(V4_ARGS) : launch4<T, S, true, false, true, true, MODE>(V4_ARGS);
  });
#undef V4_ARGS
}
#define V4R_SIG(T) template int launch_implsch4r<T>(const void*, int, int, void*, const void*, void*, void*, int*, void*, void*, double*, void*, int, void*, int, int, int, int, int, Implsch4Variant, hipStream_t)
#if V4R_PREC & 1
V4R_SIG(float);
#endif
#if V4R_PREC & 2
V4R_SIG(double);
#endif
