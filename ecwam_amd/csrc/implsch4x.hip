// Launcher of the k_implsch4 builds for the alternate physics of SURVEY.md 8f rank 4 that the registered test configurations select:
// IPHYS = 0 (Janssen wind input + WAM cycle 4 dissipation: etopo1_oper_an_fc_O48_iphys_0) and ISNONLIN = 1 (the DIA scaled per
// interaction frequency), both on flag set A (LLGCBZ0 = F, LLNORMAGAM = F): the variants iphys0 and isnonlin1 of launch.h, at every shape of
// implsch_v4_shapes.h.  A translation unit of its own: the builds compile beside those of implsch4.hip.
#include "implsch_v4_launch.h"
#include "launch.h"

// v: iphys0 (JAN) or isnonlin1 (ENHMC).  Returns 0 when launched, -1 when no instantiation covers the configuration (ecwam_hip_create refuses those).
template <typename T>
int launch_implsch4x(const void* tab, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws,
                     void* fin, double* w2n, void* gfast, int gk, void* wi, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s) {
  if (kijl - kijs <= 0) return 0;
  if (NFRE != V4_NFRE || (v != Implsch4Variant::iphys0 && v != Implsch4Variant::isnonlin1)) return -1;
#define V4_ARGS tab, kijs, kijl, fl1, wvprpt, ff, intf, mij, xllws, fin, w2n, gfast, gk, wi, V4Adv<T>{}, s
  return v4_for_shape(NANG, r1, r2, nh, [&](auto sh) {
    using S = decltype(sh);
    return v == Implsch4Variant::iphys0 ? launch4<T, S, false, true, false>(V4_ARGS) : launch4<T, S, false, false, true>(V4_ARGS);
  });
#undef V4_ARGS
}
template int launch_implsch4x<float>(const void*, int, int, void*, const void*, void*, void*, int*, void*, void*, double*, void*, int, void*, int, int, int, int, int, Implsch4Variant, hipStream_t);
template int launch_implsch4x<double>(const void*, int, int, void*, const void*, void*, void*, int*, void*, void*, double*, void*, int, void*, int, int, int, int, int, Implsch4Variant, hipStream_t);
