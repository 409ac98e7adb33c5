// Launcher of the common builds of k_implsch4 (implsch_v4.h: PP sea points per wavefront on adjacent direction pairs, every rotation in K
// through LDS rows): implsch.F90:10-468 on flag set A (LLGCBZ0 = F, LLNORMAGAM = F) and, in the EXT build, flag set B (either or both of
// them T: cy49r1 / cy50r1), with or without the sea-ice damping LCIWA1 / LCIWA3 / LCISCAL and the NEMO coupling outputs of LWNEMOCOU; IPHYS = 1,
// ISNONLIN = 0, ICODE = 3; NFRE = 36, every shape of implsch_v4_shapes.h, single and double precision: the variants A and B of launch.h.
// (IPHYS 0 / ISNONLIN 1: implsch4x.hip; every other switch: implsch4r.hip.)
#include "implsch_v4_launch.h"
#include "launch.h"

// v: A or B (EXT).  Returns 0 when launched, -1 when no instantiation covers the variant or (NANG, r1, r2, nh): ecwam_hip_create refuses those
// configurations
template <typename T>
int launch_implsch4(const void* tab, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws,
                    void* fin, double* w2n, void* gfast, int gk, void* wi, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s) {
  if (kijl - kijs <= 0) return 0;
  if (NFRE != V4_NFRE || (v != Implsch4Variant::A && v != Implsch4Variant::B)) return -1;
#define V4_ARGS tab, kijs, kijl, fl1, wvprpt, ff, intf, mij, xllws, fin, w2n, gfast, gk, wi, V4Adv<T>{}, s
  return v4_for_shape(NANG, r1, r2, nh, [&](auto sh) {
    using S = decltype(sh);
    return v == Implsch4Variant::B ? launch4<T, S, true>(V4_ARGS) : launch4<T, S, false>(V4_ARGS);
  });
#undef V4_ARGS
}
// elements of the working precision per sea point the caller provides in fin (indexed by the absolute point number, like FL1)
int implsch4_fin_row() { return V4_NFIN; }
template int launch_implsch4<float>(const void*, int, int, void*, const void*, void*, void*, int*, void*, void*, double*, void*, int, void*, int, int, int, int, int, Implsch4Variant, hipStream_t);
template int launch_implsch4<double>(const void*, int, int, void*, const void*, void*, void*, int*, void*, void*, double*, void*, int, void*, int, int, int, int, int, Implsch4Variant, hipStream_t);
