// Launch glue of k_implsch4 (implsch_v4.h), shared by the translation units that instantiate it: implsch4.hip (flag sets A and B),
// implsch4x.hip (IPHYS = 0, ISNONLIN = 1), implsch4r.hip (RARE), implsch4a.hip (the one-kernel step) and implsch4w.hip (WDFLUXES).
#pragma once
#include "implsch_common.h"
#include "implsch_point.h"
#include "implsch_v4.h"
#include "implsch_v4_shapes.h"

template <typename T, int NANG, int PP>
static constexpr size_t v4_lds_bytes() {
  return (size_t)((V4_NFRE + V4_NSTG) * PP * NANG + PP * V4_NFRE * 4 + 2 * V4_PLN(PP, NANG) + PP * NSC) * sizeof(T);
}

// What launch4 runs between the pre and the fin kernel: V4_STEP the one kernel (PART = 0); V4_SPLIT PART 1 and PART 2 of it one after the other
// instead (needs the context's wi rows, n x NANG x NFRE); V4_WDF WDFLUXES (PART = 3 with the matching pre / fin): fl1 and ff are only read; of intf
// the flux members, of w2n columns 0, 1 are written, and those only with WDFLUXES' own LCFLX
enum { V4_STEP, V4_SPLIT, V4_WDF };

// One launch of k_implsch4 at shape S (implsch_v4_shapes.h): one workgroup per PP points, in the natural order.  ADV != 0: the one-kernel WAMINTGR
// step (the tile load is PROPAGS2 of the wave's points from the rows of adv.f_in; fl1 = the rows the new spectrum is stored to, another buffer).
template <typename T, typename S, bool EXT, bool JAN = false, bool ENHMC = false, bool RARE = false, int MODE = V4_STEP, int ADV = 0>
static int launch4(const void* tab, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws, void* fin,
                   double* w2n, void* gfast, int gk, void* wi, const V4Adv<T>& adv, hipStream_t s) {
  constexpr int NANG = S::NANG, PP = S::template PP<T>;
  constexpr bool SPLIT = MODE == V4_SPLIT, WDF = MODE == V4_WDF;
  const int n = kijl - kijs;
  constexpr size_t shmem0 = v4_lds_bytes<T, NANG, PP>();
  static_assert(shmem0 <= 160 * 1024, "LDS");
  size_t shmem = shmem0;
  if constexpr (!WDF && ADV == 0) {
    // diagnostics (tools/occupancy_sweep4.py): ECWAM_HIP_IMPLSCH_PADLDS=<bytes> pads the LDS request, i.e. lowers the resident waves per CU
    static const int pad = [] { const char* e = getenv("ECWAM_HIP_IMPLSCH_PADLDS"); return e ? atoi(e) : 0; }();
    if (pad > 0 && shmem0 + (size_t)pad <= 160 * 1024) shmem = shmem0 + (size_t)pad;
  }
  if (SPLIT && !wi) return -1;
  // the scalar start of the step (first TAUT_Z0), one point per lane, into the rows of fin
  hipLaunchKernelGGL((k_implsch4_pre<T, EXT, RARE, WDF>), dim3((n + 63) / 64), dim3(64), 0, s, (const DevTab<T>*)tab, kijs, kijl, (const T*)ff, (T*)fin);
#define V4_KERNEL(PART) k_implsch4<T, NANG, PP, S::R1, S::R2, S::NH, EXT, JAN, ENHMC, RARE, PART, ADV>
  auto lds = [&](auto k) { if (shmem > 64 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem); };
  auto run = [&](auto k) {
    hipLaunchKernelGGL(k, dim3((n + PP - 1) / PP), dim3(64), shmem, s, (const DevTab<T>*)tab, kijs, kijl, (T*)fl1, (const T*)wvprpt, (T*)ff, (T*)intf, mij,
                       (T*)xllws, (T*)fin, (T*)gfast, gk, (T*)wi, adv);
  };
  if constexpr (SPLIT) {
    lds(V4_KERNEL(1)); lds(V4_KERNEL(2));
    run(V4_KERNEL(1)); run(V4_KERNEL(2));
  } else {
    lds(V4_KERNEL(WDF ? 3 : 0));
    run(V4_KERNEL(WDF ? 3 : 0));
  }
#undef V4_KERNEL
  // the scalar end of the step (second STRESSO, WNFLUXES), one point per lane, from the rows the kernel above left in fin
  hipLaunchKernelGGL((k_implsch4_fin<T, EXT, WDF>), dim3((n + 63) / 64), dim3(64), 0, s, (const DevTab<T>*)tab, kijs, kijl, (const T*)fin, (T*)ff,
                     (T*)intf, w2n);
  return 0;
}
