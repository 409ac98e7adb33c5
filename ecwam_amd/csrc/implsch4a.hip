// Launcher of the ADV builds of k_implsch4 (implsch_v4.h): the one-kernel WAMINTGR step of round 6 -- PROPAGS2 (IREFRA = 0, one time step for
// every frequency, no obstructions) fused into IMPLSCH's tile load (wamintgr.F90:94-146, propag_wam.F90:247-251, propags2.F90:99-121).
// The variants A and B of launch.h (EXT; IPHYS = 1, ISNONLIN = 0, ICODE = 3) at the shapes and in the forms v4_adv_built states below; ADV = 1 the plain step, ADV = 3 the
// last advection step of the native O1280 cycle (fast waves M <= IFRELFMAX with their own time step, read from the compact rows of their sub-steps);
// ADV = 5 / 7 the same with the sub-grid obstructions of LSUBGRID (the reference's default on real bathymetry).  Everything else runs the
// two kernels (ecwam_hip_propags2_otf + ecwam_hip_implsch), which is also the A/B partner: the results are bit-identical.
#include "implsch_v4_launch.h"
#include "launch.h"

// Whether the form ADV (1 the plain step, 3 with fast waves, 5 with obstructions, 7 with both; each for flag sets A and B) is built at shape S in precision T.
// Single precision: every shape; 48 directions without the fast-wave forms (two points per wave: the LDS the tile load borrows has no room for
// the fast waves' second table).  The strict build of the weights (ECWAM_HIP_CTU_STRICT) has the plain form only: the caller runs the two kernels.
// Double precision: 36 directions only.  The other double precision builds were built and measured in round 6 and are NOT
// shipped: at -O3 the 12-direction builds and the fast-wave builds at 24 directions give wrong numbers (34 000 .. 58 000 of the bins of a
// 1 109-point grid differ from the two kernels, errors of order one from frequency 7 on), at -O1 the same source is bit-identical to the
// two kernels in every case -- the code-generation problem of the large double precision functions (256 VGPRs + 70 .. 84 AGPR copies + up to
// 100 SGPR spills) that the RARE builds met in round 4 (implsch4r.hip; profiles/r05_rare_dp_rootcause.txt, r06_fused_step_experiments.txt).
// Double precision at 48 / 24 / 12 directions runs the two kernels; the 36-direction builds are held to the two kernels bit for bit by
// tests/test_gpu_fused.py in every form.
template <typename T, typename S, int ADV>
constexpr bool v4_adv_built = (sizeof(T) == 4 || S::NANG == 36) && (ADV == 1 || !ECWAM_HIP_CTU_STRICT) && (!(ADV & 2) || S::NANG != 48);

// v: A or B (EXT).  Returns 0 when launched, -1 when no ADV build covers the configuration (the caller then runs the two kernels)
template <typename T>
int launch_implsch4_adv(const void* tab, int kijs, int kijl, void* fl_out, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws, void* fin,
                        double* w2n, const Implsch4AdvArgs* a, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s) {
  if (kijl - kijs <= 0) return 0;
  if (NFRE != V4_NFRE || (v != Implsch4Variant::A && v != Implsch4Variant::B)) return -1;
  V4Adv<T> adv;
  adv.f_in = (const T*)a->f_in; adv.klon = a->klon; adv.klat = a->klat; adv.kcor = a->kcor; adv.cg = (const T*)a->cg; adv.pt = (const T*)a->pt;
  adv.dirT = (const T*)a->dirT; adv.dirI = a->dirI; adv.xdella = (T)a->xdella; adv.delpro = (T)a->delpro; adv.m0 = a->m0; adv.m1 = a->m1;
  adv.gin = (const T*)a->gin; adv.delpro_lf = (T)a->delpro_lf; adv.gin_k = a->gin_k; adv.mlf = a->mlf; adv.obs = (const T*)a->obs;
  if (!a->gin && a->mlf != 0) return -1;
  const int form = 1 | (a->gin ? 2 : 0) | (a->obs ? 4 : 0);
#define V4_ARGS tab, kijs, kijl, fl_out, wvprpt, ff, intf, mij, xllws, fin, w2n, a->gfast, a->gfast_k, nullptr, adv, s
  return v4_for_shape(NANG, r1, r2, nh, [&](auto sh) {
    using S = decltype(sh);
    auto run = [&](auto adv_c) -> int {
      constexpr int ADV = decltype(adv_c)::value;
      if constexpr (v4_adv_built<T, S, ADV>)
        return v == Implsch4Variant::B ? launch4<T, S, true, false, false, false, V4_STEP, ADV>(V4_ARGS) : launch4<T, S, false, false, false, false, V4_STEP, ADV>(V4_ARGS);
      return -1;
    };
    switch (form) {
      case 1: return run(std::integral_constant<int, 1>{});
      case 5: return run(std::integral_constant<int, 5>{});
      case 3: return run(std::integral_constant<int, 3>{});
      default: return run(std::integral_constant<int, 7>{});
    }
  });
#undef V4_ARGS
}
template int launch_implsch4_adv<float>(const void*, int, int, void*, const void*, void*, void*, int*, void*, void*, double*, const Implsch4AdvArgs*, int, int, int, int, int, Implsch4Variant, hipStream_t);
template int launch_implsch4_adv<double>(const void*, int, int, void*, const void*, void*, void*, int*, void*, void*, double*, const Implsch4AdvArgs*, int, int, int, int, int, Implsch4Variant, hipStream_t);
// the forms of the one-kernel step this library holds for a direction count: bit 0 the plain step, bit 1 fast-wave sub-steps (compact input
// rows), bit 2 sub-grid obstructions (ecwam_hip_propags2_implsch_supported)
template <typename T, typename S>
constexpr int v4_adv_forms = (v4_adv_built<T, S, 1> ? 1 : 0) | (v4_adv_built<T, S, 3> ? 2 : 0) | (v4_adv_built<T, S, 5> ? 4 : 0);
int implsch4_adv_forms(int NANG, int real_bytes) {
  const int forms = v4_for_nang(NANG, [&](auto sh) { return real_bytes == 4 ? v4_adv_forms<float, decltype(sh)> : v4_adv_forms<double, decltype(sh)>; });
  return forms < 0 ? 0 : forms;
}
