// The forcing of a stand-alone run on the device (include/ecwam_hip_readwind.h): what READWIND and CURRENT2WAM do with decoded GRIB messages.
//   k_grib2wgrid   GRIB2WGRID's rearrangement or interpolation of VALUES (grib2wgrid.F90:783-1130) through the per-cell table of
//                  ecwam_hip_set_input_grid, followed per field by READWIND's rule for the plane it fills (readwind.F90:341-494)
//   k_current2wam  the three statements of CURRENT2WAM per component (current2wam.F90:253-259, 270-276), with KUPDATE as k_getcurr writes it
// One thread per cell (k_current2wam: per sea point).  k_grib2wgrid is a gather: a cell's table is one 16-byte load of its four positions and one
// (single) or two (double precision) 16-byte loads of the weights with the kind beside them, read once for all the fields of the launch; the four
// corner values of a field are independent loads, all issued before the first is used, and those of the next field are issued before the arithmetic
// of the current one.  The positions were validated on the host; a position of -1 (a padded row) loads nothing and is PMISS.  The stores of a
// plane are those of neighbouring threads to neighbouring cells.  The arithmetic keeps the reference's order, without contraction; the division of
// the mean is the compiler's correctly rounded one.
#include "../../include/ecwam_hip_readwind.h"
#include "dev.h"
#include "launch.h"

template <typename T> struct alignas(16) G2wWeights { T dk1, dii1, diip1, kind; };      // the kind (0, 1, 2) as a real, so that the record is whole pieces

template <typename T>
struct G2wPar {
  int nfld;
  signed char target[ECWAM_HIP_G2W_MAXFLD];
  unsigned char flags[ECWAM_HIP_G2W_MAXFLD];
  T roair, wstar0, pmiss, rad, deg;
};

template <typename T> struct G2wCorners { T a, b, c, d; };

// the four corners of one field; without INTERPOL only the first is read
template <typename T, bool INTERPOL>
__device__ __forceinline__ G2wCorners<T> g2w_gather(const T* __restrict__ v, const int4 p, const T pm) {
  G2wCorners<T> r;
  r.a = p.x >= 0 ? v[p.x] : pm;
  if constexpr (INTERPOL) {
    r.b = p.y >= 0 ? v[p.y] : pm;
    r.c = p.z >= 0 ? v[p.z] : pm;
    r.d = p.w >= 0 ? v[p.w] : pm;
  } else {
    r.b = r.c = r.d = r.a;
  }
  return r;
}

template <typename T, bool INTERPOL>
__global__ void __launch_bounds__(256) k_grib2wgrid(int ncell, const int4* __restrict__ pos, const G2wWeights<T>* __restrict__ wgt, const T* __restrict__ values,
                                                    size_t vstride, T* __restrict__ out, size_t ld, T* __restrict__ fieldg, size_t ncell_in, const G2wPar<T> a) {
#pragma clang fp contract(off)
  const int c = (int)(blockIdx.x * 256 + threadIdx.x);
  if (c >= ncell) return;
  const int4 p = pos[c];
  const G2wWeights<T> w = wgt[c];
  const int kind = (int)w.kind;
  const T pm = a.pmiss;
  const bool go = kind == 2;      // the other cells read nothing
  const int4 pg = go ? p : make_int4(-1, -1, -1, -1);
  const T dk1 = w.dk1, dk2 = T(1) - dk1, dii1 = w.dii1, dii2 = T(1) - dii1, diip1 = w.diip1, diip2 = T(1) - diip1;
  const bool top = dk1 <= T(0.5);
  const bool first = top ? dii1 <= T(0.5) : diip1 <= T(0.5);      // KCL, ICL of grib2wgrid.F90:1049-1057
  G2wCorners<T> nx = g2w_gather<T, INTERPOL>(values, pg, pm);
  for (int f = 0; f < a.nfld; f++) {
    const G2wCorners<T> v = nx;
    if (f + 1 < a.nfld) nx = g2w_gather<T, INTERPOL>(values + vstride * (size_t)(f + 1), pg, pm);
    const int target = a.target[f], flags = a.flags[f];
    T field = pm;
    if (go) {
      if constexpr (!INTERPOL) {
        field = v.a;
      } else {
        const bool dir = flags & ECWAM_HIP_G2W_DIRFLD;
        // WORK(.,.,1) and WORK(.,.,2): a direction's sine and cosine, PMISS kept (grib2wgrid.F90:895-908)
        T s0 = v.a, s1 = v.b, s2 = v.c, s3 = v.d, c0 = pm, c1 = pm, c2 = pm, c3 = pm;
        if (dir) {
          if (v.a != pm) { s0 = sin(a.rad * v.a); c0 = cos(a.rad * v.a); }
          if (v.b != pm) { s1 = sin(a.rad * v.b); c1 = cos(a.rad * v.b); }
          if (v.c != pm) { s2 = sin(a.rad * v.c); c2 = cos(a.rad * v.c); }
          if (v.d != pm) { s3 = sin(a.rad * v.d); c3 = cos(a.rad * v.d); }
        }
        const bool m0 = s0 == pm, m1 = s1 == pm, m2 = s2 == pm, m3 = s3 == pm;
        if (m0 || m1 || m2 || m3) {
          const T ns = top ? (first ? s0 : s1) : (first ? s2 : s3);
          const T nc = top ? (first ? c0 : c1) : (first ? c2 : c3);
          field = dir ? (nc != pm ? a.deg * atan2(ns, nc) : pm) : ns;
          if ((flags & ECWAM_HIP_G2W_NONWAVE) && field == pm) {
            T sum = T(0);
            sum = m0 ? sum : sum + s0;
            sum = m1 ? sum : sum + s1;
            sum = m2 ? sum : sum + s2;
            sum = m3 ? sum : sum + s3;
            const int ncount = 4 - (int)m0 - (int)m1 - (int)m2 - (int)m3;
            field = ncount > 0 ? sum / T(ncount) : sum;
          }
        } else {
          const T wk1 = dk2 * (dii2 * s0 + dii1 * s1) + dk1 * (diip2 * s2 + diip1 * s3);
          if (dir) {
            const T wk2 = dk2 * (dii2 * c0 + dii1 * c1) + dk1 * (diip2 * c2 + diip1 * c3);
            field = a.deg * atan2(wk1, wk2);
          } else {
            field = wk1;
          }
        }
      }
    }
    if (target == ECWAM_HIP_G2W_FIELD) {
      out[ld * (size_t)f + c] = field;
    } else if (kind != 0) {      // READWIND's loops end at NLONRGG_LOC(JSN)
      const bool miss = field == pm;
      T r = field;
      if (target == ECWAM_HIP_FG_WSWAVE) r = miss ? T(0) : field;
      else if (target == ECWAM_HIP_FG_WDWAVE) r = miss ? T(0) : a.rad * (field - T(180));
      else if (target == ECWAM_HIP_FG_AIRD) r = miss ? a.roair : field;
      else if (target == ECWAM_HIP_FG_WSTAR) r = miss ? a.wstar0 : field;
      fieldg[ncell_in * (size_t)target + c] = r;
    }
  }
}

// SIGN(MIN(ABS(x), CURRENT_MAX), x) after the two tests of CURRENT2WAM
template <typename T>
__device__ __forceinline__ T c2w_rule(T u, T wlowest, T zmiss) {
  if (fabs(u) <= wlowest) u = T(0);
  if (u <= zmiss) u = T(0);
  return copysign(fmin(fabs(u), T(1.5)), u);
}

template <typename T>
__global__ void __launch_bounds__(256) k_current2wam(int kijs, int kijl, const int* __restrict__ map, const T* __restrict__ field_u, const T* __restrict__ field_v,
                                                     T wlowest, T zmiss, T* __restrict__ ucur, T* __restrict__ vcur, int* __restrict__ changed) {
  const int ij = kijs + (int)(blockIdx.x * 256 + threadIdx.x);
  if (ij >= kijl) return;
  const int cell = map[ij];
  bool diff = false;
  if (field_u) {
    const T u = c2w_rule(field_u[cell], wlowest, zmiss);
    diff = diff || u != ucur[ij];
    ucur[ij] = u;
  }
  if (field_v) {
    const T v = c2w_rule(field_v[cell], wlowest, zmiss);
    diff = diff || v != vcur[ij];
    vcur[ij] = v;
  }
  // KUPDATE: every lane that sees a change stores the same 1 (an ordinary store: no atomic, no reduction)
  if (changed && diff) *changed = 1;
}

template <typename T>
void launch_grib2wgrid(int ncell, const void* pos, const void* wgt, int interpol, const void* values, size_t vstride, int nfld, const ecwam_hip_g2w_field* desc,
                       double roair, double wstar0, double pmiss, void* out, size_t ld, void* fieldg, size_t ncell_in, hipStream_t s) {
  if (ncell <= 0) return;
  G2wPar<T> a = {};
  a.nfld = nfld;
  for (int f = 0; f < nfld; f++) {
    a.target[f] = (signed char)desc[f].target;
    a.flags[f] = (unsigned char)desc[f].flags;
  }
  a.roair = T(roair);
  a.wstar0 = T(wstar0);
  a.pmiss = T(pmiss);
  a.rad = T(4) * std::atan(T(1)) / T(180);      // grib2wgrid.F90:194-195
  a.deg = T(1) / a.rad;
  const dim3 grid((unsigned)((ncell + 255) / 256));
  if (interpol)
    hipLaunchKernelGGL((k_grib2wgrid<T, true>), grid, dim3(256), 0, s, ncell, (const int4*)pos, (const G2wWeights<T>*)wgt, (const T*)values, vstride, (T*)out, ld,
                       (T*)fieldg, ncell_in, a);
  else
    hipLaunchKernelGGL((k_grib2wgrid<T, false>), grid, dim3(256), 0, s, ncell, (const int4*)pos, (const G2wWeights<T>*)wgt, (const T*)values, vstride, (T*)out, ld,
                       (T*)fieldg, ncell_in, a);
}
template <typename T>
void launch_current2wam(int kijs, int kijl, const int* map, const void* field_u, const void* field_v, double wlowest, double zmiss, void* ucur, void* vcur,
                        int* changed, hipStream_t s) {
  if (kijl <= kijs || (!field_u && !field_v)) return;
  hipLaunchKernelGGL((k_current2wam<T>), dim3((unsigned)((kijl - kijs + 255) / 256)), dim3(256), 0, s, kijs, kijl, map, (const T*)field_u, (const T*)field_v,
                     T(wlowest), T(zmiss), (T*)ucur, (T*)vcur, changed);
}

#define READWIND_INSTANTIATE(T)                                                                                                                                  \
  template void launch_grib2wgrid<T>(int, const void*, const void*, int, const void*, size_t, int, const ecwam_hip_g2w_field*, double, double, double, void*,   \
                                     size_t, void*, size_t, hipStream_t);                                                                                        \
  template void launch_current2wam<T>(int, int, const int*, const void*, const void*, double, double, void*, void*, int*, hipStream_t);
READWIND_INSTANTIATE(float)
READWIND_INSTANTIATE(double)
#undef READWIND_INSTANTIATE
