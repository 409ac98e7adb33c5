// Decoded GRIB spectra and READFL's record into FL1 on the device (include/ecwam_hip_gribin.h): k_outspec_tile of gribout.hip run backwards.
//   k_getspec_tile   field vectors values[f][ival[ij]] (GETSPEC's GRIB read on one task: grib2wgrid.F90:764-802 + getspec.F90:454-463, 541-557) or
//                    block vectors blk[f][ij] (the receiving half on many tasks, getspec.F90:602-619; the record of readfl.F90) -> FL1 rows [K][M],
//                    with the un-scaling 10**(v - |PPREC|) - PPEPS and ZMISS -> EPSMIN on the way
// One launch per call, on the caller's stream, no allocation, no wait.
//
// The transposition.  A field holds one real of every point; a point's row wants NANG runs of NFRE reals.  A block takes a tile of 64 points and
// ONE 16-byte piece (4 single or 2 double precision frequencies) of each direction: NANG VEC field columns in, lanes along consecutive points
// (the cells of consecutive points are consecutive within a latitude row, so the gather through the map coalesces), each value transformed and
// written into an LDS tile [64][NANG VEC | 1] -- the odd pitch of the outbound kernel: the transposed write, lanes along the points, hits 32
// different banks -- and 64 x NANG pieces out, every lane storing whole 16-byte pieces of FL1 rows.  A piece whose frequencies are not all inside
// the field range (its edges, and NFRE_RED where it is no multiple of VEC) is stored element by element, so that what lies outside the range keeps
// its bits.  The pieces of one row lie 16 bytes apart in memory, so the blocks that write the other pieces of a tile are numbered to run on the
// same XCD one after the other (blocks go to the XCDs round robin): the partial lines of a row meet in that XCD's L2 before they leave it.
#include "../../include/ecwam_hip_gribin.h"
#include "launch.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int TILE = 64, NTHR = 256, NWAVE = NTHR / 64, NXCD = 8;

// 10**x in the working precision; single precision through the double precision function, rounded once (as the LOG10 of gribout.hip)
__device__ __forceinline__ float g_pow10(float x) { return (float)pow(10.0, (double)x); }
__device__ __forceinline__ double g_pow10(double x) { return pow(10.0, x); }

template <typename T>
struct GetspecPar {
  T zmiss, ppeps, absprec, epsmin;
  int unscale, missing;
};

// grib2wgrid.F90:771-775, then getspec.F90:550-552
template <typename T>
__device__ __forceinline__ T decoded(T v, const GetspecPar<T>& a) {
#pragma clang fp contract(off)
  if (a.unscale && v != a.zmiss) v = g_pow10(v - a.absprec) - a.ppeps;
  if (a.missing && v == a.zmiss) v = a.epsmin;
  return v;
}

// MAP: element (f, ij) is src[(f - ifld0) stride + ival[ij]]; otherwise src[(f - ifld0) stride + ij].  Frequencies below mlim only.
template <typename T, bool MAP>
__global__ void __launch_bounds__(NTHR) k_getspec_tile(const T* __restrict__ src, long long stride, const int* __restrict__ ival, int kijs, int kijl, int ifld0, int ifld1,
                                                       int NANG, int NFRE, int mlim, int p_lo, int ny, int ntiles, const GetspecPar<T> a, T* __restrict__ fl1) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ncol = NANG * VEC, P = ncol | 1;
  T* __restrict__ tile = reinterpret_cast<T*>(smem);      // [TILE][P]
  // blocks b, b + 8, b + 16 ... run on one XCD: they take the ny pieces of one tile, then those of the tile 8 further on
  const int b = (int)blockIdx.x, j = b / NXCD, t = (j / ny) * NXCD + b % NXCD, p = p_lo + j % ny;
  if (t >= ntiles) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ij0 = kijs + t * TILE, npt = kijl - ij0 < TILE ? kijl - ij0 : TILE;
  if (lane < npt) {
    const int ij = ij0 + lane;
    const long long at = MAP ? (long long)ival[ij] : (long long)ij;
    for (int c = wave; c < ncol; c += NWAVE) {
      const int k = c / VEC, m = p * VEC + c % VEC, f = m * NANG + k;
      if (m >= mlim || f < ifld0 || f >= ifld1) continue;      // the same for the whole wave
      tile[lane * P + c] = decoded(src[(long long)(f - ifld0) * stride + at], a);
    }
  }
  __syncthreads();
  for (int idx = tid; idx < npt * NANG; idx += NTHR) {
    const int pt = idx / NANG, k = idx - pt * NANG;
    const T* __restrict__ col = tile + pt * P + k * VEC;
    T* __restrict__ row = fl1 + ((size_t)(ij0 + pt) * NANG + k) * NFRE + p * VEC;
    // the frequencies of the piece that the call writes for this direction: a run [i0, i1)
    int i0 = VEC, i1 = 0;
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      const int m = p * VEC + i, f = m * NANG + k;
      if (m < mlim && f >= ifld0 && f < ifld1) {
        i0 = i < i0 ? i : i0;
        i1 = i + 1;
      }
    }
    if (i0 == 0 && i1 == VEC) {
      VT x;
#pragma unroll
      for (int i = 0; i < VEC; i++) x[i] = col[i];
      *reinterpret_cast<VT*>(row) = x;
    } else {
      for (int i = i0; i < i1; i++) row[i] = col[i];      // f grows with the frequency: the elements inside the range are one run
    }
  }
}

}  // namespace

template <typename T>
int launch_getspec_fields(int kijs, int kijl, const void* src, long long stride, const int* ival, int ifld0, int nfld, int flags, const ecwam_hip_grib_opts* o,
                          double epsmin, void* fl1, int NANG, int NFRE, int mlim, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (kijl <= kijs) return 0;
  if (NFRE % VEC != 0) return -1;
  const int ncol = NANG * VEC;
  const size_t lds = (size_t)TILE * (ncol | 1) * sizeof(T);
  if (lds > 64 * 1024) return 1;
  GetspecPar<T> a = {};
  a.unscale = (flags & ECWAM_HIP_GETSPEC_UNSCALE) != 0;
  a.missing = (flags & ECWAM_HIP_GETSPEC_MISSING) != 0;
  a.epsmin = T(epsmin);
  if (flags) a.zmiss = T(o->zmiss);
  if (a.unscale) {
    a.ppeps = T(o->ppeps);
    a.absprec = std::fabs(T(o->pprec));
  }
  const int m_lo = ifld0 / NANG, m_hi = (ifld0 + nfld - 1) / NANG + 1;      // the frequencies of the field range
  const int p_lo = m_lo / VEC, ny = (m_hi + VEC - 1) / VEC - p_lo;
  const int ntiles = (kijl - kijs + TILE - 1) / TILE;
  const unsigned nblk = (unsigned)((ntiles + NXCD - 1) / NXCD) * NXCD * (unsigned)ny;
  if (ival)
    hipLaunchKernelGGL((k_getspec_tile<T, true>), dim3(nblk), dim3(NTHR), lds, s, (const T*)src, stride, ival, kijs, kijl, ifld0, ifld0 + nfld, NANG, NFRE, mlim, p_lo, ny,
                       ntiles, a, (T*)fl1);
  else
    hipLaunchKernelGGL((k_getspec_tile<T, false>), dim3(nblk), dim3(NTHR), lds, s, (const T*)src, stride, ival, kijs, kijl, ifld0, ifld0 + nfld, NANG, NFRE, mlim, p_lo, ny,
                       ntiles, a, (T*)fl1);
  return 0;
}

template int launch_getspec_fields<float>(int, int, const void*, long long, const int*, int, int, int, const ecwam_hip_grib_opts*, double, void*, int, int, int, hipStream_t);
template int launch_getspec_fields<double>(int, int, const void*, long long, const int*, int, int, int, const ecwam_hip_grib_opts*, double, void*, int, int, int, hipStream_t);
