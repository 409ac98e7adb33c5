// GRIB-ready spectra and parameter fields on the device (include/ecwam_hip_gribout.h): from FL1 and BOUT to the vector VALUES of the encoder.
//   k_outspec_tile   OUTSPEC's ice mask (outspec.F90:96-118) and the transposition of FL1 rows [K][M] into fields f = M NANG + K: either straight
//                    to VALUES through the map (outwspec.F90:219-227 + wgribencode_values.F90:152-178: scatter, LOG10, per-field maximum) or to the
//                    field-major send buffer (outwspec.F90:186-195)
//   k_grib_scatter   the same scatter from block vectors (MAKEGRID, or the receiving half of OUTWSPEC)
//   k_grib_fill      the cells no row fills, and the start value of the maxima
//   k_grib_pole      the pole padding (wgribencode_values.F90:103-148), from the source values, in the reference's order of summation
//   k_grib_thresh    PPMIN and the threshold to missing (wgribencode_values.F90:186-196)
// The launch sequence of a call: fill, tile / scatter, pole, thresh -- on one stream, no allocation, no wait.
//
// The transposition.  A point's row is NANG runs of NFRE reals; a field wants one real of every point.  A block takes a tile of 64 points and ONE
// 16-byte piece (4 single or 2 double precision frequencies) of each direction: 64 x NANG pieces through an LDS tile [64][NANG VEC | 1] (an odd
// pitch: the transposed read, lanes along the points, then hits 32 different banks; a pitch that is a multiple of 64 dwords would put all lanes
// on one), and NANG VEC field columns out, lanes along consecutive points, whose cells are consecutive within a latitude row.  Only the pieces
// that hold a frequency of the field range below NFRE_RED are loaded.  The pieces of one row lie 16 bytes apart in memory, so the blocks that
// take the other pieces of a tile are numbered to run on the same XCD one after the other (blocks go to the XCDs round robin): the lines one of
// them fetched serve the others from that XCD's L2.  A block walks several tiles and keeps the running maximum of each of its columns in LDS;
// at the end it issues one vector atomic per column on the order-preserving integer image of the real.
#include "../../include/ecwam_hip_gribout.h"
#include "launch.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int TILE = 64, NTHR = 256, NWAVE = NTHR / 64, NXCD = 8;

// the order-preserving integer image of a real: a < b  <=>  enc(a) < enc(b)
__device__ __forceinline__ unsigned enc(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ unsigned long long enc(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec(unsigned long long k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k)); }
template <typename T> struct KeyOf { typedef unsigned type; };
template <> struct KeyOf<double> { typedef unsigned long long type; };

// LOG10 in the working precision; single precision through the double precision function, rounded once
__device__ __forceinline__ float g_log10(float x) { return (float)log10((double)x); }
__device__ __forceinline__ double g_log10(double x) { return log10(x); }
__device__ __forceinline__ float g_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double g_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float g_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double g_min(double a, double b) { return fmin(a, b); }

template <typename T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = g_max(x, __shfl_xor(x, o, 64));
  return x;
}

template <typename T>
struct GribPar {
  T zmiss, ppeps, absprec, zminspec, ppmiss, deltapp, ppmin_reset;
  int spectral;
};

__device__ __forceinline__ bool in_pole(const GribMapDev& g, int c) {
  return (unsigned)(c - g.north.pole0) < (unsigned)g.north.npole || (unsigned)(c - g.south.pole0) < (unsigned)g.south.npole;
}

// step 3: LOG10(v + PPEPS) + |PPREC|, or ZMINSPEC for a missing value
template <typename T>
__device__ __forceinline__ T log_scale(T v, const GribPar<T>& a) {
#pragma clang fp contract(off)
  return v != a.zmiss ? g_log10(v + a.ppeps) + a.absprec : a.zminspec;
}

// outspec.F90:101-115
template <typename T>
__device__ __forceinline__ T ice_masked(T v, T zmask, T flmin) {
#pragma clang fp contract(off)
  return (T(1) - zmask) * v + zmask * flmin;
}

// the sources of a field value before the scatter: FL1 with OUTSPEC's mask, or a block vector with strides
template <typename T>
struct SrcFl1 {
  const T* fl1;
  const T* ff;
  int NANG, NFRE, ifld0, ice;
  T cithrsh, flmin;
  __device__ __forceinline__ T get(int f, int ij) const {
    const int fa = f + ifld0, m = fa / NANG, k = fa - m * NANG;
    T v = fl1[((size_t)ij * NANG + k) * NFRE + m];
    if (ice) v = ice_masked(v, ff[(size_t)ij * ECWAM_HIP_NFF + 2] > cithrsh ? T(1) : T(0), flmin);
    return v;
  }
};
template <typename T>
struct SrcStrided {
  const T* src;
  long long fs, ps;
  __device__ __forceinline__ T get(int f, int ij) const { return src[(long long)f * fs + (long long)ij * ps]; }
};

// TO_VALUES: through the map into values[nfld][ntencode] with the logarithm and the maxima; otherwise into blk[nfld][ld] as the values stand
template <typename T, bool TO_VALUES>
__global__ void __launch_bounds__(NTHR) k_outspec_tile(const T* __restrict__ fl1, const T* __restrict__ ff, int kijs, int kijl, int ifld0, int ifld1, int NANG, int NFRE,
                                                       int NFRE_RED, int p_lo, int ny, int ngroups, int tpb, int ice, T cithrsh, T flmin, const GribMapDev g,
                                                       const GribPar<T> a, T* __restrict__ out, size_t ld, typename KeyOf<T>::type* __restrict__ keys) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ncol = NANG * VEC, P = ncol | 1;
  T* __restrict__ tile = reinterpret_cast<T*>(smem);      // [TILE][P]
  T* __restrict__ colmax = tile + (size_t)TILE * P;       // [ncol]
  // blocks b, b + 8, b + 16 ... run on one XCD: they take the ny pieces of one group of tiles, then those of the group 8 further on
  const int b = (int)blockIdx.x, j = b / NXCD, grp = (j / ny) * NXCD + b % NXCD, p = p_lo + j % ny;
  if (grp >= ngroups) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntiles = (kijl - kijs + TILE - 1) / TILE;
  if (TO_VALUES) {
    for (int c = tid; c < ncol; c += NTHR) colmax[c] = a.zminspec;
  }
  const int t1 = (grp + 1) * tpb < ntiles ? (grp + 1) * tpb : ntiles;
  for (int t = grp * tpb; t < t1; t++) {
    const int ij0 = kijs + t * TILE, npt = kijl - ij0 < TILE ? kijl - ij0 : TILE;
    __syncthreads();      // the tile of the previous turn has been read; colmax is set
    for (int idx = tid; idx < npt * NANG; idx += NTHR) {
      const int pt = idx / NANG, k = idx - pt * NANG;
      const VT x = *reinterpret_cast<const VT*>(fl1 + ((size_t)(ij0 + pt) * NANG + k) * NFRE + p * VEC);
#pragma unroll
      for (int i = 0; i < VEC; i++) tile[pt * P + k * VEC + i] = x[i];
    }
    __syncthreads();
    const bool valid = lane < npt;
    const int ij = ij0 + lane;
    T zmask = T(0);
    if (ice && valid) zmask = ff[(size_t)ij * ECWAM_HIP_NFF + 2] > cithrsh ? T(1) : T(0);
    int cell = 0;
    bool store = valid;
    if (TO_VALUES && valid) {
      cell = g.ival[ij];
      store = !in_pole(g, cell);      // a pole row is k_grib_pole's
    }
    for (int c = wave; c < ncol; c += NWAVE) {
      const int k = c / VEC, m = p * VEC + c % VEC, f = m * NANG + k;
      if (m >= NFRE_RED || f < ifld0 || f >= ifld1) continue;      // the same for the whole wave
      T v = valid ? tile[lane * P + c] : T(0);
      if (ice) v = ice_masked(v, zmask, flmin);
      if (TO_VALUES) {
        T x = a.zminspec;
        if (store) {
          x = log_scale(v, a);
          out[(size_t)(f - ifld0) * g.ntencode + cell] = x;
        }
        x = wave_max(x);
        if (lane == 0) colmax[c] = g_max(colmax[c], x);      // column c is this wave's alone
      } else if (valid) {
        out[(size_t)(f - ifld0) * ld + ij] = v;
      }
    }
  }
  if (TO_VALUES) {
    __syncthreads();
    for (int c = tid; c < ncol; c += NTHR) {
      const int k = c / VEC, m = p * VEC + c % VEC, f = m * NANG + k;
      if (m < NFRE_RED && f >= ifld0 && f < ifld1) atomicMax(&keys[f - ifld0], enc(colmax[c]));
    }
  }
}

// steps 1 and 4's start: the cells no row fills (those of a pole row excepted) hold the missing value; the maximum starts from ZMINSPEC
template <typename T>
__global__ void __launch_bounds__(NTHR) k_grib_fill(const GribMapDev g, const GribPar<T> a, T* __restrict__ values, typename KeyOf<T>::type* __restrict__ keys) {
  const int f = (int)blockIdx.y, t = (int)(blockIdx.x * NTHR + threadIdx.x);
  if (t < g.nunf) values[(size_t)f * g.ntencode + g.unfilled[t]] = a.spectral ? a.zminspec : a.zmiss;
  if (a.spectral && t == 0) keys[f] = enc(a.zminspec);
}

template <typename T, typename SRC>
__global__ void __launch_bounds__(NTHR) k_grib_scatter(int kijs, int kijl, const SRC src, const GribMapDev g, const GribPar<T> a, T* __restrict__ values,
                                                       typename KeyOf<T>::type* __restrict__ keys) {
  const int f = (int)blockIdx.y, ij = kijs + (int)(blockIdx.x * NTHR + threadIdx.x);
  T x = a.zminspec;
  if (ij < kijl) {
    const int cell = g.ival[ij];
    if (!in_pole(g, cell)) {
      const T v = src.get(f, ij);
      x = a.spectral ? log_scale(v, a) : v;
      values[(size_t)f * g.ntencode + cell] = x;
    }
  }
  if (a.spectral) {
    x = wave_max(x);
    if ((threadIdx.x & 63) == 0) atomicMax(&keys[f], enc(x));
  }
}

// One wave per field and pole.  Lane 0 sums the row beside the pole in the reference's order (wgribencode_values.F90:105-119, 127-141): the rows are
// short, and a serial sum is the same number as a same-precision restatement gives.  Rows outside [kijs,kijl) and land count as missing.
template <typename T, typename SRC>
__global__ void __launch_bounds__(64) k_grib_pole(int kijs, int kijl, const SRC src, const GribMapDev g, const GribPar<T> a, T* __restrict__ values,
                                                  typename KeyOf<T>::type* __restrict__ keys) {
#pragma clang fp contract(off)
  const int f = (int)blockIdx.y, south = (int)blockIdx.x, lane = (int)threadIdx.x;
  const ecwam_hip_grib_pole pl = south ? g.south : g.north;
  if (pl.npole == 0) return;
  const int* __restrict__ adj = g.adj + (south ? g.north.nadj : 0);
  T temp = T(0);
  if (lane == 0) {
    int nn = 0;
    for (int i = 0; i < pl.nadj; i++) {
      const int ij = adj[i];
      if (ij < kijs || ij >= kijl) continue;      // land (-1) or a row that is not part of the call
      const T v = src.get(f, ij);
      if (v != a.zmiss) {
        temp = temp + v;
        nn++;
      }
    }
    temp = nn > 0 ? temp / T(nn) : a.zmiss;
    if (a.spectral) {
      temp = log_scale(temp, a);
      atomicMax(&keys[f], enc(temp));
    }
  }
  temp = __shfl(temp, 0, 64);
  for (int i = lane; i < pl.npole; i += 64) values[(size_t)f * g.ntencode + pl.pole0 + i] = temp;
}

// steps 5 and 6 on the cells the call wrote: those of rows [kijs,kijl), those no row fills, the pole rows
template <typename T>
__global__ void __launch_bounds__(NTHR) k_grib_thresh(int kijs, int kijl, const GribMapDev g, const GribPar<T> a, T* __restrict__ values,
                                                      const typename KeyOf<T>::type* __restrict__ keys, T* __restrict__ ppmax_out) {
#pragma clang fp contract(off)
  const int f = (int)blockIdx.y;
  int t = (int)(blockIdx.x * NTHR + threadIdx.x);
  const T ppmax = dec(keys[f]);
  if (t == 0 && ppmax_out) ppmax_out[f] = ppmax;
  const T ppmin = g_min(g_min(a.ppmiss, ppmax - a.deltapp), a.ppmin_reset);
  int cell;
  if (t < kijl - kijs) {
    cell = g.ival[kijs + t];
    if (in_pole(g, cell)) return;
  } else if ((t -= kijl - kijs) < g.nunf) {
    cell = g.unfilled[t];
  } else if ((t -= g.nunf) < g.north.npole) {
    cell = g.north.pole0 + t;
  } else if ((t -= g.north.npole) < g.south.npole) {
    cell = g.south.pole0 + t;
  } else {
    return;
  }
  T* __restrict__ v = values + (size_t)f * g.ntencode + cell;
  if (*v <= ppmin) *v = a.zmiss;
}

template <typename T>
GribPar<T> make_par(const ecwam_hip_grib_opts& o, int spectral) {
  GribPar<T> a = {};
  a.zmiss = T(o.zmiss);
  a.spectral = spectral;
  if (spectral) {
    a.ppeps = T(o.ppeps);
    a.absprec = std::fabs(T(o.pprec));
    a.zminspec = std::log10(a.ppeps) + a.absprec;
    a.ppmiss = T(o.ppmiss);
    a.deltapp = T((1 << o.ngrbress) - 1) * T(o.ppresol);
    a.ppmin_reset = T(o.ppmin_reset);
  }
  return a;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n > 0 ? n : 1) + NTHR - 1) / NTHR; }

// 0 = launched, 1 = the tile does not fit the LDS, -1 = NFRE is no whole number of 16-byte pieces
template <typename T, bool TO_VALUES>
int tile_go(int kijs, int kijl, const void* fl1, const void* ff, int ifld0, int nfld, int ice, double cithrsh, double flmin, const GribMapDev& g, const GribPar<T>& a, void* out,
            size_t ld, void* keys, int NANG, int NFRE, int NFRE_RED, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  const int ncol = NANG * VEC;
  const size_t lds = ((size_t)TILE * (ncol | 1) + ncol) * sizeof(T);
  if (lds > 64 * 1024) return 1;
  const int m_lo = ifld0 / NANG, m_hi = (ifld0 + nfld - 1) / NANG + 1;      // the frequencies of the field range
  const int p_lo = m_lo / VEC, ny = (m_hi + VEC - 1) / VEC - p_lo;
  const int ntiles = (kijl - kijs + TILE - 1) / TILE;
  long long tpb = (long long)ntiles * ny / 2048;      // enough blocks to fill the device, few enough that the atomics stay rare
  tpb = tpb < 1 ? 1 : tpb > 16 ? 16 : tpb;
  const int ngroups = (ntiles + (int)tpb - 1) / (int)tpb;
  const unsigned nblk = (unsigned)((ngroups + NXCD - 1) / NXCD) * NXCD * (unsigned)ny;
  hipLaunchKernelGGL((k_outspec_tile<T, TO_VALUES>), dim3(nblk), dim3(NTHR), lds, s, (const T*)fl1, (const T*)ff, kijs, kijl, ifld0, ifld0 + nfld, NANG, NFRE, NFRE_RED, p_lo,
                     ny, ngroups, (int)tpb, ice, T(cithrsh), T(flmin), g, a, (T*)out, ld, (typename KeyOf<T>::type*)keys);
  return 0;
}

template <typename T, typename SRC>
void finish_go(int kijs, int kijl, const SRC& src, int nfld, const GribMapDev& g, const GribPar<T>& a, void* values, void* ppmax, void* keys, hipStream_t s) {
  typedef typename KeyOf<T>::type K;
  if (g.north.npole || g.south.npole)
    hipLaunchKernelGGL((k_grib_pole<T, SRC>), dim3(2, (unsigned)nfld), dim3(64), 0, s, kijs, kijl, src, g, a, (T*)values, (K*)keys);
  if (a.spectral) {
    const long long cells = (long long)(kijl - kijs) + g.nunf + g.north.npole + g.south.npole;
    hipLaunchKernelGGL((k_grib_thresh<T>), dim3(blocks_of(cells), (unsigned)nfld), dim3(NTHR), 0, s, kijs, kijl, g, a, (T*)values, (const K*)keys, (T*)ppmax);
  }
}

}  // namespace

template <typename T>
int launch_outspec_values(int kijs, int kijl, const void* fl1, const void* ff, int ifld0, int nfld, int ice, double cithrsh, double flmin, const ecwam_hip_grib_opts& o,
                          const GribMapDev& g, void* values, void* ppmax, void* keys, int NANG, int NFRE, int NFRE_RED, hipStream_t s) {
  typedef typename KeyOf<T>::type K;
  if (kijl <= kijs) return 0;
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  if (((size_t)TILE * ((NANG * VEC) | 1) + NANG * VEC) * sizeof(T) > 64 * 1024) return 1;
  const GribPar<T> a = make_par<T>(o, 1);
  hipLaunchKernelGGL((k_grib_fill<T>), dim3(blocks_of(g.nunf), (unsigned)nfld), dim3(NTHR), 0, s, g, a, (T*)values, (K*)keys);
  tile_go<T, true>(kijs, kijl, fl1, ff, ifld0, nfld, ice, cithrsh, flmin, g, a, values, 0, keys, NANG, NFRE, NFRE_RED, s);
  const SrcFl1<T> src = {(const T*)fl1, (const T*)ff, NANG, NFRE, ifld0, ice, T(cithrsh), T(flmin)};
  finish_go<T>(kijs, kijl, src, nfld, g, a, values, ppmax, keys, s);
  return 0;
}

template <typename T>
int launch_outspec_pack(int kijs, int kijl, const void* fl1, const void* ff, int ifld0, int nfld, int ice, double cithrsh, double flmin, void* blk, int ld, int NANG, int NFRE,
                        int NFRE_RED, hipStream_t s) {
  if (kijl <= kijs) return 0;
  const GribMapDev none = {};
  const GribPar<T> a = {};
  return tile_go<T, false>(kijs, kijl, fl1, ff, ifld0, nfld, ice, cithrsh, flmin, none, a, blk, (size_t)ld, nullptr, NANG, NFRE, NFRE_RED, s);
}

template <typename T>
void launch_grib_values(int kijs, int kijl, const void* src, long long fstride, long long pstride, int nfld, int spectral, const ecwam_hip_grib_opts& o, const GribMapDev& g,
                        void* values, void* ppmax, void* keys, hipStream_t s) {
  typedef typename KeyOf<T>::type K;
  if (kijl <= kijs) return;
  const GribPar<T> a = make_par<T>(o, spectral);
  const SrcStrided<T> sr = {(const T*)src, fstride, pstride};
  hipLaunchKernelGGL((k_grib_fill<T>), dim3(blocks_of(g.nunf), (unsigned)nfld), dim3(NTHR), 0, s, g, a, (T*)values, (K*)keys);
  hipLaunchKernelGGL((k_grib_scatter<T, SrcStrided<T>>), dim3(blocks_of(kijl - kijs), (unsigned)nfld), dim3(NTHR), 0, s, kijs, kijl, sr, g, a, (T*)values, (K*)keys);
  finish_go<T>(kijs, kijl, sr, nfld, g, a, values, ppmax, keys, s);
}

#define GRIBOUT_INSTANTIATE(T)                                                                                                                                          \
  template int launch_outspec_values<T>(int, int, const void*, const void*, int, int, int, double, double, const ecwam_hip_grib_opts&, const GribMapDev&, void*, void*, \
                                        void*, int, int, int, hipStream_t);                                                                                             \
  template int launch_outspec_pack<T>(int, int, const void*, const void*, int, int, int, double, double, void*, int, int, int, int, hipStream_t);                       \
  template void launch_grib_values<T>(int, int, const void*, long long, long long, int, int, const ecwam_hip_grib_opts&, const GribMapDev&, void*, void*, void*,        \
                                      hipStream_t);
GRIBOUT_INSTANTIATE(float)
GRIBOUT_INSTANTIATE(double)
#undef GRIBOUT_INSTANTIATE
