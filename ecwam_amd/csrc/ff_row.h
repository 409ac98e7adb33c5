// A row of ff / intf in registers, shared by the point-wise kernels that read and write it in whole 16-byte pieces (forcing.hip, restart.hip).
#pragma once
#include <hip/hip_runtime.h>

// columns of ff and intf
enum { F_AIRD = 0, F_WDWAVE, F_CICOVER, F_WSWAVE, F_WSTAR, F_USTRA, F_VSTRA, F_UFRIC, F_TAUW, F_TAUWDIR, F_Z0M, F_Z0B, F_CHRNCK, F_CITHICK };
enum { I_WSEMEAN = 0, I_WSFMEAN, I_USTOKES, I_VSTOKES, I_TAUOCXD = 7, I_TAUOCYD, I_TAUICX = 10, I_TAUICY, I_PHIOCD };
constexpr unsigned col(int c) { return 1u << c; }

template <typename T>
struct FfRow {
  static constexpr int VEC = 16 / (int)sizeof(T), NP = 16 / VEC;
  typedef T VT __attribute__((ext_vector_type(VEC)));
  T v[16];
  static constexpr unsigned piece(int p) { return ((1u << VEC) - 1u) << (p * VEC); }
  // the pieces that hold a column of M
  template <unsigned M>
  __device__ __forceinline__ void load(const T* __restrict__ row) {
#pragma unroll
    for (int p = 0; p < NP; p++)
      if (M & piece(p)) {
        const VT x = *reinterpret_cast<const VT*>(row + p * VEC);
#pragma unroll
        for (int i = 0; i < VEC; i++) v[p * VEC + i] = x[i];
      }
  }
  // the pieces that hold a column of R, and those that hold a column of W beside one that is not in W (which the store must give back)
  template <unsigned R, unsigned W>
  __device__ __forceinline__ void load_for(const T* __restrict__ row) {
    constexpr unsigned need = R | kept(W);
    load<need>(row);
  }
  static constexpr unsigned kept(unsigned W) {
    unsigned m = 0;
    for (int p = 0; p < NP; p++)
      if ((W & piece(p)) && (W & piece(p)) != piece(p)) m |= piece(p);
    return m;
  }
  template <unsigned M>
  __device__ __forceinline__ void store(T* __restrict__ row) const {
#pragma unroll
    for (int p = 0; p < NP; p++)
      if (M & piece(p)) {
        VT x;
#pragma unroll
        for (int i = 0; i < VEC; i++) x[i] = v[p * VEC + i];
        *reinterpret_cast<VT*>(row + p * VEC) = x;
      }
  }
};
