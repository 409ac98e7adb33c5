// Nested-grid boundary spectra on the device: the two calls of WAMODEL between the time step and the output (wamodel.F90:333-343).
//   k_bouinpt  BOUINPT's loop over the boundary points of a limited-area run (bouinpt.F90:385-424) with Hasselmann's spectrum interpolation
//              (intspec.F90:107-229, rotspec.F90:69-86, strspec.F90:70-175): the coarse model's spectra go into FL1
//   k_outbc    OUTBC's mean parameters and point spectra for the boundary file of a finer model (outbc.F90:78-91 with FEMEAN and STHQ)
// Neither is part of the time step; they run on the order of 10^3 points per step.
#include "outbs_point.h"
#include "launch.h"

// INT(x) of the reference where x may be anything (a mean frequency of zero, negative or not finite makes GAMMA so): 0 instead of an
// undefined conversion.  The values of such a point are unspecified, its memory accesses are not.
template <typename T>
__device__ __forceinline__ int nest_int(T x) {
  return (x > T(-1.0e9) && x < T(1.0e9)) ? (int)x : 0;
}
__device__ __forceinline__ int nest_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// b**n with an integer n (strspec.F90:90: 1.1**INC), by squaring
template <typename T>
__device__ __forceinline__ T nest_powi(T b, int n) {
#pragma clang fp contract(off)
  unsigned e = n < 0 ? 0u - (unsigned)n : (unsigned)n;
  T r = T(1);
  while (e) {
    if (e & 1u) r = r * b;
    b = b * b;
    e >>= 1;
  }
  return n < 0 ? T(1) / r : r;
}

// ROTSPEC's per-call scalars (rotspec.F90:69-75): the shift in whole bins and the weight of the second tap
template <typename T>
__device__ __forceinline__ void nest_rot(T rthet, int NANG, T ZPI, int& inc, T& adif) {
#pragma clang fp contract(off)
  T fth = fmod(rthet + ZPI, ZPI);
  fth = fth * T(NANG) / ZPI;
  inc = nest_int(fth);
  adif = fth - T(inc);
  inc = nest_clamp(inc, 0, NANG);
}

enum { NEST_COPY = 0, NEST_ONLY2, NEST_ONLY1, NEST_FULL };      // BFW <= 0; EMEAN1 == 0; EMEAN2 == 0; both spectra carry energy
enum { STR_NONE = 0, STR_SHIFT, STR_INTERP };                   // GAMMA == 1; Z <= 0.001; else

// One wavefront (= one block) per boundary point.  The two coarse spectra arrive in the order of the file's records, [M][K], and are staged
// in LDS in the device layout [K][M]; every output bin is then two direction taps (ROTSPEC) times two frequency taps (STRSPEC) per source.
// A thread owns 16 bytes of the result, (direction K, frequencies M .. M + VEC - 1), as in k_setice.  The arithmetic of a bin is the
// reference's, in its order and without contraction: rotate, stretch, scale by EMEAN / EMEAN1, blend.
template <typename T>
__global__ void __launch_bounds__(64) k_bouinpt(const DevTab<T>* __restrict__ tp, int kijs, int kijl, int nijb, const int* __restrict__ ijb,
                                                const int* __restrict__ ibcl, const int* __restrict__ ibcr, const T* __restrict__ bfw, int nboinp,
                                                const T* __restrict__ f1, const T* __restrict__ par1, T* __restrict__ fl1, T* __restrict__ par_out) {
#pragma clang fp contract(off)
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T VT __attribute__((ext_vector_type(VEC)));
  extern __shared__ __align__(16) unsigned char nest_smem[];
  const DevTab<T>& tb = *tp;
  const int lane = threadIdx.x, i = blockIdx.x;
  if (i >= nijb) return;
  const int ij = ijb[i];
  if (ij < kijs || ij >= kijl) return;      // the NSTART / NEND test of bouinpt.F90:138-145 (block-uniform: no thread waits at the barrier)
  const int NANG = tb.NANG, NFRE = tb.NFRE, N = NANG * NFRE;
  T* sF = reinterpret_cast<T*>(nest_smem);                        // [2][NANG][NFRE]
  T* sWA = sF + 2 * N;                                            // [2][NFRE] STRSPEC's ADIF
  T* sWB = sWA + 2 * NFRE;                                        // [2][NFRE] its BDIF
  int* sMC = reinterpret_cast<int*>(sWB + 2 * NFRE);              // [2][NFRE] the first frequency tap, 0-based; -1: the loops leave the bin zero

  // index 0 is the land point: spectrum and means zero, nothing read (an index outside 0 .. nboinp is taken for it)
  int ib[2] = {ibcl[i], ibcr[i]};
  T EM[2], TQ[2], FM[2];
  for (int s = 0; s < 2; s++) {
    if (ib[s] < 1 || ib[s] > nboinp) ib[s] = 0;
    const T* p = par1 + (size_t)(ib[s] > 0 ? ib[s] - 1 : 0) * 3;
    EM[s] = ib[s] ? p[0] : T(0);
    TQ[s] = ib[s] ? p[1] : T(0);
    FM[s] = ib[s] ? p[2] : T(0);
  }
  const T DEL1L = bfw[i];
  const int mode = !(DEL1L > T(0)) ? NEST_COPY : EM[0] == T(0) ? NEST_ONLY2 : EM[1] == T(0) ? NEST_ONLY1 : NEST_FULL;
  // stage what the mode reads
  for (int s = 0; s < 2; s++) {
    if ((mode == NEST_COPY || mode == NEST_ONLY1) && s == 1) continue;
    if (mode == NEST_ONLY2 && s == 0) continue;
    T* d = sF + s * N;
    if (ib[s]) {
      const T* g = f1 + (size_t)(ib[s] - 1) * N;
      for (int e = lane; e < N; e += 64) {
        const int mm = e / NANG, kk = e - mm * NANG;
        d[kk * NFRE + mm] = g[e];
      }
    } else {
      for (int e = lane; e < N; e += 64) d[e] = T(0);
    }
  }

  // INTSPEC's scalars (intspec.F90:107-161): DEL12 = 1
  const T GW1 = (T(1) - DEL1L) / T(1), GW2 = DEL1L / T(1);
  T EMEAN = EM[0], FMEAN = FM[0], THETM = TQ[0];                  // NEST_COPY: the left point's values pass through
  int rinc[2] = {0, 0}, sinc[2] = {0, 0}, smode[2] = {STR_NONE, STR_NONE}, sup[2] = {0, 0};
  T radif[2] = {T(0), T(0)}, escale[2] = {T(1), T(1)};
  if (mode == NEST_ONLY2) {
    EMEAN = GW2 * EM[1]; FMEAN = FM[1]; THETM = TQ[1];
  } else if (mode == NEST_ONLY1) {
    EMEAN = GW1 * EM[0]; FMEAN = FM[0]; THETM = TQ[0];
  } else if (mode == NEST_FULL) {
    EMEAN = GW1 * EM[0] + GW2 * EM[1];
    FMEAN = GW1 * FM[0] + GW2 * FM[1];
    const T CM = GW1 * m_cos(TQ[0]) + GW2 * m_cos(TQ[1]);
    const T SM = GW1 * m_sin(TQ[0]) + GW2 * m_sin(TQ[1]);
    THETM = m_atan2(SM, CM);
    THETM = fmod(THETM + tb.ZPI, tb.ZPI);
    const T ALO = m_log10(T(1.1));                                // the literal 1.1, not FRATIO (strspec.F90:80-81)
    for (int s = 0; s < 2; s++) {
      nest_rot(THETM - TQ[s], NANG, tb.ZPI, rinc[s], radif[s]);
      escale[s] = EMEAN / EM[s];
      const T GAMMA = FM[s] / FMEAN;
      if (GAMMA == T(1)) continue;
      const int INC = nest_int(m_log10(GAMMA) / ALO);
      const T Z = m_abs(nest_powi(T(1.1), INC) - GAMMA);
      smode[s] = (Z <= T(0.001)) ? STR_SHIFT : STR_INTERP;
      sup[s] = GAMMA > T(1);
      sinc[s] = nest_clamp(INC, -(NFRE + 1), NFRE + 1);           // beyond +-NFRE every loop of STRSPEC is empty
      if (lane < NFRE) {                                          // lane = M: the taps of output frequency M + 1 (strspec.F90:103-164)
        const int m1 = lane + 1, I = sinc[s];
        int mc = -1;
        T wa = T(0), wb = T(0);
        if (smode[s] == STR_SHIFT) {
          if (sup[s] ? (m1 <= NFRE - I) : (m1 >= 1 - I)) mc = m1 + I - 1;
        } else {
          if (sup[s] ? (m1 <= NFRE - I - 1) : (m1 >= 2 - I)) {
            const T AR2 = tb.FR[lane] * GAMMA;
            const int IFR = nest_clamp(nest_int(m_log10(AR2 / tb.FR[0]) / ALO + T(1)), 1, NFRE - 1);
            wa = (tb.FR[IFR] - AR2) / (tb.FR[IFR] - tb.FR[IFR - 1]);
            wb = T(1) - wa;
            mc = (sup[s] ? m1 + I : m1 + I - 1) - 1;
          }
        }
        if (mc >= 0) mc = nest_clamp(mc, 0, smode[s] == STR_SHIFT ? NFRE - 1 : NFRE - 2);
        sMC[s * NFRE + lane] = mc;
        sWA[s * NFRE + lane] = wa;
        sWB[s * NFRE + lane] = wb;
      }
    }
  }
  __syncthreads();

  const int NC = NFRE / VEC, per = NANG * NC;
  T* out = fl1 + (size_t)ij * N;
  for (int c = lane; c < per; c += 64) {
    const int k = c / NC, m0 = (c - k * NC) * VEC;
    VT o;
    if (mode == NEST_COPY || mode == NEST_ONLY1) {
      const T* p = sF + k * NFRE + m0;
#pragma unroll
      for (int v = 0; v < VEC; v++) o[v] = mode == NEST_COPY ? p[v] : GW1 * p[v];
    } else if (mode == NEST_ONLY2) {
      const T* p = sF + N + k * NFRE + m0;
#pragma unroll
      for (int v = 0; v < VEC; v++) o[v] = GW2 * p[v];
    } else {
      T f34[2][VEC];
      for (int s = 0; s < 2; s++) {
        // ROTSPEC's taps of direction K + 1 (rotspec.F90:78-81), 0-based
        int kc = k - rinc[s];
        if (kc < 0) kc += NANG;
        int kc1 = kc - 1;
        if (kc1 < 0) kc1 += NANG;
        const T* pa = sF + s * N + kc * NFRE;
        const T* pb = sF + s * N + kc1 * NFRE;
        const T ADIF = radif[s], BDIF = T(1) - ADIF;
#pragma unroll
        for (int v = 0; v < VEC; v++) {
          const int m = m0 + v;
          T x;
          if (smode[s] == STR_NONE) {
            x = BDIF * pa[m] + ADIF * pb[m];
          } else {
            const int mc = sMC[s * NFRE + m];
            if (mc < 0) {
              x = T(0);
            } else if (smode[s] == STR_SHIFT) {
              x = BDIF * pa[mc] + ADIF * pb[mc];
            } else {
              const T r0 = BDIF * pa[mc] + ADIF * pb[mc];
              const T r1 = BDIF * pa[mc + 1] + ADIF * pb[mc + 1];
              x = sWA[s * NFRE + m] * r0 + sWB[s * NFRE + m] * r1;
            }
          }
          f34[s][v] = x * escale[s];
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; v++) o[v] = GW1 * f34[0][v] + GW2 * f34[1][v];
    }
    *reinterpret_cast<VT*>(out + k * NFRE + m0) = o;
  }
  if (par_out && lane == 0) {
    T* p = par_out + (size_t)i * 3;
    p[0] = EMEAN; p[1] = THETM; p[2] = FMEAN;
  }
}

// One wavefront per point of the list: the tile of k_outbs, FEMEAN and STHQ through csrc/outbs_point.h (the same bits as ecwam_hip_outbs on
// the same spectrum), and the spectrum transposed into the order of the file's record, [M][K].  par == NULL: the gather alone.
template <typename T>
__global__ void __launch_bounds__(256) k_outbc(const DevTab<T>* __restrict__ tp, int nbc, const int* __restrict__ ijarc, const T* __restrict__ fl1,
                                               T* __restrict__ flpts, T* __restrict__ par) {
  extern __shared__ __align__(16) unsigned char nest_smem[];
  const DevTab<T>& tb = *tp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave;
  if (i >= nbc) return;  // wave-uniform, no block barrier below
  const int ij = ijarc[i];
  if (ij < 0) return;
  const int NANG = tb.NANG, NFRE = tb.NFRE, NAP = NANG | 1, N = NANG * NFRE;
  T* sF = reinterpret_cast<T*>(nest_smem) + (size_t)wave * NFRE * NAP;
  const T* g = fl1 + (size_t)ij * N;
  for (int e = lane; e < N; e += 64) {
    const int kk = e / NFRE, mm = e - kk * NFRE;
    sF[mm * NAP + kk] = g[e];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  T* d = flpts + (size_t)i * N;
  for (int e = lane; e < N; e += 64) {
    const int mm = e / NANG, kk = e - mm * NANG;
    d[e] = sF[mm * NAP + kk];
  }
  if (par) {
    T EM, FM, THQ;
    femean_sthq_point(tb, sF, lane, EM, FM, THQ);
    if (lane == 0) {
      T* p = par + (size_t)i * 3;
      p[0] = EM; p[1] = THQ; p[2] = FM;
    }
  }
}

static size_t bouinpt_lds(int NANG, int NFRE, size_t rb) { return (size_t)2 * NANG * NFRE * rb + (size_t)2 * NFRE * (2 * rb + sizeof(int)); }

template <typename T>
int launch_bouinpt(const void* tab, int kijs, int kijl, int nijb, const int* ijb, const int* ibcl, const int* ibcr, const void* bfw, int nboinp, const void* f1,
                   const void* par1, void* fl1, void* par_out, int NANG, int NFRE, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (NFRE % VEC != 0) return -1;
  if (bouinpt_lds(NANG, NFRE, sizeof(T)) > 64 * 1024 || NFRE > 64) return 1;
  if (nijb <= 0 || kijl - kijs <= 0) return 0;
  hipLaunchKernelGGL((k_bouinpt<T>), dim3((unsigned)nijb), dim3(64), bouinpt_lds(NANG, NFRE, sizeof(T)), s, (const DevTab<T>*)tab, kijs, kijl, nijb, ijb, ibcl,
                     ibcr, (const T*)bfw, nboinp, (const T*)f1, (const T*)par1, (T*)fl1, (T*)par_out);
  return 0;
}
template <typename T>
int launch_outbc(const void* tab, int nbc, const int* ijarc, const void* fl1, void* flpts, void* par, int NANG, int NFRE, hipStream_t s) {
  if (!outbs_size_ok(NANG, NFRE, sizeof(T))) return 1;
  if (nbc <= 0) return 0;
  const size_t shmem = (size_t)4 * NFRE * (NANG | 1) * sizeof(T);
  hipLaunchKernelGGL((k_outbc<T>), dim3((unsigned)((nbc + 3) / 4)), dim3(256), shmem, s, (const DevTab<T>*)tab, nbc, ijarc, (const T*)fl1, (T*)flpts, (T*)par);
  return 0;
}
template int launch_bouinpt<float>(const void*, int, int, int, const int*, const int*, const int*, const void*, int, const void*, const void*, void*, void*, int, int, hipStream_t);
template int launch_bouinpt<double>(const void*, int, int, int, const int*, const int*, const int*, const void*, int, const void*, const void*, void*, void*, int, int, hipStream_t);
template int launch_outbc<float>(const void*, int, const int*, const void*, void*, void*, int, int, hipStream_t);
template int launch_outbc<double>(const void*, int, const int*, const void*, void*, void*, int, int, hipStream_t);
