// Extreme-wave parameters of OUTBLOCK on the device: KURTOSIS (kurtosis.F90 with PEAK_ANG, AKI, TRANSF_BFI, STAT_NL, TRANSF_R and
// H_MAX; OUTBLOCK parameters 29-31, 33, 34, 57, 70-72, outblock.F90:208-211) and W_MAXH (w_maxh.F90 with W_MODE_ST; parameters 78-81,
// outblock.F90:559-578).  Reads FL1, WAVNUM = WVPRPT[ij][0][:] and DEPTH = FF[ij][15]; writes out[ij][13] in the column order of
// ecwam_hip.h.  Differences from the reference, all bounded or order-only:
//   * AKI's open GO TO loop (aki.F90:258-267) stops after AKI_MAXIT = 100 Newton steps;
//   * the sums over frequencies (the moments, the PEAK_ANG window, the autocovariance of the golden-section search) are wave reductions
//     (tree order), not the reference's running sums; the sums over the directions of one frequency keep the reference's order.  Adding
//     the frequencies in the reference's order (a uniform loop of lane reads) measured 28 % (sp) / 30 % (dp) slower at O320 and moved no double precision
//     column by more than its rounding (profiles/outbs_extremes_O320.txt);
//   * ZEPSILON = 10 EPSILON and its square root are those of the working precision (SUM40 starts at 1.1e-3 in single precision), as in
//     the reference.
#include <algorithm>

#include "dev.h"
#include "launch.h"

namespace {

constexpr int AKI_MAXIT = 100;
constexpr int NSC = 18;  // per-point scalars phase 1 hands to phase 2

__device__ __forceinline__ float m_cosh(float x) { return coshf(x); }
__device__ __forceinline__ double m_cosh(double x) { return cosh(x); }

template <typename T> struct Eps;
template <> struct Eps<float> { static constexpr float v = __FLT_EPSILON__; };
template <> struct Eps<double> { static constexpr double v = __DBL_EPSILON__; };

// parameters of the reference (Fortran PARAMETERs: compile-time values)
template <typename T> struct XC {
  static constexpr T DKMAX = T(40.0);      // yowpcons.F90:34
  static constexpr T XKDMIN = T(0.75);     // yowshal.F90:23
  static constexpr T WP2TAIL = T(0.5);     // yowfred.F90:54
  static constexpr T EPS4 = T(0.0001);     // EPS of transf_bfi.F90 / transf_r.F90 / stat_nl.F90, EBS of aki.F90
};

// AKI (aki.F90:249-269): wave number of angular frequency OM at depth BETA, Newton on OM**2 = G K TANH(K BETA)
template <typename T>
__device__ T aki(T G, T om, T beta) {
#pragma clang fp contract(off)
  const T akm1 = om * om / (T(4) * G);
  const T akm2 = om / (T(2) * m_sqrt(G * beta));
  T ao = m_max(akm1, akm2);
  for (int it = 0; it < AKI_MAXIT; it++) {
    const T akp = ao;
    const T bo = beta * ao;
    if (bo > XC<T>::DKMAX) return om * om / G;
    const T th = G * ao * m_tanh(bo);
    const T sth = m_sqrt(th);
    const T ch = m_cosh(bo);
    ao = ao + (om - sth) * sth * T(2) / (th / ao + G * bo / (ch * ch));
    if (!(m_abs(akp - ao) > XC<T>::EPS4 * ao)) break;
  }
  return ao;
}

// group velocity with the branches of transf_bfi.F90:68-72 / stat_nl.F90:211-217 (dk: the X > DKMAX branch of STAT_NL)
template <typename T>
__device__ __forceinline__ T vgroup(T c0, T x, bool dk) {
#pragma clang fp contract(off)
  if (dk && x > XC<T>::DKMAX) return T(0.5) * c0;
  if (x < XC<T>::EPS4) return c0;
  return T(0.5) * c0 * (T(1) + T(2) * x / m_sinh(T(2) * x));
}

// TRANSF_BFI (transf_bfi.F90:56-91)
template <typename T>
__device__ T transf_bfi(T G, T BATHYMAX, T xk0, T d, T xnu, T sig_th) {
#pragma clang fp contract(off)
  if (!(d < BATHYMAX && d > T(0))) return T(1);
  if (xk0 * d > XC<T>::DKMAX) return T(1);
  const T xk = m_max(xk0, XC<T>::XKDMIN / d);
  const T x = xk * d;
  const T t0 = m_tanh(x), t0sq = t0 * t0;
  const T om = m_sqrt(G * xk * t0);
  const T c0 = om / xk;
  const T cssq = G * d;
  const T vg = vgroup(c0, x, false);
  const T vgsq = vg * vg;
  const T a = t0 - x * (T(1) - t0sq);
  const T d2om = a * a + T(4) * (x * x) * t0sq * (T(1) - t0sq);
  const T xnl1 = (T(9) * (t0sq * t0sq) - T(10) * t0sq + T(9)) / (T(8) * t0sq * t0);
  const T b = T(2) * vg - T(0.5) * c0;
  const T xnl2 = ((b * b) / (G * d - vgsq) + T(1)) / x;
  const T e = T(2) * c0 + vg * (T(1) - t0sq);
  const T xnl4 = T(1) / (T(4) * t0) * (e * e) / (cssq - vgsq);
  const T alp = (T(1) - vgsq / cssq) * (c0 * c0) / vgsq;
  const T zfac = (sig_th * sig_th) / (sig_th * sig_th + alp * (xnu * xnu));
  const T xnl3 = zfac * xnl4;
  const T tnl = xnl1 - xnl2 + xnl3;
  const T q = vg / c0;
  const T r = T(4) * (q * q) * tnl * t0 / d2om;
  return m_max(m_min(T(4), r), T(-4));
}

// TRANSF_R (transf_r.F90:325-346)
template <typename T>
__device__ T transf_r(T G, T BATHYMAX, T xk0, T d) {
#pragma clang fp contract(off)
  if (!(d < BATHYMAX && d > T(0) && xk0 > T(0))) return T(0.5);
  if (xk0 * d > XC<T>::DKMAX) return T(0.5);
  const T xk = m_max(xk0, XC<T>::XKDMIN / d);
  const T x = xk * d;
  const T t0 = m_tanh(x), t0sq = t0 * t0;
  const T om = m_sqrt(G * xk * t0);
  const T c0 = om / xk;
  const T vg = vgroup(c0, x, false);
  const T a = t0 - x * (T(1) - t0sq);
  const T d2om = a * a + T(4) * (x * x) * t0sq * (T(1) - t0sq);
  const T q = vg / c0;
  return T(4) * (q * q * q) * t0sq / d2om;
}

// STAT_NL (stat_nl.F90:185-272) for one point: C3, C4, ETA_M, R
template <typename T>
__device__ void stat_nl(T G, T PI, T BATHYMAX, T xm0, T xk0, T bf2, T xnu, T sig_th, T d, T& c3, T& c4, T& eta_m, T& r) {
#pragma clang fp contract(off)
  const T ZEPS = T(10) * Eps<T>::v;
  const T SQRT3 = m_sqrt(T(3));
  const T C4_CONST = T(0.9) * PI / (T(3) * SQRT3);
  const T ZC1 = T(4) * SQRT3 / PI;
  const T ZC2 = T(1) / T(3) + T(2) * SQRT3 / PI;
  const T ZC3 = T(2) * SQRT3 / PI - T(4) / T(3);
  const T CONST_C3 = T(1.12) * T(2), CONST_C4 = T(0.93) * T(8);
  const T transf = transf_r(G, BATHYMAX, xk0, d);
  if (!(xm0 > ZEPS && d > T(0) && xk0 > T(0))) {
    c3 = c4 = eta_m = r = T(0);
    return;
  }
  const T xk = m_max(xk0, XC<T>::XKDMIN / d);
  const T x = xk * d;
  const T t0 = m_tanh(x);
  const T om = m_sqrt(G * xk * t0);
  const T t0sq = t0 * t0;
  const T alph = xk / (T(4) * t0sq * t0) * (T(3) - t0sq);
  const T gam = T(-0.5) * (alph * alph);
  const T c0 = om / xk;
  const T cssq = G * d;
  const T vg = vgroup(c0, x, true);
  const T vgsq = vg * vg;
  const T zfac = T(-0.25) * xk * cssq / (cssq - vgsq);
  const T delta_1d = zfac * (T(2) * (T(1) - t0sq) / t0 + T(1) / x);
  const T zfac1 = T(0.5) * c0 * cssq * vg / t0;
  const T xkappa1 = zfac1 * (T(2) * c0 + vg * (T(1) - t0sq)) / (cssq - vgsq);
  const T alpha = (T(1) - vgsq / cssq) * (c0 * c0) / vgsq;
  const T zfac2 = (sig_th * sig_th) / (sig_th * sig_th + alpha * (xnu * xnu));
  const T delta_2d = T(0.5) * (xk * xk) * xkappa1 / (om * cssq) * zfac2;
  const T delta = delta_1d + delta_2d;
  eta_m = T(2) * xm0 * delta;
  c3 = CONST_C3 * m_sqrt(xm0) * (alph + T(0.9) * delta);
  c3 = m_max(m_min(T(0.25), c3), T(0));
  const T ad = alph + delta;
  const T c4b = CONST_C4 * xm0 * (gam + alph * alph + ad * ad);
  const T q = sig_th / xnu;
  r = m_max(m_min(transf * (q * q), T(16)), T(0));
  const T zr = r;
  T xj;
  if (zr > T(1))
    xj = -C4_CONST / zr * (T(1) - ZC1 / m_sqrt(zr) + ZC2 / zr + ZC3 / (zr * zr));
  else
    xj = C4_CONST * (T(1) - ZC1 * m_sqrt(zr) + ZC2 * zr + ZC3 * (zr * zr));
  c4 = xj * bf2 + c4b;
  c4 = m_max(m_min(T(0.25), c4), T(-0.25));
}

// H_MAX (h_max.F90:91-125): normalised maximum envelope height HMAXN
template <typename T>
__device__ T h_max(T PI, T c3, T c4, T xnslc) {
#pragma clang fp contract(off)
  const T ZEPS = T(10) * Eps<T>::v;
  const T GAM = T(0.5772), EB = T(10);
  const T TWOG1 = T(-2) * GAM;
  const T G2 = GAM * GAM + PI * PI / T(6);
  const T AE = T(0.5) * EB * (EB - T(2));
  const T BE = T(0.5) * EB * (EB * EB - T(6) * EB + T(6));
  const T EMIN = T(2) * T(1) * T(1), EMAX = T(2) * T(4) * T(4);
  T e = T(2) * T(2) * T(2);
  const T dfn = c4 * AE + c3 * c3 * BE;
  if (!(xnslc > T(0) && m_abs(dfn) > ZEPS)) return T(1);  // H_C_MIN
  const T f = m_log(m_max(T(1) + dfn, T(0.1)));
  const T ebf = EB - f;
  const T aa = m_min((ebf * ebf - T(2) * EB) / (T(2) * f), T(1000));
  const T bb = T(2) * (T(1) + aa);
  const T bbm1 = T(1) / (bb + ZEPS * m_sign(T(1), bb));
  for (int i = 0; i < 5; i++) {
    const T z0 = m_log(xnslc * m_sqrt(T(0.5) * e));
    e = (G2 - TWOG1 * (aa + z0) + (T(2) * aa + z0) * z0) * bbm1;
    e = m_min(m_max(e, EMIN), EMAX);
  }
  return m_sqrt(T(0.5) * e);
}

// W_MODE_ST (w_mode_st.F90:191-211): mode of the space-time extreme distribution, Newton, at most 20 steps
template <typename T>
__device__ T w_mode_st(T rn3, T rn2, T rn1) {
#pragma clang fp contract(off)
  auto F = [&](T x) { return (x * (rn3 * x + rn2) + rn1) * m_exp(T(-0.5) * (x * x)) - T(1); };
  auto DF = [&](T x) { return (-(x * x) * (rn3 * x + rn2) + (T(2) * rn3 - rn1) * x + rn1 + rn2) * m_exp(T(-0.5) * (x * x)); };
  const T l3 = m_log(rn3);
  T z0 = m_sqrt(T(2) * l3 + T(2) * m_log(T(2) * l3 + T(2) * m_log(T(2) * l3)));
  T res = m_abs(F(z0));
  for (int it = 0; it < 20 && T(1.0e-6) < res; it++) {
    const T fp = DF(z0);
    if (fp != T(0)) z0 = z0 - F(z0) / fp;
    res = m_abs(F(z0));
  }
  return z0;
}

// inclusive prefix sum over the 64 lanes
template <typename T>
__device__ __forceinline__ T scan_incl(T x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T a = __shfl_up(x, d, 64);
    if (lane >= d) x = x + a;
  }
  return x;
}

// LDS of one workgroup: the scalars [NSC][64] phase 1 hands to phase 2 (lane = point reads consecutive words), then the spectrum tile of
// the current point in the row's [K][M] order
enum { S_SUM0, S_SUM1, S_SUM2, S_SUM6, S_SUM4, S_SUM40, S_PA1, S_PA2, S_EMEAN, S_T1, S_T2, S_TEMPN, S_RLX, S_RLY, S_AXY, S_AXT, S_AYT, S_ACF };

}  // namespace

// One wavefront per workgroup, up to 64 points.  Phase 1, one point after the other, lane = frequency M: the point's row is copied from
// the registers it was prefetched into (the loads of point p+1 are issued before point p is reduced: one HBM read per bin, one memory
// latency per point hidden behind the reduction of the previous one) into an LDS tile, summed over directions in the reference's order,
// and reduced over frequencies into NSC scalars in LDS.  W_MAXH's second pass (the CX / CY weights of the global argmax direction), the
// PEAK_ANG window and the golden-section search (one COS per lane and a wave sum per evaluation) run over the tile and the registers.
// Phase 2, lane = point: the scalar tails (AKI twice, TRANSF_BFI, STAT_NL with TRANSF_R, H_MAX, W_MODE_ST) for 64 points at once.
// Contraction is off: every product and sum is rounded where the reference rounds it.
template <typename T, int NA>
__global__ void __launch_bounds__(64) k_outbs_extremes(const DevTab<T>* __restrict__ tp, int kijs, int kijl, const T* __restrict__ fl1,
                                                       const T* __restrict__ wvprpt, const T* __restrict__ ff, int flags, T* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int NP = (NA * ECWAM_HIP_MAXFRE + 63) / 64;  // prefetch registers per lane
  extern __shared__ __align__(16) unsigned char ext_smem[];
  const DevTab<T>& tb = *tp;
  T* sS = reinterpret_cast<T*>(ext_smem);  // [NSC][64]
  T* sF = sS + NSC * 64;                    // [NA][NFRE]
  const int lane = threadIdx.x;
  const int NFRE = tb.NFRE, N = NA * NFRE;
  const long long blk0 = (long long)kijs + (long long)blockIdx.x * 64;
  const int nb = (int)std::min<long long>(64, (long long)kijl - blk0);
  const bool wmaxh = !(flags & 1);
  const T ZEPS = T(10) * Eps<T>::v, ZSQREPS = m_sqrt(ZEPS);
  const T DELTH = tb.DELTH, ZPI = tb.ZPI;
  const T FRMAX = tb.FR[NFRE - 1], FRMIN = tb.FR[0];
  const T TMIN = T(1) / FRMAX, TMX = T(1) / FRMIN;
  const bool actm = lane < NFRE;
  const int mm = actm ? lane : NFRE - 1;  // inactive lanes read the last frequency again and contribute 0
  const T dfim = tb.DFIM[mm], dfimfr = tb.DFIMFR[mm], dfimofr = tb.DFIMOFR[mm];
  const T dfimfr2 = tb.DFIM[mm] * (tb.FR[mm] * tb.FR[mm]);  // DFIMFR2, initmdl.F90:447
  const T fac4 = T(2) * DELTH * dfimfr;                     // FAC4, kurtosis.F90:307
  const T omega = ZPI * tb.FR[mm];                          // OMEGA, w_maxh.F90:107
  const int NSH = 1 + (int)(m_log(T(1.5)) / m_log(tb.FRATIO));  // peak_ang.F90:80
  const T GRRM1 = T(2) / (T(1) + m_sqrt(T(5)));                // w_maxh.F90:71

  T pf[NP];
  auto prefetch = [&](int p) {
    const T* r = fl1 + (size_t)(blk0 + p) * (size_t)N;
#pragma unroll
    for (int u = 0; u < NP; u++)
      if (u * 64 < N) pf[u] = r[std::min(u * 64 + lane, N - 1)];
  };
  prefetch(0);
  for (int p = 0; p < nb; p++) {
    __syncthreads();  // the previous point's reads of the tile are done
#pragma unroll
    for (int u = 0; u < NP; u++)
      if (u * 64 + lane < N) sF[u * 64 + lane] = pf[u];
    __syncthreads();
    if (p + 1 < nb) prefetch(p + 1);
    const size_t ij = (size_t)(blk0 + p);
    const T* col = sF + mm;  // FL1(K, M) = col[K * NFRE]
    // pass 1 over directions: FF(M) (kurtosis.F90:257-267), the sine / cosine sums of PEAK_ANG, the first maximum over K
    T fs = T(0), ss = T(0), cs = T(0), wmx = T(0);
    int wk = 0;
#pragma unroll 2
    for (int k = 0; k < NA; k++) {
      const T f = col[k * NFRE];
      fs = fs + f;
      ss = ss + tb.SINTH[k] * f;
      cs = cs + tb.COSTH[k] * f;
      if (f > wmx) { wmx = f; wk = k; }
    }
    if (!actm) fs = ss = cs = wmx = T(0);
    T A0, A1, A2, A6;
    usum4(fs * dfim, fs * dfimfr, fs * dfimfr2, fs * dfimofr, A0, A1, A2, A6);
    // FFMAX; PEAK_ANG's maximum over M = 2..NFRE-1 (peak_ang.F90:127-141) and W_MAXH's over every bin (w_maxh.F90:135-146): the first
    // maximum in (M outer, K inner) order with strict >, starting from 0 -- the lowest lane holding the largest lane maximum
    const T pmx = (lane >= 1 && lane <= NFRE - 2) ? wmx : T(0);
    T FFMAX, PV;
    umax2(fs, pmx, FFMAX, PV);
    const T WV = umax(wmx);
    const unsigned long long bp = __ballot(PV > T(0) && pmx == PV), bw = __ballot(WV > T(0) && wmx == WV);
    const int MMAX = bp ? __ffsll((long long)bp) - 1 : 1;
    const int KT = bw ? __builtin_amdgcn_readlane(wk, __ffsll((long long)bw) - 1) : 0;
    // PEAK_ANG's window MMAX-NSH .. MMAX+NSH (peak_ang.F90:148-165): THMEAN from the running sums after each frequency
    const int ms = std::max(0, MMAX - NSH), me = std::min(NFRE - 1, MMAX + NSH);
    const bool inw = lane >= ms && lane <= me;
    const T S = scan_incl(inw ? ss : T(0), lane), C = ZEPS + scan_incl(inw ? cs : T(0), lane);
    T s1 = T(0), s2 = T(0);
    if (inw) {
      const T th = m_atan2(S, C);
#pragma unroll 1
      for (int k = 0; k < NA; k++) {
        const T f = col[k * NFRE];
        s1 = s1 + f * dfim;
        s2 = s2 + m_cos(tb.TH[k] - th) * f * dfim;
      }
    }
    // SUM40 / SUM4 over the frequencies above FLTHRS FFMAX (kurtosis.F90:309-321) and the window's sums, as wave reductions
    const bool sel = actm && fs > T(0.4) * FFMAX;
    T S40, S4, P1, P2;
    usum4(sel ? fs * dfim : T(0), sel ? fs * fs * fac4 : T(0), s1, s2, S40, S4, P1, P2);
    const T FFN = lane_get(fs, NFRE - 1);
    const T DELT25 = tb.WETAIL * FRMAX * DELTH;
    if (lane == 0) {
      sS[S_SUM0 * 64 + p] = ZEPS + A0 + DELT25 * FFN;
      sS[S_SUM1 * 64 + p] = A1 + tb.WP1TAIL * DELTH * (FRMAX * FRMAX) * FFN;
      sS[S_SUM2 * 64 + p] = A2 + XC<T>::WP2TAIL * DELTH * (FRMAX * FRMAX * FRMAX) * FFN;
      sS[S_SUM6 * 64 + p] = A6 + tb.FRTAIL * DELTH * FFN;
      sS[S_SUM4 * 64 + p] = S4;
      sS[S_SUM40 * 64 + p] = ZSQREPS + S40;
      sS[S_PA1 * 64 + p] = ZEPS + P1;
      sS[S_PA2 * 64 + p] = P2;
      sS[S_EMEAN * 64 + p] = A0;
      sS[S_T1 * 64 + p] = A1;
      sS[S_T2 * 64 + p] = A2;
      sS[S_TEMPN * 64 + p] = FFN;
    }
    if (wmaxh) {
      // W_MAXH's second pass (w_maxh.F90:152-197): weights of the direction of the maximum
      const T ck = tb.COSTH[KT], sk = tb.SINTH[KT];
      T tx = T(0), ty = T(0), tx2 = ZEPS, ty2 = ZEPS, txy = T(0);
#pragma unroll 2
      for (int k = 0; k < NA; k++) {
        const T cx = tb.COSTH[k] * ck + tb.SINTH[k] * sk;
        const T cy = tb.SINTH[k] * ck - tb.COSTH[k] * sk;
        const T f = col[k * NFRE];
        tx = tx + f * cx;
        ty = ty + f * cy;
        tx2 = tx2 + f * (cx * cx);
        ty2 = ty2 + f * (cy * cy);
        txy = txy + f * (cx * cy);
      }
      const T xk = wvprpt[ij * (size_t)(ECWAM_HIP_NWPR * NFRE) + mm];
      const T xk2d = (xk * xk) * dfim;
      const T xkz = xk * ZPI * dfimfr;
      T RLX, RLY, AXY, AXT, AYT, unused;
      usum4(actm ? tx2 * xk2d : T(0), actm ? ty2 * xk2d : T(0), actm ? txy * xk2d : T(0), actm ? tx * xkz : T(0), RLX, RLY, AXY, AXT);
      // the golden-section search for the first minimum of the autocovariance SUM(COS(OMEGA*TLAG)*TEMPDFIM) (w_maxh.F90:242-272) between
      // 0.3 and 1.3 T2; wave-uniform control flow.  ACFS(1) and ACFS(4) of the reference are never read.
      const T tdf = actm ? fs * dfim : T(0);  // TEMPDFIM, w_maxh.F90:188
      T ACF = T(0);
      if (A0 > ZEPS) {
        const T t2 = m_min(m_max(m_sqrt(A0 / A2), TMIN), TMX);
        auto acf = [&](T tl) { return usum(actm ? m_cos(omega * tl) * tdf : T(0)); };
        T tl1 = T(0.3) * t2, tl4 = T(1.3) * t2;
        T tl2 = tl4 - (tl4 - tl1) * GRRM1, tl3 = tl1 + (tl4 - tl1) * GRRM1;
        T a2, a3;
        usum2(actm ? m_cos(omega * tl2) * tdf : T(0), actm ? m_cos(omega * tl3) * tdf : T(0), a2, a3);
        usum2(actm ? ty * xkz : T(0), T(0), AYT, unused);
        for (int it = 0; it < 10; it++) {
          if (a2 < a3) {
            ACF = a2;
            tl4 = tl3;
            tl3 = tl2;
            a3 = a2;
            tl2 = tl4 - (tl4 - tl1) * GRRM1;
            a2 = acf(tl2);
          } else {
            ACF = a3;
            tl1 = tl2;
            tl2 = tl3;
            a2 = a3;
            tl3 = tl1 + (tl4 - tl1) * GRRM1;
            a3 = acf(tl3);
          }
          if (m_abs(tl4 - tl1) < T(0.01) * (m_abs(tl2) + m_abs(tl3))) break;
        }
      } else {
        AYT = usum(actm ? ty * xkz : T(0));
      }
      if (lane == 0) {
        sS[S_RLX * 64 + p] = RLX;
        sS[S_RLY * 64 + p] = RLY;
        sS[S_AXY * 64 + p] = AXY;
        sS[S_AXT * 64 + p] = AXT;
        sS[S_AYT * 64 + p] = AYT;
        sS[S_ACF * 64 + p] = ACF;
      }
    }
  }
  __syncthreads();

  // ---- phase 2: lane = point
  if (lane >= nb) return;
  const int p = lane;
  const size_t ij = (size_t)(blk0 + p);
  auto sc = [&](int f) { return sS[f * 64 + p]; };
  const T G = tb.G, PI = tb.PI, BATHYMAX = tb.BATHYMAX;
  const T depth = ff[ij * ECWAM_HIP_NFF + 15];
  const T SUM0 = sc(S_SUM0), SUM1 = sc(S_SUM1), SUM2 = sc(S_SUM2), SUM6 = sc(S_SUM6), SUM4 = sc(S_SUM4), SUM40 = sc(S_SUM40);
  // PEAK_ANG: XNU (peak_ang.F90:115-121), SIG_TH (:167-174)
  const T XNU = SUM0 > ZEPS ? m_sqrt(m_max(ZEPS, SUM2 * SUM0 / (SUM1 * SUM1) - T(1))) : ZEPS;
  const T PA1 = sc(S_PA1), PA2 = sc(S_PA2);
  const T SIG_TH = PA1 > ZEPS ? T(1) * m_sqrt(T(2) * (T(1) - PA2 / PA1)) : T(0);
  // KURTOSIS section 3 (kurtosis.F90:325-348)
  const T CONST_OM_ZPI = T(0.89) * ZPI;
  T F_M, QP, XKP, BF2;
  if (SUM1 > ZSQREPS && SUM0 > ZEPS) {
    F_M = m_max(m_min(SUM1 / SUM0, FRMAX), FRMIN);
    QP = m_max(m_min(SUM4 / (SUM40 * SUM40), T(15)), T(0.5));
    const T SIG_OM = T(1) / m_sqrt(PI) / QP;
    const T OM_MEAN = CONST_OM_ZPI * m_max(m_min(SUM0 / SUM6, FRMAX), FRMIN);
    XKP = aki(G, OM_MEAN, depth);
    const T EPS = XKP * m_sqrt(SUM0);
    const T TRANS = transf_bfi(G, BATHYMAX, XKP, depth, XNU, SIG_TH);
    const T q = EPS / m_max(SIG_OM, ZEPS);
    BF2 = T(2) * TRANS * (q * q);
    BF2 = m_max(m_min(BF2, T(5)), T(-5));
  } else {
    F_M = QP = BF2 = T(0);
    const T OM_MEAN = CONST_OM_ZPI * FRMAX;
    XKP = OM_MEAN * OM_MEAN / G;
  }
  T C3, C4, ETA_M, R;
  stat_nl(G, PI, BATHYMAX, SUM0, XKP, BF2, XNU, SIG_TH, depth, C3, C4, ETA_M, R);
  // XNSLC (kurtosis.F90:365-376): NINT rounds half away from zero
  const T ZFAC = T(2) * ZPI / m_sqrt(ZPI);
  const T XNSLC = F_M > T(0) ? T(m_nint(T(1200) * (ZFAC * XNU * F_M))) : T(0);
  const T HMAXN = h_max(PI, C3, C4, XNSLC);
  T TMAX = T(0);
  if (SUM1 > ZEPS && HMAXN > ZEPS) {  // kurtosis.F90:380-389
    const T z = XNU / (m_sqrt(T(2)) * HMAXN), z2 = z * z;
    TMAX = SUM0 / SUM1 * (T(1) + T(0.5) * z2 + T(0.75) * (z2 * z2));
  }
  const T HMAX = SUM0 > T(0) ? HMAXN * (T(4) * m_sqrt(SUM0)) : T(0);
  T* o = out + ij * 13;
  o[0] = C4;
  o[1] = BF2;
  o[2] = QP;
  o[3] = HMAX;
  o[4] = TMAX;
  o[5] = C3;
  o[6] = ETA_M;
  o[7] = R;
  o[8] = XNSLC;
  if (!wmaxh) return;

  // ---- W_MAXH (w_maxh.F90:200-333)
  const T EMEAN = sc(S_EMEAN);
  T CMAX_F = T(0), HMAX_N = T(0), CMAX_ST = T(0), HMAX_ST = T(0);
  if (EMEAN > ZEPS) {
    const T WVLMIN = G / (ZPI * (FRMAX * FRMAX));
    const T HS = T(4) * m_sqrt(EMEAN + tb.WETAIL * FRMAX * DELTH * sc(S_TEMPN));
    T rlx = sc(S_RLX), rly = sc(S_RLY), t1 = sc(S_T1), t2 = sc(S_T2);
    const T AXY = m_min(sc(S_AXY) / m_sqrt(rlx * rly), T(1));
    const T AXT = m_min(sc(S_AXT) / (ZPI * m_sqrt(rlx * t2)), T(1));
    const T AYT = m_min(sc(S_AYT) / (ZPI * m_sqrt(rly * t2)), T(1));
    rlx = ZPI * m_sqrt(EMEAN / rlx);
    rly = ZPI * m_sqrt(EMEAN / rly);
    const T RNI = m_sqrt(m_max(EMEAN * t2 / (t1 * t1) - T(1), ZEPS));
    const T zt = ZPI * t1;
    const T RMU = (zt * zt) * (T(1) - RNI + RNI * RNI) / (G * m_pow(EMEAN, T(3) / T(2)));
    t1 = m_min(m_max(EMEAN / t1, TMIN), TMX);
    t2 = m_min(m_max(m_sqrt(EMEAN / t2), TMIN), TMX);
    const T WMDX = m_max(rlx, WVLMIN), WMDY = m_max(rly, WVLMIN), WMDUR_ST = T(100) * t2;
    const T GAMMA_E = T(0.57721566);
    const T SQRTEM = T(0.25) * HS;
    const T WNUM1 = aki(G, ZPI / t1, depth);
    const T STEEP = ZPI * HS / (G * (t1 * t1));
    const T URSN = HS / ((WNUM1 * WNUM1) * (depth * depth * depth));
    const T ALFA = T(0.3536) + T(0.2568) * STEEP + T(0.08) * URSN;
    const T BETA = T(2) - T(1.7912) * STEEP - T(0.5302) * URSN + T(0.284) * (URSN * URSN);
    T Z0 = m_log(T(1200) / t2);
    CMAX_F = ALFA * m_pow(Z0, T(1) / BETA) * (T(1) + GAMMA_E / (BETA * Z0)) * HS;
    const T PHIST = m_min(sc(S_ACF) / EMEAN, T(1));
    HMAX_N = T(0.5) * m_sqrt(T(1) - PHIST) * m_sqrt(Z0) * (T(1) + T(0.5) * GAMMA_E / Z0) * HS;
    const T AXYT = m_sqrt(T(1) + T(2) * AXT * AXY * AYT - AXT * AXT - AXY * AXY - AYT * AYT);
    const T RN3 = ZPI * WMDX * WMDY * WMDUR_ST * AXYT / (rlx * rly * t2);
    const T RN2 = m_sqrt(ZPI) * (WMDX * WMDUR_ST / (rlx * t2) * m_sqrt(T(1) - AXT * AXT) + WMDX * WMDY / (rlx * rly) * m_sqrt(T(1) - AXY * AXY) +
                                 WMDY * WMDUR_ST / (rly * t2) * m_sqrt(T(1) - AYT * AYT));
    const T RN1 = WMDX / rlx + WMDY / rly + WMDUR_ST / t2;
    Z0 = w_mode_st(RN3, RN2, RN1);
    const T XX = T(1) / (Z0 - (T(2) * RN3 * Z0 + RN2) / (RN3 * (Z0 * Z0) + RN2 * Z0 + RN1));
    CMAX_ST = ((Z0 + T(0.5) * RMU * (Z0 * Z0)) + GAMMA_E * ((T(1) + RMU * Z0) * XX)) * SQRTEM;
    HMAX_ST = (Z0 + GAMMA_E * XX) * m_sqrt(T(2) * (T(1) - PHIST)) * SQRTEM;
  }
  o[9] = CMAX_F;
  o[10] = HMAX_N;
  o[11] = CMAX_ST;
  o[12] = HMAX_ST;
}

template <typename T>
int launch_outbs_extremes(const void* tab, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* ff, int flags, void* out, int NANG,
                          int NFRE, hipStream_t s) {
  const int n = kijl - kijs;
  if (n <= 0) return 0;
  if (NFRE < 3 || NFRE > ECWAM_HIP_MAXFRE) return 1;
  const size_t lds = ((size_t)NSC * 64 + (size_t)NANG * NFRE) * sizeof(T);
  const dim3 grid((n + 63) / 64), block(64);
  const DevTab<T>* tp = (const DevTab<T>*)tab;
  switch (NANG) {
#define EXT_CASE(NA)                                                                                                                        \
  case NA:                                                                                                                                  \
    hipLaunchKernelGGL((k_outbs_extremes<T, NA>), grid, block, lds, s, tp, kijs, kijl, (const T*)fl1, (const T*)wvprpt, (const T*)ff, flags, \
                       (T*)out);                                                                                                            \
    return 0;
    EXT_CASE(12)
    EXT_CASE(24)
    EXT_CASE(36)
    EXT_CASE(48)
#undef EXT_CASE
    default:
      return 1;
  }
}
template int launch_outbs_extremes<float>(const void*, int, int, const void*, const void*, const void*, int, void*, int, int, hipStream_t);
template int launch_outbs_extremes<double>(const void*, int, int, const void*, const void*, const void*, int, void*, int, int, hipStream_t);
