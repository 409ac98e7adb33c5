// OUTBLOCK itself (outblock.F90:159-610): which of the device output calls a request (IPFGTBL) needs, and the kernel that writes every value into
// its column ITOBOUT(IR) of BOUT(KIJL, NIPRMOUT) and applies OUTSETWMASK.  The spectral computations stay in the kernels of outbs*.hip, which are
// called as they are and leave their packed rows in the work space of the context; k_outblock_assemble moves values, converts the few that
// OUTBLOCK converts (a direction to degrees, MAX(-PHIOCD,0), IBRMEMOUT's rule, the JWRO fields of NEMO to the working precision) and masks.
// BOUT is written once.
#include <cmath>
#include <string>

#include "dev.h"
#include "launch.h"

__device__ __forceinline__ float ob_fmod(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double ob_fmod(double a, double b) { return fmod(a, b); }

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------------
// Parameter numbers are those of mpcrtbl.F90 with NTRAIN = 3 and NTEWH = 6: 42 + 3 (ITR - 1) the trains, 51 the strain, 52 SE10MEAN, 62 / 63 the
// flux, 63 + IH the bands, 70-72, 78-81, 82 IBRMEMOUT, 83 / 84 TAUICX / TAUICY, 85 CTCOR, 86 the slope at the model cut-off, 87-89 unused extra fields.
namespace {
constexpr int NTRAIN = 3, NTEWH = 6, JPPFLAG = 75 + 3 * NTRAIN + 5;
struct Where { int src, col, op; };
}  // namespace

std::string outblock_plan_build(const OutblockCtx& c, int jppflag, const int* ipfgtbl, const int* itobout, const int* icemask, const int* seamask, int niprmout,
                                int flags, OutblockPlan& plan) {
  plan = OutblockPlan();
  if (jppflag != JPPFLAG) return "jppflag must be 89 = 75 + 3 NTRAIN + 5: the library is written for NTRAIN = 3 (got " + std::to_string(jppflag) + ")";
  if (!ipfgtbl || !itobout || !icemask || !seamask) return "null pointer";
  if (niprmout < 1 || niprmout > 128) return "niprmout must be 1 .. 128";
  if (flags & ~7) return "unknown flags";
  bool req[JPPFLAG + 1];
  req[0] = false;
  for (int ir = 1; ir <= JPPFLAG; ir++) req[ir] = ipfgtbl[ir - 1] != 0;   // -1 (NFLAG only, mpcrtbl.F90:490-493) is on the list as well
  auto any = [&](int a, int b) { for (int ir = a; ir <= b; ir++) if (req[ir]) return ir; return 0; };
  std::vector<int> owner(niprmout, 0);
  for (int ir = 1; ir <= JPPFLAG; ir++) {
    if (!req[ir]) continue;
    const int col = itobout[ir - 1];
    if (col < 1 || col > niprmout) return "parameter " + std::to_string(ir) + " is requested but its column itobout = " + std::to_string(col) + " is outside 1 .. niprmout";
    if (owner[col - 1]) return "parameters " + std::to_string(owner[col - 1]) + " and " + std::to_string(ir) + " are mapped to the same column " + std::to_string(col);
    owner[col - 1] = ir;
  }
  const bool second = flags & 1, small = flags & 2;
  const bool fl1path = c.irefra < 2 && !(c.licerun && !c.lmaskice) && !second;   // FL2ND = FL1 (outblock.F90:168-194)
  const int trains = any(42, 41 + 3 * NTRAIN);                                   // LLPARTITION (mpcrtbl.F90:535-543)
  const int strain = 42 + 3 * NTRAIN, se10 = strain + 1, flux = 53 + 3 * NTRAIN, band1 = flux + 2, ctcor = 70 + 3 * NTRAIN + NTEWH;
  const int bands = req[se10] ? se10 : any(band1, band1 + NTEWH - 1);
  if (trains && small) return "parameters 42-50 (swell trains) cannot be requested with CLDOMAIN = 's' (flags bit 1): ecwam_hip_outbs_partition refuses that branch";
  if (second && !c.has_second_order) return "LSECONDORDER (flags bit 0) is set but the context has no second-order tables (ecwam_hip_set_second_order)";
  if (!fl1path && c.irefra >= 2 && !c.has_itab) return "NFRE_MAX of INTPOL exceeds the library's table";
  if (!outbs_size_ok(c.NANG, c.NFRE, (size_t)c.real_bytes)) return "unsupported spectral size";

  auto either = [](int a, int b) { return a ? a : b; };    // the first requested parameter of a group, 0: none
  const int spec = either(any(1, 3), any(6, 6)), t1 = any(20, 22);
  const int seasw = either(any(11, 16), any(23, 28)), ext = either(either(any(29, 31), any(33, 34)), either(any(57, 57), any(70, 72))), wmaxh = any(78, 81);
  const bool own_strain = req[strain] && !c.lwnemocoustrn;   // else STRNMS of INTF (outblock.F90:451-457)
  int groups = 0;
  if (req[9] || req[ctcor + 1]) groups |= 1;
  if (own_strain) groups |= 2;
  if (req[flux] || req[flux + 1]) groups |= 4;
  if (req[ctcor]) groups |= 8;
  if (bands) groups |= 16;
  if (req[7] || req[8]) groups |= 32;
  if (groups) {
    if (c.int_nband < 0) return "parameter " + std::to_string(bands ? bands : (req[7] ? 7 : req[8] ? 8 : req[9] ? 9 : own_strain ? strain : req[flux] ? flux : req[flux + 1] ? flux + 1 : req[ctcor] ? ctcor : ctcor + 1)) +
                                " is requested but the cut-off and the bands are not set (ecwam_hip_set_outbs_integrals)";
    if (c.NANG != 48 && c.NANG != 36 && c.NANG != 24 && c.NANG != 12) return "ecwam_hip_outbs_integrals has no build for this NANG (48, 36, 24 and 12 are built)";
  }
  if (second && c.NANG != 48 && c.NANG != 36 && c.NANG != 24 && c.NANG != 12) return "ecwam_hip_outbs_second_order has no build for this NANG (48, 36, 24 and 12 are built)";
  if (bands) {
    // the period intervals of the request: SE10MEAN = (10, 1 / FR(1)) (outblock.F90:460), then IPRMINFO(:,4:5) of 64-69 (mpcrtbl.F90:371-399)
    static const double lo[1 + NTEWH] = {10, 10, 12, 14, 17, 21, 25}, hi[1 + NTEWH] = {0, 12, 14, 17, 21, 25, 30};
    bool ok = c.int_nband == 1 + NTEWH;
    for (int i = 0; ok && i <= NTEWH; i++) {
      const double top = i ? hi[i] : 1.0 / c.fr1;
      ok = c.int_tb[i] == lo[i] && std::fabs(c.int_tt[i] - top) <= 1e-6 * top;
    }
    if (!ok) return "parameter " + std::to_string(bands) + " (a period band) is requested but the bands of ecwam_hip_set_outbs_integrals do not match the requested period "
                    "intervals: (10, 1/FR(1)) then (10,12) (12,14) (14,17) (17,21) (21,25) (25,30) s";
  }

  plan.niprmout = niprmout;
  plan.flags = flags;
  plan.int_groups = groups;
  plan.ext_full = wmaxh ? 1 : 0;
  plan.w8_stride = fl1path ? 5 : 8;
  plan.sep_stride = trains ? 24 : 15;
  if (fl1path && spec) plan.calls |= OB_CALL_OUTBS;
  if (!fl1path && (spec || t1 || bands)) plan.calls |= second ? OB_CALL_SECOND_ORDER : OB_CALL_ABSOLUTE;
  plan.stores_fl2nd = (!fl1path && bands) ? 1 : 0;
  if (trains) plan.calls |= OB_CALL_PARTITION;
  else if (seasw || (fl1path && t1)) plan.calls |= OB_CALL_SEPWISW;
  if (ext || wmaxh) plan.calls |= OB_CALL_EXTREMES;
  if (groups) plan.calls |= OB_CALL_INTEGRALS;

  // the caller's arrays the calls read, each with a parameter that asks for it
  auto need = [&](unsigned bits, int ir) {
    for (int b = 0; b < 12; b++)
      if ((bits >> b & 1) && !(plan.need >> b & 1)) plan.why_param[b] = ir;
    plan.need |= bits;
  };
  const bool intpol = c.irefra >= 2, icefl = c.licerun && !c.lmaskice;
  if (plan.calls & OB_CALL_OUTBS) need(OB_NEED_FL1, spec);
  if (plan.calls & (OB_CALL_ABSOLUTE | OB_CALL_SECOND_ORDER)) {
    const int ir = spec ? spec : t1 ? t1 : bands;
    need(OB_NEED_FL1, ir);
    if (intpol) need(OB_NEED_WVPRPT | OB_NEED_UCUR | OB_NEED_VCUR, ir);
    if (icefl) need(OB_NEED_FF, ir);
    if (second) need(OB_NEED_WVPRPT | OB_NEED_FF, ir);   // FKMEAN reads WAVNUM; DEPTH = ff[ij][15]
  }
  if (plan.calls & (OB_CALL_SEPWISW | OB_CALL_PARTITION)) need(OB_NEED_FL1 | OB_NEED_XLLWS | OB_NEED_WVPRPT | OB_NEED_FF, trains ? trains : seasw ? seasw : t1);
  if (plan.calls & OB_CALL_PARTITION) need(OB_NEED_MIJ, trains);
  if (plan.calls & OB_CALL_EXTREMES) need(OB_NEED_FL1 | OB_NEED_WVPRPT | OB_NEED_FF, ext ? ext : wmaxh);
  if (groups & 15) need(OB_NEED_FL1 | OB_NEED_WVPRPT | OB_NEED_FF, req[9] ? 9 : own_strain ? strain : req[flux] ? flux : req[flux + 1] ? flux + 1 : req[ctcor] ? ctcor : ctcor + 1);
  if (groups & 16) need(OB_NEED_FL1, bands);
  if (groups & 32) need(OB_NEED_FF, req[7] ? 7 : 8);

  // where every parameter comes from
  auto where = [&](int ir) -> Where {
    const int w8 = OB_W8, sep = OB_SEP;
    if (ir >= 42 && ir < strain) return {sep, 15 + (ir - 42), OB_COPY};
    if (ir >= band1 && ir < band1 + NTEWH) return {OB_INT, 9 + (ir - band1), OB_COPY};
    switch (ir) {
      case 1: return {w8, 0, OB_COPY};
      case 2: return {w8, 1, OB_COPY};
      case 3: return {w8, 2, OB_COPY};
      case 4: return {OB_FF, 7, OB_COPY};       // UFRIC
      case 5: return {OB_FF, 1, OB_DEG};        // WDWAVE
      case 6: return {w8, 4, OB_COPY};
      case 7: return {OB_INT, 0, OB_COPY};
      case 8: return {OB_INT, 1, OB_COPY};
      case 9: return {OB_INT, 2, OB_COPY};
      case 10: return {OB_FF, 3, OB_COPY};      // WSWAVE
      case 11: case 12: case 13: case 14: case 15: case 16: return {sep, 3 + (ir - 11), OB_COPY};
      case 17: case 18: case 19: return {OB_ALTIM, ir - 17, OB_COPY};
      case 20: case 21: case 22: return fl1path ? Where{sep, ir - 20, OB_COPY} : Where{w8, 5 + (ir - 20), OB_COPY};
      case 23: case 24: case 25: case 26: case 27: case 28: return {sep, 9 + (ir - 23), OB_COPY};
      case 29: case 30: case 31: return {OB_EXT, ir - 29, OB_COPY};
      case 32: return {OB_FF, 15, OB_COPY};     // DEPTH
      case 33: case 34: return {OB_EXT, 3 + (ir - 33), OB_COPY};
      case 35: case 36: return {OB_INTF, 2 + (ir - 35), OB_COPY};   // USTOKES, VSTOKES
      case 37: return {OB_UCUR, 0, OB_COPY};
      case 38: return {OB_VCUR, 0, OB_COPY};
      case 39: return {OB_INTF, 13, OB_COPY};   // PHIEPS
      case 40: return {OB_INTF, 14, OB_COPY};   // PHIAW
      case 41: return {OB_INTF, 9, OB_COPY};    // TAUOC
      case 51: return c.lwnemocoustrn ? Where{OB_INTF, 4, OB_COPY} : Where{OB_INT, 3, OB_COPY};
      case 52: return {OB_INT, 8, OB_COPY};
      case 53: return {OB_FF, 0, OB_COPY};      // AIRD
      case 54: return {OB_FF, 4, OB_COPY};      // WSTAR
      case 55: return {OB_FF, 2, OB_COPY};      // CICOVER
      case 56: return {OB_FF, 13, OB_COPY};     // CITHICK
      case 57: return {OB_EXT, 5, OB_COPY};
      case 58: case 59: case 60: case 61: return {OB_NEMO, ir - 58, OB_COPY};
      case 62: case 63: return {OB_INT, 4 + (ir - 62), OB_COPY};
      case 70: case 71: case 72: return {OB_EXT, 6 + (ir - 70), OB_COPY};
      case 73: case 74: case 75: case 76: return {OB_INTF, 5 + (ir - 73), OB_COPY};   // TAUXD TAUYD TAUOCXD TAUOCYD
      case 77: return {OB_INTF, 12, OB_NEGMAX};  // PHIOCD
      case 78: case 79: case 80: case 81: return {OB_EXT, 9 + (ir - 78), OB_COPY};
      case 82: return {OB_IBRMEM, 0, OB_IBR};
      case 83: case 84: return {OB_INTF, 10 + (ir - 83), OB_COPY};  // TAUICX, TAUICY
      case 85: return {OB_INT, 6, OB_COPY};
      case 86: return {OB_INT, 7, OB_COPY};
      default: return {OB_ZERO, 0, OB_COPY};     // the extra fields no statement fills: BOUT(KIJS:KIJL,:) = 0
    }
  };
  static const unsigned need_of[OB_NSRC] = {0, 0, 0, 0, 0, OB_NEED_FF, OB_NEED_INTF, OB_NEED_UCUR, OB_NEED_VCUR, OB_NEED_IBRMEM | OB_NEED_FF, OB_NEED_ALTIM, OB_NEED_NEMO};
  const bool icemask_on = c.licerun && !(flags & 4);   // LICERUN .AND. LLSOURCE (outsetwmask.F90:60)
  plan.desc.assign((size_t)2 * niprmout, 0);
  for (int col = 0; col < niprmout; col++) {
    const int ir = owner[col];
    if (!ir) continue;                                   // a column of no parameter stays 0, unmasked
    const Where w = where(ir);
    const int mk = (icemask[ir - 1] == 1 ? 1 : 0) | (seamask[ir - 1] == 1 ? 2 : 0);
    plan.desc[2 * col] = w.src | (w.op << 8) | (mk << 16);
    plan.desc[2 * col + 1] = w.col;
    need(need_of[w.src], ir);
    if (w.op == OB_IBR) plan.need_ci = 1;
    if ((mk & 1) && icemask_on) { plan.ice = 1; plan.need_ci = 1; need(OB_NEED_FF, ir); }
    if (mk & 2) { plan.sea = 1; need(OB_NEED_IODP, ir); }
  }
  return std::string();
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------
// One wavefront takes OB_PTS consecutive points; lane c (and c + 64 in a second pass over the lanes when NIPRMOUT > 64) owns BOUT column c, so that
// every row of BOUT is stored as one run of consecutive words.  A lane resolves its column's descriptor to an address and a stride once, before
// the loop over the points; CICOVER and IODP of a point are loaded once per point through a wave-uniform address.  Contraction is off so that the
// sea mask rounds as ecwam_hip_outsetwmask does.
constexpr int OB_PTS = 8;

template <typename T>
__global__ void __launch_bounds__(256) k_outblock_assemble(int kijs, int kijl, int ncol, const int* __restrict__ desc, OutblockSrc src, const T* __restrict__ ff,
                                                           const int* __restrict__ iodp, int ice, int sea, int need_ci, T cithrsh, T zmiss, T* __restrict__ bout) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const long long first = (long long)kijs + (long long)wave * OB_PTS;
  if (first >= kijl) return;   // wave-uniform
  const int i0 = (int)first, i1 = (int)(first + OB_PTS < kijl ? first + OB_PTS : kijl);
  const char* p[2] = {nullptr, nullptr};
  long long ps[2] = {0, 0};
  int sr[2] = {OB_ZERO, OB_ZERO}, op[2] = {OB_COPY, OB_COPY}, mk[2] = {0, 0};
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int c = q * 64 + lane;
    if (c < ncol) {
      const int d = desc[2 * c], col = desc[2 * c + 1];
      sr[q] = d & 255; op[q] = (d >> 8) & 255; mk[q] = (d >> 16) & 3;
      const void* b = nullptr;
      long long pst = 0, cst = 0;
#pragma unroll
      for (int s = 1; s < OB_NSRC; s++)
        if (sr[q] == s) { b = src.base[s]; pst = src.pstride[s]; cst = src.cstride[s]; }
      const long long esz = sr[q] == OB_NEMO ? (long long)sizeof(double) : (long long)sizeof(T);
      p[q] = (const char*)b + (long long)col * cst * esz;
      ps[q] = pst * esz;
    }
  }
  const T DEG = T(57.295778667);  // yowpcons.F90:31
  for (int ij = i0; ij < i1; ij++) {
    const T ci = need_ci ? ff[(size_t)ij * ECWAM_HIP_NFF + 2] : T(0);
    const int io = sea ? iodp[ij] : 1;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int c = q * 64 + lane;
      if (c >= ncol) continue;
      T x = T(0);
      if (sr[q] == OB_NEMO) x = (T) * (const double*)(p[q] + (long long)ij * ps[q]);   // JWRO -> JWRB
      else if (sr[q] != OB_ZERO) x = *(const T*)(p[q] + (long long)ij * ps[q]);
      if (op[q] == OB_DEG) x = ob_fmod(DEG * x + T(180), T(360));       // Fortran MOD: the sign of the dividend
      else if (op[q] == OB_NEGMAX) x = m_max(-x, T(0));
      else if (op[q] == OB_IBR) x = (ci > T(0)) ? x : zmiss;            // ibrmemout.F90:78-82
      if (ice && (mk[q] & 1) && ci > cithrsh) x = zmiss;                // outsetwmask.F90:60-65
      if (mk[q] & 2) x = x * T(io) + T(1 - io) * zmiss;                 // outsetwmask.F90:67-72
      bout[(size_t)ij * ncol + c] = x;
    }
  }
}

template <typename T>
void launch_outblock_assemble(int kijs, int kijl, int ncol, const int* desc, const OutblockSrc& src, const void* ff, const int* iodp, int ice, int sea, int need_ci,
                              double cithrsh, double zmiss, void* bout, hipStream_t s) {
  const long long n = (long long)kijl - kijs;
  if (n <= 0) return;
  const long long waves = (n + OB_PTS - 1) / OB_PTS;
  hipLaunchKernelGGL(k_outblock_assemble<T>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, kijs, kijl, ncol, desc, src, (const T*)ff, iodp, ice, sea, need_ci,
                     (T)cithrsh, (T)zmiss, (T*)bout);
}
template void launch_outblock_assemble<float>(int, int, int, const int*, const OutblockSrc&, const void*, const int*, int, int, int, double, double, void*, hipStream_t);
template void launch_outblock_assemble<double>(int, int, int, const int*, const OutblockSrc&, const void*, const int*, int, int, int, double, double, void*, hipStream_t);

// DEPTH = ff[ij][15] as the contiguous array ecwam_hip_outbs_second_order takes
template <typename T>
__global__ void __launch_bounds__(256) k_outblock_depth(int kijs, int kijl, const T* __restrict__ ff, T* __restrict__ depth) {
  const long long ij = (long long)kijs + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ij < kijl) depth[ij] = ff[ij * ECWAM_HIP_NFF + 15];
}
template <typename T>
void launch_outblock_depth(int kijs, int kijl, const void* ff, void* depth, hipStream_t s) {
  const long long n = (long long)kijl - kijs;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_outblock_depth<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kijs, kijl, (const T*)ff, (T*)depth);
}
template void launch_outblock_depth<float>(int, int, const void*, void*, hipStream_t);
template void launch_outblock_depth<double>(int, int, const void*, void*, hipStream_t);
