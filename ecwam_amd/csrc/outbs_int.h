// The constants of k_outbs_integrals (csrc/outbs_int.hip) that ecwam_hip_set_outbs_integrals works out once, in the working precision T:
// the two mean-square-slope cut-offs of OUTBLOCK (0: XKMSS_CUTOFF, parameter 9; 1: (ZPI FR(NFRE))**2 / G, parameter 86), SEBTMEAN's
// per-band constants (sebtmean.F90:81-102, 119-120, 148-149, 165, 172-175, 184) and DELKCC_GC, the one gravity-capillary table DevTab
// does not hold on its own.  One instance per context in device memory.
#pragma once
#include "dev.h"

#define ECWAM_HIP_MAXBAND 8

template <typename T>
struct IntTab {
  int NBAND;
  // meansqs.F90:99-101, meansqs_gc.F90:59.  The two indices are evaluated in double precision from the working-precision tables: with the
  // model's own cut-off FCUT is FR(NFRE) and LOG(FCUT/FR(1))/LOG(FRATIO) lies within rounding of NFRE - 1, where INT depends on the last bit
  // of the logarithm routine at hand.
  int NE[2], NFRE_EFF[2];
  T XKMSS[2], FCUT[2];
  // band b: MCUTB, MCUTT (1-based); the trapezoid runs M = M0 .. M1 (1-based) with DF[b][M-1]; WLB / WRB the interpolation weights at
  // FRLOC(MCUTB-1) (used when MCUTB > 1), WLT / WRT at FRLOC(MCUTT+1) (used when MCUTT < NFRE); FRONT: the linear front tail with factor DFT;
  // TAIL: the f**-5 extension with factor ZW
  int MCUTB[ECWAM_HIP_MAXBAND], MCUTT[ECWAM_HIP_MAXBAND], M0[ECWAM_HIP_MAXBAND], M1[ECWAM_HIP_MAXBAND], FRONT[ECWAM_HIP_MAXBAND],
      TAIL[ECWAM_HIP_MAXBAND];
  T WLB[ECWAM_HIP_MAXBAND], WRB[ECWAM_HIP_MAXBAND], WLT[ECWAM_HIP_MAXBAND], WRT[ECWAM_HIP_MAXBAND], DFT[ECWAM_HIP_MAXBAND],
      ZW[ECWAM_HIP_MAXBAND];
  T DF[ECWAM_HIP_MAXBAND][MAXF];
  T DELKCC_GC[MAXGC];  // 1-based like the tables of DevTab
};

// the column groups of ecwam_hip_outbs_integrals (flags)
enum { INT_SLOPES = 1, INT_STRAIN = 2, INT_FLUX = 4, INT_CTCOR = 8, INT_BANDS = 16, INT_POINT = 32, INT_ALL = 63 };
