/*
 * The first-order upwind propagation scheme on the device: what PROPAG_WAM does with IPROPAGS = 0 (propag_wam.F90:341-362), the namelist default
 * (mpuserin.F90:610) and the only scheme of a Cartesian grid -- PROPAGS with its four sections (propags.F90:10-998), CHECKCFL as the spherical sections
 * call it (checkcfl.F90:74-247; propags.F90:718-722, 924-928) and the dot terms of PROPDOT with GRADI (propdot.F90:109-198, gradi.F90:113-232).  The two
 * calls are additions to ABI 6 (ECWAM_HIP_ABI_VERSION stays 6) in a header of their own: the lists of entry points the other headers were published
 * with stay the ones they were.  ecwam_hip_propdot and its REFR row (ecwam_hip.h) are not touched: they serve the corner-transport scheme.
 *
 * The conventions are those of ecwam_hip.h: device pointers; rows 0-based, the land row at index nland (after the halo rows); spectra FL[row][NANG][NFRE];
 * KLON [n][2], KLAT [n][2][2], WLAT [n][2]; the *_ext arrays cover every row up to and including the land row; the launch goes to `stream`; 0 on
 * success, otherwise 1 with the reason in ecwam_hip_last_error; an empty range launches nothing.  IREFRA is the context's.
 *
 * The arithmetic is the reference's, expression by expression in its order, in the working precision, without contraction and with correctly rounded
 * divisions.  PROPAGS, CHECKCFL, PROPDOT and GRADI hold only + - * / and ABS (MIN and SIGN in the clamp of the current gradients), so the results are
 * the bits of the reference compiled without contraction.
 *
 * Not served: fast-wave sub-steps (PROPAG_WAM sub-steps only in CASE(2)), the one-kernel step.  IPROPAGS = 1 (PROPAGS1) has a header of its own,
 * ecwam_hipx_propags1.h.
 */
#ifndef ECWAM_HIP_PROPAGS_H
#define ECWAM_HIP_PROPAGS_H

#include "ecwam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the row of dot terms of a point: reals [3 NANG + 4]
 *   [0, NANG)        THDD(IJ,K)    zeros unless IREFRA is 1 or 3
 *   [NANG, 2 NANG)   THDC(IJ,K)    zeros unless IREFRA is 2 or 3
 *   [2 NANG, 3 NANG) S0(K): SDOT(IJ,K,NFRE_RED) as propdot.F90:178 leaves it before the loop over the frequencies; zeros unless IREFRA is 2 or 3
 *   [3 NANG]         OMDD(IJ)      zero unless IREFRA is 3
 *   [3 NANG + 1, 3 NANG + 4)       padding, written as zeros (the row stays a whole number of 16-byte pieces for every even NANG)
 * SDOT(IJ,K,M) is not stored: ecwam_hip_propags rebuilds it as (S0(K) CGROUP(M) + OMDD OMOSNH2KD(M)) WAVNUM(M), the expression of propdot.F90:190-191. */
#define ECWAM_HIP_PROPAGS_DOT_W(nang) (3 * (nang) + 4)

/* the flags of ecwam_hip_propags */
#define ECWAM_HIP_PROPAGS_CARTESIAN 1 /* ICASE = 2 (otherwise ICASE = 1, spherical) */
#define ECWAM_HIP_PROPAGS_IRREGULAR 2 /* IRGG = 1: section 4 weighs four latitude neighbours with WLAT and 1 - WLAT (otherwise IRGG = 0) */

/* GRADI + PROPDOT for rows [0,n), statement by statement: dot [n][3 NANG + 4] as above.  icase is 1 or 2 (DCO = COSPHM1_EXT or 1, propdot.F90:120-128).
 * DELPHI = xdella CIRC / 360 and DELLAM(KX) = zdello[KX] CIRC / 360 are formed in the working precision as readmdlconf.F90:136, 145 do.  The geometry arguments
 * are those of ecwam_hip_propdot.  With IREFRA = 0 the row is zeros.  One thread per point.
 * Refused: icase other than 1 or 2; n < 0 or nland < n ("bad range"); a null pointer; dot not 16-byte aligned. */
int ecwam_hip_propags_dot(ecwam_hip_ctx *ctx, int n, int nland, int icase, const int *kxlt, const void *zdello, double xdella, const void *cosph,
                          const int *klon, const int *klat, const void *wlat, const void *cosphm1_ext, const void *depth_ext, const void *u_ext,
                          const void *v_ext, void *dot, void *stream);

/* PROPAGS for rows [kijs,kijl) of f3 from f1, every section: flags selects ICASE and IRGG, the context IREFRA.
 *   n, nland        the rows the tables KLON, KLAT, WLAT, KXLT and dot have; the index of the land row in f1 and the *_ext arrays
 *   ngy             the entries of cosph and sinph
 *   delpro          DELPRO = REAL(IDELPRO): a whole number of seconds
 *   delphi          DELPHI in the working precision (readmdlconf.F90:136)
 *   dellam1_ext     1 / DELLAM(KXLT) per row, cosphm1_ext 1 / COSPH(KXLT) per row (mpdecomp.F90:1428-1429); row 0 is NINF
 *   kxlt, cosph, sinph, wlat, cosphm1_ext   not read on a Cartesian grid (may be NULL)
 *   omosnh2kd_ext   read with IREFRA /= 0; wavnum_ext, u_ext, v_ext with IREFRA 2, 3; dot [n][3 NANG + 4] with IREFRA /= 0: NULL otherwise
 *   copy_rest       the frequencies above NFRE_RED of the rows written are copied from f1; otherwise they keep their bits
 *   cfl             NULL, or reals [n][NANG][11]: on a spherical grid, for rows [kijs,kijl) and every direction, what PROPAGS passes to CHECKCFL at M = 1 after
 *                   DEPTH, in the order of its arguments: DTC, CFLEA, CFLWE, CFLNO, CFLSO, CFLNO2, CFLSO2, CFLTP, CFLTM, CFLOP, CFLOM.  Section 3 passes
 *                   CFLEA twice, CFLNO four times and CFLTP, CFLTM a second time in the place of CFLOP, CFLOM (propags.F90:719-721)
 *   cflfail         NULL, or int [n]: set to 1 where one of the eleven numbers of some direction exceeds 1 (where the reference aborts); never cleared.  The
 *                   Cartesian sections call no check: cfl and cflfail stay as they are
 *   f3              NULL: the check alone, no spectrum is written
 * With ecwam_hip_set_obstructions the planes OBSLAT(:,:,1:2) and OBSLON(:,:,1:2) (the first four of OBS[ij][8][NFRE]) scale the weights of the spherical
 * sections: in section 3 as the product with the midpoint velocity that propags.F90:564-575 forms on the first call (OBS CGK first, then XX (...)), in
 * section 4 as they are.  A Cartesian section reads none.  IRGG = 0 with a table whose klat[..][1] differs from klat[..][0] is the caller's business.
 * A thread owns a 16-byte piece of consecutive frequencies of one (point, direction); the piece NFRE_RED cuts is handled element by element.
 * Refused: unknown flag bits; a delpro that is no whole number; delphi <= 0; "bad range" (kijs < 0, kijl < kijs, kijl > n, nland < n); a null pointer where the
 * call reads or writes; f1 == f3; f1, f3 or a row of frequencies misaligned to 16 bytes; NFRE no whole number of 16-byte pieces; more points than the
 * obstruction table holds; a tile that does not fit the LDS (no direction count or NFRE a context can have). */
int ecwam_hip_propags(ecwam_hip_ctx *ctx, const void *f1, void *f3, int n, int nland, int ngy, double delpro, double delphi, int flags, const int *kxlt,
                      const void *cosph, const void *sinph, const void *dellam1_ext, const void *cosphm1_ext, const int *klon, const int *klat,
                      const void *wlat, const void *cgroup_ext, const void *omosnh2kd_ext, const void *wavnum_ext, const void *u_ext, const void *v_ext,
                      const void *dot, int kijs, int kijl, int copy_rest, void *cfl, int *cflfail, void *stream);

#ifdef __cplusplus
}
#endif
#endif
