/*
 * The dual rotated-quadrant propagation scheme on the device: what PROPAG_WAM does with IPROPAGS = 1 (propag_wam.F90:296-322, where the reference's own
 * GPU build aborts) -- PROPAGS1 (propags1.F90:10-1171; J. Bidlot 2004, "first order propagation scheme based on 2 rotated quadrants") with CHECKCFL as its
 * spherical sections call it (:867-878, 1096-1100).  The two calls are additions to ABI 6 (ECWAM_HIP_ABI_VERSION stays 6).
 *
 * Naming.  The list of entry points with the prefix ecwam_hip_ is held closed by the tests of the headers it was published with.  Additions from here on
 * take the prefix ecwam_hipx_ and are listed in lib.EXPORTS_X_* of the Python bindings.
 *
 * The conventions are those of ecwam_hip.h: device pointers; rows 0-based, the land row at index nland (after the halo rows); spectra FL[row][NANG][NFRE];
 * KLON [n][2], KLAT [n][2][2], WLAT [n][2]; the *_ext arrays cover every row up to and including the land row; the launch goes to `stream`; 0 on success,
 * otherwise 1 with the reason in ecwam_hip_last_error; an empty range launches nothing.  IREFRA is the context's.
 *
 * The arithmetic is the reference's, expression by expression in its order, in the working precision, without contraction and with correctly rounded
 * divisions.  PROPAGS1 holds only + - * / and ABS, so the results are the bits of the reference compiled without contraction.
 *   section 3 (spherical, IREFRA 0 or 1)   the new scheme: a kernel of its own
 *   sections 1, 2 (Cartesian)              those of PROPAGS: the kernel of the IPROPAGS = 0 call, unchanged; its bits
 *   section 4 (spherical, IREFRA 2 or 3)   that of PROPAGS with DP1, DP2 = DCO(IJ) * (1 / DCO(JH)) (propags1.F90:203-222) in place of the quotient: the same
 *                                          kernel built with the product form; it may differ from the IPROPAGS = 0 call in the last place
 *
 * Not served: a WAMINTGR_HIP branch, the one-kernel step, a decomposed grid (the halo of the Python driver does not hold the rotated neighbours), fast-wave
 * sub-steps.
 */
#ifndef ECWAM_HIPX_PROPAGS1_H
#define ECWAM_HIPX_PROPAGS1_H

#include "ecwam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the flags of ecwam_hipx_propags1: the values of the IPROPAGS = 0 call */
#define ECWAM_HIPX_PROPAGS1_CARTESIAN 1 /* ICASE = 2 (otherwise ICASE = 1, spherical) */
#define ECWAM_HIPX_PROPAGS1_IRREGULAR 2 /* IRGG = 1: section 4 weighs four latitude neighbours with WLAT and 1 - WLAT (otherwise IRGG = 0) */

/* The tables of the rotated quadrants, kept by pointer as ecwam_hip_set_obstructions keeps its table (the caller keeps them alive):
 *   krlat, krlon   int [n][2][2]: (south, north) x (closest, second closest).  KRLAT holds the SE and NW neighbours, KRLON the SW and NE ones, as PROPCONNECT
 *                  fills them with IPROPAGS = 1 (propconnect.F90:436-650), 0-based, a land neighbour = the index of the land row (mpdecomp.F90 step 5)
 *   wrlat, wrlon   reals [n][2]: the weight of the closest point (propconnect.F90:754-821, 893-961)
 *   cdr, sdr       reals [nrow][NANG]: mpdecomp.F90:1192-1241, for every row a point or a neighbour can be, nrow > n (the land row is not read)
 *   prqrt          reals [n]: the fraction of the rotated grid (mpdecomp.F90:1242-1254)
 *   sqrt2          2 SIN(PI / 4) as the working precision evaluates it (propags1.F90:570), in a double
 * All table pointers NULL switches the tables off.
 * Refused: n < 0, or nrow <= n with tables ("bad size"); some pointers NULL and others not; a sqrt2 that is not positive. */
int ecwam_hipx_set_rotated(ecwam_hip_ctx *ctx, int n, int nrow, const int *krlat, const int *krlon, const void *wrlat, const void *wrlon, const void *cdr,
                           const void *sdr, const void *prqrt, double sqrt2);

/* PROPAGS1 for rows [kijs,kijl) of f3 from f1, every section: flags selects ICASE and IRGG, the context IREFRA.  The arguments are those of the IPROPAGS = 0
 * call, one for one and in its order; dot is the row of dot terms [n][3 NANG + 4] of that scheme's dot call (read with IREFRA /= 0).
 *   cfl             NULL, or reals [n][NANG][11]: on a spherical grid what PROPAGS1 passes to CHECKCFL at M = 1 after DEPTH, in the order of its arguments.
 *                   Section 3 passes the unrotated numbers rescaled by 1 / (1 - PRQRT) and a DTC of them alone: DTC, CFLEA twice, CFLNO four times, CFLTP,
 *                   CFLTM, and CFLTP, CFLTM again (propags1.F90:867-878); F3 has used the full DTC
 *   cflfail         NULL, or int [n]: set to 1 where one of the eleven numbers of some direction exceeds 1; never cleared
 *   f3              NULL: the check alone, no spectrum is written
 * With ecwam_hip_set_obstructions section 3 reads all eight planes of OBS[ij][8][NFRE]: OBSLAT(:,:,1:2) and OBSLON(:,:,1:2) as the product with the midpoint
 * velocity that propags1.F90:656-668 forms on the first call, OBSRLAT(:,:,1:2) (planes 4-5) and OBSRLON(:,:,1:2) (planes 6-7) as they are (:804, 816).
 * Section 3, a thread owns a 16-byte piece of consecutive frequencies of one (point, direction); per point the rows CGKLON, CGKLAT, their products with the
 * obstructions, CGROUP of the point and of its eight rotated neighbours and the nine rows of CDR and SDR go through LDS once.
 * Refused: on a spherical grid with IREFRA 0 or 1, no rotated tables set, fewer points or rows in them than the call reads; unknown flag bits; a delpro that is
 * no whole number; delphi <= 0; "bad range" (kijs < 0, kijl < kijs, kijl > n, nland < n); a null pointer where the call reads or writes; f1 == f3; f1, f3 or a
 * row of frequencies misaligned to 16 bytes; NFRE no whole number of 16-byte pieces; more points than the obstruction table holds; a tile that does not fit
 * the LDS (the tile is never cut short). */
int ecwam_hipx_propags1(ecwam_hip_ctx *ctx, const void *f1, void *f3, int n, int nland, int ngy, double delpro, double delphi, int flags, const int *kxlt,
                        const void *cosph, const void *sinph, const void *dellam1_ext, const void *cosphm1_ext, const int *klon, const int *klat,
                        const void *wlat, const void *cgroup_ext, const void *omosnh2kd_ext, const void *wavnum_ext, const void *u_ext, const void *v_ext,
                        const void *dot, int kijs, int kijl, int copy_rest, void *cfl, int *cflfail, void *stream);

#ifdef __cplusplus
}
#endif
#endif
