/*
 * The start and the end of a run on the device: what WAVEMDL's sequence does with a model field before the first step and after the last one --
 * INITDPTHFLDS with DEPTHPRPT and AKI (initdpthflds.F90:54-88, depthprpt.F90:60-82, aki.F90:71-91), BUILDSTRESS with the statements GETSTRESS puts
 * around it (buildstress.F90:231-318, getstress.F90:95-97, 294-303), the sixteen restart fields of SAVSTRESS / GETSTRESS (savstress.F90:112-127,
 * getstress.F90:150-165) and the record of WRITEFL (writefl.F90:112-118), the last two with the IJ2NEWIJ relabelling of a global file
 * (writefl.F90:117, writestress.F90:105).  The host keeps the files, the dates, GRSTNAME and the exchanges between tasks.  The six calls are
 * additions to ABI 6 (ECWAM_HIP_ABI_VERSION stays 6) in a header of their own: the lists of entry points the other headers were published with
 * stay the ones they were.
 *
 * The conventions are those of ecwam_hip_forcing.h: device pointers unless called HOST; rows [kijs,kijl), 0-based; the launch goes to `stream`;
 * 0 on success, otherwise 1 with the reason in ecwam_hip_last_error; an empty range launches nothing.  No call except the setter allocates or
 * waits.  The order of the refusals: the null context ("null context"), then what the call itself refuses (flags, options, fields, a missing
 * map), then the range ("bad range": kijl < kijs, kijs < 0, rows beyond a map the call goes through, ld too small), then the buffers (null where
 * the call touches them, or misaligned: ff, fl1, wvprpt, the planes and the rows of frequencies to 16 bytes, field vectors and per-point
 * vectors to a real).  The arithmetic is the reference's, in its order, in the working precision and without contraction; TANH, COSH, SINH
 * are the device library's, the POW and EXP of CDUSTARZ0 and BUILDSTRESS those the forcing header's CDUSTARZ0 uses.
 *
 * ff is [ij][16] as in ecwam_hip.h: columns 0 .. 13 FF_NOW (AIRD WDWAVE CICOVER WSWAVE WSTAR USTRA VSTRA UFRIC TAUW TAUWDIR Z0M Z0B CHRNCK
 * CITHICK), 14 EMAXDPT, 15 DEPTH.  It is read and written in whole 16-byte pieces, and only the pieces that hold a column a call reads or writes.
 *
 * Not served: the unstructured branch (UNBLKRORD), a relabelled read of spectra, files, dates, MPGATHERSCFLD / MPDISTRIBSCFLD.
 */
#ifndef ECWAM_HIP_RESTART_H
#define ECWAM_HIP_RESTART_H

#include "ecwam_hip_forcing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what the context lacks for DEPTHPRPT: DKMAX (yowpcons.F90, the deep-water exit of AKI) and GAM_B_J (yowshal.F90, EMAXDPT) */
typedef struct ecwam_hip_depth_opts {
  double dkmax;
  double gam_b_j;
} ecwam_hip_depth_opts;

/* the flags of ecwam_hip_buildstress */
#define ECWAM_HIP_BST_Z0B_ZERO 1 /* FF_NOW%Z0B = 0 (getstress.F90:95-97) */
#define ECWAM_HIP_BST_NSESTART 2 /* LNSESTART: CHRNCK = PRCHAR, TAUW = 0 (getstress.F90:294-303) */

/* the field vectors of the LAW file (savstress.F90:112-127) */
#define ECWAM_HIP_NRESTART_FIELDS 16

/* INITDPTHFLDS for rows [kijs,kijl): per frequency M and point AK = AKI(ZPIFR(M), DEPTH), then DEPTHPRPT's fields with its switch at AK DEPTH <= 10,
 * and EMAXDPT = 0.0625 (GAM DEPTH)**2 with GAM = GAM_B_J DEPTH / 4 below 4 m.  G, PI, FR and ZPIFR are the context's.
 *   depth [>= kijl]            reals; the caller puts BATHYMAX into the land slot and gets WVPRPT_LAND (initdpthflds.F90:82-86) from the same call
 *   wvprpt [ij][5][NFRE]       WAVNUM, CGROUP, CINV, XK2CG, STOKFAC
 *   wavnum, cgroup, omosnh2kd  [ij][NFRE] each: the extended arrays of the advection, halo and land rows included
 *   ff [ij][16]                only EMAXDPT [14] and DEPTH [15] change; the other two reals of that 16-byte piece keep their bits
 * Any output may be NULL, but not all of them.  AKI's start value, its exit BO > DKMAX and its test ABS(AKP-AO) > EBS*AO are evaluated per element as
 * written: every element does its own number of Newton steps (an element that has not met the test after 4096 steps, where the reference would
 * not return, keeps its last iterate).  One thread owns one 16-byte piece of a row of frequencies.
 * Refused: opts NULL; every output NULL; NFRE no whole number of 16-byte pieces. */
int ecwam_hip_depthprpt(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *depth, const ecwam_hip_depth_opts *opts, void *wvprpt, void *wavnum,
                        void *cgroup, void *omosnh2kd, void *ff, void *stream);

/* BUILDSTRESS sections 1.2 to 1.5 and GETSTRESS around it, for rows [kijs,kijl) of ff, in this order:
 *   flags & Z0B_ZERO   Z0B = 0
 *   uwave              a plane [ncell_in] on the inbound map of the forcing header, or NULL: READWGRIB's block step with LLONLYPOS
 *                      (readwgrib.F90:165-175) -- WSWAVE takes the cell's value where it is /= zmiss and > 0
 *   CDUSTARZ0 with ZREF = zref (TEMPXNLEV) gives CD, UFRIC, Z0M; TAUW = 0.1 UFRIC**2, TAUWDIR = WDWAVE (buildstress.F90:237-241)
 *   cd                 the same kind of plane, or NULL (LNOCDIN / LNSESTART): the same conditional replacement of CD, then the loop of
 *                      buildstress.F90:296-313 with ALPHAOG = CHNKMIN(WSWAVE) GM1 when the context has LLCAPCHNK, else ALPHA GM1; it writes UFRIC,
 *                      Z0M, TAUW, TAUWDIR and CHRNCK
 *   flags & NSESTART   CHRNCK = prchar, TAUW = 0
 * Every other column of ff keeps its bits.  One thread per point.
 * Refused: unknown flag bits; a plane given without an inbound map; rows beyond the map. */
int ecwam_hip_buildstress(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *uwave, const void *cd, double zref, int flags, double prchar,
                          double zmiss, void *ff, void *stream);

/* IJ2NEWIJ, 0-based: ij2newij is a HOST int [npts]; position p of a vector in the global order holds row ij2newij[p] (writefl.F90:117,
 * writestress.F90:105).  The library validates on the host that it is a permutation of [0,npts) and uploads it: no kernel reads an unchecked
 * index.  This call may allocate and wait.  NULL removes the map.  A call that fails a check leaves the map it found.
 * Refused: npts < 0; an index outside [0,npts); an index that occurs twice. */
int ecwam_hip_set_restart_map(ecwam_hip_ctx *ctx, int npts, const int *ij2newij);

/* The restart fields of SAVSTRESS and GETSTRESS: rfield [16][ld], field f at rfield + f ld, in the order of savstress.F90:112-127 -- WSWAVE
 * WDWAVE UFRIC TAUW TAUWDIR Z0M Z0B CHRNCK AIRD WSTAR CICOVER CITHICK USTRA VSTRA (the columns 3 1 7 8 9 10 11 12 0 4 2 13 5 6 of ff), then ucur and
 * vcur (reals [>= kijl]).  Row ij is at position ij, or with relabel != 0 at the position p with ij2newij[p] = ij; ld >= kijl without, ld >= npts
 * of the map with relabel.
 * _pack reads ff and the currents and writes the positions of rows [kijs,kijl) in the sixteen vectors; every other position keeps its bits.
 * _unpack is the inverse (getstress.F90:150-165): the columns 14 and 15 of ff and every other row keep their bits.
 * Refused: relabel without a map; rows beyond the map; ld too small. */
int ecwam_hip_savstress_pack(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *ff, const void *ucur, const void *vcur, int relabel, void *rfield,
                             int ld, void *stream);
int ecwam_hip_getstress_unpack(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *rfield, int ld, int relabel, void *ff, void *ucur, void *vcur,
                               void *stream);

/* WRITEFL's record from FL1 [ij][NANG][NFRE]: blk [nfld][ld] receives the fields [ifld0, ifld0 + nfld), f = (M-1) NANG + (K-1) up to NANG NFRE, of rows
 * [kijs,kijl), row positions and ld as above.  With every field and every row blk is the record (((FL(IJ,K,M),IJ),K),M) of writefl.F90:113
 * (relabel = 0) or :117 (relabel != 0), byte for byte.  No ice mask, no arithmetic; every other element of blk keeps its bits.
 * Refused: a field range outside [0, NANG NFRE); relabel without a map; rows beyond the map; ld too small; NFRE no whole number of 16-byte pieces.
 * (The tile [64][NANG VEC | 1] fits the LDS for every direction count a context can have.) */
int ecwam_hip_savspec_pack(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, int ifld0, int nfld, int relabel, void *blk, int ld, void *stream);

#ifdef __cplusplus
}
#endif
#endif
