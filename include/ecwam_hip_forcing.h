/*
 * The forcing and coupling seam on the device: what WAVEMDL does immediately before WAMODEL (PREWIND: GETWND = WAMWND + MICEP, GETFRSTWND's
 * CDUSTARZ0, WAMADSWSTAR, GETCURR's WAMCUR and the NEMO currents) and immediately after it (OUTBETA, the WVBLOCK fill, the block-to-grid step
 * of MPFLDTOIFS), on the device-resident FF, INTF and currents.  The seven calls are additions to ABI 6 of ecwam_hip.h (adding symbols is
 * compatible: ECWAM_HIP_ABI_VERSION stays 6) and are declared in a header of their own, so that the lists of entry points of ecwam_hip.h and
 * ecwam_hip_start.h, which the bindings and the tests count, stay the ones they were published with.
 *
 * Common to the calls on rows: device pointers; ff[ij][16] and intf[ij][16] in the layouts of ecwam_hip_implsch; rows [kijs,kijl), 0-based; the
 * launch goes to `stream`; 0 on success, otherwise 1 with the reason in ecwam_hip_last_error.  The conventions are those of ecwam_hip_setice.
 * Refused by all: a null context ("null context"), kijs < 0 or kijl < kijs ("bad range"), rows beyond the map where the call reads one ("bad
 * range"), a buffer the call reads or writes that is null (with a range that is not empty) or not 16-byte aligned (checked for an empty range
 * too).  An empty range launches nothing.
 *
 * Layouts:
 *   fieldg[13][ncell_in]  reals, plane-major, the members of FIELDG the routines read in the order of the enum below; a plane is the
 *                         (NXS:NXE, NYS:NYE) array of the reference, first index fastest; ncell_in is the one given to ecwam_hip_set_forcing_map
 *   nemo                  double [4][kijl] (JWRO), the buffer of ecwam_hip_outblock: NEMOCICOVER, NEMOCITHICK, NEMOUCUR, NEMOVCUR; the planes
 *                         are kijl apart, kijl being that of the call
 *   ucur, vcur            reals [>= kijl]: ENVIRONMENT%UCUR, %VCUR
 * A kernel runs one thread per sea point and touches ff (and intf) in whole 16-byte pieces; a piece of the row that the routine neither reads
 * nor writes is neither loaded nor stored.  The arithmetic is the reference's, in its order and without contraction.
 * C1CD, C2CD, P1CD, P2CD (yowpcons.F90:61-64), AMAX, BMAX, BETAHQ_REDUCE (outbeta.F90:90-96), MICEP's C1 and C2 (micep.F90:98-99) and
 * CURRENT_MAX = 1.5 (yowcurr.F90:18) are constants of the library; WSPMIN, EPSUS, XKAPPA, XNLEV, RNUM, G, GM1, ZPI, ALPHA, ALPHAMIN, ALPHAMAX,
 * HICMIN, CDMAX, LICERUN, LMASKICE and LLGCBZ0 are those of the context.
 */
#ifndef ECWAM_HIP_FORCING_H
#define ECWAM_HIP_FORCING_H

#include "ecwam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the planes of fieldg */
enum {
  ECWAM_HIP_FG_UWND = 0, ECWAM_HIP_FG_VWND, ECWAM_HIP_FG_AIRD, ECWAM_HIP_FG_WSTAR, ECWAM_HIP_FG_CICOVER, ECWAM_HIP_FG_CITHICK, ECWAM_HIP_FG_USTRA,
  ECWAM_HIP_FG_VSTRA, ECWAM_HIP_FG_WSWAVE, ECWAM_HIP_FG_WDWAVE, ECWAM_HIP_FG_LKFR, ECWAM_HIP_FG_UCUR, ECWAM_HIP_FG_VCUR, ECWAM_HIP_NFIELDG
};

/* the switches of ecwam_hip_wvblock (wavemdl.F90:757-802) */
#define ECWAM_HIP_WVB_LWCOU2W 1
#define ECWAM_HIP_WVB_LWCOUHMF 2
#define ECWAM_HIP_WVB_LWSTOKES 4
#define ECWAM_HIP_WVB_LWFLUX 8
#define ECWAM_HIP_MAXWVFIELDS 32

/* The run-time switches of GETWND that are not in ecwam_hip_params (logicals as 0 / 1; reals are rounded to the working precision). */
typedef struct ecwam_hip_forcing_opts {
  int icode_wnd;          /* 1 friction velocity, 2 surface stress, 3 wind at 10 m (ICODE_WND, or ICODE_CPL of a coupled run) */
  int llwswave, llwdwave; /* YOWWIND: FIELDG holds WSWAVE / WDWAVE of a previous wave model run */
  int lcorrel;            /* LCORREL of wamwnd.F90:127-133, evaluated by the host from LWCOU, LWCUR, LRELWIND and IREFRA */
  double rwfac;           /* YOWWIND RWFAC */
  int iparamci;           /* IPARAMCI: 31 sea ice fraction, 139 sea surface temperature */
  int lwcou, lwnemocoucic, lwnemocoucit, lnemoicerest, liceth;
  int swamp;              /* CLDOMAIN == 's' */
  double swampcith;       /* YOWPARAM SWAMPCITH */
  double zmiss;           /* YOWPCONS ZMISS */
} ecwam_hip_forcing_opts;

/* The maps between the rows and the grids: ixy_in[ij] = the cell of fieldg that row ij reads, (JFROMIJ - NYS) nx + (IFROMIJ - NXS); ixy_out[ij] =
 * the cell of the outbound grid that row ij fills, (NGY - KXLT) NGX + (IXLG - 1) (mpfldtoifs.F90:348-350).  HOST int arrays [npts], 0-based.
 * Either may be NULL: that map is then removed, and a call that needs it refuses ("no inbound map", "no outbound map").  The library validates on
 * the host and uploads: no kernel ever reads an unchecked index.
 * Refused: npts < 0, ncell < 1 beside a map, an index outside [0, ncell), a duplicate in ixy_out (two writers to one cell would make the
 * scatter depend on their order).
 * The per-point table of FLDINTER (the setter of ecwam_hip_intake.h) was checked against the inbound map it found: an accepted call here removes it. */
int ecwam_hip_set_forcing_map(ecwam_hip_ctx *ctx, int npts, const int *ixy_in, int ncell_in, const int *ixy_out, int ncell_out);

/* GETWND per chunk (getwnd.F90:211-229): WAMWND (wamwnd.F90:126-294) followed by MICEP (micep.F90:116-254), in one kernel.  Whether ff is the NOW
 * or the NEXT buffer is the caller's choice.  Writes ff columns AIRD [0], WDWAVE [1], CICOVER [2], WSTAR [4], USTRA [5], VSTRA [6], CITHICK [13]
 * and WSWAVE [3] (ICODE_WND 3) or UFRIC [7] (ICODE_WND 1, 2); nothing else.  MICEP reads the CITHICK that WAMWND has just written.
 * ucur / vcur may be NULL unless lcorrel; nemo may be NULL unless lwnemocoucic or lwnemocoucit.
 * Refused: opts NULL; icode_wnd outside 1 .. 3; iparamci other than 31 or 139 while lwnemocoucic is off; no inbound map. */
int ecwam_hip_getwnd(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fieldg, const void *ucur, const void *vcur, const double *nemo, void *ff,
                     const ecwam_hip_forcing_opts *opts, void *stream);

/* CDUSTARZ0 with ZREF = XNLEV as GETFRSTWND calls it (getfrstwnd.F90:125-126, cdustarz0.F90:66-71): UFRIC [7] and Z0M [10] from WSWAVE [3]. */
int ecwam_hip_cdustarz0(ecwam_hip_ctx *ctx, int kijs, int kijl, void *ff, void *stream);

/* WAMADSWSTAR (wamadswstar.F90:60-69): AIRD [0], WSTAR [4], USTRA [5], VSTRA [6] from fieldg.  Refused: no inbound map. */
int ecwam_hip_wamadswstar(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fieldg, void *ff, void *stream);

/* The point-wise part of GETCURR (getcurr.F90:135-198 and 268-278).  mode 0: WAMCUR (wamcur.F90:78-85), the currents of fieldg clipped as
 * SIGN(MIN(ABS(U), CURRENT_MAX), U); mode 1: the NEMO currents (nemo planes 2, 3) with the same clip where LKFR <= 0, zero elsewhere; mode 2: zero.
 * changed: a device int, or NULL.  It becomes 1 if U or V of any point differs from what the buffer held before (KUPDATE): every thread that
 * sees a change stores the same 1.  The call never clears it; clearing it and reading it back is the caller's business.
 * fieldg may be NULL in mode 2, nemo unless mode 1.  Refused: mode outside 0 .. 2; no inbound map (modes 0, 1). */
int ecwam_hip_getcurr(ecwam_hip_ctx *ctx, int kijs, int kijl, int mode, const void *fieldg, const double *nemo, void *ucur, void *vcur, int *changed,
                      void *stream);

/* The WVBLOCK fill of wavemdl.F90:757-802: OUTBETA (outbeta.F90:113-125, without CD=) gives BETAM and BETAHQ from WSWAVE [3], UFRIC [7], Z0M [10],
 * Z0B [11], CHRNCK [12] of ff when flags has LWCOU2W; otherwise BETAM = prchar.  Then wvblock[ifld][ld] (ld >= kijl) receives, in the reference's
 * order: BETAM; BETAHQ when LWCOUHMF; USTOKES, VSTOKES when LWSTOKES; PHIOCD, TAUOCXD, TAUOCYD, TAUICX, TAUICY, WSEMEAN, WSFMEAN when LWFLUX
 * (columns 2, 3; 12, 7, 8, 10, 11, 0, 1 of intf); zeros up to nwvfields.  ff may be NULL without LWCOU2W, intf without LWSTOKES and LWFLUX.
 * Refused: unknown flag bits; LWCOUHMF without LWCOU2W (the reference leaves BETAHQ undefined there); nwvfields smaller than the switches need,
 * or above ECWAM_HIP_MAXWVFIELDS; ld < kijl. */
int ecwam_hip_wvblock(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *ff, const void *intf, int flags, int nwvfields, double prchar, void *wvblock,
                      int ld, void *stream);

/* The one-task form of MPFLDTOIFS (mpfldtoifs.F90:105-118, 346-352).  With defval (HOST double[nwvfields]) not NULL the whole
 * grid[ifld][ncell_out] is set to the defaults first (LLINIT_GRID); then rows [kijs,kijl) of wvblock[ifld][ld] are scattered through the outbound
 * map.  The exchange between tasks stays with the host.
 * Refused: no outbound map; nwvfields outside 1 .. ECWAM_HIP_MAXWVFIELDS; ld < kijl. */
int ecwam_hip_fldtoifs(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *wvblock, int ld, int nwvfields, const double *defval, void *grid, void *stream);

#ifdef __cplusplus
}
#endif
#endif
