/*
 * The forcing intake on the device: what PREWIND runs in front of GETWND -- INIT_FIELDG, IFSTOWAM's arithmetic (FLDINTER, through the tables of
 * INITIALINT) and the point-wise branches of RECVNEMOFIELDS -- and what WAMODEL runs at its end for NEMO (UPDNEMOFIELDS, UPDNEMOSTRESS).  They
 * fill and use the planes fieldg[13][ncell_in] that ecwam_hip_getwnd, _wamadswstar and _getcurr read (ecwam_hip_forcing.h), so that a coupled run
 * uploads the blocks it received, not thirteen interpolated planes.  The five calls are additions to ABI 6 (ECWAM_HIP_ABI_VERSION stays 6) in a
 * header of their own: the lists of entry points the other headers were published with stay the ones they were.
 *
 * The conventions are those of ecwam_hip_forcing.h: device pointers unless called HOST; rows [kijs,kijl), 0-based; the launch goes to `stream`;
 * 0 on success, otherwise 1 with the reason in ecwam_hip_last_error.  Refused by all: a null context ("null context"); by the calls on rows:
 * kijs < 0 or kijl < kijs ("bad range"), rows beyond the map or the table where the call reads one ("bad range"), a buffer the call reads or
 * writes that is null (with a range that is not empty) or not 16-byte aligned (checked for an empty range too).  An empty range launches
 * nothing.  No call on rows allocates or waits.  The order of the refusals is that of ecwam_hip_forcing.h: the null context, then the range (with
 * ld < kijl, ncell < 0 and rows beyond a map or table), then what the call itself refuses, then the buffers.
 *
 * Layouts: fieldg, nemo, ucur, vcur, ff, intf as in ecwam_hip_forcing.h;
 *   fields[nfields][ngptotg]  reals: FIELDS(NGPTOTG,NFIELDS) as Fortran stores it, in the order of fldinter.F90:52-61 (U10, V10, air density, w*,
 *                             sea ice fraction, lake fraction, the two surface stresses, the two surface currents)
 *   wam2nemo[ij][13]          double, the WAVE2OCEAN rows of ecwam_hip_implsch
 * The arithmetic is the reference's, in its order and without contraction; products and clips with a NEMO value are formed in double (JWRO)
 * and rounded once on the store.  CURRENT_MAX = 1.5 (yowcurr.F90:18) is a constant of the library, WSPMIN the context's.
 */
#ifndef ECWAM_HIP_INTAKE_H
#define ECWAM_HIP_INTAKE_H

#include "ecwam_hip_forcing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the switches of ecwam_hip_fldinter: the logicals of fldinter.F90:142; NEWCURR = LLNEWCURR .AND. .NOT. LWNEMOCOUCUR, evaluated by the host */
#define ECWAM_HIP_FLI_LADEN 1
#define ECWAM_HIP_FLI_LGUST 2
#define ECWAM_HIP_FLI_LLKC 4
#define ECWAM_HIP_FLI_LWCUR 8
#define ECWAM_HIP_FLI_NEWCURR 16

/* the switches of ecwam_hip_recvnemofields: its two arguments and the logicals of YOWCOUP it reads */
#define ECWAM_HIP_RNF_LREST 1
#define ECWAM_HIP_RNF_LINIT 2
#define ECWAM_HIP_RNF_LWCOU 4
#define ECWAM_HIP_RNF_LWNEMOCOUCIC 8
#define ECWAM_HIP_RNF_LWNEMOCOUCIT 16
#define ECWAM_HIP_RNF_LWNEMOCOUCUR 32
#define ECWAM_HIP_RNF_LWNEMOCOUIBR 64

/* The per-point table of FLDINTER, built once per decomposition from INITIALINT's tables and IJBLOCK.  HOST arrays:
 *   idx[npts][4]  the 0-based positions in a field vector of IJBLOCK(II,JJ), IJBLOCK(II1,JJ), IJBLOCK(IIP,JJ1), IJBLOCK(IIP1,JJ1), exactly as
 *                 fldinter.F90:227-247 forms them (II1 = MIN(II+1, ILONRGG(JSN)+IPERIODIC), the clamped JJ1)
 *   w[npts][3]    double: DJ1M(J), DII1M(I,J), DIIP1M(I,J), each a value of the working precision widened; the library narrows it back unchanged
 * interpol = 0 is LLINTERPOL = F: only idx[ij][0] = IJBLOCK(I,J) - 1 is read (fldinter.F90:181-186) and w may be NULL.
 * In single precision a weight that a float does not hold exactly is refused, so that narrowing changes nothing.
 * The library validates on the host and uploads: no kernel ever reads an unchecked index.  A call that fails leaves the table it found, or
 * (where the upload itself fails) none.  idx = NULL removes the table; so does a later ecwam_hip_set_forcing_map, whose map the table was
 * checked against.
 * Refused: npts < 0; ngptotg < 1; w NULL with interpol; an index outside [0, ngptotg); a weight that is no value of the working precision; no
 * inbound map of ecwam_hip_set_forcing_map, or one of another length; an inbound map that names a cell twice (two rows writing one cell of
 * fieldg would make the result depend on their order). */
int ecwam_hip_set_fldinter(ecwam_hip_ctx *ctx, int npts, int ngptotg, const int *idx, const double *w, int interpol);

/* FLDINTER (fldinter.F90:176-374) for the rows given.  Writes, through the inbound map, the planes UWND, VWND, AIRD (LADEN, or roair), WSTAR
 * (LGUST, or wstar0), CICOVER (with the missing-value rule of fldinter.F90:276-330 against pmiss), CITHICK = 0, LKFR (LLKC, or 0), USTRA, VSTRA
 * of fieldg[13][ncell_in] and, with NEWCURR, UCUR and VCUR (fields 9 and 10 with LWCUR, or 0); nothing else: WSWAVE, WDWAVE, the cells of other
 * rows and (without NEWCURR) the current planes keep their bits.
 * mask_in: a device int[ngptotg], 16-byte aligned like every buffer, or NULL.  Every source position a row reads becomes 1 (MASK_IN): every
 * thread stores the same 1, as `changed` of ecwam_hip_getcurr is written.  The call never clears it.
 * Refused: unknown flags; no table; ngptotg other than the table's; nfields < 8, or nfields < 10 with NEWCURR and LWCUR. */
int ecwam_hip_fldinter(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fields, int ngptotg, int nfields, int flags, double roair, double wstar0,
                       double pmiss, void *fieldg, int *mask_in, void *stream);

/* The LLINIALL branch of INIT_FIELDG (init_fieldg.F90:92-116) for the thirteen planes of fieldg[13][ncell]: 0 everywhere, except WSWAVE = WSPMIN,
 * AIRD = roair and WSTAR = wstar0.  XLON and YLAT are not planes of the device's fieldg: they stay with the host.
 * Refused: ncell < 0; fieldg null (with ncell > 0) or not 16-byte aligned. */
int ecwam_hip_init_fieldg(ecwam_hip_ctx *ctx, void *fieldg, int ncell, double roair, double wstar0, void *stream);

/* The point-wise branches of RECVNEMOFIELDS.  ZNEMOTOWAM(NTOTIJ,1:4) of NEMOGCMCOUP_WAM_GET is the block nemo[4][kijl] already: the receive itself
 * needs no kernel.  nemoibr: double[kijl] (NEMOCIIBR), read or written with LWNEMOCOUIBR only.
 *   LREST (recvnemofields.F90:101-110)           nemo <- CICOVER [2] and CITHICK [13] of ff, ucur, vcur; nemoibr <- IBRMEM = intf[ij][15]
 *   LINIT with LWCOU (recvnemofields.F90:176-235) where LKFR of fieldg <= 0: CICOVER (LWNEMOCOUCIC) and CITHICK = NEMOCICOVER NEMOCITHICK
 *                                                (LWNEMOCOUCIT) of ff, ucur / vcur clipped at CURRENT_MAX as ecwam_hip_getcurr mode 1 clips
 *                                                (LWNEMOCOUCUR), IBRMEM (LWNEMOCOUIBR) from nemo / nemoibr; elsewhere the reference's other
 *                                                branch: CICOVER of fieldg; CICOVER = 0.5 NEMOCICOVER (line 201, as the reference has it); zero
 *                                                currents; IBRMEM from nemoibr all the same
 *   LINIT without LWCOU (recvnemofields.F90:240-250)  the plain copies
 * With both, LREST runs first, as in the reference.  ff and intf are touched in whole 16-byte pieces, only those a branch reads or writes.
 * A buffer no branch of the flags reads or writes may be NULL: fieldg (and the map's entries) are read only with LINIT, LWCOU and one of
 * LWNEMOCOUCIC, LWNEMOCOUCIT, LWNEMOCOUCUR -- IBRMEM takes NEMO's value on either side of the lake test and asks for neither.
 * Refused: unknown flags; both LREST and LINIT clear; no inbound map with LINIT and LWCOU. */
int ecwam_hip_recvnemofields(ecwam_hip_ctx *ctx, int kijs, int kijl, int flags, const void *fieldg, double *nemo, double *nemoibr, void *ff, void *ucur,
                             void *vcur, void *intf, void *stream);

/* UPDNEMOFIELDS (updnemofields.F90:92-98): fields7[7][ld] double = NSWH, NMWP, NPHIEPS, NTAUOC, NEMOSTRN, NEMOUSTOKES, NEMOVSTOKES, the argument order
 * of NEMOGCMCOUP_WAM_UPDATE, from wam2nemo.  UPDNEMOSTRESS (updnemostress.F90:84-132): stress6[6][ld] double = NEMOTAUX, NEMOTAUY, NEMOWSWAVE,
 * NEMOPHIF, NEMOTAUICX, NEMOTAUICY, each times ZNEMONTAUM1 = 1 / NEMONTAU formed on the host in the working precision and widened; zeros with
 * nemontau <= 0; afterwards those six columns of wam2nemo are 0.  NEMONTAU = 0 and the call into NEMO are the host's.
 * Either output may be NULL, which skips that half (without stress6 nothing of wam2nemo changes).
 * Refused: ld < kijl. */
int ecwam_hip_updnemo(ecwam_hip_ctx *ctx, int kijs, int kijl, double *wam2nemo, int nemontau, double *fields7, double *stress6, int ld, void *stream);

#ifdef __cplusplus
}
#endif
#endif
