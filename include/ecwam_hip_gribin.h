/*
 * Warm start on the device: the decoded GRIB spectra of GETSPEC and the record of READFL into FL1, the inverse of the output path of
 * ecwam_hip_gribout.h.  GETSPEC's GRIB read (getspec.F90:396-660) with GRIB2WGRID's un-scaling and full copy (grib2wgrid.F90:764-802) does,
 * per field (K, M): un-scale the decoded vector, copy it into FIELD(IX,IY), gather WORK(IJ) = FIELD(IXLG, NGY-KXLT+1), store
 * FL1(IJ,K,M) = WORK with ZMISS -> EPSMIN; after the last field ecwam_hip_getspec_tail (ecwam_hip_start.h) fills the tail and applies
 * SDEPTHLIM.  The host uploads the vectors exactly as eccodes (or the READ of readfl.F90) handed them over and never reorders a spectrum:
 * the transposition from field-major vectors into the point-major fl1[ij][NANG][NFRE] runs here.  The two calls are additions to ABI 6 of
 * ecwam_hip.h (adding symbols is compatible: ECWAM_HIP_ABI_VERSION stays 6), declared in a header of their own as those of
 * ecwam_hip_gribout.h.  eccodes, the dates and the index checks, the sends between tasks and GRIB2WGRID's interpolation between different
 * grids (LLINTERPOL, the nearest-point fill) stay with the host.
 *
 * Common to both calls: device pointers; fl1[ij][NANG][NFRE] in the layout of ecwam_hip_implsch; rows [kijs,kijl), 0-based; a field is
 * f = (M - 1) NANG + (K - 1); the launches go to `stream`; 0 on success, otherwise 1 with the reason in ecwam_hip_last_error.  With
 * v the value read for element (ij, K, M), in the working precision, without contraction and in the reference's order:
 *   ECWAM_HIP_GETSPEC_UNSCALE   v /= ZMISS: v = 10**(v - |PPREC|) - PPEPS; a missing value stays ZMISS      (grib2wgrid.F90:771-775)
 *   ECWAM_HIP_GETSPEC_MISSING   then v == ZMISS: v = EPSMIN of the context                                    (getspec.F90:550-552, 611-613)
 * and FL1(ij,K,M) = v.  Nothing is clamped (the reference clamps nothing).  Only the elements (ij, K, M) with ij in [kijs,kijl) and f in
 * [ifld0, ifld0 + nfld) are written: every other element of fl1 keeps its bits.  An empty row range launches nothing.  No call allocates
 * or waits for the device, so a sequence of calls can be captured into a graph like the output calls.  opts is read only for the flags that
 * need it: pprec, ppeps and zmiss for bit 0, zmiss for bit 1; with flags = 0 it may be NULL.
 * Refused by both: a null context ("null context"); kijs < 0 or kijl < kijs ("bad range"); ifld0 < 0, nfld < 1 or a field range that
 * leaves the fields of the call ("bad field range"); unknown flag bits ("unknown flags"); opts NULL with a flag set ("null options"); a
 * null pointer with a range that is not empty ("null pointer"); fl1 not 16-byte aligned, the source not aligned to a real (checked for an
 * empty range too); NFRE no whole number of 16-byte pieces; a spectral size whose tile does not fit the LDS.
 */
#ifndef ECWAM_HIP_GRIBIN_H
#define ECWAM_HIP_GRIBIN_H

#include "ecwam_hip_gribout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECWAM_HIP_GETSPEC_UNSCALE 1  /* v != ZMISS: 10**(v - |PPREC|) - PPEPS (grib2wgrid.F90:764-778); a missing value stays ZMISS */
#define ECWAM_HIP_GETSPEC_MISSING 2  /* then ZMISS -> EPSMIN of the context (getspec.F90:550-552, 611-613) */

/* GETSPEC's GRIB read on one task: values[f - ifld0][fstride], the vectors as IGRIB_GET_VALUE(...,'values',...) returned them
 * ('missingValue' set to ZMISS), field f = (M-1) NANG + (K-1); FL1[ij][K][M] = g(values[f - ifld0][ival[ij]]) for rows [kijs,kijl).
 * ival is the map of ecwam_hip_set_grib_map (row -> position in the vector): the position of the row in the decoded vector when the message
 * was written by the same configuration (the restart case), and what GRIB2WGRID's full copy (grib2wgrid.F90:793-802, which has no start
 * offset) followed by GETSPEC's gather gives whenever the output's ICOUNT is 1 (a reduced grid, or CLDOMAIN = 'm').  For a message laid out
 * otherwise (a regular grid whose encoded vector begins north of the model's first row) the host sets the map of the read
 * (ecwam_amd/gribout.py::read_map) before this call and the output map afterwards; the pole ranges of the map play no part here.
 * Fields up to NANG * NFRE_RED.  Refused besides the common list: no map ("no grib map"); rows beyond the map ("bad range");
 * fstride < ntencode of the map ("bad range"). */
int ecwam_hip_getspec_values(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *values, long long fstride, int ifld0, int nfld, int flags,
                             const ecwam_hip_grib_opts *opts, void *fl1, void *stream);

/* The receiving half on many tasks (ZRECVBUF / WORK(IST:IEND), getspec.F90:541-557, 602-619) and READFL's record:
 * blk[f - ifld0][ld], row ij at index ij (the convention of ecwam_hip_outspec_pack); needs no map;
 * fields up to NANG * NFRE, so that with flags = 0 and all fields the restart record is served as the file holds it.
 * Refused besides the common list: ld < kijl ("bad range"). */
int ecwam_hip_getspec_unpack(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *blk, long long ld, int ifld0, int nfld, int flags,
                             const ecwam_hip_grib_opts *opts, void *fl1, void *stream);

#ifdef __cplusplus
}
#endif
#endif
