/*
 * GRIB-ready spectra and parameter fields on the device: the last stretch of the output path, from the arrays on the device to the vector VALUES
 * that is handed to the GRIB encoder.  OUTSPEC (outspec.F90:95-133: the sea-ice mask), OUTWSPEC (outwspec.F90:186-195: the field-major send
 * buffer; 219-227: block to grid), MAKEGRID (makegrid.F90:156-160) and WGRIBENCODE_VALUES (wgribencode_values.F90:93-197: value order, pole
 * padding, LOG10 scale, per-field maximum, threshold to missing).  The four calls are additions to ABI 6 of ecwam_hip.h (adding symbols is
 * compatible: ECWAM_HIP_ABI_VERSION stays 6) and are declared in a header of their own, as those of ecwam_hip_start.h and ecwam_hip_forcing.h.
 * eccodes and its handles, the dates and MARSTYPE, the exchange between tasks, FDB and the IFS IO server stay with the host.
 *
 * Common to the calls on rows: device pointers; fl1[ij][NANG][NFRE] and ff[ij][16] in the layouts of ecwam_hip_implsch; rows [kijs,kijl),
 * 0-based; the launches go to `stream`; 0 on success, otherwise 1 with the reason in ecwam_hip_last_error.  Refused by all: a null context
 * ("null context"), kijs < 0 or kijl < kijs or rows beyond the map ("bad range"), a buffer the call reads or writes that is null (with a range
 * that is not empty) or misaligned (checked for an empty range too: 16 bytes; for ecwam_hip_grib_values a real), no map
 * ("no grib map").  An empty range launches nothing and writes nothing.  No call allocates or waits for the device: the per-field maxima live in
 * a scratch that ecwam_hip_set_grib_map sizes (NANG * NFRE_RED fields), so a sequence of calls can be captured into a graph.
 *
 * A field is f = (M - 1) NANG + (K - 1), M <= NFRE_RED: the order of OUTWSPEC's loop over IC.  values[f - ifld0][ntencode].
 * What a call with spectral values does per field, in the reference's order of effects:
 *   1. cells that no row of the map fills are missing;
 *   2. where the map has a pole, every cell of the pole row receives the mean over the non-missing cells of the row beside it, summed in
 *      the reference's order I = 1 .. NLONRGG by one lane (ZMISS if no cell contributes); this acts on the values before the logarithm;
 *   3. every non-missing value v becomes LOG10(v + PPEPS) + |PPREC|, every missing one ZMINSPEC = LOG10(PPEPS) + |PPREC|;
 *   4. PPMAX is the maximum over the field, starting from ZMINSPEC;
 *   5. PPMIN = MIN(PPMISS, PPMAX - (2**NGRBRESS - 1) PPRESOL, PPMIN_RESET);
 *   6. values <= PPMIN become ZMISS.
 * The arithmetic is in the working precision, without contraction.
 * A call on a part of the rows, [kijs,kijl) smaller than the map, writes the cells of those rows, the cells no row fills and the pole rows;
 * the cells of the other rows keep what they held, and those rows count as absent in the pole means and in PPMAX.  (The reference's encoding
 * task sees whole fields: a whole field is one call over all rows.)
 */
#ifndef ECWAM_HIP_GRIBOUT_H
#define ECWAM_HIP_GRIBOUT_H

#include "ecwam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of ecwam_hip_outspec_values / _pack: bit 0 = LICERUN .AND. LLSOURCE (outspec.F90:96): (1 - ZMASK) FL1 + ZMASK FLMIN with
 * ZMASK = CICOVER > CITHRSH; FLMIN and CITHRSH are those of the context */
#define ECWAM_HIP_OUTSPEC_ICEMASK 1

/* One pole of the map: the cells [pole0, pole0 + npole) of VALUES are the pole row, [adj0, adj0 + nadj) the row beside it (the second and the
 * last but one row of FIELD).  npole = 0: no padding at this pole (LPADPOLES off, or NINT((+-90 - AMO?OP) / XDELLA) /= 0). */
typedef struct ecwam_hip_grib_pole {
  int pole0, npole, adj0, nadj;
} ecwam_hip_grib_pole;
typedef struct ecwam_hip_grib_poles {
  ecwam_hip_grib_pole north, south;
} ecwam_hip_grib_poles;

/* YOWGRIBHD's packing constants and YOWPCONS ZMISS (reals are rounded to the working precision) */
typedef struct ecwam_hip_grib_opts {
  double ppmiss, ppeps, pprec, ppresol, ppmin_reset;
  int ngrbress;
  double zmiss;
} ecwam_hip_grib_opts;

/* Once per decomposition.  ival: HOST int [npts], the 0-based position in VALUES that row ij fills (IX = IXLG, IY = NGY - KXLT + 1 of
 * outwspec.F90:223-225, the fill order and the start offset ICOUNT of wgribencode_values.F90:93-100, 152-156; ecwam_amd/gribout.py::value_map
 * builds it from the reference's variables).  poles: HOST, or NULL for no padding.  The library validates on the host, builds the list of the
 * cells no row fills and, for the pole means, the inverse map of the rows beside the poles (cell -> row, or land), uploads them and sizes the
 * scratch of the maxima.  This call allocates and waits for the device.
 * Refused: npts < 0, ntencode < 1, ival NULL beside npts > 0, an index outside [0, ntencode), a duplicate, a pole or adjacent range that is
 * negative, leaves the vector or overlaps another of the four. */
int ecwam_hip_set_grib_map(ecwam_hip_ctx *ctx, int npts, const int *ival, int ntencode, const ecwam_hip_grib_poles *poles);

/* OUTSPEC on one task: fields [ifld0, ifld0 + nfld) of fl1 straight into values[nfld][ntencode], steps 1 - 6.  ff is read only with the ice
 * mask (may be NULL otherwise).  ppmax: device reals [nfld], or NULL: PPMAX per field, from which the packing's reference value derives.
 * Refused: opts NULL; unknown flags; ifld0 < 0, nfld < 1 or ifld0 + nfld > NANG * NFRE_RED ("bad field range"); NGRBRESS outside 1 .. 30;
 * NFRE no whole number of 16-byte pieces. */
int ecwam_hip_outspec_values(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *ff, int ifld0, int nfld, int flags,
                             const ecwam_hip_grib_opts *opts, void *values, void *ppmax, void *stream);

/* The sending half of OUTSPEC on many tasks: the mask, then blk[f - ifld0][ld] field-major with this task's points contiguous -- ZSENDBUF of
 * outwspec.F90:186-195.  Needs no map.  Refused: the field range as above; ld < kijl ("bad range"). */
int ecwam_hip_outspec_pack(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *ff, int ifld0, int nfld, int flags, void *blk,
                           int ld, void *stream);

/* MAKEGRID + WGRIBENCODE_VALUES on block vectors: element (f, ij) is src[f fstride + ij pstride] (in reals).  spectral = 1: steps 1 - 6, the
 * receiving half of OUTSPEC on many tasks with src the gathered ZRECVBUF (nfld <= NANG * NFRE_RED).  spectral = 0: steps 1 and 2 only, OUTINT's
 * path; with fstride = 1, pstride = NIPRMOUT the source is the BOUT[npts][NIPRMOUT] of ecwam_hip_outblock as it stands.  A list of columns is
 * given as one call per run of consecutive columns, with src advanced to the first column of the run and values to its first field.
 * opts: ZMISS is always read, the packing constants with spectral = 1.  ppmax as above (ignored with spectral = 0).
 * Refused: opts NULL; spectral outside 0, 1; nfld outside 1 .. 65535 (spectral = 1: 1 .. NANG * NFRE_RED); fstride or pstride < 1. */
int ecwam_hip_grib_values(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *src, long long fstride, long long pstride, int nfld, int spectral,
                          const ecwam_hip_grib_opts *opts, void *values, void *ppmax, void *stream);

#ifdef __cplusplus
}
#endif
#endif
