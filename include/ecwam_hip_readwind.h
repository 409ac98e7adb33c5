/*
 * The forcing of a stand-alone run on the device: what READWIND and CURRENT2WAM do with a decoded GRIB message at every wind and current time --
 * GRIB2WGRID's rearrangement or bilinear interpolation of the message's VALUES to the (NXS:NXE, NYS:NYE) grid (grib2wgrid.F90:783-1130), READWIND's
 * per-parameter fill of FIELDG (readwind.F90:341-494) and CURRENT2WAM's three statements per current component (current2wam.F90:247-279).  They fill
 * the planes fieldg[13][ncell_in] and the currents that ecwam_hip_getwnd and its neighbours read (ecwam_hip_forcing.h), so that such a run uploads
 * the VALUES exactly as the GRIB decoder returned them, not thirteen finished planes: the division of labour of ecwam_hip_gribin.h.  The coupled
 * run's counterpart is the setter and the calls of the intake header.  The three calls are additions to ABI 6 (ECWAM_HIP_ABI_VERSION stays 6) in a
 * header of their own: the lists of entry points the other headers were published with stay the ones they were.
 *
 * The conventions are those of ecwam_hip_forcing.h: device pointers unless called HOST; the launch goes to `stream`; 0 on success, otherwise 1 with
 * the reason in ecwam_hip_last_error.  The order of the refusals: the null context ("null context"), then the range ("bad range": a slot outside
 * 0 .. 3, rows as in ecwam_hip_getcurr), then what the call itself refuses, then the buffers (null where the call touches them, or not 16-byte
 * aligned).  No call on cells or rows allocates or waits.  The arithmetic is the reference's, in its order, in the working precision and without
 * contraction; SIN, COS and ATAN2 of a direction field are the device library's.  RAD = 4 ATAN(1) / 180 and DEG = 1 / RAD are formed on the host
 * in the working precision, as the reference forms them; CURRENT_MAX = 1.5 (yowcurr.F90:18) is a constant of the library.
 *
 * Not served: the ocean-model messages of GRIB 1 with local definition 4 (LLOCEAN: staggered grids, grib2wgrid.F90:266-321, 512-537, 986-1003),
 * unstructured input, and the un-scaling of parameter 251 (ecwam_hip_gribin.h serves spectra).  READWIND's swamp branch, the dates, LLNOTREAD across
 * calls, ICODE / IPARAMCI, the decoding and the broadcasts stay with the host.
 */
#ifndef ECWAM_HIP_READWIND_H
#define ECWAM_HIP_READWIND_H

#include "ecwam_hip_forcing.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECWAM_HIP_G2W_NSLOT 4
#define ECWAM_HIP_G2W_MAXFLD 16
/* the target of a field that is no plane of fieldg: FIELD as GRIB2WGRID returns it */
#define ECWAM_HIP_G2W_FIELD (-1)
/* the flags of a field: LLDIRFLD (grib2wgrid.F90:836-847) and LLNONWAVE (grib2wgrid.F90:388-394), evaluated by the host */
#define ECWAM_HIP_G2W_DIRFLD 1
#define ECWAM_HIP_G2W_NONWAVE 2

typedef struct ecwam_hip_g2w_field {
  int target; /* ECWAM_HIP_G2W_FIELD, or one of ECWAM_HIP_FG_UWND, _VWND, _AIRD, _WSTAR, _CICOVER, _CITHICK, _WSWAVE, _WDWAVE */
  int flags;  /* ECWAM_HIP_G2W_* */
} ecwam_hip_g2w_field;

/* The per-cell table of GRIB2WGRID's interpolation for one input grid, built once per grid (ecwam_amd/readwind.py builds it).  Four slots, because
 * winds and currents usually come on different grids.  HOST arrays over the ncell cells of the (NXS:NXE, NYS:NYE) grid, first index fastest:
 *   pos[ncell][4]  the 0-based positions in VALUES of WORK(II,KK), WORK(II1,KK), WORK(IIP,KK1), WORK(IIP1,KK1) as grib2wgrid.F90:964-1037 forms them,
 *                  with the scan direction (893-943) and the periodic columns WORK(0,..), WORK(RLONRGG+1,..) (947-955) resolved to real positions;
 *                  -1 = a padded row (KK <= 0 or KK > NR: 877-891), whose value is PMISS
 *   w[ncell][3]    double: DK1, DII1, DIIP1, each a value of the working precision widened; DK2 = 1 - DK1 etc. are formed on the device
 *   kind[ncell]    0 = outside its row (I > KLONRGG_LOC(JSN)); 1 = FIELD = PMISS (XLON or YLAT missing, or LLSKIP); 2 = interpolate
 * interpol = 0 is LLINTERPOL = F, the full copy of grib2wgrid.F90:793-802: only pos[c][0] is read and w may be NULL.
 * The library validates on the host and uploads: no kernel ever reads an unchecked index.  A call that fails a check leaves the table it found.
 * pos = NULL removes the slot's table.
 * Refused: ncell < 0; nvalues < 1; kind NULL; w NULL with interpol; a kind outside 0 .. 2; a position outside [-1, nvalues), or with interpol = 0
 * the position of a cell of kind 2 outside [0, nvalues); a weight that is not finite or, in single precision, that a float does not hold. */
int ecwam_hip_set_input_grid(ecwam_hip_ctx *ctx, int slot, int ncell, int nvalues, const int *pos, const double *w, const int *kind, int interpol);

/* GRIB2WGRID's rearrangement or interpolation (grib2wgrid.F90:783-1130) of nfld decoded messages of one input grid in one launch, the table being
 * read once per cell, each followed by READWIND's rule for the plane it targets.
 *   values[nfld][vstride]  the decoded vectors, reals, vstride >= the table's nvalues
 *   desc[nfld]             HOST, nfld <= ECWAM_HIP_G2W_MAXFLD
 *   out[nfld][ld]          row f receives FIELD of a field f whose target is ECWAM_HIP_G2W_FIELD: every cell is written, kinds 0 and 1 with pmiss
 *                          (FIELD(:,:) = PMISS, grib2wgrid.F90:197); rows of other fields are not touched; may be NULL without such a field
 *   fieldg[13][ncell_in]   a targeted plane receives FIELD by READWIND's rule (readwind.F90:341-494): UWND, VWND, CICOVER, CITHICK plain copies;
 *                          WSWAVE: pmiss -> 0; WDWAVE: pmiss -> 0, otherwise RAD (v - 180); AIRD: pmiss -> roair; WSTAR: pmiss -> wstar0.  Cells of
 *                          kind 0 keep their bits (READWIND's loops end at NLONRGG_LOC(JSN)), and so do the planes no field targets.
 * DIRFLD: SIN and COS of RAD v per corner (PMISS kept), both interpolated, DEG ATAN2.  With interpol = 0 it degenerates to the copy, as the
 * reference's does.  NONWAVE: where the nearest corner is missing too, the mean of the corners that are not; 0 where none is (1068-1093).
 * The test for a missing corner (1044-1047) is applied always.  This equals the reference wherever the reference is defined: with LLNEAREST = F no
 * value is missing and no row is padded, and LLNEAREST_LOC, once set, stays set for the rest of a serial loop and is undefined under OpenMP.
 * Refused: no table in the slot; vstride smaller than the table's nvalues; nfld outside 1 .. 16; desc NULL; an unknown target or flag; one plane
 * twice in one call (LLNOTREAD); ncell_in other than the table's ncell when a plane is targeted; ld smaller than the table's ncell when FIELD is. */
int ecwam_hip_grib2wgrid(ecwam_hip_ctx *ctx, int slot, const void *values, int vstride, int nfld, const ecwam_hip_g2w_field *desc, double roair,
                         double wstar0, double pmiss, void *out, int ld, void *fieldg, int ncell_in, void *stream);

/* CURRENT2WAM's statements (current2wam.F90:253-259, 270-276) for rows [kijs,kijl), through the inbound map of ecwam_hip_set_forcing_map: per
 * component U = FIELD(IX,JY); ABS(U) <= WLOWEST -> 0; U <= ZMISS -> 0; SIGN(MIN(ABS(U), CURRENT_MAX), U).  field_u, field_v: FIELD planes
 * [ncell_in] as ecwam_hip_grib2wgrid writes them with target ECWAM_HIP_G2W_FIELD.  A component whose field is NULL is left alone: its current is
 * neither read nor written and may be NULL as well.  changed: as ecwam_hip_getcurr writes it (KUPDATE) -- it becomes 1 if a component the call
 * writes differs from what the buffer held; the call never clears it.
 * Refused: no inbound map. */
int ecwam_hip_current2wam(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *field_u, const void *field_v, double wlowest, double zmiss, void *ucur,
                          void *vcur, int *changed, void *stream);

#ifdef __cplusplus
}
#endif
#endif
