/*
 * Start spectra on the device: the four calls with which a model that does not begin from a restart file creates FL1 where it lives.
 * They are additions to ABI 6 of ecwam_hip.h (adding symbols is compatible: ECWAM_HIP_ABI_VERSION stays 6) and are declared in a header of
 * their own, so that the list of entry points of ecwam_hip.h, which the bindings and the tests count, is the one ABI 6 was published with.
 *
 * Common to the four: device pointers; fl1[npts][NANG][NFRE] and ff[npts][16] in the layouts of ecwam_hip_implsch; rows [kijs,kijl), 0-based;
 * the launch goes to `stream`; 0 on success, otherwise 1 with the reason in ecwam_hip_last_error.  The conventions are those of
 * ecwam_hip_setice.  Refused by all: a null context ("null context"), kijs < 0 or kijl < kijs ("bad range"), a null fl1 (or ff, where it is
 * read) with a range that is not empty, fl1 that is not 16-byte aligned (checked for an empty range too), an NFRE whose reals are no whole
 * number of 16-byte chunks per direction (NFRE odd in double, no multiple of 4 in single precision) and, by all but the noise start, NANG or NFRE above 64 or
 * a spectrum of more than 48 x 36 reals a point, rounded up to 64 chunks ("unsupported spectral size").  An empty range launches nothing.
 * A wavefront owns whole points and keeps a point's spectrum in registers between one load and one store (csrc/start.hip); the arithmetic of
 * a bin is the reference's, in its order and without contraction, and SEMEAN is summed in the reference's order.
 */
#ifndef ECWAM_HIP_START_H
#define ECWAM_HIP_START_H

#include "ecwam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MSTART (mstart.F90:104-136) for IOPTI 0, 1, 2, as preset calls it per chunk (preset.F90:630-638): PEAK's fetch law (peak.F90:88-102) and
 * SPECTRA (spectra.F90:95-120) = JONSWAP (jonswap.F90:70-91) times the cos**2 spread of SPR (spr.F90:69-81), its cut below 0.1E-08 included.
 * fl1 is written only.  Reads ff[ij][1] = WDWAVE and ff[ij][3] = WSWAVE.  The eight reals are MSTART's arguments, converted to the working
 * precision: the fetch [m], the maximum peak frequency [Hz], the mean direction [rad], and FM, ALFA, ZGAMMA, SA, SB.
 * Refused: iopti outside 0 .. 2 -- IOPTI = 3 (MSWELL) reads a gridded field from a file and is not served. */
int ecwam_hip_mstart(ecwam_hip_ctx *ctx, int kijs, int kijl, void *fl1, const void *ff, int iopti, double fetch, double frmax, double thetaq,
                     double fm, double alfa, double zgamma, double sa, double sb, void *stream);

/* UNSETICE (unsetice.F90:79-171), which INITMDL calls on every chunk at the start of a run (initmdl.F90:1024-1037): a fetch-law JONSWAP
 * spectrum at each point that holds nothing above EPSMIN and whose CICOVER <= CILIMIT (CITHRSH with LICERUN .AND. LMASKICE, else 0), the
 * noise floor (1 - 0.9 MIN(CICOVER, 0.99)) FLMIN MAX(0, COS(TH(K) - WDWAVE))**2 at every point, then SDEPTHLIM (sdepthlim.F90:64-78,
 * semean.F90:82-120) when the context has LBIWBK.  fl1 is read once and written once.
 * Reads ff[ij][1] = WDWAVE, [2] = CICOVER, [3] = WSWAVE, [14] = EMAXDPT (with LBIWBK), [15] = DEPTH.  delphi = DELPHI of YOWGRID [m].
 * flags: the two run-time switches of unsetice.F90:79 -- bit 0 LRESTARTED, bit 1 CLDOMAIN == 's'.  With either set the routine does
 * nothing: the call returns 0 without a launch (after the checks).
 * Refused: other bits in flags. */
int ecwam_hip_unsetice(ecwam_hip_ctx *ctx, int kijs, int kijl, void *fl1, const void *ff, double delphi, int flags, void *stream);

/* The noise start of GETSPEC (getspec.F90:174-188, LNSESTART): FL1 = EPSMIN on the rows.  Reads no column of ff (it has none). */
int ecwam_hip_getspec_noise(ecwam_hip_ctx *ctx, int kijs, int kijl, void *fl1, void *stream);

/* The end of GETSPEC's GRIB read (getspec.F90:648-659): frequencies nfre_red + 1 .. NFRE of every direction become
 * FL1(NFRE_RED) FR5(NFRE_RED) FRM5(M) (with nfre_red = NFRE there is nothing to fill), then SDEPTHLIM, unconditionally as there.
 * nfre_red is an argument: the spectra of the file need not end where the context's NFRE_RED does.  Reads ff[ij][14] = EMAXDPT.
 * Refused: nfre_red outside 1 .. NFRE. */
int ecwam_hip_getspec_tail(ecwam_hip_ctx *ctx, int kijs, int kijl, void *fl1, const void *ff, int nfre_red, void *stream);

#ifdef __cplusplus
}
#endif
#endif
