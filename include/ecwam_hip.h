/*
 * ecwam_hip.h -- C ABI of libecwam_hip.so: the MI355X-native WAMINTGR hot path
 * (PROPAG_WAM/PROPAGS2 advection + NEWWIND + IMPLSCH source-term integration) of ecWAM.
 *
 * This is the drop-in boundary.  Every entry point names the reference
 * interface it replaces (paths relative to ecwam/src/ecwam).  All functions return 0 on success
 * and a non-zero status otherwise (the reference aborts through WAM_ABORT/ABORT1, yowabort.F90;
 * the Fortran wrapper fortran/wamintgr_hip.F90 turns a non-zero status into WAM_ABORT).
 * ecwam_hip_last_error() gives the message.  No torch / C++ types cross this boundary.
 *
 * Precision: `real_bytes` = 4 (JWRB single build) or 8 (double build), parkind_wave.F90:23-35.
 * Every `void*` array below holds reals of that size unless the name says int.
 *
 * DEVICE LAYOUT (private to the library; converted from the reference's chunked layout by
 * ecwam_hip_chunks_to_points / _points_to_chunks):
 *   spectra   FL[ij][K][M]           ij = local sea point (0-based), K = direction, M = frequency,
 *                                    M fastest; slot ij = nland (= "NSUP+1", propag_wam.F90:146)
 *                                    holds the zero land spectrum, halo points sit between the
 *                                    owned range and nland (mpdecomp.F90:89-100 convention)
 *   WVPRPT    [ij][5][NFRE]          WAVNUM, CGROUP, CINV, XK2CG, STOKFAC (FREQUENCY type, yowdrvtype_config.yml)
 *   FF        [ij][16]               AIRD WDWAVE CICOVER WSWAVE WSTAR USTRA VSTRA UFRIC TAUW TAUWDIR Z0M Z0B
 *                                    CHRNCK CITHICK (FORCING_FIELDS) + EMAXDPT DEPTH (ENVIRONMENT)
 *   INTF      [ij][16]               WSEMEAN WSFMEAN USTOKES VSTOKES STRNMS TAUXD TAUYD TAUOCXD TAUOCYD TAUOC
 *                                    TAUICX TAUICY PHIOCD PHIEPS PHIAW (INTGT_PARAM_FIELDS) + 1 pad
 *   WAM2NEMO  double[ij][13]         NEMOUSTOKES NEMOVSTOKES NEMOSTRN NPHIEPS NTAUOC NSWH NMWP NEMOTAUX NEMOTAUY NEMOTAUICX
 *                                    NEMOTAUICY NEMOWSWAVE NEMOPHIF (WAVE2OCEAN, always double = JWRO); only with LWNEMOCOU
 *   weights   W[ij][8][NANG*NFRE_RED] OPTIONAL (ecwam_hip_propags2_otf needs none): the 8 CTU weights PROPAGS2 reads when
 *                                    IREFRA=0 (propags2.F90:107-116):
 *                                    SUMWN, WLONN(JXO(K,1)), WLATN(JYO(K,1),1), WLATN(JYO(K,1),2),
 *                                    WCORN(1,1), WCORN(1,2), WKPMN(-1), WKPMN(+1)
 */
#ifndef ECWAM_HIP_H
#define ECWAM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ECWAM_HIP_MAXANG 48
/* bumped whenever ecwam_hip_params / ecwam_hip_tables or an entry point changes: 2 = refraction entry points, SDICE1 table and
 * ice break-up parameters added.  ecwam_hip_abi_version() returns the value the library was built with. */
#define ECWAM_HIP_ABI_VERSION 6
#define ECWAM_HIP_MAXFRE 48
#define ECWAM_HIP_MAXMC 56     /* MLSTHG = NFRE - ISM <= 48 + 8 */
#define ECWAM_HIP_MAXTAP 47    /* 2*NSDSNTH+1, NSDSNTH <= NANG/2-1 */
#define ECWAM_HIP_MAXGC 96     /* NWAV_GC (initgc.F90:67) = 82 */
#define ECWAM_HIP_IAB 200      /* yowtabl.F90:25 */
#define ECWAM_HIP_JTOT_TAUHF 19 /* yowcoup.F90:60 */
#define ECWAM_HIP_NFF 16
#define ECWAM_HIP_NINTF 16
#define ECWAM_HIP_NWPR 5

/* Scalars and flags the kernels read from the reference's modules (replaces `!$loki update_device`
 * of the module globals, wamintgr_loki_gpu.F90:95-97).  Reals are passed as double and rounded
 * to the working precision inside the library. */
typedef struct ecwam_hip_params {
  /* YOWPARAM / YOWSTAT / YOWWNDG */
  int nang, nfre, nfre_red, nfre_odd;
  int idelt;                /* IDELT: source time step [s] */
  double ximp;              /* XIMP */
  int iphys, isnonlin, irefra, icode;
  /* YOWCOUP / YOWSTAT / YOWICE flags (0/1) */
  int llgcbz0, llnormagam, llcapchnk, lbiwbk, licerun, lmaskice, lwamrsetci;
  int lciwa1, lciwa2, lciwa3, lciscal;
  int lwvflx_snl, lwflux, lwfluxout, lwnemocou, lwcou, lwcouast, lwnemocouwrs, lwnemotauoc;
  int lwnemocousend, lwnemocoustk, lwnemocoustrn; /* YOWCOUP: which WAVE2OCEAN members STOKESTRN fills (stokestrn.F90:75-88) */
  /* YOWPCONS */
  double g, gm1, pi, zpi, zpi4gm1, zpi4gm2, epsmin, rowater, rowaterm1, epsus, epsu10, acd, bcd, acdlin, bcdlin, cdmax;
  double tauocmin, tauocmax, phiepsmin, phiepsmax, wsemean_min, circ, r_earth;
  /* YOWFRED scalars */
  double fratio, wetail, frtail, wp1tail, fric, delth, flogsprdm1;
  /* YOWPHYS */
  double xkappa, xnlev, rnu, rnum, betamaxoxkappa2, bmaxokap, gamnconst, zalp, alpha, alphamin, alphamax, chnkmin_u, alphapmax;
  double tauwshelter, dthrn_a, dthrn_u, tailfactor, tailfactor_pm, ang_gc_a, ang_gc_b, ang_gc_c, rn1_rn;
  double swellf, swellf2, swellf3, swellf4, swellf5, swellf6, swellf7, swellf7m1, z0rat, z0tubmax, abmin, abmax;
  double sdsbr, ssdsc2, ssdsc3, ssdsc4, ssdsc5, ssdsc6, miche;
  int nsdsnth, ipsat;
  double egrcrv, afcrv, bfcrv;
  /* YOWCOUP / YOWTABL / YOWICE / YOWSHAL / YOWWIND */
  double x0tauhf, eps1, flmin, cithrsh, ciblock, cithrsh_tail, zalpwrs, bathymax, wspmin, wspmin_reset_tauw;
  double cdis, delta_sdis, cdisvis; int idamping; /* YOWPHYS / YOWSTAT: IPHYS=0 dissipation and swell damping switch */
  double cdicwa, zalpfacb, zalpfacx; /* YOWICE: SDICE2 drag coefficient, attenuation scale factors (sdice2.F90, implsch.F90:195) */
  /* YOWICE / YOWCOUP: ice break-up coupling (icebreak_modify_attenuation.F90) and the SDICE1 scattering table geometry
   * (cigetdeac.F90:64-71, yowice.F90:23) */
  int lwnemocouibr;
  double zibrw_thrsh;
  int nict, nich;
  double ticmin, dtic, dhic, hicmin;
  /* YOWINDN scalars */
  int mfrstlw, mlsthg, kfrh;
  double dal1, dal2;
  /* gravity-capillary model (YOWFRED *_GC) */
  int nwav_gc;
  double xlogkratiom1_gc, sqrtgosurft;
} ecwam_hip_params;

/* Host pointers to the reference's module tables, reals in the working precision, ints 32-bit.
 * Index values are passed exactly as the reference holds them (1-based where the reference is
 * 1-based); INDICESSAT is 1-based on this interface as in yowphys.F90:154. */
typedef struct ecwam_hip_tables {
  const void *fr, *dfim, *dfimofr, *dfimfr, *dfim_sim, *rhowg_dfim, *zpifr, *fr5, *cofrm4, *flmax; /* [NFRE]  yowfred.F90 */
  const void *th, *costh, *sinth;                                                                     /* [NANG] */
  const void *wtauhf;                                                                                 /* [19]   yowcoup.F90:61 */
  const void *swellft;                                                                                /* [200]  yowtabl.F90:56 */
  const int *ikp, *ikp1, *ikm, *ikm1;                                                                 /* [MLSTHG] values for MC=1.. (yowindn) */
  const void *af11;                                                                                   /* [MLSTHG] AF11(1:MLSTHG) */
  const int *k1w, *k2w, *k11w, *k21w;                                                                 /* [NANG][2] C order of K1W(K,KH) */
  const int *inlcoef;                                                                                 /* [MLSTHG][5]  INLCOEF(:,MC) */
  const void *rnlcoef;                                                                                /* [MLSTHG][25] RNLCOEF(:,MC) */
  const int *indicessat;                                                                              /* [NANG][2*NSDSNTH+1] */
  const void *satweights;                                                                             /* [NANG][2*NSDSNTH+1] */
  const int *kpm, *jxo, *jyo, *kcr;                                                                   /* [NANG][3],[2],[2],[4] (yowubuf) */
  const void *xk_gc, *xkm_gc, *omega_gc, *omxkm3_gc, *cm_gc, *c2osqrtvg_gc, *xkmsqrtvgoc2_gc, *om3gmkm_gc, *delkcc_gc_ns,
      *delkcc_omxkm3_gc;                                                                              /* [NWAV_GC] */
  const void *cideac;                                                                                 /* [NICH][NICT] = CIDEAC(IT,IH) (yowice); may be NULL unless LCIWA1 */
} ecwam_hip_tables;

typedef struct ecwam_hip_ctx ecwam_hip_ctx;

const char *ecwam_hip_last_error(void);
int ecwam_hip_abi_version(void);
/* diagnostics: runs the wavefront reduction / permutation primitives of the kernels on `device` against serial sums;
   0 = all agree.  No counterpart in the reference (the OpenACC build relies on the compiler's reductions). */
int ecwam_hip_selftest(int device);

/* Context: one per (device, configuration).  Replaces the device residency of the module globals. */
int ecwam_hip_create(const ecwam_hip_params *p, const ecwam_hip_tables *t, int real_bytes, int device, ecwam_hip_ctx **out);
int ecwam_hip_destroy(ecwam_hip_ctx *ctx);

/*
 * LSUBGRID: sub-grid obstructions of YOWUBUF (OBSLAT, OBSLON, OBSCOR; getbobstrct.F90 reads them, ctuw.F90:703-733 scales
 * the space weights with them).  obs: device real OBS[n][8][NFRE], planes OBSLAT(IJ,M,1:2), OBSLON(IJ,M,1:2), OBSCOR(IJ,M,1:4)
 * (values in [0,1], 1 = open); the library keeps the POINTER (the caller owns the memory) and every later ecwam_hip_ctuw /
 * ecwam_hip_propags2_otf / ecwam_hip_propags2_refra applies it.  obs = NULL switches it off (LSUBGRID = F, the default).
 * With IPROPAGS = 1 (ecwam_hipx_propags1.h) the last four planes are read as OBSRLAT(IJ,M,1:2) (planes 4-5) and OBSRLON(IJ,M,1:2) (planes 6-7), the
 * order of the file getbobstrct.F90 reads: that scheme has no corner points and the corner-transport scheme no rotated ones.
 */
int ecwam_hip_set_obstructions(ecwam_hip_ctx *ctx, const void *obs, int n);

/*
 * PROPAGS2 (propags2.F90:10, IREFRA=0 branch :99-121) on device pointers.
 *   f1, f3      FL[npts+1][NANG][NFRE]; only rows [kijs,kijl) of f3 are written; frequencies
 *               [nd3s-1, nd3e) are advected (1-based inclusive as in the reference);
 *               if copy_rest != 0 the remaining frequencies of those rows are copied f1 -> f3
 *               (the reference leaves them in FL1, propag_wam.F90:379-386)
 *   klon[ij][2] klat[ij][2][2] kcor[ij][4][2]  0-based local indices, land = nland (yowubuf KLON/KLAT/KCOR)
 *   w           W[ij][8][NANG*NFRE_RED]
 */
int ecwam_hip_propags2(ecwam_hip_ctx *ctx, const void *f1, void *f3, const int *klon, const int *klat, const int *kcor,
                       const void *w, int kijs, int kijl, int nd3s, int nd3e, int copy_rest, void *stream);

/*
 * CTUWINI + CTUW (ctuwini.F90:58-164, ctuw.F90:146-275 + :407-484 + :536-608) for IREFRA=0, ICASE=1,
 * LSUBGRID=F: builds W for rows [0,n) and frequencies [mstart,mend] (1-based) with time step delpro.
 *   kxlt[ij] 0-based latitude row; zdello/cosph/sinph [ngy] (yowmap ZDELLO, yowgrid COSPH/SINPH)
 *   wlat[ij][2], wcor[ij][4] are MODIFIED near land exactly as ctuwini.F90:66-97 does
 *   cgroup_ext [npts+1][NFRE] group velocity incl. halo and land rows (proenvhalo.F90 BUFFER_EXT)
 *   cosphm1_ext[npts+1]
 *   cflfail  int[n] set to 1 where a CFL/weight-range check of ctuw.F90:288-357,541-685 fails
 *   w        may be NULL: checks and WLAT/WCOR snapping only (see ecwam_hip_propags2_otf)
 */
int ecwam_hip_ctuw(ecwam_hip_ctx *ctx, int n, int nland, int ngy, double delpro, int mstart, int mend, const int *kxlt,
                   const void *zdello, double xdella, const void *cosph, const void *sinph, const int *klon, const int *klat,
                   const int *kcor, void *wlat, void *wcor, const void *cgroup_ext, const void *cosphm1_ext, void *w,
                   int *cflfail, void *stream);

/*
 * PROPAGS2 with the CTU weights rebuilt inside the stencil ("on the fly") instead of read from W: the device-side
 * replacement of PROPAGS2 + the WLATN/WLONN/WCORN/WKPMN/SUMWN module arrays of yowubuf.F90:175-193 when the weights are
 * static (IREFRA=0: ctuwupdt.F90:204-238 builds them once).  Same arguments as ecwam_hip_ctuw (the geometry, with
 * wlat/wcor as LEFT BY ecwam_hip_ctuw, i.e. after the CTUWINI land snapping) plus those of ecwam_hip_propags2; the
 * result is bit-identical to ecwam_hip_ctuw followed by ecwam_hip_propags2 with the same delpro.  ecwam_hip_ctuw with
 * w == NULL performs the CTUWINI snapping and the CFL / weight-range checks without storing the weights.
 *   order  optional int[>=kijl]: the rows order[kijs..kijl) are processed, in that sequence (chosen by the host for cache
 *          locality, e.g. longitude strips); entries < 0 are padding and skipped, so the list may be longer than n; NULL =
 *          natural order.  Results do not depend on it.
 *   copy_rest  bit 0: the frequencies outside nd3s..nd3e are copied from f1; bit 2 (value 4, needs order): the list describes
 *          2-D tiles of 16 entries, entry 4 g + w = g-th point of a longitude segment of the w-th of four adjacent latitude
 *          rows; the four wavefronts of a workgroup then work on latitude neighbours at the same time (40 % less fabric
 *          read traffic at O320, same time: DESIGN.md section 3).
 */
int ecwam_hip_propags2_otf(ecwam_hip_ctx *ctx, const void *f1, void *f3, int n, int ngy, double delpro, const int *kxlt,
                           const void *zdello, double xdella, const void *cosph, const void *sinph, const int *klon,
                           const int *klat, const int *kcor, const void *wlat, const void *wcor, const void *cgroup_ext,
                           const void *cosphm1_ext, const int *order, int kijs, int kijl, int nd3s, int nd3e, int copy_rest,
                           void *stream);

/*
 * The fast / slow wave split of PROPAG_WAM (IFRELFMAX > 0, propag_wam.F90:247-313) in one pass: frequencies 1..ifrelfmax advance
 * with delpro_lf, the others with delpro (the reference calls PROPAGS2 once per range with separately built weights).
 * ifrelfmax = 0: identical to ecwam_hip_propags2_otf.  Bit-identical to the two separate calls.
 * in_nfre: 0 (f1 has the FL layout) or the width of a COMPACT input buffer f1[npts+1][NANG][in_nfre] that holds only the first
 * in_nfre frequencies of every direction (the fast waves between sub-steps: with M fastest in memory a frequency sub-range of
 * the full rows touches every cache line; the compact rows are 4.5x smaller at IFRELFMAX = 5).  f3 always has the FL layout.
 * gout (may be NULL): compact buffer gout[npts+1][NANG][gout_nfre] that ALSO receives the first gout_nfre advected frequencies of
 * every direction (what the next fast-wave sub-step starts from; gout_nfre a multiple of 16 bytes).
 */
int ecwam_hip_propags2_otf_split(ecwam_hip_ctx *ctx, const void *f1, void *f3, int n, int ngy, double delpro, double delpro_lf,
                                 int ifrelfmax, int in_nfre, void *gout, int gout_nfre, const int *kxlt, const void *zdello, double xdella, const void *cosph,
                                 const void *sinph, const int *klon, const int *klat, const int *kcor, const void *wlat,
                                 const void *wcor, const void *cgroup_ext, const void *cosphm1_ext, const int *order, int kijs,
                                 int kijl, int nd3s, int nd3e, int copy_rest, void *stream);
/*
 * The same with the two further row formats of the fast-wave sub-steps (round 3): the sub-steps 1 .. NSTEP_LF-1 of the fast waves run
 * compact -> compact BEFORE the full pass (the fast waves do not depend on the slow ones: the same arithmetic in another order, hence
 * the same bits as propag_wam.F90:247-313), and the full pass takes their last state as the input of the last sub-step and writes
 * complete rows -- no pass writes a frequency sub-range into full rows (which touches every line of them).
 *   gin / gin_nfre (may be NULL / 0; needs full input rows, in_nfre = 0): the first gin_nfre frequencies of every direction are read
 *     from the compact buffer gin[npts+1][NANG][gin_nfre] (own point and neighbours alike) instead of f1.
 *   out_nfre: 0 (f3 has the FL layout) or the width of a compact OUTPUT buffer f3[npts+1][NANG][out_nfre] (then gout must be NULL; with a
 *     compact input of the same width copy_rest carries the frequencies beyond nd3e over, so that whole 16-byte vectors stay valid).
 */
int ecwam_hip_propags2_otf_fast(ecwam_hip_ctx *ctx, const void *f1, void *f3, int n, int ngy, double delpro, double delpro_lf,
                                int ifrelfmax, int in_nfre, const void *gin, int gin_nfre, int out_nfre, void *gout, int gout_nfre,
                                const int *kxlt, const void *zdello, double xdella, const void *cosph, const void *sinph,
                                const int *klon, const int *klat, const int *kcor, const void *wlat, const void *wcor,
                                const void *cgroup_ext, const void *cosphm1_ext, const int *order, int kijs, int kijl, int nd3s,
                                int nd3e, int copy_rest, void *stream);
/* g (may be NULL: off) = compact rows g[npts+1][NANG][g_nfre] that every later ecwam_hip_implsch / ecwam_hip_nosource call ALSO leaves the
 * first g_nfre frequencies of the spectra it wrote in: the state the next advection step's fast-wave sub-steps start from, written from
 * IMPLSCH's tile instead of extracted from the FL1 rows by a pass of its own (ecwam_hip_copy_freq_range).  The library keeps the pointer. */
int ecwam_hip_set_fastwave_copy(ecwam_hip_ctx *ctx, void *g, int g_nfre);
/* dst[ij][K][m_first-1 .. m_last-1] = src[...] for rows [0,n): FL1_EXT(:,:,1:IFRELFMAX) = FL3_EXT(...) between the fast-wave
 * sub-steps (propag_wam.F90:287-291).  dst_nfre: 0 (dst has the FL layout) or the width of a compact buffer dst[..][NANG][dst_nfre] */
int ecwam_hip_copy_freq_range(ecwam_hip_ctx *ctx, const void *src, void *dst, int n, int m_first, int m_last, int dst_nfre,
                              void *stream);

/*
 * Refraction, IREFRA = 1 (depth), 2 (currents), 3 (depth + currents) -- params.irefra selects it at ecwam_hip_create.
 *
 * ecwam_hip_propdot: GRADI + the per-point part of PROPDOT (gradi.F90:113-232, propdot.F90:108-196), called whenever the
 * reference sets LLUPDTTD (new currents, propag_wam.F90:175-213).  Replaces the module arrays THDD/THDC/SDOT of yowubuf:
 *   depth_ext, u_ext, v_ext [npts+1]  DEPTH / UCUR / VCUR incl. halo rows and the land slot as proenvhalo.F90:99-106
 *                                     fills it (BATHYMAX, 0, 0)
 *   wlat[ij][2]                       as read from the grid tables (before or after CTUWINI: GRADI only uses entries
 *                                     CTUWINI never changes)
 *   refr  out, real[n][2*NANG+5]:     THD(K) (THDD for IREFRA=1, THDC for 2/3), S0(K) (current-gradient factor of SDOT,
 *                                     propdot.F90:172), U, V, OMDD (propdot.F90:126), CURMASK of frequency range 0 and 1 (=1)
 *
 * ecwam_hip_ctuw_refra: CTUWINI + CTUWDRV (ctuwupdt.F90:204-238, ctuwdrv.F90:93-118) without storing weights: snaps
 * wlat/wcor, runs the CFL / range checks of every weight for frequencies [mstart,mend] with time step delpro, and when
 * llcflcuroff != 0 and a point fails with currents, repeats them with the current refraction and frequency shift of that
 * point switched off (its CURMASK in refr becomes 0, as ctuw.F90:117-131).  cflfail[n]: points still failing (the caller
 * aborts, ctuwdrv.F90:124-146).  range = 0 for the only (or the fast-wave) frequency range, 1 for the slow-wave range of a
 * split call (ctuwupdt.F90:220-256 runs CTUWDRV once per range, each with its own CURMASK); range 0 resets cflfail, range 1
 * adds its failures to those of range 0.
 *
 * ecwam_hip_propags2_refra: PROPAGS2 (propags2.F90:99-192) with all weights rebuilt inside the stencil from the geometry,
 * cgroup_ext, the point's own omosnh2kd/wavnum rows and refr.  IREFRA=1: the eight-term stencil with depth refraction in
 * WKPMN; IREFRA=2/3: all 2+4+8 space neighbours, both direction and both frequency neighbours, in the reference's
 * summation order.  Arguments as ecwam_hip_propags2_otf; range selects the CURMASK of ecwam_hip_ctuw_refra.
 */
int ecwam_hip_propdot(ecwam_hip_ctx *ctx, int n, int nland, const int *kxlt, const void *zdello, double xdella,
                      const void *cosph, const int *klon, const int *klat, const void *wlat, const void *cosphm1_ext,
                      const void *depth_ext, const void *u_ext, const void *v_ext, void *refr, void *stream);
int ecwam_hip_ctuw_refra(ecwam_hip_ctx *ctx, int n, int nland, int ngy, double delpro, int mstart, int mend, const int *kxlt,
                         const void *zdello, double xdella, const void *cosph, const void *sinph, const int *klon,
                         const int *klat, const int *kcor, void *wlat, void *wcor, const void *cgroup_ext,
                         const void *omosnh2kd_ext, const void *wavnum_ext, const void *cosphm1_ext, void *refr,
                         int llcflcuroff, int range, int *cflfail, void *stream);
int ecwam_hip_propags2_refra(ecwam_hip_ctx *ctx, const void *f1, void *f3, int n, int ngy, double delpro, const int *kxlt,
                             const void *zdello, double xdella, const void *cosph, const void *sinph, const int *klon,
                             const int *klat, const int *kcor, const void *wlat, const void *wcor, const void *cgroup_ext,
                             const void *omosnh2kd_ext, const void *wavnum_ext, const void *cosphm1_ext, const void *refr,
                             int range, int kijs, int kijl, int nd3s, int nd3e, int copy_rest, void *stream);

/*
 * IMPLSCH (implsch.F90:10-23) for local points [kijs,kijl) on device pointers (layouts above).
 *   fl1 inout, wvprpt in, ff inout, intf inout, mij out (1-based), xllws out
 *   intf[ij][15] (the spare slot of the 16-wide row) carries the INPUT ENVIRONMENT%IBRMEM when LWNEMOCOUIBR
 *   wam2nemo: double[npts][13] inout, the WAVE2OCEAN members (always JWRO = double, yowdrvtype_config.yml:44-55) in the order
 *             NEMOUSTOKES NEMOVSTOKES NEMOSTRN NPHIEPS NTAUOC NSWH NMWP NEMOTAUX NEMOTAUY NEMOTAUICX NEMOTAUICY NEMOWSWAVE
 *             NEMOPHIF; updated as wnfluxes.F90:304-328 (LNUPD = T) and stokestrn.F90:75-88 do; required when LWNEMOCOU,
 *             ignored (may be NULL) otherwise
 *   dbg: must be NULL (ABI 4: an intermediate dump of the retired one-point-per-wavefront kernel)
 */
int ecwam_hip_implsch(ecwam_hip_ctx *ctx, int kijs, int kijl, void *fl1, const void *wvprpt, void *ff, void *intf, int *mij,
                      void *xllws, double *wam2nemo, void *dbg, void *stream);
/*
 * IMPLSCH runs ONE kernel generation since ABI 5: k_implsch4 (csrc/implsch_v4.h: several sea points per wavefront; common builds for the
 * configurations the reference registers as tests, RARE builds for every other switch of SURVEY.md 8a), 48 / 36 / 24 / 12 directions x 36
 * frequencies, single and double precision.  ecwam_hip_create refuses what no build covers.  (ABI 4 carried a second, slower generation for
 * the remainder and ecwam_hip_set_implsch_generation to choose; that kernel is now test infrastructure, tests/csrc/implsch_v2.h.)
 * The generation the last ecwam_hip_implsch call of this context launched (4; 0 before the first call). */
int ecwam_hip_implsch_generation_used(ecwam_hip_ctx *ctx);
/* The device copy of the module tables the kernels read (private layout, csrc/dev.h DevTab): for diagnostics and for a second
 * implementation of a kernel that is to run on exactly the tables the library runs on (the tests' k_implsch2).  Owned by the context. */
const void *ecwam_hip_device_tables(ecwam_hip_ctx *ctx);
/*
 * k_implsch4 is bracketed by two one-point-per-lane kernels (first TAUT_Z0 before, second STRESSO and WNFLUXES after it) that exchange
 * 36 scalars per sea point through a context-owned device buffer indexed by the point number.  ecwam_hip_implsch grows that buffer when
 * kijl exceeds what it holds -- a device allocation and a device-wide wait inside an otherwise stream-ordered call.  A host that wants
 * none of that in its time loop (or captures the step into a hipGraph) sizes it once: npts = the largest kijl it will pass.  Calls on
 * several streams may share the buffer as long as their [kijs,kijl) do not overlap.  The same call sizes the tables of the one-kernel step
 * (ecwam_hip_propags2_implsch: 12 reals per point) where the context has such a build.
 */
int ecwam_hip_implsch_reserve(ecwam_hip_ctx *ctx, int npts);

/*
 * WDFLUXES (wdfluxes.F90:156-306) for rows [kijs,kijl): what OUTSTEP0 (outstep0.F90:108-169) runs before the first time step and after a
 * restart, so that the output of step 0 has MIJ, XLLWS, the flux fields and the Stokes drift.  The source terms are evaluated once on fl1 as
 * it stands -- FKMEAN, ONE SINFLX call (NGST = 2, LLSNEG; UFRIC, Z0M, Z0B, CHRNCK as ff holds them: no TAUT_Z0), and with
 * LCFLX = LWFLUX .OR. LWFLUXOUT (not IMPLSCH's, which also ORs LWNEMOCOU) SDISSIP, SNONLIN, WNFLUXES (LNUPD = F), FEMEANWS and STOKESTRN --
 * and nothing is advanced.  Layouts as for ecwam_hip_implsch.
 *   fl1, wvprpt, ff in (ff's TAUW / TAUWDIR are not touched: STRESSO's are locals of WDFLUXES); mij, xllws out
 *   intf: with LCFLX, members 2, 3 (USTOKES, VSTOKES) and 5 .. 14 (TAUXD .. PHIAW), with LWFLUX also 0, 1 (WSEMEAN, WSFMEAN) are written;
 *         without LCFLX nothing is.  intf[ij][15] is the INPUT IBRMEM as for ecwam_hip_implsch.
 *   wam2nemo: required when LWNEMOCOU (may be NULL otherwise); with LCFLX only its columns 0, 1 (NEMOUSTOKES, NEMOVSTOKES) change, as
 *             stokestrn.F90:75-88 sets them; without LCFLX nothing does
 * Served: the configurations the common and the alternate builds of k_implsch4 run (flag sets A and B; IPHYS 0 or ISNONLIN 1 on flag set A).
 * Double precision at 24 directions is not served (that build gave wrong numbers on the device and is not shipped).
 * The others (LCIWA2, LWNEMOCOUWRS, LWNEMOCOUSTRN, ISNONLIN 2, ICODE 1 / 2, LWVFLX_SNL = F, the mixed alternates) are refused:
 * ecwam_hip_wdfluxes_supported returns 1 / 0 and, with 0, leaves the refusal's text in ecwam_hip_last_error.
 * The call uses the context's rows of ecwam_hip_implsch_reserve, indexed by the point number, as ecwam_hip_implsch does.
 */
int ecwam_hip_wdfluxes(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *wvprpt, const void *ff, void *intf, int *mij,
                       void *xllws, double *wam2nemo, void *stream);
int ecwam_hip_wdfluxes_supported(ecwam_hip_ctx *ctx);
/* SETICE (setice.F90:67-86) on rows [kijs,kijl): where CICOVER = ff[ij][2] > CITHRSH the spectrum becomes
 * MAX(EPSMIN, 1 - CICOVER) FLMIN MAX(0, COS(TH(K) - WDWAVE))**2; elsewhere it is left as it is.  OUTSTEP0 calls it when LICERUN .AND. LMASKICE.
 * Refused: fl1 that is not 16-byte aligned (checked for an empty range too), and an NFRE whose reals are no whole number of 16-byte chunks
 * per direction (NFRE odd in double, no multiple of 4 in single precision): the kernel stores 16 bytes at a time. */
int ecwam_hip_setice(ecwam_hip_ctx *ctx, int kijs, int kijl, void *fl1, const void *ff, void *stream);

/*
 * The two calls of WAMODEL between the time step and the output (wamodel.F90:333-343), for nested (limited-area) runs.  All pointers are
 * device pointers; both calls work on every context ecwam_hip_create accepts.
 *
 * ecwam_hip_bouinpt: BOUINPT's loop over the fine grid's boundary points (bouinpt.F90:385-424): the coarse model's spectra, interpolated
 * between two coarse boundary points with INTSPEC / ROTSPEC / STRSPEC (Hasselmann's spectrum interpolation), replace the rows of fl1.
 *   nijb, ijb[nijb]     the boundary points: 0-based rows of fl1.  Only those with kijs <= ijb < kijl are written (the NSTART / NEND test of
 *                       bouinpt.F90:138-145: a band of a decomposed run passes its own rows); every other row of fl1 is untouched.
 *                       The entries must be distinct: two entries for one row would race, and the library cannot check a device table.
 *   ibcl, ibcr [nijb]   IBFL / IBFR: 0 = the land point (spectrum and mean parameters zero; nothing is read for it) or 1 .. nboinp
 *   bfw[nijb]           BFW, the weight of the right point (DEL12 = 1): <= 0 copies the left spectrum
 *   f1[nboinp][NFRE][NANG], par1[nboinp][3]
 *                       the records of the boundary file as it holds them: the spectrum with the direction fastest, and EMEAN, THQ
 *                       [radians], FMEAN.  Entry i - 1 is index i.
 *   par_out[nijb][3]    optional (NULL): EMEAN, THQ, FMEAN of the result -- INTSPEC's interpolated values where it ran, the left point's
 *                       where the spectrum was copied.  Rows of points outside [kijs,kijl) are left alone.
 * The reference's behaviour is kept, quirks included: the literal 1.1 for the frequency ratio, every frequency up to NFRE written, bins the
 * loops of STRSPEC do not reach zero, no EPSMIN floor.  Mean frequencies that are zero, negative or not finite give unspecified values at
 * that point and no access outside the buffers.
 * Refused: negative counts, kijs > kijl, a null required pointer with nijb > 0, fl1 not 16-byte aligned or an NFRE that does not fill
 * 16-byte chunks (the rule of ecwam_hip_setice), spectra whose two staged copies do not fit in 64 KiB of LDS.  nijb = 0 launches nothing.
 *
 * ecwam_hip_outbc: OUTBC for the coarse model's output boundary points (outbc.F90:78-91): par[nbc][3] = EMEAN (FEMEAN), THQ (STHQ, radians),
 * FMEAN (FEMEAN) of rows ijarc[nbc] (0-based) of fl1 -- EMEAN the bits of column 3 of ecwam_hip_outbs -- and flpts[nbc][NFRE][NANG] = their
 * spectra in the order of the file's record.  par may be NULL: a plain gather of point spectra.  The spectral sizes of ecwam_hip_outbs.
 * Refused: a negative count, a null ijarc / fl1 / flpts with nbc > 0.  nbc = 0 launches nothing.
 */
int ecwam_hip_bouinpt(ecwam_hip_ctx *ctx, int kijs, int kijl, int nijb, const int *ijb, const int *ibcl, const int *ibcr, const void *bfw,
                      int nboinp, const void *f1, const void *par1, void *fl1, void *par_out, void *stream);
int ecwam_hip_outbc(ecwam_hip_ctx *ctx, int nbc, const int *ijarc, const void *fl1, void *flpts, void *par, void *stream);

/*
 * One WAMINTGR step with a 1:1 ratio of advection and source-term steps as ONE pass over the spectra (wamintgr.F90:94-146: PROPAG_WAM then
 * IMPLSCH; propag_wam.F90:124-147,247-251,373-400; propags2.F90:99-121): the kernel that integrates the source terms of rows [kijs,kijl)
 * advects them itself while it loads them -- PROPAGS2 (IREFRA = 0, one time step for every frequency, CTU weights rebuilt on the fly from the
 * arguments of ecwam_hip_propags2_otf) from the rows of f1 (owned + halo + land rows: read only) straight into the kernel's working tile --
 * and stores the new spectrum to the rows of f3.  The advected spectrum never goes to memory.  Result: bit for bit what
 * ecwam_hip_propags2_otf(f1 -> f3, copy_rest = 1) followed by ecwam_hip_implsch(f3) leaves in f3, FF, INTF, MIJ, XLLWS, WAM2NEMO.
 * The caller runs NEWWIND (ecwam_hip_newwind) BEFORE this call (it touches the forcing only) and swaps f1 / f3 after it, as after PROPAGS2.
 * Rows whose stencil reads halo rows are passed in a second call behind ecwam_hip_halo_finish, exactly as with ecwam_hip_propags2_otf.
 * Fast waves (the native O1280 cycle, propag_wam.F90:247-313): ifrelfmax > 0 with gin = the compact rows [rows][NANG][gin_nfre] that hold the
 * fast waves after their sub-steps 1 .. NSTEP_LF - 1 (ecwam_hip_propags2_otf_fast, compact -> compact): the call is then the LAST sub-step
 * of the fast waves (time step delpro_lf, read from gin) together with the slow waves' step (delpro, read from f1) -- what
 * ecwam_hip_propags2_otf_fast(f1 -> f3, gin) does -- and the source terms; with ecwam_hip_set_fastwave_copy the new fast waves also go to
 * the compact rows the next advection step starts from.  Else ifrelfmax = 0, gin = NULL.
 * Covered: what ecwam_hip_propags2_implsch_supported reports (48 / 36 / 24 / 12 directions x 36 frequencies in single, 36 x 36 in double precision, the common builds of
 * IMPLSCH with IPHYS = 1 / ISNONLIN = 0, no refraction; with or without the obstructions of ecwam_hip_set_obstructions); everything else runs
 * the two calls.
 * flags: 0 only.
 */
/* 0: no one-kernel build covers the context; else a mask: bit 0 the plain step, bit 1 also with fast waves (gin), bit 2 also with obstructions */
int ecwam_hip_propags2_implsch_supported(ecwam_hip_ctx *ctx);
int ecwam_hip_propags2_implsch(ecwam_hip_ctx *ctx, const void *f1, void *f3, int n, int ngy, double delpro, const int *kxlt, const void *zdello,
                               double xdella, const void *cosph, const void *sinph, const int *klon, const int *klat, const int *kcor,
                               const void *wlat, const void *wcor, const void *cgroup_ext, const void *cosphm1_ext, int kijs, int kijl,
                               int nd3s, int nd3e, const void *wvprpt, void *ff, void *intf, int *mij, void *xllws, double *wam2nemo,
                               double delpro_lf, int ifrelfmax, const void *gin, int gin_nfre, int flags, void *stream);

/*
 * Integrated output parameters without a spectrum copy-back (the device-side part of OUTBS: outblock.F90:204,223-243,
 * LSECONDORDER=F) for rows [kijs,kijl):  out[npts][5] = significant wave height 4*SQRT(EM) (FEMEAN), mean direction in
 * degrees / meteorological convention (STHQ), mean period 1/FM or zmiss, EM, peak period pp1d (DOMINANT_PERIOD) or zmiss.
 * ecwam_hip_outwnorm: the OUTWNORM statistics of one such field: result[4] (HOST doubles) = average, minimum, maximum over the
 * n values field[i*stride] that differ from zmiss, and their count (outwnorm.F90).  Synchronises the stream.
 * These are the parameters of fl1 as passed (FL2ND = FL1); those of the absolute-frame output spectrum (IREFRA = 2 / 3, ice noise
 * reshaping): ecwam_hip_outbs_absolute.
 */
int ecwam_hip_outbs(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, double zmiss, void *out, void *stream);
int ecwam_hip_outwnorm(ecwam_hip_ctx *ctx, const void *field, int stride, int n, double zmiss, double *result, void *stream);

/*
 * Wind sea / swell and the mean-period / spread parameters of OUTBLOCK (outblock.F90:214-382 with FL2ND = FL1: IREFRA 0/1,
 * LSECONDORDER = F, no LICERUN noise reshaping, no OUTSETWMASK) for rows [kijs,kijl): SEPWISW (sepwisw.F90) with LLPARTITION = F --
 * the wind-sea mask from xllws (the XLLWS of ecwam_hip_implsch), CINV = wvprpt[ij][2][:], UFRIC = ff[ij][7] and WDWAVE = ff[ij][1],
 * then FEMEAN, STHQ, MWP1, MWP2 and WDIRSPREAD (LLPEAKF = T) of the swell and of the wind-sea part -- and MWP1, MWP2, WDIRSPREAD
 * (LLPEAKF = F) of the total spectrum.  Swell trains (SEP3TR, parameters 42-50) are not computed; MIJ and WSWAVE are not read.  When any
 * of 42-50 is requested the reference runs SEPWISW with LLPARTITION = T: use ecwam_hip_outbs_partition instead, whose columns 0-14 are
 * these columns as that configuration computes them.
 * out[npts][15] (columns; OUTBLOCK parameter numbers in brackets):
 *    0 mp1   MWP1 of the total spectrum [20]        1 mp2   MWP2 [21]        2 wdw   WDIRSPREAD [22]
 *    3 shww  wind-sea height 4*SQRT(MAX(ESEA,0)) [11]                        4 shts  swell height 4*SQRT(MAX(ESWELL,0)) [12]
 *    5 mdww  wind-sea direction, degrees, MOD(DEG*THWISEA+180,360) [13]      6 mdts  swell direction [14]
 *    7 mpww  wind-sea mean period 1/FSEA or zmiss [15]                       8 mpts  swell mean period 1/FSWELL or zmiss [16]
 *    9 P1SEA [23]  10 P1SWELL [24]  11 P2SEA [25]  12 P2SWELL [26]  13 SPRDSEA [27]  14 SPRDSWELL [28]
 * flags: bit 0 -- CLDOMAIN = 's' (a small domain): the first mask only, without the R test, the second mask and the walk over
 * frequencies (sepwisw.F90:177).  OUTWNORM statistics of a column: ecwam_hip_outwnorm(out + column, stride = 15).
 * Columns 0-2 from the absolute-frame output spectrum (IREFRA = 2 / 3, ice noise reshaping): ecwam_hip_outbs_absolute.
 */
int ecwam_hip_outbs_sepwisw(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *xllws, const void *wvprpt, const void *ff,
                            int flags, double zmiss, void *out, void *stream);

/*
 * Swell-train partitioning of OUTBLOCK (parameters 42-50; outblock.F90:214-382, 436-449 with FL2ND = FL1) for rows [kijs,kijl): SEPWISW
 * with LLPARTITION = T -- SEP3TR, FNDPRT and PARMEAN after the wind-sea / swell split of ecwam_hip_outbs_sepwisw.  Inputs as there, plus
 * mij (the 1-based MIJ of ecwam_hip_implsch; SEP3TR looks for peaks below it and drops partitions of mean period under INT(1/FR(MIJ))).
 * WSWAVE is not read.  out[npts][24] indexed by the absolute row ij: columns 0-14 those of ecwam_hip_outbs_sepwisw, as the reference
 * computes them with LLPARTITION = T (FNDPRT's factor MAX(W1,1) on the swell mask is 1, so they equal the LLPARTITION = F values), then
 * for the swell trains ITR = 1..3 (OUTBLOCK parameter numbers in brackets):
 *   15 + 3(ITR-1) swh  4*SQRT(MAX(EMTRAIN,0)) [42 + 3(ITR-1)]     16 + 3(ITR-1) mwd  MOD(DEG*THTRAIN+180,360) [43 + ...]
 *   17 + 3(ITR-1) mwp  PMTRAIN [44 + ...], 0 where there is no train (no zmiss, as outblock.F90:436-449)
 * A point has at most NPMAX = 20 peaks (in order of discovery, M-major) and at most 25 sweeps per peak.  flags: 0 only; bit 0 (CLDOMAIN =
 * 's') is refused -- the reference hands SEP3TR an FSEA it has not computed in that branch -- and so is every other bit.  The spectral
 * sizes of ecwam_hip_outbs_sepwisw.  OUTWNORM statistics of a column: ecwam_hip_outwnorm(out + column, stride = 24).
 * Columns 0-2 from the absolute-frame output spectrum (IREFRA = 2 / 3, ice noise reshaping): ecwam_hip_outbs_absolute.
 */
int ecwam_hip_outbs_partition(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *xllws, const int *mij, const void *wvprpt,
                              const void *ff, int flags, double zmiss, void *out, void *stream);

/*
 * Extreme-wave parameters of OUTBLOCK for rows [kijs,kijl): KURTOSIS (kurtosis.F90 with PEAK_ANG, AKI, TRANSF_BFI, STAT_NL, TRANSF_R,
 * H_MAX; outblock.F90:208-211, called at every output time) and W_MAXH (w_maxh.F90 with W_MODE_ST; outblock.F90:559-578).  Inputs:
 * fl1 (FL1), WAVNUM = wvprpt[ij][0][:], DEPTH = ff[ij][15] (ENVIRONMENT%DEPTH).  out[npts][13] indexed by the absolute row ij
 * (columns; OUTBLOCK parameter numbers with NTRAIN = 3, NTEWH = 6 in brackets):
 *    0 c4     kurtosis C4 [29]                 1 bfi    BF2, square of the Benjamin-Feir index [30]     2 qp    Goda peakedness QP [31]
 *    3 hmax   envelope maximum height HMAX [33]   4 tmax   period of the maximum TMAX [34]            5 c3    skewness C3 [57]
 *    6 eta_m  wave-induced sea-level correction ETA_M [70]   7 r   spectral width index R [71]     8 xnslc number of events XNSLC [72]
 *    9 cmax_f  time-domain maximum crest CMAX_F [78]         10 hmax_n  time-domain maximum height HMAX_N [79]
 *   11 cmax_st space-time maximum crest CMAX_ST [80]         12 hmax_st space-time maximum height HMAX_ST [81]
 * flags: bit 0 -- KURTOSIS only: W_MAXH is skipped and columns 9-12 are not written (the reference calls W_MAXH only when one of
 * 78-81 is requested).  Other bits: error.  AKI's open iteration is bounded at 100 Newton steps.  Not served: the FL2ND transforms
 * (INTPOL, CAL_SECOND_ORDER_SPEC; KURTOSIS and W_MAXH read FL1), OUTSETWMASK, SIG_TH / EPS / XNU and PHIST (not OUTBLOCK parameters).
 * OUTWNORM statistics of a column: ecwam_hip_outwnorm(out + column, stride = 13).
 * The INTPOL transform and the ice noise reshaping of FL2ND, for the parameters that read FL2ND: ecwam_hip_outbs_absolute.
 */
int ecwam_hip_outbs_extremes(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *wvprpt, const void *ff, int flags,
                             void *out, void *stream);

/*
 * The output spectrum FL2ND of OUTBLOCK and the parameters that read it (outblock.F90:159-263, 350-359; LSECONDORDER = F) for rows
 * [kijs,kijl).  FL2ND is built per point on the chip, as params.irefra / licerun / lmaskice of ecwam_hip_create select:
 *   IREFRA = 2 / 3: INTPOL(FL1 -> FL2ND, WAVNUM, UCUR, VCUR, IRA = 1) (intpol.F90:98-271), the spectrum in the absolute frame: every bin
 *     moves to FREQ + K.U/ZPI, the f**-5 tail up to FR(NFRE) + ZPI/G FR(NFRE)**2 CURRENT_MAX is folded back in, energy of negative
 *     shifted frequency goes to the opposite direction, a point with no bin above EPSMIN gives EPSMIN everywhere; IREFRA = 0 / 1: FL2ND = FL1;
 *   LICERUN and not LMASKICE: then the noise level under sea ice is reshaped (outblock.F90:175-194) with CICOVER = ff[ij][2] and
 *     WSWAVE = ff[ij][3].
 * Inputs: fl1; WAVNUM = wvprpt[ij][0][:] and ucur / vcur, device reals [>= kijl] (UCUR, VCUR of the point; all three may be NULL when
 * IREFRA is 0 or 1); ff (may be NULL unless the ice reshaping is on).  CURRENT_MAX = 1.5 m/s (yowcurr.F90:18) is a constant of the library:
 * the reference clips the components of the current to [-CURRENT_MAX, CURRENT_MAX] when it reads them (wamcur.F90:82-84) and sizes the tail
 * extension with it; components outside that range are the caller's error and are not clipped here.
 * out[npts][8] indexed by the absolute row ij (columns; OUTBLOCK parameter numbers in brackets):
 *    0 swh  4*SQRT(EM) of FEMEAN [1]    1 mwd  mean direction of STHQ, degrees [2]    2 mwp  mean period 1/FM or zmiss [3]    3 EM
 *    4 pp1d peak period of DOMINANT_PERIOD or zmiss [6]    5 mp1  MWP1 [20]    6 mp2  MWP2 [21]    7 wdw  WDIRSPREAD, LLPEAKF = F [22]
 * Columns 0-4 are bit for bit what ecwam_hip_outbs gives on FL2ND, columns 5-7 what ecwam_hip_outbs_sepwisw gives in its columns 0-2.
 * fl2nd (may be NULL): device FL2ND[npts][NANG][NFRE] that receives the rows [kijs,kijl) of the output spectrum (for SE10MEAN / SEBTMEAN,
 * spectral output or the host); with NULL nothing but out is written.  fl2nd must not overlap fl1 (fl2nd == fl1 is refused).  The scatter of INTPOL uses no atomics: results do not depend on
 * scheduling.  flags: 0 only.  The spectral sizes of ecwam_hip_outbs_sepwisw.  CAL_SECOND_ORDER_SPEC (LSECONDORDER = T) is served by
 * ecwam_hip_outbs_second_order.  Not served: OUTSETWMASK, IRA = -1.  OUTWNORM statistics of a column: ecwam_hip_outwnorm(out + column,
 * stride = 8).
 */
int ecwam_hip_outbs_absolute(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *wvprpt, const void *ucur, const void *vcur,
                             const void *ff, int flags, double zmiss, void *out, void *fl2nd, void *stream);

/*
 * The tables of the second-order output spectrum (LSECONDORDER = T; YOWTABL as SECONDHH_GEN and TABLES_2ND fill it, secondhh_gen.F90:73-121,
 * tables_2nd.F90:107-186), for ecwam_hip_outbs_second_order.  Only the thinning SECONDHH_GEN always selects is served: NFREH = NFRE/2,
 * NANGH = NANG/2, MR = MA = 2 (odd NANG or NFRE: refused).  All pointers are HOST arrays in the reference's storage order, copied before
 * the call returns:
 *   ndepth, deptha, depthd   NDEPTH, DEPTHA, DEPTHD of YOWSHAL (mpuserin.F90:616-618: 74, 1, 1.1)
 *   nmax                     NMAX of YOWTABL (22 at NFRE = 36)
 *   im_p, im_m               int IM_P(NFREH,NFREH), IM_M(NFREH,NFREH): values 1 .. NMAX, [M][M1] in C order
 *   ta, tb, tc_ql, tt_4m, tt_4p   reals of the working precision, TA(NDEPTH,NANGH,NFREH,NFREH): [M][M1][L][JD] in C order
 * OMEGA, OMEGA_EXT and the interpolation weights follow from FR and FRATIO of ecwam_hip_create.  ta == NULL removes the tables.  The device
 * layout is the library's own (one contiguous slice per depth index).  Not thread safe against calls in flight on the context.
 */
int ecwam_hip_set_second_order(ecwam_hip_ctx *ctx, int ndepth, double deptha, double depthd, int nmax, const int *im_p, const int *im_m,
                               const void *ta, const void *tb, const void *tc_ql, const void *tt_4m, const void *tt_4p);

/*
 * The output spectrum FL2ND of OUTBLOCK with LSECONDORDER = T and the parameters that read it (outblock.F90:168-263, 350-359) for rows
 * [kijs,kijl): the pipeline of ecwam_hip_outbs_absolute with CAL_SECOND_ORDER_SPEC(FL2ND, WAVNUM, DEPTH, SIG)
 * (cal_second_order_spec.F90:91-193, secspom.F90:127-288) between INTPOL and the ice noise reshaping:
 *   FKMEAN of the spectrum after INTPOL (EMEAN, AKMEAN); the depth index JD = NINT(LOG(MAX(1/AKMEAN, DEPTH)/DEPTHA)/LOG(DEPTHD)) + 1 within
 *   1 .. NDEPTH; thinning to NANGH x NFREH and the f**-5 extension to NMAX; SECSPOM's double sum with the tables of
 *   ecwam_hip_set_second_order, every bin in the reference's order of additions (no atomics: results do not depend on scheduling); the energy
 *   conserving interpolation back to NANG x NFRE, switched off where EMEAN > 0.6**2/16 DEPTH**2, with F = MAX(MIN(1E-6, F), F + SIG DELF).
 * Inputs as ecwam_hip_outbs_absolute, except: wvprpt is always needed (FKMEAN reads WAVNUM); depth: device reals [>= kijl], DEPTH of the
 * point; sig: +1 adds the correction (what OUTBLOCK does), -1 removes it.  out[npts][8] and fl2nd as ecwam_hip_outbs_absolute; the stages the
 * two calls share give the same bits, so with all-zero coefficient tables the results are equal bit for bit.
 * Refused with a reason: no tables set, NANG not 48 / 36 / 24 / 12, fl2nd == fl1.  The call keeps a work space of
 * NANGH (NMAX + NFREH) reals + 1 int per point on the context, grown on demand (a synchronising allocation on the first call and when
 * the range grows).  The work space is one per context: calls of this function on one context must be ordered on one stream (or separated by
 * a synchronisation); two in flight on different streams would overwrite each other's intermediate spectra.  OUTWNORM statistics of a column: ecwam_hip_outwnorm(out + column, stride = 8).
 */
int ecwam_hip_outbs_second_order(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *wvprpt, const void *depth,
                                 const void *ucur, const void *vcur, const void *ff, double sig, double zmiss, void *out, void *fl2nd,
                                 void *stream);

/*
 * The constants of ecwam_hip_outbs_integrals, worked out once in the working precision and kept on the device.  Host arrays are copied
 * before the call returns.
 *   xkmss_cutoff   XKMSS_CUTOFF of YOWFRED, the wavenumber up to which parameter 9 integrates the slope; <= 0 selects XK_GC(NWAV_GC) as
 *                  userin.F90:1214 does.  The second cut-off, (ZPI FR(NFRE))**2 / G of parameter 86 (outblock.F90:602), needs no argument.
 *   nband, tb, tt  0 .. 8 period bands as SEBTMEAN's arguments: tb[i] the shorter and tt[i] the longer period [s] of band i (host doubles,
 *                  rounded to the working precision).  The reference's seven: (10, 1/FR(1)) = SE10MEAN, then (10,12) (12,14) (14,17) (17,21)
 *                  (21,25) (25,30) (outblock.F90:460, 515-519).  Per band the library precomputes MCUTB, MCUTT, FRLOC, the interpolation
 *                  weights WL / WR at the two cut frequencies, the DF of the trapezoid, the factor of the linear front tail and ZW of the
 *                  f**-5 extension, in sebtmean.F90:81-102,172-184's order of operations.
 *   delkcc_gc      reals [NWAV_GC] of the working precision: DELKCC_GC of YOWFRED (initgc.F90), the one gravity-capillary table
 *                  ecwam_hip_tables carries only as its product with OMXKM3_GC; MEANSQS_GC sums DELKCC_GC(I) XKM_GC(I).
 * NE of MEANSQS_GC and NFRE_MSS of MEANSQS (meansqs_gc.F90:59, meansqs.F90:100) are evaluated in double precision from the working-precision
 * tables: with the model's own cut-off the argument of INT lies within rounding of NFRE - 1, where the working-precision value would depend
 * on the last bit of the logarithm routine at hand.
 * Refused with a reason: nband outside 0 .. 8, tb > tt, a band wholly below FR(1) (SEBTMEAN would read FR(0)), a cut-off below FR(1).
 * Synchronises the device; not thread safe against calls in flight on the context.
 */
int ecwam_hip_set_outbs_integrals(ecwam_hip_ctx *ctx, double xkmss_cutoff, int nband, const double *tb, const double *tt, const void *delkcc_gc);

/*
 * OUTBLOCK's remaining spectral integrals for rows [kijs,kijl) in ONE pass over the spectrum (outblock.F90:266-287, 451-462, 500-523, 597-604):
 * OUTBETA (CD=), MEANSQS (HALPHAP, MEANSQS_GC with OMEGAGC, MEANSQS_LF, the tail) at both cut-offs, CIMSSTRN (AKI_ICE), WEFLUX, CTCOR of FL1,
 * and SEBTMEAN / SE10MEAN of the output spectrum FL2ND.  Inputs: fl1; fl2nd -- NULL or equal to fl1: FL2ND = FL1 and the row is read once;
 * else the spectrum stored by ecwam_hip_outbs_absolute or ecwam_hip_outbs_second_order (read once more, by the bands only); WAVNUM =
 * wvprpt[ij][0][:], CGROUP = wvprpt[ij][1][:]; ff: WDWAVE [1], WSWAVE [3], UFRIC [7], TAUW [8], CHRNCK [12], CITHICK [13], DEPTH [15].
 * out[npts][8 + nband] indexed by the absolute row ij (columns; OUTBLOCK parameter numbers with NTRAIN = 3 in brackets):
 *    0 cd     MIN(CD of OUTBETA, 0.01) [7]                 1 tauw_n  TAUW / MAX(UFRIC**2, EPSUS) [8]
 *    2 mss    mean square slope up to XKMSS_CUTOFF [9]     3 strn    mean square strain in the ice, CIMSSTRN [51]; with LWNEMOCOUSTRN the
 *                                                                    reference outputs STRNMS of INTF instead: the host's choice
 *    4 wefmag wave energy flux magnitude [62]              5 wefdir  its direction, MOD(DEG*WEFDIR+180,360) [63]
 *    6 ctcor  crest-trough correlation or zmiss [85]       7 mss_m   mean square slope up to (ZPI FR(NFRE))**2 / G [86]
 *    8 + i    4*SQRT(MAX(E,0)) of band i [52, 64-69 with the seven bands above]
 * flags: the column groups to compute, so that a host pays only for what IPFGTBL asks -- 1 slopes (2, 7), 2 strain (3), 4 flux (4, 5),
 * 8 CTCOR (6), 16 bands (8 ...), 32 point-wise (0, 1).  Columns of unselected groups are not written; a group's columns are the same bits
 * whatever else is selected.  Other bits: error.  With only the bands selected fl1 or fl2nd alone suffices (wvprpt and ff may be NULL); with
 * only the point-wise group ff alone.
 * Every sum over K and over M runs in the reference's order of additions (FEMEAN of the wind half plane inside HALPHAP is the exception: it is
 * the wavefront reduction the other output kernels use); no atomics: results do not depend on scheduling.
 * Refused with a reason: bad range, ecwam_hip_set_outbs_integrals not called, the bands selected with nband = 0, NANG not 48 / 36 / 24 / 12,
 * unknown flags.  The spectral sizes of ecwam_hip_outbs_sepwisw.  Not served: OUTSETWMASK (ecwam_hip_outsetwmask below).  OUTWNORM statistics
 * of a column: ecwam_hip_outwnorm(out + column, stride = 8 + nband).
 */
int ecwam_hip_outbs_integrals(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *fl2nd, const void *wvprpt, const void *ff,
                              int flags, double zmiss, void *out, void *stream);

/*
 * OUTSETWMASK (outsetwmask.F90:57-75; outblock.F90:610) on rows [kijs,kijl) of any of the library's output buffers out[npts][ncol], in place.
 *   colflags  HOST int[ncol]: bit 0 -- the sea-ice mask applies to the column (IPRMINFO(IR,6) = 1), bit 1 -- the sea mask (IPRMINFO(IR,7) = 1);
 *             copied before the call returns; ncol <= 64.
 *   sea-ice mask: out = zmiss where CICOVER = ff[ij][2] > cithrsh (CITHRSH).  Applied only when the context has LICERUN; LLSOURCE, the
 *             reference's other condition, is not a parameter of the library (it integrates the source terms): a host that runs the
 *             LLSOURCE = F branch clears bit 0.
 *   sea mask: out = out*IODP + (1-IODP)*zmiss, exactly as written there.  iodp: device int[>= kijl]; may be NULL when no column has bit 1.
 * The sea-ice mask is applied first, as in the reference.  ff may be NULL when no column has bit 0 or the context has no LICERUN.
 * OUTWNORM statistics of a masked column: ecwam_hip_outwnorm(out + column, stride = ncol) skips the zmiss values.
 */
int ecwam_hip_outsetwmask(ecwam_hip_ctx *ctx, int kijs, int kijl, void *out, int ncol, const int *colflags, const void *ff, const int *iodp,
                          double cithrsh, double zmiss, void *stream);

/*
 * OUTBLOCK itself (outblock.F90:159-610; the routine the reference's GPU build runs on the device, outbs_loki_gpu.F90:104-125): one call that
 * works out what a request needs, runs only that, and fills BOUT(KIJL, NIPRMOUT) -- every value in its column ITOBOUT(IR), masked by OUTSETWMASK.
 *
 * ecwam_hip_set_outblock: the request.  All pointers are HOST int[jppflag], copied before the call returns; entry IR-1 belongs to parameter IR of
 * mpcrtbl.F90:92-469 (with NTRAIN = 3, NTEWH = 6: 42 + 3 (ITR-1) the swell trains, 51 the strain, 52 SE10MEAN, 62 / 63 the energy flux, 63 + IH the
 * bands, 70-72, 78-81, 82 IBRMEMOUT, 83 / 84 TAUICX / TAUICY, 85 CTCOR, 86 the mean square slope up to the model's cut-off, 87-89 unused extra fields).
 *   ipfgtbl   IPFGTBL: /= 0 -- the parameter is requested (-1, a parameter that is only normed, counts as in the reference)
 *   itobout   ITOBOUT: the 1-based column of the parameter in BOUT, or 0
 *   icemask, seamask   IPRMINFO(IR,6), IPRMINFO(IR,7): 1 -- the sea-ice mask / the sea mask applies
 *   niprmout  NIPRMOUT, the number of columns of BOUT (<= 128); a column no requested parameter is mapped to is written as 0
 *   flags     bit 0 LSECONDORDER; bit 1 CLDOMAIN = 's'; bit 2 LLSOURCE = F: no sea-ice mask (outsetwmask.F90:60)
 *   jppflag   must be 89 = 75 + 3 NTRAIN + 5: the library is written for NTRAIN = 3; NTEWH = 6 comes with the seven bands of
 *             ecwam_hip_set_outbs_integrals, which must be set before this call when a parameter of ecwam_hip_outbs_integrals is requested
 * The call derives a plan and keeps it on the context: which of the output calls above run and with which group flags (so that only what a
 * requested column reads is computed), whether FL2ND is stored, and one descriptor per column of BOUT (source buffer, source column, operation, mask
 * bits) on the device.  The output spectrum is built once, as params.irefra / licerun / lmaskice and bit 0 select: with FL2ND = FL1 parameters 1, 2,
 * 3, 6 come from ecwam_hip_outbs and 20-22 from ecwam_hip_outbs_sepwisw / _partition; else they come from ecwam_hip_outbs_absolute or
 * ecwam_hip_outbs_second_order, and the spectrum is stored only when a band (52, 64-69) is requested.  11-16 and 23-28 come from
 * ecwam_hip_outbs_partition when one of 42-50 is requested (LLPARTITION, mpcrtbl.F90:535-543), else from ecwam_hip_outbs_sepwisw;
 * ecwam_hip_outbs_extremes runs KURTOSIS only unless one of 78-81 is requested; with LWNEMOCOUSTRN parameter 51 is STRNMS of INTF and the strain
 * group does not run (outblock.F90:451-457).
 * Refused with a reason: jppflag /= 89; a requested parameter whose column is outside 1 .. niprmout; two parameters in one column; one of 42-50 with
 * bit 1 (ecwam_hip_outbs_partition refuses that branch); a band requested while the bands of the context are not (10, 1/FR(1)), (10,12), (12,14),
 * (14,17), (17,21), (21,25), (25,30) s; a parameter of ecwam_hip_outbs_integrals before ecwam_hip_set_outbs_integrals; bit 0 without second-order
 * tables; a spectral size or NANG a needed call has no build for; unknown flags.  Synchronises the device; not thread safe against calls in flight.
 *
 * ecwam_hip_outblock_plan: *calls = bit 0 ecwam_hip_outbs, 1 _sepwisw, 2 _partition, 3 _extremes, 4 _absolute, 5 _second_order, 6 _integrals;
 * bits 8-13 the group flags ecwam_hip_outbs_integrals runs with; bit 14 W_MAXH runs in ecwam_hip_outbs_extremes.  *stores_fl2nd: FL2ND goes to the
 * work space.  Either pointer may be NULL.
 *
 * ecwam_hip_outblock: rows [kijs,kijl) of bout[npts][niprmout] (device reals, indexed by the absolute row, row-major like every output buffer here),
 * each written exactly once.  Inputs as the calls above take them (fl1, xllws, mij, wvprpt, ff, ucur / vcur) plus
 *   intf     INTF[ij][16]: 35 / 36 USTOKES / VSTOKES, 39-41 PHIEPS, PHIAW, TAUOC, 51 STRNMS (LWNEMOCOUSTRN), 73-76 TAUXD TAUYD TAUOCXD TAUOCYD,
 *            77 MAX(-PHIOCD, 0), 83 / 84 TAUICX / TAUICY
 *   iodp     device int[>= kijl], for the sea mask
 *   ibrmem   device reals [>= kijl]: IBRMEM; 82 is IBRMEMOUT: ibrmem, or zmiss where not CICOVER > 0 (ibrmemout.F90:74-82)
 *   altim    device reals [3][kijl]: ALTWH, CALTWH, RALTCOR (17-19); plane p of point ij at altim[p * kijl + ij]
 *   nemo     device DOUBLE [4][kijl] (JWRO): NEMOCICOVER, NEMOCITHICK, NEMOUCUR, NEMOVCUR (58-61), rounded to the working precision on write;
 *            planes as altim
 * and from ff: 4 UFRIC, 5 MOD(DEG*WDWAVE+180,360), 10 WSWAVE, 32 DEPTH (ff[ij][15] everywhere; staged contiguously for ecwam_hip_outbs_second_order),
 * 53 AIRD, 54 WSTAR, 55 CICOVER, 56 CITHICK.  Requested parameters no statement of OUTBLOCK fills (87-89) are 0.  Last comes OUTSETWMASK with each
 * column's own bits, the sea-ice mask first, both as ecwam_hip_outsetwmask applies them (cithrsh, zmiss as there).
 * A pointer may be NULL when no requested parameter reads it; a NULL pointer the plan reads is refused by name before anything is launched, as is
 * a call before ecwam_hip_set_outblock.
 * Work space: the packed rows of the calls (8 + 24 + 13 + 8 + nband reals per point), DEPTH for the second-order call and FL2ND [kijl][NANG][NFRE]
 * when the bands read it live in a work space on the context, sized by kijl and grown on demand (a synchronising allocation on the first call and
 * when kijl grows).  It is one per context: calls of this function on one context must be ordered on one stream (or separated by a
 * synchronisation) -- the rule of ecwam_hip_outbs_second_order, whose work space this call uses as well.
 */
int ecwam_hip_set_outblock(ecwam_hip_ctx *ctx, int jppflag, const int *ipfgtbl, const int *itobout, const int *icemask, const int *seamask,
                           int niprmout, int flags);
int ecwam_hip_outblock_plan(ecwam_hip_ctx *ctx, int *calls, int *stores_fl2nd);
int ecwam_hip_outblock(ecwam_hip_ctx *ctx, int kijs, int kijl, const void *fl1, const void *xllws, const int *mij, const void *wvprpt, const void *ff,
                       const void *intf, const void *ucur, const void *vcur, const int *iodp, const void *ibrmem, const void *altim,
                       const double *nemo, double cithrsh, double zmiss, void *bout, void *stream);

/* NEWWIND forcing hand-over (newwind.F90:126-161): FF <- FF_NEXT members + TAUW cap.  ecwam_hip_newwind takes ICODE_WND = ICODE
 * of the parameters; a coupled host (LWCOU) passes ICODE_CPL through ecwam_hip_newwind_icode (newwind.F90:120-124). */
int ecwam_hip_newwind(ecwam_hip_ctx *ctx, int n, void *ff, const void *ff_next, void *stream);
int ecwam_hip_newwind_icode(ecwam_hip_ctx *ctx, int n, void *ff, const void *ff_next, int icode_wnd, void *stream);
/* The LLSOURCE = F branch of WAMINTGR (wamintgr.F90:152-160) on device rows [kijs, kijl): FL1 = MAX(FL1, EPSMIN), MIJ = NFRE,
 * XLLWS = 0.  fl1 == NULL: the branch of a call before the next source-term date (wamintgr.F90:178-186): MIJ = NFRE, XLLWS = 0 only. */
int ecwam_hip_nosource(ecwam_hip_ctx *ctx, int kijs, int kijl, void *fl1, int *mij, void *xllws, void *stream);

/*
 * Layout conversion between the reference's chunked host-shaped arrays and the device layout
 * (replaces the chunk<->block copies of propag_wam.F90:124-137,373-400).
 *   chunked spectra: FL1(NPROMA,NANG,NFRE,NCHNK) Fortran order; point ij = ichnk*nproma + iprm (mchunk.F90:62-68)
 *   pad lanes (iprm >= KIJL4CHNK) replicate lane 1 on the way back (propag_wam.F90:388-398)
 */
int ecwam_hip_chunks_to_points(ecwam_hip_ctx *ctx, const void *chunked, void *points, int nproma, int nchnk, int npts,
                               int n2, int n3, void *stream);
int ecwam_hip_points_to_chunks(ecwam_hip_ctx *ctx, const void *points, void *chunked, int nproma, int nchnk, int npts,
                               int n2, int n3, void *stream);

/*
 * One member of a FIELD_API-backed host type <-> its slot in the library's packed per-point rows: what FIELD_API's per-member
 * GET_DEVICE_DATA_* / SYNC_DEVICE_* (host -> device) and GET_HOST_DATA_* / SYNC_HOST_* (device -> host) copies are in the reference's
 * GPU build (drvtype_mod.fypp:116-480; the member selectors of wamodel.F90:207-226,376-385,435-470,614-642 and
 * wamintgr_loki_gpu.F90:100-157,197-200), for a device layout that is not the host's.
 *   chunked: DEVICE image of the host member M(NPROMA[,NM],NCHNK) (Fortran order, as copied with ecwam_hip_memcpy_h2d / _d2h),
 *     elements of elem_bytes = 4 or 8 bytes (JWRB reals, JWRO doubles, JWIM integers move alike);
 *   rows: device [npts][row_stride] elements of the same size; the member's NM values of point ij at rows[ij*row_stride + row_off .. + NM):
 *     FF rows (row_stride 16: the 14 FORCING_FIELDS members + ENVIRONMENT%EMAXDPT, %DEPTH), INTF rows (16: 15 INTGT_PARAM_FIELDS members +
 *     ENVIRONMENT%IBRMEM), WAVE2OCEAN rows (13 doubles), WVPRPT rows (5*NFRE: member j at row_off j*NFRE, NM = NFRE), MIJ (1 int32);
 *   scatter: chunked -> rows for the npts points; gather: rows -> chunked, pad lanes of the last chunk replicating its lane 1.
 */
int ecwam_hip_member_scatter(ecwam_hip_ctx *ctx, const void *chunked, void *rows, int nproma, int nchnk, int npts, int nm,
                             long long row_stride, long long row_off, int elem_bytes, void *stream);
int ecwam_hip_member_gather(ecwam_hip_ctx *ctx, const void *rows, void *chunked, int nproma, int nchnk, int npts, int nm,
                            long long row_stride, long long row_off, int elem_bytes, void *stream);

/* Halo pack/unpack for the advection exchange (mpexchng.F90:124-138, 217-231):
 *   pack:   buf[i][:] = fl[idx[i]][:]   for i < n   (row = NANG*NFRE reals)
 *   unpack: fl[dst0+i][:] = buf[i][:]  */
int ecwam_hip_pack_rows(ecwam_hip_ctx *ctx, const void *fl, const int *idx, int n, void *buf, void *stream);
int ecwam_hip_unpack_rows(ecwam_hip_ctx *ctx, const void *buf, int n, void *fl, int dst0, void *stream);

/*
 * MPEXCHNG inside the library (mpexchng.F90:141-231: pack the rows the neighbouring ranks need, point-to-point exchange,
 * receive into the halo rows): what a Fortran host needs to run the sea-point block decomposition (mpdecomp.F90:58-100) on
 * several GPUs, one process per GPU.
 *   ecwam_hip_halo_setup: rank / nranks of this process and, per neighbouring rank i < npeers: peer[i], send_count[i] owned local
 *     rows to send (send_idx: their 0-based local indices, the npeers lists concatenated), and the contiguous halo segment
 *     [recv_dst0[i], recv_dst0[i] + recv_count[i]) of the local row space their rows land in (the reference's NTOPE / IJTOPE and
 *     NFROMPE / NIJSTART).
 *   transport 1, RCCL over xGMI (librccl is loaded with dlopen on first use): ecwam_hip_comm_unique_id on rank 0 gives the 128-byte
 *     id the host broadcasts (MPI_Bcast); ecwam_hip_comm_init(ctx, id) on every rank (collective).  ecwam_hip_halo_start packs on
 *     `stream` and posts the grouped sends / receives on the library's own stream (the receives write fl's halo rows; rowlen = reals
 *     per row: NANG*NFRE, or NANG*LFP for the compact fast-wave rows); work enqueued on `stream` afterwards overlaps with the
 *     exchange and must not touch fl's halo rows until ecwam_hip_halo_finish(ctx, stream) has made `stream` wait for it.
 *   transport 2, host staged (an MPI library without device-pointer support; several ranks on one GPU in tests):
 *     ecwam_hip_halo_pack_host fills host_send (n_send rows, peer order, ecwam_hip_halo_counts gives the sizes) and synchronises; the
 *     host exchanges the segments; ecwam_hip_halo_unpack_host copies host_recv (n_recv rows, peer order) into the halo rows.
 */
int ecwam_hip_halo_setup(ecwam_hip_ctx *ctx, int rank, int nranks, int npeers, const int *peer, const int *send_count,
                         const int *send_idx, const int *recv_dst0, const int *recv_count);
int ecwam_hip_halo_counts(ecwam_hip_ctx *ctx, int *n_send, int *n_recv);
int ecwam_hip_comm_unique_id(void *id128);
int ecwam_hip_comm_init(ecwam_hip_ctx *ctx, const void *id128);
int ecwam_hip_comm_count(ecwam_hip_ctx *ctx, int *nranks);   /* ranks of the RCCL communicator (ncclCommCount); 0 without one */
int ecwam_hip_halo_start(ecwam_hip_ctx *ctx, void *fl, int rowlen, void *stream);
int ecwam_hip_halo_finish(ecwam_hip_ctx *ctx, void *stream);
int ecwam_hip_halo_pack_host(ecwam_hip_ctx *ctx, const void *fl, int rowlen, void *host_send, void *stream);
int ecwam_hip_halo_unpack_host(ecwam_hip_ctx *ctx, void *fl, int rowlen, const void *host_recv, void *stream);

/*
 * PROENVHALO (proenvhalo.F90:63-107) on the device: the extended (own + halo + land) rows of the fields the weights and the refraction
 * terms are built from, assembled without a round trip through the host when the currents (or the depth) change on a decomposed grid.
 *   buffer_ext: device real [nrows][3*NFRE + 3] -- per local row WAVNUM(1:NFRE), CGROUP(1:NFRE), OMOSNH2KD(1:NFRE), DEPTH, UCUR, VCUR (the
 *     reference's BUFFER_EXT without DELLAM1 / COSPHM1, which the geometry arrays of the set-up hold).
 *   ecwam_hip_proenvhalo_pack fills the n owned rows from the device-resident WVPRPT rows (members 0, 1), OMOSNH2KD[n][NFRE] and the
 *     per-point DEPTH / UCUR / VCUR;  the halo rows [n, nrows) are then exchanged like the spectra: ecwam_hip_halo_start(ctx, buffer_ext,
 *     3*NFRE + 3, stream) + ecwam_hip_halo_finish (or the host-staged pair) = MPEXCHNG(BUFFER_EXT, 3*NFRE_RED+5, 1, 1);
 *   ecwam_hip_proenvhalo_unpack spreads the nrows rows over the extended arrays [nrows + 1][..] the advection entry points read and fills
 *     the land slot (row nrows) from land[3*NFRE + 3] = (WVPRPT_LAND%WAVNUM, %CGROUP, %OMOSNH2KD, BATHYMAX, 0, 0).
 */
int ecwam_hip_proenvhalo_pack(ecwam_hip_ctx *ctx, int n, const void *wvprpt, const void *omosnh2kd, const void *depth,
                              const void *ucur, const void *vcur, void *buffer_ext, void *stream);
int ecwam_hip_proenvhalo_unpack(ecwam_hip_ctx *ctx, int nrows, const void *buffer_ext, const void *land, void *wavnum_ext,
                                void *cgroup_ext, void *omosnh2kd_ext, void *depth_ext, void *u_ext, void *v_ext, void *stream);

/* Device-memory helpers for hosts without their own HIP binding (the Fortran layer): the counterpart of FIELD_API's
 * device allocation / GET_DEVICE_DATA / SYNC_HOST copies (drvtype_mod.fypp:116-480).  `stream` may be NULL. */
int ecwam_hip_malloc(ecwam_hip_ctx *ctx, unsigned long long bytes, void **dptr);
int ecwam_hip_free(ecwam_hip_ctx *ctx, void *dptr);
int ecwam_hip_memcpy_h2d(ecwam_hip_ctx *ctx, void *dst_dev, const void *src_host, unsigned long long bytes, void *stream);
int ecwam_hip_memcpy_d2h(ecwam_hip_ctx *ctx, void *dst_host, const void *src_dev, unsigned long long bytes, void *stream);
int ecwam_hip_memset(ecwam_hip_ctx *ctx, void *dst_dev, int value, unsigned long long bytes, void *stream);
int ecwam_hip_sync(ecwam_hip_ctx *ctx, void *stream);
/* Asynchronous queues (FIELD_API's QUEUE= of SYNC_HOST_* / SYNC_DEVICE_*, WAIT_FOR_ASYNC_QUEUE: field_async_module; the OpenACC
 * build's async(1..6), wamintgr_loki_gpu.F90:100-200): a queue is a non-blocking HIP stream, usable as the `stream` of every entry
 * point.  ecwam_hip_queue_wait_for makes work enqueued on `waiter` from now on start after everything enqueued on `waited` so far
 * (either may be NULL = the default stream); ecwam_hip_sync(ctx, queue) is WAIT_FOR_ASYNC_QUEUE. */
int ecwam_hip_queue_create(ecwam_hip_ctx *ctx, void **queue);
int ecwam_hip_queue_destroy(ecwam_hip_ctx *ctx, void *queue);
int ecwam_hip_queue_wait_for(ecwam_hip_ctx *ctx, void *waiter, void *waited);
/* Page-lock host arrays the host keeps copying to / from (the reference pins its fields when WAM_HAVE_CUDA, wvalloc.F90:49-52) */
int ecwam_hip_host_register(ecwam_hip_ctx *ctx, void *host, unsigned long long bytes);
int ecwam_hip_host_unregister(ecwam_hip_ctx *ctx, void *host);

#ifdef __cplusplus
}
#endif
#endif
