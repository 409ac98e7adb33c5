/*
 * tests/csrc/wdfluxes_ref.c -- TEST INFRASTRUCTURE ONLY: the CPU reference of ecwam_hip_wdfluxes and ecwam_hip_setice.
 * WDFLUXES (wdfluxes.F90:156-306) is a driver over routines the oracle already restates as file-local functions (FKMEAN, SINFLX with
 * NCALL and LUPDTUS, SDISSIP, SNONLIN, SDICE, WNFLUXES with LNUPD, FEMEANWS, STOKESDRIFT), so this file includes the oracle's
 * source and adds the driver; tests/wdfluxes_ref.py builds it with the oracle's flags beside ora_tables.c and ora_propag.c.
 */
#include "../../oracle/ora_implsch.c"

/* wdfluxes.F90:156-306 for one point: FL1 and the forcing are inputs only (SINFLX with LUPDTUS = F changes neither) */
static int wdfluxes_point(real *FL1, real *XLLWS, point_t *p) {
  const int NANG = S.NANG, NFRE = S.NFRE;
  static __thread real FLD[NA * NF], SL[NA * NF], SPOS[NA * NF], SSOURCE[NA * NF], SLICE[NA * NF];
  real EMEAN, FMEAN, F1MEAN, AKMEAN, XKMEAN, HALP = 0, FMEANWS, EMEANWS, PHIWA, RAORW, DELT5, ALPFAC;
  real FLM[NA], COSWDIF[NA], SINWDIF2[NA], RHOWGDFTH[NF];
  const int LCFLX = S.c.lwflux || S.c.lwfluxout; /* :156 -- not IMPLSCH's, which also ORs LWNEMOCOU */
  if (S.c.isnonlin < 0 || S.c.isnonlin > 2) return 2;
  if (S.c.lciwa1 && S.NICT == 0) return 2;
  DELT5 = (real)S.c.ximp * (real)S.c.idelt;
  fkmean(FL1, p->WAVNUM, &EMEAN, &FMEAN, &F1MEAN, &AKMEAN, &XKMEAN);
  p->TAUW = C_(0.0);      /* TAUW_LOC, TAUWDIR_LOC: the caller does not copy them back */
  p->TAUWDIR = p->WDWAVE;
  FMEANWS = FMEAN;
  RAORW = RMAX(p->AIRD, C_(1.0)) * S.ROWATERM1;
  ALPFAC = S.ZALPFACX;
  for (int K = 0; K < NANG; K++) {
    FLM[K] = C_(0.0);
    COSWDIF[K] = COS(S.TH[K] - p->WDWAVE);
    real s = SIN(S.TH[K] - p->WDWAVE);
    SINWDIF2[K] = s * s;
  }
  if (S.c.lwnemocouwrs && !(S.c.lciwa1 || S.c.lciwa2 || S.c.lciwa3))
    for (int i = 0; i < NANG * NFRE; i++) SLICE[i] = C_(0.0);
  if (sinflx(1, 1, 0, FL1, p, RAORW, COSWDIF, SINWDIF2, FMEAN, &HALP, &FMEANWS, FLM, &PHIWA, FLD, SL, SPOS, RHOWGDFTH, XLLWS)) return 1;
  if (!LCFLX) return 0;
  if (S.c.iphys == 0) sdissip_jan(FL1, FLD, SL, p->WAVNUM, EMEAN, F1MEAN, XKMEAN);
  else sdissip_ard(FL1, FLD, SL, p->WAVNUM, p->XK2CG, p->UFRIC, COSWDIF, RAORW);
  if (!S.c.lwvflx_snl)
    for (int i = 0; i < NANG * NFRE; i++) SSOURCE[i] = SL[i];
  snonlin(FL1, FLD, SL, p->DEPTH, AKMEAN, p->WAVNUM);
  if (S.c.lwvflx_snl)
    for (int i = 0; i < NANG * NFRE; i++) SSOURCE[i] = SL[i] / RMAX((C_(1.0) - DELT5 * FLD[i]), C_(1.0));
  if (S.c.licerun) { /* :244-270: after SSOURCE is taken; SLICE is read with LWNEMOCOUWRS only */
    if (S.c.lciscal) {
      real BETA = C_(1.0) - p->CICOVER;
      for (int i = 0; i < NANG * NFRE; i++) { SL[i] = BETA * SL[i]; FLD[i] = BETA * FLD[i]; }
    }
    if (S.c.lwnemocouibr && p->IBRMEM <= S.ZIBRW_THRSH) ALPFAC = C_(1.0) / S.ZALPFACX;
    if (S.c.lciwa1) sdice1(FL1, FLD, SL, SLICE, p->CGROUP, p->CICOVER, p->CITHICK);
    if (S.c.lciwa2) sdice2(FL1, FLD, SL, SLICE, p->WAVNUM, p->CGROUP, p->CICOVER);
    if (S.c.lciwa3) sdice3(FL1, FLD, SL, SLICE, p->CGROUP, p->CICOVER, p->CITHICK, ALPFAC);
  }
  wnfluxes(p, RHOWGDFTH, SSOURCE, SLICE, PHIWA, EMEAN, F1MEAN, 0);
  if (S.c.lwflux) {
    femeanws(FL1, XLLWS, &FMEANWS, &EMEANWS);
    if (EMEANWS < S.WSEMEAN_MIN) { p->WSEMEAN = S.WSEMEAN_MIN; p->WSFMEAN = C_(2.) * S.FR[NFRE - 1]; }
    else { p->WSEMEAN = EMEANWS; p->WSFMEAN = FMEANWS; }
  }
  /* stokestrn.F90:66-89 */
  stokesdrift(FL1, p->STOKFAC, p->WSWAVE, p->WDWAVE, p->CICOVER, &p->USTOKES, &p->VSTOKES);
  if (S.c.lwnemocoustrn) p->STRNMS = cimsstrn(FL1, p->WAVNUM, p->DEPTH, p->CITHICK);
  if (S.c.lwnemocou && ((S.c.lwnemocousend && S.c.lwcou) || !S.c.lwcou)) {
    if (S.c.lwnemocoustk) { p->NEMOUSTOKES = p->USTOKES; p->NEMOVSTOKES = p->VSTOKES; }
    else { p->NEMOUSTOKES = 0.0; p->NEMOVSTOKES = 0.0; }
    if (S.c.lwnemocoustrn) p->NEMOSTRN = p->STRNMS;
  }
  return 0;
}

/* Batched entry, the layouts of ora_implsch_w2n.  FL1 and FF are never written; INTF, MIJ, XLLWS and W2N (may be NULL) are outputs. */
int ora_wdfluxes(int n, real *FL1, const real *WAVNUM, const real *CGROUP, const real *CINV, const real *XK2CG, const real *STOKFAC,
                 const real *ENV, const real *FF, real *INTF, int *MIJ, real *XLLWS, double *W2N, const real *IBRMEM) {
  const int NANG = S.NANG, NFRE = S.NFRE;
  int rc = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(| : rc)
  for (int ij = 0; ij < n; ij++) {
    point_t p;
    memset(&p, 0, sizeof(p));
    p.WAVNUM = WAVNUM + (size_t)ij * NFRE; p.CGROUP = CGROUP + (size_t)ij * NFRE; p.CINV = CINV + (size_t)ij * NFRE;
    p.XK2CG = XK2CG + (size_t)ij * NFRE; p.STOKFAC = STOKFAC + (size_t)ij * NFRE;
    p.EMAXDPT = ENV[ij * 2]; p.DEPTH = ENV[ij * 2 + 1];
    p.IBRMEM = IBRMEM ? IBRMEM[ij] : C_(1.0);
    const real *ff = FF + (size_t)ij * 14;
    real *it = INTF + (size_t)ij * 15;
    p.AIRD = ff[0]; p.WDWAVE = ff[1]; p.CICOVER = ff[2]; p.WSWAVE = ff[3]; p.WSTAR = ff[4]; p.USTRA = ff[5]; p.VSTRA = ff[6];
    p.UFRIC = ff[7]; p.TAUW = ff[8]; p.TAUWDIR = ff[9]; p.Z0M = ff[10]; p.Z0B = ff[11]; p.CHRNCK = ff[12]; p.CITHICK = ff[13];
    p.WSEMEAN = it[0]; p.WSFMEAN = it[1]; p.USTOKES = it[2]; p.VSTOKES = it[3]; p.STRNMS = it[4]; p.TAUXD = it[5];
    p.TAUYD = it[6]; p.TAUOCXD = it[7]; p.TAUOCYD = it[8]; p.TAUOC = it[9]; p.TAUICX = it[10]; p.TAUICY = it[11];
    p.PHIOCD = it[12]; p.PHIEPS = it[13]; p.PHIAW = it[14];
    if (W2N) {
      const double *w = W2N + (size_t)ij * 13;
      p.NEMOUSTOKES = w[0]; p.NEMOVSTOKES = w[1]; p.NEMOSTRN = w[2]; p.NPHIEPS = w[3]; p.NTAUOC = w[4]; p.NSWH = w[5]; p.NMWP = w[6];
      p.NEMOTAUX = w[7]; p.NEMOTAUY = w[8]; p.NEMOTAUICX = w[9]; p.NEMOTAUICY = w[10]; p.NEMOWSWAVE = w[11]; p.NEMOPHIF = w[12];
    }
    rc |= wdfluxes_point(FL1 + (size_t)ij * NANG * NFRE, XLLWS + (size_t)ij * NANG * NFRE, &p);
    if (W2N) {
      double *w = W2N + (size_t)ij * 13;
      w[0] = p.NEMOUSTOKES; w[1] = p.NEMOVSTOKES; w[2] = p.NEMOSTRN; w[3] = p.NPHIEPS; w[4] = p.NTAUOC; w[5] = p.NSWH; w[6] = p.NMWP;
      w[7] = p.NEMOTAUX; w[8] = p.NEMOTAUY; w[9] = p.NEMOTAUICX; w[10] = p.NEMOTAUICY; w[11] = p.NEMOWSWAVE; w[12] = p.NEMOPHIF;
    }
    it[0] = p.WSEMEAN; it[1] = p.WSFMEAN; it[2] = p.USTOKES; it[3] = p.VSTOKES; it[4] = p.STRNMS; it[5] = p.TAUXD;
    it[6] = p.TAUYD; it[7] = p.TAUOCXD; it[8] = p.TAUOCYD; it[9] = p.TAUOC; it[10] = p.TAUICX; it[11] = p.TAUICY;
    it[12] = p.PHIOCD; it[13] = p.PHIEPS; it[14] = p.PHIAW;
    MIJ[ij] = p.MIJ;
  }
  return rc;
}

/* setice.F90:67-86 on n points: CICOVER = FF[ij][2], WDWAVE = FF[ij][1] */
void ora_setice_pts(int n, real *FL1, const real *FF) {
  const int NANG = S.NANG, NFRE = S.NFRE;
  for (int ij = 0; ij < n; ij++) {
    real COSWDIF[NA];
    for (int K = 0; K < NANG; K++) COSWDIF[K] = COS(S.TH[K] - FF[(size_t)ij * 14 + 1]);
    setice(FL1 + (size_t)ij * NANG * NFRE, FF[(size_t)ij * 14 + 2], COSWDIF);
  }
}
