// C ABI of libecwam_hip.so (include/ecwam_hip.h): context management and kernel launch entry points.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is loaded with dlopen when a communicator is asked for

#include "../../include/ecwam_hip_forcing.h"
#include "../../include/ecwam_hip_start.h"
#include "dev.h"
#include "implsch_v4_shapes.h"
#include "launch.h"

static thread_local std::string g_err;
static int fail(const std::string& m) {
  g_err = m;
  return 1;
}
#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_));   \
  } while (0)
// the end of an entry point that launched something: the launch's own error, if any
static int launched() {
  HIPCHK(hipGetLastError());
  return 0;
}

struct ecwam_hip_ctx {
  int real_bytes;
  int device;
  int NANG, NFRE, NFRE_RED;
  void* dtab = nullptr;  // DevTab<T> in device memory
  double* norm_scratch = nullptr;   // ecwam_hip_outwnorm: per-context reduction scratch (4 + 4 x 256 doubles)
  void* itab = nullptr;  // IntpolTab<T> (csrc/outbs_fl2nd.hip) in device memory when IREFRA = 2 / 3: INTPOL's source-frequency tables
  // fourth kernel generation (implsch_v4.h): DIA rotations K1 = K -+ r1, K2 = K +- r2, NSDSNTH = nh; ok = the tables have that structure
  int v4_ok = 0, v4_r1 = 0, v4_r2 = 0, v4_nh = 0, v4_shelter = 0;
  int implsch_last = 0; // generation the last ecwam_hip_implsch call launched (4; 0 before the first call)
  void* fin = nullptr;  // rows of scalars k_implsch4 hands to its finishing kernel, indexed by the point number; grown on demand
  size_t fin_bytes = 0;
  void* wi = nullptr;   // rows [ij][M][K] for the wind-input coefficient between the two kernels of the split k_implsch4 (only allocated
  size_t wi_bytes = 0;  // where the split runs: the double precision RARE builds)
  // advection halo exchange (MPEXCHNG): peers, the owned rows each of them needs (concatenated in peer order) and where their rows
  // land; RCCL communicator + a stream of its own so that the exchange runs beside the interior stencil
  int rank = 0, nranks = 1;
  std::vector<int> peer, send_cnt, send_off, recv_dst0, recv_cnt;
  int n_send = 0, n_recv = 0;
  int* d_send_idx = nullptr;
  // one send buffer + event pair per row length in use (full rows, compact fast-wave rows, PROENVHALO rows): two exchanges of
  // different rows may be outstanding at once (propag_wam.F90:166,293) without the second pack waiting for the first one's sends
  struct HaloSlot {
    int rowlen = 0;
    void* buf = nullptr;
    size_t bytes = 0;
    hipEvent_t ev_packed = nullptr, ev_done = nullptr;
    bool used = false;      // an exchange has been posted from this buffer: a later pack waits for its sends (ev_done)
    bool pending = false;   // ... and no ecwam_hip_halo_finish has made a stream wait for it yet
    unsigned long long age = 0;
  };
  static constexpr int NSLOT = 4;
  HaloSlot slot[NSLOT];
  unsigned long long slot_clock = 0;
  ncclComm_t comm = nullptr;
  hipStream_t comm_stream = nullptr;
  ecwam_hip_params p;
  void* fast_g = nullptr;     // ecwam_hip_set_fastwave_copy: compact rows [ij][K][fast_gk] IMPLSCH / NOSOURCE also leave the new fast waves in
  int fast_gk = 0;
  // one-kernel step (ecwam_hip_propags2_implsch): per-point and per-direction scalars of the CTU weights (propag.hip::k_ctu_prep)
  std::string implsch_why;    // non-empty: no build of k_implsch4 covers the configuration (ecwam_hip_implsch refuses with this text)
  void* adv_pt = nullptr;     // [npts][12]
  size_t adv_pt_bytes = 0;
  void* adv_dir = nullptr;    // reals [4 NANG + 4], then ints [4 NANG]
  // LSECONDORDER (ecwam_hip_set_second_order; csrc/outbs_2nd.hip): SoTab<T>, the coefficient tables [JD][M][M1][5][NANGH], the work space
  void* so_tab = nullptr;
  void* so_coef = nullptr;
  void* so_work = nullptr;
  size_t so_work_bytes = 0;
  int so_nmax = 0;
  std::vector<unsigned char> fr_host;  // FR(1:NFRE) in the working precision
  // ecwam_hip_set_outbs_integrals (csrc/outbs_int.hip): IntTab<T> in device memory; the number of bands, -1 before the setter is called
  void* int_tab = nullptr;
  int int_nband = -1;
  std::vector<double> int_tb, int_tt;   // the bands as passed: ecwam_hip_set_outblock compares them with the period intervals of the request
  // ecwam_hip_set_outblock (csrc/outblock.hip): the plan, its per-column descriptors on the device, the work space of ecwam_hip_outblock
  OutblockPlan ob_plan;
  bool ob_set = false;
  int* ob_desc = nullptr;
  void* ob_work = nullptr;
  size_t ob_work_bytes = 0;
  // ecwam_hip_set_forcing_map (csrc/forcing.hip): the validated maps row -> cell on the device, [fmap_n] each, and the cells of their grids
  int* fmap_in = nullptr;
  int* fmap_out = nullptr;
  int fmap_n = 0;
  size_t fmap_ncell_in = 0, fmap_ncell_out = 0;
  // ecwam_hip_set_fldinter (csrc/intake.hip): the validated table on the device -- the source positions int [fli_n][4] and the weights, reals
  // [fli_n][4] (nullptr without interpolation)
  int* fli_idx = nullptr;
  void* fli_w = nullptr;
  int fli_n = 0, fli_ngptotg = 0, fli_interpol = 0;
  // ecwam_hip_set_input_grid (csrc/readwind.hip): per slot the validated table on the device -- the positions int [ncell][4] and reals [ncell][4]: DK1, DII1,
  // DIIP1 and the kind
  struct G2wSlot {
    int* pos = nullptr;
    void* w = nullptr;
    int ncell = 0, nvalues = 0, interpol = 0;
  };
  G2wSlot g2w[ECWAM_HIP_G2W_NSLOT];
  // ecwam_hip_set_restart_map (csrc/restart.hip): the inverse of the validated IJ2NEWIJ on the device -- row -> position in a vector of the global order
  int* rmap_inv = nullptr;
  int rmap_n = 0;
  // ecwam_hip_set_grib_map (csrc/gribout.hip): the validated map on the device (gmap.ival == nullptr: none), its rows, the scratch of the maxima
  GribMapDev gmap = {};
  int gmap_n = 0;
  void* gmap_keys = nullptr;
  const void* obs = nullptr;  // LSUBGRID: device OBS[n_obs][8][NFRE] (ecwam_hip_set_obstructions), read by CTUW / PROPAGS2
  int n_obs = 0;
  RotatedTables rot;          // IPROPAGS = 1: the device tables of ecwam_hipx_set_rotated, read by ecwam_hipx_propags1
};

static void grib_map_free(ecwam_hip_ctx* c) {
  if (c->gmap.ival) (void)hipFree(const_cast<int*>(c->gmap.ival));
  if (c->gmap.unfilled) (void)hipFree(const_cast<int*>(c->gmap.unfilled));
  if (c->gmap.adj) (void)hipFree(const_cast<int*>(c->gmap.adj));
  if (c->gmap_keys) (void)hipFree(c->gmap_keys);
  c->gmap = GribMapDev{};
  c->gmap_n = 0;
  c->gmap_keys = nullptr;
}

// f(T()) with T = the working precision of the context, float or double: every launch is written once, as launch_x<decltype(t)>(...)
template <typename F>
static auto in_precision(const ecwam_hip_ctx* c, F&& f) {
  return c->real_bytes == 4 ? f(float()) : f(double());
}

// Does the fourth kernel generation cover these tables?  It needs the pull-form DIA structure with K1W = K -+ r1, K11W = K1W -+ 1,
// K2W = K +- r2, K21W = K2W +- 1 (kh = 1 / 2) and saturation weights that depend on the tap only (init_sdiss_ardh.F90:88-94: they
// are COS**2 of a multiple of DELTH, equal for all K up to rounding).
template <typename T>
static void v4_probe(const DevTab<T>& h, ecwam_hip_ctx* c) {
  c->v4_ok = 0;
  const int NANG = h.NANG;
  if (!h.DIA_PULL || !h.V4_ROWS || (NANG & 1) || h.NFRE != 36) return;
  const int r1 = (NANG - h.K1W[0][0]) % NANG, r2 = h.K2W[0][0];
  if (h.D11[0] != -1 || h.D21[0] != 1 || h.D11[1] != 1 || h.D21[1] != -1) return;
  if (h.K1W[1][0] != r1 % NANG || h.K2W[1][0] != (NANG - r2) % NANG) return;
  T wmax = T(0);
  for (int t = 0; t < h.NTAP; t++) wmax = wmax > h.SATWEIGHTS[t][NANG / 2] ? wmax : h.SATWEIGHTS[t][NANG / 2];
  const T eps = sizeof(T) == 4 ? T(1.2e-7) : T(2.3e-16);
  for (int t = 0; t < h.NTAP; t++)
    for (int k = 0; k < NANG; k++) {
      const T d = h.SATWEIGHTS[t][k] - h.SATWEIGHTS[t][NANG / 2];
      if ((d < 0 ? -d : d) > T(16) * eps * wmax) return;
      const T e = h.SATWEIGHTS[t][NANG / 2] - h.SATWEIGHTS[h.NTAP - 1 - t][NANG / 2];   // symmetric about the centre tap
      if ((e < 0 ? -e : e) > T(16) * eps * wmax) return;
      if (h.INDICESSAT[t][k] != ((k - h.NSDSNTH + t) % NANG + NANG) % NANG) return;
    }
  c->v4_r1 = r1; c->v4_r2 = r2; c->v4_nh = h.NSDSNTH; c->v4_shelter = (h.TAUWSHELTER != T(0)); c->v4_ok = 1;
}

template <typename T>
static void cpv(T* dst, const void* src, int n) {
  if (src) for (int i = 0; i < n; i++) dst[i] = ((const T*)src)[i];
}

template <typename T>
static int build_tab(const ecwam_hip_params* p, const ecwam_hip_tables* t, DevTab<T>* d) {
  memset(d, 0, sizeof(*d));
  const int NANG = p->nang, NFRE = p->nfre, ML = p->mlsthg;
  d->NANG = NANG; d->NFRE = NFRE; d->NFRE_RED = p->nfre_red; d->NFRE_ODD = p->nfre_odd; d->IDELT = p->idelt;
  d->LLGCBZ0 = p->llgcbz0; d->LLNORMAGAM = p->llnormagam; d->LLCAPCHNK = p->llcapchnk; d->LBIWBK = p->lbiwbk;
  d->LICERUN = p->licerun; d->LMASKICE = p->lmaskice; d->LWAMRSETCI = p->lwamrsetci; d->LWVFLX_SNL = p->lwvflx_snl;
  d->LWFLUX = p->lwflux; d->LCFLX = (p->lwflux || p->lwfluxout || p->lwnemocou); d->LWNEMOCOU = p->lwnemocou; d->LWCOU = p->lwcou;
  d->LWCOUAST = p->lwcouast; d->LWNEMOCOUWRS = p->lwnemocouwrs; d->LCFLX_WD = (p->lwflux || p->lwfluxout);
  d->LWNEMOTAUOC = p->lwnemotauoc; d->LWNEMOCOUSEND = p->lwnemocousend; d->LWNEMOCOUSTK = p->lwnemocoustk;
  d->ICODE = p->icode; d->ISNONLIN = p->isnonlin; d->IPHYS = p->iphys; d->IDAMPING = p->idamping;
  d->LCISCAL = p->lciscal; d->LCIWA2 = p->lciwa2; d->LCIWA3 = p->lciwa3;
  d->LCIWA1 = p->lciwa1; d->LWNEMOCOUIBR = p->lwnemocouibr; d->LWNEMOCOUSTRN = p->lwnemocoustrn; d->NICT = p->nict; d->NICH = p->nich;
  for (int i = 0; i < 36 * 16; i++) d->CIDEAC[i] = T(0);
  if (p->lciwa1 && t->cideac) cpv(d->CIDEAC, t->cideac, p->nict * p->nich);
  d->DBG_SKIP = 0;
#ifdef ECWAM_HIP_DIAGNOSTICS   // timing builds only (tools/): phases of IMPLSCH skipped / early returns; never in the product library
  { const char* e_ = getenv("ECWAM_HIP_DEBUG_SKIP"); d->DBG_SKIP = e_ ? atoi(e_) : 0; }
#endif
  d->NSDSNTH = p->nsdsnth; d->NTAP = 2 * p->nsdsnth + 1; d->MFRSTLW = p->mfrstlw; d->MLSTHG = ML; d->KFRH = p->kfrh; d->NWAV_GC = p->nwav_gc;
#define S_(dst, src) d->dst = (T)p->src
  S_(ZIBRW_THRSH, zibrw_thrsh); S_(TICMIN, ticmin); S_(DTIC, dtic); S_(DHIC, dhic); S_(HICMIN, hicmin);
  S_(XIMP, ximp); S_(G, g); S_(GM1, gm1); S_(PI, pi); S_(ZPI, zpi); S_(ZPI4GM1, zpi4gm1); S_(ZPI4GM2, zpi4gm2); S_(EPSMIN, epsmin);
  S_(ROWATER, rowater); S_(ROWATERM1, rowaterm1); S_(EPSUS, epsus); S_(EPSU10, epsu10); S_(ACD, acd); S_(BCD, bcd);
  S_(ACDLIN, acdlin); S_(BCDLIN, bcdlin); S_(CDMAX, cdmax); S_(TAUOCMIN, tauocmin); S_(TAUOCMAX, tauocmax);
  S_(PHIEPSMIN, phiepsmin); S_(PHIEPSMAX, phiepsmax); S_(WSEMEAN_MIN, wsemean_min); S_(CIRC, circ); S_(R, r_earth);
  S_(FRATIO, fratio); S_(WETAIL, wetail); S_(FRTAIL, frtail); S_(WP1TAIL, wp1tail); S_(FRIC, fric); S_(DELTH, delth);
  S_(FLOGSPRDM1, flogsprdm1); S_(XKAPPA, xkappa); S_(XNLEV, xnlev); S_(RNU, rnu); S_(RNUM, rnum);
  S_(BETAMAXOXKAPPA2, betamaxoxkappa2); S_(BMAXOKAP, bmaxokap); S_(GAMNCONST, gamnconst); S_(ZALP, zalp); S_(ALPHA, alpha);
  S_(ALPHAMIN, alphamin); S_(ALPHAMAX, alphamax); S_(CHNKMIN_U, chnkmin_u); S_(TAUWSHELTER, tauwshelter); S_(DTHRN_A, dthrn_a);
  S_(DTHRN_U, dthrn_u); S_(TAILFACTOR, tailfactor); S_(TAILFACTOR_PM, tailfactor_pm); S_(ANG_GC_A, ang_gc_a);
  S_(ANG_GC_B, ang_gc_b); S_(ANG_GC_C, ang_gc_c); S_(RN1_RN, rn1_rn); S_(ALPHAPMAX, alphapmax); S_(CDIS, cdis); S_(DELTA_SDIS, delta_sdis); S_(CDISVIS, cdisvis); S_(CDICWA, cdicwa); S_(ZALPFACB, zalpfacb); S_(ZALPFACX, zalpfacx); S_(SWELLF, swellf); S_(SWELLF2, swellf2);
  S_(SWELLF3, swellf3); S_(SWELLF4, swellf4); S_(SWELLF5, swellf5); S_(SWELLF6, swellf6); S_(SWELLF7, swellf7);
  S_(SWELLF7M1, swellf7m1); S_(Z0RAT, z0rat); S_(Z0TUBMAX, z0tubmax); S_(ABMIN, abmin); S_(ABMAX, abmax); S_(SDSBR, sdsbr);
  S_(SSDSC2, ssdsc2); S_(SSDSC3, ssdsc3); S_(SSDSC4, ssdsc4); S_(SSDSC5, ssdsc5); S_(SSDSC6, ssdsc6); S_(MICHE, miche);
  S_(EGRCRV, egrcrv); S_(AFCRV, afcrv); S_(BFCRV, bfcrv); S_(X0TAUHF, x0tauhf); S_(EPS1, eps1); S_(FLMIN, flmin);
  S_(CITHRSH, cithrsh); S_(CIBLOCK, ciblock); S_(CITHRSH_TAIL, cithrsh_tail); S_(ZALPWRS, zalpwrs); S_(BATHYMAX, bathymax);
  S_(WSPMIN, wspmin); S_(WSPMIN_RESET_TAUW, wspmin_reset_tauw); S_(DAL1, dal1); S_(DAL2, dal2);
  S_(XLOGKRATIOM1_GC, xlogkratiom1_gc); S_(SQRTGOSURFT, sqrtgosurft);
#undef S_
  cpv(d->FR, t->fr, NFRE); cpv(d->DFIM, t->dfim, NFRE); cpv(d->DFIMOFR, t->dfimofr, NFRE); cpv(d->DFIMFR, t->dfimfr, NFRE);
  cpv(d->DFIM_SIM, t->dfim_sim, NFRE); cpv(d->RHOWG_DFIM, t->rhowg_dfim, NFRE); cpv(d->ZPIFR, t->zpifr, NFRE);
  cpv(d->FR5, t->fr5, NFRE); cpv(d->COFRM4, t->cofrm4, NFRE); cpv(d->FLMAX, t->flmax, NFRE);
  cpv(d->TH, t->th, NANG); cpv(d->COSTH, t->costh, NANG); cpv(d->SINTH, t->sinth, NANG);
  cpv(d->WTAUHF, t->wtauhf, JTOT);
  cpv(d->SWELLFT + 1, t->swellft, ECWAM_HIP_IAB);
  for (int i = 0; i < ML; i++) { d->IKP[i] = t->ikp[i]; d->IKP1[i] = t->ikp1[i]; d->IKM[i] = t->ikm[i]; d->IKM1[i] = t->ikm1[i]; }
  cpv(d->AF11, t->af11, ML);
  for (int k = 0; k < NANG; k++)
    for (int kh = 0; kh < 2; kh++) {
      d->K1W[kh][k] = t->k1w[k * 2 + kh] - 1; d->K2W[kh][k] = t->k2w[k * 2 + kh] - 1;
      d->K11W[kh][k] = t->k11w[k * 2 + kh] - 1; d->K21W[kh][k] = t->k21w[k * 2 + kh] - 1;
    }
  // structure check for the pull-form DIA kernel: K1W/K2W rotations, K11W/K21W = K1W/K2W +-1, row offsets -4,-3,+2,+3
  d->DIA_PULL = 1;
  for (int kh = 0; kh < 2 && d->DIA_PULL; kh++) {
    const int s1 = ((d->K1W[kh][0] - 0) % NANG + NANG) % NANG, s2 = ((d->K2W[kh][0] - 0) % NANG + NANG) % NANG;
    const int e1 = ((d->K11W[kh][0] - d->K1W[kh][0]) % NANG + NANG) % NANG, e2 = ((d->K21W[kh][0] - d->K2W[kh][0]) % NANG + NANG) % NANG;
    if (!((e1 == 1 || e1 == NANG - 1) && (e2 == 1 || e2 == NANG - 1))) { d->DIA_PULL = 0; break; }
    d->D11[kh] = (e1 == 1) ? 1 : -1;
    d->D21[kh] = (e2 == 1) ? 1 : -1;
    for (int k = 0; k < NANG; k++) {
      if (d->K1W[kh][k] != (k + s1) % NANG || d->K2W[kh][k] != (k + s2) % NANG || d->K11W[kh][k] != (k + s1 + e1) % NANG ||
          d->K21W[kh][k] != (k + s2 + e2) % NANG) { d->DIA_PULL = 0; break; }
      d->IK1[kh][(k + s1) % NANG] = k;
      d->IK2[kh][(k + s2) % NANG] = k;
    }
  }
  for (int i = 0; i < ML && d->DIA_PULL; i++) {
    const int MC = i + 1;
    if (t->ikp[i] != MC + 2 || t->ikp1[i] != MC + 3) d->DIA_PULL = 0;
    if (t->ikm[i] != MC - 4 || t->ikm1[i] != MC - 3) d->DIA_PULL = 0;
  }
  if (ML != NFRE + 4 || p->kfrh != 8 || p->mfrstlw != -3) d->DIA_PULL = 0;
  bool sep_ok = true;      // RNLCOEF factors as frequency factor x angular weight (checked below)
  for (int i = 0; i < ML; i++) {
    for (int j = 0; j < 5; j++) d->INLCOEF[i][j] = t->inlcoef[i * 5 + j] - 1;
    for (int j = 0; j < 25; j++) d->RNLCOEF[i][j] = ((const T*)t->rnlcoef)[i * 25 + j];
  }
  {
    // separable form of the interaction coefficients: CL11 + ACL1 = 1 and CL21 + ACL2 = 1 (nlweigt.F90:166-169), so the frequency factor of a
    // coefficient pair is its sum and the angular weights are the ratios, taken where the factors are largest
    double cl11 = 1.0, acl1 = 0.0, cl21 = 1.0, acl2 = 0.0, bp = 0.0, bm = 0.0;
    for (int i = 0; i < ML; i++) {
      const double pa = (double)d->RNLCOEF[i][5], pb = (double)d->RNLCOEF[i][6], ma = (double)d->RNLCOEF[i][17], mb = (double)d->RNLCOEF[i][18];
      if (fabs(pa + pb) > bp) { bp = fabs(pa + pb); cl11 = pa / (pa + pb); acl1 = pb / (pa + pb); }
      if (fabs(ma + mb) > bm) { bm = fabs(ma + mb); cl21 = ma / (ma + mb); acl2 = mb / (ma + mb); }
    }
    const double ang[8] = {cl11, acl1, cl21, acl2, cl11 * cl11, acl1 * acl1, cl21 * cl21, acl2 * acl2};
    for (int j = 0; j < 8; j++) d->DIAANG[j] = (T)ang[j];
    for (int i = 0; i < ML; i++) {
      const T* R = d->RNLCOEF[i];
      const double gp = (double)R[1] + R[2], gp1 = (double)R[3] + R[4], gm = (double)R[13] + R[14], gm1 = (double)R[15] + R[16];
      const double fp = (double)R[5] + R[6], fp1 = (double)R[8] + R[7], fm = (double)R[17] + R[18], fm1 = (double)R[20] + R[19];
      const double w[12] = {gp, gp1, gm, gm1, fp, fp1, fp * fp, fp1 * fp1, fm, fm1, fm * fm, fm1 * fm1};
      for (int j = 0; j < 12; j++) d->DIAW[i][j] = (T)w[j];
    }
    for (int i = 0; i < ML; i++)
      for (int j = 0; j < 4; j++) d->DIAW[i][12 + j] = (i + 1 < ML) ? d->DIAW[i + 1][j] : T(0);
    // The kernel never reads RNLCOEF(2:25): it forms the coefficients as frequency factor x angular weight (inisnonlin.F90:186-241).  Tables
    // that do not factor that way (not from INISNONLIN, or modified) would silently give another Snl: rebuild every word and compare;
    // V4_ROWS = 0 makes ecwam_hip_create refuse the tables with the reason.
    const double tol = (sizeof(T) == 4 ? 1.2e-7 : 2.3e-16) * 64.0;
    for (int i = 0; i < ML && sep_ok; i++) {
      const T* R = d->RNLCOEF[i];
      const T* W = d->DIAW[i];
      const double gp = W[0], gp1 = W[1], gm = W[2], gm1 = W[3], fp = W[4], fp1 = W[5], fm = W[8], fm1 = W[9];
      const double want[24] = {gp * cl11, gp * acl1, gp1 * cl11, gp1 * acl1, fp * cl11, fp * acl1, fp1 * acl1, fp1 * cl11,
                               (fp * cl11) * (fp * cl11), (fp * acl1) * (fp * acl1), (fp1 * cl11) * (fp1 * cl11), (fp1 * acl1) * (fp1 * acl1),
                               gm * cl21, gm * acl2, gm1 * cl21, gm1 * acl2, fm * cl21, fm * acl2, fm1 * acl2, fm1 * cl21,
                               (fm * cl21) * (fm * cl21), (fm * acl2) * (fm * acl2), (fm1 * cl21) * (fm1 * cl21), (fm1 * acl2) * (fm1 * acl2)};
      for (int j = 0; j < 24; j++) {
        const double scale = fabs(want[j]) > fabs((double)R[1 + j]) ? fabs(want[j]) : fabs((double)R[1 + j]);
        if (fabs(want[j] - (double)R[1 + j]) > tol * scale) sep_ok = false;
      }
    }
  }
  d->V4_ROWS = sep_ok ? 1 : 0;
  for (int i = 0; i < ML; i++) {
    // gather set (words 0..11): FTAIL, GW1..GW8, AF11; scatter set (words 12..27): FKLAMPA .. FKLAP22, FKLAMMA .. FKLAM22
    for (int j = 0; j < 32; j++) d->DIACF[i][j] = T(0);
    d->DIACF[i][0] = d->RNLCOEF[i][0];
    for (int j = 0; j < 4; j++) { d->DIACF[i][1 + j] = d->RNLCOEF[i][1 + j]; d->DIACF[i][5 + j] = d->RNLCOEF[i][13 + j]; }
    d->DIACF[i][9] = d->AF11[i];
    for (int j = 0; j < 8; j++) { d->DIACF[i][12 + j] = d->RNLCOEF[i][5 + j]; d->DIACF[i][20 + j] = d->RNLCOEF[i][17 + j]; }
    const int MC = i + 1;
    auto cl = [&](int r) { return (r < 1 ? 1 : (r > NFRE ? NFRE : r)) - 1; };
    {  // snonlin.F90:236-240: the tail factor applies outside MFR1STFR < MC < MFRLSTFR
      const int MFR1STFR = -p->mfrstlw + 1, MFRLSTFR = NFRE - p->kfrh + MFR1STFR;
      d->DIACF[i][31] = (MC > MFR1STFR && MC < MFRLSTFR) ? T(1) : d->RNLCOEF[i][0];
    }
    d->DIACF[i][10] = d->ZPIFR[cl(MC - 3)];
    const int mu = cl(MC - 5);
    d->DIACF[i][28] = d->COFRM4[mu]; d->DIACF[i][29] = d->FLMAX[mu]; d->DIACF[i][30] = d->RHOWG_DFIM[mu]; d->DIACF[i][11] = d->ZPIFR[mu];
    const int want[5] = {cl(MC), cl(MC + 2), cl(MC + 3), cl(MC - 4), cl(MC - 3)};
    for (int j = 0; j < 5; j++) if (d->INLCOEF[i][j] != want[j]) d->V4_ROWS = 0;
  }
  for (int i = 0; i <= ML; i++) {
    const int k = i < ML ? i : ML - 1;
    static const int w7[7] = {9, 10, 11, 28, 29, 30, 31};
    for (int j = 0; j < 7; j++) d->DIAREC[i][j] = d->DIACF[k][w7[j]];
    d->DIAREC[i][7] = T(0);
    for (int j = 0; j < 12; j++) d->DIAREC[i][8 + j] = d->DIAW[k][4 + j];
  }
  for (int m = 0; m < NFRE; m++) {
    T* r = d->SINROW[m];
    r[0] = d->ZPIFR[m]; r[1] = d->DFIM[m];
    r[2] = -d->SWELLF5 * T(2) * std::sqrt(T(2) * d->RNU * d->ZPIFR[m]);
    r[3] = -d->SWELLF * T(16) * (d->ZPIFR[m] * d->ZPIFR[m]) / d->G;
    r[4] = d->RHOWG_DFIM[m]; r[5] = d->DFIMOFR[m]; r[6] = d->DFIMFR[m]; r[7] = T(0);
  }
  const int ntap = 2 * p->nsdsnth + 1;
  for (int k = 0; k < NANG; k++)
    for (int j = 0; j < ntap; j++) {
      d->INDICESSAT[j][k] = t->indicessat[k * ntap + j] - 1;
      d->SATWEIGHTS[j][k] = ((const T*)t->satweights)[k * ntap + j];
    }
  for (int k = 0; k < NANG; k++) {
    for (int j = 0; j < 3; j++) d->KPM[k][j] = t->kpm[k * 3 + j] - 1;
    for (int j = 0; j < 2; j++) { d->JXO[k][j] = t->jxo[k * 2 + j] - 1; d->JYO[k][j] = t->jyo[k * 2 + j] - 1; }
    for (int j = 0; j < 4; j++) d->KCR[k][j] = t->kcr[k * 4 + j] - 1;
  }
  const int ng = p->nwav_gc;
  cpv(d->XK_GC + 1, t->xk_gc, ng); cpv(d->XKM_GC + 1, t->xkm_gc, ng); cpv(d->OMEGA_GC + 1, t->omega_gc, ng);
  cpv(d->OMXKM3_GC + 1, t->omxkm3_gc, ng); cpv(d->CM_GC + 1, t->cm_gc, ng); cpv(d->C2OSQRTVG_GC + 1, t->c2osqrtvg_gc, ng);
  cpv(d->XKMSQRTVGOC2_GC + 1, t->xkmsqrtvgoc2_gc, ng); cpv(d->OM3GMKM_GC + 1, t->om3gmkm_gc, ng);
  cpv(d->DELKCC_GC_NS + 1, t->delkcc_gc_ns, ng); cpv(d->DELKCC_OMXKM3_GC + 1, t->delkcc_omxkm3_gc, ng);
  return 0;
}

// ---- lane-primitive self test (one wave): every cross-lane helper of dev.h against serial sums over LDS ----------------
template <typename T>
__global__ void k_selftest(int* nbad) {
  __shared__ T v[4][64];
  const int lane = threadIdx.x;
  T q[4];
  for (int j = 0; j < 4; j++) {
    q[j] = (lane < 36) ? T((lane * (7 + 2 * j) + 3 * j) % 23 + j) : T(0);  // small integers: every summation order is exact
    v[j][lane] = q[j];
  }
  __syncthreads();
  T ref[4], mx[4];
  for (int j = 0; j < 4; j++) {
    ref[j] = T(0); mx[j] = T(0);
    for (int l = 0; l < 64; l++) { ref[j] += v[j][l]; mx[j] = m_max(mx[j], v[j][l]); }
  }
  int bad = 0;
  T a, b, c, d;
  bad += (usum(q[0]) != ref[0]) + (umax(q[1]) != mx[1]);
  usum2(q[0], q[1], a, b); bad += (a != ref[0]) + (b != ref[1]);
  usum4(q[0], q[1], q[2], q[3], a, b, c, d); bad += (a != ref[0]) + (b != ref[1]) + (c != ref[2]) + (d != ref[3]);
  umax2(q[2], q[3], a, b); bad += (a != mx[2]) + (b != mx[3]);
  bad += (lane_get(q[0], 5) != v[0][5]);
  bad += (lane_pull(q[1], (lane + 9) & 63) != v[1][(lane + 9) & 63]);
  bad += (rot_up(q[2], lane, 36) != ((lane < 36) ? v[2][(lane + 35) % 36] : (lane == 36 ? v[2][35] : T(0))));
  // the hot-loop replacements of the library's EXP / SQRT / 1 / SQRT (dev.h) against the library over their argument ranges
  for (int i = 0; i < 256; i++) {
    const T u = T(lane * 256 + i) / T(16384);                      // 0 .. 1
    const T xe = T(-700) * u * u + T(3) * (T(1) - u) - T(1.5);     // EXP: -701.5 .. 1.5, dense near zero
    const T tol = sizeof(T) == 8 ? T(1e-15) : T(1e-4);             // sp: v_exp_f32 of x log2(e), |x| 1.2e-7 relative
    const T ee = m_exp(xe), eg = f_exp(xe);
    bad += !(m_abs(eg - ee) <= tol * ee + (sizeof(T) == 8 ? T(1e-320) : T(1e-37)));
    const T xs = m_exp(T(sizeof(T) == 8 ? 600 : 80) * (T(2) * u - T(1)));   // SQRT, 1 / SQRT: 1e-260 .. 1e260 (sp 1e-35 .. 1e35)
    const T ts = sizeof(T) == 8 ? T(9e-16) : T(3e-7);
    const T sr = m_sqrt(xs);
    bad += !(m_abs(f_sqrt(xs) - sr) <= ts * sr) + !(m_abs(f_rsq(xs) * sr - T(1)) <= T(2) * ts);
  }
  bad += (f_sqrt(T(0)) != T(0)) + (f_exp(T(-1000)) != T(0));
  if (bad) atomicAdd(nbad, bad);
}


// ---- RCCL through dlopen: the library has no link-time dependency on it (single-GPU hosts never load it) ---------------------------
struct RcclApi {
  void* h = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static RcclApi g_rccl;
static int rccl_load() {
  if (g_rccl.h) return 0;
  // By SONAME: in a process that has already mapped an RCCL (PyTorch-ROCm links its bundled librccl.so.1) this returns THAT copy, so that
  // one RCCL and one HIP runtime serve the process; RTLD_LOCAL: a second copy must never interpose its symbols on the first.
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!h) return fail(std::string("RCCL not found (dlopen librccl.so.1): ") + dlerror());
#define SYM_(f) g_rccl.f = (decltype(g_rccl.f))dlsym(h, "nccl" #f); if (!g_rccl.f) return fail("librccl: symbol nccl" #f " missing")
  SYM_(GetUniqueId); SYM_(CommInitRank); SYM_(CommDestroy); SYM_(CommCount); SYM_(GroupStart); SYM_(GroupEnd); SYM_(Send); SYM_(Recv); SYM_(GetErrorString);
#undef SYM_
  g_rccl.h = h;
  return 0;
}
#define NCCLCHK(x)                                                                                   \
  do {                                                                                               \
    ncclResult_t r_ = (x);                                                                           \
    if (r_ != ncclSuccess) return fail(std::string(#x) + ": " + g_rccl.GetErrorString(r_));        \
  } while (0)

static void halo_release(ecwam_hip_ctx* c) {
  if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
  if (c->d_send_idx) (void)hipFree(c->d_send_idx);
  for (auto& q : c->slot) {
    if (q.buf) (void)hipFree(q.buf);
    if (q.ev_packed) (void)hipEventDestroy(q.ev_packed);
    if (q.ev_done) (void)hipEventDestroy(q.ev_done);
    q = ecwam_hip_ctx::HaloSlot();
  }
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  c->comm = nullptr; c->d_send_idx = nullptr; c->comm_stream = nullptr;
}

// the first fast_gk frequencies of rows [kijs, kijl) of FL1 -> the compact rows of ecwam_hip_set_fastwave_copy (the kernels that do not
// write them from their tile)
static void fastwave_copy(ecwam_hip_ctx* c, const void* fl1, int kijs, int kijl, hipStream_t s) {
  const size_t rb = (size_t)c->real_bytes;
  const char* src = (const char*)fl1 + (size_t)kijs * c->NANG * c->NFRE * rb;
  char* dst = (char*)c->fast_g + (size_t)kijs * c->NANG * c->fast_gk * rb;
  in_precision(c, [&](auto t) { launch_copy_freq_range<decltype(t)>(src, dst, kijl - kijs, c->NANG, c->NFRE, 0, c->fast_gk, c->fast_gk, s); });
}

// ---- one member of a FIELD_API-shaped host type <-> its slot of the library's packed per-point rows ---------------------------------
// chunked member M(NPROMA[,NM],NCHNK) (Fortran order: element (ip, m, ich) at ((ich NM + m) NPROMA + ip)) and rows[ij][row_stride]
// with the member's NM values at row_off; E = the element as an integer of its size (reals, doubles and int32 move alike)
template <typename E>
__global__ void k_member_scatter(const E* __restrict__ src, E* __restrict__ rows, int nproma, int npts, int nm, long long row_stride, long long row_off) {
  const long long total = (long long)npts * nm;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
    const int ij = (int)(g / nm), m = (int)(g - (long long)ij * nm);
    const int ich = ij / nproma, ip = ij - ich * nproma;
    rows[(long long)ij * row_stride + row_off + m] = src[((size_t)ich * nm + m) * nproma + ip];
  }
}
template <typename E>
__global__ void k_member_gather(const E* __restrict__ rows, E* __restrict__ dst, int nproma, int nchnk, int npts, int nm, long long row_stride, long long row_off) {
  const long long total = (long long)nchnk * nproma * nm;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
    const int ip = (int)(g % nproma);
    const long long r = g / nproma;
    const int m = (int)(r % nm), ich = (int)(r / nm);
    int ij = ich * nproma + ip;
    if (ij >= npts) ij = (nchnk - 1) * nproma;      // pad lanes of the ragged last chunk replicate its lane 1 (propag_wam.F90:388-398)
    dst[g] = rows[(long long)ij * row_stride + row_off + m];
  }
}

extern "C" {

const char* ecwam_hip_last_error(void) { return g_err.c_str(); }
int ecwam_hip_abi_version(void) { return ECWAM_HIP_ABI_VERSION; }

int ecwam_hip_selftest(int device) {
  HIPCHK(hipSetDevice(device));
  int* d = nullptr;
  int h[2] = {0, 0};
  HIPCHK(hipMalloc(&d, 2 * sizeof(int)));
  HIPCHK(hipMemset(d, 0, 2 * sizeof(int)));
  hipLaunchKernelGGL(k_selftest<float>, dim3(1), dim3(64), 0, 0, d);
  hipLaunchKernelGGL(k_selftest<double>, dim3(1), dim3(64), 0, 0, d + 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(h, d, 2 * sizeof(int), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  if (h[0] || h[1]) return fail("ecwam_hip_selftest: a wavefront primitive returned a wrong value");
  return 0;
}

int ecwam_hip_create(const ecwam_hip_params* p, const ecwam_hip_tables* t, int real_bytes, int device, ecwam_hip_ctx** out) {
  if (!p || !t || !out) return fail("ecwam_hip_create: null argument");
  if (real_bytes != 4 && real_bytes != 8) return fail("ecwam_hip_create: real_bytes must be 4 or 8");
  if (p->nang < 4 || p->nang > MAXA || p->nfre < 8 || p->nfre > MAXF || p->nfre_red < 1 || p->nfre_red > p->nfre)
    return fail("ecwam_hip_create: NANG/NFRE/NFRE_RED out of the supported range");
  if (p->mlsthg > MAXMC || 2 * p->nsdsnth + 1 > MAXTAP || p->nwav_gc + 1 > MAXGC) return fail("ecwam_hip_create: table size exceeds library limits");
  if ((p->iphys != 0 && p->iphys != 1) || (p->isnonlin < 0 || p->isnonlin > 2) || p->irefra < 0 || p->irefra > 3 || p->icode < 1 || p->icode > 3)
    return fail("ecwam_hip_create: only IPHYS=0/1, ISNONLIN=0/1/2, IREFRA=0..3, ICODE=1..3 are on the hot path (SURVEY.md 8a)");
  if (p->lciwa1 && (!t->cideac || p->nict < 2 || p->nich < 2 || p->nict * p->nich > 36 * 16))
    return fail("ecwam_hip_create: LCIWA1 (SDICE1) needs the CIDEAC table (tables.cideac, NICT*NICH <= 576)");
  {   // every table the kernels read must be there (the optional ones: cideac, checked above)
    const void* need[] = {t->fr, t->dfim, t->dfimofr, t->dfimfr, t->dfim_sim, t->rhowg_dfim, t->zpifr, t->fr5, t->cofrm4, t->flmax, t->th, t->costh,
                          t->sinth, t->wtauhf, t->swellft, t->ikp, t->ikp1, t->ikm, t->ikm1, t->af11, t->k1w, t->k2w, t->k11w, t->k21w, t->inlcoef,
                          t->rnlcoef, t->indicessat, t->satweights, t->kpm, t->jxo, t->jyo, t->kcr};
    for (const void* q : need) if (!q) return fail("ecwam_hip_create: a required table pointer is NULL");
    if (p->nwav_gc > 0 && (!t->xk_gc || !t->xkm_gc || !t->omega_gc || !t->omxkm3_gc || !t->cm_gc || !t->c2osqrtvg_gc || !t->xkmsqrtvgoc2_gc ||
                           !t->om3gmkm_gc || !t->delkcc_gc_ns || !t->delkcc_omxkm3_gc)) return fail("ecwam_hip_create: a gravity-capillary table pointer is NULL");
  }
  HIPCHK(hipSetDevice(device));
  ecwam_hip_ctx* c = new ecwam_hip_ctx();
  c->real_bytes = real_bytes; c->device = device; c->NANG = p->nang; c->NFRE = p->nfre; c->NFRE_RED = p->nfre_red; c->p = *p;
  c->fr_host.assign((const unsigned char*)t->fr, (const unsigned char*)t->fr + (size_t)p->nfre * real_bytes);
#define HIPCHK_CTX(x)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) { if (c->dtab) (void)hipFree(c->dtab); if (c->itab) (void)hipFree(c->itab); delete c; return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } \
  } while (0)
  const int rc_tab = in_precision(c, [&](auto prec) {
    using T = decltype(prec);
    std::vector<DevTab<T>> h(1);
    build_tab<T>(p, t, h.data());
    if (!h[0].DIA_PULL) { delete c; return fail("ecwam_hip_create: the interaction tables do not have the rotation structure of INISNONLIN (K1W = K -+ r1, K2W = K +- r2, INLCOEF = MC, MC+2, MC+3, MC-4, MC-3; KFRH = 8, MFRSTLW = -3): not supported"); }
    v4_probe<T>(h[0], c);
    HIPCHK_CTX(hipMalloc(&c->dtab, sizeof(DevTab<T>)));
    HIPCHK_CTX(hipMemcpy(c->dtab, h.data(), sizeof(DevTab<T>), hipMemcpyHostToDevice));
    return 0;
  });
  if (rc_tab) return rc_tab;
  if (p->irefra >= 2) {   // INTPOL (ecwam_hip_outbs_absolute): FREQ, DFREQTH, deep-water WAVN and the f**-5 factor of M = 1 .. NFRE_MAX
    std::vector<unsigned char> h;
    const size_t nb = intpol_tab_build(p, t, real_bytes, h);
    if (nb) {               // (NFRE_MAX beyond the table: ecwam_hip_outbs_absolute refuses, everything else is served)
      HIPCHK_CTX(hipMalloc(&c->itab, nb));
      HIPCHK_CTX(hipMemcpy(c->itab, h.data(), nb, hipMemcpyHostToDevice));
    }
  }
#undef HIPCHK_CTX
  // IMPLSCH runs k_implsch4 (implsch_v4.h) and nothing else since round 5: refuse here what its builds do not cover, with the reason
  {
    const char* why = nullptr;
    const bool inst = v4_for_shape(c->NANG, c->v4_r1, c->v4_r2, c->v4_nh, [](auto) { return 0; }) == 0;      // (implsch_v4_shapes.h)
    if (p->nfre != 36) why = "NFRE must be 36 (the frequency grid of every configuration of the reference)";
    else if (!c->v4_ok) why = "the saturation weights / indices do not have the structure of INIT_SDISS_ARDH (COS**2 taps, symmetric, the same for every direction) or the DIA mirror images differ";
    else if (!inst) why = "NANG must be 48, 36, 24 or 12 with the interaction rotations and the saturation half-width of INISNONLIN / INIT_SDISS_ARDH on that grid";
    else if (p->iphys == 1 && p->llnormagam && c->v4_shelter) why = "LLNORMAGAM needs TAUWSHELTER = 0 (setwavphys.F90:150-190: the normalised growth rate replaces the sheltering)";
    else if (p->iphys == 1 && !p->llnormagam && !c->v4_shelter) why = "IPHYS = 1 without LLNORMAGAM needs TAUWSHELTER /= 0 (setwavphys.F90:150-190)";
    // (the context is created all the same: advection, OUTBS, halo exchange and restart do not depend on IMPLSCH's builds, and the reference
    // accepts any NANG -- ecwam_hip_implsch / ecwam_hip_propags2_implsch then refuse with this reason)
    if (why) c->implsch_why = std::string("configuration not covered by the IMPLSCH kernel: ") + why;
  }
  *out = c;
  return 0;
}

int ecwam_hip_destroy(ecwam_hip_ctx* c) {
  if (!c) return 0;
  if (c->dtab) (void)hipFree(c->dtab);
  if (c->norm_scratch) (void)hipFree(c->norm_scratch);
  if (c->itab) (void)hipFree(c->itab);
  if (c->so_tab) (void)hipFree(c->so_tab);
  if (c->so_coef) (void)hipFree(c->so_coef);
  if (c->so_work) (void)hipFree(c->so_work);
  if (c->int_tab) (void)hipFree(c->int_tab);
  if (c->ob_desc) (void)hipFree(c->ob_desc);
  if (c->ob_work) (void)hipFree(c->ob_work);
  if (c->fin) (void)hipFree(c->fin);
  if (c->wi) (void)hipFree(c->wi);
  if (c->adv_pt) (void)hipFree(c->adv_pt);
  if (c->adv_dir) (void)hipFree(c->adv_dir);
  if (c->fmap_in) (void)hipFree(c->fmap_in);
  if (c->fmap_out) (void)hipFree(c->fmap_out);
  if (c->fli_idx) (void)hipFree(c->fli_idx);
  if (c->fli_w) (void)hipFree(c->fli_w);
  for (auto& g : c->g2w) {
    if (g.pos) (void)hipFree(g.pos);
    if (g.w) (void)hipFree(g.w);
  }
  if (c->rmap_inv) (void)hipFree(c->rmap_inv);
  grib_map_free(c);
  halo_release(c);
  delete c;
  return 0;
}

int ecwam_hip_set_obstructions(ecwam_hip_ctx* c, const void* obs, int n) {
  if (!c) return fail("null context");
  if (n < 0 || (obs && n == 0)) return fail("ecwam_hip_set_obstructions: bad size");
  c->obs = obs; c->n_obs = obs ? n : 0;
  return 0;
}

int ecwam_hip_propags2(ecwam_hip_ctx* c, const void* f1, void* f3, const int* klon, const int* klat, const int* kcor, const void* w,
                       int kijs, int kijl, int nd3s, int nd3e, int copy_rest, void* stream) {
  if (!c) return fail("null context");
  if (kijl < kijs || nd3s < 1 || nd3e > c->NFRE_RED || nd3e < nd3s - 1) return fail("ecwam_hip_propags2: bad range");
  if (kijl > kijs && (!f1 || !f3 || !klon || !klat || !kcor || !w)) return fail("ecwam_hip_propags2: null pointer");
  if (f1 == f3) return fail("ecwam_hip_propags2: F1 and F3 must not alias");
  const int N = (c->NANG << 16) | (c->NFRE << 8) | c->NFRE_RED;
  in_precision(c, [&](auto t) { launch_propags2<decltype(t)>(c->dtab, f1, f3, klon, klat, kcor, w, kijs, kijl, nd3s - 1, nd3e, copy_rest, N, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_ctuw(ecwam_hip_ctx* c, int n, int nland, int ngy, double delpro, int mstart, int mend, const int* kxlt, const void* zdello,
                   double xdella, const void* cosph, const void* sinph, const int* klon, const int* klat, const int* kcor, void* wlat,
                   void* wcor, const void* cgroup_ext, const void* cosphm1_ext, void* w, int* cflfail, void* stream) {
  if (!c) return fail("null context");
  if (n < 0 || mstart < 1 || mend > c->NFRE_RED || mend < mstart) return fail("ecwam_hip_ctuw: bad range");
  if (n > 0 && (!kxlt || !zdello || !cosph || !sinph || !klon || !klat || !kcor || !wlat || !wcor || !cgroup_ext || !cosphm1_ext || !cflfail))
    return fail("ecwam_hip_ctuw: null pointer");
  if (c->obs && n > c->n_obs) return fail("ecwam_hip_ctuw: more points than the obstruction table holds");
  const AdvGeom g{kxlt, zdello, xdella, cosph, sinph, klon, klat, kcor, wlat, wcor, cgroup_ext, cosphm1_ext, ngy};
  in_precision(c, [&](auto t) { launch_ctuw<decltype(t)>(c->dtab, n, nland, delpro, mstart - 1, mend, g, w, cflfail, c->NANG, c->obs, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_propags2_otf_split(ecwam_hip_ctx* c, const void* f1, void* f3, int n, int ngy, double delpro, double delpro_lf, int ifrelfmax,
                                 int in_nfre, void* gout, int gout_nfre, const int* kxlt, const void* zdello, double xdella, const void* cosph, const void* sinph, const int* klon,
                                 const int* klat, const int* kcor, const void* wlat, const void* wcor, const void* cgroup_ext,
                                 const void* cosphm1_ext, const int* order, int kijs, int kijl, int nd3s, int nd3e, int copy_rest,
                                 void* stream) {
  return ecwam_hip_propags2_otf_fast(c, f1, f3, n, ngy, delpro, delpro_lf, ifrelfmax, in_nfre, nullptr, 0, 0, gout, gout_nfre, kxlt, zdello, xdella, cosph,
                                     sinph, klon, klat, kcor, wlat, wcor, cgroup_ext, cosphm1_ext, order, kijs, kijl, nd3s, nd3e, copy_rest, stream);
}

int ecwam_hip_propags2_otf_fast(ecwam_hip_ctx* c, const void* f1, void* f3, int n, int ngy, double delpro, double delpro_lf, int ifrelfmax,
                                int in_nfre, const void* gin, int gin_nfre, int out_nfre, void* gout, int gout_nfre, const int* kxlt,
                                const void* zdello, double xdella, const void* cosph, const void* sinph, const int* klon, const int* klat,
                                const int* kcor, const void* wlat, const void* wcor, const void* cgroup_ext, const void* cosphm1_ext,
                                const int* order, int kijs, int kijl, int nd3s, int nd3e, int copy_rest, void* stream) {
  if (!c) return fail("null context");
  if (out_nfre == 0) out_nfre = c->NFRE;
  if (out_nfre != c->NFRE && (out_nfre < nd3e || out_nfre > c->NFRE || gout))
    return fail("ecwam_hip_propags2_otf_fast: a compact output buffer must hold every advected frequency and excludes a second compact copy");
  if (gin && (in_nfre != 0 && in_nfre != c->NFRE)) return fail("ecwam_hip_propags2_otf_fast: the compact fast-wave input goes with full input rows");
  if (gin && (gin_nfre < 1 || gin_nfre > c->NFRE || gin == f3 || gin == gout)) return fail("ecwam_hip_propags2_otf_fast: bad compact input buffer");
  {
    // every compact row format is read and written with 16-byte accesses along the frequencies
    const int vec = 16 / c->real_bytes;
    if ((gin && (gin_nfre % vec != 0 || ((uintptr_t)gin % 16) != 0)) || (out_nfre != c->NFRE && (out_nfre % vec != 0 || ((uintptr_t)f3 % 16) != 0)) ||
        (in_nfre != 0 && in_nfre != c->NFRE && (in_nfre % vec != 0 || ((uintptr_t)f1 % 16) != 0)))
      return fail("ecwam_hip_propags2_otf_fast: compact rows must be 16-byte aligned and hold a multiple of 16 bytes per direction");
  }
  // with a processing order kijs..kijl index its entries (entries < 0 are padding and skipped: the order may be longer than n)
  if (kijl < kijs || kijs < 0 || (!order && kijl > n) || nd3s < 1 || nd3e > c->NFRE_RED || nd3e < nd3s - 1 || ifrelfmax < 0 || ifrelfmax > c->NFRE_RED)
    return fail("ecwam_hip_propags2_otf: bad range");
  if ((copy_rest & 4) && !order) return fail("ecwam_hip_propags2_otf: 2-D tiles need a processing order");
  if (in_nfre == 0) in_nfre = c->NFRE;
  if (gout && (gout_nfre < 1 || gout_nfre > c->NFRE || gout_nfre % (16 / c->real_bytes) != 0 || gout == f1 || ((uintptr_t)gout % 16) != 0))
    return fail("ecwam_hip_propags2_otf: the compact output buffer must be 16-byte aligned, distinct from F1, and hold a multiple of 16 bytes per direction");
  if (in_nfre != c->NFRE && (in_nfre < nd3e || in_nfre > c->NFRE || ((copy_rest & 1) && out_nfre != in_nfre)))
    return fail("ecwam_hip_propags2_otf: a compact input buffer must hold every advected frequency; copy_rest only into a compact output of the same width");
  if (kijl > kijs && (!f1 || !f3 || !kxlt || !zdello || !cosph || !sinph || !klon || !klat || !kcor || !wlat || !wcor || !cgroup_ext || !cosphm1_ext))
    return fail("ecwam_hip_propags2_otf: null pointer");
  if (f1 == f3) return fail("ecwam_hip_propags2_otf: F1 and F3 must not alias");
  if (c->obs && (order ? n : kijl) > c->n_obs) return fail("ecwam_hip_propags2_otf: more points than the obstruction table holds");
  hipStream_t s = (hipStream_t)stream;
  const int N = (c->NANG << 16) | (c->NFRE << 8) | c->NFRE_RED;
  copy_rest = (copy_rest & 1) | (copy_rest & 4);   // bit 0: carry the other frequencies over; bit 2: the order describes 2-D tiles
#ifdef ECWAM_HIP_DIAGNOSTICS
  { const char* e_ = getenv("ECWAM_HIP_OTF_WALK"); if (e_ && atoi(e_) == 0) copy_rest |= 2; }  // plain grid-stride tile walk
#endif
  const AdvGeom g{kxlt, zdello, xdella, cosph, sinph, klon, klat, kcor, wlat, wcor, cgroup_ext, cosphm1_ext, ngy};
  in_precision(c, [&](auto t) {
    launch_propags2_otf<decltype(t)>(c->dtab, f1, f3, n, delpro, g, order, kijs, kijl, nd3s - 1, nd3e, copy_rest, N, c->obs, ifrelfmax, delpro_lf, in_nfre, gout,
                                     gout_nfre, gin, gin_nfre, out_nfre, s);
  });
  return launched();
}

int ecwam_hip_propags2_otf(ecwam_hip_ctx* c, const void* f1, void* f3, int n, int ngy, double delpro, const int* kxlt, const void* zdello,
                           double xdella, const void* cosph, const void* sinph, const int* klon, const int* klat, const int* kcor,
                           const void* wlat, const void* wcor, const void* cgroup_ext, const void* cosphm1_ext, const int* order,
                           int kijs, int kijl, int nd3s, int nd3e, int copy_rest, void* stream) {
  return ecwam_hip_propags2_otf_split(c, f1, f3, n, ngy, delpro, delpro, 0, 0, nullptr, 0, kxlt, zdello, xdella, cosph, sinph, klon, klat, kcor, wlat, wcor,
                                      cgroup_ext, cosphm1_ext, order, kijs, kijl, nd3s, nd3e, copy_rest, stream);
}

int ecwam_hip_copy_freq_range(ecwam_hip_ctx* c, const void* src, void* dst, int n, int m_first, int m_last, int dst_nfre, void* stream) {
  if (!c) return fail("null context");
  if (dst_nfre == 0) dst_nfre = c->NFRE;
  if (n < 0 || m_first < 1 || m_last > c->NFRE || m_last < m_first - 1 || m_last > dst_nfre) return fail("ecwam_hip_copy_freq_range: bad range");
  if (n > 0 && (!src || !dst)) return fail("ecwam_hip_copy_freq_range: null pointer");
  in_precision(c, [&](auto t) { launch_copy_freq_range<decltype(t)>(src, dst, n, c->NANG, c->NFRE, m_first - 1, m_last, dst_nfre, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_propdot(ecwam_hip_ctx* c, int n, int nland, const int* kxlt, const void* zdello, double xdella, const void* cosph,
                      const int* klon, const int* klat, const void* wlat, const void* cosphm1_ext, const void* depth_ext,
                      const void* u_ext, const void* v_ext, void* refr, void* stream) {
  if (!c) return fail("null context");
  if (n < 0) return fail("ecwam_hip_propdot: bad range");
  if (n > 0 && (!kxlt || !zdello || !cosph || !klon || !klat || !wlat || !cosphm1_ext || !depth_ext || !u_ext || !v_ext || !refr))
    return fail("ecwam_hip_propdot: null pointer");
  const AdvGeom g{kxlt, zdello, xdella, cosph, nullptr, klon, klat, nullptr, wlat, nullptr, nullptr, cosphm1_ext, 0};      // (what k_propdot reads)
  in_precision(c, [&](auto t) { launch_propdot<decltype(t)>(c->dtab, n, nland, c->p.irefra, g, depth_ext, u_ext, v_ext, refr, (hipStream_t)stream); });
  return launched();
}

// shared argument checks + launch of the general-IREFRA kernel (f1 == NULL: checks only)
static int propags2_gen_launch(ecwam_hip_ctx* c, const char* who, const void* f1, void* f3, double delpro, const AdvGeom& g, const void* omosnh2kd_ext,
                               const void* wavnum_ext, const void* refr, int* cflfail, int slot, int kijs, int kijl, int m0, int m1, int copy_rest,
                               hipStream_t s) {
  if (kijl > kijs && (!g.kxlt || !g.zdello || !g.cosph || !g.sinph || !g.klon || !g.klat || !g.kcor || !g.wlat || !g.wcor || !g.cgroup_ext ||
                      !omosnh2kd_ext || !wavnum_ext || !g.cosphm1_ext || !refr))
    return fail((std::string(who) + ": null pointer").c_str());
  const int N = (c->NANG << 16) | (c->NFRE << 8) | c->NFRE_RED;
  in_precision(c, [&](auto t) { launch_propags2_gen<decltype(t)>(c->dtab, c->p.irefra, f1, f3, delpro, g, omosnh2kd_ext, wavnum_ext, refr, cflfail, slot, kijs, kijl, m0, m1, copy_rest, N, c->obs, s); });
  return launched();
}

int ecwam_hip_ctuw_refra(ecwam_hip_ctx* c, int n, int nland, int ngy, double delpro, int mstart, int mend, const int* kxlt,
                         const void* zdello, double xdella, const void* cosph, const void* sinph, const int* klon, const int* klat,
                         const int* kcor, void* wlat, void* wcor, const void* cgroup_ext, const void* omosnh2kd_ext,
                         const void* wavnum_ext, const void* cosphm1_ext, void* refr, int llcflcuroff, int range, int* cflfail,
                         void* stream) {
  if (!c) return fail("null context");
  if (n < 0 || mstart < 1 || mend > c->NFRE_RED || mend < mstart || range < 0 || range > 1) return fail("ecwam_hip_ctuw_refra: bad range");
  if (n > 0 && (!wlat || !wcor || !cflfail || !klat || !kcor || !refr)) return fail("ecwam_hip_ctuw_refra: null pointer");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  // CTUWINI (ctuwupdt.F90:204-214; idempotent), then CTUWDRV for this frequency range (ctuwdrv.F90:93-118)
  in_precision(c, [&](auto t) { launch_ctuwini_only<decltype(t)>(n, nland, klat, kcor, wlat, wcor, s); });
  const bool cur = c->p.irefra == 2 || c->p.irefra == 3;
  std::vector<int> prev;  // flags of the first range survive the second range's own CTUWDRV
  if (range == 1) {
    prev.resize((size_t)n);
    HIPCHK(hipMemcpyAsync(prev.data(), cflfail, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  HIPCHK(hipMemsetAsync(cflfail, 0, sizeof(int) * (size_t)n, s));
  in_precision(c, [&](auto t) { launch_curmask<decltype(t)>(n, c->NANG, range, nullptr, refr, s); });  // CURMASK = 1
  const AdvGeom g{kxlt, zdello, xdella, cosph, sinph, klon, klat, kcor, wlat, wcor, cgroup_ext, cosphm1_ext, ngy};
  int rc = propags2_gen_launch(c, "ecwam_hip_ctuw_refra", nullptr, nullptr, delpro, g, omosnh2kd_ext, wavnum_ext, refr, cflfail, range, 0, n, mstart - 1, mend, 0, s);
  if (rc) return rc;
  if (cur && llcflcuroff) {
    // second CTUW call: current refraction / frequency shift switched off where the first one failed, flags reset
    std::vector<int> h((size_t)n);
    HIPCHK(hipMemcpyAsync(h.data(), cflfail, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    bool any = false;
    for (int i = 0; i < n && !any; i++) any = h[i] != 0;
    if (any) {
      in_precision(c, [&](auto t) { launch_curmask<decltype(t)>(n, c->NANG, range, cflfail, refr, s); });
      HIPCHK(hipMemsetAsync(cflfail, 0, sizeof(int) * (size_t)n, s));
      rc = propags2_gen_launch(c, "ecwam_hip_ctuw_refra", nullptr, nullptr, delpro, g, omosnh2kd_ext, wavnum_ext, refr, cflfail, range, 0, n, mstart - 1, mend, 0, s);
      if (rc) return rc;
    }
  }
  if (range == 1) {
    std::vector<int> h((size_t)n);
    HIPCHK(hipMemcpyAsync(h.data(), cflfail, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < n; i++) h[i] |= prev[i];
    HIPCHK(hipMemcpyAsync(cflfail, h.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return 0;
}

int ecwam_hip_propags2_refra(ecwam_hip_ctx* c, const void* f1, void* f3, int n, int ngy, double delpro, const int* kxlt,
                             const void* zdello, double xdella, const void* cosph, const void* sinph, const int* klon,
                             const int* klat, const int* kcor, const void* wlat, const void* wcor, const void* cgroup_ext,
                             const void* omosnh2kd_ext, const void* wavnum_ext, const void* cosphm1_ext, const void* refr, int range,
                             int kijs, int kijl, int nd3s, int nd3e, int copy_rest, void* stream) {
  if (!c) return fail("null context");
  if (kijl < kijs || kijs < 0 || kijl > n || nd3s < 1 || nd3e > c->NFRE_RED || nd3e < nd3s - 1 || range < 0 || range > 1)
    return fail("ecwam_hip_propags2_refra: bad range");
  if (kijl > kijs && (!f1 || !f3)) return fail("ecwam_hip_propags2_refra: null pointer");
  if (f1 == f3) return fail("ecwam_hip_propags2_refra: F1 and F3 must not alias");
  if (c->obs && kijl > c->n_obs) return fail("ecwam_hip_propags2_refra: more points than the obstruction table holds");
  const AdvGeom g{kxlt, zdello, xdella, cosph, sinph, klon, klat, kcor, wlat, wcor, cgroup_ext, cosphm1_ext, ngy};
  return propags2_gen_launch(c, "ecwam_hip_propags2_refra", f1, f3, delpro, g, omosnh2kd_ext, wavnum_ext, refr, nullptr, range, kijs, kijl, nd3s - 1, nd3e,
                             copy_rest ? 1 : 0, (hipStream_t)stream);
}

// ---- IPROPAGS = 0: the first-order scheme (include/ecwam_hip_propags.h; csrc/propags.hip) ----------------------------------------------------------
int ecwam_hip_propags_dot(ecwam_hip_ctx* c, int n, int nland, int icase, const int* kxlt, const void* zdello, double xdella, const void* cosph, const int* klon,
                          const int* klat, const void* wlat, const void* cosphm1_ext, const void* depth_ext, const void* u_ext, const void* v_ext, void* dot,
                          void* stream) {
  if (!c) return fail("null context");
  if (icase != 1 && icase != 2) return fail("ecwam_hip_propags_dot: ICASE must be 1 (spherical) or 2 (Cartesian)");
  if (n < 0 || nland < n) return fail("ecwam_hip_propags_dot: bad range");
  if (n > 0 && (!kxlt || !zdello || !cosph || !klon || !klat || !wlat || (icase == 1 && !cosphm1_ext) || !depth_ext || !u_ext || !v_ext || !dot))
    return fail("ecwam_hip_propags_dot: null pointer");
  if ((uintptr_t)dot % 16) return fail("ecwam_hip_propags_dot: dot must be 16-byte aligned");
  const AdvGeom g{kxlt, zdello, xdella, cosph, nullptr, klon, klat, nullptr, wlat, nullptr, nullptr, cosphm1_ext, 0};
  in_precision(c, [&](auto t) { launch_propags_dot<decltype(t)>(c->dtab, n, nland, c->p.irefra, icase, g, depth_ext, u_ext, v_ext, dot, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_propags(ecwam_hip_ctx* c, const void* f1, void* f3, int n, int nland, int ngy, double delpro, double delphi, int flags, const int* kxlt,
                      const void* cosph, const void* sinph, const void* dellam1_ext, const void* cosphm1_ext, const int* klon, const int* klat, const void* wlat,
                      const void* cgroup_ext, const void* omosnh2kd_ext, const void* wavnum_ext, const void* u_ext, const void* v_ext, const void* dot, int kijs,
                      int kijl, int copy_rest, void* cfl, int* cflfail, void* stream) {
  if (!c) return fail("null context");
  if (flags & ~(ECWAM_HIP_PROPAGS_CARTESIAN | ECWAM_HIP_PROPAGS_IRREGULAR)) return fail("ecwam_hip_propags: unknown flag bits");
  if (!(delpro == std::floor(delpro)) || delpro < 0) return fail("ecwam_hip_propags: delpro must be a whole number of seconds (DELPRO = REAL(IDELPRO))");
  if (!(delphi > 0)) return fail("ecwam_hip_propags: delphi must be positive");
  const int vec = 16 / c->real_bytes;
  if (c->NFRE % vec != 0) return fail("ecwam_hip_propags: NFRE is no whole number of 16-byte pieces");
  if (kijs < 0 || kijl < kijs || kijl > n || nland < n) return fail("ecwam_hip_propags: bad range");
  if (kijl == kijs) return 0;
  const bool cart = flags & ECWAM_HIP_PROPAGS_CARTESIAN;
  const int irefra = c->p.irefra;
  const bool cur = irefra == 2 || irefra == 3;
  if (!f1 || !dellam1_ext || !klon || !klat || !cgroup_ext || (!cart && (!kxlt || !cosph || !sinph || !cosphm1_ext || !wlat)))
    return fail("ecwam_hip_propags: null pointer");
  if (irefra != 0 && !dot) return fail("ecwam_hip_propags: IREFRA /= 0 needs the dot terms of ecwam_hip_propags_dot (dot is NULL)");
  if (irefra != 0 && !omosnh2kd_ext) return fail("ecwam_hip_propags: IREFRA /= 0 needs OMOSNH2KD_EXT");
  if (cur && (!wavnum_ext || !u_ext || !v_ext)) return fail("ecwam_hip_propags: IREFRA 2, 3 need WAVNUM_EXT, U_EXT and V_EXT");
  if (!f3 && (cart || (!cfl && !cflfail))) return fail("ecwam_hip_propags: nothing to do (f3 is NULL and the call has no check to make)");
  if (f1 == f3) return fail("ecwam_hip_propags: F1 and F3 must not alias");
  if ((uintptr_t)f1 % 16 || (uintptr_t)f3 % 16 || (uintptr_t)cgroup_ext % 16 || (uintptr_t)omosnh2kd_ext % 16 || (uintptr_t)wavnum_ext % 16 || (uintptr_t)dot % 16)
    return fail("ecwam_hip_propags: f1, f3, the rows of frequencies and dot must be 16-byte aligned");
  if ((uintptr_t)cfl % c->real_bytes || (uintptr_t)cflfail % sizeof(int)) return fail("ecwam_hip_propags: cfl or cflfail misaligned");
  if (c->obs && !cart && kijl > c->n_obs) return fail("ecwam_hip_propags: more points than the obstruction table holds");
  PropagsCall a{f1, f3, nland, cart ? 2 : 1, (flags & ECWAM_HIP_PROPAGS_IRREGULAR) ? 1 : 0, irefra, delpro, delphi, kxlt, cosph, sinph, dellam1_ext, cosphm1_ext,
                klon, klat, wlat, cgroup_ext, omosnh2kd_ext, wavnum_ext, u_ext, v_ext, irefra != 0 ? dot : nullptr, cart ? nullptr : c->obs, kijs, kijl,
                copy_rest ? 1 : 0, cfl, cflfail};
  (void)ngy;
  const int rc = in_precision(c, [&](auto t) { return launch_propags<decltype(t)>(c->dtab, a, c->NFRE, (hipStream_t)stream); });
  if (rc) return fail("ecwam_hip_propags: the tile of this NANG x NFRE does not fit the LDS (no build serves the configuration)");
  return launched();
}

// ---- IPROPAGS = 1: the dual rotated-quadrant scheme (include/ecwam_hipx_propags1.h; csrc/propags1.hip, and csrc/propags.hip for sections 1, 2, 4) ----------
int ecwam_hipx_set_rotated(ecwam_hip_ctx* c, int n, int nrow, const int* krlat, const int* krlon, const void* wrlat, const void* wrlon, const void* cdr,
                           const void* sdr, const void* prqrt, double sqrt2) {
  if (!c) return fail("null context");
  const int given = (krlat != nullptr) + (krlon != nullptr) + (wrlat != nullptr) + (wrlon != nullptr) + (cdr != nullptr) + (sdr != nullptr) + (prqrt != nullptr);
  if (given == 0) {
    c->rot = RotatedTables{};
    return 0;
  }
  if (given != 7) return fail("ecwam_hipx_set_rotated: some tables are NULL and others are not");
  if (n < 0 || nrow <= n) return fail("ecwam_hipx_set_rotated: bad size (nrow <= n: CDR and SDR cover the rows of the neighbours too)");
  if (!(sqrt2 > 0)) return fail("ecwam_hipx_set_rotated: sqrt2 must be positive");
  if ((uintptr_t)krlat % sizeof(int) || (uintptr_t)krlon % sizeof(int) || (uintptr_t)wrlat % c->real_bytes || (uintptr_t)wrlon % c->real_bytes ||
      (uintptr_t)cdr % c->real_bytes || (uintptr_t)sdr % c->real_bytes || (uintptr_t)prqrt % c->real_bytes)
    return fail("ecwam_hipx_set_rotated: a table is misaligned");
  c->rot.n = n; c->rot.nrow = nrow;
  c->rot.krlat = krlat; c->rot.krlon = krlon;
  c->rot.wrlat = wrlat; c->rot.wrlon = wrlon; c->rot.cdr = cdr; c->rot.sdr = sdr; c->rot.prqrt = prqrt;
  c->rot.sqrt2 = sqrt2;
  return 0;
}

int ecwam_hipx_propags1(ecwam_hip_ctx* c, const void* f1, void* f3, int n, int nland, int ngy, double delpro, double delphi, int flags, const int* kxlt,
                        const void* cosph, const void* sinph, const void* dellam1_ext, const void* cosphm1_ext, const int* klon, const int* klat, const void* wlat,
                        const void* cgroup_ext, const void* omosnh2kd_ext, const void* wavnum_ext, const void* u_ext, const void* v_ext, const void* dot, int kijs,
                        int kijl, int copy_rest, void* cfl, int* cflfail, void* stream) {
  if (!c) return fail("null context");
  if (flags & ~(ECWAM_HIPX_PROPAGS1_CARTESIAN | ECWAM_HIPX_PROPAGS1_IRREGULAR)) return fail("ecwam_hipx_propags1: unknown flag bits");
  if (!(delpro == std::floor(delpro)) || delpro < 0) return fail("ecwam_hipx_propags1: delpro must be a whole number of seconds (DELPRO = REAL(IDELPRO))");
  if (!(delphi > 0)) return fail("ecwam_hipx_propags1: delphi must be positive");
  const int vec = 16 / c->real_bytes;
  if (c->NFRE % vec != 0) return fail("ecwam_hipx_propags1: NFRE is no whole number of 16-byte pieces");
  if (kijs < 0 || kijl < kijs || kijl > n || nland < n) return fail("ecwam_hipx_propags1: bad range");
  const bool cart = flags & ECWAM_HIPX_PROPAGS1_CARTESIAN;
  const int irefra = c->p.irefra;
  const bool cur = irefra == 2 || irefra == 3;
  const bool rotated = !cart && !cur;      // section 3
  if (rotated && !c->rot.krlat) return fail("ecwam_hipx_propags1: a spherical grid with IREFRA 0 or 1 needs the rotated tables (ecwam_hipx_set_rotated)");
  if (rotated && (kijl > c->rot.n || nland > c->rot.nrow))
    return fail("ecwam_hipx_propags1: the rotated tables hold fewer points or rows than the call reads");
  if (kijl == kijs) return 0;
  if (!f1 || !dellam1_ext || !klon || !klat || !cgroup_ext || (!cart && (!kxlt || !cosph || !sinph || !cosphm1_ext || !wlat)))
    return fail("ecwam_hipx_propags1: null pointer");
  if (irefra != 0 && !dot) return fail("ecwam_hipx_propags1: IREFRA /= 0 needs the dot terms of the first-order scheme's dot call (dot is NULL)");
  if (irefra != 0 && !omosnh2kd_ext) return fail("ecwam_hipx_propags1: IREFRA /= 0 needs OMOSNH2KD_EXT");
  if (cur && (!wavnum_ext || !u_ext || !v_ext)) return fail("ecwam_hipx_propags1: IREFRA 2, 3 need WAVNUM_EXT, U_EXT and V_EXT");
  if (!f3 && (cart || (!cfl && !cflfail))) return fail("ecwam_hipx_propags1: nothing to do (f3 is NULL and the call has no check to make)");
  if (f1 == f3) return fail("ecwam_hipx_propags1: F1 and F3 must not alias");
  if ((uintptr_t)f1 % 16 || (uintptr_t)f3 % 16 || (uintptr_t)cgroup_ext % 16 || (uintptr_t)omosnh2kd_ext % 16 || (uintptr_t)wavnum_ext % 16 || (uintptr_t)dot % 16)
    return fail("ecwam_hipx_propags1: f1, f3, the rows of frequencies and dot must be 16-byte aligned");
  if ((uintptr_t)cfl % c->real_bytes || (uintptr_t)cflfail % sizeof(int)) return fail("ecwam_hipx_propags1: cfl or cflfail misaligned");
  if (c->obs && !cart && kijl > c->n_obs) return fail("ecwam_hipx_propags1: more points than the obstruction table holds");
  PropagsCall a{f1, f3, nland, cart ? 2 : 1, (flags & ECWAM_HIPX_PROPAGS1_IRREGULAR) ? 1 : 0, irefra, delpro, delphi, kxlt, cosph, sinph, dellam1_ext, cosphm1_ext,
                klon, klat, wlat, cgroup_ext, omosnh2kd_ext, wavnum_ext, u_ext, v_ext, irefra != 0 ? dot : nullptr, cart ? nullptr : c->obs, kijs, kijl,
                copy_rest ? 1 : 0, cfl, cflfail, 1};
  (void)ngy;
  const int rc = in_precision(c, [&](auto t) {
    return rotated ? launch_propags1<decltype(t)>(c->dtab, a, c->rot, c->NANG, c->NFRE, (hipStream_t)stream)
                   : launch_propags<decltype(t)>(c->dtab, a, c->NFRE, (hipStream_t)stream);
  });
  if (rc) return fail("ecwam_hipx_propags1: the tile of this NANG x NFRE does not fit the LDS (no build serves the configuration)");
  return launched();
}

// The variant of k_implsch4 (implsch_v4.h; launch.h: Implsch4Variant) a context runs.  The common builds (implsch4.hip): flag sets A and B
// (LLGCBZ0, LLNORMAGAM), with or without the sea-ice damping rates that depend on the frequency only (LCIWA1, LCIWA3, LCISCAL).  The alternate
// builds (implsch4x.hip), on flag set A only: IPHYS 0 (sinput_jan + sdissip_jan; its TAUWSHELTER is 0), ISNONLIN 1 (TRANSF per interaction
// frequency) -- what the reference's registered configurations select.  Everything else runs the RARE builds (implsch4r.hip: LCIWA2, the NEMO
// ice stress and strain, ISNONLIN 2, ICODE 1 / 2, LWVFLX_SNL = F, ISNONLIN 1 beside flag set B or IPHYS 0, IPHYS 0 beside flag set B).
// ecwam_hip_create has refused what no build covers.
static Implsch4Variant implsch4_variant(const ecwam_hip_ctx* c) {
  const bool ext = c->p.llnormagam || c->p.llgcbz0, jan = c->p.iphys == 0, enhmc = c->p.isnonlin == 1;
  const bool rare4 = c->p.lciwa2 || c->p.lwnemocouwrs || c->p.lwnemocoustrn || c->p.isnonlin > 1 || c->p.icode != 3 || !c->p.lwvflx_snl;
  if (rare4 || ((jan || enhmc) && (ext || (jan && enhmc)))) return jan ? Implsch4Variant::rare_iphys0 : Implsch4Variant::rare;
  return jan ? Implsch4Variant::iphys0 : enhmc ? Implsch4Variant::isnonlin1 : ext ? Implsch4Variant::B : Implsch4Variant::A;
}
static bool implsch4_rare(const ecwam_hip_ctx* c) {
  const Implsch4Variant v = implsch4_variant(c);
  return v == Implsch4Variant::rare || v == Implsch4Variant::rare_iphys0;
}
// the configurations the one-kernel step covers (implsch4a.hip: the common builds on IPHYS 1, ISNONLIN 0); everything else runs
// ecwam_hip_propags2_otf + ecwam_hip_implsch
static bool fused_ok(const ecwam_hip_ctx* c) {
  const Implsch4Variant v = implsch4_variant(c);
  return c->implsch_why.empty() && (v == Implsch4Variant::A || v == Implsch4Variant::B) && c->NFRE == 36;      // (the direction count: one of k_implsch4's, checked at create)
}
// The tables the one-kernel step takes its CTU scalars from (k_ctu_prep fills them every call): sized with the fin rows, so that a host that
// called ecwam_hip_implsch_reserve has no allocation in its time loop on this path either.  Contexts without a one-kernel build hold none.
static int adv_reserve(ecwam_hip_ctx* c, int npts) {
  if (!fused_ok(c) || !implsch4_adv_forms(c->NANG, c->real_bytes)) return 0;
  const size_t need = (size_t)(npts > 0 ? npts : 0) * 12 * c->real_bytes;
  if (need > c->adv_pt_bytes) {   // hipFree waits for the kernels still reading the old table
    if (c->adv_pt) HIPCHK(hipFree(c->adv_pt));
    c->adv_pt = nullptr; c->adv_pt_bytes = 0;
    HIPCHK(hipMalloc(&c->adv_pt, need));
    c->adv_pt_bytes = need;
  }
  if (!c->adv_dir) HIPCHK(hipMalloc(&c->adv_dir, (size_t)(6 * c->NANG + 4) * c->real_bytes + (size_t)4 * c->NANG * sizeof(int)));
  return 0;
}
// grows the context's per-point buffers to npts points.  `s`: the stream of the IMPLSCH call that needs them (the rows are zeroed ON that
// stream: a hipMemset on the null stream is not ordered against a non-blocking stream -- the caller's kernels could write their rows
// before the zeroes arrive; found by test_implsch_in_blocks_is_bit_identical in a long test process); the null stream for the set-up call
static int implsch_reserve_on(ecwam_hip_ctx* c, int npts, hipStream_t s) {
  HIPCHK(hipSetDevice(c->device));
  const size_t need = (size_t)(npts > 0 ? npts : 0) * implsch4_fin_row() * c->real_bytes;
  if (need > c->fin_bytes) {   // hipFree waits for the kernels still reading the old rows
    if (c->fin) HIPCHK(hipFree(c->fin));
    c->fin = nullptr; c->fin_bytes = 0;
    HIPCHK(hipMalloc(&c->fin, need));
    HIPCHK(hipMemsetAsync(c->fin, 0, need, s));
    // growth is a stall anyway (hipFree / hipMalloc): wait for the zeroes, so that a call on ANOTHER stream issued right after this one
    // (which needs no growth itself) cannot have its rows overwritten by a memset still pending here
    HIPCHK(hipStreamSynchronize(s));
    c->fin_bytes = need;
  }
  // the split kernel pair parks the wind-input coefficient of every bin between its two halves: a double precision context whose
  // configuration runs the RARE builds (implsch4r.hip: their dp form is the split) -- NOT every double precision context: the rows are a
  // fourth spectrum-sized array (68 GB at O1280)
  const bool split = c->real_bytes == 8 && implsch4_rare(c);
  const size_t need_wi = split ? (size_t)(npts > 0 ? npts : 0) * c->NANG * c->NFRE * c->real_bytes : 0;
  if (need_wi > c->wi_bytes) {
    if (c->wi) HIPCHK(hipFree(c->wi));
    c->wi = nullptr; c->wi_bytes = 0;
    HIPCHK(hipMalloc(&c->wi, need_wi));
    c->wi_bytes = need_wi;
  }
  return adv_reserve(c, npts);
}
int ecwam_hip_implsch(ecwam_hip_ctx* c, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws,
                      double* wam2nemo, void* dbg, void* stream) {
  if (!c) return fail("null context");
  if (kijl < kijs || kijs < 0) return fail("ecwam_hip_implsch: bad range");
  HIPCHK(hipSetDevice(c->device));
  if (kijl > kijs && (!fl1 || !wvprpt || !ff || !intf || !mij || !xllws)) return fail("ecwam_hip_implsch: null pointer");
  if (kijl > kijs && c->p.lwnemocou && !wam2nemo) return fail("ecwam_hip_implsch: LWNEMOCOU needs the WAVE2OCEAN buffer");
  if (!c->p.lwnemocou) wam2nemo = nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (!c->implsch_why.empty()) return fail("ecwam_hip_implsch: " + c->implsch_why);
  if (dbg) return fail("ecwam_hip_implsch: the per-point debug rows were an output of the retired one-point-per-wavefront kernel: pass NULL");
  const Implsch4Variant v = implsch4_variant(c);
  if (int rc2 = implsch_reserve_on(c, kijl, s)) return rc2;   // no-op once the buffer covers kijl
  const int rc = in_precision(c, [&](auto t) {
    using T = decltype(t);
    const bool alt = v == Implsch4Variant::iphys0 || v == Implsch4Variant::isnonlin1;
    const auto launch = implsch4_rare(c) ? launch_implsch4r<T> : alt ? launch_implsch4x<T> : launch_implsch4<T>;
    return launch(c->dtab, kijs, kijl, fl1, wvprpt, ff, intf, mij, xllws, c->fin, wam2nemo, c->fast_g, c->fast_gk, c->wi, c->NANG, c->NFRE, c->v4_r1, c->v4_r2,
                  c->v4_nh, v, s);
  });
  if (rc == 0) { HIPCHK(hipGetLastError()); c->implsch_last = 4; return 0; }
  return fail("ecwam_hip_implsch: no build of k_implsch4 covers the configuration (ecwam_hip_create should have refused it)");
}

// WDFLUXES: the switch of a RARE configuration that keeps it from this call (the common and the alternate builds have the mode), or NULL
static const char* wdfluxes_uncovered(const ecwam_hip_ctx* c) {
  // (the double precision build at 24 directions computed wrong fluxes on the device: implsch4w.hip does not instantiate it, and says so here)
  if (!wdfluxes_built(c->NANG, c->real_bytes)) return "24 directions in double precision";
  if (!implsch4_rare(c)) return nullptr;
  if (c->p.lciwa2) return "LCIWA2";
  if (c->p.lwnemocouwrs) return "LWNEMOCOUWRS";
  if (c->p.lwnemocoustrn) return "LWNEMOCOUSTRN";
  if (c->p.isnonlin > 1) return "ISNONLIN 2";
  if (c->p.icode != 3) return "ICODE 1/2";
  if (!c->p.lwvflx_snl) return "LWVFLX_SNL = F";
  return "IPHYS 0 or ISNONLIN 1 beside each other or beside LLGCBZ0 / LLNORMAGAM";
}
int ecwam_hip_wdfluxes_supported(ecwam_hip_ctx* c) {
  if (!c) { fail("null context"); return 0; }
  if (!c->implsch_why.empty()) { fail("ecwam_hip_wdfluxes: " + c->implsch_why); return 0; }
  if (const char* w = wdfluxes_uncovered(c)) { fail(std::string("ecwam_hip_wdfluxes: not covered: ") + w); return 0; }
  return 1;
}
int ecwam_hip_wdfluxes(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* ff, void* intf, int* mij, void* xllws,
                       double* wam2nemo, void* stream) {
  if (!c) return fail("null context");
  if (kijl < kijs || kijs < 0) return fail("ecwam_hip_wdfluxes: bad range");
  HIPCHK(hipSetDevice(c->device));
  if (kijl > kijs && (!fl1 || !wvprpt || !ff || !intf || !mij || !xllws)) return fail("ecwam_hip_wdfluxes: null pointer");
  if (kijl > kijs && c->p.lwnemocou && !wam2nemo) return fail("ecwam_hip_wdfluxes: LWNEMOCOU needs the WAVE2OCEAN buffer");
  if (!c->p.lwnemocou) wam2nemo = nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (!c->implsch_why.empty()) return fail("ecwam_hip_wdfluxes: " + c->implsch_why);
  if (const char* w = wdfluxes_uncovered(c)) return fail(std::string("ecwam_hip_wdfluxes: not covered: ") + w);
  if (int rc2 = implsch_reserve_on(c, kijl, s)) return rc2;   // no-op once the buffer covers kijl
  const Implsch4Variant v = implsch4_variant(c);
  const int rc = in_precision(c, [&](auto t) {
    return launch_wdfluxes<decltype(t)>(c->dtab, kijs, kijl, fl1, wvprpt, ff, intf, mij, xllws, c->fin, wam2nemo, c->NANG, c->NFRE, c->v4_r1, c->v4_r2, c->v4_nh, v, s);
  });
  if (rc == 0) { HIPCHK(hipGetLastError()); return 0; }
  return fail("ecwam_hip_wdfluxes: no build of k_implsch4 covers the configuration (ecwam_hip_create should have refused it)");
}
int ecwam_hip_setice(ecwam_hip_ctx* c, int kijs, int kijl, void* fl1, const void* ff, void* stream) {
  if (!c) return fail("null context");
  if (kijl < kijs || kijs < 0) return fail("ecwam_hip_setice: bad range");
  HIPCHK(hipSetDevice(c->device));
  if (kijl > kijs && (!fl1 || !ff)) return fail("ecwam_hip_setice: null pointer");
  if (((uintptr_t)fl1 % 16) != 0) return fail("ecwam_hip_setice: the spectra must be 16-byte aligned");
  const int rc = in_precision(c, [&](auto t) { return launch_setice<decltype(t)>(c->dtab, kijs, kijl, fl1, ff, c->NANG, c->NFRE, (hipStream_t)stream); });
  if (rc == 0) { HIPCHK(hipGetLastError()); return 0; }
  return fail("ecwam_hip_setice: the frequencies of a direction are no whole number of 16-byte chunks");
}

// BOUINPT (bouinpt.F90:385-424 with INTSPEC) and OUTBC (outbc.F90:78-91): the two calls of WAMODEL between the time step and the output
// (wamodel.F90:333-343); csrc/nest.hip.  They depend on no build of k_implsch4.
int ecwam_hip_bouinpt(ecwam_hip_ctx* c, int kijs, int kijl, int nijb, const int* ijb, const int* ibcl, const int* ibcr, const void* bfw, int nboinp,
                      const void* f1, const void* par1, void* fl1, void* par_out, void* stream) {
  if (!c) return fail("null context");
  if (nijb < 0 || nboinp < 0) return fail("ecwam_hip_bouinpt: negative count");
  if (kijl < kijs || kijs < 0) return fail("ecwam_hip_bouinpt: bad range");
  HIPCHK(hipSetDevice(c->device));
  if (nijb > 0 && (!ijb || !ibcl || !ibcr || !bfw || !fl1)) return fail("ecwam_hip_bouinpt: null pointer");
  if (nijb > 0 && nboinp > 0 && (!f1 || !par1)) return fail("ecwam_hip_bouinpt: null pointer (the boundary records)");
  if (((uintptr_t)fl1 % 16) != 0) return fail("ecwam_hip_bouinpt: the spectra must be 16-byte aligned");
  const int rc = in_precision(c, [&](auto t) {
    return launch_bouinpt<decltype(t)>(c->dtab, kijs, kijl, nijb, ijb, ibcl, ibcr, bfw, nboinp, f1, par1, fl1, par_out, c->NANG, c->NFRE, (hipStream_t)stream);
  });
  if (rc == 0) return launched();
  if (rc < 0) return fail("ecwam_hip_bouinpt: the frequencies of a direction are no whole number of 16-byte chunks");
  return fail("ecwam_hip_bouinpt: unsupported spectral size");
}
int ecwam_hip_outbc(ecwam_hip_ctx* c, int nbc, const int* ijarc, const void* fl1, void* flpts, void* par, void* stream) {
  if (!c) return fail("null context");
  if (nbc < 0) return fail("ecwam_hip_outbc: negative count");
  HIPCHK(hipSetDevice(c->device));
  if (nbc > 0 && (!ijarc || !fl1 || !flpts)) return fail("ecwam_hip_outbc: null pointer");
  const int rc = in_precision(c, [&](auto t) { return launch_outbc<decltype(t)>(c->dtab, nbc, ijarc, fl1, flpts, par, c->NANG, c->NFRE, (hipStream_t)stream); });
  if (rc == 0) return launched();
  return fail("ecwam_hip_outbc: unsupported spectral size");
}

// The start spectra (include/ecwam_hip_start.h; csrc/start.hip): MSTART, UNSETICE, GETSPEC's noise start and tail.  The checks every one of
// them makes, in the order of ecwam_hip_setice; 0 = go on
static int start_checks(ecwam_hip_ctx* c, const char* who, int kijs, int kijl, const void* fl1, const void* ff, bool reads_ff) {
  if (kijl < kijs || kijs < 0) return fail(std::string(who) + ": bad range");
  HIPCHK(hipSetDevice(c->device));
  if (kijl > kijs && (!fl1 || (reads_ff && !ff))) return fail(std::string(who) + ": null pointer");
  if (((uintptr_t)fl1 % 16) != 0) return fail(std::string(who) + ": the spectra must be 16-byte aligned");
  return 0;
}
static int start_done(const char* who, int rc) {
  if (rc == 0) return launched();
  if (rc < 0) return fail(std::string(who) + ": the frequencies of a direction are no whole number of 16-byte chunks");
  return fail(std::string(who) + ": unsupported spectral size");
}
int ecwam_hip_mstart(ecwam_hip_ctx* c, int kijs, int kijl, void* fl1, const void* ff, int iopti, double fetch, double frmax, double thetaq, double fm,
                     double alfa, double zgamma, double sa, double sb, void* stream) {
  if (!c) return fail("null context");
  if (int rc = start_checks(c, "ecwam_hip_mstart", kijs, kijl, fl1, ff, true)) return rc;
  if (iopti < 0 || iopti > 2) return fail("ecwam_hip_mstart: IOPTI must be 0, 1 or 2 (IOPTI = 3, MSWELL, reads a gridded field and is not served)");
  const double par[8] = {fetch, frmax, thetaq, fm, alfa, zgamma, sa, sb};
  return start_done("ecwam_hip_mstart", in_precision(c, [&](auto t) {
    return launch_mstart<decltype(t)>(c->dtab, kijs, kijl, fl1, ff, iopti, par, c->NANG, c->NFRE, (hipStream_t)stream);
  }));
}
int ecwam_hip_unsetice(ecwam_hip_ctx* c, int kijs, int kijl, void* fl1, const void* ff, double delphi, int flags, void* stream) {
  if (!c) return fail("null context");
  if (int rc = start_checks(c, "ecwam_hip_unsetice", kijs, kijl, fl1, ff, true)) return rc;
  if (flags & ~3) return fail("ecwam_hip_unsetice: unknown flags");
  if (flags) return 0;      // LRESTARTED, or CLDOMAIN == 's': unsetice.F90:79 skips the routine
  return start_done("ecwam_hip_unsetice", in_precision(c, [&](auto t) {
    return launch_unsetice<decltype(t)>(c->dtab, kijs, kijl, fl1, ff, delphi, c->p.licerun && c->p.lmaskice, c->p.lbiwbk != 0, c->NANG, c->NFRE, (hipStream_t)stream);
  }));
}
int ecwam_hip_getspec_noise(ecwam_hip_ctx* c, int kijs, int kijl, void* fl1, void* stream) {
  if (!c) return fail("null context");
  if (int rc = start_checks(c, "ecwam_hip_getspec_noise", kijs, kijl, fl1, nullptr, false)) return rc;
  return start_done("ecwam_hip_getspec_noise", in_precision(c, [&](auto t) {
    return launch_getspec_noise<decltype(t)>(c->dtab, kijs, kijl, fl1, c->NANG, c->NFRE, (hipStream_t)stream);
  }));
}
int ecwam_hip_getspec_tail(ecwam_hip_ctx* c, int kijs, int kijl, void* fl1, const void* ff, int nfre_red, void* stream) {
  if (!c) return fail("null context");
  if (int rc = start_checks(c, "ecwam_hip_getspec_tail", kijs, kijl, fl1, ff, true)) return rc;
  if (nfre_red < 1 || nfre_red > c->NFRE) return fail("ecwam_hip_getspec_tail: nfre_red outside 1 .. NFRE");
  return start_done("ecwam_hip_getspec_tail", in_precision(c, [&](auto t) {
    return launch_getspec_tail<decltype(t)>(c->dtab, kijs, kijl, fl1, ff, nfre_red, c->NANG, c->NFRE, (hipStream_t)stream);
  }));
}

// The forcing and coupling seam (include/ecwam_hip_forcing.h; csrc/forcing.hip).  The checks every call on rows makes, in the order of
// ecwam_hip_setice; 0 = go on.  Each buffer: the pointer, whether the call touches it when the range is not empty.
struct SeamBuf { const void* p; bool used; };
static int seam_checks(ecwam_hip_ctx* c, const std::string& who, int kijs, int kijl, const char* map, std::initializer_list<SeamBuf> bufs) {
  if (kijl < kijs || kijs < 0) return fail(who + ": bad range");
  if (map && !(map[0] == 'i' ? c->fmap_in : c->fmap_out)) return fail(who + ": no " + map + " map");
  if (map && kijl > c->fmap_n) return fail(who + ": bad range");
  HIPCHK(hipSetDevice(c->device));
  for (const SeamBuf& b : bufs)
    if (kijl > kijs && b.used && !b.p) return fail(who + ": null pointer");
  for (const SeamBuf& b : bufs)
    if (b.used && ((uintptr_t)b.p % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  return 0;
}
static void fldinter_free(ecwam_hip_ctx* c) {
  if (c->fli_idx) (void)hipFree(c->fli_idx);
  if (c->fli_w) (void)hipFree(c->fli_w);
  c->fli_idx = nullptr;
  c->fli_w = nullptr;
  c->fli_n = c->fli_ngptotg = c->fli_interpol = 0;
}
int ecwam_hip_set_forcing_map(ecwam_hip_ctx* c, int npts, const int* ixy_in, int ncell_in, const int* ixy_out, int ncell_out) {
  if (!c) return fail("null context");
  if (npts < 0) return fail("ecwam_hip_set_forcing_map: negative count");
  if ((ixy_in && ncell_in < 1) || (ixy_out && ncell_out < 1)) return fail("ecwam_hip_set_forcing_map: a map needs a grid of at least one cell");
  for (int i = 0; ixy_in && i < npts; i++)
    if (ixy_in[i] < 0 || ixy_in[i] >= ncell_in) return fail("ecwam_hip_set_forcing_map: inbound index " + std::to_string(i) + " outside [0, ncell_in)");
  if (ixy_out) {
    std::vector<unsigned char> seen((size_t)ncell_out, 0);
    for (int i = 0; i < npts; i++) {
      if (ixy_out[i] < 0 || ixy_out[i] >= ncell_out) return fail("ecwam_hip_set_forcing_map: outbound index " + std::to_string(i) + " outside [0, ncell_out)");
      if (seen[ixy_out[i]]) return fail("ecwam_hip_set_forcing_map: outbound index " + std::to_string(i) + " is a duplicate (two rows would write one cell)");
      seen[ixy_out[i]] = 1;
    }
  }
  HIPCHK(hipSetDevice(c->device));
  // a copy another stream may still read is not freed under it
  HIPCHK(hipDeviceSynchronize());
  if (c->fmap_in) { (void)hipFree(c->fmap_in); c->fmap_in = nullptr; }
  if (c->fmap_out) { (void)hipFree(c->fmap_out); c->fmap_out = nullptr; }
  c->fmap_n = npts; c->fmap_ncell_in = c->fmap_ncell_out = 0;
  fldinter_free(c);      // the table of ecwam_hip_set_fldinter was checked against the map that goes
  const size_t bytes = (size_t)(npts > 0 ? npts : 1) * sizeof(int);
  if (ixy_in) {
    HIPCHK(hipMalloc((void**)&c->fmap_in, bytes));
    if (npts > 0) HIPCHK(hipMemcpy(c->fmap_in, ixy_in, (size_t)npts * sizeof(int), hipMemcpyHostToDevice));
    c->fmap_ncell_in = (size_t)ncell_in;
  }
  if (ixy_out) {
    HIPCHK(hipMalloc((void**)&c->fmap_out, bytes));
    if (npts > 0) HIPCHK(hipMemcpy(c->fmap_out, ixy_out, (size_t)npts * sizeof(int), hipMemcpyHostToDevice));
    c->fmap_ncell_out = (size_t)ncell_out;
  }
  return 0;
}
int ecwam_hip_getwnd(ecwam_hip_ctx* c, int kijs, int kijl, const void* fieldg, const void* ucur, const void* vcur, const double* nemo, void* ff,
                     const ecwam_hip_forcing_opts* o, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_getwnd";
  if (!o) return fail(who + ": null options");
  if (o->icode_wnd < 1 || o->icode_wnd > 3) return fail(who + ": ICODE_WND must be 1, 2 or 3");
  if (!o->lwnemocoucic && o->iparamci != 31 && o->iparamci != 139) return fail(who + ": IPARAMCI must be 31 or 139 unless LWNEMOCOUCIC");
  const bool cur = o->lcorrel != 0 && o->icode_wnd == 3, nm = o->lwnemocoucic || o->lwnemocoucit;
  if (int rc = seam_checks(c, who, kijs, kijl, "inbound", {{fieldg, true}, {ff, true}, {ucur, cur}, {vcur, cur}, {nemo, nm}})) return rc;
  in_precision(c, [&](auto t) {
    launch_getwnd<decltype(t)>(c->dtab, kijs, kijl, c->fmap_in, fieldg, c->fmap_ncell_in, ucur, vcur, nemo, ff, *o, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_cdustarz0(ecwam_hip_ctx* c, int kijs, int kijl, void* ff, void* stream) {
  if (!c) return fail("null context");
  if (int rc = seam_checks(c, "ecwam_hip_cdustarz0", kijs, kijl, nullptr, {{ff, true}})) return rc;
  in_precision(c, [&](auto t) { launch_cdustarz0<decltype(t)>(c->dtab, kijs, kijl, ff, (hipStream_t)stream); });
  return launched();
}
int ecwam_hip_wamadswstar(ecwam_hip_ctx* c, int kijs, int kijl, const void* fieldg, void* ff, void* stream) {
  if (!c) return fail("null context");
  if (int rc = seam_checks(c, "ecwam_hip_wamadswstar", kijs, kijl, "inbound", {{fieldg, true}, {ff, true}})) return rc;
  in_precision(c, [&](auto t) { launch_wamadswstar<decltype(t)>(kijs, kijl, c->fmap_in, fieldg, c->fmap_ncell_in, ff, (hipStream_t)stream); });
  return launched();
}
int ecwam_hip_getcurr(ecwam_hip_ctx* c, int kijs, int kijl, int mode, const void* fieldg, const double* nemo, void* ucur, void* vcur, int* changed,
                      void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_getcurr";
  if (mode < 0 || mode > 2) return fail(who + ": mode must be 0 (WAMCUR), 1 (NEMO) or 2 (zero)");
  if (int rc = seam_checks(c, who, kijs, kijl, mode == 2 ? nullptr : "inbound", {{fieldg, mode != 2}, {nemo, mode == 1}, {ucur, true}, {vcur, true}})) return rc;
  if (((uintptr_t)changed % sizeof(int)) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  in_precision(c, [&](auto t) {
    launch_getcurr<decltype(t)>(kijs, kijl, mode, c->fmap_in, fieldg, c->fmap_ncell_in, nemo, ucur, vcur, changed, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_wvblock(ecwam_hip_ctx* c, int kijs, int kijl, const void* ff, const void* intf, int flags, int nwvfields, double prchar, void* wvblock, int ld,
                      void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_wvblock";
  const int all = ECWAM_HIP_WVB_LWCOU2W | ECWAM_HIP_WVB_LWCOUHMF | ECWAM_HIP_WVB_LWSTOKES | ECWAM_HIP_WVB_LWFLUX;
  if (flags & ~all) return fail(who + ": unknown flags");
  if ((flags & ECWAM_HIP_WVB_LWCOUHMF) && !(flags & ECWAM_HIP_WVB_LWCOU2W)) return fail(who + ": LWCOUHMF needs LWCOU2W (without OUTBETA there is no BETAHQ)");
  const int need = 1 + ((flags & ECWAM_HIP_WVB_LWCOUHMF) ? 1 : 0) + ((flags & ECWAM_HIP_WVB_LWSTOKES) ? 2 : 0) + ((flags & ECWAM_HIP_WVB_LWFLUX) ? 7 : 0);
  if (nwvfields < need) return fail(who + ": nwvfields is smaller than the switches need (" + std::to_string(need) + ")");
  if (nwvfields > ECWAM_HIP_MAXWVFIELDS) return fail(who + ": nwvfields above ECWAM_HIP_MAXWVFIELDS");
  const bool rf = (flags & ECWAM_HIP_WVB_LWCOU2W) != 0, ri = (flags & (ECWAM_HIP_WVB_LWSTOKES | ECWAM_HIP_WVB_LWFLUX)) != 0;
  if (int rc = seam_checks(c, who, kijs, kijl, nullptr, {{ff, rf}, {intf, ri}, {wvblock, true}})) return rc;
  if (ld < kijl) return fail(who + ": bad range");
  in_precision(c, [&](auto t) {
    launch_wvblock<decltype(t)>(c->dtab, c->p.llgcbz0, kijs, kijl, ff, intf, flags, nwvfields, prchar, wvblock, ld, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_fldtoifs(ecwam_hip_ctx* c, int kijs, int kijl, const void* wvblock, int ld, int nwvfields, const double* defval, void* grid, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_fldtoifs";
  if (nwvfields < 1 || nwvfields > ECWAM_HIP_MAXWVFIELDS) return fail(who + ": nwvfields outside 1 .. ECWAM_HIP_MAXWVFIELDS");
  if (int rc = seam_checks(c, who, kijs, kijl, "outbound", {{wvblock, true}, {grid, true}})) return rc;
  if (ld < kijl) return fail(who + ": bad range");
  if (defval && !grid) return fail(who + ": null pointer");
  in_precision(c, [&](auto t) {
    launch_fldtoifs<decltype(t)>(kijs, kijl, c->fmap_out, wvblock, ld, nwvfields, defval, grid, c->fmap_ncell_out, (hipStream_t)stream);
  });
  return launched();
}

// The forcing intake (include/ecwam_hip_intake.h; csrc/intake.hip)
int ecwam_hip_set_fldinter(ecwam_hip_ctx* c, int npts, int ngptotg, const int* idx, const double* w, int interpol) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_set_fldinter";
  if (idx) {
    if (npts < 0) return fail(who + ": negative count");
    if (ngptotg < 1) return fail(who + ": the fields need at least one point");
    if (interpol && !w) return fail(who + ": the interpolation needs its weights");
    if (!c->fmap_in) return fail(who + ": no inbound map");
    if (npts != c->fmap_n) return fail(who + ": the inbound map has " + std::to_string(c->fmap_n) + " rows, the table " + std::to_string(npts));
    // the rows must write distinct cells: the validated map is read back (a setter may wait)
    HIPCHK(hipSetDevice(c->device));
    std::vector<int> map((size_t)(npts > 0 ? npts : 1), 0);
    if (npts > 0) HIPCHK(hipMemcpy(map.data(), c->fmap_in, (size_t)npts * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<unsigned char> seen(c->fmap_ncell_in, 0);
    for (int i = 0; i < npts; i++) {
      const int cell = map[(size_t)i];
      if (seen[(size_t)cell]) return fail(who + ": row " + std::to_string(i) + " of the inbound map names a cell twice (two rows would write one cell)");
      seen[(size_t)cell] = 1;
    }
    for (int i = 0; i < npts; i++)
      for (int k = 0; k < (interpol ? 4 : 1); k++)
        if (idx[4 * (size_t)i + k] < 0 || idx[4 * (size_t)i + k] >= ngptotg)
          return fail(who + ": index " + std::to_string(k) + " of row " + std::to_string(i) + " outside [0, ngptotg)");
    if (interpol && c->real_bytes == 4)      // the library narrows the weights back: nothing may be lost
      for (size_t i = 0; i < 3 * (size_t)npts; i++)
        if ((double)(float)w[i] != w[i])
          return fail(who + ": weight " + std::to_string(i % 3) + " of row " + std::to_string(i / 3) + " is not a value of the working precision");
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());      // a copy another stream may still read is not freed under it
  fldinter_free(c);
  if (!idx) return 0;
  const size_t n = (size_t)(npts > 0 ? npts : 1);
  std::vector<int> hi(4 * n, 0);
  for (int i = 0; i < npts; i++)
    for (int k = 0; k < 4; k++) hi[4 * (size_t)i + k] = idx[4 * (size_t)i + (interpol ? k : 0)];
  // a failure half way leaves no table, not half of one
  auto upload = [&]() -> int {
    HIPCHK(hipMalloc((void**)&c->fli_idx, 4 * n * sizeof(int)));
    HIPCHK(hipMemcpy(c->fli_idx, hi.data(), 4 * n * sizeof(int), hipMemcpyHostToDevice));
    if (!interpol) return 0;
    HIPCHK(hipMalloc(&c->fli_w, 4 * n * (size_t)c->real_bytes));
    return in_precision(c, [&](auto t) {
      std::vector<decltype(t)> hw(4 * n, 0);
      for (int i = 0; i < npts; i++)
        for (int k = 0; k < 3; k++) hw[4 * (size_t)i + k] = (decltype(t))w[3 * (size_t)i + k];
      HIPCHK(hipMemcpy(c->fli_w, hw.data(), 4 * n * sizeof(decltype(t)), hipMemcpyHostToDevice));
      return 0;
    });
  };
  if (int rc = upload()) {
    fldinter_free(c);
    return rc;
  }
  c->fli_n = npts; c->fli_ngptotg = ngptotg; c->fli_interpol = interpol != 0;
  return 0;
}
int ecwam_hip_fldinter(ecwam_hip_ctx* c, int kijs, int kijl, const void* fields, int ngptotg, int nfields, int flags, double roair, double wstar0, double pmiss,
                       void* fieldg, int* mask_in, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_fldinter";
  const int all = ECWAM_HIP_FLI_LADEN | ECWAM_HIP_FLI_LGUST | ECWAM_HIP_FLI_LLKC | ECWAM_HIP_FLI_LWCUR | ECWAM_HIP_FLI_NEWCURR;
  if (kijl < kijs || kijs < 0 || (c->fli_idx && kijl > c->fli_n)) return fail(who + ": bad range");      // rows beyond the table
  if (flags & ~all) return fail(who + ": unknown flags");
  if (!c->fli_idx) return fail(who + ": no table");
  if (ngptotg != c->fli_ngptotg) return fail(who + ": ngptotg is " + std::to_string(ngptotg) + ", the table's " + std::to_string(c->fli_ngptotg));
  const bool cur = (flags & ECWAM_HIP_FLI_NEWCURR) && (flags & ECWAM_HIP_FLI_LWCUR);
  if (nfields < (cur ? 10 : 8)) return fail(who + ": nfields is smaller than the switches need (" + std::to_string(cur ? 10 : 8) + ")");
  if (int rc = seam_checks(c, who, kijs, kijl, "inbound", {{fields, true}, {fieldg, true}})) return rc;
  if (((uintptr_t)mask_in % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  in_precision(c, [&](auto t) {
    launch_fldinter<decltype(t)>(kijs, kijl, c->fli_idx, c->fli_w, c->fli_interpol, c->fmap_in, fields, (size_t)ngptotg, flags, roair, wstar0, pmiss, fieldg,
                                 c->fmap_ncell_in, mask_in, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_init_fieldg(ecwam_hip_ctx* c, void* fieldg, int ncell, double roair, double wstar0, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_init_fieldg";
  if (ncell < 0) return fail(who + ": bad range");
  HIPCHK(hipSetDevice(c->device));
  if (ncell > 0 && !fieldg) return fail(who + ": null pointer");
  if (((uintptr_t)fieldg % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  in_precision(c, [&](auto t) { launch_init_fieldg<decltype(t)>(c->dtab, fieldg, (size_t)ncell, roair, wstar0, (hipStream_t)stream); });
  return launched();
}
int ecwam_hip_recvnemofields(ecwam_hip_ctx* c, int kijs, int kijl, int flags, const void* fieldg, double* nemo, double* nemoibr, void* ff, void* ucur, void* vcur,
                             void* intf, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_recvnemofields";
  const int all = ECWAM_HIP_RNF_LREST | ECWAM_HIP_RNF_LINIT | ECWAM_HIP_RNF_LWCOU | ECWAM_HIP_RNF_LWNEMOCOUCIC | ECWAM_HIP_RNF_LWNEMOCOUCIT |
                  ECWAM_HIP_RNF_LWNEMOCOUCUR | ECWAM_HIP_RNF_LWNEMOCOUIBR;
  const bool lake = (flags & ECWAM_HIP_RNF_LINIT) && (flags & ECWAM_HIP_RNF_LWCOU);      // the branch that reads the map
  if (kijl < kijs || kijs < 0 || (lake && c->fmap_in && kijl > c->fmap_n)) return fail(who + ": bad range");
  if (flags & ~all) return fail(who + ": unknown flags");
  const bool rest = flags & ECWAM_HIP_RNF_LREST, init = flags & ECWAM_HIP_RNF_LINIT, cou = flags & ECWAM_HIP_RNF_LWCOU;
  const bool cic = flags & ECWAM_HIP_RNF_LWNEMOCOUCIC, cit = flags & ECWAM_HIP_RNF_LWNEMOCOUCIT, cur = flags & ECWAM_HIP_RNF_LWNEMOCOUCUR;
  const bool ibr = flags & ECWAM_HIP_RNF_LWNEMOCOUIBR;
  if (!rest && !init) return fail(who + ": neither LREST nor LINIT");
  // the branches that read LKFR through the map, in the kernel as here (IBRMEM takes NEMO's value on either side and reads neither)
  const bool grid = init && cou && (cic || cit || cur);
  const bool b_nemo = rest || (init && (cic || cit || cur)), b_ibr = ibr, b_ff = rest || (init && (cic || cit)), b_cur = rest || (init && cur);
  if (int rc = seam_checks(c, who, kijs, kijl, init && cou ? "inbound" : nullptr,
                           {{fieldg, grid}, {nemo, b_nemo}, {nemoibr, b_ibr}, {ff, b_ff}, {ucur, b_cur}, {vcur, b_cur}, {intf, ibr}}))
    return rc;
  in_precision(c, [&](auto t) {
    launch_recvnemofields<decltype(t)>(kijs, kijl, flags, c->fmap_in, fieldg, c->fmap_ncell_in, nemo, nemoibr, ff, ucur, vcur, intf, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_updnemo(ecwam_hip_ctx* c, int kijs, int kijl, double* wam2nemo, int nemontau, double* fields7, double* stress6, int ld, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_updnemo";
  if (kijl < kijs || kijs < 0 || ld < kijl) return fail(who + ": bad range");
  if (int rc = seam_checks(c, who, kijs, kijl, nullptr, {{wam2nemo, fields7 || stress6}})) return rc;
  if (((uintptr_t)fields7 % 16) != 0 || ((uintptr_t)stress6 % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  // ZNEMONTAUM1 = 1.0_JWRB / NEMONTAU
  const double m1 = nemontau > 0 ? in_precision(c, [&](auto t) { return (double)((decltype(t))1 / (decltype(t))nemontau); }) : 0.0;
  launch_updnemo(kijs, kijl, wam2nemo, nemontau > 0, m1, fields7, stress6, ld, (hipStream_t)stream);
  return launched();
}

// The forcing of a stand-alone run (include/ecwam_hip_readwind.h; csrc/readwind.hip)
static void g2w_free(ecwam_hip_ctx::G2wSlot& g) {
  if (g.pos) (void)hipFree(g.pos);
  if (g.w) (void)hipFree(g.w);
  g = ecwam_hip_ctx::G2wSlot{};
}
int ecwam_hip_set_input_grid(ecwam_hip_ctx* c, int slot, int ncell, int nvalues, const int* pos, const double* w, const int* kind, int interpol) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_set_input_grid";
  if (slot < 0 || slot >= ECWAM_HIP_G2W_NSLOT) return fail(who + ": bad range");
  if (pos) {
    if (ncell < 0) return fail(who + ": negative count");
    if (nvalues < 1) return fail(who + ": the message needs at least one value");
    if (!kind) return fail(who + ": null pointer");
    if (interpol && !w) return fail(who + ": the interpolation needs its weights");
    for (int i = 0; i < ncell; i++) {
      if (kind[i] < 0 || kind[i] > 2) return fail(who + ": kind of cell " + std::to_string(i) + " outside 0 .. 2");
      for (int k = 0; k < (interpol ? 4 : 1); k++) {
        const int p = pos[4 * (size_t)i + k];
        if (p < -1 || p >= nvalues || (!interpol && kind[i] == 2 && p < 0))
          return fail(who + ": position " + std::to_string(k) + " of cell " + std::to_string(i) + " outside [" + (interpol ? "-1" : "0") + ", nvalues)");
      }
    }
    if (interpol)
      for (size_t i = 0; i < 3 * (size_t)ncell; i++) {
        if (!std::isfinite(w[i])) return fail(who + ": weight " + std::to_string(i % 3) + " of cell " + std::to_string(i / 3) + " is not finite");
        if (c->real_bytes == 4 && (double)(float)w[i] != w[i])      // the library narrows the weights back: nothing may be lost
          return fail(who + ": weight " + std::to_string(i % 3) + " of cell " + std::to_string(i / 3) + " is not a value of the working precision");
      }
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());      // a copy another stream may still read is not freed under it
  ecwam_hip_ctx::G2wSlot& g = c->g2w[slot];
  g2w_free(g);
  if (!pos) return 0;
  const size_t n = (size_t)(ncell > 0 ? ncell : 1);
  std::vector<int> hp(4 * n, -1);
  for (int i = 0; i < ncell; i++)
    for (int k = 0; k < 4; k++) hp[4 * (size_t)i + k] = pos[4 * (size_t)i + (interpol ? k : 0)];
  // a failure half way leaves no table, not half of one
  auto upload = [&]() -> int {
    HIPCHK(hipMalloc((void**)&g.pos, 4 * n * sizeof(int)));
    HIPCHK(hipMemcpy(g.pos, hp.data(), 4 * n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&g.w, 4 * n * (size_t)c->real_bytes));
    return in_precision(c, [&](auto t) {
      std::vector<decltype(t)> hw(4 * n, 0);
      for (int i = 0; i < ncell; i++) {
        for (int k = 0; interpol && k < 3; k++) hw[4 * (size_t)i + k] = (decltype(t))w[3 * (size_t)i + k];
        hw[4 * (size_t)i + 3] = (decltype(t))kind[i];
      }
      HIPCHK(hipMemcpy(g.w, hw.data(), 4 * n * sizeof(decltype(t)), hipMemcpyHostToDevice));
      return 0;
    });
  };
  if (int rc = upload()) {
    g2w_free(g);
    return rc;
  }
  g.ncell = ncell; g.nvalues = nvalues; g.interpol = interpol != 0;
  return 0;
}
int ecwam_hip_grib2wgrid(ecwam_hip_ctx* c, int slot, const void* values, int vstride, int nfld, const ecwam_hip_g2w_field* desc, double roair, double wstar0,
                         double pmiss, void* out, int ld, void* fieldg, int ncell_in, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_grib2wgrid";
  if (slot < 0 || slot >= ECWAM_HIP_G2W_NSLOT) return fail(who + ": bad range");
  const ecwam_hip_ctx::G2wSlot& g = c->g2w[slot];
  if (!g.pos) return fail(who + ": no table");
  if (vstride < g.nvalues) return fail(who + ": vstride is " + std::to_string(vstride) + ", the table's nvalues " + std::to_string(g.nvalues));
  if (nfld < 1 || nfld > ECWAM_HIP_G2W_MAXFLD) return fail(who + ": nfld outside 1 .. 16");
  if (!desc) return fail(who + ": null descriptors");
  bool any_field = false, any_plane = false;
  unsigned seen = 0;
  for (int f = 0; f < nfld; f++) {
    const int t = desc[f].target;
    if (desc[f].flags & ~(ECWAM_HIP_G2W_DIRFLD | ECWAM_HIP_G2W_NONWAVE)) return fail(who + ": unknown flags of field " + std::to_string(f));
    if (t == ECWAM_HIP_G2W_FIELD) {
      any_field = true;
      continue;
    }
    if (t != ECWAM_HIP_FG_UWND && t != ECWAM_HIP_FG_VWND && t != ECWAM_HIP_FG_AIRD && t != ECWAM_HIP_FG_WSTAR && t != ECWAM_HIP_FG_CICOVER &&
        t != ECWAM_HIP_FG_CITHICK && t != ECWAM_HIP_FG_WSWAVE && t != ECWAM_HIP_FG_WDWAVE)
      return fail(who + ": unknown target of field " + std::to_string(f));
    if (seen & (1u << t)) return fail(who + ": field " + std::to_string(f) + " targets a plane a field before it fills (LLNOTREAD)");
    seen |= 1u << t;
    any_plane = true;
  }
  if (any_plane && ncell_in != g.ncell) return fail(who + ": ncell_in is " + std::to_string(ncell_in) + ", the table's ncell " + std::to_string(g.ncell));
  if (any_field && ld < g.ncell) return fail(who + ": ld is smaller than the table's ncell");
  HIPCHK(hipSetDevice(c->device));
  if (g.ncell > 0 && (!values || (any_field && !out) || (any_plane && !fieldg))) return fail(who + ": null pointer");
  if (((uintptr_t)values % 16) != 0 || (any_field && ((uintptr_t)out % 16) != 0) || (any_plane && ((uintptr_t)fieldg % 16) != 0))
    return fail(who + ": the buffers must be 16-byte aligned");
  in_precision(c, [&](auto t) {
    launch_grib2wgrid<decltype(t)>(g.ncell, g.pos, g.w, g.interpol, values, (size_t)vstride, nfld, desc, roair, wstar0, pmiss, out, (size_t)(ld > 0 ? ld : 0), fieldg,
                                   (size_t)g.ncell, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_current2wam(ecwam_hip_ctx* c, int kijs, int kijl, const void* field_u, const void* field_v, double wlowest, double zmiss, void* ucur, void* vcur,
                          int* changed, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_current2wam";
  if (int rc = seam_checks(c, who, kijs, kijl, "inbound", {{field_u, false}, {field_v, false}, {ucur, field_u != nullptr}, {vcur, field_v != nullptr}})) return rc;
  if (((uintptr_t)field_u % 16) != 0 || ((uintptr_t)field_v % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  if (((uintptr_t)changed % sizeof(int)) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  in_precision(c, [&](auto t) {
    launch_current2wam<decltype(t)>(kijs, kijl, c->fmap_in, field_u, field_v, wlowest, zmiss, ucur, vcur, changed, (hipStream_t)stream);
  });
  return launched();
}

// GRIB-ready spectra and parameter fields (include/ecwam_hip_gribout.h; csrc/gribout.hip)
int ecwam_hip_set_grib_map(ecwam_hip_ctx* c, int npts, const int* ival, int ntencode, const ecwam_hip_grib_poles* poles) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_set_grib_map";
  if (npts < 0) return fail(who + ": negative count");
  if (ntencode < 1) return fail(who + ": NTENCODE must be at least 1");
  if (npts > 0 && !ival) return fail(who + ": null pointer");
  // the four ranges: inside the vector, no two overlapping; a pole without padding takes no part
  ecwam_hip_grib_pole pl[2] = {};
  if (poles) { pl[0] = poles->north; pl[1] = poles->south; }
  int lo[4], hi[4], nr = 0;
  for (int s = 0; s < 2; s++) {
    if (pl[s].npole < 0 || pl[s].nadj < 0) return fail(who + ": a pole range has a negative length");
    if (pl[s].npole == 0) { pl[s] = ecwam_hip_grib_pole{}; continue; }
    const int r0[2] = {pl[s].pole0, pl[s].adj0}, rn[2] = {pl[s].npole, pl[s].nadj};
    for (int q = 0; q < 2; q++) {
      if (r0[q] < 0 || r0[q] > ntencode || rn[q] > ntencode - r0[q]) return fail(who + ": a pole range leaves the vector");
      if (rn[q] == 0) continue;
      for (int o = 0; o < nr; o++)
        if (r0[q] < hi[o] && lo[o] < r0[q] + rn[q]) return fail(who + ": the pole ranges overlap");
      lo[nr] = r0[q]; hi[nr] = r0[q] + rn[q]; nr++;
    }
  }
  std::vector<int> inv((size_t)ntencode, -1);      // cell -> row
  for (int i = 0; i < npts; i++) {
    if (ival[i] < 0 || ival[i] >= ntencode) return fail(who + ": index " + std::to_string(i) + " outside [0, ntencode)");
    if (inv[ival[i]] >= 0) return fail(who + ": index " + std::to_string(i) + " is a duplicate (two rows would write one value)");
    inv[ival[i]] = i;
  }
  auto in_pole = [&](int cell) { return (cell >= pl[0].pole0 && cell - pl[0].pole0 < pl[0].npole) || (cell >= pl[1].pole0 && cell - pl[1].pole0 < pl[1].npole); };
  std::vector<int> unf, adj;
  for (int cell = 0; cell < ntencode; cell++)
    if (inv[cell] < 0 && !in_pole(cell)) unf.push_back(cell);
  for (int s = 0; s < 2; s++)
    for (int i = 0; i < pl[s].nadj; i++) adj.push_back(inv[pl[s].adj0 + i]);
  HIPCHK(hipSetDevice(c->device));
  // a copy another stream may still read is not freed under it
  HIPCHK(hipDeviceSynchronize());
  grib_map_free(c);
  auto upload = [](const int* h, size_t n, const int** d) -> hipError_t {
    int* p = nullptr;
    hipError_t e = hipMalloc((void**)&p, (n > 0 ? n : 1) * sizeof(int));
    if (e == hipSuccess && n > 0) e = hipMemcpy(p, h, n * sizeof(int), hipMemcpyHostToDevice);
    *d = p;
    return e;
  };
  HIPCHK(upload(ival, (size_t)npts, &c->gmap.ival));
  HIPCHK(upload(unf.data(), unf.size(), &c->gmap.unfilled));
  HIPCHK(upload(adj.data(), adj.size(), &c->gmap.adj));
  HIPCHK(hipMalloc(&c->gmap_keys, (size_t)c->NANG * c->NFRE_RED * sizeof(unsigned long long)));
  c->gmap.nunf = (int)unf.size(); c->gmap.ntencode = ntencode; c->gmap.north = pl[0]; c->gmap.south = pl[1];
  c->gmap_n = npts;
  return 0;
}
// the checks of the three calls on rows, in the order of seam_checks; need_map: rows beyond the map are a bad range
static int grib_checks(ecwam_hip_ctx* c, const std::string& who, int kijs, int kijl, bool need_map, std::initializer_list<SeamBuf> bufs) {
  if (kijl < kijs || kijs < 0) return fail(who + ": bad range");
  if (need_map && !c->gmap.ival) return fail(who + ": no grib map");
  if (need_map && kijl > c->gmap_n) return fail(who + ": bad range");
  HIPCHK(hipSetDevice(c->device));
  for (const SeamBuf& b : bufs)
    if (kijl > kijs && b.used && !b.p) return fail(who + ": null pointer");
  for (const SeamBuf& b : bufs)
    if (b.used && ((uintptr_t)b.p % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  return 0;
}
static int grib_opts_ok(const std::string& who, const ecwam_hip_grib_opts* o, bool spectral) {
  if (!o) return fail(who + ": null options");
  if (spectral && (o->ngrbress < 1 || o->ngrbress > 30)) return fail(who + ": NGRBRESS outside 1 .. 30");
  if (spectral && !(o->ppeps > 0)) return fail(who + ": PPEPS must be positive");
  return 0;
}
static int grib_tile_done(const std::string& who, int rc) {
  if (rc == 0) return launched();
  if (rc < 0) return fail(who + ": the frequencies of a direction are no whole number of 16-byte chunks");
  return fail(who + ": unsupported spectral size");
}
int ecwam_hip_outspec_values(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* ff, int ifld0, int nfld, int flags, const ecwam_hip_grib_opts* o,
                             void* values, void* ppmax, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_outspec_values";
  if (int rc = grib_opts_ok(who, o, true)) return rc;
  if (flags & ~ECWAM_HIP_OUTSPEC_ICEMASK) return fail(who + ": unknown flags");
  if (ifld0 < 0 || nfld < 1 || nfld > c->NANG * c->NFRE_RED - ifld0) return fail(who + ": bad field range");
  const bool ice = (flags & ECWAM_HIP_OUTSPEC_ICEMASK) != 0;
  if (int rc = grib_checks(c, who, kijs, kijl, true, {{fl1, true}, {ff, ice}, {values, true}, {ppmax, false}})) return rc;
  if (((uintptr_t)ppmax % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  return grib_tile_done(who, in_precision(c, [&](auto t) {
    return launch_outspec_values<decltype(t)>(kijs, kijl, fl1, ff, ifld0, nfld, ice, c->p.cithrsh, c->p.flmin, *o, c->gmap, values, ppmax, c->gmap_keys, c->NANG, c->NFRE,
                                              c->NFRE_RED, (hipStream_t)stream);
  }));
}
int ecwam_hip_outspec_pack(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* ff, int ifld0, int nfld, int flags, void* blk, int ld, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_outspec_pack";
  if (flags & ~ECWAM_HIP_OUTSPEC_ICEMASK) return fail(who + ": unknown flags");
  if (ifld0 < 0 || nfld < 1 || nfld > c->NANG * c->NFRE_RED - ifld0) return fail(who + ": bad field range");
  const bool ice = (flags & ECWAM_HIP_OUTSPEC_ICEMASK) != 0;
  if (int rc = grib_checks(c, who, kijs, kijl, false, {{fl1, true}, {ff, ice}, {blk, true}})) return rc;
  if (ld < kijl) return fail(who + ": bad range");
  return grib_tile_done(who, in_precision(c, [&](auto t) {
    return launch_outspec_pack<decltype(t)>(kijs, kijl, fl1, ff, ifld0, nfld, ice, c->p.cithrsh, c->p.flmin, blk, ld, c->NANG, c->NFRE, c->NFRE_RED, (hipStream_t)stream);
  }));
}
int ecwam_hip_grib_values(ecwam_hip_ctx* c, int kijs, int kijl, const void* src, long long fstride, long long pstride, int nfld, int spectral,
                          const ecwam_hip_grib_opts* o, void* values, void* ppmax, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_grib_values";
  if (spectral != 0 && spectral != 1) return fail(who + ": spectral must be 0 or 1");
  if (int rc = grib_opts_ok(who, o, spectral != 0)) return rc;
  if (nfld < 1 || nfld > (spectral ? c->NANG * c->NFRE_RED : 65535)) return fail(who + ": bad field range");
  if (fstride < 1 || pstride < 1) return fail(who + ": the strides must be positive");
  if (int rc = grib_checks(c, who, kijs, kijl, true, {})) return rc;
  if (kijl > kijs && (!src || !values)) return fail(who + ": null pointer");
  // the stores are single reals: a run of columns may begin anywhere in values
  if (((uintptr_t)src | (uintptr_t)values | (uintptr_t)ppmax) % c->real_bytes != 0) return fail(who + ": the buffers must be aligned to a real");
  in_precision(c, [&](auto t) {
    launch_grib_values<decltype(t)>(kijs, kijl, src, fstride, pstride, nfld, spectral, *o, c->gmap, values, ppmax, c->gmap_keys, (hipStream_t)stream);
  });
  return launched();
}

// Decoded GRIB spectra and READFL's record into FL1 (include/ecwam_hip_gribin.h; csrc/gribin.hip).  map: the _values form (through the map of
// ecwam_hip_set_grib_map, fields below NANG NFRE_RED, stride >= ntencode); otherwise the _unpack form (fields below NANG NFRE, stride >= kijl)
static int getspec_fields(ecwam_hip_ctx* c, const std::string& who, bool map, int kijs, int kijl, const void* src, long long stride, int ifld0, int nfld, int flags,
                          const ecwam_hip_grib_opts* o, void* fl1, void* stream) {
  if (flags & ~(ECWAM_HIP_GETSPEC_UNSCALE | ECWAM_HIP_GETSPEC_MISSING)) return fail(who + ": unknown flags");
  if (flags && !o) return fail(who + ": null options");
  const int mlim = map ? c->NFRE_RED : c->NFRE;
  if (ifld0 < 0 || nfld < 1 || nfld > c->NANG * mlim - ifld0) return fail(who + ": bad field range");
  if (int rc = grib_checks(c, who, kijs, kijl, map, {})) return rc;
  if (stride < (map ? (long long)c->gmap.ntencode : (long long)kijl)) return fail(who + ": bad range");
  if (kijl > kijs && (!src || !fl1)) return fail(who + ": null pointer");
  if (((uintptr_t)fl1 % 16) != 0) return fail(who + ": the spectra must be 16-byte aligned");
  if (((uintptr_t)src % c->real_bytes) != 0) return fail(who + ": the buffers must be aligned to a real");
  return grib_tile_done(who, in_precision(c, [&](auto t) {
    return launch_getspec_fields<decltype(t)>(kijs, kijl, src, stride, map ? c->gmap.ival : nullptr, ifld0, nfld, flags, o, c->p.epsmin, fl1, c->NANG, c->NFRE, mlim,
                                              (hipStream_t)stream);
  }));
}
int ecwam_hip_getspec_values(ecwam_hip_ctx* c, int kijs, int kijl, const void* values, long long fstride, int ifld0, int nfld, int flags, const ecwam_hip_grib_opts* o,
                             void* fl1, void* stream) {
  if (!c) return fail("null context");
  return getspec_fields(c, "ecwam_hip_getspec_values", true, kijs, kijl, values, fstride, ifld0, nfld, flags, o, fl1, stream);
}
int ecwam_hip_getspec_unpack(ecwam_hip_ctx* c, int kijs, int kijl, const void* blk, long long ld, int ifld0, int nfld, int flags, const ecwam_hip_grib_opts* o, void* fl1,
                             void* stream) {
  if (!c) return fail("null context");
  return getspec_fields(c, "ecwam_hip_getspec_unpack", false, kijs, kijl, blk, ld, ifld0, nfld, flags, o, fl1, stream);
}

// The start and the end of a run (include/ecwam_hip_restart.h; csrc/restart.hip).  The checks of a call on rows after what the call itself refuses:
// the range, then the buffers -- a16: 16-byte aligned; ar: aligned to a real; used: the call touches the buffer wherever the range is not empty (a
// null pointer is refused then); the alignment is asked of every pointer that is given.  0 = go on.
static int restart_checks(ecwam_hip_ctx* c, const std::string& who, int kijs, int kijl, int row_limit, std::initializer_list<SeamBuf> a16, std::initializer_list<SeamBuf> ar) {
  if (kijl < kijs || kijs < 0 || (row_limit >= 0 && kijl > row_limit)) return fail(who + ": bad range");
  HIPCHK(hipSetDevice(c->device));
  for (const std::initializer_list<SeamBuf>& l : {a16, ar})
    for (const SeamBuf& b : l)
      if (kijl > kijs && b.used && !b.p) return fail(who + ": null pointer");
  for (const SeamBuf& b : a16)
    if (((uintptr_t)b.p % 16) != 0) return fail(who + ": the buffers must be 16-byte aligned");
  for (const SeamBuf& b : ar)
    if (((uintptr_t)b.p % c->real_bytes) != 0) return fail(who + ": the buffers must be aligned to a real");
  return 0;
}
int ecwam_hip_depthprpt(ecwam_hip_ctx* c, int kijs, int kijl, const void* depth, const ecwam_hip_depth_opts* o, void* wvprpt, void* wavnum, void* cgroup, void* omosnh2kd,
                        void* ff, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_depthprpt";
  if (!o) return fail(who + ": null options");
  if (!wvprpt && !wavnum && !cgroup && !omosnh2kd && !ff) return fail(who + ": no output");
  if (c->NFRE % (16 / c->real_bytes) != 0) return fail(who + ": the frequencies of a point are no whole number of 16-byte chunks");
  if (int rc = restart_checks(c, who, kijs, kijl, -1, {{wvprpt, false}, {wavnum, false}, {cgroup, false}, {omosnh2kd, false}, {ff, false}}, {{depth, true}})) return rc;
  in_precision(c, [&](auto t) {
    return launch_depthprpt<decltype(t)>(c->dtab, kijs, kijl, depth, o->dkmax, o->gam_b_j, wvprpt, wavnum, cgroup, omosnh2kd, ff, c->NFRE, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_buildstress(ecwam_hip_ctx* c, int kijs, int kijl, const void* uwave, const void* cd, double zref, int flags, double prchar, double zmiss, void* ff,
                          void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_buildstress";
  if (flags & ~(ECWAM_HIP_BST_Z0B_ZERO | ECWAM_HIP_BST_NSESTART)) return fail(who + ": unknown flags");
  const bool plane = uwave || cd;
  if (plane && !c->fmap_in) return fail(who + ": no inbound map");
  if (int rc = restart_checks(c, who, kijs, kijl, plane ? c->fmap_n : -1, {{ff, true}, {uwave, false}, {cd, false}}, {})) return rc;
  in_precision(c, [&](auto t) {
    launch_buildstress<decltype(t)>(c->dtab, kijs, kijl, c->fmap_in, uwave, cd, zref, flags, prchar, zmiss, ff, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_set_restart_map(ecwam_hip_ctx* c, int npts, const int* ij2newij) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_set_restart_map";
  if (npts < 0) return fail(who + ": negative count");
  std::vector<int> inv;
  if (ij2newij) {
    inv.assign((size_t)npts, -1);
    for (int p = 0; p < npts; p++) {
      const int r = ij2newij[p];
      if (r < 0 || r >= npts) return fail(who + ": index " + std::to_string(p) + " outside [0, npts)");
      if (inv[r] >= 0) return fail(who + ": index " + std::to_string(p) + " is a duplicate (no permutation)");
      inv[r] = p;
    }
  }
  HIPCHK(hipSetDevice(c->device));
  // a copy another stream may still read is not freed under it
  HIPCHK(hipDeviceSynchronize());
  if (c->rmap_inv) { (void)hipFree(c->rmap_inv); c->rmap_inv = nullptr; }
  c->rmap_n = 0;
  if (ij2newij) {
    HIPCHK(hipMalloc((void**)&c->rmap_inv, (size_t)(npts > 0 ? npts : 1) * sizeof(int)));
    if (npts > 0) HIPCHK(hipMemcpy(c->rmap_inv, inv.data(), (size_t)npts * sizeof(int), hipMemcpyHostToDevice));
    c->rmap_n = npts;
  }
  return 0;
}
// what the three calls on field vectors check of their positions: 0 = go on; row_limit and ld_min come back
static int restart_positions(ecwam_hip_ctx* c, const std::string& who, int kijl, int relabel, int* row_limit, int* ld_min) {
  if (relabel && !c->rmap_inv) return fail(who + ": no restart map");
  *row_limit = relabel ? c->rmap_n : -1;
  *ld_min = relabel ? c->rmap_n : kijl;
  return 0;
}
static int stress_fields(ecwam_hip_ctx* c, const std::string& who, int pack, int kijs, int kijl, const void* ff, const void* ucur, const void* vcur, int relabel,
                         const void* rfield, int ld, void* stream) {
  int row_limit, ld_min;
  if (int rc = restart_positions(c, who, kijl, relabel, &row_limit, &ld_min)) return rc;
  if (ld < ld_min) return fail(who + ": bad range");
  if (int rc = restart_checks(c, who, kijs, kijl, row_limit, {{ff, true}}, {{ucur, true}, {vcur, true}, {rfield, true}})) return rc;
  in_precision(c, [&](auto t) {
    launch_stress_fields<decltype(t)>(pack, kijs, kijl, relabel ? c->rmap_inv : nullptr, const_cast<void*>(ff), const_cast<void*>(ucur), const_cast<void*>(vcur),
                                      const_cast<void*>(rfield), (size_t)ld, (hipStream_t)stream);
  });
  return launched();
}
int ecwam_hip_savstress_pack(ecwam_hip_ctx* c, int kijs, int kijl, const void* ff, const void* ucur, const void* vcur, int relabel, void* rfield, int ld, void* stream) {
  if (!c) return fail("null context");
  return stress_fields(c, "ecwam_hip_savstress_pack", 1, kijs, kijl, ff, ucur, vcur, relabel, rfield, ld, stream);
}
int ecwam_hip_getstress_unpack(ecwam_hip_ctx* c, int kijs, int kijl, const void* rfield, int ld, int relabel, void* ff, void* ucur, void* vcur, void* stream) {
  if (!c) return fail("null context");
  return stress_fields(c, "ecwam_hip_getstress_unpack", 0, kijs, kijl, ff, ucur, vcur, relabel, rfield, ld, stream);
}
int ecwam_hip_savspec_pack(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, int ifld0, int nfld, int relabel, void* blk, int ld, void* stream) {
  if (!c) return fail("null context");
  const std::string who = "ecwam_hip_savspec_pack";
  if (ifld0 < 0 || nfld < 1 || nfld > c->NANG * c->NFRE - ifld0) return fail(who + ": bad field range");
  int row_limit, ld_min;
  if (int rc = restart_positions(c, who, kijl, relabel, &row_limit, &ld_min)) return rc;
  if (ld < ld_min) return fail(who + ": bad range");
  if (int rc = restart_checks(c, who, kijs, kijl, row_limit, {{fl1, true}}, {{blk, true}})) return rc;
  return grib_tile_done(who, in_precision(c, [&](auto t) {
    return launch_savspec_pack<decltype(t)>(kijs, kijl, fl1, ifld0, nfld, relabel ? c->rmap_inv : nullptr, blk, (size_t)ld, c->NANG, c->NFRE, (hipStream_t)stream);
  }));
}

// bit 0: the one-kernel step covers the context; bit 1: also with fast-wave sub-steps (gin); bit 2: also with the obstructions of
// ecwam_hip_set_obstructions -- a caller takes the one-kernel step when the bits of what it needs are set
int ecwam_hip_propags2_implsch_supported(ecwam_hip_ctx* c) { return c && fused_ok(c) ? implsch4_adv_forms(c->NANG, c->real_bytes) : 0; }

int ecwam_hip_propags2_implsch(ecwam_hip_ctx* c, const void* f1, void* f3, int n, int ngy, double delpro, const int* kxlt, const void* zdello,
                               double xdella, const void* cosph, const void* sinph, const int* klon, const int* klat, const int* kcor,
                               const void* wlat, const void* wcor, const void* cgroup_ext, const void* cosphm1_ext, int kijs, int kijl, int nd3s,
                               int nd3e, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws, double* wam2nemo, double delpro_lf,
                               int ifrelfmax, const void* gin, int gin_nfre, int flags, void* stream) {
  if (!c) return fail("null context");
  if (flags) return fail("ecwam_hip_propags2_implsch: unknown flags");
  if (!fused_ok(c) || !implsch4_adv_forms(c->NANG, c->real_bytes)) return fail("ecwam_hip_propags2_implsch: no one-kernel build covers the configuration (ecwam_hip_propags2_implsch_supported): call ecwam_hip_propags2_otf and ecwam_hip_implsch");
  if (kijl < kijs || kijs < 0 || kijl > n || nd3s < 1 || nd3e > c->NFRE_RED || nd3e < nd3s - 1) return fail("ecwam_hip_propags2_implsch: bad range");
  if (kijl > kijs && (!f1 || !f3 || !kxlt || !zdello || !cosph || !sinph || !klon || !klat || !kcor || !wlat || !wcor || !cgroup_ext || !cosphm1_ext ||
                      !wvprpt || !ff || !intf || !mij || !xllws))
    return fail("ecwam_hip_propags2_implsch: null pointer");
  if (f1 == f3) return fail("ecwam_hip_propags2_implsch: F1 and F3 must not alias (the neighbours of a point are read while other points are stored)");
  if (((uintptr_t)f1 % 16) != 0 || ((uintptr_t)f3 % 16) != 0) return fail("ecwam_hip_propags2_implsch: the spectra must be 16-byte aligned");
  // fast waves (propag_wam.F90:247-313): frequencies 1..ifrelfmax advance with delpro_lf and are read from the compact rows their sub-steps left
  if (ifrelfmax < 0 || ifrelfmax > c->NFRE_RED || (ifrelfmax > 0) != (gin != nullptr))
    return fail("ecwam_hip_propags2_implsch: fast waves (ifrelfmax > 0) come with their compact input rows (gin), and only then");
  if (gin && (nd3s != 1 || gin_nfre < ifrelfmax || gin_nfre > c->NFRE || gin_nfre % (16 / c->real_bytes) != 0 || ((uintptr_t)gin % 16) != 0 || gin == c->fast_g ||
              !(delpro_lf > 0.0)))
    return fail("ecwam_hip_propags2_implsch: the compact fast-wave rows must be 16-byte aligned, hold the fast waves in a multiple of 16 bytes per direction, and differ from the rows of ecwam_hip_set_fastwave_copy");
  if (c->p.lwnemocou && kijl > kijs && !wam2nemo) return fail("ecwam_hip_propags2_implsch: LWNEMOCOU needs the WAVE2OCEAN buffer");
  if (c->obs && kijl > c->n_obs) return fail("ecwam_hip_propags2_implsch: more points than the obstruction table holds");
  if (!c->p.lwnemocou) wam2nemo = nullptr;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  if (kijl == kijs) return 0;
  if (int rc2 = implsch_reserve_on(c, kijl, s)) return rc2;      // (also the tables of the weights: adv_reserve)
  const size_t dir_reals = (size_t)(6 * c->NANG + 4);      // [NANG][4], CMTODEG (+ 3 pad), [NANG][2] for the fast waves' time step
  int* dirI = reinterpret_cast<int*>(reinterpret_cast<char*>(c->adv_dir) + dir_reals * c->real_bytes);
  const double dlf = gin ? delpro_lf : 0.0;
  const AdvGeom g{kxlt, zdello, xdella, cosph, sinph, klon, klat, kcor, wlat, wcor, cgroup_ext, cosphm1_ext, ngy};
  in_precision(c, [&](auto t) { launch_ctu_prep<decltype(t)>(c->dtab, kijs, kijl, delpro, dlf, g, c->adv_pt, c->adv_dir, dirI, s); });
  Implsch4AdvArgs a;
  a.f_in = f1; a.klon = klon; a.klat = klat; a.kcor = kcor; a.cg = cgroup_ext; a.pt = c->adv_pt; a.dirT = c->adv_dir; a.dirI = dirI;
  a.xdella = xdella; a.delpro = delpro; a.m0 = nd3s - 1; a.m1 = nd3e;
  a.gin = gin; a.delpro_lf = dlf; a.gin_k = gin ? gin_nfre : 0; a.mlf = gin ? ifrelfmax : 0;
  a.obs = c->obs;      // ecwam_hip_set_obstructions (LSUBGRID)
  a.gfast = c->fast_g; a.gfast_k = c->fast_g ? c->fast_gk : 0;      // ecwam_hip_set_fastwave_copy, as for ecwam_hip_implsch
  const Implsch4Variant v = implsch4_variant(c);
  const int rc = in_precision(c, [&](auto t) {
    return launch_implsch4_adv<decltype(t)>(c->dtab, kijs, kijl, f3, wvprpt, ff, intf, mij, xllws, c->fin, wam2nemo, &a, c->NANG, c->NFRE, c->v4_r1, c->v4_r2,
                                            c->v4_nh, v, s);
  });
  if (rc != 0) return fail("ecwam_hip_propags2_implsch: no one-kernel build covers the configuration (the strict build of the weights has neither the fast-wave nor the obstruction form)");
  HIPCHK(hipGetLastError());
  c->implsch_last = 4;
  return 0;
}

int ecwam_hip_set_fastwave_copy(ecwam_hip_ctx* c, void* g, int g_nfre) {
  if (!c) return fail("null context");
  if (g && (g_nfre < 1 || g_nfre > c->NFRE || g_nfre % (16 / c->real_bytes) != 0 || ((uintptr_t)g % 16) != 0))
    return fail("ecwam_hip_set_fastwave_copy: the compact rows must be 16-byte aligned and hold a multiple of 16 bytes per direction");
  c->fast_g = g; c->fast_gk = g ? g_nfre : 0;
  return 0;
}

int ecwam_hip_implsch_reserve(ecwam_hip_ctx* c, int npts) {
  if (!c) return fail("ecwam_hip_implsch_reserve: null context");
  return implsch_reserve_on(c, npts, nullptr);
}

int ecwam_hip_implsch_generation_used(ecwam_hip_ctx* c) { return c ? c->implsch_last : 0; }

// The device copy of the module tables (DevTab<float> or DevTab<double>, csrc/dev.h): for diagnostics and for second implementations of a
// kernel that want to run on exactly the tables the product runs on (tests/csrc/implsch_v2.hip).
const void* ecwam_hip_device_tables(ecwam_hip_ctx* c) { return c ? c->dtab : nullptr; }

// the head and the tail the ecwam_hip_outbs* entry points share: null context, then the range; the launcher's refusal, then the launch's error
static int outbs_head(const ecwam_hip_ctx* c, int kijs, int kijl, const char* bad_range) {
  if (!c) return fail("null context");
  if (kijl < kijs || kijs < 0) return fail(bad_range);
  return 0;
}
static int outbs_tail(int rc, const char* unsupported) { return rc ? fail(unsupported) : launched(); }

int ecwam_hip_outbs(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, double zmiss, void* out, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outbs: bad range")) return 1;
  if (kijl > kijs && (!fl1 || !out)) return fail("ecwam_hip_outbs: null pointer");
  const int rc = in_precision(c, [&](auto t) { return launch_outbs<decltype(t)>(c->dtab, kijs, kijl, fl1, zmiss, out, c->NANG, c->NFRE, (hipStream_t)stream); });
  return outbs_tail(rc, "ecwam_hip_outbs: unsupported spectral size");
}

int ecwam_hip_outbs_sepwisw(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* xllws, const void* wvprpt, const void* ff, int flags,
                            double zmiss, void* out, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outbs_sepwisw: bad range")) return 1;
  if (kijl > kijs && (!fl1 || !xllws || !wvprpt || !ff || !out)) return fail("ecwam_hip_outbs_sepwisw: null pointer");
  if (flags & ~1) return fail("ecwam_hip_outbs_sepwisw: unknown flags");
  const int rc = in_precision(c, [&](auto t) { return launch_outbs_sepwisw<decltype(t)>(c->dtab, kijs, kijl, fl1, xllws, wvprpt, ff, flags, zmiss, out, c->NANG, c->NFRE, (hipStream_t)stream); });
  return outbs_tail(rc, "ecwam_hip_outbs_sepwisw: unsupported spectral size");
}

int ecwam_hip_outbs_partition(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* xllws, const int* mij, const void* wvprpt,
                              const void* ff, int flags, double zmiss, void* out, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outbs_partition: bad range")) return 1;
  if (kijl > kijs && (!fl1 || !xllws || !mij || !wvprpt || !ff || !out)) return fail("ecwam_hip_outbs_partition: null pointer");
  if (flags & 1)
    return fail("ecwam_hip_outbs_partition: CLDOMAIN = 's' (flags bit 0) is not supported: SEP3TR would read an FSEA that SEPWISW has not computed");
  if (flags) return fail("ecwam_hip_outbs_partition: unknown flags");
  const int rc = in_precision(c, [&](auto t) { return launch_outbs_partition<decltype(t)>(c->dtab, kijs, kijl, fl1, xllws, mij, wvprpt, ff, zmiss, out, c->NANG, c->NFRE, (hipStream_t)stream); });
  return outbs_tail(rc, "ecwam_hip_outbs_partition: unsupported spectral size");
}

int ecwam_hip_outbs_extremes(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* ff, int flags, void* out,
                             void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outbs_extremes: bad range")) return 1;
  if (kijl > kijs && (!fl1 || !wvprpt || !ff || !out)) return fail("ecwam_hip_outbs_extremes: null pointer");
  if (flags & ~1) return fail("ecwam_hip_outbs_extremes: unknown flags");
  const int rc = in_precision(c, [&](auto t) { return launch_outbs_extremes<decltype(t)>(c->dtab, kijs, kijl, fl1, wvprpt, ff, flags, out, c->NANG, c->NFRE, (hipStream_t)stream); });
  return outbs_tail(rc, "ecwam_hip_outbs_extremes: unsupported spectral size");
}

int ecwam_hip_outbs_absolute(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* ucur, const void* vcur,
                             const void* ff, int flags, double zmiss, void* out, void* fl2nd, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outbs_absolute: bad range")) return 1;
  if (flags) return fail("ecwam_hip_outbs_absolute: unknown flags");
  const bool intpol = c->p.irefra >= 2, ice = c->p.licerun && !c->p.lmaskice;
  if (kijl > kijs && (!fl1 || !out)) return fail("ecwam_hip_outbs_absolute: null pointer");
  if (kijl > kijs && intpol && (!wvprpt || !ucur || !vcur)) return fail("ecwam_hip_outbs_absolute: IREFRA = 2 / 3 needs wvprpt, ucur and vcur");
  if (kijl > kijs && ice && !ff) return fail("ecwam_hip_outbs_absolute: LICERUN without LMASKICE needs ff (CICOVER, WSWAVE)");
  if (fl2nd && fl2nd == fl1) return fail("ecwam_hip_outbs_absolute: FL1 and FL2ND must not alias");
  if (intpol && !c->itab) return fail("ecwam_hip_outbs_absolute: NFRE_MAX of INTPOL exceeds the library's table");
  hipStream_t s = (hipStream_t)stream;
  const int mode = (intpol ? 1 : 0) | (ice ? 2 : 0);
  const int rc = in_precision(c, [&](auto t) { return launch_outbs_absolute<decltype(t)>(c->dtab, c->itab, kijs, kijl, mode, fl1, wvprpt, ucur, vcur, ff, zmiss, out, fl2nd, c->NANG, c->NFRE, s); });
  return outbs_tail(rc, "ecwam_hip_outbs_absolute: unsupported spectral size");
}

int ecwam_hip_set_second_order(ecwam_hip_ctx* c, int ndepth, double deptha, double depthd, int nmax, const int* im_p, const int* im_m, const void* ta,
                               const void* tb, const void* tc_ql, const void* tt_4m, const void* tt_4p) {
  if (!c) return fail("null context");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  if (c->so_tab) (void)hipFree(c->so_tab);
  if (c->so_coef) (void)hipFree(c->so_coef);
  c->so_tab = c->so_coef = nullptr;
  c->so_nmax = 0;
  if (!ta) return 0;
  if (!im_p || !im_m || !tb || !tc_ql || !tt_4m || !tt_4p) return fail("ecwam_hip_set_second_order: null pointer");
  std::vector<unsigned char> h, hc;
  const char* why = so_tab_build(&c->p, c->fr_host.data(), c->real_bytes, ndepth, deptha, depthd, nmax, im_p, im_m, h);
  if (why) return fail((std::string("ecwam_hip_set_second_order: ") + why).c_str());
  const void* const src[5] = {ta, tb, tc_ql, tt_4m, tt_4p};
  so_coef_layout(c->real_bytes, ndepth, c->NANG / 2, c->NFRE / 2, src, hc);
  HIPCHK(hipMalloc(&c->so_tab, h.size()));
  HIPCHK(hipMemcpy(c->so_tab, h.data(), h.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&c->so_coef, hc.size()));
  HIPCHK(hipMemcpy(c->so_coef, hc.data(), hc.size(), hipMemcpyHostToDevice));
  c->so_nmax = nmax;
  return 0;
}

int ecwam_hip_outbs_second_order(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* depth, const void* ucur,
                                 const void* vcur, const void* ff, double sig, double zmiss, void* out, void* fl2nd, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outbs_second_order: bad range")) return 1;
  if (!c->so_tab || !c->so_coef) return fail("ecwam_hip_outbs_second_order: the second-order tables are not set (ecwam_hip_set_second_order)");
  const bool intpol = c->p.irefra >= 2, ice = c->p.licerun && !c->p.lmaskice;
  if (kijl > kijs && (!fl1 || !out || !wvprpt || !depth)) return fail("ecwam_hip_outbs_second_order: null pointer (fl1, wvprpt, depth and out are needed)");
  if (kijl > kijs && intpol && (!ucur || !vcur)) return fail("ecwam_hip_outbs_second_order: IREFRA = 2 / 3 needs ucur and vcur");
  if (kijl > kijs && ice && !ff) return fail("ecwam_hip_outbs_second_order: LICERUN without LMASKICE needs ff (CICOVER, WSWAVE)");
  if (fl2nd && fl2nd == fl1) return fail("ecwam_hip_outbs_second_order: FL1 and FL2ND must not alias");
  if (intpol && !c->itab) return fail("ecwam_hip_outbs_second_order: NFRE_MAX of INTPOL exceeds the library's table");
  if (!(sig == 1.0 || sig == -1.0)) return fail("ecwam_hip_outbs_second_order: SIG must be +1 or -1");
  if (kijl == kijs) return 0;
  hipStream_t s = (hipStream_t)stream;
  const size_t need = so_work_bytes(c->real_bytes, kijl - kijs, c->NANG / 2, c->NFRE / 2, c->so_nmax);
  if (need > c->so_work_bytes) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    if (c->so_work) (void)hipFree(c->so_work);
    c->so_work = nullptr; c->so_work_bytes = 0;
    HIPCHK(hipMalloc(&c->so_work, need));
    c->so_work_bytes = need;
  }
  const int mode = (intpol ? 1 : 0) | (ice ? 2 : 0);
  const int rc = in_precision(c, [&](auto t) {
    return launch_outbs_second_order<decltype(t)>(c->dtab, c->itab, c->so_tab, c->so_coef, c->so_work, c->so_nmax, kijs, kijl, mode, fl1, wvprpt, depth, ucur, vcur,
                                                  ff, sig, zmiss, out, fl2nd, c->NANG, c->NFRE, s);
  });
  return outbs_tail(rc, "ecwam_hip_outbs_second_order: unsupported spectral size (NANG must be 48, 36, 24 or 12)");
}

int ecwam_hip_set_outbs_integrals(ecwam_hip_ctx* c, double xkmss_cutoff, int nband, const double* tb, const double* tt, const void* delkcc_gc) {
  if (!c) return fail("null context");
  if (nband < 0 || nband > 8) return fail("ecwam_hip_set_outbs_integrals: nband must be 0 .. 8");
  if (!delkcc_gc || (nband && (!tb || !tt))) return fail("ecwam_hip_set_outbs_integrals: null pointer");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());   // no call in flight reads the table that is replaced
  std::vector<unsigned char> dt(outbs_devtab_bytes(c->real_bytes)), h;
  HIPCHK(hipMemcpy(dt.data(), c->dtab, dt.size(), hipMemcpyDeviceToHost));
  const char* why = outbs_int_tab_build(dt.data(), c->real_bytes, xkmss_cutoff, nband, tb, tt, delkcc_gc, h);
  if (why) return fail((std::string("ecwam_hip_set_outbs_integrals: ") + why).c_str());
  if (!c->int_tab) HIPCHK(hipMalloc(&c->int_tab, h.size()));
  HIPCHK(hipMemcpy(c->int_tab, h.data(), h.size(), hipMemcpyHostToDevice));
  c->int_nband = nband;
  c->int_tb.clear(); c->int_tt.clear();
  if (nband) { c->int_tb.assign(tb, tb + nband); c->int_tt.assign(tt, tt + nband); }
  return 0;
}

int ecwam_hip_outbs_integrals(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* fl2nd, const void* wvprpt, const void* ff, int flags,
                              double zmiss, void* out, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outbs_integrals: bad range")) return 1;
  if (flags & ~63) return fail("ecwam_hip_outbs_integrals: unknown flags");
  if (c->int_nband < 0) return fail("ecwam_hip_outbs_integrals: the cut-off and the bands are not set (ecwam_hip_set_outbs_integrals)");
  if ((flags & 16) && c->int_nband == 0) return fail("ecwam_hip_outbs_integrals: the band group is selected but no band is set (nband = 0)");
  if (c->NANG != 48 && c->NANG != 36 && c->NANG != 24 && c->NANG != 12) return fail("ecwam_hip_outbs_integrals: no build for this NANG (48, 36, 24 and 12 are built)");
  if (kijl > kijs && !out) return fail("ecwam_hip_outbs_integrals: null pointer");
  if (kijl > kijs && (flags & (1 | 2 | 4 | 8)) && (!fl1 || !wvprpt || !ff)) return fail("ecwam_hip_outbs_integrals: the readers of FL1 need fl1, wvprpt and ff");
  if (kijl > kijs && (flags & 32) && !ff) return fail("ecwam_hip_outbs_integrals: the point-wise group needs ff");
  if (kijl > kijs && (flags & 16) && !fl1 && !fl2nd) return fail("ecwam_hip_outbs_integrals: the bands need fl2nd or fl1");
  if (!fl2nd) fl2nd = fl1;
  if (!fl1) fl1 = fl2nd;   // bands only: the one row that is read
  const int rc = in_precision(c, [&](auto t) { return launch_outbs_integrals<decltype(t)>(c->dtab, c->int_tab, kijs, kijl, fl1, fl2nd, wvprpt, ff, flags, zmiss, out, c->NANG, c->NFRE, (hipStream_t)stream); });
  return outbs_tail(rc, "ecwam_hip_outbs_integrals: unsupported spectral size");
}

int ecwam_hip_outsetwmask(ecwam_hip_ctx* c, int kijs, int kijl, void* out, int ncol, const int* colflags, const void* ff, const int* iodp, double cithrsh,
                          double zmiss, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outsetwmask: bad range")) return 1;
  if (ncol < 1 || ncol > 64) return fail("ecwam_hip_outsetwmask: ncol must be 1 .. 64");
  if (!colflags || (kijl > kijs && !out)) return fail("ecwam_hip_outsetwmask: null pointer");
  OutMaskCols cols;
  int any = 0;
  for (int i = 0; i < 64; i++) cols.f[i] = 0;
  for (int i = 0; i < ncol; i++) {
    if (colflags[i] & ~3) return fail("ecwam_hip_outsetwmask: unknown column flags");
    cols.f[i] = (unsigned char)colflags[i];
    any |= colflags[i];
  }
  const int ice = c->p.licerun != 0;   // LICERUN .AND. LLSOURCE: the library integrates the source terms
  if (kijl > kijs && (any & 2) && !iodp) return fail("ecwam_hip_outsetwmask: a column has the sea mask but iodp is NULL");
  if (kijl > kijs && ice && (any & 1) && !ff) return fail("ecwam_hip_outsetwmask: the sea-ice mask needs ff (CICOVER)");
  in_precision(c, [&](auto t) { launch_outsetwmask<decltype(t)>(kijs, kijl, out, ncol, cols, ff, iodp, ice, cithrsh, zmiss, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_set_outblock(ecwam_hip_ctx* c, int jppflag, const int* ipfgtbl, const int* itobout, const int* icemask, const int* seamask, int niprmout, int flags) {
  if (!c) return fail("null context");
  double fr1 = 0.0;
  in_precision(c, [&](auto t) { fr1 = (double)((const decltype(t)*)c->fr_host.data())[0]; });
  const OutblockCtx oc{c->NANG, c->NFRE, c->real_bytes, c->p.irefra, c->p.licerun, c->p.lmaskice, c->p.lwnemocoustrn, c->so_tab && c->so_coef, c->itab != nullptr,
                       c->int_nband, c->int_tb.data(), c->int_tt.data(), fr1};
  OutblockPlan plan;
  const std::string why = outblock_plan_build(oc, jppflag, ipfgtbl, itobout, icemask, seamask, niprmout, flags, plan);
  if (!why.empty()) return fail("ecwam_hip_set_outblock: " + why);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());   // no call in flight reads the descriptors that are replaced
  c->ob_set = false;
  if (c->ob_desc) (void)hipFree(c->ob_desc);
  c->ob_desc = nullptr;
  HIPCHK(hipMalloc(&c->ob_desc, plan.desc.size() * sizeof(int)));
  HIPCHK(hipMemcpy(c->ob_desc, plan.desc.data(), plan.desc.size() * sizeof(int), hipMemcpyHostToDevice));
  c->ob_plan = plan;
  c->ob_set = true;
  return 0;
}

int ecwam_hip_outblock_plan(ecwam_hip_ctx* c, int* calls, int* stores_fl2nd) {
  if (!c) return fail("null context");
  if (!c->ob_set) return fail("ecwam_hip_outblock_plan: no plan (ecwam_hip_set_outblock)");
  if (calls) *calls = c->ob_plan.calls | (c->ob_plan.int_groups << 8) | (c->ob_plan.ext_full << 14);
  if (stores_fl2nd) *stores_fl2nd = c->ob_plan.stores_fl2nd;
  return 0;
}

int ecwam_hip_outblock(ecwam_hip_ctx* c, int kijs, int kijl, const void* fl1, const void* xllws, const int* mij, const void* wvprpt, const void* ff, const void* intf,
                       const void* ucur, const void* vcur, const int* iodp, const void* ibrmem, const void* altim, const double* nemo, double cithrsh, double zmiss,
                       void* bout, void* stream) {
  if (outbs_head(c, kijs, kijl, "ecwam_hip_outblock: bad range")) return 1;
  if (!c->ob_set) return fail("ecwam_hip_outblock: no plan: call ecwam_hip_set_outblock first");
  const OutblockPlan& P = c->ob_plan;
  if (kijl == kijs) return 0;
  if (!bout) return fail("ecwam_hip_outblock: bout is NULL");
  {   // every array the plan reads, before anything is launched
    static const char* const name[12] = {"fl1", "xllws", "mij", "wvprpt", "ff", "intf", "ucur", "vcur", "iodp", "ibrmem", "altim", "nemo"};
    const void* const ptr[12] = {fl1, xllws, mij, wvprpt, ff, intf, ucur, vcur, iodp, ibrmem, altim, nemo};
    for (int b = 0; b < 12; b++)
      if ((P.need >> b & 1) && !ptr[b])
        return fail(std::string("ecwam_hip_outblock: ") + name[b] + " is NULL but parameter " + std::to_string(P.why_param[b]) + " is requested and reads it");
  }
  // the state the plan was derived from must still be there
  if ((P.calls & OB_CALL_SECOND_ORDER) && (!c->so_tab || !c->so_coef)) return fail("ecwam_hip_outblock: the second-order tables were removed after ecwam_hip_set_outblock");
  if ((P.calls & OB_CALL_INTEGRALS) && c->int_nband < 0) return fail("ecwam_hip_outblock: ecwam_hip_set_outbs_integrals not called");
  if ((P.int_groups & 16) && c->int_nband != 7) return fail("ecwam_hip_outblock: the bands were changed after ecwam_hip_set_outblock");
  hipStream_t s = (hipStream_t)stream;
  // work space: the packed rows of the calls, indexed by the absolute row as they write them; DEPTH for the second-order call; FL2ND when the bands read it
  const size_t rb = (size_t)c->real_bytes, n = (size_t)kijl;
  const int wint = 8 + (c->int_nband > 0 ? c->int_nband : 0);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o8 = 0, osep = o8 + up(n * 8 * rb), oext = osep + up(n * 24 * rb), oint = oext + up(n * 13 * rb), odep = oint + up(n * wint * rb),
               ofl = odep + ((P.calls & OB_CALL_SECOND_ORDER) ? up(n * rb) : 0), need = ofl + (P.stores_fl2nd ? up(n * c->NANG * c->NFRE * rb) : 0);
  if (need > c->ob_work_bytes) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    if (c->ob_work) (void)hipFree(c->ob_work);
    c->ob_work = nullptr; c->ob_work_bytes = 0;
    HIPCHK(hipMalloc(&c->ob_work, need));
    c->ob_work_bytes = need;
  }
  char* w = (char*)c->ob_work;
  void *w8 = w + o8, *wsep = w + osep, *wext = w + oext, *wi = w + oint, *wdep = w + odep, *wfl = P.stores_fl2nd ? w + ofl : nullptr;
  if (P.calls & OB_CALL_OUTBS)
    if (ecwam_hip_outbs(c, kijs, kijl, fl1, zmiss, w8, stream)) return 1;
  if (P.calls & OB_CALL_ABSOLUTE)
    if (ecwam_hip_outbs_absolute(c, kijs, kijl, fl1, wvprpt, ucur, vcur, ff, 0, zmiss, w8, wfl, stream)) return 1;
  if (P.calls & OB_CALL_SECOND_ORDER) {
    in_precision(c, [&](auto t) { launch_outblock_depth<decltype(t)>(kijs, kijl, ff, wdep, s); });
    if (ecwam_hip_outbs_second_order(c, kijs, kijl, fl1, wvprpt, wdep, ucur, vcur, ff, 1.0, zmiss, w8, wfl, stream)) return 1;
  }
  if (P.calls & OB_CALL_SEPWISW)
    if (ecwam_hip_outbs_sepwisw(c, kijs, kijl, fl1, xllws, wvprpt, ff, (P.flags & 2) ? 1 : 0, zmiss, wsep, stream)) return 1;
  if (P.calls & OB_CALL_PARTITION)
    if (ecwam_hip_outbs_partition(c, kijs, kijl, fl1, xllws, mij, wvprpt, ff, 0, zmiss, wsep, stream)) return 1;
  if (P.calls & OB_CALL_EXTREMES)
    if (ecwam_hip_outbs_extremes(c, kijs, kijl, fl1, wvprpt, ff, P.ext_full ? 0 : 1, wext, stream)) return 1;
  if (P.calls & OB_CALL_INTEGRALS)
    if (ecwam_hip_outbs_integrals(c, kijs, kijl, fl1, wfl, wvprpt, ff, P.int_groups, zmiss, wi, stream)) return 1;
  OutblockSrc src;
  for (int i = 0; i < OB_NSRC; i++) { src.base[i] = nullptr; src.pstride[i] = 0; src.cstride[i] = 0; }
  auto rows = [&](int i, const void* b, int width) { src.base[i] = b; src.pstride[i] = width; src.cstride[i] = 1; };
  auto planes = [&](int i, const void* b) { src.base[i] = b; src.pstride[i] = 1; src.cstride[i] = kijl; };
  rows(OB_W8, w8, P.w8_stride); rows(OB_SEP, wsep, P.sep_stride); rows(OB_EXT, wext, 13); rows(OB_INT, wi, wint);
  rows(OB_FF, ff, ECWAM_HIP_NFF); rows(OB_INTF, intf, ECWAM_HIP_NINTF); rows(OB_UCUR, ucur, 1); rows(OB_VCUR, vcur, 1); rows(OB_IBRMEM, ibrmem, 1);
  planes(OB_ALTIM, altim); planes(OB_NEMO, nemo);
  in_precision(c, [&](auto t) { launch_outblock_assemble<decltype(t)>(kijs, kijl, P.niprmout, c->ob_desc, src, ff, iodp, P.ice, P.sea, P.need_ci, cithrsh, zmiss, bout, s); });
  return launched();
}

int ecwam_hip_outwnorm(ecwam_hip_ctx* c, const void* field, int stride, int n, double zmiss, double* result, void* stream) {
  if (!c) return fail("null context");
  if (n < 0 || stride < 1 || !result || (n > 0 && !field)) return fail("ecwam_hip_outwnorm: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int nb = 256;
  HIPCHK(hipSetDevice(c->device));
  if (!c->norm_scratch) HIPCHK(hipMalloc(&c->norm_scratch, (size_t)(4 + 4 * nb) * sizeof(double)));
  double* scratch = c->norm_scratch;
  in_precision(c, [&](auto t) { launch_norm<decltype(t)>(field, stride, n, zmiss, scratch, nb, s); });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(result, scratch, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int ecwam_hip_newwind_icode(ecwam_hip_ctx* c, int n, void* ff, const void* ff_next, int icode_wnd, void* stream) {
  if (!c) return fail("null context");
  if (n > 0 && (!ff || !ff_next)) return fail("ecwam_hip_newwind: null pointer");
  if (icode_wnd < 1 || icode_wnd > 3) return fail("ecwam_hip_newwind: ICODE_WND must be 1, 2 or 3");
  in_precision(c, [&](auto t) { launch_newwind<decltype(t)>(c->dtab, n, ff, ff_next, icode_wnd, (hipStream_t)stream); });
  return launched();
}
int ecwam_hip_newwind(ecwam_hip_ctx* c, int n, void* ff, const void* ff_next, void* stream) {
  if (!c) return fail("null context");
  return ecwam_hip_newwind_icode(c, n, ff, ff_next, c->p.icode, stream);
}

int ecwam_hip_nosource(ecwam_hip_ctx* c, int kijs, int kijl, void* fl1, int* mij, void* xllws, void* stream) {
  if (!c) return fail("null context");
  if (kijs < 0 || kijl < kijs) return fail("ecwam_hip_nosource: bad range");
  if (kijl > kijs && (!mij || !xllws)) return fail("ecwam_hip_nosource: null pointer");
  hipStream_t s = (hipStream_t)stream;
  in_precision(c, [&](auto t) { launch_nosource<decltype(t)>(c->dtab, kijs, kijl, c->NANG * c->NFRE, fl1, xllws, mij, s); });
  HIPCHK(hipGetLastError());
  if (c->fast_g && fl1 && kijl > kijs) { fastwave_copy(c, fl1, kijs, kijl, s); HIPCHK(hipGetLastError()); }
  return 0;
}

int ecwam_hip_host_register(ecwam_hip_ctx* c, void* host, unsigned long long bytes) {
  if (!c || !host) return fail("ecwam_hip_host_register: null argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipHostRegister(host, bytes, hipHostRegisterDefault));
  return 0;
}
int ecwam_hip_host_unregister(ecwam_hip_ctx* c, void* host) {
  if (!c || !host) return fail("ecwam_hip_host_unregister: null argument");
  HIPCHK(hipHostUnregister(host));
  return 0;
}

int ecwam_hip_chunks_to_points(ecwam_hip_ctx* c, const void* chunked, void* points, int nproma, int nchnk, int npts, int n2, int n3, void* stream) {
  if (!c) return fail("null context");
  if (nproma < 1 || nchnk < 0 || npts > nproma * nchnk || n2 < 1 || n3 < 1) return fail("ecwam_hip_chunks_to_points: bad shape");
  in_precision(c, [&](auto t) { launch_c2p<decltype(t)>(chunked, points, nproma, nchnk, npts, n2, n3, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_points_to_chunks(ecwam_hip_ctx* c, const void* points, void* chunked, int nproma, int nchnk, int npts, int n2, int n3, void* stream) {
  if (!c) return fail("null context");
  if (nproma < 1 || nchnk < 0 || npts > nproma * nchnk || npts <= nproma * (nchnk - 1) || n2 < 1 || n3 < 1) return fail("ecwam_hip_points_to_chunks: bad shape");
  in_precision(c, [&](auto t) { launch_p2c<decltype(t)>(points, chunked, nproma, nchnk, npts, n2, n3, (hipStream_t)stream); });
  return launched();
}

static int member_args(const char* who, int nproma, int nchnk, int npts, int nm, long long row_stride, long long row_off, int elem_bytes,
                       const void* a, const void* b) {
  if (nproma < 1 || nchnk < 0 || npts < 0 || npts > nproma * nchnk || (npts > 0 && npts <= nproma * (nchnk - 1)) || nm < 1 || row_off < 0 ||
      row_off + nm > row_stride || (elem_bytes != 4 && elem_bytes != 8))
    return fail(std::string(who) + ": bad shape");
  if (npts > 0 && (!a || !b)) return fail(std::string(who) + ": null pointer");
  return 0;
}

int ecwam_hip_member_scatter(ecwam_hip_ctx* c, const void* chunked, void* rows, int nproma, int nchnk, int npts, int nm, long long row_stride,
                             long long row_off, int elem_bytes, void* stream) {
  if (!c) return fail("null context");
  if (member_args("ecwam_hip_member_scatter", nproma, nchnk, npts, nm, row_stride, row_off, elem_bytes, chunked, rows)) return 1;
  if (npts == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)npts * nm;
  const int nb = (int)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
  if (elem_bytes == 4)
    hipLaunchKernelGGL(k_member_scatter<unsigned int>, dim3(nb), dim3(256), 0, s, (const unsigned int*)chunked, (unsigned int*)rows, nproma, npts, nm, row_stride, row_off);
  else
    hipLaunchKernelGGL(k_member_scatter<unsigned long long>, dim3(nb), dim3(256), 0, s, (const unsigned long long*)chunked, (unsigned long long*)rows, nproma, npts, nm, row_stride, row_off);
  return launched();
}

int ecwam_hip_member_gather(ecwam_hip_ctx* c, const void* rows, void* chunked, int nproma, int nchnk, int npts, int nm, long long row_stride,
                            long long row_off, int elem_bytes, void* stream) {
  if (!c) return fail("null context");
  if (member_args("ecwam_hip_member_gather", nproma, nchnk, npts, nm, row_stride, row_off, elem_bytes, rows, chunked)) return 1;
  if (npts == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)nchnk * nproma * nm;
  const int nb = (int)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
  if (elem_bytes == 4)
    hipLaunchKernelGGL(k_member_gather<unsigned int>, dim3(nb), dim3(256), 0, s, (const unsigned int*)rows, (unsigned int*)chunked, nproma, nchnk, npts, nm, row_stride, row_off);
  else
    hipLaunchKernelGGL(k_member_gather<unsigned long long>, dim3(nb), dim3(256), 0, s, (const unsigned long long*)rows, (unsigned long long*)chunked, nproma, nchnk, npts, nm, row_stride, row_off);
  return launched();
}

int ecwam_hip_pack_rows(ecwam_hip_ctx* c, const void* fl, const int* idx, int n, void* buf, void* stream) {
  if (!c) return fail("null context");
  if (n > 0 && (!fl || !idx || !buf)) return fail("ecwam_hip_pack_rows: null pointer");
  const int rowlen = c->NANG * c->NFRE;
  in_precision(c, [&](auto t) { launch_pack<decltype(t)>(fl, idx, n, rowlen, buf, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_unpack_rows(ecwam_hip_ctx* c, const void* buf, int n, void* fl, int dst0, void* stream) {
  if (!c) return fail("null context");
  if (n > 0 && (!fl || !buf)) return fail("ecwam_hip_unpack_rows: null pointer");
  if (n <= 0) return 0;
  const size_t row = (size_t)c->NANG * c->NFRE * c->real_bytes;
  HIPCHK(hipMemcpyAsync((char*)fl + (size_t)dst0 * row, buf, (size_t)n * row, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// ---- MPEXCHNG inside the library (mpexchng.F90:141-231) -----------------------------------------------------------------------------
int ecwam_hip_halo_setup(ecwam_hip_ctx* c, int rank, int nranks, int npeers, const int* peer, const int* send_count, const int* send_idx,
                         const int* recv_dst0, const int* recv_count) {
  if (!c) return fail("null context");
  if (nranks < 1 || rank < 0 || rank >= nranks || npeers < 0 || (npeers > 0 && (!peer || !send_count || !recv_dst0 || !recv_count)))
    return fail("ecwam_hip_halo_setup: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  if (c->d_send_idx) { (void)hipFree(c->d_send_idx); c->d_send_idx = nullptr; }
  c->rank = rank; c->nranks = nranks;
  c->peer.assign(peer, peer + npeers); c->send_cnt.assign(send_count, send_count + npeers);
  c->recv_dst0.assign(recv_dst0, recv_dst0 + npeers); c->recv_cnt.assign(recv_count, recv_count + npeers);
  c->send_off.resize(npeers);
  c->n_send = 0; c->n_recv = 0;
  for (int i = 0; i < npeers; i++) {
    // (peer[i] == rank is accepted: an exchange of a rank with itself -- rows that are their owner's own halo, e.g. a band that wraps
    //  around; RCCL pairs a send and a receive of the same rank inside one group)
    if (peer[i] < 0 || peer[i] >= nranks || send_count[i] < 0 || recv_count[i] < 0 || recv_dst0[i] < 0)
      return fail("ecwam_hip_halo_setup: bad peer entry");
    c->send_off[i] = c->n_send; c->n_send += send_count[i]; c->n_recv += recv_count[i];
  }
  if (c->n_send > 0) {
    if (!send_idx) return fail("ecwam_hip_halo_setup: send_idx missing");
    HIPCHK(hipMalloc(&c->d_send_idx, (size_t)c->n_send * sizeof(int)));
    HIPCHK(hipMemcpy(c->d_send_idx, send_idx, (size_t)c->n_send * sizeof(int), hipMemcpyHostToDevice));
  }
  if (!c->comm_stream) HIPCHK(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  return 0;
}

int ecwam_hip_proenvhalo_pack(ecwam_hip_ctx* c, int n, const void* wvprpt, const void* omosnh2kd, const void* depth, const void* ucur, const void* vcur,
                              void* buffer_ext, void* stream) {
  if (!c) return fail("null context");
  if (n < 0 || (n > 0 && (!wvprpt || !omosnh2kd || !depth || !ucur || !vcur || !buffer_ext))) return fail("ecwam_hip_proenvhalo_pack: bad arguments");
  in_precision(c, [&](auto t) { launch_proenv_pack<decltype(t)>(n, c->NFRE, wvprpt, omosnh2kd, depth, ucur, vcur, buffer_ext, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_proenvhalo_unpack(ecwam_hip_ctx* c, int nrows, const void* buffer_ext, const void* land, void* wavnum_ext, void* cgroup_ext,
                                void* omosnh2kd_ext, void* depth_ext, void* u_ext, void* v_ext, void* stream) {
  if (!c) return fail("null context");
  if (nrows < 0 || !buffer_ext || !land || !wavnum_ext || !cgroup_ext || !omosnh2kd_ext || !depth_ext || !u_ext || !v_ext)
    return fail("ecwam_hip_proenvhalo_unpack: bad arguments");
  in_precision(c, [&](auto t) { launch_proenv_unpack<decltype(t)>(nrows, c->NFRE, buffer_ext, land, wavnum_ext, cgroup_ext, omosnh2kd_ext, depth_ext, u_ext, v_ext, (hipStream_t)stream); });
  return launched();
}

int ecwam_hip_halo_counts(ecwam_hip_ctx* c, int* n_send, int* n_recv) {
  if (!c || !n_send || !n_recv) return fail("ecwam_hip_halo_counts: null argument");
  *n_send = c->n_send; *n_recv = c->n_recv;
  return 0;
}

int ecwam_hip_comm_unique_id(void* id128) {
  if (!id128) return fail("ecwam_hip_comm_unique_id: null argument");
  if (rccl_load()) return 1;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId");
  NCCLCHK(g_rccl.GetUniqueId((ncclUniqueId*)id128));
  return 0;
}

int ecwam_hip_comm_init(ecwam_hip_ctx* c, const void* id128) {
  if (!c || !id128) return fail("ecwam_hip_comm_init: null argument");
  // ncclCommInitRank is collective over all nranks: a rank of a multi-rank run joins even when it has no halo peer (a band that is an
  // enclosed basin), or the others would wait for it; only the single rank without a self exchange needs no communicator
  if (c->nranks < 2 && c->peer.empty()) return 0;
  if (rccl_load()) return 1;
  HIPCHK(hipSetDevice(c->device));
  if (c->comm) {   // a second initialisation replaces the communicator: let the posted exchange finish, then release the old one
    if (c->comm_stream) HIPCHK(hipStreamSynchronize(c->comm_stream));
    (void)g_rccl.CommDestroy(c->comm);
    c->comm = nullptr;
    for (auto& q : c->slot) q.used = q.pending = false;
  }
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  NCCLCHK(g_rccl.CommInitRank(&c->comm, c->nranks, id, c->rank));
  return 0;
}

int ecwam_hip_comm_count(ecwam_hip_ctx* c, int* nranks) {
  if (!c || !nranks) return fail("ecwam_hip_comm_count: null argument");
  *nranks = 0;
  if (!c->comm) return 0;
  NCCLCHK(g_rccl.CommCount(c->comm, nranks));
  return 0;
}

// the send buffer for rows of `rowlen` reals: the slot already serving that length, else a free one, else the least recently used
// (whose outstanding sends the caller then waits for, as for any reuse)
static ecwam_hip_ctx::HaloSlot* halo_slot(ecwam_hip_ctx* c, int rowlen) {
  ecwam_hip_ctx::HaloSlot* q = nullptr;
  for (auto& x : c->slot) if (x.rowlen == rowlen) { q = &x; break; }
  if (!q) for (auto& x : c->slot) if (x.rowlen == 0) { q = &x; break; }
  if (!q) { q = &c->slot[0]; for (auto& x : c->slot) if (x.age < q->age) q = &x; }
  q->rowlen = rowlen; q->age = ++c->slot_clock;
  return q;
}

static int halo_pack(ecwam_hip_ctx* c, ecwam_hip_ctx::HaloSlot* q, const void* fl, int rowlen, hipStream_t s) {
  const size_t need = (size_t)c->n_send * rowlen * c->real_bytes;
  if (!q->ev_packed) {
    HIPCHK(hipEventCreateWithFlags(&q->ev_packed, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&q->ev_done, hipEventDisableTiming));
  }
  // the buffer is reused: the sends of the exchange posted from it before must have read it before this pack overwrites it
  if (q->used) HIPCHK(hipStreamWaitEvent(s, q->ev_done, 0));
  if (need > q->bytes) {
    if (q->buf) HIPCHK(hipFree(q->buf));      // (hipFree waits for the device)
    q->buf = nullptr; q->bytes = 0;
    HIPCHK(hipMalloc(&q->buf, need));
    q->bytes = need;
  }
  if (c->n_send > 0) {
    in_precision(c, [&](auto t) { launch_pack<decltype(t)>(fl, c->d_send_idx, c->n_send, rowlen, q->buf, s); });
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int ecwam_hip_halo_start(ecwam_hip_ctx* c, void* fl, int rowlen, void* stream) {
  if (!c) return fail("null context");
  if (c->peer.empty()) return 0;
  if (!fl || rowlen < 1) return fail("ecwam_hip_halo_start: bad arguments");
  if (!c->comm) return fail("ecwam_hip_halo_start: no communicator (ecwam_hip_comm_init)");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(c->device));
  ecwam_hip_ctx::HaloSlot* q = halo_slot(c, rowlen);
  if (halo_pack(c, q, fl, rowlen, s)) return 1;
  HIPCHK(hipEventRecord(q->ev_packed, s));                     // everything enqueued on `stream` so far, the pack included
  HIPCHK(hipStreamWaitEvent(c->comm_stream, q->ev_packed, 0));
  const size_t rb = (size_t)rowlen * c->real_bytes;
  NCCLCHK(g_rccl.GroupStart());
  for (size_t i = 0; i < c->peer.size(); i++) {
    if (c->send_cnt[i] > 0)
      NCCLCHK(g_rccl.Send((const char*)q->buf + (size_t)c->send_off[i] * rb, (size_t)c->send_cnt[i] * rb, ncclChar, c->peer[i], c->comm, c->comm_stream));
    if (c->recv_cnt[i] > 0)
      NCCLCHK(g_rccl.Recv((char*)fl + (size_t)c->recv_dst0[i] * rb, (size_t)c->recv_cnt[i] * rb, ncclChar, c->peer[i], c->comm, c->comm_stream));
  }
  NCCLCHK(g_rccl.GroupEnd());
  HIPCHK(hipEventRecord(q->ev_done, c->comm_stream));
  q->used = q->pending = true;
  return 0;
}

// every exchange posted and not yet waited for: `stream` continues behind all of them
int ecwam_hip_halo_finish(ecwam_hip_ctx* c, void* stream) {
  if (!c) return fail("null context");
  if (c->peer.empty()) return 0;
  for (auto& q : c->slot)
    if (q.pending) {
      HIPCHK(hipStreamWaitEvent((hipStream_t)stream, q.ev_done, 0));
      q.pending = false;
    }
  return 0;
}

int ecwam_hip_halo_pack_host(ecwam_hip_ctx* c, const void* fl, int rowlen, void* host_send, void* stream) {
  if (!c) return fail("null context");
  if (c->n_send == 0) return 0;
  if (!fl || !host_send || rowlen < 1) return fail("ecwam_hip_halo_pack_host: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(c->device));
  ecwam_hip_ctx::HaloSlot* q = halo_slot(c, rowlen);
  if (halo_pack(c, q, fl, rowlen, s)) return 1;
  HIPCHK(hipMemcpyAsync(host_send, q->buf, (size_t)c->n_send * rowlen * c->real_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int ecwam_hip_halo_unpack_host(ecwam_hip_ctx* c, void* fl, int rowlen, const void* host_recv, void* stream) {
  if (!c) return fail("null context");
  if (c->n_recv == 0) return 0;
  if (!fl || !host_recv || rowlen < 1) return fail("ecwam_hip_halo_unpack_host: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const size_t rb = (size_t)rowlen * c->real_bytes;
  size_t off = 0;
  for (size_t i = 0; i < c->peer.size(); i++) {
    if (c->recv_cnt[i] > 0)
      HIPCHK(hipMemcpyAsync((char*)fl + (size_t)c->recv_dst0[i] * rb, (const char*)host_recv + off, (size_t)c->recv_cnt[i] * rb, hipMemcpyHostToDevice, s));
    off += (size_t)c->recv_cnt[i] * rb;
  }
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int ecwam_hip_malloc(ecwam_hip_ctx* c, unsigned long long bytes, void** dptr) {
  if (!c || !dptr) return fail("ecwam_hip_malloc: null argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMalloc(dptr, bytes ? bytes : 1));
  return 0;
}
int ecwam_hip_free(ecwam_hip_ctx* c, void* dptr) {
  if (!c) return fail("null context");
  if (dptr) HIPCHK(hipFree(dptr));
  return 0;
}
int ecwam_hip_memcpy_h2d(ecwam_hip_ctx* c, void* dst, const void* src, unsigned long long bytes, void* stream) {
  if (!c || (bytes && (!dst || !src))) return fail("ecwam_hip_memcpy_h2d: null argument");
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return 0;
}
int ecwam_hip_memcpy_d2h(ecwam_hip_ctx* c, void* dst, const void* src, unsigned long long bytes, void* stream) {
  if (!c || (bytes && (!dst || !src))) return fail("ecwam_hip_memcpy_d2h: null argument");
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return 0;
}
int ecwam_hip_memset(ecwam_hip_ctx* c, void* dst, int value, unsigned long long bytes, void* stream) {
  if (!c || (bytes && !dst)) return fail("ecwam_hip_memset: null argument");
  HIPCHK(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
  return 0;
}
int ecwam_hip_sync(ecwam_hip_ctx* c, void* stream) {
  if (!c) return fail("null context");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
int ecwam_hip_queue_create(ecwam_hip_ctx* c, void** queue) {
  if (!c || !queue) return fail("ecwam_hip_queue_create: null argument");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *queue = (void*)s;
  return 0;
}
int ecwam_hip_queue_destroy(ecwam_hip_ctx* c, void* queue) {
  if (!c) return fail("null context");
  if (queue) HIPCHK(hipStreamDestroy((hipStream_t)queue));
  return 0;
}
int ecwam_hip_queue_wait_for(ecwam_hip_ctx* c, void* waiter, void* waited) {
  if (!c) return fail("null context");
  if (waiter == waited) return 0;
  hipEvent_t e;
  HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e, (hipStream_t)waited));
  HIPCHK(hipStreamWaitEvent((hipStream_t)waiter, e, 0));
  HIPCHK(hipEventDestroy(e));   // released once the recorded work has completed
  return 0;
}

}  // extern "C"
