// The host launchers of the kernels, and the table builders beside them, that capi.hip calls: declared here once, with their parameter
// names.  capi.hip includes this file and so does every file that defines one of them; the explicit instantiations at the end of those files
// spell these signatures, so a definition that drifts from its declaration does not compile.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/ecwam_hip_forcing.h"
#include "../../include/ecwam_hip_intake.h"
#include "../../include/ecwam_hip_readwind.h"
#include "../../include/ecwam_hip_restart.h"
#include "../../include/ecwam_hip_gribin.h"
#include "../../include/ecwam_hip_propags.h"
#include "../../include/ecwam_hipx_propags1.h"
#include "../../include/ecwam_hip_gribout.h"
#include "implsch_adv_args.h"

// The grid geometry the advection kernels form the CTU weights from, in the untyped form and the order of the C interface's arguments
// (ecwam_hip_ctuw, ecwam_hip_propags2_otf ...).  An entry point that does not have one of them leaves it NULL / 0.
struct AdvGeom {
  const int* kxlt;
  const void* zdello;
  double xdella;
  const void *cosph, *sinph;
  const int *klon, *klat, *kcor;
  const void *wlat, *wcor;      // read by every kernel but CTUWINI (launch_ctuw), which fills them
  const void *cgroup_ext, *cosphm1_ext;
  int ngy;
};

// ---- propag.hip ----------------------------------------------------------------------------------------------------------------------
// dims = NANG << 16 | NFRE << 8 | NFRE_RED; [m0, m1) = the advected frequencies, 0-based
template <typename T> void launch_propags2(const void* tab, const void* f1, void* f3, const int* klon, const int* klat, const int* kcor, const void* w, int kijs, int kijl, int m0, int m1,
        int copy_rest, int dims, hipStream_t s);
template <typename T> void launch_ctuw(const void* tab, int n, int nland, double delpro, int m0, int m1, const AdvGeom& g, void* w, int* cflfail, int NANG, const void* obs, hipStream_t s);
template <typename T> void launch_ctuwini_only(int n, int nland, const int* klat, const int* kcor, void* wlat, void* wcor, hipStream_t s);
template <typename T> void launch_propdot(const void* tab, int n, int nland, int irefra, const AdvGeom& g, const void* depth, const void* ue, const void* ve, void* refr, hipStream_t s);
template <typename T> void launch_curmask(int n, int NANG, int slot, const int* cflfail, void* refr, hipStream_t s);
template <typename T> void launch_propags2_gen(const void* tab, int irefra, const void* f1, void* f3, double delpro, const AdvGeom& g, const void* om, const void* wn, const void* refr,
        int* cflfail, int slot, int kijs, int kijl, int m0, int m1, int copy_rest, int dims, const void* obs, hipStream_t s);
template <typename T> void launch_propags2_otf(const void* tab, const void* f1, void* f3, int n_geom, double delpro, const AdvGeom& g, const int* order, int kijs, int kijl, int m0,
        int m1, int copy_rest, int dims, const void* obs, int mlf, double delpro_lf, int in_k, void* gout, int gout_k, const void* gin, int gin_k, int out_k, hipStream_t s);
template <typename T> void launch_copy_freq_range(const void* src, void* dst, int n, int NANG, int NFRE, int m0, int m1, int dst_nfre, hipStream_t s);
template <typename T> void launch_newwind(const void* tab, int n, void* ff, const void* ffn, int icode_wnd, hipStream_t s);
template <typename T> void launch_ctu_prep(const void* tab, int kijs, int kijl, double delpro, double delpro_lf, const AdvGeom& g, void* pt, void* dirT, int* dirI, hipStream_t s);
template <typename T> void launch_nosource(const void* tab, int kijs, int kijl, int rowlen, void* fl1, void* xllws, int* mij, hipStream_t s);
template <typename T> void launch_c2p(const void* ch, void* pt, int nproma, int nchnk, int npts, int n2, int n3, hipStream_t s);
template <typename T> void launch_p2c(const void* pt, void* ch, int nproma, int nchnk, int npts, int n2, int n3, hipStream_t s);
template <typename T> void launch_pack(const void* fl, const int* idx, int n, int rowlen, void* buf, hipStream_t s);
template <typename T> void launch_proenv_pack(int n, int NFRE, const void* wvprpt, const void* om, const void* depth, const void* u, const void* v, void* buf, hipStream_t s);
template <typename T> void launch_proenv_unpack(int nrows, int NFRE, const void* buf, const void* land, void* wn, void* cg, void* om, void* dep, void* u, void* v, hipStream_t s);

// ---- propags.hip: the first-order scheme, IPROPAGS = 0 (include/ecwam_hip_propags.h).  launch_propags: 0 = launched (or nothing to do), 1 = the tile does not
// fit the LDS; f3 == nullptr: CHECKCFL alone -----------------------------------------------------------------------------------------------------------------
struct PropagsCall {
  const void *f1;
  void* f3;
  int nland, icase, irgg, irefra;
  double delpro, delphi;
  const int* kxlt;
  const void *cosph, *sinph, *dellam1, *cosphm1;
  const int *klon, *klat;
  const void *wlat, *cg, *om, *wn, *u, *v, *dot, *obs;
  int kijs, kijl, copy_rest;
  void* cfl;
  int* cflfail;
  int dp_product = 0;      // section 4 alone: DP1, DP2 = DCO(IJ) * (1 / DCO(JH)) as propags1.F90:203-222 forms them, in place of the quotient of PROPAGS
};
template <typename T> void launch_propags_dot(const void* tab, int n, int nland, int irefra, int icase, const AdvGeom& g, const void* depth, const void* ue, const void* ve, void* dot,
        hipStream_t s);
template <typename T> int launch_propags(const void* tab, const PropagsCall& c, int NFRE, hipStream_t s);

// ---- propags1.hip: the dual rotated-quadrant scheme, IPROPAGS = 1 (include/ecwam_hipx_propags1.h): section 3 of PROPAGS1.  The tables are those of
// ecwam_hipx_set_rotated: KRLAT, KRLON [n][2][2], WRLAT, WRLON [n][2], CDR, SDR [nrow][NANG], PRQRT [n].  Same return values as launch_propags ------------------
struct RotatedTables {
  int n = 0, nrow = 0;
  const int *krlat = nullptr, *krlon = nullptr;
  const void *wrlat = nullptr, *wrlon = nullptr, *cdr = nullptr, *sdr = nullptr, *prqrt = nullptr;
  double sqrt2 = 0;
};
template <typename T> int launch_propags1(const void* tab, const PropagsCall& c, const RotatedTables& r, int NANG, int NFRE, hipStream_t s);

// ---- implsch4.hip, implsch4x.hip, implsch4r.hip, implsch4a.hip, implsch4w.hip: the launchers of k_implsch4 (implsch_v4.h) ------------------------------
// The kernel is built at the spectral shapes of implsch_v4_shapes.h, in the variants below; one translation unit per group of variants (they
// compile side by side).  A context runs ONE variant, computed from its parameters in one place (capi.hip: implsch4_variant); every launcher
// takes it and returns 0 = launched, -1 = this unit has no build for the variant, the shape (NANG, r1, r2, nh) or the precision.
//   A, B                flag set A (LLGCBZ0 = F, LLNORMAGAM = F), flag set B (either or both T); IPHYS 1, ISNONLIN 0: implsch4.hip, implsch4a.hip, implsch4w.hip
//   iphys0, isnonlin1   IPHYS 0, ISNONLIN 1, each on flag set A: implsch4x.hip, implsch4w.hip
//   rare, rare_iphys0   every other switch, decided at run time inside the build, with IPHYS 1, with IPHYS 0: implsch4r.hip
enum class Implsch4Variant { A, B, iphys0, isnonlin1, rare, rare_iphys0 };
template <typename T> int launch_implsch4(const void* tab, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws, void* fin, double* w2n,
        void* gfast, int gk, void* wi, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s);
template <typename T> int launch_implsch4x(const void* tab, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws, void* fin, double* w2n,
        void* gfast, int gk, void* wi, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s);
template <typename T> int launch_implsch4r(const void* tab, int kijs, int kijl, void* fl1, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws, void* fin, double* w2n,
        void* gfast, int gk, void* wi, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s);
// the one-kernel step; the forms built for a direction count (bit 0 the plain step, bit 1 fast-wave sub-steps, bit 2 sub-grid obstructions)
template <typename T> int launch_implsch4_adv(const void* tab, int kijs, int kijl, void* fl_out, const void* wvprpt, void* ff, void* intf, int* mij, void* xllws, void* fin, double* w2n,
        const Implsch4AdvArgs* a, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s);
int implsch4_adv_forms(int NANG, int real_bytes);
// WDFLUXES, whether it is built for a direction count, and SETICE (0 = launched, -1 = not covered)
template <typename T> int launch_wdfluxes(const void* tab, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* ff, void* intf, int* mij, void* xllws, void* fin,
        double* w2n, int NANG, int NFRE, int r1, int r2, int nh, Implsch4Variant v, hipStream_t s);
bool wdfluxes_built(int NANG, int real_bytes);
template <typename T> int launch_setice(const void* tab, int kijs, int kijl, void* fl1, const void* ff, int NANG, int NFRE, hipStream_t s);
int implsch4_fin_row();

// ---- outbs*.hip: 0 = launched (or nothing to do), 1 = unsupported spectral size -------------------------------------------------------------
// the spectral sizes of the output kernels: four LDS tiles [NFRE][NANG | 1] within 64 KiB, a direction per lane, a frequency per mask bit
inline bool outbs_size_ok(int NANG, int NFRE, size_t real_bytes) {
  return (size_t)4 * NFRE * (NANG | 1) * real_bytes <= 64 * 1024 && NANG <= 64 && NFRE <= 63;
}
template <typename T> int launch_outbs(const void* tab, int kijs, int kijl, const void* fl1, double zmiss, void* out, int NANG, int NFRE, hipStream_t s);
template <typename T> void launch_norm(const void* f, int stride, int n, double zmiss, double* scratch, int nb, hipStream_t s);
template <typename T> int launch_outbs_sepwisw(const void* tab, int kijs, int kijl, const void* fl1, const void* xllws, const void* wvprpt, const void* ff, int flags, double zmiss,
        void* out, int NANG, int NFRE, hipStream_t s);
template <typename T> int launch_outbs_partition(const void* tab, int kijs, int kijl, const void* fl1, const void* xllws, const int* mij, const void* wvprpt, const void* ff, double zmiss,
        void* out, int NANG, int NFRE, hipStream_t s);
template <typename T> int launch_outbs_extremes(const void* tab, int kijs, int kijl, const void* fl1, const void* wvprpt, const void* ff, int flags, void* out, int NANG, int NFRE,
        hipStream_t s);
template <typename T> int launch_outbs_absolute(const void* tab, const void* itab, int kijs, int kijl, int mode, const void* fl1, const void* wvprpt, const void* ucur, const void* vcur,
        const void* ff, double zmiss, void* out, void* fl2nd, int NANG, int NFRE, hipStream_t s);
template <typename T> int launch_outbs_second_order(const void* tab, const void* itab, const void* sotab, const void* coef, void* work, int nmax, int kijs, int kijl, int mode,
        const void* fl1, const void* wvprpt, const void* depth, const void* ucur, const void* vcur, const void* ff, double sig, double zmiss, void* out, void* fl2nd, int NANG, int NFRE,
        hipStream_t s);
template <typename T> int launch_outbs_integrals(const void* tab, const void* inttab, int kijs, int kijl, const void* fl1, const void* fl2nd, const void* wvprpt, const void* ff,
        int flags, double zmiss, void* out, int NANG, int NFRE, hipStream_t s);   // 2 = no build for NANG
struct OutMaskCols { unsigned char f[64]; };   // OUTSETWMASK: per column, bit 0 the sea-ice mask, bit 1 the sea mask
template <typename T> void launch_outsetwmask(int kijs, int kijl, void* out, int ncol, const OutMaskCols& cols, const void* ff, const int* iodp, int ice, double cithrsh,
        double zmiss, hipStream_t s);
// IntTab<T> (csrc/outbs_int.h) from a host copy of DevTab<T>; a refusal's reason, or NULL
const char* outbs_int_tab_build(const void* devtab_host, int real_bytes, double xkmss_cutoff, int nband, const double* tbnd, const double* ttop, const void* delkcc_gc,
        std::vector<unsigned char>& host);
size_t outbs_devtab_bytes(int real_bytes);
size_t intpol_tab_build(const ecwam_hip_params* p, const ecwam_hip_tables* t, int real_bytes, std::vector<unsigned char>& host);
const char* so_tab_build(const ecwam_hip_params* p, const void* fr, int real_bytes, int ndepth, double deptha, double depthd, int nmax, const int* im_p, const int* im_m,
        std::vector<unsigned char>& host);
void so_coef_layout(int real_bytes, int ND, int AH, int NH, const void* const src[5], std::vector<unsigned char>& host);
size_t so_work_bytes(int real_bytes, int n, int AH, int NH, int NMAX);

// ---- nest.hip: BOUINPT / INTSPEC and OUTBC (wamodel.F90:333-343).  0 = launched (or nothing to do), 1 = unsupported spectral size, -1 = the frequencies
// of a direction are no whole number of 16-byte chunks (launch_bouinpt stores 16 bytes at a time, as launch_setice) ---------------------------------
template <typename T> int launch_bouinpt(const void* tab, int kijs, int kijl, int nijb, const int* ijb, const int* ibcl, const int* ibcr, const void* bfw, int nboinp,
        const void* f1, const void* par1, void* fl1, void* par_out, int NANG, int NFRE, hipStream_t s);
template <typename T> int launch_outbc(const void* tab, int nbc, const int* ijarc, const void* fl1, void* flpts, void* par, int NANG, int NFRE, hipStream_t s);

// ---- start.hip: the start spectra -- MSTART (IOPTI 0, 1, 2; par = FETCH, FRMAX, THETAQ, FM, ALFA, ZGAMMA, SA, SB), UNSETICE (cimask: LICERUN .AND. LMASKICE,
// lim: LBIWBK), GETSPEC's noise start and tail.  0 = launched (or nothing to do), 1 = unsupported spectral size, -1 = the frequencies of a direction are
// no whole number of 16-byte chunks (as launch_setice) ------------------------------------------------------------------------------------------------
template <typename T> int launch_mstart(const void* tab, int kijs, int kijl, void* fl1, const void* ff, int iopti, const double* par, int NANG, int NFRE, hipStream_t s);
template <typename T> int launch_unsetice(const void* tab, int kijs, int kijl, void* fl1, const void* ff, double delphi, int cimask, int lim, int NANG, int NFRE,
        hipStream_t s);
template <typename T> int launch_getspec_noise(const void* tab, int kijs, int kijl, void* fl1, int NANG, int NFRE, hipStream_t s);
template <typename T> int launch_getspec_tail(const void* tab, int kijs, int kijl, void* fl1, const void* ff, int nfre_red, int NANG, int NFRE, hipStream_t s);

// ---- forcing.hip: the forcing and coupling seam (include/ecwam_hip_forcing.h).  map = the validated map of ecwam_hip_set_forcing_map on the device, ncell the
// cells of a plane of fieldg / grid; nemo = double [4][kijl].  An empty range launches nothing (launch_fldtoifs still sets the defaults). ------------------------
template <typename T> void launch_getwnd(const void* tab, int kijs, int kijl, const int* map, const void* fieldg, size_t ncell, const void* ucur, const void* vcur,
        const double* nemo, void* ff, const ecwam_hip_forcing_opts& o, hipStream_t s);
template <typename T> void launch_cdustarz0(const void* tab, int kijs, int kijl, void* ff, hipStream_t s);
template <typename T> void launch_wamadswstar(int kijs, int kijl, const int* map, const void* fieldg, size_t ncell, void* ff, hipStream_t s);
template <typename T> void launch_getcurr(int kijs, int kijl, int mode, const int* map, const void* fieldg, size_t ncell, const double* nemo, void* ucur, void* vcur,
        int* changed, hipStream_t s);
template <typename T> void launch_wvblock(const void* tab, int llgcbz0, int kijs, int kijl, const void* ff, const void* intf, int flags, int nwvfields, double prchar,
        void* wvblock, int ld, hipStream_t s);
template <typename T> void launch_fldtoifs(int kijs, int kijl, const int* map, const void* wvblock, int ld, int nwvfields, const double* defval, void* grid, size_t ncell,
        hipStream_t s);

// ---- intake.hip: the forcing intake (include/ecwam_hip_intake.h).  idx = int [npts][4] and wgt = reals [npts][4] (DJ1, DII1, DIIP1, padding): the validated
// table of ecwam_hip_set_fldinter on the device; map, ncell, nemo as above.  An empty range launches nothing. -------------------------------------------------
template <typename T> void launch_fldinter(int kijs, int kijl, const void* idx, const void* wgt, int interpol, const int* map, const void* fields, size_t ngptotg,
        int flags, double roair, double wstar0, double pmiss, void* fieldg, size_t ncell, int* mask_in, hipStream_t s);
template <typename T> void launch_init_fieldg(const void* tab, void* fieldg, size_t ncell, double roair, double wstar0, hipStream_t s);
template <typename T> void launch_recvnemofields(int kijs, int kijl, int flags, const int* map, const void* fieldg, size_t ncell, double* nemo, double* nemoibr,
        void* ff, void* ucur, void* vcur, void* intf, hipStream_t s);
// scale = 0: the stresses are zeros (NEMONTAU <= 0); znemontaum1 = 1 / NEMONTAU, formed in the working precision
void launch_updnemo(int kijs, int kijl, double* wam2nemo, int scale, double znemontaum1, double* fields7, double* stress6, int ld, hipStream_t s);

// ---- readwind.hip: the forcing of a stand-alone run (include/ecwam_hip_readwind.h).  pos = int [ncell][4] and wgt = reals [ncell][4] (DK1, DII1, DIIP1, the
// kind): the validated table of ecwam_hip_set_input_grid on the device; desc is read on the host.  No cells, or no rows, launch nothing. ----------------------
template <typename T> void launch_grib2wgrid(int ncell, const void* pos, const void* wgt, int interpol, const void* values, size_t vstride, int nfld,
        const ecwam_hip_g2w_field* desc, double roair, double wstar0, double pmiss, void* out, size_t ld, void* fieldg, size_t ncell_in, hipStream_t s);
template <typename T> void launch_current2wam(int kijs, int kijl, const int* map, const void* field_u, const void* field_v, double wlowest, double zmiss, void* ucur,
        void* vcur, int* changed, hipStream_t s);

// ---- restart.hip: the start and the end of a run (include/ecwam_hip_restart.h).  map = the inbound map as above; inv = the inverse of the validated map of
// ecwam_hip_set_restart_map on the device (row -> position in a vector of the global order), or nullptr: the row itself.  An empty range launches
// nothing.  launch_depthprpt and launch_savspec_pack return as the tile launchers below. -----------------------------------------------------------------
template <typename T> int launch_depthprpt(const void* tab, int kijs, int kijl, const void* depth, double dkmax, double gam_b_j, void* wvprpt, void* wavnum, void* cgroup,
        void* omosnh2kd, void* ff, int NFRE, hipStream_t s);
template <typename T> void launch_buildstress(const void* tab, int kijs, int kijl, const int* map, const void* uwave, const void* cd, double zref, int flags, double prchar,
        double zmiss, void* ff, hipStream_t s);
// pack != 0: ff, ucur, vcur -> rfield [16][ld]; otherwise the inverse
template <typename T> void launch_stress_fields(int pack, int kijs, int kijl, const int* inv, void* ff, void* ucur, void* vcur, void* rfield, size_t ld, hipStream_t s);
template <typename T> int launch_savspec_pack(int kijs, int kijl, const void* fl1, int ifld0, int nfld, const int* inv, void* blk, size_t ld, int NANG, int NFRE, hipStream_t s);

// ---- gribout.hip: GRIB-ready spectra and parameter fields (include/ecwam_hip_gribout.h).  GribMapDev = the validated map of ecwam_hip_set_grib_map on the
// device: ival [npts] row -> cell, unfilled [nunf] the cells no row fills (those of a padded pole row excepted), adj [north.nadj + south.nadj] cell -> row
// or -1 for the rows beside the poles; a pole without padding has npole = nadj = 0.  keys = the scratch of the per-field maxima.  The tile launchers return
// 0 = launched (or nothing to do), 1 = the tile does not fit the LDS, -1 = NFRE is no whole number of 16-byte pieces. ------------------------------------
struct GribMapDev {
  const int *ival, *unfilled, *adj;
  int nunf, ntencode;
  ecwam_hip_grib_pole north, south;
};
template <typename T> int launch_outspec_values(int kijs, int kijl, const void* fl1, const void* ff, int ifld0, int nfld, int ice, double cithrsh, double flmin,
        const ecwam_hip_grib_opts& o, const GribMapDev& g, void* values, void* ppmax, void* keys, int NANG, int NFRE, int NFRE_RED, hipStream_t s);
template <typename T> int launch_outspec_pack(int kijs, int kijl, const void* fl1, const void* ff, int ifld0, int nfld, int ice, double cithrsh, double flmin, void* blk,
        int ld, int NANG, int NFRE, int NFRE_RED, hipStream_t s);
template <typename T> void launch_grib_values(int kijs, int kijl, const void* src, long long fstride, long long pstride, int nfld, int spectral,
        const ecwam_hip_grib_opts& o, const GribMapDev& g, void* values, void* ppmax, void* keys, hipStream_t s);

// ---- gribin.hip: decoded GRIB spectra and READFL's record into FL1 (include/ecwam_hip_gribin.h).  ival = the map row -> position in a vector, or nullptr: the
// row itself (the unpack form); src[nfld][stride]; mlim = the frequencies a field may have (NFRE_RED / NFRE).  Returns as the tile launchers above. ----------
template <typename T> int launch_getspec_fields(int kijs, int kijl, const void* src, long long stride, const int* ival, int ifld0, int nfld, int flags,
        const ecwam_hip_grib_opts* o, double epsmin, void* fl1, int NANG, int NFRE, int mlim, hipStream_t s);

// ---- outblock.hip: OUTBLOCK itself (outblock.F90:159-610) -- the plan of ecwam_hip_set_outblock and the kernel that fills BOUT ---------------------
// where a BOUT column comes from: the packed buffers of the output calls (in the work space of the context), the caller's per-point arrays, or nothing
enum { OB_ZERO = 0, OB_W8, OB_SEP, OB_EXT, OB_INT, OB_FF, OB_INTF, OB_UCUR, OB_VCUR, OB_IBRMEM, OB_ALTIM, OB_NEMO, OB_NSRC };
// what is done to the value: copy; MOD(DEG*x+180,360); MAX(-x,0); IBRMEMOUT's rule (zmiss where not CICOVER > 0).  OB_NEMO columns hold doubles.
enum { OB_COPY = 0, OB_DEG, OB_NEGMAX, OB_IBR };
// the calls of a plan (the bit mask ecwam_hip_outblock_plan returns; bits 8-13: the group flags of ecwam_hip_outbs_integrals, bit 14: W_MAXH runs)
enum { OB_CALL_OUTBS = 1, OB_CALL_SEPWISW = 2, OB_CALL_PARTITION = 4, OB_CALL_EXTREMES = 8, OB_CALL_ABSOLUTE = 16, OB_CALL_SECOND_ORDER = 32, OB_CALL_INTEGRALS = 64 };
// the caller's arrays a plan reads
enum { OB_NEED_FL1 = 1, OB_NEED_XLLWS = 2, OB_NEED_MIJ = 4, OB_NEED_WVPRPT = 8, OB_NEED_FF = 16, OB_NEED_INTF = 32, OB_NEED_UCUR = 64, OB_NEED_VCUR = 128,
       OB_NEED_IODP = 256, OB_NEED_IBRMEM = 512, OB_NEED_ALTIM = 1024, OB_NEED_NEMO = 2048 };
struct OutblockPlan {
  int niprmout = 0;
  int calls = 0, int_groups = 0, ext_full = 0, stores_fl2nd = 0;
  int w8_stride = 5, sep_stride = 15;   // ecwam_hip_outbs / _absolute rows, ecwam_hip_outbs_sepwisw / _partition rows
  int flags = 0;                        // as passed to ecwam_hip_set_outblock
  int ice = 0, sea = 0, need_ci = 0;    // the sea-ice mask applies to some column; the sea mask does; CICOVER is read (either mask or IBRMEMOUT)
  unsigned need = 0;                    // OB_NEED_*
  int why_param[12] = {0};              // per OB_NEED_* bit: one requested parameter that reads the array (for the refusal's text)
  std::vector<int> desc;                // [niprmout][2]: source | op << 8 | mask bits << 16, source column
};
// what ecwam_hip_set_outblock needs of the context
struct OutblockCtx {
  int NANG, NFRE, real_bytes, irefra, licerun, lmaskice, lwnemocoustrn;
  int has_second_order, has_itab, int_nband;
  const double *int_tb, *int_tt;        // the bands of ecwam_hip_set_outbs_integrals
  double fr1;                           // FR(1)
};
// a refusal's reason, or the empty string
std::string outblock_plan_build(const OutblockCtx& c, int jppflag, const int* ipfgtbl, const int* itobout, const int* icemask, const int* seamask, int niprmout,
        int flags, OutblockPlan& plan);
// element (ij, col) of source s at base[s] + ij * pstride[s] + col * cstride[s] (in elements of the source: reals, doubles for OB_NEMO)
struct OutblockSrc { const void* base[OB_NSRC]; long long pstride[OB_NSRC], cstride[OB_NSRC]; };
template <typename T> void launch_outblock_assemble(int kijs, int kijl, int ncol, const int* desc, const OutblockSrc& src, const void* ff, const int* iodp, int ice, int sea,
        int need_ci, double cithrsh, double zmiss, void* bout, hipStream_t s);
template <typename T> void launch_outblock_depth(int kijs, int kijl, const void* ff, void* depth, hipStream_t s);   // depth[ij] = ff[ij][15]
