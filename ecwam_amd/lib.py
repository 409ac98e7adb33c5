"""ctypes binding of libecwam_hip.so (include/ecwam_hip.h).  There is no CPU fallback: if the HIP
library is missing this module raises, and nothing in the product path imports the oracle."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .tables import JTOT_TAUHF, Tables

HERE = os.path.dirname(os.path.abspath(__file__))
# ECWAM_HIP_LIB: A/B timing of two builds of the same extension (tools/); never a fallback: the file must exist
LIBPATH = os.environ.get("ECWAM_HIP_LIB") or os.path.join(HERE, "lib", "libecwam_hip.so")

_INT_FIELDS_1 = ["nang", "nfre", "nfre_red", "nfre_odd", "idelt"]
_PARAM_LAYOUT = (
    [(n, C.c_int) for n in _INT_FIELDS_1]
    + [("ximp", C.c_double)]
    + [(n, C.c_int) for n in ["iphys", "isnonlin", "irefra", "icode", "llgcbz0", "llnormagam", "llcapchnk", "lbiwbk", "licerun",
                               "lmaskice", "lwamrsetci", "lciwa1", "lciwa2", "lciwa3", "lciscal", "lwvflx_snl", "lwflux",
                               "lwfluxout", "lwnemocou", "lwcou", "lwcouast", "lwnemocouwrs", "lwnemotauoc", "lwnemocousend",
                               "lwnemocoustk", "lwnemocoustrn"]]
    + [(n, C.c_double) for n in ["g", "gm1", "pi", "zpi", "zpi4gm1", "zpi4gm2", "epsmin", "rowater", "rowaterm1", "epsus",
                                  "epsu10", "acd", "bcd", "acdlin", "bcdlin", "cdmax", "tauocmin", "tauocmax", "phiepsmin",
                                  "phiepsmax", "wsemean_min", "circ", "r_earth", "fratio", "wetail", "frtail", "wp1tail", "fric",
                                  "delth", "flogsprdm1", "xkappa", "xnlev", "rnu", "rnum", "betamaxoxkappa2", "bmaxokap",
                                  "gamnconst", "zalp", "alpha", "alphamin", "alphamax", "chnkmin_u", "alphapmax", "tauwshelter", "dthrn_a",
                                  "dthrn_u", "tailfactor", "tailfactor_pm", "ang_gc_a", "ang_gc_b", "ang_gc_c", "rn1_rn", "swellf",
                                  "swellf2", "swellf3", "swellf4", "swellf5", "swellf6", "swellf7", "swellf7m1", "z0rat",
                                  "z0tubmax", "abmin", "abmax", "sdsbr", "ssdsc2", "ssdsc3", "ssdsc4", "ssdsc5", "ssdsc6", "miche"]]
    + [("nsdsnth", C.c_int), ("ipsat", C.c_int)]
    + [(n, C.c_double) for n in ["egrcrv", "afcrv", "bfcrv", "x0tauhf", "eps1", "flmin", "cithrsh", "ciblock", "cithrsh_tail",
                                  "zalpwrs", "bathymax", "wspmin", "wspmin_reset_tauw", "cdis", "delta_sdis", "cdisvis"]]
    + [("idamping", C.c_int)]
    + [(n, C.c_double) for n in ["cdicwa", "zalpfacb", "zalpfacx"]]
    + [("lwnemocouibr", C.c_int), ("zibrw_thrsh", C.c_double), ("nict", C.c_int), ("nich", C.c_int)]
    + [(n, C.c_double) for n in ["ticmin", "dtic", "dhic", "hicmin"]]
    + [("mfrstlw", C.c_int), ("mlsthg", C.c_int), ("kfrh", C.c_int), ("dal1", C.c_double), ("dal2", C.c_double),
       ("nwav_gc", C.c_int), ("xlogkratiom1_gc", C.c_double), ("sqrtgosurft", C.c_double)]
)


class Params(C.Structure):
    _fields_ = _PARAM_LAYOUT


_TABLE_NAMES = ["fr", "dfim", "dfimofr", "dfimfr", "dfim_sim", "rhowg_dfim", "zpifr", "fr5", "cofrm4", "flmax", "th", "costh",
                "sinth", "wtauhf", "swellft", "ikp", "ikp1", "ikm", "ikm1", "af11", "k1w", "k2w", "k11w", "k21w", "inlcoef",
                "rnlcoef", "indicessat", "satweights", "kpm", "jxo", "jyo", "kcr", "xk_gc", "xkm_gc", "omega_gc", "omxkm3_gc",
                "cm_gc", "c2osqrtvg_gc", "xkmsqrtvgoc2_gc", "om3gmkm_gc", "delkcc_gc_ns", "delkcc_omxkm3_gc", "cideac"]
_INT_TABLES = {"ikp", "ikp1", "ikm", "ikm1", "k1w", "k2w", "k11w", "k21w", "inlcoef", "indicessat", "kpm", "jxo", "jyo", "kcr"}


class TablePtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _TABLE_NAMES]


EXPORTS = ["ecwam_hip_last_error", "ecwam_hip_abi_version", "ecwam_hip_selftest", "ecwam_hip_create", "ecwam_hip_destroy", "ecwam_hip_set_obstructions", "ecwam_hip_propags2",
           "ecwam_hip_ctuw", "ecwam_hip_propags2_otf", "ecwam_hip_propags2_otf_split", "ecwam_hip_propags2_otf_fast", "ecwam_hip_set_fastwave_copy", "ecwam_hip_copy_freq_range", "ecwam_hip_propdot", "ecwam_hip_ctuw_refra", "ecwam_hip_propags2_refra", "ecwam_hip_implsch", "ecwam_hip_implsch_generation_used", "ecwam_hip_device_tables", "ecwam_hip_implsch_reserve", "ecwam_hip_wdfluxes", "ecwam_hip_wdfluxes_supported", "ecwam_hip_setice", "ecwam_hip_bouinpt", "ecwam_hip_outbc", "ecwam_hip_propags2_implsch_supported", "ecwam_hip_propags2_implsch", "ecwam_hip_outbs", "ecwam_hip_outbs_sepwisw", "ecwam_hip_outbs_partition", "ecwam_hip_outbs_extremes", "ecwam_hip_outbs_absolute", "ecwam_hip_set_second_order", "ecwam_hip_outbs_second_order", "ecwam_hip_set_outbs_integrals", "ecwam_hip_outbs_integrals", "ecwam_hip_outsetwmask", "ecwam_hip_set_outblock", "ecwam_hip_outblock_plan", "ecwam_hip_outblock", "ecwam_hip_outwnorm", "ecwam_hip_newwind", "ecwam_hip_newwind_icode", "ecwam_hip_nosource", "ecwam_hip_host_register", "ecwam_hip_host_unregister", "ecwam_hip_chunks_to_points",
           "ecwam_hip_points_to_chunks", "ecwam_hip_member_scatter", "ecwam_hip_member_gather", "ecwam_hip_pack_rows", "ecwam_hip_unpack_rows", "ecwam_hip_halo_setup", "ecwam_hip_halo_counts", "ecwam_hip_comm_unique_id",
           "ecwam_hip_comm_init", "ecwam_hip_comm_count", "ecwam_hip_halo_start", "ecwam_hip_halo_finish", "ecwam_hip_halo_pack_host", "ecwam_hip_halo_unpack_host", "ecwam_hip_proenvhalo_pack", "ecwam_hip_proenvhalo_unpack", "ecwam_hip_malloc", "ecwam_hip_free",
           "ecwam_hip_memcpy_h2d", "ecwam_hip_memcpy_d2h", "ecwam_hip_memset", "ecwam_hip_sync", "ecwam_hip_queue_create", "ecwam_hip_queue_destroy",
           "ecwam_hip_queue_wait_for"]

# include/ecwam_hip_start.h: the start spectra, added to ABI 6 in a header and a list of their own (EXPORTS is the list of include/ecwam_hip.h)
EXPORTS_START = ["ecwam_hip_mstart", "ecwam_hip_unsetice", "ecwam_hip_getspec_noise", "ecwam_hip_getspec_tail"]

# include/ecwam_hip_forcing.h: the forcing and coupling seam around WAMODEL, added to ABI 6 in the same way
EXPORTS_FORCING = ["ecwam_hip_set_forcing_map", "ecwam_hip_getwnd", "ecwam_hip_cdustarz0", "ecwam_hip_wamadswstar", "ecwam_hip_getcurr", "ecwam_hip_wvblock",
                   "ecwam_hip_fldtoifs"]
FG_PLANES = ["UWND", "VWND", "AIRD", "WSTAR", "CICOVER", "CITHICK", "USTRA", "VSTRA", "WSWAVE", "WDWAVE", "LKFR", "UCUR", "VCUR"]      # fieldg[13][ncell]
WVB_LWCOU2W, WVB_LWCOUHMF, WVB_LWSTOKES, WVB_LWFLUX = 1, 2, 4, 8
MAXWVFIELDS = 32


class ForcingOpts(C.Structure):
    """ecwam_hip_forcing_opts: the run-time switches of GETWND that are not in Params"""
    _fields_ = [("icode_wnd", C.c_int), ("llwswave", C.c_int), ("llwdwave", C.c_int), ("lcorrel", C.c_int), ("rwfac", C.c_double), ("iparamci", C.c_int),
                ("lwcou", C.c_int), ("lwnemocoucic", C.c_int), ("lwnemocoucit", C.c_int), ("lnemoicerest", C.c_int), ("liceth", C.c_int), ("swamp", C.c_int),
                ("swampcith", C.c_double), ("zmiss", C.c_double)]


# include/ecwam_hip_gribout.h: GRIB-ready spectra and parameter fields (OUTSPEC, OUTINT), added to ABI 6 in the same way
EXPORTS_GRIBOUT = ["ecwam_hip_set_grib_map", "ecwam_hip_outspec_values", "ecwam_hip_outspec_pack", "ecwam_hip_grib_values"]
OUTSPEC_ICEMASK = 1


class GribPole(C.Structure):
    """ecwam_hip_grib_pole"""
    _fields_ = [("pole0", C.c_int), ("npole", C.c_int), ("adj0", C.c_int), ("nadj", C.c_int)]


class GribPoles(C.Structure):
    """ecwam_hip_grib_poles"""
    _fields_ = [("north", GribPole), ("south", GribPole)]


class GribOpts(C.Structure):
    """ecwam_hip_grib_opts: YOWGRIBHD's packing constants and ZMISS"""
    _fields_ = [("ppmiss", C.c_double), ("ppeps", C.c_double), ("pprec", C.c_double), ("ppresol", C.c_double), ("ppmin_reset", C.c_double), ("ngrbress", C.c_int),
                ("zmiss", C.c_double)]


# include/ecwam_hip_gribin.h: decoded GRIB spectra and READFL's record into FL1 (GETSPEC's warm start), added to ABI 6 in the same way
EXPORTS_GRIBIN = ["ecwam_hip_getspec_values", "ecwam_hip_getspec_unpack"]
GETSPEC_UNSCALE, GETSPEC_MISSING = 1, 2

# include/ecwam_hip_intake.h: the forcing intake in front of GETWND and the hand-over to NEMO (INIT_FIELDG, FLDINTER, RECVNEMOFIELDS, UPDNEMO*), added to
# ABI 6 in the same way
EXPORTS_INTAKE = ["ecwam_hip_set_fldinter", "ecwam_hip_fldinter", "ecwam_hip_init_fieldg", "ecwam_hip_recvnemofields", "ecwam_hip_updnemo"]
FLI_LADEN, FLI_LGUST, FLI_LLKC, FLI_LWCUR, FLI_NEWCURR = 1, 2, 4, 8, 16
RNF_LREST, RNF_LINIT, RNF_LWCOU, RNF_LWNEMOCOUCIC, RNF_LWNEMOCOUCIT, RNF_LWNEMOCOUCUR, RNF_LWNEMOCOUIBR = 1, 2, 4, 8, 16, 32, 64

# include/ecwam_hip_readwind.h: the forcing of a stand-alone run (GRIB2WGRID, READWIND's fill, CURRENT2WAM), added to ABI 6 in the same way
EXPORTS_READWIND = ["ecwam_hip_set_input_grid", "ecwam_hip_grib2wgrid", "ecwam_hip_current2wam"]
G2W_NSLOT, G2W_MAXFLD, G2W_FIELD, G2W_DIRFLD, G2W_NONWAVE = 4, 16, -1, 1, 2
G2W_PLANES = ("UWND", "VWND", "AIRD", "WSTAR", "CICOVER", "CITHICK", "WSWAVE", "WDWAVE")      # the planes of fieldg a field may target


class G2wField(C.Structure):      # ecwam_hip_g2w_field
    _fields_ = [("target", C.c_int), ("flags", C.c_int)]


# include/ecwam_hip_restart.h: the start and the end of a run (INITDPTHFLDS, BUILDSTRESS, SAVSTRESS / GETSTRESS, WRITEFL's record), added to ABI 6 in the same way
EXPORTS_RESTART = ["ecwam_hip_depthprpt", "ecwam_hip_buildstress", "ecwam_hip_set_restart_map", "ecwam_hip_savstress_pack", "ecwam_hip_getstress_unpack",
                   "ecwam_hip_savspec_pack"]
BST_Z0B_ZERO, BST_NSESTART = 1, 2
NRESTART_FIELDS = 16
# the columns of ff in the order of the restart fields (savstress.F90:112-125); UCUR and VCUR follow
RESTART_FF_COLUMNS = (3, 1, 7, 8, 9, 10, 11, 12, 0, 4, 2, 13, 5, 6)


class DepthOpts(C.Structure):
    """ecwam_hip_depth_opts: DKMAX (yowpcons.F90) and GAM_B_J (yowshal.F90)"""
    _fields_ = [("dkmax", C.c_double), ("gam_b_j", C.c_double)]


# include/ecwam_hip_propags.h: the first-order propagation scheme (IPROPAGS = 0: PROPAGS, CHECKCFL, PROPDOT with GRADI), added to ABI 6 in the same way
EXPORTS_PROPAGS = ["ecwam_hip_propags_dot", "ecwam_hip_propags"]
PROPAGS_CARTESIAN, PROPAGS_IRREGULAR = 1, 2
PROPAGS_NCFL = 11      # DTC, CFLEA, CFLWE, CFLNO, CFLSO, CFLNO2, CFLSO2, CFLTP, CFLTM, CFLOP, CFLOM


def propags_dot_width(nang: int) -> int:
    """ECWAM_HIP_PROPAGS_DOT_W: THDD(K), THDC(K), S0(K), OMDD, three reals of padding"""
    return 3 * nang + 4


# include/ecwam_hipx_propags1.h: the dual rotated-quadrant scheme (IPROPAGS = 1: PROPAGS1), added to ABI 6.  The list of names with the prefix ecwam_hip_ is held
# closed by tests/test_propags_host.py: additions from here on take the prefix ecwam_hipx_ and are listed in an EXPORTS_X_* list
EXPORTS_X_PROPAGS1 = ["ecwam_hipx_set_rotated", "ecwam_hipx_propags1"]


ABI_VERSION = 6        # include/ecwam_hip.h ECWAM_HIP_ABI_VERSION
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBPATH):
        raise RuntimeError(f"{LIBPATH} not found: the HIP extension is not built (run `python -m ecwam_amd.build` or "
                           "__graft_entry__.build()); there is no CPU fallback")
    # PyTorch-ROCm bundles its own HIP runtime (same SONAME as the system one the extension was linked against).  Whichever is
    # mapped first serves the whole process, and two different copies cannot both own the devices: load torch's first so
    # that device buffers, streams and our kernels live in ONE runtime, whatever order the caller imports things in.
    import torch  # noqa: F401
    lib = C.CDLL(LIBPATH)
    lib.ecwam_hip_last_error.restype = C.c_char_p
    lib.ecwam_hip_abi_version.restype = C.c_int
    if lib.ecwam_hip_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIBPATH}: ABI version {lib.ecwam_hip_abi_version()} but this binding is written for {ABI_VERSION}; rebuild the extension")
    for name in EXPORTS[1:]:
        getattr(lib, name).restype = C.c_int
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.ecwam_hip_create.argtypes = [C.POINTER(Params), C.POINTER(TablePtrs), ci, ci, C.POINTER(vp)]
    lib.ecwam_hip_destroy.argtypes = [vp]
    lib.ecwam_hip_selftest.argtypes = [ci]
    lib.ecwam_hip_set_obstructions.argtypes = [vp, vp, ci]
    lib.ecwam_hip_propags2.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.ecwam_hip_ctuw.argtypes = [vp, ci, ci, ci, cd, ci, ci, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_propags2_otf.argtypes = [vp, vp, vp, ci, ci, cd, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.ecwam_hip_propags2_otf_split.argtypes = [vp, vp, vp, ci, ci, cd, cd, ci, ci, vp, ci, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.ecwam_hip_propags2_otf_fast.argtypes = [vp, vp, vp, ci, ci, cd, cd, ci, ci, vp, ci, ci, vp, ci, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.ecwam_hip_set_fastwave_copy.argtypes = [vp, vp, ci]
    lib.ecwam_hip_propags2_implsch_supported.argtypes = [vp]
    lib.ecwam_hip_propags2_implsch.argtypes = [vp, vp, vp, ci, ci, cd, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp,
                                               cd, ci, vp, ci, ci, vp]
    lib.ecwam_hip_copy_freq_range.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]
    lib.ecwam_hip_propdot.argtypes = [vp, ci, ci, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_ctuw_refra.argtypes = [vp, ci, ci, ci, cd, ci, ci, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp]
    lib.ecwam_hip_propags2_refra.argtypes = [vp, vp, vp, ci, ci, cd, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.ecwam_hip_implsch.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_device_tables.argtypes = [vp]
    lib.ecwam_hip_device_tables.restype = vp
    lib.ecwam_hip_implsch_reserve.argtypes = [vp, ci]
    lib.ecwam_hip_implsch_generation_used.argtypes = [vp]
    lib.ecwam_hip_wdfluxes.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_wdfluxes_supported.argtypes = [vp]
    lib.ecwam_hip_setice.argtypes = [vp, ci, ci, vp, vp, vp]
    lib.ecwam_hip_bouinpt.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    lib.ecwam_hip_outbc.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    lib.ecwam_hip_outbs.argtypes = [vp, ci, ci, vp, cd, vp, vp]
    lib.ecwam_hip_outbs_sepwisw.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, cd, vp, vp]
    lib.ecwam_hip_outbs_partition.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, cd, vp, vp]
    lib.ecwam_hip_outbs_extremes.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp]
    lib.ecwam_hip_outbs_absolute.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, cd, vp, vp, vp]
    lib.ecwam_hip_set_second_order.argtypes = [vp, ci, cd, cd, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_outbs_second_order.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, cd, cd, vp, vp, vp]
    lib.ecwam_hip_set_outbs_integrals.argtypes = [vp, cd, ci, vp, vp, vp]
    lib.ecwam_hip_outbs_integrals.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, cd, vp, vp]
    lib.ecwam_hip_outsetwmask.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, cd, cd, vp]
    lib.ecwam_hip_set_outblock.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci]
    lib.ecwam_hip_outblock_plan.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    lib.ecwam_hip_outblock.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, cd, cd, vp, vp]
    lib.ecwam_hip_outwnorm.argtypes = [vp, vp, ci, ci, cd, C.POINTER(C.c_double), vp]
    lib.ecwam_hip_newwind.argtypes = [vp, ci, vp, vp, vp]
    lib.ecwam_hip_newwind_icode.argtypes = [vp, ci, vp, vp, ci, vp]
    lib.ecwam_hip_nosource.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    lib.ecwam_hip_host_register.argtypes = [vp, vp, C.c_ulonglong]
    lib.ecwam_hip_host_unregister.argtypes = [vp, vp]
    lib.ecwam_hip_chunks_to_points.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.ecwam_hip_points_to_chunks.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.ecwam_hip_member_scatter.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.c_longlong, C.c_longlong, ci, vp]
    lib.ecwam_hip_member_gather.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.c_longlong, C.c_longlong, ci, vp]
    lib.ecwam_hip_pack_rows.argtypes = [vp, vp, vp, ci, vp, vp]
    lib.ecwam_hip_unpack_rows.argtypes = [vp, vp, ci, vp, ci, vp]
    lib.ecwam_hip_halo_setup.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.ecwam_hip_halo_counts.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    lib.ecwam_hip_comm_unique_id.argtypes = [vp]
    lib.ecwam_hip_comm_init.argtypes = [vp, vp]
    lib.ecwam_hip_comm_count.argtypes = [vp, C.POINTER(ci)]
    lib.ecwam_hip_halo_start.argtypes = [vp, vp, ci, vp]
    lib.ecwam_hip_halo_finish.argtypes = [vp, vp]
    lib.ecwam_hip_halo_pack_host.argtypes = [vp, vp, ci, vp, vp]
    lib.ecwam_hip_halo_unpack_host.argtypes = [vp, vp, ci, vp, vp]
    lib.ecwam_hip_proenvhalo_pack.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_proenvhalo_unpack.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for name in EXPORTS_START:
        getattr(lib, name).restype = C.c_int
    lib.ecwam_hip_mstart.argtypes = [vp, ci, ci, vp, vp, ci, cd, cd, cd, cd, cd, cd, cd, cd, vp]
    lib.ecwam_hip_unsetice.argtypes = [vp, ci, ci, vp, vp, cd, ci, vp]
    lib.ecwam_hip_getspec_noise.argtypes = [vp, ci, ci, vp, vp]
    lib.ecwam_hip_getspec_tail.argtypes = [vp, ci, ci, vp, vp, ci, vp]
    for name in EXPORTS_FORCING:
        getattr(lib, name).restype = C.c_int
    lib.ecwam_hip_set_forcing_map.argtypes = [vp, ci, vp, ci, vp, ci]
    lib.ecwam_hip_getwnd.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, C.POINTER(ForcingOpts), vp]
    lib.ecwam_hip_cdustarz0.argtypes = [vp, ci, ci, vp, vp]
    lib.ecwam_hip_wamadswstar.argtypes = [vp, ci, ci, vp, vp, vp]
    lib.ecwam_hip_getcurr.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_wvblock.argtypes = [vp, ci, ci, vp, vp, ci, ci, cd, vp, ci, vp]
    lib.ecwam_hip_fldtoifs.argtypes = [vp, ci, ci, vp, ci, ci, vp, vp, vp]
    for name in EXPORTS_GRIBOUT:
        getattr(lib, name).restype = C.c_int
    ll = C.c_longlong
    lib.ecwam_hip_set_grib_map.argtypes = [vp, ci, vp, ci, C.POINTER(GribPoles)]
    lib.ecwam_hip_outspec_values.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, C.POINTER(GribOpts), vp, vp, vp]
    lib.ecwam_hip_outspec_pack.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, vp, ci, vp]
    lib.ecwam_hip_grib_values.argtypes = [vp, ci, ci, vp, ll, ll, ci, ci, C.POINTER(GribOpts), vp, vp, vp]
    for name in EXPORTS_GRIBIN:
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [vp, ci, ci, vp, ll, ci, ci, ci, C.POINTER(GribOpts), vp, vp]
    for name in EXPORTS_INTAKE:
        getattr(lib, name).restype = C.c_int
    lib.ecwam_hip_set_fldinter.argtypes = [vp, ci, ci, vp, vp, ci]
    lib.ecwam_hip_fldinter.argtypes = [vp, ci, ci, vp, ci, ci, ci, cd, cd, cd, vp, vp, vp]
    lib.ecwam_hip_init_fieldg.argtypes = [vp, vp, ci, cd, cd, vp]
    lib.ecwam_hip_recvnemofields.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_updnemo.argtypes = [vp, ci, ci, vp, ci, vp, vp, ci, vp]
    for name in EXPORTS_READWIND:
        getattr(lib, name).restype = C.c_int
    lib.ecwam_hip_set_input_grid.argtypes = [vp, ci, ci, ci, vp, vp, vp, ci]
    lib.ecwam_hip_grib2wgrid.argtypes = [vp, ci, vp, ci, ci, C.POINTER(G2wField), cd, cd, cd, vp, ci, vp, ci, vp]
    lib.ecwam_hip_current2wam.argtypes = [vp, ci, ci, vp, vp, cd, cd, vp, vp, vp, vp]
    for name in EXPORTS_RESTART:
        getattr(lib, name).restype = C.c_int
    lib.ecwam_hip_depthprpt.argtypes = [vp, ci, ci, vp, C.POINTER(DepthOpts), vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_buildstress.argtypes = [vp, ci, ci, vp, vp, cd, ci, cd, cd, vp, vp]
    lib.ecwam_hip_set_restart_map.argtypes = [vp, ci, vp]
    lib.ecwam_hip_savstress_pack.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, ci, vp]
    lib.ecwam_hip_getstress_unpack.argtypes = [vp, ci, ci, vp, ci, ci, vp, vp, vp, vp]
    lib.ecwam_hip_savspec_pack.argtypes = [vp, ci, ci, vp, ci, ci, ci, vp, ci, vp]
    for name in EXPORTS_PROPAGS:
        getattr(lib, name).restype = C.c_int
    lib.ecwam_hip_propags_dot.argtypes = [vp, ci, ci, ci, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ecwam_hip_propags.argtypes = [vp, vp, vp, ci, ci, ci, cd, cd, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp]
    for name in EXPORTS_X_PROPAGS1:
        getattr(lib, name).restype = C.c_int
    lib.ecwam_hipx_set_rotated.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, cd]
    lib.ecwam_hipx_propags1.argtypes = lib.ecwam_hip_propags.argtypes
    _lib = lib
    return lib


def make_params(t: Tables) -> Params:
    c = t.cfg
    p = Params()
    for name, typ in _PARAM_LAYOUT:
        if hasattr(c, name) and name not in ("wspmin", "rnu", "rnum"):
            v = getattr(c, name)
        elif name == "r_earth":
            v = t.R
        else:
            v = getattr(t, name.upper())
        setattr(p, name, int(v) if typ is C.c_int else float(v))
    return p


def make_tables(t: Tables):
    """Returns (TablePtrs, keepalive list).  Index tables are passed 1-based as the reference holds them."""
    T = t.dtype
    keep = []
    tp = TablePtrs()
    one_based = {"indicessat": 1, "kpm": 1}  # ours are stored 0-based in Tables
    for name in _TABLE_NAMES:
        a = getattr(t, name.upper())
        if name in _INT_TABLES:
            a = np.ascontiguousarray(np.asarray(a) + one_based.get(name, 0), dtype=np.int32)
        else:
            a = np.ascontiguousarray(a, dtype=T)
        keep.append(a)
        setattr(tp, name, a.ctypes.data_as(C.c_void_p))
    assert t.WTAUHF.size == JTOT_TAUHF
    return tp, keep
