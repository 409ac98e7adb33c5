"""Host-side mirror of the reference's hot-path interfaces over the C ABI.

`HipContext` owns one `ecwam_hip_ctx`; its methods carry the reference routine names
(PROPAGS2, CTUW, IMPLSCH, NEWWIND) and take torch CUDA tensors purely as device-memory handles
(`data_ptr()` + the current HIP stream).  Shapes, dtypes and index ranges are validated on the host
before any launch, so that a wrong operand cannot reach a kernel.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as _lib
from .tables import Tables

NFF, NINTF, NWPR = 16, 16, 5
NFIELDG = len(_lib.FG_PLANES)      # the planes of fieldg (include/ecwam_hip_forcing.h)
# columns of ecwam_hip_outbs_sepwisw (include/ecwam_hip.h): OUTBLOCK parameters 20-22, 11-16, 23-28
OUTBS_SEP_FIELDS = ("mp1", "mp2", "wdw", "shww", "shts", "mdww", "mdts", "mpww", "mpts",
                    "p1sea", "p1swell", "p2sea", "p2swell", "sprdsea", "sprdswell")
# columns of ecwam_hip_outbs_partition (include/ecwam_hip.h): those of ecwam_hip_outbs_sepwisw, then the swell trains 1-3 (parameters 42-50)
OUTBS_PART_FIELDS = OUTBS_SEP_FIELDS + ("swh1", "mwd1", "mwp1", "swh2", "mwd2", "mwp2", "swh3", "mwd3", "mwp3")
# columns of ecwam_hip_outbs_extremes (include/ecwam_hip.h): OUTBLOCK parameters 29, 30, 31, 33, 34, 57, 70, 71, 72 (KURTOSIS), 78-81 (W_MAXH)
OUTBS_EXT_FIELDS = ("c4", "bfi", "qp", "hmax", "tmax", "c3", "eta_m", "r", "xnslc", "cmax_f", "hmax_n", "cmax_st", "hmax_st")
# columns of ecwam_hip_outbs_absolute (include/ecwam_hip.h): OUTBLOCK parameters 1, 2, 3, EM, 6, 20, 21, 22 of the output spectrum FL2ND
OUTBS_ABS_FIELDS = ("swh", "mwd", "mwp", "em", "pp1d", "mp1", "mp2", "wdw")
# the first eight columns of ecwam_hip_outbs_integrals (the bands follow) and its column groups (flags)
OUTBS_INT_FIELDS = ("cd", "tauw_n", "mss", "strn", "wefmag", "wefdir", "ctcor", "mss_m")
OUTBS_INT_GROUPS = dict(slopes=1, strain=2, flux=4, ctcor=8, bands=16, point=32)
OUTBS_INT_ALL = 63

# ---- OUTBLOCK's parameter table: this project's restatement of mpcrtbl.F90:92-469 as (number, short name, sea-ice mask, sea mask), the numbers from
# the reference's index formulas (outblock.F90:437-604) with the NTRAIN and NTEWH the library is written for
NTRAIN, NTEWH = 3, 6
JPPFLAG = 75 + 3 * NTRAIN + 5


def _outblock_params():
    T, F = True, False
    n3 = 3 * NTRAIN
    rows = [(1, "swh", T, T), (2, "mwd", T, T), (3, "mwp", T, T), (4, "ufric", F, T), (5, "dwi", F, F), (6, "pp1d", T, T), (7, "cdww", F, F),
            (8, "tauw_n", T, T), (9, "msqs", T, T), (10, "wind", F, F), (11, "shww", T, T), (12, "shts", T, T), (13, "mdww", T, T), (14, "mdts", T, T),
            (15, "mpww", T, T), (16, "mpts", T, T), (17, "altwh", T, T), (18, "caltwh", T, T), (19, "raltcor", T, T), (20, "mp1", T, T),
            (21, "mp2", T, T), (22, "wdw", T, T), (23, "p1ww", T, T), (24, "p1ps", T, T), (25, "p2ww", T, T), (26, "p2ps", T, T), (27, "dwww", T, T),
            (28, "dwps", T, T), (29, "wsk", T, T), (30, "bfi", T, T), (31, "wsp", T, T), (32, "wmb", F, T), (33, "hmax", T, T), (34, "tmax", T, T),
            (35, "ust", T, T), (36, "vst", T, T), (37, "ocu", F, T), (38, "vcu", F, T), (39, "phieps", F, T), (40, "phiaw", F, T), (41, "tauoc", F, T)]
    for itr in range(1, NTRAIN + 1):
        rows += [(42 + 3 * (itr - 1), f"swh{itr}", T, T), (43 + 3 * (itr - 1), f"mwd{itr}", T, T), (44 + 3 * (itr - 1), f"mwp{itr}", T, T)]
    rows += [(42 + n3, "strn", F, T), (43 + n3, "h10", T, T), (44 + n3, "aird", F, F), (45 + n3, "wstar", F, F), (46 + n3, "ci", F, T),
             (47 + n3, "cithick", F, T), (48 + n3, "c3", T, T), (49 + n3, "sic", F, F), (50 + n3, "nemocithick", F, F), (51 + n3, "ucurr", F, F),
             (52 + n3, "vcurr", F, F), (53 + n3, "wefmag", T, T), (54 + n3, "wefdir", T, T)]
    periods = (10, 12, 14, 17, 21, 25, 30)          # IPRMINFO(:,4:5) of the bands, mpcrtbl.F90:371-399
    rows += [(54 + n3 + ih, f"h{periods[ih - 1]}{periods[ih]}", T, T) for ih in range(1, NTEWH + 1)]
    b = n3 + NTEWH
    rows += [(55 + b, "eta_m", T, T), (56 + b, "r", T, T), (57 + b, "xnslc", T, T), (58 + b, "tauxd", F, T), (59 + b, "tauyd", F, T),
             (60 + b, "tauocxd", F, T), (61 + b, "tauocyd", F, T), (62 + b, "phiocd", F, T), (63 + b, "tdcmax", T, T), (64 + b, "tdhmax", T, T),
             (65 + b, "stcmax", T, T), (66 + b, "sthmax", T, T), (67 + b, "sibm", T, T), (68 + b, "xwrs", T, T), (69 + b, "ywrs", T, T)]
    # the five extra fields JPPFLAG-5+IC (mpcrtbl.F90:464-469); OUTBLOCK fills the first two "for testing" (outblock.F90:597-604)
    extra = {70 + b: "ctcor", 71 + b: "mss_m"}
    rows += [(JPPFLAG - 5 + ic, extra.get(JPPFLAG - 5 + ic, f"extra{JPPFLAG - 5 + ic:03d}"), F, F) for ic in range(1, 6)]
    assert [r[0] for r in rows] == list(range(1, JPPFLAG + 1))
    return tuple(rows)


OUTBLOCK_PARAMS = _outblock_params()
OUTBLOCK_NUMBER = {name: ir for ir, name, _, _ in OUTBLOCK_PARAMS}
# the calls of a plan, in the bit order of ecwam_hip_outblock_plan
OUTBLOCK_CALLS = ("outbs", "sepwisw", "partition", "extremes", "absolute", "second_order", "integrals")


def outblock_tables(requested):
    """(IPFGTBL, ITOBOUT, NIPRMOUT) of a request as mpcrtbl.F90:473-502 builds them: requested is an iterable of parameter numbers, or a mapping
    parameter -> IPFGTBL value (any value /= 0 puts the parameter on the list; -1 is the reference's "normed only").  Columns are handed out in the
    order of the parameter numbers."""
    val = dict(requested) if hasattr(requested, "keys") else {int(ir): 1 for ir in requested}
    for ir in val:
        if not 1 <= int(ir) <= JPPFLAG:
            raise ValueError(f"OUTBLOCK: parameter {ir} outside 1 .. {JPPFLAG}")
    ipfgtbl = np.zeros(JPPFLAG, np.int32)
    itobout = np.zeros(JPPFLAG, np.int32)
    n = 0
    for ir in range(1, JPPFLAG + 1):
        if val.get(ir, 0) != 0:
            ipfgtbl[ir - 1] = val[ir]
            n += 1
            itobout[ir - 1] = n
    return ipfgtbl, itobout, n


class EcwamHipError(RuntimeError):
    pass


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


class HipContext:
    def __init__(self, tables: Tables, device: int = 0):
        self.lib = _lib.load()
        self.t = tables
        self.dtype = torch.float32 if tables.dtype == np.float32 else torch.float64
        self.real_bytes = 4 if tables.dtype == np.float32 else 8
        self.NANG, self.NFRE, self.NR = tables.cfg.nang, tables.cfg.nfre, tables.cfg.nfre_red
        self.N = self.NANG * self.NFRE
        self.device = torch.device("cuda", device)
        params = _lib.make_params(tables)
        tp, keep = _lib.make_tables(tables)
        self._h = C.c_void_p()
        rc = self.lib.ecwam_hip_create(C.byref(params), C.byref(tp), self.real_bytes, device, C.byref(self._h))
        del keep
        self._chk(rc)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.ecwam_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int) -> None:
        if rc != 0:
            raise EcwamHipError(self.lib.ecwam_hip_last_error().decode())

    # -- validation helpers
    def _real(self, t: torch.Tensor, shape, name: str) -> int:
        if not (t.is_cuda and t.dtype == self.dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"{name}: expected contiguous {self.dtype} cuda tensor of shape {tuple(shape)}, got "
                             f"{t.dtype} {tuple(t.shape)} cuda={t.is_cuda} contiguous={t.is_contiguous()}")
        return t.data_ptr()

    @staticmethod
    def _int(t: torch.Tensor, shape, name: str) -> int:
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"{name}: expected contiguous int32 cuda tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
        return t.data_ptr()

    # -- LSUBGRID: OBS[n][8][NFRE] = OBSLAT(:,M,1:2), OBSLON(:,M,1:2), OBSCOR(:,M,1:4); the tensor is kept alive here
    @property
    def has_obstructions(self) -> bool:
        return getattr(self, "_obs", None) is not None

    def set_obstructions(self, obs) -> None:
        if obs is None:
            self._obs = None
            self._chk(self.lib.ecwam_hip_set_obstructions(self._h, None, 0))
            return
        n = obs.shape[0]
        self._obs = obs
        self._chk(self.lib.ecwam_hip_set_obstructions(self._h, self._real(obs, (n, 8, self.NFRE), "OBS"), n))

    # -- PROPAGS2(F1,F3,NINF,NSUP,KIJS,KIJL,NANG,ND3SF1,ND3EF1,ND3S,ND3E)  (propags2.F90:10)
    def propags2(self, f1, f3, klon, klat, kcor, w, kijs, kijl, nd3s=1, nd3e=None, copy_rest=True, check_indices=False):
        nd3e = self.NR if nd3e is None else nd3e
        nrow = f1.shape[0]
        n = klon.shape[0]
        p1 = self._real(f1, (nrow, self.NANG, self.NFRE), "F1")
        p3 = self._real(f3, (nrow, self.NANG, self.NFRE), "F3")
        if not (0 <= kijs <= kijl <= n):
            raise ValueError("PROPAGS2: KIJS/KIJL outside the neighbour tables")
        pk = self._int(klon, (n, 2), "KLON"), self._int(klat, (n, 2, 2), "KLAT"), self._int(kcor, (n, 4, 2), "KCOR")
        pw = self._real(w, (n, 8, self.NANG * self.NR), "W")
        if check_indices:
            for a, nm in ((klon, "KLON"), (klat, "KLAT"), (kcor, "KCOR")):
                lo, hi = int(a.min()), int(a.max())
                if lo < 0 or hi >= nrow:
                    raise ValueError(f"PROPAGS2: {nm} index out of range [{lo},{hi}] for {nrow} spectra")
        self._chk(self.lib.ecwam_hip_propags2(self._h, p1, p3, *pk, pw, kijs, kijl, nd3s, nd3e, int(copy_rest), _stream_ptr()))

    # -- CTUWINI + CTUW (ctuwupdt.F90:204-238)
    def ctuw(self, grid_dev: dict, cgroup_ext, w, cflfail, delpro: float, mstart=1, mend=None):
        mend = self.NR if mend is None else mend
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = cgroup_ext.shape[0]
        if nland >= nrow:
            raise ValueError("CTUW: CGROUP_EXT must include the land row")
        args = [self._int(g["kxlt"], (n,), "KXLT"), self._real(g["zdello"], (ngy,), "ZDELLO"), float(g["xdella"]),
                self._real(g["cosph"], (ngy,), "COSPH"), self._real(g["sinph"], (ngy,), "SINPH"),
                self._int(g["klon"], (n, 2), "KLON"), self._int(g["klat"], (n, 2, 2), "KLAT"), self._int(g["kcor"], (n, 4, 2), "KCOR"),
                self._real(g["wlat"], (n, 2), "WLAT"), self._real(g["wcor"], (n, 4), "WCOR"),
                self._real(cgroup_ext, (nrow, self.NFRE), "CGROUP_EXT"), self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"),
                None if w is None else self._real(w, (n, 8, self.NANG * self.NR), "W"), self._int(cflfail, (n,), "CFLFAIL")]
        self._chk(self.lib.ecwam_hip_ctuw(self._h, n, nland, ngy, float(delpro), mstart, mend, *args, _stream_ptr()))

    # -- PROPAGS2 with on-the-fly CTU weights (no W array): same result as ctuw() + propags2()
    def propags2_otf(self, f1, f3, grid_dev: dict, cgroup_ext, delpro: float, kijs, kijl, nd3s=1, nd3e=None, copy_rest=True,
                     order=None, ifrelfmax: int = 0, delpro_lf: float | None = None, gout=None, tiles2d: bool = False, gin=None):
        """ifrelfmax > 0: frequencies 1..ifrelfmax advance with delpro_lf, the others with delpro, in the same pass.
        gout: optional compact buffer [nrow][NANG][w] that also receives the first w advected frequencies.
        gin: optional compact buffer [nrow][NANG][w] the first w frequencies are READ from (with full rows f1).
        f1 and / or f3 may themselves be compact buffers [nrow][NANG][w] (a fast-wave sub-step)."""
        nd3e = self.NR if nd3e is None else nd3e
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = f1.shape[0]
        if not (0 <= kijs <= kijl) or (order is None and kijl > n) or nland >= nrow or cgroup_ext.shape[0] != nrow:
            raise ValueError("PROPAGS2: KIJS/KIJL outside the neighbour tables, or F1 / CGROUP_EXT without the land row")
        po = None if order is None else self._int(order, (order.shape[0],), "ORDER")
        if order is not None and order.shape[0] < kijl:
            raise ValueError("PROPAGS2: ORDER shorter than KIJL")
        if tiles2d and order is None:
            raise ValueError("PROPAGS2: 2-D tiles need the order of decomp.tile2d_order")
        dlf = float(delpro if delpro_lf is None else delpro_lf)
        in_nfre = int(f1.shape[2])          # NFRE, or the width of a compact fast-wave buffer [nrow][NANG][in_nfre]
        out_nfre = int(f3.shape[2])
        args = [self._real(f1, (nrow, self.NANG, in_nfre), "F1"), self._real(f3, (f3.shape[0], self.NANG, out_nfre), "F3"), n, ngy,
                float(delpro), dlf, int(ifrelfmax), 0 if in_nfre == self.NFRE else in_nfre,
                None if gin is None else self._real(gin, (gin.shape[0], self.NANG, gin.shape[2]), "GIN"),
                0 if gin is None else int(gin.shape[2]), 0 if out_nfre == self.NFRE else out_nfre,
                None if gout is None else self._real(gout, (gout.shape[0], self.NANG, gout.shape[2]), "GOUT"),
                0 if gout is None else int(gout.shape[2]), self._int(g["kxlt"], (n,), "KXLT"), self._real(g["zdello"], (ngy,), "ZDELLO"),
                float(g["xdella"]), self._real(g["cosph"], (ngy,), "COSPH"), self._real(g["sinph"], (ngy,), "SINPH"),
                self._int(g["klon"], (n, 2), "KLON"), self._int(g["klat"], (n, 2, 2), "KLAT"), self._int(g["kcor"], (n, 4, 2), "KCOR"),
                self._real(g["wlat"], (n, 2), "WLAT"), self._real(g["wcor"], (n, 4), "WCOR"),
                self._real(cgroup_ext, (nrow, self.NFRE), "CGROUP_EXT"), self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"), po]
        self._chk(self.lib.ecwam_hip_propags2_otf_fast(self._h, *args, kijs, kijl, nd3s, nd3e, int(bool(copy_rest)) | (4 if tiles2d else 0), _stream_ptr()))

    def set_fastwave_copy(self, g) -> None:
        """g: compact rows [nrow][NANG][w] IMPLSCH / NOSOURCE also write the first w frequencies of their result to (None: off)."""
        if g is None:
            self._chk(self.lib.ecwam_hip_set_fastwave_copy(self._h, None, 0))
        else:
            self._chk(self.lib.ecwam_hip_set_fastwave_copy(self._h, self._real(g, (g.shape[0], self.NANG, g.shape[2]), "G"), int(g.shape[2])))

    # -- FL1_EXT(:,:,M1:M2) <- FL3_EXT between the fast-wave sub-steps (propag_wam.F90:287-291)
    def copy_freq_range(self, src, dst, n, m_first, m_last):
        """dst may be a compact buffer [nrow][NANG][w] with w >= m_last."""
        shape = (src.shape[0], self.NANG, self.NFRE)
        w = int(dst.shape[2])
        if n > src.shape[0] or n > dst.shape[0] or w < m_last:
            raise ValueError("copy_freq_range: shapes")
        self._chk(self.lib.ecwam_hip_copy_freq_range(self._h, self._real(src, shape, "SRC"), self._real(dst, (dst.shape[0], self.NANG, w), "DST"),
                                                     n, m_first, m_last, 0 if w == self.NFRE else w, _stream_ptr()))

    # -- refraction (IREFRA = 1, 2, 3): GRADI + PROPDOT per point, CTUWDRV checks, PROPAGS2 with all weights on the fly
    def _geom(self, g, n, ngy):
        return [self._int(g["kxlt"], (n,), "KXLT"), self._real(g["zdello"], (ngy,), "ZDELLO"), float(g["xdella"]),
                self._real(g["cosph"], (ngy,), "COSPH"), self._real(g["sinph"], (ngy,), "SINPH"),
                self._int(g["klon"], (n, 2), "KLON"), self._int(g["klat"], (n, 2, 2), "KLAT"), self._int(g["kcor"], (n, 4, 2), "KCOR"),
                self._real(g["wlat"], (n, 2), "WLAT"), self._real(g["wcor"], (n, 4), "WCOR")]

    def propdot(self, grid_dev: dict, depth_ext, u_ext, v_ext, refr):
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = depth_ext.shape[0]
        if nland >= nrow:
            raise ValueError("PROPDOT: the *_EXT arrays must include the land row")
        self._chk(self.lib.ecwam_hip_propdot(
            self._h, n, nland, self._int(g["kxlt"], (n,), "KXLT"), self._real(g["zdello"], (ngy,), "ZDELLO"), float(g["xdella"]),
            self._real(g["cosph"], (ngy,), "COSPH"), self._int(g["klon"], (n, 2), "KLON"), self._int(g["klat"], (n, 2, 2), "KLAT"),
            self._real(g["wlat"], (n, 2), "WLAT"), self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"),
            self._real(depth_ext, (nrow,), "DEPTH_EXT"), self._real(u_ext, (nrow,), "U_EXT"), self._real(v_ext, (nrow,), "V_EXT"),
            self._real(refr, (n, 2 * self.NANG + 5), "REFR"), _stream_ptr()))

    def ctuw_refra(self, grid_dev: dict, cgroup_ext, omosnh2kd_ext, wavnum_ext, refr, cflfail, delpro: float, mstart=1, mend=None,
                   llcflcuroff=True, frange=0):
        mend = self.NR if mend is None else mend
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = cgroup_ext.shape[0]
        if nland >= nrow:
            raise ValueError("CTUW: CGROUP_EXT must include the land row")
        ext = [self._real(a, (nrow, self.NFRE), nm) for a, nm in ((cgroup_ext, "CGROUP_EXT"), (omosnh2kd_ext, "OMOSNH2KD_EXT"),
                                                                 (wavnum_ext, "WAVNUM_EXT"))]
        self._chk(self.lib.ecwam_hip_ctuw_refra(self._h, n, nland, ngy, float(delpro), mstart, mend, *self._geom(g, n, ngy), *ext,
                                                self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"),
                                                self._real(refr, (n, 2 * self.NANG + 5), "REFR"), int(llcflcuroff), int(frange),
                                                self._int(cflfail, (n,), "CFLFAIL"), _stream_ptr()))

    def propags2_refra(self, f1, f3, grid_dev: dict, cgroup_ext, omosnh2kd_ext, wavnum_ext, refr, delpro: float, kijs, kijl, nd3s=1,
                       nd3e=None, copy_rest=True, frange=0):
        nd3e = self.NR if nd3e is None else nd3e
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = f1.shape[0]
        if not (0 <= kijs <= kijl <= n) or nland >= nrow or cgroup_ext.shape[0] != nrow:
            raise ValueError("PROPAGS2: KIJS/KIJL outside the neighbour tables, or F1 / CGROUP_EXT without the land row")
        ext = [self._real(a, (nrow, self.NFRE), nm) for a, nm in ((cgroup_ext, "CGROUP_EXT"), (omosnh2kd_ext, "OMOSNH2KD_EXT"),
                                                                 (wavnum_ext, "WAVNUM_EXT"))]
        self._chk(self.lib.ecwam_hip_propags2_refra(
            self._h, self._real(f1, (nrow, self.NANG, self.NFRE), "F1"), self._real(f3, (nrow, self.NANG, self.NFRE), "F3"), n, ngy,
            float(delpro), *self._geom(g, n, ngy), *ext, self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"),
            self._real(refr, (n, 2 * self.NANG + 5), "REFR"), int(frange), kijs, kijl, nd3s, nd3e, int(copy_rest), _stream_ptr()))

    # -- IPROPAGS = 0: PROPDOT with GRADI, then PROPAGS with CHECKCFL (propag_wam.F90:341-362; include/ecwam_hip_propags.h)
    def propags_dot(self, grid_dev: dict, depth_ext, u_ext, v_ext, dot, icase: int = 1):
        """dot [n][3 NANG + 4] = THDD(K), THDC(K), S0(K), OMDD, padding: the reference's GRADI + PROPDOT statement by statement."""
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = depth_ext.shape[0]
        if nland >= nrow:
            raise ValueError("PROPDOT: the *_EXT arrays must include the land row")
        self._chk(self.lib.ecwam_hip_propags_dot(
            self._h, n, nland, int(icase), self._int(g["kxlt"], (n,), "KXLT"), self._real(g["zdello"], (ngy,), "ZDELLO"), float(g["xdella"]),
            self._real(g["cosph"], (ngy,), "COSPH"), self._int(g["klon"], (n, 2), "KLON"), self._int(g["klat"], (n, 2, 2), "KLAT"),
            self._real(g["wlat"], (n, 2), "WLAT"), self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"),
            self._real(depth_ext, (nrow,), "DEPTH_EXT"), self._real(u_ext, (nrow,), "U_EXT"), self._real(v_ext, (nrow,), "V_EXT"),
            self._real(dot, (n, _lib.propags_dot_width(self.NANG)), "DOT"), _stream_ptr()))

    def propags(self, f1, f3, grid_dev: dict, cgroup_ext, delpro: float, kijs, kijl, omosnh2kd_ext=None, wavnum_ext=None, u_ext=None, v_ext=None, dot=None,
                copy_rest=True, cfl=None, cflfail=None, icase: int = 1, irgg: int = 1, delphi: float | None = None):
        """PROPAGS for rows [kijs, kijl).  grid_dev holds, beside the tables of grid_to_device, "dellam1_ext" (propags_grid adds it).  f3 = None: the
        check of CHECKCFL alone.  delphi: DELPHI in the working precision; default XDELLA CIRC / 360 formed in it."""
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = f1.shape[0]
        if nland >= nrow or cgroup_ext.shape[0] != nrow:
            raise ValueError("PROPAGS: F1 / CGROUP_EXT without the land row")
        npdt = np.float32 if self.dtype == torch.float32 else np.float64
        if delphi is None:
            delphi = float(npdt(g["xdella"]) * npdt(self.t.CIRC) / npdt(360.0))

        def opt(t, shape, name):
            return None if t is None else self._real(t, shape, name)

        flags = (_lib.PROPAGS_CARTESIAN if icase == 2 else 0) | (_lib.PROPAGS_IRREGULAR if irgg == 1 else 0)
        self._chk(self.lib.ecwam_hip_propags(
            self._h, self._real(f1, (nrow, self.NANG, self.NFRE), "F1"), opt(f3, (nrow, self.NANG, self.NFRE), "F3"), n, nland, ngy, float(delpro), float(delphi),
            flags, self._int(g["kxlt"], (n,), "KXLT"), self._real(g["cosph"], (ngy,), "COSPH"), self._real(g["sinph"], (ngy,), "SINPH"),
            self._real(g["dellam1_ext"], (nrow,), "DELLAM1_EXT"), self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"), self._int(g["klon"], (n, 2), "KLON"),
            self._int(g["klat"], (n, 2, 2), "KLAT"), self._real(g["wlat"], (n, 2), "WLAT"), self._real(cgroup_ext, (nrow, self.NFRE), "CGROUP_EXT"),
            opt(omosnh2kd_ext, (nrow, self.NFRE), "OMOSNH2KD_EXT"), opt(wavnum_ext, (nrow, self.NFRE), "WAVNUM_EXT"), opt(u_ext, (nrow,), "U_EXT"),
            opt(v_ext, (nrow,), "V_EXT"), opt(dot, (n, _lib.propags_dot_width(self.NANG)), "DOT"), kijs, kijl, int(bool(copy_rest)),
            opt(cfl, (n, self.NANG, _lib.PROPAGS_NCFL), "CFL"), None if cflfail is None else self._int(cflfail, (n,), "CFLFAIL"), _stream_ptr()))

    # -- IPROPAGS = 1: PROPAGS1 with CHECKCFL (propag_wam.F90:296-322; include/ecwam_hipx_propags1.h)
    @property
    def has_rotated(self) -> bool:
        return getattr(self, "_rot", None) is not None

    def set_rotated(self, tables) -> None:
        """tables: device tensors krlat, krlon [n][2][2] (int32), wrlat, wrlon [n][2], cdr, sdr [nrow][NANG], prqrt [n] and the number sqrt2 (the dict of
        rotated_to_device); None switches them off.  The tensors are kept alive here."""
        if tables is None:
            self._rot = None
            self._chk(self.lib.ecwam_hipx_set_rotated(self._h, 0, 0, None, None, None, None, None, None, None, 0.0))
            return
        t = tables
        n, nrow = t["prqrt"].shape[0], t["cdr"].shape[0]
        self._chk(self.lib.ecwam_hipx_set_rotated(
            self._h, n, nrow, self._int(t["krlat"], (n, 2, 2), "KRLAT"), self._int(t["krlon"], (n, 2, 2), "KRLON"), self._real(t["wrlat"], (n, 2), "WRLAT"),
            self._real(t["wrlon"], (n, 2), "WRLON"), self._real(t["cdr"], (nrow, self.NANG), "CDR"), self._real(t["sdr"], (nrow, self.NANG), "SDR"),
            self._real(t["prqrt"], (n,), "PRQRT"), float(t["sqrt2"])))
        self._rot = dict(t)

    def propags1(self, f1, f3, grid_dev: dict, cgroup_ext, delpro: float, kijs, kijl, omosnh2kd_ext=None, wavnum_ext=None, u_ext=None, v_ext=None, dot=None,
                 copy_rest=True, cfl=None, cflfail=None, icase: int = 1, irgg: int = 1, delphi: float | None = None):
        """PROPAGS1 for rows [kijs, kijl): the arguments of propags; on a spherical grid with IREFRA 0 or 1 the tables of set_rotated are read."""
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = f1.shape[0]
        if nland >= nrow or cgroup_ext.shape[0] != nrow:
            raise ValueError("PROPAGS1: F1 / CGROUP_EXT without the land row")
        npdt = np.float32 if self.dtype == torch.float32 else np.float64
        if delphi is None:
            delphi = float(npdt(g["xdella"]) * npdt(self.t.CIRC) / npdt(360.0))

        def opt(t, shape, name):
            return None if t is None else self._real(t, shape, name)

        flags = (_lib.PROPAGS_CARTESIAN if icase == 2 else 0) | (_lib.PROPAGS_IRREGULAR if irgg == 1 else 0)
        self._chk(self.lib.ecwam_hipx_propags1(
            self._h, self._real(f1, (nrow, self.NANG, self.NFRE), "F1"), opt(f3, (nrow, self.NANG, self.NFRE), "F3"), n, nland, ngy, float(delpro), float(delphi),
            flags, self._int(g["kxlt"], (n,), "KXLT"), self._real(g["cosph"], (ngy,), "COSPH"), self._real(g["sinph"], (ngy,), "SINPH"),
            self._real(g["dellam1_ext"], (nrow,), "DELLAM1_EXT"), self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"), self._int(g["klon"], (n, 2), "KLON"),
            self._int(g["klat"], (n, 2, 2), "KLAT"), self._real(g["wlat"], (n, 2), "WLAT"), self._real(cgroup_ext, (nrow, self.NFRE), "CGROUP_EXT"),
            opt(omosnh2kd_ext, (nrow, self.NFRE), "OMOSNH2KD_EXT"), opt(wavnum_ext, (nrow, self.NFRE), "WAVNUM_EXT"), opt(u_ext, (nrow,), "U_EXT"),
            opt(v_ext, (nrow,), "V_EXT"), opt(dot, (n, _lib.propags_dot_width(self.NANG)), "DOT"), kijs, kijl, int(bool(copy_rest)),
            opt(cfl, (n, self.NANG, _lib.PROPAGS_NCFL), "CFL"), None if cflfail is None else self._int(cflfail, (n,), "CFLFAIL"), _stream_ptr()))

    # -- IMPLSCH (implsch.F90:10-23)
    def implsch(self, kijs, kijl, fl1, wvprpt, ff, intf, mij, xllws, dbg=None, wam2nemo=None):
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, wvprpt.shape[0], ff.shape[0], intf.shape[0], mij.shape[0], xllws.shape[0])):
            raise ValueError("IMPLSCH: KIJS/KIJL outside the operands")
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"),
             self._real(ff, (ff.shape[0], NFF), "FF"), self._real(intf, (intf.shape[0], NINTF), "INTF"),
             self._int(mij, (mij.shape[0],), "MIJ"), self._real(xllws, (xllws.shape[0], self.NANG, self.NFRE), "XLLWS")]
        pd = None if dbg is None else self._real(dbg, (nrow, 32), "DBG")
        pw = None
        if wam2nemo is not None:
            if not (wam2nemo.is_cuda and wam2nemo.dtype == torch.float64 and wam2nemo.is_contiguous() and wam2nemo.dim() == 2
                    and wam2nemo.shape[1] == 13 and wam2nemo.shape[0] >= kijl):
                raise ValueError("WAM2NEMO: expected contiguous float64 cuda tensor [npts >= KIJL][13]")
            pw = wam2nemo.data_ptr()
        self._chk(self.lib.ecwam_hip_implsch(self._h, kijs, kijl, *a, pw, pd, _stream_ptr()))

    # -- WDFLUXES (wdfluxes.F90:156-306) and SETICE (setice.F90:67-86): what OUTSTEP0 runs before the output of step 0
    def wdfluxes_supported(self) -> bool:
        """The flux-only mode covers the context's configuration (the common and the alternate builds of the IMPLSCH kernel)."""
        return bool(self.lib.ecwam_hip_wdfluxes_supported(self._h))

    def wdfluxes(self, kijs, kijl, fl1, wvprpt, ff, intf, mij, xllws, wam2nemo=None):
        """FL1, WVPRPT and FF are read only; MIJ and XLLWS are written, and with LWFLUX / LWFLUXOUT the flux members of INTF (and columns
        0, 1 of WAM2NEMO when LWNEMOCOU)."""
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, wvprpt.shape[0], ff.shape[0], intf.shape[0], mij.shape[0], xllws.shape[0])):
            raise ValueError("WDFLUXES: KIJS/KIJL outside the operands")
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"),
             self._real(ff, (ff.shape[0], NFF), "FF"), self._real(intf, (intf.shape[0], NINTF), "INTF"),
             self._int(mij, (mij.shape[0],), "MIJ"), self._real(xllws, (xllws.shape[0], self.NANG, self.NFRE), "XLLWS")]
        pw = None
        if wam2nemo is not None:
            if not (wam2nemo.is_cuda and wam2nemo.dtype == torch.float64 and wam2nemo.is_contiguous() and wam2nemo.dim() == 2
                    and wam2nemo.shape[1] == 13 and wam2nemo.shape[0] >= kijl):
                raise ValueError("WAM2NEMO: expected contiguous float64 cuda tensor [npts >= KIJL][13]")
            pw = wam2nemo.data_ptr()
        self._chk(self.lib.ecwam_hip_wdfluxes(self._h, kijs, kijl, *a, pw, _stream_ptr()))

    def setice(self, kijs, kijl, fl1, ff):
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, ff.shape[0])):
            raise ValueError("SETICE: KIJS/KIJL outside the operands")
        self._chk(self.lib.ecwam_hip_setice(self._h, kijs, kijl, self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"),
                                            self._real(ff, (ff.shape[0], NFF), "FF"), _stream_ptr()))

    # -- the start spectra (include/ecwam_hip_start.h; csrc/start.hip): what creates FL1 where a run does not begin from a restart file
    def _start_rows(self, who, kijs, kijl, fl1, ff=None):
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= (nrow if ff is None else min(nrow, ff.shape[0]))):
            raise ValueError(f"{who}: KIJS/KIJL outside the operands")
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1")]
        return a if ff is None else a + [self._real(ff, (ff.shape[0], NFF), "FF")]

    def mstart(self, kijs, kijl, fl1, ff, iopti, fetch, frmax, thetaq, fm, alfa, zgamma, sa, sb):
        """MSTART (mstart.F90:104-136) for IOPTI 0, 1, 2 on rows [kijs, kijl): FL1 is written from WSWAVE and WDWAVE of FF and MSTART's eight
        reals (the fetch in metres, the maximum peak frequency, the mean direction in radians, FM, ALFA, ZGAMMA, SA, SB)."""
        self._chk(self.lib.ecwam_hip_mstart(self._h, kijs, kijl, *self._start_rows("MSTART", kijs, kijl, fl1, ff), int(iopti),
                                            *(float(v) for v in (fetch, frmax, thetaq, fm, alfa, zgamma, sa, sb)), _stream_ptr()))

    def unsetice(self, kijs, kijl, fl1, ff, delphi, restarted: bool = False, small_domain: bool = False):
        """UNSETICE (unsetice.F90:79-171) on rows [kijs, kijl); delphi = DELPHI [m].  restarted / small_domain are LRESTARTED and CLDOMAIN == 's':
        with either the routine does nothing (unsetice.F90:79) and nothing is launched."""
        self._chk(self.lib.ecwam_hip_unsetice(self._h, kijs, kijl, *self._start_rows("UNSETICE", kijs, kijl, fl1, ff), float(delphi),
                                              (1 if restarted else 0) | (2 if small_domain else 0), _stream_ptr()))

    def getspec_noise(self, kijs, kijl, fl1):
        """GETSPEC's noise start (getspec.F90:174-188): FL1 = EPSMIN on rows [kijs, kijl)."""
        self._chk(self.lib.ecwam_hip_getspec_noise(self._h, kijs, kijl, *self._start_rows("GETSPEC", kijs, kijl, fl1), _stream_ptr()))

    def getspec_tail(self, kijs, kijl, fl1, ff, nfre_red=None):
        """The end of GETSPEC's GRIB read (getspec.F90:648-659) on rows [kijs, kijl): the frequencies above nfre_red (default: the context's
        NFRE_RED) from the last one read, then SDEPTHLIM with EMAXDPT of FF."""
        self._chk(self.lib.ecwam_hip_getspec_tail(self._h, kijs, kijl, *self._start_rows("GETSPEC", kijs, kijl, fl1, ff),
                                                  int(self.NR if nfre_red is None else nfre_red), _stream_ptr()))

    # -- the forcing and coupling seam (include/ecwam_hip_forcing.h; csrc/forcing.hip): what WAVEMDL runs immediately before and after WAMODEL
    def set_forcing_map(self, ixy_in=None, ncell_in: int = 0, ixy_out=None, ncell_out: int = 0) -> None:
        """The maps row -> cell (0-based, host integers of one length): ixy_in into the planes of fieldg (ncell_in cells each), ixy_out into the
        outbound grid (ncell_out cells, no cell twice).  None removes a map.  The library validates and uploads them."""
        a = [None if m is None else np.ascontiguousarray(m, dtype=np.int32).reshape(-1) for m in (ixy_in, ixy_out)]
        if a[0] is not None and a[1] is not None and a[0].size != a[1].size:
            raise ValueError("set_forcing_map: the two maps differ in length")
        npts = next((m.size for m in a if m is not None), 0)
        ptr = [None if m is None else m.ctypes.data_as(C.c_void_p) for m in a]
        self._chk(self.lib.ecwam_hip_set_forcing_map(self._h, npts, ptr[0], int(ncell_in), ptr[1], int(ncell_out)))
        self._fmap = (npts, int(ncell_in) if a[0] is not None else 0, int(ncell_out) if a[1] is not None else 0)

    def _seam(self, who, kijs, kijl, *rows):
        if not (0 <= kijs <= kijl <= min(a.shape[0] for a in rows)):
            raise ValueError(f"{who}: KIJS/KIJL outside the operands")

    def _fieldg(self, fieldg):
        ncell = getattr(self, "_fmap", (0, 0, 0))[1]
        return None if fieldg is None else self._real(fieldg, (len(_lib.FG_PLANES), ncell), "FIELDG")

    def _nemo(self, nemo, kijl):
        """float64 [4][>= kijl] -> the planes of exactly kijl points the library takes (kept alive by the caller of this method)"""
        if nemo is None:
            return None
        if not (nemo.is_cuda and nemo.dtype == torch.float64 and nemo.dim() == 2 and nemo.shape[0] == 4 and nemo.shape[1] >= kijl):
            raise ValueError("NEMO: expected a float64 cuda tensor [4][>= KIJL]")
        return nemo[:, :kijl].contiguous()

    def getwnd(self, kijs, kijl, fieldg, ff, ucur=None, vcur=None, nemo=None, icode_wnd: int | None = None, llwswave: bool = False, llwdwave: bool = False,
               lcorrel: bool = False, rwfac: float = 1.0, iparamci: int = 31, lwcou: bool | None = None, lwnemocoucic: bool = False,
               lwnemocoucit: bool = False, lnemoicerest: bool = False, liceth: bool = False, swamp: bool = False, swampcith: float = 0.0,
               zmiss: float = -999.0):
        """GETWND per chunk (getwnd.F90:211-229) on rows [kijs, kijl) of ff: WAMWND, then MICEP, from the planes fieldg [13][ncell_in] (lib.FG_PLANES)
        through the inbound map.  icode_wnd defaults to ICODE and lwcou to LWCOU of the parameters; lcorrel is LCORREL of wamwnd.F90:127-133."""
        c = self.t.cfg
        o = _lib.ForcingOpts(int(c.icode if icode_wnd is None else icode_wnd), int(llwswave), int(llwdwave), int(lcorrel), float(rwfac), int(iparamci),
                             int(c.lwcou if lwcou is None else lwcou), int(lwnemocoucic), int(lwnemocoucit), int(lnemoicerest), int(liceth), int(swamp),
                             float(swampcith), float(zmiss))
        self._seam("GETWND", kijs, kijl, ff, *[a for a in (ucur, vcur) if a is not None])
        opt = lambda a, name: None if a is None else self._real(a, (a.shape[0],), name)
        pn = self._nemo(nemo, kijl)
        self._chk(self.lib.ecwam_hip_getwnd(self._h, kijs, kijl, self._fieldg(fieldg), opt(ucur, "UCUR"), opt(vcur, "VCUR"), None if pn is None else pn.data_ptr(),
                                            self._real(ff, (ff.shape[0], NFF), "FF"), C.byref(o), _stream_ptr()))

    def cdustarz0(self, kijs, kijl, ff):
        """CDUSTARZ0 with ZREF = XNLEV (getfrstwnd.F90:125-126): UFRIC and Z0M of ff from its WSWAVE on rows [kijs, kijl)."""
        self._seam("CDUSTARZ0", kijs, kijl, ff)
        self._chk(self.lib.ecwam_hip_cdustarz0(self._h, kijs, kijl, self._real(ff, (ff.shape[0], NFF), "FF"), _stream_ptr()))

    def wamadswstar(self, kijs, kijl, fieldg, ff):
        """WAMADSWSTAR (wamadswstar.F90:60-69): AIRD, WSTAR, USTRA, VSTRA of ff from fieldg on rows [kijs, kijl)."""
        self._seam("WAMADSWSTAR", kijs, kijl, ff)
        self._chk(self.lib.ecwam_hip_wamadswstar(self._h, kijs, kijl, self._fieldg(fieldg), self._real(ff, (ff.shape[0], NFF), "FF"), _stream_ptr()))

    def getcurr(self, kijs, kijl, mode, ucur, vcur, fieldg=None, nemo=None, changed=None):
        """The point-wise part of GETCURR on rows [kijs, kijl) of ucur / vcur: mode 0 WAMCUR from fieldg, 1 the NEMO currents (nemo float64
        [4][>= kijl], planes 2 and 3) where LKFR of fieldg <= 0, 2 zero.  changed: an int32 cuda tensor of one element that becomes 1 if a value
        changed (KUPDATE); the call never clears it."""
        self._seam("GETCURR", kijs, kijl, ucur, vcur)
        pn = self._nemo(nemo, kijl)
        self._chk(self.lib.ecwam_hip_getcurr(self._h, kijs, kijl, int(mode), self._fieldg(fieldg), None if pn is None else pn.data_ptr(),
                                             self._real(ucur, (ucur.shape[0],), "UCUR"), self._real(vcur, (vcur.shape[0],), "VCUR"),
                                             None if changed is None else self._int(changed, (1,), "CHANGED"), _stream_ptr()))

    def wvblock(self, kijs, kijl, wvblock, ff=None, intf=None, lwcou2w: bool = False, lwcouhmf: bool = False, lwstokes: bool = False, lwflux: bool = False,
                prchar: float = 0.0185, flags: int | None = None):
        """The WVBLOCK fill of wavemdl.F90:757-802 on rows [kijs, kijl) of wvblock [NWVFIELDS][ld]: OUTBETA's BETAM (and BETAHQ) with lwcou2w,
        otherwise prchar; then the fields of intf the switches name, then zeros.  flags (the lib.WVB_* bits) overrides the four switches."""
        if flags is None:
            flags = (_lib.WVB_LWCOU2W if lwcou2w else 0) | (_lib.WVB_LWCOUHMF if lwcouhmf else 0) | (_lib.WVB_LWSTOKES if lwstokes else 0) | \
                (_lib.WVB_LWFLUX if lwflux else 0)
        if wvblock.dim() != 2:
            raise ValueError("WVBLOCK: expected [NWVFIELDS][ld]")
        nwv, ld = wvblock.shape
        if not (0 <= kijs <= kijl <= ld):
            raise ValueError("WVBLOCK: KIJS/KIJL outside the operands")
        self._seam("WVBLOCK", kijs, kijl, *[a for a in (ff, intf) if a is not None])
        self._chk(self.lib.ecwam_hip_wvblock(self._h, kijs, kijl, None if ff is None else self._real(ff, (ff.shape[0], NFF), "FF"),
                                             None if intf is None else self._real(intf, (intf.shape[0], NINTF), "INTF"), int(flags), nwv, float(prchar),
                                             self._real(wvblock, (nwv, ld), "WVBLOCK"), ld, _stream_ptr()))

    def fldtoifs(self, kijs, kijl, wvblock, grid, defval=None):
        """MPFLDTOIFS on one task: rows [kijs, kijl) of wvblock [NWVFIELDS][ld] into grid [NWVFIELDS][ncell_out] through the outbound map; with
        defval (NWVFIELDS host numbers) the whole grid is set to the defaults first (LLINIT_GRID)."""
        if wvblock.dim() != 2:
            raise ValueError("FLDTOIFS: expected WVBLOCK [NWVFIELDS][ld]")
        nwv, ld = wvblock.shape
        if not (0 <= kijs <= kijl <= ld):
            raise ValueError("FLDTOIFS: KIJS/KIJL outside the operands")
        d = None
        if defval is not None:
            d = np.ascontiguousarray(defval, dtype=np.float64).reshape(-1)
            if d.size != nwv:
                raise ValueError("FLDTOIFS: one default per field")
        ncell = getattr(self, "_fmap", (0, 0, 0))[2]
        self._chk(self.lib.ecwam_hip_fldtoifs(self._h, kijs, kijl, self._real(wvblock, (nwv, ld), "WVBLOCK"), ld, nwv,
                                              None if d is None else d.ctypes.data_as(C.c_void_p), self._real(grid, (nwv, ncell), "GRID"), _stream_ptr()))

    # -- the forcing intake (include/ecwam_hip_intake.h; csrc/intake.hip): what PREWIND runs in front of GETWND, and the hand-over to NEMO
    def set_fldinter(self, idx, w=None, ngptotg: int = 0, interpol: bool = True) -> None:
        """The per-point table of FLDINTER (intake.point_table builds it): idx host integers [npts][4], the 0-based positions of the four corners
        in a field vector; w host numbers [npts][3], DJ1M, DII1M, DIIP1M in the working precision; ngptotg the length of a field vector.
        interpol=False is LLINTERPOL = F: only idx[:, 0] is read.  idx=None removes the table.  The library validates and uploads it; a later
        set_forcing_map drops it."""
        if idx is None:
            self._chk(self.lib.ecwam_hip_set_fldinter(self._h, 0, 0, None, None, 0))
            self._fli = None
            return
        a = np.ascontiguousarray(idx, dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("set_fldinter: idx is [npts][4]")
        pw = None
        if w is not None:
            pw = np.ascontiguousarray(w, dtype=np.float64)
            if pw.shape != (a.shape[0], 3):
                raise ValueError("set_fldinter: w is [npts][3]")
            if not np.array_equal(pw.astype(self.t.dtype).astype(np.float64), pw):
                raise ValueError("set_fldinter: the weights are not values of the working precision")
        self._chk(self.lib.ecwam_hip_set_fldinter(self._h, a.shape[0], int(ngptotg), a.ctypes.data_as(C.c_void_p),
                                                  None if pw is None else pw.ctypes.data_as(C.c_void_p), int(bool(interpol))))
        self._fli = (a.shape[0], int(ngptotg))

    def fldinter(self, kijs, kijl, fields, fieldg, laden: bool = False, lgust: bool = False, llkc: bool = False, lwcur: bool = False, newcurr: bool = False,
                 roair: float = 1.225, wstar0: float = 0.0, pmiss: float = -999.0, mask_in=None, flags: int | None = None):
        """FLDINTER (fldinter.F90:176-374) on rows [kijs, kijl): fields [nfields][ngptotg] -> the planes of fieldg [13][ncell_in] through the inbound
        map.  newcurr is LLNEWCURR .AND. .NOT. LWNEMOCOUCUR.  mask_in: an int32 cuda tensor [ngptotg] in which every position read becomes 1 (never
        cleared).  flags (the lib.FLI_* bits) overrides the five switches."""
        if flags is None:
            flags = (_lib.FLI_LADEN if laden else 0) | (_lib.FLI_LGUST if lgust else 0) | (_lib.FLI_LLKC if llkc else 0) | (_lib.FLI_LWCUR if lwcur else 0) | \
                (_lib.FLI_NEWCURR if newcurr else 0)
        if fields.dim() != 2:
            raise ValueError("FIELDS: expected [nfields][ngptotg]")
        nf, ng = fields.shape
        self._chk(self.lib.ecwam_hip_fldinter(self._h, int(kijs), int(kijl), self._real(fields, (nf, ng), "FIELDS"), ng, nf, int(flags), float(roair), float(wstar0),
                                              float(pmiss), self._fieldg(fieldg), None if mask_in is None else self._int(mask_in, (ng,), "MASK_IN"), _stream_ptr()))

    def init_fieldg(self, fieldg, roair: float = 1.225, wstar0: float = 0.0):
        """The LLINIALL branch of INIT_FIELDG (init_fieldg.F90:92-116) on fieldg [13][ncell]: zeros, WSWAVE = WSPMIN, AIRD = roair, WSTAR = wstar0."""
        if fieldg.dim() != 2 or fieldg.shape[0] != len(_lib.FG_PLANES):
            raise ValueError("FIELDG: expected [13][ncell]")
        self._chk(self.lib.ecwam_hip_init_fieldg(self._h, self._real(fieldg, tuple(fieldg.shape), "FIELDG"), int(fieldg.shape[1]), float(roair), float(wstar0),
                                                 _stream_ptr()))

    def recvnemofields(self, kijs, kijl, nemo, ff=None, ucur=None, vcur=None, intf=None, fieldg=None, nemoibr=None, lrest: bool = False, linit: bool = False,
                       lwcou: bool | None = None, lwnemocoucic: bool = False, lwnemocoucit: bool = False, lwnemocoucur: bool = False,
                       lwnemocouibr: bool = False, flags: int | None = None):
        """The point-wise branches of RECVNEMOFIELDS on rows [kijs, kijl): lrest fills nemo (float64 [4][kijl]: exactly kijl points a plane) and
        nemoibr (float64 [kijl]) from ff, the currents and IBRMEM = intf[:, 15]; linit sets those from nemo / nemoibr, with lwcou only where
        LKFR of fieldg <= 0.  lwcou defaults to LWCOU of the parameters.  flags (the lib.RNF_* bits) overrides the switches."""
        if flags is None:
            lwcou = self.t.cfg.lwcou if lwcou is None else lwcou
            flags = sum(b for b, on in ((_lib.RNF_LREST, lrest), (_lib.RNF_LINIT, linit), (_lib.RNF_LWCOU, lwcou), (_lib.RNF_LWNEMOCOUCIC, lwnemocoucic),
                                        (_lib.RNF_LWNEMOCOUCIT, lwnemocoucit), (_lib.RNF_LWNEMOCOUCUR, lwnemocoucur), (_lib.RNF_LWNEMOCOUIBR, lwnemocouibr)) if on)
        self._seam("RECVNEMOFIELDS", kijs, kijl, *[a for a in (ff, ucur, vcur, intf) if a is not None])

        def dbl(a, shape, name):
            if a is None:
                return None
            if not (a.is_cuda and a.dtype == torch.float64 and a.is_contiguous() and tuple(a.shape) == shape):
                raise ValueError(f"{name}: expected a contiguous float64 cuda tensor of shape {shape}")
            return a.data_ptr()
        opt = lambda a, name: None if a is None else self._real(a, (a.shape[0],), name)
        self._chk(self.lib.ecwam_hip_recvnemofields(self._h, int(kijs), int(kijl), int(flags), self._fieldg(fieldg), dbl(nemo, (4, kijl), "NEMO"),
                                                    dbl(nemoibr, (kijl,), "NEMOIBR"), None if ff is None else self._real(ff, (ff.shape[0], NFF), "FF"),
                                                    opt(ucur, "UCUR"), opt(vcur, "VCUR"),
                                                    None if intf is None else self._real(intf, (intf.shape[0], NINTF), "INTF"), _stream_ptr()))

    def updnemo(self, kijs, kijl, wam2nemo, nemontau: int, fields7=None, stress6=None):
        """UPDNEMOFIELDS into fields7 (float64 [7][ld]: NSWH, NMWP, NPHIEPS, NTAUOC, NEMOSTRN, NEMOUSTOKES, NEMOVSTOKES) and UPDNEMOSTRESS into stress6
        (float64 [6][ld]: NEMOTAUX, NEMOTAUY, NEMOWSWAVE, NEMOPHIF, NEMOTAUICX, NEMOTAUICY, each times 1 / nemontau; zeros with nemontau <= 0), from
        rows [kijs, kijl) of wam2nemo (float64 [>= kijl][13]), whose six accumulated columns become 0 with stress6.  Either output may be None."""
        if not (wam2nemo.is_cuda and wam2nemo.dtype == torch.float64 and wam2nemo.is_contiguous() and wam2nemo.dim() == 2 and wam2nemo.shape[1] == 13
                and 0 <= kijs <= kijl <= wam2nemo.shape[0]):
            raise ValueError("WAM2NEMO: expected a contiguous float64 cuda tensor [>= KIJL][13]")
        ld = None
        for a, nf, name in ((fields7, 7, "FIELDS7"), (stress6, 6, "STRESS6")):
            if a is None:
                continue
            if not (a.is_cuda and a.dtype == torch.float64 and a.is_contiguous() and a.dim() == 2 and a.shape[0] == nf and a.shape[1] >= kijl
                    and ld in (None, a.shape[1])):
                raise ValueError(f"{name}: expected a contiguous float64 cuda tensor [{nf}][ld], ld >= KIJL and the same for both outputs")
            ld = a.shape[1]
        self._chk(self.lib.ecwam_hip_updnemo(self._h, int(kijs), int(kijl), wam2nemo.data_ptr(), int(nemontau), None if fields7 is None else fields7.data_ptr(),
                                             None if stress6 is None else stress6.data_ptr(), int(ld if ld is not None else kijl), _stream_ptr()))

    # -- the forcing of a stand-alone run (include/ecwam_hip_readwind.h; csrc/readwind.hip): GRIB2WGRID, READWIND's fill, CURRENT2WAM
    def set_input_grid(self, slot: int, pos, w=None, kind=None, nvalues: int = 0, interpol: bool = True) -> None:
        """The per-cell table of GRIB2WGRID for one input grid (readwind.cell_table builds it) in slot 0 .. 3: pos host integers [ncell][4], the
        0-based positions in VALUES of the four corners (-1: a padded row); w host numbers [ncell][3], DK1, DII1, DIIP1 in the working precision;
        kind host integers [ncell] (0 outside the row, 1 PMISS, 2 interpolate); nvalues the length of VALUES.  interpol=False is LLINTERPOL = F:
        only pos[:, 0] is read.  pos=None removes the slot's table.  The library validates and uploads it."""
        if pos is None:
            self._chk(self.lib.ecwam_hip_set_input_grid(self._h, int(slot), 0, 0, None, None, None, 0))
            return
        a = np.ascontiguousarray(pos, dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("set_input_grid: pos is [ncell][4]")
        k = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32).reshape(-1)
        if k is not None and k.size != a.shape[0]:
            raise ValueError("set_input_grid: one kind per cell")
        pw = None
        if w is not None:
            pw = np.ascontiguousarray(w, dtype=np.float64)
            if pw.shape != (a.shape[0], 3):
                raise ValueError("set_input_grid: w is [ncell][3]")
        self._chk(self.lib.ecwam_hip_set_input_grid(self._h, int(slot), a.shape[0], int(nvalues), a.ctypes.data_as(C.c_void_p),
                                                    None if pw is None else pw.ctypes.data_as(C.c_void_p), None if k is None else k.ctypes.data_as(C.c_void_p),
                                                    int(bool(interpol))))

    def grib2wgrid(self, slot: int, values, fields, out=None, fieldg=None, roair: float = 1.225, wstar0: float = 0.0, pmiss: float = -999.0):
        """GRIB2WGRID (grib2wgrid.F90:783-1130) of the decoded vectors values [nfld][vstride] through the table of the slot, in one launch.  fields:
        per vector (target, flags) -- target lib.G2W_FIELD (FIELD as the routine returns it, into row f of out [nfld][ld]), or the name or number of a
        plane of fieldg [13][ncell] (lib.G2W_PLANES), filled by READWIND's rule (readwind.F90:341-494); flags the lib.G2W_DIRFLD / G2W_NONWAVE bits."""
        if values.dim() != 2 or len(fields) != values.shape[0]:
            raise ValueError("GRIB2WGRID: values is [nfld][vstride], one (target, flags) per vector")
        nf, vs = values.shape
        desc = (_lib.G2wField * max(nf, 1))()
        for f, (target, flags) in enumerate(fields):
            desc[f].target = _lib.FG_PLANES.index(target) if isinstance(target, str) else int(target)
            desc[f].flags = int(flags)
        po = None if out is None else self._real(out, (nf, out.shape[-1]), "OUT")
        pg = None
        if fieldg is not None:
            if fieldg.dim() != 2 or fieldg.shape[0] != len(_lib.FG_PLANES):
                raise ValueError("FIELDG: expected [13][ncell]")
            pg = self._real(fieldg, tuple(fieldg.shape), "FIELDG")
        self._chk(self.lib.ecwam_hip_grib2wgrid(self._h, int(slot), self._real(values, (nf, vs), "VALUES"), vs, nf, desc, float(roair), float(wstar0), float(pmiss),
                                                po, 0 if out is None else int(out.shape[-1]), pg, 0 if fieldg is None else int(fieldg.shape[1]), _stream_ptr()))

    def current2wam(self, kijs, kijl, field_u, field_v, ucur, vcur, wlowest: float, zmiss: float = -999.0, changed=None):
        """CURRENT2WAM's statements (current2wam.F90:253-259, 270-276) on rows [kijs, kijl) through the inbound map: field_u / field_v are FIELD
        planes [ncell_in] of grib2wgrid; a component given as None is left alone.  changed as in getcurr."""
        ncell = getattr(self, "_fmap", (0, 0, 0))[1]
        self._seam("CURRENT2WAM", kijs, kijl, *[c for f, c in ((field_u, ucur), (field_v, vcur)) if f is not None])
        fld = lambda a, name: None if a is None else self._real(a, (ncell,), name)
        cur = lambda f, a, name: None if f is None else self._real(a, (a.shape[0],), name)
        self._chk(self.lib.ecwam_hip_current2wam(self._h, int(kijs), int(kijl), fld(field_u, "FIELD_U"), fld(field_v, "FIELD_V"), float(wlowest), float(zmiss),
                                                 cur(field_u, ucur, "UCUR"), cur(field_v, vcur, "VCUR"),
                                                 None if changed is None else self._int(changed, (1,), "CHANGED"), _stream_ptr()))

    # -- the start and the end of a run (include/ecwam_hip_restart.h; csrc/restart.hip): INITDPTHFLDS, BUILDSTRESS, the restart fields and WRITEFL's record
    def depthprpt(self, kijs, kijl, depth, wvprpt=None, wavnum=None, cgroup=None, omosnh2kd=None, ff=None, dkmax: float = 40.0, gam_b_j: float | None = None):
        """INITDPTHFLDS with DEPTHPRPT and AKI on rows [kijs, kijl) from depth [>= kijl]: wvprpt [ij][5][NFRE] (WAVNUM, CGROUP, CINV, XK2CG, STOKFAC), the
        extended arrays wavnum / cgroup / omosnh2kd [ij][NFRE], and EMAXDPT, DEPTH of ff.  Any output may be None, not all.  The land slot of depth holds
        BATHYMAX and receives WVPRPT_LAND from the same call.  dkmax: yowpcons.F90; gam_b_j defaults to the tables'."""
        outs = [a for a in (wvprpt, wavnum, cgroup, omosnh2kd, ff) if a is not None]
        self._seam("DEPTHPRPT", kijs, kijl, depth, *outs)
        o = _lib.DepthOpts(float(dkmax), float(self.t.GAM_B_J if gam_b_j is None else gam_b_j))
        row = lambda a, name: None if a is None else self._real(a, (a.shape[0], self.NFRE), name)
        self._chk(self.lib.ecwam_hip_depthprpt(self._h, int(kijs), int(kijl), self._real(depth, (depth.shape[0],), "DEPTH"), C.byref(o),
                                               None if wvprpt is None else self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"), row(wavnum, "WAVNUM"),
                                               row(cgroup, "CGROUP"), row(omosnh2kd, "OMOSNH2KD"), None if ff is None else self._real(ff, (ff.shape[0], NFF), "FF"),
                                               _stream_ptr()))

    def buildstress(self, kijs, kijl, ff, uwave=None, cd=None, zref: float | None = None, z0b_zero: bool = True, nsestart: bool = False, prchar: float = 0.0185,
                    zmiss: float = -999.0):
        """BUILDSTRESS 1.2 to 1.5 with GETSTRESS's statements around it on rows [kijs, kijl) of ff: uwave / cd are planes [ncell_in] on the inbound map
        (READWGRIB with LLONLYPOS) or None; zref is TEMPXNLEV (default XNLEV); z0b_zero: Z0B = 0; nsestart: CHRNCK = prchar, TAUW = 0."""
        self._seam("BUILDSTRESS", kijs, kijl, ff)
        ncell = getattr(self, "_fmap", (0, 0, 0))[1]
        plane = lambda a, name: None if a is None else self._real(a, (ncell,), name)
        flags = (_lib.BST_Z0B_ZERO if z0b_zero else 0) | (_lib.BST_NSESTART if nsestart else 0)
        self._chk(self.lib.ecwam_hip_buildstress(self._h, int(kijs), int(kijl), plane(uwave, "UWAVE"), plane(cd, "CD"), float(self.t.XNLEV if zref is None else zref),
                                                 flags, float(prchar), float(zmiss), self._real(ff, (ff.shape[0], NFF), "FF"), _stream_ptr()))

    def set_restart_map(self, ij2newij) -> None:
        """IJ2NEWIJ, 0-based host integers [npts]: position p of a vector in the global order holds row ij2newij[p].  None removes the map.  The library
        validates that it is a permutation and uploads it."""
        if ij2newij is None:
            self._chk(self.lib.ecwam_hip_set_restart_map(self._h, 0, None))
            self._rmap = 0
            return
        a = np.ascontiguousarray(ij2newij, dtype=np.int32).reshape(-1)
        self._chk(self.lib.ecwam_hip_set_restart_map(self._h, a.size, a.ctypes.data_as(C.c_void_p)))
        self._rmap = a.size

    def _stress_fields(self, who, kijs, kijl, ff, ucur, vcur, rfield, relabel):
        self._seam(who, kijs, kijl, ff, ucur, vcur)
        if rfield.dim() != 2 or rfield.shape[0] != _lib.NRESTART_FIELDS or rfield.shape[1] < (getattr(self, "_rmap", 0) if relabel else kijl):
            raise ValueError(f"{who}: expected RFIELD [16][ld] with ld >= the rows of the call (the points of the map with relabel)")
        return (self._real(ff, (ff.shape[0], NFF), "FF"), self._real(ucur, (ucur.shape[0],), "UCUR"), self._real(vcur, (vcur.shape[0],), "VCUR"),
                self._real(rfield, tuple(rfield.shape), "RFIELD"))

    def savstress_pack(self, kijs, kijl, ff, ucur, vcur, rfield, relabel: bool = False):
        """The sixteen restart fields of SAVSTRESS (savstress.F90:112-127) of rows [kijs, kijl) into rfield [16][ld]; relabel: through the restart map."""
        pf, pu, pv, pr = self._stress_fields("SAVSTRESS", kijs, kijl, ff, ucur, vcur, rfield, relabel)
        self._chk(self.lib.ecwam_hip_savstress_pack(self._h, int(kijs), int(kijl), pf, pu, pv, int(bool(relabel)), pr, int(rfield.shape[1]), _stream_ptr()))

    def getstress_unpack(self, kijs, kijl, rfield, ff, ucur, vcur, relabel: bool = False):
        """The inverse (getstress.F90:150-165): rfield [16][ld] into FF_NOW's columns of ff and the currents on rows [kijs, kijl)."""
        pf, pu, pv, pr = self._stress_fields("GETSTRESS", kijs, kijl, ff, ucur, vcur, rfield, relabel)
        self._chk(self.lib.ecwam_hip_getstress_unpack(self._h, int(kijs), int(kijl), pr, int(rfield.shape[1]), int(bool(relabel)), pf, pu, pv, _stream_ptr()))

    def savspec_pack(self, kijs, kijl, fl1, blk, ifld0: int = 0, relabel: bool = False):
        """WRITEFL's record: fields [ifld0, ifld0 + blk.shape[0]) (f = M NANG + K, up to NANG * NFRE) of rows [kijs, kijl) of FL1 into blk [nfld][ld], as
        the values stand; relabel: row positions through the restart map (writefl.F90:117)."""
        if blk.dim() != 2:
            raise ValueError("SAVSPEC: expected BLK [nfld][ld]")
        nfld, ld = blk.shape
        nrow = fl1.shape[0]
        if not (0 <= ifld0 and 1 <= nfld <= self.NANG * self.NFRE - ifld0):
            raise ValueError(f"SAVSPEC: fields [{ifld0}, {ifld0 + nfld}) outside NANG * NFRE = {self.NANG * self.NFRE}")
        if not (0 <= kijs <= kijl <= nrow) or ld < (getattr(self, "_rmap", 0) if relabel else kijl):
            raise ValueError("SAVSPEC: KIJS/KIJL outside the operands, or vectors too short")
        self._chk(self.lib.ecwam_hip_savspec_pack(self._h, int(kijs), int(kijl), self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), int(ifld0), int(nfld),
                                                  int(bool(relabel)), self._real(blk, (nfld, ld), "BLK"), int(ld), _stream_ptr()))

    # -- GRIB-ready spectra and parameter fields (include/ecwam_hip_gribout.h; csrc/gribout.hip): from FL1 and BOUT to the encoder's VALUES
    def set_grib_map(self, ival, ntencode: int, poles=None) -> None:
        """ival: host integers, the 0-based position in VALUES of every row; poles: a gribout.Poles (or None: no padding).  gribout.value_map
        builds all three from the reference's variables.  The library validates and uploads them."""
        a = np.ascontiguousarray(ival, dtype=np.int32).reshape(-1)
        p = None
        if poles is not None:
            p = _lib.GribPoles(_lib.GribPole(*poles.as_ints()[:4]), _lib.GribPole(*poles.as_ints()[4:]))
        self._chk(self.lib.ecwam_hip_set_grib_map(self._h, a.size, a.ctypes.data_as(C.c_void_p), int(ntencode), None if p is None else C.byref(p)))
        self._gmap = (a.size, int(ntencode))

    @staticmethod
    def _grib_opts(opts) -> _lib.GribOpts:
        from .gribout import GRIB_DEFAULTS
        unknown = set(opts or ()) - set(GRIB_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown GRIB options {sorted(unknown)}")
        o = dict(GRIB_DEFAULTS, **(opts or {}))
        return _lib.GribOpts(float(o["ppmiss"]), float(o["ppeps"]), float(o["pprec"]), float(o["ppresol"]), float(o["ppmin_reset"]), int(o["ngrbress"]), float(o["zmiss"]))

    def _grib_out(self, who, values, nfld, ppmax):
        ntencode = getattr(self, "_gmap", (0, 0))[1]
        return self._real(values, (nfld, ntencode), f"{who}: VALUES"), None if ppmax is None else self._real(ppmax, (nfld,), f"{who}: PPMAX")

    def _fields(self, who, ifld0, nfld):
        nfld = self.NANG * self.NR - ifld0 if nfld is None else nfld
        if not (0 <= ifld0 and 1 <= nfld <= self.NANG * self.NR - ifld0):
            raise ValueError(f"{who}: fields [{ifld0}, {ifld0 + nfld}) outside NANG * NFRE_RED = {self.NANG * self.NR}")
        return int(ifld0), int(nfld)

    def outspec_values(self, kijs, kijl, fl1, values, ff=None, ifld0: int = 0, nfld: int | None = None, ice_mask: bool = False, opts=None, ppmax=None):
        """The one-task OUTSPEC on rows [kijs, kijl): fields [ifld0, ifld0 + nfld) (f = M NANG + K, M < NFRE_RED) of FL1 into values [nfld][NTENCODE]
        through the map of set_grib_map -- ice mask (ice_mask = LICERUN .AND. LLSOURCE, reads CICOVER of ff), pole padding, LOG10 scale, threshold
        to missing.  opts: the entries of gribout.GRIB_DEFAULTS to override; ppmax [nfld] receives PPMAX per field."""
        ifld0, nfld = self._fields("OUTSPEC", ifld0, nfld)
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= (nrow if ff is None else min(nrow, ff.shape[0]))):
            raise ValueError("OUTSPEC: KIJS/KIJL outside the operands")
        if ice_mask and ff is None:
            raise ValueError("OUTSPEC: the ice mask reads FF")
        o = self._grib_opts(opts)
        pv, pm = self._grib_out("OUTSPEC", values, nfld, ppmax)
        self._chk(self.lib.ecwam_hip_outspec_values(self._h, kijs, kijl, self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"),
                                                    None if ff is None else self._real(ff, (ff.shape[0], NFF), "FF"), ifld0, nfld,
                                                    _lib.OUTSPEC_ICEMASK if ice_mask else 0, C.byref(o), pv, pm, _stream_ptr()))

    def outspec_pack(self, kijs, kijl, fl1, blk, ff=None, ifld0: int = 0, ice_mask: bool = False):
        """The sending half of the many-task OUTSPEC: the ice mask, then fields [ifld0, ifld0 + blk.shape[0]) of rows [kijs, kijl) into
        blk [nfld][ld], field-major (ZSENDBUF of outwspec.F90:186-195)."""
        if blk.dim() != 2:
            raise ValueError("OUTSPEC: expected BLK [nfld][ld]")
        ifld0, nfld = self._fields("OUTSPEC", ifld0, blk.shape[0])
        nrow, ld = fl1.shape[0], blk.shape[1]
        if not (0 <= kijs <= kijl <= min(ld, nrow if ff is None else min(nrow, ff.shape[0]))):
            raise ValueError("OUTSPEC: KIJS/KIJL outside the operands")
        if ice_mask and ff is None:
            raise ValueError("OUTSPEC: the ice mask reads FF")
        self._chk(self.lib.ecwam_hip_outspec_pack(self._h, kijs, kijl, self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"),
                                                  None if ff is None else self._real(ff, (ff.shape[0], NFF), "FF"), ifld0, nfld,
                                                  _lib.OUTSPEC_ICEMASK if ice_mask else 0, self._real(blk, (nfld, ld), "BLK"), ld, _stream_ptr()))

    def grib_values(self, kijs, kijl, src, values, spectral: bool, columns=None, opts=None, ppmax=None):
        """MAKEGRID + WGRIBENCODE_VALUES on rows [kijs, kijl) of block vectors.  Without columns, src is [nfld][ld] field-major (the gathered
        ZRECVBUF, or the blk of outspec_pack); with columns, src is [npts][ncol] point-major (BOUT) and columns lists the ones to take, in the
        order of values: one call goes to the library per run of consecutive columns.  spectral: the LOG10 scale and the threshold as well."""
        if src.dim() != 2 or not (src.is_cuda and src.dtype == self.dtype and src.is_contiguous()):
            raise ValueError(f"GRIB_VALUES: expected a contiguous two-dimensional {self.dtype} cuda tensor")
        o = self._grib_opts(opts)
        rb = self.real_bytes
        if columns is None:
            nfld, ld = src.shape
            runs = [(0, 0, nfld)]
            fs, ps, rows = ld, 1, ld
        else:
            cols = [int(c) for c in columns]
            rows, ncol = src.shape
            if not cols or min(cols) < 0 or max(cols) >= ncol:
                raise ValueError("GRIB_VALUES: a column outside the source")
            nfld, fs, ps = len(cols), 1, ncol
            runs, a = [], 0      # (first field of values, first column of src, length)
            for i in range(1, nfld + 1):
                if i == nfld or cols[i] != cols[i - 1] + 1:
                    runs.append((a, cols[a], i - a))
                    a = i
        if not (0 <= kijs <= kijl <= rows):
            raise ValueError("GRIB_VALUES: KIJS/KIJL outside the operands")
        pv, pm = self._grib_out("GRIB_VALUES", values, nfld, ppmax if spectral else None)
        ntencode = self._gmap[1] if hasattr(self, "_gmap") else 0
        for f0, c0, n in runs:
            self._chk(self.lib.ecwam_hip_grib_values(self._h, kijs, kijl, src.data_ptr() + c0 * rb, fs, ps, n, 1 if spectral else 0, C.byref(o),
                                                     pv + f0 * ntencode * rb, None if pm is None else pm + f0 * rb, _stream_ptr()))

    # -- the warm start (include/ecwam_hip_gribin.h; csrc/gribin.hip): decoded GRIB spectra and READFL's record into FL1
    def _getspec(self, call, who, kijs, kijl, src, stride_min, fl1, ifld0, fmax, unscale, missing, opts):
        if src.dim() != 2 or not (src.is_cuda and src.dtype == self.dtype and src.is_contiguous()):
            raise ValueError(f"{who}: expected a contiguous two-dimensional {self.dtype} cuda tensor of field vectors")
        nfld, stride = src.shape
        if not (0 <= ifld0 and 1 <= nfld <= fmax - ifld0):
            raise ValueError(f"{who}: fields [{ifld0}, {ifld0 + nfld}) outside [0, {fmax})")
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= nrow) or stride < stride_min:
            raise ValueError(f"{who}: KIJS/KIJL outside the operands, or vectors shorter than {stride_min}")
        flags = (_lib.GETSPEC_UNSCALE if unscale else 0) | (_lib.GETSPEC_MISSING if missing else 0)
        o = self._grib_opts(opts)
        self._chk(call(self._h, kijs, kijl, src.data_ptr(), stride, int(ifld0), nfld, flags, C.byref(o) if flags else None,
                       self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), _stream_ptr()))

    def getspec_values(self, kijs, kijl, values, fl1, ifld0: int = 0, unscale: bool = True, missing: bool = True, opts=None):
        """GETSPEC's GRIB read on one task for rows [kijs, kijl): values [nfld][>= NTENCODE], the decoded vectors of the fields
        [ifld0, ifld0 + nfld) (f = M NANG + K, M < NFRE_RED) as eccodes returned them, through the map of set_grib_map into FL1[ij][K][M].
        unscale: 10**(v - |PPREC|) - PPEPS where v /= ZMISS (grib2wgrid.F90:771-775); missing: then ZMISS -> EPSMIN (getspec.F90:550-552).
        Every other element of FL1 keeps its bits; getspec_tail follows the last field."""
        self._getspec(self.lib.ecwam_hip_getspec_values, "GETSPEC", kijs, kijl, values, getattr(self, "_gmap", (0, 0))[1], fl1, ifld0,
                      self.NANG * self.NR, unscale, missing, opts)

    def getspec_unpack(self, kijs, kijl, blk, fl1, ifld0: int = 0, unscale: bool = False, missing: bool = False, opts=None):
        """The receiving half of GETSPEC on many tasks (ZRECVBUF, getspec.F90:602-619) and READFL's record: blk [nfld][ld], row ij at index ij
        (the convention of outspec_pack), fields [ifld0, ifld0 + nfld) up to NANG * NFRE, into FL1[ij][K][M] for rows [kijs, kijl).  Without
        flags the values pass as they are (the restart record)."""
        self._getspec(self.lib.ecwam_hip_getspec_unpack, "GETSPEC", kijs, kijl, blk, kijl, fl1, ifld0, self.NANG * self.NFRE, unscale, missing, opts)

    # -- nested grids: BOUINPT / INTSPEC (bouinpt.F90:385-424) and OUTBC (outbc.F90:78-91), the two calls of wamodel.F90:333-343
    def bouinpt(self, kijs, kijl, ijb, ibcl, ibcr, bfw, f1, par1, fl1, par_out=None):
        """The coarse model's boundary spectra into the rows ijb (0-based, distinct) of FL1 that lie in [kijs, kijl): ibcl / ibcr = IBFL / IBFR
        (0 = land, 1 .. nboinp), bfw = BFW; f1 [nboinp][NFRE][NANG] and par1 [nboinp][3] = EMEAN, THQ, FMEAN as the boundary file holds them.
        par_out [nijb][3] (optional) receives EMEAN, THQ, FMEAN of the result."""
        nrow, nijb, nboinp = fl1.shape[0], ijb.shape[0], f1.shape[0]
        if not (0 <= kijs <= kijl <= nrow):
            raise ValueError("BOUINPT: KIJS/KIJL outside FL1")
        a = [self._int(ijb, (nijb,), "IJB"), self._int(ibcl, (nijb,), "IBFL"), self._int(ibcr, (nijb,), "IBFR"), self._real(bfw, (nijb,), "BFW"), nboinp,
             self._real(f1, (nboinp, self.NFRE, self.NANG), "F1"), self._real(par1, (nboinp, 3), "PAR1"), self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"),
             None if par_out is None else self._real(par_out, (nijb, 3), "PAR_OUT")]
        self._chk(self.lib.ecwam_hip_bouinpt(self._h, kijs, kijl, nijb, *a, _stream_ptr()))

    def outbc(self, ijarc, fl1, flpts, par=None):
        """Rows ijarc (0-based) of FL1 into flpts [nbc][NFRE][NANG] (the order of the boundary file's record) and, unless par is None, their
        EMEAN, THQ [radians], FMEAN into par [nbc][3]."""
        nrow, nbc = fl1.shape[0], ijarc.shape[0]
        a = [self._int(ijarc, (nbc,), "IJARC"), self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), self._real(flpts, (nbc, self.NFRE, self.NANG), "FLPTS"),
             None if par is None else self._real(par, (nbc, 3), "PAR")]
        self._chk(self.lib.ecwam_hip_outbc(self._h, nbc, *a, _stream_ptr()))

    # -- the one-kernel step: PROPAGS2 inside IMPLSCH's tile load (ecwam_hip_propags2_implsch)
    def fused_supported(self, fast_waves: bool = False, obstructions: bool = False) -> bool:
        """The one-kernel step covers the context (and, if asked, its forms with fast-wave sub-steps / sub-grid obstructions)."""
        mask = int(self.lib.ecwam_hip_propags2_implsch_supported(self._h))
        need = 1 | (2 if fast_waves else 0) | (4 if obstructions else 0)
        return (mask & need) == need

    def propags2_implsch(self, f1, f3, grid_dev: dict, cgroup_ext, delpro: float, kijs, kijl, wvprpt, ff, intf, mij, xllws, nd3s=1, nd3e=None,
                         wam2nemo=None, flags: int = 0, ifrelfmax: int = 0, delpro_lf: float | None = None, gin=None):
        """Rows [kijs, kijl): advect from the rows of f1 (read only) and integrate the source terms; the new spectrum goes to the rows of f3.
        Bit for bit propags2_otf(f1 -> f3) followed by implsch(f3).  ifrelfmax > 0 with gin: frequencies 1..ifrelfmax advance with delpro_lf
        from the compact rows gin [nrow][NANG][w] (the last fast-wave sub-step), the others with delpro from f1."""
        nd3e = self.NR if nd3e is None else nd3e
        g = grid_dev
        n, nland, ngy = g["n"], g["nland"], g["ngy"]
        nrow = f1.shape[0]
        if not (0 <= kijs <= kijl <= n) or nland >= nrow or cgroup_ext.shape[0] != nrow or f3.shape[0] < kijl:
            raise ValueError("PROPAGS2 + IMPLSCH: KIJS/KIJL outside the neighbour tables, or F1 / CGROUP_EXT without the land row")
        if not (kijl <= min(wvprpt.shape[0], ff.shape[0], intf.shape[0], mij.shape[0], xllws.shape[0])):
            raise ValueError("PROPAGS2 + IMPLSCH: KIJL outside the operands")
        pw = None
        if wam2nemo is not None:
            if not (wam2nemo.is_cuda and wam2nemo.dtype == torch.float64 and wam2nemo.is_contiguous() and wam2nemo.dim() == 2
                    and wam2nemo.shape[1] == 13 and wam2nemo.shape[0] >= kijl):
                raise ValueError("WAM2NEMO: expected contiguous float64 cuda tensor [npts >= KIJL][13]")
            pw = wam2nemo.data_ptr()
        args = [self._real(f1, (nrow, self.NANG, self.NFRE), "F1"), self._real(f3, (f3.shape[0], self.NANG, self.NFRE), "F3"), n, ngy, float(delpro),
                self._int(g["kxlt"], (n,), "KXLT"), self._real(g["zdello"], (ngy,), "ZDELLO"), float(g["xdella"]),
                self._real(g["cosph"], (ngy,), "COSPH"), self._real(g["sinph"], (ngy,), "SINPH"),
                self._int(g["klon"], (n, 2), "KLON"), self._int(g["klat"], (n, 2, 2), "KLAT"), self._int(g["kcor"], (n, 4, 2), "KCOR"),
                self._real(g["wlat"], (n, 2), "WLAT"), self._real(g["wcor"], (n, 4), "WCOR"),
                self._real(cgroup_ext, (nrow, self.NFRE), "CGROUP_EXT"), self._real(g["cosphm1_ext"], (nrow,), "COSPHM1_EXT"), kijs, kijl, nd3s, nd3e,
                self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"), self._real(ff, (ff.shape[0], NFF), "FF"),
                self._real(intf, (intf.shape[0], NINTF), "INTF"), self._int(mij, (mij.shape[0],), "MIJ"),
                self._real(xllws, (xllws.shape[0], self.NANG, self.NFRE), "XLLWS"), pw,
                float(delpro if delpro_lf is None else delpro_lf), int(ifrelfmax),
                None if gin is None else self._real(gin, (gin.shape[0], self.NANG, gin.shape[2]), "GIN"), 0 if gin is None else int(gin.shape[2]),
                int(flags), _stream_ptr()]
        self._chk(self.lib.ecwam_hip_propags2_implsch(self._h, *args))

    def implsch_reserve(self, npts: int) -> None:
        """Size the per-point scalar rows of the IMPLSCH kernels once, outside the time loop: ecwam_hip_implsch_reserve."""
        self._chk(self.lib.ecwam_hip_implsch_reserve(self._h, int(npts)))

    def implsch_generation_used(self) -> int:
        """Kernel generation the last implsch() call launched: 4 (k_implsch4) since the one-point-per-wavefront kernel left the product."""
        return int(self.lib.ecwam_hip_implsch_generation_used(self._h))

    def device_tables(self) -> int:
        """Address of the device copy of the module tables (ecwam_hip_device_tables): diagnostics, the tests' second IMPLSCH implementation."""
        return int(self.lib.ecwam_hip_device_tables(self._h) or 0)

    def outbs(self, kijs, kijl, fl1, out, zmiss: float = -999.0):
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, out.shape[0])):
            raise ValueError("OUTBS: KIJS/KIJL outside the operands")
        self._chk(self.lib.ecwam_hip_outbs(self._h, kijs, kijl, self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), float(zmiss),
                                           self._real(out, (out.shape[0], 5), "OUT"), _stream_ptr()))

    def outbs_sepwisw(self, kijs, kijl, fl1, xllws, wvprpt, ff, out, zmiss: float = -999.0, small_domain: bool = False):
        """Wind sea / swell and mean-period / spread parameters (ecwam_hip_outbs_sepwisw) of rows [kijs, kijl) into out[:, 15], columns
        OUTBS_SEP_FIELDS.  small_domain: CLDOMAIN = 's' (the first wind-sea mask only)."""
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, xllws.shape[0], wvprpt.shape[0], ff.shape[0], out.shape[0])):
            raise ValueError("OUTBS_SEPWISW: KIJS/KIJL outside the operands")
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), self._real(xllws, (xllws.shape[0], self.NANG, self.NFRE), "XLLWS"),
             self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"), self._real(ff, (ff.shape[0], NFF), "FF")]
        self._chk(self.lib.ecwam_hip_outbs_sepwisw(self._h, kijs, kijl, *a, 1 if small_domain else 0, float(zmiss),
                                                   self._real(out, (out.shape[0], len(OUTBS_SEP_FIELDS)), "OUT"), _stream_ptr()))

    def outbs_partition(self, kijs, kijl, fl1, xllws, mij, wvprpt, ff, out, zmiss: float = -999.0, flags: int = 0):
        """Swell-train partitioning (ecwam_hip_outbs_partition: SEPWISW with LLPARTITION = T) of rows [kijs, kijl) into out[:, 24], columns
        OUTBS_PART_FIELDS.  mij: the int32 MIJ of implsch() (1-based).  flags: 0 only (the library refuses every bit)."""
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, xllws.shape[0], mij.shape[0], wvprpt.shape[0], ff.shape[0], out.shape[0])):
            raise ValueError("OUTBS_PARTITION: KIJS/KIJL outside the operands")
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), self._real(xllws, (xllws.shape[0], self.NANG, self.NFRE), "XLLWS"),
             self._int(mij, (mij.shape[0],), "MIJ"), self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"),
             self._real(ff, (ff.shape[0], NFF), "FF")]
        self._chk(self.lib.ecwam_hip_outbs_partition(self._h, kijs, kijl, *a, int(flags), float(zmiss),
                                                     self._real(out, (out.shape[0], len(OUTBS_PART_FIELDS)), "OUT"), _stream_ptr()))

    def outbs_extremes(self, kijs, kijl, fl1, wvprpt, ff, out, kurtosis_only: bool = False):
        """Extreme-wave parameters (ecwam_hip_outbs_extremes: KURTOSIS and W_MAXH) of rows [kijs, kijl) into out[:, 13], columns
        OUTBS_EXT_FIELDS.  kurtosis_only: W_MAXH skipped, columns 9-12 left as they are."""
        nrow = fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, wvprpt.shape[0], ff.shape[0], out.shape[0])):
            raise ValueError("OUTBS_EXTREMES: KIJS/KIJL outside the operands")
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"),
             self._real(ff, (ff.shape[0], NFF), "FF")]
        self._chk(self.lib.ecwam_hip_outbs_extremes(self._h, kijs, kijl, *a, 1 if kurtosis_only else 0,
                                                    self._real(out, (out.shape[0], len(OUTBS_EXT_FIELDS)), "OUT"), _stream_ptr()))

    def outbs_absolute(self, kijs, kijl, fl1, wvprpt, ucur, vcur, ff, out, fl2nd=None, zmiss: float = -999.0, flags: int = 0):
        """The parameters of the output spectrum FL2ND (ecwam_hip_outbs_absolute: INTPOL to the absolute frame when IREFRA = 2 / 3, the ice
        noise reshaping when LICERUN and not LMASKICE) of rows [kijs, kijl) into out[:, 8], columns OUTBS_ABS_FIELDS.  ucur / vcur: reals
        [>= kijl], within [-1.5, 1.5] m/s (None when IREFRA is 0 or 1, as wvprpt).  fl2nd: receives FL2ND when given."""
        nrow = fl1.shape[0]
        rows = [nrow, out.shape[0]] + [a.shape[0] for a in (wvprpt, ucur, vcur, ff, fl2nd) if a is not None]
        if not (0 <= kijs <= kijl <= min(rows)):
            raise ValueError("OUTBS_ABSOLUTE: KIJS/KIJL outside the operands")
        opt = lambda a, shape, name: None if a is None else self._real(a, shape, name)
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"),
             opt(wvprpt, (0 if wvprpt is None else wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"),
             opt(ucur, (0 if ucur is None else ucur.shape[0],), "UCUR"), opt(vcur, (0 if vcur is None else vcur.shape[0],), "VCUR"),
             opt(ff, (0 if ff is None else ff.shape[0], NFF), "FF")]
        self._chk(self.lib.ecwam_hip_outbs_absolute(self._h, kijs, kijl, *a, int(flags), float(zmiss),
                                                    self._real(out, (out.shape[0], len(OUTBS_ABS_FIELDS)), "OUT"),
                                                    opt(fl2nd, (0 if fl2nd is None else fl2nd.shape[0], self.NANG, self.NFRE), "FL2ND"), _stream_ptr()))

    # -- LSECONDORDER: the tables of SECONDHH_GEN / TABLES_2ND (ecwam_amd.second_order.SecondOrderTables), or five arrays in their place
    @property
    def has_second_order(self) -> bool:
        return getattr(self, "_second_order", False)

    def set_second_order(self, so, coefficients=None) -> None:
        """Upload the second-order tables (ecwam_hip_set_second_order).  so: a SecondOrderTables of this context's grid and precision, or
        None to remove them.  coefficients: five arrays [NDEPTH][NANGH][NFREH][NFREH] used in place of so.TA, TB, TC_QL, TT_4M, TT_4P."""
        self._second_order = False      # the library drops its tables first: a failed upload leaves none
        if so is None:
            self._chk(self.lib.ecwam_hip_set_second_order(self._h, 0, 1.0, 1.1, 0, None, None, None, None, None, None, None))
            return
        dt = self.t.dtype
        if so.dtype != dt or so.NANGH * 2 != self.NANG or so.NFREH * 2 != self.NFRE:
            raise ValueError("second-order tables of another grid or precision")
        tabs = [getattr(so, c) for c in so.COEFFICIENTS] if coefficients is None else list(coefficients)
        shape = (so.NDEPTH, so.NANGH, so.NFREH, so.NFREH)
        # the C interface takes the reference's storage order TA(JD,L,M1,M): C order [M][M1][L][JD]
        host = [np.ascontiguousarray(np.asarray(a, dt).reshape(shape).transpose(3, 2, 1, 0)) for a in tabs]
        imp = np.ascontiguousarray(so.IM_P.T.astype(np.int32))
        imm = np.ascontiguousarray(so.IM_M.T.astype(np.int32))
        self._chk(self.lib.ecwam_hip_set_second_order(self._h, so.NDEPTH, float(so.DEPTHA), float(so.DEPTHD), so.NMAX, imp.ctypes.data, imm.ctypes.data,
                                                      *[a.ctypes.data for a in host]))
        self._second_order = True

    def outbs_second_order(self, kijs, kijl, fl1, wvprpt, depth, ucur, vcur, ff, out, fl2nd=None, sig: float = 1.0, zmiss: float = -999.0):
        """outbs_absolute with CAL_SECOND_ORDER_SPEC between INTPOL and the ice noise reshaping (ecwam_hip_outbs_second_order; LSECONDORDER = T):
        out[:, 8] in the columns OUTBS_ABS_FIELDS.  depth: reals [>= kijl]; wvprpt is always needed; sig = -1 removes the correction.  Needs
        set_second_order()."""
        nrow = fl1.shape[0]
        rows = [nrow, out.shape[0], wvprpt.shape[0], depth.shape[0]] + [a.shape[0] for a in (ucur, vcur, ff, fl2nd) if a is not None]
        if not (0 <= kijs <= kijl <= min(rows)):
            raise ValueError("OUTBS_SECOND_ORDER: KIJS/KIJL outside the operands")
        opt = lambda a, shape, name: None if a is None else self._real(a, shape, name)
        a = [self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"), self._real(wvprpt, (wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"),
             self._real(depth, (depth.shape[0],), "DEPTH"),
             opt(ucur, (0 if ucur is None else ucur.shape[0],), "UCUR"), opt(vcur, (0 if vcur is None else vcur.shape[0],), "VCUR"),
             opt(ff, (0 if ff is None else ff.shape[0], NFF), "FF")]
        self._chk(self.lib.ecwam_hip_outbs_second_order(self._h, kijs, kijl, *a, float(sig), float(zmiss),
                                                        self._real(out, (out.shape[0], len(OUTBS_ABS_FIELDS)), "OUT"),
                                                        opt(fl2nd, (0 if fl2nd is None else fl2nd.shape[0], self.NANG, self.NFRE), "FL2ND"),
                                                        _stream_ptr()))

    # -- OUTBLOCK's remaining spectral integrals (ecwam_hip_outbs_integrals) and OUTSETWMASK
    @property
    def integral_bands(self):
        """The (TB, TT) bands of the last set_outbs_integrals(), None before it."""
        return getattr(self, "_int_bands", None)

    def default_bands(self):
        """The reference's seven bands: SE10MEAN = (10, 1/FR(1)), then 10-12, 12-14, 14-17, 17-21, 21-25 and 25-30 s (outblock.F90:460, 515-519)."""
        return [(10.0, float(np.dtype(self.t.dtype).type(1.0) / self.t.FR[0]))] + [(10.0, 12.0), (12.0, 14.0), (14.0, 17.0), (17.0, 21.0), (21.0, 25.0), (25.0, 30.0)]

    def set_outbs_integrals(self, xkmss_cutoff: float = 0.0, bands=None) -> None:
        """The cut-off of the mean square slope (<= 0: XK_GC(NWAV_GC)) and the period bands [(TB, TT), ...] of outbs_integrals();
        bands = None: default_bands().  Uploads DELKCC_GC of the context's tables."""
        bands = self.default_bands() if bands is None else [(float(a), float(b)) for a, b in bands]
        tb = np.ascontiguousarray([b[0] for b in bands], dtype=np.float64)
        tt = np.ascontiguousarray([b[1] for b in bands], dtype=np.float64)
        d = np.ascontiguousarray(self.t.DELKCC_GC, dtype=self.t.dtype)
        self._int_bands = None      # a refused call leaves the previous table in the library, but this layer forgets it
        self._chk(self.lib.ecwam_hip_set_outbs_integrals(self._h, float(xkmss_cutoff), len(bands), tb.ctypes.data if len(bands) else None,
                                                         tt.ctypes.data if len(bands) else None, d.ctypes.data))
        self._int_bands = bands

    def outbs_integrals(self, kijs, kijl, fl1, wvprpt, ff, out, fl2nd=None, groups=OUTBS_INT_ALL, zmiss: float = -999.0):
        """Drag, normalised wave stress, mean square slopes, ice strain, energy flux, crest-trough correlation and band heights
        (ecwam_hip_outbs_integrals) of rows [kijs, kijl) into out[:, 8 + nband], columns OUTBS_INT_FIELDS then the bands.  fl2nd: the output
        spectrum stored by outbs_absolute() / outbs_second_order() for the bands, None: FL1.  groups: a sum of OUTBS_INT_GROUPS values."""
        rows = [out.shape[0]] + [a.shape[0] for a in (fl1, wvprpt, ff, fl2nd) if a is not None]
        if not (0 <= kijs <= kijl <= min(rows)):
            raise ValueError("OUTBS_INTEGRALS: KIJS/KIJL outside the operands")
        opt = lambda a, shape, name: None if a is None else self._real(a, shape, name)
        nb = len(self._int_bands) if self.integral_bands is not None else out.shape[1] - len(OUTBS_INT_FIELDS)
        a = [opt(fl1, (0 if fl1 is None else fl1.shape[0], self.NANG, self.NFRE), "FL1"),
             opt(fl2nd, (0 if fl2nd is None else fl2nd.shape[0], self.NANG, self.NFRE), "FL2ND"),
             opt(wvprpt, (0 if wvprpt is None else wvprpt.shape[0], NWPR, self.NFRE), "WVPRPT"), opt(ff, (0 if ff is None else ff.shape[0], NFF), "FF")]
        self._chk(self.lib.ecwam_hip_outbs_integrals(self._h, kijs, kijl, *a, int(groups), float(zmiss),
                                                     self._real(out, (out.shape[0], len(OUTBS_INT_FIELDS) + nb), "OUT"), _stream_ptr()))

    def outsetwmask(self, kijs, kijl, out, colflags, ff=None, iodp=None, cithrsh: float | None = None, zmiss: float = -999.0):
        """OUTSETWMASK (ecwam_hip_outsetwmask) on rows [kijs, kijl) of an output buffer, in place.  colflags: per column, 1 = sea-ice mask
        (zmiss where CICOVER = ff[:, 2] > cithrsh; only with LICERUN), 2 = sea mask out*IODP + (1-IODP)*zmiss, 3 = both.  cithrsh: default
        CITHRSH of the tables."""
        if not (out.is_cuda and out.dtype == self.dtype and out.is_contiguous() and out.dim() == 2):
            raise ValueError("OUTSETWMASK: expected a contiguous 2-D cuda tensor in the working precision")
        cf = np.ascontiguousarray(colflags, dtype=np.int32)
        if cf.shape != (out.shape[1],):
            raise ValueError("OUTSETWMASK: one flag per column")
        rows = [out.shape[0]] + [a.shape[0] for a in (ff, iodp) if a is not None]
        if not (0 <= kijs <= kijl <= min(rows)):
            raise ValueError("OUTSETWMASK: KIJS/KIJL outside the operands")
        pff = None if ff is None else self._real(ff, (ff.shape[0], NFF), "FF")
        pio = None if iodp is None else self._int(iodp, (iodp.shape[0],), "IODP")
        self._chk(self.lib.ecwam_hip_outsetwmask(self._h, kijs, kijl, out.data_ptr(), out.shape[1], cf.ctypes.data, pff, pio,
                                                 float(self.t.CITHRSH if cithrsh is None else cithrsh), float(zmiss), _stream_ptr()))

    # -- OUTBLOCK as one call (ecwam_hip_set_outblock / ecwam_hip_outblock_plan / ecwam_hip_outblock)
    def set_outblock(self, requested, itobout=None, niprmout=None, second_order: bool = False, small_domain: bool = False, llsource: bool = True):
        """The request of outblock(): parameter numbers (or a mapping parameter -> IPFGTBL value).  itobout / niprmout: ITOBOUT(1:JPPFLAG) and the
        number of columns when the host has its own; default: outblock_tables().  The masks are those of OUTBLOCK_PARAMS.  second_order:
        LSECONDORDER; small_domain: CLDOMAIN = 's'; llsource = False: no sea-ice mask.  Returns {parameter: 0-based column}."""
        ipf, ito, n = outblock_tables(requested)
        if itobout is not None:
            ito = np.ascontiguousarray(itobout, dtype=np.int32)
            if ito.shape != (JPPFLAG,):
                raise ValueError(f"OUTBLOCK: ITOBOUT has {JPPFLAG} entries")
        n = n if niprmout is None else int(niprmout)
        ice = np.ascontiguousarray([int(p[2]) for p in OUTBLOCK_PARAMS], dtype=np.int32)
        sea = np.ascontiguousarray([int(p[3]) for p in OUTBLOCK_PARAMS], dtype=np.int32)
        flags = (1 if second_order else 0) | (2 if small_domain else 0) | (0 if llsource else 4)
        self._outblock = None      # a refused call leaves the previous plan in the library, but this layer forgets it
        self._chk(self.lib.ecwam_hip_set_outblock(self._h, JPPFLAG, ipf.ctypes.data, ito.ctypes.data, ice.ctypes.data, sea.ctypes.data, n, flags))
        self._outblock = dict(niprmout=n, columns={ir + 1: int(ito[ir]) - 1 for ir in range(JPPFLAG) if ipf[ir] != 0})
        return dict(self._outblock["columns"])

    def outblock_plan(self) -> dict:
        """What outblock() will run: calls (names of OUTBLOCK_CALLS), int_groups (a sum of OUTBS_INT_GROUPS values), w_maxh, stores_fl2nd."""
        calls, st = C.c_int(0), C.c_int(0)
        self._chk(self.lib.ecwam_hip_outblock_plan(self._h, C.byref(calls), C.byref(st)))
        m = int(calls.value)
        return dict(calls=tuple(nm for i, nm in enumerate(OUTBLOCK_CALLS) if m >> i & 1), int_groups=(m >> 8) & 63, w_maxh=bool(m >> 14 & 1),
                    stores_fl2nd=bool(st.value), mask=m)

    def outblock(self, kijs, kijl, bout, fl1=None, xllws=None, mij=None, wvprpt=None, ff=None, intf=None, ucur=None, vcur=None, iodp=None, ibrmem=None,
                 altim=None, nemo=None, cithrsh: float | None = None, zmiss: float = -999.0):
        """Rows [kijs, kijl) of bout[:, NIPRMOUT] as OUTBLOCK fills them (ecwam_hip_outblock), for the request of set_outblock().  Operands no
        requested parameter reads may be None.  altim: reals [3][>= kijl] (ALTWH, CALTWH, RALTCOR); nemo: float64 [4][>= kijl] (NEMOCICOVER,
        NEMOCITHICK, NEMOUCUR, NEMOVCUR); ibrmem: reals [>= kijl]; iodp: int32 [>= kijl]."""
        ob = getattr(self, "_outblock", None)
        ncol = ob["niprmout"] if ob else bout.shape[1]      # without a plan the library refuses
        opt = lambda a, shape, name: None if a is None else self._real(a, shape, name)
        rows = [bout.shape[0]] + [a.shape[0] for a in (fl1, xllws, mij, wvprpt, ff, intf, ucur, vcur, iodp, ibrmem) if a is not None]
        rows += [a.shape[1] for a in (altim, nemo) if a is not None]
        if not (0 <= kijs <= kijl <= min(rows)):
            raise ValueError("OUTBLOCK: KIJS/KIJL outside the operands")

        def planes(a, k, dtype, name):       # the library takes planes of exactly kijl points
            if a is None:
                return None
            if not (a.is_cuda and a.dtype == dtype and a.dim() == 2 and a.shape[0] == k):
                raise ValueError(f"{name}: expected a {dtype} cuda tensor [{k}][>= KIJL]")
            return a[:, :kijl].contiguous()
        pa, pn = planes(altim, 3, self.dtype, "ALTIM"), planes(nemo, 4, torch.float64, "NEMO")
        r0 = lambda a: 0 if a is None else a.shape[0]
        args = [opt(fl1, (r0(fl1), self.NANG, self.NFRE), "FL1"), opt(xllws, (r0(xllws), self.NANG, self.NFRE), "XLLWS"),
                None if mij is None else self._int(mij, (mij.shape[0],), "MIJ"), opt(wvprpt, (r0(wvprpt), NWPR, self.NFRE), "WVPRPT"),
                opt(ff, (r0(ff), NFF), "FF"), opt(intf, (r0(intf), NINTF), "INTF"), opt(ucur, (r0(ucur),), "UCUR"), opt(vcur, (r0(vcur),), "VCUR"),
                None if iodp is None else self._int(iodp, (iodp.shape[0],), "IODP"), opt(ibrmem, (r0(ibrmem),), "IBRMEM"),
                None if pa is None else pa.data_ptr(), None if pn is None else pn.data_ptr()]
        self._chk(self.lib.ecwam_hip_outblock(self._h, kijs, kijl, *args, float(self.t.CITHRSH if cithrsh is None else cithrsh), float(zmiss),
                                              self._real(bout, (bout.shape[0], ncol), "BOUT"), _stream_ptr()))

    def outwnorm(self, field, column: int, n: int, zmiss: float = -999.0):
        """(average, minimum, maximum, count) of field[:n, column] over the values != zmiss."""
        if not (field.is_cuda and field.dtype == self.dtype and field.is_contiguous() and field.dim() == 2 and n <= field.shape[0]):
            raise ValueError("OUTWNORM: expected a contiguous 2-D cuda tensor in the working precision")
        import ctypes as C
        res = (C.c_double * 4)()
        ptr = field.data_ptr() + column * field.element_size()
        self._chk(self.lib.ecwam_hip_outwnorm(self._h, ptr, field.shape[1], n, float(zmiss), res, _stream_ptr()))
        return tuple(res)

    # -- NEWWIND (newwind.F90:126-161)
    def newwind(self, ff, ff_next, icode_wnd: int | None = None):
        """icode_wnd: ICODE_CPL of a coupled run (newwind.F90:120-124); default ICODE of the parameters."""
        n = ff.shape[0]
        a = (self._h, n, self._real(ff, (n, NFF), "FF"), self._real(ff_next, (n, NFF), "FF_NEXT"))
        if icode_wnd is None:
            self._chk(self.lib.ecwam_hip_newwind(*a, _stream_ptr()))
        else:
            self._chk(self.lib.ecwam_hip_newwind_icode(*a, int(icode_wnd), _stream_ptr()))

    def nosource(self, kijs, kijl, fl1, mij, xllws):
        """LLSOURCE = F (wamintgr.F90:152-160): FL1 = MAX(FL1, EPSMIN), MIJ = NFRE, XLLWS = 0 on rows [kijs, kijl).
        fl1 = None: a call before the next source-term date (wamintgr.F90:178-186): MIJ and XLLWS only."""
        nrow = xllws.shape[0] if fl1 is None else fl1.shape[0]
        if not (0 <= kijs <= kijl <= min(nrow, mij.shape[0], xllws.shape[0])):
            raise ValueError("NOSOURCE: KIJS/KIJL outside the operands")
        self._chk(self.lib.ecwam_hip_nosource(self._h, kijs, kijl, None if fl1 is None else self._real(fl1, (nrow, self.NANG, self.NFRE), "FL1"),
                                              self._int(mij, (mij.shape[0],), "MIJ"),
                                              self._real(xllws, (xllws.shape[0], self.NANG, self.NFRE), "XLLWS"), _stream_ptr()))

    # -- layout conversion (propag_wam.F90:124-137, 373-400)
    def chunks_to_points(self, chunked, points, nproma, nchnk, npts, n2, n3):
        pc = self._real(chunked, (nchnk, n3, n2, nproma), "chunked")
        pp = self._real(points, (points.shape[0], n2, n3), "points")
        if points.shape[0] < npts:
            raise ValueError("points buffer too small")
        self._chk(self.lib.ecwam_hip_chunks_to_points(self._h, pc, pp, nproma, nchnk, npts, n2, n3, _stream_ptr()))

    def points_to_chunks(self, points, chunked, nproma, nchnk, npts, n2, n3):
        pc = self._real(chunked, (nchnk, n3, n2, nproma), "chunked")
        pp = self._real(points, (points.shape[0], n2, n3), "points")
        if points.shape[0] < npts:
            raise ValueError("points buffer too small")
        self._chk(self.lib.ecwam_hip_points_to_chunks(self._h, pp, pc, nproma, nchnk, npts, n2, n3, _stream_ptr()))

    # -- halo pack / unpack (mpexchng.F90:124-138, 217-231)
    def pack_rows(self, fl, idx, buf):
        n = idx.shape[0]
        if n == 0:
            return
        self._chk(self.lib.ecwam_hip_pack_rows(self._h, self._real(fl, (fl.shape[0], self.NANG, self.NFRE), "FL"),
                                               self._int(idx, (n,), "IDX"), n, self._real(buf, (n, self.NANG, self.NFRE), "BUF"),
                                               _stream_ptr()))

    def unpack_rows(self, buf, fl, dst0):
        n = buf.shape[0]
        if n == 0:
            return
        if dst0 < 0 or dst0 + n > fl.shape[0]:
            raise ValueError("unpack_rows: destination range outside FL")
        self._chk(self.lib.ecwam_hip_unpack_rows(self._h, self._real(buf, (n, self.NANG, self.NFRE), "BUF"), n,
                                                 self._real(fl, (fl.shape[0], self.NANG, self.NFRE), "FL"), dst0, _stream_ptr()))


    # -- MPEXCHNG inside the library (include/ecwam_hip.h: ecwam_hip_halo_*)
    def halo_setup(self, dom) -> None:
        """dom: decomp.LocalDomain.  Peers in ascending rank order; send lists concatenated in that order."""
        peers = sorted(set(dom.send) | set(dom.recv))
        self._halo_peers = peers
        pa = np.asarray(peers, dtype=np.int32)
        sc = np.asarray([len(dom.send.get(p, ())) for p in peers], dtype=np.int32)
        si = np.concatenate([np.asarray(dom.send[p], dtype=np.int32) for p in peers if p in dom.send]) if sc.sum() else np.zeros(0, np.int32)
        rd = np.asarray([dom.recv.get(p, (0, 0))[0] for p in peers], dtype=np.int32)
        rc = np.asarray([dom.recv.get(p, (0, 0))[1] for p in peers], dtype=np.int32)
        self._halo_send_cnt, self._halo_recv_cnt = sc, rc
        ptr = lambda a: a.ctypes.data if a.size else None
        self._chk(self.lib.ecwam_hip_halo_setup(self._h, dom.rank, dom.nranks, len(peers), ptr(pa), ptr(sc), ptr(si), ptr(rd), ptr(rc)))

    def comm_unique_id(self) -> bytes:
        import ctypes
        buf = ctypes.create_string_buffer(128)
        self._chk(self.lib.ecwam_hip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes) -> None:
        if len(uid) != 128:
            raise ValueError("RCCL unique id: 128 bytes")
        self._chk(self.lib.ecwam_hip_comm_init(self._h, uid))

    def comm_count(self) -> int:
        """Ranks of the library's RCCL communicator as RCCL reports them (0: none)."""
        k = C.c_int(0)
        self._chk(self.lib.ecwam_hip_comm_count(self._h, C.byref(k)))
        return int(k.value)

    def _rows(self, fl):
        if not (fl.is_cuda and fl.is_contiguous() and fl.dtype == self.dtype and fl.dim() == 3):
            raise ValueError("halo: expected a contiguous device tensor [rows][NANG][M] of the context's precision")
        return int(fl.shape[1] * fl.shape[2])

    def halo_start(self, fl) -> None:
        self._chk(self.lib.ecwam_hip_halo_start(self._h, fl.data_ptr(), self._rows(fl), _stream_ptr()))

    def halo_finish(self) -> None:
        self._chk(self.lib.ecwam_hip_halo_finish(self._h, _stream_ptr()))

    # -- PROENVHALO on the device (proenvhalo.F90:63-107)
    def proenvhalo_pack(self, n, wvprpt, omosnh2kd, depth, ucur, vcur, buffer_ext) -> None:
        self._chk(self.lib.ecwam_hip_proenvhalo_pack(self._h, int(n), wvprpt.data_ptr(), omosnh2kd.data_ptr(), depth.data_ptr(), ucur.data_ptr(),
                                                     vcur.data_ptr(), buffer_ext.data_ptr(), _stream_ptr()))

    def proenvhalo_unpack(self, nrows, buffer_ext, land, wavnum_ext, cgroup_ext, omosnh2kd_ext, depth_ext, u_ext, v_ext) -> None:
        self._chk(self.lib.ecwam_hip_proenvhalo_unpack(self._h, int(nrows), buffer_ext.data_ptr(), land.data_ptr(), wavnum_ext.data_ptr(),
                                                       cgroup_ext.data_ptr(), omosnh2kd_ext.data_ptr(), depth_ext.data_ptr(), u_ext.data_ptr(),
                                                       v_ext.data_ptr(), _stream_ptr()))

    def halo_pack_host(self, fl, host_send) -> None:
        self._chk(self.lib.ecwam_hip_halo_pack_host(self._h, fl.data_ptr(), self._rows(fl), host_send.data_ptr(), _stream_ptr()))

    def halo_unpack_host(self, fl, host_recv) -> None:
        self._chk(self.lib.ecwam_hip_halo_unpack_host(self._h, fl.data_ptr(), self._rows(fl), host_recv.data_ptr(), _stream_ptr()))


def propags_grid(grid_dev: dict, grid, circ) -> dict:
    """grid_dev with "dellam1_ext" added: 1 / DELLAM(KXLT) per row and 0 in the land slot, DELLAM = ZDELLO CIRC / 360 formed in the working precision
    (readmdlconf.F90:145, mpdecomp.F90:1428), what HipContext.propags reads beside the tables of grid_to_device.  Whole-grid tables only."""
    ref = grid_dev["cosphm1_ext"]
    T = np.float32 if ref.dtype == torch.float32 else np.float64
    dellam = np.asarray(grid.zdello, T) * T(circ) / T(360.0)
    d = np.zeros(ref.shape[0], T)
    d[:grid.nsea] = T(1) / dellam[grid.kxlt]
    return dict(grid_dev, dellam1_ext=torch.from_numpy(d).to(ref.device))


def rotated_to_device(tables: dict, dtype, device) -> dict:
    """The tables of grid.rotated_tables as the device tensors HipContext.set_rotated takes."""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    out = {k: torch.from_numpy(np.ascontiguousarray(tables[k], dtype=np.int32)).to(device) for k in ("krlat", "krlon")}
    out.update({k: torch.from_numpy(np.ascontiguousarray(tables[k], dtype=npdt)).to(device) for k in ("wrlat", "wrlon", "cdr", "sdr", "prqrt")})
    out["sqrt2"] = float(npdt(tables["sqrt2"]))
    return out


def grid_to_device(grid, dtype, device, lo: int = 0, hi: int | None = None, local=None) -> dict:
    """Upload the grid tables of points [lo,hi) (or a decomp.LocalDomain) as the dict `HipContext.ctuw` expects."""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    if local is not None:
        klon, klat, kcor, kxlt = local.klon, local.klat, local.kcor, local.kxlt
        wlat, wcor = grid.wlat[local.lo:local.hi], grid.wcor[local.lo:local.hi]
        n, nland, cosphm1 = local.n, local.nland, local.cosphm1_ext
    else:
        hi = grid.nsea if hi is None else hi
        assert lo == 0 and hi == grid.nsea
        klon, klat, kcor, kxlt = grid.klon, grid.klat, grid.kcor, grid.kxlt
        wlat, wcor, n, nland, cosphm1 = grid.wlat, grid.wcor, grid.nsea, grid.nland, grid.cosphm1_ext

    def ti(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)

    def tr(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=npdt)).to(device)

    return dict(n=n, nland=nland, ngy=grid.ngy, xdella=grid.xdella, kxlt=ti(kxlt), zdello=tr(grid.zdello), cosph=tr(grid.cosph),
                sinph=tr(grid.sinph), klon=ti(klon), klat=ti(klat), kcor=ti(kcor), wlat=tr(wlat), wcor=tr(wcor),
                cosphm1_ext=tr(cosphm1))
