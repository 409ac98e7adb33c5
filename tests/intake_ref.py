"""FLDINTER, the LLINIALL branch of INIT_FIELDG, the point-wise branches of RECVNEMOFIELDS, UPDNEMOFIELDS and UPDNEMOSTRESS restated in numpy from
the reference's Fortran (fldinter.F90:176-374, init_fieldg.F90:92-116, recvnemofields.F90:101-110 and 176-250, updnemofields.F90:92-98,
updnemostress.F90:84-132), in the reference's order of operations and in the precision asked for: TEST INFRASTRUCTURE.  INITIALINT and the
per-point table are those of ecwam_amd/intake.py, which the host hands to the library.  All of it is written from the Fortran, not from the
kernels of csrc/intake.hip; tests/test_intake_host.py holds it against the reference's own results (tests/golden/intake_0.npz, recorded by
tools/make_golden_intake.py) and tests/test_gpu_intake.py takes the inputs and the gates from it.

make_cases() builds the inputs of the fixtures; the tool and the tests share it.  The gates of the tests are read from
tests/golden/intake_observed.json, which the tool writes from the reference's results and this restatement alone.
"""
from __future__ import annotations

import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ecwam_amd import intake  # noqa: E402
from ecwam_amd.tables import Config, Tables  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
NROW, KIJS, KIJL, SPLIT = 67, 3, 67, 30      # the calls act on rows [3, 67), in two launches split at 30; rows 0..2 are guard rows
NX, NY = 11, 9                               # the reduced wave grid: NGX, NGY; FIELDG is (1:NX, 1:NY)
NCELL = NX * NY
KLONRGG = np.array([11, 10, 9, 11, 8, 11, 10, 7, 11], np.int32)      # by latitude, south to north
FG = {n: i for i, n in enumerate("UWND VWND AIRD WSTAR CICOVER CITHICK USTRA VSTRA WSWAVE WDWAVE LKFR UCUR VCUR".split())}
FF_CICOVER, FF_CITHICK, INTF_IBRMEM = 2, 13, 15
PMISS = -999.0
SENT = -777.25
CURRENT_MAX = 1.5
LADEN, LGUST, LLKC, LWCUR, NEWCURR = 1, 2, 4, 8, 16
LREST, LINIT, LWCOU, CIC, CIT, CUR, IBR = 1, 2, 4, 8, 16, 32, 64
# the switches of the recorded FLDINTER calls: each of LADEN, LGUST, LLKC on and off; NEWCURR with LWCUR, without it, and no NEWCURR
FLAGSETS = {"none": 0, "all": LADEN | LGUST | LLKC | LWCUR | NEWCURR, "laden_zerocur": LADEN | NEWCURR, "gust_lake_oldcur": LGUST | LLKC | LWCUR}
CASES = ("A", "B", "C")
RECV = {"rest": LREST | IBR, "rest_noibr": LREST,
        "init_cou_all": LINIT | LWCOU | CIC | CIT | CUR | IBR, "init_cou_cic": LINIT | LWCOU | CIC, "init_cou_cit": LINIT | LWCOU | CIT,
        "init_cou_cur": LINIT | LWCOU | CUR, "init_cou_ibr": LINIT | LWCOU | IBR,
        "init_all": LINIT | CIC | CIT | CUR | IBR, "init_cic": LINIT | CIC, "init_cit": LINIT | CIT, "init_cur": LINIT | CUR, "init_ibr": LINIT | IBR,
        "rest_init_cou": LREST | LINIT | LWCOU | CIC | CIT | CUR | IBR}
NEMONTAU = (0, 1, 7)
W2N = "NEMOUSTOKES NEMOVSTOKES NEMOSTRN NPHIEPS NTAUOC NSWH NMWP NEMOTAUX NEMOTAUY NEMOTAUICX NEMOTAUICY NEMOWSWAVE NEMOPHIF".split()
UPD_FIELDS = [W2N.index(k) for k in "NSWH NMWP NPHIEPS NTAUOC NEMOSTRN NEMOUSTOKES NEMOVSTOKES".split()]
UPD_STRESS = [W2N.index(k) for k in "NEMOTAUX NEMOTAUY NEMOWSWAVE NEMOPHIF NEMOTAUICX NEMOTAUICY".split()]
ICE_BRANCHES = ("none", "near00", "near10", "near01", "near11", "mean3", "mean2", "mean1", "all4")


def dtype_of(prec):
    return np.float32 if prec == "sp" else np.float64


@functools.lru_cache(maxsize=None)
def tables(prec) -> Tables:
    return Tables(Config(nang=12, nfre=36, nfre_red=36), dtype_of(prec))


def _f32(x):
    return np.asarray(np.asarray(x, np.float32), np.float64)


def written_planes(flags):
    """the planes of fieldg a FLDINTER call writes"""
    names = ["UWND", "VWND", "AIRD", "WSTAR", "CICOVER", "CITHICK", "USTRA", "VSTRA", "LKFR"] + (["UCUR", "VCUR"] if flags & NEWCURR else [])
    return sorted(FG[n] for n in names)


def flag_kw(flags):
    return dict(laden=bool(flags & LADEN), lgust=bool(flags & LGUST), llkc=bool(flags & LLKC), lwcur=bool(flags & LWCUR), newcurr=bool(flags & NEWCURR))


# ---- the inputs of the fixtures ---------------------------------------------------------------------------------------------------------------
def _atmosphere(rng, name):
    """One atmosphere grid: the arguments of INITIALINT and FLDINTER that describe it, IJBLOCK(0:NC+1,NR) and the ten fields."""
    if name == "A":      # periodic and reduced: 7 rows of 8 to 16 points
        g = dict(iperiodic=1, ilonrgg=np.array([8, 12, 16, 16, 14, 10, 9], np.int32), rmonop=75.0, rmosop=-75.0, rmowep=0.0, rmoeap=337.5, interpol=1)
    elif name == "B":    # regional, regular, not periodic, and smaller than the wave grid: the clamps of INITIALINT and FLDINTER work
        g = dict(iperiodic=0, ilonrgg=np.full(6, 9, np.int32), rmonop=35.0, rmosop=-40.0, rmowep=30.0, rmoeap=150.0, interpol=1)
    else:                # LLINTERPOL = F: the fields are on the wave grid itself
        g = dict(iperiodic=1, ilonrgg=KLONRGG.copy(), rmonop=0.0, rmosop=0.0, rmowep=0.0, rmoeap=0.0, interpol=0)
    ilon = g["ilonrgg"]
    nr, nc = ilon.size, int(ilon.max())
    g.update(nr=nr, nc=nc, ngptotg=int(ilon.sum()))
    # IJBLOCK: a permutation of the field order; row JJ (north to south) has ILONRGG(NR - JJ + 1) points.  A periodic grid's wrap columns repeat
    # the row's last and first point (column 0 and column ILONRGG + 1); what lies beyond is never read and holds 1
    perm = rng.permutation(g["ngptotg"]) + 1
    ijb = np.ones((nc + 2, nr), np.int32)
    at = 0
    for jj in range(1, nr + 1):
        n = int(ilon[nr - jj])
        ijb[1:n + 1, jj - 1] = perm[at:at + n]
        at += n
        if g["iperiodic"]:
            ijb[0, jj - 1] = ijb[n, jj - 1]
            ijb[n + 1, jj - 1] = ijb[1, jj - 1]
    g["ijblock"] = ijb
    f = _f32(rng.uniform(-12.0, 12.0, (10, g["ngptotg"])))
    f[2] = _f32(rng.uniform(0.9, 1.35, g["ngptotg"]))
    f[3] = _f32(rng.uniform(0.0, 2.0, g["ngptotg"]))
    ci = _f32(rng.uniform(0.0, 1.0, g["ngptotg"]))
    ci[rng.uniform(size=g["ngptotg"]) < 0.45] = PMISS      # land points of the atmosphere
    f[4] = ci
    f[5] = _f32(np.where(rng.uniform(size=g["ngptotg"]) < 0.5, 0.0, rng.uniform(0.0, 1.0, g["ngptotg"])))
    f[6:8] = _f32(rng.uniform(-0.5, 0.5, (2, g["ngptotg"])))
    f[8:10] = _f32(rng.uniform(-2.0, 2.0, (2, g["ngptotg"])))
    g["fields"] = f
    return g


def make_cases(seed=20261020):
    """The inputs of every recorded call, in float64 and float32-representable unless noted (both precisions see the same numbers).
    The wave grid: 11 x 9, reduced (KLONRGG), spacings chosen so that no point lies on a meridian or parallel of an atmosphere grid; 67 rows on
    distinct cells with I <= KLONRGG, point i = row 3 + i.  A, B, C: the atmosphere grids (_atmosphere).  The NEMO blocks, the WAVE2OCEAN rows
    and NEMOIBR are float64 numbers that no float32 holds: their products and clips round once, on the store."""
    rng = np.random.default_rng(seed)
    c = dict(xdella=17.5, amosop=-70.25, amowep=1.25, zdello=_f32(360.0 / KLONRGG))
    c["amonop"] = c["amosop"] + (NY - 1) * c["xdella"]
    c["amoeap"] = float(_f32(c["amowep"] + 360.0 - 360.0 / NX))
    valid = np.array([(j - 1) * NX + (i - 1) for j in range(1, NY + 1) for i in range(1, int(KLONRGG[NY - j]) + 1)])
    cells = valid[rng.permutation(valid.size)[:NROW]]
    c["map_in"] = cells.astype(np.int32)
    c["ifromij"], c["jfromij"] = (cells % NX + 1).astype(np.int32), (cells // NX + 1).astype(np.int32)
    for name in CASES:
        c[name] = _atmosphere(rng, name)
    n = KIJL - KIJS
    i = np.arange(n)

    def col(vals):      # guard rows first
        return np.concatenate((rng.uniform(0.5, 2.0, KIJS), vals))
    fg = _f32(rng.uniform(0.5, 2.0, (len(FG), NCELL)))
    fg[FG["LKFR"], cells] = _f32(col(np.array([0.0, 0.3, 0.0, -0.5])[i % 4]))
    fg[FG["CICOVER"], cells] = _f32(col(np.array([0.0, 0.4, 0.97])[i % 3]))
    c["fieldg"] = fg
    c["nemo"] = np.stack([col(rng.uniform(0.0, 1.0, n)), col(rng.uniform(0.0, 3.0, n)), col(np.array([1.7, -0.2, 0.0, -2.25, 0.9])[i % 5] * (1 + 1e-9)),
                          col(np.array([-1.6, 0.0, 0.5])[i % 3] * (1 - 1e-9))])
    c["nemoibr"] = col(rng.uniform(0.0, 1.0, n))
    c["ff"] = _f32(rng.uniform(0.5, 2.0, (NROW, 16)))
    c["intf"] = _f32(rng.uniform(-1.0, 1.0, (NROW, 16)))
    c["ucur"], c["vcur"] = _f32(col(rng.uniform(-1.0, 1.0, n))), _f32(col(rng.uniform(-1.0, 1.0, n)))
    c["wam2nemo"] = rng.uniform(-3.0, 3.0, (NROW, 13))
    c["roair"], c["wstar0"] = float(_f32(1.225)), 0.0625
    return c


@functools.lru_cache(maxsize=None)
def cached_cases():
    """make_cases(), built once per process and shared: never modified by its users"""
    return make_cases()


def initialint_args(c, name):
    """the arguments of INITIALINT for atmosphere grid `name`, in its order (iu06 first; no dtype)"""
    g = c[name]
    return (6, g["nc"], g["nr"], NX, NY, 1, KLONRGG, c["xdella"], c["zdello"], c["amowep"], c["amosop"], c["amoeap"], c["amonop"], g["nc"], g["nr"], g["rmonop"],
            g["rmosop"], g["rmowep"], g["rmoeap"], g["ilonrgg"], g["iperiodic"], NX, NY)


def own_tables(c, name, prec):
    """intake.initialint's six tables in the precision asked for"""
    return intake.initialint(*initialint_args(c, name), dtype=dtype_of(prec))


def point_table(c, name, tabs=None):
    """(idx [67][4], w [67][3]) of atmosphere grid `name` from the six tables given (DJ1, DII1, DIIP1, JJ, II, IIP); case C needs none"""
    g = c[name]
    if not g["interpol"]:
        return intake.point_table(c["ifromij"], c["jfromij"], g["ijblock"], g["ilonrgg"], g["nr"], g["iperiodic"], None, None, None, None, None, None, False)
    dj1, dii1, diip1, jj, ii, iip = tabs
    return intake.point_table(c["ifromij"], c["jfromij"], g["ijblock"], g["ilonrgg"], g["nr"], g["iperiodic"], jj, ii, iip, dj1, dii1, diip1, True)


# ---- the routines ---------------------------------------------------------------------------------------------------------------------------------
def fldinter(prec, idx, w, fields, flags, roair, wstar0, pmiss=PMISS):
    """fldinter.F90:176-374 on the per-point table: (planes [13][n] with SENT where the routine writes nothing, the source positions read, the
    decisions: DJ1 <= 0.5, the longitude weight <= 0.5, the four == PMISS, the nearest == PMISS, and the branch of the sea-ice rule per point)."""
    T = dtype_of(prec)
    f = np.asarray(fields, T)
    n = idx.shape[0]
    out = np.full((len(FG), n), T(SENT), T)
    one, zero = T(1), T(0)
    roair, wstar0, pm = T(roair), T(wstar0), T(pmiss)
    cur = bool(flags & NEWCURR)
    if w is None:
        p = idx[:, 0]
        zl, zg, zk = (T(bool(flags & b)) for b in (LADEN, LGUST, LLKC))
        out[FG["UWND"]], out[FG["VWND"]] = f[0, p], f[1, p]
        out[FG["AIRD"]] = zl * f[2, p] + (one - zl) * roair
        out[FG["WSTAR"]] = zg * f[3, p] + (one - zg) * wstar0
        out[FG["CICOVER"]] = f[4, p]
        out[FG["LKFR"]] = zk * f[5, p]
        out[FG["USTRA"]], out[FG["VSTRA"]] = f[6, p], f[7, p]
        out[FG["CITHICK"]] = zero
        if cur:
            out[FG["UCUR"]] = f[8, p] if flags & LWCUR else zero
            out[FG["VCUR"]] = f[9, p] if flags & LWCUR else zero
        return out, np.unique(p), [], None
    w = np.asarray(w)
    assert np.array_equal(w.astype(T).astype(np.float64), w), "the weights are values of the working precision"
    dj1, dii1, diip1 = (w[:, k].astype(T) for k in range(3))
    dj2, dii2, diip2 = one - dj1, one - dii1, one - diip1

    def bil(k):
        f00, f10, f01, f11 = (f[k, idx[:, q]] for q in range(4))
        return (dj2 * (dii2 * f00 + dii1 * f10).astype(T)).astype(T) + (dj1 * (diip2 * f01 + diip1 * f11).astype(T)).astype(T)
    out[FG["UWND"]], out[FG["VWND"]] = bil(0), bil(1)
    out[FG["AIRD"]] = bil(2) if flags & LADEN else roair
    out[FG["WSTAR"]] = bil(3) if flags & LGUST else wstar0
    c4 = [f[4, idx[:, q]] for q in range(4)]
    miss = [x == pm for x in c4]
    some = miss[0] | miss[1] | miss[2] | miss[3]
    top = dj1 <= T(0.5)
    first = np.where(top, dii1 <= T(0.5), diip1 <= T(0.5))
    near = np.where(top, np.where(first, c4[0], c4[1]), np.where(first, c4[2], c4[3])).astype(T)
    total, count = np.zeros(n, T), np.zeros(n, np.int64)
    for x, m in zip(c4, miss):
        total = np.where(m, total, total + x).astype(T)
        count += ~m
    with np.errstate(all="ignore"):
        mean = np.where(count > 0, total / np.maximum(count, 1).astype(T), pm).astype(T)
    out[FG["CICOVER"]] = np.where(some, np.where(near == pm, mean, near), bil(4)).astype(T)
    out[FG["CITHICK"]] = zero
    out[FG["LKFR"]] = bil(5) if flags & LLKC else zero
    out[FG["USTRA"]], out[FG["VSTRA"]] = bil(6), bil(7)
    if cur:
        out[FG["UCUR"]] = bil(8) if flags & LWCUR else zero
        out[FG["VCUR"]] = bil(9) if flags & LWCUR else zero
    which = np.where(top, np.where(first, 0, 1), np.where(first, 2, 3))
    branch = np.where(~some, "none", np.where(near != pm, np.char.add("near", np.array(["00", "10", "01", "11"])[which]),
                                              np.where(count > 0, np.char.add("mean", count.astype(str)), "all4")))
    assert out.dtype == T
    return out, np.unique(idx), [top, first, *miss, near == pm], branch


def init_fieldg(prec, ncell, roair, wstar0):
    """init_fieldg.F90:92-116 for the thirteen planes"""
    T = dtype_of(prec)
    out = np.zeros((len(FG), ncell), T)
    out[FG["WSWAVE"]] = tables(prec).WSPMIN
    out[FG["AIRD"]], out[FG["WSTAR"]] = T(roair), T(wstar0)
    return out


def _clip(x):
    return np.copysign(np.minimum(np.abs(x), CURRENT_MAX), x)


def recvnemofields(prec, flags, lkfr, cicover_g, nemo, nemoibr, cicover, cithick, ucur, vcur, ibrmem):
    """recvnemofields.F90:101-110 and 176-250 on n points: (nemo [4][n], nemoibr [n]) float64 and (CICOVER, CITHICK, UCUR, VCUR, IBRMEM) in the
    working precision, afterwards.  lkfr, cicover_g: the planes of FIELDG gathered at the points."""
    T = dtype_of(prec)
    nemo, nemoibr = np.array(nemo, np.float64), np.array(nemoibr, np.float64)
    ci, ct, u, v, ib = (np.array(a, T) for a in (cicover, cithick, ucur, vcur, ibrmem))
    if flags & LREST:
        nemo = np.stack([ci, ct, u, v]).astype(np.float64)
        if flags & IBR:
            nemoibr = ib.astype(np.float64)
    if flags & LINIT:
        if flags & LWCOU:
            ocean = np.asarray(lkfr, T) <= T(0)
            if flags & CIC:
                ci = np.where(ocean, nemo[0].astype(T), np.asarray(cicover_g, T)).astype(T)
            if flags & CIT:
                ct = np.where(ocean, (nemo[0] * nemo[1]).astype(T), ct).astype(T)
                ci = np.where(ocean, ci, (0.5 * nemo[0]).astype(T)).astype(T)      # line 201 as the reference has it
            if flags & CUR:
                u = np.where(ocean, _clip(nemo[2]).astype(T), T(0)).astype(T)
                v = np.where(ocean, _clip(nemo[3]).astype(T), T(0)).astype(T)
        else:
            if flags & CIC:
                ci = nemo[0].astype(T)
            if flags & CIT:
                ct = (nemo[0] * nemo[1]).astype(T)
            if flags & CUR:
                u, v = nemo[2].astype(T), nemo[3].astype(T)
        if flags & IBR:
            ib = nemoibr.astype(T)
    return np.concatenate([nemo, nemoibr[None]]), np.stack([ci, ct, u, v, ib])


def updnemo(prec, wam2nemo, nemontau):
    """updnemofields.F90:92-98 and updnemostress.F90:84-132: (fields7 [7][n], stress6 [6][n], wam2nemo afterwards)"""
    T = dtype_of(prec)
    w = np.array(wam2nemo, np.float64)
    f7 = w[:, UPD_FIELDS].T.copy()
    if nemontau > 0:
        m1 = np.float64(T(1.0) / T(nemontau))
        s6 = (w[:, UPD_STRESS] * m1).T.copy()
    else:
        s6 = np.zeros((6, w.shape[0]))
    w[:, UPD_STRESS] = 0.0
    return f7, s6, w


def recv_inputs(c, A=slice(KIJS, KIJL)):
    cells = c["map_in"][A]
    return dict(lkfr=c["fieldg"][FG["LKFR"], cells], cicover_g=c["fieldg"][FG["CICOVER"], cells], nemo=c["nemo"][:, A], nemoibr=c["nemoibr"][A],
                cicover=c["ff"][A, FF_CICOVER], cithick=c["ff"][A, FF_CITHICK], ucur=c["ucur"][A], vcur=c["vcur"][A], ibrmem=c["intf"][A, INTF_IBRMEM])


# ---- the fixtures and the gates ---------------------------------------------------------------------------------------------------------------------
def load_golden():
    with np.load(os.path.join(GOLDEN, "intake_0.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_tables(g, name, prec):
    """the reference's six tables of atmosphere grid `name` from the fixture"""
    return tuple(g[f"tab_{name}_{prec}_{k}"] for k in ("dj1", "dii1", "diip1", "jj", "ii", "iip"))


def observed():
    with open(os.path.join(GOLDEN, "intake_observed.json")) as fh:
        return json.load(fh)


def plane_error(got, ref):
    """One plane over the points: the largest |got - ref| / max(|ref|, the plane's largest |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    top = np.abs(ref).max() if ref.size else 0.0
    if top == 0:
        return 0.0 if (d == 0).all() else float("inf")
    return float((d / np.maximum(np.abs(ref), top)).max())


def gate(kind, name, prec, obs=None):
    """The convention of tests/forcing_ref.py::gate.  Double precision: 10 x the largest difference between the restated chain (intake.initialint,
    intake.point_table, fldinter above) and the reference's double precision results, 8 eps where that is exactly 0.  Single precision: 3 x the
    largest difference between the reference's own single and double precision results, 8 eps (single) where that is 0.  kind: "fldinter" (name:
    a plane of fieldg) or "weights" (name: DJ1, DII1, DIIP1)."""
    obs = obs or observed()
    if prec == "dp":
        v = obs["restatement_vs_reference_dp"][kind][name]
        return 10 * v if v > 0 else 8 * float(np.finfo(np.float64).eps)
    v = obs["reference_sp_vs_dp"][kind][name]
    return 3 * v if v > 0 else 8 * float(np.finfo(np.float32).eps)
