"""OUTSPEC's sea-ice mask, the block-to-grid step of OUTWSPEC / MAKEGRID and WGRIBENCODE_VALUES restated in numpy from the reference's Fortran
(outspec.F90:96-118, outwspec.F90:124, 219-227, makegrid.F90:105-109, 156-160, wgribencode_values.F90:93-197), in the reference's order of
operations and in the precision asked for: TEST INFRASTRUCTURE.  It is written from the Fortran, through the two-dimensional FIELD as the
reference goes, not from the kernels of csrc/gribout.hip and not through the map of ecwam_amd/gribout.py, which it therefore checks as well.
tests/test_gribout_host.py holds it against the reference's own results (tests/golden/gribout_0.npz, recorded by tools/make_golden_gribout.py)
and tests/test_gpu_gribout.py takes the inputs and the gates from it.

The cases (make_cases), shared by the tool and the tests; every input is float32-representable:
  A  a reduced grid with both poles, 13 rows of 6 .. 40 .. 6 cells (292), about 70 % sea; the row beside the south pole is all land (the pole
     mean has no contributor), the one beside the north pole is mixed, and both pole rows hold sea points (which the padding overwrites); one
     point in ten lies under ice above CITHRSH.  NANG = 12, NFRE = 36, NFRE_RED = 25; JONSWAP spectra scaled per point over six decades, two
     fields with every value below PPEPS (PPMAX stays near ZMINSPEC; nothing of them is within DELTAPP of the threshold, so by the reference's
     arithmetic every cell, land included, keeps ZMINSPEC-like values instead of going missing), two fields that keep every sea value.
     Recorded with and without the ice mask, for the fields of the frequencies 1, 2, 13 and 25.
  B  a regular 8 x 5 grid, IRGG = 0, CLDOMAIN = 'g', AMONOP = 72, XDELLA = 18: the start offset ICOUNT, the ZMISS prefill, no pole.  Four fields.
  C  the path of the integrated parameters (no logarithm) on the grid of A: 7 columns of a BOUT, some entries ZMISS.
No value lies within MARGIN = 0.01 of its field's PPMIN on the log scale: the inputs are moved until that holds (make_cases), so that the
decision of the threshold never hides behind a tolerance.
"""
from __future__ import annotations

import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ecwam_amd import gribout, synthetic  # noqa: E402
from ecwam_amd.tables import Config, Tables  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
OPTS = dict(gribout.GRIB_DEFAULTS)
ZMISS = OPTS["zmiss"]
MARGIN = 0.01
NFF = 16
RECORDED_FREQ = (0, 1, 12, 24)           # frequencies 1, 2, 13 and 25, 0-based
B_FIELDS = (149, 4)                      # case B: fields [149, 153), directions 6 .. 9 of frequency 13
TINY_FIELDS = ((3, 0), (7, 12))          # (K, M), 0-based: every value below PPEPS
FULL_FIELDS = ((5, 1), (2, 24))          # every sea value kept


def config(nang=12, nfre_red=25) -> Config:
    return Config(nang=nang, nfre=36, nfre_red=nfre_red, licerun=True, lmaskice=True)      # LMASKICE: CITHRSH = 0.3


@functools.lru_cache(maxsize=None)
def tables(prec, nang=12, nfre_red=25) -> Tables:
    return Tables(config(nang, nfre_red), np.float32 if prec == "sp" else np.float64)


def recorded_fields(nang=12):
    return [m * nang + k for m in RECORDED_FREQ for k in range(nang)]


# ---- the grids: the reference's variables (IXLG, KXLT 1-based; NLONRGG south to north)
def grid_a(seed=20260101):
    nlon = np.array([6, 12, 18, 24, 30, 36, 40, 36, 30, 24, 18, 12, 6])
    rng = np.random.default_rng(seed)
    ix, ky = [], []
    for row, n in enumerate(nlon):      # sea points south to north, west to east
        sea = rng.uniform(size=n) < 0.72
        if row == 1:
            sea[:] = False              # beside the south pole: all land
        if row == 11:
            sea[:] = np.arange(n) % 3 != 1      # beside the north pole: mixed
        if row in (0, 12):
            sea[:] = np.arange(n) % 2 == 0      # the pole rows hold sea points
        ix += list(np.flatnonzero(sea) + 1)
        ky += [row + 1] * int(sea.sum())
    return dict(nlonrgg=nlon, ngy=13, ngx=40, irgg=1, amonop=90.0, amosop=-90.0, xdella=15.0, cldomain="g", lpadpoles=True,
                ixlg=np.array(ix), kxlt=np.array(ky))


def grid_b(seed=20260102):
    rng = np.random.default_rng(seed)
    sea = rng.uniform(size=(5, 8)) < 0.75
    ky, ix = np.nonzero(sea)
    return dict(nlonrgg=np.full(5, 8), ngy=5, ngx=8, irgg=0, amonop=72.0, amosop=0.0, xdella=18.0, cldomain="g", lpadpoles=True, ixlg=ix + 1, kxlt=ky + 1)


def value_map(g):
    return gribout.value_map(g["nlonrgg"], g["ixlg"], g["kxlt"], g["ngy"], g["irgg"], g["amonop"], g["amosop"], g["xdella"], g["cldomain"], g["lpadpoles"])


def _nint(x):
    return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


# ---- the restatement
def ice_mask(fl, cicover, t):
    """outspec.F90:100-116 on fl [npts][...] in the precision of the tables"""
    T = t.dtype
    zm = np.where(np.asarray(cicover, T) > t.CITHRSH, T(1), T(0)).astype(T).reshape((-1,) + (1,) * (fl.ndim - 1))
    return ((T(1) - zm) * fl.astype(T) + zm * T(t.FLMIN)).astype(T)


def fields_of(fl, fields, nang):
    """block [nfld][npts] of FL1 [npts][NANG][NFRE]: field f = M NANG + K"""
    f = np.asarray(fields)
    return np.ascontiguousarray(fl[:, f % nang, f // nang].T)


def encode(block, g, T, spectral, rows=None, o=OPTS):
    """block [nfld][npts] in T -> (VALUES [nfld][NTENCODE], PPMAX [nfld] or None) as outwspec.F90:124, 219-227 and WGRIBENCODE_VALUES give them.
    rows = (kijs, kijl): only those rows are scattered (the others count as absent)."""
    T = np.dtype(T).type
    block = np.asarray(block, T)
    nfld, npts = block.shape
    ngx, ngy, nlon = g["ngx"], g["ngy"], g["nlonrgg"]
    zmiss = T(o["zmiss"])
    k0, k1 = rows or (0, npts)
    field = np.full((nfld, ngy, ngx), zmiss, T)      # FIELD(NGX,NGY) per field; J = 1 the northernmost row
    ix, iy = g["ixlg"][k0:k1] - 1, ngy - g["kxlt"][k0:k1]
    field[:, iy, ix] = block[:, k0:k1]
    if g["irgg"] == 1 or g["cldomain"] == "m":
        ntencode = int(nlon.sum()) if g["irgg"] == 1 else ngy * ngx
        icount = 0
    else:
        icount = _nint((T(90) - T(g["amonop"])) / T(g["xdella"])) * ngx
        ntencode = (_nint(180.0 / g["xdella"]) + 1 if g["cldomain"] == "g" else ngy) * ngx
    values = np.full((nfld, ntencode), zmiss, T)      # the regular branch sets ZMISS; the reduced one fills every cell
    if g["lpadpoles"]:
        for pole, j, jadj in ((T(90) - T(g["amonop"]), 0, 1), (T(-90) - T(g["amosop"]), ngy - 1, ngy - 2)):
            if _nint(pole / T(g["xdella"])) != 0:
                continue
            temp, nn = np.zeros(nfld, T), np.zeros(nfld, np.int64)
            for i in range(nlon[ngy - 1 - jadj]):      # in the reference's order
                v = field[:, jadj, i]
                ok = v != zmiss
                temp = np.where(ok, temp + v, temp).astype(T)
                nn += ok
            temp = np.where(nn > 0, temp / np.maximum(nn, 1).astype(T), zmiss).astype(T)
            field[:, j, :nlon[ngy - 1 - j]] = temp[:, None]
    for j in range(ngy):
        n = nlon[ngy - 1 - j]
        values[:, icount:icount + n] = field[:, j, :n]
        icount += n
    if not spectral:
        return values, None
    deltapp = T(2 ** o["ngrbress"] - 1) * T(o["ppresol"])
    absprec = abs(T(o["pprec"]))
    zminspec = T(np.log10(T(o["ppeps"])) + absprec)
    ok = values != zmiss
    with np.errstate(invalid="ignore", divide="ignore"):
        logged = (np.log10(np.where(ok, values, T(1)) + T(o["ppeps"])).astype(T) + absprec).astype(T)
    values = np.where(ok, logged, zminspec).astype(T)
    ppmax = np.maximum(values.max(axis=1), zminspec).astype(T)
    ppmin = np.minimum(np.minimum(T(o["ppmiss"]), (ppmax - deltapp).astype(T)), T(o["ppmin_reset"])).astype(T)
    values = np.where(values <= ppmin[:, None], zmiss, values).astype(T)
    return values, ppmax


def ppmin_of(ppmax, T, o=OPTS):
    T = np.dtype(T).type
    return np.minimum(np.minimum(T(o["ppmiss"]), (np.asarray(ppmax, T) - T(2 ** o["ngrbress"] - 1) * T(o["ppresol"])).astype(T)), T(o["ppmin_reset"]))


def log_before_threshold(block, g, T, o=OPTS):
    """the values of encode(spectral) before step 6, for the margin"""
    return encode(block, g, T, True, o=dict(o, ppmiss=-1e30, ppmin_reset=-1e30, ngrbress=30, ppresol=1e20))[0]


def written_cells(g, rows):
    """the cells a call on rows (kijs, kijl) writes: those of the rows, those no row fills, the padded pole rows"""
    ival, ntencode, poles = value_map(g)
    w = np.ones(ntencode, bool)
    w[ival] = False
    w[ival[rows[0]:rows[1]]] = True
    for p in (poles.north, poles.south):
        w[p.pole0:p.pole0 + p.npole] = True
    return w


# ---- the inputs
def spectra(g, nang, seed, t=None):
    """FL1 [npts][NANG][36] float32: JONSWAP shapes scaled per point over six decades, the tiny and the full fields set"""
    t = t or tables("dp", nang)
    npts = g["ixlg"].size
    rng = np.random.default_rng(seed)
    fl = synthetic.jonswap_spectra(t.FR, t.TH, rng.uniform(0.08, 0.35, npts), rng.uniform(0, 2 * np.pi, npts), np.float64)
    fl = np.maximum(fl * 10.0 ** rng.uniform(-5.0, 1.0, npts)[:, None, None], 1e-30)
    for k, m in TINY_FIELDS:
        fl[:, k, m] = rng.uniform(1e-12, 5e-11, npts)
    for k, m in FULL_FIELDS:
        fl[:, k, m] = rng.uniform(0.5, 2.0, npts)
    return fl.astype(np.float32)


def _settle(fl, cic, g, nang, nfre_red):
    """moves inputs until no value lies within 2 MARGIN of its field's PPMIN (double precision, both values of the ice flag)"""
    t = tables("dp", nang, nfre_red)
    ival, ntencode, poles = value_map(g)
    inv = np.full(ntencode, -1)
    inv[ival] = np.arange(ival.size)
    fields = np.arange(nang * nfre_red)
    for _ in range(60):
        moved = False
        for ice in (0, 1):
            f64 = fl.astype(np.float64)
            blk = fields_of(ice_mask(f64, cic, t) if ice else f64, fields, nang)
            lg = log_before_threshold(blk, g, np.float64)
            ppmin = ppmin_of(np.maximum(lg.max(axis=1), np.log10(OPTS["ppeps"])), np.float64)
            bad_f, bad_c = np.nonzero(np.abs(lg - ppmin[:, None]) < 2 * MARGIN)
            for f, c in zip(bad_f, bad_c):
                k, m = f % nang, f // nang
                rows = [inv[c]] if inv[c] >= 0 and not any(p.npole and p.pole0 <= c < p.pole0 + p.npole for p in (poles.north, poles.south)) else []
                for p in (poles.north, poles.south):
                    if p.npole and p.pole0 <= c < p.pole0 + p.npole:
                        rows = [r for r in inv[p.adj0:p.adj0 + p.nadj] if r >= 0]
                if not rows or (ice and any(cic[r] > t.CITHRSH for r in rows)):      # nothing of its own to move: move the field's maximum
                    rows = [int(np.argmax(blk[f]))]
                fl[rows, k, m] = (fl[rows, k, m].astype(np.float64) * 1.15).astype(np.float32)
                moved = True
        if not moved:
            return fl
    raise AssertionError("the inputs do not settle away from PPMIN")


def make_cases():
    ga, gb = grid_a(), grid_b()
    na, nb = ga["ixlg"].size, gb["ixlg"].size
    rng = np.random.default_rng(20260103)
    cic = np.where(np.arange(na) % 10 == 4, rng.uniform(0.4, 1.0, na), rng.uniform(0.0, 0.25, na)).astype(np.float32)
    fla = _settle(spectra(ga, 12, 20260104), cic, ga, 12, 25)
    cib = np.zeros(nb, np.float32)
    flb = _settle(spectra(gb, 12, 20260105), cib, gb, 12, 25)
    bout = rng.uniform(-5.0, 30.0, (na, 7)).astype(np.float32)
    bout[rng.uniform(size=(na, 7)) < 0.15] = ZMISS
    bout[ga["kxlt"] == 12, 2] = ZMISS      # one column has nothing beside the north pole either
    return dict(grid_a=ga, grid_b=gb, cic_a=cic, fl_a=fla, cic_b=cib, fl_b=flb, bout=bout)


@functools.lru_cache(maxsize=None)
def cached_cases():
    return make_cases()


def second_geometry():
    """NANG = 36, NFRE_RED = 29 on the grid of A: another tile geometry, held against the restatement only"""
    ga = grid_a()
    c = cached_cases()
    return dict(grid=ga, cic=c["cic_a"], fl=_settle(spectra(ga, 36, 20260106, tables("dp", 36, 29)), c["cic_a"], ga, 36, 29))


def ff_of(cic, T):
    ff = np.zeros((cic.size, NFF), T)
    ff[:, 2] = cic
    return ff


def restate(name, prec, c=None, fields=None):
    """(values, ppmax) of a recorded result (A_ice0, A_ice1, B, C) in the precision; fields: other fields than the recorded ones (A, B)"""
    c = c or cached_cases()
    T = np.float32 if prec == "sp" else np.float64
    t = tables(prec)
    if name == "C":
        return encode(c["bout"].T.astype(T), c["grid_a"], T, False)
    if name == "B":
        f = list(range(B_FIELDS[0], sum(B_FIELDS))) if fields is None else fields
        return encode(fields_of(c["fl_b"].astype(T), f, 12), c["grid_b"], T, True)
    fl = c["fl_a"].astype(T)
    if name == "A_ice1":
        fl = ice_mask(fl, c["cic_a"], t)
    return encode(fields_of(fl, recorded_fields() if fields is None else fields, 12), c["grid_a"], T, True)


NAMES = ("A_ice0", "A_ice1", "B", "C")


# ---- the fixtures and the gates
def load_golden():
    with np.load(os.path.join(GOLDEN, "gribout_0.npz")) as z:
        return {k: z[k] for k in z.files}


def observed():
    with open(os.path.join(GOLDEN, "gribout_observed.json")) as fh:
        return json.load(fh)


def log_error(a, b, zmiss=ZMISS):
    """(the patterns of ZMISS agree, the largest |a - b| over the non-missing values)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ma, mb = a == zmiss, b == zmiss
    if not np.array_equal(ma, mb):
        return False, np.inf
    d = np.abs(a - b)[~ma]
    return True, float(d.max()) if d.size else 0.0


def gate(prec, obs, values, what="values"):
    """The gate of the device against the double precision fixture, per value (what: "values" or "ppmax"): double precision
    4 x restatement_vs_reference_dp, floored at 4 eps of the value; single precision 4 x reference_sp_vs_dp.  Nothing in it comes from the device."""
    if prec == "dp":
        return np.maximum(4.0 * obs["restatement_vs_reference_dp"][what], 4.0 * np.finfo(np.float64).eps * np.abs(np.asarray(values, np.float64)))
    return np.full(np.shape(values), 4.0 * obs["reference_sp_vs_dp"][what])
