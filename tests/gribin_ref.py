"""GETSPEC's GRIB read restated in numpy from the reference's Fortran, in the reference's order of operations and in the precision asked for:
TEST INFRASTRUCTURE.  Three statements --
  grib2wgrid.F90:771-775   the un-scaling: V /= PMISS: V = 10**(V - |PPREC|) - PPEPS, a missing value stays missing
  grib2wgrid.F90:793-802   the full copy of the vector into FIELD(I,K), K = 1 .. NGY north to south, from the first value on (no start offset),
  getspec.F90:458-462      and the gather WORK(IJ) = FIELD(IXLG(IJ), NGY - KXLT(IJ) + 1)
  getspec.F90:548-552      FL1(IJ,K,M) = WORK(IJ), ZMISS -> EPSMIN
-- written from the Fortran, through the two-dimensional FIELD as the reference goes, not from the kernels of csrc/gribin.hip and not through the
map of ecwam_amd/gribout.py, which it therefore checks as well.  tests/test_gribin_host.py holds it against flang's evaluation of the same
statements (tests/golden/gribin_0.npz, recorded by tools/make_golden_gribin.py with tools/gribin_driver.F90) and tests/test_gpu_gribin.py takes
the inputs and the gates from it.

The inputs are the reference's own single precision VALUES of tests/golden/gribout_0.npz (the results of WGRIBENCODE_VALUES for the cases A_ice0,
A_ice1 and B of tests/gribout_ref.py), fed to both precisions: float32-representable, with both pole rows, land and thresholded-to-missing cells
(A), and a vector that begins north of the grid (B: the full copy has no start offset, so the read of B goes through the map of the READ,
gribout.read_map, not through the output map -- the case of a message laid out otherwise than the output of the same configuration).
"""
from __future__ import annotations

import json
import os

import numpy as np

import gribout_ref as G
from ecwam_amd import gribout

GOLDEN = G.GOLDEN
NAMES = ("A_ice0", "A_ice1", "B")
PPEPS = G.OPTS["ppeps"]
ZMISS = G.ZMISS


def grid_of(name, c=None):
    c = c or G.cached_cases()
    return c["grid_b"] if name == "B" else c["grid_a"]


def fields_of(name):
    """the fields (f = M NANG + K) the inputs of a case hold, in their order"""
    return list(range(G.B_FIELDS[0], sum(G.B_FIELDS))) if name == "B" else G.recorded_fields()


def inputs(name):
    """the decoded vectors of a case [nfld][NTENCODE], float32: the reference's own single precision VALUES"""
    v = G.load_golden()[f"{name}_sp"]
    assert v.dtype == np.float32
    return v


def read_map(g):
    return gribout.read_map(g["nlonrgg"], g["ixlg"], g["kxlt"], g["ngy"])


def unscale(values, T, o=G.OPTS):
    """grib2wgrid.F90:771-775 in T"""
    T = np.dtype(T).type
    v = np.asarray(values, T)
    ok = v != T(o["zmiss"])
    with np.errstate(over="ignore"):
        p = np.power(T(10), (np.where(ok, v, T(0)) - abs(T(o["pprec"]))).astype(T)).astype(T)
    return np.where(ok, (p - T(o["ppeps"])).astype(T), T(o["zmiss"])).astype(T)


def gather(values, g):
    """grib2wgrid.F90:793-802 and getspec.F90:458-462: values [nfld][nvalues] -> WORK [nfld][npts] through FIELD(NGX,NGY)"""
    values = np.asarray(values)
    ngx, ngy, nlon = g["ngx"], g["ngy"], g["nlonrgg"]
    field = np.full((values.shape[0], ngy, ngx), np.nan, values.dtype)      # FIELD(I,K); K = 1 the northernmost row
    at = 0
    for k in range(ngy):
        n = int(nlon[ngy - 1 - k])
        field[:, k, :n] = values[:, at:at + n]
        at += n
    work = field[:, ngy - g["kxlt"], g["ixlg"] - 1]
    assert not np.isnan(work).any()
    return np.ascontiguousarray(work)


def decode(values, g, prec, unscaled=True, o=G.OPTS):
    """FL1 elements [nfld][npts] of the fields of `values`, in the precision: un-scale, copy and gather, ZMISS -> EPSMIN"""
    t = G.tables(prec)
    T = t.dtype
    v = np.asarray(values, T)
    if unscaled:
        v = unscale(v, T, o)
    w = gather(v, g)
    return np.where(w == T(o["zmiss"]), T(t.EPSMIN), w).astype(T)


def from_missing(values, g):
    """[nfld][npts]: the elements whose value was missing"""
    return gather(np.asarray(values, np.float64), g) == ZMISS


def restate(name, prec, c=None):
    return decode(inputs(name), grid_of(name, c), prec)


# ---- the fixtures and the gates
def load_golden():
    with np.load(os.path.join(GOLDEN, "gribin_0.npz")) as z:
        return {k: z[k] for k in z.files}


def observed():
    with open(os.path.join(GOLDEN, "gribin_observed.json")) as fh:
        return json.load(fh)


def rel_error(a, b):
    """the largest |a - b| / (|b| + PPEPS)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (np.abs(b) + PPEPS)).max()) if a.size else 0.0


def gate(prec, obs):
    """The gate of the device against the double precision fixture on |a - b| / (|b| + PPEPS): double precision 4 x restatement_vs_reference_dp,
    floored at 4 eps; single precision 4 x reference_sp_vs_dp.  The factor 4 is the margin of gribout_ref.gate, for the same reason: one
    power function against another.  Nothing in it comes from the device."""
    if prec == "dp":
        return max(4.0 * obs["restatement_vs_reference_dp"], 4.0 * float(np.finfo(np.float64).eps))
    return 4.0 * obs["reference_sp_vs_dp"]
