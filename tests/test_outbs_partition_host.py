"""Swell-train partitioning of OUTBLOCK (ecwam_hip_outbs_partition: SEPWISW with LLPARTITION = T, SEP3TR, FNDPRT, PARMEAN): the C ABI
declares and exports the entry point, and the numpy restatement the GPU tests check the kernel against (tests/partition_ref.py) gives the
hand results of spectra whose answer is known.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import partition_ref as P
import sepwisw_ref as S
from ecwam_amd import synthetic as syn
from ecwam_amd.tables import Config, Tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {f: i for i, f in enumerate(P.FIELDS)}
G = 9.806


def test_entry_point_is_declared_and_exported():
    from ecwam_amd import api, build, lib, wamintgr

    hdr = open(os.path.join(ROOT, "include", "ecwam_hip.h")).read()
    assert re.search(r"\bint ecwam_hip_outbs_partition\s*\(", hdr)
    assert "ecwam_hip_outbs_partition" in lib.EXPORTS
    assert api.OUTBS_PART_FIELDS == P.FIELDS and len(api.OUTBS_PART_FIELDS) == 24
    assert api.OUTBS_PART_FIELDS[:15] == api.OUTBS_SEP_FIELDS
    assert wamintgr.OUTBS_PART_FIELDS == P.FIELDS
    build.build()
    assert lib.load().ecwam_hip_outbs_partition is not None
    ftn = open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")).read()
    assert "NAME='ecwam_hip_outbs_partition'" in ftn


def test_nangh_rounds_half_away_from_zero():
    """NINT(75/360 NANG) + 1: 2.5 at 12 and 7.5 at 36 directions are exact in both precisions and round up."""
    for dt in (np.float32, np.float64):
        got = [P.nangh(Tables(Config(nang=k, nfre=25, nfre_red=25), dt)) for k in (12, 24, 36, 48)]
        assert got == [4, 6, 9, 11], (dt, got)


def multi_system_case(t, n, seed):
    """Multi-system spectra with a synthetic wind-sea mask, deep-water CINV, random UFRIC and MIJ: (fl1, xllws, mij, cinv, ufric, wdwave)."""
    T = t.dtype
    M = len(t.FR)
    rng = np.random.default_rng(seed)
    wd = rng.uniform(0.0, 2 * np.pi, n).astype(T)
    fl, _ = syn.multi_system_spectra(t.FR, t.TH, wd, T, seed=seed + 1)
    xl = S.synthetic_xllws(t, wd, 0.15)
    cinv = np.ascontiguousarray(np.broadcast_to((t.ZPI * t.FR / T(G)).astype(T), (n, M)))
    uf = rng.uniform(0.2, 0.6, n).astype(T)
    mij = rng.integers(M // 2, M + 1, n).astype(np.int32)
    return fl, xl, mij, cinv, uf, wd


@pytest.mark.parametrize("nang,nfre", [(12, 25), (24, 36)])
def test_literal_and_vectorised_fndprt_agree(nang, nfre):
    """The order-independence of a sweep: visiting the bins one by one in the reference's order and updating whole planes give the same
    partitions, sweep counts and results on a few hundred multi-system spectra (single precision: the decisions of the device)."""
    t = Tables(Config(nang=nang, nfre=nfre, nfre_red=nfre), np.float32)
    n = 300 if nang == 12 else 120
    fl, xl, mij, cinv, uf, wd = multi_system_case(t, n, seed=41)
    a, ia = P.partition(t, fl, xl, mij, cinv, uf, wd, literal=True)
    b, ib = P.partition(t, fl, xl, mij, cinv, uf, wd)
    assert np.array_equal(ia["w1"], ib["w1"]) and np.array_equal(ia["assigned"], ib["assigned"])
    assert np.array_equal(ia["sweeps"], ib["sweeps"])
    assert np.array_equal(a, b)
    assert (ib["sweeps"] > 2).any() and (ib["npeak_fndprt"] > 1).any()


def known_answer_inputs(t):
    """One point each, XLLWS and UFRIC as named, MIJ = NFRE unless stated:
      allsea   every XLLWS = 1 (no swell)                 oneswell  one swell system, everything swell (UFRIC 0)
      twoswell two separated swells, E1 > E2             trunc     one swell and an MIJ with INT(1/FR(MIJ)) <= its mean period < 1/FR(MIJ)
      manypk   a spectrum with more than NPMAX local maxima
    Returns (names, fl1, xllws, mij, cinv, ufric, wdwave, extra)."""
    T = t.dtype
    K, M = len(t.TH), len(t.FR)
    cinv1 = (t.ZPI * t.FR / T(G)).astype(T)
    names, fl, xl, mj, uf, wd = [], [], [], [], [], []

    def add(name, f, x, m, u, w):
        names.append(name); fl.append(np.asarray(f, T)); xl.append(np.asarray(x, T)); mj.append(m); uf.append(u); wd.append(w)

    def swell(fp, th, alfa):
        return syn.jonswap_spectra(t.FR, t.TH, np.array([fp]), np.array([th]), T, alfa=alfa)[0]

    zero = np.zeros((K, M), T)
    add("allsea", syn.jonswap_spectra(t.FR, t.TH, np.array([0.1]), np.array([1.0]), T)[0], np.ones((K, M), T), M, 0.3, 1.0)
    s1 = swell(0.07, 2.0, 0.004)
    add("oneswell", s1, zero, M, 0.0, 2.0)
    a, b = swell(0.06, 0.5, 0.006), swell(0.1, 3.5, 0.003)
    add("twoswell", a + b, zero, M, 0.0, 0.5)
    tr, tmij = truncation_case(t)
    add("trunc", tr, zero, tmij, 0.0, 4.0)
    add("manypk", syn.many_peak_spectra(t.FR, t.TH, 1, T)[0], zero, M, 0.0, 0.0)
    n = len(names)
    extra = dict(oneswell=(s1, 2.0), twoswell=((a, 0.5), (b, 3.5)))
    return (names, np.ascontiguousarray(np.stack(fl), T), np.ascontiguousarray(np.stack(xl), T), np.array(mj, np.int32),
            np.ascontiguousarray(np.broadcast_to(cinv1, (n, M)), T), np.array(uf, T), np.array(wd, T), extra)


def truncation_case(t):
    """A single swell system and an MIJ for which the partition's mean period lies in [INT(1/FR(MIJ)), 1/FR(MIJ)): kept only because
    SEP3TR's FRINVMIJ is an INTEGER.  Found by a scan over the peak frequency on the restatement."""
    T = t.dtype
    K, M = len(t.TH), len(t.FR)
    zero = np.zeros((1, K, M), T)
    cinv = (t.ZPI * t.FR / T(G)).astype(T)[None]
    for mij in range(M - 4, 8, -1):
        inv = float(T(1.0) / t.FR[mij - 1])
        if inv - np.trunc(inv) < 0.15:
            continue
        for fp in np.linspace(float(t.FR[mij - 4]), float(t.FR[mij - 1]), 60):
            f = syn.jonswap_spectra(t.FR, t.TH, np.array([fp]), np.array([4.0]), T, alfa=0.01)
            _, info = P.partition(t, f, zero, np.array([mij]), cinv, np.zeros(1, T), np.array([4.0], T))
            per = float(info["pmtrain"][0, 0])
            if np.trunc(inv) <= per < inv and info["nz"][0] >= 1:
                return f[0], mij
    raise AssertionError("no truncation case on this grid")


def _cyc(a, b):
    d = abs(a - b) % 360.0
    return min(d, 360.0 - d)


def known_answer_checks(t, names, fl1, out, extra, info=None):
    """The hand results of known_answer_inputs (shared with the device test)."""
    o = {nm: out[i].astype(np.float64) for i, nm in enumerate(names)}
    dbin = float(np.degrees(float(t.DELTH)))
    wdir = lambda th: float(np.fmod(P.DEG * th + 180.0, 360.0))
    # all wind sea: no trains, the directions are the wind's, the periods 0
    a = o["allsea"]
    for s in range(3):
        assert a[15 + 3 * s] == 0 and a[17 + 3 * s] == 0, a[15:]
        assert abs(a[16 + 3 * s] - wdir(1.0)) < 1e-4, a[15:]
    # one swell system: train 1 carries it, trains 2 and 3 are empty
    s1, th1 = extra["oneswell"]
    e1 = float(np.asarray(S._femean(t, s1[None].astype(t.dtype))[0][0], np.float64))
    a = o["oneswell"]
    assert abs(a[COL["swh1"]] / (4 * np.sqrt(e1)) - 1) < 0.03, (a[COL["swh1"]], 4 * np.sqrt(e1))
    assert _cyc(a[COL["mwd1"]], wdir(th1)) < dbin
    assert a[COL["swh2"]] == 0 and a[COL["swh3"]] == 0 and a[COL["mwp2"]] == 0
    # two systems: in energy order, each direction within a bin
    (sa, ta), (sb, tb) = extra["twoswell"]
    a = o["twoswell"]
    ea = float(S._femean(t, sa[None].astype(t.dtype))[0][0])
    eb = float(S._femean(t, sb[None].astype(t.dtype))[0][0])
    assert ea > eb and a[COL["swh1"]] > a[COL["swh2"]] > 0 and a[COL["swh3"]] == 0
    assert _cyc(a[COL["mwd1"]], wdir(ta)) < dbin and _cyc(a[COL["mwd2"]], wdir(tb)) < dbin
    # the truncated FRINVMIJ keeps a partition whose mean period is under 1/FR(MIJ)
    a = o["trunc"]
    assert a[COL["swh1"]] > 0 and a[COL["mwp1"]] > 0
    # more than NPMAX maxima: capped, no error
    assert np.all(np.isfinite(o["manypk"])) and o["manypk"][COL["swh1"]] > 0
    if info is not None:
        i = names.index("manypk")
        assert info["npeak_found"][i] > P.NPMAX and info["npeak_fndprt"][i] == P.NPMAX
        i = names.index("trunc")
        inv = float(t.dtype(1.0) / t.FR[int(info["mij"][i]) - 1])
        assert np.trunc(inv) <= out[i, COL["mwp1"]] < inv


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_restatement_known_answers(prec):
    t = Tables(Config(nang=36, nfre=36, nfre_red=36), np.float32 if prec == "sp" else np.float64)
    names, fl1, xl, mij, cinv, uf, wd, extra = known_answer_inputs(t)
    out, info = P.partition(t, fl1, xl, mij, cinv, uf, wd)
    info["mij"] = mij
    known_answer_checks(t, names, fl1, out, extra, info)


def test_train_energies_add_up_to_ett():
    """Where NPEAK >= NPKNA, ENEX hands the swell energy no train took to the trains in proportion: their sum is ETT."""
    t = Tables(Config(nang=36, nfre=36, nfre_red=36), np.float64)
    fl, xl, mij, cinv, uf, wd = multi_system_case(t, 400, seed=7)
    out, info = P.partition(t, fl, xl, mij, cinv, uf, wd)
    em = info["emtrain"].astype(np.float64)
    sel = (info["npeak"] >= info["npkna"]) & (info["ett"] >= em.sum(1))
    assert sel.mean() > 0.3
    rel = np.abs(em[sel].sum(1) - info["ett"][sel]) / info["ett"][sel]
    assert rel.max() < 1e-12, rel.max()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_columns_0_14_are_those_of_sepwisw(prec):
    """FNDPRT's W1 never exceeds 1, so SWM * MAX(W1,1) leaves the swell mask as SEPWISW left it and the first 15 columns are the
    LLPARTITION = F ones, bit for bit; while the trains are there at most points of the multi-system set."""
    t = Tables(Config(nang=36, nfre=36, nfre_red=36), np.float32 if prec == "sp" else np.float64)
    fl, xl, mij, cinv, uf, wd = multi_system_case(t, 400, seed=11)
    out, info = P.partition(t, fl, xl, mij, cinv, uf, wd)
    ref, _ = S.sepwisw(t, fl, xl, cinv, uf, wd)
    assert info["w1"].max() <= 2                                       # half units
    assert np.array_equal(out[:, :15], ref)
    assert (info["nz"] >= 1).mean() > 0.5 and (info["nz"] >= 2).mean() > 0.2
