"""Extreme-wave parameters of OUTBLOCK (ecwam_hip_outbs_extremes: KURTOSIS and W_MAXH): the C ABI, the Python layers and the Fortran
interface declare the entry point and the library exports it, and the numpy restatement the GPU tests check the kernel against
(tests/extremes_ref.py) gives answers derived here independently in double precision.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import extremes_ref as X
import harness as H
from ecwam_amd.tables import Config, Tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {f: i for i, f in enumerate(X.FIELDS)}
G = 9.806


def _tables(prec, nang=36, nfre=36):
    return Tables(Config(nang=nang, nfre=nfre, nfre_red=nfre), H.np_dtype(prec))


def test_entry_point_is_declared_and_exported():
    from ecwam_amd import api, build, lib, wamintgr

    hdr = open(os.path.join(ROOT, "include", "ecwam_hip.h")).read()
    assert re.search(r"\bint ecwam_hip_outbs_extremes\s*\(", hdr)
    for i, name in enumerate(X.FIELDS):                      # the header documents the columns in the same order
        assert re.search(rf"\b{i}\s+{name}\b", hdr), name
    assert "ecwam_hip_outbs_extremes" in lib.EXPORTS
    assert api.OUTBS_EXT_FIELDS == X.FIELDS == wamintgr.OUTBS_EXT_FIELDS
    build.build()
    assert lib.load().ecwam_hip_outbs_extremes is not None
    ftn = open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")).read()
    assert "NAME='ecwam_hip_outbs_extremes'" in ftn


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_transfer_functions_in_deep_water(prec):
    """TRANSF_BFI = 1 and TRANSF_R = 0.5 for DEPTH >= BATHYMAX and for K D > DKMAX; finite water depth moves both."""
    t = _tables(prec)
    T = t.dtype
    k = np.array([0.01, 0.05, 0.2], T)
    for d in (np.full(3, 998.999, T), np.full(3, 2000.0, T), (np.array([41.0, 45.0, 80.0]) / k.astype(np.float64)).astype(T)):
        assert np.all(X.transf_bfi(t, k, d, np.full(3, 0.3, T), np.full(3, 0.5, T)) == 1)
        assert np.all(X.transf_r(t, k, d) == 0.5)
    d = np.full(3, 5.0, T)
    assert np.all(X.transf_bfi(t, k, d, np.full(3, 0.3, T), np.full(3, 0.5, T)) != 1)
    assert np.all(X.transf_r(t, k, d) != 0.5)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_aki_solves_the_dispersion_relation(prec):
    """AKI: OM**2 = G K TANH(K D) to its tolerance EBS = 1e-4 (a Newton step below EBS leaves the residual at its square), and OM**2/G
    where K D exceeds DKMAX."""
    t = _tables(prec)
    T = t.dtype
    om = np.linspace(0.3, 3.0, 40)
    for depth in (2.0, 7.5, 30.0, 150.0):
        k = X.aki(t, om.astype(T), np.full(40, depth, T))[0].astype(np.float64)
        rel = np.abs(G * k * np.tanh(k * depth) - om ** 2) / om ** 2
        assert rel.max() < (1e-4 if prec == "sp" else 1e-7), (depth, rel.max())
    deep = X.aki(t, om.astype(T), np.full(40, 5000.0, T))[0].astype(np.float64)
    want = om.astype(T).astype(np.float64) ** 2 / G
    assert np.max(np.abs(deep - want) / want) < (1e-6 if prec == "sp" else 1e-14)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_h_max_without_skewness_and_kurtosis(prec):
    """H_MAX: HMAXN = H_C_MIN = 1 when C3 = C4 = 0, whatever the number of events."""
    t = _tables(prec)
    T = t.dtype
    z = np.zeros(4, T)
    h, _ = X.h_max(t, z, z, np.array([0.0, 1.0, 300.0, 5000.0], T))
    assert np.all(h == 1)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_w_mode_st_root(prec):
    """W_MODE_ST's result makes F(Z0) = (Z0 (RN3 Z0 + RN2) + RN1) EXP(-Z0**2/2) - 1 vanish to TOL = 1e-6 (in single precision to TOL plus
    the rounding of Z0 times F')."""
    t = _tables(prec)
    T = t.dtype
    rn3 = np.array([50.0, 1.0e3, 2.0e4, 3.0e5], T)
    rn2 = np.array([20.0, 150.0, 900.0, 4000.0], T)
    rn1 = np.array([10.0, 30.0, 60.0, 120.0], T)
    z = X.w_mode_st(t, rn3, rn2, rn1).astype(np.float64)
    r3, r2, r1 = (a.astype(np.float64) for a in (rn3, rn2, rn1))
    F = (z * (r3 * z + r2) + r1) * np.exp(-0.5 * z * z) - 1.0
    dF = (-z * z * (r3 * z + r2) + (2 * r3 - r1) * z + r1 + r2) * np.exp(-0.5 * z * z)
    slack = np.abs(dF) * np.spacing(z.astype(T)).astype(np.float64) * 4 if prec == "sp" else 0.0
    assert np.all(np.abs(F) <= 1e-6 + slack), F
    assert np.all(z > 2)


def _one_direction_case(t, n=6, seed=3):
    """Spectra with all the energy in direction 1 (a peaked shape in frequency), deep water."""
    T = t.dtype
    rng = np.random.default_rng(seed)
    fr = np.asarray(t.FR, np.float64)
    nang, nfre = len(t.TH), len(fr)
    fl = np.zeros((n, nang, nfre))
    for i in range(n):
        fp = rng.uniform(0.08, 0.2)
        fl[i, 0] = rng.uniform(20.0, 100.0) * np.exp(-1.25 * (fp / fr) ** 4) * (fr / fp) ** -5 * 3.3 ** np.exp(-((fr - fp) ** 2) / (2 * (0.08 * fp) ** 2))
    return fl.astype(T)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_goda_peakedness_of_a_single_direction(prec):
    """QP = 2 SUM f E(f)**2 df / m0**2 over the frequencies whose E(f) exceeds 0.4 of its maximum (Goda; kurtosis.F90's FLTHRS), with
    E(f) = F(f, theta_1) DELTH, df = DFIM / DELTH and m0 starting at SQRT(ZEPSILON) as KURTOSIS's SUM40 does -- in float64 here."""
    t = _tables(prec)
    fl = _one_direction_case(t)
    out, near, _ = X.kurtosis(t, fl, np.full(len(fl), 998.999, t.dtype))
    assert_goda(t, fl, out[:, COL["qp"]], prec)


def assert_goda(t, fl, qp, prec):
    delth = float(t.DELTH)
    df = np.asarray(t.DFIM, np.float64) / delth
    fr = np.asarray(t.FR, np.float64)
    e = fl[:, 0].astype(np.float64) * delth
    sel = e > 0.4 * e.max(1, keepdims=True)
    m0 = float(X.zeps(t.dtype)[1]) + np.where(sel, e * df, 0).sum(1)
    want = 2 * np.where(sel, fr * e * e * df, 0).sum(1) / m0 ** 2
    assert np.all((want > 0.5) & (want < 15))
    rel = np.abs(qp.astype(np.float64) - want) / want
    assert rel.max() < (2e-5 if prec == "sp" else 1e-12), rel


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_bfi_in_deep_water(prec):
    """Deep water (TRANS = 1): BF2 = 2 (EPS SQRT(PI) QP)**2 with EPS = XKP SQRT(SUM0) -- SIG_OM = 1 / (SQRT(PI) QP) -- from the
    restatement's own QP, XKP and SUM0, in float64, where BF2 is inside its clamp."""
    t = _tables(prec)
    case = H.make_point_case(300, Config(nang=36, nfre=36, nfre_red=36), prec, spectra="mixed", seed=9)
    depth = np.full(300, 998.999, t.dtype)
    out, _, diag = X.kurtosis(t, case["FL1"], depth)
    assert np.all(diag["trans"] == 1)
    qp = out[:, COL["qp"]].astype(np.float64)
    eps = diag["xkp"].astype(np.float64) * np.sqrt(diag["sum0"].astype(np.float64))
    want = 2 * (eps * np.sqrt(np.pi) * qp) ** 2
    live = (want > 1e-3) & (want < 4.9)
    assert live.mean() > 0.5
    rel = np.abs(out[live, COL["bfi"]] - want[live]) / want[live]
    assert rel.max() < (2e-6 if prec == "sp" else 1e-13), rel.max()


def test_nint_rounds_half_away_from_zero():
    """XNSLC = NINT(DUR OM_UP): a half-integer rounds upward (away from zero), unlike numpy's round half to even."""
    x = np.array([2.5, 3.5, 0.5, 1.49999, -2.5, 423.5], np.float32)
    assert list(X.nint(x)) == [3, 4, 1, 1, -3, 424]
    assert list(np.rint(x[:1])) == [2]


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_zero_spectrum(prec):
    """An empty spectrum: SUM0 = ZEPSILON, so C3 = C4 = 0, HMAXN = H_C_MIN and HMAX = 4 SQRT(ZEPSILON); every W_MAXH output 0."""
    t = _tables(prec)
    fl = np.zeros((3, 36, 36), t.dtype)
    wv = np.ones((3, 36), t.dtype) * 0.05
    out, near = X.extremes(t, fl, np.array([5.0, 100.0, 998.999], t.dtype), wv)
    ze = float(X.zeps(t.dtype)[0])
    assert np.all(out[:, [COL[c] for c in ("c4", "c3", "bfi", "qp", "tmax", "xnslc", "eta_m", "r")]] == 0)
    assert np.allclose(out[:, COL["hmax"]], 4 * np.sqrt(ze), rtol=1e-6)
    assert np.all(out[:, 9:] == 0) and not near.any()
