"""Known answers and properties of tests/integrals_ref.py, the restatement ecwam_hip_outbs_integrals and ecwam_hip_outsetwmask are checked
against (no GPU), the binding's exports, and the share of the GPU test's inputs whose decisions flip between a single- and a double-precision
evaluation of the restatement -- what justifies the 1 % exclusion cap of tests/test_gpu_outbs_integrals.py."""
import numpy as np
import pytest

import harness as H
import integrals_ref as R
from ecwam_amd.tables import Config, Tables


def _t(prec="dp", nang=12, nfre=36, **kw):
    return Tables(Config(nang=nang, nfre=nfre, nfre_red=nfre, **kw), H.np_dtype(prec))


def _spectra(t, n=40, seed=3):
    cfg = t.cfg
    case = H.make_point_case(n, cfg, "dp" if t.dtype == np.float64 else "sp", spectra="mixed", seed=seed)
    wv, ff, _ = H.pack_device_inputs(case)
    return case["FL1"], wv, ff


def test_exports_and_argument_counts():
    """Fails on the parent commit: the three entry points, with the documented numbers of arguments."""
    import ctypes as C

    from ecwam_amd import lib

    for name in ("ecwam_hip_set_outbs_integrals", "ecwam_hip_outbs_integrals", "ecwam_hip_outsetwmask"):
        assert name in lib.EXPORTS
    assert lib.ABI_VERSION == 6
    header = open(lib.INCLUDE if hasattr(lib, "INCLUDE") else __import__("os").path.join(lib.HERE, "..", "include", "ecwam_hip.h")).read()
    for name, nargs in (("ecwam_hip_set_outbs_integrals", 6), ("ecwam_hip_outbs_integrals", 11), ("ecwam_hip_outsetwmask", 11)):
        proto = header[header.index(f"int {name}("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == nargs, (name, proto)
    from ecwam_amd import api

    assert len(api.OUTBS_INT_FIELDS) == 8 and api.OUTBS_INT_FIELDS == R.FIELDS and api.OUTBS_INT_GROUPS == R.GROUPS
    assert sum(api.OUTBS_INT_GROUPS.values()) == api.OUTBS_INT_ALL == 63
    for m in ("set_outbs_integrals", "outbs_integrals", "outsetwmask"):
        assert hasattr(api.HipContext, m)
    assert _t().DELKCC_GC.shape == _t().DELKCC_GC_NS.shape
    assert np.allclose(_t().DELKCC_GC * _t().OMXKM3_GC, _t().DELKCC_OMXKM3_GC, rtol=1e-15)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_band_additivity(prec):
    """The trapezoid is additive on the piecewise-linear F1D: the energies of adjacent bands (less the EPSMIN each starts from) add up to
    the energy of their union."""
    t = _t(prec)
    F, _, _ = _spectra(t)
    tol = 40 * float(np.finfo(t.dtype).eps)
    for a, b, c in ((10.0, 12.0, 14.0), (12.0, 14.0, 17.0), (10.0, 17.0, 25.0), (3.3, 7.1, 10.0)):
        e1, e2, eu = (R.sebtmean(t, F, x, y).astype(np.float64) for x, y in ((a, b), (b, c), (a, c)))
        eps0 = float(t.EPSMIN)
        err = np.abs((e1 - eps0) + (e2 - eps0) - (eu - eps0)) / np.maximum(eu, 1e-12)
        assert err.max() < tol, (a, b, c, err.max())


def test_band_special_cases():
    t = _t("dp")
    F, _, _ = _spectra(t)
    M = len(t.FR)
    # wholly above FR(NFRE): the f**-5 term alone
    c = R.band_constants(t, 0.5, 0.9)
    assert c["tail"] and not c["front"] and all(v == 0 for v in c["df"].values())
    f1d = F[:, :, M - 1].sum(1) * t.DELTH
    want = t.EPSMIN + 0.25 * t.FR5[M - 1] * (0.9 ** 4 - 0.5 ** 4) * f1d
    assert np.allclose(R.sebtmean(t, F, 0.5, 0.9), want, rtol=1e-12)
    # 25-30 s with FR(1) = 0.0345 Hz: 1/30 < FR(1): the linear front tail
    assert abs(float(t.FR[0]) - 0.0345) < 1e-3
    c = R.band_constants(t, 25.0, 30.0)
    assert c["front"] and not c["tail"] and c["mcutb"] == 1
    assert not R.band_constants(t, 21.0, 25.0)["front"]
    # TB = TT: EPSMIN
    assert np.all(R.sebtmean(t, F, 11.0, 11.0) == t.EPSMIN)
    # SE10MEAN is the band (10, 1/FR(1)); a full-range band holds the energy of the trapezoid rule over the grid
    full = R.sebtmean(t, F, 1.0 / float(t.FR[M - 1]), 1.0 / float(t.FR[0]))
    fr = t.FR.astype(np.float64)
    f1 = F.sum(1) * t.DELTH
    trap = (0.5 * (fr[1:] - fr[:-1]) * (f1[:, 1:] + f1[:, :-1])).sum(1)
    assert np.allclose(full, trap + t.EPSMIN, rtol=1e-9)


def test_weflux_ctcor_and_slopes():
    t = _t("dp")
    F, wv, ff = _spectra(t)
    n, K, M = F.shape
    # one occupied direction returns that direction; the magnitude is ROG (sum of DFIM F CGROUP + the tail)
    one = np.zeros_like(F)
    one[:, 4, :] = F[:, 4, :]
    mag, deg, _ = R.weflux(t, one, wv[:, 1])
    want_deg = (np.degrees(float(t.TH[4])) + 180.0) % 360.0
    assert np.allclose(deg, want_deg, atol=1e-6)
    delt = t.FRTAIL * t.DELTH * t.G / (2 * t.ZPI)
    want = t.ROWATER * t.G * ((one[:, 4, :] * wv[:, 1] * t.DFIM).sum(1) + delt * one[:, 4, M - 1])
    assert np.allclose(mag, want, rtol=1e-12)
    # an empty spectrum: the EPSMIN guard
    _, deg0, d0 = R.weflux(t, np.zeros_like(F[:1]), wv[:1, 1])
    assert d0["wefy"][0][0] and deg0[0] == 180.0
    # CTCOR: a single occupied frequency gives 1, whichever it is; an empty spectrum ZMISS
    for m in (0, 7, M - 1):
        line = np.zeros_like(F)
        line[:, :, m] = 1.0
        assert np.allclose(R.ctcor(t, line, -999.0)[0], 1.0, rtol=1e-12)
    assert R.ctcor(t, np.zeros_like(F[:1]), -999.0)[0][0] == -999.0
    # mss: non-decreasing in the cut-off; a cut-off under FR(NFRE)'s wavenumber takes NFRE_EFF < NFRE
    halp, _ = R.halphap(t, F, wv[:, 0], ff[:, 1])
    ks = [float((t.ZPI * t.FR[m]) ** 2 / t.G) for m in (9, 19, 29)] + [float(R.model_xkmss(t)), 5.0, 50.0, float(R.default_xkmss(t))]
    prev = None
    for k in ks:
        x, _ = R.meansqs(t, k, F, wv[:, 0], ff[:, 7], halp, 0)
        if prev is not None:
            assert np.all(x >= prev * (1 - 1e-12))
        prev = x
    assert R.cutoff_indices(t, ks[1])[1] == 20 and R.cutoff_indices(t, ks[3])[1] == M
    # OUTBETA: Z0ATM recovered from CD (below the 0.01 cap)
    cd, z0 = R.outbeta_cd(t, ff[:, 3], ff[:, 7], ff[:, 12])
    ok = cd < 0.01
    assert ok.any()
    back = t.XNLEV / (np.exp(t.XKAPPA / np.sqrt(cd[ok])) - 1.0)
    assert np.allclose(back, z0[ok], rtol=1e-10)
    for gcb in (False, True):
        tt = _t("dp", llgcbz0=gcb)
        cap = R.outbeta_cd(tt, np.array([50.0]), np.array([2.0]), np.array([1.0]))
        amax = tt.ALPHAMAX if gcb else min(tt.ALPHAMAX, 0.02 + 0.01 * 50.0)
        z = tt.RNUM / 2.0 + tt.GM1 * amax * 4.0
        assert np.isclose(cap[1][0], z, rtol=1e-12)


def test_outsetwmask_on_a_hand_made_buffer():
    buf = np.arange(12, dtype=np.float64).reshape(4, 3)
    cic = np.array([0.0, 0.5, 0.2, 0.9])
    iodp = np.array([1, 1, 0, 0], np.int32)
    got = R.outsetwmask(buf, [1, 2, 0], cic, iodp, True, 0.3, -999.0)
    want = np.array([[0, 1, 2], [-999, 4, 5], [6, -999, 8], [-999, -999, 11]], np.float64)
    assert np.array_equal(got, want)
    assert np.array_equal(R.outsetwmask(buf, [1, 0, 1], cic, None, False, 0.3, -999.0), buf)       # no LICERUN: no ice mask
    both = R.outsetwmask(buf, [3, 3, 3], cic, iodp, True, 0.3, -999.0)
    assert np.all(both[1:] == -999.0) and np.array_equal(both[0], buf[0])


@pytest.mark.parametrize("nang,nfre,gcb", [(36, 36, True), (12, 25, False)])
def test_decision_flips_between_precisions_stay_under_the_cap(nang, nfre, gcb):
    """The mixed spectra of the GPU test (before IMPLSCH; the same generator and seed), evaluated by the restatement in single and in double
    precision: per decision, the share of points whose branch differs.  A second implementation in the same precision can flip no more
    points than lie within rounding of a threshold, and the step from single to double precision moves every quantity by far more than
    MARGIN_EPS ulp does -- so these shares bound the exclusions from above.  Also: the share of points within MARGIN_EPS = 64 eps."""
    n = 3001
    res = {}
    for prec in ("sp", "dp"):
        cfg = Config(nang=nang, nfre=nfre, nfre_red=nfre, llgcbz0=gcb)
        case = H.make_point_case(n, cfg, prec, spectra="mixed", seed=17)
        wv, ff, _ = H.pack_device_inputs(case)
        ff[::3, 13] = np.linspace(0.1, 3.0, len(ff[::3]))
        res[prec] = R.integrals(case["tables"], case["FL1"], wv, ff)[1]
    eps = float(np.finfo(np.float32).eps)
    for name in res["sp"]:
        flips = float(np.mean(res["sp"][name][0] != res["dp"][name][0]))
        near = float(np.mean(res["sp"][name][1] < 64 * eps))
        print(f"{nang}x{nfre} {name}: branch differs between sp and dp at {flips:.4%} of the points; within 64 eps of the threshold {near:.4%}")
        if name != "ctcor_cap":
            assert flips <= 0.01 and near <= 0.01, (name, flips, near)
