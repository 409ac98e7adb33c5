"""The second-order tables (ecwam_amd/second_order.py: SECONDHH_GEN, TABLES_2ND) against the known answers the reference prints itself
(secondhh_gen.F90:139-168), and properties of the numpy restatement of CAL_SECOND_ORDER_SPEC (tests/second_order_ref.py).

Tolerance of the known answers: the deep-water formulas are compared with the slice JD = NDEPTH, depth 1.1**73 = 1051 m, not infinite, and the
reference regularises its formulas (A1 / A3 add 1E-8 to the frequencies, B3 1E-5, V2 moves the wave numbers by up to 1E-5).  The agreement the
reference's own TABLES_2ND gives in double precision -- its tables recorded in tests/golden/second_order_nang12_dp.npz against the same
formulas -- is A 3.9E-8, B 3.3E-5, C_QL 1.4E-4 (test_golden_tables... prints it); each table's gate is three times its own figure.
"""
import os

import numpy as np
import pytest

import second_order_ref as R
from ecwam_amd.second_order import SecondOrderTables
from ecwam_amd.tables import Config, Tables

# three times the reference's own agreement with the deep-water formulas, per table
KNOWN_GATE = dict(A=3 * 3.9e-8, B=3 * 3.3e-5, C=3 * 1.4e-4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "second_order_nang12_dp.npz")


@pytest.fixture(scope="module")
def so12():
    t = Tables(Config(nang=12, nfre=36, nfre_red=36), np.float64)
    return SecondOrderTables(t)


def _spectra(so, n=6, seed=1, scale=1.0):
    """Smooth one-peak spectra (m^2 s / rad), deep water wave numbers, 200 m of water."""
    t = so.t
    rng = np.random.default_rng(seed)
    fp = rng.uniform(0.08, 0.2, n)[:, None, None]
    th0 = rng.uniform(0, 2 * np.pi, n)[:, None, None]
    fr, th = t.FR[None, None, :].astype(np.float64), t.TH[None, :, None].astype(np.float64)
    e = 0.5 * scale * np.exp(-0.5 * ((fr - fp) / (0.25 * fp)) ** 2) * np.maximum(np.cos(th - th0), 0.0) ** 2
    wn = np.broadcast_to(((t.ZPI * t.FR) ** 2 / t.G), (n, len(t.FR))).astype(t.dtype)
    return np.ascontiguousarray(e, t.dtype), np.ascontiguousarray(wn), np.full(n, 200.0, t.dtype)


@pytest.mark.parametrize("nang", [12, 36])
def test_sizes_and_deep_water_known_answers(nang):
    t = Tables(Config(nang=nang, nfre=36, nfre_red=36), np.float64)
    so = SecondOrderTables(t)
    assert (so.NFREH, so.NANGH, so.MR, so.MA, so.NMAX, so.NDEPTH) == (18, nang // 2, 2, 2, 22, 74)
    assert so.IM_P.min() >= 1 and so.IM_P.max() <= so.NMAX and so.IM_M.min() >= 1 and so.IM_M.max() <= so.NMAX
    for c in so.COEFFICIENTS:
        a = getattr(so, c)
        assert a.shape == (74, nang // 2, 18, 18) and np.isfinite(a).all(), c
    obs = _deep_water_agreement(so.OMEGA, so.DFDTH, t.G, so.TA[-1], so.TB[-1], so.TC_QL[-1])
    print("deep-water known answers, largest relative difference:", obs)
    for k, gate in KNOWN_GATE.items():
        assert obs[k] < gate, (k, obs[k], gate)


def _deep_water_agreement(OMEGA, DFDTH, G, TA, TB, TC):
    """The checks SECONDHH_GEN prints (secondhh_gen.F90:139-168) on the slices [L][M1][M] of the deepest table depth: the largest relative
    difference of TA / DFDTH from ((k1+k2)/2)**2, TB / DFDTH from ((k1-k2)/2)**2 and TC_QL / DFDTH from -k0**2."""
    l = TA.shape[0] - 1
    obs = dict(A=0.0, B=0.0, C=0.0)
    for m in range(len(OMEGA)):
        om0, om1 = OMEGA[m], OMEGA[1]
        if om1 < om0 / 2:
            a = ((om1 ** 2 / G + (om0 - om1) ** 2 / G) / 2) ** 2
            obs["A"] = max(obs["A"], abs(TA[l, 1, m] / DFDTH[1] / a - 1))
        b = (abs(om0 ** 2 / G - (2 * om0) ** 2 / G) / 2) ** 2
        obs["B"] = max(obs["B"], abs(TB[l, m, m] / DFDTH[m] / b - 1))
        c = -(om0 ** 2 / G) ** 2
        obs["C"] = max(obs["C"], abs(TC[l, m, m] / DFDTH[m] / c - 1))
    return obs


def test_golden_tables_of_the_reference(so12):
    """The numpy tables against the reference's own SECONDHH_GEN / TABLES_2ND (NANG = 12, double precision; tests/golden/
    second_order_nang12_dp.npz holds the five tables at the depth indices 1, 30 and 74, IM_P, IM_M, NMAX, OMEGA, DFDTH and TFAKH).
    Gate per table and depth: the formulas are ill-conditioned in shallow water (the quartet of TT_4M / TT_4P is nearly resonant where waves
    do not disperse, and V2 divides by frequency mismatches that 1E-5 regularises), so what two correct evaluations can differ by is measured
    on the formulas themselves: `sens` = the change of the table when DEPTHA moves by one unit in the last place.  A different libm or order of
    evaluation perturbs a handful of intermediates by that much, each amplified alike: gate = 8 sens, and at least 64 eps of the slice's
    largest entry where the depth has no influence left.  Observed error / slice maximum: TA 7.4E-14, 4.3E-15, 1.3E-15 at the three depths,
    TB 1.2E-13, 9.5E-17, 1.5E-17, TC_QL 8.7E-14, 1.7E-15, 4.8E-17, TT_4M 9.0E-5, 5.0E-10, 5.9E-17, TT_4P 5.8E-5, 5.1E-10, 5.9E-17; sens of
    TT_4M: 2.3E-4, 2.9E-10, 1E-19."""
    g = np.load(GOLDEN)
    so, jd = so12, g["jd"]
    assert list(jd) == [0, 29, 73] and int(g["nmax"]) == so.NMAX == 22
    assert np.array_equal(g["IM_P"], so.IM_P) and np.array_equal(g["IM_M"], so.IM_M)
    eps = np.finfo(np.float64).eps
    for name in ("FR", "TH"):
        assert np.max(np.abs(getattr(so.t, name) / g[name] - 1)) <= 2 * eps, name
    for name in ("OMEGA", "DFDTH"):
        assert np.max(np.abs(getattr(so, name) / g[name] - 1)) <= 4 * eps, name
    assert np.max(np.abs(so.TFAK[:, jd] / g["TFAK"] - 1)) <= 4 * eps
    own = _deep_water_agreement(g["OMEGA"], g["DFDTH"], so.t.G, g["TA"][2], g["TB"][2], g["TC_QL"][2])
    print("the reference's own agreement with the deep-water formulas:", own)
    for k, gate in KNOWN_GATE.items():
        assert own[k] < gate
    moved = SecondOrderTables(so.t, deptha=1.0 + eps)
    for c in so.COEFFICIENTS:
        mine, ref, other = getattr(so, c)[jd], g[c], getattr(moved, c)[jd]
        scale = np.abs(ref).max(axis=(1, 2, 3))
        err = np.abs(mine - ref).max(axis=(1, 2, 3)) / scale
        sens = np.abs(mine - other).max(axis=(1, 2, 3)) / scale
        gate = np.maximum(8 * sens, 64 * eps)
        print(c, "error / slice maximum", err, "sens", sens, "gate", gate)
        assert np.all(err <= gate), (c, err, gate)


def test_golden_spectra_of_the_reference(so12):
    """The restatement of CAL_SECOND_ORDER_SPEC against the reference's own routine on 16 points (depths 15.86 m, 5000 m and 1 m with
    short waves: the depth indices 30, 74 and 1 whose tables are recorded), with the reference's tables in place of the numpy ones so
    that the ill-conditioning of TT_4M / TT_4P does not enter: the gate is the rounding bound n u S of tests/test_gpu_second_order.py.
    Observed: equal bit for bit.  With the numpy tables the result is within 1E-9 of the peak."""
    g = np.load(GOLDEN)
    so, jd = so12, g["jd"]
    full = []
    for c in so.COEFFICIENTS:
        a = np.full(getattr(so, c).shape, np.nan)
        a[jd] = g[c]
        full.append(a)
    got, info = R.cal_second_order_spec(so, g["F1_before"], g["WAVNUM"], g["DEPTH"], 1.0, tables=full)
    assert set(info["jd"]) == {0, 29, 73} and (g["F1_after"] != g["F1_before"]).mean() > 0.3
    err = np.abs(got - g["F1_after"])
    gate = info["terms"] * np.finfo(np.float64).eps / 2 * info["bound"]
    print("largest |restatement - reference|", err.max(), "of a peak of", g["F1_after"].max())
    assert np.all(err <= gate)
    own, _ = R.cal_second_order_spec(so, g["F1_before"], g["WAVNUM"], g["DEPTH"], 1.0)
    peak = g["F1_after"].max(axis=(1, 2))
    rel = np.abs(own - g["F1_after"]).max(axis=(1, 2)) / peak
    print("with the numpy tables: largest difference / peak per point", rel)
    # the TT_4M / TT_4P slice of 1 m differs by up to 9E-5 of its maximum (above), the correction is at most 1E-2 of the peak there
    assert np.all(rel < 8 * 2.3e-4 * 1e-2)


def test_single_precision_tables_follow_the_double_ones():
    """The same formulas in single precision: finite everywhere, and TA / TB (no cancellation) within 1e-3 of the double precision values."""
    cfg = Config(nang=12, nfre=36, nfre_red=36)
    s, d = SecondOrderTables(Tables(cfg, np.float32)), SecondOrderTables(Tables(cfg, np.float64))
    assert s.NMAX == d.NMAX and np.array_equal(s.IM_P, d.IM_P) and np.array_equal(s.IM_M, d.IM_M)
    for c in s.COEFFICIENTS:
        assert getattr(s, c).dtype == np.float32 and np.isfinite(getattr(s, c)).all(), c
    for c in ("TA", "TB"):
        assert np.max(np.abs(getattr(s, c) - getattr(d, c))) < 1e-3 * np.max(np.abs(getattr(d, c))), c


def test_odd_sizes_are_refused():
    with pytest.raises(ValueError, match="even"):
        SecondOrderTables(Tables(Config(nang=12, nfre=25, nfre_red=25), np.float64))


def test_zero_spectrum_stays_within_the_clamp(so12):
    f, wn, d = _spectra(so12, 3)
    f[:] = 0
    out, info = R.cal_second_order_spec(so12, f, wn, d)
    assert np.all(out >= 0) and np.all(out <= 1e-6)


def test_inverse_returns_the_input_to_first_order(so12):
    f, wn, d = _spectra(so12)
    fwd, info = R.cal_second_order_spec(so12, f, wn, d, 1.0)
    back, _ = R.cal_second_order_spec(so12, fwd, wn, d, -1.0)
    corr = np.abs(fwd - f).max(axis=(1, 2))
    left = np.abs(back - f).max(axis=(1, 2))
    peak = f.max(axis=(1, 2))
    s = (info["bound"] - np.abs(f)).max(axis=(1, 2))          # the largest sum of |terms|: the correction is a quadratic form in F
    print("correction / peak", corr / peak, "left after the inverse / peak", left / peak, "sum of |terms| / peak", s / peak)
    assert np.all(corr > 0)
    # back - f = C(f) - C(f + C(f)) with C quadratic in F: of second order, a fraction O(S / peak) of the correction (S / peak < 0.02 here);
    # a mapping that was not inverted would leave 2 corr, one that ignored SIG would leave corr
    assert np.all(left < 0.2 * corr)


def test_emaxl_switches_the_correction_off(so12):
    f, wn, d = _spectra(so12)
    d[::2] = 1.0     # EMEAN of these spectra is above 0.6**2/16 m**2 there
    out, info = R.cal_second_order_spec(so12, f, wn, d)
    assert np.all(info["emean"][::2] > 0.0225 * d[::2] ** 2) and np.all(info["emaxl"][::2] == 0) and np.all(info["emaxl"][1::2] == 1)
    assert np.array_equal(out[::2], f[::2]) and not np.array_equal(out[1::2], f[1::2])


def test_rotation_by_ma_directions_rotates_the_result(so12):
    f, wn, d = _spectra(so12)
    out, _ = R.cal_second_order_spec(so12, f, wn, d)
    rot, _ = R.cal_second_order_spec(so12, np.roll(f, so12.MA, axis=1), wn, d)
    assert np.allclose(rot, np.roll(out, so12.MA, axis=1), rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("nang", [12, 36])
def test_device_case_covers_its_branches_and_the_near_tie_cap(nang, prec):
    """What tests/test_gpu_second_order.py relies on, from the restatement alone: the depths take the branches they are meant to, and at most
    2 % of the points have a peak period that is undetermined within the FL2ND gate."""
    T = np.float32 if prec == "sp" else np.float64
    t = Tables(Config(nang=nang, nfre=36, nfre_red=36), T)
    so = SecondOrderTables(t)
    fl1, wn, depth = R.device_case(t, so)
    out, info = R.cal_second_order_spec(so, fl1, wn, depth)
    jd = info["jd"]
    assert len(set(jd[3:67])) >= 3 and set(jd[67:131]) == {so.NDEPTH - 1}
    assert (jd == 0).any() and (1.0 / info["akmean"] > depth).any()
    assert (info["emaxl"] == 0).any() and (info["emaxl"] == 1).sum() > 100
    gate = info["terms"] * float(np.finfo(T).eps) / 2 * info["bound"]
    tie = R.near_tie(out, gate)
    print(f"{nang} {prec}: near ties {int(tie.sum())} of {len(tie)}")
    assert tie.mean() <= 0.02
