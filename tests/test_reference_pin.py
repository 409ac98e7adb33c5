"""The oracle pinned to the reference's own Fortran (run with -m "not gpu").

tests/golden/reference_*.npz hold what the reference's unmodified IMPLSCH (with its whole call tree), WDFLUXES, CTUWINI + CTUW and PROPAGS2
returned, in both precisions, on the sea states the GPU gates were set on (tools/make_golden_reference.py, tests/reference_cases.py).

  (a) the oracle (oracle/ora_*.c) against every fixture, sp and dp: runs everywhere;
  (b) where the reference libraries are built (oracle/_ref/, a reference tree exists): the live reference against the fixture -- a stale
      fixture or another compiler shows here.  Not bit-identity (another libm may be underneath): the dp gate of (a);
  (c) where they are built: the live reference against the oracle on a second seed that is in no fixture.

Gates (none invented here).  Double precision: the project's gates of the device against the oracle are the CEILING -- spectra and forcing 1e-10,
fluxes 1e-8 (WAVE2OCEAN 1e-10 of the column's scale), MIJ and XLLWS identical.  The gate that is asserted is 10 x the maximum
observed on the CPU per configuration and quantity (tests/golden/reference_pin_observed.json, written with profiles/reference_pin.txt by
tools/reference_pin_report.py; 10 x is the project's margin of a cap over an observed maximum, here for other sea states and another libm), never
looser than the ceiling.  Only where the observed figure is exactly 0 -- the oracle reproduces the reference's bits on that quantity, so 10 x 0 would
demand the same bits of another libm -- the gate is 8 eps of the compared relative quantity (reference_cases.DP_ZERO_FLOOR).  Single precision:
harness.assert_sp_gates as it stands.  NEWWIND: the bound of test_newwind_and_layout (4 eps on TAUW, every other member identical); DEPTHPRPT: the
bounds of test_depth_props_of_the_product_and_of_the_oracle_agree (8 eps; OMOSNH2KD 64 eps).
"""
import os

import numpy as np
import pytest

import harness as H
import reference_cases as RC
from ecwam_amd import grid as G
from ecwam_amd.tables import Tables
from oracle import reference as R
from oracle.oracle import Oracle

CEILING, dp_gate, stats, figures, oracle_for = RC.CEILING, RC.dp_gate, RC.stats, RC.figures, RC.oracle_for
needs_reference = pytest.mark.skipif(not R.available(), reason="no reference tree on this machine: oracle/_ref/ is not built")


def assert_dp(name: str, st: dict, gate) -> None:
    f = figures(st)
    print(f"{name} dp: " + ", ".join(f"{q} {f[q]:.2e} (gate {gate(name, q):.1e})" for q in f))
    assert st["mij_flips"] == 0 and st["xllws_bins_diff"] == 0, st
    for q in f:
        assert f[q] <= gate(name, q), (name, q, f[q], gate(name, q))


def assert_sp(name: str, st: dict, n: int) -> None:
    f = figures(st)
    print(f"{name} sp: MIJ flips {st['mij_flips']}, XLLWS points {st['xllws_pts_diff']}, " + ", ".join(f"{q} {f[q]:.2e}" for q in f))
    H.assert_sp_gates(st, n, what=("intf",) if RC.kind(name) == "wdfluxes" else ("bins", "swh", "ff", "intf"))
    assert f["w2n"] < 2e-4      # the single precision bound of test_implsch_wam2nemo_outputs


# ---- (a) the oracle against the fixtures --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", list(RC.CONFIGS))
def test_oracle_against_the_reference_fixture(name, prec):
    inp, ref = RC.load(name)
    n = inp["FL1"].shape[0]
    assert n == RC.points(name) and n % {48: 2, 36: 3, 24: 5, 12: 10}[RC.config(name).nang] != 0
    got = RC.run(oracle_for(name, prec), inp, RC.kind(name))
    st = stats(name, ref[prec], got, prec)
    if prec == "dp":
        assert_dp(name, st, dp_gate)
    else:
        assert_sp(name, st, n)


def _advection_grid(z):
    g = G.build_grid(int(z["n_oct"]), mask="continents")
    assert g.nsea == int(z["nsea"]) and np.array_equal(g.klon, z["klon"]) and np.array_equal(g.klat, z["klat"]) and np.array_equal(g.kcor, z["kcor"])
    rows = np.asarray(g.kxlt)
    assert (np.asarray(g.klat) == g.nsea).any() and rows.min() == 1 and rows.max() == g.ngy - 2      # land; the rows next to both polar rows
    klon = np.asarray(g.klon)      # the periodic seam: some row's first sea point has its row's LAST sea point as western neighbour, and the reverse
    first, last = (np.array([f(np.flatnonzero(rows == r)) for r in np.unique(rows)]) for f in (np.min, np.max))
    assert ((klon[first, 0] == last) & (klon[last, 1] == first) & (last > first + 1)).any()
    return g


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", ["advection_12x25", "advection_split"])
def test_oracle_advection_against_the_reference_fixture(name, prec):
    """CTUWINI + CTUW and PROPAGS2 of the oracle against the reference's: the bounds of test_ctuw_and_propags2_parity (weights 8 eps, F3 16 eps)."""
    z = np.load(RC.path(name))
    g = _advection_grid(z)
    cfg = RC.advection_config()
    T = H.np_dtype(prec)
    o = Oracle(cfg, prec)
    kw = dict(ifrelfmax=RC.ADV_IFRELFMAX, delpro_lf=cfg.idelpro / 2) if name == "advection_split" else {}
    w = o.ctu_weights_wam(g, z["cg"], cfg.idelpro, **kw)
    f3 = o.propags2(g, z["f1"], w)[: g.nsea, :, : cfg.nfre_red]
    eps = np.finfo(T).eps
    dw = float(np.max(np.abs(RC.w8(Tables(cfg, T), w).astype(float) - z[f"W8_{prec}"].astype(float))))
    df = float(np.max(np.abs(f3.astype(float) - z[f"F3_{prec}"].astype(float))))
    print(f"{name} {prec}: weights {dw / eps:.2f} eps, F3 {df / eps:.2f} eps")
    assert w["NFAIL"] == 0 and dw < 8 * eps and df < 16 * eps
    assert np.array_equal(w["WLAT"], z[f"WLAT_{prec}"]) and np.array_equal(w["WCOR"], z[f"WCOR_{prec}"])
    if name == "advection_split":      # the two time steps are both in the weights
        one = np.load(RC.path("advection_12x25"))[f"W8_{prec}"]
        assert np.max(np.abs(one[:, 1:, :, : RC.ADV_IFRELFMAX] - z[f"W8_{prec}"][:, 1:, :, : RC.ADV_IFRELFMAX])) > 1e-3
        assert np.array_equal(one[..., RC.ADV_IFRELFMAX:], z[f"W8_{prec}"][..., RC.ADV_IFRELFMAX:])


def fused_reference(z) -> dict:
    return dict(FL1=z["FL1_dp"], MIJ=z["MIJ"], XLLWS=z["XLLWS"].astype(np.float64), FF=z["FF_dp"], INTF=z["INTF_dp"])


def test_oracle_whole_step_against_the_reference_fixture():
    """PROPAGS2 followed by IMPLSCH at 36 x 36 in double precision: the sequence the one-kernel step of the device is compared with."""
    z = np.load(RC.path("fused_36_dp"))
    g = _advection_grid(z)
    cfg = RC.fused_config()
    o = Oracle(cfg, "dp")
    n = g.nsea
    f3 = o.propags2(g, z["f1"], o.ctu_weights(g, z["cg"], float(cfg.idelpro)))
    wv = z["WV"]
    got = o.implsch(f3[:n], wv[:, 0], wv[:, 1], wv[:, 2], wv[:, 3], wv[:, 4], z["ENV"], z["FF"], np.zeros((n, 15)))
    st = H.compare_implsch(fused_reference(z), got, Tables(cfg, np.float64))
    assert np.max(np.abs(f3[:n] - z["F3_dp"])) < 16 * np.finfo(np.float64).eps
    assert st["mij_flips"] == 0 and st["xllws_bins_diff"] == 0, st
    assert st["fl1_max_rel_peak_all"] < 1e-10 and st["ff_max_rel_all"] < 1e-10 and st["intf_max_rel_all"] < 1e-8, st


# ---- (b) the live reference against the fixtures ------------------------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("name", list(RC.CONFIGS))
def test_live_reference_reproduces_the_fixture(name):
    inp, ref = RC.load(name)
    got = RC.run(R.cached(RC.config(name), "dp"), inp, RC.kind(name))
    assert_dp(name, stats(name, ref["dp"], got, "dp"), dp_gate)


@needs_reference
@pytest.mark.parametrize("name", ["advection_12x25", "advection_split"])
def test_live_reference_reproduces_the_advection_fixture(name):
    z = np.load(RC.path(name))
    g = _advection_grid(z)
    cfg = RC.advection_config()
    r = R.cached(cfg, "dp")
    kw = dict(ifrelfmax=RC.ADV_IFRELFMAX, delpro_lf=cfg.idelpro / 2) if name == "advection_split" else {}
    w = r.ctu_weights_wam(g, z["cg"], cfg.idelpro, **kw)
    eps = np.finfo(np.float64).eps
    assert np.max(np.abs(RC.w8(Tables(cfg, np.float64), w) - z["W8_dp"])) < 8 * eps
    assert np.max(np.abs(r.propags2(g, z["f1"], w)[: g.nsea, :, : cfg.nfre_red] - z["F3_dp"])) < 16 * eps


# ---- (c) the live reference against the oracle on other sea states -------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", list(RC.CONFIGS))
def test_oracle_against_the_live_reference_on_a_second_seed(name, prec):
    """Sea states that are in no fixture (seed + 1000).  Double precision under the ceiling (the tighter figure is set on the fixtures' sea states);
    single precision under harness.assert_sp_gates, whose flip budget covers a point at which a discrete decision falls the other way."""
    n = RC.points(name)
    inp = RC.make_inputs(name, n, RC.CONFIGS[name]["seed"] + 1000)
    ref = RC.run(R.cached(RC.config(name), prec), inp, RC.kind(name))
    got = RC.run(oracle_for(name, prec), inp, RC.kind(name))
    st = stats(name, ref, got, prec)
    if prec == "dp":
        assert_dp(name, st, lambda _n, q: CEILING[q])
    else:
        assert_sp(name, st, n)


@needs_reference
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_tables_of_the_oracle_against_the_reference_initialisers(prec):
    """The tables the reference's own initialisers fill (MFREDIR, TABU_SWELLFT, INIT_X0TAUHF, INITGC, INISNONLIN + NLWEIGT, INIT_SDISS_ARDH,
    CIGETDEAC) against the oracle's restatement: integers identical, reals within 4 eps of the table's largest value."""
    cfg = RC.config("ice_ciwa1_3_scal")
    o, r = Oracle(cfg, prec), R.cached(cfg, prec)
    eps = np.finfo(H.np_dtype(prec)).eps
    for k in ("IKP", "IKP1", "IKM", "IKM1", "K1W", "K2W", "K11W", "K21W", "INLCOEF", "MFRSTLW", "MLSTHG", "KFRH", "NSDSNTH", "NWAV_GC"):
        assert np.array_equal(o.get(k), r.get(k)), k
    assert np.array_equal(o.get("INDICESSAT") + 1, r.get("INDICESSAT"))      # (the oracle keeps 0-based direction indices)
    for k in ("FR", "DFIM", "DFIMOFR", "DFIMFR", "DFIM_SIM", "RHOWG_DFIM", "ZPIFR", "FR5", "COFRM4", "FLMAX", "TH", "COSTH", "SINTH", "WTAUHF", "SWELLFT",
              "AF11", "RNLCOEF", "XK_GC", "XKM_GC", "OMEGA_GC", "OMXKM3_GC", "CM_GC", "C2OSQRTVG_GC", "XKMSQRTVGOC2_GC", "OM3GMKM_GC", "DELKCC_GC_NS",
              "DELKCC_OMXKM3_GC", "SATWEIGHTS", "DELTH", "X0TAUHF", "FLOGSPRDM1", "DAL1", "DAL2", "BETAMAXOXKAPPA2", "BMAXOKAP", "GAMNCONST",
              "TAUWSHELTER", "SQRTGOSURFT", "WSPMIN"):
        a, b = o.get(k), r.get(k)
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 4 * eps * np.abs(b).max(), (k, np.max(np.abs(a - b)) / max(np.abs(b).max(), 1e-300))
    # SDICE1's table: the reference's own tabulated block (CIGETDEAC) against the data file the oracle and the product read
    raw = np.loadtxt(os.path.join(os.path.dirname(R.__file__), "data", "cideac_kohout_meylan.txt"))
    cideac = r.get("CIDEAC").reshape(36, 16)      # CIDEAC(NICT, NICH): [IH][IT] in C order
    assert np.max(np.abs(cideac[:, 5:16] - raw)) <= 4 * eps * np.abs(raw).max()


# ---- NEWWIND and DEPTHPRPT ----------------------------------------------------------------------------------------------------------------
def _assert_newwind(got, want, ff, ffn, icode, prec):
    eps = np.finfo(H.np_dtype(prec)).eps
    got, want = got.astype(float), want.astype(float)
    assert np.array_equal(np.delete(got, 8, axis=1), np.delete(want, 8, axis=1))      # members are copies: identical
    assert np.max(np.abs(got[:, 8] - want[:, 8])) <= 4 * eps * np.abs(want[:, 8]).max()      # TAUW: a product of four factors
    # the fixture reaches both sides of the reset threshold of its forcing
    if icode == 3:
        capped = want[:, 8] < ff[:, 8]
        assert capped.any() and (~capped).any() and (ffn[:, 3] < 4.0).any() and (ffn[:, 3] >= 4.0).any()
        assert np.array_equal(want[:, 3], ffn[:, 3]) and np.array_equal(want[:, 7], ff[:, 7])
    else:
        assert (want[:, 8] == 0).any() and (want[:, 8] != 0).any() and np.array_equal(want[:, 7], ffn[:, 7]) and np.array_equal(want[:, 3], ff[:, 3])


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("icode", RC.NEWWIND_ICODES)
def test_oracle_newwind_against_the_reference_fixture(icode, prec):
    z = np.load(RC.path("newwind"))
    got = Oracle(RC.newwind_config(icode), prec).newwind(z["ff"], z["ffn"])
    _assert_newwind(got, z[f"out_icode{icode}_{prec}"], z["ff"].astype(float), z["ffn"].astype(float), icode, prec)


def _assert_depthprpt(got, want, prec, who):
    eps = np.finfo(H.np_dtype(prec)).eps
    for k in RC.DEPTHPRPT_KEYS:
        x, y = got[k].astype(float), want[k].astype(float)
        assert np.isfinite(y).all() and np.isfinite(x).all(), k
        err = float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))
        assert err <= (64 if k == "OMOSNH2KD" else 8) * eps, (who, k, err / eps)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_depth_props_against_the_reference_fixture(prec):
    """The oracle's DEPTHPRPT / AKI / EMAXDPT and the product's numpy tables (ecwam_amd/synthetic.py: what the device is fed with) against the
    reference's DEPTHPRPT + AKI on the fixture's depths."""
    from ecwam_amd import synthetic as syn

    z = np.load(RC.path("depthprpt"))
    want = {k: z[f"{k}_{prec}"] for k in RC.DEPTHPRPT_KEYS}
    assert (z["OMOSNH2KD_dp"] == 0).any() and (z["OMOSNH2KD_dp"] > 0).any()      # both branches of the deep-water switch
    cfg = RC.newwind_config(3)
    _assert_depthprpt(Oracle(cfg, prec).depthprpt(z["depth"]), want, prec, "oracle")
    _assert_depthprpt(syn.depth_props(z["depth"].astype(H.np_dtype(prec)), Tables(cfg, H.np_dtype(prec)), H.np_dtype(prec)), want, prec, "product tables")


@needs_reference
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_live_reference_newwind_and_depthprpt(prec):
    """The live reference against both fixtures and, on other inputs (seed + 1000), against the oracle."""
    z, zd = np.load(RC.path("newwind")), np.load(RC.path("depthprpt"))
    ff2, ffn2 = RC.newwind_inputs(seed=1001)
    for icode in RC.NEWWIND_ICODES:
        cfg = RC.newwind_config(icode)
        r = R.cached(cfg, prec)
        _assert_newwind(r.newwind(z["ff"], z["ffn"]), z[f"out_icode{icode}_{prec}"], z["ff"].astype(float), z["ffn"].astype(float), icode, prec)
        _assert_newwind(Oracle(cfg, prec).newwind(ff2, ffn2), r.newwind(ff2, ffn2), ff2.astype(float), ffn2.astype(float), icode, prec)
    cfg = RC.newwind_config(3)
    r = R.cached(cfg, prec)
    _assert_depthprpt(r.depthprpt(zd["depth"]), {k: zd[f"{k}_{prec}"] for k in RC.DEPTHPRPT_KEYS}, prec, "live reference")
    d2 = RC.depthprpt_depths(seed=1011)
    _assert_depthprpt(Oracle(cfg, prec).depthprpt(d2), r.depthprpt(d2), prec, "oracle, second seed")
