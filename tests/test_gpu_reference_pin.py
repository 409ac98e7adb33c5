"""The device kernels pinned to the reference's own Fortran (run with -m gpu).  Reads tests/golden/reference_*.npz only: what the reference's
unmodified IMPLSCH, WDFLUXES, NEWWIND, CTUWINI + CTUW and PROPAGS2 returned in both precisions (tools/make_golden_reference.py, tests/reference_cases.py);
no reference tree and no reference library is needed here.

Gates: exactly those of the device against the oracle.  Double precision: spectra and forcing 1e-10, fluxes 1e-8, MIJ and
XLLWS identical.  Single precision: harness.assert_sp_gates with the kind of the configuration's time step, and NO flipped discrete decision: the
fixtures hold no point at which the reference's own two precisions disagree on MIJ or XLLWS.  Where the existing parity test of a sea state
gates the spectrum and the wave height only (test_implsch_edge_cases, test_implsch_parity_isnonlin_1_2, test_implsch_parity_48_directions) so does
its fixture here (SP_WHAT).  Advection: the bounds of test_ctuw_and_propags2_parity (weights 8 eps, spectra 16 eps).
"""
import numpy as np
import pytest

import harness as H
import reference_cases as RC
from ecwam_amd import grid as G
from ecwam_amd.tables import Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SP_WHAT = {"edge": ("bins", "swh"), "isnonlin1": ("bins", "swh"), "isnonlin2": ("bins", "swh"), "A48x36": ("bins", "swh")}
IMPLSCH = [n for n in RC.CONFIGS if RC.kind(n) == "implsch"]


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


_FIX = {}


def fixture(name):
    """A fixture, loaded once and shared; the tests do not modify it."""
    if name not in _FIX:
        _FIX[name] = RC.load(name)
    return _FIX[name]


def assert_pinned(name, prec, ref, got, what=None):
    n = ref["FL1"].shape[0]
    st = H.compare_implsch(ref, got, Tables(RC.config(name), H.np_dtype(prec)))
    w2n = 0.0
    if "W2N" in ref:
        w2n = float(np.max(np.abs(got["W2N"] - ref["W2N"]) / np.maximum(np.abs(ref["W2N"]).max(axis=0, keepdims=True), 1e-12)))
    print(f"{name} {prec}: MIJ flips {st['mij_flips']}, XLLWS points {st['xllws_pts_diff']}, bins {st['fl1_max_rel_peak_all']:.2e}, swh {st['swh_max_rel']:.2e}, "
          f"forcing {st['ff_max_rel_all']:.2e}, fluxes {st['intf_max_rel_all']:.2e}, WAVE2OCEAN {w2n:.2e}")
    assert st["mij_flips"] == 0 and st["xllws_bins_diff"] == 0, st
    if prec == "dp":
        assert st["fl1_max_rel_peak_all"] < 1e-10 and st["swh_max_rel"] < 1e-10 and st["ff_max_rel_all"] < 1e-10, st
        assert st["intf_max_rel_all"] < 1e-8 and w2n < 1e-10, (st, w2n)
    else:
        H.assert_sp_gates(st, n, flip_budget=0.0, what=what or SP_WHAT.get(name, ("bins", "swh", "ff", "intf")))
        assert w2n < 2e-4      # the single precision bound of test_implsch_wam2nemo_outputs


@pytest.mark.parametrize("gen", [0, 2], ids=["k_implsch4", "k_implsch2"])
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", IMPLSCH)
def test_implsch_against_the_reference(api, name, prec, gen):
    """ecwam_hip_implsch (the product's kernel) and the tests' second implementation k_implsch2 on every fixture."""
    inp, ref = fixture(name)
    case = RC.harness_case(name, inp, prec)
    ctx = api.HipContext(case["tables"])
    ctx.set_implsch_generation(gen)
    got = H.gpu_implsch(case, ctx)
    assert ctx.implsch_generation_used() == (2 if gen == 2 else 4)
    ctx.close()
    assert np.isfinite(got["FL1"]).all() and np.isfinite(got["FF"]).all() and np.isfinite(got["INTF"]).all()
    assert_pinned(name, prec, ref[prec], got)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_wdfluxes_against_the_reference(api, prec):
    name = "wdfluxes_A36"
    inp, ref = fixture(name)
    case = RC.harness_case(name, inp, prec)
    n = case["n"]
    ctx = api.HipContext(case["tables"])
    assert ctx.wdfluxes_supported()
    dev = ctx.device
    wv, ff, intf = H.pack_device_inputs(case)
    fl1 = torch.from_numpy(case["FL1"].copy()).to(dev)
    twv, tff, tintf = (torch.from_numpy(a).to(dev) for a in (wv, ff, intf))
    mij = torch.zeros(n, dtype=torch.int32, device=dev)
    xllws = torch.zeros_like(fl1)
    ctx.wdfluxes(0, n, fl1, twv, tff, tintf, mij, xllws)
    torch.cuda.synchronize()
    got = dict(FL1=fl1.cpu().numpy(), XLLWS=xllws.cpu().numpy(), MIJ=mij.cpu().numpy(), FF=tff.cpu().numpy()[:, :14], INTF=tintf.cpu().numpy()[:, :15])
    ctx.close()
    assert np.array_equal(got["FL1"], case["FL1"])      # WDFLUXES leaves the spectrum alone
    assert_pinned(name, prec, ref[prec], got, what=("intf",))


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("icode", RC.NEWWIND_ICODES)
def test_newwind_against_the_reference(api, icode, prec):
    """ecwam_hip_newwind on the NEWWIND fixture (forcing on both sides of the two reset thresholds): every member but TAUW identical to the
    reference's, TAUW within the bounds the device has against the oracle (test_newwind_and_layout: 4 eps of itself at ICODE 3;
    test_implsch_parity_friction_velocity_forcing: 8 eps of the largest at ICODE 1 / 2)."""
    z = np.load(RC.path("newwind"))
    T = H.np_dtype(prec)
    want = z[f"out_icode{icode}_{prec}"]
    n = want.shape[0]
    ff, ffn = np.zeros((n, 16), T), np.zeros((n, 16), T)
    ff[:, :14], ffn[:, :14] = z["ff"], z["ffn"]
    ff[:, 14:] = 5.0
    ctx = api.HipContext(Tables(RC.newwind_config(icode), T))
    tff = torch.from_numpy(ff.copy()).to(ctx.device)
    ctx.newwind(tff, torch.from_numpy(ffn).to(ctx.device))
    torch.cuda.synchronize()
    got = tff.cpu().numpy()
    ctx.close()
    eps = np.finfo(T).eps
    assert np.array_equal(np.delete(got[:, :14], 8, axis=1), np.delete(want, 8, axis=1)) and np.array_equal(got[:, 14:], ff[:, 14:])
    d = np.abs(got[:, 8].astype(float) - want[:, 8].astype(float))
    print(f"newwind icode {icode} {prec}: TAUW {d.max() / eps:.2f} eps absolute")
    if icode == 3:
        assert np.max(d / np.abs(want[:, 8])) < 4 * eps
    else:
        assert d.max() < 8 * eps * np.abs(want[:, 8]).max() and (want[:, 8] == 0).any() and (want[:, 8] != 0).any()


def _grid(z):
    g = G.build_grid(int(z["n_oct"]), mask="continents")
    assert g.nsea == int(z["nsea"]) and np.array_equal(g.klon, z["klon"]) and np.array_equal(g.klat, z["klat"]) and np.array_equal(g.kcor, z["kcor"])
    return g


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", ["advection_12x25", "advection_split"])
def test_advection_against_the_reference(api, name, prec):
    """build_weights() + propag() on the advection fixture: the stored weights against the reference's CTUW (8 eps: O(1) fractions), one PROPAGS2
    with them and with the on-the-fly weights against the reference's F3 (16 eps); with the fast-wave split the weights carry both time steps."""
    from ecwam_amd.wamintgr import Wamintgr

    z = np.load(RC.path(name))
    g = _grid(z)
    cfg = RC.advection_config()
    T = H.np_dtype(prec)
    eps = np.finfo(T).eps
    n, nr = g.nsea, cfg.nfre_red
    kw = dict(ifrelfmax=RC.ADV_IFRELFMAX, delpro_lf=cfg.idelpro / 2) if name == "advection_split" else {}
    want_w, want_f3 = z[f"W8_{prec}"].astype(float), z[f"F3_{prec}"].astype(float)
    m = Wamintgr(cfg, g, prec, weights="stored", **kw)
    assert m.nrows == n + 1
    m.cgroup_ext = torch.from_numpy(z["cg"].astype(T)).to(m.dev)
    m.fl1.copy_(torch.from_numpy(z["f1"].astype(T)))
    assert m.build_weights() == 0
    w = m.w.cpu().numpy().reshape(n, 8, cfg.nang, nr).astype(float)
    dw = float(np.max(np.abs(w - want_w)))
    assert np.array_equal(m.gd["wlat"].cpu().numpy(), z[f"WLAT_{prec}"]) and np.array_equal(m.gd["wcor"].cpu().numpy(), z[f"WCOR_{prec}"])
    tf3 = torch.full_like(m.fl1, -7.0)
    m.ctx.propags2(m.fl1, tf3, m.gd["klon"], m.gd["klat"], m.gd["kcor"], m.w, 0, n, check_indices=True)
    torch.cuda.synchronize()
    f3 = tf3.cpu().numpy()
    df = float(np.max(np.abs(f3[:n, :, :nr].astype(float) - want_f3)))
    print(f"{name} {prec}: stored weights {dw / eps:.2f} eps, F3 {df / eps:.2f} eps")
    assert dw < 8 * eps and df < 16 * eps
    assert np.array_equal(f3[:n, :, nr:], z["f1"][:n, :, nr:].astype(T)) and np.all(f3[n] == -7.0)
    m.ctx.close()
    if name == "advection_12x25":      # the product's default: propag() with on-the-fly weights
        m = Wamintgr(cfg, g, prec)
        m.cgroup_ext = torch.from_numpy(z["cg"].astype(T)).to(m.dev)
        m.fl1.copy_(torch.from_numpy(z["f1"].astype(T)))
        assert m.build_weights() == 0
        m.propag()
        torch.cuda.synchronize()
        got = m.fl1.cpu().numpy()
        do = float(np.max(np.abs(got[:n, :, :nr].astype(float) - want_f3)))
        print(f"{name} {prec}: propag() with on-the-fly weights, F3 {do / eps:.2f} eps")
        assert do < 16 * eps
        m.ctx.close()


def test_one_kernel_step_against_the_reference(api):
    """step(fused=True) at 36 x 36 in double precision (the one-kernel step's dp build exists at 36 directions only) against the reference's
    PROPAGS2 followed by the reference's IMPLSCH on the same state."""
    from ecwam_amd.wamintgr import Wamintgr

    z = np.load(RC.path("fused_36_dp"))
    g = _grid(z)
    cfg = RC.fused_config()
    n = g.nsea
    m = Wamintgr(cfg, g, "dp")
    m.cgroup_ext = torch.from_numpy(z["cg"].astype(np.float64)).to(m.dev)
    m.fl1.copy_(torch.from_numpy(z["f1"].astype(np.float64)))
    m.wvprpt.copy_(torch.from_numpy(z["WV"].astype(np.float64)))
    ff = np.zeros((n, 16))
    ff[:, :14], ff[:, 14:16] = z["FF"], z["ENV"]
    m.ff.copy_(torch.from_numpy(ff))
    assert m.build_weights() == 0 and m.fused_available()
    m.step(fused=True)
    torch.cuda.synchronize()
    got = dict(FL1=m.fl1.cpu().numpy()[:n], XLLWS=m.xllws.cpu().numpy(), MIJ=m.mij.cpu().numpy(), FF=m.ff.cpu().numpy()[:, :14],
               INTF=m.intf.cpu().numpy()[:, :15])
    m.ctx.close()
    ref = dict(FL1=z["FL1_dp"], MIJ=z["MIJ"], XLLWS=z["XLLWS"].astype(np.float64), FF=z["FF_dp"], INTF=z["INTF_dp"])
    st = H.compare_implsch(ref, got, Tables(cfg, np.float64))
    print(f"one-kernel step dp: bins {st['fl1_max_rel_peak_all']:.2e}, forcing {st['ff_max_rel_all']:.2e}, fluxes {st['intf_max_rel_all']:.2e}")
    assert st["mij_flips"] == 0 and st["xllws_bins_diff"] == 0, st
    assert st["fl1_max_rel_peak_all"] < 1e-10 and st["ff_max_rel_all"] < 1e-10 and st["intf_max_rel_all"] < 1e-8, st
