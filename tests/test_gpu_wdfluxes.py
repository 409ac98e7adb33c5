"""ecwam_hip_wdfluxes / ecwam_hip_setice / Wamintgr.outstep0 on the device (run with -m gpu) against the CPU reference of tests/wdfluxes_ref.py.

403 = 13 x 31 "mixed" points per case: no multiple of any number of points per wavefront (2, 3, 4, 5, 10), so every case ends in a short wave.

Gates.  Double precision: MIJ and XLLWS identical, the flux groups of harness.compare_implsch within 1e-10 (the project's dp gate), WSEMEAN / WSFMEAN
within 1e-12 of themselves.  Single precision: the flux groups under harness.SP_GATES["long"] (1e-3, cap 5e-2) -- NOT the "short" gate of 2e-4: the
CPU reference's own two precisions differ by 8.7e-5 ... 2.8e-4 in these groups on these very inputs, so 2e-4 is below what single precision can
deliver here; MIJ / XLLWS may differ at max(1, int(0.005 n)) = 2 points (the reference's own precisions differ at no more than 1 of 403 in every
case); WSEMEAN / WSFMEAN on the points with identical XLLWS within WS_GATE_SP.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import harness as H
import wdfluxes_ref as W
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 403
B = dict(llgcbz0=True, llnormagam=True)
CASES = {
    "A-12x25": dict(nang=12, nfre_red=25), "A-24x29": dict(nang=24, nfre_red=29), "A-36x36": dict(nang=36, nfre_red=36), "A-48x36": dict(nang=48, nfre_red=36),
    "B-36x36": dict(nang=36, nfre_red=36, **B), "B-12x25": dict(nang=12, nfre_red=25, **B),
    "ice-24x29": dict(nang=24, nfre_red=29, lciwa3=True, lciscal=True, lwflux=True),
    "iphys0-36x36": dict(nang=36, nfre_red=36, iphys=0), "isnonlin1-24x29": dict(nang=24, nfre_red=29, isnonlin=1),
    "nemocou-24x29": dict(nang=24, nfre_red=29, lwnemocou=True),
    # Double precision at 24 directions is refused (see the parity test): the three switches of the 24-direction cases again at direction counts
    # that ship in both precisions, so that every selector (flag sets A and B, IPHYS 0, ISNONLIN 1), the ice rates, LWFLUX's WSEMEAN / WSFMEAN
    # and the WAVE2OCEAN columns are compared with the reference in double precision too
    "ice-12x25": dict(nang=12, nfre_red=25, lciwa3=True, lciscal=True, lwflux=True), "ice-36x36": dict(nang=36, nfre_red=36, lciwa3=True, lciscal=True, lwflux=True),
    "isnonlin1-36x36": dict(nang=36, nfre_red=36, isnonlin=1), "isnonlin1-12x25": dict(nang=12, nfre_red=25, isnonlin=1),
    "nemocou-36x36": dict(nang=36, nfre_red=36, lwnemocou=True),
}
# WSEMEAN / WSFMEAN in single precision, relative, over the points whose XLLWS equals the reference's: ten times the maximum observed on the
# device (5.80e-7, the LWFLUX case ice-36x36; 5.76e-7 at 24, 5.08e-7 at 12 directions: profiles/wdfluxes_gates.txt); the ceiling of 4e-5 = ten times the 4.0e-6 by which the reference's
# two precisions differ is not reached.  Observed on the same run: flux groups 8.3e-5 ... 2.1e-4 in single precision (every point), 7.7e-14 ...
# 2.1e-13 in double; MIJ identical everywhere, XLLWS at one point of 403 in the 24-direction single precision cases.
WS_GATE_SP = min(10 * 5.80e-7, 4e-5)
SENT = -777.25


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _cfg(**kw):
    return Config(nfre=36, **kw)


_CASES = {}


def _case(cfg_kw: dict, prec: str, n: int = N):
    """The inputs of a case and the CPU reference's WDFLUXES of them: computed once, shared, never modified."""
    key = (tuple(sorted(cfg_kw.items())), prec, n)
    if key not in _CASES:
        cfg = _cfg(**cfg_kw)
        case = H.make_point_case(n, cfg, prec, spectra="mixed")
        if cfg.lwnemocou:
            case["W2N"] = np.full((n, 13), SENT, np.float64)
        _CASES[key] = (case, W.reference(case, W.WdfluxesOracle(cfg, prec)))
    return _CASES[key]


class Dev:
    """The device arrays of a case; intf (but for the input slot 15), mij, xllws and wam2nemo start as sentinels."""

    def __init__(self, case, ctx):
        dev = ctx.device
        wv, ff, intf = H.pack_device_inputs(case)
        intf[:, :15] = SENT
        self.n = case["n"]
        self.host = dict(FL1=np.ascontiguousarray(case["FL1"]), FF=ff, INTF=intf)
        self.fl1 = torch.from_numpy(case["FL1"].copy()).to(dev)
        self.wv, self.ff, self.intf = (torch.from_numpy(a.copy()).to(dev) for a in (wv, ff, intf))
        self.mij = torch.full((self.n,), -7, dtype=torch.int32, device=dev)
        self.xllws = torch.full_like(self.fl1, SENT)
        self.w2n = torch.full((self.n, 13), SENT, dtype=torch.float64, device=dev) if case["cfg"].lwnemocou else None

    def wdfluxes(self, ctx, kijs=0, kijl=None):
        ctx.wdfluxes(kijs, self.n if kijl is None else kijl, self.fl1, self.wv, self.ff, self.intf, self.mij, self.xllws, wam2nemo=self.w2n)
        torch.cuda.synchronize()
        return self

    def implsch(self, ctx):
        ctx.implsch(0, self.n, self.fl1, self.wv, self.ff, self.intf, self.mij, self.xllws, wam2nemo=self.w2n)
        torch.cuda.synchronize()
        return self

    def out(self):
        o = dict(FL1=self.fl1.cpu().numpy(), XLLWS=self.xllws.cpu().numpy(), MIJ=self.mij.cpu().numpy(), FF=self.ff.cpu().numpy()[:, :14],
                 INTF=self.intf.cpu().numpy()[:, :15], FF16=self.ff.cpu().numpy(), INTF16=self.intf.cpu().numpy())
        if self.w2n is not None:
            o["W2N"] = self.w2n.cpu().numpy()
        return o


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _log(**kw):
    path = os.environ.get("ECWAM_TEST_STATS_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", ""), **kw)) + "\n")


# ---- 1. parity with the CPU reference
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_cpu_reference(api, name, prec):
    case, ref = _case(CASES[name], prec)
    cfg = case["cfg"]
    ctx = api.HipContext(case["tables"])
    if prec == "dp" and cfg.nang == 24:
        # Not shipped: this build returned a wrong PHIWA (PHIAW of the wrong sign at 303 of 403 points, flux groups off by 3.7) and a Stokes drift off
        # by 4e-5 on the device, with MIJ, XLLWS and the stresses right to 1e-14; the same source passes every other case here.  The library
        # refuses the configuration, and says why.
        assert not ctx.wdfluxes_supported()
        with pytest.raises(api.EcwamHipError, match="^ecwam_hip_wdfluxes: not covered: 24 directions in double precision$"):
            Dev(case, ctx).wdfluxes(ctx, 0, 0)
        ctx.close()
        return
    assert ctx.wdfluxes_supported()
    d = Dev(case, ctx).wdfluxes(ctx)
    got = d.out()
    ctx.close()
    # inputs: not a bit of them changed
    assert _same_bits(got["FL1"], d.host["FL1"]) and _same_bits(got["FF16"], d.host["FF"])
    assert np.isfinite(got["INTF"][:, H.INTF_OUT]).all() and (got["MIJ"] >= 1).all() and (got["MIJ"] <= 36).all()
    st = H.compare_implsch(ref, got, case["tables"])      # (FL1 and FF are the inputs on both sides: their statistics are zero)
    same = (ref["XLLWS"] == got["XLLWS"]).all(axis=(1, 2))
    ws = 0.0
    if cfg.lwflux:
        ws = float(H.rel_err(got["INTF"][same][:, 0:2], ref["INTF"][same][:, 0:2], 1e-300).max())
    print(f"wdfluxes {name} {prec}: MIJ flips {st['mij_flips']}, XLLWS points {st['xllws_pts_diff']}, flux groups all but 0.2 % {st['intf_rob_rel']:.2e} "
          f"every point {st['intf_max_rel_all']:.2e} ({st['intf_worst_group']}), WSEMEAN / WSFMEAN {ws:.2e}")
    _log(case=name, prec=prec, wsemean_rel=ws, mij_flips=st["mij_flips"], xllws_pts_diff=st["xllws_pts_diff"], intf_rob_rel=st["intf_rob_rel"],
         intf_max_rel_all=st["intf_max_rel_all"])
    if prec == "dp":
        assert st["mij_flips"] == 0 and st["xllws_bins_diff"] == 0, st
        assert st["intf_max_rel_all"] <= 1e-10, st
        assert ws <= 1e-12, ws
    else:
        H.assert_sp_gates(st, N, what=("intf",), kind="long")
        assert ws <= WS_GATE_SP, ws
    if cfg.lwnemocou:      # STOKESTRN's copies; LNUPD = F: nothing else of WAVE2OCEAN
        w = got["W2N"]
        assert (w[:, 2:] == SENT).all()
        assert _same_bits(w[:, 0], got["INTF"][:, 2].astype(np.float64)) and _same_bits(w[:, 1], got["INTF"][:, 3].astype(np.float64))
    # what the call does not compute stays: STRNMS and the input slot; WSEMEAN / WSFMEAN without LWFLUX
    assert (got["INTF16"][:, 4] == SENT).all() and _same_bits(got["INTF16"][:, 15], d.host["INTF"][:, 15])
    assert (got["INTF16"][:, 10:12] == 0).all()      # TAUICX, TAUICY (LWNEMOCOUWRS = F)
    if not cfg.lwflux:
        assert (got["INTF16"][:, 0:2] == SENT).all()


# ---- 2., 3. nothing else is written; absolute row ranges
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_ranges_and_sentinel_rows(api, prec):
    case, _ = _case(dict(nang=12, nfre_red=25, lwnemocou=True), prec)
    ctx = api.HipContext(case["tables"])
    one = Dev(case, ctx).wdfluxes(ctx, 3, N - 2).out()
    two = Dev(case, ctx).wdfluxes(ctx, 3, 200).wdfluxes(ctx, 200, N - 2).out()
    whole = Dev(case, ctx).wdfluxes(ctx, 3, N).out()
    parts = Dev(case, ctx).wdfluxes(ctx, 200, N).wdfluxes(ctx, 3, 200).out()
    ctx.close()
    for k in ("FL1", "FF16", "INTF16", "MIJ", "XLLWS", "W2N"):
        assert _same_bits(one[k], two[k]) and _same_bits(whole[k], parts[k]), k
    for o, rows in ((one, [0, 1, 2, N - 2, N - 1]), (whole, [0, 1, 2])):
        assert (o["INTF16"][rows, :15] == SENT).all() and (o["MIJ"][rows] == -7).all() and (o["XLLWS"][rows] == SENT).all() and (o["W2N"][rows] == SENT).all()
    assert (one["MIJ"][3:N - 2] >= 1).all() and (one["XLLWS"][3:N - 2] != SENT).all() and (one["INTF16"][3:N - 2, 2] != SENT).all()
    assert _same_bits(one["INTF16"][3:N - 2], whole["INTF16"][3:N - 2])      # a point's result does not depend on the wave it shares


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_without_lcflx_only_mij_and_xllws_are_written(api, prec):
    """LWFLUX = LWFLUXOUT = F with LWNEMOCOU = T: IMPLSCH's LCFLX is set, WDFLUXES' own is not (wdfluxes.F90:156)."""
    kw = dict(nang=12, nfre_red=25, lwflux=False, lwfluxout=False, lwnemocou=True)
    case, ref = _case(kw, prec)
    ctx = api.HipContext(case["tables"])
    d = Dev(case, ctx).wdfluxes(ctx)
    got = d.out()
    ctx.close()
    assert _same_bits(got["INTF16"], d.host["INTF"]) and (got["W2N"] == SENT).all()
    assert _same_bits(got["FL1"], d.host["FL1"]) and _same_bits(got["FF16"], d.host["FF"])
    flips, pts = int((got["MIJ"] != ref["MIJ"]).sum()), int((got["XLLWS"] != ref["XLLWS"]).any(axis=(1, 2)).sum())
    assert flips <= (0 if prec == "dp" else 2) and pts <= (0 if prec == "dp" else 2), (flips, pts)
    assert _same_bits(ref["INTF"], case["INTF"]) and (ref["W2N"] == SENT).all()      # (the reference agrees: nothing but MIJ and XLLWS)


# ---- 4. the context is undisturbed
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_implsch_after_wdfluxes_equals_implsch_on_a_fresh_context(api, prec):
    case, _ = _case(CASES["A-12x25"], prec)
    ctx = api.HipContext(case["tables"])
    Dev(case, ctx).wdfluxes(ctx)
    after = Dev(case, ctx).implsch(ctx).out()
    ctx.close()
    ctx = api.HipContext(case["tables"])
    fresh = Dev(case, ctx).implsch(ctx).out()
    ctx.close()
    for k in ("FL1", "FF16", "INTF16", "MIJ", "XLLWS"):
        assert _same_bits(after[k], fresh[k]), k
    assert not _same_bits(after["FL1"], case["FL1"])      # (IMPLSCH did advance the spectrum)


# ---- 5. known answers, without the oracle
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_known_answers_on_the_device(api, prec):
    """The two numpy restatements of tests/test_wdfluxes_host.py on the device's output: the tolerance they meet on the reference (1e-12 / 2e-5) plus
    the flux gate (1e-10 / 1e-3)."""
    case, _ = _case(dict(nang=12, nfre_red=25, lwflux=True), prec)
    t = case["tables"]
    ctx = api.HipContext(t)
    got = Dev(case, ctx).wdfluxes(ctx).out()
    ctx.close()
    tol = 1e-12 + 1e-10 if prec == "dp" else 2e-5 + 1e-3
    free = ~(case["FF"][:, 2] > t.CITHRSH)
    us, vs = W.stokes_known(t, case["FL1"], case["props"]["STOKFAC"], case["FF"])
    scale = np.maximum(np.hypot(us, vs), 1e-6)
    e_st = max(float((np.abs(got["INTF"][:, 2] - us) / scale)[free].max()), float((np.abs(got["INTF"][:, 3] - vs) / scale)[free].max()))
    em, fm = W.wsemean_known(t, case["FL1"], got["XLLWS"])
    e_ws = max(float((np.abs(got["INTF"][:, 0] - em) / em).max()), float((np.abs(got["INTF"][:, 1] - fm) / fm).max()))
    print(f"known answers {prec}: Stokes drift {e_st:.2e}, WSEMEAN / WSFMEAN {e_ws:.2e}")
    _log(case="known-answers", prec=prec, stokes_rel=e_st, wsemean_known_rel=e_ws)
    assert e_st < tol and e_ws < tol, (e_st, e_ws)


# ---- 6. SETICE
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_setice(api, prec):
    n = 64
    cfg = _cfg(nang=12, nfre_red=25)
    case = H.make_point_case(n, cfg, prec, spectra="mixed")
    t = case["tables"]
    wv, ff, _ = H.pack_device_inputs(case)
    ff[:, 2] = np.where(np.arange(n) % 3 == 0, 0.0, np.linspace(0.05, 0.995, n)).astype(ff.dtype)      # both sides of CITHRSH
    ff[5, 2] = t.CITHRSH                                                                              # exactly at it: the spectrum stays
    ice = ff[:, 2] > ff.dtype.type(t.CITHRSH)
    assert ice.sum() > 10 and (~ice).sum() > 10 and not ice[5]
    ref = W.WdfluxesOracle(cfg, prec).setice(case["FL1"], ff[:, :14])
    ctx = api.HipContext(t)
    fl1 = torch.from_numpy(case["FL1"].copy()).to(ctx.device)
    tff = torch.from_numpy(ff).to(ctx.device)
    ctx.setice(3, n - 2, fl1, tff)
    torch.cuda.synchronize()
    got = fl1.cpu().numpy()
    ctx.close()
    keep = ~ice
    keep[:3] = True
    keep[n - 2:] = True      # outside the range: untouched whatever the ice
    assert _same_bits(got[keep], case["FL1"][keep])
    rows = np.flatnonzero(~keep)
    assert rows.size > 10
    d = np.abs(got[rows].astype(np.float64) - ref[rows].astype(np.float64))
    if prec == "dp":
        err = float((d / np.maximum(np.abs(ref[rows].astype(np.float64)), 1e-300)).max())
        print(f"setice dp: {err:.2e} relative")
        assert err <= 1e-15, err
    else:
        err = float(d.max() / (np.finfo(np.float32).eps * float(t.FLMIN)))
        print(f"setice sp: {err:.2f} eps of FLMIN")
        assert err <= 4.0, err
    _log(case="setice", prec=prec, setice_err=err)


# ---- 7. Wamintgr.outstep0
def test_outstep0_of_the_driver(api):
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import Wamintgr

    cfg = _cfg(nang=12, nfre_red=25, lwflux=True)
    assert cfg.licerun and cfg.lmaskice
    req = [ir for ir in (p[0] for p in api.OUTBLOCK_PARAMS) if not (17 <= ir <= 19 or 58 <= ir <= 61 or ir in (37, 38))]

    def model():
        m = Wamintgr(cfg, G.build_grid(16, mask="continents"), "sp")
        m.init_synthetic(seed=3)
        return m

    m = model()
    fl0 = m.fl1.clone()
    m.gfast_valid = True
    bout, cols = m.outstep0(req)
    assert m.gfast_valid is False      # SETICE wrote FL1
    h = model()
    h.wdfluxes()
    h.ctx.setice(0, h.n, h.fl1, h.ff)
    bout_h, cols_h = h.outblock(req)
    torch.cuda.synchronize()
    assert cols == cols_h and _same_bits(bout.cpu().numpy(), bout_h.cpu().numpy())
    ice = (m.ff[: m.n, 2] > float(m.t.CITHRSH)).cpu().numpy()
    same = (m.fl1[: m.n] == fl0[: m.n]).all(dim=2).all(dim=1).cpu().numpy()
    assert ice.any() and (~ice).any() and (same == ~ice).all()      # SETICE ran on the spectrum, and only under ice
    assert (m.mij[: m.n] >= 1).all() and bool((m.xllws[: m.n] != 0).any()) and bool((m.intf[: m.n, 12] != 0).any())
    # LLSOURCE = F: MIJ = NFRE, XLLWS = 0, no SETICE, no request -> None
    g = model()
    fl0 = g.fl1.clone()
    g.gfast_valid = True
    assert g.outstep0(llsource=False) is None and g.gfast_valid is True
    assert bool((g.mij[: g.n] == 36).all()) and bool((g.xllws[: g.n] == 0).all()) and bool((g.fl1 == fl0).all())


# ---- 8. refusals, with their words
class Raw:
    """A context through ctypes (ecwam_amd.api validates before the library does) and one small device buffer for every pointer."""

    def __init__(self, prec, **kw):
        from ecwam_amd import lib as L

        self.lib = L.load()
        t = Tables(_cfg(nang=12, nfre_red=36, **kw), H.np_dtype(prec))
        params = L.make_params(t)
        tp, keep = L.make_tables(t)
        self.h = C.c_void_p()
        rc = self.lib.ecwam_hip_create(C.byref(params), C.byref(tp), 4 if prec == "sp" else 8, 0, C.byref(self.h))
        assert rc == 0, self.lib.ecwam_hip_last_error().decode()
        self.buf = torch.zeros(8 * 12 * 36, dtype=torch.float64, device="cuda:0")
        self.a = self.buf.data_ptr()

    def wdfluxes(self, kijs=0, kijl=0, null_ctx=False, **over):
        p = dict(fl1=self.a, wvprpt=self.a, ff=self.a, intf=self.a, mij=self.a, xllws=self.a, wam2nemo=None)
        p.update(over)
        rc = self.lib.ecwam_hip_wdfluxes(None if null_ctx else self.h, kijs, kijl, p["fl1"], p["wvprpt"], p["ff"], p["intf"], p["mij"], p["xllws"],
                                         p["wam2nemo"], None)
        return rc, self.lib.ecwam_hip_last_error().decode()

    def setice(self, kijs=0, kijl=0, null_ctx=False, **over):
        p = dict(fl1=self.a, ff=self.a)
        p.update(over)
        rc = self.lib.ecwam_hip_setice(None if null_ctx else self.h, kijs, kijl, p["fl1"], p["ff"], None)
        return rc, self.lib.ecwam_hip_last_error().decode()

    def close(self):
        self.lib.ecwam_hip_destroy(self.h)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_refusals(api, prec):
    """Every case is refused before anything is launched; the ranges are empty wherever the refusal itself needs no points."""
    c = Raw(prec)
    try:
        assert c.lib.ecwam_hip_wdfluxes_supported(c.h) == 1
        assert c.wdfluxes()[0] == 0      # the well-formed empty call
        assert c.wdfluxes(null_ctx=True) == (1, "null context") and c.setice(null_ctx=True) == (1, "null context")
        assert c.lib.ecwam_hip_wdfluxes_supported(None) == 0
        assert c.wdfluxes(kijs=1, kijl=0) == (1, "ecwam_hip_wdfluxes: bad range") and c.wdfluxes(kijs=-1) == (1, "ecwam_hip_wdfluxes: bad range")
        assert c.wdfluxes(kijs=1, kijl=0, fl1=None) == (1, "ecwam_hip_wdfluxes: bad range")      # the range comes first
        for k in ("fl1", "wvprpt", "ff", "intf", "mij", "xllws"):
            assert c.wdfluxes(kijl=8, **{k: None}) == (1, "ecwam_hip_wdfluxes: null pointer"), k
        assert c.setice(kijs=1, kijl=0) == (1, "ecwam_hip_setice: bad range") and c.setice(kijs=-1) == (1, "ecwam_hip_setice: bad range")
        assert c.setice(kijl=8, ff=None) == (1, "ecwam_hip_setice: null pointer") and c.setice(kijl=8, fl1=None) == (1, "ecwam_hip_setice: null pointer")
        assert c.setice(fl1=c.a + 8) == (1, "ecwam_hip_setice: the spectra must be 16-byte aligned")
    finally:
        c.close()
    c = Raw(prec, lwnemocou=True)
    try:
        assert c.wdfluxes(kijl=8) == (1, "ecwam_hip_wdfluxes: LWNEMOCOU needs the WAVE2OCEAN buffer")
        assert c.wdfluxes(kijl=8, xllws=None) == (1, "ecwam_hip_wdfluxes: null pointer")      # ... after the null pointers
        assert c.wdfluxes()[0] == 0      # an empty range needs no buffer
    finally:
        c.close()
    c = Raw(prec, lciwa2=True)      # a RARE configuration
    try:
        assert c.lib.ecwam_hip_wdfluxes_supported(c.h) == 0
        assert c.lib.ecwam_hip_last_error().decode() == "ecwam_hip_wdfluxes: not covered: LCIWA2"
        assert c.wdfluxes() == (1, "ecwam_hip_wdfluxes: not covered: LCIWA2")
        assert c.wdfluxes(kijs=1, kijl=0) == (1, "ecwam_hip_wdfluxes: bad range")
    finally:
        c.close()
