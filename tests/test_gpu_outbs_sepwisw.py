"""Wind sea / swell separation and the mean-period / spread parameters of OUTBLOCK on the device (ecwam_hip_outbs_sepwisw) against the
numpy restatement tests/sepwisw_ref.py on the same FL1 / XLLWS / CINV / FF.

Gates.  Heights and periods relative, directions cyclic in degrees, spreads absolute (SP_GATES / DP_GATES: at most 10 x the observed
maxima, which each test prints); in double precision also 1e-12 relative on every column (directions where the part carries energy).  A bin's wind-sea mask is a comparison of CHECKTA with 1
(sepwisw.F90:166-173, 197-205) and COSWDIF differs by an ulp between the device's COS and numpy's: points where the restatement finds a
CHECKTA within 4 ulp of 1 are counted (at most 0.5 % of the points) and left out of the value gates.  A part's direction is compared where
that part carries energy (its height above 1e-3 m): the direction of a part at the EPSMIN floor is the direction of rounding noise.
"""
import numpy as np
import pytest

import harness as H
import sepwisw_ref as S
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COL = {f: i for i, f in enumerate(S.FIELDS)}
HEIGHTS_PERIODS = ("mp1", "mp2", "shww", "shts", "mpww", "mpts", "p1sea", "p1swell", "p2sea", "p2swell")
DIRECTIONS = (("mdww", "shww"), ("mdts", "shts"))
SPREADS = ("wdw", "sprdsea", "sprdswell")
# observed maxima over every test of this file (36 x 36 and 24 x 36 after IMPLSCH, 12 x 25, CLDOMAIN 's', O48 after four steps):
#   sp: heights / periods 8.7e-7 relative, directions 6.1e-5 degrees, spreads 5.5e-6
#   dp: heights / periods 1.5e-15 relative, directions 2.3e-13 degrees, spreads 1.5e-14
SP_GATES = dict(rel=2e-6, deg=5e-4, spread=5e-5)
DP_GATES = dict(rel=1.4e-14, deg=2e-12, spread=1.4e-13)


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _device(ctx, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) for a in arrays]


def _run(api, ctx, fl1, xllws, wv, ff, kijs=0, kijl=None, small_domain=False, fill=-1.0):
    n = fl1.shape[0]
    kijl = n if kijl is None else kijl
    tfl, txl, twv, tff = _device(ctx, fl1, xllws, wv, ff)
    out = torch.full((n, len(S.FIELDS)), fill, dtype=ctx.dtype, device=ctx.device)
    ctx.outbs_sepwisw(kijs, kijl, tfl, txl, twv, tff, out, small_domain=small_domain)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _compare(got, ref, near, prec, what):
    """Observed maxima per gate class over the points without a CHECKTA near 1; asserts the gates and returns the figures."""
    ok = ~near
    assert near.mean() <= 0.005, (what, int(near.sum()))
    g, r = got[ok].astype(np.float64), ref[ok].astype(np.float64)
    obs = {}
    obs["rel"] = max(float(np.max(H.rel_err(g[:, COL[c]], r[:, COL[c]], 1e-3))) for c in HEIGHTS_PERIODS)
    dd = []
    for c, h in DIRECTIONS:
        live = r[:, COL[h]] > 1e-3
        d = np.abs(g[live, COL[c]] - r[live, COL[c]]) % 360.0
        dd.append(float(np.max(np.minimum(d, 360.0 - d))) if live.any() else 0.0)
    obs["deg"] = max(dd)
    obs["spread"] = max(float(np.max(np.abs(g[:, COL[c]] - r[:, COL[c]]))) for c in SPREADS)
    print(f"{what} {prec}: points {len(near)}, CHECKTA near 1 at {int(near.sum())}; observed maxima", {k: f"{v:.2e}" for k, v in obs.items()})
    if prec == "dp":
        live = {c: r[:, COL[h]] > 1e-3 for c, h in DIRECTIONS}
        for c, name in enumerate(S.FIELDS):
            sel = live.get(name, np.ones(len(r), bool))
            e = float(np.max(H.rel_err(g[sel, c], r[sel, c], 1e-300), initial=0.0))
            assert e < 1e-12, (what, name, e)
    for k, gate in (DP_GATES if prec == "dp" else SP_GATES).items():
        assert obs[k] < gate, (what, k, obs[k], gate)
    return obs


def _implsch_case(api, cfg, prec, n, seed):
    """XLLWS, FF (UFRIC) and FL1 from IMPLSCH on the device; CINV of the case."""
    case = H.make_point_case(n, cfg, prec, spectra="mixed", seed=seed)
    ctx = api.HipContext(case["tables"])
    r = H.gpu_implsch(case, ctx)
    wv, ff, _ = H.pack_device_inputs(case)
    ff[:, :14] = r["FF"]
    return ctx, case["tables"], r["FL1"], r["XLLWS"], wv, ff


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("nang", [36, 24])
def test_parity_after_implsch(api, prec, nang):
    cfg = Config(nang=nang, nfre=36, nfre_red=36)
    n = 3001
    ctx, t, fl1, xl, wv, ff = _implsch_case(api, cfg, prec, n, seed=17)
    assert 0 < xl.mean() < 1                                           # both wind sea and swell bins
    got = _run(api, ctx, fl1, xl, wv, ff, kijs=7, kijl=n - 3)
    assert np.all(got[:7] == -1.0) and np.all(got[n - 3:] == -1.0)      # rows outside [kijs, kijl) untouched
    ref, info = S.sepwisw(t, fl1, xl, wv[:, 2], ff[:, 7], ff[:, 1])
    _compare(got[7:n - 3], ref[7:n - 3], info["near"][7:n - 3], prec, f"after IMPLSCH {nang}x36")
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_parity_odd_nfre(api, prec):
    """NFRE odd: NFRE_ODD = NFRE (the 36-frequency grids run NFRE_ODD = NFRE - 1).  IMPLSCH covers 36 frequencies only, so XLLWS is the
    synthetic rule of sepwisw_ref and FF the case's forcing.  The first odd NFRE the context accepts."""
    for nfre in (25, 27, 29, 35):
        cfg = Config(nang=12, nfre=nfre, nfre_red=nfre)
        case = H.make_point_case(3001, cfg, prec, spectra="mixed", seed=23)
        try:
            ctx = api.HipContext(case["tables"])
            break
        except api.EcwamHipError as e:
            assert "rotation structure" in str(e), str(e)
    else:
        pytest.fail("no odd NFRE accepted by the context")
    t, n = case["tables"], case["n"]
    assert t.NFRE_ODD == nfre
    wv, ff, _ = H.pack_device_inputs(case)
    xl = S.synthetic_xllws(t, ff[:, 1], 0.15)
    got = _run(api, ctx, case["FL1"], xl, wv, ff, kijs=7, kijl=n - 3)
    assert np.all(got[:7] == -1.0) and np.all(got[n - 3:] == -1.0)
    ref, info = S.sepwisw(t, case["FL1"], xl, wv[:, 2], ff[:, 7], ff[:, 1])
    _compare(got[7:n - 3], ref[7:n - 3], info["near"][7:n - 3], prec, f"12x{nfre}")
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_known_answers_on_the_device(api, prec):
    from test_outbs_sepwisw_host import known_answer_checks

    t = Tables(Config(nang=36, nfre=36, nfre_red=36), H.np_dtype(prec))
    names, fl1, xl, cinv, uf, wd, extra = S.known_answer_inputs(t)
    n = len(names)
    wv = np.zeros((n, 5, len(t.FR)), t.dtype)
    wv[:, 2] = cinv
    ff = np.zeros((n, 16), t.dtype)
    ff[:, 1], ff[:, 7] = wd, uf
    ctx = api.HipContext(t)
    got = _run(api, ctx, fl1, xl, wv, ff)
    known_answer_checks(t, names, fl1, got, extra)
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_small_domain_flag(api, prec):
    """flags bit 0 (CLDOMAIN = 's'): the first mask only.  Against the restatement's small_domain path, and different from flags 0."""
    cfg = Config(nang=36, nfre=36, nfre_red=36)
    ctx, t, fl1, xl, wv, ff = _implsch_case(api, cfg, prec, 1001, seed=29)
    got_s = _run(api, ctx, fl1, xl, wv, ff, small_domain=True)
    got_0 = _run(api, ctx, fl1, xl, wv, ff)
    ref, info = S.sepwisw(t, fl1, xl, wv[:, 2], ff[:, 7], ff[:, 1], small_domain=True)
    _compare(got_s, ref, info["near"], prec, "CLDOMAIN s")
    assert np.any(got_s != got_0)
    assert np.array_equal(got_s[:, :3], got_0[:, :3])                    # the total spectrum's columns do not depend on the split
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_wamintgr_on_the_o48_grid(api, prec):
    """Four WAMINTGR steps, then Wamintgr.outbs_sepwisw() against the restatement on the state copied back; OUTWNORM of shww; and where
    the one-kernel step covers the context, a model whose last step is the one kernel gives the same state and the same 15 columns."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import OUTBS_SEP_FIELDS, Wamintgr

    assert OUTBS_SEP_FIELDS == S.FIELDS
    cfg = Config(nang=36, nfre=36, nfre_red=36, idelt=450, idelpro=450)
    g = G.build_grid(48, mask="continents")
    m = Wamintgr(cfg, g, prec)
    m.init_synthetic(seed=3)
    assert m.build_weights() == 0
    for _ in range(4):
        m.step()
    out = m.outbs_sepwisw()
    torch.cuda.synchronize()
    n = m.n
    assert tuple(out.shape) == (n, 15)
    fl = m.fl1[:n].cpu().numpy()
    xl = m.xllws[:n].cpu().numpy()
    ff = m.ff[:n].cpu().numpy()
    wv = m.wvprpt[:n].cpu().numpy()
    got = out.cpu().numpy()
    ref, info = S.sepwisw(m.t, fl, xl, wv[:, 2], ff[:, 7], ff[:, 1])
    _compare(got, ref, info["near"], prec, "O48 after 4 steps")
    avg, mn, mx, cnt = m.ctx.outwnorm(out, 3, n)
    col = got[:, 3].astype(np.float64)
    assert cnt == n and mn == col.min() and mx == col.max() and abs(avg - col.mean()) < 1e-12 * max(1.0, abs(avg))
    if m.fused_available():
        f = Wamintgr(cfg, g, prec)
        f.init_synthetic(seed=3)                                          # the same state
        assert f.build_weights() == 0
        for i in range(4):
            f.step(fused=(i == 3))
        out_f = f.outbs_sepwisw()
        torch.cuda.synchronize()
        for name in ("fl1", "xllws", "ff"):
            assert torch.equal(getattr(f, name)[:n], getattr(m, name)[:n]), name
        assert torch.equal(out_f, out)
        f.ctx.close()
    m.ctx.close()


def test_rows_beyond_2_32_elements(api):
    """64-bit row addressing: FL1 / XLLWS with just over 2**32 / (NANG NFRE) rows (about 17 GB each in single precision); a case in the
    last 64 rows gives what the same case gives at row 0."""
    cfg = Config(nang=36, nfre=36, nfre_red=36)
    prec = "sp"
    k = 64
    ctx, t, fl1, xl, wv, ff = _implsch_case(api, cfg, prec, k, seed=31)
    N = 36 * 36
    rows = (2 ** 32) // N + 2 * k
    dev, dt = ctx.device, ctx.dtype
    want = _run(api, ctx, fl1, xl, wv, ff)
    big = {}
    try:
        big["fl1"] = torch.empty((rows, 36, 36), dtype=dt, device=dev)
        big["xl"] = torch.empty((rows, 36, 36), dtype=dt, device=dev)
        big["wv"] = torch.empty((rows, 5, 36), dtype=dt, device=dev)
        big["ff"] = torch.empty((rows, 16), dtype=dt, device=dev)
        big["out"] = torch.full((rows, 15), -1.0, dtype=dt, device=dev)
        a = rows - k
        assert a * N > 2 ** 32
        for name, arr in (("fl1", fl1), ("xl", xl), ("wv", wv), ("ff", ff)):
            big[name][a:] = torch.from_numpy(arr).to(dev)
        ctx.outbs_sepwisw(a, rows, big["fl1"], big["xl"], big["wv"], big["ff"], big["out"])
        torch.cuda.synchronize()
        got = big["out"][a:].cpu().numpy()
        assert float(big["out"][a - 1, 0]) == -1.0
    finally:
        big.clear()
        torch.cuda.empty_cache()
    assert np.array_equal(got, want)
    ctx.close()
