"""Extreme-wave parameters of OUTBLOCK on the device (ecwam_hip_outbs_extremes: KURTOSIS and W_MAXH) against the numpy restatement
tests/extremes_ref.py on the same FL1 / WAVNUM / DEPTH.

Gates.  Double precision: 1e-12 relative on every column; C3, C4, BFI and R relative to their clamp bounds (C3MAX = C4MAX = 0.25,
BF2MAX = 5, RMAX = 16: stat_nl.F90:157-162, kurtosis.F90:216-217), because they cross zero -- TRANSF_BFI changes sign near K D = 1.363
and C4 = XJ BF2 + C4_B cancels -- and the cancellations in XNU and SIG_TH (SUM2 SUM0 / SUM1**2 - 1, 1 - R1) turn rounding differences
of 1e-16 into 1e-13 of those bounds.  Single precision (SP_GATES, at most 10 x the observed maxima, which each test prints): relative on
heights, periods, QP, ETA_M and XNSLC, absolute on C3, C4, BFI and R.  The sums over frequencies are tree
reductions on the device and running sums in the restatement; points where the restatement finds a discrete decision within the noise
of single precision (NINT of XNSLC, an AKI exit, TRANSF_BFI's K D = DKMAX switch, H_MAX's ZEPSILON test) are counted (at most 0.5 % of
the points) and left out of the value gates.
"""
import numpy as np
import pytest

import extremes_ref as X
import harness as H
from ecwam_amd import synthetic as syn
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COL = {f: i for i, f in enumerate(X.FIELDS)}
RELATIVE = ("qp", "hmax", "tmax", "eta_m", "xnslc", "cmax_f", "hmax_n", "cmax_st", "hmax_st")
ABSOLUTE = ("c4", "bfi", "c3", "r")
# observed maxima over every test of this file (36 x 36 and 24 x 36 after IMPLSCH, 12 x 25, KURTOSIS only, O48 after four steps):
#   sp: relative 2.4e-5 (HMAX), absolute 7.2e-4 (BFI)
#   dp: relative 3.0e-14 (HMAX); C4 2.6e-14, BFI 5.5e-13, R 4.9e-13 absolute, that is <= 1.1e-13 of their clamp bounds
SP_GATES = dict(rel=2e-4, abs=5e-3)
DP_SCALE = dict(c3=0.25, c4=0.25, bfi=5.0, r=16.0)


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _run(ctx, fl1, wv, ff, kijs=0, kijl=None, kurtosis_only=False, fill=-1.0):
    n = fl1.shape[0]
    kijl = n if kijl is None else kijl
    tfl, twv, tff = (torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) for a in (fl1, wv, ff))
    out = torch.full((n, len(X.FIELDS)), fill, dtype=ctx.dtype, device=ctx.device)
    ctx.outbs_extremes(kijs, kijl, tfl, twv, tff, out, kurtosis_only=kurtosis_only)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _compare(got, ref, near, prec, what, cols=None):
    cols = X.FIELDS if cols is None else cols
    assert near.mean() <= 0.005, (what, int(near.sum()))
    ok = ~near
    g, r = got[ok].astype(np.float64), ref[ok].astype(np.float64)
    assert np.all(np.isfinite(g[:, [COL[c] for c in cols]])), what
    obs = dict(rel=0.0, abs=0.0)
    per = {}
    for c in cols:
        i = COL[c]
        if c in RELATIVE:
            e = float(np.max(H.rel_err(g[:, i], r[:, i], 1e-6), initial=0.0))
            obs["rel"] = max(obs["rel"], e)
        else:
            e = float(np.max(np.abs(g[:, i] - r[:, i]), initial=0.0))
            obs["abs"] = max(obs["abs"], e)
        per[c] = f"{e:.1e}"
    print(f"{what} {prec}: points {len(near)}, near a decision {int(near.sum())}; observed maxima", {k: f"{v:.2e}" for k, v in obs.items()}, per)
    if prec == "dp":
        for c in cols:
            e = float(np.max(H.rel_err(g[:, COL[c]], r[:, COL[c]], DP_SCALE.get(c, 1e-300)), initial=0.0))
            assert e < 1e-12, (what, c, e)
    else:
        for k, gate in SP_GATES.items():
            assert obs[k] < gate, (what, k, obs[k], gate)
    return obs


def _depths(n, seed):
    """Shallow (2-20 m), intermediate (20-200 m), deep (200-999 m) and BATHYMAX or more, a quarter each."""
    rng = np.random.default_rng(seed)
    d = np.concatenate([rng.uniform(2, 20, n), rng.uniform(20, 200, n), rng.uniform(200, 998, n), rng.choice([998.999, 1500.0], n)])
    return rng.permutation(d)[:n]


def _implsch_case(api, cfg, prec, n, seed):
    """FL1 after IMPLSCH on the device at the depths of _depths; WVPRPT and FF (DEPTH in column 15) of the case."""
    case = H.make_point_case(n, cfg, prec, spectra="mixed", seed=seed)
    t = case["tables"]
    depth = _depths(n, seed)
    case["props"] = syn.depth_props(depth, t, t.dtype)
    case["ENV"] = np.stack([case["props"]["EMAXDPT"], depth.astype(t.dtype)], 1)
    ctx = api.HipContext(t)
    r = H.gpu_implsch(case, ctx)
    wv, ff, _ = H.pack_device_inputs(case)
    ff[:, :14] = r["FF"]
    return ctx, t, r["FL1"], wv, ff


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("nang", [36, 24])
def test_parity_after_implsch(api, prec, nang):
    cfg = Config(nang=nang, nfre=36, nfre_red=36)
    n = 3001
    ctx, t, fl1, wv, ff = _implsch_case(api, cfg, prec, n, seed=17)
    got = _run(ctx, fl1, wv, ff, kijs=7, kijl=n - 3)
    assert np.all(got[:7] == -1.0) and np.all(got[n - 3:] == -1.0)      # rows outside [kijs, kijl) untouched
    ref, near = X.extremes(t, fl1, ff[:, 15], wv[:, 0])
    _compare(got[7:n - 3], ref[7:n - 3], near[7:n - 3], prec, f"after IMPLSCH {nang}x36")
    d = ff[7:n - 3, 15]
    for lo, hi in ((0, 20), (20, 200), (200, 998.99), (998.99, 1e9)):   # every depth class is present
        assert np.sum((d >= lo) & (d < hi)) > 100
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_parity_odd_nfre(api, prec):
    """12 directions and an odd NFRE (the first the context accepts of 25, 27, 29, 35); FL1 is the case's spectra."""
    for nfre in (25, 27, 29, 35):
        cfg = Config(nang=12, nfre=nfre, nfre_red=nfre)
        case = H.make_point_case(2001, cfg, prec, spectra="mixed", seed=23)
        try:
            ctx = api.HipContext(case["tables"])
            break
        except api.EcwamHipError as e:
            assert "rotation structure" in str(e), str(e)
    else:
        pytest.fail("no odd NFRE accepted by the context")
    t = case["tables"]
    depth = _depths(2001, 23)
    case["props"] = syn.depth_props(depth, t, t.dtype)
    case["ENV"] = np.stack([case["props"]["EMAXDPT"], depth.astype(t.dtype)], 1)
    wv, ff, _ = H.pack_device_inputs(case)
    got = _run(ctx, case["FL1"], wv, ff)
    ref, near = X.extremes(t, case["FL1"], ff[:, 15], wv[:, 0])
    _compare(got, ref, near, prec, f"12x{nfre}")
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_kurtosis_only_leaves_columns_9_to_12(api, prec):
    """flags bit 0: KURTOSIS only -- columns 9-12 keep the sentinel, columns 0-8 equal those of the full call."""
    cfg = Config(nang=36, nfre=36, nfre_red=36)
    ctx, t, fl1, wv, ff = _implsch_case(api, cfg, prec, 500, seed=29)
    got_k = _run(ctx, fl1, wv, ff, kurtosis_only=True, fill=-7.0)
    got = _run(ctx, fl1, wv, ff)
    assert np.all(got_k[:, 9:] == -7.0)
    assert np.array_equal(got_k[:, :9], got[:, :9])
    ref, near = X.extremes(t, fl1, ff[:, 15], wv[:, 0], kurtosis_only=True)
    _compare(got_k, ref, near, prec, "KURTOSIS only", cols=X.FIELDS[:9])
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_known_answers_on_the_device(api, prec):
    """The host file's known answers on the device: Goda's QP of single-direction spectra, the empty spectrum, and BF2 in deep water
    from the device's QP and the restatement's XKP and SUM0."""
    from test_outbs_extremes_host import _one_direction_case, assert_goda

    t = Tables(Config(nang=36, nfre=36, nfre_red=36), H.np_dtype(prec))
    ctx = api.HipContext(t)
    fl = np.concatenate([_one_direction_case(t), np.zeros((2, 36, 36), t.dtype)])
    n = len(fl)
    wv = np.zeros((n, 5, 36), t.dtype)
    wv[:, 0] = (2 * np.pi * np.asarray(t.FR, np.float64)) ** 2 / 9.806
    ff = np.zeros((n, 16), t.dtype)
    ff[:, 15] = 998.999
    got = _run(ctx, fl, wv, ff)
    assert_goda(t, fl[:6], got[:6, COL["qp"]], prec)
    ze = float(X.zeps(t.dtype)[0])
    z = got[6:]
    assert np.all(z[:, [COL[c] for c in ("c4", "c3", "bfi", "qp", "tmax", "xnslc")]] == 0) and np.all(z[:, 9:] == 0)
    assert np.allclose(z[:, COL["hmax"]], 4 * np.sqrt(ze), rtol=1e-6)
    case = H.make_point_case(300, Config(nang=36, nfre=36, nfre_red=36), prec, spectra="mixed", seed=9)
    wv, ff, _ = H.pack_device_inputs(case)
    ff[:, 15] = 998.999
    got = _run(ctx, case["FL1"], wv, ff)
    _, _, diag = X.kurtosis(t, case["FL1"], ff[:, 15])
    eps = diag["xkp"].astype(np.float64) * np.sqrt(diag["sum0"].astype(np.float64))
    want = 2 * (eps * np.sqrt(np.pi) * got[:, COL["qp"]].astype(np.float64)) ** 2
    live = (want > 1e-3) & (want < 4.9)
    assert live.mean() > 0.5
    rel = np.abs(got[live, COL["bfi"]] - want[live]) / want[live]
    assert rel.max() < (1e-4 if prec == "sp" else 1e-12), rel.max()
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_wamintgr_on_the_o48_grid(api, prec):
    """Four WAMINTGR steps, then Wamintgr.outbs_extremes() against the restatement on the state copied back; OUTWNORM of hmax."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import OUTBS_EXT_FIELDS, Wamintgr

    assert OUTBS_EXT_FIELDS == X.FIELDS
    cfg = Config(nang=36, nfre=36, nfre_red=36, idelt=450, idelpro=450)
    g = G.build_grid(48, mask="continents")
    m = Wamintgr(cfg, g, prec)
    m.init_synthetic(seed=3)
    assert m.build_weights() == 0
    for _ in range(4):
        m.step()
    out = m.outbs_extremes()
    torch.cuda.synchronize()
    n = m.n
    assert tuple(out.shape) == (n, 13)
    fl = m.fl1[:n].cpu().numpy()
    ff = m.ff[:n].cpu().numpy()
    wv = m.wvprpt[:n].cpu().numpy()
    got = out.cpu().numpy()
    ref, near = X.extremes(m.t, fl, ff[:, 15], wv[:, 0])
    _compare(got, ref, near, prec, "O48 after 4 steps")
    avg, mn, mx, cnt = m.ctx.outwnorm(out, COL["hmax"], n)
    col = got[:, COL["hmax"]].astype(np.float64)
    assert cnt == n and mn == col.min() and mx == col.max()
    k = m.outbs_extremes(kurtosis_only=True)
    assert torch.equal(k[:, :9], out[:, :9]) and not k[:, 9:].any()
    m.ctx.close()


def test_rows_beyond_2_32_elements(api):
    """64-bit row addressing: FL1 with just over 2**32 / (NANG NFRE) rows (about 17 GB in single precision); a case in the last 64 rows
    gives what the same case gives at row 0."""
    cfg = Config(nang=36, nfre=36, nfre_red=36)
    k = 64
    ctx, t, fl1, wv, ff = _implsch_case(api, cfg, "sp", k, seed=31)
    N = 36 * 36
    rows = (2 ** 32) // N + 2 * k
    dev, dt = ctx.device, ctx.dtype
    want = _run(ctx, fl1, wv, ff)
    big = {}
    try:
        big["fl1"] = torch.empty((rows, 36, 36), dtype=dt, device=dev)
        big["wv"] = torch.empty((rows, 5, 36), dtype=dt, device=dev)
        big["ff"] = torch.empty((rows, 16), dtype=dt, device=dev)
        big["out"] = torch.full((rows, 13), -1.0, dtype=dt, device=dev)
        a = rows - k
        assert a * N > 2 ** 32
        for name, arr in (("fl1", fl1), ("wv", wv), ("ff", ff)):
            big[name][a:] = torch.from_numpy(arr).to(dev)
        ctx.outbs_extremes(a, rows, big["fl1"], big["wv"], big["ff"], big["out"])
        torch.cuda.synchronize()
        got = big["out"][a:].cpu().numpy()
        assert float(big["out"][a - 1, 0]) == -1.0
    finally:
        big.clear()
        torch.cuda.empty_cache()
    assert np.array_equal(got, want)
    ctx.close()
