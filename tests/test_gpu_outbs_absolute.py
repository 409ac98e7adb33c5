"""The absolute-frame output spectrum FL2ND and its parameters on the device (ecwam_hip_outbs_absolute) against the numpy restatement
tests/fl2nd_ref.py (INTPOL with IRA = 1, the ice noise reshaping) with the consumers of tests/sepwisw_ref.py and oracle.outbs on the
restated FL2ND.

Gates.  The stored FL2ND is compared bin by bin, the error relative to the largest bin of the point's restated FL2ND; no point is left
out (INTPOL is continuous in the shifted frequency, tests/test_outbs_absolute_host.py).  The eight columns are compared with the gates the
same columns have on FL1 inputs (test_outbs_parameters_and_norms: 2e-6 / 1e-12 relative, peak period 4 x, direction 2e-2 / 1e-9 degrees;
SP_GATES / DP_GATES of tests/test_gpu_outbs_sepwisw.py) where the absolute-frame inputs stay within them; where they need more the
gate is at most 10 x the observed maximum, written below.  Every test prints what it observes.
A-priori size of the per-bin error: a weight is GWH (FNEW - FR(NEWM)) / DFTH, and FNEW carries a few eps of its own size over a bin
width of 0.1 FNEW, so a contribution is known to some tens of eps; up to four contributions and a DFTH ratio of a few land in a bin.
Observed maxima over every test of this file (36 x 36 and 24 x 36 after IMPLSCH, 12 x 25, ice reshaping with and without currents, O48
after four steps):
  sp: FL2ND bin error / peak 3.4e-7; swh and mean period 7.7e-7 relative, peak period 4.7e-7, direction 4.4e-4 degrees, MWP1 / MWP2
      6.9e-7, spread 2.3e-6
  dp: FL2ND equal to the restatement bit for bit under INTPOL (9.9e-21 of the peak after the ice reshaping's EXP); swh and mean period
      1.5e-15 relative, peak period 9.3e-16, direction 7.7e-13 degrees, MWP1 / MWP2 1.2e-15, spread 2.1e-15
BIN_GATE: sp 3e-6 (under 10 x the observed maximum).  dp 2.2e-15 = 10 eps of the peak: the observed error is zero, and 10 x zero is no
gate a second libm could meet -- a LOG10 or EXP that differs by one ulp from numpy's moves a weight by a few eps (the interpolation is
continuous), which is what the gate leaves room for.  The columns stay within the gates they have on FL1 inputs, which are kept.
"""
import numpy as np
import pytest

import fl2nd_ref as F2
import harness as H
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COL = {f: i for i, f in enumerate(F2.FIELDS)}
# per-bin error of the stored FL2ND relative to the point's peak
BIN_GATE = dict(sp=3e-6, dp=2.2e-15)
# the eight columns: swh / mwp relative, pp1d relative, mwd cyclic degrees, mp1 / mp2 relative, wdw absolute
ABS_GATES = dict(sp=dict(rel=2e-6, pp1d=8e-6, deg=2e-2, mp=2e-6, spread=5e-5),
                 dp=dict(rel=1e-12, pp1d=4e-12, deg=1e-9, mp=1.4e-14, spread=1.4e-13))


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _oracle(cfg, prec):
    from oracle.oracle import Oracle

    return Oracle(cfg, prec)


def _dev(ctx, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _run(ctx, fl1, wv=None, u=None, v=None, ff=None, kijs=0, kijl=None, store=True, fill=-1.0):
    """(out [n][8], FL2ND [n][NANG][NFRE] or None) of ecwam_hip_outbs_absolute; rows outside [kijs, kijl) keep `fill`."""
    n = fl1.shape[0]
    kijl = n if kijl is None else kijl
    tfl = _dev(ctx, fl1)
    out = torch.full((n, 8), fill, dtype=ctx.dtype, device=ctx.device)
    f2 = torch.full_like(tfl, fill) if store else None
    ctx.outbs_absolute(kijs, kijl, tfl, _dev(ctx, wv), _dev(ctx, u), _dev(ctx, v), _dev(ctx, ff), out, fl2nd=f2)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (f2.cpu().numpy() if store else None)


def _bin_error(got, ref):
    peak = ref.astype(np.float64).max(axis=(1, 2), keepdims=True)
    return float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)) / peak))


def _compare_columns(got, ref, prec, what):
    g, r = got.astype(np.float64), ref.astype(np.float64)
    obs = {}
    obs["rel"] = max(float(np.max(np.abs(g[:, c] - r[:, c]) / np.maximum(np.abs(r[:, c]), 1e-3))) for c in (COL["swh"], COL["mwp"]))
    obs["pp1d"] = float(np.max(np.abs(g[:, 4] - r[:, 4]) / np.abs(r[:, 4])))
    dd = np.abs(g[:, 1] - r[:, 1]) % 360.0
    obs["deg"] = float(np.max(np.minimum(dd, 360.0 - dd)))
    obs["mp"] = max(float(np.max(H.rel_err(g[:, c], r[:, c], 1e-3))) for c in (COL["mp1"], COL["mp2"]))
    obs["spread"] = float(np.max(np.abs(g[:, 7] - r[:, 7])))
    print(f"{what} {prec}: columns, observed maxima", {k: f"{v:.2e}" for k, v in obs.items()})
    for k, gate in ABS_GATES[prec].items():
        assert obs[k] < gate, (what, k, obs[k], gate)
    return obs


def _currents(n, seed, dtype):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.5, 1.5, n).astype(dtype), rng.uniform(-1.5, 1.5, n).astype(dtype)


def _case(api, nang, nfre, prec, n, seed, **cfgkw):
    """FL1 after IMPLSCH on the device where IMPLSCH covers the grid (36 frequencies), else the mixed spectra themselves."""
    tried = (nfre,) if nfre == 36 else (nfre, nfre + 2, nfre + 4, nfre + 10)
    for nf in tried:
        cfg = Config(nang=nang, nfre=nf, nfre_red=nf, **cfgkw)
        case = H.make_point_case(n, cfg, prec, spectra="mixed", seed=seed)
        try:
            ctx = api.HipContext(case["tables"])
            break
        except api.EcwamHipError as e:
            assert "rotation structure" in str(e), str(e)
    else:
        pytest.fail("no NFRE accepted by the context")
    wv, ff, _ = H.pack_device_inputs(case)
    fl1 = case["FL1"]
    if nf == 36:
        r = H.gpu_implsch(case, ctx)
        fl1 = r["FL1"]
        ff[:, :14] = r["FF"]
    return ctx, cfg, case["tables"], fl1, wv, ff


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("nang,nfre", [(36, 36), (24, 36), (12, 36), (12, 25)])
def test_spectrum_and_column_parity(api, prec, nang, nfre):
    """3001 mixed spectra, UCUR and VCUR uniform in [-1.5, 1.5]: the stored FL2ND bin by bin and the eight columns against the
    restatement; rows outside [kijs, kijl) untouched.  The restatement takes each of the four NEWM cases, and at 36 frequencies the
    change of direction.  (It cannot occur with 25 frequencies: FNEF < 0 needs K |U| / ZPI > FREQ, in deep water FREQ > G / (ZPI |U|) =
    0.74 Hz at |U| = 1.5 SQRT(2), and the source loop ends at FMAX = 0.45 Hz there.)"""
    n = 3001
    ctx, cfg, t, fl1, wv, ff = _case(api, nang, nfre, prec, n, seed=17, irefra=2)
    u, v = _currents(n, 41, t.dtype)
    got, f2 = _run(ctx, fl1, wv, u, v, ff, kijs=7, kijl=n - 3)
    assert np.all(got[:7] == -1.0) and np.all(got[n - 3:] == -1.0)
    assert np.all(f2[:7] == -1.0) and np.all(f2[n - 3:] == -1.0)
    ref, info = F2.intpol(t, fl1, wv[:, 0], u, v)
    cases = info["cases"]
    assert all(cases[c] > 0 for c in F2.CASES[:4]), cases
    assert (cases["flip"] > 0) == (cfg.nfre == 36), cases
    sl = slice(7, n - 3)
    e = _bin_error(f2[sl], ref[sl])
    print(f"FL2ND {nang}x{cfg.nfre} {prec}: NFRE_MAX {info['nfre_max']}, cases {cases}, largest bin error / peak {e:.2e}")
    assert np.all(f2[sl] >= t.EPSMIN)
    assert e < BIN_GATE[prec], (e, BIN_GATE[prec])
    cols = F2.consumers(t, _oracle(cfg, prec), ref[sl])
    _compare_columns(got[sl], cols, prec, f"{nang}x{cfg.nfre}")
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_bit_identity_with_the_existing_entry_points(api, prec):
    """No tolerance: columns 0-4 are ecwam_hip_outbs of the stored FL2ND, columns 5-7 are columns 0-2 of ecwam_hip_outbs_sepwisw of it; on an
    IREFRA = 0, LMASKICE = T context the call on FL1 equals the two existing calls on FL1 and stores FL1; the result does not depend on
    the fl2nd buffer; a second call gives the same bits (the scatter is deterministic)."""
    n = 2001
    ctx, cfg, t, fl1, wv, ff = _case(api, 36, 36, prec, n, seed=19, irefra=2)
    u, v = _currents(n, 43, t.dtype)
    got, f2 = _run(ctx, fl1, wv, u, v, ff)
    again, f2b = _run(ctx, fl1, wv, u, v, ff)
    nostore, _ = _run(ctx, fl1, wv, u, v, ff, store=False)
    assert np.array_equal(got, again) and np.array_equal(f2, f2b) and np.array_equal(got, nostore)

    def old_calls(c, f):
        tf = _dev(c, f)
        o5 = torch.zeros((n, 5), dtype=c.dtype, device=c.device)
        o15 = torch.zeros((n, 15), dtype=c.dtype, device=c.device)
        c.outbs(0, n, tf, o5)
        c.outbs_sepwisw(0, n, tf, torch.zeros_like(tf), _dev(c, wv), _dev(c, ff), o15)
        torch.cuda.synchronize()
        return o5.cpu().numpy(), o15.cpu().numpy()[:, :3]

    o5, o3 = old_calls(ctx, f2)
    assert np.array_equal(got[:, :5], o5)
    assert np.array_equal(got[:, 5:], o3)
    ctx.close()
    plain = api.HipContext(Tables(Config(nang=36, nfre=36, nfre_red=36), H.np_dtype(prec)))
    gp, fp = _run(plain, fl1)                                              # no WAVNUM, currents or FF needed
    o5, o3 = old_calls(plain, fl1)
    assert np.array_equal(fp, fl1) and np.array_equal(gp[:, :5], o5) and np.array_equal(gp[:, 5:], o3)
    assert not np.array_equal(gp, got)                                     # the currents matter
    o8, tf = torch.zeros((n, 8), dtype=plain.dtype, device=plain.device), _dev(plain, fl1)
    with pytest.raises(api.EcwamHipError):
        plain.outbs_absolute(0, n, tf, None, None, None, None, o8, flags=1)
    with pytest.raises(api.EcwamHipError, match="alias"):
        plain.outbs_absolute(0, n, tf, None, None, None, None, o8, fl2nd=tf)      # in place: refused
    plain.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_known_answers_on_the_device(api, prec):
    from test_outbs_absolute_host import known_answer_checks

    t = Tables(Config(nang=36, nfre=36, nfre_red=36, irefra=2), H.np_dtype(prec))
    names, fl1, wn, u, v, extra = F2.known_answer_inputs(t)
    n = len(names)
    wv = np.zeros((n, 5, len(t.FR)), t.dtype)
    wv[:, 0] = wn
    ctx = api.HipContext(t)
    _, f2 = _run(ctx, fl1, wv, u, v, np.zeros((n, 16), t.dtype))
    i = names.index("tail")
    extra["tail_trunc"] = F2.intpol(t, fl1[i:i + 1], wn[i:i + 1], u[i:i + 1], v[i:i + 1], m_last=len(t.FR))[0][0]
    known_answer_checks(t, names, fl1, f2, extra)
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("irefra", [0, 2])
def test_ice_noise_reshaping(api, prec, irefra):
    """LICERUN = T, LMASKICE = F with CICOVER from 0 to 1, with and without currents: the stored FL2ND against the restatement (the
    reshaping follows INTPOL), the hand formula on the device's own result, and the columns."""
    from test_outbs_absolute_host import ice_checks

    n = 1001
    cfg = Config(nang=36, nfre=36, nfre_red=36, irefra=irefra, licerun=True, lmaskice=False)
    case = H.make_point_case(n, cfg, prec, spectra="mixed", seed=23)
    t = case["tables"]
    ctx = api.HipContext(t)
    wv, ff, _ = H.pack_device_inputs(case)
    ff[:, 2] = np.linspace(0.0, 1.0, n)
    ff[:, 3] = np.linspace(0.2, 25.0, n)[::-1]
    u, v = _currents(n, 47, t.dtype) if irefra else (None, None)
    got, f2 = _run(ctx, case["FL1"], wv if irefra else None, u, v, ff)
    ref, _ = F2.fl2nd(t, case["FL1"], wv[:, 0], u, v, ff[:, 2], ff[:, 3])
    e = _bin_error(f2, ref)
    before = F2.intpol(t, case["FL1"], wv[:, 0], u, v)[0] if irefra else case["FL1"]
    print(f"ice reshaping IREFRA {irefra} {prec}: largest bin error / peak {e:.2e}, bins reshaped {int((ref != before).sum())} of {ref.size}")
    assert e < BIN_GATE[prec], (e, BIN_GATE[prec])
    if not irefra:
        ice_checks(t, case["FL1"], f2, ff[:, 2], ff[:, 3])
    assert (ref != before).mean() > 0.05
    _compare_columns(got, F2.consumers(t, _oracle(cfg, prec), ref), prec, f"ice IREFRA {irefra}")
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_wamintgr_with_currents_on_the_o48_grid(api, prec):
    """IREFRA = 2 on the O48 grid with continents, four steps, then Wamintgr.outbs_absolute() against the restatement on the state copied
    back.  Where synthetic.currents is exactly zero the result agrees with outbs() to the zero-current bound (16 eps per bin, the
    roundings of two sums over 36 bins on top: 100 eps); where the current exceeds 0.3 m/s the mean period differs from outbs() by more than
    the gate at some points, so a call that ignored the currents could not pass.  OUTWNORM of the swh column."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import OUTBS_ABS_FIELDS, Wamintgr

    assert OUTBS_ABS_FIELDS == F2.FIELDS
    cfg = Config(nang=36, nfre=36, nfre_red=36, idelt=450, idelpro=450, irefra=2)
    g = G.build_grid(48, mask="continents")
    m = Wamintgr(cfg, g, prec)
    m.init_synthetic(seed=3)
    assert m.build_weights() == 0
    for _ in range(4):
        m.step()
    out, f2 = m.outbs_absolute(store_spectrum=True)
    plain = m.outbs()
    torch.cuda.synchronize()
    n = m.n
    assert tuple(out.shape) == (n, 8) and torch.equal(out, m.outbs_absolute())
    fl = m.fl1[:n].cpu().numpy()
    wv = m.wvprpt[:n].cpu().numpy()
    u, v = m.u_ext[:n].cpu().numpy(), m.v_ext[:n].cpu().numpy()
    got, gf2, old = out.cpu().numpy(), f2.cpu().numpy(), plain.cpu().numpy().astype(np.float64)
    ref, info = F2.intpol(m.t, fl, wv[:, 0], u, v)
    e = _bin_error(gf2, ref)
    print(f"O48 IREFRA 2 after 4 steps {prec}: {n} points, largest bin error / peak {e:.2e}, cases {info['cases']}")
    assert e < BIN_GATE[prec], (e, BIN_GATE[prec])
    _compare_columns(got, F2.consumers(m.t, _oracle(cfg, prec), ref), prec, "O48 IREFRA 2")
    g64 = got.astype(np.float64)
    still = (u == 0) & (v == 0)
    fast = np.hypot(u, v) > 0.3
    assert still.sum() > 50 and fast.sum() > 500
    eps = float(np.finfo(m.t.dtype).eps)
    for c in (COL["swh"], COL["mwp"]):
        assert np.max(np.abs(g64[still, c] - old[still, c]) / np.abs(old[still, c])) < 100 * eps
    # every column at those points: FL2ND is FL1 to rounding there, so they agree with outbs() / outbs_sepwisw() on FL1 within the gates
    # the same columns have against the restatement (direction cyclic)
    sep = m.outbs_sepwisw().cpu().numpy().astype(np.float64)
    _compare_columns(g64[still], np.concatenate([old, sep[:, :3]], 1)[still], prec, "O48 zero-current points against the FL1 calls")
    moved = np.abs(g64[fast, COL["mwp"]] - old[fast, COL["mwp"]]) / old[fast, COL["mwp"]] > ABS_GATES[prec]["rel"]
    print(f"  mean period differs from outbs() at {int(moved.sum())} of {int(fast.sum())} points with a current above 0.3 m/s")
    assert moved.sum() > 0
    avg, mn, mx, cnt = m.ctx.outwnorm(out, 0, n)
    col = g64[:, 0]
    assert cnt == n and mn == col.min() and mx == col.max() and abs(avg - col.mean()) < 1e-12 * max(1.0, abs(avg))
    m.ctx.close()


def test_rows_beyond_2_32_elements(api):
    """64-bit row addressing: FL1 and FL2ND with just over 2**32 / (NANG NFRE) rows (about 17 GB each in single precision); a case in the
    last 64 rows gives what the same case gives at row 0, in out and in the stored spectrum."""
    prec, k = "sp", 64
    ctx, cfg, t, fl1, wv, ff = _case(api, 36, 36, prec, k, seed=31, irefra=2)
    u, v = _currents(k, 53, t.dtype)
    N = 36 * 36
    rows = (2 ** 32) // N + 2 * k
    dev, dt = ctx.device, ctx.dtype
    want, want_f2 = _run(ctx, fl1, wv, u, v, ff)
    big = {}
    try:
        big["fl1"] = torch.empty((rows, 36, 36), dtype=dt, device=dev)
        big["f2"] = torch.empty((rows, 36, 36), dtype=dt, device=dev)
        big["wv"] = torch.empty((rows, 5, 36), dtype=dt, device=dev)
        big["ff"] = torch.empty((rows, 16), dtype=dt, device=dev)
        big["u"] = torch.empty((rows,), dtype=dt, device=dev)
        big["v"] = torch.empty((rows,), dtype=dt, device=dev)
        big["out"] = torch.full((rows, 8), -1.0, dtype=dt, device=dev)
        a = rows - k
        assert a * N > 2 ** 32
        big["f2"][a - 1] = -1.0
        for name, arr in (("fl1", fl1), ("wv", wv), ("ff", ff), ("u", u), ("v", v)):
            big[name][a:] = torch.from_numpy(arr).to(dev)
        ctx.outbs_absolute(a, rows, big["fl1"], big["wv"], big["u"], big["v"], big["ff"], big["out"], fl2nd=big["f2"])
        torch.cuda.synchronize()
        got, got_f2 = big["out"][a:].cpu().numpy(), big["f2"][a:].cpu().numpy()
        assert float(big["out"][a - 1, 0]) == -1.0 and bool((big["f2"][a - 1] == -1.0).all())
    finally:
        big.clear()
        torch.cuda.empty_cache()
    assert np.array_equal(got, want) and np.array_equal(got_f2, want_f2)
    ctx.close()
