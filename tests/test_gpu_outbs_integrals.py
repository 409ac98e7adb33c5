"""OUTBLOCK's remaining spectral integrals and OUTSETWMASK on the device (ecwam_hip_outbs_integrals, ecwam_hip_outsetwmask) against the numpy
restatement tests/integrals_ref.py.

Inputs: 3001 mixed spectra (FL1 after one IMPLSCH call where the grid has a build) with, from row 8 on, the crafted points of
integrals_ref-independent known shape (crafted_points below) that take the branches ordinary sea states do not: an empty spectrum (WEFLUX's
EPSMIN guard, CTCOR's ZMISS), single frequencies (CTCOR = 1; the mean period at M = 1 sits on the cap 1/FR(1) within rounding, which is the
only way to reach it: MIN is continuous there, so no point is left out for it), a strong single frequency at NFRE - 3 (ALPHAP > ALPHAPMAX) and
one at NFRE (FM >= FR(NFRE-2)).

Gates.  Start: 2e-6 (sp) / 1e-12 (dp) relative for heights, energies, slopes and coefficients, 2e-2 / 1e-9 degrees (cyclic) for the flux
direction.  A point is left out of a column only where one of the restatement's own decisions for that column (integrals_ref.DECISIONS_OF)
has a margin under MARGIN_EPS = 64 eps; at most 1 % per column; tests/test_outbs_integrals_host.py shows on the CPU that the inputs stay
under that cap.  Every test prints what it observes.
A-priori sizes where a column needs more than the start gate:
  strn: E**2 carries XKI**6, and AKI_ICE's Newton iteration stops at a relative step of 1e-6, so XKI is known to the few ulp the last step
        leaves on either side (POW, TANH, SINH of two libraries): 6 x a few ulp.
  mss:  HALP = XMSS / (LOG(FR(NFRE)) - LOG(FM)) amplifies the ulp of two logarithms by 1 / LOG(FR(NFRE)/FM) (<= 5 in the mean branch), and
        FEMEAN of the half plane is a wavefront reduction, not the reference's serial sum.
GATES holds the start gates for every column: no larger gate has been derived from an observation, and no observed maxima are recorded here
yet (the tests print them).
"""
import numpy as np
import pytest

import fl2nd_ref as F2
import harness as H
import integrals_ref as R
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MARGIN_EPS = 64
GATES = dict(sp=dict(cd=2e-6, tauw_n=2e-6, mss=2e-6, strn=2e-6, wefmag=2e-6, wefdir=2e-2, ctcor=2e-6, bands=2e-6),
             dp=dict(cd=1e-12, tauw_n=1e-12, mss=1e-12, strn=1e-12, wefmag=1e-12, wefdir=1e-9, ctcor=1e-12, bands=1e-12))
COLS = dict(cd=(0,), tauw_n=(1,), mss=(2, 7), strn=(3,), wefmag=(4,), wefdir=(5,), ctcor=(6,))
# floors of the relative errors: a slope of 1e-4, a strain of 1e-12, 1 W/m, a height of 1 mm
FLOOR = dict(cd=1e-5, tauw_n=1e-4, mss=1e-4, strn=1e-12, wefmag=1.0, ctcor=1e-3, bands=1e-3)
NCRAFT = 5
CRAFT0 = 8


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _dev(ctx, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def crafted_points(t, nang, nfre):
    """FL1 [5][NANG][NFRE]: empty; M = 1 only; a strong line at NFRE - 3; a weak line at NFRE; one occupied direction at M = 10"""
    f = np.zeros((NCRAFT, nang, nfre), t.dtype)
    f[1, :, 0] = 1.0
    f[2, :, nfre - 4] = 10.0
    f[3, :, nfre - 1] = 0.01
    f[4, 3, 9] = 2.0
    return f


def _case(api, nang, nfre, prec, n, seed, ice=False, implsch=True, **cfgkw):
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
    if nf == 36 and implsch:
        r = H.gpu_implsch(case, ctx)
        fl1 = r["FL1"]
        ff[:, :14] = r["FF"]
    if ice:
        ff[::3, 13] = np.linspace(0.1, 3.0, len(ff[::3]))      # CITHICK > 0 on a third of the points
        ff[::3, 2] = np.linspace(0.0, 1.0, len(ff[::3]))
    t = case["tables"]
    # the crafted points go to rows CRAFT0 .. CRAFT0 + NCRAFT - 1, inside every [kijs, kijl) the tests use
    fl1 = np.concatenate([fl1[:CRAFT0], crafted_points(t, nang, nf), fl1[CRAFT0:]]).astype(t.dtype)
    wv = np.concatenate([wv[:CRAFT0], wv[:NCRAFT], wv[CRAFT0:]])
    ff = np.concatenate([ff[:CRAFT0], ff[:NCRAFT], ff[CRAFT0:]])
    return ctx, cfg, t, fl1, wv, ff


def _run(ctx, fl1, wv, ff, nband, fl2nd=None, groups=63, kijs=0, kijl=None, fill=-7.0):
    n = (fl1 if fl1 is not None else fl2nd).shape[0]
    kijl = n if kijl is None else kijl
    out = torch.full((n, 8 + nband), fill, dtype=ctx.dtype, device=ctx.device)
    tf = _dev(ctx, fl1)
    t2 = tf if fl2nd is fl1 and fl1 is not None else (fl2nd if torch.is_tensor(fl2nd) else _dev(ctx, fl2nd))
    ctx.outbs_integrals(kijs, kijl, tf, _dev(ctx, wv), _dev(ctx, ff), out, fl2nd=t2, groups=groups)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _keep(dec, col, eps, n):
    keep = np.ones(n, bool)
    for name in R.DECISIONS_OF.get(col, ()):
        if name == "ctcor_cap":      # MIN is continuous at the cap
            continue
        keep &= dec[name][1] >= MARGIN_EPS * eps
    return keep


def _compare(got, ref, dec, prec, what, sl=slice(None)):
    eps = float(np.finfo(np.float32 if prec == "sp" else np.float64).eps)
    g, r = got.astype(np.float64)[sl], ref.astype(np.float64)[sl]
    n = g.shape[0]
    obs, left = {}, {}
    for name, cols in list(COLS.items()) + [("bands", tuple(range(8, g.shape[1])))]:
        worst = 0.0
        for c in cols:
            keep = _keep({k: (v[0][sl], v[1][sl]) for k, v in dec.items()}, c, eps, n)
            left[c] = int((~keep).sum())
            assert left[c] <= 0.01 * n, (what, c, left[c])
            if name == "wefdir":
                dd = np.abs(g[keep, c] - r[keep, c]) % 360.0
                e = np.minimum(dd, 360.0 - dd)
            else:
                miss = r[keep, c] == -999.0
                assert np.array_equal(g[keep, c] == -999.0, miss), (what, c)
                e = H.rel_err(g[keep, c][~miss], r[keep, c][~miss], FLOOR[name])
            worst = max(worst, float(e.max()) if e.size else 0.0)
        obs[name] = worst
    print(f"{what} {prec}: observed maxima", {k: f"{v:.2e}" for k, v in obs.items()}, "left out per column", {c: v for c, v in left.items() if v})
    for name, gate in GATES[prec].items():
        assert obs[name] < gate, (what, name, obs[name], gate)
    return obs


def _branch_counts(dec, what):
    c = {k: (int(np.sum(v[0] != 0)), int(np.sum(v[0] == 0))) for k, v in dec.items() if k != "ns_gc"}
    c["ns_gc values"] = int(np.unique(dec["ns_gc"][0]).size)
    print(f"{what}: branches (taken, not taken)", c)
    return c


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("nang,nfre,gcb", [(36, 36, True), (24, 36, False), (12, 36, True), (12, 25, False)])
def test_parity(api, prec, nang, nfre, gcb):
    """Every column against the restatement with the seven default bands plus one band above FR(NFRE), XKMSS_CUTOFF at its default (36 x 36,
    12 x 36) or at the wavenumber of FR(20) (24 x 36, 12 x 25); LLGCBZ0 on and off; sea ice on a third of the points; rows outside
    [kijs, kijl) keep their fill.  Asserts that every listed branch is taken by a compared point."""
    n = 3001
    ctx, cfg, t, fl1, wv, ff = _case(api, nang, nfre, prec, n, seed=17, ice=True, llgcbz0=gcb)
    bands = R.default_bands(t) + [(0.5, 0.9)]
    assert R.band_constants(t, 0.5, 0.9)["tail"] and R.band_constants(t, 0.5, 0.9)["m1"] == len(t.FR) - 1
    zf = t.ZPI * t.FR[19]
    xk = 0.0 if gcb else float(zf * zf / t.G)
    ctx.set_outbs_integrals(xk, bands)
    N = fl1.shape[0]
    got = _run(ctx, fl1, wv, ff, len(bands), kijs=3, kijl=N - 2)
    assert np.all(got[:3] == -7.0) and np.all(got[N - 2:] == -7.0)
    ref, dec = R.integrals(t, fl1, wv, ff, bands=bands, xkmss=xk)
    sl = slice(3, N - 2)
    _compare(got, ref, dec, prec, f"{nang}x{len(t.FR)} LLGCBZ0={gcb}", sl)
    c = _branch_counts({k: (v[0][sl], v[1][sl]) for k, v in dec.items()}, f"{nang}x{len(t.FR)}")
    assert c["halp_mean"][0] > 0 and c["halp_mean"][1] > 0 and c["halp_max"][0] > 0
    assert c["ns_gc values"] >= 2
    assert c["xks_1"][0] > 0 and (c["xks_0"][1] > 0 if gcb else c["xks_0"][0] > 0)
    assert c["f1lim"][1] > 0 and np.any(ref[sl, 3] > 0)       # bins under F1LIM at some points, bins over it wherever the strain is positive
    assert c["wefy"][0] > 0 and c["wefy"][1] > 0
    assert c["ctcor_em"][1] > 0 and np.any(dec["ctcor_cap"][1][sl] < 1e-6)
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_separate_fl2nd(api, prec):
    """IREFRA = 2 with currents: FL2ND stored by ecwam_hip_outbs_absolute and passed on; the bands against the restatement on fl2nd_ref's
    FL2ND; the FL1 readers unchanged bit for bit from the call without fl2nd; fl2nd = NULL and fl2nd = fl1 agree bit for bit."""
    n = 2001
    ctx, cfg, t, fl1, wv, ff = _case(api, 36, 36, prec, n, seed=19, irefra=2)
    N = fl1.shape[0]
    rng = np.random.default_rng(41)
    u, v = rng.uniform(-1.5, 1.5, N).astype(t.dtype), rng.uniform(-1.5, 1.5, N).astype(t.dtype)
    bands = R.default_bands(t)
    ctx.set_outbs_integrals(0.0, bands)
    tfl = _dev(ctx, fl1)
    f2 = torch.empty_like(tfl)
    o8 = torch.zeros((N, 8), dtype=ctx.dtype, device=ctx.device)
    ctx.outbs_absolute(0, N, tfl, _dev(ctx, wv), _dev(ctx, u), _dev(ctx, v), _dev(ctx, ff), o8, fl2nd=f2)
    plain = _run(ctx, fl1, wv, ff, len(bands))
    alias = _run(ctx, fl1, wv, ff, len(bands), fl2nd=fl1)
    sep = _run(ctx, fl1, wv, ff, len(bands), fl2nd=f2)
    assert np.array_equal(plain, alias)
    assert np.array_equal(plain[:, :8], sep[:, :8]) and not np.array_equal(plain[:, 8:], sep[:, 8:])
    only = _run(ctx, None, None, None, len(bands), fl2nd=f2, groups=16)
    assert np.array_equal(only[:, 8:], sep[:, 8:]) and np.all(only[:, :8] == -7.0)
    ref2, _ = F2.intpol(t, fl1, wv[:, 0], u, v)
    want = R.band_heights(t, ref2, bands).astype(np.float64)
    e = float(np.max(H.rel_err(sep[:, 8:].astype(np.float64), want, FLOOR["bands"])))
    print(f"separate FL2ND {prec}: bands against the restatement on the restated FL2ND, largest relative error {e:.2e}")
    assert e < GATES[prec]["bands"], (e, GATES[prec]["bands"])
    ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_group_flags_and_refusals(api, prec):
    """Each group alone writes exactly its columns, bit-identical to the all-groups call; every refusal with its message."""
    n = 501
    ctx, cfg, t, fl1, wv, ff = _case(api, 24, 36, prec, n, seed=23)
    N = fl1.shape[0]
    tf, tw, tff = _dev(ctx, fl1), _dev(ctx, wv), _dev(ctx, ff)
    o = torch.zeros((N, 15), dtype=ctx.dtype, device=ctx.device)
    with pytest.raises(api.EcwamHipError, match="not set"):
        ctx.outbs_integrals(0, N, tf, tw, tff, o)
    ctx.set_outbs_integrals(0.0, [])
    o8 = torch.zeros((N, 8), dtype=ctx.dtype, device=ctx.device)
    with pytest.raises(api.EcwamHipError, match="nband = 0"):
        ctx.outbs_integrals(0, N, tf, tw, tff, o8, groups=63)
    ctx.outbs_integrals(0, N, tf, tw, tff, o8, groups=63 - 16)          # the other groups need no band
    with pytest.raises(api.EcwamHipError, match="TB <= TT"):
        ctx.set_outbs_integrals(0.0, [(12.0, 10.0)])
    with pytest.raises(api.EcwamHipError, match="below FR"):
        ctx.set_outbs_integrals(0.0, [(40.0, 50.0)])
    with pytest.raises(api.EcwamHipError, match="nband"):
        ctx.set_outbs_integrals(0.0, [(10.0, 12.0)] * 9)
    bands = R.default_bands(t)
    ctx.set_outbs_integrals(0.0, bands)
    with pytest.raises(api.EcwamHipError, match="unknown flags"):
        ctx.outbs_integrals(0, N, tf, tw, tff, o, groups=64)
    rc = ctx.lib.ecwam_hip_outbs_integrals(ctx._h, 5, 2, tf.data_ptr(), None, tw.data_ptr(), tff.data_ptr(), 63, -999.0, o.data_ptr(), None)
    assert rc != 0 and b"bad range" in ctx.lib.ecwam_hip_last_error()
    full = _run(ctx, fl1, wv, ff, len(bands))
    assert not np.any(full == -7.0)
    for g, cols in R.GROUP_COLUMNS.items():
        cols = tuple(range(8, 8 + len(bands))) if cols is None else cols
        one = _run(ctx, fl1, wv, ff, len(bands), groups=g)
        rest = [c for c in range(full.shape[1]) if c not in cols]
        assert np.array_equal(one[:, cols], full[:, cols]), g
        assert np.all(one[:, rest] == -7.0), g
    ctx.close()
    other = api.HipContext(Tables(Config(nang=18, nfre=36, nfre_red=36), H.np_dtype(prec)))
    other.set_outbs_integrals(0.0, bands)
    z = torch.zeros((4, 18, 36), dtype=other.dtype, device=other.device)
    with pytest.raises(api.EcwamHipError, match="no build for this NANG"):
        other.outbs_integrals(0, 4, z, torch.ones((4, 5, 36), dtype=other.dtype, device=other.device),
                              torch.ones((4, 16), dtype=other.dtype, device=other.device), torch.zeros((4, 15), dtype=other.dtype, device=other.device))
    other.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_outsetwmask(api, prec):
    """ecwam_hip_outsetwmask on a buffer of this call and on one of ecwam_hip_outbs, bit for bit against numpy; LICERUN off applies no ice
    mask; iodp = NULL with no sea-mask column."""
    n = 1001
    for licerun in (True, False):
        ctx, cfg, t, fl1, wv, ff = _case(api, 12, 36, prec, n, seed=29, ice=True, implsch=False, licerun=licerun, lmaskice=False)
        N = fl1.shape[0]
        rng = np.random.default_rng(5)
        iodp = (rng.uniform(size=N) > 0.2).astype(np.int32)
        ff[:, 2] = rng.uniform(0.0, 1.0, N)
        bands = R.default_bands(t)
        ctx.set_outbs_integrals(0.0, bands)
        a = _run(ctx, fl1, wv, ff, len(bands))
        b5 = torch.zeros((N, 5), dtype=ctx.dtype, device=ctx.device)
        ctx.outbs(0, N, _dev(ctx, fl1), b5)
        for buf, flags in ((a, [(i * 7) % 4 for i in range(a.shape[1])]), (b5.cpu().numpy(), [3, 2, 1, 0, 3])):
            tb = _dev(ctx, buf)
            ctx.outsetwmask(2, N - 1, tb, flags, ff=_dev(ctx, ff), iodp=_dev(ctx, iodp), cithrsh=0.3)
            want = buf.copy()
            want[2:N - 1] = R.outsetwmask(buf[2:N - 1], flags, ff[2:N - 1, 2], iodp[2:N - 1], licerun, 0.3, -999.0)
            got = tb.cpu().numpy()
            assert np.array_equal(got, want)
            masked = int((got != buf).sum())
            print(f"OUTSETWMASK {prec} LICERUN={licerun} {buf.shape[1]} columns: {masked} values masked")
            assert masked > 0
            ice_only = [f & 1 for f in flags]
            tb = _dev(ctx, buf)
            ctx.outsetwmask(0, N, tb, ice_only, ff=_dev(ctx, ff), iodp=None, cithrsh=0.3)
            want = R.outsetwmask(buf, ice_only, ff[:, 2], None, licerun, 0.3, -999.0)
            assert np.array_equal(tb.cpu().numpy(), want)
            assert licerun or np.array_equal(want, buf)
        with pytest.raises(api.EcwamHipError, match="iodp is NULL"):
            ctx.outsetwmask(0, N, _dev(ctx, a), [2] * a.shape[1], ff=_dev(ctx, ff), iodp=None)
        ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_wamintgr_outbs_integrals(api, prec):
    """The driver method on the O48 grid after two steps: the setter on first use with the default bands, the columns against the
    restatement on the state copied back."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import OUTBS_INT_FIELDS, Wamintgr

    assert OUTBS_INT_FIELDS == R.FIELDS
    cfg = Config(nang=36, nfre=36, nfre_red=36, idelt=450, idelpro=450)
    m = Wamintgr(cfg, G.build_grid(48, mask="continents"), prec)
    m.init_synthetic(seed=3)
    assert m.build_weights() == 0
    for _ in range(2):
        m.step()
    out = m.outbs_integrals()
    torch.cuda.synchronize()
    n = m.n
    assert tuple(out.shape) == (n, 15) and m.ctx.integral_bands == R.default_bands(m.t)
    ref, dec = R.integrals(m.t, m.fl1[:n].cpu().numpy(), m.wvprpt[:n].cpu().numpy(), m.ff[:n].cpu().numpy())
    _compare(out.cpu().numpy(), ref, dec, prec, "O48 after 2 steps")
    m.ctx.close()
