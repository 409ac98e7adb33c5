"""The second-order output spectrum on the device (ecwam_hip_set_second_order, ecwam_hip_outbs_second_order) against the numpy restatement
tests/second_order_ref.py, through the C interface, in single and double precision.

Gate on FL2ND, per bin: |device - restatement| <= n u S, the standard bound of a sum of n floating-point operations with unit round-off
u, S = the sum of the absolute values of the terms behind the bin (SECSPOM's double sum carried through the interpolation, and |F1|) and
n = 4 NANGH NFREH + 8.  No measured constant enters.  The eight columns: the gates of tests/test_gpu_outbs_absolute.py, on the points whose
peak period is determined within the FL2ND gate (second_order_ref.near_tie; at most 2 % may be left out, which
tests/test_second_order_host.py checks on the restatement alone).
"""
import numpy as np
import pytest

import fl2nd_ref as F2
import harness as H
import second_order_ref as R
from ecwam_amd.second_order import SecondOrderTables
from ecwam_amd.tables import Config, Tables
from test_gpu_outbs_absolute import ABS_GATES, COL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KIJS = 3


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


_cache = {}


def _setup(nang, prec, **cfgkw):
    """Tables, second-order tables and the inputs of second_order_ref.device_case, built once per (NANG, precision)."""
    key = (nang, prec, tuple(sorted(cfgkw.items())))
    if key not in _cache:
        t = Tables(Config(nang=nang, nfre=36, nfre_red=36, **cfgkw), H.np_dtype(prec))
        so = SecondOrderTables(t)
        _cache[key] = (t, so) + R.device_case(t, so)
    return _cache[key]


def _dev(ctx, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _wv(t, wavnum):
    wv = np.zeros((len(wavnum), 5, len(t.FR)), t.dtype)
    wv[:, 0] = wavnum
    return wv


def _run(ctx, fl1, wavnum, depth, u=None, v=None, ff=None, kijs=0, sig=1.0, absolute=False):
    n = fl1.shape[0]
    tfl = _dev(ctx, fl1)
    out = torch.full((n, 8), -1.0, dtype=ctx.dtype, device=ctx.device)
    f2 = torch.full_like(tfl, -1.0)
    if absolute:
        ctx.outbs_absolute(kijs, n, tfl, _dev(ctx, _wv(ctx.t, wavnum)), _dev(ctx, u), _dev(ctx, v), _dev(ctx, ff), out, fl2nd=f2)
    else:
        ctx.outbs_second_order(kijs, n, tfl, _dev(ctx, _wv(ctx.t, wavnum)), _dev(ctx, depth), _dev(ctx, u), _dev(ctx, v), _dev(ctx, ff), out,
                               fl2nd=f2, sig=sig)
    torch.cuda.synchronize()
    return out.cpu().numpy(), f2.cpu().numpy()


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("nang,sig", [(12, 1.0), (12, -1.0), (24, 1.0), (36, 1.0), (48, 1.0)])
def test_spectrum_and_columns_against_the_restatement(api, nang, prec, sig):
    t, so, fl1, wn, depth = _setup(nang, prec)
    ctx = api.HipContext(t)
    ctx.set_second_order(so)
    got, f2 = _run(ctx, fl1, wn, depth, kijs=KIJS, sig=sig)
    again, f2b = _run(ctx, fl1, wn, depth, kijs=KIJS, sig=sig)
    ctx.close()
    assert np.array_equal(got, again) and np.array_equal(f2, f2b)                  # scheduling: the same bits twice
    assert np.all(got[:KIJS] == -1.0) and np.all(f2[:KIJS] == -1.0)
    ref, info = R.cal_second_order_spec(so, fl1, wn, depth, sig)
    u = float(np.finfo(t.dtype).eps) / 2
    gate = info["terms"] * u * info["bound"]
    sl = slice(KIJS, None)
    err = np.abs(f2[sl].astype(np.float64) - ref[sl].astype(np.float64))
    worst = float(np.max(err / np.maximum(gate[sl], 1e-300)))
    print(f"FL2ND {nang} {prec} SIG {sig:+.0f}: largest error / gate {worst:.3e}; depth indices {sorted(set(info['jd'][sl]))}, "
          f"EMAXL off at {int((info['emaxl'][sl] == 0).sum())} points, changed bins {int((ref[sl] != fl1[sl]).sum())} of {ref[sl].size}")
    assert (ref[sl] != fl1[sl]).mean() > 0.3
    assert np.all(err <= gate[sl]), worst
    from oracle.oracle import Oracle

    keep = ~R.near_tie(ref, gate)
    keep[:KIJS] = False
    assert (~keep[sl]).mean() <= 0.02
    cols = F2.consumers(t, Oracle(t.cfg, prec), ref[keep])
    g, r = got[keep].astype(np.float64), cols.astype(np.float64)
    obs = {}
    obs["rel"] = max(float(np.max(np.abs(g[:, c] - r[:, c]) / np.maximum(np.abs(r[:, c]), 1e-3))) for c in (COL["swh"], COL["mwp"]))
    obs["pp1d"] = float(np.max(np.abs(g[:, 4] - r[:, 4]) / np.abs(r[:, 4])))
    dd = np.abs(g[:, 1] - r[:, 1]) % 360.0
    obs["deg"] = float(np.max(np.minimum(dd, 360.0 - dd)))
    obs["mp"] = max(float(np.max(H.rel_err(g[:, c], r[:, c], 1e-3))) for c in (COL["mp1"], COL["mp2"]))
    obs["spread"] = float(np.max(np.abs(g[:, 7] - r[:, 7])))
    print(f"columns {nang} {prec}: observed maxima", {k: f"{v:.2e}" for k, v in obs.items()})
    for k, gt in ABS_GATES[prec].items():
        assert obs[k] < gt, (k, obs[k], gt)


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("case", ["irefra0", "irefra2", "ice"])
def test_zero_tables_equal_outbs_absolute_bit_for_bit(api, prec, case):
    kw = dict(irefra0={}, irefra2=dict(irefra=2), ice=dict(licerun=True, lmaskice=False))[case]
    t, so, fl1, wn, depth = _setup(36, prec, **kw)
    n = len(fl1)
    rng = np.random.default_rng(7)
    u = v = ff = None
    if case == "irefra2":
        u, v = rng.uniform(-1.5, 1.5, n).astype(t.dtype), rng.uniform(-1.5, 1.5, n).astype(t.dtype)
    if case == "ice":
        ff = np.zeros((n, 16), t.dtype)
        ff[:, 2] = np.linspace(0.0, 1.0, n)
        ff[:, 3] = np.linspace(0.2, 25.0, n)[::-1]
    ctx = api.HipContext(t)
    zero = [np.zeros_like(so.TA)] * 5
    ctx.set_second_order(so, coefficients=zero)
    got, f2 = _run(ctx, fl1, wn, depth, u, v, ff, kijs=KIJS)
    want, wf2 = _run(ctx, fl1, wn, depth, u, v, ff, kijs=KIJS, absolute=True)
    ctx.close()
    assert np.array_equal(f2, wf2) and np.array_equal(got, want)
    assert not np.array_equal(f2[KIJS:], fl1[KIJS:]) or case == "irefra0"


def test_refused_without_tables(api):
    t, so, fl1, wn, depth = _setup(12, "sp")
    ctx = api.HipContext(t)
    with pytest.raises(api.EcwamHipError, match="tables are not set"):
        _run(ctx, fl1, wn, depth)
    ctx.set_second_order(so)
    _run(ctx, fl1, wn, depth)
    ctx.set_second_order(None)
    with pytest.raises(api.EcwamHipError, match="tables are not set"):
        _run(ctx, fl1, wn, depth)
    ctx.close()


def test_wamintgr_builds_the_tables_on_first_use(api):
    """Wamintgr.outbs_second_order() on the O48 grid after one step: the tables are built and uploaded by the first call, the result is
    what the context gives on the same state with the driver's default depth, and it differs from outbs_absolute()."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import Wamintgr

    m = Wamintgr(Config(nang=12, nfre=36, nfre_red=36, idelt=450, idelpro=450), G.build_grid(48, mask="continents"), "sp")
    m.init_synthetic(seed=3)
    assert m.build_weights() == 0
    m.step()
    assert not m.ctx.has_second_order
    out, f2 = m.outbs_second_order(store_spectrum=True)
    assert m.ctx.has_second_order and tuple(out.shape) == (m.n, 8) and tuple(f2.shape) == (m.n, 12, 36)
    depth = torch.full((m.n,), 999.0, dtype=m.dtype, device=m.dev)
    direct = torch.zeros_like(out)
    m.ctx.outbs_second_order(0, m.n, m.fl1, m.wvprpt, depth, None, None, m.ff, direct)
    plain = m.outbs_absolute()
    torch.cuda.synchronize()
    assert torch.equal(out, direct) and torch.equal(out, m.outbs_second_order()) and bool(torch.isfinite(out).all())
    assert not torch.equal(out[:, 0], plain[:, 0])
    m.ctx.close()
