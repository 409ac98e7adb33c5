"""OUTBLOCK as one device call (ecwam_hip_set_outblock, ecwam_hip_outblock_plan, ecwam_hip_outblock).

The spectral columns are compared BIT FOR BIT with the existing device calls run separately in the same test and masked with
ecwam_hip_outsetwmask: the same kernels run on the same inputs and the new kernel only moves values, so no tolerance is needed.  The copied and
converted columns are compared bit for bit with their numpy restatement written here (astype for the NEMO doubles, MAX(-PHIOCD,0), IBRMEMOUT's
rule, the masks of integrals_ref.outsetwmask).  The one exception is parameter 5, MOD(DEG*WDWAVE+180,360): compared cyclically within
2 eps x 540 degrees -- one rounding of DEG*x + 180, contracted or not, at its largest magnitude (|DEG*x| <= 360, + 180).

Inputs: 259 = 4 x 64 + 3 points -- 254 mixed spectra after one IMPLSCH call with the five crafted points of
test_gpu_outbs_integrals.crafted_points at rows 8-12; sea ice on every third point with CICOVER from 0 to 1; IODP = 0 on every seventh point;
IBRMEM in {0, 1}; altimeter, NEMO and INTF fields random; BOUT pre-filled with a sentinel.
"""
import numpy as np
import pytest

import harness as H
import integrals_ref as R
from ecwam_amd.tables import Config

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 259
NCRAFT, CRAFT0 = 5, 8
SENTINEL = -7.0
ZMISS = -999.0
CITH = 0.3      # CITHRSH as passed to the calls: the tables of a run without LMASKICE hold 1, which no CICOVER exceeds
ALL = list(range(1, 90))
CONFIGS = {
    1: dict(nang=24, cfg=dict(irefra=0, licerun=False), second=False, calls=("outbs", "partition", "extremes", "integrals")),
    2: dict(nang=24, cfg=dict(irefra=0, licerun=True, lmaskice=False), second=False, calls=("partition", "extremes", "absolute", "integrals")),
    3: dict(nang=12, cfg=dict(irefra=2), second=True, calls=("partition", "extremes", "second_order", "integrals")),
}


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _dev(ctx, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


_cache = {}


def _inputs(api, which, prec, **extra):
    """Context and host inputs of a configuration, built once (the arrays are never modified)."""
    key = (which, prec, tuple(sorted(extra.items())))
    if key in _cache:
        return _cache[key]
    from test_gpu_outbs_integrals import crafted_points

    c = CONFIGS[which]
    cfg = Config(nang=c["nang"], nfre=36, nfre_red=36, **c["cfg"], **extra)
    case = H.make_point_case(N - NCRAFT, cfg, prec, spectra="mixed", seed=31)
    t = case["tables"]
    ctx = api.HipContext(t)
    wv, ff, intf = H.pack_device_inputs(case)
    r = H.gpu_implsch(case, ctx)
    ff[:, :14] = r["FF"]

    def craft(a, rows):
        return np.concatenate([a[:CRAFT0], rows, a[CRAFT0:]])
    fl1 = craft(r["FL1"], crafted_points(t, c["nang"], 36)).astype(t.dtype)
    xllws = craft(r["XLLWS"], r["XLLWS"][:NCRAFT])
    mij = craft(r["MIJ"], r["MIJ"][:NCRAFT]).astype(np.int32)
    wv, ff = craft(wv, wv[:NCRAFT]), craft(ff, ff[:NCRAFT])
    rng = np.random.default_rng(97 + which)
    ff[::3, 13] = np.linspace(0.1, 3.0, len(ff[::3]))
    ff[::3, 2] = np.linspace(0.0, 1.0, len(ff[::3]))
    intf = rng.normal(size=(N, 16)).astype(t.dtype)
    iodp = np.ones(N, np.int32)
    iodp[::7] = 0
    d = dict(ctx=ctx, t=t, cfg=cfg, fl1=fl1, xllws=xllws.astype(t.dtype), mij=mij, wv=wv, ff=ff, intf=intf, iodp=iodp,
             ibrmem=rng.integers(0, 2, N).astype(t.dtype), altim=rng.uniform(0.0, 9.0, (3, N)).astype(t.dtype),
             nemo=rng.normal(size=(4, N)).astype(np.float64) * (1.0 + 1e-9 * np.pi),
             u=rng.uniform(-1.5, 1.5, N).astype(t.dtype), v=rng.uniform(-1.5, 1.5, N).astype(t.dtype), second=c["second"])
    d["dev"] = {k: _dev(ctx, d[k]) for k in ("fl1", "xllws", "mij", "wv", "ff", "intf", "iodp", "ibrmem", "altim", "nemo", "u", "v")}
    ctx.set_outbs_integrals(0.0, R.default_bands(t))
    if c["second"]:
        from ecwam_amd.second_order import SecondOrderTables

        ctx.set_second_order(SecondOrderTables(t))
    _cache[key] = d
    return d


def _outblock(d, ncol, kijs=0, kijl=N, **drop):
    """ecwam_hip_outblock on a sentinel-filled BOUT; drop: operands passed as NULL"""
    ctx, g = d["ctx"], d["dev"]
    bout = torch.full((N, ncol), SENTINEL, dtype=ctx.dtype, device=ctx.device)
    a = dict(fl1=g["fl1"], xllws=g["xllws"], mij=g["mij"], wvprpt=g["wv"], ff=g["ff"], intf=g["intf"], ucur=g["u"], vcur=g["v"], iodp=g["iodp"],
             ibrmem=g["ibrmem"], altim=g["altim"], nemo=g["nemo"])
    for k in drop:
        a[k] = None
    ctx.outblock(kijs, kijl, bout, zmiss=ZMISS, cithrsh=CITH, **a)
    torch.cuda.synchronize()
    return bout.cpu().numpy()


def _same_bits(a, b):
    """bit for bit, so that a NaN (the extreme-wave columns of an empty spectrum) equals itself"""
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def _mask_bits(api, ir):
    p = api.OUTBLOCK_PARAMS[ir - 1]
    return (1 if p[2] else 0) | (2 if p[3] else 0)


# where the separate calls leave the spectral parameters: buffer, column (include/ecwam_hip.h)
def _spectral_sources(fl1path, coustrn=False):
    w8 = "o5" if fl1path else "o8"
    s = {1: (w8, 0), 2: (w8, 1), 3: (w8, 2), 6: (w8, 4), 7: ("int", 0), 8: ("int", 1), 9: ("int", 2), 52: ("int", 8), 57: ("ext", 5), 62: ("int", 4),
         63: ("int", 5), 85: ("int", 6), 86: ("int", 7)}
    if not coustrn:
        s[51] = ("int", 3)
    for i in range(6):
        s[11 + i] = ("part", 3 + i)
        s[23 + i] = ("part", 9 + i)
        s[64 + i] = ("int", 9 + i)
    for i in range(3):
        s[20 + i] = ("part", i) if fl1path else ("o8", 5 + i)
        s[29 + i] = ("ext", i)
        s[70 + i] = ("ext", 6 + i)
    for i in range(9):
        s[42 + i] = ("part", 15 + i)
    s[33], s[34] = ("ext", 3), ("ext", 4)
    for i in range(4):
        s[78 + i] = ("ext", 9 + i)
    return s


def _separate_calls(api, d, fl1path):
    """The existing calls on the same inputs, each followed by ecwam_hip_outsetwmask with the bits of the parameters its columns serve."""
    ctx, g = d["ctx"], d["dev"]
    z = lambda w: torch.zeros((N, w), dtype=ctx.dtype, device=ctx.device)
    buf = dict(part=z(24), ext=z(13), int=z(15))
    f2 = None
    if fl1path:
        buf["o5"] = z(5)
        ctx.outbs(0, N, g["fl1"], buf["o5"], zmiss=ZMISS)
    else:
        buf["o8"] = z(8)
        f2 = torch.empty_like(g["fl1"])
        if d["second"]:
            depth = g["ff"][:, 15].contiguous()
            ctx.outbs_second_order(0, N, g["fl1"], g["wv"], depth, g["u"], g["v"], g["ff"], buf["o8"], fl2nd=f2, zmiss=ZMISS)
        else:
            uv = (g["u"], g["v"]) if d["cfg"].irefra >= 2 else (None, None)
            ctx.outbs_absolute(0, N, g["fl1"], g["wv"], *uv, g["ff"], buf["o8"], fl2nd=f2, zmiss=ZMISS)
    ctx.outbs_partition(0, N, g["fl1"], g["xllws"], g["mij"], g["wv"], g["ff"], buf["part"], zmiss=ZMISS)
    ctx.outbs_extremes(0, N, g["fl1"], g["wv"], g["ff"], buf["ext"])
    ctx.outbs_integrals(0, N, g["fl1"], g["wv"], g["ff"], buf["int"], fl2nd=f2, zmiss=ZMISS)
    src = _spectral_sources(fl1path)
    for name, b in buf.items():
        flags = [0] * b.shape[1]
        for ir, (bn, col) in src.items():
            if bn == name:
                flags[col] = _mask_bits(api, ir)
        ctx.outsetwmask(0, N, b, flags, ff=g["ff"], iodp=g["iodp"], cithrsh=CITH, zmiss=ZMISS)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in buf.items()}, src


def _copied(api, d):
    """The copied and converted parameters, unmasked and masked, in numpy: {parameter: (before OUTSETWMASK, after)}; 5 is handled by the caller."""
    t, ff, intf = d["t"], d["ff"], d["intf"]
    T = t.dtype
    raw = {4: ff[:, 7], 10: ff[:, 3], 32: ff[:, 15], 35: intf[:, 2], 36: intf[:, 3], 37: d["u"], 38: d["v"], 39: intf[:, 13], 40: intf[:, 14],
           41: intf[:, 9], 53: ff[:, 0], 54: ff[:, 4], 55: ff[:, 2], 56: ff[:, 13], 77: np.maximum(-intf[:, 12], T(0)),
           82: np.where(ff[:, 2] > 0, d["ibrmem"], T(ZMISS)), 83: intf[:, 10], 84: intf[:, 11], 87: np.zeros(N, T), 88: np.zeros(N, T), 89: np.zeros(N, T)}
    for i in range(3):
        raw[17 + i] = d["altim"][i]
    for i in range(4):
        raw[58 + i] = d["nemo"][i].astype(T)
        raw[73 + i] = intf[:, 5 + i]
    out = {}
    for ir, x in raw.items():
        x = np.ascontiguousarray(x, dtype=T)
        m = R.outsetwmask(x[:, None], [_mask_bits(api, ir)], ff[:, 2], d["iodp"], bool(d["cfg"].licerun), CITH, ZMISS)[:, 0]
        out[ir] = (x, m.astype(T))
    return out


_full = {}


def _full_run(api, which, prec):
    key = (which, prec)
    if key not in _full:
        d = _inputs(api, which, prec)
        cols = d["ctx"].set_outblock(ALL, second_order=d["second"])
        assert cols == {ir: ir - 1 for ir in ALL}
        _full[key] = _outblock(d, 89)
    return _full[key]


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("which", [1, 2, 3])
def test_all_parameters_match_the_separate_calls(api, which, prec):
    d = _inputs(api, which, prec)
    ctx, t = d["ctx"], d["t"]
    fl1path = which == 1
    got = _full_run(api, which, prec)
    assert not np.any(got == SENTINEL)                   # niprmout = 89: every column of both lane passes is written
    plan = ctx.outblock_plan()
    assert plan["calls"] == CONFIGS[which]["calls"] and plan["int_groups"] == 63 and plan["w_maxh"] and plan["stores_fl2nd"] == (not fl1path)
    bufs, src = _separate_calls(api, d, fl1path)
    for ir, (bn, col) in sorted(src.items()):
        a, b = got[:, ir - 1], bufs[bn][:, col]
        bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
        assert _same_bits(a, b), (which, prec, ir, bn, col, bad[:8], a[bad[:8]], b[bad[:8]], a[np.isnan(a)].size)
    cp = _copied(api, d)
    for ir, (_, masked) in sorted(cp.items()):
        assert np.array_equal(got[:, ir - 1], masked), (which, prec, ir)
    assert set(src) | set(cp) | {5} == set(ALL)
    for ir in (87, 88, 89):
        assert np.all(cp[ir][0] == 0) and np.all(got[:, ir - 1] == 0)       # 0 before masking; no mask applies to the extra fields
    # 5: the wind direction, no mask (mpcrtbl.F90:117)
    eps = float(np.finfo(t.dtype).eps)
    want = np.fmod(57.295778667 * d["ff"][:, 1].astype(np.float64) + 180.0, 360.0)
    dd = np.abs(got[:, 4].astype(np.float64) - want) % 360.0
    e = float(np.minimum(dd, 360.0 - dd).max())
    print(f"configuration {which} {prec}: parameter 5 within {e:.3e} degrees (bound {2 * eps * 540:.3e})")
    assert e <= 2 * eps * 540.0
    # the masks and the special rules took both branches
    ice_on = bool(d["cfg"].licerun)
    assert np.any(cp[82][0] == ZMISS) and np.any(cp[82][0] != ZMISS) and np.any(cp[77][0] == 0) and np.any(cp[77][0] > 0)
    assert np.any((got[:, 0] == ZMISS) & (d["iodp"] == 0)) and np.any(got[:, 0] != ZMISS)
    assert ice_on == bool(np.any((got[:, 0] == ZMISS) & (d["iodp"] == 1)))
    assert np.array_equal(got[:, 57], d["nemo"][0].astype(t.dtype)) and (prec == "dp" or not np.array_equal(got[:, 57].astype(np.float64), d["nemo"][0]))


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_sparse_request_and_plan(api, prec):
    d = _inputs(api, 1, prec)
    ctx = d["ctx"]
    full = _full_run(api, 1, prec)
    ito = np.zeros(89, np.int32)
    ito[[0, 4, 43, 81]] = [3, 1, 4, 2]                   # a shuffled ITOBOUT
    cols = ctx.set_outblock({1: 1, 5: -1, 44: 2, 82: 1}, itobout=ito, niprmout=4)
    assert cols == {1: 2, 5: 0, 44: 3, 82: 1}
    plan = ctx.outblock_plan()
    assert plan["calls"] == ("outbs", "partition") and plan["int_groups"] == 0 and not plan["w_maxh"] and not plan["stores_fl2nd"]
    # nothing but what the four read is needed
    got = _outblock(d, 4, intf=None, ucur=None, vcur=None, altim=None, nemo=None)
    for ir, c in cols.items():
        assert _same_bits(got[:, c], full[:, ir - 1]), ir
    ctx.set_outblock(ALL)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_row_range(api, prec):
    d = _inputs(api, 2, prec)
    full = _full_run(api, 2, prec)
    d["ctx"].set_outblock(ALL)
    got = _outblock(d, 89, kijs=5, kijl=200)
    assert np.all(got[:5] == SENTINEL) and np.all(got[200:] == SENTINEL)
    assert _same_bits(got[5:200], full[5:200])


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_strain_source_switch(api, prec):
    from ecwam_amd.tables import Tables

    base = _inputs(api, 1, prec)
    # the inputs of configuration 1 on a context that differs by LWNEMOCOUSTRN alone
    ctx = api.HipContext(Tables(Config(nang=CONFIGS[1]["nang"], nfre=36, nfre_red=36, lwnemocoustrn=True, **CONFIGS[1]["cfg"]), base["t"].dtype))
    ctx.set_outbs_integrals(0.0, R.default_bands(base["t"]))
    d = dict(base, ctx=ctx)
    cols = ctx.set_outblock([51, 9])
    plan = ctx.outblock_plan()
    assert plan["calls"] == ("integrals",) and plan["int_groups"] == api.OUTBS_INT_GROUPS["slopes"]       # no strain group
    got = _outblock(d, 2)
    want = R.outsetwmask(d["intf"][:, 4:5], [_mask_bits(api, 51)], d["ff"][:, 2], d["iodp"], False, CITH, ZMISS)[:, 0]
    assert np.array_equal(got[:, cols[51]], want)
    ctx.set_outblock([51])
    assert ctx.outblock_plan()["calls"] == ()
    ctx.close()
    other = base["ctx"]
    other.set_outblock([51])
    assert other.outblock_plan()["int_groups"] == api.OUTBS_INT_GROUPS["strain"]
    other.set_outblock(ALL)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_refusals(api, prec):
    """Every refusal returns a non-zero code with a reason that names the cause, and launches nothing: BOUT keeps its sentinel."""
    d = _inputs(api, 1, prec)
    t = d["t"]
    fresh = api.HipContext(t)
    d2 = dict(d, ctx=fresh)
    with pytest.raises(api.EcwamHipError, match="ecwam_hip_set_outblock first"):
        _outblock(d2, 89)
    with pytest.raises(api.EcwamHipError, match="no plan"):
        fresh.outblock_plan()
    with pytest.raises(api.EcwamHipError, match="ecwam_hip_set_outbs_integrals"):
        fresh.set_outblock([9])
    fresh.set_outbs_integrals(0.0, R.default_bands(t)[:3])
    with pytest.raises(api.EcwamHipError, match="do not match the requested period"):
        fresh.set_outblock([65])
    fresh.set_outbs_integrals(0.0, [(10.0, 12.0)] + R.default_bands(t)[1:])
    with pytest.raises(api.EcwamHipError, match="do not match the requested period"):
        fresh.set_outblock([52])
    fresh.set_outblock([9])                                    # no band requested: the bands do not matter
    fresh.set_outbs_integrals(0.0, R.default_bands(t))
    one = np.ones(89, np.int32)
    p = lambda a: a.ctypes.data
    rc = fresh.lib.ecwam_hip_set_outblock(fresh._h, 88, p(one), p(one), p(one), p(one), 89, 0)
    assert rc != 0 and b"jppflag must be 89" in fresh.lib.ecwam_hip_last_error()
    ito = np.zeros(89, np.int32)
    ito[0], ito[4] = 1, 3
    with pytest.raises(api.EcwamHipError, match="parameter 5 .* outside 1 .. niprmout"):
        fresh.set_outblock([1, 5], itobout=ito, niprmout=2)
    ito[4] = 0
    with pytest.raises(api.EcwamHipError, match="parameter 5 .* outside 1 .. niprmout"):
        fresh.set_outblock([1, 5], itobout=ito, niprmout=2)
    ito[4] = 1
    with pytest.raises(api.EcwamHipError, match="parameters 1 and 5 are mapped to the same column"):
        fresh.set_outblock([1, 5], itobout=ito, niprmout=2)
    with pytest.raises(api.EcwamHipError, match="42-50 .* CLDOMAIN = 's'"):
        fresh.set_outblock([1, 47], small_domain=True)
    with pytest.raises(api.EcwamHipError, match="no second-order tables"):
        fresh.set_outblock([1], second_order=True)
    fresh.set_outblock(ALL)
    for drop, name, ir in (("altim", "altim", 17), ("nemo", "nemo", 58), ("ibrmem", "ibrmem", 82), ("ucur", "ucur", 37), ("intf", "intf", 35),
                           ("iodp", "iodp", 1), ("mij", "mij", 42), ("fl1", "fl1", 1)):
        with pytest.raises(api.EcwamHipError, match=f"{name} is NULL but parameter {ir} is requested"):
            _outblock(d2, 89, **{drop: None})
    # nothing was launched by any refused call: a last one on a BOUT we keep
    bout = torch.full((N, 89), SENTINEL, dtype=fresh.dtype, device=fresh.device)
    g = d["dev"]
    with pytest.raises(api.EcwamHipError, match="altim is NULL"):
        fresh.outblock(0, N, bout, fl1=g["fl1"], xllws=g["xllws"], mij=g["mij"], wvprpt=g["wv"], ff=g["ff"], intf=g["intf"], ucur=g["u"], vcur=g["v"],
                       iodp=g["iodp"], ibrmem=g["ibrmem"], altim=None, nemo=g["nemo"], cithrsh=CITH)
    rc = fresh.lib.ecwam_hip_outblock(fresh._h, 7, 3, *([None] * 12), 0.3, ZMISS, bout.data_ptr(), None)
    assert rc != 0 and b"bad range" in fresh.lib.ecwam_hip_last_error()
    torch.cuda.synchronize()
    assert bool((bout == SENTINEL).all())
    # without 17-19 and 58-61 the two arrays may be NULL
    req = [ir for ir in ALL if not (17 <= ir <= 19 or 58 <= ir <= 61)]
    cols = fresh.set_outblock(req)
    got = _outblock(d2, len(req), altim=None, nemo=None)
    full = _full_run(api, 1, prec)
    assert all(_same_bits(got[:, c], full[:, ir - 1]) for ir, c in cols.items())
    fresh.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_wamintgr_outblock(api, prec):
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import Wamintgr

    want = [ir for ir in ALL if not (17 <= ir <= 19 or 58 <= ir <= 61 or ir in (37, 38))]
    for licerun in (False, True):
        # without an ice run OUTSETWMASK leaves swh as OUTBS gives it (IODP = 1 everywhere); with one, the sea-ice mask of parameter 1 applies
        cfg = Config(nang=12, nfre=36, nfre_red=36, idelt=450, idelpro=450, licerun=licerun)
        m = Wamintgr(cfg, G.build_grid(16, mask="continents"), prec)
        m.init_synthetic(seed=3)
        assert m.build_weights() == 0
        m.step()
        bout, cols = m.outblock()
        assert sorted(cols) == want and sorted(cols.values()) == list(range(len(want))) and tuple(bout.shape) == (m.n, len(want))
        swh = m.outbs()[:, 0]
        if licerun:
            ice = m.ff[: m.n, 2] > float(m.t.CITHRSH)
            print(f"O16 {prec}: {int(ice.sum())} of {m.n} points under the sea-ice mask")
            swh = torch.where(ice, torch.full_like(swh, ZMISS), swh)
        assert torch.equal(bout[:, cols[1]], swh)
        b2, c2 = m.outblock([6, 1])
        assert c2 == {1: 0, 6: 1} and torch.equal(b2[:, 0], bout[:, cols[1]]) and torch.equal(b2[:, 1], bout[:, cols[6]])
        assert m.ctx.outblock_plan()["calls"] == ("outbs",)
        m.ctx.close()
