"""ecwam_hip_getspec_values / _getspec_unpack and the Wamintgr methods over them on the device (run with -m gpu), against flang's evaluation of
the statements of GETSPEC's GRIB read: tests/golden/gribin_0.npz, recorded by tools/make_golden_gribin.py in both precisions, with the inputs
and the restatement of tests/gribin_ref.py.  Case A has 204 points: three tiles of 64 and a ragged fourth.

Gates (tests/gribin_ref.py::gate, from tests/golden/gribin_observed.json; nothing in them comes from the device) on |a - b| / (|b| + PPEPS),
against the DOUBLE precision fixture, per element: double precision 4 x restatement_vs_reference_dp, floored at 4 eps; single precision
4 x reference_sp_vs_dp.  Elements that came from missing values equal EPSMIN exactly; untouched elements are compared bit for bit with the
sentinel they held.  The round trip OUTSPEC -> GETSPEC on the device is held to ln 10 x (the outbound gate of tests/gribout_ref.py, an absolute
error of the logarithm) + (the inbound gate): both from the observed files, derived and not tuned.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gribin_ref as R
import gribout_ref as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -777.25
NF = 300


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _T(prec):
    return np.float32 if prec == "sp" else np.float64


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _context(api, prec, gmap=None, nang=12, nfre_red=25):
    ctx = api.HipContext(G.tables(prec, nang, nfre_red))
    if gmap is not None:
        ctx.set_grib_map(*gmap)
    return ctx


def _up(ctx, a, T):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=T)).to(ctx.device)


def _sent(ctx, n, nang=12):
    return torch.full((n, nang, 36), SENT, dtype=ctx.dtype, device=ctx.device)


def _field_index(fields, nang=12):
    f = np.asarray(fields)
    return f % nang, f // nang


def _untouched(fl, fields, nang=12):
    """every element of fl [n][NANG][36] outside the fields still holds the sentinel"""
    w = np.zeros(fl.shape[1:], bool)
    w[_field_index(fields, nang)] = True
    return (fl[:, ~w] == fl.dtype.type(SENT)).all()


def _hold(prec, what, got, ref_dp, miss, extra=0.0):
    """got [nfld][npts] (device, working precision) against a double precision reference: EPSMIN exactly where the value was missing, the rest
    within the gate (+ extra) on |a - b| / (|b| + PPEPS)"""
    T = _T(prec)
    assert got.dtype == T and got.shape == ref_dp.shape == miss.shape
    eps = T(G.tables(prec).EPSMIN)
    assert np.array_equal(got == eps, miss), f"{what}: the pattern of EPSMIN differs at {int(((got == eps) != miss).sum())} places"
    lim = R.gate(prec, R.observed()) + extra
    a, b = got.astype(np.float64), np.asarray(ref_dp, np.float64)
    err = np.where(miss, 0.0, np.abs(a - b) / (np.abs(b) + R.PPEPS))
    print(f"{what} {prec}: largest error {float(err.max()):.3e}, {float(err.max()) / lim:.3f} of its gate {lim:.3e}")
    assert lim <= 8 * np.finfo(T).eps      # a gate above this would not be a matter of rounding
    assert (err <= lim).all(), what


def _runs(fields):
    """(first field, position in the list, length) of every run of consecutive fields"""
    out, a = [], 0
    for i in range(1, len(fields) + 1):
        if i == len(fields) or fields[i] != fields[i - 1] + 1:
            out.append((fields[a], a, i - a))
            a = i
    return out


# ---- 1. the recorded cases against the fixture.  A reads through the output map (a reduced grid: the map of the read is the same); B, whose
# encoded vector begins north of the grid, through the map of the read, as the reference's full copy without start offset goes
@pytest.mark.parametrize("name", R.NAMES)
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_cases_against_the_reference(prec, name, api):
    gold = R.load_golden()
    T = _T(prec)
    g = R.grid_of(name)
    n = g["ixlg"].size
    v = R.inputs(name)
    fields = R.fields_of(name)
    if name == "B":
        ival, nval = R.read_map(g)
        assert nval == 40 and v.shape[1] == 88
        gmap = (ival, nval, None)
    else:
        gmap = G.value_map(g)
        assert np.array_equal(gmap[0], R.read_map(g)[0])
    ctx = _context(api, prec, gmap)
    try:
        fl = _sent(ctx, n)
        vd = _up(ctx, v, T)
        for f0, at, nf in _runs(fields):
            ctx.getspec_values(0, n, vd[at:at + nf], fl, ifld0=f0)
        torch.cuda.synchronize()
        got = fl.cpu().numpy()
        assert _untouched(got, fields)
        k, m = _field_index(fields)
        _hold(prec, name, np.ascontiguousarray(got[:, k, m].T), gold[f"{name}_dp"], R.from_missing(v, g))
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_case_b_through_the_output_map(prec, api):
    """The restart case on the regular grid: the message was written through the map with the start offset, and is read through it."""
    T = _T(prec)
    g = R.grid_of("B")
    n = g["ixlg"].size
    v = R.inputs("B")
    ival, ntencode, poles = G.value_map(g)
    assert ival.min() >= 8 and ntencode == 88
    ctx = _context(api, prec, (ival, ntencode, poles))
    try:
        fl = _sent(ctx, n)
        ctx.getspec_values(0, n, _up(ctx, v, T), fl, ifld0=G.B_FIELDS[0])
        torch.cuda.synchronize()
        got = fl.cpu().numpy()
        fields = R.fields_of("B")
        assert _untouched(got, fields)
        k, m = _field_index(fields)
        want = R.unscale(v, np.float64)[:, ival]
        miss = want == R.ZMISS
        assert 0 < miss.sum() < miss.size
        _hold(prec, "B through the output map", np.ascontiguousarray(got[:, k, m].T), want, miss, R.observed()["restatement_vs_reference_dp"])
    finally:
        ctx.close()


# ---- 2. the round trip on the device: OUTSPEC -> GETSPEC, case A over all 300 fields and the second tile geometry (NANG = 36, NFRE_RED = 29:
# the pitch of the tile, the pieces per direction and the last piece, cut at NFRE_RED, all change)
@functools.lru_cache(maxsize=None)
def _round_trip(prec, second):
    from ecwam_amd import api
    T = _T(prec)
    if second:
        s = G.second_geometry()
        g, fl_in, nang, nred = s["grid"], s["fl"], 36, 29
    else:
        c = G.cached_cases()
        g, fl_in, nang, nred = c["grid_a"], c["fl_a"], 12, 25
    n = fl_in.shape[0]
    ctx = _context(api, prec, G.value_map(g), nang, nred)
    try:
        values = torch.full((nang * nred, 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.outspec_values(0, n, _up(ctx, fl_in, T), values)
        back = _sent(ctx, n, nang)
        ctx.getspec_values(0, n, values, back)
        torch.cuda.synchronize()
        return g, fl_in, values.cpu().numpy(), back.cpu().numpy()
    finally:
        ctx.close()


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_round_trip_on_the_device(prec, second, api):
    T = _T(prec)
    g, fl_in, values, back = _round_trip(prec, second)
    nang, nred = (36, 29) if second else (12, 25)
    ival, _, poles = G.value_map(g)
    eps = T(G.tables(prec, nang, nred).EPSMIN)
    assert (back[:, :, nred:] == T(SENT)).all() and not (back[:, :, :nred] == T(SENT)).any()
    f = np.arange(nang * nred)
    sent_back = np.ascontiguousarray(back[:, f % nang, f // nang].T)      # [nfld][npts]
    orig = G.fields_of(fl_in.astype(np.float64), f, nang)
    v = values[:, ival]
    miss = v == T(R.ZMISS)
    assert 0 < miss.sum() < miss.size
    assert np.array_equal(sent_back == eps, miss)      # where the encoder wrote ZMISS: EPSMIN exactly, and nowhere else
    # where the encoder kept the value of the point itself (a pole row holds the mean of the row beside it instead)
    on_pole = np.zeros(ival.size, bool)
    for p in (poles.north, poles.south):
        on_pole |= (ival >= p.pole0) & (ival < p.pole0 + p.npole)
    assert 0 < on_pole.sum() < 16
    kept = ~miss & ~on_pole[None, :]
    out_gate = np.broadcast_to(G.gate(prec, G.observed(), v.astype(np.float64)), v.shape)
    lim = np.log(10.0) * out_gate + R.gate(prec, R.observed())
    err = np.abs(sent_back.astype(np.float64) - orig) / (orig + R.PPEPS)
    print(f"round trip {prec} {nang} x {nred}: largest error {float(err[kept].max()):.3e}, {float((err / lim)[kept].max()):.3f} of its bound "
          f"({float(lim[kept].min()):.3e} .. {float(lim[kept].max()):.3e})")
    assert (err[kept] <= lim[kept]).all()
    # the points of a pole row read one number per field
    for p in (poles.north, poles.south):
        rows = (ival >= p.pole0) & (ival < p.pole0 + p.npole)
        assert (sent_back[:, rows] == sent_back[:, rows][:, :1]).all()


# ---- 3. field and row ranges, on vectors made for the purpose: values over the whole scale with one in seven missing
@functools.lru_cache(maxsize=None)
def _vectors():
    rng = np.random.default_rng(20260201)
    v = rng.uniform(-10.5, 1.5, (NF, 292)).astype(np.float32)
    v[rng.uniform(size=v.shape) < 1 / 7] = R.ZMISS
    return v


@functools.lru_cache(maxsize=None)
def _full(prec):
    """all 300 fields of _vectors() in one call over all rows of grid A, computed once and left unchanged"""
    from ecwam_amd import api
    g = R.grid_of("A_ice0")
    ctx = _context(api, prec, G.value_map(g))
    try:
        fl = _sent(ctx, g["ixlg"].size)
        ctx.getspec_values(0, g["ixlg"].size, _up(ctx, _vectors(), _T(prec)), fl)
        torch.cuda.synchronize()
        out = fl.cpu().numpy()
        out.setflags(write=False)
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_the_full_call_against_the_restatement(prec, api):
    g = R.grid_of("A_ice0")
    full = _full(prec)
    assert (full[:, :, 25:] == _T(prec)(SENT)).all()
    f = np.arange(NF)
    want = R.decode(_vectors(), g, "dp")
    _hold(prec, "300 fields", np.ascontiguousarray(full[:, f % 12, f // 12].T), want, R.from_missing(_vectors(), g), R.observed()["restatement_vs_reference_dp"])


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_field_ranges(prec, api):
    """Slabs that cut inside a 16-byte piece (frequencies 3 and 13, 0-based, in both precisions) and inside a direction run, together: the one
    call, bit for bit; one slab alone: nothing outside its fields is touched."""
    T = _T(prec)
    g = R.grid_of("A_ice0")
    n = g["ixlg"].size
    full = _full(prec)
    ctx = _context(api, prec, G.value_map(g))
    try:
        vd = _up(ctx, _vectors(), T)
        cuts = [0, 7, 43, 161, 299, 300]      # (M, K) = (0, 7), (3, 7), (13, 5), (24, 11)
        fl = _sent(ctx, n)
        for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
            ctx.getspec_values(0, n, vd[a:b], fl, ifld0=a)
        alone = _sent(ctx, n)
        ctx.getspec_values(0, n, vd[43:161], alone, ifld0=43)
        one = _sent(ctx, n)
        ctx.getspec_values(0, n, vd[298:299], one, ifld0=298)
        torch.cuda.synchronize()
        assert _bits(fl.cpu().numpy(), full)
        for got, fields in ((alone.cpu().numpy(), np.arange(43, 161)), (one.cpu().numpy(), np.arange(298, 299))):
            k, m = _field_index(fields)
            assert _untouched(got, fields) and _bits(got[:, k, m], full[:, k, m])
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_row_ranges(prec, api):
    """Two disjoint ranges are the one call; rows outside a range keep the sentinel -- a range smaller than a tile of 64 points, one that ends
    off a tile edge, and in the unpack form as well."""
    T = _T(prec)
    g = R.grid_of("A_ice0")
    n = g["ixlg"].size
    full = _full(prec)
    ctx = _context(api, prec, G.value_map(g))
    try:
        vd = _up(ctx, _vectors(), T)
        two = _sent(ctx, n)
        ctx.getspec_values(70, n, vd, two)
        ctx.getspec_values(0, 70, vd, two)
        parts = []
        for k0, k1 in ((10, 40), (3, 131), (64, 65)):
            fl = _sent(ctx, n)
            ctx.getspec_values(k0, k1, vd, fl)
            parts.append((k0, k1, fl))
        torch.cuda.synchronize()
        assert _bits(two.cpu().numpy(), full)
        for k0, k1, fl in parts:
            got = fl.cpu().numpy()
            assert _bits(got[k0:k1], full[k0:k1]) and (got[:k0] == T(SENT)).all() and (got[k1:] == T(SENT)).all(), (k0, k1)
    finally:
        ctx.close()


# ---- 4. the unpack form: outspec_pack -> getspec_unpack reproduces the packed fields of FL1 bit for bit, with ld > kijl, and part by part
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_pack_then_unpack(prec, api):
    c = G.cached_cases()
    T = _T(prec)
    n = c["fl_a"].shape[0]
    ld = n + 3
    ctx = _context(api, prec)      # no map: neither call needs one
    try:
        fl_in = _up(ctx, c["fl_a"], T)
        blk = torch.full((NF, ld), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.outspec_pack(0, n, fl_in, blk)
        back = _sent(ctx, n)
        ctx.getspec_unpack(0, n, blk, back)
        part = _sent(ctx, n)
        ctx.getspec_unpack(5, 150, blk[30:95], part, ifld0=30)
        torch.cuda.synchronize()
        got, want = back.cpu().numpy(), c["fl_a"].astype(T)
        assert _bits(got[:, :, :25], want[:, :, :25]) and (got[:, :, 25:] == T(SENT)).all()
        p = part.cpu().numpy()
        fields = np.arange(30, 95)
        k, m = _field_index(fields)
        assert _bits(p[5:150][:, k, m], want[5:150][:, k, m]) and _untouched(p, fields) and (p[:5] == T(SENT)).all() and (p[150:] == T(SENT)).all()
        # with the flags the block is decoded like a vector: the same numbers as through a map that is the identity
        dec = _sent(ctx, n)
        v = _up(ctx, np.ascontiguousarray(_vectors()[:, :n]), T)
        ctx.getspec_unpack(0, n, v, dec, unscale=True, missing=True)
        ctx.set_grib_map(np.arange(n), n, None)
        via = _sent(ctx, n)
        ctx.getspec_values(0, n, v, via)
        torch.cuda.synchronize()
        assert _bits(dec.cpu().numpy(), via.cpu().numpy()) and not (dec[:, :, :25] == SENT).any()
    finally:
        ctx.close()


# ---- 5. the driver: the restart record without a transposition on the host, and getspec() = the separate calls + getspec_tail
@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_the_methods_of_the_driver(prec, api, tmp_path):
    from ecwam_amd import grid as grid_mod
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    m = Wamintgr(Config(nang=12, nfre=36, nfre_red=29, idelt=450, idelpro=450), grid_mod.build_grid(16, mask="continents"), prec)
    try:
        m.init_synthetic(seed=3)
        n = m.n
        assert n > 64
        # the record covers the fields up to NANG * NFRE, beyond those of a GRIB read
        state = m.fl1[:n].clone()
        path = str(tmp_path / "restart.bin")
        m.write_restart(path)
        m.fl1.fill_(SENT)
        m.read_restart(path)
        host = m.fl1[:n].clone()
        m.fl1.fill_(SENT)
        m.gfast_valid = True
        m.read_restart_device(path)
        torch.cuda.synchronize()
        assert torch.equal(host, state) and torch.equal(m.fl1[:n], host) and (m.fl1[n:] == SENT).all() and m.gfast_valid is False
        # getspec
        with pytest.raises(RuntimeError, match="set_grib_map"):
            m.getspec(torch.zeros((1, 1), dtype=m.dtype, device=m.dev))
        m.set_grib_map()
        values, _ = m.outspec()
        nf = 12 * 29
        m.fl1.fill_(SENT)
        m.ctx.getspec_values(0, n, values, m.fl1)
        m.ctx.getspec_tail(0, n, m.fl1, m.ff)
        want = m.fl1[:n].clone()
        m.fl1.fill_(SENT)
        m.gfast_valid = True
        m.getspec(values)
        one = m.fl1[:n].clone()
        assert m.gfast_valid is False
        m.fl1.fill_(SENT)
        m.getspec([(0, values[:100].cpu().numpy()), (100, values[100:])])
        slabs = m.fl1[:n].clone()
        m.fl1.fill_(SENT)
        m.getspec(values[:nf - 12], fields=(0, nf - 12), nfre_red=28)      # a file that holds one frequency less: the tail starts below it
        short = m.fl1[:n].clone()
        m.fl1.fill_(SENT)
        m.ctx.getspec_values(0, n, values[:nf - 12], m.fl1)
        m.ctx.getspec_tail(0, n, m.fl1, m.ff, 28)
        torch.cuda.synchronize()
        assert torch.equal(one, want) and torch.equal(slabs, want) and not (want == SENT).any()
        assert torch.equal(short, m.fl1[:n]) and not (short == SENT).any() and not torch.equal(short[:, :, 28:], want[:, :, 28:])
    finally:
        m.ctx.close()


# ---- 6. refusals, by the text of ecwam_hip_last_error; after a refusal, and after an empty range, the output is unchanged
def test_refusals(api):
    from ecwam_amd import lib
    from ecwam_amd.tables import Config, Tables

    g = R.grid_of("A_ice0")
    ival, ntencode, poles = G.value_map(g)
    n = ival.size
    ctx = _context(api, "sp")
    h, L = ctx._h, ctx.lib
    err = lambda: L.ecwam_hip_last_error().decode()
    try:
        dev = ctx.device
        fl = torch.full((n, 12, 36), SENT, dtype=torch.float32, device=dev)
        v = torch.zeros((4, ntencode + 4), dtype=torch.float32, device=dev)
        o = lib.GribOpts(-3.0, 1e-10, 0.0, 0.002, 0.0, 9, -999.0)
        ob = C.byref(o)
        p = lambda t: C.c_void_p(t.data_ptr())
        off = lambda t, b: C.c_void_p(t.data_ptr() + b)
        fs = ntencode + 4
        values = lambda *a: L.ecwam_hip_getspec_values(*a)
        unpack = lambda *a: L.ecwam_hip_getspec_unpack(*a)
        for call in (values, unpack):
            assert call(None, 0, n, p(v), fs, 0, 4, 3, ob, p(fl), None) == 1 and err() == "null context"
        # no map yet: the values form refuses, the unpack form needs none
        assert values(h, 0, n, p(v), fs, 0, 4, 3, ob, p(fl), None) == 1 and err().endswith("no grib map")
        ctx.set_grib_map(ival, ntencode, poles)
        assert values(h, 0, n, p(v), fs, 0, 4, 3, ob, p(fl), None) == 0
        torch.cuda.synchronize()
        fl.fill_(SENT)
        # the row range: bad, or beyond the map (values) / beyond ld (unpack)
        for k0, k1 in ((-1, n), (5, 4), (0, n + 1)):
            assert values(h, k0, k1, p(v), fs, 0, 4, 3, ob, p(fl), None) == 1 and err().endswith("bad range"), (k0, k1)
        for k0, k1 in ((-1, n), (5, 4)):
            assert unpack(h, k0, k1, p(v), fs, 0, 4, 3, ob, p(fl), None) == 1 and err().endswith("bad range"), (k0, k1)
        assert values(h, 0, n, p(v), ntencode - 1, 0, 4, 3, ob, p(fl), None) == 1 and err().endswith("bad range")      # fstride < ntencode
        assert unpack(h, 0, n, p(v), n - 1, 0, 4, 3, ob, p(fl), None) == 1 and err().endswith("bad range")      # ld < kijl
        # the field range: NANG NFRE_RED = 300 for the values form, NANG NFRE = 432 for the unpack form
        for f0, nf in ((-1, 4), (0, 0), (297, 4), (300, 1), (0, 301)):
            assert values(h, 0, n, p(v), fs, f0, nf, 3, ob, p(fl), None) == 1 and err().endswith("bad field range"), (f0, nf)
        for f0, nf in ((-1, 4), (0, 0), (429, 4), (432, 1), (0, 433)):
            assert unpack(h, 0, n, p(v), fs, f0, nf, 3, ob, p(fl), None) == 1 and err().endswith("bad field range"), (f0, nf)
        for call in (values, unpack):
            assert call(h, 0, n, p(v), fs, 0, 4, 4, ob, p(fl), None) == 1 and err().endswith("unknown flags")
            assert call(h, 0, n, p(v), fs, 0, 4, 7, ob, p(fl), None) == 1 and err().endswith("unknown flags")
            for flags in (1, 2, 3):
                assert call(h, 0, n, p(v), fs, 0, 4, flags, None, p(fl), None) == 1 and err().endswith("null options"), flags
            assert call(h, 0, n, None, fs, 0, 4, 3, ob, p(fl), None) == 1 and err().endswith("null pointer")
            assert call(h, 0, n, p(v), fs, 0, 4, 3, ob, None, None) == 1 and err().endswith("null pointer")
            assert call(h, 0, n, p(v), fs, 0, 4, 3, ob, off(fl, 4), None) == 1 and err().endswith("16-byte aligned")
            assert call(h, 0, 0, p(v), fs, 0, 4, 3, ob, off(fl, 8), None) == 1 and err().endswith("16-byte aligned")      # an empty range too
            assert call(h, 0, n, off(v, 2), fs, 0, 4, 3, ob, p(fl), None) == 1 and err().endswith("aligned to a real")
            # an empty range returns 0 and launches nothing, with null pointers too
            assert call(h, 7, 7, p(v), fs, 0, 4, 3, ob, p(fl), None) == 0
            assert call(h, 0, 0, None, fs, 0, 4, 0, None, None, None) == 0
        torch.cuda.synchronize()
        assert (fl == SENT).all()      # none of the refusals and empty ranges wrote anything
        # what the refusals border on is served: a source that begins at any real, the last fields of either form, flags = 0 without options
        assert values(h, 0, n, off(v, 4), ntencode, 296, 4, 0, None, p(fl), None) == 0
        assert unpack(h, 0, n, p(v), n, 428, 4, 0, None, p(fl), None) == 0
        torch.cuda.synchronize()
        got = fl.cpu().numpy()
        assert _untouched(got, list(range(296, 300)) + list(range(428, 432))) and (got[:, 8:, 24] == 0).all() and (got[:, 8:, 35] == 0).all()
    finally:
        ctx.close()
    # NFRE = 30 in single precision: 30 reals are no whole number of 16-byte pieces
    ctx = api.HipContext(Tables(Config(nang=12, nfre=30, nfre_red=30), np.float32))
    try:
        fl = torch.full((4, 12, 30), SENT, dtype=torch.float32, device=ctx.device)
        blk = torch.zeros((4, 4), dtype=torch.float32, device=ctx.device)
        with pytest.raises(api.EcwamHipError, match="no whole number of 16-byte chunks"):
            ctx.getspec_unpack(0, 4, blk, fl)
        ctx.set_grib_map(np.arange(4), 4, None)
        with pytest.raises(api.EcwamHipError, match="no whole number of 16-byte chunks"):
            ctx.getspec_values(0, 4, blk, fl)
        torch.cuda.synchronize()
        assert (fl == SENT).all()
    finally:
        ctx.close()


# ---- 7. a read captured in a graph replays bit-identically: the call path holds no allocation and no wait
def test_getspec_in_a_graph(api):
    g = R.grid_of("A_ice0")
    n = g["ixlg"].size
    full = _full("sp")
    ctx = _context(api, "sp", G.value_map(g))
    try:
        vd = _up(ctx, _vectors(), np.float32)
        fl = _sent(ctx, n)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            ctx.getspec_values(0, n, vd, fl)      # warm up on the side stream
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                ctx.getspec_values(0, n, vd[:120], fl)
                ctx.getspec_values(0, n, vd[120:], fl, ifld0=120)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            fl.fill_(SENT)
            graph.replay()
            torch.cuda.synchronize()
            assert _bits(fl.cpu().numpy(), full)
    finally:
        ctx.close()
