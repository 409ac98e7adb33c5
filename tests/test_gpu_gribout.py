"""ecwam_hip_set_grib_map / _outspec_values / _outspec_pack / _grib_values and the Wamintgr methods over them on the device (run with -m gpu),
against the reference's own WGRIBENCODE_VALUES: tests/golden/gribout_0.npz, recorded by tools/make_golden_gribout.py in both precisions, and
against the numpy restatement of tests/gribout_ref.py where the fixture does not reach (all 300 fields, row ranges, a second tile geometry).
Case A has 204 points on 292 cells: three tiles of 64 and a ragged fourth.

Gates (tests/gribout_ref.py::gate, from tests/golden/gribout_observed.json; nothing in them comes from the device), on the log scale, against
the DOUBLE precision fixture: double precision 4 x restatement_vs_reference_dp, floored at 4 eps of the value; single precision
4 x reference_sp_vs_dp.  Against the double precision restatement, where there is no fixture, the figure restatement_vs_reference_dp is added
(the restatement stands that far from the reference).  The pattern of ZMISS is compared exactly, everywhere, and no cell is left out.  What
involves no logarithm -- the path of the integrated parameters with its pole means and its scatter, the mask and the transposition of
outspec_pack -- is compared bit for bit with the restatement in the same precision.
"""
import ctypes as C
import functools

import numpy as np
import pytest

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


def _context(api, prec, g=None, nang=12, nfre_red=25):
    ctx = api.HipContext(G.tables(prec, nang, nfre_red))
    if g is not None:
        ctx.set_grib_map(*G.value_map(g))
    return ctx


def _up(ctx, a, T):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=T)).to(ctx.device)


@functools.lru_cache(maxsize=None)
def _restated(name, prec):
    """the restatement over all 300 fields, computed once"""
    return G.restate(name, prec, fields=list(range(NF)))


@functools.lru_cache(maxsize=None)
def _device_a(prec, ice):
    """case A through outspec_values, all fields: (values, ppmax), computed once and shared"""
    from ecwam_amd import api
    c = G.cached_cases()
    T = _T(prec)
    ctx = _context(api, prec, c["grid_a"])
    try:
        values = torch.full((NF, 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ppmax = torch.full((NF,), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.outspec_values(0, c["fl_a"].shape[0], _up(ctx, c["fl_a"], T), values, _up(ctx, G.ff_of(c["cic_a"], T), T), ice_mask=bool(ice), ppmax=ppmax)
        torch.cuda.synchronize()
        return values.cpu().numpy(), ppmax.cpu().numpy()
    finally:
        ctx.close()


def _hold(prec, what, got, ref_dp, extra=0.0):
    """got (device, working precision) against a double precision reference: the pattern exactly, the rest within the gate (+ extra)"""
    obs = G.observed()
    got, ref_dp = np.asarray(got, np.float64), np.asarray(ref_dp, np.float64)
    assert got.shape == ref_dp.shape
    miss = ref_dp == G.ZMISS
    assert np.array_equal(got == G.ZMISS, miss), f"{what}: the patterns of ZMISS differ at {int(((got == G.ZMISS) != miss).sum())} places"
    kind = "ppmax" if what.endswith("ppmax") else "values"
    lim = G.gate(prec, obs, ref_dp, kind) + extra
    err = np.where(miss, 0.0, np.abs(got - ref_dp))
    worst = float((err / lim).max()) if err.size else 0.0
    print(f"{what} {prec}: largest difference {float(err.max()):.3e}, {worst:.3f} of its gate ({float(lim.min()):.3e} .. {float(lim.max()):.3e})")
    assert float(lim.max()) <= G.OPTS["ppresol"] / 100      # a gate above this would not be a matter of rounding
    assert (err <= lim).all(), what


# ---- 1. case A: the fixture (48 fields) and the restatement (300), both values of the ice flag
@pytest.mark.parametrize("ice", [0, 1])
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_case_a_against_the_reference(prec, ice, api):
    gold, obs = G.load_golden(), G.observed()
    values, ppmax = _device_a(prec, ice)
    assert not (values == SENT).any() and not (ppmax == SENT).any()      # every cell of every field is written
    rec = G.recorded_fields()
    _hold(prec, f"A_ice{ice} values", values[rec], gold[f"A_ice{ice}_dp"])
    _hold(prec, f"A_ice{ice} ppmax", ppmax[rec], gold[f"A_ice{ice}_ppmax_dp"])
    rv, rp = _restated(f"A_ice{ice}", "dp")
    _hold(prec, f"A_ice{ice} all fields values", values, rv, obs["restatement_vs_reference_dp"]["values"])
    _hold(prec, f"A_ice{ice} all fields ppmax", ppmax, rp, obs["restatement_vs_reference_dp"]["ppmax"])
    # a pole row holds one number per field
    assert (values[:, :6] == values[:, :1]).all() and (values[:, 286:] == values[:, 286:287]).all()


# ---- 2. the two halves of the many-task path: bit-identical to the one-task call, and the send buffer to the restatement
@pytest.mark.parametrize("ice", [0, 1])
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_pack_then_grib_values_is_outspec_values(prec, ice, api):
    c = G.cached_cases()
    T = _T(prec)
    n = c["fl_a"].shape[0]
    ld = n + 3
    ctx = _context(api, prec, c["grid_a"])
    try:
        blk = torch.full((NF, ld), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.outspec_pack(0, n, _up(ctx, c["fl_a"], T), blk, _up(ctx, G.ff_of(c["cic_a"], T), T), ice_mask=bool(ice))
        values = torch.full((NF, 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ppmax = torch.full((NF,), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.grib_values(0, n, blk, values, True, ppmax=ppmax)
        torch.cuda.synchronize()
        b = blk.cpu().numpy()
        fl = c["fl_a"].astype(T)
        want = G.fields_of(G.ice_mask(fl, c["cic_a"], G.tables(prec)) if ice else fl, range(NF), 12)
        assert _bits(b[:, :n], want) and (b[:, n:] == SENT).all()
        v1, p1 = _device_a(prec, ice)
        assert _bits(values.cpu().numpy(), v1) and _bits(ppmax.cpu().numpy(), p1)
    finally:
        ctx.close()


# ---- 3. field ranges: each bit-identical to the same fields of the full call
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_field_ranges(prec, api):
    c = G.cached_cases()
    T = _T(prec)
    n = c["fl_a"].shape[0]
    full_v, full_p = _device_a(prec, 1)
    ctx = _context(api, prec, c["grid_a"])
    try:
        fl, ff = _up(ctx, c["fl_a"], T), _up(ctx, G.ff_of(c["cic_a"], T), T)
        # one field; the last five; inside one frequency (fields 36 .. 47 are frequency 4); across three frequencies; from the middle of a 16-byte piece
        for f0, nf in ((7, 1), (295, 5), (38, 5), (20, 30), (66, 100)):
            values = torch.full((nf, 292), SENT, dtype=ctx.dtype, device=ctx.device)
            ppmax = torch.full((nf,), SENT, dtype=ctx.dtype, device=ctx.device)
            blk = torch.full((nf, n), SENT, dtype=ctx.dtype, device=ctx.device)
            ctx.outspec_values(0, n, fl, values, ff, ifld0=f0, nfld=nf, ice_mask=True, ppmax=ppmax)
            ctx.outspec_pack(0, n, fl, blk, ff, ifld0=f0, ice_mask=True)
            torch.cuda.synchronize()
            assert _bits(values.cpu().numpy(), full_v[f0:f0 + nf]) and _bits(ppmax.cpu().numpy(), full_p[f0:f0 + nf]), (f0, nf)
            assert _bits(blk.cpu().numpy(), G.fields_of(G.ice_mask(c["fl_a"].astype(T), c["cic_a"], G.tables(prec)), range(f0, f0 + nf), 12)), (f0, nf)
    finally:
        ctx.close()


# ---- 4. row ranges: the cells of the other rows keep what they held; the rest is the restatement restricted to the rows
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_row_range(prec, api):
    c = G.cached_cases()
    T = _T(prec)
    g = c["grid_a"]
    n = c["fl_a"].shape[0]
    rows = (3, n - 5)
    fields = list(range(100, 160))
    obs = G.observed()
    ctx = _context(api, prec, g)
    try:
        values = torch.full((len(fields), 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ppmax = torch.full((len(fields),), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.outspec_values(rows[0], rows[1], _up(ctx, c["fl_a"], T), values, _up(ctx, G.ff_of(c["cic_a"], T), T), ifld0=fields[0], nfld=len(fields),
                           ice_mask=True, ppmax=ppmax)
        torch.cuda.synchronize()
        got = values.cpu().numpy()
        w = G.written_cells(g, rows)
        assert 0 < (~w).sum() <= 8 and (got[:, ~w] == SENT).all()      # the eight rows left out, less those on a pole row, which the padding writes
        blk = G.fields_of(G.ice_mask(c["fl_a"].astype(np.float64), c["cic_a"], G.tables("dp")), fields, 12)
        rv, rp = G.encode(blk, g, np.float64, True, rows=rows)
        _hold(prec, "rows [3, n - 5) values", got[:, w], rv[:, w], obs["restatement_vs_reference_dp"]["values"])
        _hold(prec, "rows [3, n - 5) ppmax", ppmax.cpu().numpy(), rp, obs["restatement_vs_reference_dp"]["ppmax"])
    finally:
        ctx.close()


# ---- 5. case B (a regular grid: the start offset and the prefill) and case C (no logarithm: bit for bit)
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_case_b_against_the_reference(prec, api):
    c, gold = G.cached_cases(), G.load_golden()
    T = _T(prec)
    n = c["fl_b"].shape[0]
    ctx = _context(api, prec, c["grid_b"])
    try:
        values = torch.full((G.B_FIELDS[1], 88), SENT, dtype=ctx.dtype, device=ctx.device)
        ppmax = torch.full((G.B_FIELDS[1],), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.outspec_values(0, n, _up(ctx, c["fl_b"], T), values, ifld0=G.B_FIELDS[0], nfld=G.B_FIELDS[1], ppmax=ppmax)
        torch.cuda.synchronize()
        _hold(prec, "B values", values.cpu().numpy(), gold["B_dp"])
        _hold(prec, "B ppmax", ppmax.cpu().numpy(), gold["B_ppmax_dp"])
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_case_c_bit_for_bit(prec, api):
    c, gold = G.cached_cases(), G.load_golden()
    T = _T(prec)
    n = c["bout"].shape[0]
    ctx = _context(api, prec, c["grid_a"])
    try:
        bout = _up(ctx, c["bout"], T)
        values = torch.full((7, 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.grib_values(0, n, bout, values, False, columns=range(7))      # one run of seven columns of BOUT as it stands
        some = torch.full((3, 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.grib_values(0, n, bout, some, False, columns=[5, 0, 1])      # two runs
        major = torch.full((7, 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.grib_values(0, n, bout.T.contiguous(), major, False)         # the same block, field-major
        torch.cuda.synchronize()
        ref = gold[f"C_{prec}"]
        assert _bits(values.cpu().numpy(), ref) and _bits(major.cpu().numpy(), ref) and _bits(some.cpu().numpy(), ref[[5, 0, 1]])
        assert _bits(ref, G.restate("C", prec)[0])
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_outint_from_the_bout_of_outblock(prec, api):
    """Wamintgr.outint on the BOUT its own outblock() leaves: the scatter of the columns swh and mwd, and nothing else but ZMISS."""
    from ecwam_amd import grid as grid_mod
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    m = Wamintgr(Config(nang=12, nfre=36, nfre_red=36, idelt=450, idelpro=450), grid_mod.build_grid(16, mask="continents"), prec)
    try:
        m.init_synthetic(seed=3)
        with pytest.raises(RuntimeError, match="set_grib_map"):
            m.outint(["swh"])
        m.set_grib_map()
        with pytest.raises(RuntimeError, match="outblock"):
            m.outint(["swh"])
        bout, cols = m.outblock([1, 2, 3, 6])
        values = m.outint(["mwd", "swh"])
        torch.cuda.synchronize()
        g = m.grid
        assert m.ntencode == int(g.nlonrgg.sum()) and tuple(values.shape) == (2, m.ntencode)
        start = np.concatenate([[0], np.cumsum(g.nlonrgg[::-1])])      # row J (north first) of VALUES
        ival = start[g.ngy - 1 - g.kxlt] + g.ixlg
        want = np.full((2, m.ntencode), G.ZMISS, _T(prec))
        b = bout.cpu().numpy()
        want[0, ival], want[1, ival] = b[:, cols[2]], b[:, cols[1]]
        assert _bits(values.cpu().numpy(), want) and (want != G.ZMISS).sum() > m.n // 2
    finally:
        m.ctx.close()


# ---- 6. a second tile geometry: NANG = 36, NFRE_RED = 29 (the pitch of the tile, the pieces per direction and the last piece, cut at NFRE_RED, all change)
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_second_geometry(prec, api):
    s = G.second_geometry()
    T = _T(prec)
    g, n, nf = s["grid"], s["fl"].shape[0], 36 * 29
    obs = G.observed()
    ctx = _context(api, prec, g, 36, 29)
    try:
        values = torch.full((nf, 292), SENT, dtype=ctx.dtype, device=ctx.device)
        ppmax = torch.full((nf,), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.outspec_values(0, n, _up(ctx, s["fl"], T), values, _up(ctx, G.ff_of(s["cic"], T), T), ice_mask=True, ppmax=ppmax)
        torch.cuda.synchronize()
        blk = G.fields_of(G.ice_mask(s["fl"].astype(np.float64), s["cic"], G.tables("dp", 36, 29)), range(nf), 36)
        rv, rp = G.encode(blk, g, np.float64, True)
        _hold(prec, "36 x 29 values", values.cpu().numpy(), rv, obs["restatement_vs_reference_dp"]["values"])
        _hold(prec, "36 x 29 ppmax", ppmax.cpu().numpy(), rp, obs["restatement_vs_reference_dp"]["ppmax"])
    finally:
        ctx.close()


# ---- 7. refusals, by the text of ecwam_hip_last_error, and the empty range
def test_refusals(api):
    from ecwam_amd import lib

    c = G.cached_cases()
    g = c["grid_a"]
    ival, ntencode, poles = G.value_map(g)
    n = ival.size
    ctx = _context(api, "sp")
    h, L = ctx._h, ctx.lib
    err = lambda: L.ecwam_hip_last_error().decode()
    try:
        dev = ctx.device
        fl = torch.zeros((n, 12, 36), dtype=torch.float32, device=dev)
        ff = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        values = torch.full((4, ntencode + 4), SENT, dtype=torch.float32, device=dev)
        ppmax = torch.full((4,), SENT, dtype=torch.float32, device=dev)
        o = lib.GribOpts(-3.0, 1e-10, 0.0, 0.002, 0.0, 9, -999.0)
        ob = C.byref(o)
        p = lambda t: C.c_void_p(t.data_ptr())
        iv = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.c_void_p)
        pl = lambda *a: C.byref(lib.GribPoles(lib.GribPole(*a[:4]), lib.GribPole(*a[4:])))
        # no map yet
        assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), p(ff), 0, 4, 0, ob, p(values), p(ppmax), None) == 1 and err().endswith("no grib map")
        assert L.ecwam_hip_grib_values(h, 0, n, p(fl), 1, 1, 1, 0, ob, p(values), None, None) == 1 and err().endswith("no grib map")
        # the map itself
        bad = ival.copy()
        bad[5] = ntencode
        assert L.ecwam_hip_set_grib_map(h, n, iv(bad), ntencode, None) == 1 and "index 5 outside [0, ntencode)" in err()
        bad[5] = -1
        assert L.ecwam_hip_set_grib_map(h, n, iv(bad), ntencode, None) == 1 and "index 5 outside" in err()
        bad[5] = ival[2]
        assert L.ecwam_hip_set_grib_map(h, n, iv(bad), ntencode, None) == 1 and "index 5 is a duplicate" in err()
        assert L.ecwam_hip_set_grib_map(h, n, iv(ival), ntencode, pl(0, 6, 4, 12, 0, 0, 0, 0)) == 1 and err().endswith("the pole ranges overlap")
        assert L.ecwam_hip_set_grib_map(h, n, iv(ival), ntencode, pl(0, 6, 6, 12, 286, 6, 12, 12)) == 1 and err().endswith("the pole ranges overlap")
        assert L.ecwam_hip_set_grib_map(h, n, iv(ival), ntencode, pl(0, 6, 6, 12, 288, 6, 274, 12)) == 1 and err().endswith("a pole range leaves the vector")
        assert L.ecwam_hip_set_grib_map(h, n, iv(ival), ntencode, pl(0, -1, 6, 12, 0, 0, 0, 0)) == 1 and "negative length" in err()
        assert L.ecwam_hip_set_grib_map(h, n, iv(ival), 0, None) == 1 and "NTENCODE" in err()
        assert L.ecwam_hip_set_grib_map(h, -1, iv(ival), ntencode, None) == 1 and "negative count" in err()
        assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), p(ff), 0, 4, 0, ob, p(values), p(ppmax), None) == 1 and err().endswith("no grib map")      # still none
        ctx.set_grib_map(ival, ntencode, poles)
        ok = lambda: L.ecwam_hip_outspec_values(h, 0, n, p(fl), p(ff), 0, 4, 1, ob, p(values), p(ppmax), None)
        assert ok() == 0
        # the calls on rows
        assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), p(ff), 0, 4, 1, None, p(values), p(ppmax), None) == 1 and err().endswith("null options")
        assert L.ecwam_hip_grib_values(h, 0, n, p(fl), 1, 1, 1, 0, None, p(values), None, None) == 1 and err().endswith("null options")
        for f0, nf in ((-1, 4), (0, 0), (297, 4), (300, 1), (0, 301)):
            assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), p(ff), f0, nf, 0, ob, p(values), p(ppmax), None) == 1 and err().endswith("bad field range"), (f0, nf)
            assert L.ecwam_hip_outspec_pack(h, 0, n, p(fl), p(ff), f0, nf, 0, p(values), n, None) == 1 and err().endswith("bad field range"), (f0, nf)
        assert L.ecwam_hip_grib_values(h, 0, n, p(fl), 1, 1, 301, 1, ob, p(values), None, None) == 1 and err().endswith("bad field range")
        assert L.ecwam_hip_outspec_pack(h, 0, n, p(fl), p(ff), 0, 4, 0, p(values), n - 1, None) == 1 and err().endswith("bad range")      # ld < kijl
        for k0, k1 in ((-1, n), (5, 4), (0, n + 1)):
            assert L.ecwam_hip_outspec_values(h, k0, k1, p(fl), p(ff), 0, 4, 0, ob, p(values), p(ppmax), None) == 1 and err().endswith("bad range"), (k0, k1)
            assert L.ecwam_hip_grib_values(h, k0, k1, p(fl), 1, 1, 1, 0, ob, p(values), None, None) == 1 and err().endswith("bad range"), (k0, k1)
        off = lambda t, b: C.c_void_p(t.data_ptr() + b)
        assert L.ecwam_hip_outspec_values(h, 0, n, off(fl, 4), p(ff), 0, 4, 0, ob, p(values), p(ppmax), None) == 1 and err().endswith("16-byte aligned")
        assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), p(ff), 0, 4, 0, ob, off(values, 8), p(ppmax), None) == 1 and err().endswith("16-byte aligned")
        assert L.ecwam_hip_outspec_values(h, 0, 0, off(fl, 4), p(ff), 0, 4, 0, ob, p(values), p(ppmax), None) == 1 and err().endswith("16-byte aligned")      # empty range too
        assert L.ecwam_hip_outspec_pack(h, 0, n, p(fl), p(ff), 0, 4, 0, off(values, 4), n, None) == 1 and err().endswith("16-byte aligned")
        assert L.ecwam_hip_grib_values(h, 0, n, off(fl, 2), 1, 1, 1, 0, ob, p(values), None, None) == 1 and err().endswith("aligned to a real")
        assert L.ecwam_hip_outspec_values(h, 0, n, None, p(ff), 0, 4, 0, ob, p(values), p(ppmax), None) == 1 and err().endswith("null pointer")
        assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), None, 0, 4, 1, ob, p(values), p(ppmax), None) == 1 and err().endswith("null pointer")      # the mask reads ff
        assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), None, 0, 4, 0, ob, p(values), None, None) == 0      # ... and only the mask; ppmax is optional
        assert L.ecwam_hip_outspec_values(h, 0, n, p(fl), p(ff), 0, 4, 2, ob, p(values), p(ppmax), None) == 1 and err().endswith("unknown flags")
        assert L.ecwam_hip_grib_values(h, 0, n, p(fl), 1, 1, 1, 2, ob, p(values), None, None) == 1 and "spectral must be 0 or 1" in err()
        assert L.ecwam_hip_grib_values(h, 0, n, p(fl), 0, 1, 1, 0, ob, p(values), None, None) == 1 and "strides" in err()
        o.ngrbress = 31
        assert ok() == 1 and "NGRBRESS" in err()
        o.ngrbress = 9
        # an empty range returns 0 and touches nothing
        torch.cuda.synchronize()
        values.fill_(SENT)
        ppmax.fill_(SENT)
        assert L.ecwam_hip_outspec_values(h, 7, 7, p(fl), p(ff), 0, 4, 1, ob, p(values), p(ppmax), None) == 0
        assert L.ecwam_hip_outspec_values(h, 0, 0, None, None, 0, 4, 1, ob, None, None, None) == 0
        assert L.ecwam_hip_outspec_pack(h, 7, 7, p(fl), p(ff), 0, 4, 1, p(values), n, None) == 0
        assert L.ecwam_hip_grib_values(h, 7, 7, p(fl), 1, 1, 4, 1, ob, p(values), p(ppmax), None) == 0
        torch.cuda.synchronize()
        assert (values == SENT).all() and (ppmax == SENT).all()
    finally:
        ctx.close()


# ---- 8. two consecutive outspec() calls captured in a graph replay bit-identically: the call path holds no allocation and no wait
@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_outspec_in_a_graph(prec, api):
    from ecwam_amd import grid as grid_mod
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    m = Wamintgr(Config(nang=12, nfre=36, nfre_red=29, idelt=450, idelpro=450, licerun=True, lmaskice=True), grid_mod.build_grid(16, mask="continents"), prec)
    try:
        m.init_synthetic(seed=3)
        m.set_grib_map()
        nf = 12 * 29
        eager, pe = m.outspec()
        lo, plo = m.outspec(fields=(0, 100))
        torch.cuda.synchronize()
        assert tuple(eager.shape) == (nf, m.ntencode) and torch.equal(lo, eager[:100]) and torch.equal(plo, pe[:100])
        v1, p1 = torch.full_like(eager, SENT), torch.full_like(pe, SENT)
        v2, p2 = torch.full_like(eager[:100], SENT), torch.full_like(pe[:100], SENT)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            m.outspec(values=v1, ppmax=p1)      # warm up on the side stream
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                m.outspec(values=v1, ppmax=p1)
                m.outspec(fields=(0, 100), values=v2, ppmax=p2)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            for t in (v1, p1, v2, p2):
                t.fill_(SENT)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(v1, eager) and torch.equal(p1, pe) and torch.equal(v2, eager[:100]) and torch.equal(p2, pe[:100])
        # the spectra changed: the replay follows them
        m.fl1.mul_(2.0)
        graph.replay()
        torch.cuda.synchronize()
        again, _ = m.outspec()
        assert torch.equal(v1, again) and not torch.equal(v1, eager)
    finally:
        m.ctx.close()
