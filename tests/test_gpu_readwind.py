"""ecwam_hip_set_input_grid / _grib2wgrid / _current2wam and the Wamintgr methods over them on the device (run with -m gpu), against the
reference's own results: tests/golden/readwind_0.npz, recorded by tools/make_golden_readwind.py from the reference's unmodified GRIB2WGRID behind a
stand-in decoder, in both precisions (READWIND's fill and CURRENT2WAM's statements restated in the driver around its FIELD).  The 11 x 9 reduced
wave grid, 99 cells: no whole number of wavefronts or of 16-byte pieces; input grids A (periodic reduced Gaussian, north to south), B (regional:
padded rows, LLSKIP, the II1 clamp), C (the model's own grid, LLINTERPOL = F) and D (A scanned south to north).

The table is that of ecwam_amd/readwind.py.  A field that is no direction is the reference's bit for bit wherever the numpy restatement was
(tests/golden/readwind_observed.json: the same IEEE operations in the same order, no contraction); elsewhere, and for directions (SIN, COS, ATAN2
of the device library; compared on the circle), the gates are tests/readwind_ref.py::device_gate -- dp 10 x what the restatement showed against
the reference (directions: a floor of 8 eps of the period), sp 3 x the reference's own single-against-double difference.  Nothing in a gate comes
from the device; what the device measured is in profiles/readwind_device.txt.
"""
import ctypes as C

import numpy as np
import pytest

import readwind_ref as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RANGES = {"one": [(F.KIJS, F.KIJL)], "two": [(F.KIJS, F.SPLIT), (F.SPLIT, F.KIJL)]}
FIELD_KEYS = ("plain", "miss", "dir", "ucur", "vcur")      # the messages whose FIELD the fixture holds


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _context(api, name, prec, slot=0, cells=None):
    ctx = api.HipContext(F.tables(prec))
    ctx.set_forcing_map(F.cached_cases()["map_in"], F.NCELL)
    _set(ctx, name, prec, slot, cells)
    return ctx


def _set(ctx, name, prec, slot=0, cells=None):
    tab = F.table(name, prec)[1]
    s = slice(None) if cells is None else slice(0, cells)
    ctx.set_input_grid(slot, tab["pos"][s], None if tab["w"] is None else tab["w"][s], tab["kind"][s], tab["nvalues"], tab["interpol"])
    return tab


def _up(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F.dtype_of("sp" if ctx.dtype == torch.float32 else "dp"))).to(ctx.device)


def _msgs(name, keys):
    m = {k: (fl, v) for k, _, _, fl, v in F.messages(F.cached_cases(), name)}
    return [m[k] for k in keys]


def _check(name, key, prec, got, ref, bad):
    gate = F.device_gate(name, key, prec)
    err = F.error(key, got, ref)
    print(f"{name} {key} {prec}: device against the reference {err:.3e} (gate {'the same bits' if gate is None else format(gate, '.3e')})")
    if not F.same_pattern(got, ref):
        bad[key] = "the pattern of PMISS differs"
    elif gate is None:
        if not _same_bits(got, ref):
            bad[key] = ("bits differ", err)
    elif not err <= gate:
        bad[key] = (err, gate)


def _fieldg(ctx, ncell=F.NCELL):
    """fieldg [13][ncell] full of sentinels, with four sentinel reals behind it: (the whole buffer, the view)"""
    buf = torch.full((13 * ncell + 4,), F.SENT, dtype=ctx.dtype, device=ctx.device)
    return buf, buf[:13 * ncell].view(13, ncell)


# ---- 1. FIELD as GRIB2WGRID returns it
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", F.CASES)
def test_field_against_the_reference(api, name, prec):
    ref = F.golden_case(name, prec)
    T = F.dtype_of(prec)
    ctx = _context(api, name, prec)
    bad = {}
    try:
        msgs = _msgs(name, FIELD_KEYS)
        values = _up(ctx, np.stack([v for _, v in msgs]))
        out = torch.full((len(msgs), 100), F.SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.grib2wgrid(0, values, [(F.FIELD, fl) for fl, _ in msgs], out=out, pmiss=F.PMISS)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:, F.NCELL:] == T(F.SENT)).all() and (got[:, :F.NCELL] != T(F.SENT)).all()      # every cell is written, nothing behind them
        kind = F.table(name, prec)[1]["kind"]
        assert (got[:, :F.NCELL][:, kind != 2] == T(F.PMISS)).all()
        for i, key in enumerate(FIELD_KEYS):
            _check(name, key, prec, got[i, :F.NCELL], ref[key if key in F.FIELDS else "field_" + key], bad)
    finally:
        ctx.close()
    assert not bad, bad


# ---- 2. READWIND's eight parameters in one call
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", F.CASES)
def test_readwind_fills_fieldg(api, name, prec):
    ref = F.golden_case(name, prec)["fieldg"]
    T = F.dtype_of(prec)
    planes = [p for p, *_ in F.READWIND]
    ctx = _context(api, name, prec)
    bad = {}
    try:
        msgs = _msgs(name, ["fg_" + p for p in planes])
        values = _up(ctx, np.stack([v for _, v in msgs]))
        buf, fieldg = _fieldg(ctx)
        ctx.grib2wgrid(0, values, [(p, fl) for p, (fl, _) in zip(planes, msgs)], fieldg=fieldg, roair=F.ROAIR, wstar0=F.WSTAR0, pmiss=F.PMISS)
        torch.cuda.synchronize()
        got = fieldg.cpu().numpy()
        # the planes no message targets, the cells of kind 0 and what lies behind the buffer keep their bits -- as in the reference
        assert np.array_equal(got == T(F.SENT), ref == T(F.SENT)) and bool((buf[13 * F.NCELL:] == F.SENT).all())
        kind = F.table(name, prec)[1]["kind"]
        for p in ("USTRA", "VSTRA", "LKFR", "UCUR", "VCUR"):
            assert (got[F.FG[p]] == T(F.SENT)).all(), p
        for p in planes:
            assert (got[F.FG[p], kind == 0] == T(F.SENT)).all() and (got[F.FG[p], kind != 0] != T(F.SENT)).all(), p
            _check(name, "fg_" + p, prec, got[F.FG[p]], ref[F.FG[p]], bad)
        # eight calls of one field give the bits of the one call of eight
        buf1, one = _fieldg(ctx)
        for i, p in enumerate(planes):
            ctx.grib2wgrid(0, values[i:i + 1].clone(), [(p, msgs[i][0])], fieldg=one, roair=F.ROAIR, wstar0=F.WSTAR0, pmiss=F.PMISS)
        torch.cuda.synchronize()
        assert _same_bits(buf1.cpu().numpy(), buf.cpu().numpy())
    finally:
        ctx.close()
    assert not bad, bad


# ---- 3. CURRENT2WAM's statements: copies, compares, SIGN and MIN -- the reference's bits
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", F.CASES)
def test_current2wam(api, name, prec):
    ref = F.golden_case(name, prec)
    T = F.dtype_of(prec)
    ctx = api.HipContext(F.tables(prec))
    try:
        ctx.set_forcing_map(F.cached_cases()["map_in"], F.NCELL)
        fu, fv = _up(ctx, ref["field_ucur"]), _up(ctx, ref["field_vcur"])
        A = slice(F.KIJS, F.KIJL)

        def run(ranges, u=fu, v=fv):
            uc = torch.full((F.NROW,), F.SENT, dtype=ctx.dtype, device=ctx.device)
            vc = torch.full((F.NROW,), F.SENT, dtype=ctx.dtype, device=ctx.device)
            ch = torch.zeros(1, dtype=torch.int32, device=ctx.device)
            for k0, k1 in ranges:
                ctx.current2wam(k0, k1, u, v, uc, vc, F.WLOWEST, F.PMISS, ch)
            torch.cuda.synchronize()
            return uc, vc, ch
        uc, vc, ch = run(RANGES["one"])
        gu, gv = uc.cpu().numpy(), vc.cpu().numpy()
        assert _same_bits(gu[A], ref["ucur"][A]) and _same_bits(gv[A], ref["vcur"][A])
        assert (gu[:F.KIJS] == T(F.SENT)).all() and (gv[:F.KIJS] == T(F.SENT)).all()      # the rows outside the range
        assert int(ch.item()) == 1
        assert (gu[A] == 0).any() and (np.abs(gu[A]) == F.CURRENT_MAX).any() and (np.abs(gu[A]) < F.CURRENT_MAX).any()
        ch.zero_()      # an identical second call changes nothing
        ctx.current2wam(F.KIJS, F.KIJL, fu, fv, uc, vc, F.WLOWEST, F.PMISS, ch)
        torch.cuda.synchronize()
        assert int(ch.item()) == 0 and _same_bits(uc.cpu().numpy(), gu) and _same_bits(vc.cpu().numpy(), gv)
        u2, v2, _ = run(RANGES["two"])
        assert _same_bits(u2.cpu().numpy(), gu) and _same_bits(v2.cpu().numpy(), gv)
        # a component that is not given is left alone, and its current may be missing too
        u3, v3, ch3 = run(RANGES["one"], v=None)
        assert _same_bits(u3.cpu().numpy(), gu) and (v3.cpu().numpy() == T(F.SENT)).all() and int(ch3.item()) == 1
        ch3.zero_()
        ctx.current2wam(F.KIJS, F.KIJL, None, fv, None, v3, F.WLOWEST, F.PMISS, ch3)
        torch.cuda.synchronize()
        assert _same_bits(v3.cpu().numpy(), gv) and int(ch3.item()) == 1
    finally:
        ctx.close()


# ---- 4. small tables: planes that begin inside a 16-byte piece
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_tables_of_few_cells_are_slices_of_the_whole(api, name, prec):
    planes = [p for p, *_ in F.READWIND]
    msgs = _msgs(name, ["fg_" + p for p in planes] + ["miss"])
    fields = [(p, fl) for p, (fl, _) in zip(planes, msgs)] + [(F.FIELD, msgs[-1][0])]
    ctx = _context(api, name, prec)
    try:
        values = _up(ctx, np.stack([v for _, v in msgs]))

        def run(n):
            buf, fieldg = _fieldg(ctx, n)
            out = torch.full((len(fields), n), F.SENT, dtype=ctx.dtype, device=ctx.device)
            ctx.grib2wgrid(0, values, fields, out=out, fieldg=fieldg, roair=F.ROAIR, wstar0=F.WSTAR0, pmiss=F.PMISS)
            torch.cuda.synchronize()
            assert bool((buf[13 * n:] == F.SENT).all()) and bool((out[:len(planes)] == F.SENT).all())      # rows of out no FIELD targets
            return fieldg.cpu().numpy(), out[-1].cpu().numpy()
        whole = run(F.NCELL)
        for n in (1, 2, 64):
            _set(ctx, name, prec, 0, n)
            fg, f = run(n)
            assert _same_bits(fg, whole[0][:, :n]) and _same_bits(f, whole[1][:n]), n
    finally:
        ctx.close()


# ---- 5. refusals, with their words and their order, each before any launch
class Raw:
    """A context through ctypes (ecwam_amd.api validates before the library does) and one small device buffer for every pointer."""

    def __init__(self, prec):
        from ecwam_amd import lib as L

        self.L = L
        self.lib = L.load()
        t = F.tables(prec)
        params = L.make_params(t)
        tp, keep = L.make_tables(t)
        self.h = C.c_void_p()
        rc = self.lib.ecwam_hip_create(C.byref(params), C.byref(tp), 4 if prec == "sp" else 8, 0, C.byref(self.h))
        assert rc == 0, self.lib.ecwam_hip_last_error().decode()
        self.buf = torch.full((64 * 64,), F.SENT, dtype=torch.float64, device="cuda:0")
        self.a = self.buf.data_ptr()

    def err(self, rc):
        return rc, self.lib.ecwam_hip_last_error().decode()

    def set_map(self, inbound, ncell=8):
        m = None if inbound is None else np.ascontiguousarray(inbound, np.int32)
        return self.err(self.lib.ecwam_hip_set_forcing_map(self.h, 8, None if m is None else m.ctypes.data_as(C.c_void_p), ncell, None, 0))

    def set_grid(self, slot=0, ncell=8, nvalues=20, pos="ok", w="ok", kind="ok", interpol=1):
        rows = ncell if ncell > 0 else 8
        p_ = np.ascontiguousarray(np.arange(4 * rows).reshape(rows, 4) % 20 if isinstance(pos, str) else pos, np.int32) if pos is not None else None
        w_ = np.zeros((rows, 3)) if isinstance(w, str) else w
        k_ = np.full(rows, 2, np.int32) if isinstance(kind, str) else (None if kind is None else np.ascontiguousarray(kind, np.int32))
        p = lambda m: None if m is None else m.ctypes.data_as(C.c_void_p)
        return self.err(self.lib.ecwam_hip_set_input_grid(self.h, slot, ncell, nvalues, p(p_), p(w_), p(k_), interpol))

    def g2w(self, slot=0, values="a", vstride=20, nfld=1, desc=((0, 0),), out="a", ld=8, fieldg="a", ncell_in=8):
        values, out, fieldg = (self.a if p == "a" else p for p in (values, out, fieldg))
        d = None
        if desc is not None:
            d = (self.L.G2wField * 17)()
            for i, (t, fl) in enumerate(desc):
                d[i].target, d[i].flags = t, fl
        return self.err(self.lib.ecwam_hip_grib2wgrid(self.h, slot, values, vstride, nfld, d, 1.225, 0.0, -999.0, out, ld, fieldg, ncell_in, None))

    def c2w(self, kijs=0, kijl=0, **p):
        g = lambda k: p.get(k, self.a)
        return self.err(self.lib.ecwam_hip_current2wam(self.h, kijs, kijl, g("fu"), g("fv"), 1e-4, -999.0, g("ucur"), g("vcur"), p.get("changed"), None))

    def close(self):
        self.lib.ecwam_hip_destroy(self.h)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_refusals(api, prec):
    """Every refusal comes before anything is launched: the buffer all of them were given keeps its sentinels.  To see that, the table accepted
    last has no cells, so that the accepted calls launch nothing either."""
    c = Raw(prec)
    a = c.a
    S, G, W = "ecwam_hip_set_input_grid", "ecwam_hip_grib2wgrid", "ecwam_hip_current2wam"
    try:
        # the setter: the range (the slot), then its own, and a refused table leaves the one before it
        assert c.g2w() == (1, G + ": no table")
        assert c.set_grid(slot=4) == (1, S + ": bad range") and c.set_grid(slot=-1, ncell=-1) == (1, S + ": bad range")
        assert c.set_grid(ncell=-1) == (1, S + ": negative count")
        assert c.set_grid(nvalues=0) == (1, S + ": the message needs at least one value")
        assert c.set_grid(kind=None) == (1, S + ": null pointer")
        assert c.set_grid(w=None) == (1, S + ": the interpolation needs its weights")
        assert c.set_grid(ncell=0)[0] == 0 and c.g2w(ncell_in=0, ld=0)[0] == 0      # a table without cells: the call launches nothing
        bad = np.arange(32).reshape(8, 4) % 20
        bad[3, 2] = 20
        assert c.set_grid(pos=bad) == (1, S + ": position 2 of cell 3 outside [-1, nvalues)")
        bad[3, 2] = -2
        assert c.set_grid(pos=bad) == (1, S + ": position 2 of cell 3 outside [-1, nvalues)")
        bad[3, 2] = -1      # a padded row
        kinds = np.full(8, 2)
        kinds[5] = 3
        assert c.set_grid(pos=bad, kind=kinds) == (1, S + ": kind of cell 5 outside 0 .. 2")
        kinds[5] = -1
        assert c.set_grid(pos=bad, kind=kinds) == (1, S + ": kind of cell 5 outside 0 .. 2")
        bad[3, 0] = -1      # without interpolation a cell of kind 2 needs its value; one of kind 1 does not
        assert c.set_grid(pos=bad, w=None, interpol=0) == (1, S + ": position 0 of cell 3 outside [0, nvalues)")
        nan = np.zeros((8, 3))
        nan[2, 1] = np.inf
        assert c.set_grid(w=nan) == (1, S + ": weight 1 of cell 2 is not finite")
        tenth = np.full((8, 3), 0.1)      # a double that no float holds: single precision would not narrow it back unchanged
        if prec == "sp":
            assert c.set_grid(w=tenth) == (1, S + ": weight 0 of cell 0 is not a value of the working precision")
        assert c.g2w(ncell_in=0, ld=0)[0] == 0      # all of these left the table without cells
        assert c.set_grid(slot=3, ncell=0)[0] == 0 and c.set_grid(slot=3, pos=None)[0] == 0 and c.g2w(slot=3) == (1, G + ": no table")
        # GRIB2WGRID: the range, its own refusals in the header's order, the buffers
        assert c.g2w(slot=4, nfld=0) == (1, G + ": bad range")
        assert c.g2w(slot=1, nfld=0) == (1, G + ": no table")
        assert c.g2w(vstride=19, nfld=0) == (1, G + ": vstride is 19, the table's nvalues 20")
        assert c.g2w(nfld=0, desc=None) == (1, G + ": nfld outside 1 .. 16") and c.g2w(nfld=17) == (1, G + ": nfld outside 1 .. 16")
        assert c.g2w(desc=None) == (1, G + ": null descriptors")
        assert c.g2w(desc=((0, 4),)) == (1, G + ": unknown flags of field 0")
        for t in (-2, 6, 7, 10, 11, 12, 13):      # USTRA, VSTRA, LKFR, UCUR, VCUR are no targets
            assert c.g2w(desc=((t, 0),)) == (1, G + ": unknown target of field 0"), t
        assert c.g2w(nfld=3, desc=((0, 0), (-1, 0), (0, 2))) == (1, G + ": field 2 targets a plane a field before it fills (LLNOTREAD)")
        assert c.g2w(nfld=2, desc=((-1, 0), (-1, 1)), ld=0)[0] == 0      # FIELD may be asked for more than once
        assert c.g2w(ncell_in=8) == (1, G + ": ncell_in is 8, the table's ncell 0") and c.g2w(desc=((-1, 0),), ncell_in=8)[0] == 0
        assert c.g2w(desc=((-1, 0),), ld=-1) == (1, G + ": ld is smaller than the table's ncell")
        assert c.g2w(ncell_in=0, values=a + 8) == (1, G + ": the buffers must be 16-byte aligned")
        assert c.g2w(ncell_in=0, fieldg=a + 4) == (1, G + ": the buffers must be 16-byte aligned") and c.g2w(ncell_in=0, out=a + 4)[0] == 0
        assert c.g2w(desc=((-1, 0),), out=a + 4) == (1, G + ": the buffers must be 16-byte aligned") and c.g2w(desc=((-1, 0),), fieldg=a + 4)[0] == 0
        assert c.g2w(slot=4, values=a + 8) == (1, G + ": bad range") and c.g2w(nfld=0, values=a + 8) == (1, G + ": nfld outside 1 .. 16")
        # CURRENT2WAM
        assert c.c2w() == (1, W + ": no inbound map")
        assert c.c2w(kijs=1, kijl=0) == (1, W + ": bad range")      # the range before the map
        assert c.set_map(np.arange(8))[0] == 0
        assert c.c2w()[0] == 0 and c.c2w(kijl=9) == (1, W + ": bad range") and c.c2w(kijs=-1) == (1, W + ": bad range")
        assert c.c2w(kijl=8, ucur=None) == (1, W + ": null pointer") and c.c2w(kijl=8, vcur=None) == (1, W + ": null pointer")
        assert c.c2w(fu=None, ucur=None)[0] == 0 and c.c2w(fu=None, fv=None, ucur=None, vcur=None, kijl=8)[0] == 0      # nothing to do
        assert c.c2w(ucur=a + 8) == (1, W + ": the buffers must be 16-byte aligned") and c.c2w(fv=a + 4) == (1, W + ": the buffers must be 16-byte aligned")
        assert c.c2w(changed=a + 2) == (1, W + ": the buffers must be 16-byte aligned") and c.c2w(changed=a + 4)[0] == 0
        torch.cuda.synchronize()
        assert bool((c.buf == F.SENT).all())      # nothing was launched on the one buffer all of them were given
    finally:
        c.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_a_refused_table_leaves_the_one_before_it(api, prec):
    name = "A"
    ctx = _context(api, name, prec)
    try:
        tab = F.table(name, prec)[1]
        fl, v = _msgs(name, ["plain"])[0]
        values = _up(ctx, v[None])

        def field():
            out = torch.full((1, F.NCELL), F.SENT, dtype=ctx.dtype, device=ctx.device)
            ctx.grib2wgrid(0, values, [(F.FIELD, fl)], out=out, pmiss=F.PMISS)
            torch.cuda.synchronize()
            return out.cpu().numpy()
        before = field()
        bad = tab["pos"].copy()
        bad[7, 1] = tab["nvalues"]
        with pytest.raises(api.EcwamHipError, match=r"position 1 of cell 7 outside \[-1, nvalues\)"):
            ctx.set_input_grid(0, bad, tab["w"], tab["kind"], tab["nvalues"], True)
        assert _same_bits(field(), before)
        with pytest.raises(api.EcwamHipError, match="vstride is 112, the table's nvalues 113"):      # a message of another grid
            ctx.set_input_grid(0, tab["pos"], tab["w"], tab["kind"], tab["nvalues"] + 1, True)
            field()
        ctx.set_input_grid(0, None)
        with pytest.raises(api.EcwamHipError, match="no table"):
            field()
        # two grids side by side: the slots do not disturb each other
        _set(ctx, "A", prec, 0)
        _set(ctx, "B", prec, 2)
        assert _same_bits(field(), before)
    finally:
        ctx.close()


# ---- 6. the chain: READWIND, then GETWND, against GETWND on the reference's FIELDG
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name,llwdwave", [("A", False), ("C", True)])
def test_readwind_then_getwnd(api, name, llwdwave, prec):
    """Wamintgr.readwind, then getwnd, gives the ff of "upload the reference's FIELDG, then getwnd": bit for bit where every plane GETWND reads is
    the reference's bit for bit (device_gate None), otherwise within the gates of tests/golden/forcing_observed.json.  Case A runs without the
    direction of the previous wave run (its plane goes through SIN, COS and ATAN2 and is the reference's only within a gate: the message is
    skipped, as READWIND skips it without LLWDWAVE); case C, a copy and RAD (v - 180), runs with it."""
    import forcing_ref as FF
    from ecwam_amd import grid as G
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    c = F.cached_cases()
    T = F.dtype_of(prec)
    cfg = Config(nang=12, nfre=36, nfre_red=36, lmaskice=False)

    def model():
        m = Wamintgr(cfg, G.build_grid(16, mask="continents"), prec)
        m.init_synthetic(seed=3)
        return m

    m, h = model(), model()
    n = m.n
    assert n > F.NROW
    # rows 0 .. 69 are those of the fixture; the further rows of the model read cells of their own behind the grid, which the table leaves alone
    ncell = F.NCELL + n - F.NROW
    cells = np.concatenate([c["map_in"], np.arange(F.NCELL, ncell)]).astype(np.int32)
    tab = dict(F.table(name, prec)[1])
    extra = ncell - F.NCELL
    tab["pos"] = np.concatenate([tab["pos"], np.full((extra, 4), -1, np.int32)])
    tab["kind"] = np.concatenate([tab["kind"], np.zeros(extra, np.int32)])
    if tab["w"] is not None:
        tab["w"] = np.concatenate([tab["w"], np.zeros((extra, 3))])
    for x in (m, h):
        x.set_forcing_map(cells, ncell)
    m.set_input_grid(1, tab)
    init = m.init_fieldg(roair=F.ROAIR, wstar0=F.WSTAR0).cpu().numpy().copy()
    msgs = [(param, v) for key, param, _, _, v in F.messages(c, name) if key.startswith("fg_")]
    fieldg, icode, iparamci = m.readwind(msgs, slot=1, roair=F.ROAIR, wstar0=F.WSTAR0, llwswave=True, llwdwave=llwdwave, pmiss=F.PMISS)
    torch.cuda.synchronize()
    assert fieldg is m.fieldg and tuple(fieldg.shape) == (13, ncell) and (icode, iparamci) == (3, 31)
    # the reference's FIELDG: INIT_FIELDG's planes, then what READWIND wrote inside the rows
    gold = F.golden_case(name, prec)["fieldg"]
    ref = init.copy()
    inrow = np.flatnonzero(tab["kind"][:F.NCELL] != 0)
    planes = [p for p, *_ in F.READWIND if llwdwave or p != "WDWAVE"]
    for p in planes:
        ref[F.FG[p], inrow] = gold[F.FG[p], inrow]
    got = fieldg.cpu().numpy()
    # the reference's bits are expected where the restatement had them: every plane GETWND reads here is a copy, a mean or a bilinear sum
    seen = F.observed()[f"restatement_vs_reference_{prec}"][name]
    exact = all(seen["fg_" + p] == 0.0 for p in planes)      # holds in both cases of this test
    if exact:
        assert _same_bits(got, ref)
    sw = dict(liceth=True, llwswave=True, llwdwave=llwdwave, icode_wnd=icode, iparamci=iparamci)
    m.getwnd(fieldg, "now", **sw)
    h.getwnd(torch.from_numpy(ref).to(h.dev), "now", **sw)
    torch.cuda.synchronize()
    a, b = m.ff.cpu().numpy(), h.ff.cpu().numpy()
    rows = slice(0, F.NROW)
    if exact:
        assert _same_bits(a[rows], b[rows]) and not _same_bits(a[rows], np.zeros_like(a[rows]))
    else:
        cols = {"AIRD": 0, "WDWAVE": 1, "CICOVER": 2, "WSWAVE": 3, "WSTAR": 4, "USTRA": 5, "VSTRA": 6, "CITHICK": 13}
        for col, j in cols.items():
            assert FF.column_error(a[rows, j], b[rows, j], col) <= FF.gate("getwnd", col, prec), col
    # stresses are ICODE 2; a parameter twice, or one READWIND does not know, is refused by name
    uv = {k: v for k, _, _, _, v in F.messages(c, name) if k in ("fg_UWND", "fg_VWND")}
    assert m.readwind([(180, uv["fg_UWND"]), (181, uv["fg_VWND"])], slot=1)[1] == 2
    assert m.readwind([(165, uv["fg_UWND"]), (140245, uv["fg_VWND"]), (140249, uv["fg_VWND"])], slot=1)[1] == 3      # both skipped
    with pytest.raises(ValueError, match="LLNOTREAD"):
        m.readwind([(165, uv["fg_UWND"]), (33, uv["fg_UWND"])], slot=1)
    with pytest.raises(ValueError, match="suspicious wind or sea ice field param 167"):
        m.readwind([(167, uv["fg_UWND"])], slot=1)
    # the currents of the same grid through Wamintgr.current2wam: the reference's bits on the fixture's rows
    cur = {k: v for k, _, _, _, v in F.messages(c, name) if k in ("ucur", "vcur")}
    if F.device_gate(name, "ucur", prec) is None and F.device_gate(name, "vcur", prec) is None:
        assert m.current2wam(cur["ucur"], cur["vcur"], slot=1, wlowest=F.WLOWEST, zmiss=F.PMISS) is True
        torch.cuda.synchronize()
        u, v = m._currents()
        g = F.golden_case(name, prec)
        assert _same_bits(u[:F.NROW].cpu().numpy(), g["ucur"]) and _same_bits(v[:F.NROW].cpu().numpy(), g["vcur"])
        assert m.current2wam(cur["ucur"], cur["vcur"], slot=1, wlowest=F.WLOWEST, zmiss=F.PMISS) is False
