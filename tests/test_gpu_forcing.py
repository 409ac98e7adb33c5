"""ecwam_hip_set_forcing_map / _getwnd / _cdustarz0 / _wamadswstar / _getcurr / _wvblock / _fldtoifs and the Wamintgr methods over them on the
device (run with -m gpu), against the reference's own results: tests/golden/forcing_0.npz, recorded by tools/make_golden_forcing.py from the
reference's unmodified WAMWND, MICEP, CDUSTARZ0, WAMADSWSTAR, WAMCUR and OUTBETA in both precisions.  67 rows, the calls act on [3, 67): three
guard rows and 64 points on an 11 x 9 grid.

Gates (tests/forcing_ref.py::gate, from tests/golden/forcing_observed.json; nothing in them comes from the device), per routine and column, on
|a - b| / max(|b|, the column's largest |b|), WDWAVE on the circle.  Double precision: 10 x the largest difference between the numpy
restatement and the reference's double precision results, 8 eps where that is exactly 0.  Single precision: 3 x the largest difference between
the reference's own single and double precision results, 8 eps (single) where that is 0.  A column the reference copies has no gate: it is
bit-identical.
What the device measured against them is in profiles/forcing_device.txt.
"""
import ctypes as C

import numpy as np
import pytest

import forcing_ref as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -777.25
A = slice(F.KIJS, F.KIJL)
SPLIT = 30      # rows [3, 30) and [30, 67) in two calls
LD = F.NROW + 5  # the leading dimension of WVBLOCK: longer than the rows


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _context(api, call, prec):
    c = F.cached_cases()
    ctx = api.HipContext(F.tables_of(call, prec))
    ctx.set_forcing_map(c["map_in"], F.NCELL, c["map_out"], F.NCELL)
    return ctx


def _opts(call):
    o = F.GETWND[call]
    return dict(icode_wnd=o["icode_wnd"], llwswave=o["llwswave"], llwdwave=o["llwdwave"], lcorrel=F.lcorrel(o), rwfac=o["rwfac"], iparamci=o["iparamci"],
                lwcou=o["lwcou"], lwnemocoucic=o["lwnemocoucic"], lwnemocoucit=o["lwnemocoucit"], lnemoicerest=o["lnemoicerest"], liceth=o["liceth"],
                swamp=o["swamp"], swampcith=F.SWAMPCITH, zmiss=F.ZMISS)


def _run(api, call, prec, ranges):
    """One recorded call on the device over the row ranges given (one launch each): (the buffer it writes afterwards, what it held before, the
    positions of the recorded columns in it)."""
    T = np.float32 if prec == "sp" else np.float64
    c = F.cached_cases()
    r = F.routine_of(call)
    ctx = _context(api, call, prec)
    dev = ctx.device
    try:
        up = lambda a, dt=T: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        fieldg, nemo = up(F.fieldg_of(call, c)), up(c["nemo"], np.float64)
        if r in ("getwnd", "cdustarz0", "adswstar"):
            before = c["ff"].astype(T)
            buf = up(before)
            where = [F.FF[k] for k in F.columns(call)]
        elif r == "getcurr":
            before = np.full((F.NROW, 2), SENT, T)
            u, v = up(before[:, 0]), up(before[:, 1])
            where = [0, 1]
        else:
            flags, _, nwv = F.WVBLOCK[call]
            before = np.full((LD, nwv), SENT, T)
            buf = up(before.T)
            ff, intf = up(c["ff"]), up(c["intf"])
            where = list(range(nwv))
        for k0, k1 in ranges:
            if r == "getwnd":
                lc = F.lcorrel(F.GETWND[call])
                ctx.getwnd(k0, k1, fieldg, buf, up(c["ucur"]) if lc else None, up(c["vcur"]) if lc else None, nemo, **_opts(call))
            elif r == "cdustarz0":
                ctx.cdustarz0(k0, k1, buf)
            elif r == "adswstar":
                ctx.wamadswstar(k0, k1, fieldg, buf)
            elif r == "getcurr":
                ctx.getcurr(k0, k1, int(call[-1]), u, v, fieldg, nemo)
            else:
                ctx.wvblock(k0, k1, buf, ff, intf, flags=flags, prchar=F.PRCHAR)
        torch.cuda.synchronize()
        if r == "getcurr":
            got = np.stack([u.cpu().numpy(), v.cpu().numpy()], 1)
        elif r == "wvblock":
            got = np.ascontiguousarray(buf.cpu().numpy().T)
        else:
            got = buf.cpu().numpy()
        return got, before, where
    finally:
        ctx.close()


# ---- 1. parity with the reference and the exact properties, per recorded call and precision
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("call", F.CALLS)
def test_parity_with_the_reference(api, call, prec):
    g, obs = F.load_golden(), F.observed()
    T = np.float32 if prec == "sp" else np.float64
    ref = g[f"{call}_{prec}"]
    r = F.routine_of(call)
    got, before, where = _run(api, call, prec, [(F.KIJS, F.KIJL)])
    # the guard rows, the rows past the range and every column the routine does not write keep their bits
    keep = np.ones(got.shape, bool)
    keep[F.KIJS:F.KIJL, where] = False
    assert _same_bits(got[keep], before[keep]), f"{call}: something outside the written columns of the rows changed"
    res = got[A][:, where]
    err = F.errors(call, res, ref)
    bad = {}
    for j, name in enumerate(F.columns(call)):
        if name in F.COMPUTED[r]:
            gate = F.gate(r, name, prec, obs)
            print(f"{call} {name} {prec}: device against the reference {err[name]:.3e} (gate {gate:.3e})")
            if not err[name] <= gate:
                bad[name] = (err[name], gate)
        else:
            assert _same_bits(res[:, j], ref[:, j]), f"{call} {name}: a copied column differs"
    # a value the reference gives as exactly 0, 1, WSPMIN, EPSUS, PRCHAR, ALPHAMIN or +-CURRENT_MAX is exactly that
    for value in F.exact_values(call, prec):
        assert (res[ref == T(value)] == T(value)).all(), (call, value)
    # two calls on disjoint rows = one call over both
    two, _, _ = _run(api, call, prec, [(F.KIJS, SPLIT), (SPLIT, F.KIJL)])
    assert _same_bits(two, got), f"{call}: two calls differ from one"
    assert not bad, bad


# ---- 2. GETCURR's KUPDATE
def test_getcurr_reports_a_change(api):
    c = F.cached_cases()
    ctx = _context(api, "getcurr0", "sp")
    try:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ctx.device)
        fg = c["fieldg"].copy()
        fieldg = up(fg)
        u, v = up(np.full(F.NROW, SENT)), up(np.full(F.NROW, SENT))
        changed = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        ctx.getcurr(F.KIJS, F.KIJL, 0, u, v, fieldg, None, changed)
        assert int(changed.item()) == 1      # the sentinels went
        changed.zero_()
        ctx.getcurr(F.KIJS, F.KIJL, 0, u, v, fieldg, None, changed)
        assert int(changed.item()) == 0      # the buffers already hold the result
        ctx.getcurr(5, 5, 0, u, v, fieldg, None, changed)      # an empty range
        assert int(changed.item()) == 0
        cell = int(c["map_in"][F.KIJS + 40])
        fg[F.FG["VCUR"], cell] += 0.25      # one point's input moves (point 40 holds V = 0)
        moved = up(fg)
        ctx.getcurr(F.KIJS, F.KIJL, 0, u, v, moved, None, changed)
        assert int(changed.item()) == 1
        ctx.getcurr(F.KIJS, F.KIJL, 0, u, v, moved, None, changed)      # nothing changes now: a prior 1 is not cleared
        assert int(changed.item()) == 1
        changed.zero_()
        ctx.getcurr(F.KIJS, F.KIJL, 2, u, v, None, None, changed)
        assert int(changed.item()) == 1 and not u[A].any() and not v[A].any() and bool((u[: F.KIJS] == SENT).all())
    finally:
        ctx.close()


# ---- 3. MPFLDTOIFS on one task
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_fldtoifs(api, prec):
    T = np.float32 if prec == "sp" else np.float64
    c = F.cached_cases()
    rng = np.random.default_rng(5)
    nwv = 5
    ctx = _context(api, "adswstar", prec)
    try:
        block = rng.uniform(-1.0, 1.0, (nwv, LD)).astype(T)
        wv = torch.from_numpy(block).to(ctx.device)
        defval = np.array([0.0185, 0.0, -3.5, 1.0e-3, 7.0])
        grid = torch.full((nwv, F.NCELL), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.fldtoifs(F.KIJS, SPLIT, wv, grid, defval)      # LLINIT_GRID with the first rows,
        ctx.fldtoifs(SPLIT, F.KIJL, wv, grid)              # the others without
        torch.cuda.synchronize()
        got = grid.cpu().numpy()
        want = np.repeat(defval.astype(T)[:, None], F.NCELL, 1)
        want[:, c["map_out"][A]] = block[:, A]
        assert _same_bits(got, want)      # the defaults in the unmapped cells (those of the guard rows among them), the block's bits in the mapped ones
        grid = torch.full((nwv, F.NCELL), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.fldtoifs(F.KIJS, F.KIJL, wv, grid)
        torch.cuda.synchronize()
        want = np.full((nwv, F.NCELL), SENT, T)
        want[:, c["map_out"][A]] = block[:, A]
        assert _same_bits(grid.cpu().numpy(), want)       # without defval the unmapped cells keep the sentinel
    finally:
        ctx.close()


# ---- 4. refusals, with their words, each before any launch
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
        self.buf = torch.zeros(64 * 64, dtype=torch.float64, device="cuda:0")
        self.a = self.buf.data_ptr()

    def err(self, rc):
        return rc, self.lib.ecwam_hip_last_error().decode()

    def set_map(self, n=8, ncell=16, inbound="ok", outbound="ok"):
        mk = lambda m: None if m is None else np.ascontiguousarray(m, np.int32)
        i = mk(np.arange(n) if isinstance(inbound, str) else inbound)
        o = mk(np.arange(n)[::-1] if isinstance(outbound, str) else outbound)
        p = lambda m: None if m is None else m.ctypes.data_as(C.c_void_p)
        return self.err(self.lib.ecwam_hip_set_forcing_map(self.h, n, p(i), ncell, p(o), ncell))

    def getwnd(self, kijs=0, kijl=0, ff="a", fieldg="a", **kw):
        o = self.L.ForcingOpts(kw.get("icode_wnd", 3), 0, 0, 0, 1.0, kw.get("iparamci", 31), 0, kw.get("lwnemocoucic", 0), 0, 0, 0, 0, 0.0, -999.0)
        ff, fieldg = (self.a if p == "a" else p for p in (ff, fieldg))
        return self.err(self.lib.ecwam_hip_getwnd(self.h, kijs, kijl, fieldg, None, None, self.a if kw.get("lwnemocoucic") else None, ff, C.byref(o), None))

    def wvblock(self, kijs=0, kijl=0, flags=0, nwv=12, ld=8, ff="a"):
        return self.err(self.lib.ecwam_hip_wvblock(self.h, kijs, kijl, self.a if ff == "a" else ff, self.a, flags, nwv, 0.0185, self.a, ld, None))

    def close(self):
        self.lib.ecwam_hip_destroy(self.h)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_refusals(api, prec):
    """Every case is refused before anything is launched; the ranges are empty wherever the refusal itself needs no points."""
    c = Raw(prec)
    lib, h, a = c.lib, c.h, c.a
    try:
        # without a map
        assert c.getwnd() == (1, "ecwam_hip_getwnd: no inbound map")
        assert c.err(lib.ecwam_hip_wamadswstar(h, 0, 0, a, a, None)) == (1, "ecwam_hip_wamadswstar: no inbound map")
        assert c.err(lib.ecwam_hip_getcurr(h, 0, 0, 0, a, None, a, a, None, None)) == (1, "ecwam_hip_getcurr: no inbound map")
        assert c.err(lib.ecwam_hip_getcurr(h, 0, 0, 2, None, None, a, a, None, None))[0] == 0      # the zero currents read no map
        assert c.err(lib.ecwam_hip_fldtoifs(h, 0, 0, a, 8, 2, None, a, None)) == (1, "ecwam_hip_fldtoifs: no outbound map")
        # the maps themselves
        for bad in (np.array([0, 1, 2, 3, 4, 5, 6, 16]), np.array([0, 1, 2, -1, 4, 5, 6, 7])):
            rc, msg = c.set_map(inbound=bad)
            assert rc == 1 and "inbound index" in msg and "outside [0, ncell_in)" in msg, msg
            rc, msg = c.set_map(outbound=bad)
            assert rc == 1 and "outbound index" in msg and "outside [0, ncell_out)" in msg, msg
        rc, msg = c.set_map(outbound=np.array([0, 1, 2, 3, 4, 2, 6, 7]))
        assert rc == 1 and msg == "ecwam_hip_set_forcing_map: outbound index 5 is a duplicate (two rows would write one cell)"
        assert c.set_map(inbound=np.array([0, 1, 2, 3, 4, 2, 6, 7]))[0] == 0      # two rows may read one cell
        assert c.getwnd()[0] == 0      # a refused map leaves the one before it; an accepted one serves: the well-formed empty call
        assert c.set_map(inbound=None)[0] == 0 and c.getwnd() == (1, "ecwam_hip_getwnd: no inbound map")
        assert c.set_map()[0] == 0
        # the conventions of ecwam_hip_setice
        for who, call in (("getwnd", lambda **k: c.getwnd(**k)), ("wvblock", lambda **k: c.wvblock(flags=1, **k)),
                          ("cdustarz0", lambda kijs=0, kijl=0, ff=a: c.err(lib.ecwam_hip_cdustarz0(h, kijs, kijl, ff, None)))):
            who = "ecwam_hip_" + who
            assert call()[0] == 0, who
            assert call(kijs=1, kijl=0) == (1, who + ": bad range") and call(kijs=-1) == (1, who + ": bad range")
            assert call(kijl=8, ff=None) == (1, who + ": null pointer")
            assert call(ff=a + 8) == (1, who + ": the buffers must be 16-byte aligned")      # misaligned ff, for an empty range too
        assert c.getwnd(kijl=9) == (1, "ecwam_hip_getwnd: bad range")      # rows beyond the map
        assert c.getwnd(fieldg=a + 4) == (1, "ecwam_hip_getwnd: the buffers must be 16-byte aligned")
        # the per-call refusals
        for icode in (0, 4, -1):
            assert c.getwnd(icode_wnd=icode) == (1, "ecwam_hip_getwnd: ICODE_WND must be 1, 2 or 3")
        for ip in (0, 32, 140):
            assert c.getwnd(iparamci=ip) == (1, "ecwam_hip_getwnd: IPARAMCI must be 31 or 139 unless LWNEMOCOUCIC")
            assert c.getwnd(iparamci=ip, lwnemocoucic=1)[0] == 0
        assert c.getwnd(iparamci=139)[0] == 0
        assert c.err(lib.ecwam_hip_getwnd(h, 0, 0, a, None, None, None, a, None, None)) == (1, "ecwam_hip_getwnd: null options")
        assert c.err(lib.ecwam_hip_getcurr(h, 0, 0, 3, a, None, a, a, None, None))[1].startswith("ecwam_hip_getcurr: mode must be")
        assert c.wvblock(flags=16) == (1, "ecwam_hip_wvblock: unknown flags")
        assert c.wvblock(flags=2)[1].startswith("ecwam_hip_wvblock: LWCOUHMF needs LWCOU2W")
        for flags, need in ((0, 1), (1, 1), (3, 2), (4, 3), (8, 8), (15, 11)):
            assert c.wvblock(flags=flags, nwv=need)[0] == 0
            assert c.wvblock(flags=flags, nwv=need - 1) == (1, f"ecwam_hip_wvblock: nwvfields is smaller than the switches need ({need})")
        assert c.wvblock(nwv=33) == (1, "ecwam_hip_wvblock: nwvfields above ECWAM_HIP_MAXWVFIELDS")
        assert c.wvblock(kijl=8, ld=7) == (1, "ecwam_hip_wvblock: bad range")
        assert c.err(lib.ecwam_hip_fldtoifs(h, 0, 0, a, 8, 0, None, a, None)) == (1, "ecwam_hip_fldtoifs: nwvfields outside 1 .. ECWAM_HIP_MAXWVFIELDS")
        assert c.err(lib.ecwam_hip_fldtoifs(h, 0, 0, a, 8, 2, None, a, None))[0] == 0
    finally:
        c.close()


# ---- 5. the driver: Wamintgr's methods = the context's calls over the local rows, bit for bit
def test_the_methods_of_the_driver(api):
    from ecwam_amd import grid as G
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=36, lmaskice=False)

    def model():
        m = Wamintgr(cfg, G.build_grid(16, mask="continents"), "sp")
        m.init_synthetic(seed=3)
        return m

    m, h = model(), model()
    n = m.n
    rng = np.random.default_rng(11)
    ncell = n + 9
    cells = rng.permutation(ncell)[:n]
    out_cells = rng.permutation(ncell)[:n]
    for x in (m, h):
        x.set_forcing_map(cells, ncell, out_cells, ncell)
    fg = rng.uniform(-8.0, 8.0, (13, ncell)).astype(np.float32)
    fg[F.FG["AIRD"]] = rng.uniform(1.0, 1.3, ncell)
    fg[F.FG["CICOVER"]] = rng.choice([0.0, 0.5, 0.97], ncell)
    fg[F.FG["CITHICK"]] = rng.uniform(0.5, 2.0, ncell)
    fieldg = torch.from_numpy(fg).to(m.dev)
    sw = dict(liceth=True)
    W = [0, 1, 2, 3, 4, 5, 6, 13]      # what GETWND writes with ICODE_WND = 3, and what NEWWIND hands over
    # first_wind = getwnd on NOW + cdustarz0
    m.first_wind(fieldg, **sw)
    h.ctx.getwnd(0, n, fieldg, h.ff, **sw)
    h.ctx.cdustarz0(0, n, h.ff)
    torch.cuda.synchronize()
    assert _same_bits(m.ff.cpu().numpy(), h.ff.cpu().numpy()) and m.ff_next is None
    assert bool((m.ff[:, 3] >= float(m.t.WSPMIN)).all()) and bool((m.ff[:, 7] > 0).all()) and bool((m.ff[:, 2] > 0).any())
    # getwnd(target="next"), then newwind(): the fields reach NOW
    fg2 = fg.copy()
    fg2[:2] = rng.uniform(-12.0, 12.0, (2, ncell))
    fieldg2 = torch.from_numpy(fg2).to(m.dev)
    now0 = m.ff.clone()
    m.getwnd(fieldg2, **sw)
    assert _same_bits(m.ff.cpu().numpy(), now0.cpu().numpy())      # NOW is untouched until NEWWIND
    want = now0.clone()
    h.ctx.getwnd(0, n, fieldg2, want, **sw)
    torch.cuda.synchronize()
    assert _same_bits(m.ff_next.cpu().numpy(), want.cpu().numpy()) and not _same_bits(want[:, 3].cpu().numpy(), now0[:, 3].cpu().numpy())
    m.newwind()
    torch.cuda.synchronize()
    assert _same_bits(m.ff[:, W].cpu().numpy(), want[:, W].cpu().numpy())
    # adswstar, the currents, the coupling fields
    m.adswstar(fieldg)
    assert _same_bits(m.ff[:, [0, 4, 5, 6]].cpu().numpy(), fg[[2, 3, 6, 7]][:, cells].T)
    assert m.getcurr(fieldg) is True and m.getcurr(fieldg) is False
    assert _same_bits(m.ucur.cpu().numpy(), np.clip(fg[F.FG["UCUR"], cells], -1.5, 1.5))
    assert m.getcurr(mode=2) is True and not bool(m.ucur.any())
    wv = m.wvblock(lwcou2w=True, lwcouhmf=True, lwstokes=True)
    assert tuple(wv.shape) == (4, n) and _same_bits(wv[2].cpu().numpy(), m.intf[:, 2].cpu().numpy())
    grid = m.fldtoifs(wv, defval=[0.0185, 0.0, 0.0, 0.0])
    torch.cuda.synchronize()
    got = grid.cpu().numpy()
    assert tuple(got.shape) == (4, ncell) and _same_bits(got[:, out_cells], wv.cpu().numpy())
    rest = np.setdiff1d(np.arange(ncell), out_cells)
    assert (got[0, rest] == np.float32(0.0185)).all() and not got[1:, rest].any()
