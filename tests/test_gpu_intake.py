"""ecwam_hip_set_fldinter / _fldinter / _init_fieldg / _recvnemofields / _updnemo and the Wamintgr methods over them on the device (run with
-m gpu), against the reference's own results: tests/golden/intake_0.npz, recorded by tools/make_golden_intake.py from the reference's unmodified
INITIALINT, FLDINTER, INIT_FIELDG and RECVNEMOFIELDS in both precisions (UPDNEMOFIELDS and UPDNEMOSTRESS: their statements restated around the
routines, whose results are local arrays).  67 rows, the calls act on [3, 67): three guard rows and 64 points of an 11 x 9 reduced wave grid;
atmosphere grids A (periodic, reduced), B (regional: the clamps) and C (LLINTERPOL = F).

Fed with the reference's own tables the device gives the reference's FIELDG bit for bit: the same IEEE operations in the same order, no
contraction, no transcendental -- there is no tolerance.  Fed with ecwam_amd/intake.py's tables it is gated per plane
(tests/intake_ref.py::gate, from tests/golden/intake_observed.json; nothing in the gates comes from the device) on |a - b| / max(|b|, the
plane's largest |b|).  Double precision: 10 x the largest difference between the restated chain and the reference's double precision result,
8 eps where that is exactly 0.  Single precision: 3 x the reference's own single-against-double difference.
What the device measured against them is in profiles/intake_device.txt.
"""
import ctypes as C

import numpy as np
import pytest

import intake_ref as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

A = slice(F.KIJS, F.KIJL)
N = F.KIJL - F.KIJS
RANGES = {"one": [(F.KIJS, F.KIJL)], "two": [(F.KIJS, F.SPLIT), (F.SPLIT, F.KIJL)]}


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _context(api, prec):
    ctx = api.HipContext(F.tables(prec))
    ctx.set_forcing_map(F.cached_cases()["map_in"], F.NCELL)
    return ctx


def _up(ctx, a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F.dtype_of("sp" if ctx.dtype == torch.float32 else "dp") if dt is None else dt)).to(ctx.device)


def _fldinter(ctx, name, flags, ranges):
    """FLDINTER on a fieldg and a MASK_IN full of sentinels / zeros, over the row ranges given: (fieldg [13][99], mask [ngptotg]) afterwards"""
    c = F.cached_cases()
    g = c[name]
    fields = _up(ctx, g["fields"])
    fieldg = torch.full((13, F.NCELL), F.SENT, dtype=ctx.dtype, device=ctx.device)
    mask = torch.zeros(g["ngptotg"], dtype=torch.int32, device=ctx.device)
    for k0, k1 in ranges:
        ctx.fldinter(k0, k1, fields, fieldg, roair=c["roair"], wstar0=c["wstar0"], pmiss=F.PMISS, mask_in=mask, flags=flags)
    torch.cuda.synchronize()
    return fieldg.cpu().numpy(), mask.cpu().numpy()


# ---- (a) with the reference's own tables: the reference's FIELDG, bit for bit
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", F.CASES)
def test_fldinter_gives_the_bits_of_the_reference(api, name, prec):
    c, g = F.cached_cases(), F.load_golden()
    T = F.dtype_of(prec)
    gr = c[name]
    cells = c["map_in"][A]
    idx, w = F.point_table(c, name, F.golden_tables(g, name, prec) if gr["interpol"] else None)
    ctx = _context(api, prec)
    try:
        ctx.set_fldinter(idx, w, gr["ngptotg"], bool(gr["interpol"]))
        for fs, flags in F.FLAGSETS.items():
            ref = g[f"fli_{name}_{fs}_{prec}"]
            got, mask = _fldinter(ctx, name, flags, RANGES["one"])
            written = F.written_planes(flags)
            bad = [k for k, i in F.FG.items() if i in written and not _same_bits(got[i, cells], ref[i])]
            assert not bad, f"{name} {fs} {prec}: planes {bad} differ from the reference's bits"
            # the planes FLDINTER does not write, the cells of the guard rows and the cells of no row keep the sentinel
            keep = np.ones(got.shape, bool)
            keep[np.ix_(written, cells)] = False
            assert (got[keep] == T(F.SENT)).all() and (got[~keep] != T(F.SENT)).all(), (name, fs)
            assert np.array_equal(mask, g[f"mask_{name}_{fs}"].astype(np.int32)), (name, fs)
            two, mask2 = _fldinter(ctx, name, flags, RANGES["two"])
            assert _same_bits(two, got) and np.array_equal(mask2, mask), f"{name} {fs}: two launches differ from one"
    finally:
        ctx.close()


# ---- (b) with the tables of ecwam_amd/intake.py: within the gates
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_fldinter_with_the_tables_of_intake_py(api, name, prec):
    c, g, obs = F.cached_cases(), F.load_golden(), F.observed()
    gr = c[name]
    cells = c["map_in"][A]
    idx, w = F.point_table(c, name, F.own_tables(c, name, prec))
    ctx = _context(api, prec)
    bad = {}
    try:
        ctx.set_fldinter(idx, w, gr["ngptotg"], True)
        for fs, flags in F.FLAGSETS.items():
            ref = g[f"fli_{name}_{fs}_{prec}"]
            got, mask = _fldinter(ctx, name, flags, RANGES["one"])
            assert np.array_equal(mask, g[f"mask_{name}_{fs}"].astype(np.int32)), (name, fs)
            for plane, ip in F.FG.items():
                if ip in F.written_planes(flags):
                    err, gate = F.plane_error(got[ip, cells], ref[ip]), F.gate("fldinter", plane, prec, obs)
                    print(f"{name} {fs} {plane} {prec}: device with intake.py's tables against the reference {err:.3e} (gate {gate:.3e})")
                    if not err <= gate:
                        bad[(fs, plane)] = (err, gate)
    finally:
        ctx.close()
    assert not bad, bad


# ---- (c) the point-wise routines: exact bits
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_init_fieldg(api, prec):
    c, g = F.cached_cases(), F.load_golden()
    T = F.dtype_of(prec)
    ctx = _context(api, prec)
    try:
        for ncell in (F.NCELL, 1, 2, 64):      # 99: no whole number of 16-byte pieces, planes that begin inside a piece
            buf = torch.full((13 * ncell + 4,), F.SENT, dtype=ctx.dtype, device=ctx.device)
            ctx.init_fieldg(buf[:13 * ncell].view(13, ncell), c["roair"], c["wstar0"])
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert (got[13 * ncell:] == T(F.SENT)).all(), ncell      # nothing behind the planes is touched
            want = g[f"initfg_{prec}"][:, :ncell] if ncell <= F.NCELL else None
            assert _same_bits(got[:13 * ncell].reshape(13, ncell), np.ascontiguousarray(want)), ncell
        assert (g[f"initfg_{prec}"][F.FG["WSWAVE"]] == F.tables(prec).WSPMIN).all()
    finally:
        ctx.close()


def _recv(ctx, prec, flags, ranges, with_fieldg=True):
    c = F.cached_cases()
    nemo, ibr = _up(ctx, c["nemo"], np.float64), _up(ctx, c["nemoibr"], np.float64)
    ff, intf, u, v, fieldg = (_up(ctx, c[k]) for k in ("ff", "intf", "ucur", "vcur", "fieldg"))
    if not with_fieldg:
        fieldg = None
    for k0, k1 in ranges:
        # nemo's planes are kijl apart, kijl being that of the call: each launch is given the block cut to its own kijl
        nk, ik = nemo[:, :k1].contiguous(), ibr[:k1].contiguous()
        ctx.recvnemofields(k0, k1, nk, ff, u, v, intf, fieldg, ik, flags=flags)
        nemo[:, k0:k1], ibr[k0:k1] = nk[:, k0:k1], ik[k0:k1]
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in (nemo, ibr, ff, intf, u, v)]


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_recvnemofields(api, prec):
    c, g = F.cached_cases(), F.load_golden()
    T = F.dtype_of(prec)
    ctx = _context(api, prec)
    try:
        for call, flags in F.RECV.items():
            nemo, ibr, ff, intf, u, v = _recv(ctx, prec, flags, RANGES["one"])
            got_n = np.concatenate([nemo[:, A], ibr[None, A]])
            got_s = np.stack([ff[A, F.FF_CICOVER], ff[A, F.FF_CITHICK], u[A], v[A], intf[A, F.INTF_IBRMEM]])
            assert _same_bits(got_n, g[f"recv_{call}_nemo_{prec}"]), f"{call}: NEMO2WAM differs from the reference's bits"
            assert _same_bits(got_s, g[f"recv_{call}_state_{prec}"]), f"{call}: the state differs from the reference's bits"
            # the guard rows and every column of ff and intf that RECVNEMOFIELDS does not name keep their bits
            keep = np.ones(ff.shape, bool)
            keep[A, [F.FF_CICOVER, F.FF_CITHICK]] = False
            assert _same_bits(ff[keep], c["ff"].astype(T)[keep]), call
            keep[:] = True
            keep[A, F.INTF_IBRMEM] = False
            assert _same_bits(intf[keep], c["intf"].astype(T)[keep]), call
            assert _same_bits(nemo[:, :F.KIJS], c["nemo"][:, :F.KIJS]) and _same_bits(u[:F.KIJS], c["ucur"].astype(T)[:F.KIJS]), call
            two = _recv(ctx, prec, flags, RANGES["two"])
            assert all(_same_bits(x, y) for x, y in zip(two, (nemo, ibr, ff, intf, u, v))), f"{call}: two launches differ from one"
        # IBRMEM takes NEMO's value on either side of the lake test: with LINIT and LWCOU but none of the cover, the thickness and the currents
        # the call reads neither the map's entries nor fieldg, which may be NULL
        nemo, ibr, ff, intf, u, v = _recv(ctx, prec, F.RECV["init_cou_ibr"], RANGES["one"], with_fieldg=False)
        got_s = np.stack([ff[A, F.FF_CICOVER], ff[A, F.FF_CITHICK], u[A], v[A], intf[A, F.INTF_IBRMEM]])
        assert _same_bits(got_s, g[f"recv_init_cou_ibr_state_{prec}"]) and _same_bits(np.concatenate([nemo[:, A], ibr[None, A]]), g[f"recv_init_cou_ibr_nemo_{prec}"])
        assert _same_bits(intf[:F.KIJS], c["intf"].astype(T)[:F.KIJS])
        before = [c["nemo"], c["nemoibr"], c["ff"].astype(T), c["intf"].astype(T), c["ucur"].astype(T), c["vcur"].astype(T)]
        after = _recv(ctx, prec, F.LINIT | F.LWCOU, RANGES["one"], with_fieldg=False)      # no coupling flag at all: nothing is read or written
        assert all(_same_bits(x, y) for x, y in zip(after, before))
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_updnemo(api, prec):
    c, g = F.cached_cases(), F.load_golden()
    ld = F.NROW + 5
    ctx = _context(api, prec)
    try:
        for nt in F.NEMONTAU:
            for ranges in RANGES.values():
                w2n = _up(ctx, c["wam2nemo"], np.float64)
                f7 = torch.full((7, ld), F.SENT, dtype=torch.float64, device=ctx.device)
                s6 = torch.full((6, ld), F.SENT, dtype=torch.float64, device=ctx.device)
                for k0, k1 in ranges:
                    ctx.updnemo(k0, k1, w2n, nt, f7, s6)
                torch.cuda.synchronize()
                w, a7, a6 = w2n.cpu().numpy(), f7.cpu().numpy(), s6.cpu().numpy()
                assert _same_bits(a7[:, A], g[f"upd_{nt}_fields7_{prec}"]) and _same_bits(a6[:, A], g[f"upd_{nt}_stress6_{prec}"]), nt
                assert _same_bits(w[A], g[f"upd_{nt}_wam2nemo_{prec}"]) and not w[A][:, F.UPD_STRESS].any(), nt      # the six accumulators start again
                assert _same_bits(w[:F.KIJS], c["wam2nemo"][:F.KIJS]), nt      # the guard rows keep theirs
                for out in (a7, a6):
                    assert (out[:, :F.KIJS] == F.SENT).all() and (out[:, F.KIJL:] == F.SENT).all(), nt
            # either half alone
            w2n = _up(ctx, c["wam2nemo"], np.float64)
            f7 = torch.full((7, ld), F.SENT, dtype=torch.float64, device=ctx.device)
            ctx.updnemo(F.KIJS, F.KIJL, w2n, nt, f7, None)
            torch.cuda.synchronize()
            assert _same_bits(w2n.cpu().numpy(), c["wam2nemo"]) and _same_bits(f7.cpu().numpy()[:, A], g[f"upd_{nt}_fields7_{prec}"]), nt
            s6 = torch.full((6, ld), F.SENT, dtype=torch.float64, device=ctx.device)
            ctx.updnemo(F.KIJS, F.KIJL, w2n, nt, None, s6)
            torch.cuda.synchronize()
            assert _same_bits(s6.cpu().numpy()[:, A], g[f"upd_{nt}_stress6_{prec}"]) and _same_bits(w2n.cpu().numpy()[A], g[f"upd_{nt}_wam2nemo_{prec}"]), nt
    finally:
        ctx.close()


# ---- (d) the chain: IFSTOWAM, then GETWND, against GETWND on the reference's FIELDG
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_ifstowam_then_getwnd(api, prec):
    from ecwam_amd import grid as G
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    c, g = F.cached_cases(), F.load_golden()
    T = F.dtype_of(prec)
    cfg = Config(nang=12, nfre=36, nfre_red=36, lmaskice=False)

    def model():
        m = Wamintgr(cfg, G.build_grid(16, mask="continents"), prec)
        m.init_synthetic(seed=3)
        return m

    m, h = model(), model()
    n = m.n
    assert n > F.NROW
    gr = c["A"]
    flags = F.FLAGSETS["all"]
    # rows 0 .. 66 are those of the fixture; the further rows of the model read the first source point into cells of their own behind the grid
    ncell = F.NCELL + n - F.NROW
    cells = np.concatenate([c["map_in"], np.arange(F.NCELL, ncell)]).astype(np.int32)
    idx67, w67 = F.point_table(c, "A", F.golden_tables(g, "A", prec))
    idx, w = np.zeros((n, 4), np.int32), np.zeros((n, 3))
    idx[:F.NROW], w[:F.NROW] = idx67, w67
    for x in (m, h):
        x.set_forcing_map(cells, ncell)
    m.set_fldinter(idx, w, gr["ngptotg"], True)
    fields = torch.from_numpy(gr["fields"].astype(T)).to(m.dev)
    fieldg = m.ifstowam(fields, roair=c["roair"], wstar0=c["wstar0"], pmiss=F.PMISS, **F.flag_kw(flags))
    assert fieldg is m.fieldg and tuple(fieldg.shape) == (13, ncell)
    # the reference's FIELDG: INIT_FIELDG's planes, then what its FLDINTER wrote on the active rows
    ref = np.repeat(g[f"initfg_{prec}"][:, :1], ncell, 1)
    ref[np.ix_(F.written_planes(flags), c["map_in"][A])] = g[f"fli_A_all_{prec}"][F.written_planes(flags)]
    got = fieldg.cpu().numpy()
    assert _same_bits(got[:, c["map_in"][A]], ref[:, c["map_in"][A]])
    rest = sorted(set(range(13)) - set(F.written_planes(flags)))
    assert _same_bits(got[rest], ref[rest])      # WSWAVE and WDWAVE are INIT_FIELDG's everywhere
    sw = dict(liceth=True)
    m.getwnd(fieldg, "now", **sw)
    h.getwnd(torch.from_numpy(ref).to(h.dev), "now", **sw)
    torch.cuda.synchronize()
    a, b = m.ff.cpu().numpy(), h.ff.cpu().numpy()
    assert _same_bits(a[A], b[A]) and not _same_bits(a[A], np.zeros_like(a[A]))
    # the same rows through the context, with the resident state of the driver: RECVNEMOFIELDS and UPDNEMO* act on FF_NOW, the currents, INTFLDS
    nemo = torch.from_numpy(np.ascontiguousarray(np.resize(c["nemo"], (4, n)))).to(m.dev)
    ff0 = m.ff.clone()
    m.recvnemofields(nemo, linit=True, lwcou=False, lwnemocoucic=True, lwnemocoucur=True)
    torch.cuda.synchronize()
    assert _same_bits(m.ff[:, F.FF_CICOVER].cpu().numpy(), nemo[0].cpu().numpy().astype(T))
    assert _same_bits(m.ucur.cpu().numpy(), nemo[2].cpu().numpy().astype(T))
    keep = [k for k in range(16) if k != F.FF_CICOVER]
    assert _same_bits(m.ff[:, keep].cpu().numpy(), ff0[:, keep].cpu().numpy())
    w2n = torch.from_numpy(np.ascontiguousarray(np.resize(c["wam2nemo"], (n, 13)))).to(m.dev)
    before = w2n.cpu().numpy()
    f7, s6 = m.updnemo(w2n, 4)
    torch.cuda.synchronize()
    assert _same_bits(f7.cpu().numpy(), before[:, F.UPD_FIELDS].T) and _same_bits(s6.cpu().numpy(), (before[:, F.UPD_STRESS] * 0.25).T)
    assert not w2n[:, F.UPD_STRESS].any() and _same_bits(w2n[:, F.UPD_FIELDS].cpu().numpy(), before[:, F.UPD_FIELDS])


# ---- (e) refusals, with their words, each before any launch
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

    def set_map(self, inbound, ncell=16):
        m = None if inbound is None else np.ascontiguousarray(inbound, np.int32)
        return self.err(self.lib.ecwam_hip_set_forcing_map(self.h, 8, None if m is None else m.ctypes.data_as(C.c_void_p), ncell, None, 0))

    def set_table(self, npts=8, ngptotg=20, idx="ok", w="ok", interpol=1):
        rows = npts if npts > 0 else 8
        i = np.ascontiguousarray(np.arange(4 * rows).reshape(rows, 4) % 20 if isinstance(idx, str) else idx, np.int32) if idx is not None else None
        ww = np.zeros((rows, 3)) if isinstance(w, str) else w
        p = lambda m: None if m is None else m.ctypes.data_as(C.c_void_p)
        return self.err(self.lib.ecwam_hip_set_fldinter(self.h, npts, ngptotg, p(i), p(ww), interpol))

    def fldinter(self, kijs=0, kijl=0, fields="a", ngptotg=20, nfields=10, flags=0, fieldg="a", mask=None):
        fields, fieldg = (self.a if p == "a" else p for p in (fields, fieldg))
        return self.err(self.lib.ecwam_hip_fldinter(self.h, kijs, kijl, fields, ngptotg, nfields, flags, 1.225, 0.0, -999.0, fieldg, mask, None))

    def recv(self, kijs=0, kijl=0, flags=1, **p):
        g = lambda k: p.get(k, self.a)
        return self.err(self.lib.ecwam_hip_recvnemofields(self.h, kijs, kijl, flags, g("fieldg"), g("nemo"), g("nemoibr"), g("ff"), g("ucur"), g("vcur"), g("intf"),
                                                          None))

    def upd(self, kijs=0, kijl=0, w2n="a", nt=1, f7="a", s6="a", ld=8):
        w2n, f7, s6 = (self.a if p == "a" else p for p in (w2n, f7, s6))
        return self.err(self.lib.ecwam_hip_updnemo(self.h, kijs, kijl, w2n, nt, f7, s6, ld, None))

    def close(self):
        self.lib.ecwam_hip_destroy(self.h)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_refusals(api, prec):
    """Every case is refused before anything is launched (the buffer keeps its sentinels); the ranges are empty wherever the refusal itself
    needs no points."""
    c = Raw(prec)
    lib, h, a = c.lib, c.h, c.a
    S, R = "ecwam_hip_set_fldinter", "ecwam_hip_recvnemofields"
    try:
        # the table needs the inbound map, of its own length and with no cell twice
        assert c.fldinter() == (1, "ecwam_hip_fldinter: no table")
        assert c.set_table() == (1, S + ": no inbound map")
        assert c.set_map(np.array([0, 1, 2, 3, 4, 2, 6, 7]))[0] == 0      # two rows may read one cell ...
        assert c.set_table() == (1, S + ": row 5 of the inbound map names a cell twice (two rows would write one cell)")      # ... but not write it
        assert c.set_map(np.arange(8))[0] == 0
        assert c.set_table(npts=7) == (1, S + ": the inbound map has 8 rows, the table 7")
        assert c.set_table(npts=-1) == (1, S + ": negative count")
        assert c.set_table(ngptotg=0) == (1, S + ": the fields need at least one point")
        assert c.set_table(w=None) == (1, S + ": the interpolation needs its weights")
        tenth = np.full((8, 3), 0.1)      # a double that no float holds: single precision would not narrow it back unchanged
        if prec == "sp":
            assert c.set_table(w=tenth) == (1, S + ": weight 0 of row 0 is not a value of the working precision")
            assert c.set_table(w=tenth.astype(np.float32).astype(np.float64))[0] == 0
        else:
            assert c.set_table(w=tenth)[0] == 0
        assert c.set_table(idx=None)[0] == 0
        bad = np.arange(32).reshape(8, 4) % 20
        bad[3, 2] = 20
        assert c.set_table(idx=bad) == (1, S + ": index 2 of row 3 outside [0, ngptotg)")
        bad[3, 2] = -1
        assert c.set_table(idx=bad) == (1, S + ": index 2 of row 3 outside [0, ngptotg)")
        assert c.set_table(idx=bad, w=None, interpol=0)[0] == 0 and c.fldinter()[0] == 0      # without interpolation only the first position is read
        bad[3, 0] = 20
        assert c.set_table(idx=bad, w=None, interpol=0) == (1, S + ": index 0 of row 3 outside [0, ngptotg)")
        assert c.fldinter()[0] == 0      # a refused table leaves the one before it
        assert c.set_table(idx=None)[0] == 0 and c.fldinter() == (1, "ecwam_hip_fldinter: no table")
        assert c.set_table()[0] == 0 and c.fldinter()[0] == 0
        assert c.set_map(np.arange(8))[0] == 0 and c.fldinter() == (1, "ecwam_hip_fldinter: no table")      # a new map drops the table checked against the old
        assert c.set_table()[0] == 0
        # FLDINTER
        F_ = "ecwam_hip_fldinter"
        assert c.fldinter(flags=32) == (1, F_ + ": unknown flags")
        assert c.fldinter(kijs=1, kijl=0, flags=32) == (1, F_ + ": bad range") and c.fldinter(kijl=9, ngptotg=21) == (1, F_ + ": bad range")      # the range first
        assert c.fldinter(kijs=1, kijl=0) == (1, F_ + ": bad range") and c.fldinter(kijs=-1) == (1, F_ + ": bad range")
        assert c.fldinter(kijl=9) == (1, F_ + ": bad range")      # rows beyond the table
        assert c.fldinter(ngptotg=21) == (1, F_ + ": ngptotg is 21, the table's 20")
        assert c.fldinter(nfields=7) == (1, F_ + ": nfields is smaller than the switches need (8)")
        assert c.fldinter(nfields=9, flags=24) == (1, F_ + ": nfields is smaller than the switches need (10)")
        assert c.fldinter(nfields=8, flags=16)[0] == 0 and c.fldinter(nfields=8, flags=8)[0] == 0      # zero currents, or none, read no field 9
        assert c.fldinter(kijl=8, fields=None) == (1, F_ + ": null pointer") and c.fldinter(kijl=8, fieldg=None) == (1, F_ + ": null pointer")
        assert c.fldinter(fieldg=a + 8) == (1, F_ + ": the buffers must be 16-byte aligned")
        assert c.fldinter(mask=a + 2) == (1, F_ + ": the buffers must be 16-byte aligned")
        assert c.fldinter(mask=a + 4) == (1, F_ + ": the buffers must be 16-byte aligned") and c.fldinter(mask=a + 16)[0] == 0
        # INIT_FIELDG
        d = C.c_double(1.0)
        I_ = "ecwam_hip_init_fieldg"
        assert c.err(lib.ecwam_hip_init_fieldg(h, a, -1, d, d, None)) == (1, I_ + ": bad range")
        assert c.err(lib.ecwam_hip_init_fieldg(h, None, 4, d, d, None)) == (1, I_ + ": null pointer")
        assert c.err(lib.ecwam_hip_init_fieldg(h, a + 8, 0, d, d, None)) == (1, I_ + ": the buffers must be 16-byte aligned")
        assert c.err(lib.ecwam_hip_init_fieldg(h, None, 0, d, d, None))[0] == 0
        # RECVNEMOFIELDS
        assert c.recv(flags=128) == (1, R + ": unknown flags") and c.recv(kijs=1, kijl=0, flags=128) == (1, R + ": bad range")
        assert c.recv(flags=2 | 4 | 64, fieldg=None)[0] == 0 and c.recv(flags=2 | 4, fieldg=None)[0] == 0      # IBRMEM alone, or nothing, asks for no fieldg
        assert c.recv(flags=4 | 8) == (1, R + ": neither LREST nor LINIT")
        assert c.recv(kijs=1, kijl=0) == (1, R + ": bad range") and c.recv(flags=2 | 4 | 8, kijl=9) == (1, R + ": bad range")
        assert c.recv(flags=1, kijl=8, nemo=None) == (1, R + ": null pointer") and c.recv(flags=1, kijl=8, ff=None) == (1, R + ": null pointer")
        assert c.recv(flags=1 | 64, kijl=8, nemoibr=None) == (1, R + ": null pointer") and c.recv(flags=1, nemoibr=None, intf=None)[0] == 0
        assert c.recv(flags=2 | 4 | 32, kijl=8, fieldg=None) == (1, R + ": null pointer") and c.recv(flags=2 | 32, fieldg=None, ff=None)[0] == 0
        assert c.recv(ff=a + 8) == (1, R + ": the buffers must be 16-byte aligned")
        assert c.set_map(None)[0] == 0
        assert c.recv(flags=2 | 4 | 8) == (1, R + ": no inbound map") and c.recv(flags=2 | 8)[0] == 0 and c.recv(flags=1)[0] == 0
        # UPDNEMO
        U_ = "ecwam_hip_updnemo"
        assert c.upd()[0] == 0 and c.upd(f7=None, s6=None, w2n=None)[0] == 0
        assert c.upd(kijs=1, kijl=0) == (1, U_ + ": bad range") and c.upd(kijl=8, ld=7) == (1, U_ + ": bad range")
        assert c.upd(kijl=8, ld=7, w2n=None, s6=a + 8) == (1, U_ + ": bad range")      # the range before the buffers
        assert c.upd(kijl=8, w2n=None) == (1, U_ + ": null pointer")
        assert c.upd(s6=a + 8) == (1, U_ + ": the buffers must be 16-byte aligned")
        torch.cuda.synchronize()
        assert bool((c.buf == F.SENT).all())      # nothing was launched on the one buffer all of them were given
    finally:
        c.close()
