"""ecwam_hip_bouinpt / ecwam_hip_outbc / the nest methods of Wamintgr on the device (run with -m gpu).

bouinpt is compared with what the reference's own INTSPEC returned (tests/golden/intspec_nang12.npz, 12 directions, the golden outputs of
the same precision) and, at 36 directions, with the numpy restatement tests/intspec_ref.py.  Two error figures: per bin |device - reference|
over the peak of the reference spectrum, and per point the DFIM-weighted sum of the differences over the reference's energy.  The gates were
not chosen: they are three times what the restatement itself differs from the reference by on the CPU (tests/test_nest_host.py):
  double: per bin 3.54e-15 of the peak, energy 3.35e-15, THQ 1.78e-15 rad; single: per bin 1.91e-6, energy 2.11e-6, THQ 9.54e-7 rad;
  EMEAN and FMEAN bit-equal in both (so the device's must be bit-equal too).
Measured on the device (MI355X; printed by the tests):
  12 directions against the reference:   dp per bin 1.67e-15, energy 1.93e-15, THQ 1.78e-15; sp per bin 1.91e-6, energy 2.10e-6, THQ 9.54e-7
  36 directions against the restatement: dp per bin 3.79e-15, energy 3.10e-15, THQ 1.78e-15; sp per bin 7.45e-7, energy 4.37e-7, THQ 2.38e-7
  EMEAN and FMEAN bit-equal everywhere.  outbc against numpy: FMEAN 6e-16 (dp) / 1.6e-7 (sp) relative, THQ 5e-14 / 1.8e-5 degrees.
Everything else is exact: the copies, the single-weight products, the zeros, the rotation whose weights involve no transcendental, the
range filter, the gather of outbc and its round trip through bouinpt are compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import intspec_ref as R
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DT = dict(dp=np.float64, sp=np.float32)
NROW = 64


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def golden():
    import os

    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intspec_nang12.npz")))


class Dev:
    """A context and the tensors of one bouinpt call; spectra of the fine grid start as noise, so that an untouched row shows."""

    def __init__(self, api, nang, prec, nrow=NROW, seed=1):
        self.prec, self.dt = prec, DT[prec]
        self.t = Tables(Config(nang=nang, nfre=36, nfre_red=36), self.dt)
        self.ctx = api.HipContext(self.t)
        self.dev = self.ctx.device
        self.nrow, self.nang = nrow, nang
        self.fl0 = np.random.default_rng(seed).uniform(0.5, 1.5, (nrow, nang, 36)).astype(self.dt)

    def to(self, a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype or self.dt)).to(self.dev)

    def bouinpt(self, ijb, ibcl, ibcr, bfw, f1, par1, kijs=0, kijl=None, fl1=None, par_fill=-7.0):
        """(fl1 [nrow][K][M], par_out [nijb][3]) after one call, as numpy arrays"""
        fl1 = self.to(self.fl0) if fl1 is None else fl1
        po = torch.full((len(ijb), 3), par_fill, dtype=fl1.dtype, device=self.dev)
        self.ctx.bouinpt(kijs, self.nrow if kijl is None else kijl, self.to(ijb, np.int32), self.to(ibcl, np.int32), self.to(ibcr, np.int32), self.to(bfw),
                         self.to(f1), self.to(par1), fl1, po)
        torch.cuda.synchronize()
        return fl1.cpu().numpy(), po.cpu().numpy()

    def close(self):
        self.ctx.close()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _pairs(bfw, f, par):
    """n cases as a boundary file of 2 n records: case i interpolates between records 2 i + 1 and 2 i + 2"""
    n = len(bfw)
    return np.arange(1, 2 * n, 2), np.arange(2, 2 * n + 1, 2), f.reshape(2 * n, *f.shape[2:]), par.reshape(2 * n, 3)


def _check_against(d, got_fl, got_par, ijb, ref_fl, ref_par, what):
    ebin = een = eth = 0.0
    for i, ij in enumerate(ijb):
        a, b = R.errors(got_fl[ij].T, ref_fl[i], d.t.DFIM)      # the device holds [K][M]
        ebin, een = max(ebin, a), max(een, b)
        dth = abs(float(got_par[i, 1]) - float(ref_par[i][1]))
        eth = max(eth, min(dth, 2 * np.pi - dth))
        assert got_par[i, 0] == ref_par[i][0] and got_par[i, 2] == ref_par[i][2], (i, got_par[i], ref_par[i])
    gate = R.GATE[d.prec]
    print(f"bouinpt {what} {d.prec}: per bin {ebin:.3e} of the peak (gate {gate['bin']:.2e}), energy {een:.3e} (gate {gate['energy']:.2e}), "
          f"THQ {eth:.3e} rad (gate {gate['thq']:.2e})")
    assert ebin < gate["bin"] and een < gate["energy"] and eth < gate["thq"], (ebin, een, eth, gate)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_bouinpt_against_the_reference(api, golden, prec):
    """12 directions: the 96 golden cases against the reference's own results of the same precision."""
    g = golden
    n = g["bfw"].size
    d = Dev(api, 12, prec, nrow=n + 8)
    try:
        ijb = np.random.default_rng(2).permutation(n + 8)[:n]
        ibcl, ibcr, f1, par1 = _pairs(g["bfw"], g["f"], g["par"])
        fl, po = d.bouinpt(ijb, ibcl, ibcr, g["bfw"], f1, par1)
        _check_against(d, fl, po, ijb, g["fl_" + prec], g["par_" + prec], "12 directions against the reference")
        rest = np.setdiff1d(np.arange(n + 8), ijb)
        assert _same(fl[rest], d.fl0[rest])
    finally:
        d.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_bouinpt_36_directions_against_the_restatement(api, prec):
    d = Dev(api, 36, prec)
    try:
        n = 48
        bfw, f, par, _ = R.make_cases(np.random.default_rng(36), n, d.t.FR, d.t.TH)
        ijb = np.random.default_rng(3).permutation(NROW)[:n]
        ibcl, ibcr, f1, par1 = _pairs(bfw, f, par)
        fl, po = d.bouinpt(ijb, ibcl, ibcr, bfw, f1, par1)
        ref = [R.bouinpt_point(d.t.FR, bfw[i], ibcl[i], ibcr[i], f1, par1, d.dt) for i in range(n)]
        _check_against(d, fl, po, ijb, [r[0] for r in ref], [r[1] for r in ref], "36 directions against the restatement")
    finally:
        d.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("nang", [12, 36])
def test_bouinpt_exact_cases(api, nang, prec):
    """Bit for bit: BFW <= 0 copies the left record; EMEAN1 == 0 / EMEAN2 == 0 give the other spectrum times its weight; the land index 0 on
    either side; |INC| >= NFRE in both directions leaves zeros; a rotation by NANG - 1 bins and a half (and one by half a bin) wraps in K."""
    d = Dev(api, nang, prec)
    try:
        T = d.dt
        rng = np.random.default_rng(7)
        f1 = rng.uniform(0.1, 1.0, (6, 36, nang)).astype(T)
        a = T(0.5) * T(d.t.DELTH)
        par1 = np.array([[1.0, 0.3, 0.1], [2.0, 1.1, 0.2], [0.0, 0.7, 0.15], [1.0, 0.3, 0.2e-4], [1.5, a, 0.125], [1.5, -a, 0.125]], dtype=T)
        #        what                     IBFL IBFR BFW
        cases = [("copy, BFW = 0",          2, 1, 0.0), ("copy, BFW < 0", 1, 2, -0.5), ("EMEAN1 = 0", 3, 2, 0.25), ("EMEAN2 = 0", 1, 3, 0.25),
                 ("land left",              0, 2, 0.375), ("land right", 1, 0, 0.375), ("land both", 0, 0, 0.5), ("land left copied", 0, 2, 0.0),
                 ("|INC| >= NFRE",          2, 4, 0.99), ("|INC| >= NFRE, swapped", 4, 2, 0.01), ("rotation", 5, 6, 0.5), ("rotation, swapped", 6, 5, 0.5)]
        ijb = rng.permutation(NROW)[: len(cases)]
        fl, po = d.bouinpt(ijb, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], f1, par1)
        for i, (what, l, r, w) in enumerate(cases):
            ref, rpar = R.bouinpt_point(d.t.FR, T(w), l, r, f1, par1, T)
            assert _same(np.ascontiguousarray(fl[ijb[i]].T), np.ascontiguousarray(ref)), what
            rpar = np.array(rpar, dtype=T)
            if what.startswith("|INC|"):      # the only cases here whose THQ comes out of COS / SIN / ATAN2
                dth = abs(float(po[i, 1]) - float(rpar[1]))
                assert _same(po[i, [0, 2]], rpar[[0, 2]]) and min(dth, 2 * np.pi - dth) < R.GATE[prec]["thq"], (what, po[i], rpar)
            else:
                assert _same(po[i], rpar), (what, po[i], rpar)
            if what.startswith("|INC|") or what == "land both" or what == "land left copied":
                assert not fl[ijb[i]].any(), what
        # the rotation is what it says: spectrum 1 by NANG - 1 bins and a half, spectrum 2 by half a bin (both wrap in K), GAMMA = 1, EMEAN / EMEAN1 = 1
        i = [c[0] for c in cases].index("rotation")
        want = 0.5 * (0.5 * np.roll(f1[4], -1, axis=1) + 0.5 * f1[4]) + 0.5 * (0.5 * f1[5] + 0.5 * np.roll(f1[5], 1, axis=1))
        assert np.allclose(fl[ijb[i]].T, want, rtol=1e-5, atol=0) and po[i, 1] == 0
        rest = np.setdiff1d(np.arange(NROW), ijb)
        assert _same(fl[rest], d.fl0[rest])
    finally:
        d.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_bouinpt_range_and_split(api, prec):
    """Only listed rows inside [kijs, kijl) change -- the whole tensor is compared -- and two calls over two halves of the range equal one call."""
    d = Dev(api, 12, prec)
    try:
        n = 40
        bfw, f, par, _ = R.make_cases(np.random.default_rng(11), n, d.t.FR, d.t.TH)
        bfw[::7] = 0.0
        ijb = np.random.default_rng(5).permutation(NROW)[:n]
        ibcl, ibcr, f1, par1 = _pairs(bfw, f, par)
        full, pfull = d.bouinpt(ijb, ibcl, ibcr, bfw, f1, par1)
        ks, km, kl = 10, 27, 45
        part, ppart = d.bouinpt(ijb, ibcl, ibcr, bfw, f1, par1, kijs=ks, kijl=kl)
        inside = (ijb >= ks) & (ijb < kl)
        assert 5 < inside.sum() < n - 5
        want = d.fl0.copy()
        want[ijb[inside]] = full[ijb[inside]]
        assert _same(part, want)
        wantp = np.full_like(pfull, -7.0)
        wantp[inside] = pfull[inside]
        assert _same(ppart, wantp)
        fl1 = d.to(d.fl0)
        d.bouinpt(ijb, ibcl, ibcr, bfw, f1, par1, kijs=ks, kijl=km, fl1=fl1)
        two, _ = d.bouinpt(ijb, ibcl, ibcr, bfw, f1, par1, kijs=km, kijl=kl, fl1=fl1)
        assert _same(two, part)
        # an empty range and an empty list change nothing
        none, _ = d.bouinpt(ijb, ibcl, ibcr, bfw, f1, par1, kijs=20, kijl=20)
        assert _same(none, d.fl0)
        none, _ = d.bouinpt(ijb[:0], ibcl[:0], ibcr[:0], bfw[:0], f1, par1)
        assert _same(none, d.fl0)
    finally:
        d.close()


def _femean_sthq(t, fl):
    """FEMEAN (femean.F90:84-121) and STHQ (sthq.F90:75-120) of spectra [n][K][M] in float64"""
    fl = fl.astype(np.float64)
    fr, dfim, delth = (np.asarray(x, dtype=np.float64) for x in (t.FR, t.DFIM, t.DELTH))
    t2 = np.maximum(fl, float(t.EPSMIN)).sum(axis=1)
    em = (t2 * dfim).sum(axis=1) + float(t.WETAIL) * fr[-1] * delth * t2[:, -1]
    fm = (t2 * dfim / fr).sum(axis=1) + float(t.FRTAIL) * delth * t2[:, -1]
    fm = np.maximum(em / fm, fr[0])
    temp = (fl * dfim).sum(axis=2)
    si, ci = (temp * np.sin(np.asarray(t.TH, np.float64))).sum(axis=1), (temp * np.cos(np.asarray(t.TH, np.float64))).sum(axis=1)
    thq = np.arctan2(si, ci)
    return em, np.where(thq < 0, thq + 2 * np.pi, thq), fm


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("nang", [12, 36])
def test_outbc(api, nang, prec):
    """The gathered spectra bit-exact, in record order; EMEAN the bits of column 3 of ecwam_hip_outbs; THQ and FMEAN against numpy with the gates
    of the OUTBS parity test (tests/test_gpu_parity.py::test_outbs_parameters_and_norms: period 1e-12 / 2e-6 relative, direction 1e-9 / 2e-2
    degrees); par = NULL gathers only; and the round trip outbc -> bouinpt with BFW = 0 reproduces the coarse spectra at the fine points."""
    d = Dev(api, nang, prec)
    try:
        rng = np.random.default_rng(13)
        coarse = np.stack([R.spectrum(rng, d.t.FR, d.t.TH).T for _ in range(NROW)]).astype(d.dt)      # [n][K][M]
        fl1 = d.to(coarse)
        nbc = 21
        ijarc = rng.permutation(NROW)[:nbc]
        tij = d.to(ijarc, np.int32)
        par = torch.full((nbc, 3), -7.0, dtype=fl1.dtype, device=d.dev)
        flpts = torch.full((nbc, 36, nang), -7.0, dtype=fl1.dtype, device=d.dev)
        d.ctx.outbc(tij, fl1, flpts, par)
        out5 = torch.zeros((NROW, 5), dtype=fl1.dtype, device=d.dev)
        d.ctx.outbs(0, NROW, fl1, out5)
        only = torch.full((nbc, 36, nang), -7.0, dtype=fl1.dtype, device=d.dev)
        d.ctx.outbc(tij, fl1, only)
        torch.cuda.synchronize()
        assert _same(fl1.cpu().numpy(), coarse)
        p, s = par.cpu().numpy(), flpts.cpu().numpy()
        assert _same(s, np.ascontiguousarray(coarse[ijarc].transpose(0, 2, 1))) and _same(only.cpu().numpy(), s)
        assert _same(p[:, 0], np.ascontiguousarray(out5.cpu().numpy()[ijarc, 3]))
        em, thq, fm = _femean_sthq(d.t, coarse[ijarc])
        tol = 1e-12 if prec == "dp" else 2e-6
        dth = np.abs(p[:, 1].astype(np.float64) - thq)
        dth = np.minimum(dth, 2 * np.pi - dth)
        efm = np.max(np.abs(p[:, 2] - fm) / fm)
        print(f"outbc {nang} {prec}: FMEAN {efm:.2e} relative, THQ {np.degrees(dth.max()):.2e} degrees, EMEAN {np.max(np.abs(p[:, 0] - em) / em):.2e} relative")
        assert efm < tol and np.degrees(dth.max()) < (1e-9 if prec == "dp" else 2e-2) and np.all((p[:, 1] >= 0) & (p[:, 1] < 2 * np.pi + 1e-6))
        # the round trip: the records of outbc as the boundary file of a finer grid, every fine point copying "its" coarse point
        ijb = rng.permutation(NROW)[:nbc]
        fine, po = d.bouinpt(ijb, np.arange(1, nbc + 1), np.zeros(nbc), np.zeros(nbc), s, p)
        assert _same(fine[ijb], coarse[ijarc]) and _same(po, p)
    finally:
        d.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_bouinpt_hostile_means(api, prec):
    """Mean frequencies of zero, a negative one and non-finite ones in some records: the call returns 0, every boundary point that reads none of
    them has its correct values (bit for bit those of a call without the others), and no row that is not listed changes.  The kernel clamps
    every index and guards every conversion to an integer (csrc/nest.hip): this checks that by its results."""
    d = Dev(api, 12, prec)
    try:
        n = 30
        bfw, f, par, _ = R.make_cases(np.random.default_rng(17), n, d.t.FR, d.t.TH)
        ibcl, ibcr, f1, par1 = _pairs(bfw, f, par)
        par1 = par1.astype(d.dt)
        bad = {0: 0.0, 3: -0.1, 8: np.inf, 13: np.nan, 20: -np.inf, 27: 0.0}      # record (0-based) -> its FMEAN
        for rec, v in bad.items():
            par1[rec, 2] = v
        par1[26, 2] = 0.0                                                             # both records of case 13 without a mean frequency
        hit = np.array([(ibcl[i] - 1 in bad) or (ibcr[i] - 1 in bad) for i in range(n)])
        assert 5 <= hit.sum() <= 8
        ijb = np.random.default_rng(19).permutation(NROW)[:n]
        with np.errstate(all="ignore"):
            fl, po = d.bouinpt(ijb, ibcl, ibcr, bfw, f1, par1)                       # HipContext raises unless the call returned 0
        ok = ~hit
        clean, pclean = d.bouinpt(ijb[ok], ibcl[ok], ibcr[ok], bfw[ok], f1, par1)
        assert _same(fl[ijb[ok]], clean[ijb[ok]]) and _same(po[ok], pclean)
        assert np.isfinite(fl[ijb[ok]]).all()
        rest = np.setdiff1d(np.arange(NROW), ijb)
        assert _same(fl[rest], d.fl0[rest])
        # and the same values as the restatement gives for them, within the gates
        ref = [R.bouinpt_point(d.t.FR, bfw[i], ibcl[i], ibcr[i], f1, par1, d.dt) for i in np.nonzero(ok)[0]]
        _check_against(d, clean, pclean, ijb[ok], [r[0] for r in ref], [r[1] for r in ref], "beside hostile means, against the restatement")
    finally:
        d.close()


class Raw:
    """A context through ctypes (ecwam_amd.api validates before the library does) and one small device buffer for every pointer."""

    def __init__(self, prec, nfre=36):
        from ecwam_amd import lib as L

        self.lib = L.load()
        t = Tables(Config(nang=12, nfre=nfre, nfre_red=nfre), DT[prec])
        params = L.make_params(t)
        tp, keep = L.make_tables(t)
        self.h = C.c_void_p()
        rc = self.lib.ecwam_hip_create(C.byref(params), C.byref(tp), 4 if prec == "sp" else 8, 0, C.byref(self.h))
        assert rc == 0, self.lib.ecwam_hip_last_error().decode()
        self.buf = torch.full((8 * 12 * 36,), 3.0, dtype=torch.float64, device="cuda:0")
        self.a = self.buf.data_ptr()

    def bouinpt(self, kijs=0, kijl=0, nijb=0, nboinp=0, null_ctx=False, **over):
        p = dict(ijb=self.a, ibcl=self.a, ibcr=self.a, bfw=self.a, f1=self.a, par1=self.a, fl1=self.a, par_out=None)
        p.update(over)
        rc = self.lib.ecwam_hip_bouinpt(None if null_ctx else self.h, kijs, kijl, nijb, p["ijb"], p["ibcl"], p["ibcr"], p["bfw"], nboinp, p["f1"], p["par1"],
                                        p["fl1"], p["par_out"], None)
        return rc, self.lib.ecwam_hip_last_error().decode()

    def outbc(self, nbc=0, null_ctx=False, **over):
        p = dict(ijarc=self.a, fl1=self.a, flpts=self.a, par=None)
        p.update(over)
        rc = self.lib.ecwam_hip_outbc(None if null_ctx else self.h, nbc, p["ijarc"], p["fl1"], p["flpts"], p["par"], None)
        return rc, self.lib.ecwam_hip_last_error().decode()

    def close(self):
        self.lib.ecwam_hip_destroy(self.h)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_refusals(api, prec):
    """Every case is refused before anything is launched, with its own text; a count of zero launches nothing."""
    c = Raw(prec)
    try:
        assert c.bouinpt()[0] == 0 and c.outbc()[0] == 0                      # the well-formed empty calls
        assert c.bouinpt(kijl=8, nboinp=4)[0] == 0                            # no boundary point: nothing is launched
        assert c.bouinpt(fl1=None, ijb=None, ibcl=None, ibcr=None, bfw=None, f1=None, par1=None)[0] == 0 and c.outbc(ijarc=None, fl1=None, flpts=None)[0] == 0
        torch.cuda.synchronize()
        assert bool((c.buf == 3.0).all())
        assert c.bouinpt(null_ctx=True) == (1, "null context") and c.outbc(null_ctx=True) == (1, "null context")
        assert c.bouinpt(nijb=-1) == (1, "ecwam_hip_bouinpt: negative count") and c.bouinpt(nboinp=-1) == (1, "ecwam_hip_bouinpt: negative count")
        assert c.outbc(nbc=-1) == (1, "ecwam_hip_outbc: negative count")
        assert c.bouinpt(kijs=1, kijl=0) == (1, "ecwam_hip_bouinpt: bad range") and c.bouinpt(kijs=-1) == (1, "ecwam_hip_bouinpt: bad range")
        for k in ("ijb", "ibcl", "ibcr", "bfw", "fl1"):
            assert c.bouinpt(kijl=8, nijb=2, nboinp=2, **{k: None}) == (1, "ecwam_hip_bouinpt: null pointer"), k
        for k in ("f1", "par1"):
            assert c.bouinpt(kijl=8, nijb=2, nboinp=2, **{k: None}) == (1, "ecwam_hip_bouinpt: null pointer (the boundary records)"), k
        assert c.bouinpt(fl1=c.a + 8) == (1, "ecwam_hip_bouinpt: the spectra must be 16-byte aligned")
        for k in ("ijarc", "fl1", "flpts"):
            assert c.outbc(nbc=2, **{k: None}) == (1, "ecwam_hip_outbc: null pointer"), k
    finally:
        c.close()
    c = Raw(prec, nfre=30 if prec == "sp" else 31)      # 30 floats / 31 doubles are no whole number of 16-byte chunks
    try:
        assert c.bouinpt() == (1, "ecwam_hip_bouinpt: the frequencies of a direction are no whole number of 16-byte chunks")
        assert c.outbc()[0] == 0
    finally:
        c.close()


def test_wamintgr_nest(api):
    """set_nest_input / bouinpt and set_nest_output / outbc of the driver on a small synthetic case: the boundary rows equal the direct call, the
    other rows are untouched, and step(); bouinpt(); outbc() repeated twice leaves a finite spectrum."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=36, idelt=450, idelpro=450)
    m = Wamintgr(cfg, G.build_grid(12, mask="continents"), "sp")
    try:
        m.init_synthetic(seed=5)
        assert m.build_weights() == 0
        with pytest.raises(RuntimeError):
            m.bouinpt(np.zeros((1, 36, 12)), np.zeros((1, 3)))
        with pytest.raises(RuntimeError):
            m.outbc()
        n = 24
        rng = np.random.default_rng(23)
        bfw, f, par, _ = R.make_cases(rng, n, m.t.FR, m.t.TH)
        ibcl, ibcr, f1, par1 = _pairs(bfw, f, par)
        ijb = rng.permutation(m.n)[:n]
        with pytest.raises(ValueError):
            m.set_nest_input(np.r_[ijb, ijb[:1]], np.r_[ibcl, 1], np.r_[ibcr, 1], np.r_[bfw, 0.5])      # a row twice
        with pytest.raises(ValueError):
            m.set_nest_input(np.r_[ijb[:-1], m.n], ibcl, ibcr, bfw)                                       # a row this instance does not own
        m.set_nest_input(ijb, ibcl, ibcr, bfw)
        ijarc = rng.permutation(m.n)[:9]
        m.set_nest_output(ijarc)
        before = m.fl1.clone()
        direct = before.clone()
        tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(m.dev)      # noqa: E731
        m.ctx.bouinpt(0, m.n, tt(ijb, np.int32), tt(ibcl, np.int32), tt(ibcr, np.int32), tt(bfw, np.float32), tt(f1, np.float32), tt(par1, np.float32), direct)
        m.gfast_valid = True
        m.bouinpt(f1, par1)
        assert m.gfast_valid is False and torch.equal(m.fl1, direct)
        rest = np.setdiff1d(np.arange(m.fl1.shape[0]), ijb)
        assert torch.equal(m.fl1[rest], before[rest]) and not torch.equal(m.fl1[ijb], before[ijb])
        par_o, flpts = m.outbc()
        assert par_o.shape == (9, 3) and torch.equal(flpts, m.fl1[ijarc].transpose(1, 2))
        with pytest.raises(ValueError):
            m.bouinpt(f1[:5], par1[:5])                                                                   # fewer records than IBFL / IBFR name
        for _ in range(2):
            m.step()
            m.bouinpt(f1, par1)
            par_o, flpts = m.outbc()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(m.fl1).all()) and bool(torch.isfinite(par_o).all()) and bool((par_o[:, 0] > 0).all())
    finally:
        m.ctx.close()
