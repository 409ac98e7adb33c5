"""ecwam_hip_mstart / ecwam_hip_unsetice / ecwam_hip_getspec_noise / ecwam_hip_getspec_tail and the Wamintgr methods over them on the device
(run with -m gpu), against the reference's own results: tests/golden/start_*.npz, recorded by tools/make_golden_start.py from the reference's
unmodified MSTART, UNSETICE and SDEPTHLIM in both precisions.  67 rows, the calls act on [3, 67): three guard rows, and 64 points over
wavefronts that own whole points.  UNSETICE's recorded variants (tests/start_ref.py::UNSETICE_VARIANTS) set LICERUN, LMASKICE and LBIWBK of the
context: LICERUN off beside LMASKICE on is among them at 36 directions.

Gates (tests/start_ref.py::gate, from tests/golden/start_observed.json; nothing in them comes from the device).  The error is per bin over
the point's largest bin.  Double precision: 10 x the largest difference between the numpy restatement and the reference's double precision
results, per routine (1.6e-14 for MSTART and UNSETICE: two mathematical libraries' POW and EXP), 8 eps where that difference is exactly 0
(the tail of GETSPEC, which has no transcendental function: SEMEAN is summed in the reference's order).  Single precision: 3 x the largest
difference between the reference's own single and double precision results (1.5e-5, 2.1e-5, 2.6e-6).
What the device measured against them is in profiles/start_device.txt.
"""
import ctypes as C

import numpy as np
import pytest

import start_ref as S
from ecwam_amd.tables import Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -777.25
A = slice(S.KIJS, S.KIJL)
SPLIT = 30      # the second property: rows [3, 30) and [30, 67) in two calls


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _run(api, shape, prec, name, cases, ranges):
    """One recorded call on the device over the row ranges given (one launch each): the whole buffer [67][NANG][NFRE] afterwards, and what it held before."""
    T = np.float32 if prec == "sp" else np.float64
    r = S.routine_of(name)
    c = cases[r]
    lrun, lmask, lbiwbk, which = S.variant(name) if r == "unsetice" else (1, 1, 1, None)
    ctx = api.HipContext(S.tables(shape, T, lrun, lmask, lbiwbk))
    try:
        before = np.full((S.NROW, shape[0], shape[1]), SENT, T) if r == "mstart" else c["fl"].astype(T)
        fl1 = torch.from_numpy(before.copy()).to(ctx.device)
        ff = torch.from_numpy(c["ff"].astype(T)).to(ctx.device)
        for k0, k1 in ranges:
            if r == "mstart":
                ctx.mstart(k0, k1, fl1, ff, int(name[-1]), *c["params"])
            elif r == "unsetice":
                ctx.unsetice(k0, k1, fl1, ff, S.DELPHI[which])
            else:
                ctx.getspec_tail(k0, k1, fl1, ff, shape[2])
        torch.cuda.synchronize()
        return fl1.cpu().numpy(), before
    finally:
        ctx.close()


# ---- 1. parity with the reference, and the exact properties, per shape and precision
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.shape_tag)
def test_parity_with_the_reference(api, shape, prec):
    g, obs, cases = S.load_golden(shape), S.observed(), S.cached_cases(shape)
    T = np.float32 if prec == "sp" else np.float64
    eps = float(S.tables(shape, T).EPSMIN)
    worst = {}
    for name in S.calls(shape):
        ref = g[f"{name}_{prec}"]
        got, before = _run(api, shape, prec, name, cases, [(S.KIJS, S.KIJL)])
        assert _same_bits(got[: S.KIJS], before[: S.KIJS]), f"{name}: the guard rows changed"
        err = float(S.bin_error(got[A], ref).max())
        gate = S.gate(name, prec, obs)
        print(f"{S.shape_tag(shape)} {name} {prec}: device against the reference {err:.3e} (gate {gate:.3e})")
        worst[name] = (err, gate)
        # a bin the reference gives as exactly 0 / exactly EPSMIN is exactly that
        assert (got[A][ref == 0] == 0).all(), name
        assert (got[A][ref == eps] == T(eps)).all(), name
        # two calls on disjoint rows = one call over both
        two, _ = _run(api, shape, prec, name, cases, [(S.KIJS, SPLIT), (SPLIT, S.KIJL)])
        assert _same_bits(two, got), f"{name}: two calls differ from one"
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.shape_tag)
def test_noise_start_is_bit_exact(api, shape, prec):
    T = np.float32 if prec == "sp" else np.float64
    t = S.tables(shape, T)
    ctx = api.HipContext(t)
    try:
        fl1 = torch.full((S.NROW, shape[0], shape[1]), SENT, dtype=ctx.dtype, device=ctx.device)
        ctx.getspec_noise(S.KIJS, SPLIT, fl1)
        ctx.getspec_noise(SPLIT, S.KIJL, fl1)
        ctx.getspec_noise(5, 5, fl1)      # an empty range: nothing
        torch.cuda.synchronize()
        got = fl1.cpu().numpy()
    finally:
        ctx.close()
    want = np.full_like(got, T(SENT))
    want[A] = t.EPSMIN
    assert _same_bits(got, want)


def test_a_no_op_unsetice_launches_nothing(api):
    """LRESTARTED, or CLDOMAIN == 's' (unsetice.F90:79): the spectra stay as they are."""
    shape = (12, 36, 36)
    c = S.cached_cases(shape)["unsetice"]
    ctx = api.HipContext(S.tables(shape, np.float32))
    try:
        fl1 = torch.from_numpy(c["fl"].astype(np.float32)).to(ctx.device)
        ff = torch.from_numpy(c["ff"].astype(np.float32)).to(ctx.device)
        ctx.unsetice(S.KIJS, S.KIJL, fl1, ff, 1000.0, restarted=True)
        ctx.unsetice(S.KIJS, S.KIJL, fl1, ff, 1000.0, small_domain=True)
        torch.cuda.synchronize()
        assert _same_bits(fl1.cpu().numpy(), c["fl"].astype(np.float32))
    finally:
        ctx.close()


# ---- 2. refusals, with their words (the conventions of ecwam_hip_setice)
class Raw:
    """A context through ctypes (ecwam_amd.api validates before the library does) and one small device buffer for every pointer."""

    def __init__(self, prec):
        from ecwam_amd import lib as L

        self.lib = L.load()
        t = Tables(S.config((12, 36, 36)), np.float32 if prec == "sp" else np.float64)
        params = L.make_params(t)
        tp, keep = L.make_tables(t)
        self.h = C.c_void_p()
        rc = self.lib.ecwam_hip_create(C.byref(params), C.byref(tp), 4 if prec == "sp" else 8, 0, C.byref(self.h))
        assert rc == 0, self.lib.ecwam_hip_last_error().decode()
        self.buf = torch.zeros(8 * 12 * 36, dtype=torch.float64, device="cuda:0")
        self.a = self.buf.data_ptr()

    def call(self, which, kijs=0, kijl=0, null_ctx=False, fl1="a", ff="a", iopti=1, flags=0, nfre_red=36):
        h = None if null_ctx else self.h
        fl1, ff = (self.a if p == "a" else p for p in (fl1, ff))
        if which == "mstart":
            rc = self.lib.ecwam_hip_mstart(h, kijs, kijl, fl1, ff, iopti, 3.0e4, 0.25, 0.7, 0.1, 0.018, 3.0, 0.07, 0.09, None)
        elif which == "unsetice":
            rc = self.lib.ecwam_hip_unsetice(h, kijs, kijl, fl1, ff, 1000.0, flags, None)
        elif which == "getspec_noise":
            rc = self.lib.ecwam_hip_getspec_noise(h, kijs, kijl, fl1, None)
        else:
            rc = self.lib.ecwam_hip_getspec_tail(h, kijs, kijl, fl1, ff, nfre_red, None)
        return rc, self.lib.ecwam_hip_last_error().decode()

    def close(self):
        self.lib.ecwam_hip_destroy(self.h)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_refusals(api, prec):
    """Every case is refused before anything is launched; the ranges are empty wherever the refusal itself needs no points."""
    c = Raw(prec)
    try:
        for w in ("mstart", "unsetice", "getspec_noise", "getspec_tail"):
            who = "ecwam_hip_" + w
            assert c.call(w)[0] == 0, w      # the well-formed empty call
            assert c.call(w, null_ctx=True) == (1, "null context")
            assert c.call(w, kijs=1, kijl=0) == (1, who + ": bad range") and c.call(w, kijs=-1) == (1, who + ": bad range")
            assert c.call(w, kijs=1, kijl=0, fl1=None) == (1, who + ": bad range")      # the range comes first
            assert c.call(w, kijl=8, fl1=None) == (1, who + ": null pointer")
            if w != "getspec_noise":
                assert c.call(w, kijl=8, ff=None) == (1, who + ": null pointer")
            assert c.call(w, fl1=c.a + 8) == (1, who + ": the spectra must be 16-byte aligned")      # for an empty range too
        for iopti in (3, -1):
            rc, msg = c.call("mstart", iopti=iopti)
            assert rc == 1 and msg.startswith("ecwam_hip_mstart: IOPTI must be 0, 1 or 2"), msg
        for nr in (0, 37, -5):
            assert c.call("getspec_tail", nfre_red=nr) == (1, "ecwam_hip_getspec_tail: nfre_red outside 1 .. NFRE")
        assert c.call("unsetice", flags=4) == (1, "ecwam_hip_unsetice: unknown flags")
        assert c.call("unsetice", flags=1)[0] == 0 and c.call("unsetice", flags=2)[0] == 0
    finally:
        c.close()


def test_a_frequency_count_that_fills_no_chunks_is_refused(api):
    """NFRE = 30 in single precision: 30 reals are no whole number of 16-byte chunks."""
    from ecwam_amd.tables import Config

    ctx = api.HipContext(Tables(Config(nang=12, nfre=30, nfre_red=30), np.float32))
    try:
        fl1 = torch.zeros((4, 12, 30), dtype=torch.float32, device=ctx.device)
        ff = torch.zeros((4, 16), dtype=torch.float32, device=ctx.device)
        for call in (lambda: ctx.getspec_noise(0, 0, fl1), lambda: ctx.getspec_tail(0, 0, fl1, ff), lambda: ctx.unsetice(0, 0, fl1, ff, 1000.0),
                     lambda: ctx.mstart(0, 0, fl1, ff, 1, 3.0e4, 0.25, 0.7, 0.1, 0.018, 3.0, 0.07, 0.09)):
            with pytest.raises(api.EcwamHipError, match="no whole number of 16-byte chunks"):
                call()
    finally:
        ctx.close()


# ---- 3. the driver: Wamintgr's methods = the context's calls over the local rows, bit for bit
def test_the_methods_of_the_driver(api):
    from ecwam_amd import grid as G
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=25)

    def model():
        m = Wamintgr(cfg, G.build_grid(16, mask="continents"), "sp")
        m.init_synthetic(seed=3)
        return m

    m, h = model(), model()
    eps = float(m.t.EPSMIN)
    halo0 = m.fl1[m.n:].clone()
    # preset's defaults: IOPTI = 1 with FM = 0 caps the peak frequency at 0 -- an empty sea
    m.gfast_valid = True
    m.cold_start()
    assert m.gfast_valid is False and bool((m.fl1[: m.n] == 0).all())
    # a cold start from the winds
    m.cold_start(iopti=2, fetch=3.0e4, fm=0.25, alfa=0.018, gamma=3.0, sa=0.07, sb=0.09, theta=40.0)
    h.ctx.mstart(0, h.n, h.fl1, h.ff, 2, 3.0e4, 0.25, 40.0 * float(h.t.RAD), 0.25, 0.018, 3.0, 0.07, 0.09)
    torch.cuda.synchronize()
    assert _same_bits(m.fl1.cpu().numpy(), h.fl1.cpu().numpy()) and bool((m.fl1[: m.n] > 0).any())
    assert _same_bits(m.fl1[m.n:].cpu().numpy(), halo0.cpu().numpy())      # the local rows only
    # the end of a GRIB read that stopped at NFRE_RED = 25
    m.gfast_valid = True
    m.getspec_tail()
    h.ctx.getspec_tail(0, h.n, h.fl1, h.ff, 25)
    torch.cuda.synchronize()
    assert m.gfast_valid is False and _same_bits(m.fl1.cpu().numpy(), h.fl1.cpu().numpy())
    # a noise start, then the sea freed from ice
    m.noise_start()
    assert bool((m.fl1[: m.n] == eps).all())
    m.gfast_valid = True
    m.unsetice(restarted=True)
    assert m.gfast_valid is True and bool((m.fl1[: m.n] == eps).all())
    m.unsetice()
    h.ctx.getspec_noise(0, h.n, h.fl1)
    h.ctx.unsetice(0, h.n, h.fl1, h.ff, h.delphi())
    torch.cuda.synchronize()
    assert m.gfast_valid is False and _same_bits(m.fl1.cpu().numpy(), h.fl1.cpu().numpy())
    assert m.delphi() == m.grid.xdella * float(m.t.CIRC) / 360.0      # readmdlconf.F90:136, CIRC in the working precision
    free = (m.ff[: m.n, 2] <= float(m.t.CITHRSH)) & (m.ff[: m.n, 3] > 3.0)
    assert bool(free.any()) and bool((m.fl1[: m.n][free].amax(dim=(1, 2)) > 1.0e-6).all())      # a wind sea where the sea is open
    with pytest.raises(api.EcwamHipError, match="IOPTI must be 0, 1 or 2"):
        m.cold_start(iopti=3)
