"""GPU parity of the refraction paths (IREFRA = 1 depth, 2 currents, 3 depth + currents): GRADI + PROPDOT, the CTUWDRV
checks with the LLCFLCUROFF second call, and PROPAGS2 with every weight rebuilt on the fly, against the oracle's
restatement of the reference's stored-weight scheme (gradi.F90, propdot.F90, ctuwdrv.F90, ctuw.F90, propags2.F90:124-192).

Tolerances: the device forms each weight with the reference's operations in the reference's order (contraction off), so
differences come from the division / reciprocal roundings only: theta-dot terms within 16 eps of their scale, F3 within
32 eps of the spectrum's maximum; CFL flags and CURMASK identical.

The same gates hold against what the reference's own Fortran returned (tests/golden/ctu_*.npz; tests/test_ctu_host.py holds the oracle to these files bit
for bit), there through every build of k_propags2_gen, which must agree bit for bit; the shapes the files cannot hold run against the oracle (below).
"""
import numpy as np
import pytest

import harness as H
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _case(prec, irefra, n_oct=20, nang=24, nred=29, delpro=600, cur_amp=0.8, smooth_depth=True, g=None):
    from ecwam_amd import grid as G, synthetic as syn

    g = G.build_grid(n_oct, mask="continents") if g is None else g
    cfg = Config(nang=nang, nfre=36, nfre_red=nred, idelpro=delpro, idelt=delpro, irefra=irefra)
    dt = H.np_dtype(prec)
    t = Tables(cfg, dt)
    n = g.nsea
    rng = np.random.default_rng(5)
    lat = np.deg2rad(g.lat_deg)
    lon = np.deg2rad(g.ixlg * g.zdello[g.kxlt])
    if smooth_depth:   # shelf-like bathymetry: 20 m .. 900 m, smooth on the grid scale so that the depth refraction respects the CFL limit
        depth = 460.0 + 440.0 * np.sin(2 * lon + 1.0) * np.cos(3 * lat)
    else:
        depth = np.where(rng.uniform(0, 1, n) < 0.3, 10 ** rng.uniform(0.5, 3, n), 998.999)
    depth = np.minimum(depth, 998.999)
    props = syn.depth_props(depth, t, dt)
    land = syn.depth_props(np.array([998.999]), t, dt)

    def ext(a, lv):
        e = np.zeros((n + 1,) + a.shape[1:], dt)
        e[:n] = a
        e[n] = lv
        return e

    u, v = syn.currents(g, amp=cur_amp)
    if irefra < 2:
        u, v = np.zeros(n), np.zeros(n)
    c = dict(g=g, cfg=cfg, t=t, n=n, cg=ext(props["CGROUP"], land["CGROUP"][0]), om=ext(props["OMOSNH2KD"], land["OMOSNH2KD"][0]),
             wn=ext(props["WAVNUM"], land["WAVNUM"][0]), dep=ext(depth.astype(dt), 998.999), u=ext(u.astype(dt), 0.0), v=ext(v.astype(dt), 0.0))
    f1 = np.zeros((n + 1, cfg.nang, cfg.nfre), dt)
    f1[:n] = rng.uniform(0, 1, (n, cfg.nang, cfg.nfre)) ** 4
    c["f1"] = f1
    return c


def _oracle_run(c, prec, llcflcuroff=True):
    from oracle.oracle import Oracle

    o = Oracle(c["cfg"], prec)
    ir = c["cfg"].irefra
    dot = o.propdot(c["g"], ir, c["dep"], c["u"], c["v"], c["wn"], c["cg"], c["om"])
    w = o.ctu_weights_gen(c["g"], ir, c["cg"], c["om"], c["u"], c["v"], dot, float(c["cfg"].idelpro), llcflcuroff=llcflcuroff)
    f3 = o.propags2_gen(c["g"], c["f1"], w) if ir >= 2 else o.propags2(c["g"], c["f1"], w)
    return dot, w, f3


def _device_run(api, c, llcflcuroff=True):
    ctx = api.HipContext(c["t"])
    dev, cfg, n = ctx.device, c["cfg"], c["n"]
    gd = api.grid_to_device(c["g"], ctx.dtype, dev)
    td = {k: torch.from_numpy(c[k]).to(dev) for k in ("cg", "om", "wn", "dep", "u", "v", "f1")}
    refr = torch.zeros((n, 2 * cfg.nang + 5), dtype=ctx.dtype, device=dev)
    fail = torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.propdot(gd, td["dep"], td["u"], td["v"], refr)
    ctx.ctuw_refra(gd, td["cg"], td["om"], td["wn"], refr, fail, float(cfg.idelpro), llcflcuroff=llcflcuroff)
    f3 = torch.full_like(td["f1"], -7.0)
    ctx.propags2_refra(td["f1"], f3, gd, td["cg"], td["om"], td["wn"], refr, float(cfg.idelpro), 0, n)
    torch.cuda.synchronize()
    out = dict(refr=refr.cpu().numpy(), fail=fail.cpu().numpy(), f3=f3.cpu().numpy(), wlat=gd["wlat"].cpu().numpy(),
               wcor=gd["wcor"].cpu().numpy())
    return ctx, gd, td, refr, out


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("irefra", [1, 2, 3])
def test_refraction_parity(api, prec, irefra):
    c = _case(prec, irefra)
    cfg, n, NANG, NR = c["cfg"], c["n"], c["cfg"].nang, c["cfg"].nfre_red
    dot, w, f3ref = _oracle_run(c, prec)
    assert w["NFAIL"] == 0 and np.all(w["CURMASK"] == 1)
    ctx, gd, td, refr, out = _device_run(api, c)
    eps = np.finfo(H.np_dtype(prec)).eps
    r = out["refr"].astype(float)
    # PROPDOT: THD(K) = THDD (IREFRA = 1) or THDC (2, 3); SDOT rebuilt from S0, OMDD as the kernel does
    thd_ref = (dot["THDD"] if irefra == 1 else dot["THDC"]).astype(float)
    sc = max(np.abs(thd_ref).max(), 1e-300)
    assert np.abs(r[:, :NANG] - thd_ref).max() < 16 * eps * sc
    if irefra >= 2:
        cg, om, wn = (c[k][:n, :NR].astype(float) for k in ("cg", "om", "wn"))
        sdot = (r[:, NANG:2 * NANG, None] * cg[:, None, :] + r[:, 2 * NANG + 2, None, None] * om[:, None, :]) * wn[:, None, :]
        ssc = np.abs(dot["SDOT"]).max()
        assert ssc > 0 and np.abs(sdot - dot["SDOT"].astype(float)).max() < 32 * eps * ssc
        assert np.array_equal(out["refr"][:, 2 * NANG], c["u"][:n]) and np.array_equal(out["refr"][:, 2 * NANG + 1], c["v"][:n])
    assert np.all(r[:, 2 * NANG + 3] == 1.0) and int(out["fail"].sum()) == 0
    assert np.array_equal(out["wlat"], w["WLAT"]) and np.array_equal(out["wcor"], w["WCOR"])
    # PROPAGS2
    f3 = out["f3"]
    fsc = np.abs(f3ref).max()
    assert np.abs(f3[:n, :, :NR].astype(float) - f3ref[:n, :, :NR].astype(float)).max() < 32 * eps * fsc
    assert np.array_equal(f3[:n, :, NR:], c["f1"][:n, :, NR:]) and np.all(f3[n] == -7.0)
    # the refraction terms matter in this case (the test would otherwise not exercise them)
    from oracle.oracle import Oracle
    o0 = Oracle(Config(nang=cfg.nang, nfre=cfg.nfre, nfre_red=cfg.nfre_red, idelpro=cfg.idelpro, idelt=cfg.idelt), prec)
    f3_0 = o0.propags2(c["g"], c["f1"], o0.ctu_weights(c["g"], c["cg"], float(cfg.idelpro)))
    assert np.abs(f3ref[:n] - f3_0[:n]).max() > 1e3 * eps * fsc
    # frequency sub-range (fast-wave sub-step): only M <= 5 of rows [3, n-2) rewritten
    f3b = torch.full_like(td["f1"], -7.0)
    ctx.propags2_refra(td["f1"], f3b, gd, td["cg"], td["om"], td["wn"], refr, float(cfg.idelpro), 3, n - 2, 1, 5, copy_rest=False)
    torch.cuda.synchronize()
    f3b = f3b.cpu().numpy()
    assert np.all(f3b[:3] == -7.0) and np.all(f3b[n - 2:] == -7.0) and np.all(f3b[3:n - 2, :, 5:] == -7.0)
    assert np.array_equal(f3b[3:n - 2, :, :5], f3[3:n - 2, :, :5])
    ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_current_cfl_failure_switches_refraction_off_locally(api, prec):
    """LLCFLCUROFF (ctuwdrv.F90:101-118): currents strong enough to break the CFL / weight-range checks at some points.
    The second CTUW call masks the current refraction and frequency shift of exactly those points; what still fails
    afterwards is reported (the reference aborts, ctuwdrv.F90:124-146)."""
    # depth + currents over rough bathymetry: the depth-gradient part of sigma-dot (OMDD, propdot.F90:126) pushes the
    # frequency-shift weights out of range at a few shallow points
    c = _case(prec, 3, delpro=900, cur_amp=6.0, smooth_depth=False)
    n, NANG = c["n"], c["cfg"].nang
    dot, w1, _ = _oracle_run(c, prec, llcflcuroff=False)
    assert w1["NFAIL"] > 0
    dot, w, f3ref = _oracle_run(c, prec, llcflcuroff=True)
    nmask = int((w["CURMASK"] == 0).sum())
    assert nmask == w1["NFAIL"] and 0 < nmask < n
    ctx, gd, td, refr, out = _device_run(api, c, llcflcuroff=True)
    assert np.array_equal(out["refr"][:, 2 * NANG + 3], w["CURMASK"])
    assert np.array_equal(out["fail"], w["FAIL"])
    ok = w["FAIL"] == 0
    eps = np.finfo(H.np_dtype(prec)).eps
    NR = c["cfg"].nfre_red
    d = np.abs(out["f3"][:n, :, :NR].astype(float) - f3ref[:n, :, :NR].astype(float))
    assert d[ok].max() < 32 * eps * np.abs(f3ref).max()
    ctx.close()
    # without the second call the flags are those of the first
    ctx, gd, td, refr, out = _device_run(api, c, llcflcuroff=False)
    assert np.array_equal(out["fail"], w1["FAIL"]) and np.all(out["refr"][:, 2 * NANG + 3] == 1)
    ctx.close()


def test_zero_currents_reduce_to_the_plain_scheme(api):
    """IREFRA = 2 with UCUR = VCUR = 0 everywhere: no upwind switch, no current refraction, no frequency shift -- the
    general branch then differs from the IREFRA = 0 stencil by its summation order only."""
    c = _case("dp", 2, cur_amp=0.0)
    n, NR = c["n"], c["cfg"].nfre_red
    ctx, gd, td, refr, out = _device_run(api, c)
    f3plain = torch.full_like(td["f1"], -7.0)
    ctx.propags2_otf(td["f1"], f3plain, gd, td["cg"], float(c["cfg"].idelpro), 0, n)
    torch.cuda.synchronize()
    a, b = out["f3"][:n, :, :NR], f3plain.cpu().numpy()[:n, :, :NR]
    assert np.abs(a - b).max() < 8 * np.finfo(np.float64).eps * np.abs(b).max()
    ctx.close()


class _LateHalo:
    """Stands in for HaloExchange on emulated ranks: the halo rows hold NaN until `finish`, so an interior pass that read
    one would poison its result."""

    def __init__(self, m, source):
        self.m, self.source = m, source

    def start(self, fl):
        fl[self.m.n: self.m.n + self.m.dom.nh] = float("nan")
        return []

    def finish(self, reqs):
        glob = self.source()
        hg = torch.from_numpy(np.asarray(self.m.dom.halo_global, dtype=np.int64)).to(glob.device)
        self.m.fl1[self.m.n: self.m.n + self.m.dom.nh] = glob[hg]

    def __call__(self, fl):
        self.finish(self.start(fl))


@pytest.mark.parametrize("irefra,weights", [(0, "otf"), (0, "stored"), (2, "otf"), (3, "otf")])
def test_decomposed_step_with_overlapped_exchange_is_bit_identical(api, irefra, weights):
    """Wamintgr.propag on 3 emulated ranks -- halo exchange posted, interior rows advected, exchange completed, the two
    ends of the band advected (what `bench.py --gpus N` runs; with currents the halo rows of DEPTH/UCUR/VCUR come from the
    global fields as PROENVHALO exchanges them) -- reproduces the single-domain run bit for bit."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=28, idelt=600, idelpro=600, irefra=irefra)
    g = G.build_grid(20, mask="continents")
    ref = Wamintgr(cfg, g, "sp", weights=weights)
    ref.init_synthetic(seed=11)
    assert ref.build_weights() == 0
    nr = 3
    parts = []
    snapshot = {}
    for r in range(nr):
        m = Wamintgr(cfg, g, "sp", rank=r, nranks=nr, weights=weights)
        m.init_synthetic(seed=11)
        assert m.build_weights() == 0
        a, b = m.interior
        assert 0 < a < b < m.n or r in (0, nr - 1)                 # a band in the middle has halo readers at both ends
        assert b - a > 0.5 * m.n
        m.halo = _LateHalo(m, lambda: snapshot["glob"])
        parts.append(m)
    if irefra:
        assert float(ref.refr[:, 2 * cfg.nang].abs().max()) > 0.1     # currents present
    for _ in range(2):
        ref.step()
        snapshot["glob"] = torch.cat([m.fl1[: m.n] for m in parts])   # owned rows of every rank at the old time level
        for m in parts:
            m.step()
    torch.cuda.synchronize()
    got = torch.cat([m.fl1[: m.n] for m in parts]).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref.fl1[: g.nsea].cpu().numpy())
    for m in parts + [ref]:
        m.ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_proenvhalo_on_the_device_equals_the_host_assembly(api, prec):
    """PROENVHALO (proenvhalo.F90:63-107) on the device: owned rows packed from the device-resident fields, halo rows exchanged as rows of
    3 NFRE + 3 reals (here: copied from the owners' packed rows, what MPEXCHNG delivers), land slot from WVPRPT_LAND -- the extended DEPTH /
    UCUR / VCUR / OMOSNH2KD / WAVNUM / CGROUP arrays of every rank equal those assembled on the host from the global fields bit for bit, and
    so do the dot terms and CFL flags built from them."""
    from ecwam_amd import grid as G
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=28, idelt=600, idelpro=600, irefra=3)
    g = G.build_grid(20, mask="continents")
    nr = 3
    host = [Wamintgr(cfg, g, prec, rank=r, nranks=nr) for r in range(nr)]
    dev = [Wamintgr(cfg, g, prec, rank=r, nranks=nr) for r in range(nr)]
    for m in host + dev:
        m.init_synthetic(seed=11)                       # extended rows assembled on the host from the global synthetic fields
    names = ("depth_ext", "u_ext", "v_ext", "omosnh2kd_ext", "wavnum_ext", "cgroup_ext")
    packed = []
    for m, h in zip(dev, host):
        n = m.n
        own = [getattr(h, k)[:n].clone() for k in names[:4]]
        for k in names:                                  # poison what PROENVHALO has to rebuild
            getattr(m, k).fill_(float("nan"))
        packed.append(m.proenvhalo_pack(*own))
    owned = torch.cat([b[: m.n] for b, m in zip(packed, dev)])            # rows of all ranks in global point order
    for m, b in zip(dev, packed):
        hg = torch.from_numpy(np.asarray(m.dom.halo_global, dtype=np.int64)).to(owned.device)
        b[m.n: m.n + m.dom.nh] = owned[hg]                                 # MPEXCHNG(BUFFER_EXT, 3*NFRE_RED+5, 1, 1)
        m.proenvhalo_unpack()
    torch.cuda.synchronize()
    for m, h in zip(dev, host):
        for k in names:
            assert torch.equal(getattr(m, k), getattr(h, k)), k
        assert m.weights_ready is False
        assert m.build_weights() == h.build_weights()
        assert torch.equal(m.refr, h.refr) and torch.equal(m.cflfail, h.cflfail)
    assert float(host[1].u_ext.abs().max()) > 0.1 and host[1].dom.nh > 0
    for m in host + dev:
        m.ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("irefra", [0, 2])
def test_subgrid_obstructions(api, prec, irefra):
    """LSUBGRID (ctuw.F90:703-733): the transmission coefficients OBSLAT/OBSLON/OBSCOR scale the space weights of the
    neighbours after the checks; SUMWN is left alone (blocked energy is lost).  Stored weights, on-the-fly weights and the
    refraction kernel against the oracle; switching the table off restores the plain result."""
    from ecwam_amd import synthetic as syn

    c = _case(prec, irefra)
    cfg, n, NR, g = c["cfg"], c["n"], c["cfg"].nfre_red, c["g"]
    obs = syn.obstructions(g, cfg.nfre).astype(H.np_dtype(prec))
    from oracle.oracle import Oracle
    o = Oracle(cfg, prec)
    o.set_obstructions(obs)
    if irefra:
        dot = o.propdot(g, irefra, c["dep"], c["u"], c["v"], c["wn"], c["cg"], c["om"])
        w = o.ctu_weights_gen(g, irefra, c["cg"], c["om"], c["u"], c["v"], dot, float(cfg.idelpro))
        f3ref = o.propags2_gen(g, c["f1"], w)
    else:
        w = o.ctu_weights(g, c["cg"], float(cfg.idelpro))
        f3ref = o.propags2(g, c["f1"], w)
    assert w["NFAIL"] == 0
    o.set_obstructions(None)
    w0 = o.ctu_weights(g, c["cg"], float(cfg.idelpro))
    assert np.array_equal(w0["SUMWN"], w["SUMWN"]) if not irefra else True
    assert (w["WLONN"] <= o.ctu_weights_gen(g, irefra, c["cg"], c["om"], c["u"], c["v"], dot, float(cfg.idelpro))["WLONN"]).all() if irefra else (w["WLONN"] <= w0["WLONN"]).all()
    ctx = api.HipContext(c["t"])
    dev = ctx.device
    gd = api.grid_to_device(g, ctx.dtype, dev)
    td = {k: torch.from_numpy(c[k]).to(dev) for k in ("cg", "om", "wn", "dep", "u", "v", "f1")}
    tobs = torch.from_numpy(obs).to(dev)
    ctx.set_obstructions(tobs)
    fail = torch.zeros(n, dtype=torch.int32, device=dev)
    eps = np.finfo(H.np_dtype(prec)).eps
    fsc = np.abs(f3ref).max()
    if irefra:
        refr = torch.zeros((n, 2 * cfg.nang + 5), dtype=ctx.dtype, device=dev)
        ctx.propdot(gd, td["dep"], td["u"], td["v"], refr)
        ctx.ctuw_refra(gd, td["cg"], td["om"], td["wn"], refr, fail, float(cfg.idelpro))
        f3 = torch.full_like(td["f1"], -7.0)
        ctx.propags2_refra(td["f1"], f3, gd, td["cg"], td["om"], td["wn"], refr, float(cfg.idelpro), 0, n)
        torch.cuda.synchronize()
        got = f3.cpu().numpy()
        assert np.abs(got[:n, :, :NR].astype(float) - f3ref[:n, :, :NR].astype(float)).max() < 32 * eps * fsc
        ctx.set_obstructions(None)
        f3b = torch.full_like(td["f1"], -7.0)
        ctx.propags2_refra(td["f1"], f3b, gd, td["cg"], td["om"], td["wn"], refr, float(cfg.idelpro), 0, n)
        torch.cuda.synchronize()
        assert np.abs(f3b.cpu().numpy()[:n] - got[:n]).max() > 1e3 * eps * fsc       # the table acted
    else:
        wdev = torch.zeros((n, 8, cfg.nang * NR), dtype=ctx.dtype, device=dev)
        ctx.ctuw(gd, td["cg"], wdev, fail, float(cfg.idelpro))
        f3s = torch.full_like(td["f1"], -7.0)
        ctx.propags2(td["f1"], f3s, gd["klon"], gd["klat"], gd["kcor"], wdev, 0, n)
        f3o = torch.full_like(td["f1"], -7.0)
        ctx.propags2_otf(td["f1"], f3o, gd, td["cg"], float(cfg.idelpro), 0, n)
        f3p = torch.full_like(td["f1"], -7.0)
        ctx.propags2_otf(td["f1"], f3p, gd, td["cg"], float(cfg.idelpro), 3, n - 2, 1, 5, copy_rest=False)   # scalar kernel variant
        torch.cuda.synchronize()
        got = f3o.cpu().numpy()
        H.assert_same_advection(got, f3s.cpu().numpy(), eps, fsc)                    # stored and on-the-fly weights
        assert np.array_equal(f3p.cpu().numpy()[3:n - 2, :, :5], got[3:n - 2, :, :5])
        assert np.abs(got[:n, :, :NR].astype(float) - f3ref[:n, :, :NR].astype(float)).max() < 16 * eps * fsc
        ctx.set_obstructions(None)
        f3b = torch.full_like(td["f1"], -7.0)
        ctx.propags2_otf(td["f1"], f3b, gd, td["cg"], float(cfg.idelpro), 0, n)
        torch.cuda.synchronize()
        plain = o.propags2(g, c["f1"], w0)
        assert np.abs(f3b.cpu().numpy()[:n, :, :NR].astype(float) - plain[:n, :, :NR].astype(float)).max() < 16 * eps * fsc
        assert np.abs(f3b.cpu().numpy()[:n] - got[:n]).max() > 1e3 * eps * fsc
        # energy only leaves: the obstructed field never exceeds the open one
        assert (got[:n, :, :NR] <= f3b.cpu().numpy()[:n, :, :NR] * (1 + 8 * eps) + 1e-300).all()
    assert int(fail.sum()) == 0
    ctx.close()


def test_decomposed_step_with_obstructions_is_bit_identical(api):
    from ecwam_amd import grid as G, synthetic as syn
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=28, idelt=600, idelpro=600)
    g = G.build_grid(20, mask="continents")
    obs = syn.obstructions(g, cfg.nfre)
    ref = Wamintgr(cfg, g, "sp")
    ref.init_synthetic(seed=11)
    ref.set_obstructions(obs)
    assert ref.build_weights() == 0
    plain = Wamintgr(cfg, g, "sp")
    plain.init_synthetic(seed=11)
    parts, snapshot = [], {}
    for r in range(3):
        m = Wamintgr(cfg, g, "sp", rank=r, nranks=3)
        m.init_synthetic(seed=11)
        m.set_obstructions(obs)
        assert m.build_weights() == 0
        m.halo = _LateHalo(m, lambda: snapshot["glob"])
        parts.append(m)
    for _ in range(2):
        ref.step()
        plain.step()
        snapshot["glob"] = torch.cat([m.fl1[: m.n] for m in parts])
        for m in parts:
            m.step()
    torch.cuda.synchronize()
    got = torch.cat([m.fl1[: m.n] for m in parts]).cpu().numpy()
    assert np.array_equal(got, ref.fl1[: g.nsea].cpu().numpy())
    assert not np.array_equal(got, plain.fl1[: g.nsea].cpu().numpy())
    for m in parts + [ref, plain]:
        m.ctx.close()


# ---- the device against what the reference's own Fortran returned (tests/golden/ctu_*.npz, tools/make_golden_ctu.py) ----------------------------------------------
# The gates are the ones the device has against the oracle above (THD 16 eps, SDOT and F3 32 eps of their scales, 16 eps at IREFRA 0 as
# test_ctuw_and_propags2_parity; flags and CURMASK identical); the oracle equals these files bit for bit (tests/test_ctu_host.py).  NFRE_RED is 26: the
# full range 1..26 has even bounds and takes k_propags2_gen<T, 2, false, OBS>; a sub-range with an odd bound and an F1 / F3 pair off 16-byte alignment
# take <T, 1, false, OBS> (launch_propags2_gen); the checks of ctuw_refra run <T, 1, true, false>.
import ctu_ref as CT  # noqa: E402
import propags_ref as P  # noqa: E402

SENTINEL = -7.0


def _report(*a):
    print("CTUPIN", *a)


class _CtuDevice:
    """The inputs of a recorded case on the device, and the calls of Wamintgr.build_weights / propag on them."""

    def __init__(self, api, name, prec):
        self.T = T = CT.PREC[prec]
        self.name, self.prec = name, prec
        self.irefra, self.with_obs, self.ifm, _ = CT.CASES[name]
        self.c = c = CT.make_case(name, T)
        self.ctx = ctx = api.HipContext(P.tables_of(T, CT.NANG, CT.NFRE, CT.NFRE_RED, self.irefra))
        self.dev = dev = ctx.device
        self.gd = api.grid_to_device(CT.grid_view(c), ctx.dtype, dev)
        self.n = self.gd["n"]
        self.td = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("cg", "om", "wn", "depth", "u", "v", "f1")}
        ctx.set_obstructions(None if c["obs"] is None else torch.from_numpy(c["obs"]).to(dev))
        self.env = (self.td["cg"], self.td["om"], self.td["wn"])

    def weights(self, llcflcuroff=True):
        """PROPDOT, then CTUWDRV per frequency range -> REFR [n][2 NANG + 5], CFLFAIL [n]"""
        refr = torch.zeros((self.n, 2 * CT.NANG + 5), dtype=self.ctx.dtype, device=self.dev)
        fail = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        self.ctx.propdot(self.gd, self.td["depth"], self.td["u"], self.td["v"], refr)
        for i, (dt, ms, me) in enumerate(CT.ranges(self.name)):
            self.ctx.ctuw_refra(self.gd, *self.env, refr, fail, dt, ms, me, llcflcuroff=llcflcuroff, frange=i)
        return refr, fail

    def sentinel_like_f1(self, offset=0):
        """F1 and a sentinel-filled F3, `offset` elements off the alignment of the allocation"""
        f1 = self.td["f1"]
        if not offset:
            return f1, torch.full_like(f1, SENTINEL)
        size = f1.numel()
        a, b = (torch.full((size + 4,), SENTINEL, dtype=f1.dtype, device=self.dev) for _ in range(2))
        v1, v3 = a[offset:offset + size].view(f1.shape), b[offset:offset + size].view(f1.shape)
        v1.copy_(f1)
        assert v1.data_ptr() % 16 != 0 and v3.data_ptr() % 16 != 0
        return v1, v3

    def advect(self, refr, f1, f3, dt, ms, me, frange=0, rows=None):
        k0, k1 = rows or (0, self.n)
        self.ctx.propags2_refra(f1, f3, self.gd, *self.env, refr, dt, k0, k1, ms, me, copy_rest=False, frange=frange)

    def step(self, refr):
        """PROPAG_WAM's sequence (propag_wam.F90:247-313) -> F3 on the host"""
        f1, f3 = self.sentinel_like_f1()
        f1 = f1.clone()
        rg = CT.ranges(self.name)
        for i, (dt, ms, me) in enumerate(rg):
            self.advect(refr, f1, f3, dt, ms, me, frange=i)
        if self.ifm:
            self.ctx.copy_freq_range(f3, f1, self.n, 1, self.ifm)
            self.advect(refr, f1, f3, rg[0][0], 1, self.ifm, frange=0)
        torch.cuda.synchronize()
        return f3.cpu().numpy()


def _check_untouched(f3, n, nr):
    assert np.all(f3[:n, :, nr:] == SENTINEL), "frequencies above NFRE_RED were written"
    assert np.all(f3[n:] == SENTINEL), "the land row was written"


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("name", [k for k, v in CT.CASES.items() if v[0] >= 1])
def test_device_against_the_reference_fixtures(api, name, prec):
    """PROPDOT -> CTUWDRV -> PROPAGS2 on the device against the recorded results of the reference's own routines; then the same stencil through the other
    builds of k_propags2_gen, which must give the same bits on the frequencies they share."""
    d = _CtuDevice(api, name, prec)
    fx = CT.load_fixture(name)
    T, n, NANG, NR, irefra, c = d.T, d.n, CT.NANG, CT.NFRE_RED, d.irefra, d.c
    eps = np.finfo(T).eps
    _, fail1 = d.weights(llcflcuroff=False)
    refr, fail = d.weights()
    torch.cuda.synchronize()
    r = refr.cpu().numpy().astype(float)
    # the dot terms: THD(K) = THDD (IREFRA = 1) or THDC (2, 3); SDOT rebuilt from S0, OMDD as the kernel does
    thd_ref = fx[f"thdd_{prec}" if irefra == 1 else f"thdc_{prec}"].astype(float)
    sc = np.abs(thd_ref).max()
    e_thd = np.abs(r[:, :NANG] - thd_ref).max() / (eps * sc)
    e_sdot = 0.0
    if irefra >= 2:
        mi = [m - 1 for m in CT.SDOT_M]
        cg, om, wn = (c[k][:n][:, mi].astype(float) for k in ("cg", "om", "wn"))
        sdot = (r[:, NANG:2 * NANG, None] * cg[:, None, :] + r[:, 2 * NANG + 2, None, None] * om[:, None, :]) * wn[:, None, :]
        sref = fx[f"sdot_{prec}"].astype(float)
        ssc = np.abs(sref).max()
        assert ssc > 0
        e_sdot = np.abs(sdot - sref).max() / (eps * ssc)
    f3 = d.step(refr)
    f3ref = fx[f"f3_{prec}"].astype(float)
    fsc = np.abs(f3ref).max()
    e_f3 = np.abs(f3[:n, :, :NR].astype(float) - f3ref).max() / (eps * fsc)
    _report(name, prec, f"THD {e_thd:.2f} eps  SDOT {e_sdot:.2f} eps  F3 {e_f3:.2f} eps")
    assert sc > 0 and e_thd < 16
    assert e_sdot < 32
    # flags of the first call, both CURMASK slots, the final flags
    assert np.array_equal(fail1.cpu().numpy(), fx[f"fail1_{prec}"].max(axis=1))
    assert np.array_equal(refr.cpu().numpy()[:, 2 * NANG + 3:2 * NANG + 5], fx[f"curmask_{prec}"])
    assert np.array_equal(fail.cpu().numpy(), fx[f"fail_{prec}"].max(axis=1))
    assert e_f3 < 32
    _check_untouched(f3, n, NR)
    # ---- the other builds: one time step and CURMASK slot for every variant, so that they differ in the build alone
    dt = float(CT.IDELPRO)
    full = torch.full_like(d.td["f1"], SENTINEL)
    d.advect(refr, d.td["f1"], full, dt, 1, NR)                                   # VW = 2
    parts = torch.full_like(d.td["f1"], SENTINEL)
    d.advect(refr, d.td["f1"], parts, dt, 1, 5)                                   # VW = 1: an odd upper bound
    d.advect(refr, d.td["f1"], parts, dt, 6, 25)                                  # VW = 1: an odd lower bound
    u1, u3 = d.sentinel_like_f1(offset=1)
    d.advect(refr, u1, u3, dt, 1, NR)                                             # VW = 1: not 16-byte aligned
    torch.cuda.synchronize()
    full, parts, u3 = full.cpu().numpy(), parts.cpu().numpy(), u3.cpu().numpy()
    if not d.ifm:
        assert np.array_equal(full, f3)
    _check_untouched(full, n, NR)
    _check_untouched(u3, n, NR)
    assert np.all(parts[:n, :, 25:] == SENTINEL) and np.all(parts[n:] == SENTINEL)
    assert np.array_equal(parts[:n, :, :25], full[:n, :, :25]), int((parts[:n, :, :25] != full[:n, :, :25]).sum())
    assert np.array_equal(u3, full), int((u3 != full).sum())
    assert np.abs(full[:n, :, :NR] - c["f1"][:n, :, :NR]).max() > 0.05            # the step moved the spectrum
    d.ctx.close()


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("name", ["irefra0", "obs_irefra0"])
def test_device_against_the_reference_fixtures_irefra0(api, name, prec):
    """IREFRA 0: the on-the-fly stencil and CTUW + the stored-weight stencil against the recorded F3, within the 16 eps of
    test_ctuw_and_propags2_parity; no flag is raised."""
    d = _CtuDevice(api, name, prec)
    fx = CT.load_fixture(name)
    T, n, NANG, NR = d.T, d.n, CT.NANG, CT.NFRE_RED
    eps = np.finfo(T).eps
    dt = float(CT.IDELPRO)
    f1 = d.td["f1"]
    w = torch.zeros((n, 8, NANG * NR), dtype=d.ctx.dtype, device=d.dev)
    fail = torch.zeros(n, dtype=torch.int32, device=d.dev)
    d.ctx.ctuw(d.gd, d.td["cg"], w, fail, dt)      # CTUWINI first: it snaps WLAT / WCOR next to land, for the on-the-fly weights too
    f3o = torch.full_like(f1, SENTINEL)
    d.ctx.propags2_otf(f1, f3o, d.gd, d.td["cg"], dt, 0, n, copy_rest=False)
    f3s = torch.full_like(f1, SENTINEL)
    d.ctx.propags2(f1, f3s, d.gd["klon"], d.gd["klat"], d.gd["kcor"], w, 0, n, copy_rest=False)
    torch.cuda.synchronize()
    f3ref = fx[f"f3_{prec}"].astype(float)
    fsc = np.abs(f3ref).max()
    for what, f3 in (("on the fly", f3o.cpu().numpy()), ("stored", f3s.cpu().numpy())):
        e = np.abs(f3[:n, :, :NR].astype(float) - f3ref).max() / (eps * fsc)
        _report(name, prec, what, f"F3 {e:.2f} eps")
        assert e < 16, what
        _check_untouched(f3, n, NR)
    assert not fail.cpu().numpy().any() and not fx[f"fail1_{prec}"].any() and not fx[f"fail_{prec}"].any()
    assert np.all(fx[f"curmask_{prec}"] == 1)
    d.ctx.close()


# ---- the shapes the fixtures cannot hold, against the oracle the fixtures pin ---------------------------------------------------------------------------------------
_SWEEP_GRID = {}


def _sweep_grid():
    """the O5 grid of tests/test_gpu_propags.py: 176 sea points, eleven tiles of k_propags2_gen"""
    if "g" not in _SWEEP_GRID:
        from ecwam_amd import grid

        _SWEEP_GRID["g"] = grid.build_grid(5, "continents", seed=11, land_fraction=0.3)
    return _SWEEP_GRID["g"]


@pytest.mark.parametrize("with_obs", [False, True], ids=["plain", "obstructed"])
@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("irefra", [1, 2, 3])
@pytest.mark.parametrize("shape", [(12, 26), (36, 36), (48, 36), (24, 28)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_refraction_parity_at_the_other_shapes(api, shape, irefra, prec, with_obs):
    """The gates of test_refraction_parity at 12, 36 and 48 directions and at an even NFRE_RED below NFRE (all of them take the VW = 2 build; with the table
    the OBS build), with a time step that makes the weights large; then row ranges that cut the 16-point tile of k_propags2_gen."""
    from ecwam_amd import synthetic as syn
    from oracle.oracle import Oracle

    g = _sweep_grid()
    c = _case(prec, irefra, nang=shape[0], nred=shape[1], delpro=5000, g=g)
    cfg, n, NANG, NR = c["cfg"], c["n"], c["cfg"].nang, c["cfg"].nfre_red
    assert n > 10 * 16      # more than one block's worth of tiles
    delpro = float(cfg.idelpro)
    obs = syn.obstructions(g, cfg.nfre).astype(H.np_dtype(prec)) if with_obs else None
    o = Oracle(cfg, prec)
    o.set_obstructions(obs)
    dot = o.propdot(g, irefra, c["dep"], c["u"], c["v"], c["wn"], c["cg"], c["om"])
    w = o.ctu_weights_gen(g, irefra, c["cg"], c["om"], c["u"], c["v"], dot, delpro)
    f3ref = o.propags2_gen(g, c["f1"], w) if irefra >= 2 else o.propags2(g, c["f1"], w)
    o.set_obstructions(None)
    assert w["NFAIL"] == 0 and np.all(w["CURMASK"] == 1) and w["SUMWN"].max() > 0.2      # the weights are not small: a fifth of the CFL limit or more
    ctx = api.HipContext(c["t"])
    dev = ctx.device
    gd = api.grid_to_device(g, ctx.dtype, dev)
    td = {k: torch.from_numpy(c[k]).to(dev) for k in ("cg", "om", "wn", "dep", "u", "v", "f1")}
    ctx.set_obstructions(None if obs is None else torch.from_numpy(obs).to(dev))
    refr = torch.zeros((n, 2 * NANG + 5), dtype=ctx.dtype, device=dev)
    fail = torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.propdot(gd, td["dep"], td["u"], td["v"], refr)
    ctx.ctuw_refra(gd, td["cg"], td["om"], td["wn"], refr, fail, delpro)
    f3 = torch.full_like(td["f1"], SENTINEL)
    ctx.propags2_refra(td["f1"], f3, gd, td["cg"], td["om"], td["wn"], refr, delpro, 0, n)
    torch.cuda.synchronize()
    eps = np.finfo(H.np_dtype(prec)).eps
    r = refr.cpu().numpy().astype(float)
    thd_ref = (dot["THDD"] if irefra == 1 else dot["THDC"]).astype(float)
    sc = max(np.abs(thd_ref).max(), 1e-300)
    assert np.abs(r[:, :NANG] - thd_ref).max() < 16 * eps * sc
    if irefra >= 2:
        cg, om, wn = (c[k][:n, :NR].astype(float) for k in ("cg", "om", "wn"))
        sdot = (r[:, NANG:2 * NANG, None] * cg[:, None, :] + r[:, 2 * NANG + 2, None, None] * om[:, None, :]) * wn[:, None, :]
        ssc = np.abs(dot["SDOT"]).max()
        assert ssc > 0 and np.abs(sdot - dot["SDOT"].astype(float)).max() < 32 * eps * ssc
        assert np.array_equal(refr.cpu().numpy()[:, 2 * NANG], c["u"][:n]) and np.array_equal(refr.cpu().numpy()[:, 2 * NANG + 1], c["v"][:n])
    assert np.all(r[:, 2 * NANG + 3] == 1.0) and int(fail.sum()) == 0
    assert np.array_equal(gd["wlat"].cpu().numpy(), w["WLAT"]) and np.array_equal(gd["wcor"].cpu().numpy(), w["WCOR"])
    f3 = f3.cpu().numpy()
    fsc = np.abs(f3ref).max()
    assert np.abs(f3[:n, :, :NR].astype(float) - f3ref[:n, :, :NR].astype(float)).max() < 32 * eps * fsc
    assert np.array_equal(f3[:n, :, NR:], c["f1"][:n, :, NR:]) and np.all(f3[n] == SENTINEL)
    # the refraction terms matter (against IREFRA = 0 with the same table)
    o0 = Oracle(Config(nang=cfg.nang, nfre=cfg.nfre, nfre_red=cfg.nfre_red, idelpro=cfg.idelpro, idelt=cfg.idelt), prec)
    o0.set_obstructions(obs)
    f3_0 = o0.propags2(g, c["f1"], o0.ctu_weights(g, c["cg"], delpro))
    o0.set_obstructions(None)
    assert np.abs(f3ref[:n] - f3_0[:n]).max() > 1e3 * eps * fsc
    # row ranges across the tile: KIJS off a multiple of 16 with a partial last tile, less than one tile, one point
    assert (n - 2 - 3) % 16 != 0 and (n - 5) % 16 != 0
    for k0, k1 in ((3, n - 2), (0, n - 5), (21, 30), (37, 38)):
        part = torch.full_like(td["f1"], SENTINEL)
        ctx.propags2_refra(td["f1"], part, gd, td["cg"], td["om"], td["wn"], refr, delpro, k0, k1)
        torch.cuda.synchronize()
        part = part.cpu().numpy()
        assert np.all(part[:k0] == SENTINEL) and np.all(part[k1:] == SENTINEL), (k0, k1)
        assert np.array_equal(part[k0:k1], f3[k0:k1]), (k0, k1)
    ctx.close()
