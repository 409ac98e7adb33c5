"""The first-order propagation scheme on the device (IPROPAGS = 0: ecwam_hip_propags_dot, ecwam_hip_propags; include/ecwam_hip_propags.h).

The gate is THE SAME BITS, in single and in double precision: PROPAGS, CHECKCFL, PROPDOT and GRADI hold only + - * / and ABS (MIN and SIGN in the clamp of the
current gradients), every one correctly rounded, and the kernels keep the reference's order without contraction.
  1  against the fixtures tests/golden/propags_*.npz: what the reference's own unmodified Fortran returned (tools/make_golden_propags.py)
  2  the shapes the fixtures do not have, against the restatement tests/propags_ref.py (which tests/test_propags_host.py holds to the fixtures bit for bit)
  3  row ranges, sentinels   4  the CFL check   5  the driver Wamintgr(ipropags=0)   6  the refusals
"""
import numpy as np
import pytest

import propags_ref as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PREC = {"sp": np.float32, "dp": np.float64}
SENTINEL = -7.0


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _context(api, T, nang, nfre, nfre_red, irefra):
    return api.HipContext(P.tables_of(T, nang, nfre, nfre_red, irefra))


def _upload(ctx, c, ngy):
    """the inputs of propags_ref.make_inputs on the device: the grid dict of HipContext.propags and the fields"""
    dev = ctx.device

    def ti(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)

    def tr(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    n = c["klon"].shape[0]
    gd = dict(n=n, nland=c["nland"], ngy=ngy, xdella=c["xdella"], kxlt=ti(c["kxlt"]), zdello=tr(c["zdello"]), cosph=tr(c["cosph"]), sinph=tr(c["sinph"]),
              klon=ti(c["klon"]), klat=ti(c["klat"]), wlat=tr(c["wlat"]), cosphm1_ext=tr(c["cosphm1"]), dellam1_ext=tr(c["dellam1"]))
    td = {k: tr(c[k]) for k in ("cg", "om", "wn", "depth", "u", "v", "f1")}
    return gd, td


def _device(api, c, T, nang, nfre, ngy, kijs=0, kijl=None, copy_rest=False, f3=None, check_only=False, cflfail0=None, ctx=None):
    """-> dict(dot, f3 [nrow][K][NFRE], cfl [n][K][11], fail [n]) of the two calls on the inputs c"""
    ctx = ctx or _context(api, T, nang, nfre, c["nr"], c["irefra"])
    gd, td = _upload(ctx, c, ngy)
    n, dev = gd["n"], ctx.device
    kijl = n if kijl is None else kijl
    ctx.set_obstructions(None if c["obs"] is None else torch.from_numpy(c["obs"]).to(dev))
    dot = None
    if c["irefra"]:
        dot = torch.full((n, P.dot_width(nang)), SENTINEL, dtype=ctx.dtype, device=dev)
        ctx.propags_dot(gd, td["depth"], td["u"], td["v"], dot, icase=c["icase"])
    if f3 is None and not check_only:
        f3 = torch.full_like(td["f1"], SENTINEL)
    cfl = torch.full((n, nang, P.NCFL), SENTINEL, dtype=ctx.dtype, device=dev)
    fail = torch.zeros(n, dtype=torch.int32, device=dev) if cflfail0 is None else torch.from_numpy(cflfail0.astype(np.int32)).to(dev)
    env = dict(omosnh2kd_ext=td["om"], wavnum_ext=td["wn"], u_ext=td["u"], v_ext=td["v"], dot=dot) if c["irefra"] else {}
    f1_before = td["f1"].clone()
    ctx.propags(td["f1"], None if check_only else f3, gd, td["cg"], c["delpro"], kijs, kijl, copy_rest=copy_rest, cfl=cfl, cflfail=fail, icase=c["icase"],
                irgg=c["irgg"], delphi=float(c["delphi"]), **env)
    torch.cuda.synchronize()
    assert torch.equal(td["f1"], f1_before), "F1 was written"
    return dict(ctx=ctx, dot=None if dot is None else dot.cpu().numpy(), f3=None if f3 is None else f3.cpu().numpy(), cfl=cfl.cpu().numpy(),
                fail=fail.cpu().numpy(), f3_dev=f3)


def _assert_bits(got, want, what):
    assert P.same_bits(got, want), (what, "differing elements:", int((np.asarray(got) != np.asarray(want)).sum()), "largest difference:",
                                    float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()))


# ---- 1. the device against what the reference's own Fortran returned -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("name", list(P.CASES))
def test_device_reproduces_the_reference_bit_for_bit(api, name, prec):
    T = PREC[prec]
    fx = P.load_fixture(name)
    c = P.make_case(name, T)
    g = P.fixture_grid()
    d = _device(api, c, T, P.NANG, P.NFRE, g.ngy)
    n, nr = g.nsea, P.NFRE_RED
    _assert_bits(d["f3"][:n, :, :nr], fx[f"f3_{prec}"], "F3")
    assert np.all(d["f3"][:n, :, nr:] == SENTINEL) and np.all(d["f3"][n:] == SENTINEL), "frequencies above NFRE_RED or the land row were written"
    if c["irefra"]:
        nang = P.NANG
        _assert_bits(d["dot"][:, :nang], fx[f"thdd_{prec}"], "THDD")
        _assert_bits(d["dot"][:, nang:2 * nang], fx[f"thdc_{prec}"], "THDC")
        assert np.all(d["dot"][:, 3 * nang + 1:] == 0)
        if c["irefra"] >= 2:      # SDOT as the stencil rebuilds it from the row: the expression of propdot.F90:190-191 on the device's S0 and OMDD
            sd = P.sdot(d["dot"][:, 2 * nang:3 * nang], d["dot"][:, 3 * nang], c["cg"], c["om"], c["wn"], nr)
            _assert_bits(sd.astype(T), fx[f"sdot_{prec}"], "SDOT")
    if c["icase"] == 1:
        _assert_bits(d["cfl"], fx[f"cfl_{prec}"], "the arguments of CHECKCFL")
        assert np.array_equal(d["fail"], (fx[f"cfl_{prec}"].max(axis=(1, 2)) > 1).astype(np.int32))
    else:      # the Cartesian sections call no check
        assert np.all(d["cfl"] == SENTINEL) and not d["fail"].any()


# ---- 2. the other shapes against the restatement: the 16-byte edge pieces at 29, the widest direction wrap, the LDS sizing at 48 --------------------------------
_SHAPE_GRID = {}


def _shape_grid():
    if "g" not in _SHAPE_GRID:
        from ecwam_amd import grid

        _SHAPE_GRID["g"] = grid.build_grid(5, "continents", seed=11, land_fraction=0.3)
    return _SHAPE_GRID["g"]


@pytest.mark.parametrize("with_obs", [False, True], ids=["plain", "obstructed"])
@pytest.mark.parametrize("irefra", [0, 3])
@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("shape", [(24, 36, 29), (36, 36, 36), (48, 36, 36)], ids=lambda s: f"{s[0]}x{s[2]}")
def test_other_shapes_against_the_restatement(api, shape, prec, irefra, with_obs):
    T = PREC[prec]
    nang, nfre, nr = shape
    g = _shape_grid()
    assert g.nsea > 4 * 8      # more than one block
    c = P.make_inputs(T, g, P.tables_of(T, nang, nfre, nr, irefra), 1, 1, irefra, with_obs, 300, seed=3)
    r = P.restate(c, T)
    d = _device(api, c, T, nang, nfre, g.ngy)
    n = g.nsea
    _assert_bits(d["f3"][:n, :, :nr], r["f3"], "F3")
    assert np.all(d["f3"][:n, :, nr:] == SENTINEL) and np.all(d["f3"][n:] == SENTINEL)
    _assert_bits(d["cfl"], r["cfl"], "the arguments of CHECKCFL")
    if irefra:
        _assert_bits(d["dot"], r["dot"], "the dot terms")


# ---- 3. row ranges and what is not written -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sph_irgg1_irefra3", "cart_irefra3", "sph_obs_irefra0"])
def test_row_ranges_and_sentinels(api, name):
    T = np.float32
    c = P.make_case(name, T)
    g = P.fixture_grid()
    n, nr = g.nsea, P.NFRE_RED
    whole = _device(api, c, T, P.NANG, P.NFRE, g.ngy, copy_rest=True)
    assert P.same_bits(whole["f3"][:n, :, nr:], c["f1"][:n, :, nr:]), "copy_rest carries the frequencies above NFRE_RED over"
    assert np.all(whole["f3"][n:] == SENTINEL)
    a, b = 9, 47
    parts = _device(api, c, T, P.NANG, P.NFRE, g.ngy, a, b, copy_rest=True, ctx=whole["ctx"])
    assert np.all(parts["f3"][:a] == SENTINEL) and np.all(parts["f3"][b:] == SENTINEL), "rows outside [kijs, kijl) were written"
    assert np.all(parts["cfl"][:a] == SENTINEL) and np.all(parts["cfl"][b:] == SENTINEL)
    for k0, k1 in ((0, a), (b, n)):
        parts = _device(api, c, T, P.NANG, P.NFRE, g.ngy, k0, k1, copy_rest=True, f3=parts["f3_dev"], ctx=whole["ctx"])
    _assert_bits(parts["f3"], whole["f3"], "three parts against one call")
    nocopy = _device(api, c, T, P.NANG, P.NFRE, g.ngy, copy_rest=False, ctx=whole["ctx"])
    assert np.all(nocopy["f3"][:, :, nr:] == SENTINEL)
    _assert_bits(nocopy["f3"][:n, :, :nr], whole["f3"][:n, :, :nr], "copy_rest changes the advected frequencies")


# ---- 4. the CFL check ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("name", ["cfl_irefra0", "cfl_irefra3"])
def test_cfl_flags_and_the_check_alone(api, name, prec):
    T = PREC[prec]
    fx = P.load_fixture(name)
    c = P.make_case(name, T)
    g = P.fixture_grid()
    want = (fx[f"cfl_{prec}"].max(axis=(1, 2)) > 1).astype(np.int32)
    assert 0 < want.sum() < g.nsea / 2
    full = _device(api, c, T, P.NANG, P.NFRE, g.ngy)
    assert np.array_equal(full["fail"], want)
    alone = _device(api, c, T, P.NANG, P.NFRE, g.ngy, check_only=True, ctx=full["ctx"])
    assert alone["f3"] is None and np.array_equal(alone["fail"], want)
    _assert_bits(alone["cfl"], fx[f"cfl_{prec}"], "the arguments of CHECKCFL, check alone")


def test_a_flag_that_was_set_stays_set(api):
    T = np.float32
    g = P.fixture_grid()
    set_before = (np.arange(g.nsea) % 3 == 0)
    for name in ("cart_irefra0", "cart_irefra3", "sph_irgg1_irefra0"):      # no check on a Cartesian grid; none failing on the spherical one
        d = _device(api, P.make_case(name, T), T, P.NANG, P.NFRE, g.ngy, cflfail0=set_before)
        assert np.array_equal(d["fail"], set_before.astype(np.int32)), name


# ---- 5. the driver -------------------------------------------------------------------------------------------------------------------------------------------
def _model(irefra, prec="sp", idelpro=300, **kw):
    from ecwam_amd import grid
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    g = grid.build_grid(8, "continents")
    cfg = Config(nang=12, nfre=36, nfre_red=29, idelpro=idelpro, idelt=idelpro, irefra=irefra)
    m = Wamintgr(cfg, g, prec, **kw)
    m.init_synthetic(seed=4)
    return m


@pytest.mark.parametrize("irefra", [0, 3])
def test_wamintgr_ipropags_0_is_the_sequence_of_calls(api, irefra):
    m, b = _model(irefra, ipropags=0), _model(irefra, ipropags=0)
    assert not m.fused_available()
    assert m.build_weights() == 0
    for _ in range(2):
        m.step()
    c = b.cfg
    for _ in range(2):
        env = {}
        if irefra:
            b.ctx.propags_dot(b.gd, b.depth_ext, b.u_ext, b.v_ext, b.dot)
            env = dict(omosnh2kd_ext=b.omosnh2kd_ext, wavnum_ext=b.wavnum_ext, u_ext=b.u_ext, v_ext=b.v_ext, dot=b.dot)
        b.halo(b.fl1)
        b.ctx.propags(b.fl1, b.fl3, b.gd, b.cgroup_ext, float(c.idelpro), 0, b.n, copy_rest=True, **env)
        b.fl1, b.fl3 = b.fl3, b.fl1
        b.newwind()
        b.implsch()
    torch.cuda.synchronize()
    assert torch.equal(m.fl1[: m.n], b.fl1[: b.n])
    assert torch.equal(m.ff, b.ff)
    # the scheme is not the corner-transport one
    other = _model(irefra)
    other.step()
    other.step()
    assert not torch.equal(other.fl1[: other.n], m.fl1[: m.n])


def test_wamintgr_refuses_a_time_step_too_long_for_the_grid(api):
    m = _model(0, idelpro=40000, ipropags=0)
    assert m.build_weights() > 0
    m.weights_ready = False
    with pytest.raises(api.EcwamHipError, match="CFL"):
        m.step()


def test_default_scheme_keeps_its_bits(api):
    a, b = _model(0), _model(0, ipropags=2)
    assert a.ipropags == 2
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.fl1, b.fl1) and torch.equal(a.ff, b.ff)


# ---- 6. the refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(api):
    T = np.float32
    g = P.fixture_grid()
    c = P.make_case("sph_irgg1_irefra3", T)
    ctx = _context(api, T, P.NANG, P.NFRE, P.NFRE_RED, 3)
    gd, td = _upload(ctx, c, g.ngy)
    n = gd["n"]
    dot = torch.zeros((n, P.dot_width(P.NANG)), dtype=ctx.dtype, device=ctx.device)
    f3 = torch.zeros_like(td["f1"])
    env = dict(omosnh2kd_ext=td["om"], wavnum_ext=td["wn"], u_ext=td["u"], v_ext=td["v"])
    ok = dict(icase=1, irgg=1, delphi=float(c["delphi"]))
    with pytest.raises(api.EcwamHipError, match="dot"):      # a missing dot at IREFRA /= 0
        ctx.propags(td["f1"], f3, gd, td["cg"], 900.0, 0, n, **env, **ok)
    with pytest.raises(api.EcwamHipError, match="whole number"):      # DELPRO = REAL(IDELPRO)
        ctx.propags(td["f1"], f3, gd, td["cg"], 900.5, 0, n, dot=dot, **env, **ok)
    with pytest.raises(api.EcwamHipError, match="bad range"):
        ctx.propags(td["f1"], f3, gd, td["cg"], 900.0, 5, n + 1, dot=dot, **env, **ok)
    # misaligned buffers: a view one real into an allocation, through the C interface (the binding passes whole tensors)
    lib, h = ctx.lib, ctx._h
    big = torch.zeros(td["f1"].numel() + 4, dtype=ctx.dtype, device=ctx.device)

    def call(f1p, f3p, dotp):
        return lib.ecwam_hip_propags(h, f1p, f3p, n, gd["nland"], g.ngy, 900.0, float(c["delphi"]), 2, gd["kxlt"].data_ptr(), gd["cosph"].data_ptr(),
                                     gd["sinph"].data_ptr(), gd["dellam1_ext"].data_ptr(), gd["cosphm1_ext"].data_ptr(), gd["klon"].data_ptr(),
                                     gd["klat"].data_ptr(), gd["wlat"].data_ptr(), td["cg"].data_ptr(), td["om"].data_ptr(), td["wn"].data_ptr(),
                                     td["u"].data_ptr(), td["v"].data_ptr(), dotp, 0, n, 0, None, None, None)

    assert call(td["f1"].data_ptr(), big.data_ptr() + 4, dot.data_ptr()) == 1 and b"16-byte" in lib.ecwam_hip_last_error()
    assert call(big.data_ptr() + 4, f3.data_ptr(), dot.data_ptr()) == 1 and b"16-byte" in lib.ecwam_hip_last_error()
    assert call(td["f1"].data_ptr(), f3.data_ptr(), big.data_ptr() + 4) == 1 and b"16-byte" in lib.ecwam_hip_last_error()
    assert call(td["f1"].data_ptr(), f3.data_ptr(), dot.data_ptr()) == 0
    assert lib.ecwam_hip_propags_dot(h, n, gd["nland"], 3, gd["kxlt"].data_ptr(), gd["zdello"].data_ptr(), float(gd["xdella"]), gd["cosph"].data_ptr(),
                                     gd["klon"].data_ptr(), gd["klat"].data_ptr(), gd["wlat"].data_ptr(), gd["cosphm1_ext"].data_ptr(), td["depth"].data_ptr(),
                                     td["u"].data_ptr(), td["v"].data_ptr(), dot.data_ptr(), None) == 1 and b"ICASE" in lib.ecwam_hip_last_error()
    assert lib.ecwam_hip_propags_dot(h, n, gd["nland"], 1, gd["kxlt"].data_ptr(), gd["zdello"].data_ptr(), float(gd["xdella"]), gd["cosph"].data_ptr(),
                                     gd["klon"].data_ptr(), gd["klat"].data_ptr(), gd["wlat"].data_ptr(), gd["cosphm1_ext"].data_ptr(), td["depth"].data_ptr(),
                                     td["u"].data_ptr(), td["v"].data_ptr(), big.data_ptr() + 4, None) == 1 and b"16-byte" in lib.ecwam_hip_last_error()
    torch.cuda.synchronize()
