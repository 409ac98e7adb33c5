"""The dual rotated-quadrant propagation scheme on the device (IPROPAGS = 1: ecwam_hipx_set_rotated, ecwam_hipx_propags1; include/ecwam_hipx_propags1.h).

The gate is THE SAME BITS, in single and in double precision: PROPAGS1 and CHECKCFL hold only + - * / and ABS, every one correctly rounded, and the kernels
keep the reference's order without contraction.  No quantity needed an exception.
  1  against the fixtures tests/golden/propags1_*.npz: what the reference's own unmodified Fortran returned (tools/make_golden_propags1.py), the device fed
     the recorded rotated tables
  2  the shapes the fixtures do not have, against the restatement tests/propags1_ref.py (which tests/test_propags1_host.py holds to the fixtures bit for bit)
  3  row ranges cutting a tile   4  the check alone   5  a flag once set stays set   6  the driver Wamintgr(ipropags=1)   7  the refusals
"""
import numpy as np
import pytest

import propags1_ref as P1
import propags_ref as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PREC = P1.PREC
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


def _device(api, c, rot, T, nang, nfre, ngy, kijs=0, kijl=None, copy_rest=False, f3=None, check_only=False, cflfail0=None, ctx=None):
    """-> dict(f3 [nrow][K][NFRE], cfl [n][K][11], fail [n]) of ecwam_hipx_propags1 on the inputs c and the rotated tables rot"""
    ctx = ctx or _context(api, T, nang, nfre, c["nr"], c["irefra"])
    gd, td = _upload(ctx, c, ngy)
    n, dev = gd["n"], ctx.device
    kijl = n if kijl is None else kijl
    ctx.set_obstructions(None if c["obs"] is None else torch.from_numpy(c["obs"]).to(dev))
    ctx.set_rotated(None if rot is None else api.rotated_to_device(rot, ctx.dtype, dev))
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
    ctx.propags1(td["f1"], None if check_only else f3, gd, td["cg"], c["delpro"], kijs, kijl, copy_rest=copy_rest, cfl=cfl, cflfail=fail, icase=c["icase"],
                 irgg=c["irgg"], delphi=float(c["delphi"]), **env)
    torch.cuda.synchronize()
    assert torch.equal(td["f1"], f1_before), "F1 was written"
    return dict(ctx=ctx, f3=None if f3 is None else f3.cpu().numpy(), cfl=cfl.cpu().numpy(), fail=fail.cpu().numpy(), f3_dev=f3)


def _assert_bits(got, want, what):
    assert P.same_bits(got, want), (what, "differing elements:", int((np.asarray(got) != np.asarray(want)).sum()), "largest difference:",
                                    float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()))


def _case(name, prec):
    T = PREC[prec]
    fx = P1.load_fixture(name)
    return T, fx, P1.make_case(name, T), P1.recorded_rot(fx, prec), P1.fixture_grid(P1.CASES[name][0])


# ---- 1. the device against what the reference's own Fortran returned -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("name", list(P1.CASES))
def test_device_reproduces_the_reference_bit_for_bit(api, name, prec):
    T, fx, c, rot, g = _case(name, prec)
    d = _device(api, c, rot, T, P1.NANG, P1.NFRE, g.ngy)
    n, nr = g.nsea, c["nr"]
    _assert_bits(d["f3"][:n, :, :nr], fx[f"f3_{prec}"], "F3")
    assert np.all(d["f3"][:n, :, nr:] == SENTINEL) and np.all(d["f3"][n:] == SENTINEL), "frequencies above NFRE_RED or the land row were written"
    if c["icase"] == 1:
        _assert_bits(d["cfl"], fx[f"cfl_{prec}"], "the arguments of CHECKCFL")
        assert np.array_equal(d["fail"], (fx[f"cfl_{prec}"].max(axis=(1, 2)) > 1).astype(np.int32))
    else:      # the Cartesian sections call no check
        assert np.all(d["cfl"] == SENTINEL) and not d["fail"].any()


# ---- 2. the other shapes against the restatement: the 16-byte edge pieces at 29, the per-point upwind choice at 36 directions, the LDS sizing at 48 -----------
_SHAPE = {}


def _shape_grid():
    if "g" not in _SHAPE:
        from ecwam_amd import grid

        _SHAPE["g"] = grid.build_grid(5, "continents", seed=11, land_fraction=0.3)
    return _SHAPE["g"]


def _shape_rot(T, nang):
    from ecwam_amd import grid

    key = (T, nang)
    if key not in _SHAPE:
        t = P.tables_of(T, nang)
        _SHAPE[key] = grid.rotated_tables(P1.rounded_grid(_shape_grid()), T, np.asarray(t.SINTH, T), np.asarray(t.COSTH, T))
    return _SHAPE[key]


@pytest.mark.parametrize("with_obs", [False, True], ids=["plain", "obstructed"])
@pytest.mark.parametrize("irefra", [0, 1])
@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("shape", [(24, 36, 29), (36, 36, 36), (48, 36, 36)], ids=lambda s: f"{s[0]}x{s[2]}")
def test_other_shapes_against_the_restatement(api, shape, prec, irefra, with_obs):
    T = PREC[prec]
    nang, nfre, nr = shape
    g = _shape_grid()
    assert g.nsea > 4 * 4      # more than one block (the 61 and 117 points of the fixtures cut the last tile)
    rot = _shape_rot(T, nang)
    c = P.make_inputs(T, g, P.tables_of(T, nang, nfre, nr, irefra), 1, 1, irefra, with_obs, 300, seed=3, obscor=with_obs)
    choice = {}
    r = P1.restate(c, T, rot, choice=choice)
    if nang == 36:      # the upwind side of a rotated axis differs between two points in some direction
        assert any((choice[k] != choice[k][0]).any() for k in ("IJRLA", "IJRPH"))
    d = _device(api, c, rot, T, nang, nfre, g.ngy)
    n = g.nsea
    _assert_bits(d["f3"][:n, :, :nr], r["f3"], "F3")
    assert np.all(d["f3"][:n, :, nr:] == SENTINEL) and np.all(d["f3"][n:] == SENTINEL)
    _assert_bits(d["cfl"], r["cfl"], "the arguments of CHECKCFL")


# ---- 3. row ranges and what is not written -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rot_obs_irefra1", "sec4_irefra3"])
def test_row_ranges_and_sentinels(api, name):
    T, fx, c, rot, g = _case(name, "sp")
    n, nr = g.nsea, c["nr"]
    args = (T, P1.NANG, P1.NFRE, g.ngy)
    whole = _device(api, c, rot, *args, copy_rest=True)
    assert P.same_bits(whole["f3"][:n, :, nr:], c["f1"][:n, :, nr:]), "copy_rest carries the frequencies above NFRE_RED over"
    assert np.all(whole["f3"][n:] == SENTINEL)
    a, b = 9, 47      # neither is a multiple of the tile
    parts = _device(api, c, rot, *args, a, b, copy_rest=True, ctx=whole["ctx"])
    assert np.all(parts["f3"][:a] == SENTINEL) and np.all(parts["f3"][b:] == SENTINEL), "rows outside [kijs, kijl) were written"
    assert np.all(parts["cfl"][:a] == SENTINEL) and np.all(parts["cfl"][b:] == SENTINEL)
    for k0, k1 in ((0, a), (b, n)):
        parts = _device(api, c, rot, *args, k0, k1, copy_rest=True, f3=parts["f3_dev"], ctx=whole["ctx"])
    _assert_bits(parts["f3"], whole["f3"], "three parts against one call")
    nocopy = _device(api, c, rot, *args, copy_rest=False, ctx=whole["ctx"])
    assert np.all(nocopy["f3"][:, :, nr:] == SENTINEL)
    _assert_bits(nocopy["f3"][:n, :, :nr], whole["f3"][:n, :, :nr], "copy_rest changes the advected frequencies")


# ---- 4. the CFL check ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_cfl_flags_and_the_check_alone(api, prec):
    T, fx, c, rot, g = _case("rot_cfl_irefra0", prec)
    want = (fx[f"cfl_{prec}"].max(axis=(1, 2)) > 1).astype(np.int32)
    assert 0 < want.sum() < g.nsea / 2
    full = _device(api, c, rot, T, P1.NANG, P1.NFRE, g.ngy)
    assert np.array_equal(full["fail"], want)
    alone = _device(api, c, rot, T, P1.NANG, P1.NFRE, g.ngy, check_only=True, ctx=full["ctx"])
    assert alone["f3"] is None and np.array_equal(alone["fail"], want)
    _assert_bits(alone["cfl"], fx[f"cfl_{prec}"], "the arguments of CHECKCFL, check alone")


# ---- 5. a flag once set stays set ----------------------------------------------------------------------------------------------------------------------------
def test_a_flag_that_was_set_stays_set(api):
    g = P1.fixture_grid("o3")
    set_before = (np.arange(g.nsea) % 3 == 0)
    for name in ("cart_irefra1", "rot_irefra0", "sec4_irefra3"):      # no check on a Cartesian grid; none failing on the spherical one
        T, fx, c, rot, _ = _case(name, "sp")
        d = _device(api, c, rot, T, P1.NANG, P1.NFRE, g.ngy, cflfail0=set_before)
        assert np.array_equal(d["fail"], set_before.astype(np.int32)), name


# ---- 6. the driver -------------------------------------------------------------------------------------------------------------------------------------------
def _model(irefra, prec="sp", idelpro=300, ipropags=2):
    from ecwam_amd import grid
    from ecwam_amd.tables import Config, Tables
    from ecwam_amd.wamintgr import Wamintgr

    if "model_grid" not in _SHAPE:
        _SHAPE["model_grid"] = grid.build_grid(8, "continents")
    g = _SHAPE["model_grid"]
    cfg = Config(nang=12, nfre=36, nfre_red=29, idelpro=idelpro, idelt=idelpro, irefra=irefra)
    kw = {}
    if ipropags == 1:
        T = PREC[prec]
        t = Tables(cfg, T)
        kw["rotated"] = grid.rotated_tables(g, T, t.SINTH, t.COSTH)
    m = Wamintgr(cfg, g, prec, ipropags=ipropags, **kw)
    m.init_synthetic(seed=4)
    return m


@pytest.mark.parametrize("irefra", [0, 1])
def test_wamintgr_ipropags_1_is_the_sequence_of_calls(api, irefra):
    m, b = _model(irefra, ipropags=1), _model(irefra, ipropags=1)
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
        b.ctx.propags1(b.fl1, b.fl3, b.gd, b.cgroup_ext, float(c.idelpro), 0, b.n, copy_rest=True, **env)
        b.fl1, b.fl3 = b.fl3, b.fl1
        b.newwind()
        b.implsch()
    torch.cuda.synchronize()
    assert torch.equal(m.fl1[: m.n], b.fl1[: b.n])
    assert torch.equal(m.ff, b.ff)
    assert torch.isfinite(m.fl1).all()
    # the scheme is neither the plain first-order one nor the corner-transport one
    for other_scheme in (0, 2):
        other = _model(irefra, ipropags=other_scheme)
        other.step()
        other.step()
        assert not torch.equal(other.fl1[: other.n], m.fl1[: m.n]), other_scheme


def test_wamintgr_refuses_a_time_step_too_long_for_the_grid(api):
    m = _model(0, idelpro=40000, ipropags=1)
    assert m.build_weights() > 0
    m.weights_ready = False
    with pytest.raises(api.EcwamHipError, match="CFL"):
        m.step()


def test_default_scheme_keeps_its_bits(api):
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    a = _model(0)
    g = _SHAPE["model_grid"]
    b = Wamintgr(Config(nang=12, nfre=36, nfre_red=29, idelpro=300, idelt=300, irefra=0), g, "sp")      # no keyword of the scheme at all
    b.init_synthetic(seed=4)
    assert a.ipropags == 2 and b.ipropags == 2 and not b.ctx.has_rotated
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.fl1, b.fl1) and torch.equal(a.ff, b.ff)


# ---- 7. the refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(api):
    T, fx, c, rot, g = _case("rot_irefra1", "sp")
    ctx = _context(api, T, P1.NANG, P1.NFRE, c["nr"], 1)
    gd, td = _upload(ctx, c, g.ngy)
    n = gd["n"]
    dot = torch.zeros((n, P.dot_width(P1.NANG)), dtype=ctx.dtype, device=ctx.device)
    f3 = torch.zeros_like(td["f1"])
    env = dict(omosnh2kd_ext=td["om"])
    ok = dict(icase=1, irgg=1, delphi=float(c["delphi"]))
    with pytest.raises(api.EcwamHipError, match="rotated tables"):      # no tables set on a spherical grid with IREFRA 1
        ctx.propags1(td["f1"], f3, gd, td["cg"], 900.0, 0, n, dot=dot, **env, **ok)
    rd = api.rotated_to_device(rot, ctx.dtype, ctx.device)
    with pytest.raises(api.EcwamHipError, match="bad size"):      # nrow <= n
        ctx.set_rotated(dict(rd, cdr=rd["cdr"][:n].contiguous(), sdr=rd["sdr"][:n].contiguous()))
    lib, h = ctx.lib, ctx._h
    assert lib.ecwam_hipx_set_rotated(h, n, n + 1, rd["krlat"].data_ptr(), None, None, None, None, None, None, 1.4) == 1
    assert b"NULL" in lib.ecwam_hip_last_error()
    assert not ctx.has_rotated
    ctx.set_rotated(rd)
    with pytest.raises(api.EcwamHipError, match="dot"):      # a missing dot at IREFRA /= 0
        ctx.propags1(td["f1"], f3, gd, td["cg"], 900.0, 0, n, **env, **ok)
    with pytest.raises(api.EcwamHipError, match="whole number"):      # DELPRO = REAL(IDELPRO)
        ctx.propags1(td["f1"], f3, gd, td["cg"], 900.5, 0, n, dot=dot, **env, **ok)
    with pytest.raises(api.EcwamHipError, match="bad range"):
        ctx.propags1(td["f1"], f3, gd, td["cg"], 900.0, 5, n + 1, dot=dot, **env, **ok)
    with pytest.raises(api.EcwamHipError, match="alias"):
        ctx.propags1(td["f1"], td["f1"], gd, td["cg"], 900.0, 0, n, dot=dot, **env, **ok)
    big = torch.zeros(td["f1"].numel() + 4, dtype=ctx.dtype, device=ctx.device)

    def call(f1p, f3p, flags=2):
        return lib.ecwam_hipx_propags1(h, f1p, f3p, n, gd["nland"], g.ngy, 900.0, float(c["delphi"]), flags, gd["kxlt"].data_ptr(), gd["cosph"].data_ptr(),
                                       gd["sinph"].data_ptr(), gd["dellam1_ext"].data_ptr(), gd["cosphm1_ext"].data_ptr(), gd["klon"].data_ptr(),
                                       gd["klat"].data_ptr(), gd["wlat"].data_ptr(), td["cg"].data_ptr(), td["om"].data_ptr(), td["wn"].data_ptr(),
                                       td["u"].data_ptr(), td["v"].data_ptr(), dot.data_ptr(), 0, n, 0, None, None, None)

    assert call(td["f1"].data_ptr(), big.data_ptr() + 4) == 1 and b"16-byte" in lib.ecwam_hip_last_error()
    assert call(big.data_ptr() + 4, f3.data_ptr()) == 1 and b"16-byte" in lib.ecwam_hip_last_error()
    assert call(td["f1"].data_ptr(), f3.data_ptr(), flags=4) == 1 and b"unknown flag" in lib.ecwam_hip_last_error()
    assert call(td["f1"].data_ptr(), f3.data_ptr()) == 0
    # tables of fewer points than the call reads
    ctx.set_rotated({k: (v[: n - 1].contiguous() if k in ("krlat", "krlon", "wrlat", "wrlon", "prqrt") else v) for k, v in rd.items()})
    with pytest.raises(api.EcwamHipError, match="fewer points"):
        ctx.propags1(td["f1"], f3, gd, td["cg"], 900.0, 0, n, dot=dot, **env, **ok)
    torch.cuda.synchronize()
