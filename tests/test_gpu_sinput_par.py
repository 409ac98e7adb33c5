"""SINPUT's no-growth run found in one lane-parallel pass (csrc/implsch_v4.h::v4_sinput, V4_SINPUT_PAR, single precision; run with -m gpu on
an MI355X).  The product finds the length m0 of the leading run of rows without growth from the minimum of 1 / COSLP over the point's
directions and one test per (point, row); the library built with -DV4_SINPUT_PAR=0 (build variant "nopar") tests the rows one after the
other, one ballot and branch per row; "nolead" sends every row through the row loop.  All three must give the SAME BITS -- FL1, XLLWS, FF,
INTF, MIJ --

* through implsch(), through the one-kernel step (ecwam_hip_propags2_implsch on rows [0, n)) and through WDFLUXES,
* at 36 / 24 / 12 directions on 73 / 121 / 241 points (24 full wavefronts of three / five / ten points and a short one), two consecutive
  calls each so that the second runs on the UFRIC / Z0M the first one left,
* with the wavefronts of tests/test_gpu_sinput_lead.py -- the run empty (all points at 35 m/s), all rows (1 m/s), in between (8 m/s), set by one
  windy point (20 m/s) between calm ones -- and two more:
  - the points of a wavefront at 5, 8 and 13 m/s: their runs end at three different rows, and the minimum over the points is what counts;
  - one point of an 8 m/s wavefront with a friction velocity of 1e-12 m/s in FF: its stress vanishes, the chain gives it the direction
    (0, 0), COSLP = 0 <= 0.01 in every direction, the minimum of 1 / COSLP over "the directions that pass" is +infinity, and the other
    points of the wavefront set the run.  This case occurs THROUGH WDFLUXES ONLY, in its first call (both gust states of its one SINFLX
    call): WDFLUXES hands FF's friction velocity to SINPUT as it came.  implsch() and the step compute the friction velocity from the wind
    (TAUT_Z0 with IUSFG = 0) before the first SINFLX call and never look at that column, so there the point is an 8 m/s point like its
    neighbours, and so it is for WDFLUXES after one implsch().  A friction velocity that small cannot be brought about from a wind speed.
    test_the_point_without_stress_occurs_through_wdfluxes asserts the case on the FF that call reads and on what it wrote: no XLLWS bit at
    that point, some at every other point of its wavefront.
* in double precision, which keeps its code: implsch() at 36 directions on 31 points against "nopar".

That the other cases occur is asserted on the host, in float64, as tests/test_gpu_sinput_lead.py does it (bounds `lo`, `hi` of the row where a
point's growth starts), from every FF state the calls read or leave.  The helpers are restated here: that file's edits are not this test's.

What these comparisons can and cannot see: a run found too LONG changes bits (rows with growth would be skipped); a run found too short does
not -- the row loop then does those rows, with the same bits by construction.  That the one-pass test finds the whole run is what the executed
instruction counts of the benchmark show, not this file.

The variants run in child processes (ECWAM_HIP_LIB): this file run as a program writes its results to the file named on its command line."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":      # the child process of the variant fixtures: the suite's module path and seeds
    import conftest  # noqa: F401

import harness as H
from ecwam_amd import synthetic as syn
from ecwam_amd.tables import Config

pytestmark = pytest.mark.gpu

NAMES = ("fl1", "xllws", "ff", "intf", "mij")
PP = {36: 3, 24: 5, 12: 10}      # sea points per wavefront in single precision
NFRE_RED = {36: 36, 24: 29, 12: 25}      # of the reference's registered configuration with that many directions
WAVES = 24
# directions -> (points, grid size with at least that many sea points)
SHAPES = {nang: (WAVES * PP[nang] + 1, 16) for nang in (36, 24, 12)}
NDP = 31
HOT, CALM, MID, WINDY = 35.0, 1.0, 8.0, 20.0
THREE = (5.0, 8.0, 13.0)
DEAD_UFRIC = 1e-12
SEED = 78
NKIND = 6


def _cfg(nang):
    return Config(nang=nang, nfre=36, nfre_red=NFRE_RED[nang], idelt=450, idelpro=450)


@contextlib.contextmanager
def deep_water():
    """Every synthetic point in deep water: in two metres of water a wave of any frequency is slower than a light wind, and the wind speeds
    above would not decide the cases."""
    drawn = syn.point_params
    syn.point_params = lambda n, seed=12345, **kw: drawn(n, seed, **dict(kw, shallow_fraction=0.0))
    try:
        yield
    finally:
        syn.point_params = drawn


def _snap(out, key, fl1, xllws, ff, intf, mij, n):
    for name, t in zip(NAMES, (fl1, xllws, ff, intf, mij)):
        out[f"{key}/{name}"] = t[:n].cpu().numpy().copy()


def gustiness(ff, tables):
    """SIG_N of wsigstar.F90 (the form without LLGCBZ0 / LLNORMAGAM) from WSTAR, UFRIC and Z0M of FF, in float64."""
    t = tables
    ufric, z0m, wstar = (ff[:, i].astype(np.float64) for i in (7, 10, 4))
    c1, c2, p1, p2 = 1.03e-3, 0.04e-3, 1.48, -0.21
    u10 = np.maximum(ufric / float(t.XKAPPA) * (np.log(10.0) - np.log(z0m)), float(t.WSPMIN))
    c2u10p1, u10p2 = c2 * u10 ** p1, u10 ** p2
    c_d = (c1 + c2u10p1) * u10p2
    dc_ddu = (p2 * c1 + (p1 + p2) * c2u10p1) * u10p2 / u10
    sig_conv = 1.0 + 0.5 * u10 / c_d * dc_ddu
    return np.minimum(0.9, sig_conv / u10 * np.cbrt(0.5 * float(t.XKAPPA) * wstar ** 3))


def first_growing_row(ff, wavnum, cinv, tables, sig_n, coslp):
    """Per point the first row M (0-based; NFRE: none) in which ZLOG < 0 at the given gustiness and COSLP, in float64."""
    ufric, z0m = ff[:, 7].astype(np.float64)[:, None], ff[:, 10].astype(np.float64)[:, None]
    k, ci = wavnum.astype(np.float64), cinv.astype(np.float64)
    zlog = np.log(k * z0m) + float(tables.XKAPPA) / (ufric * (1.0 + np.reshape(sig_n, (-1, 1))) * ci + float(tables.ZALP)) / coslp
    grows = zlog < 0.0
    return np.where(grows.any(1), grows.argmax(1), grows.shape[1])


def wave_kinds(n, pp):
    """The case of every wavefront: 0 .. 3 those of test_gpu_sinput_lead, 4 three speeds, 5 a point without stress between points at the
    middle speed; the last (short) wavefront calm."""
    kinds = np.arange((n + pp - 1) // pp) % NKIND
    kinds[-1] = 1
    return kinds


def wind_speeds(n, pp):
    kinds = wave_kinds(n, pp)
    ws = np.empty(n)
    for i in range(n):
        k, q = kinds[i // pp], i % pp
        ws[i] = (HOT, CALM, MID, WINDY if q == pp // 2 else CALM, THREE[q % 3], MID)[k]
    return ws


def dead_points(n, pp):
    kinds = wave_kinds(n, pp)
    return np.array([i for i in range(n) if kinds[i // pp] == 5 and i % pp == pp // 2])


def calm_wstar(wstar, n, pp):
    calm = wave_kinds(n, pp)[np.arange(n) // pp] == 1
    return np.where(calm, 0.0, wstar[:n])


def forcing(params, rows, tables, dt, n, pp):
    """FF of the given rows with the first n points in their cases (columns: 7 UFRIC)."""
    p = dict(params)
    p["WSWAVE"] = p["WSWAVE"].copy()
    p["WSWAVE"][:n] = wind_speeds(n, pp)
    p["WSTAR"] = p["WSTAR"].copy()
    p["WSTAR"][:n] = calm_wstar(p["WSTAR"], n, pp)
    ff = syn.forcing(p, rows, tables, dt)
    ff[dead_points(n, pp), 7] = DEAD_UFRIC
    return p, ff


_CASES = {}


def point_case(nang, prec="sp"):
    """make_point_case's inputs with the wind speeds of the cases: built once, shared, never modified."""
    if (nang, prec) not in _CASES:
        n = SHAPES[nang][0] if prec == "sp" else NDP
        with deep_water():
            case = H.make_point_case(n, _cfg(nang), prec, seed=SEED)
        case["params"], case["FF"] = forcing(case["params"], slice(0, n), case["tables"], H.np_dtype(prec), n, PP[nang])
        _CASES[(nang, prec)] = case
    return _CASES[(nang, prec)]


def run_all():
    """Every comparison's device results with the library this process loads: {"<directions>/<path>/<call>/<array>": numpy array}."""
    import torch

    from ecwam_amd import api, grid as G
    from ecwam_amd.wamintgr import Wamintgr

    out = {}
    for nang, prec in [(a, "sp") for a in SHAPES] + [(36, "dp")]:
        case = point_case(nang, prec)
        n = case["n"]
        tag = f"{nang}" if prec == "sp" else f"{nang}dp"
        ctx = api.HipContext(case["tables"])
        dev = ctx.device
        wv, ff0, intf0 = H.pack_device_inputs(case)

        def fresh():
            fl1 = torch.from_numpy(case["FL1"].copy()).to(dev)
            return (fl1, torch.zeros_like(fl1), torch.from_numpy(ff0.copy()).to(dev), torch.from_numpy(intf0.copy()).to(dev),
                    torch.zeros(n, dtype=torch.int32, device=dev))

        twv = torch.from_numpy(wv).to(dev)
        fl1, xllws, ff, intf, mij = fresh()
        for call in (1, 2):
            ctx.implsch(0, n, fl1, twv, ff, intf, mij, xllws)
            _snap(out, f"{tag}/implsch/{call}", fl1, xllws, ff, intf, mij, n)
        if prec == "dp":
            torch.cuda.synchronize()
            ctx.close()
            continue
        assert ctx.wdfluxes_supported()
        fl1, xllws, ff, intf, mij = fresh()
        ctx.wdfluxes(0, n, fl1, twv, ff, intf, mij, xllws)
        _snap(out, f"{tag}/wdfluxes/1", fl1, xllws, ff, intf, mij, n)
        ctx.implsch(0, n, fl1, twv, ff, intf, mij, xllws)
        ctx.wdfluxes(0, n, fl1, twv, ff, intf, mij, xllws)
        _snap(out, f"{tag}/wdfluxes/2", fl1, xllws, ff, intf, mij, n)
        torch.cuda.synchronize()
        ctx.close()
        # the one-kernel step on rows [0, n) of a grid, twice
        g = G.build_grid(SHAPES[nang][1], mask="continents")
        assert g.nsea >= n
        m = Wamintgr(case["cfg"], g, "sp")
        with deep_water():
            m.init_synthetic(seed=SEED)
        assert m.fused_available() and m.build_weights() == 0
        _, ffg = forcing(m.params, slice(0, g.nsea), m.t, np.float32, n, PP[nang])
        m.ff[:, :14] = torch.from_numpy(ffg).to(m.dev)
        out[f"{tag}/step-in/ff"] = m.ff[:n].cpu().numpy().copy()
        out[f"{tag}/step-in/wvprpt"] = m.wvprpt[:n].cpu().numpy().copy()
        m.fl3.copy_(m.fl1)      # (the rows from n on are not stepped: they keep the start spectra in both buffers)
        for call in (1, 2):
            m.ctx.propags2_implsch(m.fl1, m.fl3, m.gd, m.cgroup_ext, float(m.cfg.idelpro), 0, n, m.wvprpt, m.ff, m.intf, m.mij, m.xllws, 1,
                                   m.cfg.nfre_red)
            m.fl1, m.fl3 = m.fl3, m.fl1
            _snap(out, f"{tag}/step/{call}", m.fl1, m.xllws, m.ff, m.intf, m.mij, n)
        torch.cuda.synchronize()
        m.ctx.close()
    return out


@pytest.fixture(scope="module")
def product():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert not os.environ.get("ECWAM_HIP_LIB"), "this test compares the product library with the variants: ECWAM_HIP_LIB must not be set"
    return run_all()


def _variant(name, tmp_path_factory):
    from ecwam_amd import build

    lib = build.lib_path(name)
    if not os.path.exists(lib):
        build.build(variant=name)
    path = str(tmp_path_factory.mktemp(name) / "variant.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, ECWAM_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def nopar(product, tmp_path_factory):
    return _variant("nopar", tmp_path_factory)


@pytest.fixture(scope="module")
def nolead(product, tmp_path_factory):
    return _variant("nolead", tmp_path_factory)


def stressless(ufric):
    """No direction passes COSLP > 0.01: the chain's direction vector TAU / SQRT(MAX(|TAU|**2, 1e-36)), |TAU| = UFRIC**2, is shorter than 0.01."""
    u2 = ufric.astype(np.float64) ** 2
    return u2 / np.sqrt(np.maximum(u2 * u2, 1e-36)) < 0.01


def assert_cases_occur(ff, wavnum, cinv, tables, nang, what, first_guess):
    """first_guess: an FF as the test set it up, the marked points of the wavefronts of kind 5 with their tiny friction velocity -- which only
    WDFLUXES hands to SINPUT (test_the_point_without_stress_occurs_through_wdfluxes); the bounds are not asked of those points."""
    n, pp, nfre = ff.shape[0], PP[nang], wavnum.shape[1]
    kinds = wave_kinds(n, pp)
    ws = wind_speeds(n, pp)
    dead = np.zeros(n, bool)
    dead[dead_points(n, pp)] = True
    assert not stressless(ff[~dead if first_guess else slice(None), 7]).any(), (what, "every point the bounds are asked of has a stress direction")
    live = ~dead if first_guess else np.ones(n, bool)
    ffl = ff.copy()
    ffl[~live, 7] = 0.3      # (the bounds below are not asked of a point without stress)
    lo = first_growing_row(ffl, wavnum, cinv, tables, np.minimum(0.9, 1.25 * gustiness(ffl, tables) + 0.02), 1.0)
    hi = first_growing_row(ffl, wavnum, cinv, tables, np.zeros(n), np.cos(np.pi / nang))
    assert (lo <= hi).all()
    seen = set()
    for w, kind in enumerate(kinds):
        a, b = w * pp, min(n, (w + 1) * pp)
        idx = np.arange(a, b)
        if kind == 0:
            assert (hi[a:b] == 0).all(), (what, w, "35 m/s: growth in row 0", hi[a:b])
        elif kind == 1:
            assert (lo[a:b] == nfre).all(), (what, w, "1 m/s: no growth in any row", lo[a:b])
        elif kind == 2:
            assert (lo[a:b] > 0).all() and (hi[a:b] < nfre).all(), (what, w, "8 m/s: a leading run that ends before the last row", lo[a:b], hi[a:b])
        elif kind == 3:
            windy = a + pp // 2
            calm = [i for i in idx if i != windy]
            assert (hi[windy] < lo[calm]).all(), (what, w, "the windy point sets the run", hi[windy], lo[calm])
        elif kind == 4:
            s = [idx[ws[idx] == v] for v in THREE]      # slow, middle, fast
            assert all(len(x) for x in s)
            assert hi[s[2]].max() < lo[s[1]].min() and hi[s[1]].max() < lo[s[0]].min() and hi[s[0]].max() < nfre and lo[s[2]].min() > 0, \
                (what, w, "three runs that end at three different rows", lo[a:b], hi[a:b])
        else:
            others = idx[live[idx]] if first_guess else idx
            assert (lo[others] > 0).all() and (hi[others] < nfre).all(), (what, w, "the points with stress set a run that ends before the last row")
        seen.add(int(kind))
    assert seen == set(range(NKIND)) and kinds[-1] == 1 and n % pp != 0, "every case, and a short calm last wavefront"


def _same(product, variant, prefix, ncalls=2):
    keys = [k for k in product if k.startswith(prefix) and k.rsplit("/", 1)[1] in NAMES]
    assert len(keys) == ncalls * len(NAMES) and all(k in variant for k in keys)
    for k in keys:
        x, y = product[k], variant[k]
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.isfinite(x).all(), k
        # (torch.equal's sense of "the same": element-wise ==, so that -0 equals +0)
        assert np.array_equal(x, y), f"{k}: {int((x != y).sum())} of {x.size} elements differ"


@pytest.mark.parametrize("nang", list(SHAPES))
def test_the_cases_occur(product, nang):
    """Every FF state an SINPUT call of the comparisons starts from or leaves puts the wavefronts into the cases they were built for."""
    case = point_case(nang)
    pr = case["props"]
    _, ff0, _ = H.pack_device_inputs(case)
    for what, ff in (("first guess", ff0), ("after one implsch()", product[f"{nang}/implsch/1/ff"]), ("after two", product[f"{nang}/implsch/2/ff"])):
        assert_cases_occur(ff, pr["WAVNUM"], pr["CINV"], case["tables"], nang, what, what == "first guess")
    wv = product[f"{nang}/step-in/wvprpt"]
    for what, key in (("step: first guess", "step-in"), ("after one step", "step/1"), ("after two", "step/2")):
        assert_cases_occur(product[f"{nang}/{key}/ff"], wv[:, 0], wv[:, 2], case["tables"], nang, what, key == "step-in")


@pytest.mark.parametrize("nang", list(SHAPES))
def test_the_point_without_stress_occurs_through_wdfluxes(product, nang):
    """The first WDFLUXES call reads the FF in which one point of every wavefront of kind 5 has no stress direction, hands that friction velocity
    to SINPUT, and shows it: no direction of that point is wind sea, every other point of its wavefront has some."""
    case = point_case(nang)
    n, pp = case["n"], PP[nang]
    _, ff0, _ = H.pack_device_inputs(case)
    dead = dead_points(n, pp)
    assert len(dead) == (wave_kinds(n, pp) == 5).sum() > 0 and stressless(ff0[dead, 7]).all()
    x = product[f"{nang}/wdfluxes/1/xllws"]
    for d in dead:
        a = d - d % pp
        assert not x[d].any(), ("XLLWS at the point without stress", int(d))
        assert all(x[i].any() for i in range(a, a + pp) if i != d), ("XLLWS at the other points of its wavefront", int(d))
    # (implsch() in between computes the friction velocity from the wind: the second WDFLUXES call finds the point with its neighbours)
    assert all(product[f"{nang}/wdfluxes/2/xllws"][d].any() for d in dead)
    assert not stressless(product[f"{nang}/implsch/1/ff"][:, 7]).any()


@pytest.mark.parametrize("path", ["implsch", "step", "wdfluxes"])
@pytest.mark.parametrize("nang", list(SHAPES))
def test_one_pass_run_length_gives_the_bits_of_the_row_by_row_test(product, nopar, nang, path):
    _same(product, nopar, f"{nang}/{path}/")
    if path != "wdfluxes":      # (WDFLUXES leaves the spectrum alone)
        assert not np.array_equal(product[f"{nang}/{path}/1/fl1"], product[f"{nang}/{path}/2/fl1"]), "the second call moved the spectrum"


@pytest.mark.parametrize("path", ["implsch", "step", "wdfluxes"])
@pytest.mark.parametrize("nang", list(SHAPES))
def test_one_pass_run_length_gives_the_bits_of_the_row_loop(product, nolead, nang, path):
    _same(product, nolead, f"{nang}/{path}/")


def test_double_precision_keeps_its_bits(product, nopar):
    _same(product, nopar, "36dp/implsch/")


if __name__ == "__main__":
    np.savez(sys.argv[1], **run_all())
