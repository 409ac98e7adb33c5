"""The code a wavefront of k_implsch4 runs once, trimmed (csrc/implsch_v4.h::V4_ONCE_TRIM; run with -m gpu on an MI355X): the product evaluates
WSIGSTAR with its free-convection power handed in by k_implsch4_pre, writes XLLWS from the 32-bit halves of the masks, takes FKMEAN's
DFIM / SQRT(WAVNUM) from the factor table (single precision) and skips SETICE's rows on a wave without an ice point; the library built with -DV4_ONCE_TRIM=0 (build
variant "notrim") runs the code as it was.  Both must give the SAME BITS -- FL1, XLLWS, FF, INTF, MIJ, compared as bit patterns (so that a -0 is not
a +0: SETICE's skipped F * 1 + 0 would turn one into the other) --

* through implsch() (twice: the second call runs on the UFRIC / Z0M the first one left), through the one-kernel step on the first rows of a tiny
  grid (twice) and through WDFLUXES (on the first guess and on the state one IMPLSCH call leaves),
* at 36, 24 and 12 directions in single precision and at 36 directions in double precision, on two full wavefronts and a short one (7 / 11 /
  21 / 7 points), in two scenarios each (the point count stays; a scenario is one more set of forcing on it).

The forcing of a scenario, point by point (SPEEDS, rotated by three points in the second scenario):
* wind speeds 35, 8, 2.13, 1.75, 1.0 and 0.5 m/s over one sea (the same JONSWAP peak along the wind at every point, deep water).  The rows of XLLWS
  that are set in the wind direction are a run [m0, 35]: 35 m/s gives m0 = 0 (row 0 set), 8 m/s an m0 between (row 0 clear, rows 31, 32, 35
  set), 2.13 m/s m0 = 32 (row 31 clear, row 32 set: the boundary of the mask's 32-bit halves), 1.75 m/s m0 = 34 or 35 (row 32 clear, row 35
  set), 1.0 and 0.5 m/s no wind-sea bin at all.  All but the first two without free convection (WSTAR = 0: the base of WSIGSTAR's third
  power is zero); at 0.5 m/s the log-profile wind UFRIC / XKAPPA LOG(10 / Z0M) is below WSPMIN, where WSIGSTAR's clamp acts.
* sea ice (CICOVER = 0.6 > CITHRSH): scenario 0 none in the first wavefront, the middle point of the second, the (one) point of the short third;
  scenario 1 every point of the first, none elsewhere.  A point under ice has MIJ = NFRE (IMPHFTAIL's loop is empty).
* one ice-free point of each scenario starts from a spectrum whose bins against the wind are -0.

That those cases occur is asserted on the host, in float64, from the FF the first implsch() call leaves (the UFRIC / Z0M its second SINFLX call
ran on): a direction can grow in row M only if LOG(WAVNUM(M) Z0M) + XKAPPA / (UFRIC (1 + SIG_N) CINV(M) + ZALP) < 0 at COSLP = 1
(sinput_ard.F90: ZLOG) -- "cannot grow" with the gustiness of the point widened by a quarter and 0.02, "grows" with none at COS of half a
direction bin, as tests/test_gpu_sinput_lead.py has it -- and the device's XLLWS is held against those bounds, so that the comparison
cannot pass on empty masks.

IMPHFTAIL with MIJ = 1 cannot be reached from a spectrum that is not negative: FRCUTINDEX's MIJ is the row of 2.5 FMEAN at the least, and
FMEAN >= FR(1) puts that at row 11 (asserted below from the tables); that some ice-free point has its cut-off below NFRE is asserted
instead, beside the points with MIJ = NFRE.  The product leaves IMPHFTAIL's division as it was.

The variant runs in a child process (ECWAM_HIP_LIB, as tests/test_gpu_sinput_lead.py runs "nolead"): this file run as a program writes its
results to the file named on its command line."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":      # the child process of the `variant` fixture: the suite's module path and seeds
    import conftest  # noqa: F401

import harness as H
from ecwam_amd import synthetic as syn
from ecwam_amd.tables import Config

pytestmark = pytest.mark.gpu

NAMES = ("fl1", "xllws", "ff", "intf", "mij")
# (directions, precision) -> (sea points per wavefront, NFRE_RED of the reference's registered configuration with that many directions)
SHAPES = {(36, "sp"): (3, 36), (24, "sp"): (5, 29), (12, "sp"): (10, 25), (36, "dp"): (3, 36)}
IDS = [f"{nang}-{prec}" for nang, prec in SHAPES]
GRID = 12      # the tiny grid of the one-kernel step (the smoke test's)
NSCEN = 2
HOT, MID, R32, R33, CALM, SLOW = 35.0, 8.0, 2.13, 1.75, 1.0, 0.5
SPEEDS = (HOT, MID, R32, R33, CALM, SLOW)
ICE = 0.6
SEED = 91
ROWS = (0, 31, 32, 35)


def npoints(key):
    return 2 * SHAPES[key][0] + 1      # two full wavefronts and a short one


def _cfg(key):
    return Config(nang=key[0], nfre=36, nfre_red=SHAPES[key][1], idelt=450, idelpro=450)


def scenario(key, s, wstar):
    """WSWAVE, WSTAR, CICOVER of the points of scenario s (wstar: the drawn free-convection velocities, kept where the wind is strong)."""
    pp, n = SHAPES[key][0], npoints(key)
    ws = np.array([SPEEDS[(i + 3 * s) % len(SPEEDS)] for i in range(n)])
    wst = np.where(ws >= MID, np.maximum(wstar[:n], 0.05), 0.0)
    ci = np.zeros(n)
    if s == 0:
        ci[pp + pp // 2] = ICE
        ci[2 * pp] = ICE
        ci[0] = 0.2      # ice below CITHRSH: no ice point
    else:
        ci[:pp] = ICE
    return ws, wst, ci


def minus_zero_point(key, s):
    """The ice-free point of scenario s whose spectrum starts with -0 against the wind."""
    return 1 if s == 0 else SHAPES[key][0] + 1


@contextlib.contextmanager
def deep_water(one_sea=False):
    """Every synthetic point in deep water: in two metres of water a wave of any frequency is slower than a light wind, and the wind speeds
    above would not decide the cases.  one_sea: the same JONSWAP peak at every point, along the point's wind -- the wave stress, and with it
    the row where the growth starts, then follows from the wind speed alone."""
    drawn = syn.point_params

    def params(n, seed=12345, **kw):
        p = drawn(n, seed, **dict(kw, shallow_fraction=0.0))
        if one_sea:
            p["FP"] = np.full(n, 0.2)
            p["THETAQ"] = p["WDWAVE"].copy()
        return p

    syn.point_params = params
    try:
        yield
    finally:
        syn.point_params = drawn


_CASES = {}


def point_case(key, s):
    """make_point_case's inputs with the forcing of scenario s: built once, shared, never modified."""
    if (key, s) not in _CASES:
        n = npoints(key)
        with deep_water(one_sea=True):
            case = H.make_point_case(n, _cfg(key), key[1], seed=SEED)
        p = case["params"]
        p["WSWAVE"], p["WSTAR"], p["CICOVER"] = scenario(key, s, p["WSTAR"])
        case["FF"] = syn.forcing(p, slice(0, n), case["tables"], H.np_dtype(key[1]))
        th = np.asarray(case["tables"].TH, dtype=np.float64)
        q = minus_zero_point(key, s)
        against = np.cos(th - p["WDWAVE"][q]) < -0.05
        case["FL1"][q, against, :] = -0.0
        _CASES[(key, s)] = case
    return _CASES[(key, s)]


def _snap(out, name, fl1, xllws, ff, intf, mij, n):
    for nm, t in zip(NAMES, (fl1, xllws, ff, intf, mij)):
        out[f"{name}/{nm}"] = t[:n].cpu().numpy().copy()


def run_all():
    """Every comparison's device results with the library this process loads: {"<directions>-<precision>/<scenario>/<path>/<call>/<array>": array}."""
    import torch

    from ecwam_amd import api, grid as G
    from ecwam_amd.wamintgr import Wamintgr

    out = {}
    for key, kid in zip(SHAPES, IDS):
        n = npoints(key)
        dt = H.np_dtype(key[1])
        for s in range(NSCEN):
            case = point_case(key, s)
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
                _snap(out, f"{kid}/{s}/implsch/{call}", fl1, xllws, ff, intf, mij, n)
            assert ctx.wdfluxes_supported()
            fl1, xllws, ff, intf, mij = fresh()
            ctx.wdfluxes(0, n, fl1, twv, ff, intf, mij, xllws)
            _snap(out, f"{kid}/{s}/wdfluxes/1", fl1, xllws, ff, intf, mij, n)
            ctx.implsch(0, n, fl1, twv, ff, intf, mij, xllws)
            ctx.wdfluxes(0, n, fl1, twv, ff, intf, mij, xllws)
            _snap(out, f"{kid}/{s}/wdfluxes/2", fl1, xllws, ff, intf, mij, n)
            torch.cuda.synchronize()
            ctx.close()
            # the one-kernel step on rows [0, n) of the tiny grid, twice
            g = G.build_grid(GRID, mask="continents")
            assert g.nsea >= n
            m = Wamintgr(case["cfg"], g, key[1])
            with deep_water():
                m.init_synthetic(seed=SEED)
            assert m.fused_available() and m.build_weights() == 0
            p = {k: np.array(v, copy=True) for k, v in m.params.items()}
            p["WSWAVE"][:n], p["WSTAR"][:n], p["CICOVER"][:n] = scenario(key, s, p["WSTAR"])
            m.ff[:, :14] = torch.from_numpy(syn.forcing(p, slice(0, g.nsea), m.t, dt)).to(m.dev)
            m.fl3.copy_(m.fl1)      # (the rows from n on are not stepped: they keep the start spectra in both buffers)
            for call in (1, 2):
                m.ctx.propags2_implsch(m.fl1, m.fl3, m.gd, m.cgroup_ext, float(m.cfg.idelpro), 0, n, m.wvprpt, m.ff, m.intf, m.mij, m.xllws, 1,
                                       m.cfg.nfre_red)
                m.fl1, m.fl3 = m.fl3, m.fl1
                _snap(out, f"{kid}/{s}/step/{call}", m.fl1, m.xllws, m.ff, m.intf, m.mij, n)
            torch.cuda.synchronize()
            m.ctx.close()
    return out


@pytest.fixture(scope="module")
def product():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert not os.environ.get("ECWAM_HIP_LIB"), "this test compares the product library with the variant: ECWAM_HIP_LIB must not be set"
    return run_all()


@pytest.fixture(scope="module")
def variant(product, tmp_path_factory):
    from ecwam_amd import build

    lib = build.lib_path("notrim")
    if not os.path.exists(lib):
        build.build(variant="notrim")
    path = str(tmp_path_factory.mktemp("notrim") / "variant.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, ECWAM_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def gustiness(ff, tables):
    """SIG_N of wsigstar.F90 (the form without LLGCBZ0 / LLNORMAGAM) from WSTAR, UFRIC and Z0M of FF, in float64."""
    u10 = np.maximum(log_profile_wind(ff, tables), float(tables.WSPMIN))
    wstar = ff[:, 4].astype(np.float64)
    c1, c2, p1, p2 = 1.03e-3, 0.04e-3, 1.48, -0.21
    c2u10p1, u10p2 = c2 * u10 ** p1, u10 ** p2
    c_d = (c1 + c2u10p1) * u10p2
    dc_ddu = (p2 * c1 + (p1 + p2) * c2u10p1) * u10p2 / u10
    sig_conv = 1.0 + 0.5 * u10 / c_d * dc_ddu
    return np.minimum(0.9, sig_conv / u10 * np.cbrt(0.5 * float(tables.XKAPPA) * wstar ** 3))


def log_profile_wind(ff, tables):
    """WSIGSTAR's U10 before its clamp at WSPMIN."""
    ufric, z0m = ff[:, 7].astype(np.float64), ff[:, 10].astype(np.float64)
    return ufric / float(tables.XKAPPA) * (np.log(10.0) - np.log(z0m))


def first_growing_row(ff, wavnum, cinv, tables, sig_n, coslp):
    """Per point the first row M (0-based; NFRE: none) in which ZLOG < 0 at the given gustiness and COSLP, in float64."""
    ufric, z0m = ff[:, 7].astype(np.float64)[:, None], ff[:, 10].astype(np.float64)[:, None]
    k, ci = wavnum.astype(np.float64), cinv.astype(np.float64)
    zlog = np.log(k * z0m) + float(tables.XKAPPA) / (ufric * (1.0 + np.reshape(sig_n, (-1, 1))) * ci + float(tables.ZALP)) / coslp
    grows = zlog < 0.0
    return np.where(grows.any(1), grows.argmax(1), grows.shape[1])


def mask_bounds(ff, wavnum, cinv, tables, nang):
    """(lo, hi) per point: no direction has a wind-sea bin in a row below lo, the wind direction's neighbour has one in every row from hi on."""
    lo = first_growing_row(ff, wavnum, cinv, tables, np.minimum(0.9, 1.25 * gustiness(ff, tables) + 0.02), 1.0)
    hi = first_growing_row(ff, wavnum, cinv, tables, np.zeros(ff.shape[0]), np.cos(np.pi / nang))
    assert (lo <= hi).all()
    return lo, hi


def _same(product, variant, prefix):
    keys = [k for k in product if k.startswith(prefix) and k.rsplit("/", 1)[1] in NAMES]
    assert len(keys) == 2 * len(NAMES) and all(k in variant for k in keys)
    for k in keys:
        x, y = product[k], variant[k]
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.isfinite(x).all(), k
        # the same bits (torch.equal's element-wise == and, beyond it, the sign of a zero)
        assert np.array_equal(x, y) and x.tobytes() == y.tobytes(), f"{k}: {int((x != y).sum())} of {x.size} elements differ (or the sign of a zero)"


@pytest.mark.parametrize("key", list(SHAPES), ids=IDS)
def test_the_cases_occur(product, key):
    """The FF the first implsch() call leaves puts the points into the cases they were built for, and the device's XLLWS has the rows the
    host's bounds ask for."""
    nang, pp, n, nfre = key[0], SHAPES[key][0], npoints(key), 36
    t = point_case(key, 0)["tables"]
    # FRCUTINDEX: MIJ >= the row of TAILFACTOR FR(1), whatever the spectrum (FMEAN >= FR(1))
    assert int(round(np.log10(float(t.TAILFACTOR)) * float(t.FLOGSPRDM1))) + 1 >= 11
    seen = {r: set() for r in ROWS}
    boundary = above = none = clamp = noclamp = wstar0 = cut = 0
    for s in range(NSCEN):
        case = point_case(key, s)
        pr = case["props"]
        kid = IDS[list(SHAPES).index(key)]
        ff, xl, mij = (product[f"{kid}/{s}/implsch/1/{nm}"] for nm in ("ff", "xllws", "mij"))
        ws, wst, ci = scenario(key, s, case["params"]["WSTAR"])
        lo, hi = mask_bounds(ff, pr["WAVNUM"], pr["CINV"], t, nang)
        anyk = (xl != 0).any(1)      # [point][M]: some direction has a wind-sea bin in row M
        assert set(np.unique(xl)) <= {0.0, 1.0}
        for i in range(n):
            assert not anyk[i, :lo[i]].any() and anyk[i, hi[i]:].all(), (s, i, ws[i], lo[i], hi[i], anyk[i])
            for r in ROWS:
                if r < lo[i]:
                    seen[r].add(False)
                if r >= hi[i]:
                    seen[r].add(True)
        # item 2: the runs of set rows the wind speeds were chosen for
        assert (hi[ws == HOT] == 0).all() and ((lo[ws == MID] > 0) & (hi[ws == MID] <= 31)).all()
        boundary += int(((lo == 32) & (hi == 32)).sum())
        above += int(((lo > 32) & (hi < nfre)).sum())
        none += int((lo == nfre).sum())
        assert (lo[ws <= CALM] == nfre).all(), "1 m/s and below: no wind-sea bin at all"
        # item 1: the clamp at WSPMIN, a zero base of the third power
        u10 = log_profile_wind(ff, t)
        clamp += int((u10[ws == SLOW] < float(t.WSPMIN)).sum())
        assert (u10[ws == SLOW] < float(t.WSPMIN)).all() and (u10[ws >= MID] > float(t.WSPMIN)).all()
        noclamp += int((ws >= MID).sum())
        wstar0 += int((ff[:, 4] == 0).sum())
        assert (ff[:, 4][ws >= MID] > 0).all()
        # item 4: the ice points of the wavefronts; item 3: MIJ = NFRE under ice, a cut-off inside the range in a strong wind
        icy = ff[:, 2] > float(t.CITHRSH)
        per_wave = [int(icy[w * pp:(w + 1) * pp].sum()) for w in range(3)]
        assert per_wave == ([0, 1, 1] if s == 0 else [pp, 0, 0]) and (ff[:, 2] > 0).sum() == sum(per_wave) + (s == 0)
        assert (mij[icy] == nfre).all()
        cut += int((mij[~icy] < nfre).sum())
        q = minus_zero_point(key, s)
        assert not icy[q] and np.signbit(case["FL1"][q]).any()
    assert all(seen[r] == {False, True} for r in ROWS), seen
    assert min(boundary, above, none, clamp, noclamp, wstar0, cut) > 0, (boundary, above, none, clamp, noclamp, wstar0, cut)


@pytest.mark.parametrize("path", ["implsch", "step", "wdfluxes"])
@pytest.mark.parametrize("s", range(NSCEN))
@pytest.mark.parametrize("key", list(SHAPES), ids=IDS)
def test_trimmed_once_per_wave_code_gives_the_same_bits(product, variant, key, s, path):
    kid = IDS[list(SHAPES).index(key)]
    _same(product, variant, f"{kid}/{s}/{path}/")
    if path != "wdfluxes":      # (WDFLUXES leaves the spectrum alone)
        assert not np.array_equal(product[f"{kid}/{s}/{path}/1/fl1"], product[f"{kid}/{s}/{path}/2/fl1"]), "the second call moved the spectrum"


if __name__ == "__main__":
    np.savez(sys.argv[1], **run_all())
