"""SINPUT's leading rows without growth (csrc/implsch_v4.h::v4_sinput, single precision; run with -m gpu on an MI355X): the product takes the
run of low-frequency rows in which no direction of any point of the wavefront grows out in front of the row loop; the library built with
-DV4_SINPUT_LEAD=0 (build variant "nolead") sends every row through the row loop.  Both must give the SAME BITS -- FL1, XLLWS, FF, INTF, MIJ --

* through implsch(), through the one-kernel step (ecwam_hip_propags2_implsch on rows [0, n)) and through WDFLUXES,
* at 36 directions on 1 501 points (500 full wavefronts of three points and a short one), at 24 and 12 directions on 1 001 (five / ten points
  per wavefront), two consecutive calls each so that the second runs on the UFRIC / Z0M the first one left,
* with the wind speed set per wavefront so that the run is empty (all points at 35 m/s), all 36 rows (all at 1 m/s; the kernel hands the
  last two of them back to its row loop, which takes rows in pairs), in between (all at 8 m/s), and set by one windy point (20 m/s)
  between calm ones; the short last wavefront is calm.

That those cases occur is asserted on the host, in float64, from every FF state the calls read or leave: a direction can grow in row M only if
LOG(WAVNUM(M) Z0M) + XKAPPA / (UFRIC (1 + SIG_N) CINV(M) + ZALP) < 0 at COSLP = 1 (sinput_ard.F90: ZLOG).  "Cannot grow" is asserted with the
gustiness of the point (wsigstar.F90 restated in float64, widened by a quarter and 0.02), "grows" with none and at COS of half a direction
bin.  The free-convection velocity WSTAR is zero in the calm wavefronts: at 1 m/s a WSTAR of 0.5 m/s alone is a gustiness of 0.3, under which
the slowest waves of the grid (rows 34, 35) do grow.

The variant runs in a child process (ECWAM_HIP_LIB, as tests/test_gpu_fused.py runs "ctustrict"): this file run as a program writes its
results to the file named on its command line.  The 36-direction implsch() result is also held against the oracle at the harness's gates."""
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
# directions -> (points, NFRE_RED of the reference's registered configuration with that many directions, grid size with at least that many sea points)
SHAPES = {36: (1501, 36, 24), 24: (1001, 29, 17), 12: (1001, 25, 17)}
PP = {36: 3, 24: 5, 12: 10}      # sea points per wavefront in single precision
HOT, CALM, MID, WINDY = 35.0, 1.0, 8.0, 20.0
SEED = 77


def _cfg(nang):
    return Config(nang=nang, nfre=36, nfre_red=SHAPES[nang][1], idelt=450, idelpro=450)


def wave_kinds(n, pp):
    """The case of every wavefront: 0 all hot, 1 all calm, 2 all at the middle speed, 3 one windy point between calm ones; the last
    (short) wavefront calm."""
    kinds = np.arange((n + pp - 1) // pp) % 4
    kinds[-1] = 1
    return kinds


def wind_speeds(n, pp):
    kinds = wave_kinds(n, pp)
    ws = np.empty(n)
    for i in range(n):
        k = kinds[i // pp]
        ws[i] = (HOT, CALM, MID, WINDY if i % pp == pp // 2 else CALM)[k]
    return ws


def calm_wstar(wstar, n, pp):
    """WSTAR with the calm wavefronts' points at zero (no gustiness there)."""
    calm = wave_kinds(n, pp)[np.arange(n) // pp] == 1
    return np.where(calm, 0.0, wstar[:n])


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


_CASES = {}


def point_case(nang):
    """make_point_case's inputs with the wind speeds of the cases: built once, shared, never modified."""
    if nang not in _CASES:
        n = SHAPES[nang][0]
        with deep_water():
            case = H.make_point_case(n, _cfg(nang), "sp", seed=SEED)
        case["params"]["WSWAVE"] = wind_speeds(n, PP[nang])
        case["params"]["WSTAR"] = calm_wstar(case["params"]["WSTAR"], n, PP[nang])
        case["FF"] = syn.forcing(case["params"], slice(0, n), case["tables"], np.float32)
        _CASES[nang] = case
    return _CASES[nang]


def _snap(out, key, fl1, xllws, ff, intf, mij, n):
    for name, t in zip(NAMES, (fl1, xllws, ff, intf, mij)):
        out[f"{key}/{name}"] = t[:n].cpu().numpy().copy()


def run_all():
    """Every comparison's device results with the library this process loads: {"<directions>/<path>/<call>/<array>": numpy array}."""
    import torch

    from ecwam_amd import api, grid as G
    from ecwam_amd.wamintgr import Wamintgr

    out = {}
    for nang in SHAPES:
        case = point_case(nang)
        n = case["n"]
        ctx = api.HipContext(case["tables"])
        dev = ctx.device
        wv, ff0, intf0 = H.pack_device_inputs(case)

        def fresh():
            fl1 = torch.from_numpy(case["FL1"].copy()).to(dev)
            return (fl1, torch.zeros_like(fl1), torch.from_numpy(ff0.copy()).to(dev), torch.from_numpy(intf0.copy()).to(dev),
                    torch.zeros(n, dtype=torch.int32, device=dev))

        twv = torch.from_numpy(wv).to(dev)
        # implsch(), twice
        fl1, xllws, ff, intf, mij = fresh()
        for call in (1, 2):
            ctx.implsch(0, n, fl1, twv, ff, intf, mij, xllws)
            _snap(out, f"{nang}/implsch/{call}", fl1, xllws, ff, intf, mij, n)
        # WDFLUXES on the first guess, and on the state one IMPLSCH call leaves
        assert ctx.wdfluxes_supported()
        fl1, xllws, ff, intf, mij = fresh()
        ctx.wdfluxes(0, n, fl1, twv, ff, intf, mij, xllws)
        _snap(out, f"{nang}/wdfluxes/1", fl1, xllws, ff, intf, mij, n)
        ctx.implsch(0, n, fl1, twv, ff, intf, mij, xllws)
        ctx.wdfluxes(0, n, fl1, twv, ff, intf, mij, xllws)
        _snap(out, f"{nang}/wdfluxes/2", fl1, xllws, ff, intf, mij, n)
        torch.cuda.synchronize()
        ctx.close()
        # the one-kernel step on rows [0, n) of a grid, twice
        g = G.build_grid(SHAPES[nang][2], mask="continents")
        assert g.nsea >= n
        m = Wamintgr(case["cfg"], g, "sp")
        with deep_water():
            m.init_synthetic(seed=SEED)
        assert m.fused_available() and m.build_weights() == 0
        p = dict(m.params)
        p["WSWAVE"] = p["WSWAVE"].copy()
        p["WSWAVE"][:n] = wind_speeds(n, PP[nang])
        p["WSTAR"] = p["WSTAR"].copy()
        p["WSTAR"][:n] = calm_wstar(p["WSTAR"], n, PP[nang])
        m.ff[:, :14] = torch.from_numpy(syn.forcing(p, slice(0, g.nsea), m.t, np.float32)).to(m.dev)
        out[f"{nang}/step-in/ff"] = m.ff[:n].cpu().numpy().copy()
        out[f"{nang}/step-in/wvprpt"] = m.wvprpt[:n].cpu().numpy().copy()
        m.fl3.copy_(m.fl1)      # (the rows from n on are not stepped: they keep the start spectra in both buffers)
        for call in (1, 2):
            m.ctx.propags2_implsch(m.fl1, m.fl3, m.gd, m.cgroup_ext, float(m.cfg.idelpro), 0, n, m.wvprpt, m.ff, m.intf, m.mij, m.xllws, 1,
                                   m.cfg.nfre_red)
            m.fl1, m.fl3 = m.fl3, m.fl1
            _snap(out, f"{nang}/step/{call}", m.fl1, m.xllws, m.ff, m.intf, m.mij, n)
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

    lib = build.lib_path("nolead")
    if not os.path.exists(lib):
        build.build(variant="nolead")
    path = str(tmp_path_factory.mktemp("nolead") / "variant.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, ECWAM_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


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


def assert_cases_occur(ff, wavnum, cinv, tables, nang, what):
    n, pp, nfre = ff.shape[0], PP[nang], wavnum.shape[1]
    kinds = wave_kinds(n, pp)
    # bounds of the row where a point's growth starts: not before `lo` (COSLP = 1, the stronger gust state with a margin on its gustiness), at
    # `hi` at the latest (no gustiness -- the first call has none --, the direction half a bin off the stress)
    lo = first_growing_row(ff, wavnum, cinv, tables, np.minimum(0.9, 1.25 * gustiness(ff, tables) + 0.02), 1.0)
    hi = first_growing_row(ff, wavnum, cinv, tables, np.zeros(n), np.cos(np.pi / nang))
    assert (lo <= hi).all()
    seen = set()
    for w, kind in enumerate(kinds):
        a, b = w * pp, min(n, (w + 1) * pp)
        if kind == 0:
            assert (hi[a:b] == 0).all(), (what, w, "35 m/s: growth in row 0", hi[a:b])
        elif kind == 1:
            assert (lo[a:b] == nfre).all(), (what, w, "1 m/s: no growth in any row", lo[a:b])
        elif kind == 2:
            assert (lo[a:b] > 0).all() and (hi[a:b] < nfre).all(), (what, w, "8 m/s: a leading run that ends before the last row", lo[a:b], hi[a:b])
        else:
            windy = a + pp // 2
            calm = [i for i in range(a, b) if i != windy]
            assert (hi[windy] < lo[calm]).all(), (what, w, "the windy point sets the run", hi[windy], lo[calm])
        seen.add(int(kind))
    assert seen == {0, 1, 2, 3} and kinds[-1] == 1 and n % pp != 0, "every case, and a short calm last wavefront"


def _same(product, variant, prefix):
    keys = [k for k in product if k.startswith(prefix) and k.rsplit("/", 1)[1] in NAMES]
    assert len(keys) == 2 * len(NAMES) and all(k in variant for k in keys)
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
        assert_cases_occur(ff, pr["WAVNUM"], pr["CINV"], case["tables"], nang, what)
    wv = product[f"{nang}/step-in/wvprpt"]
    for what, key in (("step: first guess", "step-in"), ("after one step", "step/1"), ("after two", "step/2")):
        assert_cases_occur(product[f"{nang}/{key}/ff"], wv[:, 0], wv[:, 2], case["tables"], nang, what)


@pytest.mark.parametrize("path", ["implsch", "step", "wdfluxes"])
@pytest.mark.parametrize("nang", list(SHAPES))
def test_leading_rows_taken_out_give_the_same_bits(product, variant, nang, path):
    _same(product, variant, f"{nang}/{path}/")
    if path != "wdfluxes":      # (WDFLUXES leaves the spectrum alone)
        assert not np.array_equal(product[f"{nang}/{path}/1/fl1"], product[f"{nang}/{path}/2/fl1"]), "the second call moved the spectrum"


def test_implsch_with_the_leading_rows_taken_out_matches_the_oracle(product):
    """The 36-direction case, first call, against the oracle at the harness's single-precision gates."""
    from oracle.oracle import Oracle

    case = point_case(36)
    ref = H.oracle_implsch(case, Oracle(case["cfg"], "sp"))
    got = {"FL1": product["36/implsch/1/fl1"], "XLLWS": product["36/implsch/1/xllws"], "MIJ": product["36/implsch/1/mij"],
           "FF": product["36/implsch/1/ff"][:, :14], "INTF": product["36/implsch/1/intf"][:, :15]}
    st = H.compare_implsch(ref, got, case["tables"])
    H.assert_sp_gates(st, case["n"])


if __name__ == "__main__":
    np.savez(sys.argv[1], **run_all())
