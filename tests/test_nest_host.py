"""Nested-grid boundary spectra without a GPU: the numpy restatement of INTSPEC (tests/intspec_ref.py) against what the reference's own
INTSPEC returned (tests/golden/intspec_nang12.npz, written by tools/make_golden_nest.py), the construction of that fixture, the interface
the library exports, and the boundary file of ecwam_amd/nest.py.

Measured here, restatement against the reference over the 96 cases (printed by test_restatement_against_the_reference):
  float64 against the double precision build: per bin 3.54e-15 of the peak, energy 3.35e-15, THQ 1.78e-15 rad, EMEAN and FMEAN bit-equal
  float32 against the single precision build: per bin 1.91e-6 of the peak, energy 2.11e-6, THQ 9.54e-7 rad, EMEAN and FMEAN bit-equal
Three times these figures are the gates of this file and of tests/test_gpu_nest.py (intspec_ref.GATE).
The reference alone, single against double precision: at most 1.46e-6 of the peak in a bin (median 4.1e-7); the condition is 1e-4.
"""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import intspec_ref as R
from ecwam_amd import lib, nest
from ecwam_amd.tables import Config, Tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = dict(dp=np.float64, sp=np.float32)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "intspec_nang12.npz")))


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the two entry points, with the documented argument counts, at ABI 6, 72 exports in all."""
    want = {"ecwam_hip_bouinpt": 14, "ecwam_hip_outbc": 7}
    assert set(want) <= set(lib.EXPORTS) and len(lib.EXPORTS) == 72 and len(set(lib.EXPORTS)) == 72
    with open(os.path.join(ROOT, "include", "ecwam_hip.h")) as fh:
        hdr = fh.read()
    for name, nargs in want.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    assert "must be distinct" in hdr
    assert lib.ABI_VERSION == 6 and re.search(r"#define ECWAM_HIP_ABI_VERSION 6\b", hdr)
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in want:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    assert h.ecwam_hip_bouinpt(None, 0, 0, 0, None, None, None, None, 0, None, None, None, None, None) == 1 and h.ecwam_hip_last_error() == b"null context"
    assert h.ecwam_hip_outbc(None, 0, None, None, None, None, None) == 1 and h.ecwam_hip_last_error() == b"null context"
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    assert "NAME='ecwam_hip_bouinpt'" in f90 and "NAME='ecwam_hip_outbc'" in f90


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_restatement_against_the_reference(golden, prec):
    g, dt = golden, DT[prec]
    t = Tables(Config(nang=int(g["nang"]), nfre=int(g["nfre"]), nfre_red=int(g["nfre"])), dt)
    assert np.array_equal(np.asarray(t.FR), g["fr_" + prec]) and g["fr_" + prec].dtype == dt      # the model's own frequencies
    ebin = een = eth = 0.0
    for i in range(g["bfw"].size):
        par = g["par"][i]
        fl, fm, em, th = R.intspec(t.FR, g["bfw"][i], g["f"][i, 0], par[0, 2], par[0, 0], par[0, 1], g["f"][i, 1], par[1, 2], par[1, 0], par[1, 1], dt)
        assert fl.dtype == dt
        a, b = R.errors(fl, g["fl_" + prec][i], t.DFIM)
        ebin, een = max(ebin, a), max(een, b)
        ref = g["par_" + prec][i]
        assert em == ref[0] and fm == ref[2], (i, em, ref[0], fm, ref[2])
        d = abs(float(th) - float(ref[1]))
        eth = max(eth, min(d, 2 * np.pi - d))
    print(f"restatement against the reference, {prec}: per bin {ebin:.3e} of the peak, energy {een:.3e}, THQ {eth:.3e} rad")
    gate = R.GATE[prec]
    assert ebin < gate["bin"] and een < gate["energy"] and eth < gate["thq"], (ebin, een, eth, gate)


def test_the_fixture_has_no_knife_edges(golden):
    """Each GAMMA is 1.1**(n+f) with f in [0.1, 0.9] and n in -3 .. 2, 1.1**n (1 +- 3e-4) with the sign away from zero, or 1 -- checked from the
    stored inputs -- and the reference's single and double precision results then agree to 1e-4 of the peak in every bin of every case."""
    g = golden
    n = g["bfw"].size
    assert 90 <= n <= 110 and g["f"].dtype == np.float32 and g["par"].dtype == np.float32 and g["bfw"].dtype == np.float32
    seen = set()
    for i in range(n):
        w2 = np.float64(g["bfw"][i])
        assert 0 < w2 < 1
        fm1, fm2 = np.float64(g["par"][i, 0, 2]), np.float64(g["par"][i, 1, 2])
        fmean = (1 - w2) * fm1 + w2 * fm2
        for fm in (fm1, fm2):
            if fm1 == fm2:
                seen.add("one")
                continue
            gam = fm / fmean
            x = np.log(gam) / np.log(1.1)
            nn = int(np.rint(x))
            r = gam / 1.1 ** nn - 1
            if abs(abs(r) - 3e-4) < 2e-5:
                assert -3 <= nn <= 2 and (nn == 0 or np.sign(r) == np.sign(nn)), (i, gam)
                seen.add("shift")
            else:
                fl = np.floor(x)
                assert -3 <= fl <= 2 and 0.1 - 1e-3 <= x - fl <= 0.9 + 1e-3, (i, gam, x)
                seen.add("interp")
    assert seen == {"one", "shift", "interp"}
    peak = np.abs(g["fl_dp"]).max(axis=(1, 2), keepdims=True)
    d = np.abs(g["fl_sp"].astype(np.float64) - g["fl_dp"]) / peak
    print(f"the reference, single against double precision: max {d.max():.2e} of the peak, median of the cases {np.median(d.max(axis=(1, 2))):.2e}")
    assert np.isfinite(d).all() and d.max() < 1e-4


def test_bouinpt_point_quirks():
    """The restatement keeps the reference's quirks: BFW <= 0 copies the left record, a spectrum without energy leaves the other one times its
    weight, |INC| >= NFRE leaves zeros, and a rotation by NANG - 1 bins and a half wraps in K."""
    t = Tables(Config(nang=12, nfre=36, nfre_red=36), np.float64)
    rng = np.random.default_rng(3)
    f1 = rng.uniform(0.1, 1.0, (2, 36, 12))
    par1 = np.array([[1.0, 0.3, 0.1], [2.0, 1.1, 0.2]])
    fl, par = R.bouinpt_point(t.FR, 0.0, 2, 1, f1, par1, np.float64)
    assert np.array_equal(fl, f1[1]) and par == (2.0, 1.1, 0.2)
    fl, par = R.bouinpt_point(t.FR, 0.25, 0, 2, f1, par1, np.float64)
    assert np.array_equal(fl, 0.25 * f1[1]) and par == (0.5, 1.1, 0.2)
    fl, par = R.bouinpt_point(t.FR, 0.25, 1, 0, f1, par1, np.float64)
    assert np.array_equal(fl, 0.75 * f1[0]) and par == (0.75, 0.3, 0.1)
    fl, _ = R.bouinpt_point(t.FR, 0.99, 1, 2, f1, np.array([[1.0, 0.3, 0.2], [1.0, 0.3, 0.2e-4]]), np.float64)
    assert not fl.any()
    a = 0.5 * float(t.DELTH)
    fl, par = R.bouinpt_point(t.FR, 0.5, 1, 2, f1, np.array([[1.0, a, 0.1], [1.0, -a, 0.1]]), np.float64)
    assert par[1] == 0.0
    want = 0.5 * (0.5 * np.roll(f1[0], -1, axis=1) + 0.5 * f1[0]) + 0.5 * (0.5 * f1[1] + 0.5 * np.roll(f1[1], 1, axis=1))
    assert np.allclose(fl, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_boundary_file_round_trip_and_bytes(prec):
    dt = DT[prec]
    rb = np.dtype(dt).itemsize
    t = Tables(Config(nang=12, nfre=36, nfre_red=36), dt)
    rng = np.random.default_rng(5)
    n = 3
    par = rng.uniform(0.1, 2.0, (2, n, 3)).astype(dt)
    fl = rng.uniform(0.0, 1.0, (2, n, 36, 12)).astype(dt)
    lon, lat = np.arange(n, dtype=dt) * dt(0.5), np.arange(n, dtype=dt) * dt(0.25) + dt(40)
    dates = ["20261019000000", "20261019003000"]
    f = io.BytesIO()
    nest.write_header(f, 12, 36, t.TH[0], t.FR[0], t.FRATIO, n, 1800, dt)
    for s in range(2):
        nest.write_points(f, lon, lat, dates[s], par[s], fl[s], dt)
    raw = f.getvalue()
    # the bytes: every record framed by its length; the header seven reals, a point record five reals and the 14 characters, a spectrum NANG NFRE reals
    lens, off = [], 0
    while off < len(raw):
        m = int(np.frombuffer(raw[off: off + 4], "<i4")[0])
        assert int(np.frombuffer(raw[off + 4 + m: off + 8 + m], "<i4")[0]) == m
        lens.append(m)
        off += 8 + m
    assert off == len(raw)
    assert lens == [7 * rb] + [5 * rb + 14, 12 * 36 * rb] * (2 * n)
    assert np.array_equal(np.frombuffer(raw[4: 4 + 7 * rb], np.dtype(dt).newbyteorder("<")),
                          np.array([12, 36, t.TH[0], t.FR[0], t.FRATIO, n, 1800], dtype=dt))
    p0 = 8 + 7 * rb + 4
    assert raw[p0 + 2 * rb: p0 + 2 * rb + 14] == b"20261019000000"
    assert np.array_equal(np.frombuffer(raw[p0 + 2 * rb + 14: p0 + 5 * rb + 14], np.dtype(dt).newbyteorder("<")), par[0, 0])
    s0 = p0 + 5 * rb + 14 + 8
    assert np.array_equal(np.frombuffer(raw[s0: s0 + 12 * 36 * rb], np.dtype(dt).newbyteorder("<")), fl[0, 0].reshape(-1))      # [M][K], K fastest
    # and back
    f.seek(0)
    h = nest.read_header(f, dt)
    assert (h.nang, h.nfre, h.nbou, h.idelpro) == (12, 36, n, 1800) and h.th0 == t.TH[0] and h.fr1 == t.FR[0] and h.fratio == t.FRATIO
    for s in range(2):
        xlon, xlat, cdate, p, sp = nest.read_points(f, h, dt)
        assert cdate == dates[s] and np.array_equal(xlon, lon) and np.array_equal(xlat, lat)
        assert p.dtype == dt and np.array_equal(p, par[s]) and np.array_equal(sp, fl[s])
    assert nest.read_points(f, h, dt) is None
    # a truncated file and a short date are errors
    with pytest.raises(nest.NestFileError):
        g = io.BytesIO(raw[:-10])
        hh = nest.read_header(g, dt)
        while nest.read_points(g, hh, dt) is not None:
            pass
    with pytest.raises(nest.NestFileError):
        nest.write_points(io.BytesIO(), lon, lat, "2026101900", par[0], fl[0], dt)


def test_header_consistency_checks():
    """bouinpt.F90:186-187: NANG, NFRE, TH(1), FR(1), and the input step a multiple of IDELPRO and not smaller."""
    t = Tables(Config(nang=12, nfre=36, nfre_red=36), np.float32)
    ok = dict(nang=12, nfre=36, th0=t.TH[0], fr1=t.FR[0], fratio=t.FRATIO, nbou=5, idelpro=1800)
    nest.check_header(nest.Header(**ok), 12, 36, t.TH[0], t.FR[0], 900)
    nest.check_header(nest.Header(**ok), 12, 36, t.TH[0], t.FR[0], 1800)
    for change, word in ((dict(nang=24), "NANG"), (dict(nfre=30), "NFRE"), (dict(th0=np.nextafter(t.TH[0], np.float32(1))), "TH(1)"),
                         (dict(fr1=np.nextafter(t.FR[0], np.float32(1))), "FR(1)"), (dict(idelpro=1000), "multiple"), (dict(idelpro=0), "smaller")):
        with pytest.raises(nest.NestFileError, match=re.escape(word)):
            nest.check_header(nest.Header(**{**ok, **change}), 12, 36, t.TH[0], t.FR[0], 900)
    with pytest.raises(nest.NestFileError, match="multiple"):
        nest.check_header(nest.Header(**ok), 12, 36, t.TH[0], t.FR[0], 3600)      # 1800 is smaller than 3600, and no multiple of it
