"""GRIB-ready output without a GPU: the interface the library exports (include/ecwam_hip_gribout.h), the map of ecwam_amd/gribout.py::value_map
against hand-written positions, and the numpy restatement of OUTSPEC's mask, the block-to-grid step and WGRIBENCODE_VALUES
(tests/gribout_ref.py) against the reference's own results (tests/golden/gribout_0.npz, recorded by tools/make_golden_gribout.py), in both
precisions.  The figures are read from tests/golden/gribout_observed.json, where the tool wrote what the reference and the restatement gave --
nothing there comes from the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gribout_ref as G
from ecwam_amd import gribout, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hip_set_grib_map": 5, "ecwam_hip_outspec_values": 12, "ecwam_hip_outspec_pack": 11, "ecwam_hip_grib_values": 12}


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the entry points, in a header and a list of their own, at ABI 6 and beside the lists published before."""
    assert lib.EXPORTS_GRIBOUT == list(WANT)
    assert len(lib.EXPORTS) == 72 and len(lib.EXPORTS_START) == 4 and len(lib.EXPORTS_FORCING) == 7 and lib.ABI_VERSION == 6
    assert not set(WANT) & (set(lib.EXPORTS) | set(lib.EXPORTS_START) | set(lib.EXPORTS_FORCING))
    with open(os.path.join(ROOT, "include", "ecwam_hip_gribout.h")) as fh:
        hdr = fh.read()
    assert '#include "ecwam_hip.h"' in hdr
    assert re.findall(r"^int (ecwam_hip_\w+)\(", hdr, re.M) == list(WANT)      # exactly these, in this order
    for name, nargs in WANT.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    for other in ("ecwam_hip.h", "ecwam_hip_start.h", "ecwam_hip_forcing.h"):
        with open(os.path.join(ROOT, "include", other)) as fh:
            assert not set(WANT) & set(re.findall(r"\b(ecwam_hip_\w+)\s*\(", fh.read())), other
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    for name in WANT:
        assert f"NAME='{name}'" in f90, name
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in WANT:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    ll = C.c_longlong(1)
    calls = (lambda: h.ecwam_hip_set_grib_map(None, 0, None, 1, None),
             lambda: h.ecwam_hip_outspec_values(None, 0, 0, None, None, 0, 1, 0, None, None, None, None),
             lambda: h.ecwam_hip_outspec_pack(None, 0, 0, None, None, 0, 1, 0, None, 0, None),
             lambda: h.ecwam_hip_grib_values(None, 0, 0, None, ll, ll, 1, 0, None, None, None, None))
    assert len(calls) == len(WANT)
    for call in calls:
        assert call() == 1 and h.ecwam_hip_last_error() == b"null context"      # refused before anything else


def test_the_structs_have_the_layout_the_c_compiler_gives_them(tmp_path):
    src = ('#include "ecwam_hip_gribout.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %d", sizeof(ecwam_hip_grib_opts), '
           'offsetof(ecwam_hip_grib_opts, ngrbress), offsetof(ecwam_hip_grib_opts, zmiss), sizeof(ecwam_hip_grib_poles), offsetof(ecwam_hip_grib_poles, south), '
           'ECWAM_HIP_OUTSPEC_ICEMASK);return 0;}')
    exe = str(tmp_path / "grib_structs")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got == [C.sizeof(lib.GribOpts), lib.GribOpts.ngrbress.offset, lib.GribOpts.zmiss.offset, C.sizeof(lib.GribPoles), lib.GribPoles.south.offset,
                   lib.OUTSPEC_ICEMASK]
    assert [n for n, _ in lib.GribOpts._fields_] == list(gribout.GRIB_DEFAULTS)


def test_value_map_against_hand_written_positions():
    # a reduced grid of 5 rows, NLONRGG = 4 6 8 6 4 south to north (28 values), both poles: row J of FIELD starts at 0, 4, 10, 18, 24
    nlon = [4, 6, 8, 6, 4]
    ixlg = [1, 3, 2, 6, 1, 8, 5, 4, 2]
    kxlt = [1, 1, 2, 2, 3, 3, 4, 5, 5]
    ival, ntencode, poles = gribout.value_map(nlon, ixlg, kxlt, 5, 1, 90.0, -90.0, 45.0, "g", True)
    assert ntencode == 28 and ival.dtype == np.int32
    assert ival.tolist() == [24, 26, 19, 23, 10, 17, 8, 3, 1]
    assert poles.north == gribout.Pole(0, 4, 4, 6) and poles.south == gribout.Pole(24, 4, 18, 6)
    assert poles.as_ints() == [0, 4, 4, 6, 24, 4, 18, 6]
    # the same grid ending short of the poles, or without LPADPOLES: no padding
    assert gribout.value_map(nlon, ixlg, kxlt, 5, 1, 60.0, -60.0, 30.0, "g", True)[2] == gribout.Poles()
    assert gribout.value_map(nlon, ixlg, kxlt, 5, 1, 90.0, -90.0, 45.0, "g", False)[2] == gribout.Poles()
    one = gribout.value_map(nlon, ixlg, kxlt, 5, 1, 90.0, -30.0, 30.0, "g", True)[2]
    assert one.north.npole == 4 and one.south.npole == 0
    # case B: a regular 8 x 5 grid from 72 N to the equator in steps of 18: one row of 8 precedes it, NJ = 11 rows are encoded
    g = G.grid_b()
    ival, ntencode, poles = G.value_map(g)
    assert ntencode == 88 and poles == gribout.Poles()
    assert ival.tolist() == [8 + (5 - ky) * 8 + ix - 1 for ix, ky in zip(g["ixlg"], g["kxlt"])]
    assert ival.min() >= 8 and ival.max() < 48
    # CLDOMAIN = 'm': no offset, NTENCODE = NGY NGX
    ival_m, nt_m, _ = gribout.value_map(g["nlonrgg"], g["ixlg"], g["kxlt"], 5, 0, 72.0, 0.0, 18.0, "m", True)
    assert nt_m == 40 and (ival_m == ival - 8).all()


def test_value_map_refuses_what_does_not_fit():
    nlon = [4, 6, 8, 6, 4]
    ok = ([1, 6], [1, 2])
    gribout.value_map(nlon, *ok, 5, 1, 90.0, -90.0, 45.0)
    with pytest.raises(ValueError, match="NLONRGG must hold NGY"):
        gribout.value_map(nlon[:4], *ok, 5, 1, 90.0, -90.0, 45.0)
    with pytest.raises(ValueError, match="rows of NLONRGG differ"):
        gribout.value_map(nlon, *ok, 5, 0, 90.0, -90.0, 45.0)
    with pytest.raises(ValueError, match="IXLG outside"):
        gribout.value_map(nlon, [5, 6], [1, 2], 5, 1, 90.0, -90.0, 45.0)      # the fifth point of a row of four
    with pytest.raises(ValueError, match="KXLT outside"):
        gribout.value_map(nlon, [1, 1], [0, 6], 5, 1, 90.0, -90.0, 45.0)
    with pytest.raises(ValueError, match="does not fit"):
        gribout.value_map([8] * 5, [1], [1], 5, 0, -36.0, -108.0, 18.0)      # 7 rows lie north of the grid: 12 rows where NJ = 11
    with pytest.raises(ValueError, match="CLDOMAIN = 's'"):
        gribout.value_map(nlon, *ok, 5, 1, 90.0, -90.0, 45.0, "s")


def test_the_map_agrees_with_the_restatement_through_field():
    """value_map against the restatement, which goes through FIELD(NGX,NGY) as the reference does: a block of distinct numbers lands where the map says."""
    c = G.cached_cases()
    for g in (c["grid_a"], c["grid_b"]):
        ival, ntencode, poles = G.value_map(g)
        npts = g["ixlg"].size
        blk = np.arange(1.0, npts + 1.0)[None, :]
        v, _ = G.encode(blk, dict(g, lpadpoles=False), np.float64, False)
        assert v.shape == (1, ntencode) and np.unique(ival).size == npts
        assert np.array_equal(v[0, ival], blk[0]) and (np.delete(v[0], ival) == G.ZMISS).all()
    ga = c["grid_a"]
    _, _, poles = G.value_map(ga)
    assert (poles.north, poles.south) == (gribout.Pole(0, 6, 6, 12), gribout.Pole(286, 6, 274, 12))
    ky = ga["kxlt"]
    assert not (ky == 2).any() and 0 < (ky == 12).sum() < 12 and (ky == 1).any() and (ky == 13).any() and 190 <= ky.size <= 215 and ky.size % 64 != 0


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_restatement_against_the_reference(prec):
    """All recorded cases: the pattern of ZMISS exactly, the values within the figures the tool recorded, the path without logarithm bit for bit."""
    gold, obs = G.load_golden(), G.observed()
    T = np.float32 if prec == "sp" else np.float64
    for name in G.NAMES:
        ref = gold[f"{name}_{prec}"]
        got, ppmax = G.restate(name, prec)
        assert ref.dtype == T and got.dtype == T and got.shape == ref.shape, name
        if name == "C":
            assert got.tobytes() == ref.tobytes()
            continue
        same, err = G.log_error(got, ref)
        rec = obs["per_case"][name][f"restatement_vs_reference_{prec}"]
        perr = float(np.abs(ppmax.astype(np.float64) - gold[f"{name}_ppmax_{prec}"]).max())
        print(f"{name} {prec}: restatement against the reference {err:.3e} (recorded {rec['values']:.3e}), PPMAX {perr:.3e} (recorded {rec['ppmax']:.3e})")
        assert same, f"{name}: the patterns of ZMISS differ"
        assert err <= rec["values"] and perr <= rec["ppmax"]


def test_the_fixtures_hold_what_the_cases_claim():
    gold, c = G.load_golden(), G.cached_cases()
    f = G.recorded_fields()
    assert len(f) == 48 and gold["A_ice0_dp"].shape == (48, 292) and gold["B_dp"].shape == (4, 88) and gold["C_dp"].shape == (7, 292)
    for k, v in c.items():
        if not k.startswith("grid"):
            assert (v == v.astype(np.float32)).all(), k
    assert 0.05 < (c["cic_a"] > 0.3).mean() < 0.15
    for prec in ("dp", "sp"):
        a0, a1 = gold[f"A_ice0_{prec}"], gold[f"A_ice1_{prec}"]
        miss = (a0 == G.ZMISS).sum(axis=1)
        tiny = [f.index(m * 12 + k) for k, m in G.TINY_FIELDS]
        full = [f.index(m * 12 + k) for k, m in G.FULL_FIELDS]
        sea = c["grid_a"]["ixlg"].size
        # the tiny fields: PPMAX near ZMINSPEC, and by the reference's arithmetic nothing at all goes missing, land included
        assert (miss[tiny] == 0).all() and (gold[f"A_ice0_ppmax_{prec}"][tiny] < -9.5).all()
        # the full fields lose the land, the south pole row (no contributor) and nothing else: sea points on a pole row are overwritten
        _, _, poles = G.value_map(c["grid_a"])
        w = np.zeros(292, bool)
        w[G.value_map(c["grid_a"])[0]] = True
        w[:6] = True
        w[286:] = False
        assert ((a0[full] == G.ZMISS) == ~w[None, :]).all()
        assert ((miss > 292 - sea + 20) & (miss < 292)).any()      # fields that lose a tail to the threshold
        # the pole rows: one number per field; the south one is missing wherever the threshold left nothing ... or ZMINSPEC-like in a tiny field
        assert (a0[:, :6] == a0[:, :1]).all() and (a0[:, 286:] == a0[:, 286:287]).all()
        assert not np.array_equal(a0 == G.ZMISS, a1 == G.ZMISS)      # the ice mask changes what is kept
        b = gold[f"B_{prec}"]
        pre = np.concatenate([b[:, :8], b[:, 48:]], axis=1)      # the cells outside the grid: ZMISS from the prefill, or -- in a field without energy -- ZMINSPEC
        assert ((pre == G.ZMISS).all(axis=1) | (pre < -9.5).all(axis=1)).all() and (pre == G.ZMISS).all(axis=1).sum() >= 2
        assert ((b[:, 8:48] != G.ZMISS) & (b[:, 8:48] > -9.0)).any()
        cc = gold[f"C_{prec}"]
        assert (cc[2, :6] == G.ZMISS).all() and (cc[0, :6] != G.ZMISS).all() and (cc[:, 286:] == G.ZMISS).all()
    obs = G.observed()
    assert obs["restatement_vs_reference_dp"]["values"] < 1e-13 and 4 * obs["reference_sp_vs_dp"]["values"] < G.OPTS["ppresol"] / 100


def test_no_value_lies_near_the_threshold():
    """On the double precision fixture and on the restatement over all 300 fields, both values of the ice flag: |value - PPMIN| >= MARGIN."""
    gold = G.load_golden()
    for name in ("A_ice0", "A_ice1", "B"):
        v, pm = gold[f"{name}_dp"], gold[f"{name}_ppmax_dp"]
        assert (np.abs(np.where(v != G.ZMISS, v, 1e9) - G.ppmin_of(pm, np.float64)[:, None]) >= G.MARGIN).all(), name
        v, pm = G.restate(name, "dp", fields=list(range(300)))
        assert v.shape[0] == 300 and (np.abs(np.where(v != G.ZMISS, v, 1e9) - G.ppmin_of(pm, np.float64)[:, None]) >= G.MARGIN).all(), name
        s, _ = G.restate(name, "sp", fields=list(range(300)))
        assert np.array_equal(s == G.ZMISS, v == G.ZMISS), name      # and both precisions decide alike everywhere
