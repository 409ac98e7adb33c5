"""The stand-alone forcing without a GPU: the interface the library exports (include/ecwam_hip_readwind.h), and ecwam_amd/readwind.py with the
numpy restatement of GRIB2WGRID's arithmetic, READWIND's fill and CURRENT2WAM's statements (tests/readwind_ref.py) against the reference's own
results (tests/golden/readwind_0.npz, recorded by tools/make_golden_readwind.py from the unmodified GRIB2WGRID behind a stand-in decoder), in both
precisions.  The gates are read from tests/golden/readwind_observed.json, where the tool wrote what the reference and the restatement gave --
nothing there comes from the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import readwind_ref as F
from ecwam_amd import lib
from ecwam_amd import readwind as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hip_set_input_grid": 8, "ecwam_hip_grib2wgrid": 14, "ecwam_hip_current2wam": 11}


def _headers():
    inc = os.path.join(ROOT, "include")
    out = {}
    for name in sorted(os.listdir(inc)):
        with open(os.path.join(inc, name)) as fh:
            out[name] = fh.read()
    return out


def test_the_header_and_the_bindings_declare_the_three_calls():
    hdrs = _headers()
    hdr = hdrs["ecwam_hip_readwind.h"]
    assert '#include "ecwam_hip_forcing.h"' in hdr and "ECWAM_HIP_ABI_VERSION" in hdr
    declared = re.findall(r"^int (ecwam_hip_\w+)\(([^;]*)\);", hdr, re.M)
    assert [d[0] for d in declared] == list(WANT)      # exactly the three, in this order
    for name, args in declared:
        assert len(args.split(",")) == WANT[name], (name, args)
    for other, text in hdrs.items():      # none of the three is declared, or spoken of, in another header
        if other != "ecwam_hip_readwind.h":
            assert not set(WANT) & set(re.findall(r"\becwam_hip_\w+", text)), other
    assert lib.EXPORTS_READWIND == list(WANT)
    assert (len(lib.EXPORTS), len(lib.EXPORTS_START), len(lib.EXPORTS_FORCING), len(lib.EXPORTS_GRIBOUT), len(lib.EXPORTS_GRIBIN),
            len(lib.EXPORTS_INTAKE)) == (72, 4, 7, 4, 2, 5)
    assert lib.ABI_VERSION == 6
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    for name in WANT:
        assert f"NAME='{name}'" in f90, name
    for k, v in (("G2W_NSLOT", 4), ("G2W_MAXFLD", 16), ("G2W_FIELD", "(-1)"), ("G2W_DIRFLD", 1), ("G2W_NONWAVE", 2)):
        assert re.search(rf"#define ECWAM_HIP_{k} {re.escape(str(v))}(\s|$)", hdr), k
    assert (lib.G2W_NSLOT, lib.G2W_MAXFLD, lib.G2W_FIELD, lib.G2W_DIRFLD, lib.G2W_NONWAVE) == (4, 16, -1, 1, 2) == (4, 16, F.FIELD, F.DIRFLD, F.NONWAVE)
    assert C.sizeof(lib.G2wField) == 8 and lib.FG_PLANES == list(F.FG) and set(lib.G2W_PLANES) == {p for p, *_ in F.READWIND}
    from ecwam_amd import build
    assert "readwind.hip" in build.SOURCES


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the built library holds the three symbols, at ABI 6, and each refuses a null context before anything else."""
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in WANT:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    d = C.c_double(0.0)
    calls = (lambda: h.ecwam_hip_set_input_grid(None, 9, -1, 0, None, None, None, 0),
             lambda: h.ecwam_hip_grib2wgrid(None, 9, None, 0, 0, None, d, d, d, None, 0, None, 0, None),
             lambda: h.ecwam_hip_current2wam(None, 1, 0, None, None, d, d, None, None, None, None))
    assert len(calls) == len(WANT)
    for call in calls:
        assert call() == 1 and h.ecwam_hip_last_error() == b"null context"


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", F.CASES)
def test_restatement_against_the_reference(name, prec):
    """input_grid -> cell_table -> interpolate, READWIND's fill and CURRENT2WAM's statements against the reference: the pattern of PMISS exact;
    the same bits wherever the recorder observed 0, otherwise within 10 x the recorded figure; directions on the circle."""
    own, _, _ = F.chain(prec, name)
    ref = F.golden_case(name, prec)
    T = F.dtype_of(prec)
    bad = {}
    for (key, mine), (_, theirs) in zip(F.fixture_items(name, own), F.fixture_items(name, ref)):
        assert mine.dtype == theirs.dtype == T
        assert F.same_pattern(mine, theirs), (name, key)
        gate = F.host_gate(name, key, prec)
        err = F.error(key, mine, theirs)
        print(f"{name} {key} {prec}: restatement against the reference {err:.3e} (gate {'the same bits' if gate is None else format(gate, '.3e')})")
        if gate is None:
            if mine.tobytes() != theirs.tobytes():
                bad[key] = err
        elif not err <= gate:
            bad[key] = (err, gate)
    assert not bad, bad
    # what READWIND leaves alone: the planes no message targets and the cells of kind 0
    assert np.array_equal(own["fieldg"] == T(F.SENT), ref["fieldg"] == T(F.SENT))
    for comp in ("ucur", "vcur"):
        assert own["field_" + comp].tobytes() == ref["field_" + comp].tobytes() or F.host_gate(name, comp, prec) is not None


def test_the_messages_carry_what_the_reference_read():
    g = F.load_golden()
    for name in F.CASES:
        for key, param, wave, flags, _ in F.messages(F.cached_cases(), name):
            iparam, iforp, cdate, kzlev = (int(x) for x in g[f"meta_{key}_{name}"])
            assert (iparam, iforp, cdate, kzlev) == (param % 1000, 21600, 20261020180000, 0), (name, key)      # 12 UTC + 6 h
            assert bool(flags & F.DIRFLD) == (iparam == 249 and wave) == RW.dirfld(iparam, wave)
    assert RW.dirfld(230, True) and not RW.dirfld(249, False) and not RW.dirfld(245, True)


def test_the_cases_cover_what_they_claim():
    """Recomputed from the inputs: every branch of GRIB2WGRID's loop is taken by a cell, in the cases that are meant to take it."""
    c, obs = F.cached_cases(), F.observed()
    assert np.unique(c["map_in"]).size == F.NROW and c["map_in"].max() < F.NCELL and F.NCELL % 64 != 0 and F.NCELL % 4 != 0
    assert (c["ifromij"] <= F.KLONRGG[F.NY - c["jfromij"]]).all() and np.unique(F.KLONRGG).size > 3      # a reduced grid, every row inside it
    taken, cond = set(), np.inf
    for name in F.CASES:
        _, tk, cd = F.chain("dp", name)
        taken |= {f"{name}:{t}" for t in tk}
        cond = min(cond, cd)
    assert sorted(taken) == obs["branches"] and cond == obs["smallest_direction_vector"] >= 0.1
    for b in F.BRANCHES:
        assert any(t.endswith(":" + b) for t in taken), b
    has = lambda name, key, b: f"{name}:{key}:{b}" in taken
    for name in ("A", "B", "D"):      # each interpolating case takes the branches of the missing-value rule itself
        for b in ("bilinear", "nearest", "mean1", "mean2", "mean3"):
            assert any(has(name, key, b) for key in ("miss", "fg_CICOVER", "fg_AIRD", "ucur")), (name, b)
        assert has(name, "dir", "missing_wave") and has(name, "dir", "nearest") and has(name, "plain", "kind0")
    assert any(has(n, k, "mean0") for n in "ABD" for k in ("miss", "fg_CICOVER"))
    assert "A:table:wrap" in taken and "D:table:wrap" in taken and "B:table:padded" in taken and has("B", "plain", "llskip")
    assert not any(t.startswith("C:") and t.split(":")[2] not in ("copy", "kind0") for t in taken)
    # the rows of the currents read cells of kind 1 (FIELD = ZMISS), values below WLOWEST and above CURRENT_MAX
    for name in F.CASES:
        tab = F.table(name, "dp")[1]
        f = F.golden_case(name, "dp")["field_ucur"][c["map_in"]]
        assert (tab["kind"][c["map_in"]] == 1).any() == tab["interpol"] and (f == F.PMISS).any()
        assert (np.abs(f) <= F.WLOWEST).any() and (np.abs(f) > F.CURRENT_MAX).any() and ((np.abs(f) > F.WLOWEST) & (np.abs(f) < F.CURRENT_MAX)).any()


def test_input_grid_reproduces_the_geometry():
    want = {"A": dict(llinterpol=True, itop=0, ibot=0, iperiodic=1, llscanns=True, nr=8, nc=20),
            "B": dict(llinterpol=True, itop=4, ibot=4, iperiodic=0, llscanns=True, nr=6, nc=9),
            "C": dict(llinterpol=False, itop=0, ibot=0, iperiodic=1, llscanns=True, nr=9, nc=11),
            "D": dict(llinterpol=True, itop=0, ibot=0, iperiodic=1, llscanns=False, nr=8, nc=20)}
    for name, w in want.items():
        for prec in ("dp", "sp"):
            for wave in (False, True):
                grid, tab = F.table(name, prec, wave)
                assert {k: grid[k] for k in w} == w, (name, prec, wave)
                assert grid["llnonwave"] == (not wave) and grid["wave_stream"] == wave
                assert tab["pos"].shape == (F.NCELL, 4) and tab["pos"].max() < grid["nvalues"] == F.cached_cases()[name]["nvalues"]
                assert tab["interpol"] == w["llinterpol"]
    # A and D hold the same numbers in the other order: the positions differ, the weights do not
    a, d = F.table("A", "dp")[1], F.table("D", "dp")[1]
    assert np.array_equal(a["w"], d["w"]) and np.array_equal(a["kind"], d["kind"]) and not np.array_equal(a["pos"], d["pos"])
    b = F.table("B", "dp")[1]
    go = b["kind"] == 2
    assert (b["pos"][go, 0] == b["pos"][go, 1]).any() and b["ii1_clamped"].any()      # II1 = II at the eastern edge
    assert (b["pos"][go] == -1).all(axis=1).any() and b["llskip"].sum() > 4
    c = F.table("C", "dp")[1]
    assert c["w"] is None and np.array_equal(np.sort(c["pos"][c["kind"] == 2, 0]), np.arange(int(F.KLONRGG.sum())))
    assert set(np.unique(a["kind"])) == {0, 1, 2} and (a["kind"] == 1).sum() == len(F.NO_VALUE)


def test_input_grid_refuses_what_the_reference_and_the_device_do_not_serve():
    c = F.cached_cases()
    args = (c["xlon"], c["ylat"], F.KLONRGG, F.NY, 1, F.NX, 1, F.NY, F.PMISS)
    keys = F.message_keys(c, "B", 167, False)
    with pytest.raises(ValueError, match="THE MODEL DOMAIN IS OUTSIDE THE INPUT DOMAIN"):      # grib2wgrid.F90:631-651
        RW.input_grid(dict(keys, latitudeOfFirstGridPointInDegrees=-75.0, latitudeOfLastGridPointInDegrees=-89.0), *args)
    with pytest.raises(ValueError, match="THE MODEL DOMAIN IS OUTSIDE THE INPUT DOMAIN"):
        RW.input_grid(dict(keys, latitudeOfFirstGridPointInDegrees=89.0, latitudeOfLastGridPointInDegrees=75.0), *args)
    with pytest.raises(ValueError, match="LLOCEAN"):
        RW.input_grid(dict(keys, editionNumber=1, localDefinitionNumber=4, stream=1045), *args)
    with pytest.raises(ValueError, match="unstructured"):
        RW.input_grid(keys, *args, llunstr=True)
    with pytest.raises(ValueError, match="251"):
        RW.input_grid(F.message_keys(c, "A", 140251, True), *args)
    with pytest.raises(ValueError, match="SCANNING MODE"):
        RW.input_grid(dict(keys, jScansPositively=2), *args)
    with pytest.raises(ValueError, match="GRID TYPE"):
        RW.input_grid(dict(keys, gridType="sh"), *args)
    # a message scanned south to north on rows that are not symmetric: the reference reads values it never filled
    keys = dict(F.message_keys(c, "D", 167, False), pl=np.array([8, 12, 16, 20, 20, 16, 12, 10]))
    with pytest.raises(ValueError, match="not symmetric"):
        RW.cell_table(RW.input_grid(keys, *args), *args)
