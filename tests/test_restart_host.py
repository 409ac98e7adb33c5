"""The start and the end of a run without a GPU: the interface the library exports (include/ecwam_hip_restart.h), the numpy restatement of
BUILDSTRESS (tests/restart_ref.py) against the reference's own results (tests/golden/restart_0.npz, recorded by tools/make_golden_restart.py from the
unmodified CDUSTARZ0, CHNKMIN, WRITEFL, WRITESTRESS and READSTRESS), and ecwam_amd/restart.py against the bytes of the files the reference wrote.
The gates are read from tests/golden/restart_observed.json, where the tool wrote what the reference and the restatement gave -- nothing there comes
from the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import restart_ref as F
from ecwam_amd import lib
from ecwam_amd import restart as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hip_depthprpt": 11, "ecwam_hip_buildstress": 11, "ecwam_hip_set_restart_map": 3, "ecwam_hip_savstress_pack": 10, "ecwam_hip_getstress_unpack": 10,
        "ecwam_hip_savspec_pack": 10}


def _headers():
    inc = os.path.join(ROOT, "include")
    out = {}
    for name in sorted(os.listdir(inc)):
        with open(os.path.join(inc, name)) as fh:
            out[name] = fh.read()
    return out


def test_the_header_and_the_bindings_declare_the_six_calls():
    hdrs = _headers()
    hdr = hdrs["ecwam_hip_restart.h"]
    assert '#include "ecwam_hip_forcing.h"' in hdr and "ECWAM_HIP_ABI_VERSION" in hdr
    declared = re.findall(r"^int (ecwam_hip_\w+)\(([^;]*)\);", hdr, re.M)
    assert [d[0] for d in declared] == list(WANT)      # exactly the six, in this order
    for name, args in declared:
        assert len(args.split(",")) == WANT[name], (name, args)
    for other, text in hdrs.items():      # none of the six is declared, or spoken of, in another header
        if other != "ecwam_hip_restart.h":
            assert not set(WANT) & set(re.findall(r"\becwam_hip_\w+", text)), other
    # and this header speaks of no entry point of another one
    others = set(lib.EXPORTS[1:] + lib.EXPORTS_START + lib.EXPORTS_FORCING + lib.EXPORTS_GRIBOUT + lib.EXPORTS_GRIBIN + lib.EXPORTS_INTAKE + lib.EXPORTS_READWIND)
    assert not others & set(re.findall(r"\becwam_hip_\w+", hdr))
    assert lib.EXPORTS_RESTART == list(WANT)
    assert (len(lib.EXPORTS), len(lib.EXPORTS_START), len(lib.EXPORTS_FORCING), len(lib.EXPORTS_GRIBOUT), len(lib.EXPORTS_GRIBIN), len(lib.EXPORTS_INTAKE),
            len(lib.EXPORTS_READWIND)) == (72, 4, 7, 4, 2, 5, 3)
    assert lib.ABI_VERSION == 6
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    for name in WANT:
        assert f"NAME='{name}'" in f90, name
    for k, v in (("BST_Z0B_ZERO", 1), ("BST_NSESTART", 2), ("NRESTART_FIELDS", 16)):
        assert re.search(rf"#define ECWAM_HIP_{k} {v}(\s|$)", hdr), k
    assert (lib.BST_Z0B_ZERO, lib.BST_NSESTART, lib.NRESTART_FIELDS) == (1, 2, 16) and lib.RESTART_FF_COLUMNS == F.RESTART_FF_COLUMNS
    assert C.sizeof(lib.DepthOpts) == 16 and R.NRESTART_FIELDS == 16
    from ecwam_amd import build
    assert "restart.hip" in build.SOURCES


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the built library holds the six symbols, at ABI 6, and each refuses a null context before anything else."""
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in WANT:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    d = C.c_double(0.0)
    calls = (lambda: h.ecwam_hip_depthprpt(None, 1, 0, None, None, None, None, None, None, None, None),
             lambda: h.ecwam_hip_buildstress(None, 1, 0, None, None, d, 99, d, d, None, None),
             lambda: h.ecwam_hip_set_restart_map(None, -1, None),
             lambda: h.ecwam_hip_savstress_pack(None, 1, 0, None, None, None, 1, None, 0, None),
             lambda: h.ecwam_hip_getstress_unpack(None, 1, 0, None, 0, 1, None, None, None, None),
             lambda: h.ecwam_hip_savspec_pack(None, 1, 0, None, -1, 0, 1, None, 0, None))
    assert len(calls) == len(WANT)
    for call in calls:
        assert call() == 1 and h.ecwam_hip_last_error() == b"null context"


@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", list(F.CASES))
def test_restatement_against_the_reference(name, prec):
    """tests/restart_ref.py::buildstress against the reference: the same branch at every point; every column within 10 x the recorded figure (a few
    units in the last place where the recorder observed 0); the columns BUILDSTRESS does not write keep their bits."""
    g = F.load_golden()
    ff, cd, br = F.buildstress(prec, name, F.cached_inputs())
    ref = g[f"ff_{name}_{prec}"]
    T = F.dtype_of(prec)
    assert ff.dtype == ref.dtype == T and ref.shape == (F.N, F.NFF)
    assert np.array_equal(br, g[f"branch_{name}"])
    err = F.rel_error(ff[:, :14], ref[:, :14])
    bad = {}
    for c, col in enumerate(F.FF_NAMES):
        gate = F.host_gate(name, col, prec)
        print(f"{name} {col} {prec}: restatement against the reference {err[c]:.3e} (gate {gate:.3e})")
        if not err[c] <= gate:
            bad[col] = (err[c], gate)
    assert not bad, bad
    written = {F.UFRIC, F.TAUW, F.TAUWDIR, F.Z0M, F.Z0B} | ({F.WSWAVE} if F.CASES[name][2] else set()) | ({F.CHRNCK} if F.CASES[name][1] or F.CASES[name][4] else set())
    inp = F.cached_inputs()["ff"].astype(T)
    for c in range(F.NFF):
        if c not in written:
            assert ref[:, c].tobytes() == inp[:, c].tobytes() == ff[:, c].tobytes(), c
    assert F.rel_error(cd[:, None], g[f"cd_{name}_{prec}"][:, None])[0] <= F.host_gate(name, "UFRIC", prec)
    assert np.array_equal(F.tauw_zero(ref, T), (g[f"branch_{name}"] & F.BR_TAUW0) != 0) or not F.CASES[name][1]


def test_the_cases_cover_what_they_claim():
    """Recomputed from the inputs and the fixture: the cases of the issue, and every branch taken and left by some point."""
    cases = set(F.CASES.values())
    assert {c[0] for c in cases} == {c[1] for c in cases} == {c[2] for c in cases} == {True, False}
    assert {c[3] for c in cases} == {10.0, 8.0} and any(c[4] for c in cases)
    obs, g, inp = F.observed(), F.load_golden(), F.cached_inputs()
    for n, (taken, left) in obs["branches"].items():
        assert left and (taken or n == "z0min"), n      # Hersbach's CD never lets Z0 down to Z0MIN at U10 >= WSPMIN: that floor is never reached
    ws = inp["ff"][:, F.WSWAVE]
    assert (ws < 1.0).any() and (ws > 1.0).any() and np.unique(inp["map_in"]).size == F.N and inp["map_in"].max() < F.NCELL
    cdp = inp["cd"][inp["map_in"]]
    assert (cdp == F.ZMISS).any() and ((cdp <= 0) & (cdp != F.ZMISS)).any() and (cdp > 0).any()
    br = g["branch_A"]
    for bit in (F.BR_UWAVE, F.BR_CD, F.BR_WSPMIN, F.BR_EPSUS, F.BR_FLOOR_Z0M, F.BR_TAUW0):
        assert (br & bit).any() and not (br & bit).all(), bit
    assert (g["ff_A_dp"][:, F.TAUW] == 0).any()      # TAUW clipped at 0
    assert obs["aki"]["bins_near_the_threshold"] == 0 and obs["aki"]["closest_ratio_distance_from_1"] > 1e-6
    assert obs["aki"]["largest_change_of_one_further_step"] < 0.5 * np.finfo(np.float32).eps
    p = F.permutation()
    assert np.array_equal(np.sort(p), np.arange(F.N)) and (p != np.arange(F.N)).sum() > F.N // 2


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_the_files_of_the_reference(prec, tmp_path):
    """write_record and write_stress reproduce the bytes WRITEFL and WRITESTRESS wrote, LL1D and relabelled; read_stress returns what READSTRESS did
    (which relabels back); read_record is the inverse of write_record."""
    g, st, T = F.load_golden(), F.restart_state(), F.dtype_of(prec)
    perm = F.permutation()
    ff, u, v = st["ff"].astype(T), st["ucur"].astype(T), st["vcur"].astype(T)
    for f, pm in (("ll1d", None), ("relab", perm)):
        path = str(tmp_path / f"BLS_{f}")
        rec = F.record_of(st["fl"].astype(T), pm)
        R.write_record(path, rec)
        with open(path, "rb") as fh:
            assert fh.read() == g[f"file_BLS_{f}_{prec}"].tobytes(), f
        assert R.read_record(path, dtype=T).tobytes() == rec.tobytes()
        if pm is None:      # and the host path that transposes writes the same file
            R.write_fl(path + "_fl", st["fl"].astype(T))
            with open(path + "_fl", "rb") as fh:
                assert fh.read() == g[f"file_BLS_{f}_{prec}"].tobytes()
        path = str(tmp_path / f"LAW_{f}")
        R.write_stress(path, F.DATES, F.rfield_of(ff, u, v, pm))
        with open(path, "rb") as fh:
            assert fh.read() == g[f"file_LAW_{f}_{prec}"].tobytes(), f
        dates, rf = R.read_stress(path, F.N, T)
        assert tuple(dates) == F.DATES
        back = rf if pm is None else rf[:, np.argsort(pm)]      # readstress.F90:120: RFIELD(IJ2NEWIJ(IJ)) = the file's IJ
        assert back.tobytes() == g[f"readstress_{f}_{prec}"].tobytes() == F.rfield_of(ff, u, v).tobytes()
    with pytest.raises(ValueError):
        R.write_stress(str(tmp_path / "x"), F.DATES[:3], F.rfield_of(ff, u, v))
    with pytest.raises(ValueError):
        R.read_stress(str(tmp_path / "LAW_ll1d"), F.N + 1, T)


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_emaxdpt_of_the_reference(prec):
    """initdpthflds.F90:61-73 as the driver recorded it: the restatement's bits (products, one division by 4), the existing fixture's from 4 m
    on, smaller below."""
    import reference_cases as RC
    d, g = RC.depthprpt_depths(), F.load_golden()
    with np.load(os.path.join(F.GOLDEN, "reference_depthprpt.npz")) as z:
        old = z[f"EMAXDPT_{prec}"]
    new = g[f"emaxdpt_{prec}"]
    assert new.tobytes() == F.emaxdpt(d, prec).tobytes()
    assert new[d >= 4].tobytes() == old[d >= 4].tobytes() and (new[d < 4] < old[d < 4]).all() and (d < 4).sum() > 3


def test_the_fixture_is_small():
    assert os.path.getsize(os.path.join(F.GOLDEN, "restart_0.npz")) <= 600_000
