"""The warm start without a GPU: the interface the library exports (include/ecwam_hip_gribin.h), the numpy restatement of GETSPEC's GRIB read
(tests/gribin_ref.py) against flang's evaluation of the same statements (tests/golden/gribin_0.npz, recorded by tools/make_golden_gribin.py), in
both precisions, the map of the read (ecwam_amd/gribout.py::read_map) against the restatement, which goes through FIELD, and the untransposed
restart record (ecwam_amd/restart.py::read_record).  The figures are read from tests/golden/gribin_observed.json -- nothing there comes from
the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gribin_ref as R
import gribout_ref as G
from ecwam_amd import gribout, lib, restart

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hip_getspec_values": 11, "ecwam_hip_getspec_unpack": 11}


def test_the_lists_and_the_header():
    assert lib.EXPORTS_GRIBIN == list(WANT)
    assert (lib.GETSPEC_UNSCALE, lib.GETSPEC_MISSING) == (1, 2)
    assert len(lib.EXPORTS) == 72 and len(lib.EXPORTS_START) == 4 and len(lib.EXPORTS_FORCING) == 7 and len(lib.EXPORTS_GRIBOUT) == 4 and lib.ABI_VERSION == 6
    assert not set(WANT) & (set(lib.EXPORTS) | set(lib.EXPORTS_START) | set(lib.EXPORTS_FORCING) | set(lib.EXPORTS_GRIBOUT))
    with open(os.path.join(ROOT, "include", "ecwam_hip_gribin.h")) as fh:
        hdr = fh.read()
    assert '#include "ecwam_hip_gribout.h"' in hdr
    assert re.findall(r"^int (ecwam_hip_\w+)\(", hdr, re.M) == list(WANT)      # exactly these, in this order
    for name, nargs in WANT.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    assert re.search(r"#define ECWAM_HIP_GETSPEC_UNSCALE 1\b", hdr) and re.search(r"#define ECWAM_HIP_GETSPEC_MISSING 2\b", hdr)
    for other in ("ecwam_hip.h", "ecwam_hip_start.h", "ecwam_hip_forcing.h", "ecwam_hip_gribout.h"):
        with open(os.path.join(ROOT, "include", other)) as fh:
            text = fh.read()
        assert not set(WANT) & set(re.findall(r"\b(ecwam_hip_\w+)\b", text)), other
        assert other != "ecwam_hip.h" or re.search(r"#define ECWAM_HIP_ABI_VERSION 6\b", text)
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    for name in WANT:
        assert f"NAME='{name}'" in f90, name


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the built library exports both calls, and both refuse a null context before anything else."""
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in WANT:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    ll = C.c_longlong(1)
    for name in WANT:
        assert getattr(h, name)(None, 0, 0, None, ll, 0, 1, 0, None, None, None) == 1 and h.ecwam_hip_last_error() == b"null context", name


def test_the_flags_are_those_of_the_header(tmp_path):
    src = ('#include "ecwam_hip_gribin.h"\n#include <stdio.h>\nint main(){printf("%d %d %zu", ECWAM_HIP_GETSPEC_UNSCALE, ECWAM_HIP_GETSPEC_MISSING, '
           'sizeof(ecwam_hip_grib_opts));return 0;}')
    exe = str(tmp_path / "gribin_flags")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got == [lib.GETSPEC_UNSCALE, lib.GETSPEC_MISSING, C.sizeof(lib.GribOpts)]


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_restatement_against_the_reference(prec):
    """All recorded cases: the elements from missing values are EPSMIN exactly, the rest within the figures the tool recorded."""
    gold, obs = R.load_golden(), R.observed()
    T = np.float32 if prec == "sp" else np.float64
    eps = T(G.tables(prec).EPSMIN)
    for name in R.NAMES:
        ref = gold[f"{name}_{prec}"]
        got = R.restate(name, prec)
        assert ref.dtype == T and got.dtype == T and got.shape == ref.shape == (len(R.fields_of(name)), R.grid_of(name)["ixlg"].size), name
        miss = R.from_missing(R.inputs(name), R.grid_of(name))
        assert np.array_equal(got == eps, miss) and np.array_equal(ref == eps, miss), name
        err = R.rel_error(got, ref)
        rec = obs["per_case"][name][f"restatement_vs_reference_{prec}"]
        print(f"{name} {prec}: restatement against the reference {err:.3e} (recorded {rec:.3e})")
        assert err <= rec <= obs[f"restatement_vs_reference_{prec}"]


def test_the_fixtures_hold_what_the_cases_claim():
    gold, obs = R.load_golden(), R.observed()
    assert sorted(gold) == sorted(f"{n}_{p}" for n in R.NAMES for p in ("dp", "sp"))
    assert gold["A_ice0_dp"].shape == (48, 204) and gold["B_dp"].shape == (4, G.cached_cases()["grid_b"]["ixlg"].size)
    for name in R.NAMES:
        v = R.inputs(name)
        miss = R.from_missing(v, R.grid_of(name))
        assert 0 < miss.sum() < miss.size, name                                  # missing and kept values in every case
        kept = gold[f"{name}_dp"][~miss]
        assert (kept > -2 * R.PPEPS).all() and kept.max() > 1e-3, name           # un-scaled: spectral densities again, down to rounding about zero
        assert np.array_equal(gold[f"{name}_sp"].astype(np.float64) == float(np.float32(G.tables("sp").EPSMIN)), miss), name
    a = gold["A_ice0_dp"]
    ky = G.cached_cases()["grid_a"]["kxlt"]
    assert (a[:, ky == 13] == a[:, ky == 13][:, :1]).all() and (a[:, ky == 1] == a[:, ky == 1][:, :1]).all()      # the pole rows read their mean back
    # the gates that follow from the figures are matters of rounding
    assert R.gate("dp", obs) == 4 * np.finfo(np.float64).eps and obs["restatement_vs_reference_dp"] < np.finfo(np.float64).eps
    assert np.finfo(np.float32).eps / 2 < obs["reference_sp_vs_dp"] < 2 * np.finfo(np.float32).eps and R.gate("sp", obs) == 4 * obs["reference_sp_vs_dp"]
    assert max(os.path.getsize(os.path.join(R.GOLDEN, f)) for f in os.listdir(R.GOLDEN) if f.startswith("gribin_")) <= 600_000


def test_read_map_agrees_with_the_restatement_through_field():
    """A vector of distinct numbers, gathered through FIELD as the reference goes, is the vector indexed by read_map; on the reduced grid the map
    of the read is the output map, on the regular grid of B (ICOUNT = 9) it is the output map less the start offset."""
    c = G.cached_cases()
    for g in (c["grid_a"], c["grid_b"]):
        ival, nval = R.read_map(g)
        assert nval == int(np.sum(g["nlonrgg"])) and ival.dtype == np.int32 and np.unique(ival).size == g["ixlg"].size
        v = np.arange(1.0, nval + 1.0)[None, :]
        assert np.array_equal(R.gather(v, g)[0], v[0, ival])
    assert np.array_equal(R.read_map(c["grid_a"])[0], G.value_map(c["grid_a"])[0])
    assert np.array_equal(R.read_map(c["grid_b"])[0], G.value_map(c["grid_b"])[0] - 8) and R.read_map(c["grid_b"])[1] == 40
    # hand-written: NLONRGG = 4 6 8 6 4 south to north, rows of FIELD start at 0, 4, 10, 18, 24
    ival, nval = gribout.read_map([4, 6, 8, 6, 4], [1, 3, 2, 6, 1, 8, 5, 4, 2], [1, 1, 2, 2, 3, 3, 4, 5, 5], 5)
    assert nval == 28 and ival.tolist() == [24, 26, 19, 23, 10, 17, 8, 3, 1]
    with pytest.raises(ValueError, match="IXLG outside"):
        gribout.read_map([4, 6, 8, 6, 4], [5], [1], 5)
    with pytest.raises(ValueError, match="KXLT outside"):
        gribout.read_map([4, 6, 8, 6, 4], [1], [6], 5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_read_record_transposed_is_read_fl(dtype, tmp_path, monkeypatch):
    rng = np.random.default_rng(7)
    n, nang, nfre = 37, 12, 36
    a = rng.standard_normal((n, nang, nfre)).astype(dtype)
    b = rng.standard_normal((n, nang, nfre)).astype(dtype)
    path = str(tmp_path / "fl.bin")
    restart.write_fl(path, a)
    restart.write_fl(path, b, append=True)
    for rec, x in ((0, a), (1, b)):
        flat = restart.read_record(path, rec, dtype)
        assert flat.ndim == 1 and flat.dtype == dtype and flat.size == x.size
        back = np.ascontiguousarray(flat.reshape(nfre, nang, n).transpose(2, 1, 0))
        want = restart.read_fl(path, n, nang, nfre, dtype, rec)
        assert back.tobytes() == want.tobytes() == x.tobytes()
        assert restart.read_record(path, rec).dtype == np.uint8 and restart.read_record(path, rec).tobytes() == flat.tobytes()
    with pytest.raises(EOFError):
        restart.read_record(path, 2)
    # a record in sub-records (the scheme of payloads beyond 2 GiB, here with a small limit)
    monkeypatch.setattr(restart, "_MAX_SUB", 4096)
    restart.write_fl(path, a)
    assert os.path.getsize(path) > a.nbytes + 8      # more than one pair of markers
    flat = restart.read_record(path, 0, dtype)
    assert flat.tobytes() == np.ascontiguousarray(a.transpose(2, 1, 0)).tobytes()
    assert restart.read_fl(path, n, nang, nfre, dtype).tobytes() == a.tobytes()
    with open(path, "r+b") as fh:      # a tail marker that disagrees
        fh.seek(4 + 4096)
        fh.write(np.array([17], "<i4").tobytes())
    with pytest.raises(ValueError, match="corrupt record markers"):
        restart.read_record(path, 0, dtype)
