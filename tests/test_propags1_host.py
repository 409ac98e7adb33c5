"""The dual rotated-quadrant propagation scheme (IPROPAGS = 1) without a GPU: the interface the library exports (include/ecwam_hipx_propags1.h), the fixtures
tests/golden/propags1_*.npz -- what the reference's own unmodified PROPCONNECT, PROPAGS1, PROPDOT and GRADI returned behind tools/propags1_driver.F90, with the
CFL numbers its stand-in CHECKCFL recorded -- the coverage conditions on them, the numpy restatement tests/propags1_ref.py against them (THE SAME BITS, in both
precisions) and ecwam_amd.grid.rotated_tables against the recorded tables.  Nothing here comes from the device."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import propags1_ref as P1
import propags_ref as P
from ecwam_amd import grid as G
from ecwam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hipx_set_rotated": 11, "ecwam_hipx_propags1": 29}
PREC = P1.PREC


def test_the_header_and_the_bindings_declare_the_two_calls():
    with open(os.path.join(ROOT, "include", "ecwam_hipx_propags1.h")) as fh:
        hdr = fh.read()
    assert re.findall(r'^#include\s+(\S+)', hdr, re.M) == ['"ecwam_hip.h"']
    declared = re.findall(r"^int (ecwam_hipx?_\w+)\(([^;]*)\);", hdr, re.M)
    assert [d[0] for d in declared] == list(WANT)      # exactly the two, in this order
    for name, args in declared:
        assert len(args.split(",")) == WANT[name], (name, args)
    assert re.search(r"#define ECWAM_HIPX_PROPAGS1_CARTESIAN 1\s", hdr) and re.search(r"#define ECWAM_HIPX_PROPAGS1_IRREGULAR 2\s", hdr)
    assert lib.EXPORTS_X_PROPAGS1 == list(WANT) and lib.ABI_VERSION == 6
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    for name in WANT:
        assert f"NAME='{name}'" in f90, name
    from ecwam_amd import build

    assert "propags1.hip" in build.SOURCES and "propags1.hip" not in build.IMPLSCH_SOURCES      # its divisions stay correctly rounded


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the built library holds the two symbols, at ABI 6, each refuses a null context before anything else; and every
    ecwam_hipx_* symbol the library defines is in an EXPORTS_X_* list of the bindings (a subset: the next addition brings its own list)."""
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in WANT:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    d = C.c_double(0.0)
    assert h.ecwam_hipx_set_rotated(None, 1, 0, None, None, None, None, None, None, None, d) == 1
    assert h.ecwam_hip_last_error() == b"null context"
    assert h.ecwam_hipx_propags1(None, None, None, 1, 0, 0, d, d, 99, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 1, 0,
                                 0, None, None, None) == 1
    assert h.ecwam_hip_last_error() == b"null context"
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if not (shutil.which("nm") or os.path.exists(nm)):
        pytest.skip("no nm on this machine")
    out = subprocess.run([nm, "-D", "--defined-only", lib.LIBPATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = set(re.findall(r"\b(ecwam_hipx_\w+)$", out, re.M))
    known = {n for k in dir(lib) if k.startswith("EXPORTS_X_") for n in getattr(lib, k)}
    assert set(WANT) <= defined <= known, sorted(defined - known)


def test_the_refusals_of_wamintgr_need_no_device():
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=25)
    with pytest.raises(ValueError, match=re.escape("IPROPAGS = 1 needs the rotated tables of grid.rotated_tables (rotated=...)")):
        Wamintgr(cfg, None, "sp", ipropags=1)
    with pytest.raises(ValueError, match="ipropags must be 0, 1 or 2"):
        Wamintgr(cfg, None, "sp", ipropags=3)
    with pytest.raises(ValueError, match="sub-steps"):
        Wamintgr(cfg, None, "sp", ifrelfmax=5, delpro_lf=225.0, ipropags=1, rotated={})
    with pytest.raises(ValueError, match="stored"):
        Wamintgr(cfg, None, "sp", weights="stored", ipropags=1, rotated={})
    with pytest.raises(ValueError, match="one rank"):
        Wamintgr(cfg, None, "sp", nranks=2, ipropags=1, rotated={})


def test_the_fixtures_are_the_cases_of_the_issue_and_small():
    files = sorted(f for f in os.listdir(P1.GOLDEN) if f.startswith("propags1_"))
    assert files == sorted([f"propags1_{n}.npz" for n in P1.CASES] + ["propags1_observed.json"])
    for f in files:
        assert os.path.getsize(os.path.join(P1.GOLDEN, f)) <= 600_000, f
    assert P1.CASES == {
        "rot_irefra0": ("o3", 1, 1, 0, False, 900, 25), "rot_irefra1": ("o3", 1, 1, 1, False, 900, 25),
        "rot_obs_irefra0": ("o3", 1, 1, 0, True, 900, 25), "rot_obs_irefra1": ("o3", 1, 1, 1, True, 900, 25),
        "rot_cfl_irefra0": ("o3", 1, 1, 0, False, 40000, 25), "rot_hilat_irefra0": ("o5", 1, 1, 0, False, 900, 13),
        "sec4_irefra3": ("o3", 1, 1, 3, False, 900, 25), "cart_irefra1": ("o3", 2, 1, 1, False, 900, 25), "cart_irefra3": ("o3", 2, 1, 3, False, 900, 25)}
    assert (P1.NANG, P1.NFRE) == (12, 36)
    assert P1.fixture_grid("o3").nsea == 61 and P1.fixture_grid("o5").nsea == 117


@pytest.mark.parametrize("name", list(P1.CASES))
def test_coverage_and_the_restatement_bit_for_bit(name):
    """The coverage conditions on the committed file (propags1_ref asserts them), and the restatement against it: F3 and the CFL numbers, the same bits in
    single and in double precision."""
    fx = P1.load_fixture(name)
    key, icase, irgg, irefra, with_obs, idelpro, nr = P1.CASES[name]
    g = P1.fixture_grid(key)
    assert set(fx) == {f"{k}_{p}" for p in PREC for k in P1.TABLES + ("f3", "cfl", "ncall")}
    seen = P1.observed()
    for p, T in PREC.items():
        assert all(fx[f"{k}_{p}"].dtype == T for k in ("f3", "cfl", "wlat", "wrlat", "wrlon", "cdr", "sdr", "prqrt", "sqrt2"))
        assert fx[f"f3_{p}"].shape == (g.nsea, P1.NANG, nr) and fx[f"cfl_{p}"].shape == (g.nsea, P1.NANG, P1.NCFL)
        assert int(fx[f"ncall_{p}"][0]) == (P1.NANG if icase == 1 else 0)
        tab = {k: fx[f"{k}_{p}"] for k in P1.TABLES}
        cov = P1.table_coverage(key, tab, g.nsea)
        want = {k: v for k, v in seen["grid"][key][p].items() if k in cov}
        assert json.loads(json.dumps(cov)) == want
        c = P1.make_case(name, T)
        mine = P1.restate(c, T, P1.recorded_rot(fx, p))
        assert P1.same_bits(mine["f3"], fx[f"f3_{p}"]), (name, p, "f3")
        assert P1.same_bits(mine["cfl"], fx[f"cfl_{p}"]), (name, p, "cfl")
    other = P1.load_fixture(P1.UNOBSTRUCTED[name]) if name in P1.UNOBSTRUCTED else None
    obs = P1.case_coverage(name, fx, other)
    rec = seen["cases"][name]
    assert {k: rec[k] for k in obs} == json.loads(json.dumps(obs))
    assert all(all(v.values()) for v in rec["bit_identical"].values())


@pytest.mark.parametrize("key", ["o3", "o5"])
@pytest.mark.parametrize("p", list(PREC))
def test_rotated_tables_against_the_reference(key, p):
    """KRLAT, KRLON, WRLAT and WRLON exactly.  CDR, SDR, PRQRT and SQRT2 hold SIN and ATAN2: within twice the distance the tool observed (at least one unit
    in the last place), the signs of CDR and SDR equal everywhere.  (KLAT and KLON are build_grid's: PROPCONNECT's differ from them in the few ties that the
    increments rounded to single precision break the other way, which propags1_observed.json counts; PROPAGS1 ran with build_grid's.)"""
    T = PREC[p]
    name = next(n for n, c in P1.CASES.items() if c[0] == key)
    fx = P1.load_fixture(name)
    g = P1.fixture_grid(key)
    t = P.tables_of(T)
    mine = G.rotated_tables(P1.rounded_grid(g), T, np.asarray(t.SINTH, T), np.asarray(t.COSTH, T))
    for k in ("krlat", "krlon", "wrlat", "wrlon"):
        assert P1.same_bits(np.ascontiguousarray(mine[k]), fx[f"{k}_{p}"]), k
    seen = P1.observed()
    for k in ("cdr", "sdr", "prqrt", "sqrt2"):
        a, b = np.atleast_1d(np.asarray(mine[k], T)), np.atleast_1d(fx[f"{k}_{p}"])
        cap = max(1, 2 * int(seen["tables_ulp"][k]))
        assert P1.ulps(a, b) <= cap, (k, P1.ulps(a, b), cap)
        if k in ("cdr", "sdr"):
            assert np.array_equal(a < 0, b < 0) and np.array_equal(np.signbit(a), np.signbit(b)), k
    differ = {k: int((fx[f"{k}_{p}"] != getattr(g, k)).sum()) for k in ("klat", "klon")}
    assert differ == seen["grid"][key][p]["entries_differing_from_input"]


def test_rotated_tables_build_in_seconds_at_o48():
    import time

    g = G.build_grid(48)
    t = P.tables_of(np.float32, nang=36)
    t0 = time.perf_counter()
    r = G.rotated_tables(g, np.float32, t.SINTH, t.COSTH)
    assert time.perf_counter() - t0 < 5.0
    assert r["krlat"].shape == (g.nsea, 2, 2) and r["cdr"].shape == (g.nsea + 1, 36) and np.all(r["cdr"][g.nsea] == 0)
    assert r["krlat"].max() <= g.nland and r["krlon"].min() >= 0


@pytest.mark.parametrize("name", list(P1.PROPAGS0))
def test_sections_1_2_4_against_the_ipropags0_fixtures(name):
    """Sections 1 and 2 are PROPAGS: the bits of the committed propags_cart_* fixtures.  Section 4 differs in the form of DP1 / DP2 alone: the number of
    differing bins is recorded (propags1_observed.json), not required to be non-zero."""
    fx, f0 = P1.load_fixture(name), P.load_fixture(P1.PROPAGS0[name])
    rec = P1.observed()["cases"][name]["bins_differing_from_ipropags0"]
    for p in PREC:
        differing = int((fx[f"f3_{p}"] != f0[f"f3_{p}"]).sum())
        assert differing == rec[p]
        if name.startswith("cart_"):
            assert P1.same_bits(fx[f"f3_{p}"], f0[f"f3_{p}"]) and P1.same_bits(fx[f"cfl_{p}"], f0[f"cfl_{p}"])


def test_the_tool_reproduces_the_fixtures(tmp_path):
    """Where a reference tree exists: the driver builds around the unmodified routines and the recorded files reproduce."""
    sys.path.insert(0, ROOT)
    from oracle import ref_build

    ref = ref_build.reference_root()
    if ref is None:
        pytest.skip("no reference tree on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_propags1.py"), ref, str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    committed = sorted(f for f in os.listdir(P1.GOLDEN) if f.startswith("propags1_"))
    assert sorted(os.listdir(tmp_path)) == committed
    for f in committed:
        new, old = os.path.join(tmp_path, f), os.path.join(P1.GOLDEN, f)
        if f.endswith(".json"):
            with open(new) as a, open(old) as b:
                assert json.load(a) == json.load(b), f
        else:
            with np.load(new) as z, np.load(old) as g:
                assert sorted(z.files) == sorted(g.files), f
                for k in z.files:
                    assert z[k].dtype == g[k].dtype and z[k].shape == g[k].shape and z[k].tobytes() == g[k].tobytes(), (f, k)
