"""The first-order propagation scheme (IPROPAGS = 0) without a GPU: the interface the library exports (include/ecwam_hip_propags.h), the fixtures
tests/golden/propags_*.npz -- what the reference's own unmodified PROPAGS, PROPDOT and GRADI returned behind tools/propags_driver.F90, with the CFL numbers its
stand-in CHECKCFL recorded -- the coverage conditions on them, and the numpy restatement tests/propags_ref.py against them: THE SAME BITS, in both precisions
(the routines hold only correctly rounded operations in a fixed order).  Nothing here comes from the device."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import propags_ref as P
from ecwam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hip_propags_dot": 17, "ecwam_hip_propags": 29}
PREC = {"sp": np.float32, "dp": np.float64}


def _header():
    with open(os.path.join(ROOT, "include", "ecwam_hip_propags.h")) as fh:
        return fh.read()


def test_the_header_and_the_bindings_declare_the_two_calls():
    hdr = _header()
    assert '#include "ecwam_hip.h"' in hdr
    declared = re.findall(r"^int (ecwam_hip_\w+)\(([^;]*)\);", hdr, re.M)
    assert [d[0] for d in declared] == list(WANT)      # exactly the two, in this order
    for name, args in declared:
        assert len(args.split(",")) == WANT[name], (name, args)
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):      # neither is declared, or spoken of, in another header
        if other != "ecwam_hip_propags.h":
            with open(os.path.join(inc, other)) as fh:
                assert not set(WANT) & set(re.findall(r"\becwam_hip_\w+", fh.read())), other
    assert lib.EXPORTS_PROPAGS == list(WANT) and lib.ABI_VERSION == 6
    before = (lib.EXPORTS + lib.EXPORTS_START + lib.EXPORTS_FORCING + lib.EXPORTS_GRIBOUT + lib.EXPORTS_GRIBIN + lib.EXPORTS_INTAKE + lib.EXPORTS_READWIND
              + lib.EXPORTS_RESTART)
    assert not set(WANT) & set(before)
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    for name in WANT:
        assert f"NAME='{name}'" in f90, name
    assert re.search(r"#define ECWAM_HIP_PROPAGS_CARTESIAN 1\s", hdr) and re.search(r"#define ECWAM_HIP_PROPAGS_IRREGULAR 2\s", hdr)
    assert (lib.PROPAGS_CARTESIAN, lib.PROPAGS_IRREGULAR, lib.PROPAGS_NCFL) == (1, 2, P.NCFL)
    assert lib.propags_dot_width(12) == P.dot_width(12) == 40 and "(3 * (nang) + 4)" in hdr
    from ecwam_amd import build

    assert "propags.hip" in build.SOURCES and "propags.hip" not in build.IMPLSCH_SOURCES      # its divisions stay correctly rounded


def test_the_library_exports_the_entry_points_and_only_those_are_new():
    """Fails without the feature: the built library holds the two symbols, at ABI 6, each refuses a null context before anything else; and every
    ecwam_hip_* symbol the library defines is in one of the lists of the bindings."""
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in WANT:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    d = C.c_double(0.0)
    assert h.ecwam_hip_propags_dot(None, 1, 0, 7, None, None, d, None, None, None, None, None, None, None, None, None, None) == 1
    assert h.ecwam_hip_last_error() == b"null context"
    assert h.ecwam_hip_propags(None, None, None, 1, 0, 0, d, d, 99, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 1, 0, 0,
                               None, None, None) == 1
    assert h.ecwam_hip_last_error() == b"null context"
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if not (shutil.which("nm") or os.path.exists(nm)):
        pytest.skip("no nm on this machine")
    out = subprocess.run([nm, "-D", "--defined-only", lib.LIBPATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = set(re.findall(r"\b(ecwam_hip_\w+)$", out, re.M))
    known = set(lib.EXPORTS + lib.EXPORTS_START + lib.EXPORTS_FORCING + lib.EXPORTS_GRIBOUT + lib.EXPORTS_GRIBIN + lib.EXPORTS_INTAKE + lib.EXPORTS_READWIND
                + lib.EXPORTS_RESTART)
    assert defined - known == set(WANT), sorted(defined - known)


def test_the_refusals_of_wamintgr_need_no_device():
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=25)
    with pytest.raises(ValueError, match="sub-steps"):
        Wamintgr(cfg, None, "sp", ifrelfmax=5, delpro_lf=225.0, ipropags=0)
    with pytest.raises(ValueError, match="stored"):
        Wamintgr(cfg, None, "sp", weights="stored", ipropags=0)
    with pytest.raises(ValueError, match="IPROPAGS = 1"):
        Wamintgr(cfg, None, "sp", ipropags=1)


def test_the_fixtures_are_the_cases_of_the_issue_and_small():
    files = sorted(f for f in os.listdir(P.GOLDEN) if f.startswith("propags_"))
    assert files == sorted([f"propags_{n}.npz" for n in P.CASES] + ["propags_observed.json"])
    for f in files:
        assert os.path.getsize(os.path.join(P.GOLDEN, f)) <= 600_000, f
    c = P.CASES
    sph = [v for v in c.values() if v[0] == 1 and v[4] == P.DELPRO]
    assert {v[2] for v in sph if v[1] == 1 and not v[3]} == {0, 1, 2, 3}                 # spherical IRGG 1, IREFRA 0 .. 3
    assert (1, 0, 3, False, P.DELPRO) in sph                                             # spherical IRGG 0, IREFRA 3
    assert {v[2] for v in sph if v[3]} == {0, 3}                                         # obstruction planes at IREFRA 0 and 3
    assert {v[2] for v in c.values() if v[0] == 2} == {0, 1, 3}                          # Cartesian
    assert {v[2] for v in c.values() if v[4] != P.DELPRO} == {0, 3}                      # a time step too long for the grid
    g = P.fixture_grid()
    assert 50 <= g.nsea <= 70 and (P.NANG, P.NFRE, P.NFRE_RED) == (12, 36, 25) and P.NFRE_RED % 4 != 0


def test_the_grid_covers_what_it_claims():
    with open(os.path.join(P.GOLDEN, "propags_observed.json")) as fh:
        obs = json.load(fh)
    assert P.grid_coverage(P.fixture_grid()) == obs["grid"]


@pytest.mark.parametrize("name", list(P.CASES))
def test_coverage_and_the_restatement_bit_for_bit(name):
    """The coverage conditions on the committed file (propags_ref.coverage asserts them), and the restatement against it: F3, THDD, THDC, SDOT and the
    CFL numbers, the same bits in single and in double precision."""
    fx = P.load_fixture(name)
    irefra = P.CASES[name][2]
    want = {f"{k}_{p}" for p in PREC for k in ("f3", "thdd", "thdc", "cfl") + (("sdot",) if irefra in (2, 3) else ())}
    assert set(fx) == want
    for p, T in PREC.items():
        assert all(fx[f"{k}_{p}"].dtype == T for k in ("f3", "thdd", "thdc", "cfl"))
    other = P.load_fixture(P.UNOBSTRUCTED[name]) if name in P.UNOBSTRUCTED else None
    obs = P.coverage(name, fx, other)
    for p in PREC:
        assert all(obs["bit_identical"][p].values()), (p, obs["bit_identical"][p])
        assert p in obs["zero_fraction"]
    with open(os.path.join(P.GOLDEN, "propags_observed.json")) as fh:
        assert json.load(fh)["cases"][name] == json.loads(json.dumps(obs))


def test_the_tool_reproduces_the_fixtures(tmp_path):
    """Where a reference tree exists: the driver builds around the unmodified routines and the recorded files reproduce (as tests/test_golden_tools.py does
    for the other tools)."""
    sys.path.insert(0, ROOT)
    from oracle import ref_build

    ref = ref_build.reference_root()
    if ref is None:
        pytest.skip("no reference tree on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_propags.py"), ref, str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    committed = sorted(f for f in os.listdir(P.GOLDEN) if f.startswith("propags_"))
    assert sorted(os.listdir(tmp_path)) == committed
    for f in committed:
        new, old = os.path.join(tmp_path, f), os.path.join(P.GOLDEN, f)
        if f.endswith(".json"):
            with open(new) as a, open(old) as b:
                assert json.load(a) == json.load(b), f
        else:
            with np.load(new) as z, np.load(old) as g:
                assert sorted(z.files) == sorted(g.files), f
                for k in z.files:
                    assert z[k].dtype == g[k].dtype and z[k].shape == g[k].shape and z[k].tobytes() == g[k].tobytes(), (f, k)
