"""The forcing and coupling seam without a GPU: the interface the library exports (include/ecwam_hip_forcing.h), and the numpy restatement of
WAMWND, MICEP, CDUSTARZ0, WAMADSWSTAR, WAMCUR, OUTBETA and the WVBLOCK fill (tests/forcing_ref.py) against the reference's own results
(tests/golden/forcing_*.npz, recorded by tools/make_golden_forcing.py), in both precisions.  The gates are those of the device tests: read from
tests/golden/forcing_observed.json, where the tool wrote what the reference and the restatement gave -- nothing there comes from the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import forcing_ref as F
from ecwam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hip_set_forcing_map": 6, "ecwam_hip_getwnd": 10, "ecwam_hip_cdustarz0": 5, "ecwam_hip_wamadswstar": 6, "ecwam_hip_getcurr": 10,
        "ecwam_hip_wvblock": 11, "ecwam_hip_fldtoifs": 9}
A = slice(F.KIJS, F.KIJL)


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the seven entry points, in a header and a list of their own, at ABI 6 and beside its 72 + 4 entry points."""
    assert lib.EXPORTS_FORCING == list(WANT)
    assert len(lib.EXPORTS) == 72 and len(lib.EXPORTS_START) == 4 and lib.ABI_VERSION == 6
    assert not set(WANT) & (set(lib.EXPORTS) | set(lib.EXPORTS_START))
    with open(os.path.join(ROOT, "include", "ecwam_hip_forcing.h")) as fh:
        hdr = fh.read()
    assert '#include "ecwam_hip.h"' in hdr
    for name, nargs in WANT.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    for other in ("ecwam_hip.h", "ecwam_hip_start.h"):
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
    # a null context is refused before anything else
    h.ecwam_hip_last_error.restype = C.c_char_p
    d = C.c_double(0.0)
    calls = (lambda: h.ecwam_hip_set_forcing_map(None, 0, None, 0, None, 0),
             lambda: h.ecwam_hip_getwnd(None, 0, 0, None, None, None, None, None, None, None),
             lambda: h.ecwam_hip_cdustarz0(None, 0, 0, None, None),
             lambda: h.ecwam_hip_wamadswstar(None, 0, 0, None, None, None),
             lambda: h.ecwam_hip_getcurr(None, 0, 0, 0, None, None, None, None, None, None),
             lambda: h.ecwam_hip_wvblock(None, 0, 0, None, None, 0, 1, d, None, 0, None),
             lambda: h.ecwam_hip_fldtoifs(None, 0, 0, None, 0, 1, None, None, None))
    assert len(calls) == len(WANT)
    for call in calls:
        assert call() == 1 and h.ecwam_hip_last_error() == b"null context"


def test_the_options_struct_has_the_size_the_c_compiler_gives_it(tmp_path):
    src = ('#include "ecwam_hip_forcing.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %d", sizeof(ecwam_hip_forcing_opts), '
           'offsetof(ecwam_hip_forcing_opts, rwfac), offsetof(ecwam_hip_forcing_opts, zmiss), ECWAM_HIP_NFIELDG);return 0;}')
    exe = str(tmp_path / "opts_size")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    size, rwfac, zmiss, nplanes = (int(x) for x in subprocess.run([exe], capture_output=True, check=True).stdout.split())
    assert (size, rwfac, zmiss) == (C.sizeof(lib.ForcingOpts), lib.ForcingOpts.rwfac.offset, lib.ForcingOpts.zmiss.offset)
    assert nplanes == len(lib.FG_PLANES) == len(F.FG) and lib.FG_PLANES == list(F.FG)


def test_the_cases_cover_what_they_claim():
    """make_cases alone: every kind of point the fixtures are meant to hold is among the 64 active rows."""
    c = F.cached_cases()
    t = F.tables("dp")
    assert (np.unique(c["map_in"]).size, np.unique(c["map_out"]).size) == (F.NROW, F.NROW) and c["map_in"].max() < F.NCELL > c["map_out"].max()
    g = {k: c["fieldg"][i, c["map_in"][A]] for k, i in F.FG.items()}
    u, v, w = g["UWND"], g["VWND"], g["WSWAVE"]
    speed = np.hypot(u, v)
    wspmin = float(t.WSPMIN)
    # the wind
    assert ((u == 0) & (v == 0)).any() and (u < 0).any() and ((u == 0) & (v < 0)).any() and ((u == 0) & (v > 0)).any()
    assert ((speed > 0) & (speed < 0.5 * wspmin)).any() and (speed > 2 * wspmin).any()
    assert (w == 0).any() and (w < 0).any() and (w == F.ZMISS).any() and (w > 2 * wspmin).any() and ((w > 0) & (w < 0.5 * wspmin)).any()
    assert ((w > 0) & (speed == 0)).any() and ((w <= 0) & (speed == 0)).any() and ((w <= 0) & (speed > 0)).any()      # every arm of wamwnd.F90:166-176, 214-224
    # the ice
    for value in (F.ZMISS, 0.0, 0.005, 0.5, 0.97, 1.0, 1.2):
        assert (g["CICOVER"] == np.float32(value)).any(), value
    sst = c["sst"][c["map_in"][A]]
    assert (sst == 260.0).any() and (sst == 280.0).any()
    assert (g["LKFR"] == 0).any() and (g["LKFR"] > 0).any()
    half = 0.5 * float(t.HICMIN)
    for call in ("getwnd3", "getwnd4", "getwnd5"):      # the three forms of the thickness the consistency check follows
        o = F.GETWND[call]
        tt = F.tables_of(call, "dp")
        w_, _ = F.wamwnd(tt, o, c["fieldg"][:, c["map_in"][A]], c["ucur"][A], c["vcur"][A], c["ff"][A, 3], c["ff"][A, 7])
        o2 = dict(o, liceth=0, lwnemocoucit=0)      # the cover alone: MICEP's first part does not depend on the thickness switches
        cover, _, _ = F.micep(tt, o2, c["fieldg"][:, c["map_in"][A]], c["nemo"][:, A], w_["CITHICK"])
        if o["liceth"]:
            prod = cover * g["CITHICK"]
        elif o["lnemoicerest"]:
            prod = np.where(cover > 0, c["nemo"][1, A], 0.0)
        else:
            prod = cover * c["nemo"][1, A]
        ice = cover > 0
        assert (ice & (prod < 0.8 * half)).any() and (ice & (prod > 1.2 * half)).any(), call
        assert not (ice & (prod >= 0.8 * half) & (prod <= 1.2 * half)).any(), call
    nemo = c["nemo"][:, A]
    assert (nemo[0] == 0).any() and (nemo[0] == 1).any() and ((nemo[0] > 0) & (nemo[0] < 1)).any()
    # the currents: beyond +-CURRENT_MAX, negative, exactly 0 -- in the atmosphere's planes and in NEMO's
    for a in (g["UCUR"], g["VCUR"], nemo[2], nemo[3]):
        assert (a > F.CURRENT_MAX).any() or (a < -F.CURRENT_MAX).any()
        assert (a < 0).any() and (a == 0).any() and ((a != 0) & (np.abs(a) < F.CURRENT_MAX)).any()
    assert (g["UCUR"] > F.CURRENT_MAX).any() and (g["UCUR"] < -F.CURRENT_MAX).any()
    # Charnock and the stress
    ff = c["ff"][A]
    ch, uf = ff[:, F.FF["CHRNCK"]], ff[:, F.FF["UFRIC"]]
    assert (ch < float(t.ALPHAMIN)).any() and (ch > float(t.ALPHAMAX)).any() and ((ch > float(t.ALPHAMIN)) & (ch < 0.02)).any()
    assert (uf < float(t.EPSUS)).any() and (uf == 0).any() and (uf > 0.05).any()
    assert (ff[:, F.FF["WSWAVE"]] < 0.5 * wspmin).any() and (ff[:, F.FF["WSWAVE"]] > 30).any()      # CDUSTARZ0: below WSPMIN, and where CD is capped
    for k, val in c.items():
        assert k.startswith("map") or (val == val.astype(np.float32)).all(), k
    # the recorded calls are the ones the table of variants names
    assert [F.lcorrel(F.GETWND[f"getwnd{i}"]) for i in range(1, 7)] == [False, True, True, False, False, False]
    assert [F.GETWND[f"getwnd{i}"]["icode_wnd"] for i in range(1, 7)] == [3, 3, 3, 3, 1, 2]
    assert F.GETWND["getwnd2"]["rwfac"] not in (0.0, 1.0) and F.GETWND["getwnd2"]["iparamci"] == 139


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_restatement_against_the_reference(prec):
    """The restatement stays within the figures the tool recorded, per call and column, and is bit-identical in the copied columns."""
    g, obs, cases = F.load_golden(), F.observed(), F.cached_cases()
    T = np.float32 if prec == "sp" else np.float64
    for call in F.CALLS:
        ref = g[f"{call}_{prec}"]
        names = F.columns(call)
        assert ref.dtype == T and ref.shape == (F.KIJL - F.KIJS, len(names)), call
        got = F.restate(call, prec, cases)
        assert got.dtype == T
        err = F.errors(call, got, ref)
        rec = obs["per_call"][call][f"restatement_vs_reference_{prec}"]
        r = F.routine_of(call)
        for j, name in enumerate(names):
            print(f"{call} {name} {prec}: restatement against the reference {err[name]:.3e} (recorded {rec[name]:.3e})")
            assert err[name] <= rec[name], (call, name)
            if name not in F.COMPUTED[r]:
                assert got[:, j].tobytes() == ref[:, j].tobytes(), (call, name)
        for value in F.exact_values(call, prec):
            assert np.array_equal(got == T(value), ref == T(value)), (call, value)


def test_the_fixtures_hold_every_branch():
    """The recorded results themselves: the clamps and the branches of the routines are taken at some points and not at others."""
    g = F.load_golden()
    for prec in ("dp", "sp"):
        t = F.tables("dp" if prec == "dp" else "sp")
        w1 = g[f"getwnd1_{prec}"]
        cols = F.columns("getwnd1")
        ws, wd = w1[:, cols.index("WSWAVE")], w1[:, cols.index("WDWAVE")]
        assert (ws == t.WSPMIN).any() and (ws > t.WSPMIN).any() and (wd == 0).any() and (wd >= 0).all() and (wd > np.pi).any()
        assert (w1[:, cols.index("CITHICK")] == 0).all()      # LMASKICE
        for call in ("getwnd5", "getwnd6"):
            uf = g[f"{call}_{prec}"][:, F.columns(call).index("UFRIC")]
            assert (uf == t.EPSUS).any() and (uf > t.EPSUS).any()
        for call in ("getwnd3", "getwnd4", "getwnd5"):      # the consistency check removed some ice and kept some
            a = g[f"{call}_{prec}"]
            ci, th = a[:, F.columns(call).index("CICOVER")], a[:, F.columns(call).index("CITHICK")]
            assert ((ci == 0) & (th == 0)).any() and ((ci > 0) & (th >= 0.5 * t.HICMIN)).any() and not ((ci > 0) & (th < 0.5 * t.HICMIN)).any()
        sw = g[f"getwnd6_{prec}"]
        th = sw[:, F.columns("getwnd6").index("CITHICK")]
        assert set(np.unique(th)) == {0.0, float(t.dtype(F.SWAMPCITH))}
        for call in ("getcurr0", "getcurr1"):
            a = g[f"{call}_{prec}"]
            assert (a == F.CURRENT_MAX).any() and (a == -F.CURRENT_MAX).any() and (a == 0).any() and (np.abs(a) <= F.CURRENT_MAX).all()
        assert not g[f"getcurr2_{prec}"].any()
        b = g[f"wvblock_all_{prec}"]
        assert (b[:, 0] == t.ALPHAMIN).any() and (b[:, 0] > t.ALPHAMIN).any() and (b[:, 1] == t.ALPHAMIN).any() and (b[:, 1] > t.ALPHAMIN).any()
        assert not b[:, -1].any() and (g[f"wvblock_off_{prec}"][:, 0] == t.dtype(F.PRCHAR)).all()
        assert (g[f"wvblock_all_gcbz0_{prec}"][:, 0] == t.ALPHAMAX).any()
        cd = g[f"cdustarz0_{prec}"]
        assert (cd > 0).all()


def test_the_gates_are_the_measured_ones():
    obs = F.observed()
    e64, e32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
    for r, cols in F.COMPUTED.items():
        for name in cols:
            v = obs["restatement_vs_reference_dp"][r][name]
            assert F.gate(r, name, "dp", obs) == (10 * v if v > 0 else 8 * e64)
            s = obs["reference_sp_vs_dp"][r][name]
            assert F.gate(r, name, "sp", obs) == (3 * s if s > 0 else 8 * e32)
            for kind in ("restatement_vs_reference_dp", "reference_sp_vs_dp"):
                per = [c[kind][name] for k, c in obs["per_call"].items() if F.routine_of(k) == r and name in c[kind]]
                assert obs[kind][r][name] == max(per), (r, name, kind)
    # a copied column is the same number in both precisions of the reference: no gate, the device is held to its bits
    for r, per in obs["reference_sp_vs_dp"].items():
        for name, v in per.items():
            assert name in F.COMPUTED[r] or v == 0, (r, name)
    # the figures are those the fixtures give
    g = F.load_golden()
    for call in F.CALLS:
        assert F.errors(call, g[f"{call}_sp"], g[f"{call}_dp"]) == obs["per_call"][call]["reference_sp_vs_dp"], call
