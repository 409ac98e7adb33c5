"""The forcing intake without a GPU: the interface the library exports (include/ecwam_hip_intake.h), and ecwam_amd/intake.py with the numpy
restatement of FLDINTER, INIT_FIELDG, RECVNEMOFIELDS, UPDNEMOFIELDS and UPDNEMOSTRESS (tests/intake_ref.py) against the reference's own results
(tests/golden/intake_0.npz, recorded by tools/make_golden_intake.py), in both precisions.  The gates are those of the device tests: read from
tests/golden/intake_observed.json, where the tool wrote what the reference and the restatement gave -- nothing there comes from the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import intake_ref as F
from ecwam_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"ecwam_hip_set_fldinter": 6, "ecwam_hip_fldinter": 13, "ecwam_hip_init_fieldg": 6, "ecwam_hip_recvnemofields": 12, "ecwam_hip_updnemo": 9}
A = slice(F.KIJS, F.KIJL)
N = F.KIJL - F.KIJS
TABS = ("dj1", "dii1", "diip1", "jj", "ii", "iip")


def _headers():
    inc = os.path.join(ROOT, "include")
    out = {}
    for name in sorted(os.listdir(inc)):
        with open(os.path.join(inc, name)) as fh:
            out[name] = fh.read()
    return out


def test_the_header_and_the_bindings_declare_the_five_calls():
    hdrs = _headers()
    hdr = hdrs["ecwam_hip_intake.h"]
    assert '#include "ecwam_hip_forcing.h"' in hdr and "ECWAM_HIP_ABI_VERSION" in hdr
    declared = re.findall(r"^int (ecwam_hip_\w+)\(([^;]*)\);", hdr, re.M)
    assert [d[0] for d in declared] == list(WANT)      # exactly the five, in this order
    for name, args in declared:
        assert len(args.split(",")) == WANT[name], (name, args)
    assert lib.EXPORTS_INTAKE == list(WANT)
    assert (len(lib.EXPORTS), len(lib.EXPORTS_START), len(lib.EXPORTS_FORCING), len(lib.EXPORTS_GRIBOUT), len(lib.EXPORTS_GRIBIN)) == (72, 4, 7, 4, 2)
    assert lib.ABI_VERSION == 6
    for other, text in hdrs.items():      # none of the five is declared, or spoken of, in another header
        if other != "ecwam_hip_intake.h":
            assert not set(WANT) & set(re.findall(r"\becwam_hip_\w+", text)), other
    with open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")) as fh:
        f90 = fh.read()
    for name in WANT:
        assert f"NAME='{name}'" in f90, name
    for k, v in (("FLI_LADEN", 1), ("FLI_LGUST", 2), ("FLI_LLKC", 4), ("FLI_LWCUR", 8), ("FLI_NEWCURR", 16), ("RNF_LREST", 1), ("RNF_LINIT", 2), ("RNF_LWCOU", 4),
                 ("RNF_LWNEMOCOUCIC", 8), ("RNF_LWNEMOCOUCIT", 16), ("RNF_LWNEMOCOUCUR", 32), ("RNF_LWNEMOCOUIBR", 64)):
        assert re.search(rf"#define ECWAM_HIP_{k} {v}\b", hdr) and getattr(lib, k) == v, k
    assert (F.LADEN, F.LGUST, F.LLKC, F.LWCUR, F.NEWCURR) == (1, 2, 4, 8, 16) and (F.LREST, F.LINIT, F.LWCOU, F.CIC, F.CIT, F.CUR, F.IBR) == (1, 2, 4, 8, 16, 32, 64)


def test_the_library_exports_the_entry_points():
    """Fails without the feature: the built library holds the five symbols, at ABI 6, and each refuses a null context before anything else."""
    h = C.CDLL(lib.LIBPATH)      # the built library itself (no device is touched by loading it)
    for name in WANT:
        assert hasattr(h, name), name
    h.ecwam_hip_abi_version.restype = C.c_int
    assert h.ecwam_hip_abi_version() == 6
    h.ecwam_hip_last_error.restype = C.c_char_p
    d = C.c_double(0.0)
    calls = (lambda: h.ecwam_hip_set_fldinter(None, 0, 0, None, None, 0),
             lambda: h.ecwam_hip_fldinter(None, 0, 0, None, 0, 0, 0, d, d, d, None, None, None),
             lambda: h.ecwam_hip_init_fieldg(None, None, 0, d, d, None),
             lambda: h.ecwam_hip_recvnemofields(None, 0, 0, 0, None, None, None, None, None, None, None, None),
             lambda: h.ecwam_hip_updnemo(None, 0, 0, None, 0, None, None, 0, None))
    assert len(calls) == len(WANT)
    for call in calls:
        assert call() == 1 and h.ecwam_hip_last_error() == b"null context"


def test_the_cases_cover_what_they_claim():
    c, g, obs = F.cached_cases(), F.load_golden(), F.observed()
    assert np.unique(c["map_in"]).size == F.NROW and c["map_in"].max() < F.NCELL
    assert (c["ifromij"] <= F.KLONRGG[F.NY - c["jfromij"]]).all() and np.unique(F.KLONRGG).size > 3      # a reduced grid, every row inside it
    a, b = c["A"], c["B"]
    assert a["iperiodic"] == 1 and a["nr"] == 7 and a["ilonrgg"].min() == 8 and a["ilonrgg"].max() == 16
    assert b["iperiodic"] == 0 and np.unique(b["ilonrgg"]).size == 1 and not c["C"]["interpol"]
    for name in F.CASES:      # IJBLOCK is a permutation of the field order
        gr = c[name]
        used = np.concatenate([gr["ijblock"][1:int(gr["ilonrgg"][gr["nr"] - jj]) + 1, jj - 1] for jj in range(1, gr["nr"] + 1)])
        assert sorted(used) == list(range(1, gr["ngptotg"] + 1)), name
    # case B: the wave grid reaches beyond the atmosphere grid on every side, so the clamps of INITIALINT and FLDINTER work
    jj, ii = g["tab_B_dp_jj"], g["tab_B_dp_ii"]
    assert c["amonop"] > b["rmonop"] and c["amosop"] < b["rmosop"] and (jj == 1).sum() > 1 and (jj == b["nr"]).sum() > 1
    assert (ii == 9).any() and (g["tab_B_dp_dii1"] > 1).any()      # MIN(III, ILONRGG): a point east of the grid keeps the last column
    idx, _ = F.point_table(c, "B", F.golden_tables(g, "B", "dp"))
    assert (idx[A, 0] == idx[A, 1]).any() and (idx[A, 0] == idx[A, 2]).any()      # II1 = II at the eastern edge, JJ1 = JJ at the southern one
    idx, _ = F.point_table(c, "A", F.golden_tables(g, "A", "dp"))
    wrap = [a["ijblock"][int(a["ilonrgg"][a["nr"] - jj]) + 1, jj - 1] - 1 for jj in range(1, a["nr"] + 1)]
    assert np.isin(idx[A, 1], wrap).any() or np.isin(idx[A, 3], wrap).any()      # the wrap column of the periodic grid is read
    # every branch of the sea-ice rule is taken by an active row, in each interpolating case
    for name in ("A", "B"):
        idx, w = F.point_table(c, name, F.golden_tables(g, name, "dp"))
        branch = F.fldinter("dp", idx[A], w[A], c[name]["fields"], F.FLAGSETS["all"], c["roair"], c["wstar0"])[3]
        assert set(branch) == set(F.ICE_BRANCHES), (name, set(F.ICE_BRANCHES) - set(branch))
        assert {f"{name}:{x}" for x in F.ICE_BRANCHES} <= set(obs["branches"])
    sets = list(F.FLAGSETS.values())
    for bit in (F.LADEN, F.LGUST, F.LLKC):
        assert any(s & bit for s in sets) and any(not s & bit for s in sets)
    cur = {(bool(s & F.NEWCURR), bool(s & F.LWCUR)) for s in sets}
    assert {(True, True), (True, False)} <= cur and any(not n for n, _ in cur)
    lk = c["fieldg"][F.FG["LKFR"], c["map_in"][A]]
    assert (lk == 0).any() and (lk > 0).any() and (lk < 0).any()
    for k in (2, 3):
        assert (np.abs(c["nemo"][k, A]) > F.CURRENT_MAX).any() and (c["nemo"][k, A] < 0).any() and (c["nemo"][k, A] == 0).any()
    for k in ("nemo", "nemoibr", "wam2nemo"):      # doubles that no float32 holds: the single precision stores round
        assert (c[k] != c[k].astype(np.float32)).any(), k
    for name in F.CASES:
        assert (c[name]["fields"] == c[name]["fields"].astype(np.float32)).all()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_initialint_and_the_point_table_against_the_reference(prec):
    c, g, obs = F.cached_cases(), F.load_golden(), F.observed()
    T = F.dtype_of(prec)
    for name in ("A", "B"):
        own = F.own_tables(c, name, prec)
        ref = F.golden_tables(g, name, prec)
        for k, mine, theirs in zip(TABS, own, ref):
            if k in ("jj", "ii", "iip"):
                assert theirs.dtype == np.int32 and np.array_equal(mine, theirs), (name, k)
                assert np.array_equal(theirs, g[f"tab_{name}_{'sp' if prec == 'dp' else 'dp'}_{k}"]), (name, k)      # both precisions of the reference agree
            else:
                assert theirs.dtype == T and mine.dtype == T
                err = F.plane_error(mine, theirs)
                print(f"{name} {k} {prec}: intake.initialint against the reference {err:.3e} (gate {F.gate('weights', k.upper(), prec, obs):.3e})")
                assert err <= obs["per_call"][f"tab_{name}"][f"restatement_vs_reference_{prec}"][k.upper()]
                assert err <= F.gate("weights", k.upper(), prec, obs)
        idx, w = F.point_table(c, name, ref)
        assert idx.dtype == np.int32 and idx.shape == (F.NROW, 4) and w.shape == (F.NROW, 3) and idx.min() >= 0 and idx.max() < c[name]["ngptotg"]
        assert np.array_equal(w.astype(T).astype(np.float64), w)
    idx, w = F.point_table(c, "C")
    assert w is None and (idx == idx[:, :1]).all() and np.unique(idx[:, 0]).size == F.NROW


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_restatement_against_the_reference(prec):
    """With the reference's own tables the restated FLDINTER gives the reference's FIELDG bit for bit, in every case and flag set, and its
    MASK_IN; so do the three small routines."""
    c, g = F.cached_cases(), F.load_golden()
    T = F.dtype_of(prec)
    for name in F.CASES:
        gr = c[name]
        idx, w = F.point_table(c, name, F.golden_tables(g, name, prec) if gr["interpol"] else None)
        for fs, flags in F.FLAGSETS.items():
            ref = g[f"fli_{name}_{fs}_{prec}"]
            assert ref.dtype == T and ref.shape == (13, N)
            got, pos, _, _ = F.fldinter(prec, idx[A], None if w is None else w[A], gr["fields"], flags, c["roair"], c["wstar0"])
            assert got.tobytes() == ref.tobytes(), (name, fs, [k for k, i in F.FG.items() if got[i].tobytes() != ref[i].tobytes()])
            rest = sorted(set(range(13)) - set(F.written_planes(flags)))
            assert (ref[rest] == T(F.SENT)).all() and (ref[F.written_planes(flags)] != T(F.SENT)).all(), (name, fs)
            mask = np.zeros(gr["ngptotg"], np.int8)
            mask[pos] = 1
            assert np.array_equal(mask, g[f"mask_{name}_{fs}"]) and 0 < mask.sum() <= gr["ngptotg"], (name, fs)
    assert F.init_fieldg(prec, F.NCELL, c["roair"], c["wstar0"]).tobytes() == g[f"initfg_{prec}"].tobytes()
    ri = F.recv_inputs(c)
    for call, flags in F.RECV.items():
        nemo, state = F.recvnemofields(prec, flags, **ri)
        assert nemo.tobytes() == g[f"recv_{call}_nemo_{prec}"].tobytes() and state.tobytes() == g[f"recv_{call}_state_{prec}"].tobytes(), call
    for nt in F.NEMONTAU:
        f7, s6, w2n = F.updnemo(prec, c["wam2nemo"][A], nt)
        assert f7.tobytes() == g[f"upd_{nt}_fields7_{prec}"].tobytes() and s6.tobytes() == g[f"upd_{nt}_stress6_{prec}"].tobytes(), nt
        assert w2n.tobytes() == g[f"upd_{nt}_wam2nemo_{prec}"].tobytes() and not w2n[:, F.UPD_STRESS].any() and w2n[:, F.UPD_FIELDS].all()


def test_the_fixtures_hold_every_branch():
    g, c = F.load_golden(), F.cached_cases()
    for prec in ("dp", "sp"):
        T = F.dtype_of(prec)
        ci = g[f"fli_A_all_{prec}"][F.FG["CICOVER"]]
        assert (ci == T(F.PMISS)).any() and ((ci >= 0) & (ci <= 1)).any()
        assert (g[f"fli_A_none_{prec}"][F.FG["AIRD"]] == T(c["roair"])).all() and (g[f"fli_A_none_{prec}"][F.FG["WSTAR"]] == T(c["wstar0"])).all()
        assert not g[f"fli_A_none_{prec}"][F.FG["LKFR"]].any() and g[f"fli_A_all_{prec}"][F.FG["LKFR"]].any()
        assert not g[f"fli_A_laden_zerocur_{prec}"][F.FG["UCUR"]].any() and g[f"fli_A_all_{prec}"][F.FG["UCUR"]].all()
        assert (g[f"fli_A_gust_lake_oldcur_{prec}"][F.FG["UCUR"]] == T(F.SENT)).all()
        st = g[f"recv_init_cou_cur_state_{prec}"]
        assert (np.abs(st[2:4]) == F.CURRENT_MAX).any() and (st[2:4] == 0).any() and (np.abs(st[2:4]) <= F.CURRENT_MAX).all()
        assert (np.abs(g[f"recv_init_cur_state_{prec}"][2:4]) > F.CURRENT_MAX).any()      # without LWCOU the plain copy: no clip
        a, b = g[f"recv_init_cou_cit_state_{prec}"], g[f"recv_init_cit_state_{prec}"]
        lake = c["fieldg"][F.FG["LKFR"], c["map_in"][A]] > 0
        assert (a[0, lake] == (0.5 * c["nemo"][0, A][lake]).astype(T)).all() and (a[1, lake] == c["ff"][A, F.FF_CITHICK][lake].astype(T)).all()      # line 201
        assert (a[1, ~lake] == b[1, ~lake]).all() and (a[0, ~lake] == c["ff"][A, F.FF_CICOVER][~lake].astype(T)).all()
        assert not g[f"upd_0_stress6_{prec}"].any() and g[f"upd_7_stress6_{prec}"].all()
    assert not np.array_equal(g["upd_7_stress6_sp"], g["upd_7_stress6_dp"]) and np.array_equal(g["upd_1_stress6_sp"], g["upd_1_stress6_dp"])


def test_the_gates_are_the_measured_ones():
    obs, g = F.observed(), F.load_golden()
    e64, e32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
    for kind, names in (("fldinter", list(F.FG)), ("weights", ["DJ1", "DII1", "DIIP1"])):
        for name in names:
            v, s = obs["restatement_vs_reference_dp"][kind][name], obs["reference_sp_vs_dp"][kind][name]
            assert F.gate(kind, name, "dp", obs) == (10 * v if v > 0 else 8 * e64) and F.gate(kind, name, "sp", obs) == (3 * s if s > 0 else 8 * e32)
            for k in ("restatement_vs_reference_dp", "reference_sp_vs_dp"):
                per = [cc[k][name] for call, cc in obs["per_call"].items() if call.startswith("fli_" if kind == "fldinter" else "tab_")]
                assert obs[k][kind][name] == max(per), (kind, name, k)
    for name in F.CASES:      # the figures are those the fixtures give
        for fs in F.FLAGSETS:
            call = f"fli_{name}_{fs}"
            for plane, ip in F.FG.items():
                assert F.plane_error(g[f"{call}_sp"][ip], g[f"{call}_dp"][ip]) == obs["per_call"][call]["reference_sp_vs_dp"][plane], (call, plane)
    for plane in ("CITHICK", "WSWAVE", "WDWAVE"):      # constants and what FLDINTER leaves alone: the same in both precisions
        assert obs["reference_sp_vs_dp"]["fldinter"][plane] == 0
