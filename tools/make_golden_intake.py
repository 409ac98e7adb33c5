"""Generates tests/golden/intake_0.npz and tests/golden/intake_observed.json by RUNNING the reference's own INITIALINT, FLDINTER, INIT_FIELDG,
RECVNEMOFIELDS, UPDNEMOFIELDS and UPDNEMOSTRESS (src/ecwam/*.F90) behind tools/intake_driver.F90, built by
oracle/ref_build.py::build_driver with the reference's own modules in double and in single precision.  Everything is built in a temporary directory
outside the tree; the reference's text is read by the compiler, never copied.  The fixture holds outputs only, per case and precision: the six
tables of INITIALINT, FIELDG on the 64 active rows and MASK_IN per FLDINTER call, INIT_FIELDG's planes, and what RECVNEMOFIELDS and the two
UPDNEMO routines leave; the inputs are those of tests/intake_ref.py::make_cases, which the tests rebuild (float32-representable, so that both
precisions see the same numbers).  Only usable where the reference tree exists.

UPDNEMOFIELDS and UPDNEMOSTRESS keep their results in local arrays that only the call into NEMO would see: the driver restates their copies and
products and runs the routines for what does show, the accumulators starting again and NEMONTAU = 0.

The tool fails ("widen the margins") unless the reference's single and double precision integer tables are equal, ecwam_amd/intake.py's
integer tables equal both, and both precisions decide every <= 0.5 and == PMISS of FLDINTER alike; and unless every branch of the sea-ice rule
(tests/intake_ref.py::ICE_BRANCHES) is taken by an active row.  No case is dropped.  It then writes the observed figures the tests take their
gates from, per plane of FIELDG and per weight table (the largest over the recorded calls):
  restatement_vs_reference_dp  the restated chain (intake.initialint -> intake.point_table -> tests/intake_ref.py::fldinter) in float64 against
                               the double precision results
  restatement_vs_reference_sp  the same in single precision (reported; no gate comes from it)
  reference_sp_vs_dp           the reference's own single against its double precision results
each |a - b| / max(|b|, the plane's largest |b| over the points).

    python tools/make_golden_intake.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intake_ref as F  # noqa: E402  (the construction of the inputs and the restatement, shared with the tests)
import golden_common as GC  # noqa: E402

REF, OUT = GC.arguments(__doc__, F.GOLDEN)
ROUTINES = ("initialint", "fldinter", "init_fieldg", "recvnemofields", "updnemofields", "updnemostress")
# the driver's own modules (its header says why), and YOWPD, which INIT_FIELDG names only behind WAM_HAVE_UNWAM, which is not defined
STANDINS = ("YOWGRIB", "YOWPCONS", "MPL_MODULE", "MPL_DATA_MODULE", "YOWPD")
A = slice(F.KIJS, F.KIJL)
N = F.KIJL - F.KIJS
TABS = ("dj1", "dii1", "diip1", "jj", "ii", "iip")
_r, _i = GC.r, GC.i


def _fort(a):
    """an array indexed [i][j] as the Fortran one, in Fortran's storage order"""
    return np.asarray(a).T


def run(exe, tmp, prec, c):
    """-> the fixture's arrays of one precision (the keys without the precision) and MASK_IN per FLDINTER call"""
    T = F.dtype_of(prec)
    t = F.tables(prec)
    shapes = []      # per record: the names and shapes of what it returns
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(_i(N, F.NX, F.NY, c["ifromij"][A], c["jfromij"][A]))
        for name in F.CASES:
            g = c[name]
            if g["interpol"]:
                a = F.initialint_args(c, name)
                fh.write(_i(1, a[1], a[2], a[5], a[13], a[14], a[20], a[6], a[19]) + _r(a[7], a[8], a[9], a[10], a[11], a[12], a[15], a[16], a[17], a[18]))
                shapes.append([(f"tab_{name}_dj1", (F.NY,)), (f"tab_{name}_dii1", (F.NY, F.NX)), (f"tab_{name}_diip1", (F.NY, F.NX)), (f"tab_{name}_jj", (F.NY,)),
                               (f"tab_{name}_ii", (F.NY, F.NX)), (f"tab_{name}_iip", (F.NY, F.NX))])
            for fs, flags in F.FLAGSETS.items():
                fh.write(_i(2, g["ngptotg"], g["nc"], g["nr"], 10, g["iperiodic"], flags & F.LADEN, flags & F.LGUST, flags & F.LLKC, flags & F.LWCUR,
                            flags & F.NEWCURR, g["interpol"], 1, N, g["ilonrgg"], _fort(g["ijblock"]), F.KLONRGG))
                fh.write(_r(F.PMISS, c["roair"], c["wstar0"], F.SENT, g["fields"]))
                shapes.append([(f"fli_{name}_{fs}", (13, F.NY, F.NX)), (f"mask_{name}_{fs}", (g["ngptotg"],))])
        fh.write(_i(3) + _r(c["roair"], c["wstar0"], float(t.WSPMIN), 0.0185, -999.0, F.SENT))
        shapes.append([("initfg", (13, F.NY, F.NX))])
        ri = F.recv_inputs(c)
        for call, flags in F.RECV.items():
            fh.write(_i(4, *[int(bool(flags & b)) for b in (F.LREST, F.LINIT, F.LWCOU, F.CIC, F.CIT, F.CUR, F.IBR)]))
            fh.write(_r(F.CURRENT_MAX, c["fieldg"], ri["nemo"], ri["nemoibr"], ri["cicover"], ri["cithick"], ri["ucur"], ri["vcur"], ri["ibrmem"]))
            shapes.append([(f"recv_{call}_nemo", (5, N)), (f"recv_{call}_state", (5, N))])
        for nt in F.NEMONTAU:
            fh.write(_i(5, nt) + _r(_fort(c["wam2nemo"][A])))
            shapes.append([(f"upd_{nt}_fields7", (7, N)), (f"upd_{nt}_stress6", (6, N)), (f"upd_{nt}_wam2nemo", (13, N))])
        fh.write(_i(0))
    flat = GC.drive(exe, tmp)
    out, at = {}, 0
    for rec in shapes:
        for key, shape in rec:
            n = int(np.prod(shape))
            out[key] = flat[at:at + n].reshape(shape)
            at += n
    assert at == flat.size, (at, flat.size)
    res = {}
    cells = c["map_in"][A]
    for key, a in out.items():
        kind = T      # what the fixture holds the array as: the working precision unless it is integers or NEMO's doubles
        if key.startswith("tab_"):
            a = _fort(a) if a.ndim == 2 else a      # [i - 1][j - 1]
            kind = np.int32 if key.rsplit("_", 1)[1] in ("jj", "ii", "iip") else T
        elif key.startswith("fli_"):
            planes = a.reshape(13, F.NCELL)
            rest = np.ones(F.NCELL, bool)
            rest[cells] = False
            assert (planes[:, rest] == F.SENT).all(), key      # the cells of no active row keep what they held
            a = planes[:, cells]
        elif key.startswith("mask_"):
            kind = np.int8
        elif key == "initfg":
            a = a.reshape(13, F.NCELL)
        elif key.endswith("_wam2nemo"):
            a, kind = a.T, np.float64
        elif not key.endswith("_state"):
            kind = np.float64
        res[key] = np.ascontiguousarray(a, dtype=kind)
        assert np.array_equal(res[key].astype(np.float64), a), key      # nothing is lost by narrowing what the driver widened
    return res


def margins(c, ref):
    """Fails unless the integer tables agree everywhere and both precisions take every decision of FLDINTER alike; returns the branches of the
    sea-ice rule the active rows take."""
    taken = set()
    for name in F.CASES:
        g = c[name]
        if not g["interpol"]:
            continue
        for prec in ("dp", "sp"):
            own = F.own_tables(c, name, prec)
            for k, mine in zip(TABS[3:], own[3:]):
                for p2 in ("dp", "sp"):
                    if not np.array_equal(mine, ref[p2][f"tab_{name}_{k}"]):
                        raise SystemExit(f"case {name}: table {k} of intake.initialint ({prec}) differs from the reference's ({p2}): widen the margins of "
                                         "tests/intake_ref.py::make_cases")
        dec = {}
        for prec in ("dp", "sp"):
            idx, w = F.point_table(c, name, F.golden_tables({f"tab_{name}_{prec}_{k}": ref[prec][f"tab_{name}_{k}"] for k in TABS}, name, prec))
            _, _, dec[prec], branch = F.fldinter(prec, idx[A], w[A], g["fields"], F.FLAGSETS["all"], c["roair"], c["wstar0"])
            taken |= {f"{name}:{b}" for b in branch}
        for i, (a, b) in enumerate(zip(dec["sp"], dec["dp"])):
            if not np.array_equal(a, b):
                raise SystemExit(f"case {name}: the single and the double precision reference differ in decision {i} at {int((a != b).sum())} points: widen the "
                                 "margins of tests/intake_ref.py::make_cases")
    return taken


def main():
    tmp = tempfile.mkdtemp(prefix="golden_intake_")
    try:
        c = F.make_cases()
        exe = GC.executables(REF, "intake", ROUTINES, tmp, STANDINS, ('-D__FILENAME__="reference"',))
        ref = {p: run(exe[p], tmp, p, c) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    taken = margins(c, ref)
    missing = [b for b in F.ICE_BRANCHES if not any(t.endswith(":" + b) for t in taken)]
    if missing:
        raise SystemExit(f"no active row takes the branches {missing} of the sea-ice rule: change the fields of tests/intake_ref.py::make_cases")
    print("branches of the sea-ice rule:", " ".join(sorted(taken)))
    kinds = ("restatement_vs_reference_dp", "restatement_vs_reference_sp", "reference_sp_vs_dp")
    obs = {k: {"fldinter": {n: 0.0 for n in F.FG}, "weights": {n: 0.0 for n in ("DJ1", "DII1", "DIIP1")}} for k in kinds}
    per_call = {}

    def note(kind, group, name, v, call):
        obs[kind][group][name] = max(obs[kind][group][name], float(v))
        per_call.setdefault(call, {}).setdefault(kind, {})[name] = float(v)
    arrays = {}
    for name in F.CASES:
        g = c[name]
        own = {p: F.own_tables(c, name, p) if g["interpol"] else None for p in ("dp", "sp")}
        if g["interpol"]:
            for j, k in enumerate(TABS[:3]):
                r = {p: ref[p][f"tab_{name}_{k}"] for p in ("dp", "sp")}
                note("restatement_vs_reference_dp", "weights", k.upper(), F.plane_error(own["dp"][j], r["dp"]), f"tab_{name}")
                note("restatement_vs_reference_sp", "weights", k.upper(), F.plane_error(own["sp"][j], r["sp"]), f"tab_{name}")
                note("reference_sp_vs_dp", "weights", k.upper(), F.plane_error(r["sp"], r["dp"]), f"tab_{name}")
            for k in TABS[3:]:
                assert np.array_equal(ref["dp"][f"tab_{name}_{k}"], ref["sp"][f"tab_{name}_{k}"]), (name, k)
        for fs, flags in F.FLAGSETS.items():
            call = f"fli_{name}_{fs}"
            assert np.array_equal(ref["dp"][f"mask_{name}_{fs}"], ref["sp"][f"mask_{name}_{fs}"]), call
            chain = {}
            for p in ("dp", "sp"):
                idx, w = F.point_table(c, name, own[p])
                chain[p], pos, _, _ = F.fldinter(p, idx[A], None if w is None else w[A], g["fields"], flags, c["roair"], c["wstar0"])
                mask = np.zeros(g["ngptotg"], np.int8)
                mask[pos] = 1
                assert np.array_equal(mask, ref[p][f"mask_{name}_{fs}"]), call
            for plane, ip in F.FG.items():
                note("restatement_vs_reference_dp", "fldinter", plane, F.plane_error(chain["dp"][ip], ref["dp"][call][ip]), call)
                note("restatement_vs_reference_sp", "fldinter", plane, F.plane_error(chain["sp"][ip], ref["sp"][call][ip]), call)
                note("reference_sp_vs_dp", "fldinter", plane, F.plane_error(ref["sp"][call][ip], ref["dp"][call][ip]), call)
            print(call, " ".join(f"{pl} {per_call[call]['restatement_vs_reference_dp'][pl]:.1e}/{per_call[call]['reference_sp_vs_dp'][pl]:.1e}"
                                 for pl in ("UWND", "CICOVER")))
    for p in ("dp", "sp"):
        for key, a in ref[p].items():
            if key.startswith("mask_"):
                arrays[key] = a
            elif key.startswith("tab_"):
                head, k = key.rsplit("_", 1)
                arrays[f"{head}_{p}_{k}"] = a
            else:
                arrays[f"{key}_{p}"] = a
    GC.write_npz(OUT, "intake_0.npz", arrays)
    obs["per_call"] = per_call
    obs["branches"] = sorted(taken)
    obs["error_measure"] = "per plane: |a - b| / max(|b|, the plane's largest |b| over the points), the maximum over the points"
    GC.write_observed(OUT, "intake_observed.json", obs)


if __name__ == "__main__":
    main()
