"""Generates tests/golden/forcing_0.npz and tests/golden/forcing_observed.json by RUNNING the reference's own WAMWND, MICEP, CDUSTARZ0,
WAMADSWSTAR, WAMCUR and OUTBETA (src/ecwam/*.F90) behind tools/forcing_driver.F90, built by oracle/ref_build.py::build_driver with the
reference's own modules in double and in single precision.  Everything is built in a temporary
directory outside the tree; the reference's text is read by the compiler, never copied.  The fixtures hold outputs only: what the routines
returned on the 64 active rows, per recorded call (tests/forcing_ref.py::CALLS) and precision; the inputs are those of
tests/forcing_ref.py::make_cases, which the tests rebuild (float32-representable, so that both precisions see the same numbers).  Only usable
where the reference tree exists.

The NEMO currents (getcurr.F90:168-181) and the WVBLOCK fill (wavemdl.F90:757-802) are statements of larger routines: the driver restates
those few lines around the reference's OUTBETA.  The zero currents of getcurr.F90:189-192 need no program: their result is recorded as zeros.

The tool asserts that the single and the double precision reference took the same branch at every point -- the decisions of the routines
evaluated in both precisions on the inputs (tests/forcing_ref.py returns them beside its results) and the sets of values the two results give
as exactly 0, 1, WSPMIN, EPSUS, PRCHAR, ALPHAMIN and +-CURRENT_MAX -- and fails if they did not: no case is dropped.  It then writes the
observed figures the tests take their gates from, per routine and output column (the largest over the recorded calls of the routine):
  restatement_vs_reference_dp  the difference between tests/forcing_ref.py in float64 and the double precision results
  restatement_vs_reference_sp  the same in single precision (reported; no gate comes from it)
  reference_sp_vs_dp           the difference between the reference's own single and double precision results
each |a - b| / max(|b|, the column's largest |b| over the points); for WDWAVE the difference is taken on the circle.

    python tools/make_golden_forcing.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import glob
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forcing_ref as F  # noqa: E402  (the construction of the inputs and the restatement, shared with the tests)
import golden_common as GC  # noqa: E402

REF, OUT = GC.arguments(__doc__, F.GOLDEN)
ROUTINES = ("wamwnd", "micep", "cdustarz0", "wamadswstar", "wamcur", "outbeta")
A = slice(F.KIJS, F.KIJL)
N = F.KIJL - F.KIJS
# what the driver returns for GETWND, in its order
GETWND_OUT = ["AIRD", "WDWAVE", "CICOVER", "WSWAVE", "WSTAR", "USTRA", "VSTRA", "UFRIC", "CITHICK"]


_r = GC.r


def _head(op, call, prec, o=None):
    """OP, the 24 reals and the 16 switches of a record"""
    t = F.tables_of(call, prec)
    o = o or F._G
    s = [t.G, t.GM1, t.ZPI, t.EPSUS, F.ZMISS, t.XKAPPA, t.XNLEV, t.RNUM, F.PRCHAR, t.ALPHAMIN, t.ALPHAMAX, t.ALPHA, t.WSPMIN, o["rwfac"], t.HICMIN, t.CITHRSH,
         F.SWAMPCITH, t.CDMAX, 1.03e-3, 0.04e-3, 1.48, -0.21, F.CURRENT_MAX, 0.0]
    sw = [o["icode_wnd"], o["llwswave"], o["llwdwave"], o["lwcou"], o["lwcur"], o["lrelwind"], o["irefra"], o["iparamci"], o["lwnemocoucic"], o["lwnemocoucit"],
          o["lnemoicerest"], o["liceth"], int(t.cfg.licerun), int(t.cfg.lmaskice), o["swamp"], int(t.cfg.llgcbz0)]
    return np.array([op], "<i4").tobytes() + _r([float(v) for v in s]) + np.array(sw, "<i4").tobytes()


def run(exe, tmp, prec, cases):
    cell = cases["map_in"][A]
    nemo = cases["nemo"][:, A]
    ff, intf = cases["ff"][A], cases["intf"][A]
    ncols = []
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(np.array([N, F.NX, F.NY], "<i4").tobytes())
        fh.write(np.asarray(cell % F.NX + 1, "<i4").tobytes() + np.asarray(cell // F.NX + 1, "<i4").tobytes())
        for call in F.CALLS:
            r = F.routine_of(call)
            g = _r(F.fieldg_of(call, cases))      # [13][NY][NX] = FIELDG(NX,NY,13)
            if r == "getwnd":
                fh.write(_head(1, call, prec, F.GETWND[call]) + g + _r(cases["ucur"][A]) + _r(cases["vcur"][A]) + _r(nemo) + _r(ff[:, F.FF["WSWAVE"]])
                         + _r(ff[:, F.FF["UFRIC"]]))
                ncols.append(9)
            elif r == "cdustarz0":
                fh.write(_head(2, call, prec) + _r(ff[:, F.FF["WSWAVE"]]))
                ncols.append(2)
            elif r == "adswstar":
                fh.write(_head(3, call, prec) + g)
                ncols.append(4)
            elif call == "getcurr0":
                fh.write(_head(4, call, prec) + g)
                ncols.append(2)
            elif call == "getcurr1":
                fh.write(_head(5, call, prec) + g + _r(nemo))
                ncols.append(2)
            elif call == "getcurr2":
                ncols.append(0)
            else:
                flags, _, nwv = F.WVBLOCK[call]
                fh.write(_head(6, call, prec) + np.array([flags & 1, flags & 2, flags & 4, flags & 8, nwv], "<i4").tobytes())
                fh.write(_r(np.stack([ff[:, F.FF[k]] for k in ("WSWAVE", "UFRIC", "Z0M", "Z0B", "CHRNCK")] + [intf[:, F.INTF[k]] for k in F.WVB_NAMES[2:]])))
                ncols.append(nwv)
        fh.write(np.array([0], "<i4").tobytes())
    flat = GC.drive(exe, tmp)
    assert flat.size == N * sum(ncols), (flat.size, ncols)
    out, at = {}, 0
    for call, nc in zip(F.CALLS, ncols):
        a = flat[at:at + N * nc].reshape(nc, N).T
        at += N * nc
        if F.routine_of(call) == "getwnd":
            a = a[:, [GETWND_OUT.index(k) for k in F.columns(call)]]
        elif call == "getcurr2":
            a = np.zeros((N, 2))
        out[call] = np.ascontiguousarray(a)
    return out


def same_branches(cases, ref):
    """Fails unless both precisions decide alike everywhere (the module docstring lists the decisions)."""
    for call in F.CALLS:
        dec = {}
        for p in ("sp", "dp"):
            dec[p] = list(F.restate(call, p, cases, with_decisions=True)[1])
            dec[p] += [ref[p][call] == v for v in F.exact_values(call, p)]
        for i, (a, b) in enumerate(zip(dec["sp"], dec["dp"])):
            if not np.array_equal(a, b):
                raise SystemExit(f"{call}: the single and the double precision reference differ in decision {i} at "
                                 f"{int((np.asarray(a) != np.asarray(b)).sum())} places: widen the margins of tests/forcing_ref.py::make_cases")


def main():
    tmp = tempfile.mkdtemp(prefix="golden_forcing_")
    kinds = ("restatement_vs_reference_dp", "restatement_vs_reference_sp", "reference_sp_vs_dp")
    obs = {k: {} for k in kinds}
    per_call = {}
    try:
        cases = F.make_cases()
        exe = GC.executables(REF, "forcing", ROUTINES, tmp, standins=("YOWWIND",))
        ref = {p: run(exe[p], tmp, p, cases) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    same_branches(cases, ref)
    arrays = {}
    for call in F.CALLS:
        r = F.routine_of(call)
        figs = dict(restatement_vs_reference_dp=F.errors(call, F.restate(call, "dp", cases), ref["dp"][call]),
                    restatement_vs_reference_sp=F.errors(call, F.restate(call, "sp", cases), ref["sp"][call]),
                    reference_sp_vs_dp=F.errors(call, ref["sp"][call], ref["dp"][call]))
        per_call[call] = figs
        for k in kinds:
            for name, v in figs[k].items():
                name = "ZERO" if name.startswith("ZERO") else name
                obs[k].setdefault(r, {})[name] = max(obs[k].get(r, {}).get(name, 0.0), float(v))
        print(call, " ".join(f"{c} {figs['restatement_vs_reference_dp'][c]:.2e}/{figs['reference_sp_vs_dp'][c]:.2e}" for c in F.columns(call)))
        for name in F.columns(call):      # what the reference copies is the same number in both precisions
            if name not in F.COMPUTED[r]:
                assert figs["reference_sp_vs_dp"][name] == 0, (call, name)
        arrays[f"{call}_dp"] = ref["dp"][call]
        arrays[f"{call}_sp"] = ref["sp"][call].astype(np.float32)
        assert np.array_equal(arrays[f"{call}_sp"].astype(np.float64), ref["sp"][call]), call
    for old in glob.glob(os.path.join(OUT, "forcing_*.npz")):
        os.remove(old)
    GC.write_npz(OUT, "forcing_0.npz", arrays)
    obs["per_call"] = per_call
    obs["error_measure"] = "per column: |a - b| / max(|b|, the column's largest |b| over the points), the maximum over the points; WDWAVE on the circle"
    GC.write_observed(OUT, "forcing_observed.json", obs)


if __name__ == "__main__":
    main()
