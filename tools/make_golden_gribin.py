"""Generates tests/golden/gribin_0.npz and tests/golden/gribin_observed.json: the statements of GETSPEC's GRIB read evaluated by the ROCm flang in
double and in single precision, built by oracle/ref_build.py::build_driver as every driver is.

What is pinned, and what is not.  None of these statements compiles alone: the un-scaling and the full copy sit inside GRIB2WGRID
(grib2wgrid.F90:771-775, 793-802), the gather and the store inside GETSPEC (getspec.F90:458-462, 548-552), and both routines are bound to eccodes
and MPL.  So, unlike tools/make_golden_gribout.py, this tool compiles NO file of the reference tree: tools/gribin_driver.F90 is the project's own
few lines around Fortran's own `**`.  The fixture therefore pins flang's evaluation of the statement 10**(V - |PPREC|) - PPEPS in each
precision -- the power function the reference's build would call -- not a compiled reference routine.  The reference tree is not read at all;
the argument is kept so that the tools are called alike.

The inputs are the reference's own single precision VALUES already committed in tests/golden/gribout_0.npz (cases A_ice0, A_ice1, B: the recorded
fields only), fed to both precisions; the fixture holds outputs only: the decoded FL1 elements [nfld][npts] per case and precision.  Everything is
built in a temporary directory outside the tree.

The tool fails if the pattern of EPSMIN-from-missing differs between the precisions or from the missing values of the input.  It then writes
the observed figures the tests take their gates from, each the largest |a - b| / (|b| + PPEPS) over all elements of all cases:
  restatement_vs_reference_dp  tests/gribin_ref.py in float64 against flang's double precision results
  restatement_vs_reference_sp  the same in single precision
  reference_sp_vs_dp           flang's single against its double precision results

    python tools/make_golden_gribin.py <root of the reference tree (not read)> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gribin_ref as R  # noqa: E402  (the inputs and the restatement, shared with the tests)
import gribout_ref as G  # noqa: E402
import golden_common as GC  # noqa: E402

_, OUT = GC.arguments(__doc__, R.GOLDEN)


def run(exe, tmp, prec, g, values):
    """values [nfld][nvalues] (float32-representable) through the driver: FL1 elements [nfld][npts] as float64"""
    t = G.tables(prec)
    nfld, nval = values.shape
    npts = g["ixlg"].size
    o = G.OPTS
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(np.array([g["ngx"], g["ngy"], npts, nval, nfld, 1], "<i4").tobytes())
        fh.write(np.array([float(t.dtype(o["ppeps"])), o["pprec"], o["zmiss"], float(t.EPSMIN)], "<f8").tobytes())
        for a in (g["nlonrgg"], g["ixlg"], g["kxlt"]):
            fh.write(np.asarray(a, "<i4").tobytes())
        fh.write(np.ascontiguousarray(values, "<f8").tobytes())      # V8(NVAL,NFLD): the value index fastest
    flat = GC.drive(exe, tmp)
    assert flat.size == nfld * npts, (flat.size, nfld, npts)
    return flat.reshape(nfld, npts)


def main():
    c = G.cached_cases()
    tmp = tempfile.mkdtemp(prefix="golden_gribin_")
    try:
        exe = GC.executables(None, "gribin", (), tmp)
        ref = {p: {name: run(exe[p], tmp, p, R.grid_of(name, c), R.inputs(name)) for name in R.NAMES} for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kinds = ("restatement_vs_reference_dp", "restatement_vs_reference_sp", "reference_sp_vs_dp")
    obs = {k: 0.0 for k in kinds}
    per_case, arrays = {}, {}
    for name in R.NAMES:
        dp, sp = ref["dp"][name], ref["sp"][name]
        assert np.array_equal(sp.astype(np.float32).astype(np.float64), sp), name
        miss = R.from_missing(R.inputs(name), R.grid_of(name, c))
        eps = {p: float(G.tables(p).EPSMIN) for p in ("dp", "sp")}
        # the elements that came from missing values are EPSMIN, in both precisions alike, and nothing else is
        for p, r in (("dp", dp), ("sp", sp)):
            if not np.array_equal(r == eps[p], miss):
                raise SystemExit(f"{name} {p}: the pattern of EPSMIN differs from the missing values of the input at {int(((r == eps[p]) != miss).sum())} places")
        arrays[f"{name}_dp"], arrays[f"{name}_sp"] = dp, sp.astype(np.float32)
        rs = {p: R.restate(name, p, c).astype(np.float64) for p in ("dp", "sp")}
        for p in ("dp", "sp"):
            if not np.array_equal(rs[p] == eps[p], miss):
                raise SystemExit(f"{name} {p}: the restatement's pattern of EPSMIN differs")
        figs = {"restatement_vs_reference_dp": R.rel_error(rs["dp"], dp), "restatement_vs_reference_sp": R.rel_error(rs["sp"], sp),
                "reference_sp_vs_dp": R.rel_error(sp, dp)}
        for k in kinds:
            obs[k] = max(obs[k], figs[k])
        per_case[name] = figs
        print(name, " ".join(f"{k} {figs[k]:.2e}" for k in kinds), f"from missing {int(miss.sum())} of {miss.size}")
    GC.write_npz(OUT, "gribin_0.npz", arrays)
    obs["per_case"] = per_case
    obs["error_measure"] = "the largest |a - b| / (|b| + PPEPS) over the decoded FL1 elements; the elements from missing values equal EPSMIN in both"
    GC.write_observed(OUT, "gribin_observed.json", obs)


if __name__ == "__main__":
    main()
