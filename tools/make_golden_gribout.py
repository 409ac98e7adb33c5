"""Generates tests/golden/gribout_0.npz and tests/golden/gribout_observed.json by RUNNING the reference's own WGRIBENCODE_VALUES
(src/ecwam/wgribencode_values.F90) behind tools/gribout_driver.F90, built by oracle/ref_build.py::build_driver (with -fopenmp) in double and
in single precision.  Everything is built in a temporary directory outside the tree; the
reference's text is read by the compiler, never copied.  The driver restates the few statements of OUTSPEC, OUTWSPEC and MAKEGRID around the
routine (the sea-ice mask, FIELD = ZMISS, the block-to-grid loop).  The fixtures hold outputs only: VALUES per recorded case
(tests/gribout_ref.py::NAMES), field and precision, and PPMAX per field -- a local of the routine, recovered as the largest non-missing value
of VALUES (the maximum is never at or below PPMIN, so it is always kept).  The inputs are those of tests/gribout_ref.py::make_cases, which the
tests rebuild.  Only usable where the reference tree exists.

The tool asserts, on the double precision reference, that no value lies within 0.01 of its field's PPMIN on the log scale, and that the single
and the double precision reference give the same pattern of ZMISS; it fails otherwise -- no cell is ever left out of a comparison.  It then
writes the observed figures the tests take their gates from, each the largest absolute difference on the log scale over the non-missing
values of the spectral cases ("values") and the same for PPMAX ("ppmax"):
  restatement_vs_reference_dp  tests/gribout_ref.py in float64 against the double precision results
  restatement_vs_reference_sp  the same in single precision
  reference_sp_vs_dp           the reference's own single against its double precision results

    python tools/make_golden_gribout.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gribout_ref as G  # noqa: E402  (the construction of the inputs and the restatement, shared with the tests)
import golden_common as GC  # noqa: E402

REF, OUT = GC.arguments(__doc__, G.GOLDEN)


def run(exe, tmp, prec, g, block, cic, ice, spectral):
    """block [nfld][npts] (float32-representable) through the driver: VALUES [nfld][NTENCODE] as float64"""
    t = G.tables(prec)
    _, ntencode, _ = G.value_map(g)
    nfld, npts = block.shape
    o = G.OPTS
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(np.array([g["ngx"], g["ngy"], npts, g["irgg"], ntencode, nfld, 140251 if spectral else 140229, ice, int(g["lpadpoles"]), o["ngrbress"],
                           ord(g["cldomain"])], "<i4").tobytes())
        fh.write(np.array([g["amonop"], g["amosop"], g["xdella"], o["ppmiss"], float(t.dtype(o["ppeps"])), o["pprec"], float(t.dtype(o["ppresol"])), o["ppmin_reset"],
                           o["zmiss"], float(t.CITHRSH), float(t.FLMIN)], "<f8").tobytes())
        for a in (g["nlonrgg"], g["ixlg"], g["kxlt"]):
            fh.write(np.asarray(a, "<i4").tobytes())
        fh.write(np.asarray(cic, "<f8").tobytes())
        fh.write(np.ascontiguousarray(block, "<f8").tobytes())      # BLOCK(NPTS,NFLD): the point index fastest
    flat = GC.drive(exe, tmp, env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert flat.size == nfld * ntencode, (flat.size, nfld, ntencode)
    return flat.reshape(nfld, ntencode)


def reference(exe, tmp, prec, c):
    fa = G.fields_of(c["fl_a"], G.recorded_fields(), 12)
    fb = G.fields_of(c["fl_b"], range(G.B_FIELDS[0], sum(G.B_FIELDS)), 12)
    return {"A_ice0": run(exe, tmp, prec, c["grid_a"], fa, c["cic_a"], 0, True), "A_ice1": run(exe, tmp, prec, c["grid_a"], fa, c["cic_a"], 1, True),
            "B": run(exe, tmp, prec, c["grid_b"], fb, c["cic_b"], 0, True), "C": run(exe, tmp, prec, c["grid_a"], c["bout"].T, c["cic_a"], 0, False)}


def ppmax_of(values):
    return np.array([row[row != G.ZMISS].max() for row in values])


def main():
    tmp = tempfile.mkdtemp(prefix="golden_gribout_")
    try:
        c = G.make_cases()
        exe = GC.executables(REF, "gribout", ("wgribencode_values",), tmp, standins=("YOWGRIB", "OML_MOD"), flags=("-fopenmp",))
        ref = {p: reference(exe[p], tmp, p, c) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kinds = ("restatement_vs_reference_dp", "restatement_vs_reference_sp", "reference_sp_vs_dp")
    obs = {k: {"values": 0.0, "ppmax": 0.0} for k in kinds}
    per_case, arrays = {}, {}
    for name in G.NAMES:
        dp, sp = ref["dp"][name], ref["sp"][name]
        assert np.array_equal(sp.astype(np.float32).astype(np.float64), sp), name
        # the same pattern of ZMISS in both precisions, and (spectral) no value within MARGIN of PPMIN
        if not np.array_equal(dp == G.ZMISS, sp == G.ZMISS):
            raise SystemExit(f"{name}: the single and the double precision reference differ in {int(((dp == G.ZMISS) != (sp == G.ZMISS)).sum())} missing values")
        arrays[f"{name}_dp"], arrays[f"{name}_sp"] = dp, sp.astype(np.float32)
        figs = {}
        if name == "C":
            for p, r in (("dp", dp), ("sp", sp)):
                assert np.array_equal(G.restate(name, p, c)[0].astype(np.float64), r), (name, p)      # no logarithm: the same numbers
        else:
            pm = {"dp": ppmax_of(dp), "sp": ppmax_of(sp)}
            arrays[f"{name}_ppmax_dp"], arrays[f"{name}_ppmax_sp"] = pm["dp"], pm["sp"].astype(np.float32)
            ppmin = G.ppmin_of(pm["dp"], np.float64)
            kept = dp != G.ZMISS
            near = np.abs(np.where(kept, dp, 1e9) - ppmin[:, None]) < G.MARGIN
            if near.any():
                raise SystemExit(f"{name}: {int(near.sum())} values lie within {G.MARGIN} of PPMIN: move the inputs (tests/gribout_ref.py::_settle)")
            rv, rp = {}, {}
            for p in ("dp", "sp"):
                rv[p], rp[p] = G.restate(name, p, c)
            pairs = {"restatement_vs_reference_dp": (rv["dp"], dp, rp["dp"], pm["dp"]), "restatement_vs_reference_sp": (rv["sp"], sp, rp["sp"], pm["sp"]),
                     "reference_sp_vs_dp": (sp, dp, pm["sp"], pm["dp"])}
            for k, (a, b, pa, pb) in pairs.items():
                same, e = G.log_error(a, b)
                if not same:
                    raise SystemExit(f"{name}: {k}: the patterns of ZMISS differ")
                figs[k] = {"values": e, "ppmax": float(np.abs(np.asarray(pa, np.float64) - pb).max())}
                for w in ("values", "ppmax"):
                    obs[k][w] = max(obs[k][w], figs[k][w])
            # what is masked, scattered or padded without arithmetic differs between the precisions by the logarithm alone
            print(name, " ".join(f"{k} {figs[k]['values']:.2e}/{figs[k]['ppmax']:.2e}" for k in kinds), f"missing {int((dp == G.ZMISS).sum())} of {dp.size}")
        per_case[name] = figs
    GC.write_npz(OUT, "gribout_0.npz", arrays)
    obs["per_case"] = per_case
    obs["error_measure"] = "the largest |a - b| on the log scale over the non-missing values of VALUES (values) and over PPMAX (ppmax); the patterns of ZMISS are equal"
    GC.write_observed(OUT, "gribout_observed.json", obs)


if __name__ == "__main__":
    main()
