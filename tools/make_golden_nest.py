"""Generates tests/golden/intspec_nang12.npz by RUNNING the reference's own INTSPEC / ROTSPEC / STRSPEC (src/ecwam/intspec.F90,
rotspec.F90, strspec.F90) behind tools/intspec_driver.F90, built by oracle/ref_build.py::build_driver with the reference's own modules in
double and in single precision.  Everything is built in a temporary directory outside the tree;
the reference's text is read by the compiler, never copied.  The fixture holds data only: the inputs (float32-representable, so that both
precisions see the same numbers), the two frequency tables, and what INTSPEC returned.  Only usable where the reference tree exists.

The mean frequencies are constructed so that STRSPEC's INT(LOG10(GAMMA)/LOG10(1.1)) is nowhere near a discontinuity
(tests/intspec_ref.py::make_cases, which the tests' 36-direction cases share).

    python tools/make_golden_nest.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ecwam_amd.tables import Config, Tables  # noqa: E402
from intspec_ref import make_cases  # noqa: E402  (the construction of the inputs, shared with the tests)
import golden_common as GC  # noqa: E402

REF, OUT = GC.arguments(__doc__, os.path.join(ROOT, "tests", "golden"))
NCASE, NANG, NFRE = 96, 12, 36


def cases(rng):
    t = Tables(Config(nang=NANG, nfre=NFRE, nfre_red=NFRE), np.float64)
    return make_cases(rng, NCASE, np.asarray(t.FR), np.asarray(t.TH))


def run(exe, tmp, fr, bfw, f, par):
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(np.array([NCASE, NANG, NFRE], "<i4").tobytes())
        fh.write(np.asarray(fr, "<f8").tobytes())
        for i in range(NCASE):
            s = [bfw[i], par[i, 0, 2], par[i, 0, 0], par[i, 0, 1], par[i, 1, 2], par[i, 1, 0], par[i, 1, 1]]
            fh.write(np.asarray(s, "<f8").tobytes())
            fh.write(f[i, 0].astype("<f8").tobytes())      # [M][K] in C order = F(K,M) in Fortran order
            fh.write(f[i, 1].astype("<f8").tobytes())
    a = GC.drive(exe, tmp).reshape(NCASE, 3 + NANG * NFRE)
    return a[:, 3:].reshape(NCASE, NFRE, NANG), a[:, [1, 2, 0]]      # FL [M][K]; EMEAN, THQ, FMEAN


def main():
    rng = np.random.default_rng(20261019)
    bfw, f, par, form = cases(rng)
    fr = {p: np.asarray(Tables(Config(nang=NANG, nfre=NFRE, nfre_red=NFRE), dt).FR) for p, dt in (("sp", np.float32), ("dp", np.float64))}
    tmp = tempfile.mkdtemp(prefix="golden_nest_")
    try:
        exe = GC.executables(REF, "intspec", ("rotspec", "strspec", "intspec"), tmp)
        out = {p: run(exe[p], tmp, fr[p], bfw, f, par) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    peak = np.abs(out["dp"][0]).max(axis=(1, 2))
    d = np.abs(out["sp"][0] - out["dp"][0]).max(axis=(1, 2)) / peak
    print(f"{NCASE} cases: single against double precision, per bin over the peak: max {d.max():.2e}, median {np.median(d):.2e}")
    GC.write_npz(OUT, "intspec_nang12.npz", dict(nang=NANG, nfre=NFRE, fr_sp=fr["sp"], fr_dp=fr["dp"], bfw=bfw, f=f, par=par, form=form, fl_dp=out["dp"][0],
                                                 par_dp=out["dp"][1], fl_sp=out["sp"][0].astype(np.float32), par_sp=out["sp"][1].astype(np.float32)))


if __name__ == "__main__":
    main()
