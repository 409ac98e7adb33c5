"""Generates tests/golden/intspec_nang12.npz by RUNNING the reference's own INTSPEC / ROTSPEC / STRSPEC (src/ecwam/intspec.F90,
rotspec.F90, strspec.F90), compiled unmodified with the ROCm flang against the two-module stub of tools/intspec_driver.F90 and empty
*.intfb.h files, in double and in single precision (-ffp-contract=off).  Everything is built in a temporary directory outside the tree;
the reference's text is read by the compiler, never copied.  The fixture holds data only: the inputs (float32-representable, so that both
precisions see the same numbers), the two frequency tables, and what INTSPEC returned.  Only usable where the reference tree exists.

The mean frequencies are constructed so that STRSPEC's INT(LOG10(GAMMA)/LOG10(1.1)) is nowhere near a discontinuity
(tests/intspec_ref.py::make_cases, which the tests' 36-direction cases share).

    python tools/make_golden_nest.py <root of the reference tree> [number of cases]
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ecwam_amd.tables import Config, Tables  # noqa: E402
from intspec_ref import make_cases  # noqa: E402  (the construction of the inputs, shared with the tests)

if len(sys.argv) < 2:
    sys.exit(__doc__)
REF = sys.argv[1]
NCASE = int(sys.argv[2]) if len(sys.argv) > 2 else 96
NANG, NFRE = 12, 36
FLANG = shutil.which("amdflang") or "/opt/rocm/lib/llvm/bin/flang"
OUT = os.path.join(ROOT, "tests", "golden", "intspec_nang12.npz")


def cases(rng):
    t = Tables(Config(nang=NANG, nfre=NFRE, nfre_red=NFRE), np.float64)
    return make_cases(rng, NCASE, np.asarray(t.FR), np.asarray(t.TH))


def build(tmp, single):
    tag = "sp" if single else "dp"
    d = os.path.join(tmp, tag)
    os.makedirs(d)
    for h in ("rotspec.intfb.h", "strspec.intfb.h"):
        open(os.path.join(d, h), "w").close()
    flags = ["-cpp", "-O2", "-ffp-contract=off", "-module-dir", d, "-I", d] + (["-DSINGLE"] if single else [])
    objs = []
    for src in [os.path.join(ROOT, "tools", "intspec_driver.F90")] + [os.path.join(REF, "src", "ecwam", n) for n in ("rotspec.F90", "strspec.F90", "intspec.F90")]:
        o = os.path.join(d, os.path.basename(src).replace(".F90", ".o"))
        subprocess.run([FLANG, *flags, "-c", src, "-o", o], check=True)
        objs.append(o)
    exe = os.path.join(d, "intspec_driver")
    subprocess.run([FLANG, "-o", exe, *objs], check=True)
    return exe


def run(exe, tmp, fr, bfw, f, par):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.array([NCASE, NANG, NFRE], "<i4").tobytes())
        fh.write(np.asarray(fr, "<f8").tobytes())
        for i in range(NCASE):
            s = [bfw[i], par[i, 0, 2], par[i, 0, 0], par[i, 0, 1], par[i, 1, 2], par[i, 1, 0], par[i, 1, 1]]
            fh.write(np.asarray(s, "<f8").tobytes())
            fh.write(f[i, 0].astype("<f8").tobytes())      # [M][K] in C order = F(K,M) in Fortran order
            fh.write(f[i, 1].astype("<f8").tobytes())
    subprocess.run([exe, fin, fout], check=True)
    a = np.fromfile(fout, "<f8").reshape(NCASE, 3 + NANG * NFRE)
    return a[:, 3:].reshape(NCASE, NFRE, NANG), a[:, [1, 2, 0]]      # FL [M][K]; EMEAN, THQ, FMEAN


def main():
    rng = np.random.default_rng(20261019)
    bfw, f, par, form = cases(rng)
    fr = {p: np.asarray(Tables(Config(nang=NANG, nfre=NFRE, nfre_red=NFRE), dt).FR) for p, dt in (("sp", np.float32), ("dp", np.float64))}
    tmp = tempfile.mkdtemp(prefix="golden_nest_")
    try:
        out = {p: run(build(tmp, p == "sp"), tmp, fr[p], bfw, f, par) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    peak = np.abs(out["dp"][0]).max(axis=(1, 2))
    d = np.abs(out["sp"][0] - out["dp"][0]).max(axis=(1, 2)) / peak
    print(f"{NCASE} cases: single against double precision, per bin over the peak: max {d.max():.2e}, median {np.median(d):.2e}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, nang=NANG, nfre=NFRE, fr_sp=fr["sp"], fr_dp=fr["dp"], bfw=bfw, f=f, par=par, form=form,
                        fl_dp=out["dp"][0], par_dp=out["dp"][1], fl_sp=out["sp"][0].astype(np.float32), par_sp=out["sp"][1].astype(np.float32))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
