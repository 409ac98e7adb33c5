"""Generates tests/golden/propags_<case>.npz and tests/golden/propags_observed.json by RUNNING the reference's own PROPAGS, PROPDOT and GRADI
(src/ecwam/*.F90, unmodified) behind tools/propags_driver.F90, built by oracle/ref_build.py::build_driver with the reference's own modules in double and
in single precision.  Everything is built in a temporary directory outside the tree; the reference's text is read by the compiler, never copied.  The
driver supplies one routine in place of the reference's: an external CHECKCFL that records its eleven arguments per (K, M = 1) instead of aborting, so
that the CFL numbers of the unmodified PROPAGS are had, those above 1 included.

The fixtures hold data only: per case what the routines returned in both precisions -- F3, THDD, THDC, SDOT and the recorded CFL numbers.  The inputs are
those of tests/propags_ref.py::make_case, which the tests rebuild (every field is rounded to single precision, so that both precisions see the same
numbers).  The grid is an O3 octahedral grid with pseudo-continents: 61 sea points and the land slot, NANG 12, NFRE 36, NFRE_RED 25.

The tool asserts the coverage conditions of tests/propags_ref.py::coverage on what the REFERENCE ALONE computed (the upwind weights are those of the
restatement only where the restatement has reproduced the reference's F3 and CFL numbers bit for bit, which the tool requires first), and writes the
branches taken to propags_observed.json.  Only usable where the reference tree exists.

    python tools/make_golden_propags.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import propags_ref as P  # noqa: E402  (the construction of the inputs and the restatement, shared with the tests)
import golden_common as GC  # noqa: E402

ROUTINES = ("propags", "propdot", "gradi")
PREC = {"sp": np.float32, "dp": np.float64}


def _col(a):      # C order [i][j][k] -> the bytes of the Fortran array A(I,J,K)
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(*range(a.ndim - 1, -1, -1)))


def run(exe, tmp, prec, names):
    """-> {case: dict(f3, thdd, thdc, sdot, cfl)} of the reference in precision prec"""
    T = PREC[prec]
    g = P.fixture_grid()
    n, nang, nr = g.nsea, P.NANG, P.NFRE_RED
    first = P.make_case(names[0], T)
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(GC.i([n, nang, nr, g.ngy]))
        fh.write(GC.r(first["fr"][:nr], first["sinth"], first["costh"], [first["delth"], first["r_earth"], first["zpi"], P.tables_of(T).PI]))
        fh.write(GC.i(g.kxlt + 1, _col(g.klon + 1), _col(g.klat + 1)))
        for name in names:
            c = P.make_case(name, T)
            fh.write(GC.i([1, c["icase"], c["irgg"], c["irefra"], int(c["delpro"]), int(c["obs"] is not None)]))
            fh.write(GC.r([c["delphi"]], c["dellam"], c["sinph"], c["cosph"], _col(c["wlat"])))
            fh.write(GC.r(c["dellam1"], c["cosphm1"], c["depth"], c["u"], c["v"]))
            fh.write(GC.r(_col(c["cg"][:, :nr]), _col(c["om"][:, :nr]), _col(c["wn"][:, :nr])))
            if c["obs"] is not None:      # OBSLAT(N,NFRE_RED,2), OBSLON(N,NFRE_RED,2) from OBS[ij][8][NFRE]
                fh.write(GC.r(_col(c["obs"][:, 0:2, :nr].transpose(0, 2, 1)), _col(c["obs"][:, 2:4, :nr].transpose(0, 2, 1))))
            fh.write(GC.r(_col(c["f1"][:, :, :nr])))
        fh.write(GC.i([0]))
    a = GC.drive(exe, tmp)
    sizes = dict(f3=(nr, nang, n), thdd=(nang, n), thdc=(nang, n), sdot=(nr, nang, n), cfl=(P.NCFL, nang, n), ncall=(1,))
    out, pos = {}, 0
    for name in names:
        d = {}
        for k, shp in sizes.items():
            cnt = int(np.prod(shp))
            d[k] = np.ascontiguousarray(a[pos:pos + cnt].reshape(shp).transpose(*range(len(shp) - 1, -1, -1))).astype(T)
            pos += cnt
        assert np.array_equal(d[k], d[k])
        out[name] = d
    assert pos == a.size, (pos, a.size)
    return out


def main():
    ref_root, out = GC.arguments(__doc__, P.GOLDEN)
    tmp = tempfile.mkdtemp(prefix="golden_propags_")
    names = list(P.CASES)
    observed = {"cases": {}, "grid": {}}
    try:
        exe = GC.executables(ref_root, "propags", ROUTINES, tmp)
        ref = {p: run(exe[p], tmp, p, names) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    observed["grid"] = P.grid_coverage(P.fixture_grid())
    total = 0
    for name in names:
        icase, irgg, irefra, with_obs, idelpro = P.CASES[name]
        arrays = {}
        for p, T in PREC.items():
            r = ref[p][name]
            assert int(r["ncall"][0]) == (P.NANG if icase == 1 else 0), (name, p, r["ncall"])
            for k in ("f3", "thdd", "thdc", "sdot", "cfl"):
                if k == "sdot" and irefra not in (2, 3):
                    continue
                arrays[f"{k}_{p}"] = r[k]
        other = {f"{k}_{p}": ref[p][P.UNOBSTRUCTED[name]][k] for p in PREC for k in ("f3",)} if name in P.UNOBSTRUCTED else None
        observed["cases"][name] = P.coverage(name, arrays, other)
        GC.write_npz(out, f"propags_{name}.npz", arrays)
        total += os.path.getsize(os.path.join(out, f"propags_{name}.npz"))
    observed["note"] = ("per case: the section of PROPAGS taken, the fraction of zeros of every upwind weight of the section, the largest recorded CFL number and "
                        "the points where one exceeds 1 (both precisions), whether the restatement reproduced every recorded quantity bit for bit")
    GC.write_observed(out, "propags_observed.json", observed)
    print("fixtures:", total, "bytes")


if __name__ == "__main__":
    main()
