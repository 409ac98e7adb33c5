"""Generates tests/golden/ctu_<case>.npz and tests/golden/ctu_observed.json by RUNNING the reference's own corner-transport path with refraction and sub-grid
obstructions -- PROPDOT with GRADI, CTUWINI, CTUWDRV with CTUW, PROPAGS2 (src/ecwam/*.F90, unmodified) -- behind tools/ctu_driver.F90, built by
oracle/ref_build.py::build_driver with the reference's own modules in double and in single precision.  Everything is built in a temporary directory outside
the tree; the reference's text is read by the compiler, never copied.

The fixtures hold data only: per case what the routines returned in both precisions -- F3 over the owned points, THDD, THDC, SDOT at M = 1, 13 and 26, the
LCFLFAIL of the first CTUW call, CURMASK and the final LCFLFAIL (one column per CTUWDRV call).  The inputs are those of tests/ctu_ref.py::make_case, which the
tests rebuild.  The weights are too large to commit (21 per bin): the tool compares EVERY weight array of Oracle.ctu_weights_gen with the reference's bit
for bit, in memory, in both precisions, and writes the outcome per case to ctu_observed.json; tests/test_ctu_host.py requires it to be "all the same".

The tool asserts the coverage conditions of tests/ctu_ref.py::coverage on what the REFERENCE ALONE computed before it writes.  Only usable where the reference
tree exists.

    python tools/make_golden_ctu.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import propags_ref as P  # noqa: E402
import ctu_ref as CT  # noqa: E402  (the cases, their inputs and the coverage conditions, shared with the tests)
import golden_common as GC  # noqa: E402

ROUTINES = ("gradi", "propdot", "ctuwini", "ctuw", "ctuwdrv", "propags2")


def _col(a):      # C order [i][j][k] -> the bytes of the Fortran array A(I,J,K)
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(*range(a.ndim - 1, -1, -1)))


def run(exe, tmp, prec, names):
    """-> {case: the keys of ctu_ref.KEYS, WLAT, WCOR and the weight arrays} of the reference in precision prec"""
    T = CT.PREC[prec]
    g = P.fixture_grid()
    n, nang, nr = g.nsea, CT.NANG, CT.NFRE_RED
    first = CT.make_case(names[0], T)
    t = P.tables_of(T, nang, CT.NFRE, nr)
    sinth, costh = CT.direction_tables(prec)
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(GC.i([n, nang, nr, g.ngy]))
        fh.write(GC.r(first["fr"][:nr], sinth, costh, [first["delth"], first["r_earth"], first["zpi"], t.PI, first["xdella"], first["delphi"]]))
        fh.write(GC.r(first["zdello"], first["dellam"], first["sinph"], first["cosph"]))
        fh.write(GC.i(g.kxlt + 1, _col(g.klon + 1), _col(g.klat + 1), _col(g.kcor + 1)))
        fh.write(GC.r(_col(first["wlat"]), _col(first["wcor"]), first["cosphm1"]))
        for name in names:
            irefra, with_obs, ifm, amp = CT.CASES[name]
            c = CT.make_case(name, T)
            for k in ("zdello", "dellam", "sinph", "cosph", "wlat", "wcor", "cosphm1"):      # the grid is the same for every case
                assert P.same_bits(c[k], first[k]), k
            fh.write(GC.i([1, irefra, CT.IDELPRO, int(with_obs), 1, ifm]))
            fh.write(GC.r([CT.delpro_lf(name)], c["depth"], c["u"], c["v"]))
            fh.write(GC.r(_col(c["cg"][:, :nr]), _col(c["om"][:, :nr]), _col(c["wn"][:, :nr])))
            if with_obs:      # O8(N,NFRE_RED,8) from OBS[ij][8][NFRE]
                fh.write(GC.r(_col(c["obs"][:, :, :nr].transpose(0, 2, 1))))
            fh.write(GC.r(_col(c["f1"][:, :, :nr])))
        fh.write(GC.i([0]))
    a = GC.drive(exe, tmp)
    assert T(a[0]) == T(t.CIRC) and T(a[1]) == T(t.FRATIO), ("the reference's CIRC and FRATIO are not the tables'", a[:2])
    sizes = dict(f3=(nr, nang, n), thdd=(nang, n), thdc=(nang, n), sdot=(nr, nang, n), fail1=(2, n), curmask=(2, n), fail=(2, n), WLAT=(2, n), WCOR=(4, n),
                 SUMWN=(nr, nang, n), WLONN=(2, nr, nang, n), WLATN=(2, 2, nr, nang, n), WCORN=(2, 4, nr, nang, n), WKPMN=(3, nr, nang, n), WMPMN=(3, nr, nang, n))
    out, pos = {}, 2
    for name in names:
        d = {}
        for k, shp in sizes.items():
            cnt = int(np.prod(shp))
            d[k] = np.ascontiguousarray(a[pos:pos + cnt].reshape(shp).transpose(*range(len(shp) - 1, -1, -1))).astype(T)
            pos += cnt
        d["sdot"] = np.ascontiguousarray(d["sdot"][:, :, [m - 1 for m in CT.SDOT_M]])
        d["fail1"], d["fail"] = d["fail1"].astype(np.int8), d["fail"].astype(np.int8)
        out[name] = d
    assert pos == a.size, (pos, a.size)
    return out


def main():
    ref_root, out = GC.arguments(__doc__, CT.GOLDEN)
    tmp = tempfile.mkdtemp(prefix="golden_ctu_")
    names = list(CT.CASES)
    try:
        exe = GC.executables(ref_root, "ctu", ROUTINES, tmp, standins=("OML_MOD",))
        ref = {p: run(exe[p], tmp, p, names) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    observed = {"grid": CT.grid_coverage(), "idelpro": CT.IDELPRO, "cases": {}}
    total = 0
    for name in names:
        per = {p: ref[p][name] for p in CT.PREC}
        other = {p: ref[p][CT.UNOBSTRUCTED[name]] for p in CT.PREC} if name in CT.UNOBSTRUCTED else None
        obs = CT.coverage(name, per, other)      # on the reference alone
        # the oracle's weights against the reference's, every array, bit for bit, and what the fixtures hold as well
        for p in CT.PREC:
            o = CT.oracle_run(name, p)
            same = {k: bool(P.same_bits(o["w"][k], per[p][k])) for k in CT.WEIGHTS + ("WLAT", "WCOR")}
            same.update({k: bool(P.same_bits(o[k], per[p][k])) for k in CT.KEYS})
            obs[p]["oracle_bit_identical"] = same
            if not all(same.values()):
                for k, ok in same.items():
                    if not ok:
                        a, b = (o["w"][k] if k in o["w"] else o[k]).astype(np.float64), per[p][k].astype(np.float64)
                        print(f"{name} {p} {k}: {int((a != b).sum())} of {a.size} differ, largest {np.abs(a - b).max():.3e} (scale {np.abs(b).max():.3e})", file=sys.stderr)
        observed["cases"][name] = obs
        arrays = {f"{k}_{p}": per[p][k] for p in CT.PREC for k in CT.KEYS}
        GC.write_npz(out, f"ctu_{name}.npz", arrays)
        total += os.path.getsize(os.path.join(out, f"ctu_{name}.npz"))
    observed["note"] = ("per case and precision: the largest and smallest SUMWN of the plain cases, the fraction of zeros of WKPMN(+-1) and WMPMN(+-1), the points the "
                        "first CTUW call failed and the second masked, the fraction of bins the obstructions lowered, and whether the oracle reproduced each "
                        "weight array and each recorded array bit for bit")
    GC.write_observed(out, "ctu_observed.json", observed)
    print("fixtures:", total, "bytes")


if __name__ == "__main__":
    main()
