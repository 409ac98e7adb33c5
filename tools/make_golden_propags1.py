"""Generates tests/golden/propags1_<case>.npz and tests/golden/propags1_observed.json by RUNNING the reference's own PROPCONNECT (IPROPAGS = 1), PROPAGS1,
PROPDOT and GRADI (src/ecwam/*.F90, unmodified) behind tools/propags1_driver.F90, built by oracle/ref_build.py::build_driver with the reference's own
modules in double and in single precision.  Everything is built in a temporary directory outside the tree; the reference's text is read by the compiler,
never copied.  The driver supplies an external CHECKCFL that records its eleven arguments per (K, M = 1) instead of aborting, and restates the few
statements of mpdecomp.F90 that turn PROPCONNECT's 0 into the land index and fill CDR, SDR and PRQRT (its header says which).

The fixtures hold data only, per case and precision: the tables of the case's grid (KLAT, KLON, KRLAT, KRLON 0-based, WLAT, WRLAT, WRLON, CDR, SDR, PRQRT,
SQRT2), F3, the recorded CFL numbers and the number of CHECKCFL calls.  The inputs are those of tests/propags1_ref.py::make_case (propags_ref.make_inputs
with its defaults; every field rounded to single precision), which the tests rebuild.  Grids: the O3 grid of the propags_* fixtures (61 sea points) and,
for PRQRT < 0.5, an O5 grid (117 sea points, NFRE_RED 13).

The tool asserts the coverage conditions of tests/propags1_ref.py on what the REFERENCE ALONE computed, counts the entries of PROPCONNECT's KLAT and KLON
that differ from the grid's (ties of the second closest point, which the increments rounded to single precision break the other way; PROPAGS1 runs with the
grid's), and writes what it observed to propags1_observed.json: the conditions, the distance of ecwam_amd.grid.rotated_tables from the recorded CDR, SDR, PRQRT
and SQRT2 in units in the last place, whether tests/propags1_ref.py reproduced F3 and CFL bit for bit, and the number of bins in which section 4 differs
from the IPROPAGS = 0 fixture.  Only usable where the reference tree exists.

    python tools/make_golden_propags1.py <root of the reference tree> [<directory to write to; default tests/golden>]
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
import propags1_ref as P1  # noqa: E402
import golden_common as GC  # noqa: E402
from ecwam_amd import grid as G  # noqa: E402

ROUTINES = ("propags1", "propconnect", "propdot", "gradi")
PREC = P1.PREC


def _col(a):      # C order [i][j][k] -> the bytes of the Fortran array A(I,J,K)
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(*range(a.ndim - 1, -1, -1)))


def _row(a, shp):      # the values of the Fortran array A(shp reversed) -> C order
    return np.ascontiguousarray(a.reshape(shp).transpose(*range(len(shp) - 1, -1, -1)))


def run(exe, tmp, prec, key, names):
    """-> the tables of grid `key` and {case: dict(f3, cfl, ncall)} of the reference in precision prec"""
    T = PREC[prec]
    g = P1.fixture_grid(key)
    first = P1.make_case(names[0], T)
    n, nang, nr = g.nsea, P1.NANG, first["nr"]
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(GC.i([n, nang, nr, g.ngy]))
        fh.write(GC.r(first["fr"][:nr], first["sinth"], first["costh"], [first["delth"], first["r_earth"], first["zpi"], P.tables_of(T).PI]))
        fh.write(GC.i(g.nlonrgg, g.ixlg + 1, g.kxlt + 1, _col(g.klon + 1), _col(g.klat + 1)))
        fh.write(GC.r([first["xdella"], first["delphi"]], first["zdello"], first["dellam"], first["sinph"], first["cosph"], _col(first["wlat"])))
        for name in names:
            c = P1.make_case(name, T)
            assert c["nr"] == nr
            fh.write(GC.i([1, c["icase"], c["irgg"], c["irefra"], int(c["delpro"]), int(c["obs"] is not None)]))
            fh.write(GC.r(c["dellam1"], c["cosphm1"], c["depth"], c["u"], c["v"]))
            fh.write(GC.r(_col(c["cg"][:, :nr]), _col(c["om"][:, :nr]), _col(c["wn"][:, :nr])))
            if c["obs"] is not None:      # OBSLAT, OBSLON, OBSRLAT, OBSRLON (N,NFRE_RED,2) from OBS[ij][8][NFRE]
                fh.write(GC.r(*(_col(c["obs"][:, j:j + 2, :nr].transpose(0, 2, 1)) for j in (0, 2, 4, 6))))
            fh.write(GC.r(_col(c["f1"][:, :, :nr])))
        fh.write(GC.i([0]))
    a = GC.drive(exe, tmp)
    pos = 0

    def take(shp):
        nonlocal pos
        cnt = int(np.prod(shp))
        out = _row(a[pos:pos + cnt], shp)
        pos += cnt
        return out
    tab = {}
    for k, shp in (("klat", (2, 2, n)), ("klon", (2, n)), ("krlat", (2, 2, n)), ("krlon", (2, 2, n))):
        tab[k] = (take(shp) - 1).astype(np.int32)
    for k, shp in (("wlat", (2, n)), ("wrlat", (2, n)), ("wrlon", (2, n)), ("cdr", (nang, n + 1)), ("sdr", (nang, n + 1)), ("prqrt", (n,)), ("sqrt2", (1,))):
        tab[k] = take(shp).astype(T)
    out = {}
    for name in names:
        out[name] = dict(f3=take((nr, nang, n)).astype(T), cfl=take((P.NCFL, nang, n)).astype(T), ncall=take((1,)).astype(np.int32))
    assert pos == a.size, (pos, a.size)
    return tab, out


def main():
    ref_root, out = GC.arguments(__doc__, P.GOLDEN)
    tmp = tempfile.mkdtemp(prefix="golden_propags1_")
    groups = {}
    for name, case in P1.CASES.items():
        groups.setdefault(case[0], []).append(name)
    try:
        exe = GC.executables(ref_root, "propags1", ROUTINES, tmp)
        ref = {(p, key): run(exe[p], tmp, p, key, names) for p in PREC for key, names in groups.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    observed = {"cases": {}, "grid": {}, "tables_ulp": {}}
    ulp = {k: 0 for k in ("cdr", "sdr", "prqrt", "sqrt2")}
    for key in groups:
        g = P1.fixture_grid(key)
        observed["grid"][key] = {"points": int(g.nsea)}
        for p, T in PREC.items():
            tab = ref[(p, key)][0]
            # PROPAGS1 ran with the grid's KLAT, KLON (the driver's header): how far PROPCONNECT's, formed in the working precision, are from them
            differ = {k: int((tab[k] != getattr(g, k)).sum()) for k in ("klat", "klon")}
            observed["grid"][key][p] = P1.table_coverage(key, tab, g.nsea)
            observed["grid"][key][p]["entries_differing_from_input"] = differ
            observed["grid"][key][p]["wlat_max_distance_from_input"] = float(np.abs(tab["wlat"].astype(np.float64) - P._f32(g.wlat)).max())
            t = P.tables_of(T)
            mine = G.rotated_tables(P1.rounded_grid(g), T, np.asarray(t.SINTH, T), np.asarray(t.COSTH, T))
            for k in ("krlat", "krlon", "wrlat", "wrlon"):
                assert P.same_bits(np.ascontiguousarray(mine[k]), tab[k]), (key, p, k)
            for k in ulp:
                a, b = np.atleast_1d(np.asarray(mine[k], T)), np.atleast_1d(tab[k])
                if k in ("cdr", "sdr"):
                    assert np.array_equal(np.signbit(a), np.signbit(b)) and np.array_equal(a < 0, b < 0), (key, p, k)
                ulp[k] = max(ulp[k], P1.ulps(a, b))
    observed["tables_ulp"] = ulp
    total = 0
    for name, case in P1.CASES.items():
        key, icase, irgg, irefra, with_obs, idelpro, nr = case
        arrays = {}
        for p, T in PREC.items():
            tab, res = ref[(p, key)]
            r = res[name]
            assert int(r["ncall"][0]) == (P1.NANG if icase == 1 else 0), (name, p, r["ncall"])
            for k in P1.TABLES:
                arrays[f"{k}_{p}"] = tab[k]
            for k in ("f3", "cfl", "ncall"):
                arrays[f"{k}_{p}"] = r[k]
        other = {f"f3_{p}": ref[(p, key)][1][P1.UNOBSTRUCTED[name]]["f3"] for p in PREC} if name in P1.UNOBSTRUCTED else None
        obs = P1.case_coverage(name, arrays, other)
        obs.update(grid=key, icase=icase, irgg=irgg, irefra=irefra, obstructions=with_obs, idelpro=idelpro, nfre_red=nr, bit_identical={})
        for p, T in PREC.items():
            c = P1.make_case(name, T)
            mine = P1.restate(c, T, P1.recorded_rot(arrays, p))
            obs["bit_identical"][p] = {k: bool(P.same_bits(mine[k], arrays[f"{k}_{p}"])) for k in ("f3", "cfl")}
            if name in P1.PROPAGS0:
                f0 = P.load_fixture(P1.PROPAGS0[name])[f"f3_{p}"]
                obs.setdefault("bins_differing_from_ipropags0", {})[p] = int((f0 != arrays[f"f3_{p}"]).sum())
        observed["cases"][name] = obs
        GC.write_npz(out, f"propags1_{name}.npz", arrays)
        total += os.path.getsize(os.path.join(out, f"propags1_{name}.npz"))
    observed["note"] = ("grid: per grid and precision the neighbours of the four rotated positions (closest is land, exactly one of two is land, two distinct sea "
                        "points), the fraction of points with a weight strictly inside (0, 1), PRQRT, the fraction of (IJ, K) with IJRLA, IJRPH = 2; tables_ulp: the "
                        "largest distance of ecwam_amd.grid.rotated_tables from the recorded table; cases: the largest recorded CFL number, the points where one "
                        "exceeds 1, whether tests/propags1_ref.py reproduced F3 and CFL bit for bit, the bins of F3 that differ from the IPROPAGS = 0 fixture")
    GC.write_observed(out, "propags1_observed.json", observed)
    print("fixtures:", total, "bytes")


if __name__ == "__main__":
    main()
