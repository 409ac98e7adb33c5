"""Generates tests/golden/readwind_0.npz and tests/golden/readwind_observed.json by RUNNING the reference's own GRIB2WGRID (src/ecwam/grib2wgrid.F90,
with adjust.F90, incdate.F90 and wstream_strg.F90) behind tools/readwind_driver.F90, built by oracle/ref_build.py::build_driver in double and in
single precision.  The routine asks a stand-in GRIB decoder
(a YOWGRIB that answers the keys from a table) for the message; READWIND's fill and CURRENT2WAM's three statements are bound to files and to the
message passing library, so the driver restates those few statements around the reference's FIELD.  Everything is built in a temporary directory
outside the tree; the reference's text is read by the compiler, never copied.  The fixture holds outputs only, per case and precision: FIELD of the
three fields, FIELDG after READWIND's eight parameters, the two currents and their FIELDs, and IPARAM, IFORP, CDATE, KZLEV per message; the inputs
are those of tests/readwind_ref.py::make_cases, which the tests rebuild (float32-representable, so that both precisions see the same numbers).
Only usable where the reference tree exists.

The tool stops, naming what it missed, unless some cell takes every branch of tests/readwind_ref.py::BRANCHES, the pattern of PMISS of the
restated chain is the reference's in both precisions, and HYPOT(WK(1), WK(2)) >= 0.1 in every interpolated direction cell.  No case is dropped.
It then writes the observed figures the tests take their gates from, per case and field:
  restatement_vs_reference_dp  the restated chain (readwind.input_grid -> readwind.cell_table -> tests/readwind_ref.py::interpolate) in float64
                               against the double precision results
  restatement_vs_reference_sp  the same in single precision
  reference_sp_vs_dp           the reference's own single against its double precision results
each |a - b| / max(|b|, the plane's largest |b|) over the cells that are not PMISS; a direction: the difference on the circle over its period.

    python tools/make_golden_readwind.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import readwind_ref as F  # noqa: E402  (the construction of the inputs and the restatement, shared with the tests)
import golden_common as GC  # noqa: E402

REF, OUT = GC.arguments(__doc__, F.GOLDEN)
ROUTINES = ("grib2wgrid", "adjust", "incdate", "wstream_strg")
_r, _i = GC.r, GC.i


def _name(s, n=40):
    return s.encode().ljust(n)


def _message(keys, values):
    """the key table of the stand-in decoder for one message"""
    ints = {k: v for k, v in keys.items() if isinstance(v, (int, np.integer))}
    reals = {k: v for k, v in keys.items() if isinstance(v, float)}
    chars = {k: v for k, v in keys.items() if isinstance(v, str)}
    pl = keys.get("pl")
    ints["getNumberOfValues"] = len(values)
    ints["PLPresent"] = int(pl is not None)
    if pl is not None:
        ints["numberOfPointsAlongAMeridian"] = len(pl)
    b = _i(len(ints)) + b"".join(_name(k) + _i(v) for k, v in ints.items())
    b += _i(len(reals)) + b"".join(_name(k) + _r(v) for k, v in reals.items())
    b += _i(len(chars)) + b"".join(_name(k) + _name(v, 12) for k, v in chars.items())
    b += _i(0) if pl is None else _i(len(pl), pl)
    return b + _i(len(values)) + _r(values)


def run(exe, tmp, prec, c):
    """-> {case: {key: array}} of one precision"""
    T = F.dtype_of(prec)
    order = []
    with open(GC.infile(tmp), "wb") as fh:
        fh.write(_i(F.NX, F.NY, F.NROW, F.KLONRGG, c["ifromij"], c["jfromij"]) + _r(c["xlon"], c["ylat"], F.PMISS, F.ROAIR, F.WSTAR0, F.WLOWEST, F.CURRENT_MAX, F.SENT))
        for name in F.CASES:
            fh.write(_i(2))
            for key, param, wave, _, v in F.messages(c, name):
                post = 1 if key.startswith("fg_") else 2 if key in ("ucur", "vcur") else 0
                fh.write(_i(1, post, 1, 1, 1) + _message(F.message_keys(c, name, param, wave), v))
                order.append((name, key))
            fh.write(_i(3))
            order.append((name, None))
        fh.write(_i(0))
    flat = GC.drive(exe, tmp)
    res, at = {n: {} for n in F.CASES}, 0

    def take(n, kind=T):
        nonlocal at
        a = flat[at:at + n]
        at += n
        out = np.ascontiguousarray(a, dtype=kind)
        assert np.array_equal(out.astype(np.float64), a)      # nothing is lost by narrowing what the driver widened
        return out
    for name, key in order:
        if key is None:
            res[name]["fieldg"] = take(13 * F.NCELL).reshape(13, F.NCELL)
            res[name]["ucur"], res[name]["vcur"] = take(F.NROW), take(F.NROW)
        else:
            f = take(F.NCELL)
            res[name]["meta_" + key] = take(4, np.int64)      # IPARAM, IFORP, CDATE, KZLEV
            if not key.startswith("fg_"):
                res[name][("field_" + key) if key in ("ucur", "vcur") else key] = f
    assert at == flat.size, (at, flat.size)
    return res


def main():
    tmp = tempfile.mkdtemp(prefix="golden_readwind_")
    try:
        c = F.make_cases()
        exe = GC.executables(REF, "readwind", ROUTINES, tmp, standins=("YOWGRIB",))
        ref = {p: run(exe[p], tmp, p, c) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kinds = ("restatement_vs_reference_dp", "restatement_vs_reference_sp", "reference_sp_vs_dp")
    obs = {k: {n: {} for n in F.CASES} for k in kinds}
    taken, cond = set(), np.inf
    for name in F.CASES:
        for wave in (False, True):      # one table serves the messages of both kinds of stream
            for p in ("dp", "sp"):
                a, b = F.table(name, p, False)[1], F.table(name, p, wave)[1]
                assert all(np.array_equal(a[k], b[k]) for k in ("pos", "kind")) and (a["w"] is None or np.array_equal(a["w"], b["w"])), (name, p)
        own = {}
        for p in ("dp", "sp"):
            own[p], tk, cd = F.chain(p, name)
            if p == "dp":
                taken |= {f"{name}:{t}" for t in tk}
                cond = min(cond, cd)
        assert np.array_equal(F.table(name, "dp")[1]["pos"], F.table(name, "sp")[1]["pos"]) and np.array_equal(F.table(name, "dp")[1]["kind"],
                                                                                                            F.table(name, "sp")[1]["kind"]), name
        for p in ("dp", "sp"):
            for key, mine in F.fixture_items(name, own[p]):
                theirs = dict(F.fixture_items(name, ref[p][name]))[key]
                if not F.same_pattern(mine, theirs):
                    raise SystemExit(f"case {name} {key} {p}: the restated chain and the reference differ in where FIELD is PMISS")
                obs[f"restatement_vs_reference_{p}"][name][key] = F.error(key, mine, theirs)
            keep = own[p]["fieldg"] == F.dtype_of(p)(F.SENT)
            assert np.array_equal(keep, ref[p][name]["fieldg"] == F.dtype_of(p)(F.SENT)), (name, p)      # the same cells and planes are left alone
        for key, sp in F.fixture_items(name, ref["sp"][name]):
            dp = dict(F.fixture_items(name, ref["dp"][name]))[key]
            if not F.same_pattern(sp, dp):
                raise SystemExit(f"case {name} {key}: the single and the double precision reference differ in where FIELD is PMISS")
            obs["reference_sp_vs_dp"][name][key] = F.error(key, sp, dp)
        print(name, " ".join(f"{k} {obs['restatement_vs_reference_dp'][name][k]:.1e}/{obs['restatement_vs_reference_sp'][name][k]:.1e}/"
                             f"{obs['reference_sp_vs_dp'][name][k]:.1e}" for k in obs["reference_sp_vs_dp"][name]))
    missing = [b for b in F.BRANCHES if not any(t.endswith(":" + b) for t in taken)]
    if missing:
        raise SystemExit(f"no cell takes the branches {missing}: change the inputs of tests/readwind_ref.py::make_cases")
    if not cond >= 0.1:
        raise SystemExit(f"an interpolated direction cell is ill-conditioned: HYPOT(WK(1), WK(2)) = {cond}")
    arrays = {}
    for p in ("dp", "sp"):
        for name in F.CASES:
            for key, a in ref[p][name].items():
                if key.startswith("meta_"):
                    assert np.array_equal(a, ref["dp"][name][key])
                    arrays[f"{key}_{name}"] = a
                else:
                    arrays[f"{key}_{name}_{p}"] = a
    GC.write_npz(OUT, "readwind_0.npz", arrays)
    obs["branches"] = sorted(taken)
    obs["smallest_direction_vector"] = cond
    obs["error_measure"] = ("per field: |a - b| / max(|b|, the field's largest |b|) over the cells that are not PMISS, the maximum; dir and fg_WDWAVE: the "
                            "difference on the circle over the period (360 degrees, 2 pi)")
    GC.write_observed(OUT, "readwind_observed.json", obs)


if __name__ == "__main__":
    main()
