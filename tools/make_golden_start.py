"""Generates tests/golden/start_<NANG>x<NFRE_RED>_<i>.npz and tests/golden/start_observed.json by RUNNING the reference's own MSTART, PEAK,
SPECTRA, JONSWAP, SPR, UNSETICE, SDEPTHLIM and SEMEAN (src/ecwam/*.F90) behind tools/start_driver.F90, built by
oracle/ref_build.py::build_driver with the reference's own modules in double and in single precision.
Everything is built in a temporary directory outside the tree; the reference's text is read by the compiler, never copied.  The fixtures
hold data only: the two frequency tables and what the routines returned on the active rows, per call (tests/start_ref.py::calls); the
inputs are those of tests/start_ref.py::make_cases, which the tests rebuild (float32-representable, so that both precisions see the same
numbers).  Only usable where the reference tree exists.

The tail of GETSPEC (getspec.F90:648-659) sits inside a routine that reads GRIB files: for that fixture the driver restates the fill loop
(three lines) and calls the reference's SDEPTHLIM on the result, as GETSPEC does.

The tool asserts that the single and the double precision reference took the same branch at every point -- the decisions of the routines
evaluated in both precisions on the inputs (the wind test, the reset of UNSETICE, its depth class, the sign of every cosine and SPR's cut,
which side of 1 SDEPTHLIM's EMAXDPT / EM falls) and the sets of bins the two results give as exactly 0 and as exactly EPSMIN -- and fails if
they did not: no case is dropped.  It then writes the observed figures the tests take their gates from:
  restatement_vs_reference_dp  per routine, the largest difference between tests/start_ref.py in float64 and the double precision results
  restatement_vs_reference_sp  the same in single precision (reported; no gate comes from it)
  reference_sp_vs_dp           per routine, the largest difference between the reference's own single and double precision results
each per bin over the point's largest bin.  A result is split over files so that none exceeds 0.6 MB.  A shape with NFRE_RED < NFRE shares the
inputs of MSTART and UNSETICE with the full shape (neither routine knows NFRE_RED): the tool runs them, requires the same results and records
the tail only.

    python tools/make_golden_start.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import glob
import io
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import start_ref as S  # noqa: E402  (the construction of the inputs and the restatement, shared with the tests)
import golden_common as GC  # noqa: E402

REF, OUT = GC.arguments(__doc__, S.GOLDEN)
LIMIT = GC.LIMIT
ROUTINES = ("semean", "sdepthlim", "jonswap", "spr", "peak", "spectra", "mstart", "unsetice")
A = slice(S.KIJS, S.KIJL)


def _f(a):      # [ij][K][M] -> the bytes of FL1(IJ,K,M)
    return np.ascontiguousarray(np.asarray(a, "<f8").transpose(2, 1, 0)).tobytes()


def run(exe, tmp, shape, prec, cases):
    nang, nfre, nfre_red = shape
    T = np.float32 if prec == "sp" else np.float64
    n = S.KIJL - S.KIJS
    names = S.calls(shape)
    with open(GC.infile(tmp), "wb") as fh:
        t = S.tables(shape, T)
        fh.write(np.array([n, nang, nfre], "<i4").tobytes())
        for a in (t.FR, t.TH, t.DFIM, t.FR5):
            fh.write(np.asarray(a, "<f8").tobytes())
        fh.write(np.asarray([t.G, t.PI, t.ZPI, t.ZPI4GM2, t.EPSMIN, t.DELTH, t.WETAIL, t.FLMIN], "<f8").tobytes())
        for name in names:
            r, c = S.routine_of(name), cases[S.routine_of(name)]
            ff = c["ff"][A]
            if r == "mstart":
                fh.write(np.array([1, int(name[-1])], "<i4").tobytes())
                fh.write(np.asarray(c["params"], "<f8").tobytes())
                fh.write(np.asarray(ff[:, S.C_WSWAVE], "<f8").tobytes() + np.asarray(ff[:, S.C_WDWAVE], "<f8").tobytes())
            elif r == "unsetice":
                lrun, lmask, lbiwbk, which = S.variant(name)
                tv = S.tables(shape, T, lrun, lmask, lbiwbk)
                fh.write(np.array([2, lrun, lmask, lbiwbk], "<i4").tobytes())
                fh.write(np.asarray([tv.CITHRSH, S.DELPHI[which]], "<f8").tobytes())
                for col in (S.C_DEPTH, S.C_EMAXDPT, S.C_WDWAVE, S.C_WSWAVE, S.C_CICOVER):
                    fh.write(np.asarray(ff[:, col], "<f8").tobytes())
                fh.write(_f(c["fl"][A]))
            else:
                fh.write(np.array([3, nfre_red], "<i4").tobytes())
                fh.write(np.asarray(ff[:, S.C_EMAXDPT], "<f8").tobytes())
                fh.write(_f(c["fl"][A]))
        fh.write(np.array([0], "<i4").tobytes())
    a = GC.drive(exe, tmp).reshape(len(names), nfre, nang, n).transpose(0, 3, 2, 1)
    return {name: np.ascontiguousarray(a[i]) for i, name in enumerate(names)}


def same_branches(shape, cases, ref):
    """Fails unless both precisions decide alike everywhere (the module docstring lists the decisions)."""
    tag = S.shape_tag(shape)
    t = {p: S.tables(shape, T) for p, T in (("sp", np.float32), ("dp", np.float64))}
    for name in S.calls(shape):
        r, c = S.routine_of(name), cases[S.routine_of(name)]
        ff = c["ff"][A]
        dec = {}
        for p, T in (("sp", np.float32), ("dp", np.float64)):
            cosd = np.cos(t[p].TH[None, :] - ff[:, S.C_WDWAVE].astype(T)[:, None])
            d = [cosd > 0, S.spr(t[p], ff[:, S.C_WDWAVE].astype(T)) > 0, ff[:, S.C_WSWAVE].astype(T) > T(0.1e-08)]
            if r == "mstart":
                d.append(S.spr(t[p], np.full(1, T(c["params"][2]))) > 0)
            if r == "unsetice":
                lrun, lmask, lbiwbk, which = S.variant(name)
                d += list(S.unsetice_branches(S.tables(shape, T, lrun, lmask, lbiwbk), c["fl"][A].astype(T), ff[:, S.C_DEPTH], ff[:, S.C_WSWAVE], ff[:, S.C_CICOVER]))
            if r == "tail" or (r == "unsetice" and S.variant(name)[2]):
                d.append(ff[:, S.C_EMAXDPT].astype(T) / S.pre_limit_energy(shape, name, p, cases) < T(1))
            dec[p] = d
            dec[p] += [ref[p][name] == 0, ref[p][name] == float(t[p].EPSMIN)]
        for i, (a, b) in enumerate(zip(dec["sp"], dec["dp"])):
            if not np.array_equal(a, b):
                raise SystemExit(f"{tag} {name}: the single and the double precision reference differ in decision {i} at "
                                 f"{int((np.asarray(a) != np.asarray(b)).sum())} places: widen the margins of tests/start_ref.py::make_cases")


def write_split(tag, arrays):
    """The arrays into start_<tag>_<i>.npz, a new file whenever the one at hand would pass LIMIT."""
    for old in glob.glob(os.path.join(OUT, f"start_{tag}_*.npz")):
        os.remove(old)
    files, cur = [], {}

    def size(d):
        b = io.BytesIO()
        np.savez_compressed(b, **d)
        return b.getbuffer().nbytes

    for k, v in arrays.items():
        if cur and size({**cur, k: v}) > LIMIT:
            files.append(cur)
            cur = {}
        cur[k] = v
        if size(cur) > LIMIT:
            raise SystemExit(f"{tag} {k}: one array alone exceeds {LIMIT} bytes")
    files.append(cur)
    total = 0
    for i, d in enumerate(files):
        path = os.path.join(OUT, f"start_{tag}_{i}.npz")
        np.savez_compressed(path, **d)
        total += os.path.getsize(path)
        print(path, os.path.getsize(path), "bytes", sorted(d))
    return total


def main():
    tmp = tempfile.mkdtemp(prefix="golden_start_")
    obs = {k: {} for k in ("restatement_vs_reference_dp", "restatement_vs_reference_sp", "reference_sp_vs_dp")}
    per_call = {}
    total = 0
    recorded = {}
    try:
        exe = GC.executables(REF, "start", ROUTINES, tmp)
        for shape in S.SHAPES:
            cases = S.make_cases(shape)
            ref = {p: run(exe[p], tmp, shape, p, cases) for p in ("dp", "sp")}
            same_branches(shape, cases, ref)
            tag = S.shape_tag(shape)
            recorded[shape] = ref
            full = recorded.get(S.full_shape(shape)) if shape != S.full_shape(shape) else None
            arrays = dict(fr_sp=np.asarray(S.tables(shape, np.float32).FR), fr_dp=np.asarray(S.tables(shape, np.float64).FR))
            for name in S.calls(shape):
                r = S.routine_of(name)
                figs = dict(restatement_vs_reference_dp=S.bin_error(S.restate(shape, name, "dp", cases), ref["dp"][name]).max(),
                            restatement_vs_reference_sp=S.bin_error(S.restate(shape, name, "sp", cases), ref["sp"][name]).max(),
                            reference_sp_vs_dp=S.bin_error(ref["sp"][name], ref["dp"][name]).max())
                for k, v in figs.items():
                    obs[k][r] = max(obs[k].get(r, 0.0), float(v))
                per_call[f"{tag} {name}"] = {k: float(v) for k, v in figs.items()}
                print(tag, name, " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
                if full is not None and r != "tail":      # the same inputs gave the same results: recorded once, with the full shape
                    assert all(np.array_equal(ref[p][name], full[p][name]) for p in ("dp", "sp")), (tag, name)
                    continue
                arrays[f"{name}_dp"] = ref["dp"][name]
                arrays[f"{name}_sp"] = ref["sp"][name].astype(np.float32)
            total += write_split(tag, arrays)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    obs["per_call"] = per_call
    obs["error_measure"] = "per point, the largest |a - b| over the point's largest |b| bin; the maximum over the points"
    GC.write_observed(OUT, "start_observed.json", obs)
    print("fixtures:", total, "bytes")


if __name__ == "__main__":
    main()
