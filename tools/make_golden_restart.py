"""Generates tests/golden/restart_0.npz and tests/golden/restart_observed.json by RUNNING the reference's own CDUSTARZ0, CHNKMIN, WRITEFL, WRITESTRESS
and READSTRESS (src/ecwam/*.F90) behind tools/restart_driver.F90, built by oracle/ref_build.py::build_driver with the reference's own modules in
double and in single precision.  BUILDSTRESS, READWGRIB, SAVSTRESS and GETSTRESS are bound to files and to the message
passing library, so the driver restates their statements on the fields around the reference's routines; IWAM_GET_UNIT is a stand-in that opens the
file in the byte order of the machine (the driver's header says why).  Everything is built in a temporary directory outside the tree; the
reference's text is read by the compiler, never copied.  The fixture holds, per precision: the rows of ff after every case of
tests/restart_ref.py::CASES with the drag coefficient and the branch code per point, the bytes of the BLS and LAW files the reference's WRITEFL and
WRITESTRESS wrote (LL1D, and the relabelled branch with the permutation of tests/restart_ref.py::permutation), what READSTRESS returned from the
LAW files, and EMAXDPT by initdpthflds.F90:61-73 on the depths of tests/golden/reference_depthprpt.npz (whose own EMAXDPT, a statement of
oracle/ref_driver.F90, lacks the reduction of GAM below 4 m).  The inputs are those of tests/restart_ref.py, which the tests rebuild (float32-representable, so that both precisions see the same
numbers).  Only usable where the reference tree exists.

The tool stops, naming what it missed, unless the single and the double precision reference took the same branch at every point of every case, the
restatement took those branches too, every branch of tests/restart_ref.py::BRANCH_NAMES but the unreachable Z0MIN floor is taken AND left by some
point, and no bin of tests/golden/reference_depthprpt.npz has AKI's termination test within 1e-6 of its threshold.  No case is dropped.  It then writes the
observed figures the tests take their gates from, per case and column of ff (and, section "depthprpt", per array of DEPTHPRPT, from the fixture
that already exists and ecwam_amd.synthetic.depth_props):
  reference_sp_vs_dp           the reference's own single against its double precision results
  restatement_vs_reference_dp  numpy in float64 against the double precision results
  restatement_vs_reference_sp  numpy in float32 against the single precision results
each |a - b| / max(|b|, the column's largest |b|), the maximum; and for AKI per bin of a float64 restatement the ratio |AKP-AO| / (EBS AO) of the
steps, of which the one closest to 1 is recorded, and the relative change one further Newton step would make.

    python tools/make_golden_restart.py <root of the reference tree> [<directory to write to; default tests/golden>]
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_cases as RC  # noqa: E402
import restart_ref as F  # noqa: E402  (the construction of the inputs and the restatement, shared with the tests)
from ecwam_amd import synthetic as syn  # noqa: E402
import golden_common as GC  # noqa: E402

REF, OUT = GC.arguments(__doc__, F.GOLDEN)
ROUTINES = ("cdustarz0", "chnkmin", "writefl", "writestress", "readstress")
STANDINS = ("YOWUNBLKRORD",)      # the three file routines name it only behind WAM_HAVE_UNWAM, which is not defined: no module is supplied
FILES = ("BLS_ll1d", "BLS_relab", "LAW_ll1d", "LAW_relab")


_r, _i = GC.r, GC.i


def run(exe, tmp, prec, inp, state):
    """-> the arrays of one precision, keyed as the fixture keys them without the precision"""
    d = os.path.join(tmp, prec)
    T = F.dtype_of(prec)
    with open(GC.infile(d), "wb") as fh:
        fh.write(_i(F.N, F.NANG, F.NFRE, F.NCELL, inp["map_in"] + 1, F.permutation() + 1))
        t = F.tables(prec)
        fh.write(_r([float(getattr(t, k)) for k in F.CONSTANTS], F.ZMISS, F.PRCHAR))
        fh.write(_r(inp["ff"], inp["uwave"], inp["cd"]))
        fh.write(_i(len(F.CASES)))
        for cap, has_cd, has_uw, zref, nse in F.CASES.values():
            fh.write(_i(int(cap), int(has_cd), int(has_uw), int(nse)) + _r(zref))
        fh.write(_r(state["fl"], state["ff"], state["ucur"], state["vcur"]))
        fh.write("".join(F.DATES).encode("ascii"))
        depth = RC.depthprpt_depths()
        fh.write(_i(depth.size) + _r(depth, float(t.GAM_B_J)))
    flat = GC.drive(exe, d, d)
    res, at = {}, 0

    def take(n, kind=T):
        nonlocal at
        a = flat[at:at + n]
        at += n
        out = np.ascontiguousarray(a, dtype=kind)
        assert np.array_equal(out.astype(np.float64), a)      # nothing is lost by narrowing what the driver widened
        return out
    for name in F.CASES:
        res[f"ff_{name}"] = take(F.N * F.NFF).reshape(F.N, F.NFF)
        res[f"cd_{name}"] = take(F.N)
        res[f"branch_{name}"] = take(F.N, np.int32)
    for f in ("ll1d", "relab"):
        res[f"readstress_{f}"] = take(16 * F.N).reshape(16, F.N)      # RFIELD(N,16): field-major in memory
    res["emaxdpt"] = take(RC.depthprpt_depths().size)
    assert at == flat.size, (at, flat.size)
    for f in FILES:
        res[f"file_{f}"] = np.fromfile(os.path.join(d, f), np.uint8)
    return res


def aki_steps(depth, t):
    """AKI in float64 on every bin: (the ratio |AKP-AO| / (EBS AO) closest to 1 over the steps, the relative change of one further step), per bin"""
    G, ebs, dkmax = float(t.G), 0.0001, 40.0
    d = np.asarray(depth, np.float64)[:, None]
    om = np.asarray(t.ZPIFR, np.float64)[None, :]
    ao = np.maximum(om * om / (4.0 * G), om / (2.0 * np.sqrt(G * d))) * np.ones_like(d)
    done = np.zeros(ao.shape, bool)
    closest = np.full(ao.shape, np.inf)

    def step(a):
        bo = np.minimum(d * a, 45.0)
        th = G * a * np.tanh(bo)
        sth = np.sqrt(th)
        return a + (om - sth) * sth * 2.0 / (th / a + G * bo / np.cosh(bo) ** 2)
    for _ in range(200):
        deep = (d * ao > dkmax) & ~done
        done |= deep
        if done.all():
            break
        new = np.where(done, ao, step(ao))
        ratio = np.abs(ao - new) / (ebs * new)
        act = ~done
        closest = np.where(act & (np.abs(ratio - 1.0) < np.abs(closest - 1.0)), ratio, closest)
        done |= act & ~(ratio > 1.0)
        ao = new
    assert done.all()
    further = np.where(d * ao > dkmax, 0.0, np.abs(step(ao) - ao) / ao)
    return closest, further


def main():
    tmp = tempfile.mkdtemp(prefix="golden_restart_")
    try:
        inp, state = F.make_inputs(), F.restart_state()
        exe = GC.executables(REF, "restart", ROUTINES, tmp, STANDINS, ('-D__FILENAME__="reference"',))
        ref = {p: run(exe[p], tmp, p, inp, state) for p in ("dp", "sp")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kinds = ("reference_sp_vs_dp", "restatement_vs_reference_dp", "restatement_vs_reference_sp")
    obs = {k: {} for k in kinds}
    taken = np.zeros(len(F.BRANCH_NAMES), bool)
    left = np.zeros(len(F.BRANCH_NAMES), bool)
    for name, (cap, has_cd, has_uw, zref, nse) in F.CASES.items():
        if not np.array_equal(ref["sp"][f"branch_{name}"], ref["dp"][f"branch_{name}"]):
            bad = np.nonzero(ref["sp"][f"branch_{name}"] != ref["dp"][f"branch_{name}"])[0]
            raise SystemExit(f"case {name}: the single and the double precision reference took different branches at the points {bad.tolist()}")
        br = ref["dp"][f"branch_{name}"]
        for b in range(len(F.BRANCH_NAMES)):
            applies = (b != 0 or has_uw) and (b != 1 or has_cd) and (b < 4 or has_cd)
            if applies:
                taken[b] |= bool(((br >> b) & 1).any())
                left[b] |= bool((((br >> b) & 1) == 0).any())
        obs["reference_sp_vs_dp"][name] = dict(zip(F.FF_NAMES, F.rel_error(ref["sp"][f"ff_{name}"][:, :14], ref["dp"][f"ff_{name}"][:, :14]).tolist()))
        for p in ("dp", "sp"):
            ff, cd, mine = F.buildstress(p, name, inp)
            if not np.array_equal(mine, br):
                raise SystemExit(f"case {name} {p}: the restatement and the reference took different branches at {np.nonzero(mine != br)[0].tolist()}")
            obs[f"restatement_vs_reference_{p}"][name] = dict(zip(F.FF_NAMES, F.rel_error(ff[:, :14], ref[p][f"ff_{name}"][:, :14]).tolist()))
            assert ff[:, 14:].tobytes() == ref[p][f"ff_{name}"][:, 14:].tobytes()
        print(name, " ".join(f"{c} {obs['reference_sp_vs_dp'][name][c]:.1e}/{obs['restatement_vs_reference_dp'][name][c]:.1e}/"
                             f"{obs['restatement_vs_reference_sp'][name][c]:.1e}" for c in ("UFRIC", "TAUW", "Z0M", "CHRNCK")))
    want = [i for i, n in enumerate(F.BRANCH_NAMES) if n != "z0min"]
    missing = [F.BRANCH_NAMES[i] for i in want if not (taken[i] and left[i])]
    if missing:
        raise SystemExit(f"no point takes, or no point leaves, the branches {missing}: change the inputs of tests/restart_ref.py::make_inputs")
    # ---- the files: both precisions hold the same numbers, the relabelled file the permuted rows
    perm = F.permutation()
    for p in ("dp", "sp"):
        T = F.dtype_of(p)
        for f, pm in (("ll1d", None), ("relab", perm)):
            rec = F.record_of(state["fl"].astype(T), pm)
            raw = ref[p][f"file_BLS_{f}"]
            assert raw.size == rec.nbytes + 8 and raw[4:-4].tobytes() == rec.tobytes(), (p, f)
            assert ref[p][f"readstress_{f}"].tobytes() == F.rfield_of(state["ff"], state["ucur"], state["vcur"]).astype(T).tobytes(), (p, f)
    # ---- DEPTHPRPT: the fixture that exists.  Its EMAXDPT is oracle/ref_driver.F90's statement, which does not reduce GAM below 4 m as
    # initdpthflds.F90:66-70 does: EMAXDPT is the driver's record of the reference's statement, equal to the fixture's from 4 m on
    with np.load(os.path.join(F.GOLDEN, "reference_depthprpt.npz")) as z:
        dg = {k: z[k] for k in z.files}
    depth = dg["depth"]
    assert np.array_equal(depth, RC.depthprpt_depths()) and (depth < 4).sum() > 3
    for p in ("dp", "sp"):
        new = ref[p]["emaxdpt"]
        assert new[depth >= 4].tobytes() == dg[f"EMAXDPT_{p}"][depth >= 4].tobytes() and (new[depth < 4] < dg[f"EMAXDPT_{p}"][depth < 4]).all()
        dg[f"EMAXDPT_{p}"] = new
    obs["reference_sp_vs_dp"]["depthprpt"] = {k: float(F.rel_error(dg[k + "_sp"].reshape(len(depth), -1), dg[k + "_dp"].reshape(len(depth), -1)).max())
                                              for k in RC.DEPTHPRPT_KEYS}
    for p in ("dp", "sp"):
        own = syn.depth_props(depth, F.tables(p), F.dtype_of(p))
        own["EMAXDPT"] = F.emaxdpt(depth, p)
        obs[f"restatement_vs_reference_{p}"]["depthprpt"] = {
            k: float(F.rel_error(own[k].reshape(len(depth), -1), dg[f"{k}_{p}"].reshape(len(depth), -1)).max()) for k in RC.DEPTHPRPT_KEYS}
    closest, further = aki_steps(depth, F.tables("dp"))
    dist = float(np.abs(closest - 1.0).min())
    if not dist > 1e-6:
        raise SystemExit(f"a bin's termination test of AKI lies {dist} from its threshold: the fixture would need an exclusion")
    obs["aki"] = dict(closest_ratio_distance_from_1=dist, largest_change_of_one_further_step=float(further.max()), bins_near_the_threshold=0)
    print("depthprpt", obs["reference_sp_vs_dp"]["depthprpt"], obs["aki"])
    arrays = {}
    for p in ("dp", "sp"):
        for key, a in ref[p].items():
            if key.startswith("branch_"):
                arrays[key] = a
            else:
                arrays[f"{key}_{p}"] = a
    GC.write_npz(OUT, "restart_0.npz", arrays)
    obs["branches"] = {n: [bool(taken[i]), bool(left[i])] for i, n in enumerate(F.BRANCH_NAMES)}
    obs["error_measure"] = "per column or array: |a - b| / max(|b|, the column's largest |b|), the maximum"
    GC.write_observed(OUT, "restart_observed.json", obs)


if __name__ == "__main__":
    main()
