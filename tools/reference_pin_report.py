"""Measures the oracle against the reference fixtures (tests/golden/reference_*.npz) on the CPU and records the observed maxima per
configuration and quantity: tests/golden/reference_pin_observed.json (what tests/test_reference_pin.py sets its double precision gates from:
10 x the observed value, never looser than the project's dp gates) and profiles/reference_pin.txt (the same, readable, with the single
precision figures and the share of candidate points each fixture's generator dropped).

    python tools/reference_pin_report.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_cases as RC  # noqa: E402

Q = ("bins", "swh", "ff", "intf", "w2n")


def main():
    obs, lines = {}, []
    lines.append("Oracle (oracle/ora_*.c) against the reference's own Fortran, on the fixtures tests/golden/reference_*.npz.  CPU, both builds with")
    lines.append("contraction off.  bins: worst bin over the point's spectral peak; swh: significant wave height; ff: forcing outputs; intf: flux groups;")
    lines.append("w2n: WAVE2OCEAN columns over the column's scale (harness.compare_implsch).  MIJ and XLLWS identical in every row.")
    lines.append("dropped: share of the generator's candidate points at which the reference's own sp and dp builds disagree on MIJ / XLLWS.")
    lines.append("")
    lines.append(f"{'configuration':<20}{'points':>7}{'dropped':>9}  prec " + "".join(f"{q:>11}" for q in Q) + "   dp gate asserted (10 x observed; 8 eps where observed is 0; never above the ceiling)")
    for name in RC.CONFIGS:
        inp, ref = RC.load(name)
        n = inp["FL1"].shape[0]
        meta = json.loads(str(np.load(RC.path(name))["meta"]))
        for prec in ("dp", "sp"):
            got = RC.run(RC.oracle_for(name, prec), inp, RC.kind(name))
            st = RC.stats(name, ref[prec], got, prec)
            assert st["mij_flips"] == 0 and st["xllws_bins_diff"] == 0, (name, prec, st)
            f = RC.figures(st)
            gates = ""
            if prec == "dp":
                obs[name] = {q: float(f[q]) for q in Q}
                gates = "   " + " ".join(f"{RC.dp_gate_of(f[q], q):.1e}" for q in Q)
            lines.append(f"{name:<20}{n:>7}{100 * meta['dropped']:>8.1f}%  {prec:>4} " + "".join(f"{f[q]:>11.2e}" for q in Q) + gates)
    with open(RC.OBSERVED, "w") as fh:
        json.dump(obs, fh, indent=1, sort_keys=True)
        fh.write("\n")
    out = os.path.join(ROOT, "profiles", "reference_pin.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(RC.OBSERVED, out)


if __name__ == "__main__":
    main()
