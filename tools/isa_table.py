#!/usr/bin/env python3
"""One line per k_implsch4 instantiation of every IMPLSCH translation unit the library ships (ecwam_amd.build.IMPLSCH_SOURCES, the derived
single / double precision RARE objects included): static instruction count, VALU count (tools/isa_summary.py's classes), VGPR / AGPR,
scratch bytes, occupancy.  Two build variants side by side make the before / after table of a change that has a bit-identity partner:

python tools/isa_table.py notrim ""  > table.txt      (variant keys of ecwam_amd.build.VARIANTS; "" = the product)
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ecwam_amd import build as B  # noqa: E402
from isa_summary import summarise  # noqa: E402


def kernels(obj: str, variant: str) -> dict:
    """{(object, demangled kernel name): (instructions, VALU, VGPR, AGPR, scratch, occupancy)} of one object of the library"""
    src, extra = B.DERIVED.get(obj, (obj, []))
    flags = [f for f in B.FLAGS if f != "-fPIC"] + extra + B.VARIANTS[variant]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([B.HIPCC, *flags, "-S", "--cuda-device-only", "-o", out, os.path.join(B.CSRC, src)], check=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        text = open(out).read().split("\n")
    starts = [(i, ln.split(":")[0]) for i, ln in enumerate(text) if re.match(r"^_Z\w+:", ln)]
    names = [n for _, n in starts if "k_implsch4I" in n]
    dem = subprocess.run(["c++filt", *names], stdout=subprocess.PIPE, text=True).stdout.split("\n") if names else []
    res, k = {}, 0
    for n, (i, name) in enumerate(starts):
        if "k_implsch4I" not in name:
            continue
        body = text[i:(starts[n + 1][0] if n + 1 < len(starts) else len(text))]
        stop = next((q for q, ln in enumerate(body) if ln.strip().startswith("s_endpgm")), len(body))
        h = summarise(body[: stop + 1])
        meta = {}
        for ln in body[stop:]:
            m = re.match(r"\s*; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", ln)
            if m:
                meta.setdefault(m.group(1), int(m.group(2)))
        short = re.sub(r"^void k_implsch4<(.*)>\(.*$", r"\1", dem[k]).replace("false", "0").replace("true", "1").replace("(bool)", "")
        k += 1
        res[(obj.replace(".hip", ""), short)] = (sum(h.values()), sum(v for c, v in h.items() if c.startswith("VALU")), meta.get("NumVgprs", -1),
                                                 meta.get("NumAgprs", 0), meta.get("ScratchSize", -1), meta.get("Occupancy", -1))
    return res


def main() -> None:
    va, vb = (sys.argv[1:3] + ["", ""])[:2] if len(sys.argv) > 2 else ("notrim", "")
    jobs = [(o, v) for v in (va, vb) for o in B.IMPLSCH_SOURCES]
    with ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as ex:
        out = list(ex.map(lambda a: kernels(*a), jobs))
    a, b = {}, {}
    for i, r in enumerate(out):
        (a if i < len(B.IMPLSCH_SOURCES) else b).update(r)
    print(f"# k_implsch4<T, NANG, PP, R1, R2, NH, EXT, JAN, ENHMC, RARE, PART, ADV>: variant {va or 'product'!r} / variant {vb or 'product'!r}")
    print(f"{'object':11s} {'instantiation':44s} {'instructions':>15s} {'VALU':>13s} {'VGPR':>9s} {'AGPR':>9s} {'scratch B':>9s} {'occupancy':>9s}")
    tot = [0, 0]
    for key in sorted(a):
        x, y = a[key], b[key]
        tot[0] += x[1]; tot[1] += y[1]
        print(f"{key[0]:11s} {key[1]:44s} " + " ".join(f"{f'{p}/{q}':>{w}s}" for p, q, w in zip(x, y, (15, 13, 9, 9, 9, 9)))
              + ("" if x[2:] == y[2:] else "   <-- resources differ"))
    print(f"# VALU, all instantiations: {tot[0]} / {tot[1]}")


if __name__ == "__main__":
    main()
