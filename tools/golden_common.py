"""What the tools/make_golden_*.py share: the command line, the build of their driver in both precisions by the oracle's recipe
(oracle/ref_build.py::build_driver -- the one place that invokes the compiler), the stream the drivers read and write, and the two writers
of a fixture.  The record formats are each tool's own."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_build  # noqa: E402

LIMIT = 600_000      # bytes: the largest fixture file a tool writes


def arguments(doc, golden):
    """-> the root of the reference tree, the directory to write to (default: tests/golden)"""
    if len(sys.argv) < 2:
        sys.exit(doc)
    return sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else golden


def executables(ref, name, routines, tmp, standins=(), flags=()):
    """-> {"dp": ..., "sp": ...}: tools/<name>_driver.F90 around the reference's `routines`, built under tmp"""
    driver = os.path.join(ROOT, "tools", name + "_driver.F90")
    return {p: ref_build.build_driver(driver, routines, tmp, p, standins, flags, ref) for p in ("dp", "sp")}


def r(*a):
    return b"".join(np.ascontiguousarray(np.asarray(x, "<f8")).tobytes() for x in a)


def i(*a):
    return b"".join(np.ascontiguousarray(np.asarray(x, "<i4")).tobytes() for x in a)


def infile(d):
    return os.path.join(d, "in.bin")


def drive(exe, d, *more, env=None):
    """Runs the driver on infile(d) -> the real64 values it wrote"""
    fout = os.path.join(d, "out.bin")
    subprocess.run([exe, infile(d), fout, *more], check=True, stdout=subprocess.DEVNULL, env=env)
    return np.fromfile(fout, "<f8")


def write_npz(out, name, arrays):
    path = os.path.join(out, name)
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= LIMIT, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


def write_observed(out, name, obs):
    with open(os.path.join(out, name), "w") as fh:
        json.dump(obs, fh, indent=1, sort_keys=True)
        fh.write("\n")
