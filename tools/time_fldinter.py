"""Time ecwam_hip_fldinter at the O320 size: 421,080 sea points interpolated from ten fields of an atmosphere grid of --ngptotg points (default
1,661,440, an octahedral O640 grid), on one GPU, device-event median over --iters calls after --warmup.

Two tables: "banded", where neighbouring sea points read neighbouring source points (corners p, p + 1, p + r, p + r + 1 with p rising along the
rows, r = 2560: what a real pair of grids gives), and "scattered", the same corners at random places (no locality at all: the worst a table
could be).  All switches on (ten fields read, eleven planes written), with and without MASK_IN; and LLINTERPOL = F on a field vector of the
wave grid's own length.  The algorithmic bytes of a call: the table (the four positions and the padded weights) and the map read once, every
source value a point reads counted once per field (the distinct positions), eleven planes written, MASK_IN's distinct positions when given;
the share of the HBM peak they imply is printed.

Prints one JSON line per measurement.  No gate.  Not measured: the host's FLDINTER (the path this call replaces was never timed: no speed-up is
claimed), the upload of the fields, more than one GPU, the kernel under a profiler.

usage: python tools/time_fldinter.py [--npts 421080] [--ngptotg 1661440] [--prec sp] [--iters 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--npts", type=int, default=421080)
    ap.add_argument("--ngptotg", type=int, default=1661440)
    ap.add_argument("--prec", choices=("sp", "dp"), default="sp")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api, lib
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    n, ng, nf = a.npts, a.ngptotg, 10
    T = np.float32 if a.prec == "sp" else np.float64
    s = np.dtype(T).itemsize
    ctx = api.HipContext(Tables(Config(nang=36, nfre=36, nfre_red=36), T))
    ncell = n + 40
    ctx.set_forcing_map(20 + np.arange(n, dtype=np.int32), ncell)
    rng = np.random.default_rng(7)
    fieldg = torch.empty((13, ncell), dtype=ctx.dtype, device=ctx.device)
    ctx.init_fieldg(fieldg)
    mask = torch.zeros(max(ng, n), dtype=torch.int32, device=ctx.device)
    w = rng.uniform(0.0, 1.0, (n, 3)).astype(T).astype(np.float64)
    row = 2560
    p = (np.arange(n, dtype=np.int64) * (ng - row - 2)) // n
    banded = np.stack([p, p + 1, p + row, p + row + 1], 1).astype(np.int32)
    q = rng.integers(0, ng - row - 2, n)
    scattered = np.stack([q, q + 1, q + row, q + row + 1], 1).astype(np.int32)
    flags = lib.FLI_LADEN | lib.FLI_LGUST | lib.FLI_LLKC | lib.FLI_LWCUR | lib.FLI_NEWCURR
    base = dict(prec=a.prec, npts=n, nfields=nf)

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        return times

    def report(name, times, nbytes, **kw):
        med = float(np.median(times))
        print(json.dumps(dict(call=name, **base, iters=len(times), median_us=med * 1e6, min_us=float(np.min(times)) * 1e6, max_us=float(np.max(times)) * 1e6,
                              algorithmic_bytes=int(nbytes), bytes_per_s=nbytes / med, hbm_peak_share=nbytes / med / HBM_PEAK, **kw)), flush=True)

    for name, idx, ngp, interpol in (("banded", banded, ng, True), ("scattered", scattered, ng, True), ("LLINTERPOL = F", banded[:, :1].repeat(4, 1) % n, n, False)):
        fields = torch.empty((nf, ngp), dtype=ctx.dtype, device=ctx.device).uniform_(-10.0, 10.0)
        ctx.set_fldinter(np.ascontiguousarray(idx), w if interpol else None, ngp, interpol)
        distinct = int(np.unique(idx if interpol else idx[:, 0]).size)
        nbytes = n * (16 + (4 * s if interpol else 0) + 4) + distinct * nf * s + 11 * n * s
        report(f"fldinter, {name}", timed(lambda: ctx.fldinter(0, n, fields, fieldg, flags=flags)), nbytes, ngptotg=ngp, distinct_positions=distinct)
        m = mask[:ngp]
        report(f"fldinter, {name}, with MASK_IN", timed(lambda: ctx.fldinter(0, n, fields, fieldg, flags=flags, mask_in=m)), nbytes + distinct * 4, ngptotg=ngp,
               distinct_positions=distinct)
    report("init_fieldg", timed(lambda: ctx.init_fieldg(fieldg)), 13 * ncell * s, ncell=ncell)
    ctx.close()


if __name__ == "__main__":
    main()
