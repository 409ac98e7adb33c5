"""Time ecwam_hip_grib2wgrid at the O320 size: READWIND's eight parameters of one wind time in one call, on a grid of --ncell cells (default
421,120: the O320 wave grid's points rounded up to its longest row) from messages of --nvalues values (default 1,661,440, an octahedral O640
grid), on one GPU, device-event median over --iters calls after --warmup.

Synthetic tables: "banded", where neighbouring cells read neighbouring values (corners p, p + 1, p + r, p + r + 1 with p rising along the rows,
r = 2560: what a real pair of grids gives), and "scattered", the same corners at random places (no locality at all).  A tenth of the values is
missing, so that the nearest-corner and mean branches run; WDWAVE is a direction field (SIN, COS, ATAN2).  Also the eight as eight calls of one
field, and LLINTERPOL = F on a message of the wave grid's own length.  The algorithmic bytes of a call: the table (the four positions, the
weights and the kind) read once, every value a cell reads counted once per field (the distinct positions), eight planes written; the share of
the HBM peak they imply is printed.

Prints one JSON line per measurement.  No gate.  Not measured: the host's GRIB2WGRID and READWIND (the path this call replaces was never timed:
no speed-up is claimed), the decoding and the upload of the values, more than one GPU, the kernel under a profiler.

usage: python tools/time_readwind.py [--ncell 421120] [--nvalues 1661440] [--prec sp] [--iters 20] [--warmup 3]
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
    ap.add_argument("--ncell", type=int, default=421120)
    ap.add_argument("--nvalues", type=int, default=1661440)
    ap.add_argument("--prec", choices=("sp", "dp"), default="sp")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api, lib
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    n, nv = a.ncell, a.nvalues
    T = np.float32 if a.prec == "sp" else np.float64
    s = np.dtype(T).itemsize
    ctx = api.HipContext(Tables(Config(nang=36, nfre=36, nfre_red=36), T))
    rng = np.random.default_rng(7)
    planes = list(lib.G2W_PLANES)
    fields = [(p, lib.G2W_DIRFLD if p == "WDWAVE" else 0 if p == "WSWAVE" else lib.G2W_NONWAVE) for p in planes]
    nf = len(fields)
    fieldg = torch.zeros((13, n), dtype=ctx.dtype, device=ctx.device)
    w = rng.uniform(0.0, 1.0, (n, 3)).astype(T).astype(np.float64)
    kind = np.full(n, 2, np.int32)
    kind[rng.uniform(size=n) < 0.02] = 0
    row = 2560
    p = (np.arange(n, dtype=np.int64) * (nv - row - 2)) // n
    banded = np.stack([p, p + 1, p + row, p + row + 1], 1).astype(np.int32)
    q = rng.integers(0, nv - row - 2, n)
    scattered = np.stack([q, q + 1, q + row, q + row + 1], 1).astype(np.int32)
    base = dict(prec=a.prec, ncell=n, nfld=nf)

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

    def values_of(length):
        v = torch.empty((nf, length), dtype=ctx.dtype, device=ctx.device).uniform_(150.0, 250.0)
        v[torch.rand((nf, length), device=ctx.device) < 0.1] = -999.0
        return v

    for name, pos, length, interpol in (("banded", banded, nv, True), ("scattered", scattered, nv, True), ("LLINTERPOL = F", banded[:, :1].repeat(4, 1) % n, n, False)):
        values = values_of(length)
        ctx.set_input_grid(0, np.ascontiguousarray(pos), w if interpol else None, kind, length, interpol)
        distinct = int(np.unique(pos if interpol else pos[:, 0]).size)
        nbytes = n * (16 + 4 * s) + distinct * nf * s + nf * n * s
        report(f"grib2wgrid, {name}, eight fields in one call", timed(lambda: ctx.grib2wgrid(0, values, fields, fieldg=fieldg)), nbytes, nvalues=length,
               distinct_positions=distinct)
        ones = [values[i:i + 1].clone() for i in range(nf)]

        def eight():
            for i in range(nf):
                ctx.grib2wgrid(0, ones[i], fields[i:i + 1], fieldg=fieldg)
        report(f"grib2wgrid, {name}, eight calls of one field", timed(eight), nbytes + (nf - 1) * n * (16 + 4 * s), nvalues=length, distinct_positions=distinct)
    ctx.close()


if __name__ == "__main__":
    main()
