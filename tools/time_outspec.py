"""Time ecwam_hip_outspec_values at the O320 size (421,080 sea points on 421,120 values), 36 x 29 and 24 x 29 fields, single precision, on
one GPU: device-event median over --iters calls after --warmup, of one call over all fields and of the same fields in slabs of 64 (what a
host with a bounded buffer does), with the bytes the algorithm moves and the share of the HBM peak they imply.  The algorithmic bytes of a
call: the NFRE_RED leading frequencies of every FL1 row read once, values written once, and the finish the library chose (the threshold pass)
reading values once more; what the threshold stores (the missing values only) is not counted.  A slab reads less of FL1 algorithmically, but
the pieces it needs lie in every line of a row: the figure printed for the slabs counts what the algorithm needs, not what the memory moves.
Beside it, the device-to-host copy of FL1 (pageable memory) that the call replaces -- the copy only: the host's transposition, logarithm and
threshold are not timed here.  Prints one JSON line per measurement.

Not measured: double precision, more than one GPU, the kernels under a profiler, the call inside a model run.

usage: python tools/time_outspec.py [--npts 421080] [--iters 10] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s
SLAB = 64


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--npts", type=int, default=421080)       # O320 sea points: the first and the last row of the octahedral grid, 20 cells each, are land
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api, synthetic as syn
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    n, M, MR, s = a.npts, 36, 29, 4
    ntencode = n + 40
    ival = 20 + np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(11)
    for K in (36, 24):
        t = Tables(Config(nang=K, nfre=M, nfre_red=MR, licerun=True, lmaskice=True), np.float32)
        ctx = api.HipContext(t)
        ctx.set_grib_map(ival, ntencode)
        fl1 = torch.empty((n, K, M), dtype=ctx.dtype, device=ctx.device)
        for c0 in range(0, n, 65536):
            m = min(n, c0 + 65536) - c0
            fl1[c0:c0 + m] = torch.from_numpy(syn.jonswap_spectra(t.FR, t.TH, rng.uniform(0.08, 0.35, m), rng.uniform(0, 2 * np.pi, m), np.float32)).to(ctx.device)
        ffh = np.zeros((n, api.NFF), np.float32)
        ffh[:, 2] = np.where(rng.uniform(size=n) < 0.1, rng.uniform(0.0, 1.0, n), 0.0)
        ff = torch.from_numpy(ffh).to(ctx.device)
        nf = K * MR
        values = torch.empty((nf, ntencode), dtype=ctx.dtype, device=ctx.device)
        slab = torch.empty((SLAB, ntencode), dtype=ctx.dtype, device=ctx.device)
        ppmax = torch.empty(nf, dtype=ctx.dtype, device=ctx.device)

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
            print(json.dumps(dict(call=name, prec="sp", nang=K, nfre_red=MR, npts=n, ntencode=ntencode, iters=a.iters, median_ms=med * 1e3, min_ms=float(np.min(times)) * 1e3,
                                  max_ms=float(np.max(times)) * 1e3, algorithmic_bytes=nbytes, bytes_per_s=nbytes / med, hbm_peak_share=nbytes / med / HBM_PEAK, **kw)),
                  flush=True)

        def bytes_of(f):      # FL1: the fields' reals and CICOVER; values: written, then read by the threshold pass
            return (n * f + n) * s + 2 * f * ntencode * s

        report("outspec_values, all fields in one call", timed(lambda: ctx.outspec_values(0, n, fl1, values, ff, ice_mask=True, ppmax=ppmax)), bytes_of(nf), nfld=nf)

        def slabs():
            for f0 in range(0, nf, SLAB):
                k = min(SLAB, nf - f0)
                ctx.outspec_values(0, n, fl1, slab[:k], ff, ifld0=f0, nfld=k, ice_mask=True, ppmax=ppmax[f0:f0 + k])

        ts = timed(slabs)
        nslab = (nf + SLAB - 1) // SLAB
        report(f"outspec_values, {nslab} slabs of {SLAB} fields", ts, bytes_of(nf) + (nslab - 1) * n * s, nfld=nf, nslab=nslab,
               median_ms_per_slab=float(np.median(ts)) * 1e3 / nslab)
        # the copy the call replaces: FL1 to the host (pageable memory, one blocking copy)
        host = np.empty((n, K, M), np.float32)
        th = torch.from_numpy(host)
        copies = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            th.copy_(fl1)
            torch.cuda.synchronize()
            copies.append(time.perf_counter() - t0)
        print(json.dumps(dict(call="device-to-host copy of FL1 (the host path's first step; its transposition and logarithm are not timed)", prec="sp", nang=K,
                              npts=n, bytes=n * K * M * s, median_ms=float(np.median(copies)) * 1e3, min_ms=float(np.min(copies)) * 1e3)), flush=True)
        del fl1, values, slab
        ctx.close()


if __name__ == "__main__":
    main()
