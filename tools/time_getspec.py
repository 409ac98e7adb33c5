"""Time the warm start at the O320 size (421,080 sea points on 421,120 values), 36 x 36 = 1296 fields, single precision, on one GPU.

The device path: ecwam_hip_getspec_values (un-scaling and ZMISS -> EPSMIN on) on vectors that are on the device -- device-event median over
--iters calls after --warmup, of one call over all fields and of the same fields in slabs of 64 (what a host with a bounded buffer does, per
slab and in total) -- and, reported separately, the upload of what the host holds (pageable memory, blocking copies timed on the host): one
slab, and all vectors.  ecwam_hip_getspec_unpack on the restart record (flags = 0) is timed the same way.  The algorithmic bytes of a call: the
fields read once, the same number of reals of FL1 written once, and the map read once per call; the share of the HBM peak they imply is printed.

What the parent commit does for the same job, from the same record on the host: the numpy transposition of restart.read_fl
(np.ascontiguousarray(np.transpose(record.reshape(NFRE, NANG, n), (2, 1, 0)))), timed on the host, plus the upload of FL1.

Prints one JSON line per measurement.  No gate.  Not measured: double precision, more than one GPU, the kernels under a profiler, reading the
file, the GRIB decoding itself.

usage: python tools/time_getspec.py [--npts 421080] [--iters 10] [--warmup 2]
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

    from ecwam_amd import api
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    n, K, M, s = a.npts, 36, 36, 4
    nf = K * M
    ntencode = n + 40
    ival = 20 + np.arange(n, dtype=np.int32)
    ctx = api.HipContext(Tables(Config(nang=K, nfre=M, nfre_red=M), np.float32))
    ctx.set_grib_map(ival, ntencode)
    gen = torch.Generator(device=ctx.device).manual_seed(11)
    values = torch.empty((nf, ntencode), dtype=ctx.dtype, device=ctx.device)
    values.uniform_(-10.0, 1.0, generator=gen)
    values[torch.rand(values.shape, device=ctx.device, generator=gen) < 0.05] = -999.0
    fl1 = torch.empty((n, K, M), dtype=ctx.dtype, device=ctx.device)
    base = dict(prec="sp", nang=K, nfre=M, npts=n, ntencode=ntencode, nfld=nf)

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
        print(json.dumps(dict(call=name, **base, iters=len(times), median_ms=med * 1e3, min_ms=float(np.min(times)) * 1e3, max_ms=float(np.max(times)) * 1e3,
                              algorithmic_bytes=nbytes, bytes_per_s=nbytes / med, hbm_peak_share=nbytes / med / HBM_PEAK, **kw)), flush=True)

    def host_timed(name, call, nbytes, reps=3, **kw):
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        print(json.dumps(dict(call=name, **base, reps=reps, bytes=nbytes, median_ms=float(np.median(times)) * 1e3, min_ms=float(np.min(times)) * 1e3, **kw)), flush=True)
        return float(np.median(times))

    def bytes_of(f, calls=1):      # the fields read, as many reals of FL1 written, the map per call
        return 2 * f * n * s + calls * n * 4

    # ---- the device path
    report("getspec_values, all fields in one call", timed(lambda: ctx.getspec_values(0, n, values, fl1)), bytes_of(nf))
    nslab = (nf + SLAB - 1) // SLAB

    def slabs():
        for f0 in range(0, nf, SLAB):
            ctx.getspec_values(0, n, values[f0:min(nf, f0 + SLAB)], fl1, ifld0=f0)

    ts = timed(slabs)
    report(f"getspec_values, {nslab} slabs of {SLAB} fields", ts, bytes_of(nf, nslab), nslab=nslab, median_ms_per_slab=float(np.median(ts)) * 1e3 / nslab)
    rec_d = values[:, :n].contiguous()      # the restart record: NANG NFRE vectors of n reals
    report("getspec_unpack, the restart record (flags = 0)", timed(lambda: ctx.getspec_unpack(0, n, rec_d, fl1)), 2 * nf * n * s)
    # ---- the uploads of what the host holds
    slab_h = values[:SLAB].cpu()
    slab_d = torch.empty_like(values[:SLAB])
    host_timed(f"upload of one slab of {SLAB} decoded vectors (pageable)", lambda: slab_d.copy_(slab_h), SLAB * ntencode * s)
    rec_h = rec_d.cpu()
    up_rec = host_timed("upload of the record as the file holds it (pageable)", lambda: rec_d.copy_(rec_h), nf * n * s)
    # ---- what the parent commit does: the transposition of restart.read_fl on the host, then the upload of FL1
    rec_np = rec_h.numpy().reshape(M, K, n)
    out = {}

    def transpose():
        out["fl"] = np.ascontiguousarray(np.transpose(rec_np, (2, 1, 0)))

    tr = host_timed("host transposition of restart.read_fl (numpy)", transpose, 2 * nf * n * s, reps=2)
    fl_h = torch.from_numpy(out["fl"])
    up_fl = host_timed("upload of FL1 (pageable)", lambda: fl1.copy_(fl_h), nf * n * s)
    ctx.getspec_unpack(0, n, rec_d, fl1)
    torch.cuda.synchronize()
    same = bool(torch.equal(fl1.cpu(), fl_h))
    print(json.dumps(dict(call="summary", **base, parent_host_path_ms=(tr + up_fl) * 1e3, device_path_upload_ms=up_rec * 1e3, same_bits=same)), flush=True)
    assert same
    ctx.close()


if __name__ == "__main__":
    main()
