"""Time the start spectra (ecwam_hip_mstart, ecwam_hip_unsetice, ecwam_hip_getspec_noise, ecwam_hip_getspec_tail) at the O320 size, 36 x 36,
in single and double precision on one GPU: device-event median over --iters calls after --warmup, with the bytes each call must move (FL1
once per direction of transfer, two or five columns of FF) and the share of the HBM peak they imply; and, for comparison, the host path
the calls replace: numpy synthetic.jonswap_spectra of the same points plus the upload of the result.  Prints one JSON line per call and
precision.

UNSETICE is timed on a sea that holds energy everywhere (what INITMDL meets after preset: no point is reset, ET is still evaluated where the
ice cover allows a reset) and after a noise start (every open point is reset).  Not measured: more than one GPU, other sizes than O320,
the kernels under a profiler (counters, achieved occupancy), and the calls inside a model run, where FL1 may be in the Infinity Cache.

usage: python tools/time_start.py [--npts 421080] [--iters 30] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--npts", type=int, default=421080)       # O320 sea points
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api, synthetic as syn
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    n, K, M = a.npts, 36, 36
    rng = np.random.default_rng(11)
    ws = rng.uniform(0.5, 25.0, n)
    wd = rng.uniform(0.0, 2 * np.pi, n)
    ci = np.where(rng.uniform(size=n) < 0.1, rng.uniform(0.0, 1.0, n), 0.0)
    depth = np.where(rng.uniform(size=n) < 0.1, rng.uniform(5.0, 250.0, n), 999.0)
    for prec in ("sp", "dp"):
        dt = np.float32 if prec == "sp" else np.float64
        s = np.dtype(dt).itemsize
        t = Tables(Config(nang=K, nfre=M, nfre_red=M), dt)
        ctx = api.HipContext(t)
        ffh = np.zeros((n, api.NFF), dt)
        ffh[:, 1], ffh[:, 2], ffh[:, 3], ffh[:, 15] = wd, ci, ws, depth
        ffh[:, 14] = 0.0625 * (0.5 * depth) ** 2
        ff = torch.from_numpy(ffh).to(ctx.device)
        fl1 = torch.zeros((n, K, M), dtype=ctx.dtype, device=ctx.device)
        spec = n * K * M * s

        def timed(call, before=None):
            for _ in range(a.warmup):
                if before:
                    before()
                call()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.iters):
                if before:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3)
            return times

        def report(name, times, nbytes, **kw):
            med = float(np.median(times))
            print(json.dumps(dict(call=name, prec=prec, npts=n, iters=a.iters, median_s=med, min_s=float(np.min(times)), max_s=float(np.max(times)),
                                  bytes=nbytes, bytes_per_s=nbytes / med, hbm_peak_share=nbytes / med / HBM_PEAK, **kw)), flush=True)

        sea = lambda: ctx.mstart(0, n, fl1, ff, 2, 3.0e4, 0.25, 0.0, 0.25, 0.018, 3.0, 0.07, 0.09)
        report("mstart", timed(sea), spec + 2 * n * s)
        report("getspec_noise", timed(lambda: ctx.getspec_noise(0, n, fl1)), spec)
        report("unsetice", timed(lambda: ctx.unsetice(0, n, fl1, ff, 31000.0), before=sea), 2 * spec + 5 * n * s, spectra="a sea everywhere: no point is reset")
        report("unsetice", timed(lambda: ctx.unsetice(0, n, fl1, ff, 31000.0), before=lambda: ctx.getspec_noise(0, n, fl1)), 2 * spec + 5 * n * s,
               spectra="after a noise start: every open point is reset")
        report("getspec_tail", timed(lambda: ctx.getspec_tail(0, n, fl1, ff, M), before=sea), 2 * spec + n * s, nfre_red=M)
        report("getspec_tail", timed(lambda: ctx.getspec_tail(0, n, fl1, ff, 29), before=sea), 2 * spec + n * s, nfre_red=29)
        assert bool(torch.isfinite(fl1).all())
        # the host path: numpy spectra of the same points, then the upload (pageable memory, as tests/harness.py and the tools do it)
        fp = np.clip(0.13 * 9.806 / np.maximum(ws, 0.5), 0.05, 0.4)
        tn = tu = 0.0
        for c0 in range(0, n, 65536):      # in chunks, as Wamintgr.init_synthetic does
            sl = slice(c0, min(n, c0 + 65536))
            t0 = time.perf_counter()
            host = syn.jonswap_spectra(t.FR, t.TH, fp[sl], wd[sl], dt)
            t1 = time.perf_counter()
            fl1[sl].copy_(torch.from_numpy(host))
            torch.cuda.synchronize()
            tn, tu = tn + (t1 - t0), tu + (time.perf_counter() - t1)
        print(json.dumps(dict(call="host: numpy jonswap_spectra + upload", prec=prec, npts=n, numpy_s=tn, upload_s=tu, total_s=tn + tu, bytes=spec)), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
