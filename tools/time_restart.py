"""Time the start and the end of a run on the device at the O320 size (--npts rows, default 421,120; 36 directions x 36 frequencies), single and
double precision, on one GPU:
  ecwam_hip_depthprpt       INITDPTHFLDS for every row: wvprpt, the three extended arrays and EMAXDPT / DEPTH of ff from the depths
  ecwam_hip_savspec_pack    WRITEFL's record from FL1, plain and relabelled through a random permutation
  ecwam_hip_savstress_pack  the sixteen restart fields, plain and relabelled
and, in the same session, the host paths they replace in ecwam_amd/wamintgr.py: ecwam_amd.synthetic.depth_props in numpy with the upload of its
arrays (init_synthetic), and write_restart's copy of FL1 to the host with the transposition of ecwam_amd.restart.write_fl (without the file).

Device calls: the median of --windows windows of --iters calls each between two device events, after --warmup calls.  The host paths: the median of
--host-iters wall-clock times around work that ends in a device synchronise.  The algorithmic bytes of a device call are what it must read and
write once (depthprpt: the depths read, 8 rows of NFRE reals and two reals of ff written, and the piece of ff read back in single precision;
the pack calls: every value read once and written once, and the map); bytes / time and its share of the HBM peak are printed.  depthprpt is
not bound by bytes: each bin runs AKI's Newton iteration with TANH, COSH and SQRT.

Prints one JSON line per measurement.  No gate.  Not measured: the file system, more than one GPU, the kernels under a profiler.

usage: python tools/time_restart.py [--npts 421120] [--prec sp,dp] [--iters 5] [--windows 7] [--warmup 2] [--host-iters 3]
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
    ap.add_argument("--npts", type=int, default=421120)
    ap.add_argument("--prec", default="sp,dp")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-iters", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api
    from ecwam_amd import synthetic as syn
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    n, NANG, NFRE = a.npts, 36, 36

    def device(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3 / a.iters)
        return times

    def host(call):
        times = []
        for _ in range(a.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return times

    for prec in a.prec.split(","):
        T = np.float32 if prec == "sp" else np.float64
        s = np.dtype(T).itemsize
        t = Tables(Config(nang=NANG, nfre=NFRE, nfre_red=NFRE), T)
        ctx = api.HipContext(t)
        base = dict(prec=prec, npts=n, nang=NANG, nfre=NFRE)

        def report(name, times, nbytes, kind, **kw):
            med = float(np.median(times))
            print(json.dumps(dict(call=name, **base, timing=kind, samples=len(times), median_ms=med * 1e3, min_ms=float(np.min(times)) * 1e3,
                                  max_ms=float(np.max(times)) * 1e3, algorithmic_bytes=int(nbytes), gbytes_per_s=nbytes / med / 1e9,
                                  hbm_peak_share=nbytes / med / HBM_PEAK, **kw)), flush=True)

        rng = np.random.default_rng(11)
        depth_h = np.where(rng.uniform(size=n) < 0.3, 10.0 ** rng.uniform(0.3, 3.0, n), 998.999).astype(T)
        z = dict(dtype=ctx.dtype, device=ctx.device)
        depth = torch.from_numpy(depth_h).to(ctx.device)
        wvprpt, ff = torch.zeros((n, 5, NFRE), **z), torch.zeros((n, 16), **z)
        wn, cg, om = (torch.zeros((n, NFRE), **z) for _ in range(3))
        nb = n * (s + 8 * NFRE * s + 2 * s + (16 if prec == "sp" else 0))
        report("ecwam_hip_depthprpt, every output", device(lambda: ctx.depthprpt(0, n, depth, wvprpt, wn, cg, om, ff)), nb, "device events")

        def host_depth():
            pr = syn.depth_props(depth_h, t, T)
            wv = np.stack([pr[k] for k in ("WAVNUM", "CGROUP", "CINV", "XK2CG", "STOKFAC")], 1)
            wvprpt.copy_(torch.from_numpy(wv))
            for dst, k in ((wn, "WAVNUM"), (cg, "CGROUP"), (om, "OMOSNH2KD")):
                dst.copy_(torch.from_numpy(pr[k]))
            ff[:, 14] = torch.from_numpy(pr["EMAXDPT"]).to(ctx.device)
        report("host: synthetic.depth_props in numpy + upload (what init_synthetic does)", host(host_depth), nb, "wall clock")
        del wvprpt, wn, cg, om

        fl1 = torch.rand((n, NANG, NFRE), **z)
        blk = torch.empty((NANG * NFRE, n), **z)
        perm = rng.permutation(n).astype(np.int32)
        ctx.set_restart_map(perm)
        nb = 2 * n * NANG * NFRE * s
        report("ecwam_hip_savspec_pack, all fields", device(lambda: ctx.savspec_pack(0, n, fl1, blk)), nb, "device events")
        report("ecwam_hip_savspec_pack, all fields, relabelled", device(lambda: ctx.savspec_pack(0, n, fl1, blk, 0, True)), nb + 4 * n * (NFRE * s // 16), "device events",
               note="the map is read once per tile and piece")
        u, v = torch.rand(n, **z), torch.rand(n, **z)
        rf = torch.empty((16, n), **z)
        nb = 2 * 16 * n * s
        report("ecwam_hip_savstress_pack", device(lambda: ctx.savstress_pack(0, n, ff, u, v, rf)), nb, "device events")
        report("ecwam_hip_savstress_pack, relabelled", device(lambda: ctx.savstress_pack(0, n, ff, u, v, rf, True)), nb + 4 * n, "device events")
        report("the record to the host as the device formed it (write_restart_device without the file)", host(lambda: blk.cpu().numpy()), n * NANG * NFRE * s, "wall clock")
        del blk

        def host_record():
            a_ = np.ascontiguousarray(np.transpose(fl1.cpu().numpy(), (2, 1, 0)))
            return a_.reshape(-1).view(np.uint8)
        report("host: FL1 to the host + the transposition of restart.write_fl (write_restart without the file)", host(host_record), 2 * n * NANG * NFRE * s, "wall clock")
        del fl1
        ctx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
