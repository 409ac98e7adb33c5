"""Time the dual rotated-quadrant propagation scheme (IPROPAGS = 1, section 3 of PROPAGS1) on the device at the O320 size (36 directions x 36 frequencies), on
one GPU, beside the two other schemes in the same process and session, IREFRA 0:
  ecwam_hipx_propags1       the ten-term stencil on two rotated quadrants
  ecwam_hip_propags         the first-order scheme, IPROPAGS = 0 (section 3 of PROPAGS)
  ecwam_hip_propags2_otf    the corner-transport scheme
Single precision, and double precision once (--prec sp,dp).  Every call: the median of --windows windows of --iters calls each between two device events,
after --warmup calls.  The algorithmic bytes of a call are what it must read and write once per point: F1 read and F3 written (2 NANG NFRE reals) and the row
of CGROUP; the neighbour gathers are counted once, as the point's own read (the rotated scheme gathers seven neighbour spectra per point and direction, the
first-order scheme three, the corner-transport scheme up to nine: what the caches do not serve of them is on top).  bytes / time and its share of the HBM peak
are printed.

Prints one JSON line per measurement and writes the table to --out.  No time is a gate and no speed-up is claimed: the kernel has no parent to compare with.
Not measured: more than one GPU, the halo exchange, the kernels under a profiler.

usage: python tools/time_propags1.py [--n-oct 320] [--prec sp,dp] [--iters 5] [--windows 7] [--warmup 2] [--out profiles/propags1_device.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-oct", type=int, default=320)
    ap.add_argument("--prec", default="sp,dp")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propags1_device.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api, grid
    from ecwam_amd import synthetic as syn
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    NANG = NFRE = 36
    g = grid.build_grid(a.n_oct, "aqua")
    n, nrow = g.nsea, g.nsea + 1
    rng = np.random.default_rng(11)
    depth_h = np.where(rng.uniform(size=nrow) < 0.3, 10.0 ** rng.uniform(0.5, 3.0, nrow), 998.999)
    depth_h[n] = 998.999
    rows = []

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

    for prec in a.prec.split(","):
        T = np.float32 if prec == "sp" else np.float64
        s = np.dtype(T).itemsize
        cfg = Config(nang=NANG, nfre=NFRE, nfre_red=NFRE, idelpro=450, idelt=450, irefra=0)
        t = Tables(cfg, T)
        ctx = api.HipContext(t)
        dev = ctx.device
        z = dict(dtype=ctx.dtype, device=dev)
        props = syn.depth_props(depth_h, t, T)
        cg = torch.from_numpy(np.ascontiguousarray(props["CGROUP"], dtype=T)).to(dev)
        f1 = torch.rand((nrow, NANG, NFRE), **z)
        f1[n] = 0
        f3 = torch.zeros_like(f1)
        gd = api.propags_grid(api.grid_to_device(g, ctx.dtype, dev), g, t.CIRC)
        ctx.set_rotated(api.rotated_to_device(grid.rotated_tables(g, T, t.SINTH, t.COSTH), ctx.dtype, dev))
        base = dict(prec=prec, npts=n, nang=NANG, nfre=NFRE, irefra=0)
        per_point = 2 * NANG * NFRE * s + NFRE * s

        def report(name, times):
            med = float(np.median(times))
            nb = per_point * n
            r = dict(call=name, **base, samples=len(times), median_ms=med * 1e3, min_ms=float(np.min(times)) * 1e3, max_ms=float(np.max(times)) * 1e3,
                     algorithmic_bytes_per_point=int(per_point), gbytes_per_s=nb / med / 1e9, hbm_peak_share=nb / med / HBM_PEAK)
            rows.append(r)
            print(json.dumps(r), flush=True)

        fail = torch.zeros(n, dtype=torch.int32, device=dev)
        ctx.propags1(f1, None, gd, cg, 450.0, 0, n, cflfail=fail)
        assert int(fail.sum().item()) == 0, "the time step is too long for the grid"
        report("ecwam_hipx_propags1", device(lambda: ctx.propags1(f1, f3, gd, cg, 450.0, 0, n)))
        report("ecwam_hip_propags", device(lambda: ctx.propags(f1, f3, gd, cg, 450.0, 0, n)))
        ctx.ctuw(gd, cg, None, fail, 450.0, 1, NFRE)
        report("ecwam_hip_propags2_otf", device(lambda: ctx.propags2_otf(f1, f3, gd, cg, 450.0, 0, n)))
        del ctx, f1, f3
        torch.cuda.empty_cache()

    def ms(prec, call):
        return next(r["median_ms"] for r in rows if (r["prec"], r["call"]) == (prec, call))

    with open(a.out, "w") as fh:
        fh.write(f"Dual rotated-quadrant propagation scheme (IPROPAGS = 1, section 3) beside the two other schemes, O{a.n_oct} ({n} sea points), {NANG} x {NFRE},\n"
                 f"IREFRA 0, one MI355X, one process; median of {a.windows} windows of {a.iters} calls between device events after {a.warmup} warm-up calls\n"
                 "(tools/time_propags1.py).  bytes/pt = algorithmic bytes per point (F1 read once, F3 written once, the row of CGROUP); share = bytes / time over\n"
                 "the 8 TB/s HBM peak.  No time is a gate and no speed-up is claimed.\n\n")
        fh.write(f"{'call':28s} {'prec':4s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'bytes/pt':>9s} {'GB/s':>8s} {'share':>6s}\n")
        for r in rows:
            fh.write(f"{r['call']:28s} {r['prec']:4s} {r['median_ms']:10.3f} {r['min_ms']:8.3f} {r['max_ms']:8.3f} "
                     f"{r['algorithmic_bytes_per_point']:9d} {r['gbytes_per_s']:8.0f} {r['hbm_peak_share']:6.2f}\n")
        fh.write("\n")
        for prec in a.prec.split(","):
            p1, p0, c2 = ms(prec, "ecwam_hipx_propags1"), ms(prec, "ecwam_hip_propags"), ms(prec, "ecwam_hip_propags2_otf")
            fh.write(f"{prec}: the rotated scheme takes {p1:.3f} ms against {p0:.3f} ms of the first-order scheme ({p1 / p0:.2f} x) and {c2:.3f} ms of the "
                     f"corner-transport scheme ({p1 / c2:.2f} x).\n")


if __name__ == "__main__":
    main()
