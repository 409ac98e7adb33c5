"""Time the first-order propagation scheme (IPROPAGS = 0) on the device at the O320 size (421,120 sea points, 36 directions x 36 frequencies), on one GPU,
beside the corner-transport scheme in the same process and session:
  ecwam_hip_propags         IREFRA 0 (section 3) and IREFRA 2 (section 4, the eleven-term stencil with currents)
  ecwam_hip_propags2_otf    the CTU scheme, IREFRA 0
  ecwam_hip_propags2_refra  the CTU scheme with currents, IREFRA 2
  ecwam_hip_propags_dot     the dot terms of the first-order scheme (once per change of the currents, not per step)
Single precision, and double precision once (--prec sp,dp).  Every call: the median of --windows windows of --iters calls each between two device events,
after --warmup calls.  The algorithmic bytes of a call are what it must read and write once per point: F1 read and F3 written (2 NANG NFRE reals), the rows
of frequencies it reads (CGROUP; with currents OMOSNH2KD and WAVNUM) and, with currents, the row of dot terms; the neighbour gathers are counted once, as
the point's own read.  bytes / time and its share of the HBM peak are printed.

Prints one JSON line per measurement and writes the table to --out.  No time is a gate: the first-order kernel has no parent to compare with.  Not measured:
more than one GPU, the halo exchange, the kernels under a profiler.

usage: python tools/time_propags.py [--n-oct 320] [--prec sp,dp] [--iters 5] [--windows 7] [--warmup 2] [--out profiles/propags_device.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propags_device.txt"))
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
    u_h, v_h = syn.currents(g)
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
        props = None
        f1 = f3 = None
        for irefra in (0, 2):
            cfg = Config(nang=NANG, nfre=NFRE, nfre_red=NFRE, idelpro=450, idelt=450, irefra=irefra)
            t = Tables(cfg, T)
            ctx = api.HipContext(t)
            dev = ctx.device
            z = dict(dtype=ctx.dtype, device=dev)
            if props is None:
                props = syn.depth_props(depth_h, t, T)
                cg, om, wn = (torch.from_numpy(np.ascontiguousarray(props[k], dtype=T)).to(dev) for k in ("CGROUP", "OMOSNH2KD", "WAVNUM"))
                f1 = torch.rand((nrow, NANG, NFRE), **z)
                f1[n] = 0
                f3 = torch.zeros_like(f1)
                ext = np.zeros(nrow)
                depth = torch.from_numpy(depth_h.astype(T)).to(dev)
                ext[:n] = u_h
                u = torch.from_numpy(ext.astype(T)).to(dev)
                ext[:n] = v_h
                v = torch.from_numpy(ext.astype(T)).to(dev)
            gd = api.propags_grid(api.grid_to_device(g, ctx.dtype, dev), g, t.CIRC)
            base = dict(prec=prec, npts=n, nang=NANG, nfre=NFRE, irefra=irefra)

            def report(name, times, per_point, **kw):
                med = float(np.median(times))
                nb = per_point * n
                r = dict(call=name, **base, samples=len(times), median_ms=med * 1e3, min_ms=float(np.min(times)) * 1e3, max_ms=float(np.max(times)) * 1e3,
                         algorithmic_bytes_per_point=int(per_point), gbytes_per_s=nb / med / 1e9, hbm_peak_share=nb / med / HBM_PEAK, **kw)
                rows.append(r)
                print(json.dumps(r), flush=True)

            spectra = 2 * NANG * NFRE * s
            if irefra == 0:
                report("ecwam_hip_propags", device(lambda: ctx.propags(f1, f3, gd, cg, 450.0, 0, n)), spectra + NFRE * s)
                fail = torch.zeros(n, dtype=torch.int32, device=dev)
                ctx.ctuw(gd, cg, None, fail, 450.0, 1, NFRE)
                report("ecwam_hip_propags2_otf", device(lambda: ctx.propags2_otf(f1, f3, gd, cg, 450.0, 0, n)), spectra + NFRE * s)
            else:
                dot = torch.zeros((n, 3 * NANG + 4), **z)
                report("ecwam_hip_propags_dot", device(lambda: ctx.propags_dot(gd, depth, u, v, dot)), (3 * NANG + 4 + 3) * s)
                env = dict(omosnh2kd_ext=om, wavnum_ext=wn, u_ext=u, v_ext=v, dot=dot)
                report("ecwam_hip_propags", device(lambda: ctx.propags(f1, f3, gd, cg, 450.0, 0, n, **env)), spectra + (3 * NFRE + 3 * NANG + 6) * s)
                refr = torch.zeros((n, 2 * NANG + 5), **z)
                fail = torch.zeros(n, dtype=torch.int32, device=dev)
                ctx.propdot(gd, depth, u, v, refr)
                ctx.ctuw_refra(gd, cg, om, wn, refr, fail, 450.0)
                report("ecwam_hip_propags2_refra", device(lambda: ctx.propags2_refra(f1, f3, gd, cg, om, wn, refr, 450.0, 0, n)),
                       spectra + (3 * NFRE + 2 * NANG + 5) * s)
            del ctx
        del f1, f3
        torch.cuda.empty_cache()

    def ms(prec, irefra, call):
        for r in rows:
            if (r["prec"], r["irefra"], r["call"]) == (prec, irefra, call):
                return r["median_ms"]
        return None

    with open(a.out, "w") as fh:
        fh.write(f"First-order propagation scheme (IPROPAGS = 0) beside the corner-transport scheme, O{a.n_oct} ({n} sea points), {NANG} x {NFRE}, one MI355X, one\n"
                 f"process; median of {a.windows} windows of {a.iters} calls between device events after {a.warmup} warm-up calls (tools/time_propags.py).\n"
                 "bytes/pt = algorithmic bytes per point (F1 read once, F3 written once, the rows of frequencies and the dot terms the call reads);\n"
                 "share = bytes / time over the 8 TB/s HBM peak.  No time is a gate.\n\n")
        fh.write(f"{'call':28s} {'prec':4s} {'IREFRA':6s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'bytes/pt':>9s} {'GB/s':>8s} {'share':>6s}\n")
        for r in rows:
            fh.write(f"{r['call']:28s} {r['prec']:4s} {r['irefra']:<6d} {r['median_ms']:10.3f} {r['min_ms']:8.3f} {r['max_ms']:8.3f} "
                     f"{r['algorithmic_bytes_per_point']:9d} {r['gbytes_per_s']:8.0f} {r['hbm_peak_share']:6.2f}\n")
        fh.write("\n")
        for prec in a.prec.split(","):
            p0, c0 = ms(prec, 0, "ecwam_hip_propags"), ms(prec, 0, "ecwam_hip_propags2_otf")
            p2, c2 = ms(prec, 2, "ecwam_hip_propags"), ms(prec, 2, "ecwam_hip_propags2_refra")
            fh.write(f"{prec}: without refraction the first-order scheme takes {p0:.3f} ms against {c0:.3f} ms of the corner-transport scheme ({p0 / c0:.2f} x).\n")
            verdict = "the cheaper" if p2 < c2 else "not the cheaper"
            fh.write(f"{prec}: with currents (IREFRA 2) the first-order scheme takes {p2:.3f} ms against {c2:.3f} ms of ecwam_hip_propags2_refra ({p2 / c2:.2f} x): it is "
                     f"{verdict} way to refraction on this hardware, by {abs(c2 - p2):.3f} ms per step.  (The two schemes differ in order of accuracy; this compares cost only.)\n")


if __name__ == "__main__":
    main()
