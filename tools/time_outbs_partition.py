"""Time ecwam_hip_outbs_partition (SEPWISW with LLPARTITION = T: the wind-sea / swell split and the three swell trains) at the O320 size:
device-event median over --iters calls on the multi-system workload of ecwam_amd.synthetic.multi_system_spectra (a wind sea and 0-4
swells per point), or with --worst on many_peak_spectra (every point at NPMAX = 20 peaks).  Prints one JSON line with the algorithmic
bytes per call (FL1 + XLLWS + MIJ + CINV + 3 FF scalars + 24 outputs per point).  Run the kernel-time measurement under
`rocprofv3 --kernel-trace --stats -- python ...` in a run of its own.  --hist N: no GPU; the histograms of NPEAK and of the sweep counts of
the first N points of the workload, from the restatement tests/partition_ref.py.

usage: python tools/time_outbs_partition.py [--prec sp|dp] [--npts 421080] [--iters 50] [--warmup 5] [--worst] [--hist N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s
CHUNK = 32768


def workload(t, n, worst: bool, chunk: int = CHUNK):
    """Yields (row0, FL1, XLLWS, MIJ, CINV, UFRIC, WDWAVE) chunks of the workload, reproducible by row."""
    import numpy as np

    from ecwam_amd import synthetic as syn

    T = t.dtype
    K, M = len(t.TH), len(t.FR)
    for r0 in range(0, n, chunk):
        c = min(chunk, n - r0)
        rng = np.random.default_rng(1000 + r0 // chunk)
        wd = rng.uniform(0.0, 2 * np.pi, c).astype(T)
        if worst:
            fl = syn.many_peak_spectra(t.FR, t.TH, c, T)
            xl = np.zeros((c, K, M), T)
            uf = np.zeros(c, T)
            mij = np.full(c, M, np.int32)
        else:
            fl, _ = syn.multi_system_spectra(t.FR, t.TH, wd, T, seed=2000 + r0 // chunk)
            cw = np.cos(t.TH[None, :] - wd[:, None])
            xl = ((cw[:, :, None] > 0.5) & (t.FR[None, None, :] > 0.15)).astype(T)
            uf = rng.uniform(0.2, 0.6, c).astype(T)
            mij = rng.integers(24, M + 1, c).astype(np.int32)
        cinv = np.broadcast_to((t.ZPI * t.FR / T(9.806)).astype(T), (c, M))
        yield r0, fl, xl, mij, cinv, uf, wd


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", choices=["sp", "dp"], default="sp")
    ap.add_argument("--npts", type=int, default=421080)       # O320 sea points
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worst", action="store_true")
    ap.add_argument("--hist", type=int, default=0)
    a = ap.parse_args()

    import numpy as np

    from ecwam_amd.tables import Config, Tables

    dt = np.float32 if a.prec == "sp" else np.float64
    t = Tables(Config(nang=36, nfre=36, nfre_red=36), dt)
    if a.hist:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import partition_ref as P

        npk, swp = [], []
        for _, fl, xl, mij, cinv, uf, wd in workload(t, a.hist, a.worst, chunk=2048):
            _, info = P.partition(t, fl, xl, mij, cinv, uf, wd)
            npk.append(info["npeak_found"].clip(0, P.NPMAX + 1))
            s = info["sweeps"]
            swp.append(s[s > 0])
        npk, swp = np.concatenate(npk), np.concatenate(swp)
        print(json.dumps(dict(points=a.hist, prec=a.prec, worst=a.worst, npeak_hist=np.bincount(npk, minlength=P.NPMAX + 2).tolist(),
                              sweeps_hist=np.bincount(swp, minlength=26).tolist(), peaks=int(swp.size), mean_sweeps=float(swp.mean()))))
        return

    import torch

    from ecwam_amd import api

    assert torch.cuda.is_available(), "needs a GPU"
    ctx = api.HipContext(t)
    dev, tdt = ctx.device, ctx.dtype
    n, K, M = a.npts, 36, 36
    fl1 = torch.empty((n, K, M), dtype=tdt, device=dev)
    xllws = torch.empty((n, K, M), dtype=tdt, device=dev)
    mij = torch.empty(n, dtype=torch.int32, device=dev)
    wv = torch.zeros((n, api.NWPR, M), dtype=tdt, device=dev)
    ff = torch.zeros((n, api.NFF), dtype=tdt, device=dev)
    for r0, fl, xl, mj, cinv, uf, wd in workload(t, n, a.worst):
        s = slice(r0, r0 + len(fl))
        fl1[s] = torch.from_numpy(fl).to(dev)
        xllws[s] = torch.from_numpy(xl).to(dev)
        mij[s] = torch.from_numpy(mj).to(dev)
        wv[s, 2] = torch.from_numpy(np.ascontiguousarray(cinv)).to(dev)
        ff[s, 1] = torch.from_numpy(wd).to(dev)
        ff[s, 7] = torch.from_numpy(uf).to(dev)
    out = torch.zeros((n, 24), dtype=tdt, device=dev)
    for _ in range(a.warmup):
        ctx.outbs_partition(0, n, fl1, xllws, mij, wv, ff, out)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.outbs_partition(0, n, fl1, xllws, mij, wv, ff, out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    assert bool(torch.isfinite(out).all())
    ntr = (out[:, 15::3] > 0).sum(1).cpu().numpy()
    s = np.dtype(dt).itemsize
    nbytes = n * ((2 * K * M + M + 3 + 24) * s + 4)
    med = float(np.median(times))
    print(json.dumps(dict(kernel=f"k_outbs_sepwisw<{'float' if a.prec == 'sp' else 'double'}, true>", prec=a.prec, worst=a.worst, npts=n, iters=a.iters, median_s=med, min_s=float(np.min(times)),
                          max_s=float(np.max(times)), bytes=nbytes, bytes_per_s=nbytes / med, hbm_peak_share=nbytes / med / HBM_PEAK,
                          trains_per_point=np.bincount(ntr, minlength=4).tolist())))
    ctx.close()


if __name__ == "__main__":
    main()
