"""Time ecwam_hip_outbs_sepwisw (wind sea / swell + mean-period / spread parameters) at the O320 size: device-event median over --iters
calls on synthetic spectra, with the algorithmic bytes per call (FL1 + XLLWS + CINV + 3 FF scalars + 15 outputs per point) and the share of
the HBM peak they imply.  Prints one JSON line.  Run the kernel-time measurement under `rocprofv3 --kernel-trace --stats -- python ...`
in a run of its own.

usage: python tools/time_outbs_sepwisw.py [--prec sp|dp] [--npts 421080] [--iters 50] [--warmup 5]
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
    ap.add_argument("--prec", choices=["sp", "dp"], default="sp")
    ap.add_argument("--npts", type=int, default=421080)       # O320 sea points
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    dt = np.float32 if a.prec == "sp" else np.float64
    t = Tables(Config(nang=36, nfre=36, nfre_red=36), dt)
    ctx = api.HipContext(t)
    dev, tdt = ctx.device, ctx.dtype
    n, K, M = a.npts, 36, 36
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    fr = torch.from_numpy(np.asarray(t.FR, np.float64)).to(dev, tdt)
    th = torch.from_numpy(np.asarray(t.TH, np.float64)).to(dev, tdt)
    # spectra: a wind sea along the wind and a swell against it, random peak frequencies and directions
    wd = torch.rand(n, device=dev, generator=g, dtype=tdt) * 6.2832
    fp1 = 0.12 + 0.15 * torch.rand(n, device=dev, generator=g, dtype=tdt)
    fp2 = 0.05 + 0.05 * torch.rand(n, device=dev, generator=g, dtype=tdt)
    spec = lambda fp, amp: amp * fr[None, None, :] ** -5 * torch.exp(-1.25 * (fp[:, None, None] / fr[None, None, :]) ** 4)
    c1 = torch.clamp(torch.cos(th[None, :] - wd[:, None]), min=0.0) ** 2
    c2 = torch.clamp(-torch.cos(th[None, :] - wd[:, None]), min=0.0) ** 2
    fl1 = (spec(fp1, 1e-3) * c1[:, :, None] + spec(fp2, 2e-4) * c2[:, :, None]).contiguous()
    xllws = ((c1[:, :, None] > 0.25) & (fr[None, None, :] > fp1[:, None, None])).to(tdt).contiguous()
    wv = torch.zeros((n, api.NWPR, M), dtype=tdt, device=dev)
    wv[:, 2] = (2 * np.pi / 9.806) * fr[None, :]
    ff = torch.zeros((n, api.NFF), dtype=tdt, device=dev)
    ff[:, 1] = wd
    ff[:, 7] = 0.2 + 0.4 * torch.rand(n, device=dev, generator=g, dtype=tdt)
    out = torch.zeros((n, 15), dtype=tdt, device=dev)
    for _ in range(a.warmup):
        ctx.outbs_sepwisw(0, n, fl1, xllws, wv, ff, out)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.outbs_sepwisw(0, n, fl1, xllws, wv, ff, out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    assert bool(torch.isfinite(out).all())
    s = np.dtype(dt).itemsize
    nbytes = n * (2 * K * M + M + 3 + 15) * s
    med = float(np.median(times))
    print(json.dumps(dict(kernel=f"k_outbs_sepwisw<{'float' if a.prec == 'sp' else 'double'}, false>", prec=a.prec, npts=n, iters=a.iters, median_s=med, min_s=float(np.min(times)),
                          max_s=float(np.max(times)), bytes=nbytes, bytes_per_s=nbytes / med, hbm_peak_share=nbytes / med / HBM_PEAK)))
    ctx.close()


if __name__ == "__main__":
    main()
