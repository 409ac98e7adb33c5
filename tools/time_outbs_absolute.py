"""Time ecwam_hip_outbs_absolute (the absolute-frame output spectrum FL2ND and the eight parameters that read it) at the O320 size:
device-event median over --iters calls on synthetic spectra with the currents of ecwam_amd.synthetic.currents on the O320 grid, with and
without the store of FL2ND, next to ecwam_hip_outbs on the same FL1 (what five of the columns cost without the transform), the calls
alternating in one process.  Algorithmic bytes per call = points x (FL1 + WAVNUM + 2 currents + 16 FF + 8 outputs [+ FL2ND]) reals, and the
share of the HBM peak they imply.  Prints one JSON line.  ECWAM_HIP_LIB=<another build of this source> with --only outbs times that
build's ecwam_hip_outbs (a library of an earlier commit lacks the new symbol and needs that commit's Python package).  What was
measured: profiles/outbs_absolute_O320.txt.  Run the kernel-time measurement under `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own.

usage: python tools/time_outbs_absolute.py [--prec sp|dp] [--iters 50] [--warmup 5] [--only outbs] [--irefra 2] [--ice]
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
    ap.add_argument("--ng", type=int, default=320)            # O320: 421 080 sea points
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["outbs"], default=None)
    ap.add_argument("--irefra", type=int, default=2)
    ap.add_argument("--ice", action="store_true")             # LICERUN = T, LMASKICE = F: the noise reshaping on top
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api, grid as G, synthetic as syn
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    dt = np.float32 if a.prec == "sp" else np.float64
    t = Tables(Config(nang=36, nfre=36, nfre_red=36, irefra=a.irefra, licerun=True, lmaskice=not a.ice), dt)
    ctx = api.HipContext(t)
    dev, tdt = ctx.device, ctx.dtype
    g = G.build_grid(a.ng)
    n, K, M = g.nsea, 36, 36
    ug, vg = syn.currents(g)
    u = torch.from_numpy(np.ascontiguousarray(ug, dt)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(vg, dt)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    fr = torch.from_numpy(np.asarray(t.FR, np.float64)).to(dev, tdt)
    th = torch.from_numpy(np.asarray(t.TH, np.float64)).to(dev, tdt)
    # spectra: a wind sea along the wind and a swell against it, random peak frequencies and directions
    wd = torch.rand(n, device=dev, generator=gen, dtype=tdt) * 6.2832
    fp1 = 0.12 + 0.15 * torch.rand(n, device=dev, generator=gen, dtype=tdt)
    fp2 = 0.05 + 0.05 * torch.rand(n, device=dev, generator=gen, dtype=tdt)
    spec = lambda fp, amp: amp * fr[None, None, :] ** -5 * torch.exp(-1.25 * (fp[:, None, None] / fr[None, None, :]) ** 4)
    c1 = torch.clamp(torch.cos(th[None, :] - wd[:, None]), min=0.0) ** 2
    c2 = torch.clamp(-torch.cos(th[None, :] - wd[:, None]), min=0.0) ** 2
    fl1 = (spec(fp1, 1e-3) * c1[:, :, None] + spec(fp2, 2e-4) * c2[:, :, None]).contiguous()
    wv = torch.zeros((n, api.NWPR, M), dtype=tdt, device=dev)
    wv[:, 0] = (2 * np.pi) ** 2 / 9.806 * fr[None, :] ** 2                  # deep water
    ff = torch.zeros((n, api.NFF), dtype=tdt, device=dev)
    ff[:, 2] = torch.rand(n, device=dev, generator=gen, dtype=tdt)
    ff[:, 3] = 25.0 * torch.rand(n, device=dev, generator=gen, dtype=tdt)
    out5 = torch.zeros((n, 5), dtype=tdt, device=dev)
    out8 = torch.zeros((n, 8), dtype=tdt, device=dev)
    fl2nd = torch.empty_like(fl1)
    s = np.dtype(dt).itemsize
    calls = {"outbs": (lambda: ctx.outbs(0, n, fl1, out5), n * (K * M + 5) * s)}
    if a.only is None:
        per_point = K * M + M + 2 + api.NFF + 8
        calls["absolute"] = (lambda: ctx.outbs_absolute(0, n, fl1, wv, u, v, ff, out8), n * per_point * s)
        calls["absolute_store"] = (lambda: ctx.outbs_absolute(0, n, fl1, wv, u, v, ff, out8, fl2nd=fl2nd), n * (per_point + K * M) * s)
    for _ in range(a.warmup):
        for fn, _b in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.iters):
        for k, (fn, _b) in calls.items():                                    # alternating: the same clocks and neighbours for every call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    assert bool(torch.isfinite(out5).all()) and bool(torch.isfinite(out8).all())
    res = dict(lib=os.environ.get("ECWAM_HIP_LIB", "product"), prec=a.prec, npts=n, iters=a.iters, irefra=a.irefra, ice=bool(a.ice),
               current_rms=float(np.sqrt(np.mean(ug ** 2 + vg ** 2))))
    for k, (_fn, nbytes) in calls.items():
        med = float(np.median(times[k]))
        res[k] = dict(median_s=med, min_s=float(np.min(times[k])), max_s=float(np.max(times[k])), bytes=nbytes, bytes_per_s=nbytes / med,
                      hbm_peak_share=nbytes / med / HBM_PEAK)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
