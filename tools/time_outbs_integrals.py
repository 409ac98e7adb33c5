"""Time ecwam_hip_outbs_integrals (all groups, the reference's seven bands) at the O320 size: device-event median over --iters calls on
synthetic spectra, with FL2ND = FL1 and with a separate FL2ND (a second buffer), next to ecwam_hip_outbs_sepwisw on the same FL1 -- the calls
alternating in one process -- and to the HBM roofline of one read of the spectrum (two with a separate FL2ND).  Prints one JSON line per
precision.

usage: python tools/time_outbs_integrals.py [--prec sp|dp|both] [--iters 20] [--warmup 3] [--nang 36]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # MI355X, bytes/s


def run(prec: str, a) -> dict:
    import numpy as np
    import torch

    from ecwam_amd import api, grid as G
    from ecwam_amd.tables import Config, Tables

    dt = np.float32 if prec == "sp" else np.float64
    t = Tables(Config(nang=a.nang, nfre=36, nfre_red=36), dt)
    ctx = api.HipContext(t)
    ctx.set_outbs_integrals()
    nb = len(ctx.integral_bands)
    dev, tdt = ctx.device, ctx.dtype
    n, K, M = G.build_grid(a.ng).nsea, a.nang, 36
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    fr = torch.from_numpy(np.asarray(t.FR, np.float64)).to(dev, tdt)
    th = torch.from_numpy(np.asarray(t.TH, np.float64)).to(dev, tdt)
    wd = torch.rand(n, device=dev, generator=gen, dtype=tdt) * 6.2832
    fp1 = 0.12 + 0.15 * torch.rand(n, device=dev, generator=gen, dtype=tdt)
    fp2 = 0.05 + 0.05 * torch.rand(n, device=dev, generator=gen, dtype=tdt)
    spec = lambda fp, amp: amp * fr[None, None, :] ** -5 * torch.exp(-1.25 * (fp[:, None, None] / fr[None, None, :]) ** 4)
    c1 = torch.clamp(torch.cos(th[None, :] - wd[:, None]), min=0.0) ** 2
    c2 = torch.clamp(-torch.cos(th[None, :] - wd[:, None]), min=0.0) ** 2
    fl1 = (spec(fp1, 1e-3) * c1[:, :, None] + spec(fp2, 2e-4) * c2[:, :, None]).contiguous()
    fl2 = (fl1 * 1.01).contiguous()
    xllws = (fl1 > fl1.amax(dim=(1, 2), keepdim=True) * 0.1).to(tdt).contiguous()
    wv = torch.zeros((n, api.NWPR, M), dtype=tdt, device=dev)
    wv[:, 0] = (2 * np.pi) ** 2 / 9.806 * fr[None, :] ** 2                  # deep water: WAVNUM, CGROUP, CINV
    wv[:, 1] = 9.806 / (4 * np.pi * fr[None, :])
    wv[:, 2] = 2 * np.pi * fr[None, :] / 9.806
    ff = torch.zeros((n, api.NFF), dtype=tdt, device=dev)
    ff[:, 1], ff[:, 3], ff[:, 7], ff[:, 8], ff[:, 12], ff[:, 15] = wd, 10.0, 0.35, 0.05, 0.018, 5000.0
    ff[::4, 13] = 1.0                                                        # sea ice on a quarter of the points: AKI_ICE iterates there
    oi = torch.zeros((n, 8 + nb), dtype=tdt, device=dev)
    o15 = torch.zeros((n, 15), dtype=tdt, device=dev)
    calls = {"sepwisw": lambda: ctx.outbs_sepwisw(0, n, fl1, xllws, wv, ff, o15),
             "integrals_fl2nd_is_fl1": lambda: ctx.outbs_integrals(0, n, fl1, wv, ff, oi),
             "integrals_separate_fl2nd": lambda: ctx.outbs_integrals(0, n, fl1, wv, ff, oi, fl2nd=fl2)}
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.iters):
        for k, fn in calls.items():                                          # alternating: the same clocks and neighbours for every call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    assert bool(torch.isfinite(oi).all())
    row = n * K * M * np.dtype(dt).itemsize
    res = dict(prec=prec, npts=n, nang=a.nang, nband=nb, iters=a.iters, spectrum_bytes=row, hbm_roofline_one_read_s=row / HBM_PEAK,
               hbm_roofline_two_reads_s=2 * row / HBM_PEAK)
    for k in calls:
        res[k] = dict(median_s=float(np.median(times[k])), min_s=float(np.min(times[k])), max_s=float(np.max(times[k])))
    res["integrals_over_sepwisw"] = res["integrals_fl2nd_is_fl1"]["median_s"] / res["sepwisw"]["median_s"]
    ctx.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", choices=["sp", "dp", "both"], default="both")
    ap.add_argument("--ng", type=int, default=320)            # O320: 421 080 sea points
    ap.add_argument("--nang", type=int, default=36)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    for prec in (("sp", "dp") if a.prec == "both" else (a.prec,)):
        print(json.dumps(run(prec, a)), flush=True)


if __name__ == "__main__":
    main()
