"""Time ecwam_hip_outbs_second_order (the output spectrum FL2ND with CAL_SECOND_ORDER_SPEC and the eight parameters that read it) at the
O320 size, without currents: device-event median over --iters calls on synthetic spectra, next to ecwam_hip_outbs_absolute on the same
FL1 (the pipeline without the correction), the calls alternating in one process.  Two depth fields: "deep" (5000 m everywhere: one depth
index, the LLSAMEDPTH case) and "mixed" (log-uniform between 5 m and 5000 m, independent from point to point: the worst case for a
wavefront, which then repeats the sum for every distinct depth index among its 64 points), and "shelf" (an estimate of a real depth
field: 87 % of the points deep, the rest in runs of 256 consecutive points that ramp from 20 m to 2000 m, about six indices per wavefront).  Derived flop count per point: SECSPOM's
NANGH**2 NFREH**2 terms x 14 flops (TA term 5: two products, a sum, a multiply-add; XINCR term 9: 2 TB F2, TC F, two Stokes products and
their difference, two sums, a multiply-add), and the share of the vector peak that implies; table bytes per wavefront and depth index:
5 NANGH NFREH**2 reals; spectrum bytes per point: FL1 read twice, NANGH (NMAX + NFREH) work reals written and read.  Prints one JSON line.
What was measured: profiles/outbs_second_order_O320.txt.

usage: python tools/time_outbs_second_order.py [--prec sp|dp] [--iters 20] [--warmup 3] [--nang 36]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VECTOR_PEAK = dict(sp=157.3e12, dp=78.6e12)     # MI355X vector FP32 / FP64, flop/s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", choices=["sp", "dp"], default="sp")
    ap.add_argument("--ng", type=int, default=320)            # O320: 421 080 sea points
    ap.add_argument("--nang", type=int, default=36)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    from ecwam_amd import api, grid as G
    from ecwam_amd.second_order import SecondOrderTables
    from ecwam_amd.tables import Config, Tables

    assert torch.cuda.is_available(), "needs a GPU"
    dt = np.float32 if a.prec == "sp" else np.float64
    t = Tables(Config(nang=a.nang, nfre=36, nfre_red=36), dt)
    so = SecondOrderTables(t)
    ctx = api.HipContext(t)
    ctx.set_second_order(so)
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
    wv = torch.zeros((n, api.NWPR, M), dtype=tdt, device=dev)
    wv[:, 0] = (2 * np.pi) ** 2 / 9.806 * fr[None, :] ** 2                  # deep water
    ff = torch.zeros((n, api.NFF), dtype=tdt, device=dev)
    deep = torch.full((n,), 5000.0, dtype=tdt, device=dev)
    mixed = (5.0 * 1000.0 ** torch.rand(n, device=dev, generator=gen, dtype=tdt)).contiguous()
    ramp = 20.0 * 100.0 ** (torch.arange(256, device=dev, dtype=tdt) / 255.0)
    shelf = deep.clone()
    for start in range(0, n - 256, 2048):                                   # 256 of every 2048 points: 12.5 %
        shelf[start:start + 256] = ramp
    out8 = torch.zeros((n, 8), dtype=tdt, device=dev)
    calls = {"absolute": lambda: ctx.outbs_absolute(0, n, fl1, wv, None, None, ff, out8),
             "second_order_deep": lambda: ctx.outbs_second_order(0, n, fl1, wv, deep, None, None, ff, out8),
             "second_order_shelf": lambda: ctx.outbs_second_order(0, n, fl1, wv, shelf, None, None, ff, out8),
             "second_order_mixed": lambda: ctx.outbs_second_order(0, n, fl1, wv, mixed, None, None, ff, out8)}
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
    assert bool(torch.isfinite(out8).all())
    s = np.dtype(dt).itemsize
    AH, NH = so.NANGH, so.NFREH
    flops = n * (AH * NH) ** 2 * 14
    res = dict(prec=a.prec, npts=n, nang=a.nang, iters=a.iters, flops_per_call=flops, table_slice_bytes=5 * AH * NH * NH * s,
               spectrum_bytes_per_call=n * (2 * K * M + 2 * AH * (so.NMAX + NH)) * s)
    for k in calls:
        med = float(np.median(times[k]))
        res[k] = dict(median_s=med, min_s=float(np.min(times[k])), max_s=float(np.max(times[k])))
        if k != "absolute":
            res[k].update(flops_per_s=flops / med, vector_peak_share=flops / med / VECTOR_PEAK[a.prec])
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
