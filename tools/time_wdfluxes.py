"""Time ecwam_hip_wdfluxes next to ecwam_hip_implsch at the O320 size: device-event median over --iters calls on the synthetic state of the
driver (ecwam_amd.wamintgr.Wamintgr.init_synthetic), the two calls alternating in one process.  IMPLSCH advances its operands, so each of its
calls gets a fresh copy of the spectrum and the forcing (copied outside the timed region); WDFLUXES only reads them.  Prints one JSON line per
precision.

usage: python tools/time_wdfluxes.py [--prec sp|dp|both] [--ng 320] [--nang 36] [--iters 10] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(prec: str, a) -> dict:
    import numpy as np
    import torch

    from ecwam_amd import grid as G
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=a.nang, nfre=36, nfre_red=36, idelt=450, idelpro=450)
    m = Wamintgr(cfg, G.build_grid(a.ng), prec)
    m.init_synthetic(seed=12345)
    n, ctx = m.n, m.ctx
    assert ctx.wdfluxes_supported()
    ctx.implsch_reserve(n)
    fl, ff, intf = m.fl1.clone(), m.ff.clone(), m.intf.clone()

    def implsch():
        ctx.implsch(0, n, fl, m.wvprpt, ff, intf, m.mij, m.xllws)

    def wdfluxes():
        ctx.wdfluxes(0, n, m.fl1, m.wvprpt, m.ff, m.intf, m.mij, m.xllws)

    calls = {"implsch": implsch, "wdfluxes": wdfluxes}
    times = {k: [] for k in calls}
    for it in range(a.warmup + a.iters):
        for k, fn in calls.items():      # alternating: the same clocks and neighbours for both
            if k == "implsch":
                fl.copy_(m.fl1)
                ff.copy_(m.ff)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e-3)
    assert bool(torch.isfinite(m.intf[:n]).all()) and bool((m.mij[:n] >= 1).all())
    res = dict(prec=prec, npts=n, nang=a.nang, iters=a.iters)
    for k in calls:
        res[k] = dict(median_s=float(np.median(times[k])), min_s=float(np.min(times[k])), max_s=float(np.max(times[k])))
    res["wdfluxes_over_implsch"] = res["wdfluxes"]["median_s"] / res["implsch"]["median_s"]
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", choices=["sp", "dp", "both"], default="sp")
    ap.add_argument("--ng", type=int, default=320)            # O320: 421 080 sea points
    ap.add_argument("--nang", type=int, default=36)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    for prec in (("sp", "dp") if a.prec == "both" else (a.prec,)):
        print(json.dumps(run(prec, a)), flush=True)


if __name__ == "__main__":
    main()
