"""Generates tests/golden/reference_*.npz by RUNNING the reference's own Fortran -- IMPLSCH with its call tree, WDFLUXES, NEWWIND, DEPTHPRPT, CTUWINI + CTUW
and PROPAGS2 -- through oracle/reference.py (oracle/_ref/libecwam_ref_{sp,dp}.so, built from the reference tree by oracle/ref_build.py), in double
and in single precision.  The fixtures hold data only: the inputs (float32-representable, so that both precisions see the same numbers) and
what the reference returned.  Only usable where the reference tree exists.

Discrete decisions.  MIJ and XLLWS are discrete and these samples are too small for a flip budget, so a candidate point at which the
reference's OWN two precisions disagree on MIJ or XLLWS is dropped; at most 10 % of the candidates of a configuration may go (the share is
printed); if the reference alone exceeds that, the configuration's sea states have to change, not the cap.

    python tools/make_golden_reference.py [name ...]      (no name: every fixture)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_cases as RC  # noqa: E402
from ecwam_amd import grid as G, synthetic as syn  # noqa: E402
from ecwam_amd.tables import Config, Tables  # noqa: E402
from oracle.reference import Reference, available  # noqa: E402

MAX_DROP = 0.10


def point_fixture(name):
    n = RC.points(name)
    ncand = n + n // 10                      # what the cap allows to go
    cfg = RC.config(name)
    inp = RC.make_inputs(name, ncand, RC.CONFIGS[name]["seed"])
    res = {p: RC.run(Reference(cfg, p), inp, RC.kind(name)) for p in ("dp", "sp")}
    same = (res["dp"]["MIJ"] == res["sp"]["MIJ"]) & (res["dp"]["XLLWS"] == res["sp"]["XLLWS"]).all(axis=(1, 2))
    dropped = float((~same).sum()) / ncand
    keep = np.nonzero(same)[0][:n]
    print(f"{name}: {ncand} candidates, {int((~same).sum())} dropped ({100 * dropped:.1f} %: the reference's sp and dp disagree on MIJ / XLLWS), {keep.size} kept")
    if dropped > MAX_DROP or keep.size < n:
        raise SystemExit(f"{name}: the reference's own precisions disagree at more than {MAX_DROP:.0%} of the candidates: change the sea states")
    out = {p: {k: v[keep] for k, v in res[p].items()} for p in res}
    f = RC.save(name, RC.select(inp, keep), out, dropped)
    print(f"  {f}: {os.path.getsize(f)} bytes")


# ---- advection --------------------------------------------------------------------------------------------------------------------------
def advection_inputs(g, cfg, seed=5):
    """Group velocities [(n+1)][NFRE] (land slot: deep water) and a spectrum [(n+1)][NANG][NFRE] (land row zero), float32."""
    dt = np.float32
    t = Tables(cfg, dt)
    rng = np.random.default_rng(seed)
    depth = np.where(rng.uniform(0, 1, g.nsea) < 0.3, 10 ** rng.uniform(0.5, 3, g.nsea), 998.999).astype(dt)
    cg = np.zeros((g.nsea + 1, cfg.nfre), dt)
    cg[: g.nsea] = syn.depth_props(depth, t, dt)["CGROUP"]
    cg[g.nsea] = syn.depth_props(np.array([998.999], dt), t, dt)["CGROUP"][0]
    f1 = np.zeros((g.nsea + 1, cfg.nang, cfg.nfre), dt)
    f1[: g.nsea] = (rng.uniform(0, 1, (g.nsea, cfg.nang, cfg.nfre)) ** 4).astype(dt)
    return depth, cg, f1


def grid_arrays(g):
    return dict(n_oct=RC.ADV_NOCT, nsea=g.nsea, klon=np.asarray(g.klon, np.int32), klat=np.asarray(g.klat, np.int32), kcor=np.asarray(g.kcor, np.int32))


def advection_fixture(name):
    """12 x 25 on the smallest "continents" grid with land, both polar rows and the periodic seam: the reference's CTUW weights and PROPAGS2's F3;
    name "advection_split": the fast waves M <= IFRELFMAX = 12 with DELPRO_LF = IDELPRO / 2 (ctuwupdt.F90:220-256)."""
    g = G.build_grid(RC.ADV_NOCT, mask="continents")
    cfg = RC.advection_config()
    _, cg, f1 = advection_inputs(g, cfg)
    kw = dict(ifrelfmax=RC.ADV_IFRELFMAX, delpro_lf=cfg.idelpro / 2) if name == "advection_split" else {}
    d = dict(cg=cg, f1=f1, **grid_arrays(g))
    for p, T in (("dp", np.float64), ("sp", np.float32)):
        r = Reference(cfg, p)
        w = r.ctu_weights_wam(g, cg, cfg.idelpro, **kw)
        assert w["NFAIL"] == 0
        d[f"W8_{p}"] = RC.w8(Tables(cfg, T), w).astype(T)
        d[f"WLAT_{p}"], d[f"WCOR_{p}"] = w["WLAT"].astype(T), w["WCOR"].astype(T)
        d[f"F3_{p}"] = r.propags2(g, f1, w)[: g.nsea, :, : cfg.nfre_red].astype(T)
    f = RC.path(name)
    np.savez_compressed(f, **d)
    print(f"{name}: {g.nsea} sea points; {f}: {os.path.getsize(f)} bytes")


def fused_fixture(name):
    """One whole step at 36 x 36 in double precision (the one-kernel step's dp build exists at 36 directions only) on the same grid: the
    reference's PROPAGS2 with the reference's CTUW weights, followed by the reference's IMPLSCH."""
    g = G.build_grid(RC.ADV_NOCT, mask="continents")
    cfg = RC.fused_config()
    dt = np.float32
    t = Tables(cfg, dt)
    n = g.nsea
    depth, cg, _ = advection_inputs(g, cfg)
    p = syn.point_params(n, seed=4)
    p["DEPTH"] = depth.astype(np.float64)
    pr = syn.depth_props(depth, t, dt)
    f1 = np.zeros((n + 1, cfg.nang, cfg.nfre), dt)
    f1[:n] = syn.jonswap_spectra(t.FR, t.TH, p["FP"], p["THETAQ"], dt)
    wv = np.stack([pr[k] for k in ("WAVNUM", "CGROUP", "CINV", "XK2CG", "STOKFAC")], 1).astype(dt)
    ff = syn.forcing(p, slice(0, n), t, dt).astype(dt)
    env = np.stack([pr["EMAXDPT"], depth], 1).astype(dt)
    r = Reference(cfg, "dp")
    w = r.ctu_weights(g, cg, float(cfg.idelpro))
    assert w["NFAIL"] == 0
    f3 = r.propags2(g, f1, w)
    o = r.implsch(f3[:n], wv[:, 0], wv[:, 1], wv[:, 2], wv[:, 3], wv[:, 4], env, ff, np.zeros((n, 15)))
    assert np.isin(o["XLLWS"], (0.0, 1.0)).all()
    f = RC.path(name)
    np.savez_compressed(f, cg=cg, f1=f1, WV=wv, FF=ff, ENV=env, F3_dp=f3[:n], FL1_dp=o["FL1"], MIJ=o["MIJ"], XLLWS=o["XLLWS"].astype(np.uint8),
                        FF_dp=o["FF"], INTF_dp=o["INTF"], **grid_arrays(g))
    print(f"{name}: {n} sea points; {f}: {os.path.getsize(f)} bytes")


def newwind_fixture(name):
    """NEWWIND at ICODE 3, 1 and 2 on forcing on both sides of its two reset thresholds: FF_NOW after the call, both precisions."""
    ff, ffn = RC.newwind_inputs()
    d = dict(ff=ff, ffn=ffn)
    for icode in RC.NEWWIND_ICODES:
        for p, T in (("dp", np.float64), ("sp", np.float32)):
            d[f"out_icode{icode}_{p}"] = Reference(RC.newwind_config(icode), p).newwind(ff, ffn).astype(T)
    f = RC.path(name)
    np.savez_compressed(f, **d)
    print(f"{name}: {ff.shape[0]} points; {f}: {os.path.getsize(f)} bytes")


def depthprpt_fixture(name):
    """DEPTHPRPT + AKI (and EMAXDPT of initdpthflds.F90:64-75) over the whole depth range, both precisions."""
    depth = RC.depthprpt_depths()
    d = dict(depth=depth)
    for p, T in (("dp", np.float64), ("sp", np.float32)):
        r = Reference(RC.newwind_config(3), p).depthprpt(depth)
        for k in RC.DEPTHPRPT_KEYS:
            d[f"{k}_{p}"] = r[k].astype(T)
    f = RC.path(name)
    np.savez_compressed(f, **d)
    print(f"{name}: {depth.size} depths; {f}: {os.path.getsize(f)} bytes")


OTHER = {"newwind": newwind_fixture, "depthprpt": depthprpt_fixture, "advection_12x25": advection_fixture, "advection_split": advection_fixture, "fused_36_dp": fused_fixture}


def main():
    if not available():
        sys.exit("the reference libraries are not built: python -c 'from oracle import ref_build; ref_build.build()' where the reference tree exists")
    names = sys.argv[1:] or list(RC.CONFIGS) + list(OTHER)
    for name in names:
        (OTHER[name] if name in OTHER else point_fixture)(name)
    tot = sum(os.path.getsize(os.path.join(RC.GOLDEN, f)) for f in os.listdir(RC.GOLDEN) if f.startswith("reference_") and f.endswith(".npz"))
    print(f"all reference fixtures together: {tot} bytes")


if __name__ == "__main__":
    main()
