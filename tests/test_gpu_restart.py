"""The six calls of include/ecwam_hip_restart.h and the Wamintgr methods over them on the device (run with -m gpu), against the reference's own
results: tests/golden/reference_depthprpt.npz (DEPTHPRPT / AKI on 70 depths) and tests/golden/restart_0.npz (BUILDSTRESS with GETSTRESS's statements
around it on 67 rows; the bytes of the BLS and LAW files WRITEFL and WRITESTRESS wrote, LL1D and relabelled), both precisions.

The gates are tests/restart_ref.py::device_gate, read from tests/golden/restart_observed.json: single precision 4 x the reference's own single
against double precision, double precision 10 x what a float64 restatement showed against the reference (8 eps where that was exactly 0); per column
or array |a - b| / max(|b|, the column's largest |b|).  Nothing in a gate comes from the device.  The pack and unpack calls have no gate: bit for
bit.  67 rows and 91 cells are no whole number of wavefronts, tiles or 16-byte pieces; the sub-range [5, 61) begins and ends inside a tile."""
import ctypes as C
import os

import numpy as np
import pytest

import harness as H
import reference_cases as RC
import restart_ref as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = F.SENT
KIJS, KIJL, LD = 5, 61, 80
ND = 70      # the depths of the fixture; row 70 is the land row


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _up(ctx, a, T):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=T)).to(ctx.device)


def _sent(ctx, *shape):
    return torch.full(shape, SENT, dtype=ctx.dtype, device=ctx.device)


@pytest.fixture(scope="module")
def depth_fixture():
    with np.load(os.path.join(F.GOLDEN, "reference_depthprpt.npz")) as z:
        return {k: z[k] for k in z.files}


def _depths(prec):
    t = F.tables(prec)
    return np.concatenate([RC.depthprpt_depths(), [np.float32(t.BATHYMAX)]]).astype(F.dtype_of(prec))


def _depthprpt(ctx, prec, kijs=0, kijl=ND + 1, skip=None, rows=ND + 1):
    """one call into sentinel-filled buffers: {name: numpy}"""
    out = dict(wvprpt=_sent(ctx, rows, 5, F.NFRE), wavnum=_sent(ctx, rows, F.NFRE), cgroup=_sent(ctx, rows, F.NFRE), omosnh2kd=_sent(ctx, rows, F.NFRE),
               ff=_sent(ctx, rows, F.NFF))
    d = _up(ctx, _depths(prec)[:rows], F.dtype_of(prec))
    ctx.depthprpt(kijs, kijl, d, **{k: (None if k == skip else v) for k, v in out.items()})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. DEPTHPRPT
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_depthprpt_against_the_reference(api, prec, depth_fixture):
    """The 70 depths of the fixture and a land row, every output within the gates; the land row is the row of the fixture's BATHYMAX depth."""
    T = F.dtype_of(prec)
    ctx = api.HipContext(F.tables(prec))
    try:
        got = _depthprpt(ctx, prec)
    finally:
        ctx.close()
    ref = {k: depth_fixture[f"{k}_{prec}"] for k in RC.DEPTHPRPT_KEYS}
    # EMAXDPT of that fixture is oracle/ref_driver.F90's statement without the reduction of GAM below 4 m: the reference's own statement
    # (initdpthflds.F90:61-73) is recorded in restart_0.npz, equal to the fixture's from 4 m on
    ref["EMAXDPT"] = F.load_golden()[f"emaxdpt_{prec}"]
    d = RC.depthprpt_depths()
    assert _bits(ref["EMAXDPT"][d >= 4], depth_fixture[f"EMAXDPT_{prec}"][d >= 4]) and (d < 4).sum() > 3
    mine = dict(WAVNUM=got["wvprpt"][:, 0], CGROUP=got["wvprpt"][:, 1], CINV=got["wvprpt"][:, 2], XK2CG=got["wvprpt"][:, 3], STOKFAC=got["wvprpt"][:, 4],
                OMOSNH2KD=got["omosnh2kd"], EMAXDPT=got["ff"][:, 14])
    assert _bits(got["wavnum"], mine["WAVNUM"]) and _bits(got["cgroup"], mine["CGROUP"]) and _bits(got["ff"][:, 15], _depths(prec))
    assert (got["ff"][:, :14] == T(SENT)).all()
    bad = {}
    for k in RC.DEPTHPRPT_KEYS:
        a, b = mine[k][:ND].reshape(ND, -1), ref[k].reshape(ND, -1)
        err, gate = float(F.rel_error(a, b).max()), F.device_gate("depthprpt", k, prec)
        print(f"DEPTHPRPT {k} {prec}: device against the reference {err:.3e} (gate {gate:.3e})")
        if not err <= gate:
            bad[k] = (err, gate)
    assert not bad, bad
    # the switches fall as the reference's: deep water where it has OMOSNH2KD = 0
    assert np.array_equal(mine["OMOSNH2KD"][:ND] == 0, ref["OMOSNH2KD"] == 0)
    deep = int(np.nonzero(RC.depthprpt_depths() == np.float32(998.999))[0][0])
    for k in RC.DEPTHPRPT_KEYS:
        assert _bits(mine[k][ND], mine[k][deep]), k      # WVPRPT_LAND


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_depthprpt_ranges_and_null_outputs(api, prec):
    """Rows [3, 67): everything outside keeps its sentinel, and so do the columns of ff other than 14 and 15; each output NULL in turn; one call or
    two calls split at row 31 give the same bits."""
    T = F.dtype_of(prec)
    ctx = api.HipContext(F.tables(prec))
    try:
        full = _depthprpt(ctx, prec)
        part = _depthprpt(ctx, prec, 3, 67)
        for k, a in part.items():
            assert (a[:3] == T(SENT)).all() and (a[67:] == T(SENT)).all(), k
            assert _bits(a[3:67], full[k][3:67]), k
        assert (part["ff"][:, :14] == T(SENT)).all() and not (part["ff"][3:67, 14:] == T(SENT)).any()
        for skip in ("wvprpt", "wavnum", "cgroup", "omosnh2kd", "ff"):
            one = _depthprpt(ctx, prec, skip=skip)
            for k, a in one.items():
                assert (a == T(SENT)).all() if k == skip else _bits(a, full[k]), (skip, k)
        out = dict(wvprpt=_sent(ctx, ND + 1, 5, F.NFRE), wavnum=_sent(ctx, ND + 1, F.NFRE), cgroup=_sent(ctx, ND + 1, F.NFRE), omosnh2kd=_sent(ctx, ND + 1, F.NFRE),
                   ff=_sent(ctx, ND + 1, F.NFF))
        d = _up(ctx, _depths(prec), T)
        ctx.depthprpt(0, 31, d, **out)
        ctx.depthprpt(31, ND + 1, d, **out)
        ctx.depthprpt(40, 40, d, **out)      # an empty range launches nothing
        torch.cuda.synchronize()
        for k, v in out.items():
            a = v.cpu().numpy()
            assert _bits(a[:, 14:] if k == "ff" else a, full[k][:, 14:] if k == "ff" else full[k]), k
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_depthprpt_known_answers(api, prec):
    """Deep water: WAVNUM = OM**2 / G and CGROUP = G / (4 PI FR), the same IEEE operations, bit for bit; everywhere OM**2 = G K TANH(K D) to the
    tolerance of AKI's Newton iteration (a step below EBS = 1e-4 of the iterate leaves a residual far below 2 EBS)."""
    T = F.dtype_of(prec)
    t = F.tables(prec)
    ctx = api.HipContext(t)
    try:
        got = _depthprpt(ctx, prec)
    finally:
        ctx.close()
    d = _depths(prec)
    om, fr, g = np.asarray(t.ZPIFR, T), np.asarray(t.FR, T), T(t.G)
    ak = got["wavnum"]
    start = np.maximum(om[None, :] * om[None, :] / (T(4) * g), om[None, :] / (T(2) * np.sqrt(g * d[:, None])))
    exit0 = d[:, None] * start > T(40)      # BO > DKMAX at the start value
    assert exit0.any() and not exit0.all()
    want = np.broadcast_to(om * om / g, ak.shape)
    assert _bits(ak[exit0], want[exit0])
    deep = ak * d[:, None] > T(10)
    gh = g / (T(4) * T(t.PI))
    assert deep.any() and _bits(got["cgroup"][deep], np.broadcast_to(gh / fr, ak.shape)[deep]) and (got["omosnh2kd"][deep] == 0).all()
    akd = ak.astype(np.float64) * d[:, None].astype(np.float64)
    res = np.abs(om.astype(np.float64)[None, :] ** 2 - float(g) * ak.astype(np.float64) * np.tanh(akd)) / om.astype(np.float64)[None, :] ** 2
    print(f"dispersion relation {prec}: largest relative residual {res.max():.3e}")
    assert res.max() <= 2e-4


@pytest.mark.parametrize("nang,prec,irefra", [(12, "sp", 0), (36, "sp", 0), (12, "dp", 0), (36, "dp", 0), (12, "sp", 2)])
def test_initdpthflds_of_the_driver(api, nang, prec, irefra):
    """Wamintgr.initdpthflds() reproduces what init_synthetic computed on the host and uploaded, within the gates of DEPTHPRPT, and one step
    afterwards agrees with a twin model within the step gates of tests/harness.py.  EMAXDPT is compared with the host's where the depth is at least
    4 m; below, ecwam_amd.synthetic.depth_props does not reduce GAM as initdpthflds.F90:66-70 does, and the device is compared with the
    reference's statement (tests/restart_ref.py::emaxdpt)."""
    from ecwam_amd import grid as grid_mod
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    T = F.dtype_of(prec)
    cfg = Config(nang=nang, nfre=36, nfre_red=36 if nang == 36 else 29, idelt=450, idelpro=450, irefra=irefra)
    g = grid_mod.build_grid(16, mask="continents")
    m, twin = Wamintgr(cfg, g, prec), Wamintgr(cfg, g, prec)
    try:
        m.init_synthetic(seed=5)
        twin.init_synthetic(seed=5)
        n = m.n
        names = ["wvprpt", "cgroup_ext"] + (["omosnh2kd_ext", "wavnum_ext"] if irefra else [])
        host = {k: getattr(m, k).cpu().numpy().copy() for k in names}
        host["ff"] = m.ff.cpu().numpy().copy()
        for k in names:
            getattr(m, k).fill_(SENT)
        m.ff[:, 14] = SENT
        m.weights_ready = True
        depth = None
        if not irefra:      # the depths of the owned rows are in ff; there are no halo rows on one task
            assert m.nrows == n + 1
        m.initdpthflds(depth)
        torch.cuda.synchronize()
        assert m.weights_ready is False
        dev = {k: getattr(m, k).cpu().numpy() for k in names}
        ff = m.ff.cpu().numpy()
        assert _bits(ff[:, :14], host["ff"][:, :14]) and _bits(ff[:, 15], host["ff"][:, 15])
        pairs = {"WAVNUM": (dev["wvprpt"][:, 0], host["wvprpt"][:, 0]), "CGROUP": (dev["cgroup_ext"], host["cgroup_ext"]), "CINV": (dev["wvprpt"][:, 2], host["wvprpt"][:, 2]),
                 "XK2CG": (dev["wvprpt"][:, 3], host["wvprpt"][:, 3]), "STOKFAC": (dev["wvprpt"][:, 4], host["wvprpt"][:, 4])}
        assert _bits(dev["wvprpt"][:, 1], dev["cgroup_ext"][:n])
        if irefra:
            pairs["OMOSNH2KD"] = (dev["omosnh2kd_ext"], host["omosnh2kd_ext"])
            assert _bits(dev["wavnum_ext"][:n], dev["wvprpt"][:, 0])
            pairs["WAVNUM"] = (dev["wavnum_ext"], host["wavnum_ext"])
        d = ff[:, 15]
        shallow = d < T(4)
        assert shallow.any() and not shallow.all()
        pairs["EMAXDPT"] = (ff[:, 14][:, None], np.where(shallow, F.emaxdpt(d, prec), host["ff"][:, 14])[:, None])
        bad = {}
        for k, (a, b) in pairs.items():
            err, gate = float(F.rel_error(a, b).max()), F.device_gate("depthprpt", k, prec)
            print(f"initdpthflds {k} NANG {nang} {prec} IREFRA {irefra}: device against the host's upload {err:.3e} (gate {gate:.3e})")
            if not err <= gate:
                bad[k] = (err, gate)
        assert not bad, bad
        # the twin gets the reference's EMAXDPT below 4 m as well: the limit of the wave energy there is half the host's and less
        twin.ff[:, 14] = torch.from_numpy(pairs["EMAXDPT"][1][:, 0].astype(T)).to(twin.dev)
        m.step()
        twin.step()
        torch.cuda.synchronize()
        res = [dict(FL1=x.fl1[:n].cpu().numpy(), MIJ=x.mij.cpu().numpy(), XLLWS=x.xllws.cpu().numpy(), FF=x.ff.cpu().numpy()[:, :14], INTF=x.intf.cpu().numpy())
               for x in (twin, m)]
        st = H.compare_implsch(res[0], res[1], m.t)
        print("one step after initdpthflds against the twin:", RC.figures(dict(st, w2n_max_rel=0.0)))
        if prec == "sp":
            H.assert_sp_gates(st, n)
        else:
            fig = RC.figures(dict(st, w2n_max_rel=0.0))
            for q in ("bins", "swh", "ff", "intf"):
                assert fig[q] <= RC.CEILING[q], (q, fig[q])
    finally:
        m.ctx.close()
        twin.ctx.close()


# ---- 2. BUILDSTRESS
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("name", list(F.CASES))
def test_buildstress_against_the_reference(api, name, prec):
    """Every recorded case: the ten columns of ff from WSWAVE to CHRNCK within the gates; no flipped branch (the points at the floors EPSUS, Z0MIN
    and at the clip of TAUW, and the points that took the plane's wind speed, are the reference's); the columns the case does not write, and the rows
    outside the call, keep their bits.  The drag coefficient is not an output: which points took the plane's value shows in UFRIC, inside its gate."""
    T = F.dtype_of(prec)
    cap, has_cd, has_uw, zref, nse = F.CASES[name]
    inp, g = F.cached_inputs(), F.load_golden()
    ref = g[f"ff_{name}_{prec}"]
    ctx = api.HipContext(F.tables(prec, cap))
    try:
        ctx.set_forcing_map(inp["map_in"], F.NCELL)
        ff0 = np.full((F.N + 3, F.NFF), SENT, T)
        ff0[:F.N] = inp["ff"].astype(T)
        ff = _up(ctx, ff0, T)
        uw = _up(ctx, inp["uwave"], T) if has_uw else None
        cd = _up(ctx, inp["cd"], T) if has_cd else None
        ctx.buildstress(0, F.N, ff, uw, cd, zref, True, nse, F.PRCHAR, F.ZMISS)
        torch.cuda.synchronize()
        got = ff.cpu().numpy()
        # a sub-range on a fresh copy: the rows outside keep their bits
        ff2 = _up(ctx, ff0, T)
        ctx.buildstress(KIJS, KIJL, ff2, uw, cd, zref, True, nse, F.PRCHAR, F.ZMISS)
        ctx.buildstress(9, 9, ff2, uw, cd, zref, True, nse, F.PRCHAR, F.ZMISS)
        torch.cuda.synchronize()
        sub = ff2.cpu().numpy()
    finally:
        ctx.close()
    assert (got[F.N:] == T(SENT)).all()
    assert _bits(sub[KIJS:KIJL], got[KIJS:KIJL]) and _bits(sub[:KIJS], ff0[:KIJS]) and _bits(sub[KIJL:], ff0[KIJL:])
    got = got[:F.N]
    err = F.rel_error(got[:, :14], ref[:, :14])
    bad = {}
    for c in F.GATED:
        col = F.FF_NAMES[c]
        gate = F.device_gate(name, col, prec)
        print(f"BUILDSTRESS {name} {col} {prec}: device against the reference {err[c]:.3e} (gate {gate:.3e})")
        if not err[c] <= gate:
            bad[col] = (err[c], gate)
    assert not bad, bad
    written = {F.UFRIC, F.TAUW, F.TAUWDIR, F.Z0M, F.Z0B} | ({F.WSWAVE} if has_uw else set()) | ({F.CHRNCK} if has_cd or nse else set())
    for c in range(F.NFF):
        if c not in written:
            assert _bits(got[:, c], ff0[:F.N, c]), F.FF_NAMES[c] if c < 14 else c
    assert _bits(got[:, F.WSWAVE], ref[:, F.WSWAVE]) and _bits(got[:, F.TAUWDIR], ref[:, F.TAUWDIR]) and (got[:, F.Z0B] == 0).all()
    floors = lambda a: (a[:, F.UFRIC] == np.sqrt(T(F.tables(prec).EPSUS)), a[:, F.Z0M] == T(F.Z0MIN), F.tauw_zero(a, T))
    for mine, theirs, what in zip(floors(got), floors(ref), ("EPSUS", "Z0MIN", "TAUW = 0")):
        assert np.array_equal(mine, theirs), what
    if has_cd:
        # the CD replacement mask: recomputed from the inputs it is the reference's, and the device took the plane's value exactly there --
        # UFRIC**2 is CD MAX(WSWAVE**2, EPSU10**2) wherever that stays above EPSUS -- and Hersbach's CD elsewhere
        plane = inp["cd"].astype(T)[inp["map_in"]]
        mask = (plane != T(F.ZMISS)) & (plane > T(0))
        assert np.array_equal(mask, (g[f"branch_{name}"] & F.BR_CD) != 0) and mask.any() and not mask.all()
        tb = F.tables(prec, cap)
        ws = got[:, F.WSWAVE]
        wind2 = np.maximum(ws * ws, T(tb.EPSU10) * T(tb.EPSU10))
        cd_ref = g[f"cd_{name}_{prec}"]
        assert _bits(cd_ref[mask], plane[mask])
        open_ = ~floors(got)[0]      # UFRIC**2 above EPSUS
        want = np.sqrt(cd_ref * wind2)
        assert (mask & open_).any() and (~mask & open_).any()
        assert _bits(got[mask & open_, F.UFRIC], want[mask & open_])      # the plane's value, one product, one square root: the same bits
        rest = ~mask & open_
        assert F.rel_error(got[rest, F.UFRIC][:, None], want[rest][:, None])[0] <= F.device_gate(name, "UFRIC", prec)      # Hersbach's CD
        # and where the two sources of CD lie apart, UFRIC tells which of them was taken
        u10p = np.maximum(ws, T(tb.WSPMIN)).astype(np.float64)
        hers = np.minimum((F.C1CD + F.C2CD * u10p ** F.P1CD) * u10p ** F.P2CD, float(tb.CDMAX))
        apart = open_ & (plane > T(0)) & (np.abs(plane.astype(np.float64) - hers) > 1e-3 * hers)
        took = np.abs(got[:, F.UFRIC].astype(np.float64) ** 2 / wind2 - plane) <= 1e-5 * np.abs(plane)
        assert apart.sum() > 10 and np.array_equal(took[apart], mask[apart])
        assert np.array_equal(floors(ref)[2], (g[f"branch_{name}"] & F.BR_TAUW0) != 0) and np.array_equal(floors(ref)[0], (g[f"branch_{name}"] & F.BR_EPSUS) != 0)
    if nse:
        assert (got[:, F.TAUW] == 0).all() and (got[:, F.CHRNCK] == T(F.PRCHAR)).all()


# ---- 3. the restart fields and WRITEFL's record
def _state(nang, T):
    st = F.restart_state()
    if nang != F.NANG:
        ij, k, m = np.meshgrid(np.arange(F.N), np.arange(nang), np.arange(F.NFRE), indexing="ij")
        st["fl"] = ij + F.N * (k + nang * m) + 0.5
    return {k: np.ascontiguousarray(v, dtype=T) for k, v in st.items()}


def _payload(raw, T):
    """the payloads of the records of a file the reference wrote"""
    out, at = [], 0
    while at < raw.size:
        ln = int(raw[at:at + 4].view("<i4")[0])
        out.append(raw[at + 4:at + 4 + ln])
        assert int(raw[at + 4 + ln:at + 8 + ln].view("<i4")[0]) == ln
        at += ln + 8
    return out


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("prec", ["dp", "sp"])
@pytest.mark.parametrize("nang", [12, 36])
def test_savspec_pack(api, nang, prec, relabel):
    """All fields and rows: the record of writefl.F90:113 / :117 (the recorded file at NANG = 12, the numpy transposition at 36); the sub-range
    [5, 61) with ld = 80 and the fields [7, 57), which cross a frequency: everything outside the rows and fields of the call keeps its sentinel."""
    T = F.dtype_of(prec)
    st = _state(nang, T)
    perm = F.permutation() if relabel else None
    inv = np.argsort(perm) if relabel else np.arange(F.N)
    nf = nang * F.NFRE
    ctx = api.HipContext(F.tables(prec, True, nang))
    try:
        if relabel:
            ctx.set_restart_map(perm)
        fl = _up(ctx, st["fl"], T)
        blk = _sent(ctx, nf, F.N)
        ctx.savspec_pack(0, F.N, fl, blk, 0, relabel)
        sub = _sent(ctx, 50, LD)
        ctx.savspec_pack(KIJS, KIJL, fl, sub, 7, relabel)
        ctx.savspec_pack(20, 20, fl, sub, 7, relabel)
        torch.cuda.synchronize()
        rec, sub = blk.cpu().numpy(), sub.cpu().numpy()
    finally:
        ctx.close()
    want = F.record_of(st["fl"], perm)
    assert _bits(rec.reshape(-1), want)
    if nang == F.NANG:
        raw = F.load_golden()[f"file_BLS_{'relab' if relabel else 'll1d'}_{prec}"]
        assert rec.tobytes() == raw[4:-4].tobytes()
    exp = np.full((50, LD), SENT, T)
    pos = inv[KIJS:KIJL]
    exp[:, pos] = want.reshape(nf, F.N)[7:57][:, pos]
    assert _bits(sub, exp)


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_savstress_pack_and_getstress_unpack(api, prec, relabel):
    """savstress_pack gives the payload of the LAW file the reference wrote; getstress_unpack of it restores ff, ucur and vcur bit for bit and leaves
    the columns 14 and 15 alone; a sub-range touches its rows and positions only."""
    T = F.dtype_of(prec)
    st = _state(F.NANG, T)
    perm = F.permutation() if relabel else None
    inv = np.argsort(perm) if relabel else np.arange(F.N)
    law = _payload(F.load_golden()[f"file_LAW_{'relab' if relabel else 'll1d'}_{prec}"], T)
    assert len(law) == 17 and law[0].tobytes() == "".join(F.DATES).encode()
    want = np.stack([r.view(T) for r in law[1:]])
    ctx = api.HipContext(F.tables(prec))
    try:
        if relabel:
            ctx.set_restart_map(perm)
        ff, u, v = _up(ctx, st["ff"], T), _up(ctx, st["ucur"], T), _up(ctx, st["vcur"], T)
        rf = _sent(ctx, 16, F.N)
        ctx.savstress_pack(0, F.N, ff, u, v, rf, relabel)
        sub = _sent(ctx, 16, LD)
        ctx.savstress_pack(KIJS, KIJL, ff, u, v, sub, relabel)
        ctx.savstress_pack(30, 30, ff, u, v, sub, relabel)
        # unpack into sentinels; then a sub-range into sentinels
        ff2, u2, v2 = _sent(ctx, F.N, F.NFF), _sent(ctx, F.N), _sent(ctx, F.N)
        ctx.getstress_unpack(0, F.N, rf, ff2, u2, v2, relabel)
        ff3, u3, v3 = _sent(ctx, F.N, F.NFF), _sent(ctx, F.N), _sent(ctx, F.N)
        ctx.getstress_unpack(KIJS, KIJL, sub, ff3, u3, v3, relabel)
        ctx.getstress_unpack(30, 30, sub, ff3, u3, v3, relabel)
        torch.cuda.synchronize()
        rf, sub = rf.cpu().numpy(), sub.cpu().numpy()
        ff2, u2, v2, ff3, u3, v3 = (x.cpu().numpy() for x in (ff2, u2, v2, ff3, u3, v3))
        assert _bits(ff.cpu().numpy(), st["ff"])
    finally:
        ctx.close()
    assert _bits(rf, want) and _bits(rf, F.rfield_of(st["ff"], st["ucur"], st["vcur"], perm))
    exp = np.full((16, LD), SENT, T)
    pos = inv[KIJS:KIJL]
    exp[:, pos] = want[:, pos]
    assert _bits(sub, exp)
    assert _bits(ff2[:, :14], st["ff"][:, :14]) and (ff2[:, 14:] == T(SENT)).all() and _bits(u2, st["ucur"]) and _bits(v2, st["vcur"])
    e3 = np.full((F.N, F.NFF), SENT, T)
    e3[KIJS:KIJL, :14] = st["ff"][KIJS:KIJL, :14]
    eu, ev = np.full(F.N, SENT, T), np.full(F.N, SENT, T)
    eu[KIJS:KIJL], ev[KIJS:KIJL] = st["ucur"][KIJS:KIJL], st["vcur"][KIJS:KIJL]
    assert _bits(ff3, e3) and _bits(u3, eu) and _bits(v3, ev)


# ---- 4. the driver: a complete restart, spectra and stress, both directions
@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_round_trip_through_the_driver(api, prec, tmp_path):
    from ecwam_amd import grid as grid_mod
    from ecwam_amd import restart as R
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=12, nfre=36, nfre_red=29, idelt=450, idelpro=450)
    g = grid_mod.build_grid(16, mask="continents")
    a, b = Wamintgr(cfg, g, prec), Wamintgr(cfg, g, prec)
    try:
        a.init_synthetic(seed=7)
        b.init_synthetic(seed=7)
        n = a.n
        a.step()      # a state a run would save: stress fields the source terms have written
        u, v = a._currents()
        u.copy_(torch.linspace(-1.0, 1.0, n, dtype=a.dtype, device=a.dev))
        v.copy_(torch.linspace(0.5, -0.5, n, dtype=a.dtype, device=a.dev))
        p0, p1, law = str(tmp_path / "bls_host"), str(tmp_path / "bls_dev"), str(tmp_path / "law")
        a.write_restart(p0)
        a.write_restart_device(p1, law, F.DATES)
        with open(p0, "rb") as f0, open(p1, "rb") as f1:
            assert f0.read() == f1.read()      # the file write_restart writes
        dates, rf = R.read_stress(law, n, a.npdt)
        assert tuple(dates) == F.DATES and _bits(rf, F.rfield_of(a.ff.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()))
        assert _bits(a.savstress().cpu().numpy(), rf)
        b.fl1[:n].fill_(SENT)
        b.ff[:, :14] = SENT
        assert b.build_weights() == 0 and b.weights_ready is True
        b.gfast_valid = True
        b.read_restart_device(p1)
        assert tuple(b.read_stress_device(law)) == F.DATES
        torch.cuda.synchronize()
        assert b.weights_ready is True      # IREFRA = 0: the weights stay (getstress.F90:188-191)
        same = lambda x, y: _bits(x.cpu().numpy(), y.cpu().numpy())
        assert same(a.fl1[:n], b.fl1[:n])
        assert same(a.ff, b.ff)
        assert same(b.ucur, u) and same(b.vcur, v)
        b.mij.copy_(a.mij)
        b.xllws.copy_(a.xllws)
        b.intf.copy_(a.intf)
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert same(a.fl1[:n], b.fl1[:n]) and same(a.ff, b.ff) and same(a.intf, b.intf) and same(a.mij, b.mij)
        # relabelled: the files of a global order; getstress relabels back
        perm = F.permutation(n)
        a.set_restart_map(perm)
        rl = a.savstress().cpu().numpy()
        assert _bits(rl, F.rfield_of(a.ff.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(), perm))
        a.write_restart_device(p1)
        assert _bits(R.read_record(p1, dtype=a.npdt), F.record_of(a.fl1[:n].cpu().numpy(), perm))
        keep = a.ff.clone()
        a.ff[:, :14] = SENT
        a.getstress(torch.from_numpy(rl))
        torch.cuda.synchronize()
        assert same(a.ff, keep)
        a.set_restart_map(None)
    finally:
        a.ctx.close()
        b.ctx.close()


# ---- 5. refusals, by the text of ecwam_hip_last_error: error returns only, nothing is launched
def test_refusals(api):
    from ecwam_amd import lib
    from ecwam_amd.tables import Config, Tables

    ctx = api.HipContext(F.tables("sp"))
    h, L = ctx._h, ctx.lib
    err = lambda: L.ecwam_hip_last_error().decode()
    p = lambda t: C.c_void_p(t.data_ptr())
    off = lambda t, b: C.c_void_p(t.data_ptr() + b)
    n = F.N
    try:
        d, wv, row, ff = _sent(ctx, n), _sent(ctx, n, 5, 36), _sent(ctx, n, 36), _sent(ctx, n, 16)
        u, v, rf, fl, blk, plane = _sent(ctx, n), _sent(ctx, n), _sent(ctx, 16, LD), _sent(ctx, n, 12, 36), _sent(ctx, 432, LD), _sent(ctx, F.NCELL)
        o = lib.DepthOpts(40.0, 0.8)
        ob = C.byref(o)
        z = C.c_double(0.0)
        dp = lambda *a: L.ecwam_hip_depthprpt(*a)
        # DEPTHPRPT
        assert dp(None, 0, n, p(d), ob, p(wv), None, None, None, None, None) == 1 and err() == "null context"
        assert dp(h, 0, n, p(d), None, p(wv), None, None, None, None, None) == 1 and err().endswith("null options")
        assert dp(h, 0, n, p(d), ob, None, None, None, None, None, None) == 1 and err().endswith("no output")
        for k0, k1 in ((-1, n), (5, 4)):
            assert dp(h, k0, k1, p(d), ob, p(wv), None, None, None, None, None) == 1 and err().endswith("bad range")
        assert dp(h, 0, n, None, ob, p(wv), None, None, None, None, None) == 1 and err().endswith("null pointer")
        assert dp(h, 0, n, off(d, 2), ob, p(wv), None, None, None, None, None) == 1 and err().endswith("aligned to a real")
        for i in range(5):
            a = [None] * 5
            a[i] = off((wv, row, row, row, ff)[i], 4)
            assert dp(h, 0, n, p(d), ob, *a, None) == 1 and err().endswith("16-byte aligned"), i
        assert dp(h, 7, 7, None, ob, p(wv), None, None, None, None, None) == 0      # an empty range launches nothing
        # BUILDSTRESS
        bs = lambda *a: L.ecwam_hip_buildstress(*a)
        assert bs(None, 0, n, None, None, z, 0, z, z, p(ff), None) == 1 and err() == "null context"
        for flags in (4, 8, 7, -1):
            assert bs(h, 0, n, None, None, z, flags, z, z, p(ff), None) == 1 and err().endswith("unknown flags"), flags
        assert bs(h, 0, n, p(plane), None, z, 0, z, z, p(ff), None) == 1 and err().endswith("no inbound map")
        assert bs(h, 0, n, None, p(plane), z, 0, z, z, p(ff), None) == 1 and err().endswith("no inbound map")
        ctx.set_forcing_map(F.cached_inputs()["map_in"][:n - 4], F.NCELL)
        assert bs(h, 0, n, p(plane), None, z, 0, z, z, p(ff), None) == 1 and err().endswith("bad range")      # rows beyond the map
        for k0, k1 in ((-1, n), (5, 4)):
            assert bs(h, k0, k1, None, None, z, 0, z, z, p(ff), None) == 1 and err().endswith("bad range")
        assert bs(h, 0, n, None, None, z, 0, z, z, None, None) == 1 and err().endswith("null pointer")
        assert bs(h, 0, n, None, None, z, 0, z, z, off(ff, 4), None) == 1 and err().endswith("16-byte aligned")
        assert bs(h, 0, n - 4, off(plane, 4), None, z, 0, z, z, p(ff), None) == 1 and err().endswith("16-byte aligned")
        assert bs(h, 3, 3, None, None, z, 3, z, z, None, None) == 0
        # the map: no permutation
        sm = lambda a: L.ecwam_hip_set_restart_map(h, len(a), np.asarray(a, np.int32).ctypes.data_as(C.c_void_p))
        assert L.ecwam_hip_set_restart_map(None, 0, None) == 1 and err() == "null context"
        assert L.ecwam_hip_set_restart_map(h, -1, None) == 1 and err().endswith("negative count")
        assert sm([0, 1, 3]) == 1 and "outside [0, npts)" in err()
        assert sm([0, -1, 2]) == 1 and "outside [0, npts)" in err()
        assert sm([0, 1, 1]) == 1 and "duplicate" in err()
        # the field vectors: relabel without a map, rows beyond the map, ld too small
        pk = lambda *a: L.ecwam_hip_savstress_pack(*a)
        un = lambda *a: L.ecwam_hip_getstress_unpack(*a)
        sp = lambda *a: L.ecwam_hip_savspec_pack(*a)
        assert pk(None, 0, n, p(ff), p(u), p(v), 0, p(rf), LD, None) == 1 and err() == "null context"
        assert un(None, 0, n, p(rf), LD, 0, p(ff), p(u), p(v), None) == 1 and err() == "null context"
        assert sp(None, 0, n, p(fl), 0, 432, 0, p(blk), LD, None) == 1 and err() == "null context"
        assert pk(h, 0, n, p(ff), p(u), p(v), 1, p(rf), LD, None) == 1 and err().endswith("no restart map")
        assert un(h, 0, n, p(rf), LD, 1, p(ff), p(u), p(v), None) == 1 and err().endswith("no restart map")
        assert sp(h, 0, n, p(fl), 0, 432, 1, p(blk), LD, None) == 1 and err().endswith("no restart map")
        assert sm(list(range(n - 4))) == 0      # a map of 63 rows
        for rl, k1, ld in ((1, n, LD), (0, n, n - 1), (1, n - 4, n - 5), (0, 4, LD), (0, -2, LD)):
            k0 = 5 if k1 == 4 else -1 if k1 == -2 else 0
            k1 = n if k1 == -2 else k1
            assert pk(h, k0, k1, p(ff), p(u), p(v), rl, p(rf), ld, None) == 1 and err().endswith("bad range"), (rl, k1, ld)
            assert un(h, k0, k1, p(rf), ld, rl, p(ff), p(u), p(v), None) == 1 and err().endswith("bad range"), (rl, k1, ld)
            assert sp(h, k0, k1, p(fl), 0, 432, rl, p(blk), ld, None) == 1 and err().endswith("bad range"), (rl, k1, ld)
        for f0, nf in ((-1, 4), (0, 0), (429, 4), (432, 1), (0, 433)):
            assert sp(h, 0, n, p(fl), f0, nf, 0, p(blk), LD, None) == 1 and err().endswith("bad field range"), (f0, nf)
        assert pk(h, 0, n, None, p(u), p(v), 0, p(rf), LD, None) == 1 and err().endswith("null pointer")
        assert un(h, 0, n, None, LD, 0, p(ff), p(u), p(v), None) == 1 and err().endswith("null pointer")
        assert sp(h, 0, n, p(fl), 0, 4, 0, None, LD, None) == 1 and err().endswith("null pointer")
        assert pk(h, 0, n, off(ff, 8), p(u), p(v), 0, p(rf), LD, None) == 1 and err().endswith("16-byte aligned")
        assert un(h, 0, n, p(rf), LD, 0, p(ff), off(u, 2), p(v), None) == 1 and err().endswith("aligned to a real")
        assert sp(h, 0, n, off(fl, 4), 0, 4, 0, p(blk), LD, None) == 1 and err().endswith("16-byte aligned")
        assert sp(h, 0, n, p(fl), 0, 4, 0, off(blk, 2), LD, None) == 1 and err().endswith("aligned to a real")
        assert pk(h, 9, 9, None, None, None, 0, None, LD, None) == 0 and sp(h, 9, 9, None, 0, 4, 0, None, LD, None) == 0
        torch.cuda.synchronize()
        for t in (wv, row, ff, u, v, rf, blk):      # none of the refusals and empty ranges wrote anything
            assert (t == SENT).all()
        # what the refusals border on is served: vectors that begin at any real, the last fields, the last row of the map
        assert sp(h, 0, n, p(fl), 428, 4, 0, off(blk, 4), n, None) == 0
        assert pk(h, 0, n - 4, p(ff), p(u), p(v), 1, off(rf, 4), n - 4, None) == 0
        torch.cuda.synchronize()
    finally:
        ctx.close()
    # NFRE = 30 in single precision: 30 reals are no whole number of 16-byte pieces
    ctx = api.HipContext(Tables(Config(nang=12, nfre=30, nfre_red=30), np.float32))
    try:
        fl, blk, d, row = _sent(ctx, 4, 12, 30), _sent(ctx, 4, 4), _sent(ctx, 4), _sent(ctx, 4, 30)
        with pytest.raises(api.EcwamHipError, match="no whole number of 16-byte chunks"):
            ctx.savspec_pack(0, 4, fl, blk)
        with pytest.raises(api.EcwamHipError, match="no whole number of 16-byte chunks"):
            ctx.depthprpt(0, 4, d, cgroup=row)
        torch.cuda.synchronize()
        assert (blk == SENT).all() and (row == SENT).all()
    finally:
        ctx.close()


# ---- 6. the two pack calls captured in a graph on one stream replay to the same bytes: the call path holds no allocation and no wait
def test_the_pack_calls_in_a_graph(api):
    T = np.float32
    st = _state(F.NANG, T)
    perm = F.permutation()
    ctx = api.HipContext(F.tables("sp"))
    try:
        ctx.set_restart_map(perm)
        fl, ff, u, v = (_up(ctx, st[k], T) for k in ("fl", "ff", "ucur", "vcur"))
        blk, rf = _sent(ctx, 432, F.N), _sent(ctx, 16, F.N)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            ctx.savspec_pack(0, F.N, fl, blk, 0, True)      # warm up on the side stream
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=s):
                ctx.savspec_pack(0, F.N, fl, blk, 0, True)
                ctx.savstress_pack(0, F.N, ff, u, v, rf, True)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            blk.fill_(SENT)
            rf.fill_(SENT)
            graph.replay()
            torch.cuda.synchronize()
            assert _bits(blk.cpu().numpy().reshape(-1), F.record_of(st["fl"], perm))
            assert _bits(rf.cpu().numpy(), F.rfield_of(st["ff"], st["ucur"], st["vcur"], perm))
    finally:
        ctx.close()
