"""The host side of the stand-alone forcing (include/ecwam_hip_readwind.h): what GRIB2WGRID decides from a message's keys and the wave model's
grid, restated in numpy from the reference's Fortran in its order of operations and in the working precision.

  input_grid   grib2wgrid.F90:197-420 (only what decides the geometry and LLNONWAVE) and 475-737: RLONRGG, RDELLO, RMONOP, RMOWEP, DELLA,
               IPERIODIC, ITOP, IBOT, LLSCANNS, LLINTERPOL, with the routine's domain checks as exceptions in its words
  cell_table   grib2wgrid.F90:964-1037 (and 793-802 for LLINTERPOL = F): the per-cell table ecwam_hip_set_input_grid takes -- the positions in
               VALUES of the four corners, with the scan direction (893-943) and the periodic columns (947-955) resolved, the three weights, the kind
  dirfld       the test of grib2wgrid.F90:836-847

Once per input grid; the arithmetic on the fields at every wind and current time is the device's (csrc/readwind.hip).  Not served, and refused
here by name: the ocean-model messages of GRIB 1 with local definition 4 (LLOCEAN: staggered grids), unstructured input, and the un-scaling of
parameter 251 (ecwam_amd/gribin.py reads spectra).
"""
from __future__ import annotations

import numpy as np

# WSTREAM_STRG (wstream_strg.F90): the streams of wave data (LASTREAM = F) and the atmosphere's (LASTREAM = T); any other stream is '****'
WAVE_STREAMS = frozenset((1045, 1077, 1125, 1079, 1080, 1081, 1123, 1082, 1083, 1084, 1124, 1024, 1078, 1086, 1027, 1029, 1248, 1092, 1095, 1096, 1203, 1204,
                          1205, 1209, 1210, 1211, 1222, 1223, 1087, 1088, 1250))
ATMOSPHERE_STREAMS = frozenset((1025, 1071, 1035, 1122, 1090, 1033, 1040, 1121, 1037, 1039, 1120, 1085, 1032, 1034, 1026, 1028, 1247, 1098, 1091, 1093, 1094,
                                1200, 1201, 1202, 1206, 1207, 1208, 1220, 1221, 1030, 1249))
DIRECTION_PARAMS = frozenset((230, 235, 238, 242, 249, 122, 125, 128, 113))


def dtype_of(prec):
    return np.float32 if prec == "sp" else np.float64


def dirfld(iparam: int, wave_stream: bool) -> bool:
    """LLDIRFLD (grib2wgrid.F90:836-847): a direction in degrees, interpolated through its sine and cosine; wave_stream is CSTREAM /= '****'"""
    return int(iparam) in DIRECTION_PARAMS and bool(wave_stream)


def _nint(x):
    """Fortran's NINT: halves away from zero"""
    x = float(x)
    return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def _adjust(west, east, T):
    """ADJUST (adjust.F90:58-64)"""
    old_west, old_east = west, east
    west = np.fmod(west + T(720), T(360))
    east = np.fmod(east + T(720), T(360))
    if old_west != old_east and west >= east:
        west = west - T(360)
    return west, east


def input_grid(keys, xlon, ylat, nlonrgg_loc, ngy, nxs, nxe, nys, nye, pmiss, prec="dp", krgg=1, llchkint=True, llunstr=False):
    """grib2wgrid.F90:197-420 and 475-737 for one message.  keys: a dict of the message keys the routine asks for -- Nj; Ni (regular) or pl
    (reduced); jScansPositively; gridType; latitudeOfFirstGridPointInDegrees, latitudeOfLastGridPointInDegrees,
    longitudeOfFirstGridPointInDegrees, longitudeOfLastGridPointInDegrees; jDirectionIncrementInDegrees (a reduced grid with empty rows);
    optional paramId, editionNumber (2), localDefinitionNumber (absent: none), stream, levtype.  xlon, ylat: [nye - nys + 1][nxe - nxs + 1], the
    wave model's XLON and YLAT (pmiss where a cell needs no value); nlonrgg_loc[ngy]: KLONRGG_LOC, south to north.
    Returns a dict: RLONRGG (south to north), RDELLO, RMONOP, RMOSOP, RMOWEP, RMOEAP, DELLA, NC, NR, IPERIODIC, ITOP, IBOT, LLSCANNS, LLINTERPOL,
    LLNONWAVE, wave_stream, IPARAM, nvalues (lower case keys)."""
    T = dtype_of(prec)
    xlon, ylat = np.asarray(xlon, T), np.asarray(ylat, T)
    klon = np.asarray(nlonrgg_loc, np.int64)
    nx, ny = nxe - nxs + 1, nye - nys + 1
    if xlon.shape != (ny, nx) or ylat.shape != (ny, nx) or klon.size != ngy:
        raise ValueError("input_grid: XLON and YLAT are [NYS:NYE][NXS:NXE], KLONRGG_LOC has NGY rows")
    if llunstr:
        raise ValueError("input_grid: unstructured input is not served on the device")
    pm = T(pmiss)
    # the model's domain among the cells that need a value (197-224)
    inrow = np.arange(nxs, nxe + 1)[None, :] <= np.minimum(klon[ngy - np.arange(nys, nye + 1)], nxe)[:, None]
    need = inrow & (ylat != pm) & (xlon != pm)
    if need.any():
        pmowep, pmoeap, pmosop, pmonop = xlon[need].min(), xlon[need].max(), ylat[need].min(), ylat[need].max()
    else:
        pmowep = pmoeap = pmosop = pmonop = T(0)
    edition = int(keys.get("editionNumber", 2))
    nr = int(keys["Nj"])
    iscan = int(keys["jScansPositively"])
    if iscan not in (0, 1):
        raise ValueError(f"GRIB2WGRID: SCANNING MODE NOT RECOGNIZED !!! ISCAN = {iscan}")
    llscanns = iscan == 0
    itabpar = int(keys.get("paramId", 0))
    iparam = itabpar - (itabpar // 1000) * 1000
    iloc = int(keys.get("localDefinitionNumber", -1))
    if iloc == 4 and edition == 1:
        raise ValueError("input_grid: old ocean model data (LLOCEAN: GRIB 1, local definition 4, staggered grids) is not served on the device")
    gt = str(keys["gridType"])
    if gt.startswith("regular_gg"):
        jrgg, irepr = 0, 4
    elif gt.startswith("reduced_gg"):
        jrgg, irepr = 1, 4
    elif gt.startswith("regular"):
        jrgg, irepr = 0, 0
    elif gt.startswith("reduced"):
        jrgg, irepr = 1, 0
    else:
        raise ValueError(f"GRIB2WGRID: GRID TYPE NOT RECOGNIZED !!! gridType = {gt}")
    if jrgg == 1:
        if "pl" not in keys:
            raise ValueError("GRIB2WGRID: NUMBER OF POINTS PER LATITUDE MISSING !!!")
        pl = np.asarray(keys["pl"], np.int64)
        nc = int(pl.max()) if pl.size else 0
        nr = int((pl != 0).sum())
    else:
        pl = None
        nc = int(keys["Ni"])
    ilevtype = int(keys.get("levtype", 0))
    istream = int(keys["stream"]) if iloc >= 0 else 0
    wave_stream = istream in WAVE_STREAMS or istream in ATMOSPHERE_STREAMS      # CSTREAM /= '****'
    lastream = istream not in WAVE_STREAMS
    llnonwave = (not wave_stream) or (lastream and ilevtype != 209 and ilevtype != 212)
    if itabpar == 140251 and wave_stream:
        raise ValueError("input_grid: parameter 251 (spectra) is un-scaled and read by ecwam_amd/gribin.py, not here")

    # the grid's parameters (475-586)
    yfrst, ylast = T(keys["latitudeOfFirstGridPointInDegrees"]), T(keys["latitudeOfLastGridPointInDegrees"])
    rmonop, rmosop = (yfrst, ylast) if llscanns else (ylast, yfrst)
    rmowep = T(keys["longitudeOfFirstGridPointInDegrees"])
    if irepr == 4 and llnonwave:      # a Gaussian grid of the atmosphere is global
        dello = T(360) / T(max(1, nc))
        rmoeap = rmowep + T(360) - dello
        iperiodic = 1
    else:
        rmoeap = T(keys["longitudeOfLastGridPointInDegrees"])
        rmowep, rmoeap = _adjust(rmowep, rmoeap, T)
        iperiodic = 0
        dello = (rmoeap - rmowep) / T(max(1, nc - 1))
        if rmoeap - rmowep + T(1.5) * dello >= T(360):
            iperiodic = 1
    rlonrgg = np.zeros(nr, np.int64)
    if jrgg == 1:
        istart = 0
        while pl[istart] == 0 and istart + 1 < pl.size:
            istart += 1
        istop = 0
        while pl[pl.size - 1 - istop] == 0 and istop < pl.size:
            istop += 1
        for j in range(1, nr + 1):
            jsn = nr - j + 1 if llscanns else j
            rlonrgg[jsn - 1] = pl[j + istart - 1]
        if istart != 0 or istop != 0:
            della = T(keys["jDirectionIncrementInDegrees"])
            yfrst = yfrst - T(istart) * della
            ylast = ylast + T(istop) * della
        rmonop, rmosop = (yfrst, ylast) if llscanns else (ylast, yfrst)
    else:
        rlonrgg[:] = nc

    # whether interpolation is needed (588-737)
    della = (rmonop - rmosop) / T(max(1, nr - 1))
    kp = [_nint(v * T(100)) for v in (pmowep, pmoeap, pmonop, pmosop)]
    kr = [_nint(v * T(100)) for v in (rmowep, rmoeap, rmonop, rmosop)]
    kpmowep, kpmoeap, kpmonop, kpmosop = kp
    krmowep, krmoeap, krmonop, krmosop = kr
    if iperiodic == 1:
        rdello = T(360) / np.maximum(1, rlonrgg).astype(T)
    else:
        rdello = (rmoeap - rmowep) / np.maximum(1, rlonrgg - 1).astype(T)
    itop = int((pmonop - rmonop) / della) + 2 if kpmonop > krmonop else 0
    ibot = int((rmosop - pmosop) / della) + 2 if kpmosop < krmosop else 0
    if kpmonop < krmosop or kpmosop > krmonop:
        raise ValueError(f"GRIB2WGRID: THE MODEL DOMAIN IS OUTSIDE THE INPUT DOMAIN FOR PARAMETER {iparam}: PMOSOP {pmosop} RMOSOP {rmosop} PMONOP {pmonop} "
                         f"RMONOP {rmonop}")
    if llchkint:
        llinterpol = True
        if kp == kr and jrgg == krgg and nxs == 1 and nc == nxe and nys == 1 and nr == ngy:
            llinterpol = bool(krgg == 1 and not np.array_equal(rlonrgg, klon))
        if not llscanns:
            llinterpol = True
    else:
        if jrgg != krgg or nr != ngy or (krgg == 1 and not np.array_equal(rlonrgg, klon)) or (krgg != 1 and nc != klon[0]):
            raise ValueError("GRIB2WGRID: NO INTERPOLATION WAS REQUEST BUT IT DOES SEEM LIKE GRIDS ARE DIFFERENT !!!")
        llinterpol = False
    nvalues = int(rlonrgg.sum())
    return dict(rlonrgg=rlonrgg, rdello=rdello, rmonop=rmonop, rmosop=rmosop, rmowep=rmowep, rmoeap=rmoeap, della=della, dello=dello, nc=nc, nr=nr,
                iperiodic=iperiodic, itop=itop, ibot=ibot, llscanns=llscanns, llinterpol=llinterpol, llnonwave=llnonwave, wave_stream=wave_stream, iparam=iparam,
                llchkint=bool(llchkint), nvalues=nvalues, prec=prec)


def cell_table(grid, xlon, ylat, nlonrgg_loc, ngy, nxs, nxe, nys, nye, pmiss, prec=None):
    """grib2wgrid.F90:964-1037 for every cell of the (NXS:NXE, NYS:NYE) grid, first index fastest: a dict of pos int32 [ncell][4], w float64
    [ncell][3] (DK1, DII1, DIIP1 in the working precision, widened), kind int32 [ncell], nvalues, interpol -- what ecwam_hip_set_input_grid
    takes -- and, for the tests, kk, ii1_clamped, wrapped, padded, llskip per cell."""
    prec = grid["prec"] if prec is None else prec
    T = dtype_of(prec)
    xlon, ylat = np.asarray(xlon, T), np.asarray(ylat, T)
    klon = np.asarray(nlonrgg_loc, np.int64)
    nx, ny = nxe - nxs + 1, nye - nys + 1
    ncell = nx * ny
    pm = T(pmiss)
    K = np.repeat(np.arange(nys, nye + 1), nx)
    I = np.tile(np.arange(nxs, nxe + 1), ny)
    jsn = ngy - K + 1
    inrow = I <= np.minimum(klon[jsn - 1], nxe)
    xl, yl = xlon.reshape(-1), ylat.reshape(-1)
    pos = np.full((ncell, 4), -1, np.int32)
    w = np.zeros((ncell, 3), np.float64)
    kind = np.where(inrow, 2, 0).astype(np.int32)
    extra = dict(kk=np.zeros(ncell, np.int64), ii1_clamped=np.zeros(ncell, bool), wrapped=np.zeros(ncell, bool), padded=np.zeros(ncell, bool),
                 llskip=np.zeros(ncell, bool))
    if not grid["llinterpol"]:
        if not grid["llchkint"]:
            raise ValueError("cell_table: the partial copy of LLCHKINT = F (grib2wgrid.F90:806-824) is not served; READWIND and CURRENT2WAM ask for the check")
        # the full copy (793-802): NXS = NYS = 1, rows K = 1 .. NGY of KLONRGG_LOC(NGY - K + 1) values
        start = np.concatenate(([0], np.cumsum(klon[::-1])))[:-1]      # by K
        pos[:, 0] = np.where(inrow, start[K - 1] + I - 1, -1)
        return dict(pos=pos, w=None, kind=kind, nvalues=grid["nvalues"], interpol=False, **extra)
    rlon, rdello = grid["rlonrgg"], np.asarray(grid["rdello"], T)
    nr, iper = grid["nr"], grid["iperiodic"]
    kkmin, kkmax = 1 - grid["itop"], nr + grid["ibot"]
    # where row KK of WORK lies in VALUES: a message scanned north to south fills KK = 1 .. NR with RLONRGG(NR - KK + 1) values each (896-916);
    # one scanned south to north fills KK = NR .. 1 with RLONRGG(KK) values each (921-941) -- the lengths of the mirrored rows
    if grid["llscanns"]:
        filled = rlon[::-1]                                        # by KK
        start = np.concatenate(([0], np.cumsum(filled)))[:-1]
    else:
        filled = rlon.copy()
        if not np.array_equal(rlon, rlon[::-1]):
            raise ValueError("cell_table: a message scanned south to north whose rows are not symmetric about the equator: the reference fills row KK with "
                             "RLONRGG(KK) values and reads RLONRGG(NR - KK + 1), so part of WORK is undefined")
        start = (np.concatenate(([0], np.cumsum(filled[::-1])))[:-1])[::-1]
    missing = (yl == pm) | (xl == pm)
    kind[inrow & missing] = 1
    act = inrow & ~missing
    with np.errstate(invalid="ignore", over="ignore"):
        xk = grid["rmonop"] - yl
        xk = (xk / grid["della"]) + T(0.5) * (T(1) + np.copysign(T(1), xk))
        kk = np.maximum(kkmin, np.trunc(xk).astype(np.int64))
        if (kk[act] > kkmax).any():
            raise ValueError("cell_table: a cell lies below the padded rows of the input (KK > KKMAX)")
        kk = np.minimum(kk, kkmax)
        ksn = nr - kk + 1
        kk1 = np.minimum(kk + 1, kkmax)
        ksn1 = nr - kk1 + 1
        dk1 = np.abs(xk - kk.astype(np.float32).astype(T))
        xi = np.fmod((xl - grid["rmowep"]) + T(720), T(360))
        llskip = np.zeros(ncell, bool)

        def column(ks):
            lim = np.clip(ks, 1, nr)
            n = rlon[lim - 1]
            xii = xi / rdello[lim - 1] + T(1)
            ii = np.trunc(xii).astype(np.int64)
            skip = (ii < 1 - iper) | (ii > n)
            ii = np.minimum(np.maximum(1 - iper, ii), n)
            ii1 = ii + 1
            clamped = ii1 > n + iper
            ii1 = np.minimum(ii1, n + iper)
            dii1 = xii - ii.astype(np.float32).astype(T)
            return ii, ii1, dii1, skip, clamped, n
        ii, ii1, dii1, s0, c0, n0 = column(ksn)
        iip, iip1, diip1, s1, c1, n1 = column(ksn1)
    llskip = s0 | s1
    kind[act & llskip] = 1
    go = act & ~llskip

    def position(i, k, n):
        """0-based position in VALUES of WORK(i, k): the periodic columns are the row's last and first value; a padded row has none"""
        inside = (k >= 1) & (k <= nr)
        wrap = (i == 0) | (i == n + 1)
        i = np.where(i == 0, n, np.where(i == n + 1, 1, i))
        kc = np.clip(k, 1, nr)
        if (go & inside & (i > filled[kc - 1])).any():
            raise ValueError("cell_table: a corner lies beyond the values its row was filled with")
        return np.where(inside, start[kc - 1] + i - 1, -1), wrap & inside
    wrapped = np.zeros(ncell, bool)
    for col, (i, k, n) in enumerate(((ii, kk, n0), (ii1, kk, n0), (iip, kk1, n1), (iip1, kk1, n1))):
        p, wr = position(i, k, n)
        pos[:, col] = np.where(go, p, -1)
        wrapped |= wr & go
    for col, v in enumerate((dk1, dii1, diip1)):
        w[:, col] = np.where(go, v.astype(np.float64), 0.0)
    extra.update(kk=kk, ii1_clamped=(c0 | c1) & go, wrapped=wrapped, padded=go & (pos < 0).any(axis=1), llskip=act & llskip)
    return dict(pos=pos, w=w, kind=kind, nvalues=grid["nvalues"], interpol=True, **extra)
