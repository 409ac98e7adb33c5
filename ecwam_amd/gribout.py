"""The host side of the GRIB-ready output (include/ecwam_hip_gribout.h): where in the vector VALUES handed to the GRIB encoder each sea point
lands.  value_map restates, from the reference's own variables, the three things that decide it --
  the block-to-grid step  IX = IXLG, IY = NGY - KXLT + 1                      (outwspec.F90:223-225, makegrid.F90:156-160)
  the fill order          row J = 1 .. NGY holds NLONRGG(NGY - J + 1) values   (wgribencode_values.F90:152-156)
  the start offset        ICOUNT                                             (wgribencode_values.F90:93-100)
-- and the ranges of the pole rows and of the rows beside them (LPADPOLES, wgribencode_values.F90:103-148), so that no caller restates them.
"""
from __future__ import annotations

import dataclasses

import numpy as np

# yowgribhd.F90:39-48 and yowpcons ZMISS: the defaults of the opts of ecwam_hip_outspec_values / ecwam_hip_grib_values
GRIB_DEFAULTS = dict(ppmiss=-3.0, ppeps=1.0e-10, pprec=0.0, ppresol=0.002, ppmin_reset=0.0, ngrbress=9, zmiss=-999.0)


@dataclasses.dataclass(frozen=True)
class Pole:
    """The cells [pole0, pole0 + npole) of VALUES are a pole row, [adj0, adj0 + nadj) the row beside it; npole = 0: no padding at this pole"""
    pole0: int = 0
    npole: int = 0
    adj0: int = 0
    nadj: int = 0


@dataclasses.dataclass(frozen=True)
class Poles:
    north: Pole = Pole()
    south: Pole = Pole()

    def as_ints(self):
        return [self.north.pole0, self.north.npole, self.north.adj0, self.north.nadj, self.south.pole0, self.south.npole, self.south.adj0, self.south.nadj]


def _nint(x: float) -> int:
    """Fortran's NINT: half away from zero"""
    return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def read_map(nlonrgg, ixlg, kxlt, ngy):
    """(ival, nvalues) of the READ of a GRIB spectrum (include/ecwam_hip_gribin.h): where in the decoded vector GRIB2WGRID's full copy
    (grib2wgrid.F90:793-802: row K = 1 .. NGY of FIELD takes the next NLONRGG(NGY - K + 1) values, from the first value on -- there is no
    start offset) and GETSPEC's gather WORK(IJ) = FIELD(IXLG, NGY - KXLT + 1) (getspec.F90:458-462) find point ij; nvalues is the number of
    values the copy consumes.  Equal to the ival of value_map wherever the output's ICOUNT is 1 (IRGG = 1, or CLDOMAIN = 'm'); a message
    laid out otherwise is read with this map set (ecwam_hip_set_grib_map(ival, ntencode >= nvalues, no poles)) and the output map set
    afterwards."""
    nlonrgg = np.asarray(nlonrgg, dtype=np.int64).reshape(-1)
    ixlg = np.asarray(ixlg, dtype=np.int64).reshape(-1)
    kxlt = np.asarray(kxlt, dtype=np.int64).reshape(-1)
    ngy = int(ngy)
    if nlonrgg.size != ngy or ngy < 1 or (nlonrgg < 1).any():
        raise ValueError(f"read_map: NLONRGG must hold NGY = {ngy} positive row lengths")
    if ixlg.size != kxlt.size:
        raise ValueError("read_map: IXLG and KXLT differ in length")
    if kxlt.size and (kxlt.min() < 1 or kxlt.max() > ngy):
        raise ValueError("read_map: KXLT outside 1 .. NGY")
    if ixlg.size and (ixlg.min() < 1 or (ixlg > nlonrgg[kxlt - 1]).any()):
        raise ValueError("read_map: IXLG outside 1 .. NLONRGG(KXLT)")
    length = nlonrgg[::-1]      # by K - 1
    start = np.concatenate([[0], np.cumsum(length)[:-1]])
    return (start[ngy - kxlt] + ixlg - 1).astype(np.int32), int(length.sum())


def value_map(nlonrgg, ixlg, kxlt, ngy, irgg, amonop, amosop, xdella, cldomain="g", lpadpoles=True):
    """(ival, ntencode, poles) from the reference's variables: NLONRGG(1:NGY) south to north, BLK2GLO%IXLG and %KXLT of the points (1-based, as
    the reference holds them), IRGG, AMONOP, AMOSOP, XDELLA, CLDOMAIN, LPADPOLES.  ival[ij] is the 0-based position in VALUES of point ij;
    NTENCODE is that of preset_wgrib_template.F90:589-593, 679-686 (no Gaussian regular grid: IQGAUSS /= 1 where IRGG = 0).
    Refused: CLDOMAIN = 's', NLONRGG of another length than NGY, a regular grid whose rows differ, a point outside its row."""
    nlonrgg = np.asarray(nlonrgg, dtype=np.int64).reshape(-1)
    ixlg = np.asarray(ixlg, dtype=np.int64).reshape(-1)
    kxlt = np.asarray(kxlt, dtype=np.int64).reshape(-1)
    ngy = int(ngy)
    if cldomain == "s":
        raise ValueError("value_map: CLDOMAIN = 's' (one-point output) is not served")
    if nlonrgg.size != ngy or ngy < 1 or (nlonrgg < 1).any():
        raise ValueError(f"value_map: NLONRGG must hold NGY = {ngy} positive row lengths")
    if ixlg.size != kxlt.size:
        raise ValueError("value_map: IXLG and KXLT differ in length")
    if irgg not in (0, 1):
        raise ValueError("value_map: IRGG is 0 (regular) or 1 (reduced)")
    ngx = int(nlonrgg.max())
    if irgg == 0 and (nlonrgg != ngx).any():
        raise ValueError("value_map: IRGG = 0 but the rows of NLONRGG differ in length")
    if kxlt.size and (kxlt.min() < 1 or kxlt.max() > ngy):
        raise ValueError("value_map: KXLT outside 1 .. NGY")
    if ixlg.size and (ixlg.min() < 1 or (ixlg > nlonrgg[kxlt - 1]).any()):
        raise ValueError("value_map: IXLG outside 1 .. NLONRGG(KXLT)")
    north = _nint((90.0 - float(amonop)) / float(xdella))      # rows between the north pole and the grid
    if irgg == 1 or cldomain == "m":
        icount = 0
    else:
        icount = north * ngx      # wgribencode_values.F90:98; VALUES is set to ZMISS there first
    if irgg == 1:
        ntencode = int(nlonrgg.sum())
    else:
        nj = _nint(180.0 / float(xdella)) + 1 if cldomain == "g" else ngy
        ntencode = nj * ngx
    # row J of FIELD (J = 1 the northernmost) starts at ICOUNT + the lengths of the rows north of it
    length = nlonrgg[::-1]      # by J - 1
    start = icount + np.concatenate([[0], np.cumsum(length)[:-1]])
    j0 = ngy - kxlt      # IY - 1
    ival = (start[j0] + ixlg - 1).astype(np.int32)
    if icount + int(length.sum()) > ntencode or icount < 0:
        raise ValueError("value_map: the grid does not fit the NTENCODE values of its template (AMONOP, XDELLA and NLONRGG disagree)")
    n, s = Pole(), Pole()
    if lpadpoles and ngy >= 2:
        if north == 0:
            n = Pole(int(start[0]), int(length[0]), int(start[1]), int(length[1]))
        if _nint((-90.0 - float(amosop)) / float(xdella)) == 0:
            s = Pole(int(start[ngy - 1]), int(length[ngy - 1]), int(start[ngy - 2]), int(length[ngy - 2]))
        if ngy == 2 and n.npole and s.npole:
            raise ValueError("value_map: two rows that are both poles leave no row to pad from")
    return ival, int(ntencode), Poles(n, s)
