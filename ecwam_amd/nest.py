"""The boundary value file of nested runs in the reference's binary layout: what OUTBC writes for a finer model (headbc.F90:70-74,
outbc.F90:110-112) and BOUINPT reads from a coarser one (bouinpt.F90:162,251-252).

Fortran sequential unformatted records, framed as in restart.py (``<int32 nbytes> payload <int32 nbytes>``), reals in the working precision:

  header   XANG, XFRE, TH0, FR1, FRATIO, XBOU, XDEL     seven reals: NANG, NFRE, TH(1), FR(1), FRATIO, the number of boundary points and
                                                       the propagation time step of the model that wrote the file [s]
  then, per output time and per boundary point, two records:
  point    XLON, XLAT, CDATE (14 characters), EMEAN, THQ, FMEAN
  spectrum ((F(K,M), K = 1, NANG), M = 1, NFRE)         [M][K] with K fastest: the layout ecwam_hip_outbc writes and ecwam_hip_bouinpt reads

`check_header` applies BOUINPT's consistency checks (bouinpt.F90:186-187) and raises where the reference aborts.
"""
from __future__ import annotations

import dataclasses

import numpy as np

_HEADER_NAMES = ("xang", "xfre", "th0", "fr1", "fratio", "xbou", "xdel")


class NestFileError(ValueError):
    pass


@dataclasses.dataclass
class Header:
    nang: int
    nfre: int
    th0: float
    fr1: float
    fratio: float
    nbou: int
    idelpro: int


def _put(f, payload: bytes) -> None:
    m = np.array([len(payload)], dtype="<i4").tobytes()
    f.write(m); f.write(payload); f.write(m)


def _get(f, want: int | None = None, what: str = "record"):
    """The payload of the next record; None at a clean end of file."""
    h = f.read(4)
    if len(h) == 0:
        return None
    if len(h) != 4:
        raise NestFileError(f"boundary file: truncated marker of a {what}")
    n = int(np.frombuffer(h, "<i4")[0])
    if n < 0 or (want is not None and n != want):
        raise NestFileError(f"boundary file: the {what} holds {n} bytes" + (f", expected {want}" if want is not None else ""))
    payload = f.read(n)
    t = f.read(4)
    if len(payload) != n or len(t) != 4 or int(np.frombuffer(t, "<i4")[0]) != n:
        raise NestFileError(f"boundary file: corrupt or truncated {what}")
    return payload


def write_header(f, nang: int, nfre: int, th0, fr1, fratio, nbou: int, idelpro: int, dtype) -> None:
    """HEADBC (headbc.F90:70-74)."""
    dt = np.dtype(dtype).newbyteorder("<")
    _put(f, np.array([nang, nfre, th0, fr1, fratio, nbou, idelpro], dtype=dt).tobytes())


def read_header(f, dtype) -> Header:
    dt = np.dtype(dtype).newbyteorder("<")
    p = _get(f, 7 * dt.itemsize, "header")
    if p is None:
        raise NestFileError("boundary file: no header")
    v = np.frombuffer(p, dt)
    # NINT as bouinpt.F90:177-180
    return Header(nang=int(np.rint(v[0])), nfre=int(np.rint(v[1])), th0=v[2], fr1=v[3], fratio=v[4], nbou=int(np.rint(v[5])), idelpro=int(np.rint(v[6])))


def check_header(h: Header, nang: int, nfre: int, th1, fr1, idelpro: int) -> None:
    """bouinpt.F90:186-187: the coarse model's spectral grid must be the fine model's (NANG, NFRE, TH(1), FR(1) compared exactly, in the
    working precision) and its output step a multiple of the fine model's propagation step, and not smaller."""
    bad = []
    if h.nang != nang:
        bad.append(f"NANG {h.nang} /= {nang}")
    if h.nfre != nfre:
        bad.append(f"NFRE {h.nfre} /= {nfre}")
    if h.fr1 != fr1:
        bad.append(f"FR(1) {h.fr1!r} /= {fr1!r}")
    if h.th0 != th1:
        bad.append(f"TH(1) {h.th0!r} /= {th1!r}")
    if idelpro <= 0 or h.idelpro % idelpro != 0:
        bad.append(f"the input step {h.idelpro} s is no multiple of IDELPRO {idelpro} s")
    elif h.idelpro < idelpro:
        bad.append(f"the input step {h.idelpro} s is smaller than IDELPRO {idelpro} s")
    if bad:
        raise NestFileError("values in the boundary file header are inconsistent with the model set-up: " + "; ".join(bad))


def write_points(f, xlon, xlat, cdate: str, par, flpts, dtype) -> None:
    """One output time (outbc.F90:98-114): par [n][3] = EMEAN, THQ, FMEAN and flpts [n][NFRE][NANG] as ecwam_hip_outbc returns them."""
    dt = np.dtype(dtype).newbyteorder("<")
    date = cdate.encode("ascii")
    if len(date) != 14:
        raise NestFileError(f"the date of a boundary record has 14 characters (YYYYMMDDHHMMSS), got {cdate!r}")
    par = np.asarray(par, dtype=dt)
    flpts = np.asarray(flpts, dtype=dt)
    n = par.shape[0]
    if par.shape != (n, 3) or flpts.ndim != 3 or flpts.shape[0] != n or len(xlon) != n or len(xlat) != n:
        raise NestFileError("write_points: par [n][3], flpts [n][NFRE][NANG], xlon [n], xlat [n]")
    for i in range(n):
        _put(f, np.array([xlon[i], xlat[i]], dtype=dt).tobytes() + date + par[i].tobytes())
        _put(f, np.ascontiguousarray(flpts[i]).tobytes())


def read_points(f, h: Header, dtype):
    """The records of the next output time: (xlon [n], xlat [n], cdate, par [n][3], f1 [n][NFRE][NANG]), or None at the end of the file.
    The date is that of the last point, as in bouinpt.F90:250-257."""
    dt = np.dtype(dtype).newbyteorder("<")
    n, rb = h.nbou, dt.itemsize
    lonlat = np.zeros((n, 2), dtype=dt)
    par = np.zeros((n, 3), dtype=dt)
    f1 = np.zeros((n, h.nfre, h.nang), dtype=dt)
    cdate = ""
    for i in range(n):
        p = _get(f, 5 * rb + 14, "point record")
        if p is None:
            if i == 0:
                return None
            raise NestFileError(f"boundary file: ends after {i} of {n} points of an output time")
        lonlat[i] = np.frombuffer(p[: 2 * rb], dt)
        cdate = p[2 * rb: 2 * rb + 14].decode("ascii")
        par[i] = np.frombuffer(p[2 * rb + 14:], dt)
        s = _get(f, h.nang * h.nfre * rb, "spectrum record")
        if s is None:
            raise NestFileError("boundary file: a point record without its spectrum")
        f1[i] = np.frombuffer(s, dt).reshape(h.nfre, h.nang)
    native = np.dtype(dtype)
    return lonlat[:, 0].astype(native), lonlat[:, 1].astype(native), cdate, par.astype(native), f1.astype(native)
