"""Restart spectra in the reference's binary layout.

`writefl.F90:110-118` writes ONE Fortran unformatted sequential record per rank:
``WRITE(IUNIT) (((FL(IJ,K,M),IJ=IJINF,IJSUP),K=KINF,KSUP),M=MINF,MSUP)`` -- IJ fastest, then K, then M, reals in the
working precision -- and `getspec`/`readfl` read it back the same way.  The device keeps spectra point-major
(`FL[ij][K][M]`, include/ecwam_hip.h), so the conversion is a transpose of the three axes.

Record framing is the 4-byte length-marker convention of gfortran/flang/ifort (`-assume byterecl` not needed for
sequential files): ``<int32 nbytes> payload <int32 nbytes>``.  Payloads beyond 2^31-9 bytes use gfortran's sub-record
scheme (every sub-record framed, a negative head marker = "continued", a negative tail marker = "has a predecessor"),
which is what a gfortran-built ecWAM produces for the 2.18 GB single-rank O320 record.
"""
from __future__ import annotations

import numpy as np

_MAX_SUB = 2147483639  # gfortran: GFC_MAX_SUBRECORD_LENGTH


def write_fl(path: str, fl_points: np.ndarray, append: bool = False) -> None:
    """fl_points: [n][NANG][NFRE] (owned rows only, device layout).  Appends like IWAM_GET_UNIT(...,'a',...) when asked."""
    a = np.ascontiguousarray(np.transpose(fl_points, (2, 1, 0)))  # C order [M][K][IJ] == Fortran FL(IJ,K,M) element order
    raw = a.reshape(-1).view(np.uint8)
    nb = raw.size
    with open(path, "ab" if append else "wb") as f:
        if nb <= _MAX_SUB:
            m = np.array([nb], dtype="<i4").tobytes()
            f.write(m); f.write(raw.tobytes() if nb < (1 << 26) else memoryview(raw)); f.write(m)
            return
        off, first = 0, True
        while off < nb:
            ln = min(_MAX_SUB, nb - off)
            last = off + ln >= nb
            head = np.array([ln if last else -ln], dtype="<i4").tobytes()
            tail = np.array([ln if first else -ln], dtype="<i4").tobytes()
            f.write(head); f.write(memoryview(raw[off:off + ln])); f.write(tail)
            off += ln
            first = False


def read_fl(path: str, n: int, nang: int, nfre: int, dtype, record: int = 0) -> np.ndarray:
    """Reads record number `record` (0-based) and returns [n][NANG][NFRE]."""
    dt = np.dtype(dtype)
    want = n * nang * nfre * dt.itemsize
    with open(path, "rb") as f:
        for rec in range(record + 1):
            chunks, total = [], 0
            while True:
                h = f.read(4)
                if len(h) != 4:
                    raise EOFError(f"{path}: record {rec} not found")
                head = int(np.frombuffer(h, "<i4")[0])
                ln = abs(head)
                if rec == record:
                    chunks.append(f.read(ln))
                else:
                    f.seek(ln, 1)
                total += ln
                tail = int(np.frombuffer(f.read(4), "<i4")[0])
                if abs(tail) != ln:
                    raise ValueError(f"{path}: corrupt record markers ({head} / {tail})")
                if head >= 0:  # last (or only) sub-record
                    break
            if rec == record:
                if total != want:
                    raise ValueError(f"{path}: record holds {total} bytes, expected {want} for FL({n},{nang},{nfre}) {dt}")
                a = np.frombuffer(b"".join(chunks), dtype=dt).reshape(nfre, nang, n)
                return np.ascontiguousarray(np.transpose(a, (2, 1, 0)))
    raise AssertionError("unreachable")


def read_record(path: str, record: int = 0, dtype=np.uint8) -> np.ndarray:
    """The payload of record number `record` (0-based) as the file holds it, flat and not transposed: the elements of
    ``(((FL(IJ,K,M),IJ),K),M)`` in file order when viewed in the working precision (`dtype`), i.e. NANG * NFRE field vectors of n reals
    each -- what ecwam_hip_getspec_unpack takes (Wamintgr.read_restart_device).  The record markers are read as in read_fl: sub-records are
    joined, the markers checked."""
    with open(path, "rb") as f:
        # first pass over the markers: where the sub-records of the wanted record lie
        for rec in range(record + 1):
            parts, total = [], 0
            while True:
                h = f.read(4)
                if len(h) != 4:
                    raise EOFError(f"{path}: record {rec} not found")
                head = int(np.frombuffer(h, "<i4")[0])
                ln = abs(head)
                parts.append((f.tell(), ln))
                f.seek(ln, 1)
                total += ln
                t = f.read(4)
                if len(t) != 4 or abs(int(np.frombuffer(t, "<i4")[0])) != ln:
                    raise ValueError(f"{path}: corrupt record markers ({head} / {t!r})")
                if head >= 0:  # last (or only) sub-record
                    break
        dt = np.dtype(dtype)
        if total % dt.itemsize:
            raise ValueError(f"{path}: record holds {total} bytes, no whole number of {dt}")
        raw = np.empty(total, np.uint8)
        off = 0
        for pos, ln in parts:
            f.seek(pos)
            if f.readinto(memoryview(raw)[off:off + ln]) != ln:
                raise EOFError(f"{path}: record {record} is cut short")
            off += ln
    return raw.view(dt)


def write_record(path: str, data: np.ndarray, append: bool = False) -> None:
    """One unformatted sequential record from a flat array, as the array holds it: the counterpart of read_record (the framing of write_fl,
    sub-records included, without its transposition).  With `append` the record follows what the file holds."""
    raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    nb = raw.size
    with open(path, "ab" if append else "wb") as f:
        off, first = 0, True
        while True:
            ln = min(_MAX_SUB, nb - off)
            last = off + ln >= nb
            f.write(np.array([ln if last else -ln], dtype="<i4").tobytes())
            f.write(memoryview(raw[off:off + ln]))
            f.write(np.array([ln if first else -ln], dtype="<i4").tobytes())
            off += ln
            first = False
            if last:
                break


NRESTART_FIELDS = 16      # savstress.F90:112-127
_DATE_LEN = 14


def write_stress(path: str, dates, rfield: np.ndarray) -> None:
    """The LAW file of WRITESTRESS (writestress.F90:88-107): record 1 holds CDTPRO, CDATEWO, CDAWIFL, CDATEFL (14 characters each), then one record
    of n reals per restart field.  rfield: [16][n] in the working precision, already in the order of the file (ecwam_hip_savstress_pack relabels)."""
    a = np.asarray(rfield)
    if a.ndim != 2 or a.shape[0] != NRESTART_FIELDS:
        raise ValueError("write_stress: rfield is [16][n]")
    if len(dates) != 4:
        raise ValueError("write_stress: four dates (CDTPRO, CDATEWO, CDAWIFL, CDATEFL)")
    head = b"".join(str(d).encode("ascii").ljust(_DATE_LEN)[:_DATE_LEN] for d in dates)
    write_record(path, np.frombuffer(head, np.uint8))
    for f in range(NRESTART_FIELDS):
        write_record(path, a[f], append=True)


def read_stress(path: str, n: int, dtype=np.float32):
    """(dates, rfield [16][n]) of a LAW file, as READSTRESS reads it without relabelling (readstress.F90:99-115)."""
    head = read_record(path, 0)
    if head.size != 4 * _DATE_LEN:
        raise ValueError(f"{path}: record 1 holds {head.size} bytes, expected the four dates of {_DATE_LEN} characters")
    dates = [head[i * _DATE_LEN:(i + 1) * _DATE_LEN].tobytes().decode("ascii") for i in range(4)]
    out = np.empty((NRESTART_FIELDS, n), np.dtype(dtype))
    for f in range(NRESTART_FIELDS):
        rec = read_record(path, 1 + f, dtype)
        if rec.size != n:
            raise ValueError(f"{path}: field {f + 1} holds {rec.size} reals, expected {n}")
        out[f] = rec
    return dates, out
