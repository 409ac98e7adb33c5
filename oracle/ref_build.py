"""Builds the reference's own Fortran (IMPLSCH with its whole call tree, WDFLUXES, NEWWIND, CTUW, PROPAGS2 and the table initialisers)
into oracle/_ref/libecwam_ref_{sp,dp}.so.  TEST INFRASTRUCTURE ONLY: the product, bench.py and smoke() never load these libraries.

The reference's files are compiled IN PLACE and unmodified (-I to their directory); nothing of their text is copied into this repository.
What the reference's build generates -- one <routine>.intfb.h per routine -- is generated here too, into oracle/_ref/, by cutting each
routine's own header: the statement line, the USE lines and the declarations of the dummies.  What the reference takes from other
packages (fiat's PARKIND1 / YOMHOOK / EC_LUN, field_api's FIELD_MODULE, the fypp-generated YOWDRVTYPE) are the few-line stand-ins of
oracle/ref_stubs.F90; oracle/ref_driver.F90 is the BIND(C) layer oracle/reference.py calls.

The tree is found from ECWAM_REFERENCE_PATH, else from "reference_path" of BASELINE.json.  Where it does not exist nothing is built and
one line says so; where it exists a failure to compile is fatal.  Flags: -O2 -ffp-contract=off, no fast-math: the order of operations
of the source, which is what the oracle (oracle/Makefile) restates.

build_driver() builds the executables of the fixture drivers (tools/*_driver.F90, run by tools/make_golden_*.py) by the same recipe, in a
temporary directory: it is the one place that invokes the compiler for them.  A driver USEs the reference's real modules and restates none.
The rule: a driver holds a module of its own only where the reference's names another package, where the fake is the point of the driver,
or where a fixture cannot be recorded with the reference's (a finding about the recorded case; the fixture stays).  The survivors:

  module            driver    why
  YOWGRIB           readwind  the point of the driver: answers GRIB2WGRID's keys from a table in place of the GRIB decoder
  YOWGRIB           intake    the reference's is bound to GRIB_API; INITIALINT imports one name and calls nothing
  YOWGRIB           gribout   the same: WGRIBENCODE_VALUES imports three names it does not use on this path
  OML_MOD           gribout   another package (fiat); one name, used by this driver alone
  OML_MOD           ctu       the same package; CTUWDRV calls its one function, which answers 1 thread here (one block of all points)
  MPL_MODULE        intake    another package (fiat); one name (MPL_COMM), used by this driver alone
  MPL_DATA_MODULE   intake    the same
  YOWWIND           forcing   the reference's RWFAC is a PARAMETER (0.5); the recorded GETWND cases weigh the current with 1 and 0.625
  YOWPCONS          intake    the reference's WSTAR0 is a PARAMETER (0); the recorded INIT_FIELDG call sets 0.0625

Two procedures are a driver's own as well, external ones whose interface header is cut from the driver: IWAM_GET_UNIT (restart: opens the
file in the machine's byte order) and OUTMDLDCP (intake: never reached).  YOWUNBLKRORD (restart) and YOWPD (intake) are named in `standins`
without a module behind them: the routines name them only behind WAM_HAVE_UNWAM, which is not defined.
"""
from __future__ import annotations

import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
OUT = os.path.join(_HERE, "_ref")
FLANG = shutil.which("amdflang") or "/opt/rocm/lib/llvm/bin/flang"
FLAGS = ["-cpp", "-O2", "-ffp-contract=off", "-fPIC"]

# The routines of the reference that are compiled (src/ecwam/<name>.F90); the modules they USE are found from their text.
ROUTINES = """
implsch sdepthlim fkmean femean semean sinflx sinput sinput_ard sinput_jan wsigstar airsea taut_z0 z0wave halphap femeanws frcutindex
stresso tau_phi_hf stress_gc omegagc ns_gc chnkmin sdissip sdissip_ard sdissip_jan snonlin peak_ang transf transf_snl sdiwbk sdice sdice1
sdice2 sdice3 icebreak_modify_attenuation ciwabr sbottom wnfluxes imphftail setice stokestrn stokesdrift cimsstrn aki_ice
wdfluxes newwind ctuwini ctuw propags2
iniwcst mfr mfredir setwavphys tabu_swellft kerkei kzeone init_x0tauhf initgc inisnonlin nlweigt jafu init_sdiss_ardh cigetdeac
depthprpt aki meansqs_lf incdate
""".split()
OURS = ["ref_stubs.F90", "ref_driver.F90"]      # this project's own text: the stand-ins (first) and the BIND(C) layer (last)


def reference_root() -> str | None:
    p = os.environ.get("ECWAM_REFERENCE_PATH")
    if not p:
        try:
            with open(os.path.join(ROOT, "BASELINE.json")) as fh:
                p = json.load(fh).get("reference_path")
        except (OSError, ValueError):
            p = None
    return p if p and os.path.isdir(os.path.join(p, "src", "ecwam")) else None


def lib_path(precision: str) -> str:
    return os.path.join(OUT, f"libecwam_ref_{precision}.so")


# ---- interface headers ---------------------------------------------------------------------------------------------------------------
_DECL = re.compile(r"^\s*(INTEGER|REAL|LOGICAL|CHARACTER|COMPLEX|DOUBLE\s+PRECISION|TYPE\s*\(|CLASS\s*\(|EXTERNAL|DIMENSION|PARAMETER|SAVE|DATA)\b", re.I)
_UNIT = re.compile(r"^\s*(?:(?:RECURSIVE|PURE|ELEMENTAL)\s+)*(?:(?P<rtype>(?:INTEGER|REAL|LOGICAL|DOUBLE\s+PRECISION)\s*(?:\([^)]*\))?)\s+)?"
                   r"(?P<kind>SUBROUTINE|FUNCTION)\s+(?P<name>\w+)\s*(?:\((?P<args>[^)]*)\))?", re.I)


def _statements(text: str):
    """The statements of free-form source: comments dropped, continuation lines joined, preprocessor lines kept as they are."""
    cur = ""
    for raw in text.splitlines():
        if raw.startswith("#"):
            yield raw
            continue
        line = raw
        # a trailing comment (no header of the reference has a '!' inside a character constant)
        if "!" in line:
            line = line[:line.index("!")]
        if not line.strip():
            continue
        s = line.strip()
        if s.startswith("&"):
            s = s[1:].lstrip()
        if s.endswith("&"):
            cur += s[:-1] + " "
            continue
        yield cur + s
        cur = ""


def _entities(stmt: str) -> list[str]:
    body = stmt.split("::", 1)[1] if "::" in stmt else re.sub(_DECL, "", stmt, count=1)
    out, depth, tok = [], 0, ""
    for ch in body + ",":
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
        if ch == "," and depth == 0:
            m = re.match(r"\s*(\w+)", tok)
            if m:
                out.append(m.group(1).upper())
            tok = ""
        else:
            tok += ch
    return out


def interface_of(text: str) -> str | None:
    """INTERFACE ... END INTERFACE of the first program unit of `text`: None for a module or a program."""
    it = _statements(text)
    head = None
    for st in it:
        if st.startswith("#"):
            continue
        head = _UNIT.match(st)
        if head is None:
            return None
        stmt0 = st
        break
    if head is None:
        return None
    names = {a.strip().upper() for a in (head.group("args") or "").split(",") if a.strip()}
    names.add(head.group("name").upper())
    res = re.search(r"RESULT\s*\(\s*(\w+)\s*\)", stmt0, re.I)
    if res:
        names.add(res.group(1).upper())
    keep, cond = [stmt0], 0
    skip_iface = False
    for st in it:
        if st.startswith("#"):
            if re.match(r"#\s*include", st):
                continue
            if re.match(r"#\s*if", st):
                cond += 1
            elif re.match(r"#\s*endif", st):
                cond -= 1
            keep.append(st)
            continue
        u = st.strip().upper()
        if skip_iface:
            skip_iface = not u.startswith("END INTERFACE")
            continue
        if u.startswith("INTERFACE"):
            skip_iface = True
            continue
        if u.startswith("USE ") or u.startswith("USE,") or u.startswith("IMPLICIT") or u.startswith("IMPORT"):
            keep.append(st.strip())
        elif _DECL.match(st):
            attr = st.split("::", 1)[0].upper()
            if "PARAMETER" in attr or names.intersection(_entities(st)):
                keep.append(st.strip())
        else:
            break
    if cond != 0:
        keep = [k for k in keep if not k.startswith("#")]
    else:      # drop conditionals that enclose nothing
        changed = True
        while changed:
            changed = False
            for i in range(len(keep) - 1):
                if re.match(r"#\s*if", keep[i]) and re.match(r"#\s*endif", keep[i + 1]):
                    del keep[i:i + 2]
                    changed = True
                    break
    return "INTERFACE\n" + "\n".join(keep) + f"\nEND {head.group('kind').upper()} {head.group('name')}\nEND INTERFACE\n"


def write_headers(src: str, dst: str) -> int:
    """One <routine>.intfb.h for every routine file of the tree (every routine the compiled files may name in an #include)."""
    n = 0
    for f in sorted(os.listdir(src)):
        if not f.endswith(".F90"):
            continue
        with open(os.path.join(src, f), errors="replace") as fh:
            h = interface_of(fh.read())
        if h is None:
            continue
        with open(os.path.join(dst, f[:-4] + ".intfb.h"), "w") as fh:
            fh.write(h)
        n += 1
    return n


# ---- modules -------------------------------------------------------------------------------------------------------------------------
_USE = re.compile(r"^\s*USE\s*(?:,\s*INTRINSIC\s*)?(?:::)?\s*(\w+)", re.I | re.M)
_STANDINS = {"PARKIND1", "YOMHOOK", "EC_LUN", "FIELD_MODULE", "YOWDRVTYPE", "REF_DRIVER_MOD", "REF_ADVECTION_MOD", "ISO_C_BINDING", "ISO_FORTRAN_ENV", "IEEE_ARITHMETIC"}


def _uses(path: str, standins: frozenset[str] = frozenset()) -> set[str]:
    with open(path, errors="replace") as fh:
        return {m.upper() for m in _USE.findall(fh.read())} - _STANDINS - standins


def module_order(src: str, files: list[str], standins=()) -> list[str]:
    """The reference's module files (src/ecwam/<module>.F90) that `files` need, each after the modules it uses.  `standins` are modules the
    caller supplies itself (or that only a branch the preprocessor drops names): they are not looked for in the tree."""
    standins = frozenset(m.upper() for m in standins)
    order: list[str] = []
    seen: set[str] = set()

    def visit(mod: str) -> None:
        if mod in seen:
            return
        seen.add(mod)
        p = os.path.join(src, mod.lower() + ".F90")
        if not os.path.exists(p):
            raise RuntimeError(f"reference module {mod} not found at {p}")
        for d in sorted(_uses(p, standins)):
            visit(d)
        order.append(p)

    for f in files:
        for d in sorted(_uses(f, standins)):
            visit(d)
    return order


# ---- build ---------------------------------------------------------------------------------------------------------------------------
def _compile(src: str, obj: str, flags: list[str]) -> None:
    r = subprocess.run([FLANG, *flags, "-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError(f"reference build: flang failed for {src}:\n{r.stdout[-4000:]}")


def _includes(files: list[str]) -> set[str]:
    """The <routine>.intfb.h that `files` include."""
    names: set[str] = set()
    for f in files:
        with open(f, errors="replace") as fh:
            names.update(re.findall(r'^#include\s+"(\w+\.intfb\.h)"', fh.read(), re.M))
    return names


def _empty_headers(files: list[str], hdr: str, src: str) -> None:
    """Headers of routines of other packages (fiat's ABOR1 ...) that `files` include: empty, the stand-ins have explicit-shape dummies."""
    for h in _includes(files):
        if not os.path.exists(os.path.join(hdr, h)) and not os.path.exists(os.path.join(src, h)):
            open(os.path.join(hdr, h), "w").close()


def _stale(ref: str) -> bool:
    """The libraries are older than something they are made of: this project's own files (this one holds the list of routines) or a file of
    the reference tree's source directory."""
    libs = [lib_path(p) for p in ("sp", "dp")]
    if not all(os.path.exists(x) for x in libs):
        return True
    t = min(os.path.getmtime(x) for x in libs)
    src = os.path.join(ref, "src", "ecwam")
    made_of = [os.path.join(_HERE, f) for f in OURS] + [os.path.abspath(__file__)] + [os.path.join(src, f) for f in os.listdir(src)]
    return any(os.path.getmtime(f) > t for f in made_of)


def build(force: bool = False) -> bool:
    """True where the libraries exist afterwards, False where there is no reference tree."""
    ref = reference_root()
    if ref is None:
        print("[build] no reference tree (ECWAM_REFERENCE_PATH / BASELINE.json reference_path): oracle/_ref/ not built, "
              "the live-reference tests skip", file=sys.stderr)
        return False
    if not force and not _stale(ref):
        return True
    src = os.path.join(ref, "src", "ecwam")
    hdr = os.path.join(OUT, "intfb")
    shutil.rmtree(hdr, ignore_errors=True)
    os.makedirs(hdr, exist_ok=True)
    write_headers(src, hdr)
    routines = [os.path.join(src, r + ".F90") for r in ROUTINES]
    missing = [r for r in routines if not os.path.exists(r)]
    if missing:
        raise RuntimeError(f"reference build: not in the tree: {missing}")
    ours = [os.path.join(_HERE, f) for f in OURS]
    mods = module_order(src, routines + ours[1:])
    _empty_headers(routines + mods, hdr, src)
    for prec in ("dp", "sp"):
        d = os.path.join(OUT, prec)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        flags = FLAGS + ["-module-dir", d, "-I", d, "-I", hdr, "-I", src] + (["-DREF_SINGLE"] if prec == "sp" else [])
        objs = []

        def obj(p):
            o = os.path.join(d, os.path.basename(p)[:-4] + ".o")
            objs.append(o)
            return o

        for p in [ours[0], *mods]:                 # the stand-ins, then the modules in order
            _compile(p, obj(p), flags)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            list(ex.map(lambda p: _compile(p, obj(p), flags), routines))
        _compile(ours[1], obj(ours[1]), flags)
        tmp = lib_path(prec) + ".tmp"
        r = subprocess.run([FLANG, "-shared", "-fPIC", "-Wl,--no-undefined", "-o", tmp, *objs], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise RuntimeError(f"reference build: link failed:\n{r.stdout[-4000:]}")
        os.replace(tmp, lib_path(prec))
    return True


# ---- fixture drivers -----------------------------------------------------------------------------------------------------------------
def _external_units(text: str) -> dict[str, str]:
    """The external procedures of a driver (the program units that are neither its modules nor its program), by name: the driver carries
    the interface of a routine it supplies in place of the reference's, and its header is cut from there."""
    units, inside, cur = {}, None, None
    for line in text.splitlines():
        if line.lstrip().startswith(("!", "#")):
            continue
        if cur is not None:
            units[cur] += line + "\n"
            if re.match(rf"\s*END\s+(SUBROUTINE|FUNCTION)\s+{cur}\b", line, re.I):
                cur = None
        elif inside:
            inside = not re.match(r"\s*END\s+(MODULE|PROGRAM)\b", line, re.I)
        elif re.match(r"\s*(MODULE|PROGRAM)\s+\w+", line, re.I):
            inside = True
        elif _UNIT.match(line):
            cur = _UNIT.match(line).group("name")
            units[cur] = line + "\n"
    return units


def build_driver(driver_src: str, routines, workdir: str, precision: str, standins=(), flags=(), ref: str | None = None) -> str:
    """The executable of a fixture driver (tools/*_driver.F90), built in `workdir` (outside the tree) by the recipe of build(): the stand-ins
    of ref_stubs.F90, the reference's real modules that `routines` (names of src/ecwam/<name>.F90) and the driver use, in order, the driver,
    the routines, and the link.  `standins` names the modules of the reference tree that are not taken from it (the table in the module
    docstring); `flags` are the driver's own (-D..., -fopenmp).  The headers are written once per `workdir`, for both precisions: those of the
    tree's routines, over them those of the external procedures the driver defines, and empty ones as in build()."""
    src = os.path.join(ref or reference_root() or "", "src", "ecwam")
    if routines and not os.path.isdir(src):
        raise RuntimeError(f"driver build: no reference tree at {src}")
    routines = [os.path.join(src, r + ".F90") for r in routines]
    hdr = os.path.join(workdir, "intfb")
    fresh = not os.path.isdir(hdr)
    if fresh:
        os.makedirs(hdr)
        if os.path.isdir(src):
            write_headers(src, hdr)
        with open(driver_src) as fh:
            for name, unit in _external_units(fh.read()).items():
                with open(os.path.join(hdr, name.lower() + ".intfb.h"), "w") as out:
                    out.write(interface_of(unit))
    # a header names the modules of its routine: they are built too, though the routine itself (ABORT1 ...) may not be
    files = routines + [driver_src]
    while True:
        mods = module_order(src, files, standins)
        more = [p for p in (os.path.join(hdr, h) for h in sorted(_includes(files + mods))) if os.path.exists(p) and p not in files]
        if not more:
            break
        files += more
    if fresh:
        _empty_headers(routines + mods, hdr, src)
    d = os.path.join(workdir, precision)
    os.makedirs(d)
    # FLAGS without -fPIC (an executable, as the fixtures were recorded); -fopenmp, where a driver asks for it, goes to the link as well
    flags = [f for f in FLAGS if f != "-fPIC"] + ["-module-dir", d, "-I", d, "-I", hdr, "-I", src, *flags] + (["-DREF_SINGLE"] if precision == "sp" else [])
    # the driver before the routines: where it supplies a module (YOWGRIB ...), the routines use it
    first = [os.path.join(_HERE, OURS[0]), *mods, driver_src]
    objs = {p: os.path.join(d, os.path.basename(p)[:-4] + ".o") for p in first + routines}
    for p in first:
        _compile(p, objs[p], flags)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda p: _compile(p, objs[p], flags), routines))
    exe = os.path.join(d, os.path.basename(driver_src)[:-4])
    r = subprocess.run([FLANG, *[f for f in flags if f == "-fopenmp"], "-o", exe, *objs.values()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError(f"driver build: link failed:\n{r.stdout[-4000:]}")
    return exe


if __name__ == "__main__":
    build(force=True)
