"""What the C interface refuses, and with which words: every case below returns 1 and leaves exactly the given text in
ecwam_hip_last_error().  The library is called through lib.load() with ctypes, not through ecwam_amd.api, which validates before the library
does.  The expected texts are the literals of csrc/capi.hip; the order in which an entry point makes its checks decides which of two
mistakes is reported, and the cases pin that order too.

Every case is refused before anything is launched: no case hands over a pointer or a size the library would go on to use.  Wherever the
refusal does not itself need points, the range is empty (n = 0, kijs = kijl = 0), so that a check that went missing would launch nothing.
The loop stops at the first case that is not refused.
"""
import ctypes as C

import numpy as np
import pytest

from ecwam_amd import lib as L
from ecwam_amd.tables import Config, Tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NANG, NFRE, NPTS = 12, 36, 8

# argument names of the entry points (include/ecwam_hip.h), the context first
SPEC = {
    "set_obstructions": "obs n",
    "propags2": "f1 f3 klon klat kcor w kijs kijl nd3s nd3e copy_rest stream",
    "ctuw": "n nland ngy delpro mstart mend kxlt zdello xdella cosph sinph klon klat kcor wlat wcor cgroup_ext cosphm1_ext w cflfail stream",
    "propags2_otf": "f1 f3 n ngy delpro kxlt zdello xdella cosph sinph klon klat kcor wlat wcor cgroup_ext cosphm1_ext order kijs kijl nd3s nd3e "
                    "copy_rest stream",
    "propags2_otf_split": "f1 f3 n ngy delpro delpro_lf ifrelfmax in_nfre gout gout_nfre kxlt zdello xdella cosph sinph klon klat kcor wlat wcor "
                          "cgroup_ext cosphm1_ext order kijs kijl nd3s nd3e copy_rest stream",
    "propags2_otf_fast": "f1 f3 n ngy delpro delpro_lf ifrelfmax in_nfre gin gin_nfre out_nfre gout gout_nfre kxlt zdello xdella cosph sinph klon "
                         "klat kcor wlat wcor cgroup_ext cosphm1_ext order kijs kijl nd3s nd3e copy_rest stream",
    "set_fastwave_copy": "g g_nfre",
    "copy_freq_range": "src dst n m_first m_last dst_nfre stream",
    "propdot": "n nland kxlt zdello xdella cosph klon klat wlat cosphm1_ext depth_ext u_ext v_ext refr stream",
    "ctuw_refra": "n nland ngy delpro mstart mend kxlt zdello xdella cosph sinph klon klat kcor wlat wcor cgroup_ext omosnh2kd_ext wavnum_ext "
                  "cosphm1_ext refr llcflcuroff range cflfail stream",
    "propags2_refra": "f1 f3 n ngy delpro kxlt zdello xdella cosph sinph klon klat kcor wlat wcor cgroup_ext omosnh2kd_ext wavnum_ext cosphm1_ext "
                      "refr range kijs kijl nd3s nd3e copy_rest stream",
    "implsch": "kijs kijl fl1 wvprpt ff intf mij xllws wam2nemo dbg stream",
    "propags2_implsch": "f1 f3 n ngy delpro kxlt zdello xdella cosph sinph klon klat kcor wlat wcor cgroup_ext cosphm1_ext kijs kijl nd3s nd3e "
                        "wvprpt ff intf mij xllws wam2nemo delpro_lf ifrelfmax gin gin_nfre flags stream",
    "outbs": "kijs kijl fl1 zmiss out stream",
    "outbs_sepwisw": "kijs kijl fl1 xllws wvprpt ff flags zmiss out stream",
    "outbs_partition": "kijs kijl fl1 xllws mij wvprpt ff flags zmiss out stream",
    "outbs_extremes": "kijs kijl fl1 wvprpt ff flags out stream",
    "outbs_absolute": "kijs kijl fl1 wvprpt ucur vcur ff flags zmiss out fl2nd stream",
    "outbs_second_order": "kijs kijl fl1 wvprpt depth ucur vcur ff sig zmiss out fl2nd stream",
    "outwnorm": "field stride n zmiss result stream",
    "newwind_icode": "n ff ff_next icode_wnd stream",
    "nosource": "kijs kijl fl1 mij xllws stream",
    "chunks_to_points": "chunked points nproma nchnk npts n2 n3 stream",
    "points_to_chunks": "points chunked nproma nchnk npts n2 n3 stream",
    "member_scatter": "chunked rows nproma nchnk npts nm row_stride row_off elem_bytes stream",
    "member_gather": "rows chunked nproma nchnk npts nm row_stride row_off elem_bytes stream",
    "pack_rows": "fl idx n buf stream",
    "unpack_rows": "buf n fl dst0 stream",
    "halo_setup": "rank nranks npeers peer send_count send_idx recv_dst0 recv_count",
    "proenvhalo_pack": "n wvprpt omosnh2kd depth ucur vcur buffer_ext stream",
    "proenvhalo_unpack": "nrows buffer_ext land wavnum_ext cgroup_ext omosnh2kd_ext depth_ext u_ext v_ext stream",
}
# entry points whose only refusal here is the null context (no arguments of interest)
NULL_CONTEXT_ONLY = ["set_second_order", "newwind", "halo_start", "halo_finish", "halo_pack_host", "halo_unpack_host"]
# integer arguments that are not 0 in a well-formed call with an empty range, and the pointers that are optional (NULL by default)
INT_DEFAULT = dict(nd3s=1, nd3e=NFRE, mstart=1, mend=NFRE, m_first=1, m_last=NFRE, ngy=4, nland=NPTS, stride=1, icode_wnd=3, nproma=4, nchnk=2, n2=1,
                   n3=1, nm=1, row_stride=1, elem_bytes=4, nranks=1)
OPTIONAL = {"stream", "order", "gin", "gout", "dbg", "wam2nemo", "fl2nd", "cflfail", "obs", "g", "peer", "send_count", "send_idx", "recv_dst0",
            "recv_count", "result"}
SECOND = {"f3", "dst", "out", "points", "rows", "buf"}      # outputs: another buffer than the inputs, so that nothing aliases by default


class Ctx:
    """One context of 12 directions x 36 frequencies and its 8-point device buffers."""

    def __init__(self, prec):
        self.lib = L.load()
        self.prec = prec
        self.rb = 4 if prec == "sp" else 8
        self.t = Tables(Config(nang=NANG, nfre=NFRE, nfre_red=NFRE), np.float32 if prec == "sp" else np.float64)
        params = L.make_params(self.t)
        tp, keep = L.make_tables(self.t)
        self.h = C.c_void_p()
        rc = self.lib.ecwam_hip_create(C.byref(params), C.byref(tp), self.rb, 0, C.byref(self.h))
        assert rc == 0, self.lib.ecwam_hip_last_error().decode()
        dt = torch.float32 if prec == "sp" else torch.float64
        self.bufs = [torch.zeros(NPTS * NANG * NFRE, dtype=dt, device="cuda:0") for _ in range(2)]
        self.a, self.b = (x.data_ptr() for x in self.bufs)
        assert self.a % 16 == 0 and self.b % 16 == 0
        self.result = (C.c_double * 4)()

    def close(self):
        self.lib.ecwam_hip_destroy(self.h)

    def call(self, name, null_ctx=False, **over):
        """The entry point with an empty range and every mandatory pointer set, except for what `over` names."""
        fn = getattr(self.lib, "ecwam_hip_" + name)
        names = SPEC[name].split()
        assert len(names) + 1 == len(fn.argtypes), name
        assert set(over) <= set(names), (name, over)
        args = []
        for nm, typ in zip(names, fn.argtypes[1:]):
            if nm in over:
                v = over[nm]
            elif typ is C.c_double:
                v = 1.0
            elif typ in (C.c_int, C.c_longlong):
                v = INT_DEFAULT.get(nm, 0)
            elif nm == "result":
                v = self.result
            else:
                v = None if nm in OPTIONAL else (self.b if nm in SECOND else self.a)
            args.append(v)
        rc = fn(None if null_ctx else self.h, *args)
        return rc, self.lib.ecwam_hip_last_error().decode()

    def set_second_order(self):
        """The tables of ecwam_amd.second_order in the storage order of the C interface (as ecwam_amd.api uploads them)."""
        from ecwam_amd.second_order import SecondOrderTables

        so = SecondOrderTables(self.t)
        shape = (so.NDEPTH, so.NANGH, so.NFREH, so.NFREH)
        host = [np.ascontiguousarray(np.asarray(getattr(so, c), self.t.dtype).reshape(shape).transpose(3, 2, 1, 0)) for c in so.COEFFICIENTS]
        imp, imm = (np.ascontiguousarray(x.T.astype(np.int32)) for x in (so.IM_P, so.IM_M))
        rc = self.lib.ecwam_hip_set_second_order(self.h, so.NDEPTH, float(so.DEPTHA), float(so.DEPTHD), so.NMAX, imp.ctypes.data, imm.ctypes.data,
                                                 *[x.ctypes.data for x in host])
        assert rc == 0, self.lib.ecwam_hip_last_error().decode()


@pytest.fixture(scope="module", params=["sp", "dp"])
def ctx(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = Ctx(request.param)
    yield c
    c.close()


SOME = dict(kijs=0, kijl=NPTS)      # a non-empty range of points
OTF_BAD_RANGE = "ecwam_hip_propags2_otf: bad range"
OTF_FAST_ROWS = "ecwam_hip_propags2_otf_fast: compact rows must be 16-byte aligned and hold a multiple of 16 bytes per direction"
OTF_GOUT = ("ecwam_hip_propags2_otf: the compact output buffer must be 16-byte aligned, distinct from F1, and hold a multiple of 16 bytes per "
            "direction")
FASTCOPY = "ecwam_hip_set_fastwave_copy: the compact rows must be 16-byte aligned and hold a multiple of 16 bytes per direction"
FUSED = "ecwam_hip_propags2_implsch: "
FUSED_NO_BUILD = (FUSED + "no one-kernel build covers the configuration (ecwam_hip_propags2_implsch_supported): call ecwam_hip_propags2_otf and "
                  "ecwam_hip_implsch")
FUSED_GIN = (FUSED + "the compact fast-wave rows must be 16-byte aligned, hold the fast waves in a multiple of 16 bytes per direction, and differ "
             "from the rows of ecwam_hip_set_fastwave_copy")
FUSED_LF = FUSED + "fast waves (ifrelfmax > 0) come with their compact input rows (gin), and only then"


def cases(c):
    """(entry point, arguments that differ from the well-formed empty call, expected text)"""
    a, b, odd = c.a, c.b, c.a + c.rb      # odd: a pointer into a buffer that is not 16-byte aligned
    tab = [
        ("set_obstructions", dict(n=-1), "ecwam_hip_set_obstructions: bad size"),
        ("set_obstructions", dict(obs=a, n=0), "ecwam_hip_set_obstructions: bad size"),
        # stored weights
        ("propags2", dict(kijs=1, kijl=0), "ecwam_hip_propags2: bad range"),
        ("propags2", dict(nd3e=NFRE + 1), "ecwam_hip_propags2: bad range"),
        ("propags2", dict(nd3s=0), "ecwam_hip_propags2: bad range"),
        ("propags2", dict(SOME, f1=None), "ecwam_hip_propags2: null pointer"),
        ("propags2", dict(SOME, w=None), "ecwam_hip_propags2: null pointer"),
        ("propags2", dict(f3=a), "ecwam_hip_propags2: F1 and F3 must not alias"),
        ("ctuw", dict(n=-1), "ecwam_hip_ctuw: bad range"),
        ("ctuw", dict(mend=NFRE + 1), "ecwam_hip_ctuw: bad range"),
        ("ctuw", dict(mstart=0), "ecwam_hip_ctuw: bad range"),
        ("ctuw", dict(n=NPTS, cflfail=None), "ecwam_hip_ctuw: null pointer"),
        ("ctuw", dict(n=NPTS, cflfail=a, cosphm1_ext=None), "ecwam_hip_ctuw: null pointer"),
        ("ctuw", dict(n=NPTS, cflfail=a, kxlt=None), "ecwam_hip_ctuw: null pointer"),
        # on-the-fly weights: the three entry points are one function
        ("propags2_otf", dict(kijs=1, kijl=0), OTF_BAD_RANGE),
        ("propags2_otf", dict(kijs=-1), OTF_BAD_RANGE),
        ("propags2_otf", dict(nd3e=NFRE + 1), OTF_BAD_RANGE),
        ("propags2_otf", dict(kijl=1, n=0), OTF_BAD_RANGE),
        ("propags2_otf", dict(copy_rest=4), "ecwam_hip_propags2_otf: 2-D tiles need a processing order"),
        ("propags2_otf", dict(SOME, n=NPTS, f3=None), "ecwam_hip_propags2_otf: null pointer"),
        ("propags2_otf", dict(SOME, n=NPTS, wcor=None), "ecwam_hip_propags2_otf: null pointer"),
        ("propags2_otf", dict(f3=a), "ecwam_hip_propags2_otf: F1 and F3 must not alias"),
        ("propags2_otf_split", dict(kijs=1, kijl=0), OTF_BAD_RANGE),
        ("propags2_otf_split", dict(ifrelfmax=NFRE + 1), OTF_BAD_RANGE),
        ("propags2_otf_split", dict(SOME, n=NPTS, sinph=None), "ecwam_hip_propags2_otf: null pointer"),
        ("propags2_otf_split", dict(f3=a), "ecwam_hip_propags2_otf: F1 and F3 must not alias"),
        ("propags2_otf_split", dict(gout=a, gout_nfre=8), OTF_GOUT),                       # gout == F1
        ("propags2_otf_split", dict(gout=b + 16 + c.rb, gout_nfre=8), OTF_GOUT),            # not aligned
        ("propags2_otf_split", dict(gout=b + 16, gout_nfre=7), OTF_GOUT),                   # 7 reals are no multiple of 16 bytes
        ("propags2_otf_split", dict(gout=b + 16, gout_nfre=NFRE + 4), OTF_GOUT),
        ("propags2_otf_split", dict(in_nfre=16), "ecwam_hip_propags2_otf: a compact input buffer must hold every advected frequency; copy_rest "
                                                 "only into a compact output of the same width"),
        ("propags2_otf_fast", dict(kijs=1, kijl=0), OTF_BAD_RANGE),
        ("propags2_otf_fast", dict(SOME, n=NPTS, klon=None), "ecwam_hip_propags2_otf: null pointer"),
        ("propags2_otf_fast", dict(f3=a), "ecwam_hip_propags2_otf: F1 and F3 must not alias"),
        ("propags2_otf_fast", dict(out_nfre=16), "ecwam_hip_propags2_otf_fast: a compact output buffer must hold every advected frequency and "
                                                 "excludes a second compact copy"),
        ("propags2_otf_fast", dict(out_nfre=16, nd3e=16, gout=b + 16, gout_nfre=8),
         "ecwam_hip_propags2_otf_fast: a compact output buffer must hold every advected frequency and excludes a second compact copy"),
        ("propags2_otf_fast", dict(gin=b + 16, gin_nfre=8, in_nfre=16), "ecwam_hip_propags2_otf_fast: the compact fast-wave input goes with full "
                                                                        "input rows"),
        ("propags2_otf_fast", dict(gin=b + 16, gin_nfre=0), "ecwam_hip_propags2_otf_fast: bad compact input buffer"),
        ("propags2_otf_fast", dict(gin=b, gin_nfre=8), "ecwam_hip_propags2_otf_fast: bad compact input buffer"),      # gin == F3
        ("propags2_otf_fast", dict(gin=b + 16 + c.rb, gin_nfre=8), OTF_FAST_ROWS),
        ("propags2_otf_fast", dict(gin=b + 16, gin_nfre=7), OTF_FAST_ROWS),
        ("propags2_otf_fast", dict(out_nfre=16, nd3e=16, f3=b + c.rb), OTF_FAST_ROWS),
        ("propags2_otf_fast", dict(in_nfre=16, nd3e=16, f1=odd), OTF_FAST_ROWS),
        ("set_fastwave_copy", dict(g=odd, g_nfre=8), FASTCOPY),
        ("set_fastwave_copy", dict(g=a, g_nfre=7), FASTCOPY),
        ("set_fastwave_copy", dict(g=a, g_nfre=0), FASTCOPY),
        ("set_fastwave_copy", dict(g=a, g_nfre=NFRE + 4), FASTCOPY),
        ("copy_freq_range", dict(n=-1), "ecwam_hip_copy_freq_range: bad range"),
        ("copy_freq_range", dict(m_last=NFRE + 1), "ecwam_hip_copy_freq_range: bad range"),
        ("copy_freq_range", dict(dst_nfre=16), "ecwam_hip_copy_freq_range: bad range"),
        ("copy_freq_range", dict(n=NPTS, dst=None), "ecwam_hip_copy_freq_range: null pointer"),
        # refraction
        ("propdot", dict(n=-1), "ecwam_hip_propdot: bad range"),
        ("propdot", dict(n=NPTS, refr=None), "ecwam_hip_propdot: null pointer"),
        ("propdot", dict(n=NPTS, zdello=None), "ecwam_hip_propdot: null pointer"),
        ("ctuw_refra", dict(n=-1), "ecwam_hip_ctuw_refra: bad range"),
        ("ctuw_refra", dict(mend=NFRE + 1), "ecwam_hip_ctuw_refra: bad range"),
        ("ctuw_refra", dict(range=2), "ecwam_hip_ctuw_refra: bad range"),
        ("ctuw_refra", dict(range=-1), "ecwam_hip_ctuw_refra: bad range"),
        ("ctuw_refra", dict(n=NPTS, cflfail=None), "ecwam_hip_ctuw_refra: null pointer"),
        ("ctuw_refra", dict(n=NPTS, cflfail=a, wlat=None), "ecwam_hip_ctuw_refra: null pointer"),
        ("propags2_refra", dict(kijs=1, kijl=0), "ecwam_hip_propags2_refra: bad range"),
        ("propags2_refra", dict(kijs=-1), "ecwam_hip_propags2_refra: bad range"),
        ("propags2_refra", dict(nd3e=NFRE + 1), "ecwam_hip_propags2_refra: bad range"),
        ("propags2_refra", dict(range=2), "ecwam_hip_propags2_refra: bad range"),
        ("propags2_refra", dict(SOME, n=NPTS, f1=None), "ecwam_hip_propags2_refra: null pointer"),
        ("propags2_refra", dict(SOME, n=NPTS, wavnum_ext=None), "ecwam_hip_propags2_refra: null pointer"),      # the shared checks of the kernel
        ("propags2_refra", dict(SOME, n=NPTS, kxlt=None), "ecwam_hip_propags2_refra: null pointer"),
        ("propags2_refra", dict(f3=a), "ecwam_hip_propags2_refra: F1 and F3 must not alias"),
        # source terms
        ("implsch", dict(kijs=1, kijl=0), "ecwam_hip_implsch: bad range"),
        ("implsch", dict(kijs=-1), "ecwam_hip_implsch: bad range"),
        ("implsch", dict(SOME, xllws=None), "ecwam_hip_implsch: null pointer"),
        ("implsch", dict(dbg=a), "ecwam_hip_implsch: the per-point debug rows were an output of the retired one-point-per-wavefront kernel: pass NULL"),
        ("nosource", dict(kijs=1, kijl=0), "ecwam_hip_nosource: bad range"),
        ("nosource", dict(kijs=-1), "ecwam_hip_nosource: bad range"),
        ("nosource", dict(SOME, mij=None), "ecwam_hip_nosource: null pointer"),
        ("newwind_icode", dict(n=NPTS, ff=None), "ecwam_hip_newwind: null pointer"),
        ("newwind_icode", dict(icode_wnd=4), "ecwam_hip_newwind: ICODE_WND must be 1, 2 or 3"),
        ("propags2_implsch", dict(flags=1), FUSED + "unknown flags"),
        # outputs
        ("outbs", dict(kijs=1, kijl=0), "ecwam_hip_outbs: bad range"),
        ("outbs", dict(kijs=-1), "ecwam_hip_outbs: bad range"),
        ("outbs", dict(SOME, out=None), "ecwam_hip_outbs: null pointer"),
        ("outbs_sepwisw", dict(kijs=1, kijl=0), "ecwam_hip_outbs_sepwisw: bad range"),
        ("outbs_sepwisw", dict(kijs=-1), "ecwam_hip_outbs_sepwisw: bad range"),
        ("outbs_sepwisw", dict(SOME, xllws=None), "ecwam_hip_outbs_sepwisw: null pointer"),
        ("outbs_sepwisw", dict(flags=2), "ecwam_hip_outbs_sepwisw: unknown flags"),
        ("outbs_sepwisw", dict(SOME, ff=None, flags=2), "ecwam_hip_outbs_sepwisw: null pointer"),
        ("outbs_partition", dict(kijs=1, kijl=0), "ecwam_hip_outbs_partition: bad range"),
        ("outbs_partition", dict(kijs=-1), "ecwam_hip_outbs_partition: bad range"),
        ("outbs_partition", dict(SOME, mij=None), "ecwam_hip_outbs_partition: null pointer"),
        ("outbs_partition", dict(flags=1), "ecwam_hip_outbs_partition: CLDOMAIN = 's' (flags bit 0) is not supported: SEP3TR would read an FSEA that "
                                           "SEPWISW has not computed"),
        ("outbs_partition", dict(flags=3), "ecwam_hip_outbs_partition: CLDOMAIN = 's' (flags bit 0) is not supported: SEP3TR would read an FSEA that "
                                           "SEPWISW has not computed"),
        ("outbs_partition", dict(flags=2), "ecwam_hip_outbs_partition: unknown flags"),
        ("outbs_extremes", dict(kijs=1, kijl=0), "ecwam_hip_outbs_extremes: bad range"),
        ("outbs_extremes", dict(kijs=-1), "ecwam_hip_outbs_extremes: bad range"),
        ("outbs_extremes", dict(SOME, wvprpt=None), "ecwam_hip_outbs_extremes: null pointer"),
        ("outbs_extremes", dict(flags=2), "ecwam_hip_outbs_extremes: unknown flags"),
        ("outbs_absolute", dict(kijs=1, kijl=0), "ecwam_hip_outbs_absolute: bad range"),
        ("outbs_absolute", dict(kijs=-1), "ecwam_hip_outbs_absolute: bad range"),
        ("outbs_absolute", dict(flags=1), "ecwam_hip_outbs_absolute: unknown flags"),
        ("outbs_absolute", dict(SOME, fl1=None, flags=1), "ecwam_hip_outbs_absolute: unknown flags"),      # the flags come first here
        ("outbs_absolute", dict(SOME, fl1=None), "ecwam_hip_outbs_absolute: null pointer"),
        ("outbs_absolute", dict(fl2nd=a), "ecwam_hip_outbs_absolute: FL1 and FL2ND must not alias"),
        ("outbs_second_order", dict(kijs=1, kijl=0), "ecwam_hip_outbs_second_order: bad range"),
        ("outbs_second_order", dict(kijs=-1), "ecwam_hip_outbs_second_order: bad range"),
        ("outbs_second_order", dict(), "ecwam_hip_outbs_second_order: the second-order tables are not set (ecwam_hip_set_second_order)"),
        ("outbs_second_order", dict(sig=2.0), "ecwam_hip_outbs_second_order: the second-order tables are not set (ecwam_hip_set_second_order)"),
        ("outwnorm", dict(n=-1), "ecwam_hip_outwnorm: bad arguments"),
        ("outwnorm", dict(stride=0), "ecwam_hip_outwnorm: bad arguments"),
        ("outwnorm", dict(result=None), "ecwam_hip_outwnorm: bad arguments"),
        ("outwnorm", dict(n=NPTS, field=None), "ecwam_hip_outwnorm: bad arguments"),
        # layout and exchange helpers
        ("chunks_to_points", dict(nproma=0), "ecwam_hip_chunks_to_points: bad shape"),
        ("chunks_to_points", dict(npts=9), "ecwam_hip_chunks_to_points: bad shape"),
        ("points_to_chunks", dict(npts=4), "ecwam_hip_points_to_chunks: bad shape"),
        ("member_scatter", dict(elem_bytes=2), "ecwam_hip_member_scatter: bad shape"),
        ("member_scatter", dict(npts=NPTS, chunked=None), "ecwam_hip_member_scatter: null pointer"),
        ("member_gather", dict(row_off=1), "ecwam_hip_member_gather: bad shape"),
        ("member_gather", dict(npts=NPTS, chunked=None), "ecwam_hip_member_gather: null pointer"),
        ("pack_rows", dict(n=NPTS, idx=None), "ecwam_hip_pack_rows: null pointer"),
        ("unpack_rows", dict(n=NPTS, fl=None), "ecwam_hip_unpack_rows: null pointer"),
        ("halo_setup", dict(nranks=0), "ecwam_hip_halo_setup: bad arguments"),
        ("halo_setup", dict(npeers=1), "ecwam_hip_halo_setup: bad arguments"),
        ("proenvhalo_pack", dict(n=-1), "ecwam_hip_proenvhalo_pack: bad arguments"),
        ("proenvhalo_pack", dict(n=NPTS, depth=None), "ecwam_hip_proenvhalo_pack: bad arguments"),
        ("proenvhalo_unpack", dict(nrows=-1), "ecwam_hip_proenvhalo_unpack: bad arguments"),
        ("proenvhalo_unpack", dict(land=None), "ecwam_hip_proenvhalo_unpack: bad arguments"),
    ]
    # the one-kernel step: single precision has a 12-direction build, double precision has none and says so after the flags
    fused = dict(n=NPTS)
    if c.prec == "dp":
        tab += [("propags2_implsch", fused, FUSED_NO_BUILD), ("propags2_implsch", dict(fused, kijs=1, kijl=0), FUSED_NO_BUILD)]
    else:
        tab += [
            ("propags2_implsch", dict(fused, kijs=1, kijl=0), FUSED + "bad range"),
            ("propags2_implsch", dict(fused, kijs=-1), FUSED + "bad range"),
            ("propags2_implsch", dict(fused, kijl=NPTS + 1), FUSED + "bad range"),
            ("propags2_implsch", dict(fused, nd3e=NFRE + 1), FUSED + "bad range"),
            ("propags2_implsch", dict(fused, **SOME, xllws=None), FUSED + "null pointer"),
            ("propags2_implsch", dict(fused, **SOME, cgroup_ext=None), FUSED + "null pointer"),
            ("propags2_implsch", dict(fused, f3=a), FUSED + "F1 and F3 must not alias (the neighbours of a point are read while other points are stored)"),
            ("propags2_implsch", dict(fused, f1=odd), FUSED + "the spectra must be 16-byte aligned"),
            ("propags2_implsch", dict(fused, f3=b + c.rb), FUSED + "the spectra must be 16-byte aligned"),
            ("propags2_implsch", dict(fused, ifrelfmax=4), FUSED_LF),
            ("propags2_implsch", dict(fused, gin=a + 16, gin_nfre=8), FUSED_LF),
            ("propags2_implsch", dict(fused, ifrelfmax=NFRE + 1, gin=a + 16, gin_nfre=8), FUSED_LF),
            ("propags2_implsch", dict(fused, ifrelfmax=4, gin=a + 16 + c.rb, gin_nfre=8), FUSED_GIN),
            ("propags2_implsch", dict(fused, ifrelfmax=4, gin=a + 16, gin_nfre=7), FUSED_GIN),
            ("propags2_implsch", dict(fused, ifrelfmax=4, gin=a + 16, gin_nfre=2), FUSED_GIN),      # narrower than the fast waves
            ("propags2_implsch", dict(fused, ifrelfmax=4, gin=a + 16, gin_nfre=8, nd3s=2), FUSED_GIN),
            ("propags2_implsch", dict(fused, ifrelfmax=4, gin=a + 16, gin_nfre=8, delpro_lf=0.0), FUSED_GIN),
        ]
    return tab


def refused(c, name, over, want, **kw):
    rc, msg = c.call(name, **over, **kw)
    assert rc == 1 and msg == want, (c.prec, name, over, rc, msg)


def test_null_context(ctx):
    for name in list(SPEC) + NULL_CONTEXT_ONLY:
        fn = getattr(ctx.lib, "ecwam_hip_" + name)
        zero = [0.0 if t is C.c_double else (0 if t in (C.c_int, C.c_longlong) else None) for t in fn.argtypes[1:]]
        assert fn(None, *zero) == 1 and ctx.lib.ecwam_hip_last_error().decode() == "null context", name
    # ... and with every other argument well formed
    for name in SPEC:
        refused(ctx, name, {}, "null context", null_ctx=True)
    assert ctx.lib.ecwam_hip_implsch_reserve(None, NPTS) == 1
    assert ctx.lib.ecwam_hip_last_error().decode() == "ecwam_hip_implsch_reserve: null context"
    assert ctx.lib.ecwam_hip_propags2_implsch_supported(None) == 0


def test_refusals_and_their_order(ctx):
    assert bool(ctx.lib.ecwam_hip_propags2_implsch_supported(ctx.h) & 1) == (ctx.prec == "sp")
    tab = cases(ctx)
    assert {name for name, _, _ in tab} == set(SPEC)      # every entry point of the table has a case
    for name, over, want in tab:
        refused(ctx, name, over, want)


def test_more_points_than_the_obstruction_table_holds(ctx):
    """A table of 4 points (the library only keeps the pointer) and calls that need 8."""
    assert ctx.lib.ecwam_hip_set_obstructions(ctx.h, ctx.a, 4) == 0
    try:
        geom = dict(n=NPTS)
        tab = [("ctuw", dict(geom, cflfail=ctx.a), "ecwam_hip_ctuw"), ("propags2_otf", dict(geom, **SOME), "ecwam_hip_propags2_otf"),
               ("propags2_otf_fast", dict(geom, **SOME), "ecwam_hip_propags2_otf"), ("propags2_refra", dict(geom, **SOME), "ecwam_hip_propags2_refra")]
        if ctx.prec == "sp":
            tab.append(("propags2_implsch", dict(geom, **SOME), "ecwam_hip_propags2_implsch"))
        for name, over, who in tab:
            refused(ctx, name, over, who + ": more points than the obstruction table holds")
        # a processing order: the points it may name count, not the range of its entries
        refused(ctx, "propags2_otf", dict(n=NPTS, kijs=0, kijl=2, order=ctx.a), "ecwam_hip_propags2_otf: more points than the obstruction table holds")
        # the checks before it keep their place
        refused(ctx, "propags2_otf", dict(geom, **SOME, f3=ctx.a), "ecwam_hip_propags2_otf: F1 and F3 must not alias")
        refused(ctx, "propags2_refra", dict(geom, **SOME, f3=None), "ecwam_hip_propags2_refra: null pointer")
    finally:
        assert ctx.lib.ecwam_hip_set_obstructions(ctx.h, None, 0) == 0


def test_second_order_refusals(ctx):
    """With the tables set, the checks behind "not set": null pointers, FL1 / FL2ND, SIG."""
    ctx.set_second_order()
    try:
        so = "ecwam_hip_outbs_second_order: "
        refused(ctx, "outbs_second_order", dict(kijs=1, kijl=0), so + "bad range")
        refused(ctx, "outbs_second_order", dict(SOME, depth=None), so + "null pointer (fl1, wvprpt, depth and out are needed)")
        refused(ctx, "outbs_second_order", dict(SOME, out=None, sig=2.0), so + "null pointer (fl1, wvprpt, depth and out are needed)")
        refused(ctx, "outbs_second_order", dict(fl2nd=ctx.a), so + "FL1 and FL2ND must not alias")
        refused(ctx, "outbs_second_order", dict(fl2nd=ctx.a, sig=2.0), so + "FL1 and FL2ND must not alias")
        for sig in (2.0, 0.0, -1.5, float("nan")):
            refused(ctx, "outbs_second_order", dict(sig=sig), so + "SIG must be +1 or -1")
    finally:
        assert ctx.lib.ecwam_hip_set_second_order(ctx.h, 0, 1.0, 1.1, 0, None, None, None, None, None, None, None) == 0
    refused(ctx, "outbs_second_order", {}, "ecwam_hip_outbs_second_order: the second-order tables are not set (ecwam_hip_set_second_order)")
