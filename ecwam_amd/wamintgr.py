"""WAMINTGR on the device: the reference's per-step call sequence (wamintgr.F90:94-146)

    IF (CDATE == CDTPRA) CALL PROPAG_WAM      -> halo exchange (MPEXCHNG) + PROPAGS2 (+ fast-wave sub-steps)
    CALL NEWWIND                              -> forcing hand-over when a new wind field is due
    IF (CDATE >= CDTIMPNEXT) CALL IMPLSCH     -> source-term integration of every owned point

with the state resident in HBM between steps (the GPU variant's behaviour, wamintgr_loki_gpu.F90:99-201).
One instance = one rank = one GPU; ranks own contiguous sea-point ranges (decomp.py) and exchange
halo spectra point-to-point through torch.distributed (backend "nccl" = RCCL over xGMI).
"""
from __future__ import annotations

import numpy as np
import torch

from . import api, decomp, synthetic as syn
from .tables import Config, Tables

OUTBS_SEP_FIELDS = api.OUTBS_SEP_FIELDS     # the columns of Wamintgr.outbs_sepwisw()
OUTBS_EXT_FIELDS = api.OUTBS_EXT_FIELDS     # the columns of Wamintgr.outbs_extremes()
OUTBS_PART_FIELDS = api.OUTBS_PART_FIELDS   # the columns of Wamintgr.outbs_partition()
OUTBS_ABS_FIELDS = api.OUTBS_ABS_FIELDS     # the columns of Wamintgr.outbs_absolute()
OUTBS_INT_FIELDS = api.OUTBS_INT_FIELDS     # the first eight columns of Wamintgr.outbs_integrals(); the bands follow


class HaloExchange:
    """MPEXCHNG (mpexchng.F90:141-206): pack -> point-to-point exchange with the neighbouring ranks -> halo rows.

    transport "torch": torch.distributed P2P (backend "nccl" = RCCL) on tensors packed by ecwam_hip_pack_rows.
    transport "lib":   the library's own exchange (ecwam_hip_halo_start / _finish: RCCL loaded by the library, its own stream) --
                       what a Fortran host calls; the unique id travels through torch.distributed here, MPI_Bcast there.
    transport "host":  host-staged (ecwam_hip_halo_pack_host / _unpack_host) with the segments exchanged through the process
                       group's CPU backend (gloo): an MPI without device pointers, or several ranks sharing one GPU in tests."""

    def __init__(self, dom: decomp.LocalDomain, device, ctx=None, transport: str = "torch"):
        self.dom = dom
        self.ctx = ctx
        self.transport = transport
        if transport not in ("torch", "lib", "host"):
            raise ValueError("halo transport: torch, lib or host")
        self.send_idx = {p: torch.from_numpy(np.ascontiguousarray(ix)).to(device) for p, ix in dom.send.items()}
        self.bufs = {}
        if transport != "torch" and dom.nranks > 1:
            if ctx is None:
                raise ValueError("library halo transports need the HipContext")
            ctx.halo_setup(dom)
            if transport == "lib":
                import torch.distributed as dist
                uid = torch.zeros(128, dtype=torch.uint8)
                if dom.rank == 0:
                    uid = torch.frombuffer(bytearray(ctx.comm_unique_id()), dtype=torch.uint8).clone()
                try:                          # a CPU tensor where the group has a CPU backend (gloo, or "cpu:gloo,cuda:nccl") ...
                    dist.broadcast(uid, src=0)
                except RuntimeError:          # ... a device tensor in a pure RCCL group (the same on every rank)
                    t = uid.to(device)
                    dist.broadcast(t, src=0)
                    uid = t.cpu()
                ctx.comm_init(bytes(uid.numpy().tobytes()))

    def start(self, fl: torch.Tensor) -> list:
        """Pack the rows the neighbours need and post every send / receive; returns the pending requests.  Until `finish`
        the caller must leave the halo rows [n, n+nh) of `fl` alone (the receives land there) -- the owned rows may be read."""
        if self.dom.nranks == 1:
            return []
        import torch.distributed as dist

        if self.transport == "lib":
            self.ctx.halo_start(fl)
            return [None]
        if self.transport == "host":
            rl = int(fl.shape[1] * fl.shape[2])
            sc, rc = self.ctx._halo_send_cnt, self.ctx._halo_recv_cnt
            hs = torch.empty((int(sc.sum()), rl), dtype=fl.dtype).pin_memory()
            hr = torch.empty((int(rc.sum()), rl), dtype=fl.dtype).pin_memory()
            self.ctx.halo_pack_host(fl, hs)
            ops, so, ro = [], 0, 0
            for p, ns, nr in zip(self.ctx._halo_peers, sc, rc):
                if ns:
                    ops.append(dist.P2POp(dist.isend, hs[so:so + int(ns)], p))
                if nr:
                    ops.append(dist.P2POp(dist.irecv, hr[ro:ro + int(nr)], p))
                so += int(ns); ro += int(nr)
            reqs = dist.batch_isend_irecv(ops) if ops else []
            return [("host", reqs, fl, hr, hs)]
        ops = []
        for p, ix in sorted(self.send_idx.items()):
            buf = self.bufs.get((p, int(fl.shape[2])))
            if buf is None or buf.dtype != fl.dtype or buf.shape[1:] != fl.shape[1:]:
                buf = self.bufs[(p, int(fl.shape[2]))] = torch.empty((ix.numel(),) + tuple(fl.shape[1:]), dtype=fl.dtype, device=fl.device)
            if fl.is_cuda and self.ctx is not None and fl.shape[2] == self.ctx.NFRE:
                self.ctx.pack_rows(fl, ix, buf)
            else:
                torch.index_select(fl, 0, ix.long(), out=buf)
            ops.append(dist.P2POp(dist.isend, buf, p))
        for p, (dst0, cnt) in sorted(self.dom.recv.items()):
            ops.append(dist.P2POp(dist.irecv, fl[dst0:dst0 + cnt], p))
        return dist.batch_isend_irecv(ops) if ops else []

    def finish(self, reqs: list) -> None:
        for r in reqs:
            if r is None:
                self.ctx.halo_finish()
            elif isinstance(r, tuple):
                _, rr, fl, hr, _hs = r
                for q in rr:
                    q.wait()
                self.ctx.halo_unpack_host(fl, hr)
            else:
                r.wait()

    def __call__(self, fl: torch.Tensor) -> None:
        self.finish(self.start(fl))


class Wamintgr:
    """Device-resident WAMINTGR for one rank."""

    def __init__(self, cfg: Config, grid, prec: str = "sp", device: int = 0, rank: int = 0, nranks: int = 1,
                 ifrelfmax: int = 0, delpro_lf: float | None = None, weights: str = "otf", strip_width: int = 0,
                 halo_transport: str = "torch", ipropags: int = 2, rotated: dict | None = None):
        # ipropags: the propagation scheme of PROPAG_WAM (propag_wam.F90:217-363).  2 = PROPAGS2, the corner-transport scheme (every path below);
        # 0 = PROPAGS, the first-order upwind scheme with CHECKCFL (HipContext.propags); 1 = PROPAGS1, the first-order scheme on two rotated
        # quadrants (HipContext.propags1), which reads the tables of grid.rotated_tables (rotated=...), whole grid only.
        if ipropags not in (0, 1, 2):
            raise ValueError("ipropags must be 0, 1 or 2")
        if ipropags == 1 and rotated is None:
            raise ValueError("IPROPAGS = 1 needs the rotated tables of grid.rotated_tables (rotated=...)")
        if ipropags != 2 and ifrelfmax > 0:
            raise ValueError(f"ipropags = {ipropags} has no fast-wave sub-steps: PROPAG_WAM sub-steps only in CASE(2) (ifrelfmax must be 0)")
        if ipropags != 2 and weights == "stored":
            raise ValueError(f"ipropags = {ipropags} has no stored weights: the first-order schemes form their weights in every call (weights must be 'otf')")
        if ipropags == 1 and nranks > 1:
            raise ValueError("ipropags = 1 runs on one rank: the halo of the decomposition does not hold the rotated neighbours (nranks must be 1)")
        self.ipropags = ipropags
        # weights: "otf" rebuilds the CTU weights inside PROPAGS2 (no W array, default); "stored" keeps the reference's
        # scheme (CTUW once into W[ij][8][NANG*NFRE_RED], PROPAGS2 streams them).  Bit-identical results.
        self.cfg, self.grid, self.prec = cfg, grid, prec
        self.npdt = np.float32 if prec == "sp" else np.float64
        self.t = Tables(cfg, self.npdt)
        self.ctx = api.HipContext(self.t, device)
        self.dev, self.dtype = self.ctx.device, self.ctx.dtype
        self.dom = decomp.local_domain(grid, rank, nranks)
        self.n, self.nrows = self.dom.n, self.dom.nrows
        self.gd = api.grid_to_device(grid, self.dtype, self.dev, local=self.dom)
        self.halo = HaloExchange(self.dom, self.dev, self.ctx, transport=halo_transport)
        self.interior = self.dom.interior()      # rows [a, b) whose stencil reads no halo row
        NANG, NFRE, NR = cfg.nang, cfg.nfre, cfg.nfre_red
        z = dict(dtype=self.dtype, device=self.dev)
        self.fl1 = torch.zeros((self.nrows, NANG, NFRE), **z)
        self.fl3 = torch.zeros((self.nrows, NANG, NFRE), **z)
        if weights not in ("otf", "stored"):
            raise ValueError("weights must be 'otf' or 'stored'")
        self.weights = weights
        self.w = torch.zeros((self.n, 8, NANG * NR), **z) if weights == "stored" else None
        # optional processing order of the advection (longitude strips); measured neutral on MI355X (the 256 MB Infinity Cache
        # already serves the latitude neighbours), kept as an option
        self.order = None
        self.tiles2d = False
        if strip_width > 0 and self.n > 4 * strip_width:
            self.order = torch.from_numpy(decomp.strip_order(grid, self.dom, strip_width)).to(self.dev)
        elif strip_width < 0:      # 2-D tiles of four latitude rows x four longitudes
            self.order = torch.from_numpy(decomp.tile2d_order(grid, self.dom)).to(self.dev)
            self.tiles2d = True
        if self.order is not None and (int(cfg.irefra) or weights == "stored" or ipropags != 2):
            # the refraction and stored-weight kernels walk the rows in their natural order: a work order (whose padded length would
            # otherwise replace the row range handed to them) does not apply
            self.order, self.tiles2d = None, False
        self.wvprpt = torch.zeros((self.n, api.NWPR, NFRE), **z)
        self.ff = torch.zeros((self.n, api.NFF), **z)
        self.ff_next = None
        self.intf = torch.zeros((self.n, api.NINTF), **z)
        self.mij = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        self.xllws = torch.zeros((self.n, NANG, NFRE), **z)
        self.ctx.implsch_reserve(self.n)        # no allocation inside the time loop
        self.cflfail = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        self.ifrelfmax = ifrelfmax
        self.delpro_lf = delpro_lf
        # fast waves between the sub-steps: compact rows [ij][K][LFP] (a frequency sub-range of the full rows would touch every
        # cache line of the spectra; these are 36/LFP times smaller, for the stencil and for the halo exchange)
        self.g1 = self.g2 = None
        self.gfast_valid = False        # g1 holds the first LFP frequencies of the current FL1 (fast waves + the slow ones that fill its last vector)
        # "compact": sub-steps 1 .. NSTEP_LF-1 compact -> compact BEFORE the full pass, which reads the fast waves' last state from the
        # compact buffer and writes complete rows (round 3); "rows": the full pass first, the further sub-steps write the fast-wave slots
        # of the FL3 rows (round 2; every line of FL3 touched once more per sub-step).  Same bits.
        self._fast_mode = "compact"
        if 0 < ifrelfmax < cfg.nfre_red and weights == "otf" and not int(cfg.irefra):
            lfp = min(cfg.nfre, (ifrelfmax + 3) // 4 * 4)
            self.g1 = torch.zeros((self.nrows, NANG, lfp), **z)
            self.g2 = torch.zeros((self.nrows, NANG, lfp), **z)
        self.weights_ready = False
        self.relabel = False            # set_restart_map: the restart records go out in the order of a global file
        self.halo_events = None         # a list: propag() appends a (before, after) event pair around every wait for a halo exchange
        # refraction (IREFRA = 1 depth, 2 currents, 3 both): per-point THD/S0/U/V/OMDD/CURMASK instead of the reference's
        # THDD/THDC/SDOT and 21 weight arrays; PROPAGS2 rebuilds every weight on the fly
        self.irefra = int(cfg.irefra)
        self.llcflcuroff = True                 # mpuserin.F90:575
        if self.irefra:
            if weights != "otf":
                raise ValueError("IREFRA != 0 runs with on-the-fly weights only")
            self.refr = torch.zeros((self.n, 2 * NANG + 5), **z)
            self.depth_ext = torch.zeros(self.nrows, **z)
            self.u_ext = torch.zeros(self.nrows, **z)
            self.v_ext = torch.zeros(self.nrows, **z)
            self.omosnh2kd_ext = torch.zeros((self.nrows, NFRE), **z)
            self.wavnum_ext = torch.zeros((self.nrows, NFRE), **z)
        if ipropags != 2:
            # DELLAM1_EXT = 1 / DELLAM(KXLT) of the owned and the halo rows, DELLAM = ZDELLO CIRC / 360 (readmdlconf.F90:145, mpdecomp.F90:1428); land slot 0
            T = self.npdt
            dellam = np.asarray(grid.zdello, T) * T(self.t.CIRC) / T(360.0)
            d1 = np.zeros(self.nrows, T)
            d1[:self.dom.nland] = T(1) / dellam[np.asarray(grid.kxlt)[self.dom.ext_global()]]
            self.gd = dict(self.gd, dellam1_ext=torch.from_numpy(d1).to(self.dev))
            self.dot = torch.zeros((self.n, 3 * NANG + 4), **z) if self.irefra else None
        if ipropags == 1:
            self.ctx.set_rotated(api.rotated_to_device(rotated, self.dtype, self.dev))

    @property
    def fast_mode(self) -> str:
        return self._fast_mode

    @fast_mode.setter
    def fast_mode(self, mode: str) -> None:
        if mode not in ("compact", "rows"):
            raise ValueError("fast_mode: 'compact' or 'rows'")
        self._fast_mode = mode
        self.gfast_valid = False      # the rows mode uses g1 as scratch: whatever it holds no longer describes FL1

    # ---- synthetic initial state; identical for every decomposition
    def init_synthetic(self, seed: int = 12345, chunk: int = 65536, currents: bool | None = None, env_on_device: bool = False) -> None:
        """env_on_device (refraction on a decomposed grid): the extended DEPTH / UCUR / VCUR / OMOSNH2KD / WAVNUM / CGROUP rows are not
        assembled on the host from the global fields but by PROENVHALO on the device -- owned rows + one halo exchange (proenvhalo())."""
        g, d, t = self.grid, self.dom, self.t
        self.gfast_valid = False      # new spectra: the compact fast-wave rows are extracted again by the next propag()
        p = syn.point_params(g.nsea, seed=seed)
        self.params = p
        ext = d.ext_global()
        props_ext_cg = np.zeros((self.nrows, self.cfg.nfre), self.npdt)
        if self.irefra:
            om_ext = np.zeros((self.nrows, self.cfg.nfre), self.npdt)
            wn_ext = np.zeros((self.nrows, self.cfg.nfre), self.npdt)
        for s in range(0, ext.size, chunk):
            sl = ext[s:s + chunk]
            pr = syn.depth_props(p["DEPTH"][sl], t, self.npdt)
            props_ext_cg[s:s + sl.size] = pr["CGROUP"]
            if self.irefra:
                om_ext[s:s + sl.size] = pr["OMOSNH2KD"]
                wn_ext[s:s + sl.size] = pr["WAVNUM"]
            own = sl[(sl >= d.lo) & (sl < d.hi)]
            if own.size:
                a, b = s, s + own.size  # owned rows come first in ext
                wv = np.stack([pr[k][: own.size] for k in ("WAVNUM", "CGROUP", "CINV", "XK2CG", "STOKFAC")], 1)
                self.wvprpt[a:b] = torch.from_numpy(wv).to(self.dev)
                ff = np.zeros((own.size, api.NFF), self.npdt)
                ff[:, :14] = syn.forcing(p, own, t, self.npdt)
                ff[:, 14] = pr["EMAXDPT"][: own.size]
                ff[:, 15] = p["DEPTH"][own]
                self.ff[a:b] = torch.from_numpy(ff).to(self.dev)
                fl = syn.jonswap_spectra(t.FR, t.TH, p["FP"][own], p["THETAQ"][own], self.npdt)
                self.fl1[a:b] = torch.from_numpy(fl).to(self.dev)
        land = syn.depth_props(np.array([float(t.BATHYMAX)]), t, self.npdt)      # WVPRPT_LAND (initdpthflds.F90:85-88)
        props_ext_cg[self.dom.nland] = land["CGROUP"][0]
        self.cgroup_ext = torch.from_numpy(props_ext_cg).to(self.dev)
        if self.irefra:
            # PROENVHALO (proenvhalo.F90:69-106): own + halo values, land slot = (WVPRPT_LAND, BATHYMAX, U = V = 0)
            om_ext[self.dom.nland] = land["OMOSNH2KD"][0]
            wn_ext[self.dom.nland] = land["WAVNUM"][0]
            dep = np.full(self.nrows, float(t.BATHYMAX), self.npdt)
            dep[: ext.size] = p["DEPTH"][ext]
            u = np.zeros(self.nrows, self.npdt)
            v = np.zeros(self.nrows, self.npdt)
            if currents if currents is not None else self.irefra >= 2:
                ug, vg = syn.currents(g)
                u[: ext.size] = ug[ext]
                v[: ext.size] = vg[ext]
            if env_on_device:
                n = self.n
                self.proenvhalo(dep[:n], u[:n], v[:n], om_ext[:n])
            else:
                self.set_environment(dep, u, v, om_ext, wn_ext)
        self.fl1[self.dom.nland].zero_()
        self.fl3[self.dom.nland].zero_()

    def set_obstructions(self, obs_global) -> None:
        """LSUBGRID: OBS[nsea][8][NFRE] for ALL sea points (this rank keeps its owned rows); None switches it off.  The
        weights change: the next step re-runs the CTUW checks (and rebuilds W in the stored-weight scheme)."""
        if obs_global is None:
            self.ctx.set_obstructions(None)
        else:
            own = np.ascontiguousarray(np.asarray(obs_global)[self.dom.lo:self.dom.hi], dtype=self.npdt)
            self.ctx.set_obstructions(torch.from_numpy(own).to(self.dev))
        self.weights_ready = False

    def set_environment(self, depth_ext, u_ext, v_ext, omosnh2kd_ext, wavnum_ext) -> None:
        """DEPTH / UCUR / VCUR [nrows] and OMOSNH2KD / WAVNUM [nrows][NFRE] including halo and land rows (what PROENVHALO
        assembles): a new current field makes the next step rebuild the dot terms and re-check the weights (LLUPDTTD /
        LUPDTWGHT, propag_wam.F90:175-236)."""
        for dst, src in ((self.depth_ext, depth_ext), (self.u_ext, u_ext), (self.v_ext, v_ext), (self.omosnh2kd_ext, omosnh2kd_ext),
                         (self.wavnum_ext, wavnum_ext)):
            dst.copy_(torch.as_tensor(np.ascontiguousarray(src, dtype=self.npdt)))
        self.weights_ready = False

    # ---- PROENVHALO (proenvhalo.F90:63-107) on the device
    def proenvhalo_pack(self, depth, ucur, vcur, omosnh2kd) -> torch.Tensor:
        """Owned DEPTH / UCUR / VCUR [n] and OMOSNH2KD [n][NFRE] (device tensors or arrays) + the WAVNUM / CGROUP of the device-resident
        WVPRPT rows -> the owned rows of BUFFER_EXT [nrows][1][3 NFRE + 3]; its halo rows are to be exchanged like spectra."""
        if not self.irefra:
            raise ValueError("PROENVHALO serves the refraction set-up (IREFRA = 1, 2, 3)")
        NFRE = self.cfg.nfre
        if getattr(self, "env_buf", None) is None:
            self.env_buf = torch.zeros((self.nrows - 1, 1, 3 * NFRE + 3), dtype=self.dtype, device=self.dev)
            land = syn.depth_props(np.array([float(self.t.BATHYMAX)]), self.t, self.npdt)      # WVPRPT_LAND (initdpthflds.F90:85-88)
            row = np.concatenate([land["WAVNUM"][0], land["CGROUP"][0], land["OMOSNH2KD"][0], [float(self.t.BATHYMAX), 0.0, 0.0]]).astype(self.npdt)
            self.env_land = torch.from_numpy(row).to(self.dev)
        a = [torch.as_tensor(np.ascontiguousarray(x, dtype=self.npdt)).to(self.dev) if not torch.is_tensor(x) else x.to(self.dev, self.dtype).contiguous()
             for x in (depth, ucur, vcur, omosnh2kd)]
        assert a[0].shape[0] == self.n and tuple(a[3].shape) == (self.n, NFRE)
        self.ctx.proenvhalo_pack(self.n, self.wvprpt, a[3], a[0], a[1], a[2], self.env_buf)
        return self.env_buf

    def proenvhalo_unpack(self) -> None:
        self.ctx.proenvhalo_unpack(self.nrows - 1, self.env_buf, self.env_land, self.wavnum_ext, self.cgroup_ext, self.omosnh2kd_ext,
                                   self.depth_ext, self.u_ext, self.v_ext)
        self.weights_ready = False      # LLUPDTTD / LUPDTWGHT (propag_wam.F90:175-236)

    def proenvhalo(self, depth, ucur, vcur, omosnh2kd) -> None:
        """New depth / currents on a decomposed grid without a host round trip: pack, MPEXCHNG(BUFFER_EXT, 3*NFRE_RED+5, 1, 1), unpack."""
        self.halo(self.proenvhalo_pack(depth, ucur, vcur, omosnh2kd))
        self.proenvhalo_unpack()

    # ---- CTUWUPDT (ctuwupdt.F90:220-256): weights for the (sub-)step structure
    def build_weights(self) -> int:
        c = self.cfg
        self.cflfail.zero_()
        if self.ipropags != 2:
            # PROPDOT with refraction (propag_wam.F90:298-305, 343-350), then CHECKCFL as PROPAGS / PROPAGS1 calls it, without a spectrum written
            if self.irefra:
                self.ctx.propags_dot(self.gd, self.depth_ext, self.u_ext, self.v_ext, self.dot)
            first_order = self.ctx.propags1 if self.ipropags == 1 else self.ctx.propags
            first_order(self.fl1, None, self.gd, self.cgroup_ext, float(c.idelpro), 0, self.n, cflfail=self.cflfail, **self._propags_env())
            self.weights_ready = True
            return int(self.cflfail.sum().item())
        if self.irefra:
            # PROPDOT, then CTUWINI + CTUWDRV per frequency range (checks only: the weights are rebuilt inside PROPAGS2)
            self.ctx.propdot(self.gd, self.depth_ext, self.u_ext, self.v_ext, self.refr)
            a = (self.gd, self.cgroup_ext, self.omosnh2kd_ext, self.wavnum_ext, self.refr, self.cflfail)
            if self.ifrelfmax <= 0:
                self.ctx.ctuw_refra(*a, float(c.idelpro), 1, c.nfre_red, llcflcuroff=self.llcflcuroff, frange=0)
            else:
                self.ctx.ctuw_refra(*a, float(self.delpro_lf), 1, self.ifrelfmax, llcflcuroff=self.llcflcuroff, frange=0)
                if self.ifrelfmax < c.nfre_red:
                    self.ctx.ctuw_refra(*a, float(c.idelpro), self.ifrelfmax + 1, c.nfre_red, llcflcuroff=self.llcflcuroff, frange=1)
            self.weights_ready = True
            return int(self.cflfail.sum().item())
        # weights == "otf": w is None, CTUW only snaps WLAT/WCOR near land and runs the CFL / range checks
        if self.ifrelfmax <= 0:
            self.ctx.ctuw(self.gd, self.cgroup_ext, self.w, self.cflfail, float(c.idelpro), 1, c.nfre_red)
        else:
            self.ctx.ctuw(self.gd, self.cgroup_ext, self.w, self.cflfail, float(self.delpro_lf), 1, self.ifrelfmax)
            if self.ifrelfmax < c.nfre_red:
                self.ctx.ctuw(self.gd, self.cgroup_ext, self.w, self.cflfail, float(c.idelpro), self.ifrelfmax + 1, c.nfre_red)
        self.weights_ready = True
        return int(self.cflfail.sum().item())

    def _propags_env(self) -> dict:
        """what HipContext.propags reads beside CGROUP_EXT at the context's IREFRA"""
        if not self.irefra:
            return {}
        return dict(omosnh2kd_ext=self.omosnh2kd_ext, wavnum_ext=self.wavnum_ext, u_ext=self.u_ext, v_ext=self.v_ext, dot=self.dot)

    def _halo_finish_timed(self, reqs) -> None:
        """halo.finish between two events on the compute stream when the caller collects them (bench.py: what the overlap did not hide)."""
        if self.halo_events is None:
            self.halo.finish(reqs)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.halo.finish(reqs)
        e1.record()
        self.halo_events.append((e0, e1))

    # ---- PROPAG_WAM (propag_wam.F90:166-313), IPROPAGS = 2; (propag_wam.F90:341-362), IPROPAGS = 0; (propag_wam.F90:296-322), IPROPAGS = 1
    def propag(self) -> None:
        if not self.weights_ready:
            nfail = self.build_weights()
            if nfail:
                where = "checkcfl.F90:74-247" if self.ipropags != 2 else "ctuwdrv.F90:128-146"
                raise api.EcwamHipError(f"CFL criterion violated at {nfail} points ({where})")
        c, g = self.cfg, self.gd
        lf = 0 < self.ifrelfmax < c.nfre_red

        def advect_rows(k0, k1, m1, m2, delpro, copy_rest, split=0, src=None):
            if k1 <= k0:
                return
            if self.ipropags != 2:
                first_order = self.ctx.propags1 if self.ipropags == 1 else self.ctx.propags
                first_order(self.fl1, self.fl3, g, self.cgroup_ext, delpro, k0, k1, copy_rest=copy_rest, **self._propags_env())
                return
            tiled = self.tiles2d and (k0, k1) == (0, self.n)
            if tiled:                                        # the range indexes the entries of the (padded) tile order
                k1 = int(self.order.shape[0])
            if src is not None and src is not self.fl1:      # compact fast-wave rows -> fast-wave slots of FL3
                self.ctx.propags2_otf(src, self.fl3, g, self.cgroup_ext, delpro, k0, k1, m1, m2, copy_rest=False, order=self.order, tiles2d=tiled)
                return
            if self.irefra:
                self.ctx.propags2_refra(self.fl1, self.fl3, g, self.cgroup_ext, self.omosnh2kd_ext, self.wavnum_ext, self.refr, delpro, k0,
                                        k1, m1, m2, copy_rest=copy_rest, frange=int(0 < self.ifrelfmax < m1))
            elif self.weights == "stored":
                self.ctx.propags2(self.fl1, self.fl3, g["klon"], g["klat"], g["kcor"], self.w, k0, k1, m1, m2, copy_rest=copy_rest)
            else:
                self.ctx.propags2_otf(self.fl1, self.fl3, g, self.cgroup_ext, delpro, k0, k1, m1, m2, copy_rest=copy_rest,
                                      order=self.order, tiles2d=tiled, ifrelfmax=split, delpro_lf=self.delpro_lf if split else None,
                                      gout=self.g1 if split else None)   # the fast waves also into the compact buffer

        def advect(m1, m2, delpro, copy_rest, split=0, rows=None, src=None):
            k0, k1 = rows if rows is not None else (0, self.n)
            advect_rows(k0, k1, m1, m2, delpro, copy_rest, split, src)

        def exchange_and_advect(passes, src=None):
            """MPEXCHNG + PROPAGS2 (propag_wam.F90:166,247-313) with the exchange hidden behind the interior: post the halo
            exchange, advect the rows that read no halo row, wait, advect the two ends of the band.  src: the buffer whose
            halo rows are exchanged and that the stencil reads (FL1, or the compact fast-wave buffer)."""
            src = self.fl1 if src is None else src
            overlap = self.dom.nranks > 1 and self.order is None
            if not overlap:
                self._halo_finish_timed(self.halo.start(src))
                for a in passes:
                    advect(*a, src=src)
                return
            ia, ib = self.interior
            reqs = self.halo.start(src)
            for a in passes:
                advect(*a, rows=(ia, ib), src=src)
            self._halo_finish_timed(reqs)
            for a in passes:
                advect(*a, rows=(0, ia), src=src)
                advect(*a, rows=(ib, self.n), src=src)

        otf_plain = self.weights == "otf" and not self.irefra
        if lf and otf_plain and self.g1 is not None and self.fast_mode == "compact" and self.order is None:
            self._propag_fast_compact(advect_rows)
            return
        if self.weights == "stored" or self.ifrelfmax <= 0:
            exchange_and_advect([(1, c.nfre_red, float(c.idelpro), True)])      # stored W already carries the per-range time steps
        elif otf_plain:
            # fast and slow waves in ONE pass, each with its own time step (the reference calls PROPAGS2 per range)
            exchange_and_advect([(1, c.nfre_red, float(c.idelpro), True, self.ifrelfmax if lf else c.nfre_red)])
        else:
            passes = [(1, self.ifrelfmax, float(self.delpro_lf), True)]
            if lf:
                passes.append((self.ifrelfmax + 1, c.nfre_red, float(c.idelpro), False))
            exchange_and_advect(passes)
        if lf:
            nstep_lf = int(round(float(c.idelpro) / float(self.delpro_lf)))
            for isub in range(2, nstep_lf + 1):
                # FL1_EXT(:,:,1:IFRELFMAX) <- FL3_EXT ; exchange ; PROPAGS2 on the fast waves only
                if self.g1 is not None:
                    if isub > 2:      # the first pass wrote the compact buffer itself
                        self.ctx.copy_freq_range(self.fl3, self.g1, self.n, 1, self.ifrelfmax)
                    exchange_and_advect([(1, self.ifrelfmax, float(self.delpro_lf), False)], src=self.g1)
                else:
                    self.ctx.copy_freq_range(self.fl3, self.fl1, self.n, 1, self.ifrelfmax)
                    exchange_and_advect([(1, self.ifrelfmax, float(self.delpro_lf), False)])
        self.fl1, self.fl3 = self.fl3, self.fl1
        self.gfast_valid = False      # (the rows mode and the stored-weight / refraction paths overwrite or bypass the compact rows)

    def _propag_fast_compact(self, advect_rows) -> None:
        """PROPAG_WAM with fast-wave sub-steps (propag_wam.F90:247-313) in the order that writes no frequency sub-range into full rows:
        the fast waves do not depend on the slow ones, so their sub-steps 1 .. NSTEP_LF-1 run first, compact -> compact (rows 4.5 x
        shorter at IFRELFMAX = 5, for the stencil and for MPEXCHNG), and the one full pass takes their last state as the input of the last
        sub-step next to the slow waves of FL1 and writes complete FL3 rows (+ the compact copy the next advection step starts from)."""
        c, g = self.cfg, self.gd
        lfm, dlf = self.ifrelfmax, float(self.delpro_lf)
        nstep_lf = int(round(float(c.idelpro) / dlf))
        lfp = int(self.g1.shape[2])
        if not self.gfast_valid:      # (after IMPLSCH or a new initial state) FL1's first LFP frequencies -> compact rows
            self.ctx.copy_freq_range(self.fl1, self.g1, self.n, 1, lfp)
        ga, gb = self.g1, self.g2
        overlap = self.dom.nranks > 1
        ia, ib = self.interior if overlap else (0, self.n)

        def run(passes, exchanges):
            """post the exchanges, advect the rows that read no halo row, wait, advect the two ends of the band"""
            reqs = [self.halo.start(x) for x in exchanges] if self.dom.nranks > 1 else []
            passes(ia, ib)
            for r in reqs:
                self._halo_finish_timed(r)
            if overlap:
                passes(0, ia)
                passes(ib, self.n)

        for _ in range(nstep_lf - 1):
            src, dst = ga, gb
            run(lambda k0, k1: k1 > k0 and self.ctx.propags2_otf(src, dst, g, self.cgroup_ext, dlf, k0, k1, 1, lfm, copy_rest=True), [src])
            ga, gb = gb, ga
        # the full pass: slow waves from FL1 with IDELPRO, the fast waves' last sub-step from the compact rows with DELPRO_LF
        run(lambda k0, k1: k1 > k0 and self.ctx.propags2_otf(self.fl1, self.fl3, g, self.cgroup_ext, float(c.idelpro), k0, k1, 1, c.nfre_red, copy_rest=True,
                                                            ifrelfmax=lfm, delpro_lf=dlf, gin=ga, gout=gb), [ga, self.fl1])      # the short rows first (as WAMINTGR_HIP posts them)
        self.g1, self.g2 = gb, ga
        self.gfast_valid = True
        self.fl1, self.fl3 = self.fl3, self.fl1

    def newwind(self) -> None:
        if self.ff_next is not None:
            self.ctx.newwind(self.ff, self.ff_next)

    def _fast_sink(self) -> bool:
        """IMPLSCH / NOSOURCE leave the fast waves of their result in the compact rows the next advection step starts from."""
        on = self.g1 is not None and self.fast_mode == "compact" and self.order is None
        self.ctx.set_fastwave_copy(self.g1 if on else None)
        return on

    def implsch(self, wam2nemo=None) -> None:
        """(Whoever writes FL1 by another route -- a direct ctx.implsch, a tensor assignment -- resets `gfast_valid`: the compact
        fast-wave rows then no longer describe FL1 and the next propag() extracts them again.)"""
        self.gfast_valid = False
        on = self._fast_sink()
        try:
            self.ctx.implsch(0, self.n, self.fl1, self.wvprpt, self.ff, self.intf, self.mij, self.xllws, wam2nemo=wam2nemo)
        finally:
            if on:
                self.ctx.set_fastwave_copy(None)      # the library keeps no pointer into a buffer this object may swap or free
        self.gfast_valid = on

    def nosource(self) -> None:
        """NO SOURCE TERM CONTRIBUTION (wamintgr.F90:152-160, LLSOURCE = F)."""
        self.gfast_valid = False
        on = self._fast_sink()
        try:
            self.ctx.nosource(0, self.n, self.fl1, self.mij, self.xllws)
        finally:
            if on:
                self.ctx.set_fastwave_copy(None)
        self.gfast_valid = on

    # ---- OUTSTEP0 (outstep0.F90:106-221): the output before the first time step and after a restart
    def wdfluxes(self, wam2nemo=None) -> None:
        """WDFLUXES (wdfluxes.F90): MIJ, XLLWS, the flux members of INTF and the Stokes drift from FL1 as it stands; FL1 and FF are not written."""
        self.ctx.wdfluxes(0, self.n, self.fl1, self.wvprpt, self.ff, self.intf, self.mij, self.xllws, wam2nemo=wam2nemo)

    def outstep0(self, requested=None, llsource: bool = True, second_order: bool = False, wam2nemo=None):
        """WDFLUXES (LLSOURCE = F: MIJ = NFRE, XLLWS = 0), SETICE when LICERUN .AND. LMASKICE .AND. LLSOURCE, then OUTBLOCK of `requested`
        (what outblock() returns; None without a request).  wam2nemo: the WAVE2OCEAN block WDFLUXES needs with LWNEMOCOU."""
        if llsource:
            self.wdfluxes(wam2nemo)
        else:
            self.ctx.nosource(0, self.n, None, self.mij, self.xllws)
        if self.cfg.licerun and self.cfg.lmaskice and llsource:
            self.ctx.setice(0, self.n, self.fl1, self.ff)
            self.gfast_valid = False      # FL1 changed: the compact fast-wave rows no longer describe it
        return None if requested is None else self.outblock(requested, second_order)

    # ---- the 1:1 step as one kernel (round 6): PROPAGS2 inside IMPLSCH's tile load (ecwam_hip_propags2_implsch)
    def fused_available(self) -> bool:
        """The one-kernel step covers this model: a build exists (36 x 36, common IMPLSCH builds) and the advection is IREFRA = 0 with
        on-the-fly weights in the natural row order, with or without sub-grid obstructions; fast-wave sub-steps run on compact rows (the
        last one inside the kernel)."""
        lf = 0 < self.ifrelfmax < self.cfg.nfre_red
        if self.ipropags != 2:      # the one-kernel step advects with PROPAGS2
            return False
        return (self.ctx.fused_supported(fast_waves=lf, obstructions=self.ctx.has_obstructions) and not self.irefra and self.weights == "otf"
                and self.order is None and (not lf or (self.g1 is not None and self.fast_mode == "compact")))

    def step_fused(self, wam2nemo=None, flags: int = 0) -> None:
        """PROPAG_WAM + NEWWIND + IMPLSCH of one step (wamintgr.F90:94-146) with the advection done by the source-term kernel's tile load.
        NEWWIND touches the forcing only and runs first; the halo exchange is posted, the rows that read no halo row are integrated while
        it runs, then the two ends of the band (propag_wam.F90:166, mpexchng.F90)."""
        if not self.weights_ready:
            nfail = self.build_weights()
            if nfail:
                raise api.EcwamHipError(f"CFL criterion violated at {nfail} points (ctuwdrv.F90:128-146)")
        self.newwind()
        c = self.cfg
        lf = 0 < self.ifrelfmax < c.nfre_red
        multi = self.dom.nranks > 1
        ia, ib = self.interior if multi else (0, self.n)
        ga = gb = None
        kw = {}
        if lf:
            # the fast waves' sub-steps 1 .. NSTEP_LF-1 on compact rows (propag_wam.F90:285-313, as _propag_fast_compact); their last sub-step
            # and the slow waves' step are the tile load of the source-term kernel, which also leaves the new fast waves in compact rows
            lfm, dlf = self.ifrelfmax, float(self.delpro_lf)
            nstep_lf = int(round(float(c.idelpro) / dlf))
            lfp = int(self.g1.shape[2])
            if not self.gfast_valid:
                self.ctx.copy_freq_range(self.fl1, self.g1, self.n, 1, lfp)
            ga, gb = self.g1, self.g2
            for _ in range(nstep_lf - 1):
                reqs = self.halo.start(ga) if multi else []
                self.ctx.propags2_otf(ga, gb, self.gd, self.cgroup_ext, dlf, ia, ib, 1, lfm, copy_rest=True)
                if multi:
                    self._halo_finish_timed(reqs)
                    for k0, k1 in ((0, ia), (ib, self.n)):
                        if k1 > k0:
                            self.ctx.propags2_otf(ga, gb, self.gd, self.cgroup_ext, dlf, k0, k1, 1, lfm, copy_rest=True)
                ga, gb = gb, ga
            kw = dict(ifrelfmax=lfm, delpro_lf=dlf, gin=ga)
            self.ctx.set_fastwave_copy(gb)

        def rows(k0, k1):
            if k1 > k0:
                self.ctx.propags2_implsch(self.fl1, self.fl3, self.gd, self.cgroup_ext, float(c.idelpro), k0, k1, self.wvprpt, self.ff, self.intf,
                                          self.mij, self.xllws, 1, c.nfre_red, wam2nemo=wam2nemo, flags=flags, **kw)

        try:
            if multi:
                reqs = ([self.halo.start(ga)] if lf else []) + [self.halo.start(self.fl1)]      # the short rows first
                rows(ia, ib)
                for r in reqs:
                    self._halo_finish_timed(r)
                rows(0, ia)
                rows(ib, self.n)
            else:
                rows(0, self.n)
        finally:
            if lf:
                self.ctx.set_fastwave_copy(None)
        self.fl1, self.fl3 = self.fl3, self.fl1
        if lf:
            self.g1, self.g2 = gb, ga
        self.gfast_valid = lf

    def step(self, advect: bool = True, source: bool = True, llsource: bool = True, fused: bool = False) -> None:
        if fused and advect and source and llsource and self.fused_available():
            self.step_fused()
            return
        if advect:
            self.propag()
        self.newwind()
        if source:
            if llsource:
                self.implsch()
            else:
                self.nosource()

    # ---- restart spectra in the reference's file layout (writefl.F90:110-118, one record per rank)
    def write_restart(self, path: str) -> None:
        from . import restart
        restart.write_fl(path, self.fl1[: self.n].cpu().numpy())

    def read_restart(self, path: str) -> None:
        from . import restart
        a = restart.read_fl(path, self.n, self.cfg.nang, self.cfg.nfre, self.npdt)
        self.fl1[: self.n] = torch.from_numpy(a).to(self.dev)
        self.gfast_valid = False

    def read_restart_device(self, path: str) -> None:
        """read_restart without a transposition on the host: the record goes to the device as the file holds it (NANG * NFRE field vectors
        of n reals, staged in the storage of FL3) and ecwam_hip_getspec_unpack turns it into FL1's rows.  The same bits as read_restart."""
        from . import restart
        nf = self.cfg.nang * self.cfg.nfre
        rec = restart.read_record(path, dtype=self.npdt)
        if rec.size != self.n * nf:
            raise ValueError(f"{path}: record holds {rec.size} reals, expected {self.n * nf} for FL({self.n},{self.cfg.nang},{self.cfg.nfre})")
        if self.n:
            blk = self.fl3.view(-1)[: rec.size].view(nf, self.n)
            blk.copy_(torch.from_numpy(rec).view(nf, self.n))
            self.ctx.getspec_unpack(0, self.n, blk, self.fl1)
        self.gfast_valid = False

    # ---- the start and the end of a run on the device (include/ecwam_hip_restart.h): INITDPTHFLDS, BUILDSTRESS, SAVSTRESS / GETSTRESS, WRITEFL's record
    def initdpthflds(self, depth=None) -> None:
        """INITDPTHFLDS on the device: wvprpt, EMAXDPT and DEPTH of ff, cgroup_ext and, with refraction, omosnh2kd_ext / wavnum_ext from the depths of
        the owned, halo and land rows.  depth: a device vector [nrows] (the land slot is set to BATHYMAX here), or None: the depths the model holds
        (depth_ext with refraction, otherwise DEPTH of ff for the owned rows; then the halo rows keep the cgroup_ext they have)."""
        n, nland = self.n, self.dom.nland
        rows = self.nrows
        if depth is None and not hasattr(self, "cgroup_ext"):
            raise RuntimeError("initdpthflds() without depths recomputes what the model holds: call init_synthetic() first, or pass the depths")
        if not hasattr(self, "cgroup_ext"):      # the depths of every row are given: nothing is kept from an earlier state
            self.cgroup_ext = torch.empty((self.nrows, self.cfg.nfre), dtype=self.dtype, device=self.dev)
        if depth is None:
            if self.irefra:
                depth = self.depth_ext.clone()
            else:
                depth = torch.empty(self.nrows, dtype=self.dtype, device=self.dev)
                depth[:n] = self.ff[:, 15]
                rows = n      # the depths of the halo rows are not kept without refraction
        else:
            depth = torch.as_tensor(depth, dtype=self.dtype, device=self.dev).clone()
        if depth.shape != (self.nrows,):
            raise ValueError(f"initdpthflds: depth is [{self.nrows}] (owned, halo and land rows)")
        depth[nland] = float(self.t.BATHYMAX)
        om, wn = (self.omosnh2kd_ext, self.wavnum_ext) if self.irefra else (None, None)
        self.ctx.depthprpt(0, n, depth, wvprpt=self.wvprpt, wavnum=wn, cgroup=self.cgroup_ext, omosnh2kd=om, ff=self.ff)
        if rows > n:
            self.ctx.depthprpt(n, rows, depth, wavnum=wn, cgroup=self.cgroup_ext, omosnh2kd=om)
        elif nland >= n:
            self.ctx.depthprpt(nland, nland + 1, depth, wavnum=wn, cgroup=self.cgroup_ext, omosnh2kd=om)
        if self.irefra:
            self.depth_ext.copy_(depth)
        self.weights_ready = False

    def buildstress(self, uwave=None, cd=None, zref: float | None = None, nsestart: bool = False, prchar: float = 0.0185, zmiss: float = -999.0) -> None:
        """What GETSTRESS runs for a GRIB or noise start: Z0B = 0, BUILDSTRESS from WSWAVE / WDWAVE of ff and the planes uwave / cd [ncell_in]
        (or None), then the reset of a noise start."""
        self.ctx.buildstress(0, self.n, self.ff, uwave, cd, zref, True, nsestart, prchar, zmiss)

    def set_restart_map(self, ij2newij) -> None:
        """IJ2NEWIJ for the owned rows, 0-based (None removes it): savstress / write_restart_device then write in the global order."""
        if ij2newij is not None and np.asarray(ij2newij).size != self.n:
            raise ValueError(f"restart map: one entry per owned row ({self.n})")
        self.ctx.set_restart_map(ij2newij)
        self.relabel = ij2newij is not None

    def savstress(self) -> torch.Tensor:
        """The sixteen restart fields of SAVSTRESS as a device tensor [16][n], relabelled when a restart map is set."""
        u, v = self._currents()
        rfield = torch.empty((16, self.n), dtype=self.dtype, device=self.dev)
        self.ctx.savstress_pack(0, self.n, self.ff, u, v, rfield, self.relabel)
        return rfield

    def getstress(self, rfield) -> None:
        """GETSTRESS's binary restart (getstress.F90:95-97, 150-165, 188-191): Z0B = 0 is overwritten by field 7; FF_NOW and the currents from rfield
        [16][n]; with refraction the weights are built again."""
        u, v = self._currents()
        r = torch.as_tensor(rfield, dtype=self.dtype, device=self.dev).contiguous()
        self.ctx.getstress_unpack(0, self.n, r, self.ff, u, v, self.relabel)
        if self.irefra:
            self.weights_ready = False

    def write_restart_device(self, path: str, stress_path: str | None = None, dates=None) -> None:
        """write_restart without a transposition on the host: ecwam_hip_savspec_pack forms WRITEFL's record in the storage of FL3 (as
        read_restart_device stages it) and the field vectors are copied back as the file holds them.  stress_path: the LAW file of SAVSTRESS as
        well, with the four dates (CDTPRO, CDATEWO, CDAWIFL, CDATEFL).  The same bytes as write_restart without a restart map."""
        from . import restart
        nf = self.cfg.nang * self.cfg.nfre
        if self.n:
            blk = self.fl3.view(-1)[: self.n * nf].view(nf, self.n)
            self.ctx.savspec_pack(0, self.n, self.fl1, blk, 0, self.relabel)
            rec = blk.cpu().numpy()
        else:
            rec = np.empty(0, self.npdt)
        restart.write_record(path, rec)
        if stress_path is not None:
            restart.write_stress(stress_path, dates if dates is not None else [" " * 14] * 4, self.savstress().cpu().numpy())

    def read_stress_device(self, path: str):
        """The LAW file into FF_NOW and the currents through ecwam_hip_getstress_unpack; returns the four dates."""
        from . import restart
        dates, rfield = restart.read_stress(path, self.n, self.npdt)
        self.getstress(torch.from_numpy(rfield).to(self.dev))
        return dates

    def getspec(self, values, fields=None, unscale: bool = True, nfre_red: int | None = None, opts=None) -> None:
        """GETSPEC's GRIB read on one task (getspec.F90:396-660) from decoded vectors: values is one slab [nfld][NTENCODE] of the fields
        (ifld0, nfld) -- default: from field 0 -- or an iterable of slabs (ifld0, array); arrays on the host are uploaded as they are.  Every
        slab goes through the map of set_grib_map into FL1 (un-scaled unless unscale is off, ZMISS -> EPSMIN); after the last one the tail
        above nfre_red (default NFRE_RED) is filled and SDEPTHLIM applied (getspec_tail)."""
        if getattr(self, "ntencode", None) is None:
            raise RuntimeError("getspec: set_grib_map() first")
        if isinstance(values, (np.ndarray, torch.Tensor)):
            if fields is not None and int(fields[1]) != values.shape[0]:
                raise ValueError("getspec: the slab does not hold the fields named")
            values = [(0 if fields is None else int(fields[0]), values)]
        elif fields is not None:
            raise ValueError("getspec: every slab of an iterable names its own first field")
        for ifld0, a in values:
            if isinstance(a, np.ndarray):
                a = torch.from_numpy(np.ascontiguousarray(a, dtype=self.npdt))
            self.ctx.getspec_values(0, self.n, a.to(self.dev), self.fl1, int(ifld0), unscale, True, opts)
        self.ctx.getspec_tail(0, self.n, self.fl1, self.ff, nfre_red)
        self.gfast_valid = False

    # ---- the start spectra on the device-resident FL1 and FF, over the local rows (csrc/start.hip): a run that does not begin from a restart file
    def delphi(self) -> float:
        """DELPHI, the latitude increment in metres (readmdlconf.F90:136: XDELLA CIRC / 360)"""
        return float(self.grid.xdella) * float(self.t.CIRC) / 360.0

    def cold_start(self, iopti: int = 1, fetch: float = 0.0, fm: float = 0.0, alfa: float = 0.0, gamma: float = 0.0, sa: float = 0.0, sb: float = 0.0,
                   theta: float = 0.0) -> None:
        """preset's cold start (preset.F90:618-638): MSTART on every local row from WSWAVE and WDWAVE of FF.  The defaults are preset's namelist
        defaults (preset.F90:237, 240-246: IOPTI = 1, ALFA = FM = GAMMA = SA = SB = THETA = FETCH = 0): as there, a run sets what its option
        reads.  theta is in degrees (THETAQ = THETA RAD, preset.F90:631), a fetch below 0.1E-5 becomes 0.5 DELPHI (preset.F90:618) and
        FRMAX = FM (preset.F90:619).  IOPTI = 3 is refused."""
        if fetch < 0.1e-5:
            fetch = 0.5 * self.delphi()
        self.ctx.mstart(0, self.n, self.fl1, self.ff, iopti, fetch, fm, theta * float(self.t.RAD), fm, alfa, gamma, sa, sb)
        self.gfast_valid = False

    def noise_start(self) -> None:
        """GETSPEC's LNSESTART (getspec.F90:174-188): FL1 = EPSMIN."""
        self.ctx.getspec_noise(0, self.n, self.fl1)
        self.gfast_valid = False

    def getspec_tail(self, nfre_red: int | None = None) -> None:
        """The end of GETSPEC's GRIB read (getspec.F90:648-659) on the spectra as they stand: the frequencies above nfre_red (default NFRE_RED)
        filled, then SDEPTHLIM."""
        self.ctx.getspec_tail(0, self.n, self.fl1, self.ff, nfre_red)
        self.gfast_valid = False

    def unsetice(self, delphi: float | None = None, restarted: bool = False, small_domain: bool = False) -> None:
        """UNSETICE (unsetice.F90:79-171) as INITMDL calls it on every chunk (initmdl.F90:1024-1037); delphi defaults to the grid's."""
        self.ctx.unsetice(0, self.n, self.fl1, self.ff, self.delphi() if delphi is None else delphi, restarted, small_domain)
        if not (restarted or small_domain):
            self.gfast_valid = False

    # ---- the forcing and coupling seam (csrc/forcing.hip): what WAVEMDL runs immediately before and after WAMODEL, over the local rows.  The host
    # reads the fields (GRIB, IFSTOWAM), keeps the dates and exchanges between tasks; the arithmetic on the state runs where the state lives.
    def set_forcing_map(self, ixy_in=None, ncell_in: int = 0, ixy_out=None, ncell_out: int = 0) -> None:
        """The cells of the local rows, 0-based: ixy_in = (JFROMIJ - NYS) nx + (IFROMIJ - NXS) into the planes of fieldg, ixy_out =
        (NGY - KXLT) NGX + (IXLG - 1) into the outbound grid (mpfldtoifs.F90:348-350)."""
        for m in (ixy_in, ixy_out):
            if m is not None and np.asarray(m).size != self.n:
                raise ValueError("set_forcing_map: one cell per local row")
        self.ctx.set_forcing_map(ixy_in, ncell_in, ixy_out, ncell_out)
        self.ncell_out = int(ncell_out) if ixy_out is not None else 0

    def _currents(self):
        """UCUR, VCUR of the local rows: the refraction's extended rows where there are any, else buffers of their own (zero until getcurr())"""
        if self.irefra:
            return self.u_ext, self.v_ext
        if getattr(self, "ucur", None) is None:
            self.ucur = torch.zeros(self.n, dtype=self.dtype, device=self.dev)
            self.vcur = torch.zeros(self.n, dtype=self.dtype, device=self.dev)
        return self.ucur, self.vcur

    def getwnd(self, fieldg, target: str = "next", nemo=None, **switches) -> None:
        """GETWND (WAMWND + MICEP) from fieldg [13][ncell_in] into FF_NEXT (target="next": NEWWIND hands it to FF_NOW later, as with a wind
        that is read ahead) or into FF_NOW (target="now").  switches: those of HipContext.getwnd.  FF_NEXT starts as a copy of FF_NOW."""
        if target not in ("next", "now"):
            raise ValueError("getwnd: target is 'next' or 'now'")
        if target == "next" and self.ff_next is None:
            self.ff_next = self.ff.clone()
        u, v = self._currents() if switches.get("lcorrel") else (None, None)
        self.ctx.getwnd(0, self.n, fieldg, self.ff_next if target == "next" else self.ff, u, v, nemo, **switches)

    def first_wind(self, fieldg, nemo=None, **switches) -> None:
        """GETFRSTWND (getfrstwnd.F90:113-130): GETWND on FF_NOW, then CDUSTARZ0."""
        self.getwnd(fieldg, "now", nemo, **switches)
        self.ctx.cdustarz0(0, self.n, self.ff)

    def adswstar(self, fieldg) -> None:
        """WAMADSWSTAR: AIRD, WSTAR, USTRA, VSTRA of FF_NOW from fieldg."""
        self.ctx.wamadswstar(0, self.n, fieldg, self.ff)

    def getcurr(self, fieldg=None, nemo=None, mode: int = 0) -> bool:
        """The new currents of GETCURR (mode 0 WAMCUR, 1 NEMO, 2 none).  True if any of them changed (KUPDATE): the caller then rebuilds what
        depends on them (LLUPDTTD: the refraction terms and the advection weights)."""
        u, v = self._currents()
        changed = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.ctx.getcurr(0, self.n, mode, u, v, fieldg, nemo, changed)
        return bool(changed.item())

    def wvblock(self, nwvfields: int | None = None, lwcou2w: bool = False, lwcouhmf: bool = False, lwstokes: bool = False, lwflux: bool = False,
                prchar: float = 0.0185) -> torch.Tensor:
        """WVBLOCK [NWVFIELDS][n] of wavemdl.F90:757-802 from FF_NOW and INTFLDS (OUTBETA with lwcou2w)."""
        need = 1 + int(lwcouhmf) + 2 * int(lwstokes) + 7 * int(lwflux)
        out = torch.empty((need if nwvfields is None else nwvfields, self.n), dtype=self.dtype, device=self.dev)
        self.ctx.wvblock(0, self.n, out, self.ff, self.intf, lwcou2w, lwcouhmf, lwstokes, lwflux, prchar)
        return out

    def fldtoifs(self, wvblock, defval=None, grid=None) -> torch.Tensor:
        """The block-to-grid step of MPFLDTOIFS on one task: grid [NWVFIELDS][ncell_out] (a new one unless given; without defval a given grid
        keeps what the map does not reach)."""
        if grid is None:
            if defval is None:
                raise ValueError("fldtoifs: a new grid needs its defaults")
            grid = torch.empty((wvblock.shape[0], getattr(self, "ncell_out", 0)), dtype=self.dtype, device=self.dev)
        self.ctx.fldtoifs(0, self.n, wvblock, grid, defval)
        return grid

    # ---- the forcing intake (csrc/intake.hip): INIT_FIELDG, IFSTOWAM's FLDINTER and RECVNEMOFIELDS in front of getwnd(), UPDNEMOFIELDS and
    # UPDNEMOSTRESS behind the step.  The exchange with the IFS and with NEMO, IJBLOCK and INITIALINT's once-per-run tables stay with the host.
    def set_fldinter(self, idx, w=None, ngptotg: int = 0, interpol: bool = True) -> None:
        """The per-point table of FLDINTER for the local rows (intake.point_table), after set_forcing_map()."""
        if idx is not None and np.asarray(idx).shape[0] != self.n:
            raise ValueError("set_fldinter: one table row per local row")
        self.ctx.set_fldinter(idx, w, ngptotg, interpol)

    def init_fieldg(self, ncell: int | None = None, roair: float = 1.225, wstar0: float = 0.0) -> torch.Tensor:
        """INIT_FIELDG with LLINIALL on a new (or the resident) fieldg [13][ncell]; ncell defaults to the inbound map's."""
        ncell = int(getattr(self.ctx, "_fmap", (0, 0, 0))[1] if ncell is None else ncell)
        if getattr(self, "fieldg", None) is None or tuple(self.fieldg.shape) != (api.NFIELDG, ncell):
            self.fieldg = torch.empty((api.NFIELDG, ncell), dtype=self.dtype, device=self.dev)
        self.ctx.init_fieldg(self.fieldg, roair, wstar0)
        return self.fieldg

    def ifstowam(self, fields, mask_in=None, **switches) -> torch.Tensor:
        """IFSTOWAM's arithmetic: FLDINTER of fields [nfields][ngptotg] (a cuda tensor of the working precision) into the resident fieldg, which
        init_fieldg() creates on the first call.  switches: those of HipContext.fldinter (laden, lgust, llkc, lwcur, newcurr, roair, wstar0,
        pmiss).  Returns fieldg, what getwnd(), adswstar() and getcurr() take."""
        if getattr(self, "fieldg", None) is None:
            self.init_fieldg(roair=switches.get("roair", 1.225), wstar0=switches.get("wstar0", 0.0))
        self.ctx.fldinter(0, self.n, fields, self.fieldg, mask_in=mask_in, **switches)
        return self.fieldg

    def recvnemofields(self, nemo, nemoibr=None, fieldg=None, **switches) -> None:
        """RECVNEMOFIELDS on the resident FF_NOW, currents and INTFLDS (IBRMEM); nemo float64 [4][n], nemoibr float64 [n].  fieldg defaults to the
        resident one.  switches: lrest, linit, lwcou, lwnemocoucic, lwnemocoucit, lwnemocoucur, lwnemocouibr."""
        u, v = self._currents()
        self.ctx.recvnemofields(0, self.n, nemo, self.ff, u, v, self.intf, getattr(self, "fieldg", None) if fieldg is None else fieldg, nemoibr, **switches)

    def updnemo(self, wam2nemo, nemontau: int, fields: bool = True, stress: bool = True):
        """UPDNEMOFIELDS and UPDNEMOSTRESS on the WAVE2OCEAN block of the step: (fields7 [7][n] or None, stress6 [6][n] or None), float64; with
        stress the six accumulated columns of wam2nemo become 0 (NEMONTAU = 0 is the caller's)."""
        f7 = torch.empty((7, self.n), dtype=torch.float64, device=self.dev) if fields else None
        s6 = torch.empty((6, self.n), dtype=torch.float64, device=self.dev) if stress else None
        self.ctx.updnemo(0, self.n, wam2nemo, nemontau, f7, s6)
        return f7, s6

    # ---- the forcing of a stand-alone run (csrc/readwind.hip): READWIND and CURRENT2WAM behind the GRIB decoder.  The files, eccodes, the dates,
    # LLNOTREAD across calls and READWIND's swamp branch stay with the host; ecwam_amd/readwind.py builds the table of an input grid.
    READWIND_PLANES = {165: "UWND", 33: "UWND", 131: "UWND", 180: "UWND", 166: "VWND", 34: "VWND", 132: "VWND", 181: "VWND", 31: "CICOVER", 139: "CICOVER",
                       92: "CITHICK", 245: "WSWAVE", 249: "WDWAVE", 209: "AIRD", 208: "WSTAR"}

    def set_input_grid(self, slot: int, table) -> None:
        """The table of one input grid (readwind.cell_table's dict: pos, w, kind, nvalues, interpol; None removes it) in slot 0 .. 3."""
        if table is None:
            self.ctx.set_input_grid(slot, None)
            return
        self.ctx.set_input_grid(slot, table["pos"], table["w"], table["kind"], table["nvalues"], table["interpol"])

    def readwind(self, messages, slot: int = 0, roair: float = 1.225, wstar0: float = 0.0, llwswave: bool = False, llwdwave: bool = False, pmiss: float = -999.0):
        """READWIND's loop over the decoded messages of one wind time (readwind.F90:272-494) into the resident fieldg, which init_fieldg() creates on
        the first call: messages = [(paramId, values)] or [(paramId, values, flags)], values the vector as the decoder returned it (host numbers or
        a cuda tensor), all of the input grid in `slot`.  IPARAM = paramId modulo 1000 chooses the plane (READWIND_PLANES); 245 and 249 are skipped
        unless llwswave / llwdwave.  flags (lib.G2W_*) default to LLNONWAVE for a parameter of table 0 and to readwind.dirfld for one of table 140
        (a wave stream).  Raises on a parameter it does not know, on 251, and on a plane filled twice.  Returns (fieldg, icode, iparamci): icode = 2
        for 180 / 181 (stresses), else 3."""
        from . import readwind as rw
        if getattr(self, "fieldg", None) is None:
            self.init_fieldg(roair=roair, wstar0=wstar0)
        vecs, fields, seen, icode, iparamci = [], [], set(), 3, 0
        for msg in messages:
            param, values = int(msg[0]), msg[1]
            iparam = param - (param // 1000) * 1000
            if iparam == 251:
                raise ValueError("readwind: parameter 251 (spectra) is un-scaled and read by getspec_values, not here")
            plane = self.READWIND_PLANES.get(iparam)
            if plane is None:
                raise ValueError(f"readwind: suspicious wind or sea ice field param {iparam}")
            if (iparam == 245 and not llwswave) or (iparam == 249 and not llwdwave):
                continue
            if plane in seen:
                raise ValueError(f"readwind: parameter {iparam} fills {plane}, which a message before it has filled (LLNOTREAD)")
            seen.add(plane)
            if iparam in (180, 181):
                icode = 2
            elif plane in ("UWND", "VWND"):
                icode = 3
            if iparam in (31, 139):
                iparamci = iparam
            wave = param // 1000 == 140
            flags = int(msg[2]) if len(msg) > 2 else ((api._lib.G2W_DIRFLD if rw.dirfld(iparam, True) else 0) if wave else api._lib.G2W_NONWAVE)
            vecs.append(torch.as_tensor(np.asarray(values) if not torch.is_tensor(values) else values, dtype=self.dtype, device=self.dev).reshape(-1))
            fields.append((plane, flags))
        if vecs:
            self.ctx.grib2wgrid(slot, torch.stack(vecs), fields, fieldg=self.fieldg, roair=roair, wstar0=wstar0, pmiss=pmiss)
        return self.fieldg, icode, iparamci

    def current2wam(self, u_values=None, v_values=None, slot: int = 0, wlowest: float = 0.0, zmiss: float = -999.0, flags: int | None = None) -> bool:
        """CURRENT2WAM behind the decoder: the decoded U and V vectors of the input grid in `slot` (either may be None) through GRIB2WGRID and the
        three statements of current2wam.F90:253-259 into the currents of the local rows.  True if any of them changed."""
        given = [(k, v) for k, v in (("u", u_values), ("v", v_values)) if v is not None]
        if not given:
            return False
        vec = torch.stack([torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=self.dtype, device=self.dev).reshape(-1) for _, v in given])
        ncell = int(getattr(self.ctx, "_fmap", (0, 0, 0))[1])
        out = torch.empty((len(given), -(-ncell // 4) * 4), dtype=self.dtype, device=self.dev)      # every FIELD begins a 16-byte piece
        fl = api._lib.G2W_NONWAVE if flags is None else int(flags)
        self.ctx.grib2wgrid(slot, vec, [(api._lib.G2W_FIELD, fl)] * len(given), out=out, pmiss=zmiss)
        planes = {k: out[i, :ncell] for i, (k, _) in enumerate(given)}
        u, v = self._currents()
        changed = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.ctx.current2wam(0, self.n, planes.get("u"), planes.get("v"), u, v, wlowest, zmiss, changed)
        return bool(changed.item())

    # ---- GRIB-ready output (csrc/gribout.hip): OUTSPEC and OUTINT up to the vector VALUES the encoder takes.  eccodes, the dates, the exchange
    # between tasks and FDB stay with the host.
    def set_grib_map(self, ival=None, ntencode: int | None = None, poles=None, lpadpoles: bool = True) -> None:
        """Without arguments: the map of this instance's rows on its own grid (a reduced grid, IRGG = 1, CLDOMAIN = 'g'), from gribout.value_map.
        The poles are padded only where one instance owns the whole grid: a pole mean across a decomposition belongs to the encoding task."""
        if ival is None:
            from . import gribout
            g, d = self.grid, self.dom
            amonop = float(g.amosop) + (g.ngy - 1) * float(g.xdella)
            ival, ntencode, poles = gribout.value_map(g.nlonrgg, g.ixlg[d.lo:d.hi] + 1, g.kxlt[d.lo:d.hi] + 1, g.ngy, 1, amonop, g.amosop, g.xdella, "g",
                                                      lpadpoles and d.nranks == 1)
        if np.asarray(ival).size != self.n:
            raise ValueError("set_grib_map: one value position per local row")
        self.ctx.set_grib_map(ival, ntencode, poles)
        self.ntencode = int(ntencode)

    def outspec(self, fields=None, ice_mask: bool = True, opts=None, values=None, ppmax=None):
        """OUTSPEC on one task: (values [nfld][NTENCODE], ppmax [nfld]) of the fields (ifld0, nfld) -- default all NANG * NFRE_RED -- of FL1.
        ice_mask is LLSOURCE: the mask applies when the run has LICERUN.  values / ppmax: buffers to write into (new ones otherwise)."""
        if getattr(self, "ntencode", None) is None:
            raise RuntimeError("outspec: set_grib_map() first")
        ifld0, nfld = (0, self.cfg.nang * self.cfg.nfre_red) if fields is None else (int(fields[0]), int(fields[1]))
        if values is None:
            values = torch.empty((nfld, self.ntencode), dtype=self.dtype, device=self.dev)
        if ppmax is None:
            ppmax = torch.empty(nfld, dtype=self.dtype, device=self.dev)
        self.ctx.outspec_values(0, self.n, self.fl1, values, self.ff, ifld0, nfld, bool(ice_mask and self.cfg.licerun), opts, ppmax)
        return values, ppmax

    def outint(self, columns, opts=None, values=None) -> torch.Tensor:
        """OUTINT's path for the BOUT that the last outblock() left: values [len(columns)][NTENCODE]; columns are parameter numbers or short
        names of api.OUTBLOCK_PARAMS that the request held."""
        if getattr(self, "ntencode", None) is None:
            raise RuntimeError("outint: set_grib_map() first")
        if getattr(self, "_bout", None) is None:
            raise RuntimeError("outint: outblock() first")
        bout, where = self._bout
        cols = [where[api.OUTBLOCK_NUMBER[c] if isinstance(c, str) else int(c)] for c in columns]
        if values is None:
            values = torch.empty((len(cols), self.ntencode), dtype=self.dtype, device=self.dev)
        self.ctx.grib_values(0, self.n, bout, values, False, columns=cols, opts=opts)
        return values

    # ---- nested grids (wamodel.F90:333-343): the caller sequences step(); bouinpt(); outbc(); outblock() as WAMODEL does.  The tables are the
    # host's (MBOUNF / MBOUNC): ijb = IJARF and ijarc = IJARC as 0-based local rows, ibcl / ibcr = IBFL / IBFR (0 = land, 1 .. NBOINP), bfw = BFW
    def set_nest_input(self, ijb, ibcl, ibcr, bfw) -> None:
        ijb, ibcl, ibcr = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (ijb, ibcl, ibcr))
        bfw = np.ascontiguousarray(bfw, dtype=self.npdt).reshape(-1)
        if not (ijb.size == ibcl.size == ibcr.size == bfw.size):
            raise ValueError("set_nest_input: IJB, IBFL, IBFR and BFW differ in length")
        if ijb.size and (ijb.min() < 0 or ijb.max() >= self.n or np.unique(ijb).size != ijb.size):
            raise ValueError("set_nest_input: IJB must hold distinct rows this instance owns")
        if ijb.size and min(ibcl.min(), ibcr.min()) < 0:
            raise ValueError("set_nest_input: IBFL / IBFR are 0 (land) or 1 .. NBOINP")
        self._nest_in = tuple(torch.from_numpy(a).to(self.dev) for a in (ijb, ibcl, ibcr, bfw))
        self._nest_in_max = int(max(ibcl.max(), ibcr.max())) if ijb.size else 0

    def bouinpt(self, f1, par1, par_out=None) -> None:
        """BOUINPT on self.fl1, on the rows this instance owns: f1 [NBOINP][NFRE][NANG], par1 [NBOINP][3] = EMEAN, THQ, FMEAN (device tensors or arrays)."""
        if getattr(self, "_nest_in", None) is None:
            raise RuntimeError("bouinpt: set_nest_input() first")
        f1, par1 = (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=self.npdt)).to(self.dev) for a in (f1, par1))
        if f1.shape[0] < self._nest_in_max:
            raise ValueError(f"bouinpt: IBFL / IBFR reach {self._nest_in_max}, the boundary records hold {f1.shape[0]} points")
        self.ctx.bouinpt(0, self.n, *self._nest_in, f1, par1, self.fl1, par_out)
        self.gfast_valid = False

    def set_nest_output(self, ijarc) -> None:
        ijarc = np.ascontiguousarray(ijarc, dtype=np.int32).reshape(-1)
        if ijarc.size and (ijarc.min() < 0 or ijarc.max() >= self.n):
            raise ValueError("set_nest_output: IJARC must hold rows this instance owns")
        self._nest_out = torch.from_numpy(ijarc).to(self.dev)

    def outbc(self):
        """OUTBC: (par [NBOUNC][3] = EMEAN, THQ, FMEAN; flpts [NBOUNC][NFRE][NANG]) of the points of set_nest_output()."""
        if getattr(self, "_nest_out", None) is None:
            raise RuntimeError("outbc: set_nest_output() first")
        nbc = self._nest_out.shape[0]
        par = torch.zeros((nbc, 3), dtype=self.dtype, device=self.dev)
        flpts = torch.zeros((nbc, self.cfg.nfre, self.cfg.nang), dtype=self.dtype, device=self.dev)
        self.ctx.outbc(self._nest_out, self.fl1, flpts, par)
        return par, flpts

    # ---- OUTBS subset on the device: [n][5] = swh, mean direction, mean period, EM, peak period; norms = OUTWNORM (avg, min, max, count)
    def outbs(self) -> torch.Tensor:
        out = torch.zeros((self.n, 5), dtype=self.dtype, device=self.dev)
        self.ctx.outbs(0, self.n, self.fl1, out)
        return out

    # ---- wind sea / swell and mean-period / spread parameters on the device: [n][15], columns api.OUTBS_SEP_FIELDS
    def outbs_sepwisw(self, small_domain: bool = False) -> torch.Tensor:
        out = torch.zeros((self.n, len(api.OUTBS_SEP_FIELDS)), dtype=self.dtype, device=self.dev)
        self.ctx.outbs_sepwisw(0, self.n, self.fl1, self.xllws, self.wvprpt, self.ff, out, small_domain=small_domain)
        return out

    # ---- swell-train partitioning on the device (SEPWISW with LLPARTITION = T): [n][24], columns api.OUTBS_PART_FIELDS
    def outbs_partition(self) -> torch.Tensor:
        out = torch.zeros((self.n, len(api.OUTBS_PART_FIELDS)), dtype=self.dtype, device=self.dev)
        self.ctx.outbs_partition(0, self.n, self.fl1, self.xllws, self.mij, self.wvprpt, self.ff, out)
        return out

    # ---- extreme-wave parameters on the device (KURTOSIS, W_MAXH): [n][13], columns api.OUTBS_EXT_FIELDS; kurtosis_only: columns 9-12 stay 0
    def outbs_extremes(self, kurtosis_only: bool = False) -> torch.Tensor:
        out = torch.zeros((self.n, len(api.OUTBS_EXT_FIELDS)), dtype=self.dtype, device=self.dev)
        self.ctx.outbs_extremes(0, self.n, self.fl1, self.wvprpt, self.ff, out, kurtosis_only=kurtosis_only)
        return out

    # ---- the parameters of OUTBLOCK's output spectrum FL2ND on the device: [n][8], columns api.OUTBS_ABS_FIELDS.  With IREFRA = 2 / 3 the
    # spectrum is first taken to the absolute frame with the model's currents (INTPOL); store_spectrum: also returns FL2ND [n][NANG][NFRE]
    def outbs_absolute(self, store_spectrum: bool = False):
        out = torch.zeros((self.n, len(api.OUTBS_ABS_FIELDS)), dtype=self.dtype, device=self.dev)
        fl2nd = torch.empty((self.n, self.cfg.nang, self.cfg.nfre), dtype=self.dtype, device=self.dev) if store_spectrum else None
        u, v = (self.u_ext, self.v_ext) if self.irefra >= 2 else (None, None)
        self.ctx.outbs_absolute(0, self.n, self.fl1, self.wvprpt, u, v, self.ff, out, fl2nd=fl2nd)
        return (out, fl2nd) if store_spectrum else out

    # ---- the same with LSECONDORDER = T (CAL_SECOND_ORDER_SPEC between INTPOL and the ice reshaping).  The tables of SECONDHH_GEN /
    # TABLES_2ND are built and uploaded on first use.  depth [n]: DEPTH of the points; default: the model's own depth with refraction,
    # else BATHYMAX = 999 m everywhere (the deep-water set-up this driver runs without IREFRA)
    def outbs_second_order(self, store_spectrum: bool = False, depth=None, sig: float = 1.0):
        if not self.ctx.has_second_order:
            from .second_order import SecondOrderTables
            self.second_order_tables = SecondOrderTables(self.t)
            self.ctx.set_second_order(self.second_order_tables)
        if depth is None:
            depth = self.depth_ext if self.irefra else torch.full((self.n,), 999.0, dtype=self.dtype, device=self.dev)
        out = torch.zeros((self.n, len(api.OUTBS_ABS_FIELDS)), dtype=self.dtype, device=self.dev)
        fl2nd = torch.empty((self.n, self.cfg.nang, self.cfg.nfre), dtype=self.dtype, device=self.dev) if store_spectrum else None
        u, v = (self.u_ext, self.v_ext) if self.irefra >= 2 else (None, None)
        self.ctx.outbs_second_order(0, self.n, self.fl1, self.wvprpt, depth, u, v, self.ff, out, fl2nd=fl2nd, sig=sig)
        return (out, fl2nd) if store_spectrum else out

    # ---- drag, normalised wave stress, mean square slopes, ice strain, energy flux, crest-trough correlation and the band heights on the
    # device: [n][8 + nband], columns api.OUTBS_INT_FIELDS then the bands of ctx.integral_bands (set on first use: the reference's seven and
    # XKMSS_CUTOFF = XK_GC(NWAV_GC)).  fl2nd: the spectrum outbs_absolute / outbs_second_order(store_spectrum=True) returned, for the bands
    def outbs_integrals(self, fl2nd=None, groups: int = api.OUTBS_INT_ALL) -> torch.Tensor:
        if self.ctx.integral_bands is None:
            self.ctx.set_outbs_integrals()
        out = torch.zeros((self.n, len(api.OUTBS_INT_FIELDS) + len(self.ctx.integral_bands)), dtype=self.dtype, device=self.dev)
        self.ctx.outbs_integrals(0, self.n, self.fl1, self.wvprpt, self.ff, out, fl2nd=fl2nd, groups=groups)
        return out

    # ---- OUTBLOCK as one device call: (bout [n][NIPRMOUT], {parameter: column}).  requested: parameter numbers of api.OUTBLOCK_PARAMS; default:
    # every parameter whose inputs this driver holds -- no altimeter data (17-19), no NEMO fields (58-61), currents (37, 38) only with IREFRA = 2 / 3.
    # ITOBOUT as mpcrtbl.F90:473-502 builds it; every point is deep enough (IODP = 1); IBRMEM is the input slot of the INTF rows.  The integrals'
    # bands and the second-order tables are set on first use, as in outbs_integrals() / outbs_second_order().
    def outblock(self, requested=None, second_order: bool = False):
        cur = self.irefra >= 2
        if requested is None:
            requested = [p[0] for p in api.OUTBLOCK_PARAMS if not (17 <= p[0] <= 19 or 58 <= p[0] <= 61 or (p[0] in (37, 38) and not cur))]
        requested = sorted(set(int(r) for r in requested))
        if self.ctx.integral_bands is None:
            self.ctx.set_outbs_integrals()
        if second_order and not self.ctx.has_second_order:
            from .second_order import SecondOrderTables
            self.second_order_tables = SecondOrderTables(self.t)
            self.ctx.set_second_order(self.second_order_tables)
        key = (tuple(requested), bool(second_order))
        if getattr(self, "_outblock_key", None) != key:
            self._outblock_key = None
            self._outblock_columns = self.ctx.set_outblock(requested, second_order=second_order)
            self._outblock_key = key
        bout = torch.zeros((self.n, len(requested)), dtype=self.dtype, device=self.dev)
        u, v = (self.u_ext, self.v_ext) if cur else (None, None)
        iodp = torch.ones(self.n, dtype=torch.int32, device=self.dev)
        self.ctx.outblock(0, self.n, bout, fl1=self.fl1, xllws=self.xllws, mij=self.mij, wvprpt=self.wvprpt, ff=self.ff, intf=self.intf, ucur=u, vcur=v,
                          iodp=iodp, ibrmem=self.intf[:, 15].contiguous())
        self._bout = (bout, dict(self._outblock_columns))      # outint() takes its columns from here
        return bout, dict(self._outblock_columns)

    def swh_norm(self):
        return self.ctx.outwnorm(self.outbs(), 0, self.n)

    # ---- diagnostics used by tests/bench (swh = 4 sqrt(EM), outbs.F90 / semean.F90)
    def swh(self) -> torch.Tensor:
        dfim = torch.from_numpy(np.asarray(self.t.DFIM, dtype=np.float64)).to(self.dev)
        e = (self.fl1[: self.n].double().sum(1) * dfim).sum(1)
        return 4.0 * torch.sqrt(e)
