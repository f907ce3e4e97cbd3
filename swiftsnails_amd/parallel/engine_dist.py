"""N>1 device set-up of the round engine (parallel/engine.py): the receive
buffers, the server-merge slots and the xGMI mailbox layout handed to the C++
RoundEngine.  Split out of PSEngine as a mixin; see engine.py for the round
itself."""
from __future__ import annotations

import os

import torch


def _hip():
    from .._native import hip

    return hip()


def _ptr(t) -> int:
    """Device pointer of a tensor, 0 for an absent one."""
    return t.data_ptr() if t is not None else 0


class _ServerSlot:
    """Device buffers of one ring slot's server-side merge (N>1, GPU)."""

    def __init__(self, rows: int, P: int, dev, snapshot: bool):
        u32 = torch.int32
        self.cnt = torch.zeros(P + 1, dtype=u32, device=dev)  # + the arrival counter
        self.bstart = torch.empty(P + 1, dtype=u32, device=dev)
        self.ubase = torch.empty(P, dtype=u32, device=dev)
        self.unum = torch.empty(P, dtype=u32, device=dev)
        self.ucount = torch.zeros(1, dtype=torch.int64, device=dev)
        self.pj = torch.empty(rows, dtype=u32, device=dev)
        self.luid = torch.empty(rows, dtype=u32, device=dev)
        self.bkeys = torch.empty(rows, dtype=torch.int64, device=dev)
        self.slots = torch.empty(rows, dtype=torch.int64, device=dev)
        self.snap = torch.empty((rows, 2), dtype=torch.float32, device=dev) if snapshot else None
        self.snap_valid = False

    def view(self, P: int):
        return (self.bkeys.data_ptr(), self.bstart.data_ptr(), self.unum.data_ptr(),
                self.ubase.data_ptr(), P)


class DeviceSetup:
    """PSEngine mixin: the N>1 GPU buffers (``_init_dist_gpu``) and the
    collective agreement on a small int64 tensor (``_agree``)."""

    # ------------------------------------------------------------ N>1 (GPU)
    def _init_dist_gpu(self) -> None:
        """Receive buffers and server-merge slots of the N>1 device path.
        Every rank lays its buckets out as a call of ``max_keys`` keys (the
        common layout the servers merge) and sends each destination its
        per-bucket runs with the keys."""
        N, cap, d, dev, h = self.world, self.max_keys, self.dim, self.device, _hip()
        for dd in self.dedupers:
            dd.lay_n = cap
        self.Pd = h.bd_buckets(cap, N, self.dedupers[0].ndest) // N
        # record exchange: a server bucket is N runs of records sized for one
        # LDS table together (bdedup.hip bd_target), no sub-buckets
        self.sub = 1 if self.records else h.srv_sub_buckets(
            N, cap, self.dedupers[0].ndest & ~h.bd_record_layout_bit())
        self.Ps = self.Pd * self.sub
        # sub > 1: every source groups its runs by the servers' sub-bucket
        # and sends the offsets with them (the server reads exact ranges)
        for dd in self.dedupers:
            dd.split_for_servers(self.sub)
            if self.records:
                dd.enable_records()
        Psub = self.Pd * self.sub if self.sub > 1 else 0
        # every rank's max_keys must agree (it fixes Pd)
        mk = torch.tensor([cap, -cap], dtype=torch.int64, device=dev)
        self._agree(mk)
        if int(mk[0]) != cap or int(-mk[1]) != cap:
            raise ValueError("PSEngine: max_keys differs across ranks (the N>1 bucket layout "
                             "is a function of it)")
        rows = N * cap
        self.rvals = torch.zeros((rows, d), dtype=torch.float32, device=dev)
        # xGMI: one slot past the ring (index `depth`) for the read-only
        # lookup's rounds (PSEngine.lookup), with its own deduper
        NS = self.depth + (1 if self.xg else 0)
        self.lookup_slot = self.depth if self.xg else None
        if self.xg:
            from ..ops.dedup import Deduper

            lk = Deduper(self.max_keys, nranks=N, frag_map=self.dedupers[0].frag_map.cpu(),
                         gdim=d, device=dev, record_layout=self.records)
            lk.lay_n = cap
            lk.split_for_servers(self.sub)
            lk.need_ukeys = True
            self._lk_dd = lk
            # the receive buffers are the arena's mailboxes: keys + the bucket
            # runs (bases, sizes) per source, rows back, gradients
            Pd, xg = self.Pd, self.xg
            xg.setup({"keys": (NS, [cap * 8, Pd * 4, Pd * 4] + ([Psub * 4] if Psub else [])),
                      "vals": (NS, [cap * 4 * d]), "grads": (NS, [cap * 4 * d])})
            # (the C++ engine reads the keys, runs and gradient rows in place)
            self.uvals = [xg.region("vals", 0, q, torch.float32, d) for q in range(NS)]
        else:
            self.rkeys = [torch.empty(rows, dtype=torch.int64, device=dev)] * self.depth
            meta = [torch.zeros(2 * N * self.Pd, dtype=torch.int32, device=dev)
                    for _ in range(self.depth)]
            self.rmeta = [(m[:N * self.Pd], m[N * self.Pd:]) for m in meta]
            self.rsub = [torch.zeros(N * Psub, dtype=torch.int32, device=dev) if Psub else None
                         for _ in range(self.depth)]
            self.rgrads = [torch.empty((rows, d), dtype=torch.float32, device=dev)] * self.depth
        # region buckets (claimed server pulls, table.hip k_pull_claim_bk):
        # every shard has the same region count (same capacity), agreed with
        # the worker-only ranks, whose buckets must follow the same regions
        own = getattr(self.table, "rbits", 0) if self.table is not None else None
        rb = torch.tensor([99 if own is None else own, 1 if own is None else -own],
                          dtype=torch.int64, device=dev)
        self._agree(rb)
        lo, hi = int(rb[0]), -int(rb[1])
        self.srv_rbits = lo if (lo == hi and 0 < lo < 99 and
                                os.environ.get("SS_CLAIM", "1") != "0") else 0
        self.claim = bool(self.srv_rbits and self.xg)
        if self.claim:
            for dd in self.dedupers:
                dd.rbits = self.srv_rbits
        # the server half of every round (keys in, merge, lookup, rows out;
        # gradients in, merge + update) on its own highest-priority stream: a
        # slow compute on this rank's main stream does not hold up the rows
        # every peer waits for (SS_SERVER_STREAM=0: on the main stream)
        # auto (default): only when every rank has its own device — ranks
        # sharing one GPU (one-GPU rehearsals) oversubscribe its hardware
        # queues with a third stream per process (8 ranks: 21.3 vs 8.35 ms
        # per 8-rank step; 4 ranks 4.62 vs 4.41)
        ss_env = os.environ.get("SS_SERVER_STREAM", "auto")
        if self.table is not None and self.xg is not None and \
                (ss_env == "1" or (ss_env == "auto" and not self.shared_device)):
            other = self._streams_of
            lo_prio, hi_prio = torch.cuda.Stream.priority_range()
            self.server_stream = (
                (other.server_stream or other._server_stream_off) if other is not None else None) or \
                torch.cuda.Stream(device=dev, priority=min(lo_prio, hi_prio))
        self.srv_ahead = os.environ.get("SS_SRV_AHEAD", "1") != "0"
        if self.table is not None:
            self.svals = torch.empty((rows, d), dtype=torch.float32, device=dev)
            self.sgrad = torch.empty((rows, d), dtype=torch.float32, device=dev)
            self.srv_err = torch.zeros(1, dtype=torch.int32, device=dev)
            snap_ok = bool(getattr(self.table, "snapshot_ok", False))
            self.srv = [_ServerSlot(rows, self.Ps, dev, snap_ok and q < self.depth)
                        for q in range(NS)]
        # record exchange: the rows of this rank's own records are written by
        # its own server into a cached buffer per ring slot (not the uncached
        # vals arena, which only peers need), and their gradients are read by
        # the server merge straight from the worker's per-sample gradient
        # through spj — never written out per occurrence (SS_REC_OCC=arena:
        # both through the arena, as the peers' records)
        if (self.records and self.table is not None and
                self.server_ranks == list(range(N)) and
                os.environ.get("SS_REC_OCC", "own") == "own" and
                os.environ.get("SS_XGMI_SELF", "1") != "0"):
            self.own_vals = [torch.empty((cap, d), dtype=torch.float32, device=dev)
                             for _ in range(self.depth)]
        if self.xg:
            # raw pointers in the C++ engine: these tensors (and the server
            # slots') stay attributes of this engine, which owns it, for its life
            self.native.set_xgmi(
                arenas=[[self.xg.arena_of(c, q) for c in ("keys", "vals", "grads")]
                        for q in range(NS)],
                keys=[sum((list(self.xg.layout("keys", p, q)) for p in range(4 if Psub else 3)),
                          []) for q in range(NS)],
                vals=[list(self.xg.layout("vals", 0, q)) for q in range(NS)],
                grads=[list(self.xg.layout("grads", 0, q)) for q in range(NS)],
                nranks=N, rank=self.rank, Pd=self.Pd, sub=self.sub, cap=cap, dim=d,
                bpp=self.xg.bpp, timeout_s=self.xg.timeout_s, rvals=self.rvals.data_ptr(),
                srv_err=_ptr(self.srv_err), svals=_ptr(self.svals), sgrad=_ptr(self.sgrad))
            # a closed transport frees its arenas: the engine forgets them first
            self.xg._close_hooks.append(self.native.clear_xgmi)
            for q, S in enumerate(self.srv or ()):
                self.native.set_server_slot(
                    q, cnt=S.cnt.data_ptr(), bstart=S.bstart.data_ptr(), ubase=S.ubase.data_ptr(),
                    unum=S.unum.data_ptr(), pj=S.pj.data_ptr(), luid=S.luid.data_ptr(),
                    bkeys=S.bkeys.data_ptr(), slots=S.slots.data_ptr(),
                    ucount=S.ucount.data_ptr(), snap=_ptr(S.snap))

    def _agree(self, t: torch.Tensor) -> None:
        """min-all-reduce of a small int64 tensor over the data transport."""
        if self.world == 1:
            return
        self.t.allreduce_(t, "min")
        if self.gpu:
            torch.cuda.current_stream(self.device).synchronize()
