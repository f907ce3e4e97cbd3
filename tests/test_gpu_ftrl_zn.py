"""``ftrl_zn`` — FTRL-Proximal in 16-byte ``[z | n | key]`` slots — on every
path it pulls, updates, trains, checkpoints and evicts through, against the
fp64 oracle of ``_ftrl_zn_oracle.py`` (table level) and ``_lr_oracle.LROracle(
"ftrl", l1=0.3)`` from zero rows (engine level), within their derived bounds.

Table level (in the pytest process): a 4096-slot table (one region) and a
2^17-slot table (2^7 regions); ~700 keys hold the planted (z, n) rows.
Engine level: sparse LR on ``_lr_oracle``'s files, each case in a spawned
process of its own (as ``test_gpu_opt_oracle.py`` runs its engine cases).

Each case prints its largest |device - oracle| / bound as ``MARGIN ...``
(reported in ``docs/TESTING.md``, not tuned).
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _ftrl_zn_oracle as Z
import _lr_oracle as L
import _opt_oracle as O
from _mp import collect, file_init, in_child, init_gloo

pytestmark = pytest.mark.gpu

NKEYS, STEPS = 700, 6
CAPS = [4096, 1 << 17]
SETTINGS = Z.settings()
WHICH = sorted(SETTINGS)


@pytest.fixture(scope="module")
def dev():
    from swiftsnails_amd._native import hip

    hip()  # loud failure if the extension is missing on a GPU box
    return torch.device("cuda", 0)


def _optimizer(h, kind="ftrl_zn"):
    from swiftsnails_amd.ops.optim import Optimizer

    return Optimizer(**{**h.kwargs(), "kind": kind})


def _keys(n=NKEYS, seed=3):
    return np.unique(np.random.default_rng(seed).integers(1, 1 << 40, size=n, dtype=np.int64))


def _absent(n=64, seed=11):
    return np.unique(np.random.default_rng(seed).integers(1 << 41, 1 << 42, size=n, dtype=np.int64))


def _table(h, dev, cap, keys=None, rows=None):
    """An ftrl_zn table of rule ``h`` holding ``keys`` with the planted
    (z, n) rows first: (table, keys, device keys, slots, rows)."""
    from swiftsnails_amd.ops.optim import InitConfig
    from swiftsnails_amd.ops.table import HbmTable

    t = HbmTable(1, cap, optimizer=_optimizer(h), init=InitConfig("zero"), device=dev)
    assert t.width == 2 and t.stride == 16 and t.snapshot_ok and t.zn and t.dt.zn == 1
    assert (t.rbits >= 6) == (cap >= 1 << 16)
    k = _keys() if keys is None else keys
    rows = Z.table_rows(h, len(k)) if rows is None else rows
    kt = torch.from_numpy(k).to(dev)
    t.assign(kt, torch.from_numpy(rows))
    slots = t.lookup_slots(kt)
    torch.cuda.synchronize()
    t.check()
    assert t.size() == len(k) and int(slots.min()) >= 0
    return t, k, kt, slots, rows


def _rows(t, k):
    d = t.to_dict(with_state=True)
    assert len(d) == len(k)
    return np.stack([d[int(x)] for x in k.view(np.uint64)])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _hold_pull(h, rows, got, label):
    """``got`` is w(z, n) of ``rows`` within the bound, +0.0 exactly where
    |z| <= l1; returns the largest ratio."""
    got = np.asarray(got, np.float32).reshape(-1)
    r, ref = Z.pull_ratio(h, rows, got)
    i = int(r.argmax())
    assert r[i] <= 1.0, (label, float(r[i]), i, float(got[i]), float(ref.v[i]), rows[i])
    zero = np.abs(rows[:, 0]) <= np.float32(h.l1)
    assert (_bits(got[zero]) == 0).all(), (label, "w = 0 must be +0.0")
    return float(r.max())


def _hold_step(h, before, g, after, label):
    r = Z.rows_ratio(Z.step(h, before[:, 0], before[:, 1], np.asarray(g).reshape(-1)), after)
    i = np.unravel_index(int(r.argmax()), r.shape)
    assert r[i] <= 1.0, (label, float(r[i]), i, after[i[0]], before[i[0]], float(np.ravel(g)[i[0]]))
    return float(r.max())


# ------------------------------------------------------------------ table
def test_table_refuses_what_the_rule_cannot_hold(dev):
    from swiftsnails_amd.ops.optim import InitConfig, Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    opt = Optimizer("ftrl_zn", l1=0.3)
    for kw, word in ((dict(dim=1, init=InitConfig("uniform", 0.01)), "InitConfig"),
                     (dict(dim=1, init=InitConfig("zero", state_init=0.1)), "state_init"),
                     (dict(dim=2, init=InitConfig("zero")), "dim"),
                     (dict(dim=1, init=InitConfig("zero"), row_dtype="bf16"), "row_dtype"),
                     (dict(dim=1, init=InitConfig("zero"), lane_group=4), "lane group")):
        with pytest.raises(ValueError, match=word):
            HbmTable(capacity=4096, optimizer=opt, device=dev, **kw)
    t = HbmTable(1, 4096, optimizer=opt, init=InitConfig("zero"), device=dev)
    with pytest.raises(ValueError):
        t.set_optimizer(Optimizer("adagrad"))          # the same width, another meaning
    with pytest.raises(ValueError):
        HbmTable(1, 4096, optimizer=Optimizer("adagrad"), device=dev).set_optimizer(opt)
    v = t.version
    t.set_optimizer(Optimizer("ftrl_zn", l1=0.5, ftrl_alpha=0.1))
    assert t.version > v and t.opt.l1 == 0.5 and t.dt.zn == 1
    p = HbmTable.plan(10**6, 1, opt)
    assert p["stride"] == 16 and p["width"] == 2
    # [w | z | n] beside it: 24 bytes of key and row in a 32-byte slot
    assert HbmTable.plan(10**6, 1, Optimizer("ftrl"))["stride"] == 32


def _bucket_view(dev, t, keys_np):
    """A bucketed dedup of ``keys_np`` (each once) laid out for ``t``: the
    view ``pull_buckets`` takes and the keys in unique-id order."""
    from swiftsnails_amd.ops.dedup import Deduper

    dd = Deduper(len(keys_np), device=dev)
    dd.rbits = t.rbits
    res = dd(torch.from_numpy(keys_np).to(dev))
    torch.cuda.synchronize()
    n = int(res.ucount[0].item())
    assert n == len(keys_np)
    uk = res.ukeys[:n].cpu().numpy()
    assert np.array_equal(np.sort(uk), np.sort(keys_np))
    return dd, dd.bucket_view(len(keys_np)), uk


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("which", WHICH)
def test_pull_returns_the_derived_weight(dev, which, cap):
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.parallel.engine import PSEngine

    h = SETTINGS[which]
    t, k, kt, slots, rows = _table(h, dev, cap)
    ab = _absent()
    mix = np.concatenate([k, ab])
    perm = np.random.default_rng(5).permutation(len(mix))
    mix, present = mix[perm], (perm < len(k))
    mrows = np.zeros((len(mix), 2), np.float32)
    mrows[present] = rows[perm[present]]
    mt = torch.from_numpy(mix).to(dev)
    worst = {}
    # read-only forms: 0 and no insert for absent keys
    v, s = t.pull(mt, insert=False)
    torch.cuda.synchronize()
    worst["pull(insert=False)"] = _hold_pull(h, mrows, v.cpu().numpy(), "insert=False")
    assert (s.cpu().numpy()[~present] == -1).all() and (_bits(v.cpu().numpy()[~present]) == 0).all()
    eng = PSEngine(t, None, max_keys=len(mix), dim=1, device=dev)
    lv = eng.lookup(mt)
    torch.cuda.synchronize()
    worst["lookup"] = _hold_pull(h, mrows, lv.cpu().numpy(), "lookup")
    assert (_bits(lv.cpu().numpy()[~present]) == 0).all()
    t.check()
    assert t.size() == len(k)
    # pull of the keys the table holds
    v, s = t.pull(kt)
    torch.cuda.synchronize()
    worst["pull"] = _hold_pull(h, rows, v.cpu().numpy(), "pull")
    assert torch.equal(s, slots) and t.size() == len(k)
    # the bucketed forms, at compact unique ids
    dd, view, uk = _bucket_view(dev, t, k)
    urows = rows[np.searchsorted(k, uk)]
    uslots = slots.cpu().numpy()[np.searchsorted(k, uk)]
    n, st = len(uk), torch.cuda.current_stream().cuda_stream
    for snap_on, s32 in ((False, False), (True, False), (True, True)):
        out = torch.full((n, 1), -7.0, device=dev)
        sl = torch.full((n,), -7, dtype=torch.int64, device=dev)
        snap = torch.full((n, 2), -7.0, device=dev) if snap_on else None
        if s32:
            hip().pull_unique_bk(t.dt, *view, sl.data_ptr(), out.data_ptr(), t._init_native,
                                 t.size_ctr.data_ptr(), t.err.data_ptr(), t.G, st,
                                 snap.data_ptr(), 1)
        else:
            t.pull_buckets(view, out, sl, snap=snap)
        torch.cuda.synchronize()
        label = f"pull_buckets snap={snap_on} slot32={s32}"
        worst[label] = _hold_pull(h, urows, out.cpu().numpy(), label)
        got = sl.view(torch.int32)[:n].cpu().numpy() if s32 else sl.cpu().numpy()
        np.testing.assert_array_equal(got, uslots)
        if snap_on:   # the snapshot keeps the row's (z, n) bits
            np.testing.assert_array_equal(_bits(snap.cpu().numpy()), _bits(urows))
    if t.rbits:   # the claimed pull: rows, the occurrence fill and the snapshot
        out = torch.full((n,), -7.0, device=dev)
        occ = torch.full((n,), -7.0, device=dev)
        sl = torch.full((n,), -7, dtype=torch.int32, device=dev)
        snap = torch.full((n, 2), -7.0, device=dev)
        before = t.storage.clone()
        hip().pull_claim_bk(t.dt, *view, sl.data_ptr(), out.data_ptr(), snap.data_ptr(),
                            t._init_native, t.size_ctr.data_ptr(), t.err.data_ptr(), st,
                            dd.luid.data_ptr(), occ.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(before, t.storage)
        worst["claimed pull"] = _hold_pull(h, urows, out.cpu().numpy(), "claimed pull")
        np.testing.assert_array_equal(sl.cpu().numpy(), uslots)
        np.testing.assert_array_equal(_bits(snap.cpu().numpy()), _bits(urows))
        # occ[p] = the pulled value of the key at bucket position p
        sc = dd.scratch.cpu().numpy()
        _, o_bs, o_un, o_ub = hip().bd_offsets(n, 1, 1)
        P = view[4]
        bstart, unum, ub0 = sc[o_bs:o_bs + P + 1], sc[o_un:o_un + P], sc[o_ub:o_ub + P]
        luid = dd.luid.cpu().numpy().view(np.uint32)
        want = np.zeros(n, np.float32)
        on = out.cpu().numpy()
        for b in range(P):
            p0, p1 = bstart[b], bstart[b + 1]
            want[p0:p1] = on[ub0[b] + luid[p0:p1].astype(np.int64)]
        np.testing.assert_array_equal(_bits(occ.cpu().numpy()), _bits(want))
    t.check()
    assert t.size() == len(k)
    # absent keys pulled with insert: (0, 0) rows, w = +0, the size grows
    at = torch.from_numpy(ab).to(dev)
    v, s = t.pull(at)
    torch.cuda.synchronize()
    t.check()
    assert (_bits(v.cpu().numpy()) == 0).all() and int(s.min()) >= 0
    assert t.size() == len(k) + len(ab)
    d = t.to_dict(with_state=True)
    assert all((_bits(d[int(x)]) == 0).all() for x in ab.view(np.uint64))
    np.testing.assert_array_equal(_bits(_rows(t, np.concatenate([k, ab]))[:len(k)]), _bits(rows))
    w = t.to_dict()
    got = np.array([w[int(x)][0] for x in k.view(np.uint64)], np.float32)
    worst["to_dict"] = _hold_pull(h, rows, got, "to_dict")
    print(f"MARGIN pull {which} cap {cap}: " + "  ".join(f"{a} {b:.3f}" for a, b in worst.items()))


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("which", WHICH)
def test_push_slots_matches_fp64_oracle(dev, which, cap):
    """Six steps of ``push_slots`` plain and with ``snap=`` (the blind store
    from the rows a pull would have snapshotted): each the oracle's step from
    the table's own rows, and each other's bits."""
    h = SETTINGS[which]
    ta, k, kt, sa, rows = _table(h, dev, cap)
    tb, _, _, sb, _ = _table(h, dev, cap)
    before = _rows(ta, k)
    np.testing.assert_array_equal(_bits(before), _bits(rows))
    worst = 0.0
    for s in range(STEPS):
        g = Z.table_grads(h, len(k), s)
        gt = torch.from_numpy(g).to(dev)
        ta.push_slots(sa, gt)
        tb.push_slots(sb, gt, snap=torch.from_numpy(before.copy()).to(dev))
        ta.next_round()
        tb.next_round()
        torch.cuda.synchronize()
        a, b = _rows(ta, k), _rows(tb, k)
        worst = max(worst, _hold_step(h, before, g, a, ("row-read", s)),
                    _hold_step(h, before, g, b, ("snapshot", s)))
        np.testing.assert_array_equal(_bits(a), _bits(b))
        before = a
    # the pulled weight of the trained rows
    v, _ = ta.pull(kt, insert=False)
    torch.cuda.synchronize()
    wp = _hold_pull(h, before, v.cpu().numpy(), "pull after training")
    print(f"MARGIN push_slots {which} cap {cap}: step {worst:.4f}  pull {wp:.4f}")


def _hold_one_step(h, before, g, after, sel, label):
    assert sel.any() and not sel.all()
    np.testing.assert_array_equal(_bits(after[~sel]), _bits(before[~sel]))
    return _hold_step(h, before[sel], g[sel], after[sel], label)


@pytest.mark.parametrize("which", WHICH)
def test_negative_slots_are_skipped(dev, which):
    h = SETTINGS[which]
    t, k, kt, slots, before = _table(h, dev, CAPS[0])
    sel = (np.arange(len(k)) % 3 != 1)
    sl = slots.clone()
    sl[torch.from_numpy(~sel).to(dev)] = -1
    g = Z.table_grads(h, len(k), 0)
    t.push_slots(sl, torch.from_numpy(g).to(dev))
    torch.cuda.synchronize()
    w = _hold_one_step(h, before, g, _rows(t, k), sel, "slots -1")
    print(f"MARGIN -1 slots {which}: {w:.3f}")


@pytest.mark.parametrize("which", WHICH)
def test_three_segments_with_gaps(dev, which):
    h = SETTINGS[which]
    t, k, kt, slots, before = _table(h, dev, CAPS[0])
    n = len(k)
    offs, cnts = [5, 200, 450], [100, 131, n - 450 - 7]
    sel = np.zeros(n, bool)
    for o, c in zip(offs, cnts):
        assert o + c <= n
        sel[o:o + c] = True
    g = Z.table_grads(h, n, 0)
    t.push_slots(slots, torch.from_numpy(g).to(dev), segs=t.segs(offs, cnts))
    torch.cuda.synchronize()
    w = _hold_one_step(h, before, g, _rows(t, k), sel, "segments")
    print(f"MARGIN segments {which}: {w:.3f}")


# ------------------------------------------------- the server merge's update
def _merge_layout(dev, nsrc, Pd=3, per=400, seed=7):
    """Received keys of ``nsrc`` sources in ``Pd`` server buckets (a key's
    bucket is a function of the key; bucket 0 holds keys of source 0 only, so
    with two sources both branches of the merge run), and the server dedup's
    tables over them — the shape of ``test_gpu_opt_oracle.py``'s server-merge
    test, built here so that this module stands on its own."""
    from swiftsnails_amd._native import hip

    h = hip()
    rng = np.random.default_rng(seed)
    pool = _keys(900, seed)
    bucket = (pool % 1000003) % Pd
    cap = per * Pd
    rows = nsrc * cap
    rkeys = np.full(rows, -1, np.int64)
    rbase, rnum = np.zeros((nsrc, Pd), np.int32), np.zeros((nsrc, Pd), np.int32)
    for s in range(nsrc):
        mine = rng.choice(pool, 500, replace=False)   # unique within a source
        at = 0
        for b in range(Pd):
            kb = mine[bucket[np.searchsorted(pool, mine)] == b]
            if b == 0 and s > 0:
                kb = kb[:0]
            kb = kb[:per]
            rkeys[s * cap + at:s * cap + at + len(kb)] = kb
            rbase[s, b], rnum[s, b] = at, len(kb)
            at += len(kb)
    i32 = dict(dtype=torch.int32, device=dev)
    P = Pd
    Lm = {"P": P, "rows": rows,
          "rkeys": torch.from_numpy(rkeys).to(dev),
          "meta": torch.from_numpy(np.concatenate([rbase.ravel(), rnum.ravel()])).to(dev),
          "cnt": torch.zeros(P + 1, **i32), "bstart": torch.empty(P + 1, **i32),
          "ubase": torch.empty(P, **i32), "unum": torch.empty(P, **i32),
          "pj": torch.empty(rows, **i32), "luid": torch.empty(rows, **i32),
          "bkeys": torch.empty(rows, dtype=torch.int64, device=dev),
          "uc": torch.zeros(1, dtype=torch.int64, device=dev), "err": torch.zeros(1, **i32)}
    st = torch.cuda.current_stream().cuda_stream
    h.srv_dedup(Lm["rkeys"].data_ptr(), Lm["meta"].data_ptr(),
                Lm["meta"].data_ptr() + 4 * nsrc * Pd, cap, nsrc, Pd, 1, 0, Lm["cnt"].data_ptr(),
                Lm["bstart"].data_ptr(), Lm["pj"].data_ptr(), Lm["luid"].data_ptr(),
                Lm["bkeys"].data_ptr(), Lm["ubase"].data_ptr(), Lm["unum"].data_ptr(),
                Lm["uc"].data_ptr(), Lm["err"].data_ptr(), st)
    torch.cuda.synchronize()
    pos = np.concatenate([np.arange(s * cap + rbase[s, b], s * cap + rbase[s, b] + rnum[s, b])
                          for s in range(nsrc) for b in range(Pd)])
    Lm["pos"], Lm["rk"] = pos, rkeys[pos]
    assert int(Lm["err"].item()) == 0
    assert int(Lm["uc"].item()) == len(np.unique(Lm["rk"]))
    assert int(Lm["bstart"][P].item()) == len(pos)
    occ = np.diff(Lm["bstart"].cpu().numpy())
    un = Lm["unum"].cpu().numpy()
    if nsrc == 1:
        assert (occ == un).all()                      # every bucket: np == nu
    else:
        assert occ[0] == un[0] and (occ[1:] > un[1:]).all()   # both branches
    return Lm


@pytest.mark.parametrize("nsrc", [2, 1])
@pytest.mark.parametrize("form", ["rmw", "snap", "store16"])
@pytest.mark.parametrize("which", ["reg", "l1"])
def test_server_merge_fused_update(dev, which, form, nsrc):
    """``launch_bd_reduce_p`` on the layout ``test_gpu_opt_oracle.py``'s
    server-merge test uses: the received gradients of a key are summed and go
    straight into the rule — read-modify-write of the row (``rmw``), from the
    pull's snapshot with an 8-byte store (``snap``), and from the snapshot
    with 4-byte slots and the whole ``[z | n | key]`` slot in one 16-byte
    store (``store16``, the claimed pull's commit).  A third of the keys are
    new to the table: the pull creates them as (0, 0)."""
    from swiftsnails_amd._native import hip

    h = SETTINGS[which]
    Lm = _merge_layout(dev, nsrc)
    P, rows_n = Lm["P"], Lm["rows"]
    distinct = np.unique(Lm["rk"])
    old = np.arange(len(distinct)) % 3 != 2
    t, k, kt, _, rows0 = _table(h, dev, CAPS[1], keys=distinct[old])
    before = np.zeros((len(distinct), 2), np.float32)
    before[old] = rows0
    view = (Lm["bkeys"].data_ptr(), Lm["bstart"].data_ptr(), Lm["unum"].data_ptr(),
            Lm["ubase"].data_ptr(), P)
    svals = torch.empty((rows_n, 1), device=dev)
    sslots = torch.full((rows_n,), -1, dtype=torch.int64, device=dev)
    snap = None if form == "rmw" else torch.zeros((rows_n, 2), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    if form == "store16":
        hip().pull_unique_bk(t.dt, *view, sslots.data_ptr(), svals.data_ptr(), t._init_native,
                             t.size_ctr.data_ptr(), t.err.data_ptr(), t.G, st, snap.data_ptr(), 1)
    else:
        t.pull_buckets(view, svals, sslots, snap=snap)
    torch.cuda.synchronize()
    t.check()
    assert t.size() == len(distinct)
    np.testing.assert_array_equal(_bits(_rows(t, distinct)), _bits(before))
    gn = np.zeros((rows_n, 1), np.float32)
    m = len(Lm["pos"])
    gn[Lm["pos"]] = np.where((np.arange(m) % 2 == 0)[:, None], Z.table_grads(h, m, 0),
                             Z.table_grads(h, m, 1))
    g = torch.from_numpy(gn).to(dev)
    hip().srv_merge(P, Lm["bstart"].data_ptr(), Lm["ubase"].data_ptr(), Lm["unum"].data_ptr(),
                    Lm["pj"].data_ptr(), Lm["luid"].data_ptr(), g.data_ptr(), 0, 1, t.dt,
                    sslots.data_ptr(), 0 if snap is None else snap.data_ptr(), t.opt.native(), st,
                    int(form == "store16"), Lm["bkeys"].data_ptr() if form == "store16" else 0)
    torch.cuda.synchronize()
    t.check()
    assert t.size() == len(distinct)
    after = _rows(t, distinct)
    idx = np.searchsorted(distinct, Lm["rk"])
    Gs, A = np.zeros(len(distinct)), np.zeros(len(distinct))
    np.add.at(Gs, idx, gn[Lm["pos"], 0].astype(np.float64))
    np.add.at(A, idx, np.abs(gn[Lm["pos"], 0]).astype(np.float64))
    cnt = np.bincount(idx, minlength=len(distinct))
    assert cnt.min() >= 1 and (cnt.max() == 2) == (nsrc == 2)
    eG = np.where(cnt > 1, cnt, 0) * O.U * A   # one received row: no sum, exact
    parts = Z.step(h, before[:, 0], before[:, 1], O.N(Gs, eG))
    r = Z.rows_ratio(parts, after)
    i = np.unravel_index(int(r.argmax()), r.shape)
    print(f"MARGIN server merge {which} {form} sources {nsrc}: {float(r.max()):.3f}")
    assert r[i] <= 1.0, (form, nsrc, float(r[i]), i, after[i[0]], before[i[0]])
    # the response rows the pull filled: the derived weight per distinct key
    bs, ub, un = (Lm[x].cpu().numpy() for x in ("bstart", "ubase", "unum"))
    bk = Lm["bkeys"].cpu().numpy()
    sv = svals.cpu().numpy()[:, 0]
    for b in range(P):
        kb = bk[bs[b]:bs[b] + un[b]]
        _hold_pull(h, before[np.searchsorted(distinct, kb)], sv[ub[b]:ub[b] + un[b]],
                   ("server pull", b))


# ---------------------------------------------------- checkpoints, eviction
def _trained(h, dev, cap, steps=3):
    """A table whose keys were created by a pull and trained ``steps`` steps."""
    from swiftsnails_amd.ops.optim import InitConfig
    from swiftsnails_amd.ops.table import HbmTable

    t = HbmTable(1, cap, optimizer=_optimizer(h), init=InitConfig("zero"), device=dev)
    k = _keys()
    kt = torch.from_numpy(k).to(dev)
    _, slots = t.pull(kt)
    for s in range(steps):
        t.push_slots(slots, torch.from_numpy(Z.table_grads(h, len(k), s + 1)).to(dev))
        t.next_round()
    torch.cuda.synchronize()
    t.check()
    return t, k, kt


def test_checkpoint_round_trips(dev, tmp_path):
    from swiftsnails_amd.ops.optim import InitConfig, Optimizer, pull_reference
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.utils import checkpoint as C

    h = SETTINGS["l1"]
    t, k, kt = _trained(h, dev, CAPS[1])
    rows = _rows(t, k)
    w = pull_reference(t.opt, rows, 1)
    assert (w == 0).any() and (w != 0).any()
    np.testing.assert_array_equal(_bits(t.weights(rows)), _bits(w))

    def fresh(kind="ftrl_zn"):
        return HbmTable(1, CAPS[1], optimizer=_optimizer(h, kind), init=InitConfig("zero"),
                        device=dev)

    # binary and with-state text: the (z, n) bits
    pb, ps, pw = (str(tmp_path / n) for n in ("t.bin", "t.state.txt", "t.w.txt"))
    assert C.save_binary(t, pb) == len(k)
    assert C._header(pb)[0]["row_rule"] == "zn"
    assert C.save_text(t, ps, with_state=True) == len(k)
    for load, p in ((C.load_binary, pb), (C.load_text, ps)):
        u = fresh()
        assert load(u, p) == len(k)
        np.testing.assert_array_equal(_bits(_rows(u, k)), _bits(rows))
    assert u.opt.step == 0       # the text loader keeps no round count; the binary one does
    # text without state: key<TAB>w, the model — at the writer's precision
    assert C.save_text(t, pw) == len(k)
    got = {}
    with open(pw) as f:
        for line in f:
            a, b = line.rstrip("\n").split("\t")
            assert "|" not in b and len(b.split()) == 1
            got[int(a)] = float(b)
    assert set(got) == set(int(x) for x in k.view(np.uint64))
    gw = np.array([got[int(x)] for x in k.view(np.uint64)])
    np.testing.assert_allclose(gw, w[:, 0].astype(np.float64), rtol=1e-8, atol=0)
    np.testing.assert_array_equal(gw.astype(np.float32), w[:, 0])   # 9 digits: the fp32 bits
    with pytest.raises(ValueError, match="ftrl_zn"):
        C.load_text(fresh(), pw)
    # an AdaGrad (w, h) file has the same width: refused both ways
    ada = HbmTable(1, CAPS[1], optimizer=Optimizer("adagrad"), init=InitConfig("zero"),
                   device=dev)
    ada.assign(kt, torch.from_numpy(rows))
    pa = str(tmp_path / "ada.bin")
    C.save_binary(ada, pa)
    assert "row_rule" not in C._header(pa)[0]
    with pytest.raises(ValueError, match="checkpoint rows"):
        C.load_binary(fresh(), pa)
    with pytest.raises(ValueError, match="checkpoint rows"):
        C.load_binary(HbmTable(1, CAPS[1], optimizer=Optimizer("adagrad"),
                               init=InitConfig("zero"), device=dev), pb)


@pytest.mark.parametrize("cap", CAPS)
def test_evict_on_the_derived_weight(dev, cap):
    from swiftsnails_amd.ops.optim import EvictRule, pull_reference

    h = SETTINGS["l1"]
    t, k, kt = _trained(h, dev, cap)
    rows = _rows(t, k)
    w = pull_reference(t.opt, rows, 1)[:, 0]
    dead = w == 0
    assert dead.any() and not dead.all()
    assert (rows[dead, 0] != 0).any()     # z itself is not 0: the rule reads the derived w
    assert t.evict(EvictRule(w_below=0.0)) == int(dead.sum())
    t.check()
    assert t.size() == int((~dead).sum())
    np.testing.assert_array_equal(_bits(_rows(t, k[~dead])), _bits(rows[~dead]))
    v, s = t.pull(kt, insert=False)
    torch.cuda.synchronize()
    assert (s.cpu().numpy()[dead] == -1).all() and (s.cpu().numpy()[~dead] >= 0).all()
    # acc_below reads n
    k2, rows2 = k[~dead], rows[~dead]
    cut = float(np.median(rows2[:, 1]))
    low = rows2[:, 1] <= np.float32(cut)
    assert low.any() and not low.all()
    assert t.evict(EvictRule(acc_below=cut)) == int(low.sum())
    np.testing.assert_array_equal(_bits(_rows(t, k2[~low])), _bits(rows2[~low]))


# ------------------------------------------------------------- engine level
LR_CAP = 1 << 20
KNOBS = ("SS_CLAIM", "SS_SLOT32", "SS_TABLE_REGIONS", "SS_ENGINE_GENERAL", "SS_DEDUP",
         "SS_REC_OCC", "SS_REC_GROUP", "SS_SRV_STAGE", "SS_XGMI_SELF", "SS_SERVER_STREAM",
         "SS_STALENESS", "SS_ENGINE_DEPTH", "SS_TABLE_G", "SS_TABLE_PREFILL", "SS_TABLE_LAYOUT")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ftrl_zn")
    return {n: L.dataset(n).write(d / f"{n}.libsvm") for n in ("binary32", "valued64")}


@functools.lru_cache(maxsize=None)
def _reference(name, world=1, steps=L.OPT_STEPS):
    """``LROracle("ftrl", l1=0.3)`` from zero rows: the fp64 reference of a
    data set, computed once per process and shared read-only."""
    from swiftsnails_amd.ops.optim import InitConfig

    orc = L.LROracle("ftrl", l1=Z.L1)
    orc.init = InitConfig("zero")
    for k, x, y in L.batches(name, world, steps):
        orc.step(k, x, y)
    r = orc.result()
    for a in (r.keys, r.w, r.h, r.tol_w, r.tol_h, r.h2, r.tol_h2):
        a.setflags(write=False)
    return r


def _lr_table(dev):
    from swiftsnails_amd.models.sparse_lr import make_lr_table
    from swiftsnails_amd.ops.optim import InitConfig, Optimizer

    opt = Optimizer("ftrl_zn", lr=L.LR["ftrl"], eps=L.EPS, l1=Z.L1)
    return make_lr_table(2_000_003, 1, opt, device=dev, capacity=LR_CAP, init=InitConfig("zero"))


def _lr_source(path, name, batch, dev, rank=0, world=1, steps=L.OPT_STEPS):
    from swiftsnails_amd.utils.dataio import FileCtrSource

    ds = L.dataset(name)
    src = FileCtrSource(path, batch_size=batch, num_fields=L.F, rank=rank, world=world,
                        resident="hbm", device=dev)
    k = torch.empty(batch * L.F, dtype=torch.int64, device=dev)
    x = torch.empty(batch * L.F, dtype=torch.float32, device=dev)
    y = torch.empty(batch, dtype=torch.float32, device=dev)
    for t in range(steps):
        src.generate(t, rank, world, k, y, xval=x if src.has_values else None)
        ek, ex, ey = ds.batch(t, batch, rank, world)
        assert np.array_equal(k.cpu().numpy().view(np.uint64), ek.reshape(-1)), t
        assert np.array_equal(y.cpu().numpy(), ey), t
        if src.has_values:
            assert np.array_equal(x.cpu().numpy(), ex.reshape(-1)), t
    return src


def _lr_train(w, table, first=0, steps=L.OPT_STEPS):
    losses = []
    for s in range(first, first + steps):
        assert table.opt.step == s
        w.step()
        losses.append(w.mean_loss())
    torch.cuda.synchronize()
    return losses


def _lr_export(table):
    ks, rs = [], []
    for k, r in table.export():
        ks.append(k.numpy())
        rs.append(r.numpy())
    return np.concatenate(ks).view(np.uint64), np.concatenate(rs)


def _lr_check(label, ref, losses, keys, rows, w, world=1, first=0):
    """The assertions of every engine case (those of ``test_gpu_opt_oracle.py``
    for FTRL with L1); prints the margin before asserting it."""
    assert ref.ill == 0  # the oracle's precondition, from the oracle alone
    for r, l in enumerate(losses):
        np.testing.assert_allclose(l, ref.mean_losses(world)[first:, r], rtol=1e-4)
    assert L.EMPTY not in keys and len(np.unique(keys)) == len(keys)  # one slot per key
    assert np.array_equal(np.sort(keys), ref.keys), (len(keys), len(ref.keys))
    assert rows.shape[1] == 2 and w.shape == (len(keys),)
    rw, rh, out = L.ratios(ref, keys, w, rows[:, 0], rows[:, 1])   # w, z = h, n = h2
    print(f"MARGIN {label}: max |engine - oracle| / tol  w {rw:.3f}  state {rh:.3f}")
    assert rw <= 1 and rh <= 1, (label, rw, rh, out)
    order = np.argsort(keys)
    near = L.ftrl_near_threshold(ref, Z.L1)
    assert near.mean() < 0.01
    dz, oz = w[order] == 0, ref.w == 0
    assert oz.any() and not oz.all()
    assert np.array_equal(dz[~near], oz[~near]), int((dz != oz)[~near].sum())
    assert not np.signbit(w[w == 0]).any()


def _engine(path, dev, table, name, file, steps=L.OPT_STEPS):
    from swiftsnails_amd.models.sparse_lr import SparseLRWorker
    from swiftsnails_amd.parallel.engine import PSEngine
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    tr = None if path == "fast" else XgmiTransport(0, 1, dev, None, timeout_s=30)
    eng = PSEngine(table, tr, max_keys=L.B * L.F, dim=1, device=dev,
                   exchange="records" if path.startswith("records") else "unique")
    w = SparseLRWorker(eng, _lr_source(file, name, L.B, dev, steps=steps))
    assert (w.xval is not None) == (name == "valued64")
    return tr, eng, w


def _body_world1(path, name, file, knob):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    if path.startswith("records"):
        os.environ["SS_REC_OCC"] = path.split("_")[1]
    if knob:
        os.environ[knob] = "0"
    table = _lr_table(dev)
    tr, eng, w = _engine(path, dev, table, name, file)
    # the feature is on: 16-byte slots through the machinery AdaGrad rows use
    assert table.stride == 16 and table.snapshot_ok
    assert (table.rbits > 0) == (knob != "SS_TABLE_REGIONS")
    if path == "fast":
        assert eng.fast1 and eng.snapshot and eng.depth == 8
        assert eng.slot32 == (knob != "SS_SLOT32")
        assert eng.claim == (knob is None)
    else:
        assert not eng.fast1 and eng.xg is not None
        assert eng.records == path.startswith("records")
        assert eng._server_update_kind() == "scalar"
        if path == "records_own":
            assert eng.own_merge()
    losses = _lr_train(w, table)
    eng.check()
    table.check()
    keys, rows = _lr_export(table)
    if tr is not None:
        tr.close()
    _lr_check(f"{path} {name} {knob or ''}", _reference(name), [losses], keys, rows,
              table.weights(rows)[:, 0])


CASES1 = [(p, n, None) for n in ("binary32", "valued64")
          for p in ("fast", "unique", "records_own", "records_arena")] + \
         [("fast", "binary32", k) for k in ("SS_CLAIM", "SS_SLOT32", "SS_TABLE_REGIONS")]


@pytest.mark.parametrize("path,name,knob", CASES1)
def test_lr_matches_fp64_oracle(files, path, name, knob):
    in_child(_body_world1, path, name, files[name], knob, always=True)


def _rank(rank, world, file, name, init, q):
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    for k in KNOBS:
        os.environ.pop(k, None)
    init_gloo(init, rank, world)
    try:
        from swiftsnails_amd.models.sparse_lr import SparseLRWorker
        from swiftsnails_amd.parallel.engine import PSEngine
        from swiftsnails_amd.parallel.transport import TorchDistTransport
        from swiftsnails_amd.parallel.xgmi import XgmiTransport

        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        tr = XgmiTransport(rank, world, dev, dist.distributed_c10d._get_default_store(),
                           aux=TorchDistTransport(), timeout_s=30)
        table = _lr_table(dev)
        eng = PSEngine(table, tr, max_keys=L.B // world * L.F, dim=1, device=dev,
                       exchange="unique")
        w = SparseLRWorker(eng, _lr_source(file, name, L.B // world, dev, rank, world),
                           rank=rank, world=world)
        assert not eng.records and w.xval is not None
        assert eng._server_update_kind() == "scalar"
        losses = _lr_train(w, table)
        eng.check()
        table.check()
        keys, rows = _lr_export(table)
        # the collective read-only lookup (k_lookup_bk): every key of the
        # model from whichever shard holds it, 0 and no insert for absent keys
        ref = _reference(name, world)
        ask = np.concatenate([ref.keys.view(np.int64), _absent(32)])
        lv = eng.lookup(torch.from_numpy(ask).to(dev)).cpu().numpy()[:, 0]
        torch.cuda.synchronize()
        table.check()
        assert table.size() == len(keys)
        assert lv.shape == (len(ask),)
        q.put((rank, losses, keys, rows, table.weights(rows)[:, 0], lv))
    finally:
        dist.destroy_process_group()


def test_lr_world2_matches_fp64_oracle(files):
    """Two ranks on one GPU over the xGMI unique exchange: one update per key
    on the sum of both ranks' gradients, the servers' merge fused with it."""
    world, name = 2, "valued64"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = file_init()
    procs = [ctx.Process(target=_rank, args=(r, world, files[name], name, init, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    assert all(len(x[2]) > 0 for x in res)  # both shards hold keys
    ref = _reference(name, world)
    keys = np.concatenate([x[2] for x in res])
    w = np.concatenate([x[4] for x in res])
    _lr_check(f"world2 unique {name}", ref, [x[1] for x in res], keys,
              np.concatenate([x[3] for x in res]), w, world=world)
    urows = np.concatenate([x[3] for x in res])[np.argsort(keys)]
    worst = 0.0
    for x in res:   # the lookup is the pull's transform of the shards' rows
        worst = max(worst, _hold_pull(SETTINGS["l1"], urows, x[5][:len(keys)], ("lookup", x[0])))
        assert (_bits(x[5][len(keys):]) == 0).all()
    print(f"MARGIN world2 lookup {name}: {worst:.3f}")


def _body_resume(name, file, ckpt):
    """Train OPT_STEPS steps, save the binary checkpoint, load it into a new
    table and train 2 more: the oracle's trajectory of OPT_STEPS + 2 steps."""
    from swiftsnails_amd.utils import checkpoint as C

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["SS_PULL_AHEAD"] = "0"
    n0, n1 = L.OPT_STEPS, L.OPT_STEPS + 2
    table = _lr_table(dev)
    _, eng, w = _engine("fast", dev, table, name, file, steps=n1)
    _lr_train(w, table)
    eng.check()
    keys0, rows0 = _lr_export(table)
    C.save_binary(table, ckpt)
    del w, eng
    t2 = _lr_table(dev)
    assert C.load_binary(t2, ckpt) == len(keys0) and t2.opt.step == n0
    k2, r2 = _lr_export(t2)
    np.testing.assert_array_equal(_bits(r2[np.argsort(k2)]), _bits(rows0[np.argsort(keys0)]))
    _, eng2, w2 = _engine("fast", dev, t2, name, file, steps=n1)
    w2.step_idx = n0
    losses = _lr_train(w2, t2, first=n0, steps=2)
    eng2.check()
    t2.check()
    keys, rows = _lr_export(t2)
    _lr_check(f"resume {name}", _reference(name, 1, n1), [losses], keys, rows,
              t2.weights(rows)[:, 0], first=n0)


def test_resume_from_binary_checkpoint(files, tmp_path):
    in_child(_body_resume, "binary32", files["binary32"], str(tmp_path / "lr.bin"), always=True)
