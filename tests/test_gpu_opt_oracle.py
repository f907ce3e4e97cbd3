"""FTRL, Adam, L1 / L2, the gradient scale and the clip on every apply path,
against the fp64 oracle of ``_opt_oracle.py`` and within its derived bound.

Table level (in the pytest process; no engine, no xGMI arena): ``push_slots``
+ ``next_round`` on ~700 keys, six steps with planted and Gaussian gradients
alternating, every step checked from the table's own exported rows and, for
SGD and Adam, the free-running fp64 trajectory from the initial rows (the
Adam one pins the round counter); ``-1`` slots; a three-segment ``SegList``;
the AdaGrad snapshot apply; bf16 rows (every stored word a bf16 neighbour of
[oracle - bound, oracle + bound]); the server merge's fused update.

The dims of ``DIMS`` come from ``launch_apply``'s own conditions (G is the
table's default lane group for the row width W = dim * (1 + state floats)):

    dim   sgd (W = dim)        adagrad (2 dim)      ftrl / adam (3 dim)
      1   k_apply, registers   k_apply, 8-byte pair k_apply, registers (G 4)
      2   k_apply, registers   k_apply_st           k_apply_st
      8   k_apply_st           k_apply_st           k_apply_st, two state blocks, W 24
      9   k_apply (odd W)      k_apply_st (W 18)    k_apply (odd W 27), registers
     16   k_apply_st           k_apply_st (W 32)    k_apply_st, W 48 = kStageMaxW, G 16
     17   k_apply, per-coordinate loop (17 > 4 G)
                               k_apply_st (W 34)    k_apply (W 51 > kStageMaxW)
     24   k_apply_st           k_apply_st, W 48     k_apply (W 72), G 16
     33   k_apply              k_apply (W 66)       k_apply (W 99)
     32 / 64 / 128             k_apply_rows<D, false> for every rule
     5 with lane group 1: dim > G * kApplyRegs with every state width, the
     per-coordinate loop (``opt_apply``) of ``apply_row``

Engine level (each case in a spawned process of its own, as the FM and
word2vec oracle modules run theirs): sparse LR on ``_lr_oracle``'s files with
``LROracle`` extended to the four rules.

Measured on an MI355X, the largest |device - oracle| / bound per path (each
case prints its own as ``MARGIN ...``; reported, not tuned):

    push_slots, every dim, step by step    sgd 0.494  adagrad 0.499  ftrl 0.500  adam 0.495
    push_slots, free-running               sgd 0.494  adam 0.487
    -1 slots / three segments, fp32        0.40-0.49          snapshot apply  0.487
    server merge, fp32, 1 and 2 sources    ftrl 0.45-0.50     adam 0.44-0.48
    bf16 rows (apply, segments, merge)     every stored word a bf16 neighbour (0 outside)
    engine, |engine - oracle| / tol (w, state)
      ftrl l1   fast 0.005 0.058   unique 0.005 0.038   world 2 0.006 0.023
      adam      fast 0.002 0.028                        world 2 0.003 0.035
      adagrad l2 + clip   fast 0.016 0.077   records_own 0.013 0.127
      sgd l2    fast 0.011 -

The table-level figures equal the CPU calibration's (0.455-0.497 for the
oracle's own fp32 evaluation): one rounding of a result just above a power
of two is worth half the bound, and nothing exceeds it.  No defect was found
in a kernel; the defects were in the host's bias corrections
(``docs/TESTING.md``).
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _lr_oracle as L
import _opt_oracle as O
from _mp import collect, file_init, in_child, init_gloo

pytestmark = pytest.mark.gpu

NKEYS, CAP, STEPS = 700, 4096, 6
KINDS = ("sgd", "adagrad", "ftrl", "adam")
DIMS = [(1, None), (2, None), (8, None), (9, None), (16, None), (17, None), (24, None),
        (33, None), (32, None), (64, None), (128, None), (5, 1)]


@pytest.fixture(scope="module")
def dev():
    from swiftsnails_amd._native import hip

    hip()  # loud failure if the extension is missing on a GPU box
    return torch.device("cuda", 0)


def _keys(n=NKEYS, seed=3):
    return np.unique(np.random.default_rng(seed).integers(1, 1 << 40, size=n, dtype=np.int64))


def _table(h, dim, dev, row_dtype="fp32", lane_group=None, keys=None, rows=None, cap=CAP):
    """A table of rule ``h`` holding ``keys`` with the oracle's initial rows
    (planted states first): (table, keys, device keys, slots)."""
    from swiftsnails_amd.ops.optim import InitConfig, Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    t = HbmTable(dim, cap, optimizer=Optimizer(**h.kwargs()), init=InitConfig("zero"),
                 device=dev, lane_group=lane_group, row_dtype=row_dtype)
    k = _keys() if keys is None else keys
    kt = torch.from_numpy(k).to(dev)
    t.assign(kt, torch.from_numpy(O.table_rows(h, len(k), dim) if rows is None else rows))
    slots = t.lookup_slots(kt)
    torch.cuda.synchronize()
    t.check()
    assert t.size() == len(k) and int(slots.min()) >= 0
    return t, k, kt, slots


def _rows(t, k):
    d = t.to_dict(with_state=True)
    assert len(d) == len(k)
    return np.stack([d[int(x)] for x in k.view(np.uint64)])


def _push(t, slots, g, dev, **kw):
    t.push_slots(slots, torch.from_numpy(np.ascontiguousarray(g)).to(dev), **kw)
    torch.cuda.synchronize()


def _expected_kernel(kind, dim, G):
    """The branch of launch_apply / apply_row a (rule, dim, G) reaches, from
    the conditions of table.hip (fp32 rows, no snapshot)."""
    ns = O.NSTATE[kind]
    W = dim * (1 + ns)
    if dim in (32, 64, 128):
        return "k_apply_rows"
    if 1 < G <= 16 and dim > 1 and W <= 48 and W % 2 == 0:
        return "k_apply_st"
    if G == 1 and dim == 1 and kind == "adagrad":
        return "k_apply pair"
    return "k_apply registers" if dim <= 4 * G else "k_apply loop"


def test_dims_reach_every_branch():
    from swiftsnails_amd.ops.table import default_lane_group

    seen = {}
    for kind in KINDS:
        for dim, lg in DIMS:
            G = lg or default_lane_group(dim * (1 + O.NSTATE[kind]))
            seen.setdefault(_expected_kernel(kind, dim, G), set()).add((kind, dim))
    for br in ("k_apply_rows", "k_apply_st"):
        assert {k for k, _ in seen[br]} == set(KINDS), br      # every state width
    assert {k for k, _ in seen["k_apply registers"]} == set(KINDS)
    assert {k for k, _ in seen["k_apply loop"]} == set(KINDS)
    assert seen["k_apply pair"] == {("adagrad", 1)}
    assert ("ftrl", 16) in seen["k_apply_st"] and ("ftrl", 17) in seen["k_apply registers"]


def _hold(h, parts, got, dim, label):
    r = O.rows_ratio(h, parts, got, dim)
    i = np.unravel_index(int(r.argmax()), r.shape)
    assert r[i] <= 1.0, (label, float(r[i]), i, float(got[i]),
                         float(O.join([None if p is None else p.v for p in parts])[i]))
    return float(r.max())


@pytest.mark.parametrize("which", ["plain", "reg"])
@pytest.mark.parametrize("dim,lane_group", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_push_slots_matches_fp64_oracle(dev, kind, dim, lane_group, which):
    h = O.setting(kind, which)
    t, k, kt, slots = _table(h, dim, dev, lane_group=lane_group)
    before = _rows(t, k)
    np.testing.assert_array_equal(before, O.table_rows(h, len(k), dim))
    free = O.split(kind, before, dim)
    worst = wfree = 0.0
    for s in range(STEPS):
        g = O.table_grads(h, len(k), dim, s)
        assert t.opt.step == s
        _push(t, slots, g, dev)
        t.next_round()
        after = _rows(t, k)
        parts = O.step_rows(h, before, g, dim, s + 1)[2]
        worst = max(worst, _hold(h, parts, after, dim, ("step", s + 1)))
        if kind in ("sgd", "adam"):
            free = O.step(h, *free, g, s + 1)
            wfree = max(wfree, _hold(h, free, after, dim, ("free-running", s + 1)))
        before = after
    print(f"MARGIN push_slots {kind} {which} dim {dim}: step {worst:.4f}  free-running {wfree:.4f}")


CASES = [("adagrad", 1, "fp32", None), ("ftrl", 8, "fp32", None), ("adam", 9, "fp32", None),
         ("sgd", 5, "fp32", 1), ("adam", 64, "fp32", None), ("ftrl", 64, "bf16", None),
         ("adam", 33, "bf16", None)]


def _hold_one_step(h, before, g, after, dim, sel, bf16, label):
    """Rows ``sel`` took one step (round 1) of the oracle; the others are
    untouched bit for bit."""
    assert sel.any() and not sel.all()
    np.testing.assert_array_equal(after[~sel].view(np.uint32), before[~sel].view(np.uint32))
    parts = O.step_rows(h, before[sel], g[sel], dim, 1)[2]
    if not bf16:
        return _hold(h, parts, after[sel], dim, label)
    return _hold_bf16(parts, after[sel], label)


def _hold_bf16(parts, got, label):
    """Every stored word is a bf16 neighbour of [oracle - bound, oracle +
    bound]; returns the largest distance from the oracle in units of the
    wider of the bound and one bf16 ulp."""
    v = O.join([None if p is None else p.v for p in parts])
    b = O.join([None if p is None else O.bound(p) for p in parts])
    assert np.isfinite(b).all()
    lo, hi = O.bf16_interval(v - b, v + b)
    assert ((got.view(np.uint32) & 0xFFFF) == 0).all()
    bad = (got < lo) | (got > hi) | np.isnan(got)
    i = np.unravel_index(int(bad.argmax()), bad.shape)
    assert not bad.any(), (label, int(bad.sum()), i, float(got[i]), float(lo[i]), float(hi[i]))
    return float((np.abs(got - v) / np.maximum(b, (hi - lo).astype(np.float64) + 1e-300)).max())


@pytest.mark.parametrize("kind,dim,row_dtype,lane_group", CASES)
def test_negative_slots_are_skipped(dev, kind, dim, row_dtype, lane_group):
    h = O.setting(kind, "reg")
    t, k, kt, slots = _table(h, dim, dev, row_dtype, lane_group)
    before = _rows(t, k)
    sel = (np.arange(len(k)) % 3 != 1)
    sl = slots.clone()
    sl[torch.from_numpy(~sel).to(dev)] = -1
    g = O.table_grads(h, len(k), dim, 0)
    _push(t, sl, g, dev)
    w = _hold_one_step(h, before, g, _rows(t, k), dim, sel, row_dtype == "bf16", "slots -1")
    print(f"MARGIN -1 slots {kind} dim {dim} {row_dtype}: {w:.3f}")


@pytest.mark.parametrize("kind,dim,row_dtype,lane_group", CASES)
def test_three_segments_with_gaps(dev, kind, dim, row_dtype, lane_group):
    h = O.setting(kind, "reg")
    t, k, kt, slots = _table(h, dim, dev, row_dtype, lane_group)
    before = _rows(t, k)
    n = len(k)
    offs, cnts = [5, 200, 450], [100, 131, n - 450 - 7]
    sel = np.zeros(n, bool)
    for o, c in zip(offs, cnts):
        assert o + c <= n
        sel[o:o + c] = True
    g = O.table_grads(h, n, dim, 0)
    _push(t, slots, g, dev, segs=t.segs(offs, cnts))
    w = _hold_one_step(h, before, g, _rows(t, k), dim, sel, row_dtype == "bf16", "segments")
    print(f"MARGIN segments {kind} dim {dim} {row_dtype}: {w:.3f}")


def test_adagrad_snapshot_apply(dev):
    """The snapshot form (the (w, h) the pull read, a blind store) and the
    row-read form of the scalar AdaGrad apply, with l2 > 0 and a clip: both
    the oracle's step, and each other's bits."""
    h = O.setting("adagrad", "reg")
    ta, k, kt, sa = _table(h, 1, dev)
    tb, _, _, sb = _table(h, 1, dev)
    assert ta.snapshot_ok and tb.snapshot_ok
    before = _rows(ta, k)
    np.testing.assert_array_equal(before, _rows(tb, k))
    worst = 0.0
    for s in range(2):
        g = O.table_grads(h, len(k), 1, s)
        snap = torch.from_numpy(before.copy()).to(dev)
        assert snap.shape == (len(k), 2)
        _push(ta, sa, g, dev)
        _push(tb, sb, g, dev, snap=snap)
        a, b = _rows(ta, k), _rows(tb, k)
        parts = O.step_rows(h, before, g, 1, s + 1)[2]
        worst = max(worst, _hold(h, parts, a, 1, "row-read"), _hold(h, parts, b, 1, "snapshot"))
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        before = a
    print(f"MARGIN snapshot apply: {worst:.3f}")


@pytest.mark.parametrize("which", ["plain", "reg"])
@pytest.mark.parametrize("dim", [4, 33, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_bf16_rows_one_step(dev, kind, dim, which):
    """Compact rows: fp32 math on bf16 values, stochastically rounded stores.
    One step from the exported rows; no coordinate excused.  Where the fp32
    result is the stored value itself (a zero gradient without L2 leaves SGD's
    w, AdaGrad's (w, n), FTRL's (z, n) and an all-zero Adam row as they
    are) it must come back exactly."""
    h = O.setting(kind, which)
    t, k, kt, slots = _table(h, dim, dev, "bf16")
    before = _rows(t, k)
    assert ((before.view(np.uint32) & 0xFFFF) == 0).all()
    g = O.table_grads(h, len(k), dim, 0)
    _push(t, slots, g, dev)
    after = _rows(t, k)
    parts = O.step_rows(h, before, g, dim, 1)[2]
    w = _hold_bf16(parts, after, (kind, dim, which))
    if which == "plain":
        z = g == 0
        assert z.any()
        bw, b1, b2 = O.split(kind, before, dim)
        aw, a1, a2 = O.split(kind, after, dim)
        same = {"sgd": [(bw, aw)], "adagrad": [(bw, aw), (b1, a1)], "ftrl": [(b1, a1), (b2, a2)],
                "adam": []}[kind]
        for x, y in same:
            np.testing.assert_array_equal(y[z].view(np.uint32), x[z].view(np.uint32))
        if kind == "adam":
            z0 = z & (bw == 0) & (b1 == 0) & (b2 == 0)
            assert z0.any() and (aw[z0] == 0).all() and (a1[z0] == 0).all() and (a2[z0] == 0).all()
    print(f"MARGIN bf16 rows {kind} {which} dim {dim}: {w:.3f}")


# ------------------------------------------------- the server merge's update
def _merge_layout(dev, nsrc, Pd=3, per=400, seed=7):
    """Received keys of ``nsrc`` sources in ``Pd`` server buckets (a key's
    bucket is a function of the key; bucket 0 holds keys of source 0 only, so
    with two sources both branches of the merge run): the server dedup's
    tables, as ``test_server_merge_matches_reference`` builds them."""
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
    L = {"P": P, "rows": rows, "h": h,
         "rkeys": torch.from_numpy(rkeys).to(dev),
         "meta": torch.from_numpy(np.concatenate([rbase.ravel(), rnum.ravel()])).to(dev),
         "cnt": torch.zeros(P + 1, **i32), "bstart": torch.empty(P + 1, **i32),
         "ubase": torch.empty(P, **i32), "unum": torch.empty(P, **i32),
         "pj": torch.empty(rows, **i32), "luid": torch.empty(rows, **i32),
         "bkeys": torch.empty(rows, dtype=torch.int64, device=dev),
         "uc": torch.zeros(1, dtype=torch.int64, device=dev), "err": torch.zeros(1, **i32)}
    st = torch.cuda.current_stream().cuda_stream
    h.srv_dedup(L["rkeys"].data_ptr(), L["meta"].data_ptr(), L["meta"].data_ptr() + 4 * nsrc * Pd,
                cap, nsrc, Pd, 1, 0, L["cnt"].data_ptr(), L["bstart"].data_ptr(),
                L["pj"].data_ptr(), L["luid"].data_ptr(), L["bkeys"].data_ptr(),
                L["ubase"].data_ptr(), L["unum"].data_ptr(), L["uc"].data_ptr(),
                L["err"].data_ptr(), st)
    torch.cuda.synchronize()
    pos = np.concatenate([np.arange(s * cap + rbase[s, b], s * cap + rbase[s, b] + rnum[s, b])
                          for s in range(nsrc) for b in range(Pd)])
    L["pos"], L["rk"] = pos, rkeys[pos]
    assert int(L["err"].item()) == 0
    assert int(L["uc"].item()) == len(np.unique(L["rk"]))
    assert int(L["bstart"][P].item()) == len(pos)
    bs, un = L["bstart"].cpu().numpy(), L["unum"].cpu().numpy()
    occ = np.diff(bs)
    if nsrc == 1:
        assert (occ == un).all()                      # every bucket: np == nu
    else:
        assert occ[0] == un[0] and (occ[1:] > un[1:]).all()   # both branches
    return L


@pytest.mark.parametrize("nsrc", [2, 1])
@pytest.mark.parametrize("kind,dim,row_dtype", [
    ("ftrl", 3, "fp32"), ("ftrl", 9, "fp32"), ("ftrl", 64, "fp32"), ("ftrl", 64, "bf16"),
    ("adam", 3, "fp32"), ("adam", 9, "fp32"), ("adam", 64, "fp32"), ("adam", 64, "bf16")])
def test_server_merge_fused_update(dev, kind, dim, row_dtype, nsrc):
    """k_srv_merge_rows with ``slots``: the received rows of a key are summed
    and go straight into the rule.  The oracle's gradient is the fp64 sum; the
    fp32 summation of |O| rows adds |O| 2^-24 sum |g| to what the rule is fed."""
    h = O.setting(kind, "reg")
    L = _merge_layout(dev, nsrc)
    hp, P, rows = L["h"], L["P"], L["rows"]
    distinct = np.unique(L["rk"])
    t, k, kt, _ = _table(h, dim, dev, row_dtype, keys=distinct)
    svals = torch.empty((rows, dim), device=dev)
    sslots = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    t.pull_buckets((L["bkeys"].data_ptr(), L["bstart"].data_ptr(), L["unum"].data_ptr(),
                    L["ubase"].data_ptr(), P), svals, sslots)
    torch.cuda.synchronize()
    t.check()
    assert t.size() == len(distinct)                  # the pull created nothing
    before = _rows(t, k)
    gn = np.zeros((rows, dim), np.float32)
    planted = O.table_grads(h, len(L["pos"]), dim, 0)
    gauss = O.table_grads(h, len(L["pos"]), dim, 1)
    gn[L["pos"]] = np.where((np.arange(len(L["pos"])) % 2 == 0)[:, None], planted, gauss)
    g = torch.from_numpy(gn).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    hp.srv_merge(P, L["bstart"].data_ptr(), L["ubase"].data_ptr(), L["unum"].data_ptr(),
                 L["pj"].data_ptr(), L["luid"].data_ptr(), g.data_ptr(), 0, dim, t.dt,
                 sslots.data_ptr(), 0, t.opt.native(), st)
    torch.cuda.synchronize()
    after = _rows(t, k)
    idx = np.searchsorted(distinct, L["rk"])
    G = np.zeros((len(distinct), dim))
    A = np.zeros((len(distinct), dim))
    np.add.at(G, idx, gn[L["pos"]].astype(np.float64))
    np.add.at(A, idx, np.abs(gn[L["pos"]]).astype(np.float64))
    cnt = np.bincount(idx, minlength=len(distinct))
    assert cnt.min() >= 1 and (cnt.max() == 2) == (nsrc == 2)
    eG = np.where(cnt > 1, cnt, 0)[:, None] * O.U * A  # one received row: no sum, exact
    parts = O.step(h, *O.split(kind, before, dim), O.N(G, eG), 1)
    if row_dtype == "bf16":
        w = _hold_bf16(parts, after, (kind, dim, nsrc))
    else:
        w = _hold(h, parts, after, dim, (kind, dim, nsrc))
    print(f"MARGIN server merge {kind} dim {dim} {row_dtype} sources {nsrc}: {w:.3f}")


# ------------------------------------------------------------- engine level
# Sparse LR on _lr_oracle's files, LROracle extended to the four rules; every
# case in a process of its own (docs/TESTING.md records why the FM and
# word2vec oracle modules do the same).
LR_CAP = 1 << 20
KNOBS = ("SS_CLAIM", "SS_SLOT32", "SS_TABLE_REGIONS", "SS_ENGINE_GENERAL", "SS_DEDUP",
         "SS_REC_OCC", "SS_REC_GROUP", "SS_SRV_STAGE", "SS_XGMI_SELF", "SS_SERVER_STREAM",
         "SS_STALENESS", "SS_ENGINE_DEPTH", "SS_TABLE_G")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("opt_oracle")
    return {n: L.dataset(n).write(d / f"{n}.libsvm") for n in ("binary32", "valued64")}


def _lr_table(tag, dev):
    from swiftsnails_amd.models.sparse_lr import lr_init, make_lr_table
    from swiftsnails_amd.ops.optim import Optimizer

    kind, reg = L.OPT_SETTINGS[tag]
    opt = Optimizer(kind, lr=L.LR[kind], eps=L.EPS, **dict(reg))
    return make_lr_table(2_000_003, 1, opt, device=dev, capacity=LR_CAP,
                         init=lr_init("uniform", L.INIT_SCALE))


def _lr_source(path, name, batch, dev, rank=0, world=1):
    """The HBM-resident file source, its batches checked against the arrays
    the oracle steps on."""
    from swiftsnails_amd.utils.dataio import FileCtrSource

    ds = L.dataset(name)
    src = FileCtrSource(path, batch_size=batch, num_fields=L.F, rank=rank, world=world,
                        resident="hbm", device=dev)
    k = torch.empty(batch * L.F, dtype=torch.int64, device=dev)
    x = torch.empty(batch * L.F, dtype=torch.float32, device=dev)
    y = torch.empty(batch, dtype=torch.float32, device=dev)
    for t in range(L.OPT_STEPS):
        src.generate(t, rank, world, k, y, xval=x if src.has_values else None)
        ek, ex, ey = ds.batch(t, batch, rank, world)
        assert np.array_equal(k.cpu().numpy().view(np.uint64), ek.reshape(-1)), t
        assert np.array_equal(y.cpu().numpy(), ey), t
        if src.has_values:
            assert np.array_equal(x.cpu().numpy(), ex.reshape(-1)), t
    return src


def _lr_train(w, table):
    losses = []
    for s in range(L.OPT_STEPS):
        assert table.opt.step == s        # the engine's round count reaches the table
        w.step()
        losses.append(w.mean_loss())
    torch.cuda.synchronize()
    assert table.opt.step == L.OPT_STEPS
    return losses


def _lr_export(table):
    ks, rs = [], []
    for k, r in table.export():
        ks.append(k.numpy())
        rs.append(r.numpy())
    return np.concatenate(ks).view(np.uint64), np.concatenate(rs)


def _lr_check(label, tag, ref, losses, keys, rows, world=1):
    """The assertions of every engine case; prints the margin before
    asserting it."""
    kind, reg = L.OPT_SETTINGS[tag]
    ns = O.NSTATE[kind]
    assert ref.ill == 0  # the oracle's precondition, from the oracle alone
    for r, l in enumerate(losses):
        np.testing.assert_allclose(l, ref.mean_losses(world)[:, r], rtol=1e-4)
    assert L.EMPTY not in keys and len(np.unique(keys)) == len(keys)  # one slot per key
    assert np.array_equal(np.sort(keys), ref.keys), (len(keys), len(ref.keys))
    assert rows.shape[1] == 1 + ns
    rw, rh, out = L.ratios(ref, keys, rows[:, 0], rows[:, 1] if ns > 0 else None,
                           rows[:, 2] if ns > 1 else None)
    print(f"MARGIN {label}: max |engine - oracle| / tol  w {rw:.3f}  state {rh:.3f}")
    assert rw <= 1 and rh <= 1, (label, rw, rh, out)
    if kind == "ftrl":
        order = np.argsort(keys)
        near = L.ftrl_near_threshold(ref, dict(reg)["l1"])
        assert near.mean() < 0.01
        dz, oz = rows[order, 0] == 0, ref.w == 0
        assert oz.any() and not oz.all()
        assert np.array_equal(dz[~near], oz[~near]), int((dz != oz)[~near].sum())


def _body_world1(path, tag, name, file):
    from swiftsnails_amd.models.sparse_lr import SparseLRWorker
    from swiftsnails_amd.parallel.engine import PSEngine
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    if path.startswith("records"):
        os.environ["SS_REC_OCC"] = path.split("_")[1]
    kind = L.OPT_SETTINGS[tag][0]
    table = _lr_table(tag, dev)
    tr = None if path == "fast" else XgmiTransport(0, 1, dev, None, timeout_s=30)
    eng = PSEngine(table, tr, max_keys=L.B * L.F, dim=1, device=dev,
                   exchange="records" if path.startswith("records") else "unique")
    w = SparseLRWorker(eng, _lr_source(file, name, L.B, dev))
    assert (w.xval is not None) == (name == "valued64")
    if path == "fast":
        assert eng.fast1
    elif path == "unique":
        assert not eng.fast1 and eng.xg is not None and not eng.records
    else:
        assert eng.records
    if kind == "adam":   # per-round host state: no graph replay (models/base.py)
        assert w.enable_graph() is False
    losses = _lr_train(w, table)
    eng.check()
    table.check()
    keys, rows = _lr_export(table)
    if tr is not None:
        tr.close()
    _lr_check(f"{path} {name} {tag}", tag, L.opt_reference(tag, name), [losses], keys, rows)


@pytest.mark.parametrize("tag,path,name", [
    ("ftrl_l1", "fast", "valued64"), ("ftrl_l1", "unique", "binary32"),
    ("adam", "fast", "binary32"),
    ("adagrad_l2_clip", "fast", "valued64"), ("adagrad_l2_clip", "records_own", "binary32"),
    ("sgd_l2", "fast", "valued64")])
def test_lr_rule_matches_fp64_oracle(files, tag, path, name):
    in_child(_body_world1, path, tag, name, files[name], always=True)


def _rank(rank, world, file, name, tag, init, q):
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
        table = _lr_table(tag, dev)
        eng = PSEngine(table, tr, max_keys=L.B // world * L.F, dim=1, device=dev,
                       exchange="unique")
        w = SparseLRWorker(eng, _lr_source(file, name, L.B // world, dev, rank, world),
                           rank=rank, world=world)
        assert not eng.records and w.xval is not None
        losses = _lr_train(w, table)
        eng.check()
        table.check()
        keys, rows = _lr_export(table)
        q.put((rank, losses, keys, rows))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("tag", ["ftrl_l1", "adam"])
def test_lr_rule_world2_matches_fp64_oracle(files, tag):
    """Two ranks on one GPU over the xGMI unique exchange: one update per key
    on the sum of both ranks' gradients, each rank's table counting the
    rounds for itself."""
    world, name = 2, "valued64"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = file_init()
    procs = [ctx.Process(target=_rank, args=(r, world, files[name], name, tag, init, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    assert all(len(x[2]) > 0 for x in res)  # both shards hold keys
    _lr_check(f"world2 unique {name} {tag}", tag, L.opt_reference(tag, name, world),
              [x[1] for x in res], np.concatenate([x[2] for x in res]),
              np.concatenate([x[3] for x in res]), world=world)
