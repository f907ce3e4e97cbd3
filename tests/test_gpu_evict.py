"""In-place eviction from the HBM table (csrc/hip/evict.hip, ``HbmTable.evict``
/ ``remove``, ``PSEngine.evict``, ``PipelinedWorker.evict``) on an MI355X.

Table level, at the smallest shapes at which the kernels can go wrong: a
region table (64 regions x 1024 slots) at loads 0.69 and 0.90 with 0 %, ~50 %
and 100 % victims — clusters that wrap a region's end included — and the other
slot layouts (wide fp32 rows with lane groups, prefilled zero-init rows, FTRL's
second state block, compact bf16 rows) through the rule, the mask and
``remove``; tables and regions without any empty slot (the state a
``TableFullError`` leaves); the temporary-memory bound.  Every case asserts:
the count and the size, the exported key set exactly the survivors with
bit-identical rows, every survivor found where its key is stored and no victim
found, every EMPTY slot byte-identical to a fresh table's, a clean ``check()``,
a grown ``version``, and that pulled again the victims restart from
``init_reference``.

Training level: sparse LR through the one-GPU fast path, the xGMI unique
exchange and the record exchange, 4 steps, ``worker.evict``, 4 more steps,
against the evicting fp64 oracle of ``_evict_oracle.py`` with the unchanged
assertions of ``test_gpu_lr_paths_oracle._check`` (each step's loss, the key set
exactly, every key's w and h within the oracle's tolerances), at world 1 and
with two ranks on one GPU.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _evict_oracle as E
import _lr_oracle as O
import test_gpu_lr_paths_oracle as P
from _mp import collect, file_init, init_gloo
from test_gpu_lr_paths_oracle import dev, files  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EMPTY = -1


# ------------------------------------------------------------------ helpers
def _make(dev, dim, cap, kind, init, row_dtype="fp32", l1=0.0):
    from swiftsnails_amd.ops.optim import InitConfig, Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    ic = InitConfig("uniform", 0.02, seed=7) if init == "uniform" else InitConfig("zero")
    return HbmTable(dim, cap, optimizer=Optimizer(kind, lr=0.1, l1=l1), init=ic, device=dev,
                    row_dtype=row_dtype)


def _fill(t, load, seed):
    """``load * capacity`` distinct keys pulled; random subsets pushed random
    gradients of mixed size a few times, a fifth of the keys never."""
    rng = np.random.default_rng(seed)
    n = int(load * t.capacity)
    keys = np.unique(rng.integers(1, 1 << 48, 2 * n, dtype=np.int64))
    rng.shuffle(keys)
    keys = keys[:n]
    kt = torch.from_numpy(keys).to(t.device)
    t.pull(kt)
    pushed = keys[: n * 4 // 5]
    for _ in range(3):
        sub = pushed[rng.random(len(pushed)) < 0.6]
        g = rng.standard_normal((len(sub), t.dim)) * rng.choice([0.01, 0.1, 1.0], (len(sub), 1))
        t.push(torch.from_numpy(sub).to(t.device),
               torch.from_numpy(g.astype(np.float32)).to(t.device))
    torch.cuda.synchronize()
    t.check()
    assert t.size() == n
    return keys


def _export(t):
    ks, rs = [], []
    for k, r in t.export():
        ks.append(k.numpy())
        rs.append(r.numpy())
    if not ks:
        return np.empty(0, np.int64), np.empty((0, t.width), np.float32)
    k, r = np.concatenate(ks), np.concatenate(rs)
    o = np.argsort(k)
    return k[o], r[o]


def _fresh_bytes(t):
    """[capacity, stride] bytes of a fresh allocation of t's layout."""
    from swiftsnails_amd.ops.table import HbmTable

    f = HbmTable(t.dim, t.capacity, optimizer=t.opt, init=t.init_cfg, device=t.device,
                 row_dtype=t.row_dtype)
    assert (f.capacity, f.stride, f.rbits, f.prefilled) == (t.capacity, t.stride, t.rbits,
                                                            t.prefilled)
    return f.storage.view(t.capacity, t.stride)


def _init_rows(t, keys):
    from swiftsnails_amd.ops.optim import init_reference

    ref = init_reference(t.init_cfg, keys, t.dim, t.width)
    if t.bf16:  # a compact row stores its initial value rounded to nearest even
        ref = torch.from_numpy(ref).to(torch.bfloat16).to(torch.float32).numpy()
    return ref


def _check_after(t, keys, rows, victim, n, version0):
    """The assertions of every table-level case.  ``keys`` / ``rows``: the
    sorted export before the call; ``victim``: bool per key; ``n``: what the
    call returned."""
    dev_ = t.device
    assert n == int(victim.sum()) and t.size() == len(keys) - n
    k2, r2 = _export(t)
    assert np.array_equal(k2, keys[~victim])  # exactly the survivors, each once
    assert np.array_equal(r2.view(np.uint32), rows[~victim].view(np.uint32))  # bit-identical
    _, s = t.pull(torch.from_numpy(keys).to(dev_), insert=False)
    s = s.cpu().numpy()
    kv = t.keys_view().cpu().numpy()
    assert (s[victim] == -1).all()
    assert (s[~victim] >= 0).all() and np.array_equal(kv[s[~victim]], keys[~victim])
    empty = torch.from_numpy(kv == EMPTY).to(dev_)
    assert int(empty.sum()) == t.capacity - (len(keys) - n)
    assert torch.equal(t.storage.view(t.capacity, t.stride)[empty], _fresh_bytes(t)[empty])
    t.check()
    assert t.version > version0
    if t.rbits:  # the observability passes describe the table as it is now
        assert int(t.region_occupancy()["mean"] * (1 << t.rbits) + 0.5) == len(keys) - n
    assert int(t.probe_histogram(16).sum()) == len(keys) - n
    # the victims come back as new keys
    if n:
        t.pull(torch.from_numpy(keys[victim]).to(dev_))
        torch.cuda.synchronize()
        t.check()
        assert t.size() == len(keys)
        k3, r3 = _export(t)
        assert np.array_equal(k3, keys)
        assert np.array_equal(r3[victim], _init_rows(t, keys[victim]))
        assert np.array_equal(r3[~victim].view(np.uint32), rows[~victim].view(np.uint32))


def _acc_block(t, rows):
    off = {"adagrad": t.dim, "ftrl": 2 * t.dim, "adam": 2 * t.dim}[t.opt.kind]
    return rows[:, off:off + t.dim].max(1)


def _wrapping_cluster_with_victim(t, keys, victim):
    """Whether some cluster wraps a region's end (the region's last and first
    slots both occupied) and contains a victim — from keys_view() alone."""
    kv = t.keys_view().cpu().numpy()
    R = 1 << t.rbits
    rlen = t.capacity // R
    vset = set(keys[victim].tolist())
    for r in range(R):
        reg = kv[r * rlen:(r + 1) * rlen]
        if reg[0] == EMPTY or reg[-1] == EMPTY or (reg != EMPTY).all():
            continue
        head = int(np.argmax(reg == EMPTY))            # first EMPTY from the start
        tail = int(np.argmax(reg[::-1] == EMPTY))      # ... and from the end
        cluster = np.concatenate([reg[rlen - tail:], reg[:head]])
        if any(int(k) in vset for k in cluster):
            return True
    return False


# ------------------------------------------------------------ 1. region table
@pytest.mark.parametrize("share", [0, 50, 100])
@pytest.mark.parametrize("load", [0.69, 0.90])
def test_region_table_evict(dev, load, share):
    from swiftsnails_amd.ops.optim import EvictRule

    t = _make(dev, 1, 65536, "adagrad", "uniform")
    assert t.rbits == 6 and t.capacity == 65536 and not t.prefilled  # 64 regions x 1024 slots
    _fill(t, load, seed=int(load * 100))
    keys, rows = _export(t)
    h = rows[:, 1]
    thr = {0: -1.0, 50: float(np.median(h)), 100: float("inf")}[share]
    victim = h <= np.float32(thr)
    assert {0: victim.sum() == 0, 50: 0.3 < victim.mean() < 0.7, 100: victim.all()}[share]
    if share == 50:
        assert _wrapping_cluster_with_victim(t, keys, victim)  # else: another seed
    before, v0 = t.storage.clone(), t.version
    n = t.evict(EvictRule(acc_below=thr))
    torch.cuda.synchronize()
    if share == 0:
        assert n == 0 and torch.equal(before, t.storage)  # not a byte changed
    if share == 100:
        assert t.size() == 0
        assert torch.equal(t.storage.view(t.capacity, t.stride), _fresh_bytes(t))
    _check_after(t, keys, rows, victim, n, v0)


# ------------------------------------------------------------ 2. other layouts
LAYOUTS = {
    "wide_fp32": dict(dim=8, kind="adagrad", init="uniform"),
    "sgd_prefilled": dict(dim=1, kind="sgd", init="zero"),
    "ftrl_prefilled": dict(dim=4, kind="ftrl", init="zero", l1=0.01),
    "bf16": dict(dim=32, kind="adagrad", init="uniform", row_dtype="bf16"),
}


@pytest.mark.parametrize("form", ["rule", "mask", "remove"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_evict(dev, layout, form):
    from swiftsnails_amd.ops.optim import EvictRule

    t = _make(dev, cap=4096, **LAYOUTS[layout])
    assert t.rbits == 0 and t.prefilled == (LAYOUTS[layout]["init"] == "zero")
    assert t.bf16 == (layout == "bf16") and t.G == {1: 1, 8: 4, 4: 4, 32: 16}[t.dim]
    _fill(t, 0.8, seed=len(layout))
    keys, rows = _export(t)
    if t.opt.kind == "sgd":
        score = np.abs(rows[:, :t.dim]).max(1)
        thr = np.float32(np.median(score[score > 0]))
        rule = EvictRule(w_below=float(thr))
    else:
        score = _acc_block(t, rows)
        thr = np.float32(np.median(score))
        rule = EvictRule(acc_below=float(thr))
    victim = score <= thr
    assert 0.2 < victim.mean() < 0.8
    v0 = t.version
    if form == "rule":
        n = t.evict(rule)
    elif form == "mask":
        # the tensor-code form: any bool tensor in slot order; bits on EMPTY slots are ignored
        kv = t.keys_view()
        vk = torch.from_numpy(keys[victim]).to(dev)
        mask = torch.isin(kv, vk) | (kv == EMPTY)
        n = t.evict(mask=mask)
    else:
        absent = torch.arange(1, 100, dtype=torch.int64, device=dev) + (1 << 55)
        vk = torch.from_numpy(keys[victim]).to(dev)
        n = t.remove(torch.cat([vk, absent, vk[:7]]))
    torch.cuda.synchronize()
    _check_after(t, keys, rows, victim, n, v0)


def test_nan_rows_survive(dev):
    """The 0xFFFFFFFF "not written yet" fill and the init marker read as NaN:
    such a row is a survivor under any threshold."""
    from swiftsnails_amd.ops.optim import EvictRule

    t = _make(dev, 2, 4096, "adagrad", "uniform")
    keys = _fill(t, 0.5, seed=3)
    marked = np.sort(keys)[:5]
    s = t.lookup_slots(torch.from_numpy(marked).to(dev))
    rv = t.rows_view()
    rv[s[:3], 0] = torch.tensor(-1, dtype=torch.int32, device=dev).view(torch.float32)
    rv[s[3:], 1] = torch.tensor(0x7FBADBAD, dtype=torch.int32, device=dev).view(torch.float32)
    n = t.evict(EvictRule(w_below=float("inf"), acc_below=float("inf")))
    assert n == len(keys) - 5 and t.size() == 5
    assert np.array_equal(_export(t)[0], marked)


# ------------------------------------------------------- 3. no empty slot left
def test_full_table_evict_by_mask(dev):
    """A 64-slot table filled to 64 / 64 has no cluster boundary: it is rebuilt
    from its survivors, and the table-full error is cleared."""
    from swiftsnails_amd.ops.table import TableFullError

    t = _make(dev, 2, 64, "adagrad", "uniform")
    assert t.rbits == 0 and t.capacity == 64
    keys = np.arange(1, 65, dtype=np.int64) * 7919
    kt = torch.from_numpy(keys).to(dev)
    t.pull(kt)
    t.push(kt[:40], torch.randn(40, 2, device=dev))
    t.check()
    assert t.size() == 64 and int((t.keys_view() == EMPTY).sum()) == 0
    t.pull(torch.tensor([123456789], dtype=torch.int64, device=dev))  # no slot for it
    with pytest.raises(TableFullError):
        t.check()
    keys, rows = _export(t)
    victim = np.arange(64) % 2 == 0
    mask = torch.isin(t.keys_view(), torch.from_numpy(keys[victim]).to(dev))
    v0 = t.version
    n = t.evict(mask=mask)
    _check_after(t, keys, rows, victim, n, v0)  # check() is clean again


def test_region_full_then_evict_trains_on(dev, monkeypatch):
    """The state of test_region_full_fails_loudly_without_silent_loss: the
    bench-path worker driven until a probe region has no empty slot.  The
    eviction frees every such region, clears the error, and training goes on."""
    from swiftsnails_amd.models.sparse_lr import CtrSynth, SparseLRWorker, lr_init, make_lr_table
    from swiftsnails_amd.ops.optim import EvictRule
    from swiftsnails_amd.ops.table import TableFullError
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    B, F = 128, 13
    data = CtrSynth(batch_size=B, num_fields=F, num_features=50_000_000, tail_frac=1.0)
    table = make_lr_table(data.num_features, 1, load=0.5, device=dev, capacity=1 << 16,
                          init=lr_init("uniform", 0.01))
    assert table.rbits == 6 and table.capacity == 1 << 16
    eng = PSEngine(table, None, max_keys=B * F, dim=1, device=dev)
    w = SparseLRWorker(eng, data)
    assert eng.claim
    err = None
    for step in range(100):
        w.step()
        if step >= 30:  # the first region fills near full load
            torch.cuda.synchronize()
            try:
                eng.check()
            except TableFullError as e:
                err = e
                break
    assert err is not None, "the table never filled"
    assert table.region_occupancy()["max_fill"] == 1.0
    keys, rows = _export(table)
    thr = float(np.median(rows[:, 1]))
    victim = rows[:, 1] <= np.float32(thr)
    n = w.evict(EvictRule(acc_below=thr))
    assert n == int(victim.sum()) and table.size() == len(keys) - n
    eng.check()  # the error is gone: every full region got slots back
    table.check()
    assert table.region_occupancy()["max_fill"] < 1.0
    k2, r2 = _export(table)
    assert np.array_equal(k2, keys[~victim])
    assert np.array_equal(r2.view(np.uint32), rows[~victim].view(np.uint32))
    l0 = None
    for _ in range(5):
        w.step()
        l0 = w.mean_loss()
    eng.check()
    assert np.isfinite(l0) and l0 > 0
    k3, _ = _export(table)
    assert len(np.unique(k3)) == len(k3) == table.size() and EMPTY not in k3
    _, s = table.pull(torch.from_numpy(k3).to(dev), insert=False)
    s = s.cpu().numpy()
    assert (s >= 0).all() and np.array_equal(table.keys_view().cpu().numpy()[s], k3)


# ------------------------------------------------------------------ 4. memory
def test_rule_evict_temporary_memory(dev):
    """A rule-based call on a table with empty slots needs one byte per slot
    (+ 1 MiB): what a rebuild through export / assign cannot meet."""
    from swiftsnails_amd.ops.optim import EvictRule

    cap = 1 << 20
    t = _make(dev, 1, cap, "adagrad", "zero")  # a 16 MiB LR shard
    assert t.nbytes == 16 << 20 and t.rbits == 10
    keys = torch.arange(1, cap // 2 + 1, dtype=torch.int64, device=dev) * 7919
    t.pull(keys)
    t.push(keys[::2].contiguous(), torch.ones(cap // 4, 1, device=dev))
    torch.cuda.synchronize()
    t.check()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    n = t.evict(EvictRule(acc_below=0.0))  # the keys never pushed
    peak = torch.cuda.max_memory_allocated(dev)
    print(f"EVICT MEMORY: peak rise {peak - base} bytes for {cap} slots")
    assert n == cap // 4 and t.size() == cap // 4
    assert peak - base <= (1 << 20) + (1 << 20)
    t.check()


# ------------------------------------------------- 5. training against the oracle
def _train_evict(w, ev):
    from swiftsnails_amd.ops.optim import EvictRule

    losses = []
    for _ in range(E.EVICT_AFTER):
        w.step()
        losses.append(w.mean_loss())
    n = w.evict(EvictRule(acc_below=ev.thr))
    for _ in range(O.STEPS - E.EVICT_AFTER):
        w.step()
        losses.append(w.mean_loss())
    torch.cuda.synchronize()
    return losses, n


def _oracle_preconditions(ev):
    assert ev.margin >= 4 and ev.reappear >= 100 and ev.res.ill == 0


@pytest.mark.parametrize("name", ["binary32", "valued64"])
@pytest.mark.parametrize("path", ["fast", "unique", "records_own"])
def test_lr_evict_matches_evicting_oracle(dev, files, monkeypatch, path, name):  # noqa: F811
    from swiftsnails_amd.models.sparse_lr import SparseLRWorker

    ev = E.evicting_reference(name)
    _oracle_preconditions(ev)
    table = P._table("adagrad", dev)
    eng, tr = P._engine(path, table, dev, monkeypatch)
    w = SparseLRWorker(eng, P._source(files[name], name, O.B, dev))
    if path == "fast":
        assert eng.fast1 and eng.claim
    else:
        assert not eng.fast1 and eng.xg is not None and eng.records == (path != "unique")
    v0 = table.version
    losses, n = _train_evict(w, ev)
    eng.check()
    table.check()
    assert table.version > v0
    keys, rows = P._export(table)
    if tr is not None:
        tr.close()
    assert n == len(ev.evicted)
    assert table.size() == len(ev.res.keys)
    P._check(f"evict {path} {name}", ev.res, [losses], keys, rows)


def _rank_evict(rank, world, path, name, init, q):
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    for k in P.KNOBS:
        os.environ.pop(k, None)
    init_gloo(init, rank, world)
    try:
        from swiftsnails_amd.models.sparse_lr import SparseLRWorker
        from swiftsnails_amd.parallel.engine import PSEngine
        from swiftsnails_amd.parallel.transport import TorchDistTransport
        from swiftsnails_amd.parallel.xgmi import XgmiTransport

        dev_ = torch.device("cuda", 0)
        torch.cuda.set_device(dev_)
        tr = XgmiTransport(rank, world, dev_, dist.distributed_c10d._get_default_store(),
                           aux=TorchDistTransport(), timeout_s=30)
        table = P._table("adagrad", dev_)
        eng = PSEngine(table, tr, max_keys=O.B // world * O.F, dim=1, device=dev_,
                       exchange="unique")
        w = SparseLRWorker(eng, P._source(path, name, O.B // world, dev_, rank, world),
                           rank=rank, world=world)
        losses, n = _train_evict(w, E.evicting_reference(name, world))
        eng.check()
        table.check()
        keys, rows = P._export(table)
        q.put((rank, losses, keys, rows, n))
    finally:
        dist.destroy_process_group()


def test_lr_evict_world2_matches_evicting_oracle(files):  # noqa: F811
    """Two ranks on one GPU, the unique exchange: every rank evicts its own
    shard between the same two rounds (not a collective)."""
    world, name = 2, "valued64"
    ev = E.evicting_reference(name, world)
    _oracle_preconditions(ev)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init = file_init()
    procs = [ctx.Process(target=_rank_evict, args=(r, world, files[name], name, init, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    assert all(len(x[2]) > 0 and x[4] > 0 for x in res)  # both shards hold and evict keys
    assert sum(x[4] for x in res) == len(ev.evicted)
    keys = np.concatenate([x[2] for x in res])
    rows = np.concatenate([x[3] for x in res])
    P._check("evict world2 unique", ev.res, [x[1] for x in res], keys, rows, world=world)


# ------------------------------------------------------------------ 6. guards
def test_evict_needs_exactly_one_of_rule_and_mask(dev):
    from swiftsnails_amd.ops.optim import EvictRule

    t = _make(dev, 1, 4096, "adagrad", "uniform")
    _fill(t, 0.3, seed=1)
    mask = torch.zeros(t.capacity, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError):
        t.evict()
    with pytest.raises(ValueError):
        t.evict(EvictRule(acc_below=1.0), mask=mask)
    with pytest.raises(ValueError):
        t.evict(EvictRule())
    with pytest.raises(ValueError):
        t.evict(mask=mask[:100])
    with pytest.raises(ValueError):
        _make(dev, 1, 4096, "sgd", "zero").evict(EvictRule(acc_below=1.0))
    assert t.evict(mask=mask) == 0 and t.size() == int(0.3 * t.capacity)


def _synth_worker(dev, monkeypatch, ahead="0"):
    from swiftsnails_amd.models.sparse_lr import CtrSynth, SparseLRWorker, lr_init, make_lr_table
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_AHEAD", ahead)
    data = CtrSynth(batch_size=1024, num_fields=13, num_features=1_000_000, tail_frac=0.3)
    table = make_lr_table(data.num_features, 1, device=dev, capacity=1 << 20,
                          init=lr_init("uniform", 0.01))
    eng = PSEngine(table, None, max_keys=1024 * 13, dim=1, device=dev)
    return SparseLRWorker(eng, data), eng, table


def test_worker_evict_refuses_live_graphs_and_pulled_rounds(dev, monkeypatch):
    from swiftsnails_amd.ops.optim import EvictRule

    rule = EvictRule(acc_below=1e-3)
    w, eng, table = _synth_worker(dev, monkeypatch)
    for _ in range(3):
        w.step()
    assert w.evict(rule) >= 0  # between eager synchronous steps: fine
    assert w.enable_graph()
    w.step()
    with pytest.raises(RuntimeError, match="graph"):
        w.evict(rule)
    torch.cuda.synchronize()
    w.close()
    # a round between its pull and its push
    w2, eng2, _ = _synth_worker(dev, monkeypatch)
    assert w2.set_pull_ahead(True)
    w2.step()
    assert len(w2._pulled) > 0
    with pytest.raises(RuntimeError, match="pulled"):
        w2.evict(rule)
    w2.set_pull_ahead(False)
    assert w2.evict(rule) >= 0 and not w2._pulled  # drained, then evicted
    w2.step()
    torch.cuda.synchronize()
    eng2.check()


def test_engine_evict_between_claimed_pull_and_push(dev, monkeypatch):
    """PSEngine.evict with a claimed round pulled but not pushed: the claims
    are committed first, the eviction moves survivors of that round to other
    slots, and the push still updates the right rows — the same rows as a
    twin run without the eviction."""
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    monkeypatch.setenv("SS_CLAIM", "1")
    rng = np.random.default_rng(5)
    allk = np.unique(rng.integers(1, 1 << 48, 60000, dtype=np.int64))
    rng.shuffle(allk)
    ka, new_b, kc = allk[:1500], allk[1500:2300], allk[2300:2300 + 38000]
    kb = np.concatenate([ka[:800], new_b])
    out = {}
    for twin in ("plain", "evict"):
        t = _make(dev, 1, 1 << 16, "adagrad", "uniform")
        assert t.rbits == 6
        eng = PSEngine(t, None, max_keys=1664, dim=1, device=dev)
        eng.claim_rounds = True
        kct = torch.from_numpy(kc).to(dev)
        t.push(kct, torch.full((len(kc), 1), 1e-3, device=dev))  # cold keys, tiny h
        ra = eng.pull(torch.from_numpy(ka).to(dev))
        eng.accumulate(ra, torch.ones(len(ka), 1, device=dev))
        eng.push(ra)
        rb = eng.pull(torch.from_numpy(kb).to(dev))
        assert rb.deferred and rb.slot32  # a claimed pull, its new keys not written yet
        nb = int(rb.dd.ucount.sum())
        s0 = rb.slots.view(torch.int32)[:nb].clone()
        if twin == "evict":
            mask = torch.isin(t.keys_view(), kct)
            n = eng.evict(mask=mask)
            assert n == len(kc) and not rb.deferred and not eng._claimed
            s1 = rb.slots.view(torch.int32)[:nb]
            assert (s0 >= 0).all() and (s1 >= 0).all() and bool((s0 != s1).any())  # keys moved
        eng.accumulate(rb, torch.full((len(kb), 1), 2.0, device=dev))
        eng.push(rb)
        torch.cuda.synchronize()
        eng.check()
        t.check()
        out[twin] = t.to_dict(with_state=True)
        assert t.size() == len(out[twin])
    live = np.concatenate([ka, new_b]).tolist()
    assert set(out["evict"]) == set(live)
    assert set(out["plain"]) == set(live) | set(kc.tolist())
    a = np.stack([out["evict"][k] for k in live])
    b = np.stack([out["plain"][k] for k in live])
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=0)
    np.testing.assert_allclose(out["evict"][int(ka[0])][1], 1.0 + 4.0, rtol=1e-6)
