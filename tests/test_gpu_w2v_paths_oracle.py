"""word2vec through every path it trains on, against the fp64 oracle of
``_w2v_oracle.py`` (built like ``test_gpu_fm_paths_oracle.py``).

Every case trains eight synchronous rounds (``SS_PULL_AHEAD=0``) from a
``PlantedW2V`` source whose batches are checked bit for bit against the arrays
the oracle steps on, and is held to the oracle **step by step**
(``_w2v_oracle.Stepwise``): the table is exported after every round, the oracle
computes that round in fp64 from the table's own rows before it, and every
coordinate of every key's parameters and AdaGrad state must sit within that
round's tolerance; keys the batch did not touch, and keys whose gradient terms
are all structurally zero, must be bit-identical.  Asserted in every case: each
step's positive-pair count (exactly) and loss per pair (within the loss's own
bound), the exported key set (exactly the oracle's, one slot per key), every
coordinate, the dedup's bucket count (at least three; two for a batch below
257 keys), and what ran
(``w.occ_reduce``, ``w.fuse``, ``w.per_pair``, ``eng.fast1``, ``eng.xg``, and
``uhot`` non-empty where a key with more than 32 occurrences is planted).
Where a bf16 tile runs the oracle is ``as_built``; the fp32 tile and the
per-pair kernels are held to ``exact``.

Every case runs in a spawned process of its own (``_fresh``): the open defect
``test_gpu_fm_paths_oracle.py`` records applies to a module of this shape, and
the per-pair knobs are read once per process anyway.

Cases: the window layout with shared negatives and the fused reduce at ``dim``
32 / 64 / 128, with SGD, and on every ``w2v_win_edge`` variant; the same with
``SS_W2V_FUSE=0`` (reduce + apply) and with ``SS_DEDUP=hash`` (the tile's row
atomics); the pairs layout on the bf16 and the fp32 tile; per-pair negatives
at every (W, K) of ``w2v_pp`` and at ``dim`` 32 / 64 / 128; the per-pair knobs
``SS_W2V_PP_ITEMS=1``, ``SS_W2V_PP_QF=4``, ``SS_W2V_PP_STAGES=4`` / ``2``,
``SS_W2V_EARLY_SLOT=0``; compact bf16 rows (every stored value a bf16 neighbour
of the fp32 update widened by the gradient bound); the xGMI unique exchange at
world 1 and world 2 (the union-batch oracle); the shipped initialiser with
``W2VSynth`` batches; and pull-ahead as shipped (staleness 1) as a replay.

No coordinate is widened.  The score gradients the oracle flags as within the
fp32 error of a bf16 rounding midpoint are settled by decoding which of them
the device rounded the other way (``_w2v_oracle.decode_flips``), and every
coordinate is held to that one candidate; every case asserts the issue's cap
on widened coordinates (1 %) over all eight steps, with a share of zero.

Measured on an MI355X, the largest |engine - oracle| / tol per path (x, h;
each case prints its own as ``MARGIN ...``; reported, not tuned):

    window, fused reduce, dim 32 / 64 / 128     x 0.005          h 0.007-0.008
    window, fused, SGD                          x 0.008
    w2v_win_edge b64 / b65 / b128 / w1 / w15    x 0.004-0.043    h 0.006-0.034
    SS_W2V_FUSE=0 (reduce + apply), five cases  x 0.005-0.043    h 0.007-0.034
    SS_DEDUP=hash (the tile's row atomics)      x 0.007-0.012    h 0.011-0.027
    SS_W2V_EARLY_SLOT=0, window                 x 0.005          h 0.007
    pairs layout, bf16 tile, dim 32 / 128       x 0.012 / 0.025  h 0.017 / 0.031
    pairs layout, fp32 tile, dim 32 / 128       x 0.017 / 0.021  h 0.048 / 0.054
    per-pair, every (W, K), dim 32 / 64 / 128   x 0.005-0.025    h 0.015-0.024
    per-pair knobs                              x 0.015-0.021    h 0.016-0.018
    bf16 rows, shared and per-pair              every stored value a bf16 neighbour
    xGMI unique, world 1, shared / per-pair     x 0.005 / 0.013  h 0.007 / 0.018
    xGMI unique, world 2, shared / per-pair     x 0.005 / 0.023  h 0.008 / 0.019
    shipped init, W2VSynth                      x 0.007          h 0.004
    pull-ahead replay (staleness 1)             x 0.005          h 0.007
    loss per pair / its bound                   0.001-0.021

The device does round flagged elements the other way: one of 410 in
``w2v_win_edge/b64`` (fused and unfused alike: 0.043 / 0.034 after it is
settled) and one of 82 in ``b65`` at dim 32.  The fp32 NumPy emulation sits
at 0.004-0.057: every path is at the model's own noise floor, and no defect
was found.  Pull-ahead: all 14080 pulled coordinates that push i-1 changed
already held its value, and every push matched the replay.  SGD free-running
against the carried bound is reported only: it is not reproducible, 0.003 to
6.4 for the same case, because under SGD a flagged element that rounds the
other way moves a parameter by lr ulp |x| ~ 3e-7, far inside a step's
tolerance but enough to move later elements across their midpoints, and the
order of the hot keys' row atomics decides which; the step-by-step check is
the gate.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _w2v_oracle as O
from _mp import collect, file_init, init_gloo, in_child

pytestmark = pytest.mark.gpu

STEPS = O.STEPS
KNOBS = ("SS_CLAIM", "SS_SLOT32", "SS_TABLE_REGIONS", "SS_ENGINE_GENERAL", "SS_DEDUP",
         "SS_SRV_STAGE", "SS_XGMI_SELF", "SS_SERVER_STREAM", "SS_STALENESS", "SS_ENGINE_DEPTH",
         "SS_TABLE_G", "SS_PULL_STREAM", "SS_W2V_FUSE", "SS_W2V_MFMA", "SS_W2V_PP_ITEMS",
         "SS_W2V_PP_QF", "SS_W2V_PP_STAGES", "SS_W2V_EARLY_SLOT", "SS_W2V_WIN_GRID",
         "SS_BD_TARGET", "SS_PULL_VEC", "SS_GRAPH")


def _setup(env, pull_ahead="0"):
    for k in KNOBS:
        os.environ.pop(k, None)
    if pull_ahead is None:
        os.environ.pop("SS_PULL_AHEAD", None)
    else:
        os.environ["SS_PULL_AHEAD"] = pull_ahead
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    from swiftsnails_amd.utils.knobs import KNOBS as TABLE

    for k, v in (env or {}).items():
        assert k in TABLE, k   # a listed knob
        os.environ[k] = v
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev


def _table(optimizer, dim, dev, init, row_dtype="fp32", nkeys=20000):
    """A table with room for ``nkeys`` distinct keys at a load below 1/3."""
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable

    opt = Optimizer(optimizer, lr=O.LR[optimizer], eps=O.EPS)
    cap = 1 << max(16, int(3 * nkeys).bit_length())
    return HbmTable(dim, cap, optimizer=opt, init=init, device=dev, row_dtype=row_dtype)


def _distinct(name, world=1):
    return len(np.unique(np.concatenate([O.data(name, r).keys.reshape(-1)
                                         for r in range(world)])))


def _init(dim, shipped=False):
    from swiftsnails_amd.models.word2vec import make_w2v_table_args
    from swiftsnails_amd.ops.optim import InitConfig

    if shipped:
        return make_w2v_table_args(dim)[1]
    return InitConfig("uniform", O.init_scale(dim), 0.0)


def _init_rows(dev, dim, init, keys, bf16=False):
    """keys -> the device's initial parameters, read from a scratch table with
    the same ``InitConfig`` (the initialiser is a function of key and column)."""
    keys = np.unique(keys)
    t = _table("sgd", dim, dev, init, nkeys=len(keys))
    rows, _ = t.pull(torch.from_numpy(keys.view(np.int64)).to(dev))
    torch.cuda.synchronize()
    t.check()
    rows = rows.cpu().numpy()[:, :dim]
    if bf16:   # a compact row holds its initial values rounded to bf16, to nearest even
        rows = O.bf16(rows).astype(np.float32)

    def f(k):
        pos = np.searchsorted(keys, k)
        assert np.array_equal(keys[pos], k)
        return rows[pos]
    return f


def _source(d, dev):
    """The planted source, its batches checked bit for bit against the arrays
    the oracle steps on (through the interface the worker uses)."""
    src = O.PlantedW2V(d, dev)
    k = torch.empty(src.n_keys, dtype=torch.int64, device=dev)
    m = torch.empty(src.run_len, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    for t in range(STEPS + 1):
        src.generate(t, 0, 1, k, stream=st.cuda_stream, meta=m)
        st.synchronize()
        ek, em = d.batch(t)
        assert np.array_equal(k.cpu().numpy().view(np.uint64), ek), t
        if em is not None:
            assert np.array_equal(m.cpu().numpy(), em), t
    return src


def _export(table):
    ks, rs = [], []
    for k, r in table.export():
        ks.append(k.numpy())
        rs.append(r.numpy())
    return np.concatenate(ks).view(np.uint64), np.concatenate(rs)


def _split(rows, D, ada):
    return rows[:, :D], (rows[:, D:2 * D] if ada else None)


def _mode(sp, env):
    if sp.neg == "per_pair" or (sp.layout == "pairs" and (env or {}).get("SS_W2V_MFMA") == "f32"):
        return "exact"
    return "as_built"


class _Loss:
    """Each step's pair count (exactly) and loss per pair (within its bound)."""

    def __init__(self):
        self.worst = 0.0

    def check(self, t, loss, pairs, g, rank=0, nshards=O.SHARDS):
        assert pairs == g.pairs[rank], (t, pairs, g.pairs)
        want = g.loss[rank] / g.pairs[rank]
        tol = g.eloss[rank] / g.pairs[rank] + O.shard_sum_error(want, nshards)
        r = abs(loss - want) / tol
        self.worst = max(self.worst, r)
        assert r <= 1, (t, loss, want, tol)


def _check(label, sw, lossr, free=None):
    """The assertions of every case; prints the margin before asserting it."""
    extra = f"  free-running x {free:.3f}" if free is not None else ""
    o = sw.orc
    wide = o.wide_coords / max(1, o.coords)
    print(f"MARGIN {label}: max |engine - oracle| / tol  x {sw.rx:.3f}  h {sw.rh:.3f}  loss "
          f"{lossr.worst:.3f}  ({o.nflip} of {o.flagged} flagged elements settled as flipped, "
          f"widened coordinates {wide:.2%}){extra}")
    assert wide <= O.WIDE_CAP   # the issue's cap, over all eight steps
    if sw.bf16_rows:
        assert sw.rx == 0 and sw.rh == 0, (label, sw.rx, sw.rh)
    else:
        assert sw.rx <= 1 and sw.rh <= 1, (label, sw.rx, sw.rh, sw.out)


def _buckets(eng, n):
    for dd in eng.dedupers:
        if dd.mode == "bucket":
            # the step's keys span at least three buckets (two where the whole batch is
            # below 257 keys: the dedup lays out 128 and more occurrences per bucket)
            assert dd.bucket_view(n)[4] >= (3 if n > 256 else 2)


def _hot_planted(d):
    return any(c > O.CHUNK for p in d.plan for c in p)


def _body_world1(name, dim, optimizer, env, xgmi, row_dtype, expect):
    """One world-1 case: eight synchronous rounds held to the oracle."""
    dev = _setup(env)
    from swiftsnails_amd.models.word2vec import Word2VecWorker
    from swiftsnails_amd.parallel.engine import PSEngine
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    sp, d = O.cases()[name], O.data(name)
    ada, bf = optimizer == "adagrad", row_dtype == "bf16"
    init = _init(dim)
    table = _table(optimizer, dim, dev, init, row_dtype, _distinct(name))
    tr = XgmiTransport(0, 1, dev, None, timeout_s=30) if xgmi else None
    src = _source(d, dev)
    eng = PSEngine(table, tr, max_keys=src.n_keys, dim=dim, device=dev)
    w = Word2VecWorker(eng, src)
    assert not eng.pull_ahead
    got = {"occ_reduce": bool(w.occ_reduce), "fuse": bool(getattr(w, "fuse", False)),
           "per_pair": bool(w.per_pair), "fast1": bool(eng.fast1), "xg": eng.xg is not None}
    assert got == expect, (got, expect)
    if sp.layout == "pairs":
        assert w.mfma_bf16 == ((env or {}).get("SS_W2V_MFMA") != "f32")
    mode = _mode(sp, env)
    sw = O.Stepwise(sp, dim, optimizer, mode=mode, init=init, bf16_rows=bf,
                    init_rows=_init_rows(dev, dim, init, d.keys.reshape(-1), bf))
    lossr, hot, uhot = _Loss(), False, getattr(w, "uhot", None)
    for t in range(STEPS):
        w.step()
        loss, pairs = w.mean_loss(), w.step_pairs()
        torch.cuda.synchronize()
        keys, rows = _export(table)
        assert len(np.unique(keys)) == len(keys)   # one slot per key
        sw.step([d.batch(t)], keys, *_split(rows, dim, ada))
        lossr.check(t, loss, pairs, sw.last.grad)
        _buckets(eng, src.n_keys)
        if uhot is not None:
            hot |= any(bool(u.any()) for u in uhot)
    eng.check()
    table.check()
    if tr is not None:
        tr.close()
    if uhot is not None and _hot_planted(d):
        assert hot   # the keys summed over several items went to the masked apply
    free = None
    if not ada and not bf:   # SGD: the free-running reference too, reported
        free = O.free_running_ratio(O.run(name, dim, optimizer, mode=mode, init=init), keys,
                                    rows[:, :dim])
    label = f"{name} dim {dim} {optimizer} {mode} {env or ''}{' xgmi' if xgmi else ''}" \
            f"{' bf16 rows' if bf else ''}"
    _check(label, sw, lossr, free)


def _body_synth(dim):
    """The shipped initialiser (output rows start at zero: ``zero_key_bit``)
    and the real generator's key distribution: the oracle's batch is
    regenerated per step through ``W2VSynth.generate`` into scratch buffers."""
    dev = _setup(None)
    from swiftsnails_amd.models.word2vec import W2VSynth, Word2VecWorker
    from swiftsnails_amd.parallel.engine import PSEngine

    data = W2VSynth(batch_size=200, window=4, vocab=3000, noise=0.1, sentence_len=11)
    sp = O.Spec("window", "shared", data.batch_size, data.window, data.negatives)
    assert sp.n_keys == data.n_keys
    kb = torch.empty(data.n_keys, dtype=torch.int64, device=dev)
    mb = torch.empty(data.run_len, dtype=torch.int32, device=dev)
    bs = []
    for t in range(STEPS):
        data.generate(t, 0, 1, kb, meta=mb)
        torch.cuda.synchronize()
        bs.append((kb.cpu().numpy().view(np.uint64).copy(), mb.cpu().numpy().copy()))
    init = _init(dim, shipped=True)
    assert init.zero_key_bit == O.OUT_BIT
    table = _table("adagrad", dim, dev, init)
    eng = PSEngine(table, None, max_keys=data.n_keys, dim=dim, device=dev)
    w = Word2VecWorker(eng, data)
    assert w.occ_reduce and w.fuse and eng.fast1 and not eng.pull_ahead
    allk = np.concatenate([k for k, _ in bs])
    rows0 = _init_rows(dev, dim, init, allk)
    assert not rows0(np.unique(allk[allk >= O.OUT])).any()   # the output namespace starts at zero
    sw = O.Stepwise(sp, dim, "adagrad", init=init, init_rows=rows0)
    lossr = _Loss()
    for t in range(STEPS):
        w.step()
        loss, pairs = w.mean_loss(), w.step_pairs()
        torch.cuda.synchronize()
        keys, rows = _export(table)
        assert len(np.unique(keys)) == len(keys)
        sw.step([bs[t]], keys, *_split(rows, dim, True))
        lossr.check(t, loss, pairs, sw.last.grad)
    eng.check()
    table.check()
    _check(f"W2VSynth shipped init dim {dim}", sw, lossr)


# ------------------------------------------------------------------ world 2
def _rank(rank, world, name, dim, optimizer, init_m, q):
    dev = _setup(None)
    init_gloo(init_m, rank, world)
    try:
        from swiftsnails_amd.models.word2vec import Word2VecWorker
        from swiftsnails_amd.parallel.engine import PSEngine
        from swiftsnails_amd.parallel.transport import TorchDistTransport
        from swiftsnails_amd.parallel.xgmi import XgmiTransport

        d = O.data(name, rank)
        init = _init(dim)
        tr = XgmiTransport(rank, world, dev, dist.distributed_c10d._get_default_store(),
                           aux=TorchDistTransport(), timeout_s=30)
        table = _table(optimizer, dim, dev, init, nkeys=_distinct(name, world))
        src = _source(d, dev)
        eng = PSEngine(table, tr, max_keys=src.n_keys, dim=dim, device=dev)
        w = Word2VecWorker(eng, src, rank=rank, world=world)
        flags = {"occ_reduce": bool(w.occ_reduce), "fuse": bool(getattr(w, "fuse", False)),
                 "per_pair": bool(w.per_pair), "fast1": bool(eng.fast1),
                 "xg": eng.xg is not None, "ahead": bool(eng.pull_ahead)}
        first = None
        if rank == 0:   # the device's initial rows, for the parent's oracle
            allk = np.unique(np.concatenate([O.data(name, r).keys.reshape(-1)
                                             for r in range(world)]))
            first = (allk, _init_rows(dev, dim, init, allk)(allk))
        out, snaps = [], []
        for _ in range(STEPS):
            w.step()
            out.append((w.mean_loss(), w.step_pairs()))
            torch.cuda.synchronize()
            dist.barrier()   # both ranks' pushes of this round are applied
            snaps.append(_export(table))
            dist.barrier()
        eng.check()
        table.check()
        q.put((rank, out, snaps, flags, first))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", ["w2v_win", "w2v_pp/w5k5"])
def test_w2v_world2_matches_fp64_oracle(name):
    """Two ranks on one GPU, each with its own planted batch: a synchronous
    round is one update per key on the sum of both ranks' gradients (rank 1's
    segment of every exchange sits at a non-zero offset)."""
    world, dim, optimizer = 2, 64, "adagrad"
    sp = O.cases()[name]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    init_m = file_init()
    procs = [ctx.Process(target=_rank, args=(r, world, name, dim, optimizer, init_m, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = collect(q, procs, world, 180)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    for _, _, _, f, _ in res:
        assert f == {"occ_reduce": True, "fuse": False, "per_pair": sp.neg == "per_pair",
                     "fast1": False, "xg": True, "ahead": False}, f
    ikeys, irows = res[0][4]

    def init_rows(k):
        pos = np.searchsorted(ikeys, k)
        assert np.array_equal(ikeys[pos], k)
        return irows[pos]

    sw = O.Stepwise(sp, dim, optimizer, mode=_mode(sp, None), init_rows=init_rows)
    lossr = _Loss()
    for t, b in enumerate(O.batches(name, world)):
        keys = np.concatenate([r[2][t][0] for r in res])
        rows = np.concatenate([r[2][t][1] for r in res])
        assert all(len(r[2][t][0]) > 0 for r in res)   # both shards hold keys
        assert len(np.unique(keys)) == len(keys)
        sw.step(b, keys, *_split(rows, dim, True))
        for r in res:
            lossr.check(t, r[1][t][0], r[1][t][1], sw.last.grad, rank=r[0])
    _check(f"world 2 xgmi unique {name}", sw, lossr)


# --------------------------------------------------------------- pull-ahead
def _pulled_rows(rnd, bk, dim):
    """The rows a pulled round holds, by key: (sorted distinct keys of the
    batch, their rows), every occurrence of a key resolving to one row."""
    uid = rnd.dd.owner.unique_ids(bk.size).cpu().numpy()
    assert (uid >= 0).all()
    u, first, inv = np.unique(bk, return_index=True, return_inverse=True)
    assert np.array_equal(uid, uid[first][inv]) and len(np.unique(uid[first])) == len(u)
    return u, rnd.uvals[torch.from_numpy(uid[first]).to(rnd.uvals.device)].cpu().numpy()[:, :dim]


def _body_pull_ahead(name, dim):
    """Pull-ahead as shipped (staleness 1, what ``Word2VecWorker`` turns on).
    The pull of round i is enqueued before push i-1 and waits only for push
    i-2, so each pulled coordinate may come from the table after push i-2 or
    after push i-1, never older and nothing else (bit for bit); the oracle
    replays every round from the rows actually pulled, and the table after
    every push must match the replay."""
    dev = _setup(None, pull_ahead=None)
    from swiftsnails_amd.models.word2vec import Word2VecWorker
    from swiftsnails_amd.parallel.engine import PSEngine

    sp, d = O.cases()[name], O.data(name)
    init = _init(dim)
    table = _table("adagrad", dim, dev, init, nkeys=_distinct(name))
    src = _source(d, dev)
    eng = PSEngine(table, None, max_keys=src.n_keys, dim=dim, device=dev)
    w = Word2VecWorker(eng, src)
    assert w.occ_reduce and eng.fast1 and eng.pull_ahead and eng.staleness == 1
    init_rows = _init_rows(dev, dim, init, d.keys.reshape(-1))
    sw = O.Stepwise(sp, dim, "adagrad", mode=_mode(sp, None), init=init, init_rows=init_rows)
    older = (np.empty(0, np.uint64), np.empty((0, dim), np.float32))   # the table after push i-2
    newer = older                                                      # ... after push i-1
    pulled, lossr, fresh, total = None, _Loss(), 0, 0

    def rows_at(state, u):
        """state's rows of keys u; keys it does not hold yet: the initial rows."""
        k, x = state
        out = init_rows(u).copy()
        if len(k):
            pos = np.searchsorted(k, u).clip(max=len(k) - 1)
            hit = k[pos] == u
            out[hit] = x[pos[hit]]
        return out

    for t in range(STEPS):
        bk = d.batch(t)[0]
        if pulled is not None:   # rows recorded after the previous step: round t's pull
            u, p = pulled
            a, b = rows_at(older, u), rows_at(newer, u)
            ok = (p == a) | (p == b)
            assert ok.all(), (t, int((~ok).sum()))
            fresh += int(((p == b) & (p != a)).sum())
            total += int((a != b).sum())
        w.step()
        loss, pairs = w.mean_loss(), w.step_pairs()
        torch.cuda.synchronize()
        keys, rows = _export(table)
        assert len(np.unique(keys)) == len(keys)
        # round t+1's pull ran already and inserted its new keys: still at their
        # initial rows, and no part of this round's model
        nxt = np.unique(d.batch(t + 1)[0])
        early = ~np.isin(keys, np.union1d(sw.keys, np.unique(bk)))
        assert np.isin(keys[early], nxt).all()
        assert np.array_equal(rows[early, :dim], init_rows(keys[early]))
        assert (rows[early, dim:] == 0).all()
        keys, rows = keys[~early], rows[~early]
        sw.step([d.batch(t)], keys, rows[:, :dim], rows[:, dim:2 * dim],
                pulled=None if pulled is None else pulled[1].astype(np.float64))
        lossr.check(t, loss, pairs, sw.last.grad)
        order = np.argsort(keys)
        older, newer = newer, (keys[order], rows[order, :dim])
        if t + 1 < STEPS:
            pulled = _pulled_rows(w._pulled[0], d.batch(t + 1)[0], dim)
    eng.check()
    table.check()
    print(f"PULLED {name}: {fresh} of {total} pulled coordinates that push i-1 changed already "
          f"held its value")
    _check(f"pull-ahead replay {name} dim {dim}", sw, lossr)


# ------------------------------------------------------- a process per case
def _fresh(fn, *args):
    """A case's body in a spawned process of its own (the module docstring
    says why)."""
    in_child(fn, *args, always=True)


FUSED = {"occ_reduce": True, "fuse": True, "per_pair": False, "fast1": True, "xg": False}
UNFUSED = dict(FUSED, fuse=False)
ATOMIC = dict(FUSED, occ_reduce=False, fuse=False)
PAIRS = dict(FUSED, occ_reduce=False, fuse=False)
PP = dict(FUSED, per_pair=True)
XG = dict(FUSED, fuse=False, fast1=False, xg=True)


@pytest.mark.parametrize("name,dim,optimizer",
                         [("w2v_win", 32, "adagrad"), ("w2v_win", 64, "adagrad"),
                          ("w2v_win", 128, "adagrad"), ("w2v_win", 64, "sgd")]
                         + [(f"w2v_win_edge/{k}", 64, "adagrad") for k in O.WIN_EDGE])
def test_window_fused_reduce_matches_fp64_oracle(name, dim, optimizer):
    _fresh(_body_world1, name, dim, optimizer, None, False, "fp32", FUSED)


@pytest.mark.parametrize("name,dim,optimizer", [("w2v_win", 64, "adagrad"),
                                                ("w2v_win", 128, "sgd"),
                                                ("w2v_win_edge/b64", 64, "adagrad"),
                                                ("w2v_win_edge/b65", 32, "adagrad"),
                                                ("w2v_win_edge/b128", 128, "adagrad")])
def test_window_reduce_then_apply_matches_fp64_oracle(name, dim, optimizer):
    _fresh(_body_world1, name, dim, optimizer, {"SS_W2V_FUSE": "0"}, False, "fp32", UNFUSED)


@pytest.mark.parametrize("name,dim,optimizer", [("w2v_win", 64, "adagrad"),
                                                ("w2v_win", 32, "sgd"),
                                                ("w2v_win_edge/w15", 128, "adagrad")])
def test_window_row_atomics_match_fp64_oracle(name, dim, optimizer):
    _fresh(_body_world1, name, dim, optimizer, {"SS_DEDUP": "hash"}, False, "fp32", ATOMIC)


def test_window_fused_reduce_late_slot_load_matches_fp64_oracle():
    """``SS_W2V_EARLY_SLOT=0`` on the path that ships: the window reduce
    (``k_w2v_oreduce<D, false>``) loads the fused update's slot after the
    occurrence gathers."""
    _fresh(_body_world1, "w2v_win", 64, "adagrad", {"SS_W2V_EARLY_SLOT": "0"}, False, "fp32",
           FUSED)


@pytest.mark.parametrize("name,dim,tile", [("w2v_pairs/b128w2", 32, "bf16"),
                                           ("w2v_pairs/b100w5", 128, "bf16"),
                                           ("w2v_pairs/b100w5", 32, "f32"),
                                           ("w2v_pairs/b128w2", 128, "f32")])
def test_pairs_layout_matches_fp64_oracle(name, dim, tile):
    _fresh(_body_world1, name, dim, "adagrad", {"SS_W2V_MFMA": tile}, False, "fp32", PAIRS)


@pytest.mark.parametrize("name,dim,optimizer",
                         [("w2v_pp/w2k1", 32, "adagrad"), ("w2v_pp/w5k5", 32, "adagrad"),
                          ("w2v_pp/w5k5", 64, "sgd"), ("w2v_pp/w5k5", 128, "adagrad"),
                          ("w2v_pp/w5k6", 64, "adagrad"), ("w2v_pp/w3k11", 128, "adagrad"),
                          ("w2v_pp/w15k16", 64, "adagrad")])
def test_per_pair_negatives_match_fp64_oracle(name, dim, optimizer):
    _fresh(_body_world1, name, dim, optimizer, None, False, "fp32", PP)


@pytest.mark.parametrize("knob,value", [("SS_W2V_PP_ITEMS", "1"), ("SS_W2V_PP_QF", "4"),
                                        ("SS_W2V_PP_STAGES", "4"), ("SS_W2V_PP_STAGES", "2"),
                                        ("SS_W2V_EARLY_SLOT", "0")])
def test_per_pair_knob_variants_match_fp64_oracle(knob, value):
    """The instantiations the defaults never run: ``k_w2v_oreduce<D, true>``
    (and its late slot load), ``k_w2v_oreduce_pp2<D, 4>``, ``k_w2v_pp<D, 5,
    4>`` and ``k_w2v_pp16`` at K = 5."""
    env = {knob: value}
    if knob == "SS_W2V_EARLY_SLOT":   # per pair it is k_w2v_oreduce<D, true> that reads it
        env["SS_W2V_PP_ITEMS"] = "1"
    _fresh(_body_world1, "w2v_pp/w5k5", 128, "adagrad", env, False, "fp32", PP)


@pytest.mark.parametrize("name", ["w2v_win", "w2v_pp/w5k5"])
def test_bf16_rows_match_fp64_oracle(name):
    pp = O.cases()[name].neg == "per_pair"
    _fresh(_body_world1, name, 64, "adagrad", None, False, "bf16", PP if pp else FUSED)


@pytest.mark.parametrize("name", ["w2v_win", "w2v_pp/w5k5"])
def test_xgmi_unique_world1_matches_fp64_oracle(name):
    pp = O.cases()[name].neg == "per_pair"
    _fresh(_body_world1, name, 64, "adagrad", None, True, "fp32", dict(XG, per_pair=pp))


def test_shipped_init_and_synthetic_stream_match_fp64_oracle():
    _fresh(_body_synth, 64)


def test_pull_ahead_replay_matches_fp64_oracle():
    _fresh(_body_pull_ahead, "w2v_win", 64)
