"""Model kernels on MI355X vs fp64/fp32 host references: word2vec SGNS, FM,
plus short end-to-end training runs through the PS engine."""
import os

import numpy as np
import pytest
import torch
from _mp import in_child

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from swiftsnails_amd._native import hip

    hip()
    return torch.device("cuda", 0)


@pytest.mark.parametrize("D,bf16", [(32, 0), (64, 0), (128, 0), (32, 1), (64, 1), (128, 1)])
def test_w2v_sgns_tile_matches_reference(dev, D, bf16):
    """fp32 tile: fp32-exact; bf16 tile (SS_W2V_MFMA=bf16): negative-sample
    GEMMs from bf16-rounded rows, checked at bf16 tolerance."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.models.word2vec import sgns_reference

    T, C, S = 128, 4, 64  # two tiles
    tiles = T // 64
    rng = np.random.default_rng(D)
    nrows = T + T * C + tiles * S  # every occurrence its own row: exact per-row check
    U = (rng.standard_normal((nrows, D)) * 0.3).astype(np.float32)
    inv = np.arange(nrows, dtype=np.int32)
    g = torch.zeros((nrows, D), device=dev)
    loss = torch.zeros(256 * 32, device=dev)
    tu, ti = torch.from_numpy(U).to(dev), torch.from_numpy(inv).to(dev)
    p, es = ti.data_ptr(), 4
    neg_scale = 0.7
    hip().w2v_sgns(p, p + T * es, p + T * (1 + C) * es, T, C, D, neg_scale, tu.data_ptr(),
                   g.data_ptr(), loss.data_ptr(), torch.cuda.current_stream().cuda_stream,
                   bf16)
    torch.cuda.synchronize()
    G = g.cpu().numpy()
    tot = 0.0
    # bf16 tile: rows rounded to 8 mantissa bits -> ~3 significant digits in
    # the negative-sample terms (the positive pairs and context grads are fp32)
    rt, at = (2e-4, 2e-5) if not bf16 else (3e-2, 1e-2)
    for t in range(tiles):
        V = U[t * 64:(t + 1) * 64]
        X = U[T:T + T * C].reshape(T, C, D)[t * 64:(t + 1) * 64]
        N = U[T + T * C + t * S:T + T * C + (t + 1) * S]
        l, gV, gX, gN = sgns_reference(V, X, N, neg_scale)
        tot += l
        np.testing.assert_allclose(G[t * 64:(t + 1) * 64], gV, rtol=rt, atol=at)
        np.testing.assert_allclose(G[T:T + T * C].reshape(T, C, D)[t * 64:(t + 1) * 64], gX,
                                   rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(G[T + T * C + t * S:T + T * C + (t + 1) * S], gN, rtol=rt,
                                   atol=at)
    np.testing.assert_allclose(loss.sum().item(), tot, rtol=1e-4 if not bf16 else 3e-3)
    # beside it, the derived bound: the fp32 tile against the exact fp64 model,
    # the bf16 tile against fp64 arithmetic on the operands it rounds
    import _w2v_oracle as O

    o = O.grad_pairs(O.Spec("pairs", "shared", T, C // 2), U.astype(np.float64),
                     "as_built" if bf16 else "exact", neg_scale=neg_scale)
    _assert_w2v_within_bound(f"sgns tile D {D} bf16 {bf16}", G, o, loss.sum().item())


def _assert_w2v_within_bound(label, G, o, loss):
    """Every occurrence row within its derived bound (``_w2v_oracle.occ_bound``;
    a row whose bound is zero is exactly zero), and the loss within its own.
    No coordinate is widened: the score gradients the oracle flags as within
    the fp32 error of a bf16 rounding midpoint are settled by decoding which
    of them the kernel rounded the other way (``settle_occ``), and every
    coordinate is held to that one candidate."""
    import _w2v_oracle as O

    ref, nflip = O.settle_occ(o, G)
    tol = O.occ_bound(o)
    err = np.abs(np.asarray(G, np.float64) - ref)
    assert not err[tol == 0].any()
    r = err / np.where(tol > 0, tol, 1.0)
    # the loss: its own bound and the fp32 sum of the counter's shards
    lr = abs(loss - o.loss) / (o.eloss + O.shard_sum_error(o.loss))
    print(f"MARGIN {label}: max |kernel - oracle| / bound {r.max():.3f} ({nflip} of {o.flagged} "
          f"flagged elements settled as flipped), loss {lr:.3f}")
    assert r.max() <= 1 and lr <= 1, (label, float(r.max()), lr)


@pytest.mark.parametrize("D,W,B", [(32, 2, 128), (64, 5, 150), (128, 5, 256), (128, 15, 100)])
def test_w2v_window_tile_matches_reference(dev, D, W, B):
    """Windowed skip-gram tile (k_w2v_win_bf16) vs the fp64 reference on the
    same band of valid pairs: every run position its own row, so each row's
    gradient (summed over the tiles whose window covers it) is checked;
    random sentence tags, reduced windows and masked positions; a partial
    last tile (B = 150, 100)."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.models.word2vec import sgns_window_reference, window_pairs_reference

    S, T = 64, 64
    tiles = (B + T - 1) // T
    R = B + 2 * W
    rng = np.random.default_rng(D + W)
    tags = np.cumsum(rng.random(R) < 0.08)  # sentences of ~12 tokens
    bs = rng.integers(1, W + 1, R)
    meta = ((tags << 4) | bs).astype(np.int32)
    meta[rng.random(R) < 0.1] = -1
    nrows = B + R + tiles * S
    U = (rng.standard_normal((nrows, D)) * 0.3).astype(np.float32)
    inv = np.arange(nrows, dtype=np.int32)
    g = torch.zeros((nrows, D), device=dev)
    loss, pairs = torch.zeros(256 * 32, device=dev), torch.zeros(256 * 32, device=dev)
    tu, ti, tm = (torch.from_numpy(U).to(dev), torch.from_numpy(inv).to(dev),
                  torch.from_numpy(meta).to(dev))
    p = ti.data_ptr()
    npp = 5 / S
    hip().w2v_win(p, p + B * 4, p + (B + R) * 4, tm.data_ptr(), B, W, D, npp, tu.data_ptr(),
                  g.data_ptr(), loss.data_ptr(), pairs.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    G = g.cpu().numpy().astype(np.float64)
    mask = window_pairs_reference(meta, B, W)
    ref = np.zeros((nrows, D))
    tot, npairs = 0.0, 0.0
    for t in range(tiles):
        c0, c1 = t * T, min(B, t * T + T)
        q0, q1 = c0, min(R, c0 + T + 2 * W)
        l, n, gV, gU, gN = sgns_window_reference(U[c0:c1], U[B + q0:B + q1],
                                                 U[B + R + t * S:B + R + (t + 1) * S],
                                                 mask[c0:c1, q0:q1], npp)
        tot, npairs = tot + l, npairs + n
        ref[c0:c1] += gV
        ref[B + q0:B + q1] += gU
        ref[B + R + t * S:B + R + (t + 1) * S] += gN
    assert mask.sum() == npairs > 0
    assert pairs.sum().item() == npairs
    # bf16 rows (8 mantissa bits) in every GEMM, fp32 accumulation
    np.testing.assert_allclose(G, ref, rtol=3e-2, atol=1e-2)
    np.testing.assert_allclose(loss.sum().item(), tot, rtol=3e-3)
    # centers without a valid pair and masked positions get no gradient
    dead = ~mask.any(1)
    assert not G[:B][dead].any()
    assert not G[B:B + R][meta < 0].any()
    # beside it, the derived bound against the as_built model (bf16 operands, fp64 arithmetic)
    import _w2v_oracle as O

    o = O.grad_window(O.Spec("window", "shared", B, W, 5), U.astype(np.float64), meta, "as_built")
    assert o.pairs == npairs
    _assert_w2v_within_bound(f"window tile D {D} W {W} B {B}", G, o, loss.sum().item())


@pytest.mark.parametrize("name", ["w2v_win", "w2v_cbow"])
def test_w2v_window_tiles_refuse_occurrence_rows_without_tail(dev, name):
    """More than one tile (B = 65) storing occurrence rows shares 2W window
    rows between neighbouring tiles: both window launchers refuse a missing
    tail buffer before anything is launched."""
    from swiftsnails_amd._native import hip

    B, W, D, S = 65, 2, 32, 64
    R, tiles = B + 2 * W, 2
    nrows = B + R + tiles * S
    inv = torch.arange(nrows, dtype=torch.int32, device=dev)
    meta = torch.full((R,), (1 << 4) | W, dtype=torch.int32, device=dev)
    u, g, og = (torch.zeros((nrows, D), device=dev) for _ in range(3))
    loss, pairs = torch.zeros(256 * 32, device=dev), torch.zeros(256 * 32, device=dev)
    p = inv.data_ptr()
    with pytest.raises(RuntimeError, match=f"{name}: occurrence rows need the tail buffer"):
        getattr(hip(), name)(p, p + B * 4, p + (B + R) * 4, meta.data_ptr(), B, W, D, 5 / S,
                             u.data_ptr(), g.data_ptr(), loss.data_ptr(), pairs.data_ptr(),
                             torch.cuda.current_stream().cuda_stream, ograd=og.data_ptr(),
                             otail=0)
    torch.cuda.synchronize()
    assert not og.any() and not g.any()


@pytest.mark.parametrize("D,W,K,B", [(32, 2, 3, 70), (64, 5, 5, 128), (128, 5, 5, 200),
                                     (128, 15, 16, 40), (64, 5, 6, 70), (32, 3, 11, 70)])
def test_w2v_per_pair_negatives_match_reference(dev, D, W, K, B):
    """Classic SGNS (k_w2v_pp + k_w2v_ppctx): K negatives per positive pair,
    gradients as occurrence rows.  The center rows and the run-position rows
    (summed over the 2W centers that pair with them) as rows, every negative
    occurrence as its (gn, center) pair — its row is gn * v_center — vs the
    fp64 reference; invalid pairs and masked positions get zero gradients."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.models.word2vec import sgns_pp_reference, window_pairs_reference

    R = B + 2 * W
    rng = np.random.default_rng(D + W + K)
    tags = np.cumsum(rng.random(R) < 0.08)
    bs = rng.integers(1, W + 1, R)
    meta = ((tags << 4) | bs).astype(np.int32)
    meta[rng.random(R) < 0.1] = -1
    nneg = B * 2 * W * K
    nrows = B + R + nneg
    U = (rng.standard_normal((nrows, D)) * 0.3).astype(np.float32)
    inv = np.arange(nrows, dtype=np.int32)
    og = torch.full((B + R, D), float("nan"), device=dev)  # every row must be written
    gnc = torch.full((nneg, 2), float("nan"), device=dev)
    gp = torch.empty(B * 2 * W, device=dev)
    loss, pairs = torch.zeros(256 * 32, device=dev), torch.zeros(256 * 32, device=dev)
    tu, ti, tm = (torch.from_numpy(U).to(dev), torch.from_numpy(inv).to(dev),
                  torch.from_numpy(meta).to(dev))
    p = ti.data_ptr()
    hip().w2v_pp(p, p + B * 4, p + (B + R) * 4, tm.data_ptr(), B, W, K, D, tu.data_ptr(),
                 og.data_ptr(), gp.data_ptr(), loss.data_ptr(), pairs.data_ptr(),
                 torch.cuda.current_stream().cuda_stream, gnc.data_ptr())
    torch.cuda.synchronize()
    gn = gnc.cpu().numpy()
    cen = gn[:, 1].copy().view(np.uint32)
    assert np.isfinite(gn[:, 0]).all()
    live = cen != 0xFFFFFFFF
    assert (gn[~live, 0] == 0).all()
    Gneg = np.zeros((nneg, D))
    Gneg[live] = gn[live, 0:1].astype(np.float64) * U[cen[live].astype(np.int64)]
    G = np.concatenate([og.cpu().numpy().astype(np.float64), Gneg])
    assert np.isfinite(G).all()
    band = window_pairs_reference(meta, B, W)  # [B, R]
    offs = [o - W if o < W else o - W + 1 for o in range(2 * W)]
    qidx = np.arange(B)[:, None] + W + np.array(offs)[None, :]  # [B, 2W] run positions
    mask = band[np.arange(B)[:, None], qidx]
    V = U[:B]
    Uc = U[B + qidx]
    N = U[B + R:].reshape(B, 2 * W, K, D)
    l, gV, gU, gN = sgns_pp_reference(V, Uc, N, mask)
    ref = np.zeros((nrows, D))
    ref[:B] = gV
    np.add.at(ref, B + qidx.reshape(-1), gU.reshape(-1, D))
    ref[B + R:] = gN.reshape(-1, D)
    assert mask.sum() > 0 and pairs.sum().item() == mask.sum()
    np.testing.assert_allclose(G, ref, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(loss.sum().item(), l, rtol=1e-4)
    # beside it, the derived bound against the exact fp64 model (k_w2v_pp for
    # K <= 5, k_w2v_pp16 from K = 6, k_w2v_ppctx; the negatives' rows are
    # expanded above in fp64, inside the bound's product rounding)
    import _w2v_oracle as O

    o = O.grad_per_pair(O.Spec("window", "per_pair", B, W, K), U.astype(np.float64), meta)
    assert o.pairs == mask.sum()
    _assert_w2v_within_bound(f"per-pair D {D} W {W} K {K} B {B}", G, o, loss.sum().item())


def test_w2v_stream_gen_window_layout(dev):
    """Synthetic stream (k_w2v_stream_gen): centers are the run's middle
    positions, sentence tags follow the position, reduced windows in [1, W],
    and the runs of consecutive steps overlap consistently by 2W positions."""
    from swiftsnails_amd.models.word2vec import OUT_BIT, W2VSynth

    d = W2VSynth(batch_size=256, window=4, vocab=10000, sentence_len=10)
    R, B, W = d.run_len, d.batch_size, d.window
    out = []
    for step in (0, 1):
        keys = torch.empty(d.n_keys, dtype=torch.int64, device=dev)
        meta = torch.empty(R, dtype=torch.int32, device=dev)
        d.generate(step, 0, 1, keys, meta=meta)
        torch.cuda.synchronize()
        out.append((keys.cpu().numpy(), meta.cpu().numpy()))
    (k0, m0), (k1, m1) = out
    ob = 1 << OUT_BIT
    for k, m, step in ((k0, m0, 0), (k1, m1, 1)):
        run = k[B:B + R]
        assert ((run & ob) != 0).all() and ((k[:B] & ob) == 0).all()
        np.testing.assert_array_equal(k[:B], run[W:W + B] & ~ob)
        assert (((k[B + R:] & ob) != 0)).all() and ((k[B + R:] & ~ob) < d.vocab).all()
        g = step * B - W + np.arange(R)
        valid = g >= 0
        assert (m[~valid] == -1).all()
        mv = m[valid].astype(np.int64)
        np.testing.assert_array_equal(mv >> 4, g[valid] // d.sentence_len)
        assert ((mv & 15) >= 1).all() and ((mv & 15) <= W).all()
    # step 1's first 2W positions are step 0's last 2W
    np.testing.assert_array_equal(k1[B:B + 2 * W], k0[B + B:B + B + 2 * W])
    np.testing.assert_array_equal(m1[:2 * W], m0[B:B + 2 * W])


@pytest.mark.parametrize("mode", ["window", "pairs"])
def test_word2vec_modes_train(dev, mode):
    """Both batch layouts train (loss per pair falls); the window layout
    counts its pairs on the device (~B x (W + 1) minus sentence edges) and
    carries B + 2W context keys instead of 2W per center."""
    from swiftsnails_amd.models.word2vec import W2VSynth, Word2VecWorker, make_w2v_table_args
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    data = W2VSynth(batch_size=2048, window=3, vocab=5000, noise=0.05, mode=mode)
    opt, init = make_w2v_table_args(64, None)
    table = HbmTable(64, 40000, optimizer=opt, init=init, device=dev)
    eng = PSEngine(table, None, max_keys=data.n_keys, dim=64, device=dev)
    w = Word2VecWorker(eng, data)
    losses = []
    for _ in range(40):
        w.step()
        losses.append(w.mean_loss())
    table.check()
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < 0.85 * np.mean(losses[:3]), losses
    if mode == "window":
        assert data.n_keys == 2048 + 2048 + 6 + 32 * 64
        assert w.samples_per_step() == 2048
        n = w.step_pairs()
        assert 0.7 * 2048 * 4 < n <= 2048 * 6, n
    else:
        assert w.step_pairs() == 2048 * 6


def test_w2v_sgns_duplicate_rows_accumulate(dev):
    """Repeated words (same unique row) must receive the SUM of their grads."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.models.word2vec import sgns_reference

    T, C, S, D = 64, 2, 64, 32
    rng = np.random.default_rng(5)
    nrows = 40
    U = (rng.standard_normal((nrows, D)) * 0.3).astype(np.float32)
    inv = rng.integers(0, nrows, size=T + T * C + S).astype(np.int32)
    g = torch.zeros((nrows, D), device=dev)
    ti = torch.from_numpy(inv).to(dev)
    tu = torch.from_numpy(U).to(dev)
    p = ti.data_ptr()
    hip().w2v_sgns(p, p + T * 4, p + T * (1 + C) * 4, T, C, D, 0.5, tu.data_ptr(), g.data_ptr(),
                   0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    V, X, N = U[inv[:T]], U[inv[T:T + T * C]].reshape(T, C, D), U[inv[T + T * C:]]
    _, gV, gX, gN = sgns_reference(V, X, N, 0.5)
    ref = np.zeros((nrows, D))
    np.add.at(ref, inv[:T], gV)
    np.add.at(ref, inv[T:T + T * C], gX.reshape(-1, D))
    np.add.at(ref, inv[T + T * C:], gN)
    np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=5e-4, atol=5e-5)


@pytest.mark.parametrize("dim", [2, 5, 9, 17])
def test_fm_fwd_bwd_matches_reference(dev, dim):
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.models.fm import fm_reference

    B, F = 1000, 13
    rng = np.random.default_rng(dim)
    U = B * F  # unique row per occurrence: exact per-row gradient check
    rows = (rng.standard_normal((U, dim)) * 0.2).astype(np.float32)
    inv = np.arange(U, dtype=np.int32)
    y = (rng.random(B) < 0.4).astype(np.float32)
    tr, ti, ty = (torch.from_numpy(a).to(dev) for a in (rows, inv, y))
    g = torch.zeros((U, dim), device=dev)
    loss = torch.zeros(256 * 32, device=dev)
    pred = torch.empty(B, device=dev)
    hip().fm_fwd_bwd(ti.data_ptr(), ty.data_ptr(), B, F, dim, tr.data_ptr(), g.data_ptr(),
                     loss.data_ptr(), pred.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    l, p, gr = fm_reference(rows.reshape(B, F, dim), y)
    np.testing.assert_allclose(pred.cpu().numpy(), p, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(loss.sum().item(), l, rtol=1e-4)
    np.testing.assert_allclose(g.cpu().numpy().reshape(B, F, dim), gr, rtol=1e-3, atol=1e-5)


def _fm_grad_reference(inv, uvals, y, B, F):
    """(G, eG, cnt) of ``_fm_oracle.key_gradient``: the fp64 per-key gradient
    rows of one batch from the unique rows, the labels and each occurrence's
    unique id, with the oracle's per-key bound.

    Measured on an MI355X, max |kernel - fp64| / eG (row atomics / LDS atomics
    / sorted lists; each test prints its own as ``MARGIN ...``):

        bucket reduce  dim 9   0.543 all three      dim 17  0.749 all three
                       dim 5, 3 ranks  0.209 / 0.199 / 0.177 (per rank, all three)
        overflow       dim 2   0.200    dim 5  0.186 / 0.169 / 0.169
                       dim 9   0.174 / 0.189 / 0.189        dim 17  0.255
        bucket of 10240  0.159 / 0.142 / 0.142    of 10241  0.155 / 0.151 / 0.151

    The fp32 NumPy evaluation at the bucket-reduce sizes sits at 0.229 (dim 9)
    and 0.841 (dim 17, ``test_fm_oracle_cpu.py::test_key_gradient_fp32_floor``):
    the dim-17 bucket-reduce case has the least headroom, watch it."""
    import _fm_oracle as O

    uid = inv.cpu().numpy().astype(np.int32).astype(np.int64).reshape(B, F)
    return O.key_gradient(uid, uvals.cpu().numpy(), y.cpu().numpy())


@pytest.mark.parametrize("dim,nranks", [(9, 1), (5, 3), (17, 1)])
def test_fm_bucket_reduce_matches_atomic_path(dev, dim, nranks):
    """Atomic-free FM (lane-group forward + per-bucket LDS row reduction) ==
    the per-occurrence atomic kernel, with heavy key duplication."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.ops.dedup import Deduper
    from swiftsnails_amd.parallel.router import HashFrag

    h = hip()
    B, F = 6000, 20
    n = B * F
    rng = np.random.default_rng(dim + nranks)
    keys = (rng.zipf(1.3, n) % 50000).astype(np.int64)
    fm = HashFrag(nranks, 64).rank_map()
    d = Deduper(n, nranks=nranks, frag_map=torch.from_numpy(fm.astype(np.int32)), gdim=dim,
                device=dev, mode="bucket")
    r = d(torch.from_numpy(keys).to(dev))
    st = torch.cuda.current_stream().cuda_stream
    U = nranks * d.ucap
    uvals = torch.randn(U, dim, device=dev) * 0.1
    y = torch.from_numpy((rng.random(B) < 0.4).astype(np.float32)).to(dev)
    g_at = torch.zeros(U, dim, device=dev)
    l_at = torch.zeros(256 * 32, device=dev)
    h.fm_fwd_bwd(r.inv.data_ptr(), y.data_ptr(), B, F, dim, uvals.data_ptr(), g_at.data_ptr(),
                 l_at.data_ptr(), 0, st)
    gs = torch.empty(B, device=dev)
    gss = torch.empty(B * (dim - 1), device=dev)
    g_b = torch.full((U, dim), float("nan"), device=dev)
    l_b = torch.zeros(256 * 32, device=dev)
    h.fm_fwd_g(0, d.index_ptrs(n), y.data_ptr(), B, F, dim,
               uvals.data_ptr(), gs.data_ptr(), gss.data_ptr(), l_b.data_ptr(), 0, st)
    h.bd_reduce_fm(n, nranks, d.scratch.data_ptr(), d.pj.data_ptr(), d.luid.data_ptr(),
                   gs.data_ptr(), gss.data_ptr(), F, dim, uvals.data_ptr(), g_b.data_ptr(), st,
                   ndest=d.ndest)
    # the sorted-list form (default with an overflow list)
    ovf = torch.zeros(h.bd_fm_ovf_words(n), dtype=torch.int32, device=dev)
    g_s = torch.full((U, dim), float("nan"), device=dev)
    h.bd_reduce_fm(n, nranks, d.scratch.data_ptr(), d.pj.data_ptr(), d.luid.data_ptr(),
                   gs.data_ptr(), gss.data_ptr(), F, dim, uvals.data_ptr(), g_s.data_ptr(), st,
                   ovf.data_ptr(), ndest=d.ndest)
    torch.cuda.synchronize()
    uc = r.ucount.cpu().numpy()
    # every kernel against the fp64 gradient, within the per-key bound of
    # _fm_oracle.py (term accuracy + |O| 2^-24 A over the factored form)
    G, eG, cnt = _fm_grad_reference(r.inv, uvals, y, B, F)
    for q in range(nranks):
        a, b = q * d.ucap, q * d.ucap + uc[q]
        assert (cnt[a:b] > 0).all() and cnt[b:(q + 1) * d.ucap].sum() == 0
        ref = g_at[a:b].cpu().numpy()
        for label, got in (("row atomics", ref), ("LDS atomics", g_b[a:b].cpu().numpy()),
                           ("sorted lists", g_s[a:b].cpu().numpy())):
            ratio = np.abs(got - G[a:b]) / eG[a:b]
            print(f"MARGIN fm reduce dim {dim} nranks {nranks} {label}: {ratio.max():.3f}")
            assert ratio.max() <= 1, (label, ratio.max())
        for got in (g_b[a:b].cpu().numpy(), g_s[a:b].cpu().numpy()):
            # fp32 sums in different orders (LDS atomics, sorted lists, global
            # atomics): a Zipf-head key sums hundreds of mixed-sign terms, so
            # a rare coordinate cancels to a few 1e-3 relative (seen: 1 of
            # 177701 at 2.6e-3); nearly all tight, every one loosely
            assert np.isclose(got, ref, rtol=2e-3, atol=2e-4).mean() > 0.9999
            np.testing.assert_allclose(got, ref, rtol=2e-2, atol=2e-3)
    np.testing.assert_allclose(l_b.sum().item(), l_at.sum().item(), rtol=1e-4)


def _fm_three_reduces(dev, keys, B, F, dim, seed):
    """One batch through the three FM gradient kernels: returns (dedup result,
    deduper, uvals, y, row-atomic / LDS-atomic / sorted-list gradients, ovf)."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.ops.dedup import Deduper

    h = hip()
    n = B * F
    rng = np.random.default_rng(seed)
    d = Deduper(n, nranks=1, gdim=dim, device=dev, mode="bucket")
    r = d(torch.from_numpy(keys).to(dev))
    st = torch.cuda.current_stream().cuda_stream
    U = d.ucap
    uvals = torch.from_numpy((rng.standard_normal((U, dim)) * 0.1).astype(np.float32)).to(dev)
    y = torch.from_numpy((rng.random(B) < 0.4).astype(np.float32)).to(dev)
    g_at = torch.zeros(U, dim, device=dev)
    h.fm_fwd_bwd(r.inv.data_ptr(), y.data_ptr(), B, F, dim, uvals.data_ptr(), g_at.data_ptr(),
                 0, 0, st)
    gs = torch.empty(B, device=dev)
    gss = torch.empty(B * (dim - 1), device=dev)
    h.fm_fwd_g(0, d.index_ptrs(n), y.data_ptr(), B, F, dim,
               uvals.data_ptr(), gs.data_ptr(), gss.data_ptr(), 0, 0, st)
    g_b = torch.full((U, dim), float("nan"), device=dev)
    h.bd_reduce_fm(n, 1, d.scratch.data_ptr(), d.pj.data_ptr(), d.luid.data_ptr(),
                   gs.data_ptr(), gss.data_ptr(), F, dim, uvals.data_ptr(), g_b.data_ptr(), st,
                   ndest=d.ndest)
    ovf = torch.zeros(h.bd_fm_ovf_words(n), dtype=torch.int32, device=dev)
    g_s = torch.full((U, dim), float("nan"), device=dev)
    h.bd_reduce_fm(n, 1, d.scratch.data_ptr(), d.pj.data_ptr(), d.luid.data_ptr(),
                   gs.data_ptr(), gss.data_ptr(), F, dim, uvals.data_ptr(), g_s.data_ptr(), st,
                   ovf.data_ptr(), ndest=d.ndest)
    torch.cuda.synchronize()
    d.check()
    return r, d, uvals, y, g_at, g_b, g_s, ovf


def _assert_fm_within_fp64_bound(label, r, uvals, y, B, F, grads):
    u = int(r.ucount[0])
    G, eG, cnt = _fm_grad_reference(r.inv, uvals, y, B, F)
    assert (cnt[:u] > 0).all() and cnt[u:].sum() == 0
    for kind, g in grads:
        ratio = np.abs(g[:u].cpu().numpy() - G[:u]) / eG[:u]
        print(f"MARGIN {label} {kind}: {ratio.max():.3f} (largest list {cnt.max()})")
        assert ratio.max() <= 1, (label, kind, ratio.max())


@pytest.mark.parametrize("dim", [2, 5, 9, 17])
def test_fm_sorted_reduce_overflow_buckets(dev, dim):
    """Sorted-list FM reduce with buckets too large to sort in LDS (a key
    with 30K occurrences): those go to the LDS-atomic form; all three kernels
    within the fp64 gradient's per-key bound, and the sorted form == the
    per-occurrence atomic kernel as before."""
    B, F = (16000, 8) if dim < 17 else (8000, 16)  # the forward needs F >= K lanes
    n = B * F
    rng = np.random.default_rng(17)
    keys = rng.integers(0, 1 << 40, size=n).astype(np.int64)
    keys[rng.random(n) < 0.25] = 12345  # ~32K occurrences of one key
    r, d, uvals, y, g_at, g_b, g_s, ovf = _fm_three_reduces(dev, keys, B, F, dim, 17)
    assert int(ovf[0]) >= 1  # the hot key's bucket overflowed
    u = int(r.ucount[0])
    _assert_fm_within_fp64_bound(f"fm overflow dim {dim}", r, uvals, y, B, F,
                                 (("row atomics", g_at), ("LDS atomics", g_b),
                                  ("sorted + overflow", g_s)))
    np.testing.assert_allclose(g_s[:u].cpu().numpy(), g_at[:u].cpu().numpy(), rtol=2e-3,
                               atol=5e-3)


@pytest.mark.parametrize("total", [10240, 10241])
def test_fm_sorted_reduce_bucket_boundary(dev, total):
    """A bucket of exactly kFmOcc = 10240 occurrences is sorted in LDS, one of
    10241 goes to the overflow list: both within the fp64 bound."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.ops.dedup import Deduper

    B, F, dim, hot = 16000, 8, 9, 12345
    n = B * F
    rng = np.random.default_rng(23)
    keys = rng.integers(0, 1 << 40, size=n).astype(np.int64)
    keys[0] = hot
    # where the hot key's bucket is, and what else falls into it
    d0 = Deduper(n, nranks=1, gdim=dim, device=dev, mode="bucket")
    d0(torch.from_numpy(keys).to(dev))
    torch.cuda.synchronize()
    bkt = d0.bkt[:n].cpu().numpy()
    others = int((bkt == bkt[0]).sum()) - 1
    assert 0 < others < total - 1000
    # more occurrences of the hot key, taken from other buckets, up to `total`
    free = np.nonzero(bkt != bkt[0])[0]
    keys[rng.choice(free, total - others - 1, replace=False)] = hot
    r, d, uvals, y, g_at, g_b, g_s, ovf = _fm_three_reduces(dev, keys, B, F, dim, total)
    P, o_bs, _, _ = hip().bd_offsets(d._lay(n), 1, d.ndest)
    bstart = d.scratch[o_bs:o_bs + P + 1].cpu().numpy().astype(np.int64)
    sizes = np.diff(bstart)
    assert sizes.max() == total and (sizes > 10240).sum() == int(total > 10240)
    assert int(ovf[0]) == int(total > 10240)
    _assert_fm_within_fp64_bound(f"fm bucket of {total}", r, uvals, y, B, F,
                                 (("row atomics", g_at), ("LDS atomics", g_b),
                                  ("sorted lists", g_s)))


def test_fm_trains_world1(dev):
    from swiftsnails_amd.models.fm import FMWorker, fm_table_args
    from swiftsnails_amd.models.sparse_lr import CtrSynth
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    data = CtrSynth(batch_size=4096, num_fields=16, num_features=100_000, tail_frac=0.0)
    opt, init = fm_table_args(8)
    table = HbmTable(9, 200_000, optimizer=opt, init=init, device=dev)
    eng = PSEngine(table, None, max_keys=4096 * 16, dim=9, device=dev)
    w = FMWorker(eng, data)
    losses = [float(w.step().sum().item()) / 4096 for _ in range(50)]
    table.check()
    assert np.mean(losses[-5:]) < np.mean(losses[:3]) - 0.02, losses


def test_word2vec_trains_world1(dev):
    from swiftsnails_amd.models.word2vec import W2VSynth, Word2VecWorker, make_w2v_table_args
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    data = W2VSynth(batch_size=2048, window=3, vocab=5000, noise=0.05)
    opt, init = make_w2v_table_args(64, None)
    table = HbmTable(64, 40000, optimizer=opt, init=init, device=dev)
    eng = PSEngine(table, None, max_keys=data.n_keys, dim=64, device=dev)
    w = Word2VecWorker(eng, data)
    losses = []
    for _ in range(40):
        w.step()
        losses.append(w.mean_loss())
    table.check()
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < 0.8 * np.mean(losses[:3]), losses


def _graph_worker(model, dev, **ek):
    from swiftsnails_amd.models.fm import FMWorker, fm_table_args
    from swiftsnails_amd.models.sparse_lr import CtrSynth, SparseLRWorker, make_lr_table
    from swiftsnails_amd.models.word2vec import W2VSynth, Word2VecWorker, make_w2v_table_args
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    if model == "lr":
        data = CtrSynth(batch_size=4096, num_fields=13, num_features=1_000_000, tail_frac=0.1)
        table = make_lr_table(data.num_features, 1, Optimizer("adagrad", lr=0.1), device=dev)
        eng = PSEngine(table, ek.pop("transport", None), max_keys=4096 * 13, dim=1, device=dev,
                       **ek)
        return SparseLRWorker(eng, data), table
    if model == "fm":
        data = CtrSynth(batch_size=2048, num_fields=16, num_features=100_000, tail_frac=0.1)
        opt, init = fm_table_args(8)
        table = HbmTable(9, 200_000, optimizer=opt, init=init, device=dev)
        eng = PSEngine(table, ek.pop("transport", None), max_keys=2048 * 16, dim=9, device=dev,
                       **ek)
        return FMWorker(eng, data), table
    data = W2VSynth(batch_size=1024, window=3, vocab=5000, noise=0.05,
                    mode="pairs" if model == "w2v_pairs" else "window")
    opt, init = make_w2v_table_args(64, None)
    table = HbmTable(64, 40000, optimizer=opt, init=init, device=dev)
    eng = PSEngine(table, ek.pop("transport", None), max_keys=data.n_keys, dim=64, device=dev, **ek)
    return Word2VecWorker(eng, data), table


def test_graph_capture_after_mode_switch_xgmi(dev):
    """N>1 path (a size-1 xGMI arena): pulled-ahead rounds, then synchronous
    ones (the launcher calibration's last switch), then the hipGraph capture.
    Synchronous rounds run the keys wait + server merge in their routes; the
    capture must start from a round routed that way (enable_graph settles one
    eager step), else every replay's first pull waits a second time on its
    slot's keys and the job hangs (here: a mailbox timeout).  (Graph tests run
    in a child process: tests/_mp.py in_child.)"""
    in_child(_graph_after_mode_switch_body, dev)


def _graph_after_mode_switch_body(dev):
    os.environ["SS_XGMI_TIMEOUT"] = "20"
    os.environ["SS_PULL_AHEAD"] = "auto"
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    torch.cuda.set_device(dev)
    w, t = _graph_worker("w2v", dev, transport=XgmiTransport(0, 1, dev, None))
    assert w.set_pull_ahead(True)
    for _ in range(3):
        w.step()
    w.set_pull_ahead(False)
    w.drain()
    assert w.enable_graph()
    assert w.engine.last_route_matches()
    for _ in range(3 * w._gper):
        w.step()
    torch.cuda.synchronize()
    w.engine.check()
    t.check()
    assert np.isfinite(w.mean_loss())


def test_graph_teardown_then_replay_same_process(dev, monkeypatch):
    """The hipGraph teardown order: a worker with captured graphs
    on the N>1 path (a size-1 xGMI arena: mailbox puts / waits and the round
    engine's events in the graph) is dropped inside a reference cycle
    without close(), and the cyclic GC collects it while a second worker's
    graphs are replaying in the same process.  The graphs are reset before the engine's events and
    arenas go away (models/base.py _GraphSet), so the replays go on and the
    second worker trains; the first worker's graphs trained as well."""
    import gc

    monkeypatch.setenv("SS_XGMI_TIMEOUT", "20")
    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    torch.cuda.set_device(dev)
    a, ta = _graph_worker("lr", dev, transport=XgmiTransport(0, 1, dev, None))
    first = [float(a.step().sum().item()) for _ in range(2)]
    assert a.enable_graph()
    for _ in range(3 * a._gper):
        a.step()
    torch.cuda.synchronize()
    a.engine.check()
    ta.check()
    assert np.isfinite(a.mean_loss()) and a.mean_loss() < first[0]
    a.cycle = a  # only the cyclic GC can free it now
    del a, ta
    b, tb = _graph_worker("lr", dev)
    b.step()
    assert b.enable_graph()
    for i in range(4 * b._gper):
        b.step()
        if i == b._gper:
            gc.collect()  # the first worker goes while these replays run
    torch.cuda.synchronize()
    tb.check()
    b.engine.check()
    assert np.isfinite(b.mean_loss()) and 0 < b.mean_loss() < 0.7
    b.close()  # explicit teardown; eager steps still work afterwards
    b.step()
    torch.cuda.synchronize()
    assert np.isfinite(b.mean_loss())


@pytest.mark.parametrize("occ", ["own", "arena"])
def test_record_exchange_world1_matches_unique(dev, monkeypatch, occ):
    """The record exchange (every occurrence shipped; the server dedups what
    it receives, fills a row per occurrence and merges the per-occurrence
    gradients with the AdaGrad update fused — no worker dedup or merge)
    through a size-1 xGMI arena trains like the unique-key exchange on the
    same path: the same keys, the same losses and parameters up to float
    summation order (SS_REC_OCC: own = the own records' rows in a cached
    buffer and their gradients read through spj by the server merge; arena =
    through the mailbox).  Graph tests run in a child process (tests/_mp.py)."""
    in_child(_record_exchange_body, dev, occ)


def _record_exchange_body(dev, occ):
    os.environ["SS_ENGINE_GENERAL"] = "xgmi"
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_REC_OCC"] = occ
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    torch.cuda.set_device(dev)
    out = {}
    for ex in ("unique", "records"):
        w, t = _graph_worker("lr", dev, transport=XgmiTransport(0, 1, dev, None), exchange=ex)
        assert w.engine.records == (ex == "records")
        assert (w.gring is not None) == (ex == "records" and occ == "own")
        losses = [float(w.step().sum().item()) for _ in range(12)]
        torch.cuda.synchronize()
        w.engine.check()
        t.check()
        out[ex] = (losses, t.to_dict(with_state=True))
        if ex == "records":  # the record round captured as hipGraphs
            assert w.enable_graph()
            for _ in range(2 * w._gper):
                w.step()
            torch.cuda.synchronize()
            w.engine.check()
            t.check()
            assert np.isfinite(w.mean_loss()) and 0 < w.mean_loss() < 0.7
    _assert_trains_like(out["unique"], out["records"])


def _assert_trains_like(ref, got):
    """``got`` = (per-step losses, table dict with state) of a run that sums
    the same gradients as ``ref`` in another order."""
    (lu, tu), (lr_, tr) = ref, got
    np.testing.assert_allclose(lr_, lu, rtol=1e-4, atol=1e-5)
    assert tr.keys() == tu.keys()
    ks = list(tu.keys())
    a, b = np.stack([tu[k] for k in ks]), np.stack([tr[k] for k in ks])
    # rows [w, h]: rtol 1e-3, atol 1e-5 — and, for w, the conditioning of the
    # AdaGrad step lr * g / sqrt(h + eps): its slope in g is lr / sqrt(h + eps),
    # so where a key's occurrences' gradients cancel (g^2 ~ h below eps = 1e-8:
    # one such key in this data, h = 1.6e-9) the last bits of g decide w.  g is
    # a sum of a few terms of magnitude < 1, each known to an ulp: 8 * 2^-24
    # bounds its error (two runs of the SAME exchange differed by 1-2 * 2^-24
    # there, 4.7e-5 / 9.5e-5 in w, and by one ulp of w, 6e-8, in every other
    # row); for a row with h >= 1 the term adds < 5e-8
    lr, eps = 0.1, 1e-8  # _graph_worker's optimizer
    tol = 1e-5 + 1e-3 * np.abs(a)
    tol[:, 0] += lr * 8 * 2.0 ** -24 / np.sqrt(np.minimum(a[:, 1], b[:, 1]) + eps)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a[:, 1] >= 0).all()
    bad = np.abs(b - a) > tol
    assert not bad.any(), (int(bad.sum()), a[bad.any(1)][:5], b[bad.any(1)][:5])


def test_srv_fill_separate_matches_fused(dev, tmp_path):
    """The claimed server pull of scalar rows with its response fill as a
    separate kernel (SS_SRV_FILL_FUSED=0: k_pull_claim_bk writes the looked-up
    rows, k_bd_fill_occ the row per received position) trains like the default,
    the fill fused into the pull — sparse LR, unique exchange, through a size-1
    xGMI arena; held to the record-exchange test's tolerance.  The knob is read
    once per process (RoundEngine), so each setting runs in a process of its own."""
    runs = []
    for fused in ("1", "0"):
        path = str(tmp_path / f"fill{fused}.npz")
        in_child(_srv_fill_body, dev, fused, path, always=True)
        z = np.load(path)
        runs.append((list(z["losses"]), dict(zip(z["keys"].tolist(), z["rows"]))))
    _assert_trains_like(runs[0], runs[1])


def _srv_fill_body(dev, fused, path):
    os.environ["SS_ENGINE_GENERAL"] = "xgmi"
    os.environ["SS_PULL_AHEAD"] = "0"
    os.environ["SS_SRV_FILL_FUSED"] = fused
    os.environ["SS_XGMI_TIMEOUT"] = "30"
    from swiftsnails_amd.parallel.xgmi import XgmiTransport

    torch.cuda.set_device(dev)
    w, t = _graph_worker("lr", dev, transport=XgmiTransport(0, 1, dev, None))
    assert w.engine.claim and w.engine.claim_rounds  # the server pulls claim
    losses = [float(w.step().sum().item()) for _ in range(12)]
    torch.cuda.synchronize()
    w.engine.check()
    t.check()
    d = t.to_dict(with_state=True)
    ks = sorted(d)
    np.savez(path, losses=np.array(losses), keys=np.array(ks, dtype=np.uint64),
             rows=np.stack([d[k] for k in ks]))
    w.close()


def test_lr_slot32_matches_slot64(dev, monkeypatch):
    """One-GPU sparse LR with the pull storing 4-byte slot indices for the
    fused merge + AdaGrad update (default, shards under 2^31 slots) trains
    exactly like 8-byte slots: same per-step losses, same table."""
    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    out = {}
    for s32 in ("1", "0"):
        monkeypatch.setenv("SS_SLOT32", s32)
        w, t = _graph_worker("lr", dev)
        assert w.engine.slot32 == (s32 == "1")
        w.step()
        # zero-initialised weights: every logit 0, the first step's loss is
        # ln 2 per sample — moved out of the forward's accumulator by the
        # merge kernel, which leaves the accumulator zero
        assert abs(w.mean_loss() - np.log(2.0)) < 1e-4
        assert float(w._acc.abs().sum()) == 0.0
        losses = [float(w.step().sum().item()) for _ in range(6)]
        torch.cuda.synchronize()
        t.check()
        out[s32] = (losses, t.to_dict(with_state=True))
    (l1, d1), (l0, d0) = out["1"], out["0"]
    np.testing.assert_allclose(l1, l0, rtol=1e-5, atol=1e-6)
    assert d1.keys() == d0.keys()
    ks = list(d0.keys())
    np.testing.assert_allclose(np.stack([d1[k] for k in ks]), np.stack([d0[k] for k in ks]),
                               rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("model", ["lr", "fm", "w2v", "w2v_pairs"])
def test_hipgraph_replay_matches_eager(dev, model):
    """hipGraph replays (one graph per ring phase, device step counter for
    the generator) train exactly like eager steps: same per-step losses and
    the same table (up to float-atomic summation order).  Pull-ahead is off
    here: with it, which of round i's updates round i+1 reads depends on
    timing (staleness 1), in eager mode as much as in graphs.  (In a child
    process: tests/_mp.py in_child.)"""
    in_child(_replay_matches_eager_body, dev, model)


def _replay_matches_eager_body(dev, model):
    os.environ["SS_PULL_AHEAD"] = "0"
    torch.cuda.set_device(dev)
    wb, tb = _graph_worker(model, dev)
    lb = [float(wb.step().sum().item())]
    assert wb.enable_graph()
    per = wb._gper  # steps per graph (SS_GRAPH_STEPS; default 4 ring periods)
    n = 1 + 3 * per
    lb += [float(wb.step().sum().item()) for _ in range(n - 1)]
    wa, ta = _graph_worker(model, dev)
    la = [float(wa.step().sum().item()) for _ in range(n)]
    torch.cuda.synchronize()
    ta.check()
    tb.check()
    # a multi-step graph (SS_GRAPH_STEPS) leaves the loss of its last step
    idx = [0] + [k for k in range(1, n) if (k - 1) % per == per - 1]
    np.testing.assert_allclose(np.array(lb)[idx], np.array(la)[idx], rtol=2e-4, atol=1e-3)
    da, db = ta.to_dict(), tb.to_dict()
    assert da.keys() == db.keys()
    ks = list(da.keys())[:5000]
    a, b = np.stack([da[k] for k in ks]), np.stack([db[k] for k in ks])
    # float-atomic summation order differs between any two runs; AdaGrad's
    # division by a still-small accumulator amplifies it for a rare
    # coordinate: a near-zero summed gradient whose sign depends on the order
    # moves the weight by +-lr on its first update (seen: 1 of 320000 off by
    # 0.05 at lr 0.05).  So: nearly all coordinates tight, and every
    # coordinate within the largest AdaGrad excursion, |step| <= lr per round
    assert np.isclose(b, a, rtol=1e-3, atol=5e-4).mean() >= 0.9995
    np.testing.assert_allclose(b, a, rtol=0, atol=2 * ta.opt.lr * n)


@pytest.mark.parametrize("model", ["fm", "w2v", "w2v_pairs"])
def test_hipgraph_pull_ahead_trains(dev, model):
    """Graph replays of the pull-ahead pipeline (rows of round i+1 pulled on
    the route stream while round i computes) keep training.  (In a child
    process: tests/_mp.py in_child.)"""
    in_child(_pull_ahead_trains_body, dev, model)


def _pull_ahead_trains_body(dev, model):
    torch.cuda.set_device(dev)
    w, t = _graph_worker(model, dev)
    assert w.engine.pull_ahead
    first = [float(w.step().sum().item()) for _ in range(3)]
    assert w.enable_graph()
    last = [float(w.step().sum().item()) for _ in range(30)]
    torch.cuda.synchronize()
    t.check()
    assert np.isfinite(last).all()
    assert np.mean(last[-5:]) < np.mean(first), (first, last[-5:])


@pytest.mark.parametrize("D,B,W", [(128, 1000, 5), (32, 640, 2), (64, 4096, 15)])
def test_word2vec_window_grad_reduce_matches_atomics(dev, monkeypatch, D, B, W):
    """Window tile gradients as occurrence rows summed per unique key
    (k_w2v_osort + k_w2v_oreduce: counting sort per dedup bucket, one wave per
    <= 32-occurrence item, shared window rows through the tail buffer, Zipf
    heads split over several items) == the tile's own row atomics; the
    per-step loss moved out of the zeroed accumulator by the reduce == the
    zero-filled one.  Partial
    last tile (B % 64 != 0), W from 2 to the maximum 15.  (The atomic form
    is what a non-bucketed dedup, SS_DEDUP=hash, runs.)"""
    from swiftsnails_amd.models.word2vec import W2VSynth, Word2VecWorker, make_w2v_table_args
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    out = {}
    for mode in ("reduce", "atomic"):
        monkeypatch.setenv("SS_DEDUP", "bucket" if mode == "reduce" else "hash")
        data = W2VSynth(batch_size=B, window=W, vocab=3000, noise=0.05, mode="window")
        opt, init = make_w2v_table_args(D, None)
        t = HbmTable(D, 40000, optimizer=opt, init=init, device=dev)
        eng = PSEngine(t, None, max_keys=data.n_keys, dim=D, device=dev)
        w = Word2VecWorker(eng, data)
        assert w.occ_reduce == (mode == "reduce")
        losses = []
        for _ in range(5):
            w.step()
            losses.append(w.mean_loss())
        torch.cuda.synchronize()
        t.check()
        if mode == "reduce":  # k_w2v_oreduce handed the accumulators off and zeroed them
            assert w._out is not w._acc and float(w._acc.abs().sum()) == 0.0
        out[mode] = (losses, t.to_dict(with_state=True))
    (lr, tr), (la, ta) = out["reduce"], out["atomic"]
    np.testing.assert_allclose(lr, la, rtol=1e-4)
    assert tr.keys() == ta.keys()
    ks = list(tr.keys())
    a, b = np.stack([ta[k] for k in ks]), np.stack([tr[k] for k in ks])
    assert np.isclose(b, a, rtol=1e-3, atol=5e-4).mean() > 0.9999
    np.testing.assert_allclose(b, a, rtol=5e-2, atol=2e-2)


@pytest.mark.parametrize("comms", [1, 3])
@pytest.mark.parametrize("model", ["lr", "fm", "w2v"])
def test_general_path_rccl_world1_matches_loopback(dev, model, comms, monkeypatch):
    """The N>1 engine path (send segments, count exchange with pinned D2H,
    bucket runs, the server's merge of received keys and merged update) on
    one GPU through real size-1 RCCL communicators — one on its comm stream
    (SS_RCCL_COMMS=1) or three on the engine's streams (3) — trains exactly
    like the same path over loopback transports: the multi-GPU RCCL call
    sequence, minus peers."""
    monkeypatch.setenv("SS_ENGINE_GENERAL", "1")
    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    n = 12
    wa, ta = _graph_worker(model, dev)
    assert not wa.engine.fast1
    la = [float(wa.step().sum().item()) for _ in range(n)]
    wb, tb = _graph_worker(model, dev, **_rccl1(dev, comms))
    lb = [float(wb.step().sum().item()) for _ in range(n)]
    torch.cuda.synchronize()
    ta.check()
    tb.check()
    np.testing.assert_allclose(lb, la, rtol=2e-4, atol=1e-3)
    assert ta.size() == tb.size()


def _rccl1(dev, comms=1):
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.parallel.transport import RcclTransport

    if comms == 1:
        t = RcclTransport(0, 1, dev, uid=hip().RcclComm.unique_id())
        assert t.nranks() == 1
        return {"transport": t}
    t, c, p = (RcclTransport(0, 1, dev, uid=hip().RcclComm.unique_id(), serial=False)
               for _ in range(3))
    return {"transport": t, "count_transport": c, "pull_transport": p}


@pytest.mark.parametrize("comms", [1, 3])
@pytest.mark.parametrize("model", ["lr", "fm", "w2v"])
def test_general_path_rccl_world1_pull_ahead_trains(dev, model, comms, monkeypatch):
    """The production N>1 pipeline — pull-ahead of round i+1 on a third
    stream while round i computes, the server's update a read-modify-write —
    on one GPU through size-1 RCCL communicators: trains and keeps the table
    sane."""
    monkeypatch.setenv("SS_ENGINE_GENERAL", "1")
    monkeypatch.setenv("SS_PULL_AHEAD", "1")  # LR runs synchronous rounds by default
    w, t = _graph_worker(model, dev, **_rccl1(dev, comms))
    assert w.engine.pull_ahead and w.engine.pull_stream is not None
    losses = [float(w.step().sum().item()) for _ in range(40)]
    torch.cuda.synchronize()
    t.check()
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:3]), losses


@pytest.mark.parametrize("pull_stream", ["0", "1"])
def test_fm_trains_with_pull_ahead_staleness_bound(dev, monkeypatch, pull_stream):
    """FM pulls round i+1 ahead on a side stream (the route stream, or its own
    with SS_PULL_STREAM=1), bounded to staleness exactly 1 (the pull waits for
    round i-1's push) — trains on both.  (Unbounded, a side stream running
    ahead read several rounds stale: on the bench configuration FM's loss then
    stayed at chance, 0.69; at this small size the unbounded run still trains,
    with larger early swings: 0.90 / 0.98 vs 0.64 / 0.77.)"""
    from swiftsnails_amd.models.fm import FMWorker, fm_table_args
    from swiftsnails_amd.models.sparse_lr import CtrSynth
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_STREAM", pull_stream)
    data = CtrSynth(batch_size=16384, num_fields=39, num_features=2_000_000, tail_frac=0.1)
    opt, init = fm_table_args(8)
    table = HbmTable(9, 4_000_000, optimizer=opt, init=init, device=dev)
    eng = PSEngine(table, None, max_keys=16384 * 39, dim=9, device=dev)
    w = FMWorker(eng, data)
    assert eng.pull_ahead and eng.staleness == 1
    assert (eng.pull_stream is not None) == (pull_stream == "1")
    losses = []
    for _ in range(60):
        w.step()
        losses.append(w.mean_loss())
    torch.cuda.synchronize()
    table.check()
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < min(0.66, np.mean(losses[5:10]) - 0.01), losses


def _bench_1gpu(extra):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, cwd=root,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_graph_mode_times_whole_periods():
    """bench.py --graph on: the timed region runs exactly --steps steps.  With
    16 timed steps the graph holds 16 steps (2 ring periods of the one-GPU
    8-slot ring, or 4 of a 4-slot one) and the warm-up one graph, so the job
    runs warmup + 16 + 16 steps in all — the same training as an eager run of
    warmup + 32 steps (identical final loss)."""
    base = ["--batch", "4096", "--features", "2000000", "--warmup", "3"]
    g = _bench_1gpu(base + ["--steps", "16", "--graph", "on"])
    e = _bench_1gpu(base + ["--steps", "32"])
    assert g["config"]["hipgraph"] is True and e["config"]["hipgraph"] is False
    assert g["steps"] == 16 and g["ms_per_step"] > 0
    assert g["config"]["loss_last"] == pytest.approx(e["config"]["loss_last"], rel=1e-4, abs=1e-5)


def test_bench_dump_outputs_repeatable(tmp_path):
    """bench.py --dump-outputs: the last timed step's loss and the trained
    rows of its keys as .npy files (float32 / float64), the same keys from run
    to run (seeded inputs) and the same rows and loss up to the order of the
    fp32 sums (duplicate merge, loss shards).

    Row tolerance: a key's gradient g = sum (p_i - y_i) is known to a few
    ulp of 1 (the order of the sum, and p through the ulp-level differences
    of the 39 weights under it: 8 * 2^-24 bounds it with room).  AdaGrad
    steps by lr * g / sqrt(h + eps), h >= g^2, whose slope in g is at most
    lr / sqrt(eps) — reached by a key whose occurrences' gradients cancel
    (labels 0 and 1 at p ~ 0.5) — so two correct runs may differ by
    lr / sqrt(eps) * 8 * 2^-24 = 2.4e-4 in such a row.  A wrong row (another
    key's, a lost update) is off by the step size lr = 0.05, 200 times that."""
    base = ["--batch", "4096", "--features", "2000000", "--warmup", "2", "--steps", "4"]
    runs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        j = _bench_1gpu(base + ["--dump-outputs", d])
        assert sorted(os.listdir(d)) == ["loss_sum.npy", "weight_keys.npy", "weights.npy"]
        out = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
        n = 4096 * 39
        assert out["loss_sum"].dtype == np.float64 and out["loss_sum"].shape == (1,)
        assert out["weight_keys"].dtype == np.float64 and out["weight_keys"].shape == (n,)
        assert out["weights"].dtype == np.float32 and out["weights"].shape == (n, 1)
        assert j["steps"] == 4 and j["ms_per_step"] > 0
        # the dumped loss is the last step's (the JSON line rounds its mean to 1e-5)
        assert out["loss_sum"][0] / 4096 == pytest.approx(j["config"]["loss_last"], abs=1.1e-5)
        k = out["weight_keys"]
        assert (k >= 0).all() and (k < 2000000).all() and (k == np.floor(k)).all()
        # every key of the batch was trained: its row exists and has moved off
        # the (u - 0.5) * 0.01 initialiser's range somewhere
        assert np.isfinite(out["weights"]).all() and np.abs(out["weights"]).max() > 0.005
        runs.append(out)
    a, b = runs
    np.testing.assert_array_equal(a["weight_keys"], b["weight_keys"])
    lr, eps = 0.05, 1e-8  # bench.py --lr, Optimizer.eps
    np.testing.assert_allclose(a["weights"], b["weights"], rtol=0,
                               atol=lr / np.sqrt(eps) * 8 * 2.0 ** -24)
    np.testing.assert_allclose(a["loss_sum"], b["loss_sum"], rtol=1e-4)


def _planted_corpus(path, clusters=20, words=40, sentences=6000, length=12, seed=5):
    """Sentences of one cluster each: word ids c*1000 + i (i < words)."""
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for _ in range(sentences):
            c = int(rng.integers(clusters))
            ids = c * 1000 + rng.integers(0, words, size=length)
            f.write(" ".join(str(int(x)) for x in ids) + "\n")
    return clusters, words


@pytest.mark.parametrize("mode,neg_mode,tile,rows", [("window", "shared", "bf16", "fp32"),
                                                     ("pairs", "shared", "bf16", "fp32"),
                                                     ("pairs", "shared", "f32", "fp32"),
                                                     ("window", "per_pair", "f32", "fp32"),
                                                     ("window", "shared", "bf16", "bf16"),
                                                     ("window", "per_pair", "f32", "bf16")])
def test_word2vec_learns_planted_clusters(dev, tmp_path, monkeypatch, mode, neg_mode, tile, rows):
    """Embedding quality, not just a falling loss: on a corpus whose
    sentences each draw from one of 20 word clusters, the learned input
    vectors of words of the same cluster are far more similar (cosine) than
    of words of different clusters — for every objective variant: the
    shared-negative tile (window layout: bf16 MFMA; pairs layout: bf16 and
    fp32 MFMA) and per-pair negatives (classic SGNS, fp32 dot products), on
    fp32 rows and on compact bf16 rows (row_dtype: bf16: updated in fp32 by the
    fused reduce, stored with stochastic rounding)."""
    from swiftsnails_amd.models.word2vec import Word2VecWorker, make_w2v_table_args
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine
    from swiftsnails_amd.utils.dataio import FileCorpusSource

    monkeypatch.setenv("SS_W2V_MFMA", tile)
    C, M = _planted_corpus(tmp_path / "corpus.txt")
    data = FileCorpusSource(str(tmp_path / "corpus.txt"), batch_size=2048, window=4,
                            negatives=5, mode=mode, neg_mode=neg_mode, device=dev)
    opt, init = make_w2v_table_args(64, None)
    table = HbmTable(64, 1 << 14, optimizer=opt, init=init, device=dev, row_dtype=rows)
    eng = PSEngine(table, None, max_keys=data.n_keys, dim=64, device=dev)
    w = Word2VecWorker(eng, data)
    assert w.mfma_bf16 == (tile == "bf16") and w.per_pair == (neg_mode == "per_pair")
    assert getattr(w, "fuse", True)  # the reduce runs the update, fp32 or bf16 rows
    for _ in range(3 * data.steps_per_pass()):  # 3 passes
        w.step()
    torch.cuda.synchronize()
    table.check()
    ids = torch.tensor([c * 1000 + i for c in range(C) for i in range(M)], device=dev)
    v, _ = table.pull(ids, insert=False)
    v = torch.nn.functional.normalize(v.double(), dim=1).cpu().numpy()
    sim = v @ v.T
    lab = np.repeat(np.arange(C), M)
    same = lab[:, None] == lab[None, :]
    off = ~np.eye(len(lab), dtype=bool)
    within, across = sim[same & off].mean(), sim[~same].mean()
    assert within - across > 0.4, (within, across)
    # nearest neighbour of almost every word is in its own cluster
    np.fill_diagonal(sim, -2)
    assert (lab[sim.argmax(1)] == lab).mean() > 0.95


@pytest.mark.parametrize("row_dtype", ["fp32", "bf16"])
def test_fm_learns_planted_model_auc(dev, row_dtype):
    """FM held-out AUC against the planted model the labels come from (not
    only a falling loss), with full fp32 rows and with compact bf16 rows
    (config 5's capacity option): both learn to within 10% of the
    Bayes-optimal AUC, and compact rows lose < 0.01 AUC against fp32."""
    from swiftsnails_amd.models.fm import FMWorker, fm_table_args
    from swiftsnails_amd.models.sparse_lr import CtrSynth
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    res = {}
    for dt in sorted({"fp32", row_dtype}):
        data = CtrSynth(batch_size=4096, num_fields=16, num_features=16 * 4000, tail_frac=0.0,
                        truth_scale=4.0)
        opt, init = fm_table_args(8)
        opt.lr = 0.2
        table = HbmTable(9, 1 << 17, optimizer=opt, init=init, device=dev, row_dtype=dt)
        eng = PSEngine(table, None, max_keys=4096 * 16, dim=9, device=dev)
        w = FMWorker(eng, data)
        for _ in range(150):
            w.step()
        table.check()
        res[dt] = w.evaluate(batches=2)
    r = res[row_dtype]
    assert r["auc_truth"] > 0.8
    assert r["auc"] > 0.9 * r["auc_truth"], res
    assert r["auc"] > res["fp32"]["auc"] - 0.01, res


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("neg_mode", ["shared", "per_pair"])
def test_w2v_fused_update_matches_apply(dev, monkeypatch, neg_mode, opt):
    """One-GPU word2vec with the optimizer update fused into the occurrence-row
    reduce (every key whose gradient row is one reduce item; the apply kernel
    masked to the keys summed over several items) trains like the reduce +
    apply pair (SS_W2V_FUSE=0): the same sums and update, up to the order of
    the hot keys' row atomics (run-to-run float noise, ~1e-6 relative).  SGD
    keeps that noise at its size (a few coordinates near cancellation: 2e-5).  AdaGrad's
    first step moves a coordinate by lr * sign(g), so a near-zero gradient
    whose sign the noise flips differs by up to 2 lr (a few hundred of 1.4M
    coordinates): 99.9 % within 1e-4, and no coordinate beyond 2 lr."""
    from swiftsnails_amd.models.word2vec import W2VSynth, Word2VecWorker, make_w2v_table_args
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    lr = 0.05
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("SS_W2V_FUSE", fuse)
        data = W2VSynth(batch_size=2048, window=3, vocab=20000, noise=0.05, mode="window",
                        neg_mode=neg_mode, negatives=5)
        opt_, init = make_w2v_table_args(64, Optimizer(opt, lr=lr))
        table = HbmTable(64, 200_000, optimizer=opt_, init=init, device=dev)
        eng = PSEngine(table, None, max_keys=data.n_keys, dim=64, device=dev)
        w = Word2VecWorker(eng, data)
        assert (w.uhot is not None) == (fuse == "1")
        losses = [None] * 0
        for _ in range(8):
            w.step()
            losses.append(w.mean_loss())
        torch.cuda.synchronize()
        table.check()
        out[fuse] = (losses, table.to_dict(with_state=True))
    (l1, t1), (l0, t0) = out["1"], out["0"]
    assert t1.keys() == t0.keys()
    np.testing.assert_allclose(np.array(l1), np.array(l0), rtol=1e-5)
    ks = list(t0)
    a, b = np.stack([t1[k] for k in ks]), np.stack([t0[k] for k in ks])
    if opt == "sgd":
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4)
    else:
        close = np.isclose(a, b, rtol=1e-4, atol=1e-7)
        assert close.mean() > 0.999, (close.size - close.sum(), close.size)
        assert np.abs(a - b).max() <= 2 * lr + 1e-3


def _osort_inputs(dev, keys):
    """A bucket ``Deduper`` over ``keys`` and ``k_w2v_osort`` on its layout:
    (deduper, uid of every key position, items [n, 4], ord [n], uhot [n])."""
    from swiftsnails_amd._native import hip
    from swiftsnails_amd.ops.dedup import Deduper

    n = len(keys)
    dd = Deduper(n, device=dev, mode="bucket", with_grad=False)
    dd(torch.from_numpy(keys.view(np.int64)).to(dev))
    _, bstart, unum, ubase, P = dd.bucket_view(n)
    assert P >= 3
    order = torch.full((n,), -1, dtype=torch.int32, device=dev)
    items = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
    uhot = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    hip().w2v_osort(P, bstart, unum, ubase, dd.pj.data_ptr(), dd.luid.data_ptr(),
                    order.data_ptr(), items.data_ptr(), torch.cuda.current_stream().cuda_stream,
                    uhot.data_ptr())
    torch.cuda.synchronize()
    dd.check()
    uid = dd.unique_ids(n).cpu().numpy()
    return dd, uid, items, order, uhot


def _check_osort(keys, uid, items, order, uhot):
    """``items`` / ``ord`` / ``uhot`` against the keys alone; returns each
    key position's item index."""
    n = len(keys)
    it, od, uh = items.cpu().numpy().view(np.uint32), order.cpu().numpy(), uhot.cpu().numpy()
    u, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    assert (uid >= 0).all() and len(np.unique(uid)) == len(u)
    first = np.zeros(len(u), np.int64)
    first[inv] = uid                      # one uid per key
    assert np.array_equal(first[inv], uid)
    live = it[:, 1] > 0
    assert not it[~live].any()            # the unused item slots are zero
    assert it[live, 1].max() <= 32        # no item exceeds 32 occurrences
    seen = np.zeros(n, np.int64)
    item_of = np.full(n, -1, np.int64)
    nit = np.zeros(len(u), np.int64)
    for s in np.nonzero(live)[0]:
        x, c, z, f = (int(v) for v in it[s])
        pos = np.array([x]) if f & 2 else od[x:x + c]
        assert (uid[pos] == z).all()      # an item holds one key's occurrences
        k = inv[pos[0]]
        seen[pos] += 1
        item_of[pos] = s
        nit[k] += 1
        # flag 2: exactly the single occurrences, the item carrying the position itself
        assert bool(f & 2) == (cnt[k] == 1) and (not f & 2 or c == 1)
        assert bool(f & 1) == (cnt[k] > 32)                            # flag 1: several items
    assert (seen == 1).all()              # every occurrence position in exactly one item
    assert np.array_equal(nit, -(-cnt // 32))
    assert np.array_equal(uh[first].astype(bool), cnt > 32)   # uhot exactly on those keys
    return item_of


def _w2v_reduce_body(D, form):
    """``k_w2v_oreduce`` (window form, or the scaled per-pair form of this
    process's ``SS_W2V_PP_ITEMS``) on random rows against ``np.add.at`` in
    fp64, within ``n 2^-24 sum |row|`` per coordinate."""
    import _w2v_oracle as O
    from swiftsnails_amd._native import hip

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(D)
    window = form == "window"
    d = O.data("w2v_win" if window else "w2v_pp/w5k5")
    sp, B, W, R = d.sp, d.sp.B, d.sp.W, d.sp.R
    for t in (0, 1):   # even steps: counts 1 .. 65; odd steps: the 300-occurrence key too
        keys = d.keys[t]
        n = len(keys)
        assert {1, 2, 31, 32, 33} <= set(d.plan[t]) and (t == 0 or O.HOT in d.plan[t])
        dd, uid, items, order, uhot = _osort_inputs(dev, keys)
        _check_osort(keys, uid, items, order, uhot)
        nu = int(uid.max()) + 1
        rows = n if window else B + R
        og = (rng.standard_normal((rows, D)) * 0.5).astype(np.float32)
        ntail = max(1, (sp.tiles - 1) * 2 * W)
        ot = (rng.standard_normal((ntail, D)) * 0.5).astype(np.float32)
        acc = rng.standard_normal(2 * 64).astype(np.float32)
        t_og, t_ot, t_acc = (torch.from_numpy(a).to(dev) for a in (og, ot, acc))
        t_out = torch.full_like(t_acc, 3.0)
        ug = torch.zeros((n, D), device=dev)   # (a several-item key's row atomics add into zeros)
        ref, mag, terms = np.zeros((nu, D)), np.zeros((nu, D)), np.zeros(nu)
        np.add.at(ref, uid[:rows], og.astype(np.float64))
        np.add.at(mag, uid[:rows], np.abs(og).astype(np.float64))
        np.add.at(terms, uid, 1)
        st = torch.cuda.current_stream().cuda_stream
        if window:
            q = np.arange(R)
            tail = (q >= 64) & (q % 64 < 2 * W) & (q // 64 <= sp.tiles - 1)
            tq = (q // 64 - 1) * 2 * W + q % 64
            assert tail.sum() == ntail and sorted(tq[tail]) == list(range(ntail))
            np.add.at(ref, uid[B + q[tail]], ot[tq[tail]].astype(np.float64))
            np.add.at(mag, uid[B + q[tail]], np.abs(ot[tq[tail]]).astype(np.float64))
            np.add.at(terms, uid[B + q[tail]], 1)
            hip().w2v_oreduce(items.data_ptr(), n, order.data_ptr(), t_og.data_ptr(),
                              t_ot.data_ptr(), B, W, D, ug.data_ptr(), st, acc=t_acc.data_ptr(),
                              acc_out=t_out.data_ptr(), acc_n=t_acc.numel())
        else:
            uv = (rng.standard_normal((nu, D)) * 0.5).astype(np.float32)
            nneg = n - rows
            gn = rng.random(nneg).astype(np.float32)
            cen = uid[rng.integers(0, B, nneg)].astype(np.uint32)
            dead = rng.random(nneg) < 0.1           # negatives of pairs that are not valid
            gn[dead], cen[dead] = 0.0, 0xFFFFFFFF
            gnc = np.stack([gn, cen.view(np.float32)], 1)
            live = ~dead
            term = gn[live, None].astype(np.float64) * uv[cen[live].astype(np.int64)]
            np.add.at(ref, uid[rows:][live], term)
            np.add.at(mag, uid[rows:][live], np.abs(term))
            t_uv, t_gnc = torch.from_numpy(uv).to(dev), torch.from_numpy(gnc).to(dev)
            hip().w2v_oreduce(items.data_ptr(), n, order.data_ptr(), t_og.data_ptr(), 0, B, W, D,
                              ug.data_ptr(), st, gnc=t_gnc.data_ptr(), negbase=rows,
                              uvals=t_uv.data_ptr(), acc=t_acc.data_ptr(),
                              acc_out=t_out.data_ptr(), acc_n=t_acc.numel())
        torch.cuda.synchronize()
        # the accumulator hand-off is exact: moved, and left zero
        assert np.array_equal(t_out.cpu().numpy(), acc) and not t_acc.cpu().numpy().any()
        got = ug.cpu().numpy()[:nu].astype(np.float64)
        assert not ug.cpu().numpy()[nu:].any()
        tol = (terms + 1)[:, None] * 2.0 ** -24 * mag
        err = np.abs(got - ref)
        assert not err[tol == 0].any()
        r = (err / np.where(tol > 0, tol, 1.0)).max()
        print(f"MARGIN oreduce {form} D {D} step {t} PP_ITEMS "
              f"{os.environ.get('SS_W2V_PP_ITEMS', '2')}: max |kernel - fp64| / bound {r:.3f}")
        assert r <= 1, (form, D, t, r)


def _w2v_reduce_child(dims, form, items):
    os.environ["SS_W2V_PP_ITEMS"] = items   # read at the first launch of this process
    for D in dims:
        _w2v_reduce_body(D, form)


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("form", ["window", "per_pair"])
def test_w2v_osort_oreduce_match_fp64_sums(dev, monkeypatch, D, form):
    """The sort and the reduce alone: ``k_w2v_osort``'s items / ord / uhot
    checked against the keys (occurrence counts 1, 2, 31, 32, 33, 64, 65 and
    300 over several buckets, tail rows at B = 200, W = 5), then
    ``k_w2v_oreduce`` (window form) and ``k_w2v_oreduce_pp2`` (the per-pair
    form's default) against fp64 sums."""
    monkeypatch.delenv("SS_W2V_PP_ITEMS", raising=False)
    _w2v_reduce_body(D, form)


def test_w2v_oreduce_scaled_one_item_per_half_wave():
    """``k_w2v_oreduce<D, true>`` at D 32 / 64 / 128 (``SS_W2V_PP_ITEMS=1``,
    read once per process: a child of its own)."""
    in_child(_w2v_reduce_child, (32, 64, 128), "per_pair", "1", always=True)
