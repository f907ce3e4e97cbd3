"""CBOW on the GPU: the tile kernel (k_w2v_cbow_bf16) and the worker's path
through it, against the fp64 reference ``cbow_window_reference``."""
import math

import numpy as np
import pytest
import torch

from swiftsnails_amd.models.word2vec import (W2VSynth, Word2VecWorker, cbow_window_reference,
                                             make_w2v_table_args, window_pairs_reference)

pytestmark = pytest.mark.gpu
T = S = 64
dev = torch.device("cuda", 0)


def _batch_reference(U, meta, B, W, npc):
    """(one gradient row per key position, loss, trained, mask) of a batch with
    rows U = [B centers | R run positions | tiles x 64 negatives], tiles summed."""
    R, tiles = B + 2 * W, (B + T - 1) // T
    mask = window_pairs_reference(meta, B, W)
    ref, tot, trained = np.zeros(U.shape), 0.0, 0
    for t in range(tiles):
        c0, c1 = t * T, min(B, t * T + T)
        q0, q1 = c0, min(R, c0 + T + 2 * W)
        n0 = B + R + t * S
        l, n, gX, gC, gN = cbow_window_reference(U[B + q0:B + q1], U[c0:c1], U[n0:n0 + S],
                                                 mask[c0:c1, q0:q1], npc)
        tot, trained = tot + l, trained + n
        ref[c0:c1] += gC
        ref[B + q0:B + q1] += gX
        ref[n0:n0 + S] += gN
    return ref, tot, trained, mask


@pytest.mark.parametrize("D,W,B", [(32, 1, 64), (64, 5, 65), (128, 15, 100), (128, 5, 256)])
def test_cbow_tile_matches_reference(D, W, B):
    """Every key position its own row, row atomics; inputs and tolerances (bf16
    operands, fp32 accumulation) of test_w2v_window_tile_matches_reference."""
    from swiftsnails_amd._native import hip

    tiles, R = (B + T - 1) // T, B + 2 * W
    rng = np.random.default_rng(D + W)
    tags = np.cumsum(rng.random(R) < 0.08)
    bs = rng.integers(1, W + 1, R)
    meta = ((tags << 4) | bs).astype(np.int32)
    meta[rng.random(R) < 0.1] = -1
    nrows = B + R + tiles * S
    U = (rng.standard_normal((nrows, D)) * 0.3).astype(np.float32)
    g = torch.zeros((nrows, D), device=dev)
    loss, pairs = torch.zeros(256 * 32, device=dev), torch.zeros(256 * 32, device=dev)
    tu, tm = torch.from_numpy(U).to(dev), torch.from_numpy(meta).to(dev)
    ti = torch.arange(nrows, dtype=torch.int32, device=dev)
    p, npc = ti.data_ptr(), 5 / S
    hip().w2v_cbow(p, p + B * 4, p + (B + R) * 4, tm.data_ptr(), B, W, D, npc, tu.data_ptr(),
                   g.data_ptr(), loss.data_ptr(), pairs.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    G = g.cpu().numpy().astype(np.float64)
    ref, tot, trained, mask = _batch_reference(U, meta, B, W, npc)
    on = mask.any(1)
    assert pairs.sum().item() == on.sum() == trained > 0 and not on.all()
    print(f"cbow tile D {D} W {W} B {B}: max |err| / tol "
          f"{(np.abs(G - ref) / (1e-2 + 3e-2 * np.abs(ref))).max():.3f}")
    np.testing.assert_allclose(G, ref, rtol=3e-2, atol=1e-2)
    np.testing.assert_allclose(loss.sum().item(), tot, rtol=3e-3)
    assert not G[:B][~on].any() and not G[B:B + R][meta < 0].any()


def test_cbow_worker_matches_stepwise_reference(monkeypatch):
    """Three SGD steps through Word2VecWorker (key swap, occurrence reduce, tail
    rows, fused update) against row -= lr * the key's summed fp64 gradient from
    the table's initial rows.  Pull-ahead off: the reference is sequential."""
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    torch.cuda.set_device(dev)
    D, lr = 64, 0.5
    data = W2VSynth(arch="cbow", batch_size=150, window=5, vocab=500, negatives=5)
    B, R = data.batch_size, data.run_len
    opt, init = make_w2v_table_args(D, Optimizer("sgd", lr=lr))
    table = HbmTable(D, 1 << 14, optimizer=opt, init=init, device=dev)
    eng = PSEngine(table, None, max_keys=data.n_keys, dim=D, device=dev)
    w = Word2VecWorker(eng, data)
    assert w.cbow and w.occ_reduce and not eng.pull_ahead
    batches = []
    for t in range(3):
        k = w._produce(t, 0, None).cpu().numpy().copy()
        batches.append((k, w.meta[0].cpu().numpy().copy()))
        assert (k[:B] >> 40 == 1).all() and (k[B:B + R] >> 40 == 0).all()
    allk = np.unique(np.concatenate([k for k, _ in batches]))
    tk = torch.from_numpy(allk).to(dev)
    rows0 = table.pull(tk)[0].cpu().numpy()[:, :D].astype(np.float64)
    assert not rows0[allk >> 40 == 1].any() and rows0[allk >> 40 == 0].any(1).all()
    w.step()
    # the output namespace starts at zero: every score of step 0 is 0
    assert w.mean_loss() == pytest.approx((1 + data.negatives) * math.log(2), rel=1e-3)
    w.step()
    w.step()
    torch.cuda.synchronize()
    table.check()
    got = table.pull(tk)[0].cpu().numpy()[:, :D].astype(np.float64)
    want = rows0.copy()
    for k, meta in batches:
        pos = np.searchsorted(allk, k)
        grad = np.zeros_like(want)
        np.add.at(grad, pos, _batch_reference(want[pos], meta, B, data.window, data.neg_per_pair)[0])
        want -= lr * grad
    dg, dw = got - rows0, want - rows0
    print(f"cbow worker: max |update| {np.abs(dw).max():.3e}, |err| / |update| (Frobenius) "
          f"{np.linalg.norm(dg - dw) / np.linalg.norm(dw):.2e}")
    np.testing.assert_allclose(dg, dw, rtol=3e-2, atol=1e-2 * lr)
    # the absolute term alone would pass a lost row at this init scale
    assert np.linalg.norm(dg - dw) <= 3e-2 * np.linalg.norm(dw)
