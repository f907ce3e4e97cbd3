"""``k_ffm_fwd_bwd`` and ``FFMWorker`` against ``ffm_reference`` (fp64 loops).

Kernel cases hold the FM kernel test's figures: ``pred`` rtol 1e-4 + atol 1e-5,
the summed loss rtol 1e-4, gradients rtol 1e-3 + atol 1e-5.  The worker is held
step by step (a carried AdaGrad bound cannot hold, ``_fm_oracle.py``): from the
table's own rows before a step, the fp64 gradient G of every key and its bound

    eG = sum_occ [ (|g| (U_G + (1 - |g|) dz) + U_A) |b| + u |g b| ] + n_occ u sum_occ |g b|
    dz = (F + F (F - 1) K) u (sum_i |w_i| + sum_{i<j} sum_k |R_i[j]_k R_j[i]_k|)

(b: the partner value, 1 for w; u = 2^-24; U_G the relative accuracy of g from
``_lr_oracle``; U_A = 1.5 u its absolute accuracy; dz: the terms the kernel sums
into z times their magnitudes; the last term: n_occ atomics in any order), and
the table after the step within ``1e-6 + 1e-4 |x| + lr eG / sqrt(h + eps)``
(SGD: ``lr eG``; h: ``1e-7 + 1e-4 h + 2 |G| eG + eG^2``).  Keys the step did not
touch are bit-identical and the key set is exact.

Measured on an MI355X, largest |kernel - fp64| / tol (printed as ``MARGIN``;
reported, not tuned).  Kernel cases in parameter order: pred 0.001 0.002 0.002
0.002 0.004 0.003, loss <= 0.001, gradient 0.000 0.001 0.001 0.001 0.002 0.003;
EMPTY / duplicates: gradient 0.006 / 0.008; worker: SGD 0.001, AdaGrad 0.056.

Beside those figures every kernel case is held to ``_ffm_oracle.key_gradient``'s
derived bounds (``dz`` for the sum the kernel forms, ``eG``, ``pred`` and the
summed loss with the counter's shards; SAFETY = 2), printed as ``MARGIN derived``:
the six shapes pred 0.011-0.090, loss <= 0.017, gradient 0.017-0.111; EMPTY /
duplicates 0.019 / 0.032; all 157 legal shapes (``test_kernel_every_legal_shape``)
pred 0.174, loss 0.014, gradient 0.100; a hot id with 2112 occurrences
(``test_kernel_hot_id``) gradient 0.021-0.146, its own row <= 0.001.
"""
import numpy as np
import pytest
import torch

import _ffm_oracle as FO
from _lr_oracle import U32, U_G

pytestmark = pytest.mark.gpu
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    from swiftsnails_amd._native import hip

    hip()
    return torch.device("cuda", 0)


def _run_kernel(dev, inv, rows, y, F, K, with_pred=True):
    """(pred, loss, ugrad) of one launch on ``inv`` [B, F] uint32, ``rows`` [U, dim];
    ``with_pred=False``: the worker's form, no ``pred`` buffer."""
    from swiftsnails_amd._native import hip

    B = len(y)
    ti = torch.from_numpy(inv.astype(np.uint32).view(np.int32).reshape(-1)).to(dev)
    tr, ty = torch.from_numpy(rows).to(dev), torch.from_numpy(y).to(dev)
    g, loss = torch.zeros_like(tr), torch.zeros(256 * 32, device=dev)
    pred = torch.empty(B, device=dev)
    hip().ffm_fwd_bwd(ti.data_ptr(), ty.data_ptr(), B, F, K, tr.data_ptr(), g.data_ptr(),
                      loss.data_ptr(), pred.data_ptr() if with_pred else 0,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (pred.cpu().numpy() if with_pred else None), loss.sum().item(), g.cpu().numpy()


def _ratio(d, tol):
    """|difference| / bound; 0 where both are 0, inf where only the bound is."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, np.abs(d) / tol)


def _derived(out, r):
    """(pred, loss, gradient) margins of a launch against ``_ffm_oracle.key_gradient``'s
    fp64 values and derived bounds (its module docstring; SAFETY = 2)."""
    pred, loss, g = out
    rp = float(_ratio(pred - r.p, r.tol_p).max()) if pred is not None else 0.0
    rl = float(abs(loss - r.loss.sum()) / r.tol_loss)
    return rp, rl, float(_ratio(g - r.G, FO.SAFETY * r.eG).max())


def _check_derived(label, out, r):
    rp, rl, rg = _derived(out, r)
    print(f"MARGIN derived {label}: pred {rp:.3f} loss {rl:.3f} grad {rg:.3f}")
    assert rp <= 1 and rl <= 1 and rg <= 1, (label, rp, rl, rg)


def _check_kernel(label, out, ref, F, K):
    (pred, loss, g), (l, p, G) = out, ref
    rp = np.abs(pred - p) / (1e-5 + 1e-4 * np.abs(p))
    rg = np.abs(g - G) / (1e-5 + 1e-3 * np.abs(G))
    print(f"MARGIN {label}: pred {rp.max():.3f} loss {abs(loss - l) / (1e-4 * abs(l)):.3f} "
          f"grad {rg.max():.3f}")
    assert rp.max() <= 1 and abs(loss - l) <= 1e-4 * abs(l) and rg.max() <= 1


@pytest.mark.parametrize("F,K,B", [(2, 2, 1000), (13, 4, 1000), (16, 8, 257), (39, 4, 67),
                                   (64, 4, 67), (32, 8, 67)])
def test_kernel_matches_reference(dev, F, K, B):
    from swiftsnails_amd.models.ffm import ffm_reference

    rng = np.random.default_rng(F * 100 + K)
    dim = 1 + F * K
    rows = (0.2 * rng.standard_normal((B * F, dim))).astype(np.float32)
    y = (rng.random(B) < 0.4).astype(np.float32)
    out = _run_kernel(dev, np.arange(B * F).reshape(B, F), rows, y, F, K)
    l, p, G = ffm_reference(rows.reshape(B, F, dim), y)
    _check_kernel(f"kernel F {F} K {K}", out, (l, p, G.reshape(B * F, dim)), F, K)
    _check_derived(f"kernel F {F} K {K}", out,
                   FO.key_gradient(np.arange(B * F).reshape(B, F), rows, y, K))
    g = out[2].reshape(B, F, dim)
    for i in range(F):  # the (i, i) block is never written
        assert not g[:, i, 1 + i * K:1 + (i + 1) * K].any()


@pytest.mark.parametrize("F,K", [(13, 4), (39, 4)])
def test_kernel_empty_and_duplicates(dev, F, K):
    from swiftsnails_amd.models.ffm import ffm_reference

    rng = np.random.default_rng(F)
    B, dim = 67, 1 + F * K
    U = B * F // 10
    rows = (0.2 * rng.standard_normal((U + 5, dim))).astype(np.float32)  # the last 5 ids: unused
    y = (rng.random(B) < 0.4).astype(np.float32)
    inv = rng.integers(0, U, (B, F))
    inv[rng.random((B, F)) < 0.2] = INVALID
    inv[0] = INVALID                       # all EMPTY: z = 0
    inv[1] = INVALID
    inv[1, F // 2] = 3                     # one occurrence: z = w
    for s in range(2, 8):                  # one id at two columns
        inv[s, [s, F - s]] = rng.integers(0, U)
    valid = inv != INVALID
    out = _run_kernel(dev, inv, rows, y, F, K)
    l, p, G = ffm_reference(rows[np.where(valid, inv, 0)], y, valid)
    want = np.zeros((U + 5, dim))
    np.add.at(want, inv[valid], G[valid])
    _check_kernel(f"empty/dup F {F} K {K}", out, (l, p, want), F, K)
    _check_derived(f"empty/dup F {F} K {K}", out, FO.key_gradient(inv, rows, y, K))
    assert p[0] == 0.5 and not out[2][np.setdiff1d(np.arange(U + 5), inv[valid])].any()


LEGAL = [(F, K) for K in (2, 4, 8) for F in range(2, 65) if F * K <= 256]


def _planted_batch(rng, F, K, B, dup_rows=1):
    """A small batch for one shape: ids shared between samples (about B F / 4
    values, three more rows unused), about 15 % EMPTY, sample 0 all EMPTY, sample 1
    with one id at two columns; rows of scale (F (F - 1) K / 2)^-1/4."""
    dim = 1 + F * K
    U = max(2, B * F // 4)
    rows = ((F * (F - 1) * K / 2) ** -0.25 * rng.standard_normal((U + 3, dim))).astype(np.float32)
    inv = rng.integers(0, U, (B, F))
    inv[rng.random((B, F)) < 0.15] = INVALID
    inv[0] = INVALID
    inv[1, [0, F - 1]] = 1
    y = (rng.random(B) < 0.4).astype(np.float32)
    return inv, rows, y, U


def test_kernel_every_legal_shape(dev):
    """All 157 legal (F, K), every one within the derived bound; the table of
    (G, di) the sweep covers is asserted, so it cannot silently shrink."""
    assert len(LEGAL) == 157
    table, worst = {}, np.zeros(3)
    for F, K in LEGAL:
        dim, G, di = FO.geometry(F, K)
        table[(F, K)] = (G, di)
        B = 2 * (256 // G) + 1
        inv, rows, y, U = _planted_batch(np.random.default_rng(1000 * K + F), F, K, B)
        out = _run_kernel(dev, inv, rows, y, F, K)
        r = FO.key_gradient(inv, rows, y, K)
        m = _derived(out, r)
        worst = np.maximum(worst, m)
        assert max(m) <= 1, (F, K, m)
        g = out[2]
        used = np.unique(inv[inv != INVALID])
        assert not g[np.setdiff1d(np.arange(U + 3), used)].any()   # unused ids: exactly 0
        live = inv != INVALID
        for i in range(F):                                         # diagonal blocks: exactly 0
            only = np.setdiff1d(inv[:, i][live[:, i]], inv[:, np.arange(F) != i][live[:, np.arange(F) != i]])
            assert not g[only, 1 + i * K:1 + (i + 1) * K].any(), (F, K, i)
        assert r.p[0] == 0.5 and out[0][0] == 0.5
    print(f"MARGIN derived every legal shape: pred {worst[0]:.3f} loss {worst[1]:.3f} "
          f"grad {worst[2]:.3f}")
    by_g = {G: {di for g2, di in table.values() if g2 == G} for G in (16, 64, 256)}
    assert by_g == {16: {0, 1, 2, 3}, 64: {0, 1, 2, 3}, 256: set(range(8))}, by_g
    # both sides of both regime edges of ``ffm_group``, for every K
    for lo, hi in (((7, 2), (8, 2)), ((5, 4), (6, 4)), ((3, 8), (4, 8))):
        assert table[lo][0] == 16 and table[hi][0] == 64
        assert lo[0] * (1 + lo[0] * lo[1]) <= 128 < hi[0] * (1 + hi[0] * hi[1])
    for K in (2, 4, 8):
        assert table[(16, K)][0] == 64 and table[(17, K)][0] == 256
    assert table[(3, 8)] == (16, 0) and table[(17, 2)] == (256, 7)
    assert len({(K - 1 - F * K) % 32 for F, K in LEGAL}) == 16  # every padding of ``ffm_row_stride``


@pytest.mark.parametrize("F,K", [(5, 2), (13, 4), (39, 4)])
def test_kernel_hot_id(dev, F, K):
    """One id at the same column of all 2048 samples and at a second column of
    64 of them: 2112 atomics into every float of one gradient row, from two
    partner blocks, within ``n u sum |g b|`` and the rest of the derived bound
    (a worst case over every order of 2112 atomics: measured, the hot row uses
    about a thousandth of it, so this holds a gross error of that row, such as a
    lost occurrence, and not its rounding); also without ``pred``, the worker's
    form."""
    B = 2048
    rng = np.random.default_rng(F)
    inv, rows, y, U = _planted_batch(rng, F, K, B)
    c1, c2 = 1, 3
    inv[inv == 0] = 2                      # id 0 is the hot one, at its two columns only
    inv[:, c1] = 0
    inv[rng.choice(B, 64, replace=False), c2] = 0
    r = FO.key_gradient(inv, rows, y, K)
    assert r.cnt[0] == B + 64
    for with_pred in (True, False):
        out = _run_kernel(dev, inv, rows, y, F, K, with_pred)
        _check_derived(f"hot id F {F} K {K} pred {int(with_pred)}", out, r)
        hot = float(_ratio(out[2][0] - r.G[0], FO.SAFETY * r.eG[0]).max())
        print(f"MARGIN derived hot row F {F} K {K}: grad {hot:.3f}")
        assert hot <= 1


def _export(table):
    parts = [(k.numpy().view(np.uint64), r.numpy()) for k, r in table.export()]
    keys, rows = (np.concatenate(x) for x in zip(*parts))
    order = np.argsort(keys)
    return keys[order], rows[order]


@pytest.mark.parametrize("optimizer,lr", [("sgd", 1e-3), ("adagrad", 0.05)])
def test_worker_step_by_step(dev, monkeypatch, optimizer, lr):
    from swiftsnails_amd.models.ffm import FFMWorker, ffm_reference, ffm_table_args
    from swiftsnails_amd.models.sparse_lr import CtrSynth
    from swiftsnails_amd.ops.optim import Optimizer
    from swiftsnails_amd.ops.table import HbmTable
    from swiftsnails_amd.parallel.engine import PSEngine

    monkeypatch.setenv("SS_PULL_AHEAD", "0")
    B, F, K, eps, ada = 512, 6, 4, 1e-8, optimizer == "adagrad"
    D = 1 + F * K
    data = CtrSynth(batch_size=B, num_fields=F, num_features=3000, tail_frac=0.0)
    opt, init = ffm_table_args(K, Optimizer(optimizer, lr=lr, eps=eps))
    table = HbmTable(D, 1 << 13, optimizer=opt, init=init, device=dev)
    w = FFMWorker(PSEngine(table, None, max_keys=B * F, dim=D, device=dev), data, K)
    assert not w.engine.pull_ahead
    tk, ty = torch.empty(B * F, dtype=torch.int64, device=dev), torch.empty(B, device=dev)
    scratch = HbmTable(D, 1 << 13, optimizer=Optimizer("sgd"), init=init, device=dev)
    keys, x = np.empty(0, np.uint64), np.empty((0, table.width), np.float32)
    worst = 0.0
    for step in range(4):
        data.generate(step, 0, 1, tk, ty)
        bk, y = tk.cpu().numpy().view(np.uint64).reshape(B, F), ty.cpu().numpy()
        u, inv = np.unique(bk, return_inverse=True)
        inv = inv.reshape(B, F)
        new = np.setdiff1d(u, keys)               # new keys start from the device's initialiser
        r0 = np.zeros((len(new), table.width), np.float32)
        if len(new):
            r0[:, :D] = scratch.pull(torch.from_numpy(new.view(np.int64)).to(dev))[0].cpu().numpy()
        allk = np.concatenate([keys, new])
        order = np.argsort(allk)
        keys0, x0 = allk[order], np.concatenate([x, r0])[order]
        pos = np.searchsorted(keys0, u)
        R = x0[pos, :D].astype(np.float64)[inv]   # [B, F, D] occurrence rows
        l, p, Go = ffm_reference(R, y)
        # the bound of the module docstring
        g = np.abs(p - y)
        V = np.abs(R[..., 1:]).reshape(B, F, F, K)
        P = (V * V.transpose(0, 2, 1, 3)).sum(3)  # [B, F, F]: sum_k |R_i[j]_k R_j[i]_k|
        A = np.abs(R[..., 0]).sum(1) + 0.5 * (P.sum((1, 2)) - np.trace(P, axis1=1, axis2=2))
        dz = (F + F * (F - 1) * K) * U32 * A
        rel = (g * (U_G + (1 - g) * dz) + 1.5 * U32)[:, None, None]
        b = np.abs(Go) / np.maximum(g, 1e-300)[:, None, None]   # |partner| (1 for w)
        G, eG, S, n = (np.zeros((len(u), D)) for _ in range(4))
        np.add.at(G, inv, Go)
        np.add.at(eG, inv, rel * b + U32 * np.abs(Go))
        np.add.at(S, inv, np.abs(Go))
        np.add.at(n, inv, 1.0)
        eG += n * U32 * S
        hw = x0[pos, D:].astype(np.float64) + (G * G if ada else 0.0)   # SGD: no state
        den = np.sqrt(hw + eps) if ada else 1.0
        xw = x0[pos, :D].astype(np.float64) - lr * G / den
        tol_x, tol_h = 1e-6 + 1e-4 * np.abs(xw) + lr * eG / den, 1e-7 + 1e-4 * hw
        if ada:
            tol_h = tol_h + 2 * np.abs(G) * eG + eG * eG
        w.step()
        torch.cuda.synchronize()
        table.check()
        keys, x = _export(table)
        assert np.array_equal(keys, keys0)        # the key set, exactly
        same = np.setdiff1d(np.arange(len(keys)), pos)
        assert np.array_equal(x[same], x0[same])  # untouched keys: bit-identical
        worst = max(worst, (np.abs(x[pos, :D] - xw) / tol_x).max())
        if ada:
            worst = max(worst, (np.abs(x[pos, D:] - hw) / tol_h).max())
        np.testing.assert_allclose(w.mean_loss(), l / B, rtol=1e-4)
    print(f"MARGIN worker {optimizer}: max |table - fp64| / tol {worst:.3f}")
    assert worst <= 1


def test_model_ffm_from_config(dev, monkeypatch):
    from swiftsnails_amd.framework.gpu import build_worker
    from swiftsnails_amd.utils.config import Config

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    cfg = Config.from_dict({"model": "ffm", "num_fields": 39, "ffm_k": 4, "batch_size": 2048,
                            "num_features": 200_000, "tail_frac": 0.0, "optimizer": "adagrad",
                            "learning_rate": 0.05, "round_timeout": 0})
    ctx, w = build_worker(cfg)
    assert type(w).__name__ == "FFMWorker" and w.engine.dim == 157 and ctx.table.width == 314
    losses = [float(w.step().sum().item()) / 2048 for _ in range(30)]
    ctx.table.check()
    assert np.mean(losses[-5:]) < np.mean(losses[:3]) - 0.02, losses
    assert np.isfinite(w.evaluate()["auc"])
    ctx.close()
