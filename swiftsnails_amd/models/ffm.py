"""Field-aware factorization machine (Juan et al. 2016, libffm) on the HBM table.

A key keeps one latent vector per *other field*: its row is ``[w | v_0 | ... |
v_{F-1}]``, each ``v_j`` of K floats (dim = 1 + F K).  The field of an
occurrence is its column in the ``[B, F]`` batch (``CtrSynth`` draws one key
per field; the ``ctr`` TSV format has one token per column).  With ``R_i`` the
row of occurrence i of a sample and ``R_i[j]`` its block j, binary features:

    z = sum_i w_i + sum_{i<j} <R_i[j], R_j[i]>

The block ``R_i[i]`` is carried in the row and never read or updated.  EMPTY
padding takes no part; a key at two columns of one sample is two occurrences.
Shapes: K in {2, 4, 8}, 2 <= F <= 64, F K <= 256 (``csrc/hip/ffm.hip``).

Sizing: F = 39, K = 4 with AdaGrad is 314 floats a key (1264-byte slots), so
5e7 keys at load 0.7 are 90 GB — one MI355X holds them in half its HBM, 1e9
keys do not fit (``plan_ffm_table``).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .._native import hip
from ..ops.optim import InitConfig, Optimizer
from ..ops.table import HbmTable
from .base import PipelinedWorker, evaluate_ctr
from .sparse_lr import CtrSynth

FFM_KS = (2, 4, 8)
FFM_MAX_F, FFM_MAX_FK = 64, 256


def check_ffm_shape(num_fields: int, k: int) -> int:
    """dim = 1 + F K of a supported shape; ValueError names the limit otherwise."""
    if k not in FFM_KS:
        raise ValueError(f"ffm: K must be one of {FFM_KS}, not {k}")
    if not 2 <= num_fields <= FFM_MAX_F:
        raise ValueError(f"ffm: num_fields must be in [2, {FFM_MAX_F}], not {num_fields}")
    if num_fields * k > FFM_MAX_FK:
        raise ValueError(f"ffm: num_fields * K must be at most {FFM_MAX_FK} (dim <= "
                         f"{FFM_MAX_FK + 1}), not {num_fields} * {k}")
    return 1 + num_fields * k


def ffm_table_args(k: int, optimizer: Optional[Optimizer] = None):
    opt = optimizer or Optimizer("adagrad", lr=0.05)
    init = InitConfig("normal", scale=0.01, state_init=0.0)
    return opt, init


def plan_ffm_table(n_keys: int, num_fields: int = 39, k: int = 4, shards: int = 1,
                   load: float = 0.7, row_dtype: str = "fp32") -> dict:
    """Per-shard table plan of an FFM table with AdaGrad (as ``plan_fm_table``)."""
    dim = check_ffm_shape(num_fields, k)
    p = HbmTable.plan(n_keys // shards, dim, Optimizer("adagrad"), load, row_dtype)
    p["GB_per_shard"] = round(p["bytes"] / 1e9, 1)
    return p


class FFMWorker(PipelinedWorker):
    """Trains the FFM through a ``PSEngine``: the generic round (dedup with the
    inverse index and zeroed gradient rows, pull, push) around
    ``k_ffm_fwd_bwd``, which adds per-occurrence gradients into the unique
    rows with float atomics."""

    def __init__(self, engine, data: CtrSynth, k: int = 4, rank: int = 0, world: int = 1,
                 active: bool = True):
        dim = check_ffm_shape(data.num_fields, k)
        if engine.dim != dim:
            raise ValueError(f"FFMWorker: dim must be 1 + num_fields * K = {dim} "
                             f"({data.num_fields} fields, K = {k}), not {engine.dim}")
        if getattr(data, "has_values", False):
            # the kernel is binary-feature: idx:val entries would be trained as val = 1
            raise ValueError("FFMWorker: the FFM kernels take binary features; this source has "
                             "feature values (idx:val), which they would ignore")
        super().__init__(engine, rank, world, active)
        self.data, self.k = data, k
        # as FM: pull the next round's (wide) rows behind its dedup
        engine.enable_pull_ahead()
        dev = engine.device
        B, F = data.batch_size, data.num_fields
        self.keys = [torch.empty(B * F, dtype=torch.int64, device=dev) for _ in range(engine.depth)]
        self.labels = [torch.empty(B, dtype=torch.float32, device=dev) for _ in range(engine.depth)]

    def _produce(self, step, slot, stream):
        self.data.generate(step, self.rank, self.world, self.keys[slot], self.labels[slot],
                           stream=stream, **self._gen_kwargs(step))
        return self.keys[slot]

    def _compute(self, rnd, slot, st):
        d = self.data
        hip().ffm_fwd_bwd(rnd.inv.data_ptr(), self.labels[slot].data_ptr(), d.batch_size,
                          d.num_fields, self.k, rnd.uvals.data_ptr(), rnd.ugrad.data_ptr(),
                          self.loss_sum.data_ptr(), 0, st)

    def samples_per_step(self) -> int:
        return self.data.batch_size if self.active else 0

    def evaluate(self, batches: int = 1) -> dict:
        """Held-out AUC / log-loss of the FFM logits vs the planted ground
        truth (models/base.py evaluate_ctr; unseen keys contribute zero).
        World > 1: collective."""
        D = self.engine.dim
        return evaluate_ctr(self, batches, lambda rows, B, F: ffm_logits(rows.view(B, F, D)))


def ffm_logits(rows: torch.Tensor) -> torch.Tensor:
    """FFM logits of [B, F, 1 + F K] rows: sum_i w_i + sum_{i<j} <R_i[j], R_j[i]>."""
    B, F, D = rows.shape
    V = rows[..., 1:].reshape(B, F, F, (D - 1) // F)
    P = (V * V.transpose(1, 2)).sum(-1)              # P[b, i, j] = <R_i[j], R_j[i]>
    return rows[..., 0].sum(1) + torch.triu(P, diagonal=1).sum((1, 2))


def ffm_reference(rows: np.ndarray, labels: np.ndarray, valid: Optional[np.ndarray] = None):
    """fp64 reference for one batch, the obvious loops.  rows [B, F, 1 + F K]
    (occurrence rows), valid [B, F] bool (False: no occurrence there).
    Returns (loss_sum, pred [B], grad rows [B, F, dim])."""
    R = rows.astype(np.float64)
    B, F, D = R.shape
    K = (D - 1) // F
    ok = np.ones((B, F), bool) if valid is None else valid.astype(bool)
    blk = lambda i, j: R[:, i, 1 + j * K:1 + (j + 1) * K]  # noqa: E731
    z = (R[..., 0] * ok).sum(1)
    for i in range(F):
        for j in range(i + 1, F):
            z += (blk(i, j) * blk(j, i)).sum(1) * (ok[:, i] & ok[:, j])
    p = 1.0 / (1.0 + np.exp(-z))
    y = labels.astype(np.float64)
    loss = float(np.sum(np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - y * z))
    g = p - y
    grad = np.zeros_like(R)
    grad[..., 0] = g[:, None] * ok
    for i in range(F):
        for j in range(F):
            if j != i:
                grad[:, i, 1 + j * K:1 + (j + 1) * K] = \
                    (g * (ok[:, i] & ok[:, j]))[:, None] * blk(j, i)
    return loss, p, grad
