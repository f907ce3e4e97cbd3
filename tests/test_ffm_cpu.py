"""The field-aware FM's host side: the fp64 reference against finite
differences of its own loss, the torch logits against it, the table plan and
the refusals of the constructor and the config."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from swiftsnails_amd.models.ffm import (FFMWorker, ffm_logits, ffm_reference, ffm_table_args,
                                        plan_ffm_table)


def _batch(F, K, B, seed=0):
    rng = np.random.default_rng(seed)
    rows = 0.3 * rng.standard_normal((B, F, 1 + F * K))
    y = (rng.random(B) < 0.4).astype(np.float64)
    valid = rng.random((B, F)) < 0.8
    return rows, y, valid


@pytest.mark.parametrize("masked", [False, True])
def test_reference_gradient_is_the_derivative_of_its_loss(masked):
    F, K, B, h = 3, 2, 5, 1e-6
    rows, y, valid = _batch(F, K, B)
    valid = valid if masked else None
    _, _, grad = ffm_reference(rows, y, valid)
    num = np.zeros_like(rows)
    for idx in np.ndindex(*rows.shape):
        d = np.zeros_like(rows)
        d[idx] = h
        up, dn = ffm_reference(rows + d, y, valid)[0], ffm_reference(rows - d, y, valid)[0]
        num[idx] = (up - dn) / (2 * h)
    # central differences of a smooth loss: O(h^2) truncation, ~1e-16 / h rounding
    np.testing.assert_allclose(grad, num, rtol=0, atol=1e-8)
    for i in range(F):  # the (i, i) block is never read
        assert not grad[:, i, 1 + i * K:1 + (i + 1) * K].any()
    if masked:
        assert not grad[~valid].any()


@pytest.mark.parametrize("F,K", [(3, 2), (7, 4)])
def test_logits_match_reference(F, K):
    rows, y, _ = _batch(F, K, 9, seed=1)
    _, p, _ = ffm_reference(rows, y)
    z = ffm_logits(torch.from_numpy(rows))
    np.testing.assert_allclose(torch.sigmoid(z).numpy(), p, rtol=1e-12)


def test_plan_and_table_args():
    p = plan_ffm_table(50_000_000, 39, 4, shards=1, load=0.7)
    assert p["width"] == 2 * (1 + 39 * 4) == 314
    assert p["stride"] == 1264 and p["capacity"] == -(-50_000_000 * 10 // 7)
    assert p["bytes"] == p["capacity"] * 1264 and p["bytes"] < 144e9  # half of 288 GB
    assert plan_ffm_table(1_000_000_000, 39, 4)["bytes"] > 288e9
    assert plan_ffm_table(80, 39, 4, shards=8)["capacity"] == -(-10 * 10 // 7)
    opt, init = ffm_table_args(4)
    assert (opt.kind, init.kind, init.scale, init.state_init) == ("adagrad", "normal", 0.01, 0.0)


@pytest.mark.parametrize("F,K,dim,has_values,msg", [
    (6, 4, 26, False, "1 \\+ num_fields \\* (K|ffm_k) = 25"), (6, 3, 19, False, "K must be one of"),
    (33, 8, 265, False, "at most 256"), (6, 4, 25, True, "binary features")])
def test_worker_and_config_refuse(F, K, dim, has_values, msg):
    from swiftsnails_amd.framework.gpu import build_worker
    from swiftsnails_amd.utils.config import Config

    data = SimpleNamespace(num_fields=F, batch_size=8, has_values=has_values)
    with pytest.raises(ValueError, match=msg):
        FFMWorker(SimpleNamespace(dim=dim), data, K)
    if not has_values:  # the same shapes through model: ffm
        cfg = Config.from_dict({"model": "ffm", "num_fields": F, "ffm_k": K, "dim": dim,
                                "batch_size": 8, "num_features": 100})
        with pytest.raises(ValueError, match=msg):
            build_worker(cfg)
