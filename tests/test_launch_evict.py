"""Periodic eviction from a config (``evict_period`` and the keys beside it,
framework/gpu.py ``evict_config`` / ``PSContext.maybe_evict``)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    from swiftsnails_amd.utils.config import Config

    return Config.from_dict(kw)


def test_evict_config_keys_and_refusals():
    from swiftsnails_amd.framework.gpu import evict_config

    assert evict_config(_cfg()) == (0, None, 0.0)
    assert evict_config(_cfg(evict_acc_below=1.0, graph=1)) == (0, None, 0.0)  # period 0: off
    p, rule, ml = evict_config(_cfg(evict_period=50, evict_acc_below=0.25, evict_min_load=0.6))
    assert (p, rule.acc_below, rule.w_below, ml) == (50, 0.25, None, 0.6)
    p, rule, ml = evict_config(_cfg(evict_period=5, evict_w_below=0, optimizer="sgd"))
    assert (p, rule.acc_below, rule.w_below, ml) == (5, None, 0.0, 0.0)
    with pytest.raises(ValueError, match="graph"):
        evict_config(_cfg(evict_period=50, evict_acc_below=0.25, graph=1))
    with pytest.raises(ValueError, match="evict_acc_below"):
        evict_config(_cfg(evict_period=50))  # a period without a rule
    with pytest.raises(ValueError, match="SGD"):
        evict_config(_cfg(evict_period=50, evict_acc_below=0.25, optimizer="sgd"))


def test_maybe_evict_crosses_period_boundaries():
    """The crossed-a-boundary rule of maybe_backup: rounds that advance in
    jumps still evict once per period; shards below evict_min_load are
    skipped."""
    from swiftsnails_amd.framework.gpu import PSContext
    from swiftsnails_amd.ops.optim import EvictRule

    class Tab:
        capacity = 100

        def __init__(self):
            self.n = 80

        def size(self):
            return self.n

    class Eng:
        pull_ahead = False

        def __init__(self, tab):
            self.tab, self.calls = tab, []

        def evict(self, rule=None, mask=None):
            self.calls.append(rule)
            self.tab.n -= 30
            return 30

    ctx = PSContext.__new__(PSContext)
    tab = Tab()
    ctx.table, ctx.engine = tab, Eng(tab)
    ctx.evict_period, ctx.evict_rule, ctx.evict_min_load = 10, EvictRule(acc_below=1.0), 0.4
    ctx._last_evict, ctx.evicted, ctx.watchdog, ctx.world, ctx.rank = 0, 0, None, 1, 0
    got = [ctx.maybe_evict(r) for r in (0, 4, 9, 16, 19, 32, 40, 41)]
    # 16 crosses 10 (80 -> 50), 32 crosses 20 and 30 (50 -> 20), 40: load 0.2 < 0.4, skipped
    assert got == [None, None, None, 30, None, 30, 0, None]
    assert ctx.evicted == 60 and len(ctx.engine.calls) == 2


@pytest.mark.gpu
def test_cli_gpu_sparse_lr_evict_period(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = [sys.executable, "-m", "swiftsnails_amd.launch", "--config",
              os.path.join(ROOT, "configs", "sparse_lr_10m.conf"), "--steps", "12",
              "--set", "batch_size=4096", "--set", "num_features=1000000"]
    runs = {}
    for name, extra in (("plain", []),
                        ("evict", ["--set", "evict_period=5", "--set", "evict_acc_below=0.3"])):
        r = subprocess.run(common + extra, cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[name] = (json.loads(r.stdout.strip().splitlines()[-1]), r.stderr)
    plain, (ev, log) = runs["plain"][0], runs["evict"]
    assert "evict" not in plain
    assert ev["evict"]["period"] == 5 and ev["evict"]["evicted"] > 0
    assert "evicted" in log  # rank 0 logs each call's count
    assert ev["steps"] == plain["steps"] == 12
    assert ev["rank0_table"]["size"] < plain["rank0_table"]["size"]
    assert ev["rank0_table"]["size"] + ev["evict"]["evicted"] >= plain["rank0_table"]["size"]
    # graph: 1 with a period is refused at start-up, with a message
    r = subprocess.run(common + ["--set", "evict_period=5", "--set", "evict_acc_below=0.3",
                                 "--set", "graph=1"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "graph" in r.stderr and "evict_period" in r.stderr
