"""The sparse-LR oracle's tolerance, checked against the reference alone.

``_lr_oracle.py`` carries a first-order error bound beside its fp64 state;
``test_gpu_lr_paths_oracle.py`` holds every exchange of the engine to it.
Here the bound is calibrated without any kernel:

* **noise floor** — the same model in fp32 with the occurrence order of both
  sums permuted (three permutations, both data sets, both optimizers) stays
  within half the tolerance, for every key.  The factor 2 left is headroom
  for the kernels' fast ``exp`` and for error carried from step to step,
  which a first-order bound omits.  Measured max |fp32 - fp64| / tol:

      binary32  adagrad  w 0.039  h 0.166      sgd  w 0.046
      valued64  adagrad  w 0.016  h 0.051      sgd  w 0.015

* **mutants** — five ways a merge kernel can be subtly wrong (feature value
  ignored, taken from the neighbouring occurrence, one occurrence of every
  multi-occurrence key dropped or counted twice, the update applied per
  occurrence) each put far more than 1 % of the keys outside the tolerance
  (12 % at the least: dropped / doubled occurrences under SGD, where only
  the keys with duplicates move).

* **no ill-conditioned key-step** in either data set (the precondition of
  every comparison), and the data sets have the edges their docstring names (row
  lengths, empty rows, 64-bit keys, hot keys and singletons).
"""
import numpy as np
import pytest

import _lr_oracle as O

DATASETS = ("binary32", "valued64")
OPTIMIZERS = ("adagrad", "sgd")


@pytest.mark.parametrize("name", DATASETS)
def test_datasets_have_the_edges(name, tmp_path):
    ds = O.dataset(name)
    n = (ds.keys != O.EMPTY).sum(1)
    assert ds.keys.shape == (O.ROWS, O.F) and set(np.unique(n)) == {0} | set(range(3, O.F + 1))
    assert 0 < (n == 0).sum() < 10
    real = ds.keys[ds.keys != O.EMPTY]
    big = real >= np.uint64(1 << 32)
    assert big.any() == ds.has_values and (not ds.has_values or 0.05 < big.mean() < 0.5)
    assert (ds.x[ds.keys == O.EMPTY] == 0).all()
    ax = np.abs(ds.x[ds.keys != O.EMPTY])
    assert (ax >= 0.25).all() and (ax <= 2).all() and (ds.has_values or (ax == 1).all())
    # a batch: a hot key, duplicates, singletons, ~20k distinct keys over the run
    k0 = ds.batch(0)[0]
    cnt = np.unique(k0[k0 != O.EMPTY], return_counts=True)[1]
    assert cnt.max() > 1000 and (cnt == 1).sum() > 1000 and ((cnt > 1) & (cnt < 10)).sum() > 100
    assert 15000 < len(np.unique(real)) < 30000
    assert 0.2 < ds.y.mean() < 0.8
    # the text is the arrays: parsed back bit for bit (the loaders read this file)
    path = ds.write(tmp_path / "d.libsvm")
    with open(path) as f:
        rows = [ln.split() for ln in f]
    assert len(rows) == O.ROWS
    for r in (0, 1, O.ROWS - 1, int(np.argmin(n))):
        ent = [e.split(":") for e in rows[r][1:]]
        assert float(rows[r][0]) == ds.y[r]
        assert [int(e[0]) for e in ent] == [int(k) for k in ds.keys[r, :n[r]]]
        assert [np.float32(e[1]) if len(e) > 1 else 1 for e in ent] == list(ds.x[r, :n[r]])
    # two ranks' shards tile the file at a line start near its middle
    (a, b), (c, d) = ds.shard(0, 2), ds.shard(1, 2)
    assert a == 0 and b == c and d == O.ROWS and abs(b - O.ROWS // 2) < O.ROWS // 20


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("optimizer", OPTIMIZERS)
@pytest.mark.parametrize("name", DATASETS)
def test_no_ill_conditioned_key_step(name, optimizer, world):
    r = O.reference(name, optimizer, world)
    assert r.ill == 0
    assert len(np.unique(r.keys)) == len(r.keys) and O.EMPTY not in r.keys
    assert np.isfinite(r.w).all() and np.isfinite(r.h).all()
    loss = r.mean_losses()[:, 0]
    assert abs(loss[0] - np.log(2)) < 0.01 and loss[-1] < loss[0]
    print(f"{name} {optimizer} world {world}: keys {len(r.keys)} max|z| {r.zmax:.2f} "
          f"median tol_w {np.median(r.tol_w):.2e} at median |w| {np.median(np.abs(r.w)):.2e}")


@pytest.mark.parametrize("optimizer", OPTIMIZERS)
@pytest.mark.parametrize("name", DATASETS)
def test_fp32_noise_floor_within_half_the_tolerance(name, optimizer):
    ref = O.reference(name, optimizer)
    worst_w = worst_h = 0.0
    for perm in range(3):
        r = O.run(name, optimizer, dtype=np.float32, perm=perm)
        rw, rh, _ = O.ratios(ref, r.keys, r.w, r.h if optimizer == "adagrad" else None)
        np.testing.assert_allclose(r.mean_losses(), ref.mean_losses(), rtol=1e-5)
        worst_w, worst_h = max(worst_w, rw), max(worst_h, rh)
    print(f"{name} {optimizer}: max |fp32 - fp64| / tol  w {worst_w:.3f}  h {worst_h:.3f}")
    assert worst_w <= 0.5 and worst_h <= 0.5, (worst_w, worst_h)


MUTANT_CASES = [(n, o, m) for n in DATASETS for o in OPTIMIZERS for m in O.MUTANTS
                # binary features hide a wrong x; SGD is linear in the occurrences
                if not (m == "x_one" and n == "binary32")
                and not (m == "per_occurrence" and o == "sgd")]


@pytest.mark.parametrize("name,optimizer,mutant", MUTANT_CASES)
def test_mutants_are_rejected(name, optimizer, mutant):
    ref = O.reference(name, optimizer)
    r = O.run(name, optimizer, mutant=mutant)
    rw, rh, out = O.ratios(ref, r.keys, r.w, r.h)
    print(f"{name} {optimizer} {mutant}: {out:.1%} of keys outside, worst w {rw:.3g} h {rh:.3g}")
    assert out > 0.01, out
