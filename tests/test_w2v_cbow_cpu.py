"""CBOW (w2v_arch: cbow): the layout checks and the fp64 reference, no GPU."""
import numpy as np
import pytest

from swiftsnails_amd.models.word2vec import W2VSynth, cbow_window_reference


@pytest.mark.parametrize("kw", [dict(arch="cbow", mode="pairs"),
                                dict(arch="cbow", neg_mode="per_pair"), dict(arch="nope")])
def test_cbow_arch_is_checked(kw):
    with pytest.raises(ValueError):
        W2VSynth(**kw)


def test_cbow_layout_is_the_window_layout():
    assert W2VSynth(arch="cbow").n_keys == W2VSynth().n_keys
    assert W2VSynth().arch == "skipgram"


def test_cbow_reference_gradients_are_its_loss_gradients():
    """Central differences of its own loss; an untrained center, unused window rows."""
    T, Q, S, D = 3, 7, 2, 4
    rng = np.random.default_rng(0)
    rows = [rng.standard_normal((n, D)) for n in (Q, T, S)]
    mask = np.array([[0, 1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 1, 0]], bool)
    f = lambda: cbow_window_reference(*rows, mask, 5 / 64)  # noqa: E731
    loss, trained, *grads = f()
    assert trained == 2 and not grads[1][1].any() and not grads[0][[0, 4, 6]].any()
    for a, g in zip(rows, grads):
        fd = np.zeros_like(a)
        for i in np.ndindex(a.shape):
            keep = a[i]
            a[i] = keep + 1e-6
            up = f()[0]
            a[i] = keep - 1e-6
            fd[i] = (up - f()[0]) / 2e-6
            a[i] = keep
        # atol: the difference quotient's own rounding, ~ulp(loss) / eps = 4e-16 * 3 / 1e-6
        np.testing.assert_allclose(g, fd, rtol=1e-6, atol=2e-9)
