"""Host check of ``qc.grad.exchange_jk`` (no GPU): the one closure through which both excited-state gradient
drivers form J and the exchange of the functional, hyb K + (alpha - hyb) K_LR, on a stub SCF object whose
``get_jk`` / ``get_k_lr`` return recognisable matrices."""
import numpy as np
import pytest

from xtddft_amd.qc import grad as G


class StubSCF:
    """J[D] = 2 D, K[D] = 3 D, K_LR[D] = 5 D; records how it was called."""

    def __init__(self):
        self.jk_calls, self.lr_calls = [], 0

    def get_jk(self, dm=None, hermi=1, with_k=True):
        self.jk_calls.append((hermi, with_k))
        return 2.0 * dm, (3.0 * dm if with_k else None)

    def get_k_lr(self, dm):
        self.lr_calls += 1
        return 5.0 * dm


@pytest.mark.parametrize("rsh", [None, (0.33, 0.65)])
@pytest.mark.parametrize("hyb", [0.0, 0.2, 1.0])
def test_exchange_jk_branches(hyb, rsh):
    """(J, K) of every branch, in the operations of the closure (so equal to the last bit), for a stack of
    non-symmetric densities; full-range exchange is formed exactly when hyb != 0 and the long-range one
    exactly when there is a range separation with alpha != hyb."""
    scf = StubSCF()
    d = np.random.default_rng(7).standard_normal((4, 5, 5))
    vj, vk = G.exchange_jk(scf, hyb, rsh)(tuple(d))
    np.testing.assert_array_equal(vj, 2.0 * d)
    if rsh is None:
        want = np.zeros_like(d) if hyb == 0 else hyb * (3.0 * d)
    else:
        lr = (rsh[1] - hyb) * (5.0 * d)
        want = lr if hyb == 0 else hyb * (3.0 * d) + lr
    np.testing.assert_array_equal(vk, want)
    assert vk.shape == d.shape
    assert scf.jk_calls == [(0, hyb != 0)]             # one call, hermi = 0, with_k=False exactly when hyb == 0
    assert scf.lr_calls == (0 if rsh is None else 1)


def test_exchange_jk_without_a_long_range_part():
    """alpha = hyb leaves no long-range exchange: ``get_k_lr`` is not called."""
    scf = StubSCF()
    d = np.arange(18.0).reshape(2, 3, 3)
    vj, vk = G.exchange_jk(scf, 0.25, (0.2, 0.25))(d)
    np.testing.assert_array_equal(vk, 0.25 * (3.0 * d))
    assert scf.lr_calls == 0 and scf.jk_calls == [(0, True)]
