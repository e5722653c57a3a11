"""CPU checks of tests/pointwise_bounds.py: the fp64 restatement of the latent 1x1 conv backward equals autograd of
``F.conv2d`` and the exact reference, and the exported bound behaves as derived."""
import pytest
import torch
import torch.nn.functional as F

import pointwise_bounds as PB


def _case(N, h, w, Z, E, ldy, ldx, seed):
    g = torch.Generator().manual_seed(seed)
    dy = PB.bf16_valued((N * h * w, ldy), g, 0.5)
    x = PB.bf16_valued((N * h * w, ldx), g)
    dy[:, Z:] = float("nan")     # the padding channels never enter a result
    x[:, E:] = float("nan")
    W = torch.randn((Z, E), generator=g) / 2
    return dy, x, W


@pytest.mark.parametrize("Z,E", [(4, 4), (3, 5), (8, 8), (1, 1)])
def test_restatement_equals_conv2d_autograd(Z, E):
    N, h, w = 3, 5, 7
    dy, x, W = _case(N, h, w, Z, E, 8, 16, 11 + Z)
    g, dW, db = PB.kernel_fp64(dy, x, W)
    xi = x[:, :E].double().reshape(N, h, w, E).permute(0, 3, 1, 2).contiguous().requires_grad_()
    wt = W.double().reshape(Z, E, 1, 1).clone().requires_grad_()
    b = torch.zeros(Z, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xi, wt, b)
    y.backward(dy[:, :Z].double().reshape(N, h, w, Z).permute(0, 3, 1, 2).contiguous())
    for got, ref in ((g, xi.grad.permute(0, 2, 3, 1).reshape(-1, E)), (dW, wt.grad.reshape(Z, E)), (db, b.grad)):
        assert not torch.isnan(got).any()
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
    (ge, dWe, dbe), (ga, dWa, dba) = PB.exact(dy, x, W)
    M = N * h * w
    for got, ref, at, n in ((g, ge, ga, Z), (dW, dWe, dWa, M), (db, dbe, dba, M)):
        assert ((got - ref).abs() <= PB.gamma(n) * at).all()      # the fp64 summation error alone


def test_bound_holds_for_the_rounded_restatement_and_is_tight_enough_to_catch_bf16():
    dy, x, W = _case(2, 9, 8, 4, 4, 8, 8, 3)
    g, dW, db = PB.kernel_fp64(dy, x, W)
    (ge, dWe, dbe), (ga, dWa, dba) = PB.exact(dy, x, W)
    M = dy.shape[0]
    old = torch.randn((4, 4), generator=torch.Generator().manual_seed(9))
    assert ((g.float().double() - ge).abs() <= PB.bound(ge, ga, 4)).all()
    assert ((dW.float().double() - dWe).abs() <= PB.bound(dWe, dWa, M)).all()
    assert ((db.float().double() - dbe).abs() <= PB.bound(dbe, dba, M)).all()
    acc = (old + dW.float()).double()
    assert ((acc - (old.double() + dWe)).abs() <= PB.bound(dWe, dWa, M, old=old)).all()
    # a gradient rounded to bf16 on the way (the MFMA route this kernel replaces) misses the bound
    rounded = g.to(torch.bfloat16).double()
    assert ((rounded - ge).abs() > PB.bound(ge, ga, 4)).any()
    assert PB.gamma(1000) < 1.2e-13 and PB.gamma(1) == pytest.approx(2.0 ** -53)
