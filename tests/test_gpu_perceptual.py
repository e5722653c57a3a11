"""VGGPerceptualLoss on the GPU against ``perc_bounds.perc_oracle`` (fp32 on the CPU): every tap value, the loss and
the gradient of the raw reconstruction, on seeded He-normal stacks (the narrow one and the full VGG16 widths).

Tolerances are the project's ("Discriminators"): values and loss within 1e-2 relative, gradient
relative L2 < 5e-2 and cosine > 0.99, nothing excluded."""
import functools
import math

import pytest
import torch

import perc_bounds as PB

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL, GRAD_L2, GRAD_COS = 1e-2, 5e-2, 0.99

# (widths, C, (H, W), resize)
CASES = {
    "narrow_1ch": (PB.NARROW, 1, (16, 24), None),
    "narrow_3ch_resize32": (PB.NARROW, 3, (20, 12), 32),
    "narrow_odd_levels": (PB.NARROW, 1, (20, 12), None),       # 20x12 -> 10x6 -> 5x3 -> 2x1
    "narrow_resize224": (PB.NARROW, 1, (48, 64), 224),
    "vgg16_widths": (PB.VGG16, 1, (16, 24), None),
}


def _module(widths, resize=None, **kw):
    from fmdiff.nn.losses import VGGPerceptualLoss
    return VGGPerceptualLoss(PB.build_features(widths, 0), resize=resize if resize is not None else False, **kw).to(DEV)


@functools.lru_cache(maxsize=None)
def _oracle(name, layers=(3, 8, 15, 22), weights=(1.0, 1.0, 1.0, 1.0)):
    """(recon, target, loss, values, d loss / d recon) of the fp32 CPU oracle; computed once per case, read-only."""
    widths, C, hw, resize = CASES[name]
    feats = PB.build_features(widths, 0)
    recon, target = PB.make_images(2, C, hw[0], hw[1], 11)
    r = recon.clone().requires_grad_()
    loss, values = PB.perc_oracle(feats, r, target, resize, layers, weights)
    loss.backward()
    return recon, target, float(loss.detach()), [float(v.detach()) for v in values], r.grad.clone()


def _grad_figures(got, ref):
    got, ref = got.double().flatten(), ref.double().flatten()
    l2 = float((got - ref).norm() / ref.norm())
    cos = float(torch.dot(got, ref) / (got.norm() * ref.norm()))
    return l2, cos


def _run(P, recon, target):
    r = recon.to(DEV).requires_grad_()
    loss = P(r, target.to(DEV))
    values = P.layer_values
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), values, r.grad


@pytest.mark.parametrize("name", list(CASES))
def test_loss_values_and_gradient_against_the_oracle(name):
    widths, C, hw, resize = CASES[name]
    recon, target, loss_ref, values_ref, grad_ref = _oracle(name)
    P = _module(widths, resize)
    loss, values, grad = _run(P, recon, target)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and values.shape == (4,)
    rels = [abs(float(v) - w) / abs(w) for v, w in zip(values, values_ref)]
    l2, cos = _grad_figures(grad.cpu(), grad_ref)
    print(f"{name}: loss hip {float(loss):.6f} oracle {loss_ref:.6f} rel {abs(float(loss) - loss_ref) / loss_ref:.2e}; "
          f"taps {[f'{v:.4f}' for v in values_ref]} rel {[f'{r:.1e}' for r in rels]}; grad relL2 {l2:.3e} cos {cos:.6f}")
    assert all(0.0 < v for v in values_ref)
    assert max(rels) <= REL
    assert abs(float(loss) - loss_ref) <= REL * abs(loss_ref)
    assert grad.shape == recon.shape and l2 < GRAD_L2 and cos > GRAD_COS
    # the same bits without grad mode, again after the backward, and from a second forward + backward
    with torch.no_grad():
        assert torch.equal(P(recon.to(DEV), target.to(DEV)), loss)
    loss2, values2, grad2 = _run(P, recon, target)
    assert torch.equal(loss2, loss) and torch.equal(values2, values) and torch.equal(grad2, grad)
    # the target receives no gradient, the stack none either
    t = target.to(DEV).requires_grad_()
    P(recon.to(DEV).requires_grad_(), t).backward()
    assert t.grad is None and all(p.grad is None for p in P.parameters())


def test_layer_weights_and_an_early_stop():
    name = "narrow_1ch"
    widths, C, hw, resize = CASES[name]
    for layers, weights in (((3, 8, 15, 22), (1.0, 0.5)), ((3, 8), (1.0, 1.0))):
        recon, target, loss_ref, values_ref, grad_ref = _oracle(name, layers, weights)
        P = _module(widths, resize, layers=layers, layer_weights=weights)
        loss, values, grad = _run(P, recon, target)
        assert values.shape == (len(layers),)
        assert max(abs(float(v) - w) / w for v, w in zip(values, values_ref)) <= REL
        assert abs(float(loss) - loss_ref) <= REL * loss_ref
        l2, cos = _grad_figures(grad.cpu(), grad_ref)
        print(f"layers {layers} weights {weights}: loss {float(loss):.6f} / {loss_ref:.6f}, grad relL2 {l2:.3e} cos {cos:.6f}")
        assert l2 < GRAD_L2 and cos > GRAD_COS
    # the weights matter: (1, 0.5, 1, 1) is not (1, 1, 1, 1)
    assert abs(_oracle(name, (3, 8, 15, 22), (1.0, 0.5))[2] - _oracle(name)[2]) > 0.1 * _oracle(name)[3][1]


def test_forward_image_fuses_the_map():
    widths, C, hw, resize = CASES["narrow_3ch_resize32"]
    recon, target = PB.make_images(2, C, hw[0], hw[1], 11)
    raw = (recon * 3 - 1.5)                      # a raw decoder output, partly outside [-1, 1]
    P = _module(widths, resize)
    for mode in ("clamp", "sigmoid"):
        feats = PB.build_features(widths, 0)
        r = raw.clone().requires_grad_()
        loss_ref, _ = PB.perc_oracle(feats, PB.image_map(r, mode), target, resize)
        loss_ref.backward()
        rd = raw.to(DEV).requires_grad_()
        loss = P.forward_image(rd, mode, target.to(DEV))
        loss.backward()
        l2, cos = _grad_figures(rd.grad.cpu(), r.grad)
        loss, loss_ref = float(loss.detach()), float(loss_ref.detach())
        print(f"forward_image {mode}: loss {loss:.6f} / {loss_ref:.6f}, grad relL2 {l2:.3e} cos {cos:.6f}")
        assert abs(loss - loss_ref) <= REL * loss_ref
        assert l2 < GRAD_L2 and cos > GRAD_COS
    with pytest.raises(ValueError, match="image map"):
        P.forward_image(raw.to(DEV), "tanh", target.to(DEV))


def test_load_vgg_state_dict_equals_a_fresh_module():
    widths, C, hw, resize = CASES["narrow_1ch"]
    recon, target = PB.make_images(2, C, hw[0], hw[1], 11)
    rd, td = recon.to(DEV), target.to(DEV)
    P = _module(widths, resize)
    with torch.no_grad():
        before = P(rd, td)
    other = PB.build_features(widths, 5)
    P.load_vgg_state_dict({f"features.{k}": v for k, v in other.state_dict().items()})
    from fmdiff.nn.losses import VGGPerceptualLoss
    fresh = VGGPerceptualLoss(other).to(DEV)
    with torch.no_grad():
        after = P(rd, td)
        assert torch.equal(after, fresh(rd, td)) and not torch.equal(after, before)


def test_descent_on_the_engines_gradient_follows_the_oracles():
    """8 Adam updates at lr 1e-2 of a leaf recon image, one run fed the engine's gradient and one the oracle's."""
    widths, C, hw, resize = CASES["narrow_1ch"]
    recon, target = PB.make_images(2, C, hw[0], hw[1], 11)
    feats = PB.build_features(widths, 0)
    P = _module(widths, resize)
    xe = torch.nn.Parameter(recon.clone())
    xo = torch.nn.Parameter(recon.clone())
    oe, oo = torch.optim.Adam([xe], lr=1e-2), torch.optim.Adam([xo], lr=1e-2)
    seq_e, seq_o = [], []
    for _ in range(9):
        rd = xe.detach().to(DEV).requires_grad_()
        le = P(rd, target.to(DEV))
        le.backward()
        seq_e.append(float(PB.perc_oracle(feats, xe.detach(), target, resize)[0]))   # both judged by the oracle
        xe.grad = rd.grad.cpu()
        oe.step()
        oo.zero_grad()
        lo, _ = PB.perc_oracle(feats, xo, target, resize)
        lo.backward()
        seq_o.append(float(lo.detach()))
        oo.step()
    print("descent, engine gradient:", " ".join(f"{v:.5f}" for v in seq_e))
    print("descent, oracle gradient:", " ".join(f"{v:.5f}" for v in seq_o))
    assert seq_e[-1] < 0.9 * seq_e[0] and seq_o[-1] < 0.9 * seq_o[0]
    assert abs(seq_e[-1] - seq_o[-1]) <= REL * seq_o[-1]
    assert math.isfinite(seq_e[-1])
