"""CPU checks of tests/vae_loss_bounds.py, the fp64 restatement the GPU tests of csrc/vae_loss.hip lean on:

* it reproduces every value and gradient the reference recorded in tests/golden/vae_loss_golden.pt within the
  reference's own fp32 error bound (no element left out: the planted kinks and saturated logits included);
* its analytic gradients equal torch autograd of an independently written fp64 forward;
* the identity behind vq_regularizer (= mean(x^2)) holds against the reference's formula as restated;
* the bounds have teeth: an exclusive clamp mask, sign(0) = 1 and a focal term built as 1 - p_t miss them.
"""
import os

import pytest
import torch

import vae_loss_bounds as lb

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ("c1_2d", "c3_2d", "c1_3d", "c3_3d")
RECON = {"l1": "l1", "mse": "mse", "bce": "bce", "focal": "bce_focal", "bce_focal": "bce_focal"}
_fx = {}


def fixture():
    if not _fx:
        _fx.update(torch.load(os.path.join(HERE, "golden", "vae_loss_golden.pt"), weights_only=True))
    return _fx


def _xt(fx, tag, term):
    return (fx[f"{tag}.rec"], fx[f"{tag}.target"]) if term in ("l1", "mse") else (fx[f"{tag}.logits"], fx[f"{tag}.soft"])


def test_fixture_holds_the_planted_values():
    fx = fixture()
    for tag in TAGS:
        rec, tgt = fx[f"{tag}.rec"].view(-1), fx[f"{tag}.target"].view(-1)
        assert rec[0] == 1.0 and rec[1] == -1.0 and 0 < 1.0 - rec[2] < 1e-7 and 0 < rec[4] - 1.0 < 2e-7
        assert torch.equal(lb.img32(rec[8:11]), tgt[8:11])
        lg, soft = fx[f"{tag}.logits"].view(-1), fx[f"{tag}.soft"].view(-1)
        assert lg[0] == 100.0 and lg[3] == -100.0 and lg[12] == 0.0 and soft[0] == 0.0 and soft[1] == 1.0
        assert 0.0 < float(soft[2]) < 1.0 and bool(((soft == 0) | (soft == 1)).sum() > 15)
    lv = fx["post.moments"][:, 4:].reshape(-1)[:5]
    assert lv.tolist() == [-31.0, -30.0, 0.0, 20.0, 21.0]
    assert fx["disc.real"].view(-1)[0] == 1.0 and fx["disc.fake"].view(-1)[1] == -1.0


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_losses(tag):
    fx = fixture()
    g = float(fx["hyper"][0])
    ratios = {}
    for rt, term in RECON.items():
        x, t = _xt(fx, tag, term)
        want, _ = lb.loss64(term, x, t, "mean")
        ratios[f"recon.{rt}"] = lb.check(tag, fx[f"{tag}.recon.{rt}"], want,
                                         lb.ref_loss_bound(term, x, t, "mean", two_sums=term == "bce_focal"), rt)
        dx, _ = lb.grad64(term, x, t, "mean", g)
        ratios[f"recon.{rt}.grad"] = lb.check(tag, fx[f"{tag}.recon.{rt}.grad"], dx,
                                              lb.ref_grad_err(term, x, t, "mean", g), rt + ".grad")
    x, t = fx[f"{tag}.logits"], fx[f"{tag}.soft"]
    for fn, term in (("focal_loss", "focal"), ("bce_focal_loss", "bce_focal")):
        for red in lb.REDUCTIONS:
            want, _ = lb.loss64(term, x, t, red)
            key = f"{fn}.{red}"
            ratios[key] = lb.check(tag, fx[f"{tag}.{key}"], want,
                                   lb.ref_loss_bound(term, x, t, red, two_sums=term == "bce_focal"), key)
            dx, _ = lb.grad64(term, x, t, red, g)
            ratios[key + ".grad"] = lb.check(tag, fx[f"{tag}.{key}.grad"], dx, lb.ref_grad_err(term, x, t, red, g),
                                             key + ".grad")
            assert bool(torch.isfinite(fx[f"{tag}.{key}.grad"]).all())
    print(f"{tag}: reference error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def test_restatement_reproduces_the_reference_hinge_regularizer_and_posterior():
    fx = fixture()
    g = float(fx["hyper"][0])
    real, fake = fx["disc.real"], fx["disc.fake"]
    (vr, _), (vf, _) = lb.loss64("hinge_real", real), lb.loss64("hinge_fake", fake)
    b = lb.ref_loss_bound("hinge_real", real) + lb.ref_loss_bound("hinge_fake", fake) + lb.U * (vr + vf)
    ratios = {"d_loss": lb.check("disc", fx["disc.d_loss"], vr + vf, b, "d_loss")}
    for key, term, x in (("d_loss.grad_real", "hinge_real", real), ("d_loss.grad_fake", "hinge_fake", fake),
                         ("g_loss.grad", "neg", fake)):
        ratios[key] = lb.check("disc", fx[f"disc.{key}"], lb.grad64(term, x, None, "mean", g)[0],
                               lb.ref_grad_err(term, x, None, "mean", g), key)
    # exactly at the kink the gradient is zero
    assert fx["disc.d_loss.grad_real"].view(-1)[0] == 0.0 and fx["disc.d_loss.grad_fake"].view(-1)[1] == 0.0
    ratios["g_loss"] = lb.check("disc", fx["disc.g_loss"], lb.loss64("neg", fake)[0], lb.ref_loss_bound("neg", fake),
                                "g_loss")
    # vq_regularizer: the reference's two-term formula, restated, and the square term it is built as
    lat = fx["vqreg.latents"]
    n = lat.numel()
    two = lb.vq_regularizer_ref64(lat)
    # reference: two means of n squares each, the per-channel mean (an fp32 sum of n / C terms) and one addition
    sq = lat.double().pow(2).sum()
    b = (2 * lb.ref_sum_err(n, sq) + 8 * lb.U * sq) / n + 2 * lb.U * two
    ratios["vqreg"] = lb.check("vqreg", fx["vqreg.loss"], two, b, "loss")
    ratios["vqreg.square"] = lb.check("vqreg", fx["vqreg.loss"], lb.loss64("square", lat)[0], b, "loss as mean(x^2)")
    # its gradient through the reference's graph is 2 x g / n up to the roundings of the two paths
    dx, _ = lb.grad64("square", lat, None, "mean", g)
    ratios["vqreg.grad"] = lb.check("vqreg", fx["vqreg.grad"], dx,
                                    8 * lb.U * (dx.abs() + g * 2.0 * lat.double().abs().mean() / n), "grad")
    m, eps, g_z = fx["post.moments"], fx["post.eps"], fx["post.g_z"]
    r = lb.gauss64(m, eps)
    bz, bkl = lb.ref_gauss_err(m, eps)
    ratios["z"] = lb.check("post", fx["post.z"], r["z"], bz + lb.TINY, "z")
    ratios["kl"] = lb.check("post", fx["post.kl"], r["kl"], bkl, "kl")
    g_kl = torch.full((m.shape[0],), g / m.shape[0], dtype=torch.float32)
    d, _ = lb.gauss_grad64(m, eps, g_z, g_kl)
    ratios["d_moments"] = lb.check("post", fx["post.grad"], d, lb.ref_gauss_grad_err(m, eps, g_z, g_kl) + lb.TINY,
                                   "d_moments")
    # the inclusive clamp mask, on the planted logvar -31, -30, 0, 20, 21
    glv = fx["post.grad"][:, 4:].reshape(-1)[:5]
    assert glv[0] == 0.0 and glv[4] == 0.0 and float(glv[1]) != 0.0 and float(glv[3]) != 0.0
    assert torch.equal(fx["post.mode"], m[:, :4])
    print("reference error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def _plain64(term, x, t, alpha=lb.ALPHA):
    """The forward written the way the reference writes it, in fp64 (an independent statement)."""
    if term in ("l1", "mse"):
        d = (x.clamp(-1.0, 1.0) + 1.0) * 0.5 - t
        return d.abs() if term == "l1" else d * d
    if term in ("bce", "focal", "bce_focal"):
        ce = torch.logaddexp(torch.zeros_like(x), x) - x * t
        p = torch.sigmoid(x)
        p_t = p * t + (1 - p) * (1 - t)
        foc = (alpha * t + (1 - alpha) * (1 - t)) * (1 - p_t).pow(2.0) * ce
        return ce if term == "bce" else (foc if term == "focal" else ce + foc)
    return {"hinge_real": lambda: torch.relu(1.0 - x), "hinge_fake": lambda: torch.relu(1.0 + x),
            "neg": lambda: -x, "square": lambda: x * x}[term]()


@pytest.mark.parametrize("term", lb.TERMS)
def test_analytic_gradients_equal_autograd_in_fp64(term):
    fx = fixture()
    for tag in ("c3_2d", "c1_3d"):
        x32, t32 = _xt(fx, tag, term)
        x = x32.double().requires_grad_()
        t = t32.double() if term in lb.TARGET_TERMS else None
        plain = _plain64(term, x, t)
        (auto,) = torch.autograd.grad(plain.sum(), x)
        r = lb.term64(term, x.detach(), t)   # fp64 in: img is formed in fp64 on both sides here
        # the plain forward cancels where the restatement does not (1 - p_t, log(1 + e^x) - x t): absolute 1e-12
        # on values of order |x| + 1
        tol = 1e-12 * (1.0 + x32.double().abs())
        assert bool(((r["v"] - plain.detach()).abs() <= tol).all()), term
        assert bool(((r["u"] - auto).abs() <= tol).all()), term
        assert bool((r["mv"] >= r["v"].abs() * (1 - 1e-12)).all()) and bool((r["mu"] >= r["u"].abs() * (1 - 1e-12)).all())


def test_posterior_gradients_equal_autograd_in_fp64():
    fx = fixture()
    m32, eps, g_z = fx["post.moments"], fx["post.eps"], fx["post.g_z"]
    g_kl = torch.tensor([0.35, -1.25])
    for e, gz, gk in ((eps, g_z, g_kl), (None, g_z, g_kl), (eps, None, g_kl), (eps, g_z, None)):
        m = m32.double().requires_grad_()
        mu, raw = torch.chunk(m, 2, dim=1)
        lv = raw.clamp(-30.0, 20.0)
        z = mu + torch.exp(0.5 * lv) * e.double() if e is not None else mu
        kl = 0.5 * torch.sum(mu.pow(2) + torch.exp(lv) - 1.0 - lv, dim=(1, 2, 3))
        obj = torch.zeros((), dtype=torch.float64)
        if gz is not None:
            obj = obj + (z * gz.double()).sum()
        if gk is not None:
            obj = obj + (kl * gk.double()).sum()
        (auto,) = torch.autograd.grad(obj, m)
        d, _ = lb.gauss_grad64(m32, e, gz, gk)
        scale = 1.0 + auto.abs() + torch.cat([torch.zeros_like(mu), torch.exp(lv)], dim=1).detach()
        assert bool(((d - auto).abs() <= 1e-12 * scale).all())
        r = lb.gauss64(m32, e)
        assert bool(((r["z"] - z.detach()).abs() <= 1e-12 * (1 + z.detach().abs())).all())
        assert bool(((r["kl"] - kl.detach()).abs() <= 1e-12 * (1 + kl.detach().abs())).all())


def test_vq_regularizer_is_the_mean_square():
    """mean(mean_c^2) + mean((x - mean_c)^2) == mean(x^2): the per-channel mean terms cancel."""
    for shape, seed in (((2, 4, 5, 7), 0), ((3, 5, 9), 1), ((2, 3, 3, 5, 7), 2), ((1, 1, 1, 1), 3)):
        x = torch.randn(shape, generator=lb.gen(f"vqreg/{seed}"), dtype=torch.float64) * 3.0 + 1.5
        two, one = lb.vq_regularizer_ref64(x), (x * x).mean()
        assert abs(float(two - one)) <= 64 * lb.U64 * float(one), shape
        x = x.requires_grad_()
        (g2,) = torch.autograd.grad(lb.vq_regularizer_ref64(x), x)
        assert bool(((g2 - 2.0 * x.detach() / x.numel()).abs() <= 64 * lb.U64 * (1 + x.detach().abs()) / x.numel() * 8).all())


def test_bounds_have_teeth():
    """Three wrong kernels one could write, each on the planted elements, each far outside the kernel bound."""
    fx = fixture()
    x, t = fx["c3_2d.rec"], fx["c3_2d.target"]
    dx, b = lb.grad64("l1", x, t, "sum", 1.0)
    d = lb.img32(x).double() - t.double()
    exclusive = torch.sign(d) * 0.5 * ((x > -1.0) & (x < 1.0)).double()
    assert not bool(((exclusive - dx).abs() <= b).all())                  # x = +-1 must pass gradient
    sign_one = torch.where(d >= 0, 0.5, -0.5) * ((x >= -1.0) & (x <= 1.0)).double()
    assert not bool(((sign_one - dx).abs() <= b).all())                   # img == t must give 0
    lg, soft = fx["c3_2d.logits"], fx["c3_2d.soft"]
    v, b = lb.loss64("focal", lg, soft, "none")
    p = torch.sigmoid(lg)                                                 # fp32, 1 - p_t by subtraction
    q32 = 1 - (p * soft + (1 - p) * (1 - soft))
    at = lb.ALPHA * soft + (1 - lb.ALPHA) * (1 - soft)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(lg, soft, reduction="none")
    assert not bool((((at * q32.pow(2) * ce).double() - v).abs() <= b).all())
