"""GPU tests of the VAE criterion (csrc/vae_loss.hip) through ops.elementwise_loss / gauss_sample_kl /
gauss_backward, fmdiff.nn.losses, reparameterize_kl, VAECriterion and VAEEngine.kl_forward.

Kernel level: every term, reduction and addressing against the fp64 restatement of vae_loss_bounds.py within the
derived bounds, no element exempt; NaN in the head layout's padding channels; every output and workspace between
sentinel guards; shapes one short of, at and one past the per-workgroup count, odd 2-D and 3-D shapes, a
many-workgroup shape and a base pointer off the 16-byte grid (the scalar path).  Then the posterior kernel and its
backward, the reference's recorded values and gradients, run-to-run bits, graph capture, the engine path and the
refusals.  Every case prints its observed error / bound.
"""
import json
import os
import types
import warnings

import pytest
import torch

import test_gpu_vq as tg
import vae_loss_bounds as lb

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
G = 0.7
NAN = float("nan")
CHUNK, ROWS, GROWS = 2048, 512, 256   # FMD_VAE_LOSS_CHUNK, FMD_VAE_LOSS_ROWS, FMD_GAUSS_ROWS

# name -> (shape of the term [N, C, *sp], head layout?)
CASES = {
    "flat_2x3x5x7": ((2, 3, 5, 7), False), "flat_2x1x3x5x7": ((2, 1, 3, 5, 7), False),
    "flat_chunk_minus_1": ((1, 1, CHUNK - 1), False), "flat_chunk": ((1, 1, CHUNK), False),
    "flat_chunk_plus_1": ((1, 1, CHUNK + 1), False), "flat_2x1x256x256": ((2, 1, 256, 256), False),
    "flat_unaligned_1001": ((1, 1, 1001), False),
    "head_2x1x5x7": ((2, 1, 5, 7), True), "head_2x3x5x7": ((2, 3, 5, 7), True), "head_2x3x3x5x7": ((2, 3, 3, 5, 7), True),
    "head_rows_minus_1": ((1, 3, ROWS - 1), True), "head_rows": ((1, 1, ROWS), True),
    "head_rows_plus_1": ((1, 3, ROWS + 1), True), "head_2x1x256x256": ((2, 1, 256, 256), True),
}
_inputs = {}
_fx = {}


def fixture():
    if not _fx:
        _fx.update(torch.load(os.path.join(HERE, "golden", "vae_loss_golden.pt"), weights_only=True))
    return _fx


def _kind(term):
    return "rec" if term in ("l1", "mse") else ("logit" if term in lb.TARGET_TERMS else "free")


def _case(name, term):
    """(x channels-first, target or None, per-element g) on the device, made once and never modified."""
    key = (name, _kind(term))
    if key not in _inputs:
        shape, _ = CASES[name]
        g = lb.gen(f"vae_loss_gpu/{name}/{key[1]}")
        t = None
        if key[1] == "rec":
            x, t = lb.plant_rec(torch.randn(shape, generator=g) * 1.2, torch.rand(shape, generator=g))
        elif key[1] == "logit":
            x, t = lb.plant_logits(torch.randn(shape, generator=g) * 3.0, torch.rand(shape, generator=g))
        else:
            x = lb.plant_disc(torch.randn(shape, generator=g) * 1.5)
        ge = torch.randn(shape, generator=g)
        _inputs[key] = tuple(None if v is None else v.to(DEV) for v in (x, t, ge))
    return _inputs[key]


def _to_head(x_cf, ld=8):
    """channels-first -> channels-last with NaN padding channels up to ld."""
    N, C = x_cf.shape[:2]
    out = torch.full((N, *x_cf.shape[2:], ld), NAN, device=DEV)
    out[..., :C] = x_cf.movedim(1, -1)
    return out


def _from_head(x_head, C):
    return x_head[..., :C].movedim(-1, 1).contiguous()


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


class Guarded:
    """Preallocated outputs between sentinel guards."""

    def __init__(self):
        self.bufs = {}

    def make(self, key, shape, dtype=torch.float32, fill=NAN):
        view, buf = tg._sentinel(tuple(shape), dtype, fill)
        self.bufs[key] = (buf, fill)
        return view

    def check(self, name):
        torch.cuda.synchronize()
        for key, (buf, fill) in self.bufs.items():
            assert tg._guards_intact(buf, fill), f"{name}: {key}: guard overwritten"


def _run_term(name, term, reduction, g, scale=1.0, everything=True):
    """One launch for the loss and one for the gradient (and one for everything at once): LossOut pieces."""
    from fmdiff.runtime import ops
    shape, head = CASES[name]
    x_cf, t, _ = _case(name, term)
    C = shape[1]
    if head:
        x = _to_head(x_cf)
    elif "unaligned" in name:
        x = torch.empty(x_cf.numel() + 1, device=DEV)[1:].view(shape).copy_(x_cf)
        assert x.data_ptr() % 16 == 4
    else:
        x = x_cf
    kw = dict(reduction=reduction, channels=C if head else None)
    need = int(ops._lib.lib().fmd_vae_loss_workspace(ops.LOSS_TERMS[term], shape[0] if head else 1, C if head else 1,
                                                     x_cf.numel() // (shape[0] * C) if head else x_cf.numel(),
                                                     8 if head else 0))
    per = ROWS * C if head else CHUNK
    assert need == 8 * -(-x_cf.numel() // per), (name, need)
    gd = Guarded()
    out = {"loss": gd.make("loss", ()), "elem": gd.make("elem", shape), "dx": gd.make("dx", x.shape)}
    ws = gd.make("ws", (need,), torch.uint8, 0xA5)
    if head:
        out["dx_bf16"] = gd.make("dx_bf16", (*x.shape[:-1], 8), torch.bfloat16)
    fwd = ops.elementwise_loss(term, x, t, out=out, ws=ws, **kw)
    bwd = ops.elementwise_loss(term, x, t, g=g, scale=scale, loss=False, grad=True, grad_bf16=head, out=out, **kw)
    val = (fwd.elem if reduction == "none" else fwd.loss).clone()
    dx, dxb = bwd.dx.clone(), None if bwd.dx_bf16 is None else bwd.dx_bf16.clone()
    gd.check(f"{name}/{term}/{reduction}")
    if everything:   # every output from ONE launch: the same bits
        both = ops.elementwise_loss(term, x, t, g=g, scale=scale, grad=True, grad_bf16=head, **kw)
        assert torch.equal(both.elem if reduction == "none" else both.loss, val), "loss: one launch vs two"
        assert torch.equal(both.dx, dx, ), "dx: one launch vs two"
        if head:
            assert torch.equal(_bits(both.dx_bf16), _bits(dxb))
    return val, dx, dxb


# terms without a target take flat addressing only (the head layout refuses them: test_refusals)
@pytest.mark.parametrize("name,term", [(n, t) for n, (_, head) in CASES.items() for t in lb.TERMS
                                       if not head or t in lb.TARGET_TERMS])
def test_terms_against_fp64(name, term):
    shape, head = CASES[name]
    x, t, ge = _case(name, term)
    C = shape[1]
    ratios = {}
    for reduction in lb.REDUCTIONS:
        g = ge if reduction == "none" else torch.tensor([G], device=DEV)
        scale = 0.5 if reduction == "sum" else 1.0
        val, dx, dxb = _run_term(name, term, reduction, g, scale)
        want, b = lb.loss64(term, x, t, reduction)
        ratios[reduction] = lb.check(name, val, want, b, f"{term}/{reduction}")
        want, b = lb.grad64(term, x, t, reduction, ge if reduction == "none" else G, scale)
        if head:
            assert bool((dx[..., C:] == 0).all()), f"{name}: {term}: padding channels of dx"
            assert torch.equal(_bits(dxb), lb.f2bf(dx)), f"{name}: {term}: bf16 copy is not f2bf of the fp32 one"
            dx = _from_head(dx, C)
        ratios[reduction + ".dx"] = lb.check(name, dx, want, b, f"{term}/{reduction}.dx")
    print(f"{name}/{term}: error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def test_planted_kinks_give_the_stated_gradients():
    """x = +-1 passes gradient, |x| > 1 gives 0, img == t gives 0; the hinges give 0 at their kinks; +-100 finite."""
    name = "flat_2x3x5x7"
    one = torch.tensor([1.0], device=DEV)
    x, t, _ = _case(name, "l1")
    for term in ("l1", "mse"):
        _, dx, _ = _run_term(name, term, "sum", one, everything=False)
        d = dx.view(-1)
        assert bool((d[:4] != 0).all()) and bool((d[4:8] == 0).all()), (term, d[:8])
        assert float(d[8]) == 0.0 and float(d[9]) == 0.0 and float(d[10]) == 0.0, (term, d[8:11])
        if term == "l1":
            assert bool((d[:4].abs() == 0.5).all())
    for term, at, other in (("hinge_real", 0, 1), ("hinge_fake", 1, 0)):
        _, dx, _ = _run_term(name, term, "sum", one, everything=False)
        assert float(dx.view(-1)[at]) == 0.0 and abs(float(dx.view(-1)[other])) == 1.0
    for term in ("bce", "focal", "bce_focal"):
        val, dx, _ = _run_term(name, term, "none", torch.ones(CASES[name][0], device=DEV), everything=False)
        assert bool(torch.isfinite(val.view(-1)[:15]).all()) and bool(torch.isfinite(dx.view(-1)[:15]).all())


# ------------------------------------------------------------------ posterior kernel
# name -> (N, E, spatial, ldm)
GAUSS = {"fix_2x4x5x7": (2, 4, (5, 7), 8), "e3_ld16_3x5x7": (2, 3, (3, 5, 7), 16), "rows_minus_1": (2, 4, (GROWS - 1,), 8),
         "rows": (1, 4, (GROWS,), 8), "rows_plus_1": (3, 4, (GROWS + 1,), 8), "e10_2x33x17": (2, 10, (33, 17), 24)}


def _gauss_case(name):
    if ("gauss", name) not in _inputs:
        N, E, sp, ldm = GAUSS[name]
        g = lb.gen(f"vae_loss_gpu/gauss/{name}")
        m = lb.plant_logvar(torch.randn(N, 2 * E, *sp, generator=g) * 2.0)
        extra = [torch.randn(N, E, *sp, generator=g) for _ in range(2)] + [torch.randn(N, generator=g)]
        _inputs[("gauss", name)] = tuple(v.to(DEV) for v in (m, *extra))
    return _inputs[("gauss", name)]


@pytest.mark.parametrize("name", list(GAUSS))
def test_posterior_against_fp64(name):
    from fmdiff.runtime import ops
    from fmdiff.runtime.engine import CPAD
    from fmdiff.runtime.vae_engine import VAEEngine
    N, E, sp, ldm = GAUSS[name]
    m_cf, eps, g_z, g_kl = _gauss_case(name)
    m = _to_head(m_cf, ldm)
    Cp = max(CPAD, -(-E // 8) * 8)
    P = m_cf[0, 0].numel()
    need = int(ops._lib.lib().fmd_gauss_workspace(N, E, P))
    assert need == 8 * N * -(-P // GROWS)
    ratios = {}
    for tag, e in (("sample", eps), ("mode", None)):
        gd = Guarded()
        out = {"z": gd.make("z", (N, E, *sp)), "kl": gd.make("kl", (N,)),
               "z_staged": gd.make("zs", (N, *sp, Cp), torch.bfloat16)}
        z, kl, zs = ops.gauss_sample_kl(m, E, e, Cp=Cp, out=out, ws=gd.make("ws", (need,), torch.uint8, 0xA5))
        gd.check(f"{name}/{tag}")
        r = lb.gauss64(m_cf, e)
        if e is None:
            assert torch.equal(z, m_cf[:, :E]), f"{name}: the mode is mu"
        else:
            ratios["z"] = lb.check(name, z, r["z"], r["bz"], "z")
        ratios[f"kl.{tag}"] = lb.check(name, kl, r["kl"], r["bkl"], "kl")
        staged = VAEEngine._stage(types.SimpleNamespace(m=None), z)
        assert staged.shape == zs.shape and torch.equal(_bits(zs), _bits(staged)), f"{name}: staged operand"
        # a sample's KL does not depend on N or on its place in the batch
        for n in range(N):
            _, kl1, _ = ops.gauss_sample_kl(m[n:n + 1].contiguous(), E, None if e is None else e[n:n + 1].contiguous())
            assert torch.equal(kl1, kl[n:n + 1]), f"{name}: kl[{n}] alone differs"
        for what, gz, gk in (("both", g_z, g_kl), ("no_gz", None, g_kl), ("no_gkl", g_z, None)):
            gd = Guarded()
            out = {"d_moments": gd.make("dm", (N, *sp, ldm)), "d_moments_bf16": gd.make("dmb", (N, *sp, ldm), torch.bfloat16)}
            dm, dmb = ops.gauss_backward(m, E, e, gz, gk, ldb=ldm, out=out)
            gd.check(f"{name}/{tag}/{what}")
            assert bool((dm[..., 2 * E:] == 0).all()), f"{name}: padding channels of d_moments"
            assert torch.equal(_bits(dmb), lb.f2bf(dm)), f"{name}: bf16 copy is not f2bf of the fp32 one"
            want, b = lb.gauss_grad64(m_cf, e, gz, gk)
            ratios[f"d.{tag}.{what}"] = lb.check(name, _from_head(dm, 2 * E), want, b, f"d_moments {tag} {what}")
            if what == "both":   # the inclusive mask on the planted logvar -31, -30, 0, 20, 21
                glv = _from_head(dm, 2 * E)[:, E:].reshape(-1)[:5]
                assert float(glv[0]) == 0.0 and float(glv[4]) == 0.0 and float(glv[1]) != 0.0 and float(glv[3]) != 0.0
    print(f"{name}: error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ------------------------------------------------------------------ the reference's record
@pytest.mark.parametrize("tag", ("c1_2d", "c3_2d", "c1_3d", "c3_3d"))
def test_module_functions_against_the_reference_fixture(tag):
    from fmdiff.nn import losses as L
    fx = fixture()
    ratios = {}

    def run(fn, x, key, term, t, reduction, two=False):
        leaf = x.to(DEV).requires_grad_()
        loss = fn(leaf)
        (G * loss).sum().backward()
        xd, td = x.to(DEV), None if t is None else t.to(DEV)
        want, b = lb.loss64(term, xd, td, reduction)
        ratios[key] = lb.check(tag, loss.detach(), fx[f"{key}"].to(DEV), b + lb.ref_loss_bound(term, xd, td, reduction,
                                                                                               two_sums=two), key)
        _, b = lb.grad64(term, xd, td, reduction, G)
        gkey = key + ".grad"
        ratios[gkey] = lb.check(tag, leaf.grad, fx[gkey].to(DEV), b + lb.ref_grad_err(term, xd, td, reduction, G), gkey)

    for rt, term in (("l1", "l1"), ("mse", "mse"), ("bce", "bce"), ("focal", "bce_focal"), ("bce_focal", "bce_focal")):
        x, t = (fx[f"{tag}.rec"], fx[f"{tag}.target"]) if term in ("l1", "mse") else (fx[f"{tag}.logits"], fx[f"{tag}.soft"])
        run(lambda a: L.recon_loss(a, t.to(DEV), rt), x, f"{tag}.recon.{rt}", term, t, "mean", term == "bce_focal")
    x, t = fx[f"{tag}.logits"], fx[f"{tag}.soft"]
    for fname, term in (("focal_loss", "focal"), ("bce_focal_loss", "bce_focal")):
        for red in lb.REDUCTIONS:
            run(lambda a: getattr(L, fname)(a, t.to(DEV), alpha=0.25, gamma=2.0, reduction=red), x,
                f"{tag}.{fname}.{red}", term, t, red, term == "bce_focal")
    print(f"{tag}: error / (kernel + reference bound): " + ", ".join(f"{k.split('.', 1)[1]} {v:.3f}" for k, v in ratios.items()))


def test_hinge_regularizer_and_posterior_against_the_reference_fixture():
    from fmdiff.nn import losses as L
    from fmdiff.nn.modules.vae import reparameterize_kl
    fx = {k: v.to(DEV) for k, v in fixture().items() if k.split(".")[0] in ("disc", "vqreg", "post")}
    ratios = {}
    real, fake = fx["disc.real"].clone().requires_grad_(), fx["disc.fake"].clone().requires_grad_()
    d = L.discriminator_hinge_loss(real, fake)
    (G * d).backward()
    (vr, br), (vf, bf) = lb.loss64("hinge_real", fx["disc.real"]), lb.loss64("hinge_fake", fx["disc.fake"])
    b = br + bf + lb.ref_loss_bound("hinge_real", fx["disc.real"]) + lb.ref_loss_bound("hinge_fake", fx["disc.fake"]) \
        + 2 * lb.U * (vr + vf)
    ratios["d_loss"] = lb.check("disc", d.detach(), fx["disc.d_loss"], b, "d_loss")
    for leaf, key, term in ((real, "grad_real", "hinge_real"), (fake, "grad_fake", "hinge_fake")):
        x = fx["disc.real" if term == "hinge_real" else "disc.fake"]
        ratios[key] = lb.check("disc", leaf.grad, fx[f"disc.d_loss.{key}"],
                               lb.grad64(term, x, None, "mean", G)[1] + lb.ref_grad_err(term, x, None, "mean", G), key)
    assert float(real.grad.view(-1)[0]) == 0.0 and float(fake.grad.view(-1)[1]) == 0.0
    fake = fx["disc.fake"].clone().requires_grad_()
    gl = L.generator_hinge_loss(fake)
    (G * gl).backward()
    ratios["g_loss"] = lb.check("disc", gl.detach(), fx["disc.g_loss"], lb.loss64("neg", fx["disc.fake"])[1]
                                + lb.ref_loss_bound("neg", fx["disc.fake"]), "g_loss")
    ratios["g_loss.grad"] = lb.check("disc", fake.grad, fx["disc.g_loss.grad"],
                                     lb.grad64("neg", fx["disc.fake"], None, "mean", G)[1]
                                     + lb.ref_grad_err("neg", fx["disc.fake"], None, "mean", G), "g_loss.grad")
    lat = fx["vqreg.latents"].clone().requires_grad_()
    v = L.vq_regularizer(lat)
    (G * v).backward()
    x = fx["vqreg.latents"]
    n, sq = x.numel(), x.double().pow(2).sum()
    want, b = lb.loss64("square", x)
    ratios["vqreg"] = lb.check("vqreg", v.detach(), fx["vqreg.loss"],
                               b + (2 * lb.ref_sum_err(n, sq) + 8 * lb.U * sq) / n + 2 * lb.U * want, "vq_regularizer")
    dx, b = lb.grad64("square", x, None, "mean", G)
    ratios["vqreg.grad"] = lb.check("vqreg", lat.grad, fx["vqreg.grad"],
                                    b + 8 * lb.U * (dx.abs() + G * 2.0 * x.double().abs().mean() / n), "vqreg.grad")
    m = fx["post.moments"].clone().requires_grad_()
    z, kl = reparameterize_kl(m, fx["post.eps"])
    ((z * fx["post.g_z"]).sum() + G * kl.mean()).backward()
    r = lb.gauss64(fx["post.moments"], fx["post.eps"])
    bz, bkl = lb.ref_gauss_err(fx["post.moments"], fx["post.eps"])
    ratios["z"] = lb.check("post", z.detach(), fx["post.z"], r["bz"] + bz, "z")
    ratios["kl"] = lb.check("post", kl.detach(), fx["post.kl"], r["bkl"] + bkl, "kl")
    g_kl = torch.full((2,), G / 2, device=DEV)
    _, b = lb.gauss_grad64(fx["post.moments"], fx["post.eps"], fx["post.g_z"], g_kl)
    ratios["d_moments"] = lb.check("post", m.grad, fx["post.grad"],
                                   b + lb.ref_gauss_grad_err(fx["post.moments"], fx["post.eps"], fx["post.g_z"], g_kl),
                                   "d_moments")
    zm, klm = reparameterize_kl(fx["post.moments"], sample=False)
    assert torch.equal(zm, fx["post.mode"]) and torch.equal(klm, kl.detach())
    zr, _ = reparameterize_kl(fx["post.moments"], generator=torch.Generator(DEV).manual_seed(3))
    assert bool(torch.isfinite(zr).all()) and not torch.equal(zr, zm)
    print("error / (kernel + reference bound): " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ------------------------------------------------------------------ determinism, graph capture
def _criterion_inputs(seed, N=2, C=1, H=64, W=64, E=4):
    g = lb.gen(f"vae_loss_gpu/criterion/{seed}")
    rec = torch.randn(N, C, H, W, generator=g) * 1.2
    target = torch.rand(N, C, H, W, generator=g)
    moments = torch.randn(N, 2 * E, H // 8, W // 8, generator=g)
    eps = torch.randn(N, E, H // 8, W // 8, generator=g)
    fake = torch.randn(N, 1, H // 16, W // 16, generator=g)
    return tuple(v.to(DEV) for v in (rec, target, moments, eps, fake))


def _criterion_step(crit, rec, target, moments, eps, fake, step=3):
    """forward + backward of the whole criterion on leaves; (loss, rec.grad, moments.grad, fake.grad)."""
    from fmdiff.nn.modules.vae import reparameterize_kl
    for t in (rec, moments, fake):
        t.grad = None
    z, kl = reparameterize_kl(moments, eps)
    out = crit(rec, target, kl=kl, fake_pred=fake, global_step=step)
    (out["loss"] + 0.01 * z.sum()).backward()
    return out["loss"].detach(), rec.grad, moments.grad, fake.grad


@pytest.mark.parametrize("recon_type", ("l1", "bce_focal"))
def test_same_inputs_same_bits(recon_type):
    from fmdiff.pipelines.train.vae_lib import VAECriterion
    crit = VAECriterion({"recon_type": recon_type, "kl_weight": 1e-3, "kl_anneal_steps": 10, "gan_weight": 0.1})
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_(i in (0, 2, 4)) for i, t in enumerate(_criterion_inputs(0, H=256, W=256))]
        runs.append([t.clone() for t in _criterion_step(crit, *leaves)])
    for a, b, what in zip(*runs, ("loss", "rec.grad", "moments.grad", "fake.grad")):
        assert torch.equal(a, b), f"{recon_type}: {what} differs between two runs"
    assert bool(torch.isfinite(runs[0][0]))


@pytest.mark.parametrize("recon_type", ("l1", "bce_focal"))
def test_criterion_graph_capture_replays_on_new_inputs(recon_type):
    from fmdiff.pipelines.train.vae_lib import VAECriterion
    crit = VAECriterion({"recon_type": recon_type, "kl_weight": 1e-3, "kl_anneal_steps": 10, "gan_weight": 0.1})
    static = [t.clone().requires_grad_(i in (0, 2, 4)) for i, t in enumerate(_criterion_inputs(1))]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _criterion_step(crit, *static)          # warm-up outside the capture (allocations, the cached zero)
        for t in static:
            t.grad = None
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = _criterion_step(crit, *static)
    torch.cuda.current_stream().wait_stream(side)
    fresh = _criterion_inputs(2)
    with torch.no_grad():
        for s, f in zip(static, fresh):
            s.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    leaves = [t.clone().requires_grad_(i in (0, 2, 4)) for i, t in enumerate(fresh)]
    want = _criterion_step(crit, *leaves)
    for a, b, what in zip(got, want, ("loss", "rec.grad", "moments.grad", "fake.grad")):
        assert torch.equal(a, b), f"{recon_type}: replayed {what} differs from eager"


# ------------------------------------------------------------------ engine path
def test_engine_kl_forward():
    from fmdiff.models.vae import AutoencoderKL
    from fmdiff.nn.losses import recon_loss
    from fmdiff.runtime.vae_engine import get_vae_engine
    Gv = torch.load(os.path.join(HERE, "golden", "vae_golden.pt"), weights_only=True)
    cfg = json.loads(bytes(Gv["cfg_json"].tolist()).decode())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = AutoencoderKL(**cfg)
    vae.load_state_dict(Gv["state"])
    vae = vae.to(DEV).eval()
    img = Gv["x"].to(DEV)
    x = vae.image_to_model_range(img)
    eng = get_vae_engine(vae)
    with torch.no_grad():
        mom, K = eng._encode_nhwc(x)
    E = K // 2
    m_cf = _from_head(mom, K)
    eps = torch.randn(m_cf.shape[0], E, *m_cf.shape[2:], generator=lb.gen("vae_loss_gpu/engine")).to(DEV)
    ratios = {}
    for tag, e, sample in (("sample", eps, True), ("mode", None, False)):
        rec, z, kl = eng.kl_forward(x, e, sample=sample)
        assert torch.equal(rec, vae.decode(z)), f"{tag}: rec is not decode(z) bit for bit"
        r = lb.gauss64(m_cf, e)
        ratios[f"z.{tag}"] = lb.check("engine", z, r["z"], r["bz"] + lb.TINY, "z")
        ratios[f"kl.{tag}"] = lb.check("engine", kl, r["kl"], r["bkl"], "kl")
    rec_d, _, _ = eng.kl_forward(x)   # eps drawn on the device
    assert rec_d.shape == rec.shape and bool(torch.isfinite(rec_d).all())
    # recon_loss on the head-layout output against the flat call on the NCHW rec
    C = rec.shape[1]
    head = _to_head(rec)
    for rt in ("l1", "mse", "bce", "bce_focal"):
        term = rt
        a, b_ = head.clone().requires_grad_(), rec.clone().requires_grad_()
        bf = []
        la, lf = recon_loss(a, img, rt, channels=C, grad_bf16=bf), recon_loss(b_, img, rt)
        (G * la).backward()
        (G * lf).backward()
        want, bound = lb.loss64(term, rec, img, "mean")
        ratios[rt] = max(lb.check("engine", la.detach(), want, bound, rt + " head"),
                         lb.check("engine", lf.detach(), want, bound, rt + " flat"))
        want, bound = lb.grad64(term, rec, img, "mean", G)
        ratios[rt + ".dx"] = max(lb.check("engine", _from_head(a.grad, C), want, bound, rt + ".dx head"),
                                 lb.check("engine", b_.grad, want, bound, rt + ".dx flat"))
        assert bool((a.grad[..., C:] == 0).all()) and torch.equal(_bits(bf[0]), lb.f2bf(a.grad))
    print("engine: error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ------------------------------------------------------------------ refusals
def test_refusals():
    from fmdiff.nn import losses as L
    from fmdiff.nn.modules.vae import reparameterize_kl
    from fmdiff.runtime import ops
    x, t = torch.zeros(2, 3, 4, 6, device=DEV), torch.zeros(2, 3, 4, 6, device=DEV)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.elementwise_loss("l1", x, t[:, :2].contiguous())
    with pytest.raises(ValueError, match="shape mismatch"):
        L.focal_loss(x, t[:1].contiguous())
    with pytest.raises(RuntimeError, match="contiguous"):
        L.recon_loss(x.transpose(2, 3), t.transpose(2, 3), "l1")
    with pytest.raises(RuntimeError, match="fp32"):
        L.bce_focal_loss(x.half(), t)
    with pytest.raises(RuntimeError, match="fp32"):
        L.generator_hinge_loss(x.double())
    with pytest.raises(NotImplementedError, match="gamma"):
        L.focal_loss(x, t, gamma=1.0)
    with pytest.raises(ValueError, match="Unsupported recon_type 'huber'"):
        L.recon_loss(x, t, "huber")
    with pytest.raises(ValueError, match="unknown term"):
        ops.elementwise_loss("huber", x, t)
    with pytest.raises(ValueError, match="flat addressing"):
        ops.elementwise_loss("square", x.movedim(1, -1).contiguous(), None, channels=3)
    with pytest.raises(ValueError, match="head layout"):
        ops.elementwise_loss("l1", x.movedim(1, -1).contiguous(), t, channels=4)
    with pytest.raises(ValueError, match="empty"):
        ops.elementwise_loss("l1", x[:0], t[:0])
    with pytest.raises(ValueError, match="upstream gradient"):
        ops.elementwise_loss("l1", x, t, grad=True)
    with pytest.raises(ValueError, match="g must have"):
        ops.elementwise_loss("l1", x, t, grad=True, g=torch.zeros(3, device=DEV))
    with pytest.raises(RuntimeError, match="workspace"):
        ops.elementwise_loss("l1", x, t, ws=torch.zeros(4, dtype=torch.uint8, device=DEV))
    lib = ops._lib.lib()
    assert lib.fmd_vae_loss_workspace(0, 1, 1, 0, 0) == -1 and lib.fmd_vae_loss_workspace(9, 1, 1, 8, 0) == -1
    assert lib.fmd_vae_loss_workspace(0, 1, 9, 8, 8) == -1 and lib.fmd_vae_loss_workspace(5, 1, 1, 8, 8) == -1
    assert lib.fmd_vae_loss_workspace(0, 1, 1, (2 ** 31) * CHUNK, 0) == -1      # a grid beyond 2^31 - 1
    assert lib.fmd_vae_loss_workspace(0, 1, 1, (2 ** 31 - 1) * CHUNK, 0) == 8 * (2 ** 31 - 1)
    assert lib.fmd_gauss_workspace(0, 4, 8) == -1 and lib.fmd_gauss_workspace(2 ** 30, 4, 3 * GROWS) == -1
    m = torch.zeros(2, 8, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="moments"):
        reparameterize_kl(m[:, :7].contiguous())
    with pytest.raises(ValueError, match="eps must be"):
        reparameterize_kl(m, torch.zeros(2, 4, 4, 5, device=DEV))
    with pytest.raises(RuntimeError, match="fp32"):
        reparameterize_kl(m, torch.zeros(2, 4, 4, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="embed_dim"):
        reparameterize_kl(m.movedim(1, -1).contiguous(), channels_last=True)
