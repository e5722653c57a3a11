"""The GAN discriminators on the device: the 4x4 conv routes on the exact lattice, both classes against the CPU
oracle of tests/bn_bounds.py (forward, running statistics, gradients of the hinge losses with two forwards alive),
eval mode, the weight caches, and a short descent.

Tolerances are the project's: forward relative L2 < 2e-2 for a bf16 trunk; gradients: loss within
1e-2 relative, relative L2 over all parameters < 5e-2, cosine > 0.99 for every tensor above 1e-3 of the whole
gradient's norm.  The fp32 oracle's own distance from fp64 is measured beside each and must be ten times inside."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import bn_bounds as B
import conv_lattice as CL

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FWD_TOL, GRAD_TOL, LOSS_TOL, COS_TOL, COS_FLOOR = 2e-2, 5e-2, 1e-2, 0.99, 1e-3


def ops():
    from fmdiff.runtime import ops as O
    return O


# ------------------------------------------------------------------------------------------ 4x4 lattice routes
# (name, N, input H x W, C, K, stride, pad): the discriminators' three 4x4 geometries on odd sizes, more than one
# image, C = 8 (the narrow-reduction lattice "int": integer x, w in eighths)
LATTICE = [("k4_s2_p1", 3, (10, 14), 8, 16, 2, 1), ("k4_s1_p0", 3, (5, 7), 8, 16, 1, 0),
           ("k4_s1_p1", 3, (5, 7), 8, 16, 1, 1)]


@functools.lru_cache(maxsize=None)
def lattice_problem(name):
    _, N, sp, C, K, stride, pad = next(r for r in LATTICE if r[0] == name)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    L = CL.LATTICES["int"]
    osp = tuple((h + 2 * pad - 4) // stride + 1 for h in sp)
    x = CL._draw(g, (N, *sp, C), L["x"])
    w = CL._draw(g, (K, C, 4, 4), L["w"], F32)
    bias = CL._draw(g, (K,), (-8, 8, 4), F32)
    dy = CL._draw(g, (N, *osp, K), CL.LATTICES["fine"]["x"])
    xd = x.double().movedim(-1, 1).requires_grad_()
    wd, bd = w.double().requires_grad_(), bias.double().requires_grad_()
    y = F.conv2d(xd, wd, bd, stride=stride, padding=pad)
    y.backward(dy.double().movedim(-1, 1))
    R = dict(y=y.detach().movedim(1, -1).contiguous(), dx=xd.grad.movedim(1, -1).contiguous(), dw=wd.grad, db=bd.grad)
    # the exactness argument: operands survive bf16, every result is a multiple of the step and, with |operands|,
    # stays below 2^24 steps; no output row or channel is all zero; some bf16 outputs do round
    for t in (x, dy, w):
        assert torch.equal(t.double(), t.to(BF16).double())
    steps = dict(y=1 / 8, dx=1 / 32, dw=1 / 4, db=1 / 4)
    ya = F.conv2d(x.double().abs().movedim(-1, 1), w.double().abs(), bias.double().abs(), stride=stride, padding=pad)
    caps = dict(y=ya.max().item(), dx=16 * K * 2 * 0.5, dw=N * osp[0] * osp[1] * 12 * 2, db=N * osp[0] * osp[1] * 2)
    for k, v in R.items():
        q = v / steps[k]
        assert torch.equal(q, q.round()), f"{name}: {k} leaves the lattice"
        assert caps[k] < 2.0 ** 24 * steps[k]
        assert (v.reshape(-1, v.shape[-1]).abs().amax(0) > 0).all()
    rounds, _ = CL.rounding_profile(R["y"])
    assert rounds > 0.05, f"{name}: only {rounds:.3f} of the outputs round"
    return dict(x=x, w=w, bias=bias, dy=dy, sp=sp, osp=osp, stride=stride, pad=pad, K=K, C=C, N=N), R


@pytest.mark.parametrize("name", [r[0] for r in LATTICE])
def test_conv4x4_routes_exact(name):
    """Forward, transposed-gather data gradient and 16-tap weight gradient as DiscEngine issues them, bit for bit."""
    O = ops()
    P, R = lattice_problem(name)
    geom = dict(ks=4, stride=P["stride"], pad=P["pad"])
    x, w, bias, dy = (P[k].to(DEV) for k in ("x", "w", "bias", "dy"))
    N, K, C = P["N"], P["K"], P["C"]
    buf, out = CL.guarded((N, *P["osp"], K), BF16, DEV)
    O.conv(x, K, O.prep_weights(w, 0), bias=bias, out=out, **geom)
    torch.cuda.synchronize()
    assert CL.guards_intact(buf, out) and CL.unwritten(out) == 0
    CL.assert_bits(out, R["y"].to(BF16), R["y"], f"{name} forward")
    buf, out = CL.guarded((N, *P["sp"], C), BF16, DEV)
    O.conv(dy, C, O.prep_weights(w, 1), transposed=True, out_hw_=P["sp"], out=out, **geom)
    torch.cuda.synchronize()
    assert CL.guards_intact(buf, out) and CL.unwritten(out) == 0
    CL.assert_bits(out, R["dx"].to(BF16), R["dx"], f"{name} data gradient")
    dwb, dw = CL.guarded((K, C, 4, 4), F32, DEV)
    dbb, db = CL.guarded((K,), F32, DEV)
    O.wgrad(x, dy, dw, db=db, accumulate=False, **geom)
    torch.cuda.synchronize()
    assert CL.guards_intact(dwb, dw) and CL.guards_intact(dbb, db) and CL.unwritten(dw) == 0 and CL.unwritten(db) == 0
    CL.assert_bits(dw, R["dw"].float(), R["dw"], f"{name} dW")
    CL.assert_bits(db, R["db"].float(), R["db"], f"{name} db")


# --------------------------------------------------------------------------------------- whole discriminators
CASES = {"magvit": (1, (3, 1, 48, 64)), "patchgan": (3, (3, 3, 32, 48))}


def _cls(name):
    from fmdiff.nn.modules.vae.discriminators import MagvitDiscriminatorND, PatchGANDiscriminatorND
    return {"magvit": MagvitDiscriminatorND, "patchgan": PatchGANDiscriminatorND}[name]


@functools.lru_cache(maxsize=None)
def golden():
    return torch.load(os.path.join(HERE, "golden", "disc_golden.pt"), weights_only=True)


def _last_conv(sd):
    return max((k for k in sd if k.endswith(".conv.weight")), key=lambda k: int(k.split(".")[1]))


@functools.lru_cache(maxsize=None)
def setup(name, base):
    """(state_dict, real batch, fake batch): base 8 from the fixture, base 64 seeded; BatchNorm parameters and
    statistics away from their defaults; the last conv scaled so that the fp64 oracle's |logit| <= 0.9 on both
    batches (asserted), so no hinge mask can flip."""
    cin, shape = CASES[name]
    if base == 8:
        pre = f"{name}.sd."
        sd = {k[len(pre):]: v.clone() for k, v in golden().items() if k.startswith(pre)}
        real = golden()[f"{name}.x"].clone()
    else:
        torch.manual_seed(5)
        m = _cls(name)(cin, base)
        g = torch.Generator().manual_seed(6)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for k in sd:
            if k.endswith("running_mean"):
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.3
            elif k.endswith("running_var"):
                sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
            elif sd[k].dim() == 1 and ".conv." not in k and sd[k].is_floating_point():
                sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5 if k.endswith("weight") else \
                    torch.randn(sd[k].shape, generator=g) * 0.2
        real = torch.randn(shape, generator=g)
    g = torch.Generator().manual_seed(7)
    fake = (real * 0.5 + 0.5 * torch.randn(shape, generator=g)).contiguous()
    lk = _last_conv(sd)
    peak = 0.0
    for xb in (real, fake):
        lg, _ = B.disc_oracle(B.oracle_params(sd, F64), B.TABLES[name], xb.double(), True, F64)
        peak = max(peak, lg.abs().max().item())
    # to a peak of 0.5, then every logit 0.3 up: the generator loss (minus the mean logit) is then not a difference
    # near zero, which a relative tolerance could not judge
    s = 0.5 / peak
    sd[lk], sd[lk.replace("weight", "bias")] = sd[lk] * s, sd[lk.replace("weight", "bias")] * s + 0.3
    for xb in (real, fake):
        lg, _ = B.disc_oracle(B.oracle_params(sd, F64), B.TABLES[name], xb.double(), True, F64)
        assert lg.abs().max().item() <= 0.9
    return sd, real, fake


def module(name, base, sd):
    m = _cls(name)(CASES[name][0], base)
    m.load_state_dict(sd)
    return m.to(DEV)


def rel_l2(got, ref):
    return ((got.double().cpu() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300)).item()


def oracle_losses(sd, name, real, fake, which, dtype):
    """The oracle's loss, parameter and input gradients and buffers for ``which`` in ("g", "d"), by torch on the CPU:
    "g": generator_hinge_loss of D(fake) plus that of D(real) (two forwards alive, one backward);
    "d": discriminator_hinge_loss(D(real), D(fake)).  Buffers are updated by the two passes in order."""
    P = B.oracle_params(sd, dtype)
    xs = [real.to(dtype).clone().requires_grad_(), fake.to(dtype).clone().requires_grad_()]
    preds = []
    for x in xs:
        lg, bufs = B.disc_oracle(P, B.TABLES[name], x, True, dtype)
        for k, v in bufs.items():
            P[k] = v
        preds.append(lg)
    if which == "g":
        loss = -preds[1].mean() - preds[0].mean()
    else:
        loss = F.relu(1 - preds[0]).mean() + F.relu(1 + preds[1]).mean()
    loss.backward()
    grads = {k: p.grad for k, p in P.items() if getattr(p, "requires_grad", False)}
    bufs = {k: v for k, v in P.items() if not getattr(v, "requires_grad", False)}
    return loss.detach(), grads, [x.grad for x in xs], bufs, [p.detach() for p in preds]


def grad_report(got, ref):
    """(relative L2 over all tensors, the worst cosine among tensors above COS_FLOOR of the whole norm)."""
    num = sum((got[k].double() - ref[k].double()).pow(2).sum().item() for k in ref)
    den = sum(ref[k].double().pow(2).sum().item() for k in ref)
    total = math.sqrt(den)
    worst = 1.0
    for k in ref:
        r, g = ref[k].double().flatten(), got[k].double().flatten()
        if r.norm().item() > COS_FLOOR * total:
            worst = min(worst, (torch.dot(r, g) / (r.norm() * g.norm()).clamp_min(1e-300)).item())
    return math.sqrt(num / den), worst


@functools.lru_cache(maxsize=None)
def run_case(name, base, which):
    """One training-mode case on the device beside the fp32 and fp64 oracles, run once and shared by the three tests
    below: {key: (engine vs fp32 oracle, fp32 oracle vs fp64, tolerance)}, the worst cosines, and what was left
    queued."""
    from fmdiff.nn.losses import discriminator_hinge_loss, generator_hinge_loss
    from fmdiff.runtime.disc_engine import get_disc_engine
    sd, real, fake = setup(name, base)
    loss32, g32, dx32, buf32, p32 = oracle_losses(sd, name, real, fake, which, F32)
    loss64, g64, dx64, buf64, p64 = oracle_losses(sd, name, real, fake, which, F64)
    m = module(name, base, sd).train()
    xs = [real.to(DEV).requires_grad_(), fake.to(DEV).requires_grad_()]
    preds = [m(x) for x in xs]            # two forwards alive
    if which == "g":
        loss = generator_hinge_loss(preds[1]) + generator_hinge_loss(preds[0])
    else:
        loss = discriminator_hinge_loss(preds[0], preds[1])
    loss.backward()
    torch.cuda.synchronize()
    rep = {}
    for i, tag in enumerate(("real", "fake")):
        assert preds[i].shape == p32[i].shape and preds[i].dtype == F32
        rep[f"logits.{tag}"] = (rel_l2(preds[i], p32[i]), rel_l2(p32[i], p64[i]), FWD_TOL)
        rep[f"dx.{tag}"] = (rel_l2(xs[i].grad, dx32[i]), rel_l2(dx32[i], dx64[i]), GRAD_TOL)
    own = dict(m.named_buffers())
    for k, v in buf32.items():
        if v.is_floating_point():
            rep[f"buf.{k}"] = (rel_l2(own[k], v), rel_l2(v, buf64[k]), FWD_TOL)
        else:
            assert own[k].dtype == torch.int64 and int(own[k]) == int(v) == 2, k
    got = {k: p.grad.cpu() for k, p in m.named_parameters()}
    l2, cos = grad_report(got, g32)
    l2o, coso = grad_report({k: v.double() for k, v in g32.items()}, g64)
    rep["grad.l2"] = (l2, l2o, GRAD_TOL)
    rep["loss"] = (abs(loss.item() - loss32.item()) / abs(loss32.item()),
                   abs(loss32.item() - loss64.item()) / abs(loss64.item()), LOSS_TOL)
    print(f"disc {name} base {base} {which}: cos {cos:.5f} (oracle fp32 vs fp64 {coso:.7f}) " +
          " ".join(f"{k}={a:.2e}/{b:.1e}" for k, (a, b, _) in rep.items() if not k.startswith("buf.")) +
          f" worst buffer {max(a for k, (a, b, _) in rep.items() if k.startswith('buf.')):.2e}")
    return rep, cos, coso, len(get_disc_engine(m)._wq)


def _hold(rep, keys):
    for k in keys:
        a, b, tol = rep[k]
        assert b * 10 <= tol, f"{k}: the fp32 oracle is {b:.2e} from fp64: choose the case again"
        assert a < tol, f"{k}: {a:.3e} >= {tol}"


GRID = [(n, b, w) for n in ("magvit", "patchgan") for b in (8, 64) for w in ("g", "d")]


@pytest.mark.parametrize("name,base,which", GRID)
def test_training_forward_statistics_and_loss(name, base, which):
    """Logits of both live forwards and every running statistic after the two passes: relative L2 < 2e-2; the loss
    within 1e-2 relative; num_batches_tracked == 2; nothing left on the weight-gradient queue."""
    rep, _, _, queued = run_case(name, base, which)
    assert queued == 0, "weight gradients left queued"
    _hold(rep, [k for k in rep if k.startswith(("logits.", "buf."))] + ["loss"])


@pytest.mark.parametrize("name,base,which", GRID)
def test_training_parameter_gradients(name, base, which):
    """Relative L2 over all parameters < 5e-2, cosine > 0.99 for every tensor above 1e-3 of the whole norm.

    Measured on MI355X (engine vs fp32 oracle; the fp32 oracle is within 3e-6 of fp64 everywhere), L2 / worst cosine:
    magvit 8 g 2.0e-3 / 0.99999, d 2.8e-3 / 0.99994; magvit 64 g 2.0e-3 / 0.99998, d 3.4e-3 / 0.99997; patchgan 8 g
    2.3e-3 / 0.99998, d 4.4e-3 / 0.99997; patchgan 64 g 2.4e-3 / 0.99998, d 4.4e-3 / 0.99995.

    These figures need the walker's two-term forward.  On plain bf16 operands the same cases gave up to 1.1e-1 / 0.980
    (four of the eight outside the tolerances): a bf16 operand moves a pre-activation by about 2^-9 of its size,
    which flips the LeakyReLU branch of the elements nearest the kink; each flip changes that element's derivative
    from 1 to 0.2, so the gradient's error grows like the square root of the flipped fraction and not like the
    perturbation (the fp32 CPU oracle with only its conv weights and activations rounded to bf16 reproduced those
    figures to two digits)."""
    rep, cos, coso, _ = run_case(name, base, which)
    _hold(rep, ["grad.l2"])
    assert 1 - coso <= (1 - COS_TOL) / 10 and cos > COS_TOL, (cos, coso)


@pytest.mark.parametrize("name,base,which", GRID)
def test_training_input_gradient(name, base, which):
    """The gradient to both inputs: relative L2 < 5e-2.

    Measured on MI355X (real / fake): magvit 8 6.9e-3 / 6.8e-3, magvit 64 7.7e-3 / 6.3e-3, patchgan 8 6.8e-3 / 6.7e-3,
    patchgan 64 6.6e-3 / 6.6e-3 (what is left is the bf16 rounding of the gradients on the way down).  On plain bf16
    forward operands these were 4.9e-2 ... 1.4e-1 (see ``test_training_parameter_gradients``)."""
    rep, _, _, _ = run_case(name, base, which)
    _hold(rep, ["dx.real", "dx.fake"])


@pytest.mark.parametrize("name", ["magvit", "patchgan"])
def test_eval_mode(name):
    sd, real, _ = setup(name, 8)
    m = module(name, 8, sd).eval()
    before = {k: v.clone() for k, v in m.named_buffers()}
    with torch.no_grad():
        lg = m(real.to(DEV))
    x = real.to(DEV).requires_grad_()
    lg2 = m(x)
    lg2.sum().backward()
    ref, _ = B.disc_oracle(B.oracle_params(sd, F32), B.TABLES[name], real, False, F32)
    assert rel_l2(lg, ref) < FWD_TOL and torch.equal(lg, lg2.detach())
    for k, v in m.named_buffers():
        assert torch.equal(v, before[k]), f"{k} changed in eval mode"
    # the eval-mode gradient (statistics are constants)
    P = B.oracle_params(sd, F32)
    xr = real.clone().requires_grad_()
    B.disc_oracle(P, B.TABLES[name], xr, False, F32)[0].sum().backward()
    got = {k: p.grad.cpu() for k, p in m.named_parameters()}
    l2, cos = grad_report(got, {k: p.grad for k, p in P.items() if getattr(p, "requires_grad", False)})
    assert l2 < GRAD_TOL and cos > COS_TOL and rel_l2(x.grad, xr.grad) < GRAD_TOL, (l2, cos)


def test_param_grads_flag_and_image_maps():
    """forward_image fuses the image map into the staging.  Against the same engine fed torch's own map on the device:
    "clamp" is exact arithmetic on both sides, so logits and the input gradient are equal bit for bit (the gradient at
    |x| = 1 included); "sigmoid" differs by the last place of sigmoid before the bf16 store, so both are held to the
    project's tolerances.  With param_grads=False the backward leaves every .grad alone and the input gradient keeps
    its bits."""
    sd, real, fake = setup("magvit", 8)
    m = module("magvit", 8, sd).train()
    raw = (fake * 1.5).to(DEV)
    raw.view(-1)[:4] = torch.tensor([1.0, -1.0, 1.5, -1.5], device=DEV)
    for mode, fn in (("clamp", lambda t: (t.clamp(-1.0, 1.0) + 1.0) * 0.5), ("sigmoid", torch.sigmoid)):
        x = raw.clone().requires_grad_()
        lg = m.forward_image(x, mode)
        lg.sum().backward()
        gfull = {k: p.grad.clone() for k, p in m.named_parameters()}
        x2 = raw.clone().requires_grad_()
        m.forward_image(x2, mode, param_grads=False).sum().backward()
        assert torch.equal(x.grad, x2.grad)
        for k, p in m.named_parameters():
            assert torch.equal(p.grad, gfull[k]), k
        x3 = raw.clone().requires_grad_()
        lg3 = m(fn(x3))
        lg3.sum().backward()
        if mode == "clamp":
            assert torch.equal(lg, lg3) and torch.equal(x.grad, x3.grad)
            assert x.grad.view(-1)[0] != 0 and x.grad.view(-1)[1] != 0 and not x.grad.view(-1)[2:4].any()
        else:
            assert rel_l2(lg, lg3.detach().cpu()) < FWD_TOL and rel_l2(x.grad, x3.grad.cpu()) < GRAD_TOL
        m.zero_grad()


def test_weight_caches():
    sd, real, fake = setup("patchgan", 8)
    m = module("patchgan", 8, sd).train()
    x = real.to(DEV)
    with torch.no_grad():
        a = m(x)
    m(x.clone().requires_grad_()).sum().backward()
    with torch.no_grad():
        b = m(x)
    assert torch.equal(a, b), "a forward + backward without an optimizer step changed the logits"
    with torch.no_grad():                       # an optimizer that bumps the version counters
        for p in m.parameters():
            p.add_(p.grad, alpha=-0.05)
        c = m(x)
        fresh = module("patchgan", 8, {k: v.cpu() for k, v in m.state_dict().items()}).train()
        assert torch.equal(c, fresh(x)) and not torch.equal(c, b)
        for p in m.parameters():                # one that writes through raw pointers: no version bump
            p.data.mul_(0.9)
        m.invalidate_weights()
        d = m(x)
        fresh = module("patchgan", 8, {k: v.cpu() for k, v in m.state_dict().items()}).train()
        assert torch.equal(d, fresh(x)) and not torch.equal(d, c)


def test_descent():
    """Eight discriminator-only AdamW updates at lr 1e-3 on a fixed real / fake pair: d_gan falls by at least 80 % of
    the CPU oracle's decrease under torch.optim.AdamW (the margin the trunk tests use)."""
    from fmdiff.nn.losses import discriminator_hinge_loss
    name = "magvit"
    sd, real, fake = setup(name, 8)
    m = module(name, 8, sd).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    xr, xf = real.to(DEV), fake.to(DEV)
    seq = []
    for _ in range(9):
        opt.zero_grad()
        d = discriminator_hinge_loss(m(xr), m(xf))
        seq.append(d.item())
        d.backward()
        opt.step()
    P = B.oracle_params(sd, F32)
    params = [p for p in P.values() if getattr(p, "requires_grad", False)]
    oopt = torch.optim.AdamW(params, lr=1e-3)
    oseq = []
    for _ in range(9):
        oopt.zero_grad()
        preds = []
        for xb in (real, fake):
            lg, bufs = B.disc_oracle(P, B.TABLES[name], xb, True, F32)
            P.update(bufs)
            preds.append(lg)
        d = F.relu(1 - preds[0]).mean() + F.relu(1 + preds[1]).mean()
        oseq.append(d.item())
        d.backward()
        oopt.step()
    print("d_gan engine:", " ".join(f"{v:.4f}" for v in seq))
    print("d_gan oracle:", " ".join(f"{v:.4f}" for v in oseq))
    assert oseq[0] - oseq[-1] > 0.01, "the oracle itself does not descend: choose the case again"
    assert seq[0] - seq[-1] >= 0.8 * (oseq[0] - oseq[-1])
