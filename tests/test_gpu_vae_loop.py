"""The VAE trainer loop on the GPU: gradient accumulation over micro-batches, the validation pass, the retry after an
interrupted step, and ``vae_lib.train`` with its checkpoints, metrics, resume, out-of-memory policy and pictures.

Everything runs on the 16 x 16 model that tests/test_vae_train_host.py calls ``SMALL`` (1 channel, 32 / 32 channels,
one res block, z_channels = embed_dim = 4) and its VQVAE counterpart (16 codes), with seeded weights and
``decoder.conv_out`` scaled by 0.25 as in the trunk tests.  The engine's kernels are deterministic, so every "equals"
here is ``torch.equal``; the only tolerances are the project's existing ones (the AdamW bound and the oracle bars of
tests/test_gpu_vae_train.py)."""
import json
import logging
import warnings

import numpy as np
import pytest
import torch

from test_vae_train_host import SMALL

pytestmark = pytest.mark.gpu

KL_WEIGHT = 1e-3
KL_CFG = {"recon_type": "mse", "kl_weight": KL_WEIGHT, "gan_weight": 0.0, "perceptual_weight": 0.0}
VQ_CFG = {"recon_type": "mse", "reg_type": "vq", "codebook_weight": 1.0}
VQ_MODEL_CFG = {"latent_type": "vq"}
GAN = {"gan_weight": 0.5, "disc_lr": 2e-3}
LR, WD = 1e-3, 0.01
_CACHE = {}


# ------------------------------------------------------------------------------------------------ fixtures
def _new(kind):
    from fmdiff.models.vae import VQVAE, AutoencoderKL
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind == "kl":
            return AutoencoderKL(**SMALL)
        return VQVAE(**SMALL, codebook_size=16, quantizer_type=kind)


def _state(kind):
    """Seeded weights of the ``kind`` model ("kl", "ema", "classic"), decoder.conv_out scaled by 0.25."""
    if ("state", kind) not in _CACHE:
        torch.manual_seed({"kl": 11, "ema": 12, "classic": 13}[kind])
        sd = {k: v.detach().clone() for k, v in _new(kind).state_dict().items()}
        for k in ("decoder.conv_out.conv.weight", "decoder.conv_out.conv.bias"):
            sd[k] = sd[k] * 0.25
        _CACHE[("state", kind)] = sd
    return _CACHE[("state", kind)]


def _model(kind, state=None):
    m = _new(kind)
    m.load_state_dict(_state(kind) if state is None else state)
    return m.cuda().train()


def _disc_state():
    if "disc" not in _CACHE:
        from fmdiff.nn.modules.vae.discriminators import PatchGANDiscriminatorND
        torch.manual_seed(31)
        sd = {k: v.detach().clone() for k, v in PatchGANDiscriminatorND(1, 8).state_dict().items()}
        g = torch.Generator().manual_seed(32)
        for k in sd:   # BatchNorm away from its defaults
            if k.endswith("running_mean"):
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.3
            elif k.endswith("running_var") or (sd[k].dim() == 1 and ".conv." not in k and k.endswith("weight")):
                sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
        _CACHE["disc"] = sd
    return _CACHE["disc"]


def _disc():
    from fmdiff.nn.modules.vae.discriminators import PatchGANDiscriminatorND
    d = PatchGANDiscriminatorND(1, 8)
    d.load_state_dict(_disc_state())
    return d.cuda().train()


def _data(n, seed=5):
    """(images [n, 1, 16, 16] in [0, 1], posterior noise [n, 4, 8, 8]) on the device."""
    if ("data", n, seed) not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        _CACHE[("data", n, seed)] = (torch.rand(n, 1, 16, 16, generator=g), torch.randn(n, 4, 8, 8, generator=g))
    x, eps = _CACHE[("data", n, seed)]
    return x.cuda(), eps.cuda()


def _step(kind, gan=False, **kw):
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    tcfg = dict(KL_CFG if kind == "kl" else VQ_CFG, **(GAN if gan else {}))
    model, disc = _model(kind), (_disc() if gan else None)
    st = VAETrainStep(model, tcfg, None if kind == "kl" else VQ_MODEL_CFG, discriminator=disc, lr=LR, weight_decay=WD,
                      **kw)
    return st, tcfg


def _forward(kind, vae, x, eps):
    if kind == "kl":
        rec, _, kl = vae.forward_train(vae.image_to_model_range(x), eps, sample_posterior=True)
        return rec, dict(kl=kl)
    rec, aux = vae.forward_train(vae.image_to_model_range(x))
    return rec, dict(vq_loss=aux["vq_loss"])


def _adamw_bound(named, state0, lr, wd):
    """The bound of tests/test_gpu_vae_train.py: torch.optim.AdamW on the CPU fed the engine's own gradients."""
    cpu = {k: torch.nn.Parameter(state0[k].clone()) for k, _ in named}
    for k, p in named:
        cpu[k].grad = p.grad.detach().cpu().clone()
    torch.optim.AdamW(list(cpu.values()), lr=lr, weight_decay=wd).step()
    worst = 0.0
    for k, p in named:
        tol = 2.0 * state0[k].abs() * 2.0 ** -23 + 1e-3 * lr
        worst = max(worst, ((p.detach().cpu() - cpu[k].detach()).abs() / tol).max().item())
    return worst


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("kind,gan", [("kl", False), ("kl", True), ("classic", False)])
def test_accumulation_is_exact(kind, gan):
    """``step(cat[A, A], micro_batch=2)`` leaves the gradients of ``step(A)`` bit for bit: each chunk's loss is
    halved, halving commutes with every fp32 and bf16 rounding as long as nothing is subnormal (asserted), and two
    equal halves sum exactly.  Fails if any path overwrites instead of accumulating or scales by anything but
    1 / accum.  With the discriminator its own gradients are compared too; ``disc_grad_from_generator=False`` there,
    because with it the discriminator receives two terms per chunk (from the backward of g_gan and from that of
    d_gan), and ``g/2 + d/2 + g/2 + d/2`` summed in that order is not ``g + d`` in floating point.  The EMA codebook
    moves between chunks and is covered by the composition test."""
    A, eps = _data(2)
    eps = eps if kind == "kl" else None
    kw = dict(disc_grad_from_generator=False) if gan else {}
    one, _ = _step(kind, gan, **kw)
    two, _ = _step(kind, gan, **kw)
    one.step(A, eps)
    two.step(torch.cat([A, A]), None if eps is None else torch.cat([eps, eps]), micro_batch=2)
    torch.cuda.synchronize()
    pairs = [(one.flat.grad, two.flat.grad)] + ([(one.disc_flat.grad, two.disc_flat.grad)] if gan else [])
    for a, b in pairs:
        nz = a[a != 0].abs()
        # a real gradient (the PatchGAN's last 3x3 conv sees a 1 x 1 map here: 8 of its 9 taps only read padding and
        # stay zero, which is most of that network's zeros), and no subnormal anywhere
        assert nz.numel() > a.numel() // 4 and nz.min().item() > 2.0 ** -100
        print(f"{kind} gan={gan}: {a.numel()} gradient values, smallest nonzero {nz.min().item():.3e}, "
              f"{(a != b).sum().item()} differ, max |diff| {(a - b).abs().max().item():.3e}")
        assert torch.equal(a, b)
    assert one.global_step == two.global_step == 1


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("kind", ["kl", "ema"])
def test_microbatched_step_equals_the_composition(kind):
    """Batch 4, ``micro_batch=3`` (chunks of 3 and 1) against the reference's body written out per chunk:
    ``forward_train``, ``VAECriterion``, ``(loss / 2).backward()``."""
    from fmdiff.pipelines.train.vae_lib import VAECriterion
    x, eps = _data(4)
    eps = eps if kind == "kl" else None
    st, tcfg = _step(kind)
    ref = _model(kind)
    crit = VAECriterion(tcfg, None if kind == "kl" else VQ_MODEL_CFG)
    outs = []
    for sl in (slice(0, 3), slice(3, 4)):
        rec, kw = _forward(kind, ref, x[sl], None if eps is None else eps[sl])
        o = crit(rec, x[sl], global_step=0, **kw)
        (o["loss"] / 2).backward()
        outs.append({k: v.detach() for k, v in o.items()})
    out = st.step(x, eps, micro_batch=3)
    torch.cuda.synchronize()
    assert st.global_step == 1 and set(out) == set(outs[0])
    for k in out:
        want = (outs[0][k] * 3 + outs[1][k] * 1) / 4
        assert out[k].is_cuda and out[k].dim() == 0 and not out[k].requires_grad and torch.equal(out[k], want), k
    for (k, p), q in zip(st.model.named_parameters(), ref.parameters()):
        if q.grad is None:      # the classic codebook; not in these cases, but the EMA model has none either
            assert not p.grad.any(), k
        else:
            assert torch.equal(p.grad, q.grad), k
    named = [(k, p) for k, p in st.model.named_parameters()]
    worst = _adamw_bound(named, _state(kind), LR, WD)
    print(f"{kind}: AdamW after two accumulated chunks vs torch.optim.AdamW: worst |error| / tol {worst:.3f}")
    assert worst <= 1.0
    if kind == "ema":   # the codebook moved once per chunk, as in the two forwards of the composition
        for name in ("ema_cluster_size", "ema_w", "embedding"):
            a, b = getattr(st.model.codebook, name), getattr(ref.codebook, name)
            assert torch.equal(a, b), name
            assert not torch.equal(a.cpu(), _state(kind)[f"codebook.{name}"]), name
    assert st.eng._head_bwd is None and len(st.eng._wq) == 0


# ------------------------------------------------------------------------------------------------ 3
def test_microbatched_gradients_against_the_oracle():
    """Batch 4 in two chunks of 2, mse + 1e-3 KL, against torch autograd over the CPU oracle on the full batch (equal
    chunks make the two mathematically equal), under the bars of tests/test_gpu_vae_train.py."""
    import test_gpu_vae_train as T
    assert T.KL_WEIGHT == KL_WEIGHT
    x, eps = _data(4)
    loss_ref, ref, _ = T._oracle_grads(dict(SMALL), _state("kl"), x.cpu(), eps.cpu(), "mse")
    st, _ = _step("kl")
    out = st.step(x, eps, micro_batch=2)
    torch.cuda.synchronize()
    T._compare(st.model, ref, out["loss"].item(), loss_ref, "micro_batch=2 vs the oracle's full batch")


# ------------------------------------------------------------------------------------------------ 4
def _snapshot(st):
    snap = {f"model.{k}": v.detach().clone() for k, v in st.model.state_dict().items()}
    snap.update({f"disc.{k}": v.detach().clone() for k, v in st.disc.state_dict().items()})
    for name in ("m", "v", "disc_m", "disc_v"):
        snap[name] = getattr(st, name).clone()
    snap["grad"], snap["disc_grad"] = st.flat.grad.clone(), st.disc_flat.grad.clone()
    snap["data"], snap["disc_data"] = st.flat.data.clone(), st.disc_flat.data.clone()
    return snap, (st.global_step, st.disc_step, st.lr, st.disc_lr)


def test_evaluate_changes_nothing():
    x, eps = _data(4)
    st, _ = _step("kl", gan=True)
    twin, _ = _step("kl", gan=True)
    st.step(x[:2], eps[:2])          # moments, gradients and running statistics away from their initial values
    twin.step(x[:2], eps[:2])
    snap, counters = _snapshot(st)
    assert any(k.endswith("num_batches_tracked") and v.item() == 3 for k, v in snap.items())
    full = st.evaluate(x)
    assert st.model.training and st.disc.training
    chunked = st.evaluate(x, micro_batch=3)
    st.model.eval()
    st.evaluate(x, epoch=2, micro_batch=1)
    assert not st.model.training and st.disc.training          # the modes they were in
    st.model.train()
    torch.cuda.synchronize()
    after, counters_after = _snapshot(st)
    assert counters == counters_after
    for k in snap:
        assert torch.equal(snap[k], after[k]), k
    # chunks: eval-mode BatchNorm does not see the chunking, so the weighted mean of the parts
    a, b = st.evaluate(x[:3]), st.evaluate(x[3:])
    for k in full:
        assert full[k].is_cuda and full[k].dim() == 0
        assert torch.equal(chunked[k], (a[k] * 3 + b[k] * 1) / 4), k
    assert full["g_gan"].item() != 0.0 and full["d_gan"].item() != 0.0 and full["kl"].item() > 0.0
    # a following step is the twin's, which never evaluated
    o1, o2 = st.step(x, eps, micro_batch=2), twin.step(x, eps, micro_batch=2)
    torch.cuda.synchronize()
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    assert torch.equal(st.flat.grad, twin.flat.grad) and torch.equal(st.disc_flat.grad, twin.disc_flat.grad)
    assert torch.equal(st.flat.data, twin.flat.data) and torch.equal(st.disc_flat.data, twin.disc_flat.data)
    for (k, v), w in zip(st.disc.state_dict().items(), twin.disc.state_dict().values()):
        assert torch.equal(v, w), k


def test_evaluate_means_what_it_says():
    """``recon``, ``kl``, ``loss`` and the adversarial terms are the criterion applied to ``model.eval()``'s own
    ``forward(sample_posterior=False)`` outputs, BatchNorm on its running statistics; the EMA VQVAE's ``vq`` is that
    of ``model.eval()(x)``, and its codebook stays."""
    from fmdiff.pipelines.train.vae_lib import VAECriterion
    x, _ = _data(4)
    st, tcfg = _step("kl", gan=True)
    out = st.evaluate(x)
    m, d = _model("kl").eval(), _disc().eval()
    with torch.no_grad():
        rec, post = m(m.image_to_model_range(x), sample_posterior=False)
        fake = d.forward_image(rec, "clamp")
        crit = VAECriterion(tcfg)
        want = crit(rec, x, kl=post.kl(), fake_pred=fake, global_step=0)
        want["d_gan"] = crit.discriminator_loss(d(x), fake)
    torch.cuda.synchronize()
    assert set(out) == set(want)
    for k in want:
        assert torch.equal(out[k], want[k]), k
    assert torch.equal(out["kl"], post.kl().mean())
    # the gate: inactive before gan_start, and then the discriminator is not run
    late, _ = _step("kl", gan=True)
    late.criterion.gan_start = 3
    off = late.evaluate(x, epoch=2)
    assert off["g_gan"].item() == 0.0 and off["d_gan"].item() == 0.0 and torch.equal(off["recon"], out["recon"])
    assert late.evaluate(x, epoch=3)["g_gan"].item() == out["g_gan"].item()

    vq, _ = _step("ema")
    before = {k: v.clone() for k, v in vq.model.state_dict().items()}
    got = vq.evaluate(x, micro_batch=4)
    e = _model("ema").eval()
    with torch.no_grad():
        rec, aux = e(e.image_to_model_range(x))
    assert torch.equal(got["vq"], aux["vq_loss"]) and got["vq"].item() > 0.0
    assert vq.model.training and vq.model.codebook.training
    for k, v in vq.model.state_dict().items():
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------------------------------------------ 5
class _FailingCriterion:
    """The step's criterion with a Python exception injected into its ``fail_on``-th call."""

    def __init__(self, inner, fail_on):
        self.inner, self.fail_on, self.calls = inner, fail_on, 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def __call__(self, *a, **kw):
        self.calls += 1
        if self.calls == self.fail_on:
            raise RuntimeError("HIP out of memory (injected)")
        return self.inner(*a, **kw)


def test_an_interrupted_step_can_be_retried():
    x, eps = _data(4)
    st, _ = _step("kl")
    twin, _ = _step("kl")
    data0 = st.flat.data.clone()
    st.criterion = _FailingCriterion(st.criterion, fail_on=2)
    with pytest.raises(RuntimeError, match="out of memory"):
        st.step(x, eps, micro_batch=2)       # the first chunk ran its backward, the second only its forward
    assert st.criterion.calls == 2 and st.flat.grad.any().item()
    assert st.global_step == 0 and torch.equal(st.flat.data, data0) and not st.m.any() and not st.v.any()
    assert st.eng._head_bwd is None and len(st.eng._wq) == 0
    fold = st.eng._fold
    assert fold is None or fold.weight.grad is None or not fold.weight.grad.any()
    a, b = st.step(x, eps, micro_batch=1), twin.step(x, eps, micro_batch=1)
    torch.cuda.synchronize()
    assert st.global_step == twin.global_step == 1
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(st.flat.grad, twin.flat.grad) and torch.equal(st.flat.data, twin.flat.data)
    assert torch.equal(st.m, twin.m) and torch.equal(st.v, twin.v)


# ------------------------------------------------------------------------------------------------ the loop
class Items(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        self.x = torch.rand(n, 1, 16, 16, generator=torch.Generator().manual_seed(seed))

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return {"target": self.x[i]}


def _config(tmp_path, kind, name="cfg", out="run", **training):
    """A config file for ``train``: the SMALL model with its seeded weights named as ``model.ckpt_path``."""
    ckpt = tmp_path / f"{kind}_init.pt"
    if not ckpt.exists():
        torch.save(_state(kind), ckpt)
    model = dict(SMALL, model_type="vae", latent_type="kl" if kind == "kl" else "vq", ckpt_path=str(ckpt))
    if kind != "kl":
        model.update(codebook_size=16, quantizer_type=kind)
    tr = dict(KL_CFG if kind == "kl" else VQ_CFG)
    tr.update(output_dir=str(tmp_path / out), batch_size=4, num_workers=0, epochs=2, seed=3, learning_rate=LR,
              weight_decay=WD, save_images=False, manual_device="cuda")
    if kind == "kl":
        tr["reg_type"], tr["codebook_weight"] = "kl", 0.0
    tr.update(training)
    path = tmp_path / f"{name}.json"
    path.write_text(json.dumps({"model": model, "training": tr}))
    return path, tr, model


def _rows(path):
    return path.read_text().splitlines()


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def _twin_rows(kind, ds, tr, model_cfg, epochs, keys):
    """What ``train`` has to write: the same (seed, epoch) order, ``VAETrainStep.step`` per batch, fp64 totals."""
    from fmdiff.pipelines.train.vae_lib import TOTALS_KEYS, VAETrainStep, epoch_order
    twin = _model(kind)
    st = VAETrainStep(twin, tr, model_cfg)
    rows = []
    for epoch in range(1, epochs + 1):
        order = epoch_order(len(ds), tr["seed"], epoch)
        tot = {k: torch.zeros((), device="cuda", dtype=torch.float64) for k in TOTALS_KEYS}
        for i in range(0, len(order), tr["batch_size"]):
            raw = torch.stack([ds[j]["target"] for j in order[i:i + tr["batch_size"]]]).cuda()
            out = st.step(raw, epoch=epoch, micro_batch=tr["batch_size"])
            for k in TOTALS_KEYS:
                tot[k] += out[k].double() * raw.shape[0]
        rows.append(",".join([f"{epoch}"] + ["%.6f" % (tot[k] / len(ds)).item() for k in keys]))
    return rows, twin, st


def test_the_loop_equals_its_parts(tmp_path):
    from fmdiff.pipelines.train import vae_lib
    torch.manual_seed(1234)          # the global CPU stream, which the batch order must not depend on
    ds = Items(7, 21)
    path, tr, model_cfg = _config(tmp_path, "ema")
    out_dir = vae_lib.train(ds, path)
    assert out_dir == tmp_path / "run_run1" and (out_dir / "train_config.json").exists()
    assert json.loads((out_dir / "train_config.json").read_text())["training"]["output_dir"] == str(out_dir)
    rows = _rows(out_dir / "metrics.csv")
    want, twin, st = _twin_rows("ema", ds, tr, model_cfg, 2, ["loss", "recon", "vq"])
    assert rows[0] == "epoch,loss,recon,vq" and rows[1:] == want, (rows, want)
    last = _load(out_dir / "vae_last.pt")
    assert set(last) == {"model", "optimizer", "disc_optimizer", "scheduler", "scaler", "epoch", "best_metric",
                         "discriminator", "cuda_rng_state"}
    assert last["epoch"] == 2 and last["scaler"] is None and last["disc_optimizer"] is None
    assert last["optimizer"]["global_step"] == 4 and st.global_step == 4
    for k, v in twin.state_dict().items():
        assert torch.equal(last["model"][k], v.cpu()), k
    sd = st.state_dict()
    for i, e in sd["state"].items():
        assert torch.equal(last["optimizer"]["state"][i]["exp_avg"], e["exp_avg"]), i
    for e in (1, 2):
        assert (out_dir / "epochs" / f"epoch{e:04d}" / "epoch.pt").exists()
    assert not list(out_dir.rglob("*.png"))
    # best_metric is written before the update in vae_last.pt and after it in vae_best.pt, as in the reference
    losses = [float(r.split(",")[1]) for r in rows[1:]]
    best = _load(out_dir / "vae_best.pt")
    assert best["epoch"] == 1 + losses.index(min(losses)) and "%.6f" % best["best_metric"] == "%.6f" % min(losses)


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("kind", ["ema", "kl"])
def test_resume_is_exact(tmp_path, kind):
    """Two epochs straight against one epoch, a new process's worth of setup, ``resume``, one more.  The
    AutoencoderKL case draws its posterior noise from the device's stream and writes pictures in between: the
    checkpoint's ``cuda_rng_state`` and the ``gen`` picture's own generator keep the second epoch's noise the same."""
    from fmdiff.pipelines.train import vae_lib
    ds = Items(20 if kind == "kl" else 7, 22)
    extra = dict(save_images=True) if kind == "kl" else {}
    straight, _, _ = _config(tmp_path, kind, "straight", "a", **extra)
    a = vae_lib.train(ds, straight)
    first, _, _ = _config(tmp_path, kind, "first", "b", epochs=1, **extra)
    b = vae_lib.train(ds, first)
    torch.manual_seed(777)           # a resumed process has drawn other numbers
    torch.cuda.manual_seed(778)
    second, _, _ = _config(tmp_path, kind, "second", b.name, **extra)
    assert vae_lib.train(ds, second, resume=True) == b
    ra, rb = _rows(a / "metrics.csv"), _rows(b / "metrics.csv")
    assert len(ra) == len(rb) == 3 and ra == rb, (ra, rb)
    la, lb = _load(a / "vae_last.pt"), _load(b / "vae_last.pt")
    assert la["epoch"] == lb["epoch"] == 2
    assert la["optimizer"]["global_step"] == lb["optimizer"]["global_step"] == 2 * len(range(0, len(ds), 4))
    for k, v in la["model"].items():
        assert torch.equal(v, lb["model"][k]), k
    for i, e in la["optimizer"]["state"].items():
        assert torch.equal(e["exp_avg_sq"], lb["optimizer"]["state"][i]["exp_avg_sq"]), i
    assert torch.equal(la["cuda_rng_state"], lb["cuda_rng_state"])
    # a path as ``resume`` and a reference-style checkpoint (no extra keys) load too: nothing left to train
    ref_style = {k: v for k, v in lb.items() if k not in ("discriminator", "cuda_rng_state")}
    ref_style["optimizer"] = {k: v for k, v in lb["optimizer"].items() if k != "global_step"}
    torch.save(ref_style, tmp_path / "ref_style.pt")
    assert vae_lib.train(ds, second, resume=str(tmp_path / "ref_style.pt")) == b
    assert _rows(b / "metrics.csv") == rb


def test_schedule_and_best_checkpoint_follow_validation(tmp_path):
    from fmdiff.pipelines.train import vae_lib
    from fmdiff.pipelines.train.vae_lib import TOTALS_KEYS, VAETrainStep
    ds, val = Items(8, 23), Items(6, 24)
    path, tr, _ = _config(tmp_path, "kl", epochs=3,
                          scheduler={"name": "StepLR", "params": {"step_size": 1, "gamma": 0.5}})
    out_dir = vae_lib.train(ds, path, val_dataset=val)
    val_loss = []
    for epoch in (1, 2, 3):
        ck = _load(out_dir / "epochs" / f"epoch{epoch:04d}" / "epoch.pt")
        # the checkpoint is written after the scheduler's step: the rate the next epoch trains with
        assert ck["optimizer"]["param_groups"][0]["lr"] == LR * 0.5 ** epoch
        assert ck["scheduler"]["last_epoch"] == epoch
        st = VAETrainStep(_model("kl", ck["model"]), tr)
        st.load_state_dict(ck["optimizer"])
        assert st.lr == LR * 0.5 ** epoch and st.global_step == 2 * epoch
        tot = torch.zeros(len(TOTALS_KEYS), device="cuda", dtype=torch.float64)
        for i in range(0, len(val), 4):
            raw = torch.stack([val[j]["target"] for j in range(i, min(i + 4, len(val)))]).cuda()
            out = st.evaluate(raw, epoch=epoch, micro_batch=4)
            tot += torch.stack([out[k] for k in TOTALS_KEYS]).double() * raw.shape[0]
        val_loss.append((tot / len(val)).tolist()[0])
    best = _load(out_dir / "vae_best.pt")
    print("validation loss per epoch:", val_loss, "best:", best["epoch"], best["best_metric"])
    assert best["epoch"] == 1 + val_loss.index(min(val_loss)) and best["best_metric"] == min(val_loss)
    train_loss = [float(r.split(",")[1]) for r in _rows(out_dir / "metrics.csv")[1:]]
    assert all(abs(t - v) > 1e-6 for t, v in zip(train_loss, val_loss))      # it is not the training loss


# ------------------------------------------------------------------------------------------------ 8
class _Collect(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def _inject(monkeypatch, fail_on):
    """One injected out-of-memory error in the ``fail_on``-th criterion call of the run; records every
    ``micro_batch`` that ``step`` and ``evaluate`` are called with."""
    from fmdiff.pipelines.train import vae_lib
    seen = {"calls": 0, "step": [], "evaluate": []}
    real_call, real_step, real_eval = (vae_lib.VAECriterion.__call__, vae_lib.VAETrainStep.step,
                                       vae_lib.VAETrainStep.evaluate)

    def call(self, *a, **kw):
        seen["calls"] += 1
        if seen["calls"] == fail_on:
            raise RuntimeError("HIP out of memory (injected)")
        return real_call(self, *a, **kw)

    def step(self, raw, *a, **kw):
        seen["step"].append((raw.shape[0], kw.get("micro_batch")))
        return real_step(self, raw, *a, **kw)

    def evaluate(self, raw, *a, **kw):
        seen["evaluate"].append((raw.shape[0], kw.get("micro_batch")))
        return real_eval(self, raw, *a, **kw)

    monkeypatch.setattr(vae_lib.VAECriterion, "__call__", call)
    monkeypatch.setattr(vae_lib.VAETrainStep, "step", step)
    monkeypatch.setattr(vae_lib.VAETrainStep, "evaluate", evaluate)
    return seen


def test_out_of_memory_halves_the_micro_batch_for_the_rest_of_the_run(tmp_path, monkeypatch):
    from fmdiff.pipelines.train import vae_lib
    ds, val = Items(7, 25), Items(4, 26)
    path, tr, _ = _config(tmp_path, "kl")
    seen = _inject(monkeypatch, fail_on=1)
    handler = _Collect()
    vae_lib._log.addHandler(handler)
    try:
        out_dir = vae_lib.train(ds, path, val_dataset=val)
    finally:
        vae_lib._log.removeHandler(handler)
    # the first batch twice (4, then 2), every later call at 2; validation capped by it
    assert seen["step"] == [(4, 4), (4, 2), (3, 2), (4, 2), (3, 2)], seen["step"]
    assert seen["evaluate"] == [(4, 2), (4, 2)]
    assert handler.messages == [vae_lib.micro_batch_warning(2, 4)], handler.messages
    rows = _rows(out_dir / "metrics.csv")
    # the run finished: the interrupted attempt advanced nothing, every batch counted once
    assert len(rows) == 3 and _load(out_dir / "vae_last.pt")["optimizer"]["global_step"] == 4
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r.split(","))


def test_out_of_memory_without_microbatching_is_the_reference_message(tmp_path, monkeypatch):
    from fmdiff.pipelines.train import vae_lib
    path, _, _ = _config(tmp_path, "kl", allow_microbatching=False)
    _inject(monkeypatch, fail_on=1)
    with pytest.raises(RuntimeError) as e:
        vae_lib.train(Items(7, 25), path)
    assert str(e.value) == vae_lib.OOM_DISABLED_MESSAGE and "out of memory" in str(e.value.__cause__)


def test_other_errors_propagate(tmp_path, monkeypatch):
    from fmdiff.pipelines.train import vae_lib

    def call(self, *a, **kw):
        raise RuntimeError("something else")

    monkeypatch.setattr(vae_lib.VAECriterion, "__call__", call)
    path, _, _ = _config(tmp_path, "kl")
    with pytest.raises(RuntimeError, match="something else"):
        vae_lib.train(Items(7, 25), path)


# ------------------------------------------------------------------------------------------------ 9
def test_artifacts(tmp_path):
    from PIL import Image
    from fmdiff import utils as U
    from fmdiff.pipelines.train import vae_lib
    ds = Items(20, 27)
    path, tr, _ = _config(tmp_path, "kl", epochs=1, save_images=True)
    out_dir = vae_lib.train(ds, path)
    epoch_dir = out_dir / "epochs" / "epoch0001"
    pics = {n: np.asarray(Image.open(epoch_dir / f"{n}.png")) for n in ("input", "recon", "gen")}
    for n, p in pics.items():
        assert p.shape == (64, 80, 3) and p.dtype == np.uint8, n
    m = _model("kl", _load(out_dir / "vae_last.pt")["model"]).eval()
    batch = U.prepare_eval_batch(ds, 20, torch.device("cuda"), seed=tr["seed"])
    with torch.no_grad():
        rec, _ = m(m.image_to_model_range(batch), sample_posterior=False)
        want = U.make_grid(m.raw_output_to_image(rec, recon_type="mse"), 4, 5)
    assert np.array_equal(pics["recon"], want)
    assert np.array_equal(pics["input"], U.make_grid(batch, 4, 5))
    assert pics["gen"].std() > 0 and not np.array_equal(pics["gen"], pics["recon"])
    with pytest.raises(ValueError, match="Need at least 20 images to build the grid, found 7"):
        vae_lib.train(Items(7, 27), path)
    dbg = vae_lib.debug_visual_only(ds, path, out_dir / "vae_last.pt", output_dir=tmp_path / "dbg", visual_samples=10)
    assert dbg == tmp_path / "dbg"
    grids = {n: np.asarray(Image.open(dbg / f"grid_{n}.png")) for n in ("input", "output", "target")}
    for n, p in grids.items():
        assert p.shape == (48, 48, 3), n
    assert np.array_equal(grids["input"], grids["target"]) and not np.array_equal(grids["input"], grids["output"])
