"""EMA weights on the GPU: fmd_adamw_sched_ema against the CPU restatement (tests/ema_ref.py) bit for bit, the
train step's EMA (eager, captured, swapped in for sampling) and the trainer loop's checkpoints."""
import json
import os

import pytest
import torch

import ema_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _launch(bufs, s, decay=None, warmup=True):
    """One launch at step count ``s`` on device copies of the CPU tensors ``bufs`` = (p, g, m, v[, ema]); returns
    the device tensors (p, g, m, v, ema or None, ctr) after it."""
    from fmdiff.runtime import ops as O
    p, g, m, v = (t.to(DEV) for t in bufs[:4])
    ema = bufs[4].to(DEV) if decay is not None else None
    ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
    hp = er.HP
    O.adamw_sched(p, g, m, v, ctr, hp["base_lr"], hp["warmup"], hp["total"], hp["beta1"], hp["beta2"], hp["eps"],
                  hp["wd"], hp["grad_scale"], ema=ema, ema_decay=decay or 0.0, ema_warmup=warmup)
    return p, g, m, v, ema, ctr


# ------------------------------------------------------------------ 3. exact recurrence
@pytest.mark.parametrize("sweep", er.SWEEPS, ids=[s[0] for s in er.SWEEPS])
def test_ema_kernel_exact_recurrence(sweep):
    """ema == the restatement applied to the p the launch wrote, bit for bit; p, m, v == fmd_adamw_sched's from
    copies of the same inputs, bit for bit; g and the step counter untouched."""
    name, decay, warmup, steps = sweep
    for n in er.NS:
        cpu = er.make_inputs(n)
        assert not torch.equal(cpu[4], cpu[0])
        for s in steps:
            p, g, m, v, ema, ctr = _launch(cpu, s, decay, warmup)
            p0, g0, m0, v0, _, ctr0 = _launch(cpu, s)                     # the old entry point
            torch.cuda.synchronize()
            for got, ref, what in ((p, p0, "p"), (m, m0, "m"), (v, v0, "v")):
                assert torch.equal(got, ref), (name, n, s, what)
            assert not torch.equal(p.cpu(), cpu[0]), (name, n, s, "the update moved p")
            assert torch.equal(g.cpu(), cpu[1]) and torch.equal(g0.cpu(), cpu[1]), (name, n, s, "g")
            assert int(ctr.item()) == s and int(ctr0.item()) == s, (name, n, s, "step_ctr")
            want = er.ema_update(cpu[4], p.cpu(), s, decay, warmup)
            assert torch.equal(ema.cpu(), want), (name, n, s, (ema.cpu() - want).abs().max().item())


def _raw_call(p, g, m, v, ema, ctr, decay):
    """Either entry point on (possibly offset) views: ops.adamw_sched wants whole contiguous buffers."""
    from fmdiff import _lib
    from fmdiff.runtime import ops as O
    hp = er.HP
    head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
    tail = (ctr.data_ptr(), hp["base_lr"], hp["warmup"], hp["total"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"],
            hp["grad_scale"])
    if ema is None:
        _lib.call("fmd_adamw_sched", *head, p.numel(), *tail, O.stream())
    else:
        _lib.call("fmd_adamw_sched_ema", *head, ema.data_ptr(), p.numel(), *tail, decay, 1, O.stream())


def test_ema_kernel_unaligned_buffers_take_the_scalar_path():
    """An ema (or p) that is only 4-byte aligned sends the whole launch down the element-wise path: the EMA is the
    restatement's and p, m, v are those of fmd_adamw_sched on buffers shifted the same way."""
    n, s, decay = 1023, 3, 0.9
    cpu = er.make_inputs(n)

    def dev(t, shift):
        view = torch.zeros(n + 4, device=DEV)[shift:shift + n]
        view.copy_(t)
        return view

    for shift_ema, shift_p in ((1, 0), (0, 1)):
        ctr = torch.tensor([s], dtype=torch.int32, device=DEV)
        p, g, m, v = dev(cpu[0], shift_p), dev(cpu[1], 0), dev(cpu[2], 0), dev(cpu[3], 0)
        ema = dev(cpu[4], shift_ema)
        assert (p.data_ptr() | ema.data_ptr()) % 16 == 4
        _raw_call(p, g, m, v, ema, ctr, decay)
        # the old entry point takes its element-wise path when p is shifted; with only ema shifted it keeps the
        # vector path, which the exact-recurrence test has compared with the element-wise one at n = 1023 (tail)
        p0, g0, m0, v0 = dev(cpu[0], shift_p), dev(cpu[1], 0), dev(cpu[2], 0), dev(cpu[3], 0)
        _raw_call(p0, g0, m0, v0, None, ctr, decay)
        torch.cuda.synchronize()
        if shift_p:
            assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        assert torch.equal(ema.cpu(), er.ema_update(cpu[4], p.cpu(), s, decay, True)), (shift_ema, shift_p)


# ------------------------------------------------------------------ 4. refusals
def test_ema_entry_point_refusals():
    """NULL ema and a decay outside [0, 1) are refused before anything is launched (real buffers all the same, so
    that a missing check would show as a return code of 0 and nothing worse)."""
    from fmdiff import _lib
    from fmdiff.runtime import ops as O
    n = 8
    p, g, m, v, ema = (t.to(DEV) for t in er.make_inputs(n))
    keep = [t.clone() for t in (p, g, m, v, ema)]
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    hp = er.HP
    fn = _lib.lib().fmd_adamw_sched_ema

    def rc(ema_ptr, decay):
        return fn(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema_ptr, n, ctr.data_ptr(), hp["base_lr"],
                  hp["warmup"], hp["total"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], hp["grad_scale"], decay, 1,
                  O.stream())
    assert rc(None, 0.9) != 0
    assert rc(ema.data_ptr(), 1.0) != 0
    assert rc(ema.data_ptr(), -0.25) != 0
    assert rc(ema.data_ptr(), float("nan")) != 0
    torch.cuda.synchronize()
    for t, k in zip((p, g, m, v, ema), keep):
        assert torch.equal(t, k)
    with pytest.raises(ValueError):
        O.adamw_sched(p, g, m, v, ctr, 1e-3, 0, 10, ema=ema[:4], ema_decay=0.9)


# ------------------------------------------------------------------ 5. successive launches
def test_ema_kernel_twelve_successive_launches():
    from fmdiff.runtime import ops as O
    n, decay = 4103, 0.9
    cp, _, cm, cv, cema = er.make_inputs(n, seed=1)
    p, m, v, ema = cp.to(DEV), cm.to(DEV), cv.to(DEV), cema.to(DEV)
    g = torch.empty(n, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    hp = er.HP
    want = cema
    for k in range(12):
        g.copy_(er.make_grad(n, k))
        O.adamw_sched(p, g, m, v, ctr, hp["base_lr"], hp["warmup"], hp["total"], hp["beta1"], hp["beta2"], hp["eps"],
                      hp["wd"], hp["grad_scale"], ema=ema, ema_decay=decay, ema_warmup=True)
        O.counter_add(ctr)
        want = er.ema_update(want, p.cpu(), k, decay, True)
        assert torch.equal(ema.cpu(), want), k
    assert int(ctr.item()) == 12


# ------------------------------------------------------------------ 6-8. the train step
@pytest.fixture(scope="module")
def small(golden):
    """The small 2-D UNet of tests/test_gpu_unet.py (ldct_fm_test: 32/64 channels, batch 2 at 32^2), its seeded
    weights and one fixed batch."""
    from oracle import spec as S
    from oracle import unet as U
    T, M = golden
    meta = M["ldct_fm_test"]
    tr = meta["training"]
    sd = U.seeded_state_dict(S.derive_spec(meta["unet"], tr["conditioning"], tr["channels"] or 1), meta["seed"])
    clean = T["ldct_fm_test/x"].clamp(0, 1).to(DEV)
    cond = T["ldct_fm_test/cond"].to(DEV)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(clean.shape, generator=g).to(DEV)
    t = torch.rand(clean.shape[0], generator=g).to(DEV)
    return meta, sd, clean, cond, noise, t


def _model(small):
    from fmdiff.models.generators import DiffusionUNetFactory
    meta, sd = small[:2]
    tr = meta["training"]
    model = DiffusionUNetFactory().build(meta["unet"], tr["conditioning"], tr["channels"] or 1).to(DEV)
    model.load_state_dict(sd)
    return model


def test_step_ema_twin_eager_steps(small):
    """EMA changes nothing else (parameters bit-identical to a twin without it after every step), and the step's
    EMA follows the recurrence on the parameters each step produced."""
    from fmdiff.pipelines.train.fused import FusedTrainStep
    _, _, clean, cond, noise, t = small
    with_ema = FusedTrainStep(_model(small), lr=1e-3, warmup=0, total_steps=100, ema_decay=0.9)
    without = FusedTrainStep(_model(small), lr=1e-3, warmup=0, total_steps=100, ema_decay=None)
    assert without.ema is None
    assert torch.equal(with_ema.ema, with_ema.flat.data) and with_ema.ema.data_ptr() != with_ema.flat.data.data_ptr()
    assert torch.equal(with_ema.flat.data, without.flat.data)
    for k in range(3):
        prev = with_ema.ema.cpu()
        before = with_ema.flat.data.cpu()
        with_ema.step(clean, cond, noise=noise, t=t)
        without.step(clean, cond, noise=noise, t=t)
        torch.cuda.synchronize()
        assert torch.equal(with_ema.flat.data, without.flat.data), k
        assert torch.equal(with_ema.m, without.m) and torch.equal(with_ema.v, without.v), k
        p_new = with_ema.flat.data.cpu()
        assert not torch.equal(p_new, before), k
        assert torch.equal(with_ema.ema.cpu(), er.ema_update(prev, p_new, k, 0.9, True)), k
    assert with_ema.steps_done() == 3


def test_step_ema_captured_graph(small):
    """capture() leaves the EMA as it was (its warm-up steps are undone), and every replay applies the recurrence
    to the parameters that replay produced."""
    from fmdiff.pipelines.train.fused import FusedTrainStep
    _, _, clean, cond, noise, t = small
    step = FusedTrainStep(_model(small), lr=1e-3, warmup=0, total_steps=100, ema_decay=0.9)
    ema0 = step.ema.cpu()
    step.capture(clean, cond, warmup_iters=2, noise=noise, t=t)
    torch.cuda.synchronize()
    assert torch.equal(step.ema.cpu(), ema0) and torch.equal(step.flat.data.cpu(), ema0)
    for k in range(3):
        prev = step.ema.cpu()
        step.replay()
        torch.cuda.synchronize()
        p_new = step.flat.data.cpu()
        assert torch.equal(step.ema.cpu(), er.ema_update(prev, p_new, k, 0.9, True)), k
        assert not torch.equal(step.ema.cpu(), p_new), k
    assert step.steps_done() == 3


def test_step_ema_swap(small):
    from fmdiff.pipelines.train.fused import FusedTrainStep
    _, _, clean, cond, noise, t = small
    model = _model(small)
    step = FusedTrainStep(model, lr=1e-3, warmup=0, total_steps=100, ema_decay=0.9)
    for _ in range(2):
        step.step(clean, cond, noise=noise, t=t)
    data0, ema0 = step.flat.data.clone(), step.ema.clone()
    ptrs = (step.flat.data.data_ptr(), step.ema.data_ptr())
    assert not torch.equal(data0, ema0)
    ema_sd = step.ema_state_dict()
    assert list(ema_sd) == list(model.state_dict()) and all(v.device.type == "cpu" for v in ema_sd.values())
    x = clean * 0.5 + 0.25 * noise
    tt = torch.tensor([100.0, 700.0], device=DEV)

    def fwd(m):
        with torch.no_grad():
            return m(x, tt, context=cond).clone()

    def same(a, b):   # bit equality where the forward is deterministic, else within twice its own noise
        return torch.equal(a, b) if noise_floor == 0.0 else (a - b).abs().max().item() <= 2.0 * noise_floor

    step.eng.invalidate_weights()           # the step wrote the masters through raw pointers
    y_raw = fwd(model)
    fresh = _model(small)
    fresh.load_state_dict(ema_sd)
    y_f1, y_f2 = fwd(fresh), fwd(fresh)
    noise_floor = (y_f1 - y_f2).abs().max().item()
    with step.ema_swap():
        sd_in = model.state_dict()
        for k, v in ema_sd.items():
            assert torch.equal(sd_in[k].cpu(), v), k
        y_swapped = fwd(model)
        with pytest.raises(RuntimeError):
            step.step(clean, cond, noise=noise, t=t)
        with pytest.raises(RuntimeError):
            step.replay()
    diff = (y_swapped - y_f1).abs().max().item()
    print(f"fresh model run-to-run max|diff| {noise_floor:.3e}; swapped vs fresh max|diff| {diff:.3e}; "
          f"swapped vs raw max|diff| {(y_swapped - y_raw).abs().max().item():.3e}")
    assert not torch.equal(y_swapped, y_raw)
    assert same(y_swapped, y_f1)
    assert torch.equal(step.flat.data, data0) and torch.equal(step.ema, ema0)
    assert ptrs == (step.flat.data.data_ptr(), step.ema.data_ptr())
    assert same(fwd(model), y_raw)   # the exit refreshed the kernel weights from the restored masters
    # round trip of the state dict, and an exception inside the context still swaps back
    step.ema.zero_()
    step.load_ema_state_dict(ema_sd)
    assert torch.equal(step.ema, ema0)
    with pytest.raises(KeyError):
        with step.ema_swap():
            raise KeyError("boom")
    assert torch.equal(step.flat.data, data0) and torch.equal(step.ema, ema0)
    step.step(clean, cond, noise=noise, t=t)    # and the step runs again afterwards
    with pytest.raises(RuntimeError):
        FusedTrainStep(_model(small), lr=1e-3).ema_state_dict()


# ------------------------------------------------------------------ 9. the trainer loop
UNET = {"sample_size": 32, "in_channels": 1, "out_channels": 1, "layers_per_block": 1, "block_out_channels": [32, 64],
        "attention_resolutions": []}
PARENT_KEYS = {"model", "optimizer", "lr_scheduler", "scaler", "epoch", "best_metric"}


def _dataset():
    """Four synthetic items ({"target", "image"}: the conditioning image rides along as in test_gpu_trainer.py)."""
    from fmdiff.data import TensorPairDataset
    g = torch.Generator().manual_seed(0)
    clean = torch.rand(4, 1, 32, 32, generator=g)
    ldct = (clean + 0.05 * torch.randn(4, 1, 32, 32, generator=g)).clamp(0, 1)
    return TensorPairDataset(clean, ldct)


def _cfg(tmp, name, out, epochs=2, ema=True, images=False):
    tr = {"batch_size": 4, "num_epochs": epochs, "learning_rate": 1e-3, "lr_warmup_steps": 0,
          "conditioning": "concatenate", "channels": 1, "num_workers": 0, "seed": 3, "save_images": images,
          "save_images_every": 1, "visual_samples": 4, "num_inference_steps": 2, "save_model_epochs": 1,
          "output_dir": out}
    if ema:
        tr["ema_decay"] = 0.9
    cfg = {"training": tr, "model": {"unet": UNET, "model_type": "flow_matching",
                                     "scheduler": {"name": "flow_match_euler", "num_train_timesteps": 1000,
                                                   "num_inference_steps": 2}}}
    path = os.path.join(tmp, f"{name}.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    return path


def _seeded_factory(made):
    """FusedTrainStep whose random draws and batch order depend on the optimizer step count and the batch's content
    alone, so that a resumed run sees exactly what the uninterrupted run saw (the loop's shuffle and the device RNG
    do not survive a restart; the reference's do not either)."""
    from fmdiff.pipelines.train.fused import FusedTrainStep

    class Seeded(FusedTrainStep):
        def _draw(self, clean, ldct):
            order = clean.flatten(1).sum(1).argsort()
            g = torch.Generator().manual_seed(1000 + self.steps_done())
            noise = torch.randn(clean.shape, generator=g).to(clean.device)
            t = torch.rand(clean.shape[0], generator=g).to(clean.device)
            return clean[order].contiguous(), ldct[order].contiguous(), noise, t

        def capture(self, clean, ldct, warmup_iters=2, context_ca=None, **kw):
            c, l, n, t = self._draw(clean, ldct)
            return super().capture(c, l, warmup_iters=warmup_iters, noise=n, t=t)

        def replay(self, clean=None, ldct=None, context_ca=None, **kw):
            c, l, n, t = self._draw(clean, ldct)
            return super().replay(clean=c, ldct=l, noise=n, t=t)

    def make(model, **kw):
        made.append(Seeded(model, **kw))
        return made[-1]
    return make


def test_trainer_ema_checkpoint_resume_and_off(tmp_path, monkeypatch):
    from fmdiff.pipelines.train import flow_matching_lib, loop
    tmp = str(tmp_path)
    ds = _dataset()
    made, swapped = [], []
    real_decode = loop.decode_diffusion_batch

    def spy_decode(model, *a, **kw):   # what the grids are sampled from: the parameter buffer at that moment
        swapped.append((made[-1]._swapped, made[-1].flat.data.clone()))
        return real_decode(model, *a, **kw)

    monkeypatch.setattr(loop, "decode_diffusion_batch", spy_decode)
    # uninterrupted: two epochs (one full batch each), grids after both
    full = _cfg(tmp, "full", os.path.join(tmp, "full"), images=True)
    out_full = str(loop.run_training(ds, full, objective="flow_matching", step_factory=_seeded_factory(made)))
    st = made[-1]
    assert [flag for flag, _ in swapped] == [True, True]
    assert torch.equal(swapped[-1][1], st.ema) and not torch.equal(swapped[-1][1], st.flat.data)
    last = torch.load(os.path.join(out_full, "flow_last.pt"), weights_only=True)
    assert set(last) == PARENT_KEYS | {"ema"} and last["epoch"] == 2
    assert list(last["ema"]) == list(last["model"])
    assert any(not torch.equal(last["ema"][k], last["model"][k]) for k in last["model"])
    for k, v in st.ema_state_dict().items():
        assert torch.equal(v, last["ema"][k]), k
    # stopped after epoch 1 (its checkpoint is all that survives) and resumed for epoch 2
    first = os.path.join(out_full, "epochs", "epoch0001", "epoch.pt")
    assert "ema" in torch.load(first, weights_only=True)
    resumed = _cfg(tmp, "resumed", os.path.join(tmp, "resumed"))
    out_res = str(loop.run_training(ds, resumed, resume=first, objective="flow_matching",
                                    step_factory=_seeded_factory(made)))
    again = torch.load(os.path.join(out_res, "flow_last.pt"), weights_only=True)
    assert again["epoch"] == 2 and set(again) == set(last)
    for key in ("model", "ema"):
        for k in last[key]:
            assert torch.equal(again[key][k], last[key][k]), (key, k)
    # the sampling side reads either set of weights from the trainer's file
    from fmdiff.utils.model_utils import build_diffusion_model
    cfg = json.load(open(full))
    m_ema = build_diffusion_model(cfg, DEV, ckpt_path=os.path.join(out_full, "flow_last.pt"), use_ema=True)
    for k, v in m_ema.state_dict().items():
        assert torch.equal(v.cpu(), last["ema"][k]), k
    # the same run without ema_decay, through the public entry point: exactly the parent's keys
    off = _cfg(tmp, "off", os.path.join(tmp, "off"), ema=False)
    flow_matching_lib.train(ds, off)
    ck = torch.load(os.path.join(tmp, "off_run1", "flow_last.pt"), weights_only=True)
    assert set(ck) == PARENT_KEYS and ck["epoch"] == 2
    # an EMA run resumed from a checkpoint without "ema" starts its EMA from the loaded parameters
    made.clear()
    cold = _cfg(tmp, "cold", os.path.join(tmp, "cold"), epochs=2)
    loop.run_training(ds, cold, resume=os.path.join(tmp, "off_run1", "flow_last.pt"), objective="flow_matching",
                      step_factory=_seeded_factory(made))
    st = made[-1]   # epochs 1..2 are done in the checkpoint: nothing trained, the EMA is the loaded model
    assert torch.equal(st.ema, st.flat.data)
    for k, v in st.ema_state_dict().items():
        assert torch.equal(v, ck["model"][k]), k
