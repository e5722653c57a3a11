"""EMA weights, the host side: the CPU restatement of fmd_adamw_sched_ema's recurrence discriminates its mutants
on the inputs of the GPU kernel test, and the configuration / checkpoint plumbing works without a GPU."""
import logging
import os

import pytest
import torch

import ema_ref as er


# ------------------------------------------------------------------ 1. the restatement and its mutants
def test_one_minus_decay_scalars():
    """The warm-up value meets decay 0.9 exactly at s = 80 and 0.9999 exactly at s = 89990, in fp32."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    assert torch.equal(er.one_minus_decay(0, 0.9), f(1.0) - f(1.0) / f(10.0))
    assert er.one_minus_decay(79, 0.9) > er.one_minus_decay(80, 0.9)
    assert torch.equal(er.one_minus_decay(80, 0.9), er.one_minus_decay(80, 0.9, warmup=False))
    assert torch.equal(er.one_minus_decay(81, 0.9), f(1.0) - f(0.9))
    # one step below the crossing the exact values differ by 1.1e-9, under an fp32 ulp of 0.9999 (6e-8)
    assert er.one_minus_decay(8991, 0.9999) > er.one_minus_decay(89989, 0.9999) >= er.one_minus_decay(89990, 0.9999)
    assert torch.equal(er.one_minus_decay(89990, 0.9999), er.one_minus_decay(89990, 0.9999, warmup=False))
    assert torch.equal(er.one_minus_decay(0, 0.9, warmup=False), f(1.0) - f(0.9))
    assert torch.equal(er.one_minus_decay(5, 0.0, warmup=True), f(1.0))   # decay 0: the EMA follows p


@pytest.mark.parametrize("mutant", er.MUTANTS)
def test_mutants_change_the_result(mutant):
    """Each mutant changes at least one bit of the result at every case where the formulas say it computes something
    else (ema_ref.MUST_SHOW), at the sizes with enough elements to see a last-place change of (1 - d) (n >= 1023);
    the handful of elements of the small sizes are counted and printed."""
    shown_small = total_small = 0
    for name, decay, warmup, steps in er.SWEEPS:
        must = er.MUST_SHOW[mutant].get(name, ())
        for s in steps:
            for n in er.NS:
                p, g, m, v, ema = er.make_inputs(n)
                p_new, _, _ = er.adamw_cpu(p, g, m, v, s)
                assert not torch.equal(p_new, p), (name, s, n)
                good = er.ema_update(ema, p_new, s, decay, warmup)
                bad = er.mutant_update(mutant, ema, p, p_new, s, decay, warmup)
                differs = not torch.equal(good, bad)
                if s in must:
                    if n >= 1023:
                        assert differs, (mutant, name, s, n)
                    else:
                        total_small += 1
                        shown_small += int(differs)
    assert any(er.MUST_SHOW[mutant].get(name) for name, *_ in er.SWEEPS[:3])
    print(f"{mutant}: visible in {shown_small}/{total_small} small-n cases where it must show at large n")


def test_restatement_is_the_recurrence_in_double_to_an_ulp():
    """Sanity of the helper itself: against ema + (1 - d)(p - ema) in fp64 it is off by rounding only."""
    for name, decay, warmup, steps in er.SWEEPS:
        for s in steps:
            p, g, m, v, ema = er.make_inputs(4103)
            p_new, _, _ = er.adamw_cpu(p, g, m, v, s)
            d = min(decay, (1.0 + s) / (10.0 + s)) if warmup else decay
            ref = ema.double() + (1.0 - d) * (p_new.double() - ema.double())
            got = er.ema_update(ema, p_new, s, decay, warmup).double()
            # three fp32 roundings on values of size <= ~3, and d itself rounded to fp32: a few 1e-7
            assert (got - ref).abs().max().item() < 2e-6, (name, s)


# ------------------------------------------------------------------ 2. configuration and checkpoint plumbing
def test_resolve_ema_off_and_on():
    from fmdiff import utils as U
    assert U.resolve_ema({}) == (None, True)
    assert U.resolve_ema({"ema_decay": None}) == (None, True)
    assert U.resolve_ema({"ema_decay": 0}) == (None, True)
    assert U.resolve_ema({"ema_decay": 0.0, "ema_warmup": False}) == (None, False)
    assert U.resolve_ema({"ema_decay": 0.999}) == (0.999, True)
    assert U.resolve_ema({"ema_decay": 0.9, "ema_warmup": False}) == (0.9, False)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            U.resolve_ema({"ema_decay": bad})


UNET = {"sample_size": 32, "in_channels": 1, "out_channels": 1, "layers_per_block": 1, "block_out_channels": [32, 64],
        "attention_resolutions": []}
CFG = {"training": {"conditioning": "concatenate", "channels": 1}, "model": {"unet": UNET}}


def _handmade_checkpoint(tmp_path, with_ema=True):
    from fmdiff.models.generators import DiffusionUNetFactory
    torch.manual_seed(5)
    m = DiffusionUNetFactory().build(UNET, "concatenate", 1)
    model_sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(6)
    ema_sd = {k: (v + 0.01 * torch.randn(v.shape, generator=gen) if v.is_floating_point() else v.clone())
              for k, v in model_sd.items()}
    payload = {"model": model_sd, "optimizer": None, "lr_scheduler": None, "scaler": None, "epoch": 3,
               "best_metric": 0.5}
    if with_ema:
        payload["ema"] = ema_sd
    path = tmp_path / ("with_ema.pt" if with_ema else "without_ema.pt")
    torch.save(payload, path)
    return path, model_sd, ema_sd


def test_build_diffusion_model_loads_ema_or_model(tmp_path):
    from fmdiff.utils.model_utils import build_diffusion_model
    path, model_sd, ema_sd = _handmade_checkpoint(tmp_path)
    got_ema = build_diffusion_model(CFG, "cpu", ckpt_path=path, use_ema=True).state_dict()
    got_model = build_diffusion_model(CFG, "cpu", ckpt_path=path, use_ema=False).state_dict()
    got_default = build_diffusion_model(CFG, "cpu", ckpt_path=path).state_dict()
    assert set(got_ema) == set(ema_sd)
    for k in ema_sd:
        assert torch.equal(got_ema[k], ema_sd[k]), k
        assert torch.equal(got_model[k], model_sd[k]), k
        assert torch.equal(got_default[k], model_sd[k]), k
    assert any(not torch.equal(ema_sd[k], model_sd[k]) for k in ema_sd)


def test_build_diffusion_model_use_ema_names_the_missing_key(tmp_path):
    from fmdiff.utils.model_utils import build_diffusion_model
    path, model_sd, _ = _handmade_checkpoint(tmp_path, with_ema=False)
    with pytest.raises(KeyError) as ei:
        build_diffusion_model(CFG, "cpu", ckpt_path=path, use_ema=True)
    assert str(path) in str(ei.value) and "'ema'" in str(ei.value)
    got = build_diffusion_model(CFG, "cpu", ckpt_path=path, use_ema=False).state_dict()   # "model" still loads
    for k in model_sd:
        assert torch.equal(got[k], model_sd[k]), k


class _FakeStep:
    """What maybe_load_checkpoint needs of a fused train step."""

    def __init__(self, ema):
        self.ema = ema
        self.calls = []

    def load_optimizer_state_dict(self, opt, sched=None):
        self.calls.append("opt")

    def load_ema_state_dict(self, sd):
        self.calls.append(("ema", sd))

    def reset_ema(self):
        self.calls.append("reset")


def test_maybe_load_checkpoint_restores_or_restarts_the_ema(tmp_path, caplog):
    from fmdiff import utils as U
    from fmdiff.models.generators import DiffusionUNetFactory
    with_ema, _, ema_sd = _handmade_checkpoint(tmp_path)
    without, _, _ = _handmade_checkpoint(tmp_path, with_ema=False)
    model = DiffusionUNetFactory().build(UNET, "concatenate", 1)
    # step with an EMA, payload with one: restored
    st = _FakeStep(ema=torch.zeros(1))
    assert U.maybe_load_checkpoint(with_ema, "flow", model, st) == (4, 0.5)
    (tag, sd), = st.calls
    assert tag == "ema" and all(torch.equal(sd[k], ema_sd[k]) for k in ema_sd)
    # step with an EMA, payload without: restart from the loaded parameters, with a warning
    st = _FakeStep(ema=torch.zeros(1))
    with caplog.at_level(logging.WARNING):
        U.maybe_load_checkpoint(without, "flow", model, st)
    assert st.calls == ["reset"]
    assert any("ema" in r.getMessage() and r.levelno == logging.WARNING for r in caplog.records)
    # step without an EMA: the payload's entry is ignored
    st = _FakeStep(ema=None)
    U.maybe_load_checkpoint(with_ema, "flow", model, st)
    assert st.calls == []


def test_abi_declares_the_ema_entry_point():
    from fmdiff import _lib
    sig = _lib.SIGNATURES["fmd_adamw_sched_ema"]
    old = _lib.SIGNATURES["fmd_adamw_sched"]
    # (p, g, m, v, ema, n, ...old tail..., ema_decay, ema_warmup, stream)
    assert sig[:5] == [_lib.p] * 5 and sig[5:-3] == old[4:-1] and sig[-3:] == [_lib.f32, _lib.i32, _lib.p]
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmdiff.h")
    assert "int fmd_adamw_sched_ema(" in open(header).read()
