"""CPU restatement of the EMA half of fmd_adamw_sched_ema, its mutants, and the inputs the tests share.

The kernel's contract (include/fmdiff.h), with s = step_ctr[0] (0-based, the s of the LR schedule):

    d   = ema_warmup ? min(decay, (1 + s) / (10 + s)) : decay
    ema = ema + (1 - d) * (p_new - ema)

where (1 + s) / (10 + s) is the fp32 division of (float)s + 1.0f by (float)s + 10.0f, 1 - d is one fp32 subtraction and
the last line is three separately rounded fp32 operations.  ``ema_update`` states exactly that with one torch op per
rounding (torch.add / sub / mul / div / minimum on fp32 CPU tensors are the IEEE operations, none of them fused), so
its result is the kernel's bit for bit; the GPU tests compare with ``torch.equal``.

``p_new`` is an input here: on the GPU it is what the launch wrote to ``p`` (checked bit for bit against
fmd_adamw_sched on copies of the same inputs).  On the CPU, where no AdamW with the kernel's FMA contraction exists,
``adamw_cpu`` gives a stand-in of the right size (the same formula in plain fp32 ops, equal to the kernel's to a few
ulp): good enough to show that the EMA inputs tell ``p`` before the update from ``p`` after it.
"""
import math

import torch

F32 = torch.float32

# AdamW hyper-parameters of the kernel tests.  LR warm-up 0 so that the LR is non-zero at s = 0 (with a warm-up the
# schedule's first step has lr = 0 and p_new = p, which would hide a kernel that averages the old p); the horizon
# keeps the cosine factor at 0.5 for s = 100000.
HP = dict(base_lr=1e-2, warmup=0, total=200000, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, grad_scale=1.0)

NS = (1, 3, 4, 5, 1023, 4103)          # vector-only, tail-only and both
# (name, decay, ema_warmup, step counts).  decay 0.9 meets the warm-up value at s = 80 (80/89 below, 81/90 equal,
# 82/91 above).  For 0.9999 the issue's {0, 8990, 8991} all lie in the warm-up region (8991/9000 = 0.999); the
# crossing of 0.9999 is at s = 89990 (89991/90000), so its neighbours are swept too.
SWEEPS = (
    ("d0.9", 0.9, True, (0, 1, 79, 80, 81, 100000)),
    ("d0.9999", 0.9999, True, (0, 8990, 8991, 89989, 89990, 89991)),
    ("d0.9-nowarm", 0.9, False, (0, 1, 79, 80, 81, 100000)),
    ("d0.9999-nowarm", 0.9999, False, (0, 8990, 8991)),
)


def make_inputs(n: int, seed: int = 0):
    """Seeded fp32 CPU (p, g, m, v, ema) with ema != p everywhere that matters."""
    gen = torch.Generator().manual_seed(1234 + 7 * n + seed)
    p = torch.randn(n, generator=gen) * 0.5
    g = torch.randn(n, generator=gen) * 0.1
    m = torch.randn(n, generator=gen) * 0.05
    v = torch.rand(n, generator=gen) * 0.01 + 1e-4
    ema = p + 0.05 * torch.randn(n, generator=gen) + 0.01
    return p, g, m, v, ema


def make_grad(n: int, k: int):
    """The fresh gradient of launch ``k`` in the successive-launch test."""
    gen = torch.Generator().manual_seed(99000 + 13 * n + k)
    return torch.randn(n, generator=gen) * 0.1


def one_minus_decay(s: int, decay: float, warmup: bool = True, mutant: str = None) -> torch.Tensor:
    """0-dim fp32 tensor (1 - d)."""
    if mutant == "no_warmup":
        warmup = False
    if mutant == "s_plus_one":
        s = s + 1
    if mutant == "s_minus_one":
        s = s - 1
    if mutant == "omd_fp64":   # d and 1 - d formed in double precision, rounded to fp32 once at the end
        d = min(decay, (1.0 + s) / (10.0 + s)) if warmup else decay
        return torch.tensor(1.0 - d, dtype=torch.float64).to(F32)
    d = torch.tensor(decay, dtype=F32)
    if warmup:
        sf = torch.tensor(s, dtype=torch.int32).to(F32)                     # (float)s
        w = torch.div(torch.add(sf, torch.tensor(1.0, dtype=F32)), torch.add(sf, torch.tensor(10.0, dtype=F32)))
        d = torch.minimum(d, w)
    return torch.sub(torch.tensor(1.0, dtype=F32), d)


def ema_update(ema: torch.Tensor, p_new: torch.Tensor, s: int, decay: float, warmup: bool = True,
               mutant: str = None) -> torch.Tensor:
    """The EMA after the launch at step count ``s`` (fp32 CPU tensors in, a new fp32 CPU tensor out)."""
    assert ema.dtype == F32 and p_new.dtype == F32 and ema.device.type == "cpu" and p_new.device.type == "cpu"
    omd = one_minus_decay(s, decay, warmup, mutant)
    return torch.add(ema, torch.mul(omd, torch.sub(p_new, ema)))


MUTANTS = ("p_before_update", "no_warmup", "s_plus_one", "s_minus_one", "omd_fp64")


def mutant_update(mutant: str, ema, p_old, p_new, s: int, decay: float, warmup: bool) -> torch.Tensor:
    if mutant == "p_before_update":
        return ema_update(ema, p_old, s, decay, warmup)
    return ema_update(ema, p_new, s, decay, warmup, mutant)


# Cases at which each mutant must be visible, from the formulas alone (sweep name -> step counts):
# * p_before_update: every case, the LR being non-zero at every s of the sweeps;
# * no_warmup: where the warm-up value (1 + s) / (10 + s) is below the decay by more than an fp32 ulp (at s = 89989
#   it is 1.1e-9 below 0.9999);
# * s_plus_one / s_minus_one: where the warm-up value is the minimum at s and at the shifted s (at s = 80 only the
#   shift down leaves the plateau; at s >= 81 neither does; at s ~ 9e3 the value still moves by 1.1e-7, two ulp);
# * omd_fp64: where d is the decay itself: 1.0f - (float)0.9 = 0.10000002 but (float)(1.0 - 0.9) = 0.1, and
#   1.0001659e-4 against 1.0000000e-4 for 0.9999.  (Where d is the warm-up value the two roundings may agree.)
MUST_SHOW = {
    "p_before_update": {name: steps for name, _, _, steps in SWEEPS},
    "no_warmup": {"d0.9": (0, 1, 79), "d0.9999": (0, 8990, 8991)},
    "s_plus_one": {"d0.9": (0, 1, 79), "d0.9999": (0, 8990, 8991)},
    "s_minus_one": {"d0.9": (0, 1, 79, 80), "d0.9999": (0, 8990, 8991)},
    "omd_fp64": {"d0.9": (81, 100000), "d0.9-nowarm": (0, 1, 79, 80, 81, 100000), "d0.9999-nowarm": (0, 8990, 8991)},
}


def lr_at(s: int) -> float:
    """get_cosine_schedule_with_warmup's LR after s scheduler steps, as fmd_adamw_sched forms it (fp64 -> fp32)."""
    w, total = HP["warmup"], HP["total"]
    if s < w:
        lam = s / max(1, w)
    else:
        lam = max(0.0, 0.5 * (1.0 + math.cos(math.pi * 2.0 * 0.5 * ((s - w) / max(1, total - w)))))
    return float(torch.tensor(HP["base_lr"] * lam, dtype=torch.float64).to(F32))


def adamw_cpu(p, g, m, v, s: int):
    """(p_new, m_new, v_new): the kernel's AdamW formula in plain fp32 torch ops.  A stand-in for the host tests only
    (the kernel contracts some of these into FMAs, so its bits differ in the last place)."""
    step = s + 1
    lr = torch.tensor(lr_at(s), dtype=F32)
    b1, b2 = torch.tensor(HP["beta1"], dtype=F32), torch.tensor(HP["beta2"], dtype=F32)
    bc1 = torch.tensor(1.0 - HP["beta1"] ** step, dtype=torch.float64).to(F32)
    bc2s = torch.tensor(1.0 - HP["beta2"] ** step, dtype=torch.float64).to(F32).sqrt()
    gs = g * torch.tensor(HP["grad_scale"], dtype=F32)
    pn = p * (1.0 - lr * torch.tensor(HP["wd"], dtype=F32))
    mn = m + (gs - m) * (1.0 - b1)
    vn = v * b2 + (1.0 - b2) * gs * gs
    denom = vn.sqrt() / bc2s + torch.tensor(HP["eps"], dtype=F32)
    pn = pn - (lr / bc1) * (mn / denom)
    return pn, mn, vn
