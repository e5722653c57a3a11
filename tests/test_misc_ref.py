"""misc_ref.py checked on the CPU before any GPU run.

1. Every fp64 restatement equals an independent torch formulation at 1e-12 relative: F.linear autograd (linear,
   linear_bwd, the grouped form, SiLU and its derivative), F.mse_loss autograd, torch.optim.AdamW(foreach=False) in
   double under transformers' get_cosine_schedule_with_warmup, F.avg_pool{1,2,3}d / F.interpolate(nearest) and their
   autograd, and the scheduler classes of fmdiff.pipelines.schedulers (one DPM-Solver++ and one UniPC plan, the
   eager ``step`` with its lincomb calls evaluated in fp64).
2. Every case the GPU modules run passes against the fp32 emulation (misc_ref.Emu): the lattices are exact, the
   guards hold, and every bound holds with no margin (ratio < 1).  Largest err / bound of the emulation:
   timestep_embedding 0.40 up to dim 128 and 0.52 at dim 320 (shift 1, t = 999), linear(in_silu) 0.07, dW 0.25,
   dx 0.97 (one fp32 rounding of old + dx: the bound is met, not padded), silu_bwd 0.33, mse loss 0.42 and dpred
   0.87 (one bf16 rounding), adamw p 0.58, m 0.85, v 0.93 (two or three roundings each).
3. Every lattice case passes unchanged with every reduction walked in a permuted order (Emu(perm=True)): no lattice
   case can pass by an accident of ordering.
4. Mutants of the emulation are rejected by the same checks at the same shapes.  Rejected / applicable cases
   (applicable: the cases of the family in which the bug can show at all, misc_ref.MUTANT_CASES):

   mutant               family               rejected   caught by
   half_no_shift        timestep_embedding     6/6      bound (shift = 1, dim > 2)
   flip_inverted        timestep_embedding    20/20     bound
   trunc_rounds         timestep_embedding     4/4      bound (t 999 with a fraction >= 1/2)
   pad_rows_stored      linear                20/20     guard / neighbour columns
   bias_twice           linear                12/12     lattice, bound (in_silu)
   dy_stride_ignored    linear_bwd            58/58     NaN around the dy slice (B > 1)
   db_not_accumulated   linear_bwd            74/74     lattice db
   cond_offset          noise_prepare         15/15     lattice
   pad_not_zeroed       noise_prepare         27/27     prefilled pad channels
   tb_sign_dropped      mse                   27/27     loss, dpred
   inv_numel_kpad       mse                   51/51     loss, dpred
   v_unscaled_g         adamw_sched           10/10     v bound
   bc2_no_sqrt          adamw                 10/10     p bound
   lambda_off_by_one    adamw_sched           20/20     p bound (s = 0: lambda = 0)
   index_zero           flow_euler             6/6      NaN sigma rows
   noise_base_ignored   ddpm_step              3/3      NaN noise rows
   ring_plus_one        sched_step             2/2      ring buffers
   last_not_updated     sched_step             1/1      last
   row_zero             gather_row             2/2      NaN table rows
   odd_row_included     resample2              8/8      lattice
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import misc_ref as mr

F64 = torch.float64
LATTICE_FAMILIES = ("linear", "linear_bwd", "grouped_linear", "noise_prepare", "mse", "sched_step", "lincomb",
                    "affine_channels", "add_", "sum_pool", "resample2")
ALL = mr.case_ids(mr.TIMEPATH + mr.STEPS + mr.RESAMPLE)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


# ------------------------------------------------------------------ 1. restatements vs independent formulations
@pytest.mark.parametrize("in_silu", [False, True])
def test_linear_refs_equal_autograd(in_silu):
    d = mr.linear_inputs(9, 200, 77, 1)
    x = d["x"].double().requires_grad_()
    w = d["w"].double().requires_grad_()
    b = d["b"].double().requires_grad_()
    y = F.linear(F.silu(x) if in_silu else x, w, b)
    y.backward(d["dy"][:, :77].double())
    assert _rel(mr.linear_ref(d["x"], d["w"], d["b"], in_silu), y.detach()) < 1e-12
    dw, db, dx = mr.linear_bwd_ref(d["x"], d["w"], d["dy"], d["dw0"], d["db0"], d["dx0"], in_silu)
    assert _rel(dw - d["dw0"].double(), w.grad) < 1e-12
    assert _rel(db - d["db0"].double(), b.grad) < 1e-12
    assert _rel(dx - d["dx0"].double(), x.grad) < 1e-12
    z = torch.linspace(-30, 30, 1001, dtype=F64).requires_grad_()
    F.silu(z).sum().backward()
    assert _rel(mr.silu_grad64(z.detach()), z.grad) < 1e-12


def test_mse_ref_equals_autograd():
    d = mr.mse_inputs("odd", 3, 8)
    pred = d["pred"].double().movedim(1, -1).contiguous().requires_grad_()
    tgt = (d["ta"].double() - d["tb"].double()).movedim(1, -1)
    loss = F.mse_loss(pred, tgt)
    (0.25 * loss).backward()
    full = torch.cat([pred.detach(), torch.full((*pred.shape[:-1], 5), float("nan"), dtype=F64)], -1)
    rl, rg, _, _ = mr.mse_ref(full, d["ta"], d["tb"], -1.0, 0.25)
    assert _rel(rl, loss.detach()) < 1e-12 and _rel(rg[..., :3], pred.grad) < 1e-12
    assert bool((rg[..., 3:] == 0).all())


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_ref_equals_torch_adamw_with_cosine_warmup(wd):
    from transformers import get_cosine_schedule_with_warmup
    hp = mr.ADAMW_HP
    p = torch.randn(257, generator=mr.rng(3)).double()
    ref = p.clone().requires_grad_()
    opt = torch.optim.AdamW([ref], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd,
                            foreach=False)
    sch = get_cosine_schedule_with_warmup(opt, mr.SCHED_WARMUP, mr.SCHED_TOTAL)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for s in range(9):                                   # through s == warmup, s == total and beyond
        g = mr.adamw_grad(257, s + 1).double()
        assert abs(opt.param_groups[0]["lr"] - hp["lr"] * mr.cosine_lambda(s, mr.SCHED_WARMUP, mr.SCHED_TOTAL)) \
            <= 1e-15
        ref.grad = g.clone()
        opt.step()
        sch.step()
        (p, m, v), _ = mr.adamw_ref(p, g, m, v, hp["lr"] * mr.cosine_lambda(s, mr.SCHED_WARMUP, mr.SCHED_TOTAL),
                                    hp["b1"], hp["b2"], hp["eps"], wd, 1 - hp["b1"] ** (s + 1),
                                    1 - hp["b2"] ** (s + 1))
        assert _rel(p, ref.detach()) < 1e-12, s
        st = opt.state[ref]
        assert _rel(m, st["exp_avg"]) < 1e-12 and _rel(v, st["exp_avg_sq"]) < 1e-12


@pytest.mark.parametrize("kind", list(mr.RESAMPLE_SETS))
def test_resample_refs_equal_pool_and_interpolate(kind):
    factors, low = mr.RESAMPLE_SETS[kind]
    nd = len(factors)
    pool = {1: F.avg_pool1d, 2: F.avg_pool2d, 3: F.avg_pool3d}[nd]
    for odd in [None] + [j for j, f in enumerate(factors) if f == 2]:
        high = tuple(f * l + (1 if j == odd else 0) for j, (f, l) in enumerate(zip(factors, low)))
        g = mr.rng(5)
        h = torch.randn((2, *high, 3), generator=g, dtype=F64)
        lo = torch.randn((2, *low, 3), generator=g, dtype=F64)
        hc = h.movedim(-1, 1).clone().requires_grad_()
        pooled = pool(hc, kernel_size=factors, stride=factors)           # floor mode drops the odd index
        nblk = 1
        for f in factors:
            nblk *= f
        assert _rel(mr.resample_down_ref(h, low, factors, 0.25), 0.25 * nblk * pooled.detach().movedim(1, -1)) < 1e-12
        pooled.backward(lo.movedim(-1, 1) * nblk)                        # avg-pool data gradient x block size
        up = mr.resample_up_ref(lo, high, factors, 1.0)
        assert _rel(up, hc.grad.movedim(1, -1)) < 1e-12
        near = F.interpolate(lo.movedim(-1, 1), scale_factor=tuple(float(f) for f in factors), mode="nearest")
        pad = []
        for j in reversed(range(nd)):
            pad += [0, high[j] - factors[j] * low[j]]
        assert _rel(up, F.pad(near, pad).movedim(1, -1)) < 1e-12
        # the nearest-x2 data gradient is the block sum: autograd of interpolate
        lc = lo.movedim(-1, 1).clone().requires_grad_()
        F.interpolate(lc, scale_factor=tuple(float(f) for f in factors), mode="nearest").backward(
            h.movedim(-1, 1)[(slice(None), slice(None), *[slice(0, f * l) for f, l in zip(factors, low)])])
        assert _rel(mr.resample_down_ref(h, low, factors, 1.0), lc.grad.movedim(1, -1)) < 1e-12


@pytest.mark.parametrize("kind", ["dpm", "unipc"])
def test_sched_step_ref_equals_scheduler_classes(kind, monkeypatch):
    """The header's formula on a scheduler's own plan() rows against the same scheduler's eager step(), whose
    lincomb calls are evaluated in fp64 here (coefficients at their fp32 ABI values, as fmd_lincomb gets them)."""
    from fmdiff.pipelines import schedulers as S
    monkeypatch.setattr(S.ops, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(S.ops, "lincomb", lambda out, ins, cs: sum(mr.f32(c) * t.double() for t, c in zip(ins, cs)))
    monkeypatch.setattr(S._MultistepBase, "_prep", staticmethod(lambda mo, x: (mo.double(), x.double())))
    sch = (S.DPMSolverMultistepScheduler(solver_order=3) if kind == "dpm"
           else S.UniPCMultistepScheduler(solver_order=3))
    sch.set_timesteps(7)
    rows = sch.plan()
    assert rows.shape == (7, mr.NCOEF)
    assert bool((rows[:, 2] != 0).any()) == (kind == "unipc")
    g = mr.rng(7)
    sh = (2, 2, 5, 7)
    x = torch.randn(sh, generator=g, dtype=F64)
    xs = x.clone()
    ring = [torch.zeros(sh, dtype=F64) for _ in range(4)]
    last = torch.zeros(sh, dtype=F64) if kind == "unipc" else None
    for i, t in enumerate(sch.timesteps):
        eps = torch.randn(sh, generator=g, dtype=F64)
        xs = sch.step(eps, t, xs).prev_sample
        x, ring, last = mr.sched_step_ref(x, eps, ring, last, rows[i], i)
        assert _rel(x, xs) < 1e-12, i


def test_noise_prepare_and_lincomb_refs():
    d = mr.noise_prepare_inputs("ddpm", 2, 3)
    v = mr.noise_prepare_ref(d["x0"], d["noise"], d["ca"], d["cb"], d["cond"], 8)
    n = 1
    want = d["ca"][n].double() * d["x0"][n].double() + d["cb"][n].double() * d["noise"][n].double()
    assert torch.equal(v[n, ..., :2], want.movedim(0, -1))
    assert torch.equal(v[n, ..., 2:5], d["cond"][n].double().movedim(0, -1))
    assert bool((v[..., 5:] == 0).all())
    d = mr.noise_prepare_inputs("fm", 1, 0)
    v = mr.noise_prepare_ref(d["x0"], d["noise"], d["ca"], None, None, 8)
    t = d["ca"].double().view(-1, 1, 1, 1)
    assert torch.equal(v[..., :1], torch.lerp(d["x0"].double(), d["noise"].double(), t).movedim(1, -1))
    ins = [torch.randn(9, dtype=F64) for _ in range(3)]
    cs = [0.5, -2.0, 3.0]
    assert _rel(mr.lincomb_ref(ins, cs), torch.stack(ins, 1) @ torch.tensor(cs, dtype=F64)) < 1e-12


# ------------------------------------------------------------------ 2. / 3. the emulation passes every case
@pytest.mark.parametrize("family,case", ALL, ids=[f"{f}-{c}" for f, c in ALL])
def test_emulation_passes(family, case):
    """Every case the GPU modules run, against the fp32 emulation: exact where a lattice is used, ratio < 1 (no
    margin) where a bound is used."""
    r = mr.CASES[family][case](mr.Emu(), "cpu")
    if r is not None:
        assert r < 1.0, f"{family} {case}: fp32 emulation at {r:.3f} of the bound"
    if family == "timestep_embedding" and "trunc" not in case and "dim320" not in case:
        assert r < 0.5                                   # the fp32 reference sits below half of the bound (dim <= 128)


LATTICE = [(f, c) for f, c in ALL if f in LATTICE_FAMILIES and "silu" not in c and "-lincomb" not in c
           and not (f == "mse" and c.startswith("odd"))]


@pytest.mark.parametrize("family,case", LATTICE, ids=[f"{f}-{c}" for f, c in LATTICE])
def test_lattice_is_order_independent(family, case):
    """The fp32 evaluation in a permuted order equals the fp64 one bit for bit."""
    mr.CASES[family][case](mr.Emu(perm=True), "cpu")


# ------------------------------------------------------------------ 4. mutants
@functools.lru_cache(maxsize=None)
def _rejected(mutant):
    family, applies = mr.MUTANT_CASES[mutant]
    out = {}
    for case, fn in mr.CASES[family].items():
        if not applies(case):
            continue
        try:
            fn(mr.Emu(mutant=mutant), "cpu")
            out[case] = False
        except AssertionError:
            out[case] = True
    return out


@pytest.mark.parametrize("mutant", list(mr.MUTANT_CASES))
def test_mutant_is_rejected_in_every_applicable_case(mutant):
    res = _rejected(mutant)
    assert res, "no applicable case"
    missed = [c for c, ok in res.items() if not ok]
    assert not missed, f"{mutant} ({mr.MUTANTS[mutant]}) passes in {missed}"


def test_every_mutant_has_cases():
    assert set(mr.MUTANT_CASES) == set(mr.MUTANTS)
