"""CPU checks of tests/bn_bounds.py: the closed forms equal torch's BatchNorm2d + LeakyReLU autograd in fp64, an fp32
emulation of the kernels' operation order lies within the derived bounds, and seven mutants of it miss them; the two-term forms likewise.

Inputs: per channel |mean| / std up to ``bn_bounds.MAX_MEAN_OVER_STD`` = 8 (so the variance's cancellation factor
reaches 193), dy with a non-zero mean, and elements with u = a x + b exactly 0 and on both sides of it.
"""
import pytest
import torch

import bn_bounds as B

F64 = torch.float64
CASES = [(105, 8), (105, 24), (2112, 64), (300, 512)]


def _setup(M, C, seed=0):
    T = B.make_inputs(M, C, seed)
    slab = B.slab_of(T["x"])
    E = B.emulate_fold(slab, M, T["gamma"], T["beta"], T["rm"], T["rv"])
    a, b = E["a"].clone(), E["b"].clone()
    B.plant_kink(T["x"], a, b)
    return T, slab, E, a, b


def test_input_ratio_and_kink_census():
    for M, C in CASES:
        T, slab, E, a, b = _setup(M, C)
        R = B.fold_ref(B.slab_of(B.make_inputs(M, C, 0)["x"]), M, T["gamma"], T["beta"], T["rm"], T["rv"])
        r = (R["mean"].abs() * R["rstd"])
        assert 7.0 < r.max().item() < 9.5, r.max().item()        # |mean| / std reaches 8
        assert B.kappa(R).max().item() > 100                      # and the variance cancels accordingly
        zero, pos, neg = B.kink_census(T["x"], a, b)
        assert zero >= 3 and pos > 0 and neg > 0, (zero, pos, neg)


def test_closed_form_equals_torch_autograd_fp64():
    torch.manual_seed(0)
    N, C, H, W = 3, 8, 5, 7
    for training in (True, False):
        x = torch.randn(N, C, H, W, dtype=F64, requires_grad=True)
        x.data[0, 0, 0, 0] = 0.0
        bn = torch.nn.BatchNorm2d(C).double()
        with torch.no_grad():
            bn.weight.copy_(torch.rand(C) + 0.5), bn.bias.copy_(torch.randn(C))
            bn.running_mean.copy_(torch.randn(C)), bn.running_var.copy_(torch.rand(C) + 0.5)
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        bn.train(training)
        y = torch.nn.functional.leaky_relu(bn(x), 0.2)
        g = torch.randn_like(y)
        (y * g).sum().backward()
        x2 = x.detach().clone().requires_grad_()
        w2, b2 = bn.weight.detach().clone().requires_grad_(), bn.bias.detach().clone().requires_grad_()
        y2, rm2, rv2 = B._BnAct.apply(x2, w2, b2, rm0, rv0, training, 1e-5, 0.1, 0.2)
        (y2 * g).sum().backward()
        for got, ref in ((y2, y), (x2.grad, x.grad), (w2.grad, bn.weight.grad), (b2.grad, bn.bias.grad),
                         (rm2, bn.running_mean), (rv2, bn.running_var)):
            assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
        # the flat restatement used for the kernels agrees with the node
        M = N * H * W
        f = x.detach().permute(0, 2, 3, 1).reshape(M, C)
        slab = torch.stack([f.sum(0), (f * f).sum(0)], -1)[None]
        R = B.fold_ref(slab, M, bn.weight.detach(), bn.bias.detach(), rm0, rv0, training=training)
        Rb = B.act_bwd_ref(g.permute(0, 2, 3, 1).reshape(M, C), f, R["a"], R["b"], R["mean"], R["rstd"], M,
                           training=training)
        assert (Rb["dx"] - x.grad.permute(0, 2, 3, 1).reshape(M, C)).abs().max().item() <= 1e-12
        assert (Rb["dgamma"] - bn.weight.grad).abs().max().item() <= 1e-11
        assert (Rb["dbeta"] - bn.bias.grad).abs().max().item() <= 1e-11


def test_derivative_at_zero_is_slope():
    x = torch.zeros(4, dtype=F64, requires_grad=True)
    torch.nn.functional.leaky_relu(x, 0.2).sum().backward()
    assert torch.equal(x.grad, torch.full((4,), 0.2, dtype=F64))
    R = B.act_bwd_ref(torch.ones(4, 1), torch.zeros(4, 1), None, None, None, None, 4)
    assert torch.equal(R["dx"], torch.full((4, 1), 0.2, dtype=F64))


def _fold_ratios(M, T, slab, E, training=True, mutant=None):
    E = B.emulate_fold(slab, M, T["gamma"], T["beta"], T["rm"], T["rv"], training=training, mutant=mutant)
    R = B.fold_ref(slab, M, T["gamma"], T["beta"], T["rm"], T["rv"], training=training)
    Bd, b_ref = B.fold_bounds(R, M, T["gamma"], T["beta"], T["rm"], T["rv"], E["a"], training=training)
    out = {k: B.ratio(E[k], R[k], Bd[k]) for k in ("mean", "rstd", "a")}
    out["b"] = B.ratio(E["b"], b_ref, Bd["b"])
    if training:
        out["rm"], out["rv"] = B.ratio(E["rm"], R["rm"], Bd["rm"]), B.ratio(E["rv"], R["rv"], Bd["rv"])
    else:
        assert torch.equal(E["rm"], T["rm"]) and torch.equal(E["rv"], T["rv"])
    return out


def _act_ratios(M, T, a, b, E, training=True, norm=True, mutant=None, acc=True, a_fwd=None):
    x, dy = T["x"], T["dy"]
    out = {}
    if not norm:
        v, b32 = B.act_fwd_ref(x, None, None)
        out["y"] = B.ratio(B.emulate_fwd(x, None, None), v, B.bf16_store(v, b32))
        R = B.act_bwd_ref(dy, x, None, None, None, None, M)
        out["dx"] = B.ratio(B.emulate_bwd(dy, x, None, None, None, None, M)["dx"], R["dx"],
                            B.act_bwd_bounds(R, x, None, None, None, M)["dx"])
        return out
    v, b32 = B.act_fwd_ref(x, a, b)
    out["y"] = B.ratio(B.emulate_fwd(x, a if a_fwd is None else a_fwd, b), v, B.bf16_store(v, b32))
    og, ob = (T["old_dgamma"], T["old_dbeta"]) if acc else (None, None)
    mean, rstd = E["mean"], E["rstd"]
    running = (T["rm"], (1 / torch.sqrt(T["rv"].double() + 1e-5)).float())
    R = B.act_bwd_ref(dy, x, a, b, mean, rstd, M, training=training, old_dgamma=og, old_dbeta=ob)
    Bd = B.act_bwd_bounds(R, x, a, mean, rstd, M, training=training, old_dgamma=og, old_dbeta=ob)
    G = B.emulate_bwd(dy, x, a, b, mean, rstd, M, training=training, old_dgamma=og, old_dbeta=ob, mutant=mutant,
                      running=running)
    for k in ("dx", "dgamma", "dbeta"):
        out[k] = B.ratio(G[k], R[k], Bd[k])
    return out


@pytest.mark.parametrize("M,C", CASES)
def test_emulation_within_bounds(M, C):
    T, slab, E, a, b = _setup(M, C)
    worst = {}
    for training in (True, False):
        worst.update({f"fold.{training}.{k}": v for k, v in _fold_ratios(M, T, slab, E, training).items()})
        for acc in (True, False):
            worst.update({f"act.{training}.{acc}.{k}": v
                          for k, v in _act_ratios(M, T, a, b, E, training, acc=acc).items()})
    worst.update({f"plain.{k}": v for k, v in _act_ratios(M, T, a, b, E, norm=False).items()})
    print(M, C, {k: round(v, 3) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_image_maps_match_torch():
    x = torch.tensor([-3.0, -1.0, -0.999, 0.0, 0.5, 1.0, 1.5], dtype=F64, requires_grad=True)
    ((x.clamp(-1, 1) + 1) / 2).sum().backward()
    v, _ = B.image_bwd_ref(torch.ones(7), x.detach(), 1)
    assert torch.equal(v, x.grad) and v[1] == 0.5 and v[5] == 0.5 and v[0] == 0 and v[6] == 0
    x.grad = None
    torch.sigmoid(x).sum().backward()
    v, _ = B.image_bwd_ref(torch.ones(7), x.detach(), 2)
    assert (v - x.grad).abs().max().item() < 1e-15


MUTANTS = {
    "biased_running_var": ("fold", "rv"),
    "momentum_wrong_side": ("fold", "rm"),
    "a_bf16": ("fwd", "y"),
    "derivative_0_at_kink": ("bwd", "dx"),
    "derivative_1_at_kink": ("bwd", "dx"),
    "xhat_from_running": ("bwd", "dx"),
    "no_mean_term": ("bwd", "dx"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
@pytest.mark.parametrize("M,C", CASES)
def test_mutants_miss_the_bounds(M, C, mutant):
    T, slab, E, a, b = _setup(M, C)
    stage, key = MUTANTS[mutant]
    if stage == "fold":
        r = _fold_ratios(M, T, slab, E, True, mutant)[key]
    elif stage == "fwd":
        r = _act_ratios(M, T, a, b, E, a_fwd=a.to(torch.bfloat16).float())[key]
    else:
        # the kink mutants are judged in eval mode too, where nothing averages the planted elements away
        r = max(_act_ratios(M, T, a, b, E, training=tr, mutant=mutant)[key]
                for tr in ((True, False) if "kink" in mutant else (True,)))
    assert r > 1.5, (mutant, r)


@pytest.mark.parametrize("M,C", CASES)
def test_two_term_forms_within_bounds(M, C):
    """fp32 x (full mantissa): the two-term store of the forward, the backward on fp32 x and the block statistics."""
    T, slab, E, a, b = _setup(M, C)
    g = torch.Generator().manual_seed(M)
    x32 = T["x"].float() * (1 + 1e-3 * torch.randn(M, C, generator=g))
    B.plant_kink(x32, a, b)
    zero, pos, neg = B.kink_census(x32, a, b)
    assert zero >= 3 and pos > 0 and neg > 0
    v, b32 = B.act_fwd_ref(x32, a, b)
    hi, lo = B.emulate_fwd(x32, a, b, split=True)
    assert B.ratio(hi, v, B.bf16_store(v, b32)) <= 1.0
    assert B.ratio(hi.double() + lo.double(), v, B.split_store(v, b32)) <= 1.0
    assert B.ratio(hi, v, B.split_store(v, b32)) > 10      # one term alone misses the two-term bound
    R = B.act_bwd_ref(T["dy"], x32, a, b, E["mean"], E["rstd"], M)
    Bd = B.act_bwd_bounds(R, x32, a, E["mean"], E["rstd"], M)
    G = B.emulate_bwd(T["dy"], x32, a, b, E["mean"], E["rstd"], M)
    assert all(B.ratio(G[k], R[k], Bd[k]) <= 1.0 for k in ("dx", "dgamma", "dbeta"))
    # the block statistics: the reduce order on the first 64-row block
    ref, bound = B.stats_f32_ref(x32[:B.BN_ROWS])
    got = torch.stack([B._block_sum(x32[:B.BN_ROWS]), B._block_fma_sum(x32[:B.BN_ROWS], x32[:B.BN_ROWS])], -1)[None]
    assert B.ratio(got, ref, bound) <= 1.0
