"""CPU checks of tests/vq_join_bounds.py: the emulated arithmetic of the latent-join kernel lies within the derived
bound of the fp64 value, the bound is tight enough to catch wrong kernels (mutants), and the kernel's value equals
the existing latent gradient (``vq_train_bounds.emulate``'s dz) rounded once to bf16."""
import pytest
import torch

import vq_join_bounds as JB
import vq_train_bounds as TB

CASES = [(105, 1), (105, 12), (2112, 32), (105, 256)]


@pytest.mark.parametrize("M,D", CASES)
@pytest.mark.parametrize("c", [0.25, -0.75])
def test_emulation_within_the_bound(M, D, c):
    g, z, e, codes, g_loss = JB.make_case(M, D, 70, 1000 * D + M)
    q = e[codes]
    s = JB.coef64(g_loss, c, M, D)
    worst = 0.0
    for gg in (g, None):
        for gl in (g_loss, None):
            sv = JB.coef64(gl, c, M, D)
            v, bd = JB.exact(gg, z, q, sv), JB.bound(gg, z, q, sv)
            worst = max(worst, JB.check(f"M={M} D={D}", JB.emulate(gg, z, q, gl, c, M, D), v, bd))
            # the saved-residual mode: z - q rounded once, the same value
            r = z - q
            assert torch.equal(JB.emulate(gg, r, None, gl, c, M, D), JB.emulate(gg, z, q, gl, c, M, D))
    assert abs(s) > 0 and worst <= 1.0
    print(f"M={M} D={D} c={c}: largest error / bound {worst:.3f}")


def test_equals_the_fp32_latent_gradient_rounded_once():
    """``vq_train_bounds.emulate``'s dz is the arithmetic of fmd_vq_backward; the join is that, to bf16."""
    M, D, K = 105, 12, 70
    g, z, e, codes, g_loss = JB.make_case(M, D, K, 5)
    for classic in (False, True):
        beta = 0.25
        c = beta - 1.0 if classic else beta
        ref = TB.emulate(z, D, codes, e, torch.ones(K), e.clone(), 0.99, 1e-5, beta, classic, g, g_loss)["dz"]
        assert torch.equal(JB.emulate(g, z, e[codes], g_loss, c, M, D), ref.to(torch.bfloat16).float())


@pytest.mark.parametrize("mutant", JB.MUTANTS)
def test_mutants_miss_the_bound(mutant):
    M, D = 2112, 32
    g, z, e, codes, g_loss = JB.make_case(M, D, 70, 77)
    if mutant == "g_rounded_to_bf16_first":
        # the four-pass composition this kernel replaces: an fp32 data gradient rounded to bf16 on the way
        g = 0.1 * torch.randn((M, D), generator=torch.Generator().manual_seed(3))
    q = e[codes]
    s = JB.coef64(g_loss, -0.75, M, D)
    v, bd = JB.exact(g, z, q, s), JB.bound(g, z, q, s)
    JB.check("kernel", JB.emulate(g, z, q, g_loss, -0.75, M, D), v, bd)
    with pytest.raises(AssertionError, match="outside the bound"):
        JB.check(mutant, JB.emulate(g, z, q, g_loss, -0.75, M, D, mutant=mutant), v, bd)
