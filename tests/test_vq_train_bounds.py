"""CPU tests of the quantizer-training yardsticks (tests/vq_train_bounds.py): the fp64 restatement reproduces the
reference's recorded steps and gradients (tests/golden/vq_train_golden*.pt) within the reference's own fp32
error; the torch fp32 emulation of the kernels' arithmetic stays inside the derived bounds; and the same
assertion rejects every mutant of the emulation:

  unused_not_decayed   codes no row chose keep ema_cluster_size / ema_w          (cs, w, e)
  zq_from_updated      z_q gathered from the embedding after the update          (zq)
  loss_from_updated    vq_loss taken against the embedding after the update      (vq_loss)
  classic_beta         the classic quantizer's dz with beta instead of beta - 1  (dz)
  no_eps               embedding = ema_w / ema_cluster_size                      (e)
  n_before             n summed before the cluster sizes are updated             (n)
  drop_row             the first row left out of its segment                     (w, e)
  pad_read             a padding channel (NaN) added into the last channel       (w, e)
"""
import pytest
import torch

import vq_bounds as vb
import vq_train_bounds as tb

BETA, DECAY, EPS, G_LOSS = 0.25, 0.99, 1e-5, 0.7
# name -> (M, K, D, sizes): K < M with repeated codes, and K > M with most codes unused
CASES = {"m105_k100_d8": (105, 100, 8, "rand"), "m128_k512_d64": (128, 512, 64, "rand"),
         "m128_k512_d64_dead": (128, 512, 64, "dead")}


def _inputs(name):
    M, K, D, sizes = CASES[name]
    emb, cs, w = tb.make_state(K, D, name, sizes)
    g = vb.gen(f"vq_train_cpu/{name}")
    j = torch.randint(0, K, (M,), generator=g)
    z = emb[j] + 0.05 * torch.randn(M, D, generator=g)
    z_pad = torch.full((M, D + 8), float("nan"))
    z_pad[:, :D] = z
    g_zq = torch.randn(M, D, generator=g)
    codes = vb.reference(z, emb)["idx"]
    return z, z_pad, codes, emb, cs, w, g_zq


@pytest.mark.parametrize("classic", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_emulation_within_bounds(name, classic):
    z, z_pad, codes, emb, cs, w, g_zq = _inputs(name)
    D = z.shape[1]
    got = tb.emulate(z_pad, D, codes, emb, cs, w, DECAY, EPS, BETA, classic, g_zq, G_LOSS)
    r = tb.check_step(name, got, z, codes, emb, cs, w, DECAY, EPS, BETA, classic, g_zq, G_LOSS)
    print(name, "classic" if classic else "ema", "error / bound:", {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) < 1.0


@pytest.mark.parametrize("mutant", tb.MUTANTS)
@pytest.mark.parametrize("name", ["m105_k100_d8", "m128_k512_d64"])
def test_mutants_are_rejected(name, mutant):
    z, z_pad, codes, emb, cs, w, g_zq = _inputs(name)
    D = z.shape[1]
    got = tb.emulate(z_pad, D, codes, emb, cs, w, DECAY, EPS, BETA, True, g_zq, G_LOSS, mutant=mutant)
    with pytest.raises(AssertionError):
        tb.check_step(f"{name} {mutant}", got, z, codes, emb, cs, w, DECAY, EPS, BETA, True, g_zq, G_LOSS)


def test_bound_constants_and_dead_codes():
    assert max(tb.C_CS, tb.C_W, tb.C_DZ, tb.C_DE) <= 8
    z, z_pad, codes, emb, cs, w, g_zq = _inputs("m128_k512_d64_dead")
    r = tb.update64(z, codes, cs, w, DECAY, EPS)
    dead = (cs == 0) & (r["n_k"] == 0)
    assert int(dead.sum()) > 50
    # a code with no mass gets ema_w / (eps n / (n + K eps)): about 1e5 times ema_w, the reference's behaviour
    want = r["w"][dead] / (EPS * r["n"] / (r["n"] + 512 * EPS))
    assert torch.allclose(r["e"][dead], want, rtol=1e-12) and float(r["e"][dead].abs().max()) > 1e4


@pytest.mark.parametrize("tag", list(tb.FIXTURE_SHAPES))
def test_restatement_reproduces_the_reference_steps(tag):
    G, h = tb.load_fixture()
    N, sp, K, D = tb.FIXTURE_SHAPES[tag]
    for s in range(tb.FIXTURE_STEPS):
        emb, cs, w = tb.fixture_state(G, tag, s)
        emb2, cs2, w2 = tb.fixture_state(G, tag, s + 1)
        z = tb.flat(G[f"{tag}.z{s}"])
        ref = vb.reference(z, emb)
        codes = G[f"{tag}.codes{s}"].reshape(-1)
        assert bool((ref["gap"] > 2.0 * vb.row_bound(ref)).all()) and torch.equal(ref["idx"], codes)
        r = tb.update64(z, codes, cs, w, h["decay"], h["eps"])
        b = tb.update_bounds(r, cs, w, h["decay"], h["eps"], reference=True)
        ratios = {k: tb.check(f"{tag} step {s}", v, r[k], b[k], k) for k, v in (("cs", cs2), ("w", w2), ("e", emb2))}
        q = emb[codes]
        want = G[f"{tag}.z{s}"] + (q.view(N, *sp, D).movedim(-1, 1) - G[f"{tag}.z{s}"])
        assert torch.equal(G[f"{tag}.z_q{s}"], want)      # the embedding from before the update
        loss64, perp64 = vb.stats64(z, emb, codes, h["beta"], False, h["eps"])
        assert abs(float(G[f"{tag}.vq_loss{s}"]) - loss64) <= 1e-5 * loss64
        assert abs(float(G[f"{tag}.perplexity{s}"]) - perp64) <= 1e-5 * perp64
        print(tag, "step", s, "reference error / its bound:", {k: round(v, 3) for k, v in ratios.items()})


@pytest.mark.parametrize("qt", ["ema", "classic"])
@pytest.mark.parametrize("tag", list(tb.FIXTURE_SHAPES))
def test_restatement_reproduces_the_reference_gradients(tag, qt):
    G, h = tb.load_fixture()
    emb = tb.fixture_state(G, tag, 0)[0]
    z, g_zq = tb.flat(G[f"{tag}.z0"]), tb.flat(G[f"{tag}.g_zq"])
    q = emb[G[f"{tag}.codes0"].reshape(-1)]
    c = h["beta"] - 1.0 if qt == "classic" else h["beta"]
    mag = h["g_loss"] * ((1.0 + h["beta"]) if qt == "classic" else h["beta"]) * 2.0 / z.numel()
    ratio = tb.check(f"{tag} {qt}", tb.flat(G[f"{tag}.{qt}.z_grad"]), tb.dz64(z, q, g_zq, h["g_loss"], c),
                     tb.dz_bound(z, q, g_zq, mag), "z.grad")
    print(tag, qt, "reference z.grad error / its bound:", round(ratio, 3))
    wrong = tb.dz64(z, q, g_zq, h["g_loss"], h["beta"] if qt == "classic" else h["beta"] - 1.0)
    with pytest.raises(AssertionError):
        tb.check(f"{tag} {qt}", tb.flat(G[f"{tag}.{qt}.z_grad"]), wrong, tb.dz_bound(z, q, g_zq, mag), "z.grad")
