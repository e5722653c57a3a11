"""GPU tests of the vector quantizer (csrc/vq.hip) through ops.vq_quantize, the codebook modules and VQVAE.

Kernel level: every case of CASES on the four input distributions of vq_bounds.py.  The codes are held to the
fp64 near-minimiser assertion (vq_bounds.check: excess <= 1.5 x bound per row, at most 3 % undecided rows, so the
fp64 argmin is forced on >= 97 % of the rows); z_q must equal torch's z + (E[codes] - z) bit for bit on the
kernel's own codes, its NHWC bf16 copy the round-to-nearest of that with zero padding channels; vq_loss (both
beta forms) and perplexity within 1e-5 relative of fp64; the histogram equal to bincount.  Every output lands
inside a sentinel buffer whose guards must come back untouched, and the latent's padding channels hold NaN.

Model level: the reference's own outputs (tests/golden/vq_golden.pt) for both quantizer types.
"""
import warnings

import pytest
import torch

import vq_bounds as vb

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64

# name -> (N, spatial, K, D, splits: "one" / "many" / None)
CASES = {
    "ragged_3x5x7_k100_d8": (3, (5, 7), 100, 8, None),
    "m105_k1000_d24": (105, (), 1000, 24, None),
    "mnist_2x8x8_k512_d64": (2, (8, 8), 512, 64, None),
    "m96_k4096_d256": (96, (), 4096, 256, "many"),
    "ldct_1x32x32_k16384_d256": (1, (32, 32), 16384, 256, "many"),
    "m200_k100_d256": (200, (), 100, 256, "one"),
}
_refs = {}


def _rows(N, sp):
    M = N
    for v in sp:
        M *= v
    return M


def _case(name, dist):
    """Device inputs and the fp64 reference of one run, computed once and shared (never modified)."""
    if (name, dist) not in _refs:
        N, sp, K, D, _ = CASES[name]
        z, e, j = vb.make_inputs(_rows(N, sp), K, D, dist)
        z, e = z.to(DEV), e.to(DEV)
        _refs[name, dist] = (z, e, None if j is None else j.to(DEV), vb.reference(z, e))
    return _refs[name, dist]


def _sentinel(shape, dtype, fill):
    """(view of the payload, whole buffer): the payload sits between two GUARD-element guards."""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(shape), buf


def _guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def _run(z, e, N, sp, D, beta, classic, eps=1e-5):
    """ops.vq_quantize into sentinel buffers; z [M, D] is widened to a NaN-padded row stride first."""
    from fmdiff.runtime import ops
    ldz = -(-D // 8) * 8 + 8
    zf = torch.full((N, *sp, ldz), float("nan"), device=DEV)
    zf[..., :D] = z.view(N, *sp, D)
    Cpad = max(8, -(-D // 8) * 8)
    K = e.shape[0]
    nan = float("nan")
    out, bufs = {}, {}
    for key, shape, dtype, fill in (("zq", (N, D, *sp), torch.float32, nan), ("zq_nhwc", (N, *sp, Cpad), torch.bfloat16, nan),
                                    ("codes", (N, *sp), torch.int64, -7), ("hist", (K,), torch.int32, 12345),
                                    ("stats", (3,), torch.float32, nan)):
        out[key], buf = _sentinel(shape, dtype, fill)
        bufs[key] = (buf, fill)
    out["hist"].zero_()
    plans = []
    q = ops.vq_quantize(zf, D, e, beta, classic, plans, eps=eps, Cpad=Cpad, out=out)
    torch.cuda.synchronize()
    for key, (buf, fill) in bufs.items():
        assert _guards_intact(buf, fill), f"{key}: guard overwritten"
    return q, plans[0], zf


def _check_outputs(q, z, e, N, sp, D, beta, classic, name, eps=1e-5):
    """Everything but the near-minimiser assertion, on the kernel's own codes."""
    codes = q.codes
    K = e.shape[0]
    assert codes.shape == (N, *sp) and int(codes.min()) >= 0 and int(codes.max()) < K, name
    zc = z.view(N, *sp, D).movedim(-1, 1).contiguous()
    qc = e[codes.reshape(-1)].view(N, *sp, D).movedim(-1, 1).contiguous()
    want = zc + (qc - zc)
    assert torch.equal(q.zq, want), f"{name}: z_q differs from z + (E[codes] - z) in {int((q.zq != want).sum())} elements"
    nh = want.movedim(1, -1).to(torch.bfloat16)
    assert torch.equal(q.zq_nhwc[..., :D].view(torch.int16), nh.contiguous().view(torch.int16)), f"{name}: NHWC bf16 z_q"
    assert bool((q.zq_nhwc[..., D:].view(torch.int16) == 0).all()), f"{name}: padding channels"
    assert torch.equal(q.hist.long(), torch.bincount(codes.reshape(-1), minlength=K)), f"{name}: histogram"
    loss64, perp64 = vb.stats64(z, e, codes, beta, classic, eps)
    loss, perp = float(q.vq_loss), float(q.perplexity)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), f"{name}: vq_loss {loss!r} vs fp64 {loss64!r}"
    assert abs(perp - perp64) <= 1e-5 * abs(perp64), f"{name}: perplexity {perp!r} vs fp64 {perp64!r}"
    assert q.vq_loss.device.type == "cuda" and q.vq_loss.dim() == 0 and q.perplexity.dim() == 0
    return loss, perp


@pytest.mark.parametrize("dist", vb.DISTRIBUTIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_vq_quantize_against_fp64(name, dist):
    N, sp, K, D, splits = CASES[name]
    z, e, j, ref = _case(name, dist)
    q, plan, _ = _run(z, e, N, sp, D, 0.25, False)
    assert (plan.splits, plan.codes_per_split, plan.Kpad, plan.Dpad) == tuple(
        vb.plan(_rows(N, sp), K, D)[k] for k in ("splits", "codes_per_split", "Kpad", "Dpad"))
    if splits == "one":
        assert plan.splits == 1
    if splits == "many":
        assert plan.splits > 1
    r = vb.check(q.codes, ref, f"{name} {dist}")
    if j is not None:
        assert torch.equal(q.codes.reshape(-1), j), f"{name}: clustered rows must return their own code"
    loss, perp = _check_outputs(q, z, e, N, sp, D, 0.25, False, f"{name} {dist}")
    q2, _, _ = _run(z, e, N, sp, D, 0.4, True)
    assert torch.equal(q2.codes, q.codes)
    loss2, _ = _check_outputs(q2, z, e, N, sp, D, 0.4, True, f"{name} {dist} classic")
    print(f"{name} {dist}: splits {plan.splits} err/bound {r['ratio']:.3f} undecided {r['undecided']:.4f} "
          f"agree-with-fp64 {r['agree']:.4f} vq_loss {loss:.6g} / {loss2:.6g} perplexity {perp:.6g}")


def test_ties_return_the_lower_index_and_zero_row_the_smallest_norm():
    z, e, expect = vb.make_tie_inputs()
    M, K, D = vb.TIE_SHAPE
    z, e, expect = z.to(DEV), e.to(DEV), expect.to(DEV)
    q, plan, _ = _run(z, e, M, (), D, 0.25, False)
    assert plan.splits > 1 and plan.codes_per_split == 2 * vb.CHUNK
    rows = expect >= 0
    assert torch.equal(q.codes[rows], expect[rows]), (q.codes[rows].tolist(), expect[rows].tolist())
    _check_outputs(q, z, e, M, (), D, 0.25, False, "ties")
    # ragged codebooks: the padded codes of the last chunk must not win the all-zero row
    for Kr in (100, 1000):
        e2 = e[:Kr].clone()
        e2[7] = 0.05 * e2[7]
        z0 = torch.zeros(4, D, device=DEV)
        q0, _, _ = _run(z0, e2, 4, (), D, 0.25, False)
        assert bool((q0.codes == 7).all()), q0.codes.tolist()


def test_codebook_planes_follow_the_codebook_value():
    """The cached planes are rebuilt when the codebook is written in place (its _version moves)."""
    from fmdiff.runtime import ops
    z, e, j, ref = _case("mnist_2x8x8_k512_d64", "clustered")
    e = e.clone()
    zf = z.view(2, 8, 8, 64).contiguous()
    a = ops.vq_quantize(zf, 64, e, 0.25, False)
    assert torch.equal(a.codes.reshape(-1), j)
    assert ops.vq_codebook_planes(e)[0] is ops.vq_codebook_planes(e)[0]
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(5)).to(DEV)
    e.copy_(e[perm])                                   # code perm[i] moves to row i
    b = ops.vq_quantize(zf, 64, e, 0.25, False)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(512, device=DEV)
    assert torch.equal(b.codes.reshape(-1), inv[j])


def test_refusals():
    from fmdiff.nn.modules.vae import VectorQuantizerEMA
    from fmdiff.runtime import ops
    with pytest.raises(NotImplementedError):
        ops.vq_quantize(torch.zeros(4, 264, device=DEV), 264, torch.zeros(16, 264, device=DEV), 0.25, False)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.vq_quantize(torch.zeros(4, 8), 8, torch.zeros(16, 8, device=DEV), 0.25, False)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.vq_quantize(torch.zeros(4, 8, device=DEV), 8, torch.zeros(16, 8), 0.25, False)
    ema = VectorQuantizerEMA(16, 8).to(DEV)
    with pytest.raises(NotImplementedError, match="EMA codebook update"):
        ema(torch.zeros(1, 8, 4, 4, device=DEV))
    zq, loss, perp, codes = ema.eval()(torch.zeros(1, 8, 4, 4, device=DEV))
    assert zq.shape == (1, 8, 4, 4) and codes.shape == (1, 4, 4) and not zq.requires_grad


# ------------------------------------------------------------------ model level, on the reference fixture
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("qt", ["ema", "classic"])
def test_vqvae_vs_reference_fixture(qt):
    G, cfg = vb.load_fixture()
    m, _ = vb.build_fixture_model(G, cfg, qt)
    m = m.to(DEV).eval()
    x = G["x"].to(DEV)
    emb = G[f"{qt}.codebook.embedding"].to(DEV)
    classic, beta, eps = qt == "classic", cfg["vq_beta"], cfg["vq_ema_eps"]
    with torch.no_grad():
        quant_in = m.encode(m.image_to_model_range(x))
        errs = dict(encode=_rel(quant_in, G["quant_in"]), decode=_rel(m.decode(G["z"].to(DEV)), G["rec_z"]),
                    decode_zq=_rel(m.decode(G[f"{qt}.z_q"].to(DEV)), G[f"{qt}.rec"]))
        assert all(v < 2e-2 for v in errs.values()), errs
        assert _rel(m.encode(m.image_to_model_range(x), normalize=True), G["quant_in"] * 0.18215) < 2e-2

        # the quantizer on the reference's own input: the kernel-level assertions, and the reference's codes
        qin_ref = G["quant_in"].to(DEV)
        z_q, loss, perp, codes = m.codebook(qin_ref)
        flat = qin_ref.movedim(1, -1).reshape(-1, cfg["embed_dim"])
        ref = vb.reference(flat, emb)
        r = vb.check(codes, ref, f"fixture {qt}")
        decided = (ref["gap"] > 2.0 * vb.row_bound(ref)).view(codes.shape)
        assert torch.equal(codes[decided], G[f"{qt}.codes"].to(DEV)[decided]) and float(decided.double().mean()) >= 0.97
        want = qin_ref + (emb[codes.reshape(-1)].view(2, 8, 8, -1).movedim(-1, 1) - qin_ref)
        assert torch.equal(z_q, want) and not z_q.requires_grad
        loss64, perp64 = vb.stats64(flat, emb, codes, beta, classic, eps)
        assert abs(float(loss) - loss64) <= 1e-5 * loss64 and abs(float(perp) - perp64) <= 1e-5 * perp64
        if bool(decided.all()):
            assert float((z_q.cpu() - G[f"{qt}.z_q"]).abs().max()) == 0.0
            assert abs(float(loss) - float(G[f"{qt}.vq_loss"])) <= 1e-5 * float(G[f"{qt}.vq_loss"])
            assert abs(float(perp) - float(G[f"{qt}.perplexity"])) <= 1e-5 * float(G[f"{qt}.perplexity"])

        # forward = decode(codebook(encode(x))[0]), without the channels-first round trip
        rec, aux = m(m.image_to_model_range(x))
        z_q2, loss2, perp2, codes2 = m.codebook(quant_in)
        assert torch.equal(rec, m.decode(z_q2))
        assert torch.equal(aux["codes"], codes2) and float(aux["vq_loss"]) == float(loss2)
        assert float(aux["perplexity"]) == float(perp2)
        share = float((aux["codes"].cpu() == G[f"{qt}.codes"]).double().mean())
    print(f"VQVAE[{qt}] vs reference: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items())
          + f"; quantizer on the reference input: err/bound {r['ratio']:.3f}, undecided {r['undecided']:.4f}; "
          f"forward: rec rel L2 {_rel(rec, G[f'{qt}.rec']):.3e}, codes agreeing with the reference's {share:.4f} "
          "(printed, not asserted: the bf16 trunk moves near-tie rows)")


@pytest.mark.parametrize("which", ["ldct", "mnist"])
def test_factory_built_config_models_run_forward(which, tmp_path):
    import json

    from fmdiff.models.generators import VAEFactory
    model = vb.LDCT_VQ if which == "ldct" else vb.MNIST_VQ
    p = tmp_path / f"{which}.json"
    p.write_text(json.dumps({"training": {}, "model": model}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAEFactory().build_from_json(p).to(DEV).eval()
    res = model["resolution"]
    x = torch.rand(1, 1, res, res, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        rec, aux = m(m.image_to_model_range(x))
    lat = res // 2 ** (len(model["down_channels"]) - 1)
    assert rec.shape == (1, 1, res, res) and bool(torch.isfinite(rec).all())
    assert aux["codes"].shape == (1, lat, lat) and aux["codes"].dtype == torch.int64
    assert 0 <= int(aux["codes"].min()) and int(aux["codes"].max()) < model["codebook_size"]
    assert float(aux["vq_loss"]) > 0 and 1.0 <= float(aux["perplexity"]) <= lat * lat + 1e-3
