"""GPU tests of the quantizer's training kernels (csrc/vq_train.hip) through ops.vq_ema_update / vq_backward /
vq_codebook_grad and the modules' quantize_train.

Kernel level: every shape of test_gpu_vq.CASES, 1024 rows that all choose one code, and a state with zero cluster
sizes, against the fp64 restatement of vq_train_bounds.py on the kernel's own codes, within the derived
per-element bounds; rows NaN-padded, every output and buffer between sentinel guards.  Then determinism, the
reference's recorded trajectory and gradients (teacher-forced), the plane cache, graph capture and the modes
that must not update.  Every case prints its observed error / bound.
"""
import pytest
import torch

import test_gpu_vq as tg
import vq_bounds as vb
import vq_train_bounds as tb

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETA, DECAY, EPS, G_LOSS = 0.25, 0.99, 1e-5, 0.7

# name -> (N, spatial, K, D, sizes, one_code)
CASES = {k: (v[0], v[1], v[2], v[3], "rand", False) for k, v in tg.CASES.items()}
CASES["long_segment_m1024_k300_d64"] = (1024, (), 300, 64, "rand", True)
CASES["dead_codes_m128_k512_d64"] = (2, (8, 8), 512, 64, "dead", False)
_inputs = {}


def _case(name):
    """Device inputs of one case, made once and never modified: (z [M, D], state, g_zq [M, D])."""
    if name not in _inputs:
        N, sp, K, D, sizes, one = CASES[name]
        M = tg._rows(N, sp)
        emb, cs, w = tb.make_state(K, D, name, sizes)
        g = vb.gen(f"vq_train_gpu/{name}")
        z = torch.randn(M, D, generator=g)
        if one:
            z = emb[5] + 0.01 * z
        _inputs[name] = tuple(t.to(DEV) for t in (z, emb, cs, w, torch.randn(M, D, generator=g)))
    return _inputs[name]


def _padded(x, N, sp, D, extra):
    ld = -(-D // 8) * 8 + extra
    out = torch.full((N, *sp, ld), float("nan"), device=DEV)
    out[..., :D] = x.view(N, *sp, D)
    return out


def _step(name):
    """quantize + residual + backward (both forms) + codebook gradient + EMA update, everything in sentinels."""
    from fmdiff.runtime import ops
    N, sp, K, D, sizes, one = CASES[name]
    z, emb, cs, w, g = _case(name)
    nan = float("nan")
    state, bufs = {}, {}
    for key, src in (("e", emb), ("cs", cs), ("w", w)):
        state[key], buf = tg._sentinel(tuple(src.shape), torch.float32, nan)
        state[key].copy_(src)
        bufs[key] = (buf, nan)
    q, _, zf = tg._run(z, state["e"], N, sp, D, BETA, False, eps=EPS)
    codes = q.codes.reshape(-1)
    gf = _padded(g, N, sp, D, 16)
    gl = torch.tensor([G_LOSS], device=DEV)
    dz, buf = tg._sentinel(tuple(zf.shape), torch.float32, nan)
    bufs["dz"] = (buf, nan)
    dE, buf = tg._sentinel((K, D), torch.float32, nan)
    bufs["dE"] = (buf, nan)
    ops.vq_backward(zf, D, q.codes, state["e"], gf, gl, BETA - 1.0, out=dz)
    dz_ema = ops.vq_backward(ops.vq_residual(zf, D, q.codes, state["e"]), D, None, None, gf, gl, BETA)
    dz_nog = ops.vq_backward(zf, D, q.codes, state["e"], None, gl, BETA)
    dE.copy_(ops.vq_codebook_grad(zf, D, q.codes, q.hist, state["e"], gl))
    planes = ops.vq_codebook_planes(state["e"])
    ver = state["e"]._version
    nsum = ops.vq_ema_update(zf, D, q.codes, q.hist, state["e"], state["cs"], state["w"], DECAY, EPS)
    torch.cuda.synchronize()
    for key, (buf, fill) in bufs.items():
        assert tg._guards_intact(buf, fill), f"{name}: {key}: guard overwritten"
    return dict(codes=codes, q=q, zf=zf, e=state["e"], cs=state["cs"], w=state["w"], n=nsum, dz=dz, dz_ema=dz_ema,
                dz_nog=dz_nog, dE=dE, planes=planes, ver=ver)


@pytest.mark.parametrize("name", list(CASES))
def test_training_kernels_against_fp64(name):
    from fmdiff.runtime import ops
    N, sp, K, D, sizes, one = CASES[name]
    z, emb, cs, w, g = _case(name)
    M = z.shape[0]
    o = _step(name)
    codes = o["codes"]
    assert int(codes.min()) >= 0 and int(codes.max()) < K
    if one:
        assert bool((codes == 5).all())
    r = tb.update64(z, codes, cs, w, DECAY, EPS)
    ratios = tb.check_update(name, dict(cs=o["cs"], w=o["w"], e=o["e"], n=o["n"][0]), r, tb.update_bounds(r, cs, w, DECAY, EPS))
    # the cached planes were rewritten in place for the new embedding, bit for bit what fmd_vq_prep makes of it
    assert o["e"]._version > o["ver"]
    planes = ops.vq_codebook_planes(o["e"])
    assert all(a is b for a, b in zip(planes, o["planes"])), f"{name}: the plane cache entry was dropped"
    if sizes != "dead":   # a dead code's row is about 1e5 times ema_w and may overflow hn; the update is what counts
        fresh = ops.vq_codebook_planes(o["e"].clone())
        for a, b, what in zip(planes, fresh, ("Eh", "El", "hn")):
            assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                               b.view(torch.int16) if b.dtype == torch.bfloat16 else b), f"{name}: {what}"
        q = emb[codes]
        for key, c, gz in (("dz", BETA - 1.0, g), ("dz_ema", BETA, g), ("dz_nog", BETA, None)):
            got = o[key].view(M, -1)
            assert bool((got[:, D:] == 0).all()), f"{name}: {key}: padding channels"
            coef = abs(G_LOSS * c * 2.0 / (M * D))
            ratios[key] = tb.check(name, got[:, :D], tb.dz64(z, q, gz, G_LOSS, c), tb.dz_bound(z, q, gz, coef), key)
        dE64, bE = tb.codebook_grad64(z, codes, emb, G_LOSS)
        ratios["dE"] = tb.check(name, o["dE"], dE64, bE, "dE")
    print(f"{name}: unused codes {int((r['n_k'] == 0).sum())} of {K}, longest segment {int(r['n_k'].max())}, "
          f"error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("name", ["ldct_1x32x32_k16384_d256", "m200_k100_d256", "long_segment_m1024_k300_d64"])
def test_same_inputs_same_bits(name):
    a, b = _step(name), _step(name)
    for key in ("codes", "e", "cs", "w", "n", "dz", "dz_ema", "dz_nog", "dE"):
        assert torch.equal(a[key], b[key]), f"{name}: {key} differs between two runs"
    for x, y in zip(a["planes"], b["planes"]):
        assert torch.equal(x.float(), y.float())


# ------------------------------------------------------------------ the reference's recorded trajectory
def _load_state(m, G, tag, s):
    emb, cs, w = tb.fixture_state(G, tag, s)
    with torch.no_grad():
        m.embedding.copy_(emb.to(DEV))
        if hasattr(m, "ema_w"):
            m.ema_cluster_size.copy_(cs.to(DEV))
            m.ema_w.copy_(w.to(DEV))


def _sum_bounds(a, b):
    return {k: a[k] + b[k] for k in a}


@pytest.mark.parametrize("tag", list(tb.FIXTURE_SHAPES))
def test_fixture_teacher_forced(tag):
    from fmdiff.nn.modules.vae import VectorQuantizer, VectorQuantizerEMA
    G, h = tb.load_fixture()
    N, sp, K, D = tb.FIXTURE_SHAPES[tag]
    ema = VectorQuantizerEMA(K, D, h["beta"], decay=h["decay"], eps=h["eps"]).to(DEV).train()
    g_zq = G[f"{tag}.g_zq"].to(DEV)
    out = []
    for s in range(tb.FIXTURE_STEPS):
        _load_state(ema, G, tag, s)
        emb, cs, w = (t.to(DEV) for t in tb.fixture_state(G, tag, s))
        z = G[f"{tag}.z{s}"].to(DEV).requires_grad_(s == 0)
        z_q, vq_loss, perp, codes = ema.quantize_train(z)
        assert torch.equal(codes.cpu(), G[f"{tag}.codes{s}"])            # every row is decided: exact
        assert torch.equal(z_q.detach().cpu(), G[f"{tag}.z_q{s}"])       # the embedding from before the update
        assert abs(float(vq_loss.detach()) - float(G[f"{tag}.vq_loss{s}"])) <= 1e-5 * float(G[f"{tag}.vq_loss{s}"])
        assert abs(float(perp) - float(G[f"{tag}.perplexity{s}"])) <= 1e-5 * float(G[f"{tag}.perplexity{s}"])
        zf = tb.flat(z.detach())
        r = tb.update64(zf, codes.reshape(-1), cs, w, h["decay"], h["eps"])
        b = _sum_bounds(tb.update_bounds(r, cs, w, h["decay"], h["eps"]),
                        tb.update_bounds(r, cs, w, h["decay"], h["eps"], reference=True))
        want = dict(zip(("e", "cs", "w"), (t.to(DEV).double() for t in tb.fixture_state(G, tag, s + 1))))
        got = dict(e=ema.embedding, cs=ema.ema_cluster_size, w=ema.ema_w)
        out.append({k: tb.check(f"{tag} step {s}", got[k], want[k], b[k], k) for k in got})
        if s == 0:
            assert z_q.requires_grad and vq_loss.requires_grad and not codes.requires_grad
            ((z_q * g_zq).sum() + h["g_loss"] * vq_loss).backward()
            q = emb[codes.reshape(-1)]
            mag = h["g_loss"] * h["beta"] * 2.0 / zf.numel()
            bz = tb.dz_bound(zf, q, tb.flat(g_zq), mag) * 2.0            # the kernel's and the reference's, both c = 7
            out[-1]["z.grad"] = tb.check(f"{tag} ema", tb.flat(z.grad), tb.flat(G[f"{tag}.ema.z_grad"]).to(DEV).double(),
                                         bz, "z.grad")
    print(f"fixture {tag} (EMA): error / bound per step: " + "; ".join(
        ", ".join(f"{k} {v:.3f}" for k, v in o.items()) for o in out))

    emb = tb.fixture_state(G, tag, 0)[0].to(DEV)
    for codebook_grad in (False, True):
        cl = VectorQuantizer(K, D, h["beta"]).to(DEV).train()
        _load_state(cl, G, tag, 0)
        z = G[f"{tag}.z0"].to(DEV).requires_grad_()
        z_q, vq_loss, perp, codes = cl.quantize_train(z, codebook_grad=codebook_grad)
        assert torch.equal(codes.cpu(), G[f"{tag}.codes0"]) and torch.equal(z_q.detach().cpu(), G[f"{tag}.z_q0"])
        ((z_q * g_zq).sum() + h["g_loss"] * vq_loss).backward()
        zf, q = tb.flat(z.detach()), emb[codes.reshape(-1)]
        mag_k = h["g_loss"] * (1.0 - h["beta"]) * 2.0 / zf.numel()
        mag_r = h["g_loss"] * (1.0 + h["beta"]) * 2.0 / zf.numel()
        bz = tb.dz_bound(zf, q, tb.flat(g_zq), mag_k) + tb.dz_bound(zf, q, tb.flat(g_zq), mag_r)
        rz = tb.check(f"{tag} classic", tb.flat(z.grad), tb.flat(G[f"{tag}.classic.z_grad"]).to(DEV).double(), bz, "z.grad")
        if not codebook_grad:
            assert cl.embedding.grad is None
            print(f"fixture {tag} (classic): z.grad error / bound {rz:.3f}")
            continue
        # the paper's loss in fp64 autograd: |sg[z] - e|^2 + beta |z - sg[e]|^2, means over M D elements
        e64 = emb.double().requires_grad_()
        q64, z64 = e64[codes.reshape(-1)], zf.double()
        (h["g_loss"] * (((q64 - z64) ** 2).mean() + h["beta"] * ((q64.detach() - z64) ** 2).mean())).backward()
        dE64, bE = tb.codebook_grad64(zf, codes.reshape(-1), emb, h["g_loss"])
        assert float((dE64 - e64.grad).abs().max()) <= 1e-12 * float(e64.grad.abs().max())
        rE = tb.check(f"{tag} classic", cl.embedding.grad, e64.grad, bE, "embedding.grad")
        print(f"fixture {tag} (classic, codebook_grad): z.grad {rz:.3f}, embedding.grad {rE:.3f} of the bound")


# ------------------------------------------------------------------ cache, graph, modes
def _ema_module(G, h, tag="b"):
    from fmdiff.nn.modules.vae import VectorQuantizerEMA
    N, sp, K, D = tb.FIXTURE_SHAPES[tag]
    m = VectorQuantizerEMA(K, D, h["beta"], decay=h["decay"], eps=h["eps"]).to(DEV).train()
    _load_state(m, G, tag, 0)
    return m


def _buffers(m):
    return [getattr(m, k).clone() for k in ("embedding", "ema_cluster_size", "ema_w")]


def test_next_quantize_reads_the_updated_codebook():
    G, h = tb.load_fixture()
    m = _ema_module(G, h)
    z0, z1 = G["b.z0"].to(DEV), G["b.z1"].to(DEV)
    ver = m.embedding._version
    m.quantize_train(z0)
    assert m.embedding._version > ver
    # z1 was drawn around the reference's embedding after step 0: decided rows of the new codebook
    codes = m.eval()(z1)[3]
    ref = vb.reference(tb.flat(z1), m.embedding)
    decided = ref["gap"] > 2.0 * vb.row_bound(ref)
    assert float(decided.double().mean()) >= 0.97
    assert torch.equal(codes.reshape(-1)[decided], ref["idx"][decided])
    assert torch.equal(codes.cpu(), G["b.codes1"])


def test_captured_step_replays_like_eager_steps():
    G, h = tb.load_fixture()
    z = G["b.z0"].to(DEV)
    eager = _ema_module(G, h)
    with torch.no_grad():
        for _ in range(3):
            eager.quantize_train(z)
    m = _ema_module(G, h)
    with torch.no_grad():
        m.quantize_train(z)              # warm-up: constants, allocator, plane buffers
        _load_state(m, G, "b", 0)
        m.eval()(z)                      # planes of the reloaded codebook, made outside the capture
        m.train()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            m.quantize_train(z)
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    for a, b, what in zip(_buffers(m), _buffers(eager), ("embedding", "ema_cluster_size", "ema_w")):
        assert torch.equal(a, b), f"{what}: three replays differ from three eager steps"
    with torch.no_grad():
        a, b = m.eval()(z), eager.eval()(z)
    assert torch.equal(a[3], b[3]) and torch.equal(a[0], b[0]) and float(a[1]) == float(b[1])


def test_modes_that_must_not_update_and_refusals():
    from fmdiff.nn.modules.vae import VectorQuantizer, VectorQuantizerEMA
    from fmdiff.runtime import ops
    G, h = tb.load_fixture()
    z = G["b.z0"].to(DEV)
    m = _ema_module(G, h)
    before = _buffers(m)
    m.eval().quantize_train(z.clone().requires_grad_())[1].backward()
    m.train()
    m.decay = 0.0
    m.quantize_train(z)
    for a, b in zip(_buffers(m), before):
        assert torch.equal(a, b)
    m.decay = h["decay"]
    with pytest.raises(NotImplementedError, match="EMA codebook update"):
        m(z)
    with pytest.raises(ValueError):
        m.quantize_train(z, codebook_grad=True)
    cpu = torch.zeros(4, 8)
    dev = torch.zeros(4, 8, device=DEV)
    codes, hist = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(16, dtype=torch.int32, device=DEV)
    e, cs = torch.zeros(16, 8, device=DEV), torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.vq_ema_update(cpu, 8, codes, hist, e, cs, e.clone(), 0.99, 1e-5)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.vq_ema_update(dev, 8, codes, hist, e.cpu(), cs, e.clone(), 0.99, 1e-5)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ops.vq_backward(cpu, 8, codes, e, None, None, 0.25)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        VectorQuantizer(16, 8).to(DEV).quantize_train(torch.zeros(1, 8, 2, 2))
    with pytest.raises(NotImplementedError):
        ops.vq_train_plan(4, 16, 264)
