"""The MFMA softmax attention (csrc/attention_mfma.hip) against an fp64 reference with per-tensor, per-element
error bounds (attn_bounds.py; test_attention_bounds.py shows on the CPU that the bounds hold for the documented
arithmetic and reject wrong kernels), every kernel instance, flat / peaked / offset logits; fmd_attn_pack /
fmd_attn_unpack bit exact against the torch index maps; fmd_context_norm_fwd / _bwd against fp64 F.group_norm.

Inputs come from generators seeded per (case, distribution); the fp64 reference runs on the device."""
import zlib

import pytest
import torch
import torch.nn.functional as F

import attn_bounds as ab

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("O", "lse", "dQ", "dK", "dV")


def ops():
    from fmdiff.runtime import ops as O
    return O


def _inst(dhp, ks_fwd, ks_dq, ks_kv, key_blocks):
    return dict(dhp=dhp, ks_fwd=ks_fwd, ks_dq=ks_dq, ks_kv=ks_kv, key_blocks=key_blocks)


# (B, T, heads, dh, raw) -> the instance it must reach: head padding, key splits of the forward and of dQ, query
# splits of dK/dV, staged key blocks (of 32 * ks_fwd keys) of the forward
SELF_CASES = []
for _T in (17, 32):                                   # one split, one block; both head splits at every DHP
    for _dh, _D in ((12, 16), (24, 32), (64, 64)):
        for _raw in (0, 1):
            SELF_CASES.append(((2, _T, 2, _dh, _raw), _inst(_D, 1, 1, 1, 1)))
SELF_CASES += [
    # two splits: T = 33 is one staged block in which split 1 owns a single key; T = 100 is two blocks, the
    # second with 32 + 4 keys
    ((2, 33, 3, 12, 0), _inst(16, 2, 2, 2, 1)), ((2, 33, 3, 24, 1), _inst(32, 2, 2, 2, 1)),
    ((2, 33, 3, 40, 0), _inst(64, 2, 2, 2, 1)), ((2, 100, 3, 12, 1), _inst(16, 2, 2, 2, 2)),
    ((2, 100, 3, 24, 0), _inst(32, 2, 2, 2, 2)), ((2, 100, 3, 40, 1), _inst(64, 2, 2, 2, 2)),
    # four splits (dQ: two at DHP 64); T = 129: three of the four splits idle in the last block
    ((2, 129, 2, 12, 0), _inst(16, 4, 4, 2, 2)), ((2, 129, 2, 32, 1), _inst(32, 4, 4, 2, 2)),
    ((2, 129, 2, 64, 0), _inst(64, 4, 2, 2, 2)), ((2, 300, 2, 12, 1), _inst(16, 4, 4, 2, 3)),
    ((2, 300, 2, 32, 0), _inst(32, 4, 4, 2, 3)), ((2, 300, 2, 64, 1), _inst(64, 4, 2, 2, 3)),
    # two splits over several staged blocks: needs >= 512 workgroups (what large batches run).  T = 200: the last
    # block has 8 keys and split 1 idles; T = 129: it has one
    ((4, 200, 64, 16, 1), _inst(16, 2, 2, 2, 4)), ((4, 200, 64, 32, 0), _inst(32, 2, 2, 2, 4)),
    ((4, 129, 64, 64, 0), _inst(64, 2, 2, 2, 3)),
]

# (B, Tq, Tk, heads, dh, raw)
CROSS_CASES = []
for _raw in (1, 0):
    CROSS_CASES += [
        ((2, 20, 200, 2, 32, _raw), _inst(32, 4, 4, 1, 2)),   # dK/dV with one query split at DHP 32 ...
        ((2, 20, 200, 2, 64, _raw), _inst(64, 4, 2, 1, 2)),   # ... and 64
        ((2, 300, 5, 3, 48, _raw), _inst(64, 1, 1, 2, 1)),    # forward / dQ with one split over three query blocks
        ((2, 70, 33, 2, 12, _raw), _inst(16, 2, 2, 2, 1)),
    ]
CROSS_CASES.append(((2, 64, 128, 4, 64, 1), _inst(64, 2, 2, 2, 2)))   # tile-transpose pack of both sets


def _ids(cases):
    return ["-".join(map(str, c[0])) for c in cases]


def _verify(tag, dist, got, q, k, v, do, dh):
    scale = dh ** -0.5
    dev = [t.to(DEV) for t in (q, k, v, do)]
    ref = ab.reference(*dev, scale)
    bnd = ab.bounds(ref, *dev, scale)
    ratios = ab.check_all(got, ref, bnd, f"{tag} {dist}")
    print(f"ATTN_RATIO {tag} {dist} " + " ".join(f"{n}={ratios[n]:.3f}" for n in NAMES))


@pytest.mark.parametrize("dist", ab.DISTRIBUTIONS)
@pytest.mark.parametrize("case,inst", SELF_CASES, ids=_ids(SELF_CASES))
def test_self_attention_bounds(case, inst, dist):
    O = ops()
    B, T, heads, dh, raw = case
    BH = B * heads
    assert ab.instance(BH, T, T, dh) == inst
    q, k, v, do = ab.make_inputs(f"self {case}", dist, BH, T, T, dh)
    qkv = ab.join_heads([q, k, v], B, heads, dh, raw).to(DEV)
    dout = ab.join_heads([do], B, heads, dh, raw).to(DEV)
    o, saved = O.attention_fwd(qkv, T, heads, dh, raw)
    assert isinstance(saved, O.AttnSaved) and saved.lse.shape == (B, heads, T)
    dqkv = O.attention_bwd(qkv, o, dout, saved, T, heads, dh, raw)
    dqkv2 = O.attention_bwd(qkv, o, dout, saved.lse, T, heads, dh, raw)   # q, k, v, o packed again
    assert torch.equal(dqkv, dqkv2)
    dq, dk, dv = ab.split_heads(dqkv, heads, dh, raw, 3)
    got = dict(O=ab.split_heads(o, heads, dh, raw, 1)[0], lse=saved.lse.reshape(BH, T), dQ=dq, dK=dk, dV=dv)
    _verify(f"self {case}", dist, got, q, k, v, do, dh)


@pytest.mark.parametrize("dist", ab.DISTRIBUTIONS)
@pytest.mark.parametrize("case,inst", CROSS_CASES, ids=_ids(CROSS_CASES))
def test_cross_attention_bounds(case, inst, dist):
    O = ops()
    B, Tq, Tk, heads, dh, raw = case
    BH = B * heads
    assert ab.instance(BH, Tq, Tk, dh) == inst
    q, k, v, do = ab.make_inputs(f"cross {case}", dist, BH, Tq, Tk, dh)
    qt = ab.join_heads([q], B, heads, dh, raw).to(DEV)
    kvt = ab.join_heads([k, v], B, heads, dh, raw).to(DEV)
    dout = ab.join_heads([do], B, heads, dh, raw).to(DEV)
    o, saved = O.cross_attention_fwd(qt, kvt, Tq, Tk, heads, dh, None, raw)
    assert isinstance(saved, O.AttnSaved) and saved.lse.shape == (B, heads, Tq)
    dq, dkv = O.cross_attention_bwd(qt, kvt, o, dout, saved, Tq, Tk, heads, dh, None, raw)
    dq2, dkv2 = O.cross_attention_bwd(qt, kvt, o, dout, saved.lse, Tq, Tk, heads, dh, None, raw)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    dk, dv = ab.split_heads(dkv, heads, dh, raw, 2)
    got = dict(O=ab.split_heads(o, heads, dh, raw, 1)[0], lse=saved.lse.reshape(BH, Tq),
               dQ=ab.split_heads(dq, heads, dh, raw, 1)[0], dK=dk, dV=dv)
    _verify(f"cross {case}", dist, got, q, k, v, do, dh)


@pytest.mark.parametrize("dh,raw", [(16, 0), (32, 1), (64, 0)])
def test_p_rounding_is_unbiased(dh, raw):
    """The signed errors of O and dV sum to zero within 6 sigma of zero-mean rounding (attn_bounds.check_unbiased:
    flat logits, v, dO > 0, 2048 rows).  P truncated instead of rounded passes check() at any shape and lands at
    -1.8 x this limit (test_attention_bounds.py::test_truncated_p_is_biased)."""
    O = ops()
    B, T, heads = 2, 128, 8
    BH = B * heads
    assert ab.instance(BH, T, T, dh) == _inst(dh, 2, 2, 2, 2)
    q, k, v, do = ab.make_inputs(f"unbiased {dh}", "flat", BH, T, T, dh, positive=True)
    qkv = ab.join_heads([q, k, v], B, heads, dh, raw).to(DEV)
    dout = ab.join_heads([do], B, heads, dh, raw).to(DEV)
    o, saved = O.attention_fwd(qkv, T, heads, dh, raw)
    dq, dk, dv = ab.split_heads(O.attention_bwd(qkv, o, dout, saved, T, heads, dh, raw), heads, dh, raw, 3)
    got = dict(O=ab.split_heads(o, heads, dh, raw, 1)[0], lse=saved.lse.reshape(BH, T), dQ=dq, dK=dk, dV=dv)
    dev = [t.to(DEV) for t in (q, k, v, do)]
    ref = ab.reference(*dev, dh ** -0.5)
    bnd = ab.bounds(ref, *dev, dh ** -0.5)
    ab.check_all(got, ref, bnd, f"unbiased {dh}")
    r = {n: ab.check_unbiased(got[n], ref[n], bnd[n], f"unbiased {dh} {n}") for n in ("O", "dV")}
    print(f"ATTN_BIAS dh={dh} O={r['O']:.3f} dV={r['dV']:.3f}")


# ------------------------------------------------------------------ pack / unpack: pure data movement, bit exact
NAN_BITS, SENTINEL_BITS = 0x7FC0, 0x7FC1   # two bf16 NaN patterns no randn value has


def _bits(t):
    return t.contiguous().view(torch.int16)


def _filled(shape, bits):
    t = torch.empty(shape, device=DEV, dtype=torch.bfloat16)
    _bits(t).fill_(bits)
    return t


def _unpack(O, cq, ck, cv, B, Tq, Tk, heads, dh, raw, cross, w0, w1, dst_q, dst_kv):
    from fmdiff import _lib
    _lib.call("fmd_attn_unpack", O._p(cq), O._p(ck), O._p(cv), B, Tq, Tk, heads, dh, int(raw), int(cross), w0, w1,
              O._p(dst_q), O._p(dst_kv), O.stream())


def _check_planes(planes, want, dh):
    for pl, w in zip(planes, want):
        assert torch.equal(_bits(pl[..., :dh]), _bits(w)), "data columns differ from the index map"
        assert not _bits(pl[..., dh:]).any(), "padding columns [dh, DHP) are not zero"


# (path, raw, Tq, Tk, heads, dh): Tk is used by the cross variant only
PACK_CASES = [
    ("tile", 1, 64, 128, 4, 16), ("tile", 1, 128, 64, 2, 32), ("tile", 1, 64, 192, 1, 64),   # raw, 64 x 64 tiles
    ("run", 1, 100, 37, 3, 24), ("run", 1, 64, 64, 2, 16),              # raw, run walk (ragged T; inner = 32)
    ("vec", 0, 50, 23, 3, 8), ("vec", 0, 33, 70, 2, 40), ("vec", 0, 17, 5, 2, 64),   # view, 16-byte loads
    ("scalar", 0, 45, 31, 3, 12),                                       # view, element walk
]


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("path,raw,Tq,Tk,heads,dh", PACK_CASES)
def test_pack_unpack_bit_exact(path, raw, Tq, Tk, heads, dh, cross):
    O = ops()
    B = 3
    inner = heads * dh
    if not cross:
        Tk = Tq
    D = ab.dhp_of(dh)
    # raw_sets() of attention_mfma.hip: the tile transpose needs dh = DHP, whole 64-token and 64-channel tiles
    sets = [(1, Tq), (2, Tk)] if cross else [(3, Tq)]
    for group in (sets, [(1, Tq)]):
        tile = bool(raw) and dh == D and all(T % 64 == 0 and (P * inner) % 64 == 0 for P, T in group)
        assert tile == (path == "tile")
    g = torch.Generator().manual_seed(zlib.crc32(f"pack {raw} {Tq} {Tk} {heads} {dh} {cross}".encode()))
    if cross:
        srcs = [torch.randn(B, Tq, inner, generator=g), torch.randn(B, Tk, 2 * inner, generator=g)]
    else:
        srcs = [torch.randn(B, Tq, 3 * inner, generator=g)]
    srcs = [s.to(torch.bfloat16).to(DEV) for s in srcs]
    src_q, src_kv = srcs[0], srcs[-1]
    if cross:
        want = ab.split_heads(src_q, heads, dh, raw, 1) + ab.split_heads(src_kv, heads, dh, raw, 2)
    else:
        want = ab.split_heads(src_q, heads, dh, raw, 3)
    # planes 0..2 (q, k, v) as the forward packs them
    cq, ck, cv = (_filled((B * heads, T, D), NAN_BITS) for T in (Tq, Tk, Tk))
    O._attn_pack(src_q, src_kv, B, Tq, Tk, heads, dh, raw, cross, 0, 2, cq, ck, cv)
    _check_planes((cq, ck, cv), want, dh)
    dsts = [_filled(s.shape, SENTINEL_BITS) for s in srcs]
    _unpack(O, cq, ck, cv, B, Tq, Tk, heads, dh, raw, cross, 0, 2, dsts[0], dsts[-1])
    for d, s in zip(dsts, srcs):
        assert not (_bits(d) == SENTINEL_BITS).any(), "unpack left destination elements unwritten"
        assert torch.equal(_bits(d), _bits(s))
    # plane 3 (o / dO: [B][Tq][inner]) as the forward unpacks and the backward packs it
    o = torch.randn(B, Tq, inner, generator=g).to(torch.bfloat16).to(DEV)
    co = _filled((B * heads, Tq, D), NAN_BITS)
    O._attn_pack(o, o, B, Tq, Tk, heads, dh, raw, cross, 3, 3, co)
    _check_planes((co,), ab.split_heads(o, heads, dh, raw, 1), dh)
    od = _filled(o.shape, SENTINEL_BITS)
    _unpack(O, co, None, None, B, Tq, Tk, heads, dh, raw, cross, 3, 3, od, None)
    assert not (_bits(od) == SENTINEL_BITS).any(), "unpack left destination elements unwritten"
    assert torch.equal(_bits(od), _bits(o))


# ------------------------------------------------------------------ context_norm
@pytest.mark.parametrize("tok_major", [0, 1])
@pytest.mark.parametrize("C,groups,Cpads", [(4, 1, (8, 32)), (4, 2, (8, 32)), (24, 8, (32,))])
def test_context_norm_vs_fp64(C, groups, Cpads, tok_major):
    """fmd_context_norm_fwd / _bwd vs fp64 F.group_norm: the bf16 output within one rounding (u |ref|) plus the
    fp32 evaluation (1e-5 max|ref|), pad channels exactly zero, (mean, rstd) within 1e-5 relative; the dgamma /
    dbeta increments on top of non-zero accumulators within 1e-5 ||t||_1 of their summands t (fp32 summation,
    the rule of test_halo_conv_matches_generic)."""
    O = ops()
    N, eps = 3, 1e-5
    for T in (1, 77, 300):
        for Cpad in Cpads:
            g = torch.Generator().manual_seed(zlib.crc32(f"ctxnorm {C} {groups} {T} {Cpad} {tok_major}".encode()))
            x = torch.randn(N, C, T, generator=g) * 1.5 + 0.7                     # channel-major values
            gamma = torch.rand(C, generator=g) + 0.5
            beta = torch.randn(C, generator=g) * 0.3
            ctx = (x.transpose(1, 2).contiguous() if tok_major else x).to(DEV)
            out, mr = O.context_norm_fwd(ctx, tok_major, groups, eps, gamma.to(DEV), beta.to(DEV), Cpad)
            assert out.shape == (N, T, 1, Cpad) and mr.shape == (N, groups, 2)
            x64 = x.double().to(DEV)
            ref = F.group_norm(x64, groups, gamma.double().to(DEV), beta.double().to(DEV), eps).transpose(1, 2)
            got = out.reshape(N, T, Cpad)
            err = (got[..., :C].double() - ref).abs()
            lim = ab.U * ref.abs() + 1e-5 * ref.abs().max()
            assert bool((err <= lim).all()), f"T={T} Cpad={Cpad}: worst err/limit {(err / lim).max().item():.3f}"
            assert not _bits(got[..., C:]).any(), "pad channels are not zero"
            xg = x64.reshape(N, groups, -1)
            mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
            mr_ref = torch.stack([mean, (var + eps).rsqrt()], -1)
            assert bool(((mr.double() - mr_ref).abs() <= 1e-5 * mr_ref.abs()).all()), f"T={T}: mean / rstd"
            # backward: dgamma[c] += sum_{n,t} dY xhat, dbeta[c] += sum_{n,t} dY
            dy = torch.randn(N, T, 1, Cpad, generator=g).to(torch.bfloat16).to(DEV)
            acc0 = torch.randn(2, C, generator=g).to(DEV)
            dgamma, dbeta = acc0[0].clone(), acc0[1].clone()
            O.context_norm_bwd(ctx, tok_major, groups, mr, dy, dgamma, dbeta)
            xhat = ((xg - mean[..., None]) * mr_ref[..., 1:]).reshape(N, C, T).transpose(1, 2)   # [N][T][C]
            d64 = dy.reshape(N, T, Cpad)[..., :C].double()
            for name, after, before, t in (("dgamma", dgamma, acc0[0], d64 * xhat), ("dbeta", dbeta, acc0[1], d64)):
                inc = after.double() - before.double()
                e = (inc - t.sum((0, 1))).abs()
                lim = 1e-5 * t.abs().sum((0, 1))
                assert bool((e <= lim).all()), f"T={T} Cpad={Cpad} {name}: worst err/limit {(e / lim).max().item():.3f}"
