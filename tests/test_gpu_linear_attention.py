"""The linear attention kernels (csrc/attention.hip) against an fp64 reference with per-tensor, per-element error
bounds (la_bounds.py; test_la_bounds.py shows on the CPU that the bounds hold for the documented arithmetic and
reject wrong kernels): every chunking la_args can produce (one token, a partial LDS sub-block, 64 / 65 rows, the
1 -> 2 chunk switch, the LA_MAXCH cap, nchq != nchk both ways), both head splits, self and cross, flat / peaked /
offset inputs, eps = 1e-6 and the eps = 0.25 rows where Z, s, ds, cc and eps are live arithmetic; the saved state
(ctx | M | Z | s) against fp64; bitwise repeatability; unbiased bf16 stores; the workspace / state extents.

Inputs come from generators seeded per (case, distribution); the fp64 reference runs on the device."""
import pytest
import torch

import la_bounds as lb

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = lb.LA_D
NAMES = lb.OUTPUTS + lb.STATE


def ops():
    from fmdiff.runtime import ops as O
    return O


def _ids(cases):
    return ["-".join(map(str, c[0])) for c in cases]


def _state_views(state, BH, dh):
    """The live part of the saved state [BH][D*D + 3D] = ctx | M | Z | s, and the padding around it."""
    assert state.numel() == BH * (D * D + 3 * D)
    assert bool(torch.isfinite(state).all()), "NaN / Inf in the saved state"
    st = state.view(BH, D * D + 3 * D)
    ctx = st[:, :D * D].view(BH, D, D)
    M, Z, s = (st[:, D * D + i * D:D * D + (i + 1) * D] for i in range(3))
    assert not ctx[:, dh:].any() and not ctx[:, :, dh:].any() and not Z[:, dh:].any() and not s[:, dh:].any(), \
        "state columns >= dh are not zero"
    return dict(ctx=ctx[:, :dh, :dh], M=M[:, :dh], Z=Z[:, :dh], s=s[:, :dh])


def _forward_backward(kind, case, eps, planes):
    """One forward + backward through fmdiff.runtime.ops; returns (raw tensors, canonical planes)."""
    O = ops()
    q, k, v, do = planes
    if kind == "self":
        B, T, heads, dh, raw = case
        qkv = lb.join_heads([q, k, v], B, heads, dh, raw).to(DEV)
        dout = lb.join_heads([do], B, heads, dh, raw).to(DEV)
        o, state = O.linear_attention_fwd(qkv, T, heads, dh, raw, eps)
        dqkv = O.linear_attention_bwd(qkv, dout, state, T, heads, dh, raw, eps)
        dq, dk, dv = lb.split_heads(dqkv, heads, dh, raw, 3)
        tensors = (o, state, dqkv)
    else:
        B, Tq, Tk, heads, dh, raw = case
        qt = lb.join_heads([q], B, heads, dh, raw).to(DEV)
        kvt = lb.join_heads([k, v], B, heads, dh, raw).to(DEV)
        dout = lb.join_heads([do], B, heads, dh, raw).to(DEV)
        o, state = O.cross_attention_fwd(qt, kvt, Tq, Tk, heads, dh, eps, raw)
        dqt, dkv = O.cross_attention_bwd(qt, kvt, o, dout, state, Tq, Tk, heads, dh, eps, raw)
        dq = lb.split_heads(dqt, heads, dh, raw, 1)[0]
        dk, dv = lb.split_heads(dkv, heads, dh, raw, 2)
        tensors = (o, state, dqt, dkv)
    got = dict(O=lb.split_heads(o, heads, dh, raw, 1)[0], dQ=dq, dK=dk, dV=dv, **_state_views(state, B * heads, dh))
    return tensors, got


def _verify(kind, case, eps, dist, positive=False):
    BH, Tq, Tk, dh = lb.canonical(kind, case)
    tag = lb.row_key(kind, case, eps)
    planes = lb.make_inputs(tag, dist, BH, Tq, Tk, dh, positive)
    tensors, got = _forward_backward(kind, case, eps, planes)
    again, _ = _forward_backward(kind, case, eps, planes)
    for a, b in zip(tensors, again):
        assert torch.equal(a, b), "a second forward + backward on the same inputs differs: not deterministic"
    dev = [t.to(DEV) for t in planes]
    ref = lb.reference(*dev, eps)
    bnd = lb.bounds(ref, *dev, eps)
    if dh == 1:
        assert not got["dQ"].any(), "dQ at dh = 1 is exactly zero"
    ratios = lb.check_all(got, ref, bnd, f"{tag} {dist}")
    print(f"LA_RATIO {tag} {dist} " + " ".join(f"{n}={ratios[n]:.3f}" for n in NAMES))
    return got, ref, bnd


@pytest.mark.parametrize("dist", lb.DISTRIBUTIONS)
@pytest.mark.parametrize("case,inst", lb.SELF_CASES, ids=_ids(lb.SELF_CASES))
def test_self_linear_attention_bounds(case, inst, dist):
    assert lb.la_instance(case[1], case[1]) == inst
    _verify("self", case, lb.EPS_DEFAULT, dist)


@pytest.mark.parametrize("dist", lb.DISTRIBUTIONS)
@pytest.mark.parametrize("case,inst", lb.CROSS_CASES, ids=_ids(lb.CROSS_CASES))
def test_cross_linear_attention_bounds(case, inst, dist):
    assert lb.la_instance(case[1], case[2]) == inst
    _verify("cross", case, lb.EPS_DEFAULT, dist)


@pytest.mark.parametrize("dist", lb.DISTRIBUTIONS)
@pytest.mark.parametrize("kind,case", lb.EPS_CASES, ids=[f"{k}-" + "-".join(map(str, c)) for k, c in lb.EPS_CASES])
def test_live_eps_bounds(kind, case, dist):
    """eps = 0.25: an error of Z, s, ds, cc or eps itself moves outputs and gradients (at 1e-6 they cancel)."""
    _verify(kind, case, lb.EPS_LIVE, dist)


@pytest.mark.parametrize("dh", [16, 64])
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_stores_are_unbiased(kind, dh):
    """The signed errors of O and dV sum to zero within 6 sigma of zero-mean rounding (attn_bounds.check_unbiased:
    v, dO > 0, 2 x 1025 rows).  A truncating bf16 store lands at about -5 x this limit
    (test_la_bounds.py::test_truncated_store_is_biased)."""
    case = (1, 1025, 2, dh, 0) if kind == "self" else (1, 1025, 1025, 2, dh, 1)
    got, ref, bnd = _verify(kind, case, lb.EPS_DEFAULT, "flat", positive=True)
    r = {n: lb.check_unbiased(got[n], ref[n], bnd[n], f"{kind} dh={dh} {n}") for n in ("O", "dV")}
    print(f"LA_BIAS {kind} dh={dh} O={r['O']:.3f} dV={r['dV']:.3f}")


# ------------------------------------------------------------------ extents of o, state, workspace, dq, dkv
PAD = 64                      # elements; keeps the float4 stores of the partial slabs 16-byte aligned
BF16_CANARY, F32_CANARY = 0x7FC1, 0x7FC00BAD   # NaN patterns no kernel result has


class _Carved:
    """`n` elements in the middle of a canary-filled allocation of n + 2 PAD."""

    def __init__(self, n, dtype):
        self.bits, self.canary = ((torch.int16, BF16_CANARY) if dtype == torch.bfloat16 else (torch.int32, F32_CANARY))
        self.whole = torch.empty(n + 2 * PAD, device=DEV, dtype=dtype)
        self.whole.view(self.bits).fill_(self.canary)
        self.t = self.whole[PAD:PAD + n]

    def intact(self):
        w = self.whole.view(self.bits)
        return bool((w[:PAD] == self.canary).all()) and bool((w[-PAD:] == self.canary).all())


# (B, Tq, Tk, heads, dh, raw): the LA_MAXCH cap on both sides / the key side, and B = 3
EXTENT_CASES = [("self", (1, 65537, 65537, 1, 8, 0)), ("self", (3, 100, 100, 3, 24, 1)),
                ("cross", (1, 100, 65537, 1, 8, 0)), ("cross", (3, 70, 2100, 2, 16, 1))]


@pytest.mark.parametrize("kind,case", EXTENT_CASES, ids=[f"{k}-" + "-".join(map(str, c)) for k, c in EXTENT_CASES])
def test_extents(kind, case):
    """fmd_linear_attention_fwd / _bwd and fmd_cross_attention_fwd / _bwd write nothing outside o, dq, dkv and the
    sizes fmd_linear_attention_state / _workspace report, and read nothing they did not write (the workspace
    starts as NaN); the results are those of the ops path."""
    from fmdiff import _lib
    O = ops()
    B, Tq, Tk, heads, dh, raw = case
    BH, inner, eps = B * heads, heads * dh, lb.EPS_DEFAULT
    assert B == 3 or lb.la_instance(Tq, Tk)[2:4] == (lb.LA_MAXCH, 1025)   # a cap row: the last slab slot is used
    q, k, v, do = lb.make_inputs(f"extents {kind} {case}", "flat", BH, Tq, Tk, dh)
    dout = lb.join_heads([do], B, heads, dh, raw).to(DEV)
    n_state = int(_lib.lib().fmd_linear_attention_state(B, heads))
    n_ws = int(_lib.lib().fmd_linear_attention_workspace(B, heads))
    assert n_state == BH * (D * D + 3 * D)
    o, state = _Carved(B * Tq * inner, torch.bfloat16), _Carved(n_state, torch.float32)
    ws_f, ws_b = _Carved(n_ws, torch.float32), _Carved(n_ws, torch.float32)
    if kind == "self":
        qkv = lb.join_heads([q, k, v], B, heads, dh, raw).to(DEV)
        dqkv = _Carved(qkv.numel(), torch.bfloat16)
        _lib.call("fmd_linear_attention_fwd", O._p(qkv), B, Tq, heads, dh, raw, eps, O._p(o.t), O._p(state.t),
                  O._p(ws_f.t), O.stream())
        _lib.call("fmd_linear_attention_bwd", O._p(qkv), O._p(dout), O._p(state.t), O._p(ws_b.t), B, Tq, heads, dh, raw,
                  eps, O._p(dqkv.t), O.stream())
        o2, state2 = O.linear_attention_fwd(qkv, Tq, heads, dh, raw, eps)
        grads = [(dqkv, O.linear_attention_bwd(qkv, dout, state2, Tq, heads, dh, raw, eps))]
    else:
        qt = lb.join_heads([q], B, heads, dh, raw).to(DEV)
        kvt = lb.join_heads([k, v], B, heads, dh, raw).to(DEV)
        dq, dkv = _Carved(qt.numel(), torch.bfloat16), _Carved(kvt.numel(), torch.bfloat16)
        _lib.call("fmd_cross_attention_fwd", O._p(qt), O._p(kvt), B, Tq, Tk, heads, dh, raw, 1, eps, O._p(o.t),
                  O._p(state.t), O._p(ws_f.t), O.stream())
        _lib.call("fmd_cross_attention_bwd", O._p(qt), O._p(kvt), O._p(o.t), O._p(dout), O._p(state.t), O._p(ws_b.t),
                  B, Tq, Tk, heads, dh, raw, 1, eps, O._p(dq.t), O._p(dkv.t), O.stream())
        o2, state2 = O.cross_attention_fwd(qt, kvt, Tq, Tk, heads, dh, eps, raw)
        dq2, dkv2 = O.cross_attention_bwd(qt, kvt, o2, dout, state2, Tq, Tk, heads, dh, eps, raw)
        grads = [(dq, dq2), (dkv, dkv2)]
    torch.cuda.synchronize()
    for name, c in [("o", o), ("state", state), ("forward workspace", ws_f), ("backward workspace", ws_b)] \
            + [(f"gradient {i}", g) for i, (g, _) in enumerate(grads)]:
        assert c.intact(), f"{name}: the canaries around the buffer were overwritten"
    assert torch.equal(o.t, o2.flatten()) and torch.equal(state.t, state2)
    for g, want in grads:
        assert bool(torch.isfinite(want.float()).all()) and torch.equal(g.t, want.flatten())
