"""The VQVAE latent join on the device (MI355X): ``ops.vq_join_bwd`` (csrc/vq_train.hip ``fmd_vq_join_bwd``) against
the derived per-element bound of tests/vq_join_bounds.py and, bit for bit, against the existing and separately
bounded ``ops.vq_backward`` on the same operands rounded to nearest even to bf16.

Rows: 105 (less than one workgroup's worth at every D) and 2112 (more than one workgroup from D = 8 on; at D = 256
with the wide output stride 2112 * 34 groups = 281 workgroups).  D: 1 and 12 (a single partial group: the scalar
path), 32 / 64 / 256 (whole groups: the 16-byte path), with strides that make the output wider than D by one and by
two whole padding groups.  K = 70."""
import pytest
import torch

import vq_join_bounds as JB

pytestmark = pytest.mark.gpu

K = 70
_CACHE = {}


def _case(N, h, w, D):
    key = (N, h, w, D)
    if key not in _CACHE:
        _CACHE[key] = JB.make_case(N * h * w, D, K, 1000 * D + N)
    return _CACHE[key]


def _rows(t, N, h, w, ld, dtype=torch.float32):
    """[M, D] fp32 -> device [N, h, w, ld] of ``dtype`` with NaN in every padding channel."""
    out = torch.full((t.shape[0], ld), float("nan"))
    out[:, :t.shape[1]] = t
    return out.reshape(N, h, w, ld).to(dtype).cuda()


def _strides(D):
    """(ldg, ldz, ld_out): the tightest rows, and rows wider by an odd number of floats (z, the residual) and by
    one and two whole groups (g, the output)."""
    D8 = -(-D // 8) * 8
    return ((D8, D, D8), (D8 + 8, D + 3, D8 + 16))


@pytest.mark.parametrize("D", [1, 12, 32, 64, 256])
@pytest.mark.parametrize("N,h,w", [(3, 5, 7), (2, 33, 32)])
def test_join_within_the_bound_and_equal_to_vq_backward_rounded(N, h, w, D):
    from fmdiff.runtime import ops
    g, z, e, codes, g_loss = _case(N, h, w, D)
    M = N * h * w
    q = e[codes]
    ed, cd = e.cuda(), codes.reshape(N, h, w).cuda()
    gl = torch.tensor([g_loss], device="cuda")
    worst = 0.0
    for ldg, ldz, ldo in _strides(D):
        zd = _rows(z, N, h, w, ldz)
        rd = _rows(z - q, N, h, w, ldz)             # the saved residual: z - q rounded once, as vq_residual leaves it
        garms = {"bf16": _rows(g, N, h, w, ldg, torch.bfloat16), "fp32": _rows(g, N, h, w, ldg), "null": None}
        assert torch.isnan(zd).any() == (ldz > D) and torch.isnan(garms["bf16"]).any() == (ldg > D)
        g32 = garms["fp32"]
        for c in (0.25, -0.75):
            for glt, glv in ((gl, g_loss), (None, None)):
                s = JB.coef64(glv, c, M, D)
                for gname, gd in garms.items():
                    gc = None if gd is None else g
                    v, bd = JB.exact(gc, z, q, s), JB.bound(gc, z, q, s)
                    ref = ops.vq_backward(zd, D, cd, ed, None if gd is None else g32, glt, c)[..., :D]
                    ref = ref.to(torch.bfloat16)
                    for mode, args in (("codebook", (zd, cd, ed)), ("residual", (rd, None, None))):
                        out = ops.vq_join_bwd(gd, D, *args, glt, c, ld_out=ldo)
                        again = ops.vq_join_bwd(gd, D, *args, glt, c, ld_out=ldo)
                        what = f"D={D} ld=({ldg},{ldz},{ldo}) c={c} g={gname} g_loss={glv} {mode}"
                        assert out.shape == (N, h, w, ldo) and out.dtype == torch.bfloat16, what
                        assert torch.equal(out, again), what
                        assert not torch.isnan(out).any(), what
                        assert (out[..., D:] == 0).all(), what
                        assert torch.equal(out[..., :D].view(torch.int16), ref.view(torch.int16)), what
                        worst = max(worst, JB.check(what, out[..., :D].float().cpu().reshape(M, D), v, bd))
    print(f"rows={M} D={D}: largest error / bound {worst:.3f}")


def test_preallocated_output_and_default_stride():
    from fmdiff.runtime import ops
    N, h, w, D = 3, 5, 7, 12
    g, z, e, codes, g_loss = _case(N, h, w, D)
    zd, gd = _rows(z, N, h, w, D), _rows(g, N, h, w, 16)
    gl = torch.tensor([g_loss], device="cuda")
    a = ops.vq_join_bwd(gd, D, zd, codes.cuda(), e.cuda(), gl, 0.25)
    assert a.shape == (N, h, w, 16)
    out = torch.full((N, h, w, 24), float("nan"), dtype=torch.bfloat16, device="cuda")
    b = ops.vq_join_bwd(gd, D, zd, codes.cuda(), e.cuda(), gl, 0.25, out=out)
    assert b is out and torch.equal(out[..., :16], a) and (out[..., 16:] == 0).all()


def test_refusals():
    from fmdiff import _lib
    from fmdiff.runtime import ops
    N, h, w = 2, 4, 4
    M = N * h * w
    z = torch.zeros((N, h, w, 264), device="cuda")
    codes = torch.zeros((N, h, w), dtype=torch.int64, device="cuda")
    out = torch.zeros((N, h, w, 264), dtype=torch.bfloat16, device="cuda")
    g = torch.zeros((N, h, w, 8), dtype=torch.bfloat16, device="cuda")
    fn = _lib.lib().fmd_vq_join_bwd
    s = ops.stream()
    ok = dict(z=z.data_ptr(), ldz=264, M=M, K=1, D=12, codes=None, e=None, g=g.data_ptr(), f32=0, ldg=8, gl=None,
              c=0.25, scale=1.0, dz=out.data_ptr(), lddz=16)
    bad = [dict(D=257, lddz=264, g=None),dict(D=0), dict(ldz=11), dict(lddz=8), dict(lddz=20), dict(ldg=4), dict(D=9, ldg=8, lddz=16),
           dict(ldg=12), dict(M=0), dict(z=None), dict(dz=None), dict(e=z.data_ptr()), dict(f32=2),
           dict(dz=out.data_ptr() + 2), dict(g=g.data_ptr() + 2)]
    for kw in bad:
        a = {**ok, **kw}
        assert fn(*a.values(), s) == -1, kw
    with pytest.raises((ValueError, RuntimeError)):      # D = 257
        ops.vq_join_bwd(None, 257, z, None, None, None, 0.25)
    with pytest.raises((ValueError, RuntimeError)):      # a g stride below D
        ops.vq_join_bwd(g, 12, z, None, None, None, 0.25)
    with pytest.raises((ValueError, RuntimeError)):      # a z stride below D
        ops.vq_join_bwd(None, 12, z[..., :8].contiguous(), None, None, None, 0.25)
    with pytest.raises((ValueError, RuntimeError)):      # an output stride below D
        ops.vq_join_bwd(None, 12, z, None, None, None, 0.25, ld_out=8)
    with pytest.raises((ValueError, RuntimeError)):      # codes of the wrong length
        ops.vq_join_bwd(None, 12, z, codes[:1], torch.zeros((K, 12), device="cuda"), None, 0.25)
    with pytest.raises((ValueError, RuntimeError)):      # a stride that is no multiple of 8
        ops.vq_join_bwd(None, 12, z, None, None, None, 0.25, ld_out=20)
    torch.cuda.synchronize()
    assert not out.any()                                  # nothing was launched
