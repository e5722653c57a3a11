"""The ResBlock backward's skip pass and dropout on the GPU: fmd_conv_gn_apply (IG_GNA64 / IG_GNA128), fmd_skip_bwd
and fmd_dropout_apply against ``fmdiff.runtime.ops``, every case of skip_lattice.CASES.  The fp64 statements, the
lattice, the conditions, the bounds and the guards live in skip_lattice.py; test_skip_lattice.py proves them on the
CPU and shows that the same checks reject the known mutants.  Every expected value is fp64 torch / numpy on the CPU."""
import pytest
import torch

import skip_lattice as sl
from misc_ref import RATIOS

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = sl.case_ids()


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    RATIOS.clear()
    yield
    for fam, r in sorted(RATIOS.items()):
        print(f"[skip_lattice] {fam}: max err / bound {r:.3f}")


@pytest.mark.parametrize("family,case", IDS, ids=[f"{f}-{c}" for f, c in IDS])
def test_skip_lattice(family, case):
    from fmdiff.runtime import ops
    sl.CASES[family][case](ops, DEV)


# ------------------------------------------------------------------ host rejections: nothing is launched
def _x(shape):
    return torch.full(shape, 0.75, dtype=torch.bfloat16, device=DEV)


def _seed():
    return torch.tensor([5], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("what", ["c_not_multiple_of_8", "p_one", "p_negative", "ep_without_a"])
def test_dropout_host_rejects(what):
    from fmdiff.runtime import ops
    C = 12 if what == "c_not_multiple_of_8" else 8
    p = {"p_one": 1.0, "p_negative": -0.25}.get(what, 0.5)
    x, out = _x((1, 2, 2, C)), _x((1, 2, 2, C))
    ep = (_x((1, 2, 2, C)), None, None) if what == "ep_without_a" else None
    with pytest.raises(RuntimeError, match="fmd_dropout_apply failed with code -1"):
        ops.dropout_apply(x, p, _seed(), 3, ep=ep, out=out)
    torch.cuda.synchronize()
    assert bool((out == 0.75).all()) and bool((x == 0.75).all())


def test_dropout_host_rejects_an_index_past_32_bits():
    """M C = 2^32 by sizes alone: an 8-element buffer expanded to 2^29 pixels (stride 0), in place so that nothing of
    that size is allocated.  The call returns before any launch."""
    from fmdiff.runtime import ops
    base = _x((8,))
    x = base.expand(1 << 29, 8)
    assert x.shape[0] * x.shape[-1] == 1 << 32
    with pytest.raises(RuntimeError, match="fmd_dropout_apply failed with code -2"):
        ops.dropout_apply(x, 0.5, _seed(), 3, out=x)
    torch.cuda.synchronize()
    assert bool((base == 0.75).all())
