"""The order bound of tests/skip_bwd_cases.py on the CPU: a plain fp32 matmul of every test case's bf16 operands
stays inside it (so a correct fp32 kernel cannot fail it), and it is far below one pixel's contribution (so a
kernel that drops or repeats a single pixel cannot pass it)."""
import pytest
import torch

import skip_bwd_cases as sc


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_fp32_matmul_is_inside_the_order_bound(name):
    dy, x = sc.flat(sc.problem(name))
    dw_ref, db_ref, _, _ = sc.reference(name)
    bw, bb = sc.order_bound(name)
    dw32 = (dy.float().t() @ x.float()).double()
    db32 = dy.float().sum(0).double()
    # against the exact sum a single fp32 summation has half the two-sum bound
    assert ((dw32 - dw_ref).abs() <= bw / 2).all(), ((dw32 - dw_ref).abs() / bw).max().item()
    assert ((db32 - db_ref).abs() <= bb / 2).all(), ((db32 - db_ref).abs() / bb).max().item()
    # another order (pixels reversed, in four chunks summed pairwise): inside the full bound of the first
    M = dy.shape[0]
    parts = [dy.float().flip(0)[i::4].t() @ x.float().flip(0)[i::4] for i in range(4)]
    dw_b = ((parts[0] + parts[1]) + (parts[2] + parts[3])).double()
    assert ((dw_b - dw32).abs() <= bw).all()
    assert M == sc.problem(name)["M"]


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_order_bound_sees_one_missing_pixel(name):
    dy, x = sc.flat(sc.problem(name))
    bw, bb = sc.order_bound(name)
    miss_w = (dy[-1][:, None] * x[-1][None, :]).abs()   # the last pixel of the partial tile left out
    miss_b = dy[-1].abs()
    assert (miss_w > bw).double().mean().item() > 0.9
    assert (miss_b > bb).double().mean().item() > 0.9
