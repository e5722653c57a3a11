"""The linear-attention error bounds of la_bounds.py, checked on the CPU before any GPU run.

1. The fp64 closed form (la_bounds.reference) is the gradient torch.autograd gives oracle.unet._linear_attention.
2. The faithful fp32 emulation of the kernels (la_bounds.emulate) stays inside the bare bounds, margin 1.0, on
   every case row x distribution of test_gpu_linear_attention.py, the T = 65537 cap rows included (as they are).
3. Kernels that are wrong in a known way (MUTANTS) are rejected at the GPU tests' margin (1.5) on the row that
   exists to catch them (MUTANT_ROW), and test_mutant_table prints (-s) what the max-norm assertion of
   test_gpu_kernels.py::test_linear_attention / test_cross_attention says to the same tensors.

At eps = 1e-6, the only value the max-norm tests use, s = sum ks = 1 makes ctx = A / (s + eps) cancel any error of
the column normaliser Z, and ds - cc collapse to -P: combining the chunk statistics without the exp(mc - M)
rescale, dropping eps and dropping cc change no output and no gradient beyond 1e-6 relative, and the max-norm
assertion passes all three (test_old_assertion_passes_dead_arithmetic).  The state check catches the first through
the Z bound; the eps = 0.25 rows catch the other two, and no_ds, through the gradients.
"""
import functools

import pytest
import torch

import la_bounds as lb

ROWS = lb.all_rows()
BIG = ("self", (1, 1025, 2, 32, 1))


def _id(row):
    return lb.row_key(*row).replace(" ", "")


@functools.lru_cache(maxsize=None)
def _case(kind, case, eps, dist, positive=False):
    BH, Tq, Tk, dh = lb.canonical(kind, case)
    q, k, v, do = lb.make_inputs(lb.row_key(kind, case, eps), dist, BH, Tq, Tk, dh, positive)
    ref = lb.reference(q, k, v, do, eps)
    return (q, k, v, do, eps), ref, lb.bounds(ref, q, k, v, do, eps)


@functools.lru_cache(maxsize=None)
def _emulated(kind, case, eps, dist, mutant, positive=False):
    return lb.emulate(*_case(kind, case, eps, dist, positive)[0], mutant=mutant)


def new_catches(row, dist, mutant, margin=lb.MARGIN, names=lb.OUTPUTS + lb.STATE):
    """Which of the tensors reject the (mutated) emulation at this margin ('M': the exact maximum)."""
    _, ref, bnd = _case(*row, dist)
    got = _emulated(*row, dist, mutant)
    bad = [] if torch.equal(got["M"].double(), ref["M"]) else ["M"]
    for n in names:
        try:
            lb.check(got[n], ref[n], bnd[n], n, margin)
        except AssertionError:
            bad.append(n)
    return bad


def old_catches(row, dist, mutant):
    """Does the max-norm assertion of test_linear_attention / test_cross_attention reject it?  o at 1.5e-2 max|ref|;
    self: the fused dqkv at 2e-2; cross: dq, and the fused dkv, at 2e-2.  The state is not looked at."""
    _, ref, _ = _case(*row, dist)
    got = _emulated(*row, dist, mutant)

    def close(names, rel):
        g = torch.cat([got[n].double().flatten() for n in names])
        r = torch.cat([ref[n].flatten() for n in names])
        return float((g - r).abs().max()) <= rel * max(float(r.abs().max()), 1e-6)   # a NaN fails

    groups = [("dQ", "dK", "dV")] if row[0] == "self" else [("dQ",), ("dK", "dV")]
    return not (close(("O",), 1.5e-2) and all(close(g, 2e-2) for g in groups))


# ------------------------------------------------------------------ 1. the closed form is the gradient
@pytest.mark.parametrize("eps", [lb.EPS_DEFAULT, lb.EPS_LIVE])
@pytest.mark.parametrize("BH,Tq,Tk,dh", [(3, 17, 17, 12), (2, 70, 130, 16), (2, 40, 5, 1)])
def test_reference_is_autograd(BH, Tq, Tk, dh, eps):
    from oracle.unet import _linear_attention
    for dist in lb.DISTRIBUTIONS:
        q, k, v, do = lb.make_inputs(f"autograd {BH} {Tq} {Tk} {dh}", dist, BH, Tq, Tk, dh)
        ref = lb.reference(q, k, v, do, eps)
        leaves = [t.double().requires_grad_() for t in (q, k, v)]
        o = _linear_attention(*leaves, eps=eps)
        o.backward(do.double())
        for n, want in zip(("O", "dQ", "dK", "dV"), [o.detach()] + [t.grad for t in leaves]):
            scale = max(float(want.abs().max()), 1e-300)
            assert float((ref[n] - want).abs().max()) <= 1e-12 * scale, (dist, n)
        assert torch.equal(ref["M"], k.double().max(1).values)
        assert float((ref["s"] - 1).abs().max()) < 1e-12


# ------------------------------------------------------------------ 2. the emulation inside the bare bounds
@pytest.mark.parametrize("dist", lb.DISTRIBUTIONS)
@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_emulation_within_bounds(row, dist):
    """Margin 1.0, every tensor, M exact; the references are finite and not degenerate (dQ at dh = 1 is exactly 0,
    in the reference and in the emulation; with one key row dQ and dK vanish mathematically)."""
    (q, k, v, do, eps), ref, bnd = _case(*row, dist)
    dh = q.shape[-1]
    for n in lb.OUTPUTS + lb.STATE + ("M",):
        assert bool(torch.isfinite(ref[n]).all()), n
        if n in bnd:
            assert bool(torch.isfinite(bnd[n]).all()), n
    for n in lb.OUTPUTS:
        if n == "dQ" and dh == 1:
            assert not ref[n].any()
        elif n in ("dQ", "dK") and k.shape[1] == 1:
            # one key row: ks = 1, so dK = ks (dks - sum ks dks) = 0 and every row of ctx is v / (1 + eps), so
            # dqs is constant over d and dQ = 0; the fp64 reference holds rounding noise or exact zeros
            assert float(ref[n].abs().max()) <= 1e-12 * float(do.double().abs().max() * v.double().abs().max())
        else:
            assert float(ref[n].abs().max()) > 0, n
    emu = _emulated(*row, dist, None)
    if dh == 1:
        assert not emu["dQ"].any()
    ratios = lb.check_all(emu, ref, bnd, f"{row} {dist}", margin=1.0)
    print(f"LA_EMU {lb.row_key(*row)} {dist} " + " ".join(f"{n}={r:.3f}" for n, r in ratios.items()))


def test_instances_and_mirror():
    """The case rows name the chunking they reach; spot values of la_chunks (source of truth: la_args)."""
    assert [lb.la_chunks(T) for T in (1, 1024, 1025, 2048, 2049, 65536, 65537, 200000)] == \
        [(1, 1), (1, 1024), (2, 513), (2, 1024), (3, 683), (64, 1024), (64, 1025), (64, 3125)]
    for c, inst in lb.SELF_CASES:
        assert lb.la_instance(c[1], c[1]) == inst, c
    for c, inst in lb.CROSS_CASES:
        assert lb.la_instance(c[1], c[2]) == inst, c
    seen = {(i[0], i[2]) for _, i in lb.SELF_CASES + lb.CROSS_CASES}
    assert {(1, 1), (2, 2), (3, 3), (64, 64), (1, 3), (3, 1), (2, 1)} <= seen


def test_distributions_are_what_they_claim():
    _, ref, _ = _case(*BIG, lb.EPS_DEFAULT, "peaked")
    assert float(ref["ks"].max(1).values.min()) > 0.9          # every column softmax is near one-hot
    assert float(ref["xq"].min()) < -25                        # exp of large negative arguments in the q softmax
    (q, k, v, do, _), ref, _ = _case(*BIG, lb.EPS_DEFAULT, "offset")
    assert float(k.float().min()) > 36 and float(q.float().max()) < -26 and float(v.float().mean()) > 2.5
    _, ref, _ = _case(*BIG, lb.EPS_DEFAULT, "flat")
    assert float(ref["ks"].max()) < 0.02


# ------------------------------------------------------------------ 3. mutants
# mutant -> (row, distribution, tensors that must reject it at margin 1.5)
_R65, _R1025, _CROSS = (("self", (2, 65, 3, 24, 0)), ("self", (1, 1025, 2, 32, 1)), ("cross", (2, 70, 2100, 2, 16, 1)))
MUTANT_ROW = {
    "drop_last_key": (_R65 + (lb.EPS_DEFAULT,), "flat", {"O", "ctx", "s"}),
    "per_floor": (_R1025 + (lb.EPS_DEFAULT,), "flat", {"O", "dQ", "dK", "dV", "ctx"}),
    "stats_no_rescale": (_R1025 + (lb.EPS_DEFAULT,), "flat", {"Z", "s"}),
    "max_first_chunk_only": (_R1025 + (lb.EPS_DEFAULT,), "peaked", {"M"}),
    "eps_dropped": (_R65 + (lb.EPS_LIVE,), "flat", {"O", "dQ", "dK", "dV", "ctx"}),
    "no_cc": (_R65 + (lb.EPS_LIVE,), "flat", {"dK"}),
    "no_ds": (_R65 + (lb.EPS_LIVE,), "flat", {"dK"}),
    "dq_no_dot": (("self", (2, 17, 2, 24, 0), lb.EPS_DEFAULT), "flat", {"dQ"}),
    "q_pad_in_softmax": (("self", (2, 17, 2, 12, 0), lb.EPS_DEFAULT), "flat", {"O", "dQ", "dK", "dV"}),
    "swap_dk_dv": (("self", (2, 64, 3, 24, 1), lb.EPS_DEFAULT), "flat", {"dK", "dV"}),
    "bwd_uses_nchk_for_dctx": (_CROSS + (lb.EPS_DEFAULT,), "flat", {"dK", "dV"}),
    "out_trunc": None,     # check_unbiased on the bias rows: test_truncated_store_is_biased
}
DEAD_AT_DEFAULT_EPS = ("stats_no_rescale", "eps_dropped", "no_cc")


def test_mutant_rows_cover_all_mutants():
    assert set(MUTANT_ROW) == set(lb.MUTANTS)
    assert all(r[0] in ROWS for r in MUTANT_ROW.values() if r)


@pytest.mark.parametrize("mutant", [m for m in lb.MUTANTS if MUTANT_ROW[m]])
def test_mutant_is_caught(mutant):
    row, dist, must = MUTANT_ROW[mutant]
    assert not new_catches(row, dist, None, margin=1.0)
    bad = set(new_catches(row, dist, mutant))
    assert must <= bad, f"{mutant}: rejected only by {sorted(bad)}"


def test_which_check_catches_what():
    """stats_no_rescale at eps = 1e-6: the state check alone (Z, and s), no output and no gradient; eps_dropped and
    no_cc at eps = 1e-6: nothing at all (dead arithmetic); all three, and no_ds, are live at eps = 0.25."""
    row = _R1025 + (lb.EPS_DEFAULT,)
    for dist in lb.DISTRIBUTIONS:
        assert set(new_catches(row, dist, "stats_no_rescale")) == {"Z", "s"}
        assert not new_catches(row, dist, "eps_dropped") and not new_catches(row, dist, "no_cc")
    for kind, case in lb.EPS_CASES:
        row = (kind, case, lb.EPS_LIVE)
        assert "dK" in new_catches(row, "flat", "no_cc", names=lb.OUTPUTS)
        assert "dK" in new_catches(row, "flat", "no_ds", names=lb.OUTPUTS)
        assert {"O", "dQ", "dK", "dV"} <= set(new_catches(row, "flat", "eps_dropped", names=lb.OUTPUTS))
    row = _R1025 + (lb.EPS_LIVE,)
    assert set(new_catches(row, "flat", "stats_no_rescale", names=lb.OUTPUTS)) & {"O", "dK", "dV"}


def test_old_assertion_passes_dead_arithmetic():
    """The point of these tests: on the same inputs the max-norm assertion passes the three corruptions."""
    for kind, case, eps in ROWS:
        if eps != lb.EPS_DEFAULT or lb.canonical(kind, case)[1] > 3000:
            continue
        for m in DEAD_AT_DEFAULT_EPS:
            assert not old_catches((kind, case, eps), "flat", m), (kind, case, m)


def test_mutant_table():
    """Printed with -s: per mutant, its row, what rejects it now, and whether the old assertion passes it."""
    print()
    for m in lb.MUTANTS:
        if MUTANT_ROW[m] is None:
            continue
        row, dist, _ = MUTANT_ROW[m]
        print(f"LA_MUTANT {m:24s} {lb.row_key(*row):36s} {dist:7s} new rejects {','.join(new_catches(row, dist, m)):24s}"
              f" old assertion {'rejects' if old_catches(row, dist, m) else 'passes'}")
    row = _R1025 + (lb.EPS_DEFAULT,)
    for m in DEAD_AT_DEFAULT_EPS + ("no_ds",):
        print(f"LA_MUTANT {m:24s} {lb.row_key(*row):36s} flat    new rejects {','.join(new_catches(row, 'flat', m)) or '-':24s}"
              f" old assertion {'rejects' if old_catches(row, 'flat', m) else 'passes'}")
    assert not old_catches(row, "flat", None)


@pytest.mark.parametrize("dh", [16, 64])
def test_truncated_store_is_biased(dh):
    """check_unbiased() on O and dV (v, dO > 0, T = 1025: the bias rows of the GPU tests) passes the faithful
    emulation with |sum / limit| < 0.2 and rejects bf16 stores that truncate."""
    row = ("self", (1, 1025, 2, dh, 0), lb.EPS_DEFAULT)
    _, ref, bnd = _case(*row, "flat", True)
    emu, mut = _emulated(*row, "flat", None, True), _emulated(*row, "flat", "out_trunc", True)
    lb.check_all(emu, ref, bnd, "emulation", margin=1.0)
    for n in ("O", "dV"):
        assert float(ref[n].min()) > 0
        assert abs(lb.check_unbiased(emu[n], ref[n], bnd[n], f"emulation {n}")) < 0.2
        with pytest.raises(AssertionError, match="biased conversion"):
            lb.check_unbiased(mut[n], ref[n], bnd[n], f"out_trunc {n}")
