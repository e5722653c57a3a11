"""The GroupNorm error bounds of gn_bounds.py, checked on the CPU before any GPU run.

1. The closed form dx = P dz + Q x + R (with dgamma, dbeta and both demb forms) equals fp64 autograd of
   F.group_norm at 1e-9, for every case of test_gpu_groupnorm.py and every embedding mode.
2. The faithful emulation of the kernel arithmetic (gn_bounds.emulate) stays inside the bare bounds, with no margin,
   for every case and distribution.  Maxima over the twelve cases of err / bound: t 0.995, dx0 0.995, dx1 0.994 (one
   bf16 rounding: the bound is met, not padded); every fp32 output below 0.34 (dbeta 0.335 at 1x1 images, a 0.19,
   P 0.13, b 0.10, rstd 0.10, dgamma 0.10, Q 0.07, demb 0.07, R 0.06, mean 0.02).  The fp32 bounds are worst-case
   chains of 17 to 276 additions; the errors add up like a random walk.
3. On corr and offset the RMS of Q (x - mean) and of R is each at least 10 % of the RMS of P dz in every case
   (Q: 0.27 .. 0.47; R: 0.33 .. 0.67 on corr, 5.5 .. 7.2 on offset); on noise (cfgB_256_128) R is below 2 %.
4. Kernels that are wrong in a known way (mutants of the emulation) are rejected by check() at the margin the GPU
   tests use (1.5) in every case where they apply, on corr and on offset.
5. The same mutants against the present check of test_gpu_kernels.py::test_groupnorm_forward_backward (_close:
   max-norm 1.5e-2 on dx; rtol = atol = 1e-3 on dgamma, dbeta, demb; a, b, mean, rstd, P, Q, R never looked at).

Rejected in how many of the cases where the mutant applies (new = per-output bounds at margin 1.5, old = _close
and assert_close as above, applied to the same twelve cases):

  mutant                  noise        corr         offset       caught by
                          new   old    new   old    new   old
  no_mean_terms           12/12  9/12   12/12 12/12   12/12 12/12   dx0, dx1
  no_R                    12/12  6/12   12/12 12/12   12/12 12/12   dx0, dx1
  uncentred_Q             12/12  3/12   12/12 10/12   12/12 12/12   R, dx0, dx1, demb (mode 2)
  rstd_1pct               12/12 12/12   12/12 12/12   12/12 12/12   rstd, a, b, P, Q, dgamma, then dx, t, R, demb
  gp_without_scale         5/5   5/5     5/5   5/5     5/5   5/5    P, Q, R, dx0
  dbeta_without_scale      5/5   5/5     5/5   5/5     5/5   5/5    dbeta
  demb_swapped             5/5   5/5     5/5   5/5     5/5   5/5    demb
  demb2_no_R               1/1   1/1     1/1   1/1     1/1   1/1    demb
  straddle_src0_only       3/3   3/3     3/3   3/3     3/3   3/3    mean, rstd, a, b, t, P, Q, R, dx0, dx1, dgamma
  acc_ignored              2/2   2/2     2/2   2/2     2/2   2/2    dx1
  extra_dropped            4/4   4/4     4/4   4/4     4/4   4/4    dx0, dx1
  last_slab_row_dropped    5/5   5/5     5/5   5/5     5/5   5/5    dbeta, dgamma, dx0, dx1, Q, R, demb
  dgamma_overwrites       12/12 12/12   12/12 12/12   12/12 12/12   dgamma

With the white-noise dz of the present test, its max-norm check lets the backward without R through in half of the
cases and the uncentred Q in nine of twelve.  Every mutant is rejected by the new check on every distribution; none
needed an exception.  The mutants of the last rows are caught by the old assertions too once a case reaches them at
all: the present suite has no case with a second source, an accumulating destination, extra, mode 2 or a non-zero
starting gradient.
The existing gradients dg0 / db0 are drawn at sqrt(N HW), the size of the sums they receive: at unit size the
70400-pixel cases (tall_slab, folded) would have an fp32 summation bound on dgamma larger than dg0 on offset, and
dgamma_overwrites would pass there.
"""
import functools

import pytest
import torch

import gn_bounds as gb

CASES = list(gb.CASES)
HARD = ("corr", "offset")          # the distributions every mutant must be rejected on


@functools.lru_cache(maxsize=None)
def _case(case, dist):
    inp = gb.make_inputs(case, dist)
    cf = gb.closed_form(inp)
    return inp, cf, gb.bounds(inp, cf)


@functools.lru_cache(maxsize=None)
def _emulated(case, dist, mutant):
    return gb.emulate(_case(case, dist)[0], mutant=mutant)


def _failing(case, dist, mutant, margin=gb.MARGIN):
    """The outputs on which check() rejects the (mutated) emulation at this margin."""
    _, cf, bnd = _case(case, dist)
    emu = _emulated(case, dist, mutant)
    bad = []
    for n in gb.NAMES:
        if cf.get(n) is None or not cf[n].numel():
            continue
        try:
            gb.check(emu[n], cf[n], bnd[n], f"{case} {dist} {mutant} {n}", margin)
        except AssertionError:
            bad.append(n)
    return bad


def _old_catches(case, dist, mutant):
    """The assertions of test_gpu_kernels.py::test_groupnorm_forward_backward as a predicate: max-norm 1.5e-2 on
    dx; rtol = atol = 1e-3 on dgamma, dbeta, demb."""
    _, cf, _ = _case(case, dist)
    emu = _emulated(case, dist, mutant)
    got = torch.cat([emu["dx0"].float(), emu["dx1"].float()], -1)
    ref = torch.cat([cf["dx0"], cf["dx1"]], -1).float()
    if (got - ref).abs().max().item() > 1.5e-2 * max(ref.abs().max().item(), 1e-6):
        return True
    for n in ("dgamma", "dbeta", "demb"):
        if cf.get(n) is not None and bool(((emu[n].double() - cf[n]).abs() > 1e-3 + 1e-3 * cf[n].abs()).any()):
            return True
    return False


@pytest.mark.parametrize("case", CASES)
def test_closed_form_equals_autograd(case):
    """dx = P dz + Q x + R, dgamma, dbeta and both demb forms equal fp64 autograd of F.group_norm at 1e-9
    (relative to 1 + the largest reference value of each output), on every distribution."""
    for dist in gb.DISTRIBUTIONS:
        inp, cf, _ = _case(case, dist)
        ref = gb.reference(inp)
        for n in gb.NAMES:
            if n in ("P", "Q", "R") or ref.get(n) is None or not ref[n].numel():
                continue
            err = float((cf[n] - ref[n]).abs().max())
            assert err <= 1e-9 * (1 + float(ref[n].abs().max())), (case, dist, n, err)
        assert (cf["demb"] is None) == (ref["demb"] is None) == (gb.geometry(case)["mode"] == 0)


@pytest.mark.parametrize("dist", gb.DISTRIBUTIONS)
@pytest.mark.parametrize("case", CASES)
def test_emulation_within_bounds(case, dist):
    """The faithful emulation stays inside the bare bounds (ratio <= 1, no margin) for every output."""
    inp, cf, bnd = _case(case, dist)
    ratios = gb.check_all(_emulated(case, dist, None), cf, bnd, f"{case} {dist}", margin=1.0)
    print(f"GN_EMU {case} {dist} " + " ".join(f"{n}={v:.3f}" for n, v in ratios.items()))


@pytest.mark.parametrize("dist", HARD)
@pytest.mark.parametrize("case", CASES)
def test_inputs_exercise_the_mean_terms(case, dist):
    """On corr and offset the RMS of Q (x - mean) and of R is each at least 10 % of the RMS of P dz: the two terms
    that make this a GroupNorm backward are not below the noise."""
    inp, cf, _ = _case(case, dist)
    x, dz = inp["x"].double(), inp["dz"].double()

    def rms(v):
        return float(v.pow(2).mean().sqrt())

    pdz = rms(cf["P"][:, None] * dz)
    q = rms(cf["Q"][:, None] * (x - cf["_mc"][:, None]))
    r = rms(cf["R"])
    print(f"GN_RMS {case} {dist} Q(x-m)/Pdz={q / pdz:.3f} R/Pdz={r / pdz:.3f}")
    assert q >= 0.1 * pdz and r >= 0.1 * pdz


def test_noise_hides_the_mean_terms():
    """What the white-noise dz of the present test does to them (the reason for the other two distributions)."""
    inp, cf, _ = _case("cfgB_256_128", "noise")
    pdz = (cf["P"][:, None] * inp["dz"].double()).pow(2).mean().sqrt()
    assert cf["R"].pow(2).mean().sqrt() < 0.02 * pdz


@pytest.mark.parametrize("mutant", gb.MUTANTS)
def test_mutant_is_caught(mutant):
    """check() at the GPU tests' margin rejects the mutant in every case where it applies, on corr and offset."""
    applied = [c for c in CASES if gb.applies(mutant, c)]
    assert applied
    for dist in HARD:
        for case in applied:
            assert _failing(case, dist, mutant), (mutant, case, dist)


def test_faithful_emulation_passes_old_and_new():
    for case in CASES:
        for dist in gb.DISTRIBUTIONS:
            assert not _failing(case, dist, None) and not _old_catches(case, dist, None), (case, dist)


def test_present_check_misses():
    """What the max-norm check of test_groupnorm_forward_backward lets through with its own white-noise dz
    (module docstring table): a dropped R and an uncentred Q in half of the cases or more."""
    for mutant in ("no_R", "uncentred_Q"):
        missed = [c for c in CASES if not _old_catches(c, "noise", mutant)]
        assert len(missed) >= len(CASES) // 2, (mutant, missed)


def test_mutant_table():
    """Prints the table of the module docstring."""
    print()
    print("  mutant                  noise        corr         offset       caught by")
    print("                          new   old    new   old    new   old")
    for mutant in gb.MUTANTS:
        applied = [c for c in CASES if gb.applies(mutant, c)]
        row, by = f"  {mutant:<22}", {}
        for dist in gb.DISTRIBUTIONS:
            new = 0
            for c in applied:
                bad = _failing(c, dist, mutant)
                new += bool(bad)
                for n in bad:
                    by[n] = by.get(n, 0) + 1
            old = sum(_old_catches(c, dist, mutant) for c in applied)
            row += f"  {new:>2}/{len(applied):<2} {old:>2}/{len(applied):<2} "
        print(row + "  " + ", ".join(sorted(by, key=lambda n: -by[n])))


def test_emulated_branches_match_the_cases():
    """The cases reach what they are there for (source of truth: gn_prep_kernel / gn_bwd_prep_kernel)."""
    g = gb.geometry
    assert [gi for gi in range(4) if gb.straddles(g("straddle_cg24"), gi)] == [2]
    assert [gi for gi in range(32) if gb.straddles(g("cfgB_512_256"), gi)] == [21]
    assert [gi for gi in range(32) if gb.straddles(g("cfgB_256_128"), gi)] == [21]
    assert not any(gb.vector_branch(g("cg3_odd_ss"), gi) for gi in range(32))
    c = g("tall_slab")
    E, T = c["HW"] // c["rows"], 256 // c["Cg"]
    assert E == 1100 and E > 3 * 256 and E % (4 * 256) and E > 3 * T and E % (4 * T)
    c = g("folded")
    assert (c["HW"] // c["rows"]) % c["fold"] == 0
    c = g("cfgB_256_128")
    assert (c["rows0"], c["rows1"]) == (64, 256)
    c = g("emb_add_slot")     # mode-2 demb reads sum x from a forward slab with other rows than s12's
    assert c["mode"] == 2 and c["fold"] == 1 and c["HW"] // c["rows0"] == 16 and c["HW"] // c["rows"] == 4
