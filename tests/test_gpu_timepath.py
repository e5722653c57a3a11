"""csrc/misc.hip on the GPU, the time path (timestep_embedding, linear, linear_bwd, GroupedLinear, silu_bwd): every case
of misc_ref.TIMEPATH against ``fmdiff.runtime.ops``. The cases, their fp64 references, lattices, bounds and guards
live in misc_ref.py; test_misc_ref.py proves them on the CPU and shows that the same checks reject the known mutants."""
import pytest

import misc_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = mr.case_ids(mr.TIMEPATH)


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    mr.RATIOS.clear()
    yield
    for fam, r in sorted(mr.RATIOS.items()):
        print(f"[misc_ref] {fam}: max err / bound {r:.3f}")


@pytest.mark.parametrize("family,case", IDS, ids=[f"{f}-{c}" for f, c in IDS])
def test_timepath(family, case):
    from fmdiff.runtime import ops
    mr.CASES[family][case](ops, DEV)
