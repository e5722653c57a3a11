"""csrc/misc.hip on the GPU, the train step and the sampler steps (noise_prepare, mse, adamw, adamw_sched, counter_add,
flow_euler, ddpm_step, sched_step, lincomb, gather_row, fill_from_table): every case of misc_ref.STEPS against
``fmdiff.runtime.ops``. The cases, their fp64 references, lattices, bounds and guards live in misc_ref.py;
test_misc_ref.py proves them on the CPU and shows that the same checks reject the known mutants."""
import pytest

import misc_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = mr.case_ids(mr.STEPS)


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    mr.RATIOS.clear()
    yield
    for fam, r in sorted(mr.RATIOS.items()):
        print(f"[misc_ref] {fam}: max err / bound {r:.3f}")


@pytest.mark.parametrize("family,case", IDS, ids=[f"{f}-{c}" for f, c in IDS])
def test_step_kernels(family, case):
    from fmdiff.runtime import ops
    mr.CASES[family][case](ops, DEV)
