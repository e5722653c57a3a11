"""csrc/misc.hip on the GPU, layout and parameter-free resampling (nchw_to_nhwc, nhwc_to_nchw, affine_channels, add_,
sum_pool2, sum_pool2_3d, resample2): every case of misc_ref.RESAMPLE against ``fmdiff.runtime.ops``. The cases, their
fp64 references, lattices, bounds and guards live in misc_ref.py; test_misc_ref.py proves them on the CPU and shows
that the same checks reject the known mutants."""
import pytest

import misc_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = mr.case_ids(mr.RESAMPLE)


@pytest.fixture(scope="module", autouse=True)
def report_ratios():
    mr.RATIOS.clear()
    yield
    for fam, r in sorted(mr.RATIOS.items()):
        print(f"[misc_ref] {fam}: max err / bound {r:.3f}")


@pytest.mark.parametrize("family,case", IDS, ids=[f"{f}-{c}" for f, c in IDS])
def test_resample(family, case):
    from fmdiff.runtime import ops
    mr.CASES[family][case](ops, DEV)
