"""The ratio test on the device (ratio_block_sums_kernel of setup_points.hip, ratio_judge_kernel of pairing.hip, through
ug_points_ratio_mask): the masks and reports zkey_locate_cases.py fixes in advance, and the host twin's on the same inputs."""
import pytest

import ultragroth_amd as ug
import zkey_locate_cases as LC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case_id", LC.RATIO_IDS)
def test_ratio_masks_and_report(case_id):
    LC.check_ratio(case_id, 0)


@pytest.mark.parametrize("case_id", ("infinities-513", "max-blocks-1-of-3-513", "plus-minus-in-one-block-257"))
def test_device_against_host(case_id):
    x, y, q, max_blocks, _ = LC.ratio_cases()[case_id]
    timing = []
    dev = ug.points_ratio_mask(list(x), list(y), q, device=0, max_blocks=max_blocks, timing=timing)
    assert dev == ug.points_ratio_mask(list(x), list(y), q, device=-1, max_blocks=max_blocks)
    assert timing[0][0] > 0 and timing[0][1] > 0          # both kernels ran
