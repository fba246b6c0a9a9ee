"""The ratio test on host threads (include/ultragroth_hip.h: ug_points_ratio_mask, device = -1; setup_host.hpp: Backend::ratio):
which of n pairs (X_i, Y_i) of G1 records have e(X_i, Q) != e(Y_i, G2)? Every expected mask is written down by construction in
zkey_locate_cases.py; test_gpu_points_ratio.py holds the device to the same answers."""
import pytest

import ultragroth_amd as ug
import zkey_locate_cases as LC


@pytest.mark.parametrize("case_id", LC.RATIO_IDS)
def test_ratio_masks_and_report(case_id):
    LC.check_ratio(case_id, -1)


def test_cases_cover_what_they_name():
    cases = LC.ratio_cases()
    assert set(cases) == set(LC.RATIO_IDS)
    x, y, q, max_blocks, wrong = cases["max-blocks-1-of-3-513"]
    rec, blk, rep = LC.expected(len(x), wrong, max_blocks)
    assert (rep["exact"], rep["resolved_blocks"], rep["bad_blocks"], rep["index"]) == (0, 1, 3, [1, 2]) and len(rec) == 256 and blk == b"\1\1\1"
    assert cases["q-is-g2-257"][2] == ug.generator_mul([1], g2=True, device=-1)[0]


def test_refusals():
    x, y, q = LC.honest(3)
    with pytest.raises(ug.SetupError, match="setup: q is the point at infinity"):
        ug.points_ratio_mask(list(x), list(y), bytes(128), device=-1)
    with pytest.raises(ug.SetupError, match="x and y differ in length"):
        ug.points_ratio_mask(list(x), list(y)[:2], q, device=-1)
    assert ug.points_ratio_mask([], [], q, device=-1) == (b"", b"", {"blocks": 0, "bad_blocks": 0, "resolved_blocks": 0, "exact": 1, "bad_records": 0, "index": []})
