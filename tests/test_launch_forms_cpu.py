"""The thresholds in tests/launch_forms.py are the ones in the source, and every size listed there still passes its threshold:
a retune of a grid cap or a tile size fails here, so the large GPU cases cannot quietly stop covering the second trips, tails
and template instantiations they were written for."""
import os
import re

import pytest

import launch_forms as LF
from conftest import ROOT


@pytest.mark.parametrize("name", sorted(LF.THRESHOLDS))
def test_threshold_is_the_one_in_the_source(name):
    path, pattern, value = LF.THRESHOLDS[name]
    with open(os.path.join(ROOT, path)) as f:
        text = f.read()
    found = re.findall(pattern, text)
    assert len(found) == 1, (f"{name}: {len(found)} matches of {pattern!r} in {path} "
                             "(the launch code changed: revisit tests/launch_forms.py)")
    assert int(found[0]) == value, f"{name} is {found[0]} in {path}, the GPU cases were sized for {value}"


def test_every_listed_size_passes_its_threshold():
    checks = LF.coverage()
    assert len(checks) >= 25
    for what, above, threshold in checks:
        assert above > threshold, f"{what}: {above} does not exceed {threshold}"


def test_score_shapes_reach_every_template_and_lds_layout():
    tiles = {(c + 15) // 16 for c, _ in LF.SCORE_SHAPES}
    assert tiles == {1, 2, 3, 4}
    padded = {(f + 15) // 16 * 16 for _, f in LF.SCORE_SHAPES}
    assert {64, 128, 192, 256} <= padded                      # the swizzled layouts
    assert (64, 256) in LF.SCORE_SHAPES                        # 64 KB of LDS
    assert any(f % 4 == 0 for _, f in LF.SCORE_SHAPES) and any(f % 4 for _, f in LF.SCORE_SHAPES)


def test_gcn_bwd_shapes_reach_the_partial_groups():
    assert any((h * w) % 32 for h, w in LF.GCN_BWD_SHAPES) and any((h * w) % 32 == 0 for h, w in LF.GCN_BWD_SHAPES)
    assert min(h for h, _ in LF.GCN_BWD_SHAPES) < 8 and max(h for h, _ in LF.GCN_BWD_SHAPES) == LF.T["GCN_BWD_MAX_HIDDEN"]
    assert {lanes for _, _, lanes in LF.GCN_BWD_OPERATORS} == {8, 16, 32}
