"""The rotated-form sequence of the grouped partial rounds (csrc/poseidon_mx.cuh, grp::step): a wave of four sets,
modelled lane by lane on exact integers -- rotated operand reads, the merge by lane group, one recombination, sigma
written back in place, the previous group's sigmas left in bsig -- against the plain Poseidon rounds.  No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_rotated_groups_equal_plain_rounds():
    import poseidon_group_model as m
    assert m.check_rotated()


@pytest.mark.parametrize("drop", ["rows", "kblocks"])
def test_rotated_model_fails_without_either_rotation(monkeypatch, drop):
    """the comparison above has teeth: reading the operands without the row rotation (forms land in the wrong lane
    group) or without the k-block rotation (sigmas meet the wrong coefficients) breaks it"""
    import poseidon_group_model as m
    rot = m.rot_lane
    if drop == "rows":
        monkeypatch.setattr(m, "rot_lane", lambda lane, s, rows, kbs: rot(lane, s, False, kbs))
    else:
        monkeypatch.setattr(m, "rot_lane", lambda lane, s, rows, kbs: rot(lane, s, rows, False))
    with pytest.raises(AssertionError):
        m.check_rotated()
