"""The two host-side helpers of the rollout drivers that hold a rule (psketch_amd/rollout.py):
_cut_episodes, which turns a pass's per-tick records into per-episode results, and _specs_array,
which normalises a pass's `specs`.  Pure numpy and host torch: no simulator."""
import numpy as np
import pytest
import torch

from psketch_amd.rollout import _cut_episodes, _pose_xyd, _specs_array


def _word(x, y, d):
    return x | y << 8 | d << 16


def _records(ticks, n):
    return (np.full((ticks, n), -1, dtype=np.int32), np.full((ticks, n), -1, dtype=np.int32),
            np.full((ticks, n), -1, dtype=np.int8))


def test_pose_xyd():
    assert _pose_xyd(np.int32(_word(11, 200, 3))) == (11, 200, 3)
    x, y, d = _pose_xyd(np.asarray([_word(0, 255, 0), _word(255, 0, 2)], dtype=np.int32))
    assert (x.tolist(), y.tolist(), d.tolist()) == ([0, 255], [255, 0], [0, 2])


def test_cut_episodes():
    """n = 2, count = 5: slot 0 runs episodes 0, 2, 4 and slot 1 runs 1, 3.  Slot 0 ends episode 0
    at tick 0 and episode 2 at tick 1 (two ends on consecutive ticks); slot 1 ends episode 1 at
    tick 2; episodes 3 and 4 are still running when the records stop."""
    n, count, T, ticks = 2, 5, 4, 4
    ended, pose, succ = _records(ticks, n)
    rec = np.asarray([[5, 0], [5, 1], [2, 3], [1, 4]], dtype=np.int32)
    ended[0, 0], pose[0, 0], succ[0, 0] = 0, _word(1, 2, 3), 1
    ended[1, 0], pose[1, 0], succ[1, 0] = 2, _word(7, 200, 0), 0
    ended[2, 1], pose[2, 1], succ[2, 1] = 1, _word(255, 9, 2), -1
    length, success, end_pose, seqs = _cut_episodes(ended, pose, succ, count, rec, T)
    assert length.dtype == np.int32 and length.tolist() == [1, 3, 1, 0, 0]
    assert seqs.dtype == np.int32 and seqs.shape == (count, T)
    assert seqs[0].tolist() == [5, -1, -1, -1]
    assert seqs[1].tolist() == [0, 1, 3, -1]
    assert seqs[2].tolist() == [5, -1, -1, -1]
    assert seqs[3].tolist() == [-1, -1, -1, -1]           # never ended: nothing of its ticks kept
    assert seqs[4].tolist() == [-1, -1, -1, -1]
    assert success.dtype == np.int8 and success.tolist() == [1, -1, 0, -2, -2]
    assert success[3] == -2
    assert end_pose.dtype == np.int32
    assert end_pose.tolist() == [[1, 2, 3], [255, 9, 2], [7, 200, 0], [0, 0, 0], [0, 0, 0]]
    # without the action records: the same cut, no table
    length2, success2, end_pose2, none = _cut_episodes(ended, pose, succ, count)
    assert none is None
    assert length2.tolist() == length.tolist()
    assert success2.tolist() == success.tolist() and end_pose2.tolist() == end_pose.tolist()


def test_cut_episodes_drops_padding():
    """n = 3, count = 2: row 2 is the copy of row 0 that pads the split.  Its end leaves no trace,
    not even on row 0, and the episodes after it in its slot would still be cut at it."""
    n, count, T, ticks = 3, 2, 3, 3
    ended, pose, succ = _records(ticks, n)
    rec = np.asarray([[0, 1, 5], [2, 5, -1], [5, -1, -1]], dtype=np.int32)
    ended[0, 2], pose[0, 2], succ[0, 2] = 2, _word(9, 9, 1), 1
    ended[1, 1], pose[1, 1], succ[1, 1] = 1, _word(4, 5, 2), 0
    ended[2, 0], pose[2, 0], succ[2, 0] = 0, _word(6, 7, 0), 1
    length, success, end_pose, seqs = _cut_episodes(ended, pose, succ, count, rec, T)
    assert length.shape == (count,) and length.tolist() == [3, 2]
    assert seqs.shape == (count, T)
    assert seqs.tolist() == [[0, 2, 5], [1, 5, -1]]
    assert success.tolist() == [1, 0]
    assert end_pose.tolist() == [[6, 7, 0], [4, 5, 2]]
    assert _cut_episodes(ended, pose, succ, count)[0].tolist() == [3, 2]


def test_specs_array_forms_agree():
    rows = np.asarray([[3, 1, 2, 0, 7], [4, 5, 6, 1, 8], [9, 0, 0, 3, 2]], dtype=np.int64)
    want = rows.astype(np.int32)
    for given in (tuple(rows[:, k] for k in range(5)),                    # Dataset.specs' 5-tuple
                  [rows[:, k].tolist() for k in range(5)],                # ... as lists
                  tuple(torch.as_tensor(rows[:, k]) for k in range(5)),   # ... as host tensors
                  rows, rows.tolist(), torch.as_tensor(rows),
                  np.asfortranarray(rows)):
        got = _specs_array(given)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32
        assert got.flags["C_CONTIGUOUS"] and got.shape == (3, 5)
        assert (got == want).all()
    # five rows in an array are rows; a list of five sequences is the 5-tuple (its columns)
    five = np.arange(25).reshape(5, 5)
    assert (_specs_array(five) == five).all()
    assert (_specs_array(five.tolist()) == five.T).all()


@pytest.mark.parametrize("bad", [np.zeros((0, 5), dtype=np.int32), np.zeros((3, 4), dtype=np.int32),
                                 np.arange(5), torch.zeros((0, 5), dtype=torch.int32)])
def test_specs_array_rejects(bad):
    with pytest.raises(ValueError, match=r"^specs must be \[count >= 1, 5\]$"):
        _specs_array(bad)
