"""The lock-step schedule of forward_test_batch (vfs_amd/labelprop.py batch_schedule) on its own: a pure host function, no backend.
Which video sits in which slot at which frame, and the descriptor rows the batched kernels read (include/vfs_hip.h)."""
import numpy as np
import pytest

from vfs_amd.labelprop import DESC_INTS, _key_frames, _ring_rows, batch_schedule, ring_position

# (lengths, nslots, precede, with_first, non_mask_len): nslots >, == and < the number of videos; lengths 2, 3 and > precede + 2
CASES = [
    ([2, 3, 7], 5, 2, True, 0),
    ([3, 2, 6], 3, 3, True, 1),
    ([2, 6, 3, 2, 9, 3], 2, 2, True, 0),
    ([5, 2, 2, 8], 1, 1, True, 1),
    ([4, 2, 7, 3, 3], 2, 2, False, 0),
    ([9, 2, 3, 12, 2, 5, 3], 3, 4, True, 1),
]


@pytest.mark.parametrize('lengths,nslots,precede,with_first,non_mask_len', CASES)
def test_batch_schedule(lengths, nslots, precede, with_first, non_mask_len):
    classes = [2 + 3 * v for v in range(len(lengths))]      # a different class count per video
    table, steps = batch_schedule(lengths, classes, nslots, precede, with_first, non_mask_len)
    assert table.dtype == np.int32 and table.shape == (len(steps), nslots, DESC_INTS)
    occupant = [None] * nslots      # the video of a slot
    frames = {v: [] for v in range(len(lengths))}      # the query frames a video was given, as (step, slot, frame)
    order, vacated = [], set()
    for i, (admitted, retired, nactive, most) in enumerate(steps):
        free = [n for n in range(nslots) if occupant[n] is None]
        for n, v in admitted:
            assert occupant[n] is None and not frames[v]
            occupant[n] = v
            order.append(v)
        # a freed slot is refilled at the next step: while videos wait, every slot vacated by the step before takes one
        waiting = len(lengths) - len(order)
        assert vacated <= {n for n, _ in admitted} or waiting == 0
        assert len(admitted) == len(free) or waiting == 0
        rows = table[i]
        active = [n for n in range(nslots) if rows[n, 0]]
        assert active == [n for n in range(nslots) if occupant[n] is not None] and 1 <= len(active) <= nslots
        assert nactive == len(active) and most == max(int(rows[n, 2]) for n in active)
        for n in range(nslots):
            if n not in active:
                assert not rows[n].any()
                continue
            v, f = occupant[n], len(frames[occupant[n]]) + 1
            keys = _key_frames(f, precede, with_first)
            assert tuple(rows[n, :6]) == (1, f, len(keys), non_mask_len, classes[v], f)      # [5]: the map position is the frame number
            assert rows[n, 8:8 + len(keys)].tolist() == keys and not rows[n, 6:8].any() and not rows[n, 8 + len(keys):].any()
            frames[v].append((i, n, f))
        vacated = {n for n, _ in retired}
        for n, v in retired:
            assert occupant[n] == v and frames[v][-1][2] == lengths[v] - 1
            occupant[n] = None
    assert order == list(range(len(lengths)))       # admitted in input order
    assert occupant == [None] * nslots              # every video retired
    for v, T in enumerate(lengths):                 # frames 1 .. T-1 exactly once, in order, in one slot, at consecutive steps
        assert [f for _, _, f in frames[v]] == list(range(1, T))
        assert len({n for _, n, _ in frames[v]}) == 1
        assert [i for i, _, _ in frames[v]] == list(range(frames[v][0][0], frames[v][0][0] + T - 1))


@pytest.mark.parametrize('lengths,nslots,precede,with_first,non_mask_len', CASES)
def test_ring_rows_change_the_bank_positions_only(lengths, nslots, precede, with_first, non_mask_len):
    """columns 1 (query frame) and 8.. (key frames) become ring positions; the map position (5) and everything else stay"""
    table, _ = batch_schedule(lengths, [2] * len(lengths), nslots, precede, with_first, non_mask_len)
    before = table.copy()
    rows = _ring_rows(table, precede)
    assert np.array_equal(table, before) and rows.dtype == table.dtype and rows.shape == table.shape
    assert np.array_equal(rows[..., 0], table[..., 0]) and np.array_equal(rows[..., 2:8], table[..., 2:8])
    active = table[..., 0] == 1
    assert np.array_equal(rows[..., 5][active], table[..., 1][active]) and not rows[..., 5][~active].any()
    assert np.array_equal(rows[..., 1], ring_position(table[..., 1], precede))
    assert np.array_equal(rows[..., 8:], ring_position(table[..., 8:], precede))
    assert rows[..., 1].max() <= precede + 1 and rows[..., 8:].max() <= precede + 1
    if max(lengths) > precede + 2:      # a ring wraps: positions and frame numbers differ somewhere
        assert (rows[..., 1] != rows[..., 5]).any()


def test_batch_schedule_of_no_videos():
    table, steps = batch_schedule([], [], 2, 2, True, 0)
    assert table.shape == (0, 2, DESC_INTS) and steps == []


def test_key_frames():
    """frame 0 is listed twice while f <= precede (as the reference does); non_mask_len must leave a key frame under the mask"""
    assert _key_frames(1, 2, True) == [0, 0]
    assert _key_frames(2, 2, True) == [0, 0, 1]
    assert _key_frames(3, 2, True) == [0, 1, 2]
    assert _key_frames(5, 2, True) == [0, 3, 4]
    assert _key_frames(1, 2, False) == [0] and _key_frames(5, 2, False) == [3, 4]
    assert _key_frames(1, 2, True, 1) == [0, 0]
    with pytest.raises(AssertionError):
        _key_frames(1, 2, False, 1)
