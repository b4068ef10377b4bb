"""SlotBook.plan_step: the streaming step of the keyed frame pool whose only new frame per sample is the window's newest -- the step's
slot table and, per sample, the slot that receives that frame (or -1).  Host only: no device, no library call."""
import copy

import pytest

from sparsebev_amd.cache import SlotBook


def state(book):
    return book.B, copy.deepcopy(book.slots), [(b, list(m)) for b, m in book.slots.items()], copy.deepcopy(book.needed)


def test_one_new_key_per_sample_gets_a_slot_and_the_table_points_at_it():
    book = SlotBook(3, 4)
    for b, k in book.missing([['a2', 'a1', 'a0'], ['b2', 'b1', 'b0']]):
        book.assign(b, k)
    rows, insert = book.plan_step([['a3', 'a2', 'a1'], ['b3', 'b2', 'b1']])
    assert all(0 <= s < 4 for s in insert)
    for b, row in enumerate(rows):
        assert row[0] == insert[b] and insert[b] not in row[1:]                  # the free fourth slot, not one the step reads
        assert row[1:] == [book.slots[b][k] for k in (['a2', 'a1'], ['b2', 'b1'])[b]]
    assert book.slots[0]['a3'] == insert[0] and book.slots[1]['b3'] == insert[1]
    assert book.table([['a3', 'a2', 'a1'], ['b3', 'b2', 'b1']]) == rows           # every key is resident now


def test_resident_newest_key_gives_minus_one():
    book = SlotBook(3, 4)
    rows0, insert0 = book.plan_step([['a0'] * 3, ['b0'] * 3])
    assert all(s >= 0 for s in insert0)
    rows, insert = book.plan_step([['a0'] * 3, ['b0'] * 3])                       # the same keys again: nothing to insert
    assert insert == [-1, -1] and rows == rows0
    rows, insert = book.plan_step([['a1', 'a0', 'a0'], ['b0'] * 3])               # one sample streams on, the other repeats
    assert insert[0] >= 0 and insert[1] == -1 and rows[0][0] == insert[0] and rows[1] == rows0[1]


def test_padded_window_of_one_unseen_key_passes():
    book = SlotBook(4, 6)
    rows, insert = book.plan_step([['s0f0'] * 4])
    assert insert == [rows[0][0]] and rows[0] == [insert[0]] * 4 and book.B == 1
    rows, insert = book.plan_step([['s0f1', 's0f0', 's0f0', 's0f0']])
    assert insert[0] == rows[0][0] != rows[0][1] == rows[0][2] == rows[0][3]
    # a scene change pads the window with the new scene's first frame
    rows, insert = book.plan_step([['s1f0'] * 4])
    assert insert[0] >= 0 and rows[0] == [insert[0]] * 4
    assert sorted(book.slots[0]) == ['s0f0', 's0f1', 's1f0']


def test_missing_key_that_is_not_the_newest_raises_and_leaves_the_book_unchanged():
    book = SlotBook(3, 3)
    book.plan_step([['a0'] * 3, ['b0'] * 3])
    book.plan_step([['a1', 'a0', 'a0'], ['b1', 'b0', 'b0']])
    before = state(book)
    # sample 0 is a proper step and would evict; sample 1 misses b2, which is not its newest key
    with pytest.raises(KeyError, match="sample 1: frame 'b2'"):
        book.plan_step([['a2', 'a1', 'a0'], ['b3', 'b2', 'b1']])
    assert state(book) == before
    with pytest.raises(KeyError, match="'a5'"):                                   # two unseen keys, the newest among them
        book.plan_step([['a6', 'a5', 'a1'], ['b1', 'b0', 'b0']])
    assert state(book) == before
    with pytest.raises(KeyError):                                                 # the newest resident, an older one not
        book.plan_step([['a1', 'a9', 'a0'], ['b1', 'b0', 'b0']])
    assert state(book) == before
    fresh = SlotBook(3, 3)
    with pytest.raises(KeyError):
        fresh.plan_step([['a1', 'a0', 'a0']])
    assert fresh.B is None and fresh.slots == {} and fresh.needed == {}
    # the shape errors of every announcement
    with pytest.raises(ValueError):
        book.plan_step([['a1', 'a0', 'a0']])
    with pytest.raises(ValueError):
        book.plan_step([['a1', 'a0'], ['b1', 'b0']])
    assert state(book) == before


def test_eviction_never_takes_a_slot_the_step_needs():
    T, n_slots = 3, 3
    book = SlotBook(T, n_slots)
    book.plan_step([['k0'] * 3])
    book.plan_step([['k1', 'k0', 'k0']])
    book.plan_step([['k2', 'k1', 'k0']])                                          # full: every slot holds a frame
    for i in range(3, 12):
        keys = [['k%d' % (i - t) for t in range(T)]]
        held = {k: s for k, s in book.slots[0].items()}
        rows, insert = book.plan_step(keys)
        assert insert[0] == held['k%d' % (i - 3)]                                 # the one frame the step does not read went
        assert rows[0][0] == insert[0] and rows[0][1:] == [held[k] for k in keys[0][1:]] and insert[0] not in rows[0][1:]
        assert len(set(rows[0])) == T
    # least recently used first where several could go; a hit refreshes a key
    book = SlotBook(2, 3)
    for keys in (['a', 'a'], ['b', 'a'], ['c', 'b']):
        book.plan_step([keys])
    book.plan_step([['c', 'a']])                                                  # all resident: a is used again
    held = dict(book.slots[0])
    rows, insert = book.plan_step([['d', 'c']])
    assert insert[0] == held['b'] and 'b' not in book.slots[0]


def test_fewer_slots_than_frames_with_duplicates():
    book = SlotBook(4, 2)
    rows, insert = book.plan_step([['a'] * 4])
    assert rows[0] == [insert[0]] * 4
    rows, insert = book.plan_step([['b', 'a', 'a', 'a']])
    assert insert[0] == rows[0][0] and rows[0][1] == rows[0][2] == rows[0][3] != rows[0][0]
    rows, insert = book.plan_step([['c', 'b', 'b', 'b']])                         # a leaves: the only slot the step does not need
    assert sorted(book.slots[0]) == ['b', 'c'] and rows[0][0] == insert[0] and len(set(rows[0])) == 2
    with pytest.raises(RuntimeError, match='3 distinct frames in one step, the pool has 2 slots'):
        book.plan_step([['d', 'c', 'b', 'b']])
    assert sorted(book.slots[0]) == ['b', 'c']


def test_drop_makes_the_next_step_an_insert_again():
    book = SlotBook(2, 4)
    book.plan_step([['x0', 'x0'], ['y0', 'y0']])
    assert book.plan_step([['x0', 'x0'], ['y0', 'y0']])[1] == [-1, -1]
    book.drop(1)
    rows, insert = book.plan_step([['x0', 'x0'], ['y0', 'y0']])
    assert insert[0] == -1 and insert[1] >= 0 and rows[1] == [insert[1]] * 2
    book.drop(0)
    with pytest.raises(KeyError, match="sample 0: frame 'x0'"):                   # after a drop the older frames are gone too
        book.plan_step([['x1', 'x0'], ['y1', 'y0']])


def test_plan_step_agrees_with_missing_assign_table():
    """the same stream through plan_step and through what FramePool.put does per step gives the same tables"""
    import random
    rnd = random.Random(3)
    T, n_slots, B = 4, 5, 3
    a, b = SlotBook(T, n_slots), SlotBook(T, n_slots)
    scene, frame = [0] * B, [0] * B
    for it in range(120):
        keys = []
        for s in range(B):
            if rnd.random() < 0.1:
                scene[s], frame[s] = scene[s] + 1, 0
            if rnd.random() < 0.15:
                frame[s] = max(frame[s] - 1, 0)                                   # a repeated step: nothing new for this sample
            keys.append([(scene[s], max(frame[s] - t, 0)) for t in range(T)])
            frame[s] += 1
        miss = b.missing(keys)
        want_insert = [-1] * B
        for s, k in miss:
            assert k == keys[s][0]
            want_insert[s] = b.assign(s, k)[0]
        want_rows = b.table(keys)
        rows, insert = a.plan_step(keys)
        assert rows == want_rows and insert == want_insert, it
