"""The keyed frame pool's bookkeeping (cache.SlotBook): key -> slot per sample, least-recently-used eviction that never takes a frame
the announced step needs, duplicates in a window, independent samples, the step's table as plain lists.  Host only: no device, no
library call."""
import pytest

from sparsebev_amd.cache import SlotBook


def step(book, keys):
    """what FramePool does per step, without the copies: announce, assign every miss, read the table"""
    miss = book.missing(keys)
    evicted = [book.assign(b, k)[1] for b, k in miss]
    return miss, evicted, book.table(keys)


def in_range(book, rows):
    return all(0 <= s < book.n_slots for row in rows for s in row)


def test_hits_misses_and_duplicates():
    book = SlotBook(4, 6)
    # first sample of a scene: the window is padded with repeats of the current frame -- ONE miss, one slot read four times
    miss, _, rows = step(book, [['a0'] * 4])
    assert miss == [(0, 'a0')] and rows == [[rows[0][0]] * 4] and in_range(book, rows)
    # second sample: one new frame, the old one still padding the tail
    miss, _, rows = step(book, [['a1', 'a0', 'a0', 'a0']])
    assert miss == [(0, 'a1')] and rows[0][1] == rows[0][2] == rows[0][3] != rows[0][0]
    # all hits: nothing to put, the same slots again
    assert book.missing([['a1', 'a0', 'a0', 'a0']]) == [] and book.table([['a1', 'a0', 'a0', 'a0']]) == rows
    # missing() lists a key once however often the window repeats it, in window order
    assert book.missing([['a3', 'a2', 'a2', 'a1']]) == [(0, 'a3'), (0, 'a2')]
    # a key that was never put is not silently mapped
    with pytest.raises(KeyError, match="'a3'"):
        book.table([['a3', 'a2', 'a2', 'a1']])


def test_lru_order_and_needed_keys_are_never_evicted():
    book = SlotBook(2, 3)
    seq = [['k1', 'k0'], ['k2', 'k1'], ['k3', 'k2'], ['k4', 'k3']]
    evictions = []
    for keys in seq:
        miss, ev, rows = step(book, [keys])
        evictions += [e for e in ev if e is not None]
        assert in_range(book, rows) and len(set(rows[0])) == 2
    assert evictions == ['k0', 'k1']                       # oldest first, one per step once the three slots are full
    assert sorted(book.slots[0]) == ['k2', 'k3', 'k4']
    # a hit refreshes a key: k2 is used again, so the next eviction takes k3 although k2 is older
    step(book, [['k4', 'k2']])
    _, ev, _ = step(book, [['k5', 'k4']])
    assert ev == ['k3']
    # every slot holds a frame this step needs except one: that one goes, whatever its age
    book = SlotBook(3, 3)
    step(book, [['a', 'b', 'c']])
    step(book, [['c', 'b', 'a']])                           # most recently used last: a (the window's oldest) is the LRU entry ...
    miss = book.missing([['d', 'a', 'b']])
    assert miss == [(0, 'd')]
    assert book.assign(0, 'd') == (book.slots[0]['d'], 'c')          # ... but a is needed: c goes
    assert book.table([['d', 'a', 'b']])[0][1:] == [book.slots[0]['a'], book.slots[0]['b']]


def test_scene_change_is_t_misses():
    book = SlotBook(4, 8)
    step(book, [['s0f3', 's0f2', 's0f1', 's0f0']])
    miss, ev, rows = step(book, [['s1f0'] * 4])            # new scene, first sample: padded by duplicates
    assert miss == [(0, 's1f0')] and ev == [None]
    miss, ev, rows = step(book, [['s1f3', 's1f2', 's1f1', 's1f0']])
    assert [k for _, k in miss] == ['s1f3', 's1f2', 's1f1'] and ev == [None, None, None]       # 8 slots: nothing evicted yet
    miss, ev, rows = step(book, [['s1f4', 's1f3', 's1f2', 's1f1']])
    assert ev == ['s0f0']                                  # the old scene's frames leave, oldest first
    assert in_range(book, rows) and len(set(rows[0])) == 4


def test_samples_are_independent_and_drop_forgets_a_stream():
    book = SlotBook(2, 2)
    miss, _, rows = step(book, [['x1', 'x0'], ['x1', 'x0']])          # the same keys in two samples are two entries
    assert miss == [(0, 'x1'), (0, 'x0'), (1, 'x1'), (1, 'x0')]
    # sample 1 changes scene, sample 0 streams on
    miss, ev, rows = step(book, [['x2', 'x1'], ['y0', 'y0']])
    assert miss == [(0, 'x2'), (1, 'y0')] and ev == ['x0', 'x0']
    assert sorted(book.slots[0]) == ['x1', 'x2'] and sorted(book.slots[1]) == ['x1', 'y0']
    assert rows[1][0] == rows[1][1]
    book.drop(1)
    assert book.missing([['x2', 'x1'], ['y0', 'y0']]) == [(1, 'y0')]
    assert 1 not in book.slots or book.slots[1] == {}
    # the batch size is fixed by the first step
    with pytest.raises(ValueError, match='B = 2'):
        book.missing([['x2', 'x1']])
    with pytest.raises(ValueError):
        book.assign(2, 'z')


def test_fewer_slots_than_frames_and_too_many_distinct_keys():
    book = SlotBook(3, 2)                                   # legal: duplicates make it meaningful
    miss, _, rows = step(book, [['b', 'a', 'a']])
    assert len(miss) == 2 and rows[0][1] == rows[0][2] and in_range(book, rows)
    with pytest.raises(RuntimeError, match='3 distinct frames in one step, the pool has 2 slots'):
        book.missing([['c', 'b', 'a']])
    with pytest.raises(RuntimeError, match='3 distinct'):
        book.table([['c', 'b', 'a']])
    with pytest.raises(ValueError):
        book.missing([['b', 'a']])                          # T entries per sample
    with pytest.raises(ValueError):
        SlotBook(17, 4)
    with pytest.raises(ValueError):
        SlotBook(4, 0)


def test_table_values_stay_in_range_over_a_long_mixed_stream():
    import random
    rnd = random.Random(7)
    T, n_slots, B = 4, 5, 3
    book = SlotBook(T, n_slots)
    scene, frame = [0] * B, [0] * B
    for it in range(200):
        keys = []
        for b in range(B):
            if rnd.random() < 0.1:
                scene[b], frame[b] = scene[b] + 1, 0
                if rnd.random() < 0.5:
                    book.drop(b)
            window = [(scene[b], max(frame[b] - t, 0)) for t in range(T)]          # first samples of a scene repeat frame 0
            keys.append(window)
            frame[b] += 1
        miss, _, rows = step(book, keys)
        assert in_range(book, rows) and [len(r) for r in rows] == [T] * B
        for b in range(B):
            assert len(book.slots[b]) <= n_slots
            assert sorted(set(book.slots[b].values())) == sorted(book.slots[b].values())        # one key per slot
            for t in range(T):                               # equal keys <-> equal slots
                for u in range(T):
                    assert (keys[b][t] == keys[b][u]) == (rows[b][t] == rows[b][u])
