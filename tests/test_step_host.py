"""The host side of a decoder step that needs no device: utils.frame_source (the one reading of "where do a step's frames live") and
runtime.StepBook (StepGraphs' admission policy: first sightings, least-recently-used eviction, the brake on address-keyed graphs that are
never replayed).  The policy tests restate on the host what tests/test_gpu_stepgraph.py asserts on the device, with fake graphs."""
import warnings

import pytest
import torch

from sparsebev_amd.runtime import CAPTURE, EAGER, REPLAY, SIGHTED, CapturedStep, StepBook, StepKey
from sparsebev_amd.utils import FrameSource, frame_source, slot_resident


# ---- frame_source --------------------------------------------------------------------------------------------------------------------

class Dense:
    def __init__(self):
        self.levels, self.B, self.T = [torch.zeros(2 * 3 * 6, 4, 4, 8)], 2, 3


class Ring(Dense):
    def __init__(self):
        super().__init__()
        self.frame_slots, self.n_slots = [2, 0, 3], 4


class Pool(Dense):
    def __init__(self):
        super().__init__()
        self.slot_table, self.n_slots = torch.zeros(2, 3, dtype=torch.int32), 5


def test_frame_source_names_the_four_kinds():
    assert frame_source([torch.zeros(2, 18, 8, 4, 4)]) == FrameSource('list', (), None, 0)
    assert frame_source(Dense()) == FrameSource('dense', (), None, 0)
    assert frame_source(Ring()) == FrameSource('ring', (2, 0, 3), None, 4)
    pool = Pool()
    src = frame_source(pool)
    assert src.kind == 'pool' and src.slot_table is pool.slot_table and src.frame_slots == () and src.n_slots == 5
    both = Pool()
    both.frame_slots = [0, 1, 2]
    with pytest.raises(RuntimeError, match='not both'):
        frame_source(both)
    for feats, resident in ((Ring(), True), (pool, True), (Dense(), False), ([torch.zeros(1)], False), ([], False), (object(), False)):
        assert slot_resident(feats) is resident and frame_source(feats).resident is resident
    assert frame_source([]).kind == 'list' and frame_source(object()).kind == 'list'


def test_the_pool_table_is_validated_where_a_shape_is_given():
    pool = Pool()                                             # a host table: named, but refused as soon as a step would read it
    with pytest.raises(RuntimeError, match=r'the decoder: slot_table must be a contiguous device int32 \[B, T\] = \[2, 3\]'):
        frame_source(pool, (2, 3), 'the decoder')
    with pytest.raises(RuntimeError, match=r'sample_mix: slot_table must be a contiguous device int32 \[B, T\]'):
        FrameSource.of(slot_table=[[0, 1, 2]], n_slots=4, shape=(1, 3), what='sample_mix')
    with pytest.raises(RuntimeError, match='slot_table must be'):          # no mapping where the caller means the pool
        FrameSource.of(n_slots=4, shape=(1, 3), plain=None)
    assert FrameSource.of(n_slots=4, shape=(1, 3)) == FrameSource('dense')
    assert frame_source(Ring(), (2, 3)).kind == 'ring'        # (nothing of the ring's to validate here)


# ---- StepBook ------------------------------------------------------------------------------------------------------------------------

class Graph:
    def __init__(self):
        self.launches, self.alive = 0, True

    def replay(self):
        assert self.alive
        self.launches += 1

    def destroy(self):
        self.alive = False


class Host:
    """what StepGraphs.run does around its book, without a device: ask, capture when told to, launch"""

    def __init__(self):
        self.sig, self.released = ('w0',), []
        self.book = StepBook(lambda: self.sig, self.released.append)
        assert (self.book.MAX, self.book.MAX_WASTED, self.book.RETRY_EVERY) == (8, 3, 64)

    def key(self, name):
        return StepKey((1, 4, 10), (1, 4, 256), name, None, self.sig, 0, (), 6, (), 0, False)

    def call(self, name, ident=(), pinned=False):
        key = self.key(name)
        verdict, e = self.book.admit(key, list(ident), pinned)
        assert (e is None) == (verdict in (EAGER, SIGHTED))
        if verdict == CAPTURE:
            e = CapturedStep(Graph(), pinned)
            self.book.captured(key, e)
        if verdict in (CAPTURE, REPLAY):
            self.book.launch(key, e)
        assert self.book.wasted >= 0 and len(self.book.entries) <= self.book.MAX
        return verdict

    def captured(self, name, ident=(), pinned=False):
        """seen, then captured; never replayed afterwards unless the test calls again"""
        assert [self.call(name, ident, pinned) for _ in range(2)] == [SIGHTED, CAPTURE]
        return self.book.entries[self.key(name)]

    def thrash(self, n, start=0):
        """n address-keyed captures over buffers that never come back"""
        return [self.captured(('nhwc', start + i), [torch.zeros(4)], pinned=True) for i in range(n)]


def test_second_call_captures_third_replays():
    h = Host()
    assert [h.call('a') for _ in range(4)] == [SIGHTED, CAPTURE, REPLAY, REPLAY]
    e = h.book.entries[h.key('a')]
    assert h.book.captures == 1 and h.book.replays == 3 and e.replays == 2 and e.graph.launches == 3      # (the entry's count leaves the capturing call's own launch out)
    buf = torch.zeros(8)
    assert [h.call('b', [buf[:4]], pinned=True) for _ in range(3)] == [SIGHTED, CAPTURE, REPLAY]      # new views of the same memory are the same input
    h.book.clear()
    assert not e.graph.alive and not h.book.entries and len(h.released) == 2


def test_a_recycled_identity_is_a_new_first_sighting():
    h = Host()
    t = torch.zeros(4)
    assert h.call('a', [t], pinned=True) == SIGHTED
    del t
    u = torch.zeros(4)                                        # another tensor under the same key (on a device: the freed address handed out again)
    assert [h.call('a', [u], pinned=True) for _ in range(2)] == [SIGHTED, CAPTURE]
    assert h.book.captures == 1


def test_the_ninth_key_evicts_the_least_recently_used():
    h = Host()
    steps = [h.captured(i) for i in range(8)]
    assert h.call(0) == REPLAY                                # key 0 is the most recently used now, key 1 the least
    assert h.call(8) == SIGHTED
    assert h.key(1) not in h.book.entries and not steps[1].graph.alive and h.released == [steps[1]]
    assert h.key(0) in h.book.entries and all(s.graph.alive for s in steps[:1] + steps[2:]) and len(h.book.entries) == 8
    assert h.book.wasted == 0                                 # (staged graphs are never counted, replayed or not)
    assert h.call(1) == SIGHTED and h.key(2) not in h.book.entries      # the evicted key starts over, at the cost of the next one


def test_three_never_replayed_address_keyed_captures_hold_the_brake_and_warn_once():
    h = Host()
    h.thrash(3)
    assert h.book._unproven() == 3 and h.book.wasted == 0
    t = torch.zeros(4)
    with pytest.warns(UserWarning, match='3 step graphs keyed on input addresses were captured and never replayed'):
        assert h.call('more', [t], pinned=True) == EAGER
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert h.call('more', [t], pinned=True) == EAGER and h.call('other', [t], pinned=True) == EAGER
    assert h.book.captures == 3 and h.key('more') not in h.book.entries
    # staged and slot-resident keys are never refused
    assert [h.call('nchw') for _ in range(3)] == [SIGHTED, CAPTURE, REPLAY]
    # a replay of an address-keyed graph shows that the caller does bring buffers back: evicted ones are forgiven
    h.book.wasted = 2
    assert h.call(('nhwc', 0), pinned=True) == REPLAY and h.book.wasted == 0


def test_every_64th_refused_call_allows_one_probe_capture():
    h = Host()
    hold = h.thrash(3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in range(3, 203):                               # the caller goes on bringing new buffers, two calls each
            t = torch.zeros(4)
            hold.append(t)
            before = h.book.captures
            verdicts = [h.call(('nhwc', i), [t], pinned=True) for _ in range(2)]
            assert verdicts in ([EAGER, EAGER], [EAGER, SIGHTED], [SIGHTED, CAPTURE])
            assert h.book.captures - before == (verdicts[1] == CAPTURE)
    assert h.book._refused >= 3 * 64 and h.book.captures == 3 + h.book._refused // 64
    # the same with nothing left alive to forgive: the counter itself gives one back, and stops at zero
    h = Host()
    h.book.wasted, h.book._refused = 3, 63
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert h.call('x', pinned=True) == EAGER and h.book.wasted == 2
        assert h.call('x', pinned=True) == SIGHTED


def test_an_entry_of_an_older_weight_signature_is_not_counted_as_wasted():
    for update in (False, True):
        h = Host()
        old = h.thrash(1)[0]
        if update:
            h.sig = ('w1',)                                   # an optimizer step: the old graph can never be hit again
        assert h.book._unproven() == (0 if update else 1)
        for i in range(8):                                    # eight newer keys push it out
            h.call(i)
        assert not old.graph.alive and h.released == [old]
        assert h.book.wasted == (0 if update else 1)
