"""Online (streaming) per-frame feature caches -- SURVEY.md section 8f rank 2: the positional ring (FrameFeatureCache) and the keyed
frame pool (FramePool).

The reference's published FPS is measured in online mode: features of past frames are cached per frame and only
the 6 new images go through the backbone (models/sparsebev.py:255-321) -- but every step it still ``torch.cat``s
all T cached frames (:297-303) and the decoder then regroup-copies them again (models/sparsebev_transformer.py:
73-85).  Here each level is ONE resident channels-last buffer ``[B, n_slots, 6, H, W, C]``; a new frame is
relayouted (NCHW -> NHWC, one launch per level) straight into the slot of the evicted frame and the sampler reads
logical frame t through a slot table (``sbev_msmv_fwd_ring``), so nothing older than the newest frame is ever moved.

The ring has ONE slot order for the whole batch, passed to the kernels by value.  The pool keeps the same buffers but finds frames by
key, per sample, through a device table the kernels read (``sbev_msmv_fwd_pool``): what the reference's file-name keyed cache does
(duplicates in a window, scene changes as plain misses), for a batch of independent streams, with one captured graph per shape.
"""
import ctypes

import torch

from . import _lib, ops
from .utils import FrameInsert

N_VIEWS = 6


def _store_level(f, dsts, storage):
    """One level of a new frame into resident slots: f [n, 6, C, H, W] (sample i -> dsts[i], a contiguous [6, H, W, C] slot view of
    ``storage`` type).  fp32 NCHW memory is relayouted by the transpose kernel; channels-last memory (what a channels_last conv stack
    emits; fp32 / fp16 / bf16) is already in the slot's layout and only copied (and widened); a 2-byte slot takes frames of its own
    type only, moved as bytes.  Shared by FrameFeatureCache.push and FramePool.put."""
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = len(dsts)
    if storage != torch.float32:                        # 2-byte ring: frames of the ring's own type only, moved as bytes
        if f.dtype != storage:
            raise RuntimeError('a %s ring takes %s frames only (got %s)' % (storage, storage, f.dtype))
        if f.stride(2) == 1 and f[0].is_contiguous(memory_format=torch.channels_last):
            for b in range(n):
                dsts[b].copy_(f[b].permute(0, 2, 3, 1))      # both sides contiguous [6, H, W, C]: a device memcpy
        else:
            f = f.contiguous()
            C, H, W = f.shape[2:]
            for b in range(n):
                st = lib.sbev_nchw_to_nhwc_b16(ctypes.c_void_p(f[b].data_ptr()), ctypes.c_void_p(dsts[b].data_ptr()),
                                               N_VIEWS, C, H * W, stream)
                _lib.check(st, 'sbev_nchw_to_nhwc_b16')
        return
    if f.stride(2) == 1 and f[0].is_contiguous(memory_format=torch.channels_last):      # NHWC memory: zero relayout
        code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}.get(f.dtype)
        if code is None:
            raise RuntimeError('channels-last frame features must be fp32 / fp16 / bf16')
        for b in range(n):          # f[b] is one contiguous [6, H, W, C] run in memory; so is dsts[b]
            st = lib.sbev_copy_widen_f32(ctypes.c_void_p(f[b].data_ptr()), code, ctypes.c_void_p(dsts[b].data_ptr()),
                                         dsts[b].numel(), stream)
            _lib.check(st, 'sbev_copy_widen_f32')
        return
    if f.dtype != torch.float32:
        raise RuntimeError('NCHW frame features must be fp32 (channels-last inputs may be fp16 / bf16)')
    f = f.contiguous()
    C, H, W = f.shape[2:]
    for b in range(n):
        st = lib.sbev_nchw_to_nhwc_f32(ctypes.c_void_p(f[b].data_ptr()), ctypes.c_void_p(dsts[b].data_ptr()),
                                       N_VIEWS, C, H * W, stream)
        _lib.check(st, 'sbev_nchw_to_nhwc_f32')


class FrameFeatureCache:
    """``dtype``: the ring's STORAGE type.  fp32 (default) takes fp32 NCHW frames and channels-last fp32 / fp16 / bf16 frames (widened);
    ``torch.float16`` / ``torch.bfloat16`` keep an fp16 backbone's / a bf16 neck's frames as they are (half the memory and the relayout
    traffic; the sampler widens a tap exactly) and take frames of that type only, NCHW (2-byte relayout) or channels-last (copied)."""

    def __init__(self, num_frames, n_slots=None, dtype=torch.float32):
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError('ring storage must be fp32, fp16 or bf16')
        self.dtype = dtype
        self.T = num_frames
        self.n_slots = n_slots or num_frames
        if not self.T <= self.n_slots <= 16:
            raise ValueError('need num_frames <= n_slots <= 16 (the reference evicts its cache at 16 frames)')
        self.buffers = None            # list[L] of [B, n_slots, 6, H, W, C]
        self.order = []                # physical slots, newest first
        self.B = None

    def _alloc(self, frame_feats):
        f0 = frame_feats[0]
        self.B = f0.shape[0]
        self.buffers = [torch.empty(self.B, self.n_slots, N_VIEWS, f.shape[3], f.shape[4], f.shape[2], device=f.device, dtype=self.dtype)
                        for f in frame_feats]

    def push(self, frame_feats):
        """frame_feats: list[L] of [B, 6, C, H_l, W_l] device tensors = the neck's output for the 6 NEW images.
        fp32 NCHW memory is relayouted by the transpose kernel; channels-last memory (what a channels_last conv stack
        emits; fp32 / fp16 / bf16) is already in the ring's layout and only copied (and widened) into its slot."""
        if self.buffers is None:
            self._alloc(frame_feats)
        slot = len(self.order) if len(self.order) < self.n_slots else self.order.pop()      # free slot, else evict the oldest
        for f, buf in zip(frame_feats, self.buffers):
            if not f.is_cuda or f.shape[0] != self.B or f.shape[1] != N_VIEWS:
                raise RuntimeError('frame features must be device tensors [B, 6, C, H, W]')
            _store_level(f, [buf[b, slot] for b in range(self.B)], self.dtype)
        self.order.insert(0, slot)
        del self.order[self.n_slots:]

    def pyramid(self):
        """View of the newest T frames for the decoder (drop-in for transformer.FeaturePyramid)."""
        if len(self.order) < self.T:
            raise RuntimeError('only %d of %d frames cached' % (len(self.order), self.T))
        return RingPyramid(self)


class _SlotPyramid:
    """What the ring's and the pool's view of a step share: every level's resident buffer as [B*n_slots*6, H, W, G*C].  The subclasses
    add the slot mapping, which is also what utils.frame_source tells them apart by."""

    def __init__(self, owner):
        self.B, self.T = owner.B, owner.T
        self.n_slots = owner.n_slots
        self.levels = [b.reshape(owner.B * owner.n_slots * N_VIEWS, b.shape[3], b.shape[4], b.shape[5]) for b in owner.buffers]
        self.GC = owner.buffers[0].shape[-1]
        self.copied = 0


class RingPyramid(_SlotPyramid):
    def __init__(self, cache):
        super().__init__(cache)
        self.frame_slots = list(cache.order[:cache.T])

    def sample(self, loc, w_bp, T, G):
        return ops.msmv_sampling_ring(self.levels, self.B, T, G, self.frame_slots, self.n_slots, loc, w_bp)


class SlotBook:
    """The keyed frame pool's bookkeeping, host only (no torch, no device): per sample a map key -> slot in least-recently-used order,
    the keys the current step needs, and the step's table (b, t) -> slot as a plain list of lists.  The counterpart of the reference's
    file-name keyed cache (models/sparsebev.py:255-321), per sample instead of per process."""

    def __init__(self, num_frames, n_slots):
        if not 1 <= num_frames <= 16 or not 1 <= n_slots <= 16:
            raise ValueError('need 1 <= num_frames <= 16 and 1 <= n_slots <= 16 (the reference evicts its cache at 16 frames)')
        self.T, self.n_slots = num_frames, n_slots
        self.B = None
        self.slots = {}                # b -> {key: slot}, insertion order = least recently used first
        self.needed = {}               # b -> the distinct keys of the step last announced (missing / table)

    def _announce(self, keys):
        """keys[b][t] of one step -> per sample its distinct keys in window order; validates the shape and what fits"""
        keys = [list(row) for row in keys]
        if not keys or any(len(row) != self.T for row in keys):
            raise ValueError('keys must be [B][T] with T = %d' % self.T)
        if self.B is None:
            self.B = len(keys)
        if len(keys) != self.B:
            raise ValueError('this pool serves B = %d samples, got keys for %d' % (self.B, len(keys)))
        for b, row in enumerate(keys):
            distinct = list(dict.fromkeys(row))
            if len(distinct) > self.n_slots:
                raise RuntimeError('sample %d needs %d distinct frames in one step, the pool has %d slots' % (b, len(distinct), self.n_slots))
            self.needed[b] = distinct
        return keys

    def missing(self, keys):
        """The distinct (b, key) pairs of this step that are not resident, in (b, t) order: what the caller has to put()."""
        self._announce(keys)
        return [(b, k) for b in range(self.B) for k in self.needed[b] if k not in self.slots.get(b, {})]

    def assign(self, b, key):
        """(slot, evicted key or None) for ``key`` of sample b: its own slot if resident, else a free one, else the least recently used
        one whose key the announced step does not need."""
        if self.B is None or not 0 <= b < self.B:
            raise ValueError('sample index %r outside the pool (announce the step with missing(keys) first)' % (b,))
        mine = self.slots.setdefault(b, {})
        if key in mine:
            slot = mine.pop(key)
            mine[key] = slot           # most recently used last
            return slot, None
        evicted = None
        if len(mine) < self.n_slots:
            slot = next(s for s in range(self.n_slots) if s not in set(mine.values()))
        else:
            need = set(self.needed.get(b, ()))
            evicted = next((k for k in mine if k not in need), None)
            if evicted is None:
                raise RuntimeError('sample %d: every one of the %d slots holds a frame this step needs' % (b, self.n_slots))
            slot = mine.pop(evicted)
        mine[key] = slot
        return slot, evicted

    def table(self, keys):
        """[B][T] slots of this step (every key must be resident); marks them most recently used, the window's newest frame last."""
        keys = self._announce(keys)
        rows = []
        for b, row in enumerate(keys):
            mine = self.slots.get(b, {})
            absent = [k for k in self.needed[b] if k not in mine]
            if absent:
                raise KeyError('sample %d: frame %r is not in the pool (missing(keys) lists what to put() first)' % (b, absent[0]))
            for k in reversed(self.needed[b]):
                mine[k] = mine.pop(k)
            rows.append([mine[k] for k in row])
            assert all(0 <= s < self.n_slots for s in rows[-1])
        return rows

    def plan_step(self, keys):
        """(rows, insert) of a streaming step whose only new frame per sample is the window's newest: ``plan_frames(keys, [0])`` with its
        one insert row unwrapped -- per sample the slot that receives ``keys[b][0]``, or -1 when that frame is resident."""
        rows, insert = self.plan_frames(keys, [0])
        return rows, insert[0]

    def plan_frames(self, keys, offered):
        """(rows, insert) of a streaming step that brings the frames of the window positions ``offered`` (any iterable of t; the caller
        has frame ``keys[b][t]`` for every sample at each of them): the step's [B][T] slot table (as ``table``) and ``insert[k][b]`` for
        the offered positions in ascending t -- the slot that receives sample b's frame of position k, or -1.  A key that is missing and
        offered gets a slot by ``assign``'s rules, at the lowest offered t that carries it and nowhere else (a key at several positions
        is inserted once), in the order ``missing`` lists them; everything else is -1, so two live entries of one sample never share a
        slot and no key the step needs is evicted.  A missing key that is not offered raises the KeyError of ``table``; any exception
        leaves the book as it was."""
        saved = (self.B, {b: dict(m) for b, m in self.slots.items()}, {b: list(k) for b, k in self.needed.items()})
        try:
            keys = self._announce(keys)
            ts = sorted(set(offered))
            if not ts or not all(isinstance(t, int) and 0 <= t < self.T for t in ts):
                raise ValueError('offered window positions must be integers in [0, %d), at least one (got %r)' % (self.T, ts))
            insert = [[-1] * self.B for _ in ts]
            for b, row in enumerate(keys):
                mine = self.slots.get(b, {})
                absent = [k for k in self.needed[b] if k not in mine]
                first = {k: next((i for i, t in enumerate(ts) if row[t] == k), None) for k in absent}
                late = [k for k in absent if first[k] is None]
                if late:
                    raise KeyError('sample %d: frame %r is not in the pool and none of the offered positions %r carries it (missing(keys) lists what to put() first)'
                                   % (b, late[0], ts))
                for k in absent:
                    insert[first[k]][b] = self.assign(b, k)[0]
            return self.table(keys), insert
        except BaseException:
            self.B, self.slots, self.needed = saved
            raise

    def drop(self, b):
        """Forget sample b's stream (its slots are free again)."""
        self.slots.pop(b, None)
        self.needed.pop(b, None)


class FramePool:
    """Keyed frame pool: the ring's resident buffers ``[B, n_slots, 6, H, W, C]`` per level, addressed by KEY per sample instead of by
    ring position for the whole batch.  Per step: ``missing(keys)`` -> ``put(b, key, feats)`` for each pair -> ``pyramid(keys)``.  The
    step's mapping (b, t) -> slot lives in ONE persistent device int32 table ``[B, T]`` that the sampler kernels read
    (``sbev_msmv_fwd_pool``); ``pyramid`` refreshes its contents in place, so a captured decoder step replays for every phase, scene
    change and mix of streams.  A frame that appears twice in a window is one slot read twice; eviction is per sample, least recently
    used, never a frame the announced step needs.  ``dtype``: the slots' storage type, as for FrameFeatureCache.

    The streaming step -- one new frame per sample, the window's newest -- is ``step(keys, frames)`` instead: the frames are not stored
    by launches of this call but travel with the returned pyramid, and the decoder call moves them into their slots itself
    (``sbev_pool_insert_frames``, destinations read from device rows behind the slot table): inside the captured step when it is
    replayed.  ``stream(keys, frames)`` is the same for as many frames as the step lacks -- the scene's first window included -- in the
    memory the backbone emits: NCHW or channels-last, 2-byte frames widened into fp32 slots (the same launch, still one); ``step`` is its
    K = 1 case with a narrower rule for what travels."""

    def __init__(self, num_frames, n_slots=16, dtype=torch.float32):
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError('pool storage must be fp32, fp16 or bf16')
        self.dtype = dtype
        self.book = SlotBook(num_frames, n_slots)
        self.T, self.n_slots = num_frames, n_slots
        self.buffers = None            # list[L] of [B, n_slots, 6, H, W, C]
        self.slot_table = None         # device int32 [B, T]: allocated once with the buffers, refreshed in place per pyramid() / step()
        self.insert_row = None         # device int32 [B] behind it in the same allocation (``_tables``): step()'s slot per sample, -1 = none
        self._tables = None
        self._rows = None              # the whole allocation: slot table, then T rows of [B] for stream() (row 0 = ``insert_row``)
        self._live = None              # the pyramid handed out last: the next pyramid() / step() ends its validity

    @property
    def B(self):
        return self.book.B

    def missing(self, keys):
        """keys[b][t]: hashable frame keys, t = 0 newest -> the distinct (b, key) pairs that are not resident."""
        return self.book.missing(keys)

    def put(self, b, key, frame_feats):
        """One sample's frame into a slot of sample b.  frame_feats: list[L] of [6, C, H_l, W_l] device tensors, NCHW or channels-last
        (dtype rules of FrameFeatureCache.push)."""
        feats = list(frame_feats)
        for f in feats:
            if not (torch.is_tensor(f) and f.is_cuda and f.dim() == 4 and f.shape[0] == N_VIEWS):
                raise RuntimeError('frame features must be device tensors [6, C, H, W]')
        if self.buffers is None:
            if self.book.B is None:
                raise RuntimeError('announce the step with missing(keys) before the first put(): the batch size is taken from it')
            self._alloc([tuple(f.shape[1:]) for f in feats], feats[0].device)
        if len(feats) != len(self.buffers) or any(tuple(buf.shape[3:]) != (f.shape[2], f.shape[3], f.shape[1]) for f, buf in zip(feats, self.buffers)):
            raise RuntimeError('frame features do not match the pool\'s levels')
        slot, _ = self.book.assign(b, key)
        for f, buf in zip(feats, self.buffers):
            _store_level(f[None], [buf[b, slot]], self.dtype)
        return slot

    def _alloc(self, chw, device):
        """buffers for levels of (C, H, W) and the two tables in ONE int32 allocation: [B, T] slot table, then the [B] insert row"""
        B = self.book.B
        self.buffers = [torch.empty(B, self.n_slots, N_VIEWS, h, w, c, device=device, dtype=self.dtype) for c, h, w in chw]
        # (stream()'s [K, B] rows, K <= T, start where the insert row does: row 0 IS the insert row, rows 1 .. T - 1 lie behind it)
        self._rows = torch.full((B * self.T + self.T * B,), -1, device=device, dtype=torch.int32)
        self._rows[:B * self.T] = 0
        self._tables = self._rows[:B * self.T + B]
        self.slot_table = self._tables[:B * self.T].view(B, self.T)
        self.insert_row = self._tables[B * self.T:]

    def _hand_out(self, pyr):
        if self._live is not None:
            self._live.insert = None          # (its frames are free again; the tables it reads now describe another step)
        self._live = pyr
        return pyr

    def pyramid(self, keys):
        """The step's view for the decoder (drop-in for transformer.FeaturePyramid): uploads the step's table into the persistent
        device table through the pinned upload ring (asynchronous, no allocation) and returns a PoolPyramid over it."""
        import numpy as np
        from .transformer import _upload
        rows = self.book.table(keys)
        if self.buffers is None:
            raise RuntimeError('the pool is empty')
        _upload(np.asarray(rows, dtype=np.int32), self.slot_table.device, out=self.slot_table)
        return self._hand_out(PoolPyramid(self))

    def _insert_takes(self, frames):
        """whether step() lets these frames travel with the pyramid: contiguous NCHW memory of the slots' own type, 16-byte aligned (a
        step's pointer table carries the addresses).  Channels-last memory and fp16 / bf16 frames for fp32 slots are _store_level's."""
        return all(f.dtype == self.dtype and f.is_contiguous() and f.data_ptr() % 16 == 0 for f in frames)

    def step(self, keys, frames):
        """One streaming step: ``frames`` = list[L] of [B, 6, C, H_l, W_l] device tensors, the backbone's output for the batch's newest
        images (as FrameFeatureCache.push takes them); sample b's goes under ``keys[b][0]`` unless that key is resident.  Every other key
        of the step must be resident (SlotBook.plan_step).  It is ``stream(keys, {0: frames})`` with its own argument check and a
        narrower rule for what travels (_insert_takes): the returned PoolPyramid carries ``FrameInsert(frames, insert row as [1, B],
        False)``, and frames the rule does not take (channels-last memory, fp16 / bf16 for fp32 slots) are stored here and now as put()
        stores them, the pyramid carrying no insert."""
        frames = list(frames)
        if not frames or not all(torch.is_tensor(f) and f.is_cuda and f.dim() == 5 and f.shape[1] == N_VIEWS and f.shape[0] == frames[0].shape[0]
                                 for f in frames):
            raise RuntimeError('frame features must be device tensors [B, 6, C, H, W]')
        keys = [list(row) for row in keys]
        if len(keys) != frames[0].shape[0]:
            raise ValueError('keys for %d samples, frames for %d' % (len(keys), frames[0].shape[0]))
        return self._feed(keys, [0], [frames], False if self._insert_takes(frames) else None)

    def _frames_layout(self, flat):
        """what stream() lets travel with the pyramid, which is all sbev_pool_insert_frames takes: frames of one type -- the slots' own,
        or fp16 / bf16 for fp32 slots -- in one layout, NCHW-contiguous (False) or channels-last (True) memory, 16-byte aligned.  None: not
        taken (misaligned or non-contiguous memory, mixed layouts or types, fp32 for 2-byte slots): those are _store_level's, which
        refuses what nothing here stores."""
        dt = flat[0].dtype
        if any(f.dtype != dt or f.data_ptr() % 16 for f in flat) or not (dt == self.dtype or (self.dtype == torch.float32 and dt in (torch.float16, torch.bfloat16))):
            return None
        if all(f.is_contiguous() for f in flat):
            return False
        if all(f.permute(0, 1, 3, 4, 2).is_contiguous() for f in flat):
            return True
        return None

    def stream(self, keys, frames):
        """One streaming step that takes the frames as the backbone emits them, as many as the step lacks: ``frames`` maps a window
        position t to a list[L] of [B, 6, C, H_l, W_l] device tensors -- the batch's frames ``keys[b][t]`` -- NCHW-contiguous or channels-
        last memory, fp32 / fp16 / bf16 (2-byte frames for fp32 slots are widened exactly), one layout and type per call.  Every key of
        the step that is not resident must be at one of the given positions (SlotBook.plan_frames).  Frames the kernel does not take
        (_frames_layout) are stored here and now as put() stores them, and the pyramid carries no insert; what put() refuses raises here
        too."""
        keys = [list(row) for row in keys]
        ts = sorted(frames)
        sets = [list(frames[t]) for t in ts]
        flat = [f for fs in sets for f in fs]
        if not flat or not all(torch.is_tensor(f) and f.is_cuda and f.dim() == 5 and f.shape[1] == N_VIEWS and f.shape[0] == len(keys) for f in flat):
            raise RuntimeError('frame features must be device tensors [B, 6, C, H, W], B = %d' % len(keys))
        return self._feed(keys, ts, sets, self._frames_layout(flat))

    def _feed(self, keys, ts, sets, nhwc):
        """What step() and stream() do alike once their arguments are checked: ``sets[k]`` = the list[L] of frames for window position
        ``ts[k]`` (ascending), ``nhwc`` = their layout for the insert kernel (False NCHW, True channels-last) or None where they take the
        eager store.  Slot table and the [K, B] destination rows (row 0 at ``insert_row``'s address) go up in one upload; the returned
        PoolPyramid carries a ``FrameInsert``: the decoder call it is handed to moves the frames into their slots in ONE launch
        (sbev_pool_insert_frames, inside the captured step when that is replayed; PoolPyramid.materialise() for other readers).  The
        pyramid keeps the frames alive until the next stream() / step() / pyramid(), which also ends its validity."""
        import numpy as np
        from .transformer import _upload
        flat = [f for fs in sets for f in fs]
        chw = [tuple(f.shape[2:]) for f in sets[0]]
        if any([tuple(f.shape[2:]) for f in fs] != chw for fs in sets) or (self.buffers is not None and (
                len(chw) != len(self.buffers) or any(tuple(buf.shape[3:]) != (h, w, c) for (c, h, w), buf in zip(chw, self.buffers)))):
            raise RuntimeError('frame features do not match the pool\'s levels')
        rows, insert = self.book.plan_frames(keys, ts)
        if self.buffers is None:
            self._alloc(chw, flat[0].device)
        if nhwc is None:
            for fs, row in zip(sets, insert):
                for b, slot in enumerate(row):
                    if slot >= 0:
                        for f, buf in zip(fs, self.buffers):
                            _store_level(f[b:b + 1], [buf[b, slot]], self.dtype)
            insert = [[-1] * len(row) for row in insert]
        B, K = len(keys), len(ts)
        up = self._rows[:B * self.T + K * B]         # (K = 1: ``_tables``)
        _upload(np.asarray([s for row in rows for s in row] + [s for row in insert for s in row], dtype=np.int32), up.device, out=up)
        pending = None if nhwc is None else FrameInsert(flat, up[B * self.T:].view(K, B), nhwc)
        return self._hand_out(PoolPyramid(self, pending))

    def drop(self, b):
        """Forget sample b's stream: its next keys are all misses."""
        self.book.drop(b)


class PoolPyramid(_SlotPyramid):
    """(no ``frame_slots`` attribute: that is the by-value ring's mapping; the pool's is ``slot_table``)"""

    def __init__(self, pool, insert=None):
        super().__init__(pool)
        self.slot_table = pool.slot_table
        self.insert = insert           # FramePool.step() / stream(): the FrameInsert (frames and their device rows) still to be moved into the slots

    def resident(self):
        """this view without the pending insert: what a captured step may hold (buffers and tables, none of the caller's frames)"""
        import copy
        pyr = copy.copy(self)
        pyr.insert = None
        return pyr

    def materialise(self):
        """Enqueue the pending insert on the current stream (sbev_pool_insert_frames, direct sources).  Idempotent -- the same frames go
        to the same slots -- and a no-op without one.  The decoder does this itself; for callers of ``sample`` outside it."""
        if self.insert is None:
            return
        ins = self.insert
        pool_insert_frames(ins.frames, self.levels, ins.rows, self.n_slots, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ins.nhwc)

    def sample(self, loc, w_bp, T, G):
        return ops.msmv_sampling_pool(self.levels, self.B, T, G, self.slot_table, self.n_slots, loc, w_bp)


def pool_insert(frames, levels, row, n_slots, stream, table=None, index=None, check=True):
    """sbev_pool_insert, the C entry for one NCHW frame set of the slots' own type (the pool itself goes through pool_insert_frames):
    ``frames`` list[L] of NCHW [B, 6, C, H_l, W_l] into the resident buffers ``levels`` ([B*n_slots*6, H_l, W_l, C] or
    any view of the same memory), sample b into slot ``row[b]`` (device int32 [B]; outside [0, n_slots): none).  Sources are the frames'
    own addresses, or -- ``table`` (device pointer table) and ``index`` (list[L]) -- read from the table when the kernel starts; the
    frames then only give shapes and dtype.  ``check=False`` returns the status instead of raising on it (a caller inside a stream capture
    has to end the capture first)."""
    L, f0 = len(frames), frames[0]
    code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[f0.dtype]
    if len(levels) != L or any(f.dtype != f0.dtype or buf.dtype != f0.dtype for f, buf in zip(frames, levels)):
        raise RuntimeError('pool insert: frames and slots must have one storage type')
    src = None if table is not None else (ctypes.c_void_p * L)(*[f.data_ptr() for f in frames])
    idx = (ctypes.c_int32 * L)(*index) if table is not None else None
    out = (ctypes.c_void_p * L)(*[buf.data_ptr() for buf in levels])
    hw = (ctypes.c_int32 * L)(*[f.shape[3] * f.shape[4] for f in frames])
    st = _lib.load().sbev_pool_insert(table, idx, src, out, L, hw, f0.shape[0], f0.shape[1], f0.shape[2], code, ctypes.c_void_p(row.data_ptr()),
                                      n_slots, stream)
    if check:
        _lib.check(st, 'sbev_pool_insert')
    return st


def pool_insert_frames(frames, levels, rows, n_slots, stream, nhwc=False, table=None, index=None, check=True):
    """sbev_pool_insert_frames: ``frames`` = K * L tensors [B, 6, C, H_l, W_l] (frame set k's levels at [k * L, (k + 1) * L)), all NCHW-
    contiguous or -- ``nhwc`` -- all channels-last memory, of one type, into the resident buffers ``levels``: sample b's frame of set k into
    slot ``rows[k, b]`` (device int32 [K, B]; outside [0, n_slots): none; two live entries of one sample must differ, SlotBook.plan_frames
    sees to it).  fp16 / bf16 frames into fp32 buffers are widened.  Sources, ``table`` / ``index`` (K * L entries) and ``check`` as for
    pool_insert."""
    L, f0 = len(levels), frames[0]
    K = rows.shape[0]
    codes = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    if len(frames) != K * L or any(f.dtype != f0.dtype for f in frames) or any(buf.dtype != levels[0].dtype for buf in levels):
        raise RuntimeError('pool insert: K * L frames of one type into L levels of one storage type')
    n = K * L
    src = None if table is not None else (ctypes.c_void_p * n)(*[f.data_ptr() for f in frames])
    idx = (ctypes.c_int32 * n)(*index) if table is not None else None
    out = (ctypes.c_void_p * L)(*[buf.data_ptr() for buf in levels])
    hw = (ctypes.c_int32 * L)(*[f.shape[3] * f.shape[4] for f in frames[:L]])
    st = _lib.load().sbev_pool_insert_frames(table, idx, src, out, K, L, hw, f0.shape[0], f0.shape[1], f0.shape[2], 1 if nhwc else 0, codes[f0.dtype],
                                             codes[levels[0].dtype], ctypes.c_void_p(rows.data_ptr()), n_slots, stream)
    if check:
        _lib.check(st, 'sbev_pool_insert_frames')
    return st
