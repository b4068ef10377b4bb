"""Module-level switches the reference exposes next to the hot path (models/utils.py:309-325)."""
import os
import tempfile
from typing import NamedTuple

import torch


class DumpConfig:
    """The ``DUMP`` debug taps (models/utils.py:309-317).  When ``enabled`` the decoder writes, per stage,
    ``sample_points_cam_stage{i}.pth`` ([B,T,N,Q,GP,3] = u, v, max(homo,eps)),
    ``sample_points_cam_valid_mask_stage{i}.pth`` ([B,T,N,Q,GP] float 0/1), ``sasa_tau_stage{i}.pth``,
    ``query_bbox_stage{i}.pth``, ``bbox_pred_stage{i}.pth`` and ``cls_score_stage{i}.pth`` into ``out_dir``
    -- the files viz_sample_points.py:83-105 reads."""

    def __init__(self):
        self.enabled = False
        self.out_dir = tempfile.mkdtemp()
        self.stage_count = 0
        self.frame_count = 0

    def save(self, name, tensor):
        torch.save(tensor.detach().cpu(), os.path.join(self.out_dir, '%s_stage%d.pth' % (name, self.stage_count)))


DUMP = DumpConfig()


class Version:
    """Checkpoint convention switch (models/utils.py:320-325): ``VERSION.name`` is 'v1.0.0' (default) or 'v0.17.1'
    (set from ``checkpoint['version']``, val.py:128-129).  It flips the rotation sign of the sample offsets
    (rotation_3d_in_axis, models/utils.py:66-77) and the box layout of ``get_bboxes`` (models/sparsebev_head.py:472-476);
    assigning it forwards the choice to the library (``sbev_set_box_convention``), which reads it at launch time."""
    _CODES = {'v1.0.0': 0, 'v0.17.1': 1}

    def __init__(self):
        self._name = 'v1.0.0'

    @property
    def name(self):
        return self._name

    @name.setter
    def name(self, value):
        if value not in self._CODES:
            raise NotImplementedError("unknown box convention %r (the reference knows 'v1.0.0' and 'v0.17.1')" % (value,))
        from . import _lib
        _lib.check(_lib.load().sbev_set_box_convention(self._CODES[value]), 'sbev_set_box_convention')
        self._name = value

    def require_supported(self):
        """The library and the Python switch must agree (someone may have called sbev_set_box_convention directly)."""
        from . import _lib
        if _lib.load().sbev_get_box_convention() != self._CODES[self._name]:
            raise RuntimeError('VERSION.name = %r but libsbev_hip.so is set to convention %d'
                               % (self._name, _lib.load().sbev_get_box_convention()))


VERSION = Version()


class FrameInsert(NamedTuple):
    """The pending insert of cache.FramePool.stream and FramePool.step (K = 1, NCHW): ``frames`` = the tensors whose addresses travel in
    a step's pointer table, ``rows`` = the device rows that say where they go.  ``frames``: K * L device tensors ``[B, 6, C, H_l, W_l]``, frame set k's levels at ``[k * L, (k + 1) * L)``, sets in ascending window position; ``rows``:
    device int32 ``[K, B]``, the slot sample b's frame of set k goes to (-1: none); ``nhwc``: the frames are channels-last memory (else
    NCHW-contiguous), one layout and one dtype per insert."""
    frames: list
    rows: object
    nhwc: bool

    @property
    def K(self):
        return self.rows.shape[0]


class FrameSource(NamedTuple):
    """Where a decoder step's frames live.  ``kind``: 'list' (a feature list, no pyramid object), 'dense' (transformer.FeaturePyramid:
    frame t of sample b is image run b*T + t), 'ring' (cache.RingPyramid: slot ``frame_slots[t]`` of ``n_slots`` for the whole batch,
    passed to the kernels by value) or 'pool' (cache.PoolPyramid: slot ``slot_table[b, t]`` of ``n_slots``, a device table the kernels read).
    ``insert`` (the pool only, else None): the step's pending ``FrameInsert`` -- K frame sets of ``[B, 6, C, H_l, W_l]`` maps the decoder
    call still has to move into slot ``rows[k, b]`` of sample b (device int32 [K, B], -1: none) before any frame is read."""
    kind: str
    frame_slots: tuple = ()
    slot_table: object = None
    n_slots: int = 0
    insert: object = None

    @property
    def resident(self):
        return self.kind in ('ring', 'pool')

    @classmethod
    def of(cls, frame_slots=None, slot_table=None, n_slots=0, shape=None, what='the frame pool', plain='dense', insert=None):
        """From the slot mapping itself (the operator layer is handed it as arguments); ``plain``: the kind without one (None: the
        caller means the pool).  With ``shape = (B, T)`` the pool's table is validated -- here and nowhere else."""
        if frame_slots is not None and slot_table is not None:
            raise RuntimeError('%s: give frame_slots (the ring) or slot_table (the frame pool), not both' % what)
        if frame_slots is not None:
            return cls('ring', tuple(int(s) for s in frame_slots), None, n_slots)
        if slot_table is None and plain is not None:
            return cls(plain)
        if shape is not None:
            if not (torch.is_tensor(slot_table) and slot_table.is_cuda and slot_table.dtype == torch.int32 and slot_table.is_contiguous()
                    and tuple(slot_table.shape) == tuple(shape)):
                raise RuntimeError('%s: slot_table must be a contiguous device int32 [B, T] = [%d, %d]' % ((what,) + tuple(shape)))
            if n_slots < 1:
                raise RuntimeError('%s: n_slots must be at least 1' % what)
        return cls('pool', (), slot_table, n_slots, insert)


def frame_source(feats, shape=None, what='the frame pool'):
    """The FrameSource of whatever the decoder is handed as features -- the ONE place that looks at the ``levels`` / ``frame_slots`` /
    ``slot_table`` / ``insert`` attributes: ``frame_slots`` marks the ring, ``slot_table`` the pool (both: refused; ``insert`` is the pool's
    alone), ``levels`` alone a dense pyramid, none of them a feature list."""
    return FrameSource.of(getattr(feats, 'frame_slots', None), getattr(feats, 'slot_table', None), getattr(feats, 'n_slots', 0), shape, what,
                          plain='dense' if hasattr(feats, 'levels') else 'list', insert=getattr(feats, 'insert', None))


def slot_resident(feats):
    """True for the two pyramids that read resident per-frame slot buffers through a slot mapping (the online ring, the keyed frame
    pool).  Both are inference caches over persistent buffers: no training path, never counted as a caller's throw-away buffers."""
    return frame_source(feats).resident
