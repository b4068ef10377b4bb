"""CPU-side checks of the fixed-capacity ground truth: the plan entry's export, declaration, signature and argument checks (no GPU call
is reached), the ``SparseBEVTrainHead(gt_capacity=...)`` constructor's refusals and ``GroundTruthSlab``'s host half."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import head_train_cases as C
import test_head_train_host as H
from sparsebev_amd import _lib
from sparsebev_amd import head_train as HT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_entry_is_exported_declared_and_typed():
    lib = _lib.load()
    assert hasattr(lib, 'sbev_head_capacity_plan') and 'sbev_head_capacity_plan' in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES['sbev_head_capacity_plan']
    assert restype is ctypes.c_int and len(argtypes) == 10 and argtypes[5] is ctypes.c_double
    header = open(os.path.join(ROOT, 'include', 'sbev_hip.h')).read()
    decl = re.search(r'int sbev_head_capacity_plan\(([^;]*)\);', header)
    assert decl is not None and len(decl.group(1).split(',')) == len(argtypes)
    assert 'double bg_cls_weight' in decl.group(1)


def test_plan_entry_validates_without_gpu():
    """Every refusal comes before the launch: a status and a text in sbev_last_error(), as the round-3 training entry points do."""
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.int32)
    ok = ctypes.c_void_p(buf.ctypes.data)           # a host address: never dereferenced, the checks come first
    plan = lambda off, B, Q, cap, N, codes, avg, status: lib.sbev_head_capacity_plan(off, B, Q, cap, N, 0.0, codes, avg, status, None)
    for args, text in [((ok, -1, 36, 4, 2, ok, ok, ok), b'bad sizes'), ((ok, 2, -1, 4, 2, ok, ok, ok), b'bad sizes'),
                       ((ok, 2, 36, -1, 2, ok, ok, ok), b'bad sizes'), ((ok, 2, 36, 4, 0, ok, ok, ok), b'bad sizes'),
                       ((ok, 1 << 20, 36, 1 << 20, 2, ok, ok, ok), b'too large'),
                       ((None, 2, 36, 4, 2, ok, ok, ok), b'null pointer'), ((ok, 2, 36, 4, 2, ok, None, ok), b'null pointer'),
                       ((ok, 2, 36, 4, 2, ok, ok, None), b'null pointer'), ((ok, 2, 36, 4, 2, None, ok, ok), b'null codes')]:
        assert plan(*args) == -1 and text in lib.sbev_last_error() and b'sbev_head_capacity_plan' in lib.sbev_last_error(), args
    with pytest.raises(RuntimeError):               # the wrapper: device int32 offsets only
        HT.capacity_plan(torch.zeros(3, dtype=torch.int32), 2, 36, 4, 2)


def test_train_head_capacity_constructor():
    head = H.make_head(assign_on='device', gt_capacity=7)
    assert head.gt_capacity == 7 and head.assign_on == 'device' and head.plan_status is None and head.dn_noise is None
    assert H.make_head().gt_capacity is None and H.make_head(assign_on='device', gt_capacity=0).gt_capacity == 0
    assert len(head.state_dict()) == 51                                  # the slab is no state
    with pytest.raises(ValueError, match="assign_on='device'"):
        H.make_head(gt_capacity=7)                                       # the default solver is the host's
    with pytest.raises(ValueError, match="assign_on='device'"):
        H.make_head(assign_on='host', gt_capacity=7)
    for bad in (-1, 2.5, '7', True):
        with pytest.raises(ValueError, match='gt_capacity'):
            H.make_head(assign_on='device', gt_capacity=bad)
    from sparsebev_amd.train_graph import CapturedHeadTrainStep
    with torch.enable_grad(), pytest.raises(ValueError, match='gt_capacity'):
        CapturedHeadTrainStep(H.make_head(assign_on='device').train(), [], [])


@pytest.mark.parametrize('bg', [0.0, 0.1])
@pytest.mark.parametrize('counts,Q,N', [((0,), 36, 2), ((0, 5, 2), 36, 3), ((5,), 3, 2), ((43, 0, 17), 36, 2)],
                         ids=['c0', 'c0-5-2', 'c5_q3', 'c43-0-17'])
def test_host_plan_vs_restatement(counts, Q, N, bg):
    """``GroundTruth.plan`` on the host's counts against the written-down restatement the device's plan launch is held to
    (test_gpu_head_capacity.py), at the batch's own ``single`` and at a ``single`` above it, bit for bit."""
    boxes, labels = C.make_gt(counts, 10, 7)
    gt = HT.GroundTruth(boxes, labels, 'cpu')
    assert gt.single == max(counts) and gt.counts == list(counts)
    for single in (max(counts), max(counts) + 2):
        gt.single = single
        codes, avg, status = gt.plan(Q, N, bg)
        want_codes, want_avg = C.host_plan(counts, Q, single, N, bg)
        assert status is None and codes.dtype == torch.int32 and avg.dtype == torch.float32
        assert codes.shape == (len(counts), N * single) and avg.shape == (2, 2)
        assert torch.equal(codes, want_codes)
        assert torch.equal(avg, want_avg), (avg.tolist(), want_avg.tolist())
        assert bool((codes.view(len(counts), N, single)[:, :, max(counts):] == -2).all())


def test_same_as_is_one_body():
    assert HT.GroundTruth.same_as is HT.GroundTruthSlab.same_as
    boxes, labels = C.make_gt((3, 0, 2), 10, 5)
    assert not HT.GroundTruth(boxes, labels, 'cpu').same_as(boxes, labels)            # the plain constructor records no objects
    gt = HT.GroundTruth.from_metas([{'gt_bboxes_3d': b, 'gt_labels_3d': l} for b, l in zip(boxes, labels)], 'cpu')
    assert gt.same_as(boxes, labels)
    assert not gt.same_as([b.clone() for b in boxes], labels) and not gt.same_as(boxes, [l.clone() for l in labels])
    assert not gt.same_as(boxes[:2], labels[:2])
    slab = HT.GroundTruthSlab(3, 4, 'cpu')
    assert not slab.same_as(boxes, labels) and slab.update(boxes, labels).same_as(boxes, labels)
    assert not slab.same_as([b.clone() for b in boxes], labels)


def test_slab_host_half():
    """On a CPU device the slab packs and validates exactly as on the GPU (the upload is a plain copy): layout, counts, refusals."""
    boxes, labels = C.make_gt((3, 0, 2), 10, 5)
    slab = HT.GroundTruthSlab(3, 4, 'cpu')
    assert (slab.B, slab.single, slab.G, slab.capacity) == (3, 4, 12, 4)
    assert slab.boxes.shape == (12, 9) and slab.labels.shape == (12,) and slab.offsets.tolist() == [0, 0, 0, 0]
    ptrs = (slab.boxes.data_ptr(), slab.labels.data_ptr(), slab.offsets.data_ptr())
    assert slab.update(boxes, labels) is slab
    assert slab.counts == [3, 0, 2] and slab.offsets.tolist() == [0, 3, 3, 5] == slab.offsets_host.tolist()
    assert torch.equal(slab.boxes[:5], torch.cat(boxes)) and torch.equal(slab.labels[:5].long(), torch.cat(labels))
    assert float(slab.boxes[5:].abs().max()) == 0.0 and int(slab.labels[5:].abs().max()) == 0
    assert (slab.boxes.data_ptr(), slab.labels.data_ptr(), slab.offsets.data_ptr()) == ptrs
    assert slab.same_as(boxes, labels) and not slab.same_as([b.clone() for b in boxes], labels)
    before = slab.buffer.clone()
    over_b, over_l = C.make_gt((5, 0, 2), 10, 6)
    with pytest.raises(ValueError, match='capacity is 4'):
        slab.update(over_b, over_l)
    with pytest.raises(ValueError, match='3'):
        slab.update(boxes[:2], labels[:2])
    with pytest.raises(ValueError, match='disagree'):
        slab.update(boxes, labels[::-1])
    with pytest.raises(ValueError):
        slab.update([torch.zeros(2, 7)] * 3, [torch.zeros(2)] * 3)
    assert torch.equal(slab.buffer, before) and slab.counts == [3, 0, 2] and slab.same_as(boxes, labels)
    import copy
    twin = copy.deepcopy(slab)                                           # a copy starts empty, with buffers of its own
    assert twin.boxes.data_ptr() != slab.boxes.data_ptr() and twin.counts == [0, 0, 0] and twin.source is None
    with pytest.raises(ValueError):
        HT.GroundTruthSlab(2, -1, 'cpu')
