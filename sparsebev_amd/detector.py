"""SparseBEV: the whole detector's training forward under the reference's parameter names -- ``ImageFrontEnd`` -> ``ResNetBackbone`` ->
``FPNNeck`` -> ``SparseBEVTrainHead`` -- as thin glue: every launch is one of those modules'.

Reference counterpart: ``SparseBEV`` (models/sparsebev.py:13-217): ``extract_feat`` and ``forward_train``.  A reference checkpoint's
``img_backbone.*`` / ``img_neck.*`` / ``pts_bbox_head.*`` entries load with ``strict=True``, and the reference's optimizer recipe
(``paramwise_cfg`` with ``img_backbone: lr_mult 0.1`` and ``sampling_offset: lr_mult 0.1``) is one call of ``param_groups``.  The step as
one graph replay: ``train_graph.CapturedDetectorTrainStep``.  Not built: ``stop_prev_grad`` (the split of the frames into a part with and
a part without gradient), the test-time methods (``simple_test*``).
"""
import torch
import torch.nn as nn

from . import optim
from .fpn import FPNNeck
from .head_train import SparseBEVTrainHead
from .image_front import ImageFrontEnd
from .resnet import ResNetBackbone


def _build(cls, spec, what, drop=('type',)):
    if isinstance(spec, cls):
        return spec
    if not isinstance(spec, dict):
        raise TypeError('sparsebev_amd.SparseBEV: %s is a %s or the dict of its arguments, not %r' % (what, cls.__name__, type(spec).__name__))
    return cls(**{k: v for k, v in spec.items() if k not in drop})


class SparseBEV(nn.Module):
    """``SparseBEV(img_backbone, img_neck, pts_bbox_head, data_aug=None, stop_prev_grad=0)``: each of the three a built module
    (``ResNetBackbone``, ``FPNNeck``, ``SparseBEVTrainHead``) or the dict of its arguments (a ``type`` entry is ignored; for the neck the
    keys mmdet does not share -- ``start_level``, ``norm_cfg``, ... -- are the caller's to drop).  ``data_aug``: the reference's dict
    (``img_norm_cfg``, ``img_pad_cfg``, ``img_color_aug``), handed to ``ImageFrontEnd.from_data_aug``; the front end is ``self.front``
    and holds no parameter.  ``stop_prev_grad != 0`` is refused."""

    def __init__(self, img_backbone, img_neck, pts_bbox_head, data_aug=None, stop_prev_grad=0, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        if stop_prev_grad != 0:
            raise ValueError('sparsebev_amd.SparseBEV: stop_prev_grad=%r is not built (the split of the frames into a part with and a part '
                             'without gradient: models/sparsebev.py:102-122); 0 is' % (stop_prev_grad,))
        self.stop_prev_grad = 0
        self.data_aug = data_aug
        self.img_backbone = _build(ResNetBackbone, img_backbone, 'img_backbone')
        self.img_neck = _build(FPNNeck, img_neck, 'img_neck')
        self.pts_bbox_head = _build(SparseBEVTrainHead, pts_bbox_head, 'pts_bbox_head')
        self.front = ImageFrontEnd.from_data_aug(data_aug or {})

    def extract_feat(self, img, img_metas, front_params=None):
        """models/sparsebev.py:61-131 without the stop_prev_grad split: img [B, N, 3, H, W] (uint8 or fp32, on the device) -> the neck's
        levels as [B, N, 256, h, w] fp32 views (channels-last in memory, what the decoder reads in place); writes the shapes into
        ``img_metas`` as the reference does.  ``front_params``: this step's ``FrontParams`` instead of a draw."""
        B = len(img_metas)
        x = self.front(img, img_metas, params=front_params)
        stages = self.img_backbone(x)
        levels = self.img_neck(stages, out_dtype=torch.float32)
        return [o.view(B, o.shape[0] // B, *o.shape[1:]) for o in levels]

    def forward_train(self, img, img_metas, gt_bboxes_3d, gt_labels_3d, front_params=None):
        """models/sparsebev.py:174-217: the head's loss dict"""
        feats = self.extract_feat(img, img_metas, front_params)
        for meta, boxes, labels in zip(img_metas, gt_bboxes_3d, gt_labels_3d):
            meta['gt_bboxes_3d'], meta['gt_labels_3d'] = boxes, labels
        outs = self.pts_bbox_head(feats, img_metas)
        return self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs)

    def forward(self, img=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None, return_loss=True, **kwargs):
        if not return_loss:
            raise NotImplementedError('sparsebev_amd.SparseBEV: the test-time methods are not built (SparseBEVHead and the runtime are the '
                                      'inference path)')
        return self.forward_train(img, img_metas, gt_bboxes_3d, gt_labels_3d, **kwargs)

    def param_groups(self, lr, weight_decay, custom_keys=None):
        """``optim.param_groups`` over the detector's prefixed names: ``det.param_groups(2e-4, 0.01, {'img_backbone': dict(lr_mult=0.1),
        'sampling_offset': dict(lr_mult=0.1)})`` is the reference's recipe (configs/r50_nuimg_704x256.py)."""
        return optim.param_groups(self.named_parameters(), lr, weight_decay, custom_keys)
