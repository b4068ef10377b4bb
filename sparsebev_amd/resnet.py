"""ResNetBackbone: the detector's image backbone (mmdet's ``ResNet``, depth 50 / 101 / 152, ``style='pytorch'``, ``norm_eval=True``:
configs/r50_nuimg_704x256.py:31-40) for inference on the matrix core, one launch of csrc/resnet.hip per convolution: the NCHW images of
``ImageFrontEnd`` in, the channels-last fp16 stage maps out that ``FPNNeck`` takes in place.

Reference counterpart: ``ResNet.forward`` under fp16 autocast (models/sparsebev.py:46) -- per convolution a convolution, a BatchNorm in
eval mode, a ReLU or add + ReLU and the casts around them, each a launch of its own.

Arithmetic (include/sbev_hip.h: sbev_resnet_forward): the BatchNorm of every convolution is folded into it on the device, per output
channel in individually rounded fp32 operations, ``s = gamma / sqrt(var + eps)``, ``w' = fp16(w * s)``, ``b' = beta - mean * s``; every
convolution multiplies fp16 operands, accumulates in fp32 and stores ``fp16(acc + b' [+ residual] [max 0])``, rounded once.  The
reference's chain rounds the convolution, the norm and the sum to fp16 one after the other.

The fold and the fragment-order pack are redone when a parameter or a buffer changed (every tensor's ``_version`` and address: an
in-place write, ``load_state_dict`` or ``.to()`` repacks at the next call).  Inference only: the parameters are created with
``requires_grad=False`` and a forward that would need a gradient raises.  There is no CPU path and no silent copy.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib

MAX_LAYERS, PLAN_HEAD, LAYER_WORDS = 160, 18, 12        # SBEV_RESNET_MAX_LAYERS, SBEV_RESNET_PLAN_HEAD, SBEV_RESNET_LAYER_WORDS
PLAN_WORDS = PLAN_HEAD + LAYER_WORDS * MAX_LAYERS
STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
KINDS = ('stem', 'pool', 'conv')
EPILOGUES = {'bias': 0, 'relu': 1, 'residual_relu': 2}
_DTYPES = {torch.float32: 0, torch.float16: 2}          # SBEV_F32, SBEV_F16


def _i32(values):
    values = [int(v) for v in values]
    return (ctypes.c_int32 * max(len(values), 1))(*values)


def _vp_array(tensors):
    return (ctypes.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def plan(depth, n, H, W, out_indices=(0, 1, 2, 3), num_stages=4, base_channels=64, stage_blocks=None, keep=False):
    """sbev_resnet_plan, a pure host function: a dict of launches, pack_bytes, workspace_bytes, macs (multiply-adds of a forward), outs
    [(C, h, w), ...] and layers, one dict per launch in launch order (stem, pool, then per block conv1, conv2, [downsample], conv3):
    kind, cin, cout, taps, stride, h, w, row_tiles, col_tiles, k_split, where (a byte offset in the workspace, or -(1 + k): outs[k]),
    epilogue.  Raises SbevError where the plan refuses."""
    out = (ctypes.c_int64 * PLAN_WORDS)()
    blocks = None if stage_blocks is None else _i32(stage_blocks)
    if stage_blocks is not None and len(stage_blocks) != num_stages:
        raise ValueError('stage_blocks must list num_stages=%d block counts' % num_stages)
    _lib.check(_lib.load().sbev_resnet_plan(int(depth), blocks, int(num_stages), int(base_channels), int(n), int(H), int(W), len(out_indices),
                                            _i32(out_indices), int(bool(keep)), out), 'sbev_resnet_plan')
    v = [int(x) for x in out]
    names = ('kind', 'cin', 'cout', 'taps', 'stride', 'h', 'w', 'row_tiles', 'col_tiles', 'k_split', 'where', 'epilogue')
    layers = []
    for i in range(v[3]):
        d = dict(zip(names, v[PLAN_HEAD + LAYER_WORDS * i:PLAN_HEAD + LAYER_WORDS * (i + 1)]))
        d['kind'] = KINDS[d['kind']]
        layers.append(d)
    return dict(launches=v[0], pack_bytes=v[1], workspace_bytes=v[2], macs=v[4], outs=[tuple(v[6 + 3 * k:9 + 3 * k]) for k in range(v[5])],
                layers=layers)


def pack_layers(layers, eps=1e-5, pack=None):
    """sbev_resnet_pack_weights on a list of ``(weight, gamma, beta, mean, var)`` device tensors (weight [Cout, Cin, k, k] with k = 1, 3,
    or 7 for the stem, fp32 or fp16; the statistics fp32): folds and packs layer after layer.  Returns (the uint8 pack tensor, the byte
    offset of every layer's image, the byte offset of every layer's fp32 bias)."""
    ws = [l[0] for l in layers]
    dev = ws[0].device
    desc, at, offs, bias_offs = [], 0, [], []
    for w in ws:
        cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        frag = (160 if k == 7 else k * k * cin) * cout * 2
        desc += [cin, cout, k * k]
        offs.append(at)
        bias_offs.append(at + frag)
        at += frag + 4 * cout
    with torch.cuda.device(dev):
        if pack is None:
            pack = torch.empty(max(at, 16), dtype=torch.uint8, device=dev)
        cols = [_vp_array([l[j] for l in layers]) for j in range(5)]
        _lib.check(_lib.load().sbev_resnet_pack_weights(len(layers), _i32(desc), *cols, float(eps), _DTYPES[ws[0].dtype],
                                                        ctypes.c_void_p(pack.data_ptr()), _stream(dev)), 'sbev_resnet_pack_weights')
    return pack, offs, bias_offs


def conv_f16(x, pack, residual, y, taps, stride, epilogue, col_tile=0):
    """sbev_conv_f16 on tensors, nothing allocated and nothing checked beyond what the C entry checks: ``x`` [n, H, W, Cin] and ``y``
    [n, h, w, Cout] contiguous fp16 (channels-last memory), ``pack`` one layer's image (``pack_layers``), ``residual`` as y or None,
    ``epilogue`` 'bias' / 'relu' / 'residual_relu'."""
    n, H, W, cin = (int(v) for v in x.shape)
    dev = x.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sbev_conv_f16(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(pack.data_ptr()),
                                             None if residual is None else ctypes.c_void_p(residual.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                             n, H, W, cin, int(y.shape[3]), int(taps), int(stride), EPILOGUES[epilogue], int(col_tile),
                                             _stream(dev)), 'sbev_conv_f16')
    return y


class _Bottleneck(nn.Module):
    """the parameters of one block under torchvision's / mmdet's names (the launches are the backbone's)"""

    def __init__(self, cin, mid, stride, downsample, eps):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, mid, 1, bias=False), nn.BatchNorm2d(mid, eps=eps)
        self.conv2, self.bn2 = nn.Conv2d(mid, mid, 3, stride, 1, bias=False), nn.BatchNorm2d(mid, eps=eps)
        self.conv3, self.bn3 = nn.Conv2d(mid, 4 * mid, 1, bias=False), nn.BatchNorm2d(4 * mid, eps=eps)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * mid, 1, stride, bias=False), nn.BatchNorm2d(4 * mid, eps=eps))

    def pairs(self):
        """(conv, bn) in launch order"""
        out = [(self.conv1, self.bn1), (self.conv2, self.bn2)]
        if hasattr(self, 'downsample'):
            out.append((self.downsample[0], self.downsample[1]))
        return out + [(self.conv3, self.bn3)]


class ResNetBackbone(nn.Module):
    """``ResNetBackbone(depth=50, num_stages=4, out_indices=(0, 1, 2, 3), style='pytorch', base_channels=64, norm_cfg=dict(type='BN2d',
    eps=1e-5), out_dtype=torch.float16)``: parameters and buffers under mmdet's / torchvision's ResNet names (a checkpoint's
    ``img_backbone.*`` entries load with ``strict=True``), He-normal weights.  ``stage_blocks`` overrides the blocks per stage (tests).
    Accepted without effect (inference only): ``frozen_stages``, ``norm_eval=True``, ``with_cp``, ``zero_init_residual``, ``init_cfg``,
    ``pretrained``, ``requires_grad`` inside ``norm_cfg``.  Not built, and refused by name: ``style='caffe'``, a depth below 50, ``dcn``,
    ``deep_stem``, ``avg_down``, dilations, ``norm_eval=False``, other strides, an ``out_dtype`` other than fp16."""

    def __init__(self, depth=50, num_stages=4, out_indices=(0, 1, 2, 3), style='pytorch', base_channels=64, norm_cfg=None,
                 out_dtype=torch.float16, stage_blocks=None, in_channels=3, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1), frozen_stages=-1,
                 norm_eval=True, with_cp=False, zero_init_residual=True, dcn=None, stage_with_dcn=(False, False, False, False),
                 deep_stem=False, avg_down=False, conv_cfg=None, plugins=None, init_cfg=None, pretrained=None):
        super().__init__()
        if style != 'pytorch':
            raise ValueError("ResNetBackbone: style=%r is not built (the stride sits on the 3 x 3: style='pytorch')" % (style,))
        if depth not in STAGE_BLOCKS:
            raise ValueError('ResNetBackbone: depth=%r is not built (the Bottleneck nets 50, 101, 152 are; 18 / 34 are BasicBlock nets)' % (depth,))
        if dcn is not None or any(stage_with_dcn):
            raise ValueError('ResNetBackbone: dcn is not built')
        if deep_stem:
            raise ValueError('ResNetBackbone: deep_stem is not built (the stem is one 7 x 7 / 2 convolution)')
        if avg_down:
            raise ValueError('ResNetBackbone: avg_down is not built (the downsample is a strided 1 x 1 convolution)')
        if any(d != 1 for d in dilations):
            raise ValueError('ResNetBackbone: dilations=%r are not built (1 everywhere)' % (tuple(dilations),))
        if not norm_eval:
            raise ValueError('ResNetBackbone: norm_eval=False is not built (BatchNorm runs in eval mode, folded into the convolutions)')
        if not 1 <= num_stages <= 4:
            raise ValueError('ResNetBackbone: num_stages=%r not in 1 .. 4' % (num_stages,))
        if tuple(strides[:num_stages]) != (1, 2, 2, 2)[:num_stages]:
            raise ValueError('ResNetBackbone: strides=%r are not built ((1, 2, 2, 2) is)' % (tuple(strides),))
        if in_channels != 3:
            raise ValueError('ResNetBackbone: in_channels=%r (3 is built)' % (in_channels,))
        if conv_cfg is not None or plugins is not None:
            raise ValueError('ResNetBackbone: conv_cfg / plugins are not built')
        if out_dtype != torch.float16:
            raise ValueError('ResNetBackbone: out_dtype=%r (torch.float16, what FPNNeck reads, is built)' % (out_dtype,))
        norm_cfg = dict(norm_cfg or {})
        if norm_cfg.get('type', 'BN2d') not in ('BN', 'BN2d'):
            raise ValueError('ResNetBackbone: norm_cfg type=%r is not built (BatchNorm2d is)' % (norm_cfg.get('type'),))
        self.eps = float(norm_cfg.get('eps', 1e-5))
        out_indices = tuple(int(i) for i in out_indices)
        if not out_indices or list(out_indices) != sorted(set(out_indices)) or out_indices[0] < 0 or out_indices[-1] >= num_stages:
            raise ValueError('ResNetBackbone: out_indices=%r must be increasing stage numbers below num_stages=%d' % (out_indices, num_stages))
        if base_channels < 64 or base_channels % 64:
            raise ValueError('ResNetBackbone: base_channels=%r must be a multiple of 64' % (base_channels,))
        blocks = tuple(STAGE_BLOCKS[depth][:num_stages]) if stage_blocks is None else tuple(int(b) for b in stage_blocks)
        if len(blocks) != num_stages or any(b < 1 for b in blocks):
            raise ValueError('ResNetBackbone: stage_blocks=%r must list num_stages=%d positive block counts' % (blocks, num_stages))
        self.depth, self.num_stages, self.out_indices, self.base_channels, self.stage_blocks = depth, num_stages, out_indices, base_channels, blocks
        self.out_channels = [4 * base_channels << s for s in out_indices]

        self.conv1 = nn.Conv2d(3, base_channels, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(base_channels, eps=self.eps)
        cin = base_channels
        for s, nb in enumerate(blocks):
            mid = base_channels << s
            stage = [_Bottleneck(cin, mid, 1 if s == 0 else 2, True, self.eps)]
            stage += [_Bottleneck(4 * mid, mid, 1, False, self.eps) for _ in range(nb - 1)]
            setattr(self, 'layer%d' % (s + 1), nn.Sequential(*stage))
            cin = 4 * mid
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        self._pack = None               # folded weight image at a fixed address per device
        self._pack_key = None
        self._workspaces = {}           # (device index, n, H, W, keep) -> (plan, uint8 workspace at a fixed address)

    # ---- weights
    def conv_bn_pairs(self):
        """(conv, bn) of every convolution in launch order: the stem, then per block conv1, conv2, [downsample], conv3"""
        pairs = [(self.conv1, self.bn1)]
        for s in range(self.num_stages):
            for block in getattr(self, 'layer%d' % (s + 1)):
                pairs += block.pairs()
        return pairs

    def pack(self):
        """Fold and pack now if any parameter or buffer changed since the last pack (forward does this itself).  Returns the image."""
        pairs = self.conv_bn_pairs()
        layers = [(c.weight, b.weight, b.bias, b.running_mean, b.running_var) for c, b in pairs]
        ws = [l[0] for l in layers]
        stats = [t for l in layers for t in l[1:]]
        dev = ws[0].device
        if dev.type != 'cuda':
            raise RuntimeError('ResNetBackbone needs its parameters on the device (no CPU fallback)')
        if any(w.device != dev or w.dtype != ws[0].dtype for w in ws) or ws[0].dtype not in _DTYPES:
            raise TypeError('ResNetBackbone: the convolution weights must be all fp32 or all fp16, on one device')
        if any(t.device != dev or t.dtype != torch.float32 for t in stats):
            raise TypeError('ResNetBackbone: the BatchNorm weights and statistics must be fp32, on the weights\' device')
        key = tuple((t.data_ptr(), t._version) for l in layers for t in l)
        if key == self._pack_key:
            return self._pack
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ResNetBackbone.forward under a capture with weights that are not packed: run one forward (or pack()) before '
                               'the capture')
        if any(not t.is_contiguous() for l in layers for t in l):
            raise ValueError('ResNetBackbone: parameters and buffers must be contiguous')
        if self._pack is not None and self._pack.device != dev:
            self._pack = None
        self._pack = pack_layers(layers, self.eps, self._pack)[0]
        self._pack_key = key
        return self._pack

    # ---- the call
    def plan(self, n, H, W, keep=False):
        return plan(self.depth, n, H, W, self.out_indices, self.num_stages, self.base_channels, self.stage_blocks, keep)

    def forward(self, x, out=None, keep=None):
        """x: [n, 3, H, W] device tensor, NCHW-contiguous, fp32 or fp16.  Returns the ``out_indices`` stage outputs [n, C, h, w], fp16,
        channels-last in memory (permuted views of [n, h, w, C] buffers).  ``out``: a list of existing destinations of those shapes in
        channels-last memory: with it the call allocates nothing once it has run for this shape, and can be captured.  ``keep``: a
        list (tests) that receives every launch's output in launch order as [n, C, h, w] views; the stage outputs among them are the
        returned tensors."""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError('ResNetBackbone: x must be [n, 3, H, W]')
        if not x.is_cuda:
            raise RuntimeError('ResNetBackbone needs device tensors (no CPU fallback)')
        if x.dtype not in _DTYPES:
            raise TypeError('ResNetBackbone: x must be fp32 or fp16 (got %s)' % x.dtype)
        if not x.is_contiguous():
            raise ValueError('ResNetBackbone: x is not NCHW-contiguous (ImageFrontEnd emits NCHW; no copy is made here)')
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError('ResNetBackbone is inference only (its backward is not built): call it under torch.no_grad() and keep the '
                               'parameters frozen')
        dev = x.device
        n, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        if H < 1 or W < 1:
            raise ValueError('ResNetBackbone: an empty image (%d x %d)' % (H, W))
        if self.conv1.weight.device != dev:
            raise ValueError('ResNetBackbone: x is on %s, the parameters on %s' % (dev, self.conv1.weight.device))
        with torch.cuda.device(dev):
            wpack = self.pack()
            key = (dev.index, n, H, W, keep is not None)
            if key not in self._workspaces:
                p = self.plan(n, H, W, keep is not None)
                self._workspaces[key] = (p, torch.empty(max(p['workspace_bytes'], 256), dtype=torch.uint8, device=dev))
            p, ws = self._workspaces[key]
            shapes = [(n, c, h, w) for c, h, w in p['outs']]
            if out is None:
                out = [torch.empty((n, h, w, c), dtype=torch.float16, device=dev).permute(0, 3, 1, 2) for _, c, h, w in shapes]
            else:
                out = list(out)
                if len(out) != len(shapes):
                    raise ValueError('ResNetBackbone: out must list %d tensors' % len(shapes))
                for o, s in zip(out, shapes):
                    if tuple(o.shape) != s or o.dtype != torch.float16 or o.device != dev or (o.numel() and not o.permute(0, 2, 3, 1).is_contiguous()):
                        raise ValueError('ResNetBackbone: out must be fp16 tensors of shape %s in channels-last memory on %s' % (s, dev))
            blocks = _i32(self.stage_blocks)
            _lib.check(_lib.load().sbev_resnet_forward(
                self.depth, blocks, self.num_stages, self.base_channels, n, H, W, len(self.out_indices), _i32(self.out_indices),
                int(keep is not None), ctypes.c_void_p(x.data_ptr()), _DTYPES[x.dtype], ctypes.c_void_p(wpack.data_ptr()),
                ctypes.c_void_p(ws.data_ptr()), _vp_array(out), _stream(dev)), 'sbev_resnet_forward')
        if keep is not None:
            for l in p['layers']:
                if l['where'] < 0:
                    keep.append(out[-1 - l['where']])
                else:
                    nbytes = n * l['h'] * l['w'] * l['cout'] * 2
                    keep.append(ws[l['where']:l['where'] + nbytes].view(torch.float16).view(n, l['h'], l['w'], l['cout']).permute(0, 3, 1, 2))
        return out
