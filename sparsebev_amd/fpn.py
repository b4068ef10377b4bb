"""FPNNeck: the detector's neck (mmdet's ``FPN`` with ``in_channels`` = the backbone's stages, ``out_channels=256``, ``num_outs`` levels,
no extra convolutions: configs/r50_nuimg_704x256.py:41-45) on the matrix core, as L + 1 launches of csrc/fpn.hip for all images of a call:
the backbone's stage outputs in channels-last memory in, the channels-last pyramid out that ``FeaturePyramid`` takes in place and
``FramePool.stream`` lets travel with its pyramid.  Inference only.

Reference counterpart: ``FPN.forward`` under fp16 autocast (models/sparsebev.py:46) -- 2 L convolutions, L - 1 interpolate + add pairs and
the casts around them, one launch each -- and the NCHW -> channels-last relayout in front of the decoder.

Arithmetic (include/sbev_hip.h: sbev_fpn_forward): inputs and weights as fp16 (fp32 ones rounded once, to nearest even), products
accumulated in fp32, fp32 biases; the merged lateral ``M_l = fp16(conv1x1(C_l) + b_l + float(M_{l+1}[nearest]))`` is rounded once (the
reference's autocast chain rounds the lateral and then adds in fp16: one rounding more); ``P_l = conv3x3(M_l) + b_l`` is stored as
fp32 or rounded once to fp16; an extra level is ``prev[:, :, ::2, ::2]``.

The weights are packed into MFMA fragment order once per weight version (the parameters' ``_version`` and address: an optimizer step,
``load_state_dict`` or ``.to()`` repacks at the next call); the biases are read where they are.  There is no CPU path and no silent
copy: a CPU tensor, NCHW-contiguous memory, mixed dtypes or a wrong channel count raise.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib

MAX_IN, MAX_OUT, PLAN_WORDS = 4, 5, 18          # SBEV_FPN_MAX_IN, SBEV_FPN_MAX_OUT, SBEV_FPN_PLAN_WORDS
_DTYPES = {torch.float32: 0, torch.float16: 2}   # SBEV_F32, SBEV_F16


def nearest_index(in_size, out_size):
    """Source index of every destination index of ``F.interpolate(size=out_size, mode='nearest')`` along one axis, torch's float32
    rule: min(floor(dst * float32(in / out)), in - 1), the product rounded in float32.  int64 numpy array [out_size]."""
    scale = np.float32(in_size) / np.float32(out_size)
    idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def plan(chw, n, num_outs):
    """sbev_fpn_plan, a pure host function, for levels ``chw`` = [(Cin, H, W), ...] (finest first), ``n`` images and ``num_outs``
    outputs: a dict of launches, pack_bytes, workspace_bytes, pixels, conv_tiles, lateral_tiles [L], extra [(H, W), ...].  Raises
    SbevError where the plan refuses."""
    flat = [int(v) for level in chw for v in level]
    arr = (ctypes.c_int32 * max(len(flat), 1))(*flat)
    out = (ctypes.c_int64 * PLAN_WORDS)()
    _lib.check(_lib.load().sbev_fpn_plan(len(chw), arr, int(n), int(num_outs), out), 'sbev_fpn_plan')
    v = [int(x) for x in out]
    return dict(launches=v[0], pack_bytes=v[1], workspace_bytes=v[2], pixels=v[3], conv_tiles=v[4], lateral_tiles=v[5:5 + len(chw)],
                extra=[(v[10 + 2 * e], v[11 + 2 * e]) for e in range(v[9])])


def _vp_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


class FPNNeck(nn.Module):
    """``FPNNeck(in_channels, out_channels=256, num_outs=None)``: parameters under mmdet's names (``lateral_convs.{i}.conv.weight`` /
    ``.bias``, ``fpn_convs.{i}.conv.weight`` / ``.bias``), Xavier-uniform weights and zero biases as mmdet's ``init_cfg`` gives them.
    ``num_outs`` None: one output per input."""

    def __init__(self, in_channels, out_channels=256, num_outs=None):
        super().__init__()
        in_channels = [int(c) for c in in_channels]
        num_outs = len(in_channels) if num_outs is None else int(num_outs)
        if out_channels != 256:
            raise ValueError('FPNNeck: out_channels=%r (256 is built)' % (out_channels,))
        if not 1 <= len(in_channels) <= MAX_IN:
            raise ValueError('FPNNeck: %d input levels (1 .. %d are built)' % (len(in_channels), MAX_IN))
        if not len(in_channels) <= num_outs <= MAX_OUT:
            raise ValueError('FPNNeck: num_outs=%d not in %d .. %d (add_extra_convs is not built)' % (num_outs, len(in_channels), MAX_OUT))
        if any(c < 32 or c % 32 for c in in_channels):
            raise ValueError('FPNNeck: in_channels %s must be multiples of 32' % (in_channels,))
        self.in_channels, self.out_channels, self.num_outs = in_channels, 256, num_outs

        def conv(cin, k):
            holder = nn.Module()
            holder.conv = nn.Conv2d(cin, 256, k, padding=k // 2)
            nn.init.xavier_uniform_(holder.conv.weight)
            nn.init.zeros_(holder.conv.bias)
            return holder

        self.lateral_convs = nn.ModuleList([conv(c, 1) for c in in_channels])
        self.fpn_convs = nn.ModuleList([conv(256, 3) for _ in in_channels])
        self.merged = None              # the last forward's merged laterals M_l: [n, 256, H_l, W_l] fp16 views of the workspace
        self._pack = None               # fp16 weight image at a fixed address per device
        self._pack_key = None
        self._workspaces = {}           # (device index, n, planes) -> fp16 workspace at a fixed address

    # ---- weights
    def _weights(self):
        return [m.conv.weight for m in self.lateral_convs], [m.conv.weight for m in self.fpn_convs]

    def _biases(self):
        return [m.conv.bias for m in self.lateral_convs], [m.conv.bias for m in self.fpn_convs]

    def pack(self, stream=None):
        """Pack the weights now if they changed since the last pack (forward does this itself).  Returns the fp16 image."""
        lat, out = self._weights()
        ws = lat + out
        dev = ws[0].device
        if dev.type != 'cuda':
            raise RuntimeError('FPNNeck needs its parameters on the device (no CPU fallback)')
        if any(w.device != dev or w.dtype != ws[0].dtype for w in ws) or ws[0].dtype not in _DTYPES:
            raise TypeError('FPNNeck: the convolution weights must be all fp32 or all fp16, on one device')
        key = tuple((w.data_ptr(), w._version) for w in ws)
        if key == self._pack_key:
            return self._pack
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FPNNeck.forward under a capture with weights that are not packed: run one forward (or pack()) before the capture')
        if any(not w.is_contiguous() for w in ws):
            raise ValueError('FPNNeck: the convolution weights must be contiguous')
        chw = [(c, 1, 1) for c in self.in_channels]
        with torch.cuda.device(dev):
            if self._pack is None or self._pack.device != dev:
                self._pack = torch.empty(plan(chw, 0, len(chw))['pack_bytes'] // 2, dtype=torch.float16, device=dev)
            flat = (ctypes.c_int32 * (3 * len(chw)))(*[v for level in chw for v in level])
            s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if stream is None else stream
            _lib.check(_lib.load().sbev_fpn_pack_weights(len(chw), flat, _vp_array([w.data_ptr() for w in lat]), _vp_array([w.data_ptr() for w in out]),
                                                         _DTYPES[ws[0].dtype], ctypes.c_void_p(self._pack.data_ptr()), s), 'sbev_fpn_pack_weights')
        self._pack_key = key
        return self._pack

    # ---- the call
    def out_shapes(self, inputs):
        """[n, 256, H, W] of every output for these inputs"""
        n = inputs[0].shape[0]
        hw = [(int(x.shape[2]), int(x.shape[3])) for x in inputs]
        for _ in range(self.num_outs - len(inputs)):
            hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
        return [(n, 256, h, w) for h, w in hw]

    def forward(self, inputs, out=None, out_dtype=torch.float16):
        """inputs: list[L] of [n, Cin_l, H_l, W_l] device tensors in channels-last memory, all fp16 or all fp32.  Returns ``num_outs``
        tensors [n, 256, H_l, W_l], channels-last in memory (permuted views of [n, H_l, W_l, 256] buffers), of ``out_dtype`` (fp16 or
        fp32).  ``out``: a list of existing destinations of those shapes in channels-last memory (their dtype is the output type): with
        it the call allocates nothing once it has run for these shapes, and can be captured."""
        inputs = list(inputs)
        L = len(self.in_channels)
        if len(inputs) != L or not all(torch.is_tensor(x) and x.dim() == 4 for x in inputs):
            raise ValueError('FPNNeck: %d inputs [n, C, H, W] expected' % L)
        dev, dt, n = inputs[0].device, inputs[0].dtype, inputs[0].shape[0]
        if any(x.dtype != dt for x in inputs) or dt not in _DTYPES:
            raise TypeError('FPNNeck: inputs must be all fp16 or all fp32 (got %s)' % ', '.join(str(x.dtype) for x in inputs))
        if any(x.device != dev or x.shape[0] != n for x in inputs):
            raise ValueError('FPNNeck: inputs must share one device and one image count')
        for l, (x, c) in enumerate(zip(inputs, self.in_channels)):
            if x.shape[1] != c:
                raise ValueError('FPNNeck: input %d has %d channels, in_channels[%d] = %d' % (l, x.shape[1], l, c))
            if x.numel() and not x.permute(0, 2, 3, 1).is_contiguous():
                raise ValueError('FPNNeck: input %d is not channels-last in memory: hand the backbone\'s output over with '
                                 'memory_format=torch.channels_last (no copy is made here)' % l)
        lat_b, out_b = self._biases()
        if torch.is_grad_enabled() and (any(x.requires_grad for x in inputs) or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError('FPNNeck is inference only (the backward of the neck is not built): call it under torch.no_grad()')
        if not all(x.is_cuda for x in inputs):
            raise RuntimeError('FPNNeck needs device tensors (no CPU fallback)')
        if any(b.dtype != torch.float32 or b.device != dev or not b.is_contiguous() for b in lat_b + out_b):
            raise TypeError('FPNNeck: the biases must be contiguous fp32 tensors on the inputs\' device')
        shapes = self.out_shapes(inputs)
        if out is None:
            if out_dtype not in _DTYPES:
                raise TypeError('FPNNeck: out_dtype must be torch.float16 or torch.float32')
            out = [torch.empty((s[0], s[2], s[3], s[1]), dtype=out_dtype, device=dev).permute(0, 3, 1, 2) for s in shapes]
        else:
            out = list(out)
            if len(out) != len(shapes):
                raise ValueError('FPNNeck: out must list %d tensors' % len(shapes))
            out_dtype = out[0].dtype
            if out_dtype not in _DTYPES:
                raise TypeError('FPNNeck: out must be fp16 or fp32')
            for o, s in zip(out, shapes):
                if tuple(o.shape) != s or o.dtype != out_dtype or o.device != dev or (o.numel() and not o.permute(0, 2, 3, 1).is_contiguous()):
                    raise ValueError('FPNNeck: out must be %s tensors of shape %s in channels-last memory on %s' % (out_dtype, s, dev))
        chw = [(c, x.shape[2], x.shape[3]) for c, x in zip(self.in_channels, inputs)]
        flat = (ctypes.c_int32 * (3 * L))(*[int(v) for level in chw for v in level])
        with torch.cuda.device(dev):
            key = (dev.index, n, tuple(chw))
            ws = self._workspaces.get(key)
            if ws is None:
                p = plan(chw, n, self.num_outs)
                ws = self._workspaces[key] = torch.empty(max(p['workspace_bytes'] // 2, 8), dtype=torch.float16, device=dev)
            wpack = self.pack()
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.load().sbev_fpn_forward(
                L, flat, n, self.num_outs, _vp_array([x.data_ptr() for x in inputs]), _DTYPES[dt], ctypes.c_void_p(wpack.data_ptr()),
                _vp_array([b.data_ptr() for b in lat_b]), _vp_array([b.data_ptr() for b in out_b]), ctypes.c_void_p(ws.data_ptr()),
                _vp_array([o.data_ptr() for o in out]), _DTYPES[out_dtype], stream), 'sbev_fpn_forward')
        self.merged, at = [], 0
        for _, h, w in chw:
            self.merged.append(ws[at:at + n * h * w * 256].view(n, h, w, 256).permute(0, 3, 1, 2))
            at += n * h * w * 256
        return out
