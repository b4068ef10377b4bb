"""FPNNeck: the detector's neck (mmdet's ``FPN`` with ``in_channels`` = the backbone's stages, ``out_channels=256``, ``num_outs`` levels,
no extra convolutions: configs/r50_nuimg_704x256.py:41-45) on the matrix core, as L + 1 launches of csrc/fpn.hip for all images of a call:
the backbone's stage outputs in channels-last memory in, the channels-last pyramid out that ``FeaturePyramid`` takes in place and
``FramePool.stream`` lets travel with its pyramid.  ``FPNNeck(..., trainable=True)`` also trains: a forward under grad goes through
``NeckFunction`` and its backward is csrc/fpn_bwd.hip (sbev_fpn_backward: 4 L + 1 launches, 5 L + 1 with input gradients).

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

from . import _lib, dense

MAX_IN, MAX_OUT, PLAN_WORDS = 4, 5, 18          # SBEV_FPN_MAX_IN, SBEV_FPN_MAX_OUT, SBEV_FPN_PLAN_WORDS
BWD_PLAN_WORDS, GRAD_WINDOW_LOG2 = 16, 3         # SBEV_FPN_BWD_PLAN_WORDS, SBEV_FPN_GRAD_WINDOW_LOG2
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


def children(in_size, out_size):
    """The preimage of ``nearest_index(in_size, out_size)``: (start, stop) int64 arrays [in_size]; destination indices start[s] ..
    stop[s] - 1 read source index s (the rule is monotone, so a preimage is a range; it is empty where no destination reads s).  The
    top-down adjoint of the neck's backward sums a parent's children over exactly these ranges."""
    idx = nearest_index(in_size, out_size)
    s = np.arange(in_size)
    return np.searchsorted(idx, s, side='left').astype(np.int64), np.searchsorted(idx, s, side='right').astype(np.int64)


def backward_plan(chw, n, num_outs, input_grads=False):
    """sbev_fpn_backward_plan, a pure host function: a dict of launches, workspace_bytes, pack_bytes, slabs [L], slab_len [L] and the
    byte offsets gm_offset, d_offset, part_offset of the scaled lateral gradients, the 3x3 data gradients of levels 1 .. and the slab
    partials inside the workspace.  Raises SbevError where the plan refuses."""
    flat = [int(v) for level in chw for v in level]
    arr = (ctypes.c_int32 * max(len(flat), 1))(*flat)
    out = (ctypes.c_int64 * BWD_PLAN_WORDS)()
    _lib.check(_lib.load().sbev_fpn_backward_plan(len(chw), arr, int(n), int(num_outs), int(bool(input_grads)), out), 'sbev_fpn_backward_plan')
    v = [int(x) for x in out]
    L = len(chw)
    return dict(launches=v[0], workspace_bytes=v[1], pack_bytes=v[2], slabs=v[3:3 + L], slab_len=v[7:7 + L], gm_offset=v[11], d_offset=v[12],
                part_offset=v[13])


def backward_raw(chw, n, num_outs, inputs, merged, grad_outs, pack_bwd, workspace, grad_inputs, grad_lateral_w, grad_lateral_b, grad_fpn_w,
                 grad_fpn_b, stream=None):
    """sbev_fpn_backward on tensors, nothing allocated and nothing checked beyond what the C entry checks: ``inputs`` / ``grad_outs`` lists
    of channels-last tensors (one dtype each), ``merged`` the forward's fp16 workspace, ``grad_inputs`` None or a list with None entries
    for the levels that need no gradient, the four parameter-gradient lists fp32 destinations."""
    L = len(chw)
    flat = (ctypes.c_int32 * (3 * L))(*[int(v) for level in chw for v in level])
    dev = workspace.device
    with torch.cuda.device(dev):
        s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if stream is None else stream
        ptrs = dense.ptr_array
        _lib.check(_lib.load().sbev_fpn_backward(
            L, flat, int(n), int(num_outs), ptrs(inputs), _DTYPES[inputs[0].dtype], ctypes.c_void_p(merged.data_ptr()), ptrs(grad_outs),
            _DTYPES[grad_outs[0].dtype], ctypes.c_void_p(pack_bwd.data_ptr()), ctypes.c_void_p(workspace.data_ptr()),
            None if grad_inputs is None else ptrs(grad_inputs), ptrs(grad_lateral_w), ptrs(grad_lateral_b), ptrs(grad_fpn_w), ptrs(grad_fpn_b),
            s), 'sbev_fpn_backward')


class NeckFunction(torch.autograd.Function):
    """A trainable neck's forward under grad.  The node keeps the inputs and parameters by reference (``save_for_backward``: no copy, and
    an in-place write between forward and backward is an error) and owns the buffer of its merged laterals, so several forwards may
    precede their backwards.  backward: the output gradients arrive materialised (zeros for an unused output); one that is not
    channels-last in memory is converted by ONE torch copy; the parameter gradients are fresh fp32 tensors from ``autograd``'s
    parameter-gradient sink, the input gradients (only for inputs that require one) channels-last tensors of the inputs' dtype."""

    @staticmethod
    def forward(ctx, neck, chw, out_dtype, *tensors):
        L = len(chw)
        inputs = tensors[:L]
        n, dev = inputs[0].shape[0], inputs[0].device
        with torch.cuda.device(dev):
            merged = torch.empty(max(plan(chw, n, neck.num_outs)['workspace_bytes'] // 2, 8), dtype=torch.float16, device=dev)
            out = [torch.empty((s[0], s[2], s[3], s[1]), dtype=out_dtype, device=dev).permute(0, 3, 1, 2) for s in neck.out_shapes(inputs)]
            neck.pack_bwd()
        neck._launch(inputs, chw, merged, out, out_dtype)
        ctx.neck, ctx.chw, ctx.merged = neck, chw, merged
        neck.merged = neck._merged_views(merged, chw, n)         # views of THIS node's buffer, until the next forward
        ctx.save_for_backward(*tensors)
        return tuple(out)

    @staticmethod
    def backward(ctx, *grad_outs):
        from . import autograd as A
        neck, chw, L = ctx.neck, ctx.chw, len(ctx.chw)
        tensors = ctx.saved_tensors
        inputs, lat_w, lat_b, out_w, out_b = (tensors[i * L:(i + 1) * L] for i in range(5))
        n, dev = inputs[0].shape[0], inputs[0].device
        gs = [g if g.permute(0, 2, 3, 1).is_contiguous() else g.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for g in grad_outs]
        if any(g.dtype != gs[0].dtype for g in gs) or gs[0].dtype not in _DTYPES:
            raise TypeError('FPNNeck backward: the output gradients must be all fp16 or all fp32')
        need = ctx.needs_input_grad[3:3 + L]
        with torch.cuda.device(dev):
            sink = lambda p: A._NO_TAP.sink(False, id(p), p, tuple(p.shape))[0]
            gwl, gbl, gw3, gb3 = ([sink(p) for p in ps] for ps in (lat_w, lat_b, out_w, out_b))
            gx = [torch.empty_like(x) if want else None for x, want in zip(inputs, need)] if any(need) else None
            if n == 0:
                for t in gwl + gbl + gw3 + gb3:
                    t.zero_()
            ws = neck._backward_workspace(chw, n, gx is not None, dev)
            backward_raw(chw, n, neck.num_outs, inputs, ctx.merged, gs, neck.pack_bwd(), ws, gx, gwl, gbl, gw3, gb3)
        params = [A._NO_TAP.commit(False, id(p), g) if want else None
                  for p, g, want in zip(lat_w + lat_b + out_w + out_b, gwl + gbl + gw3 + gb3, ctx.needs_input_grad[3 + L:])]
        return (None, None, None, *(gx if gx is not None else [None] * L), *params)


class FPNNeck(nn.Module):
    """``FPNNeck(in_channels, out_channels=256, num_outs=None, trainable=False)``: parameters under mmdet's names
    (``lateral_convs.{i}.conv.weight`` / ``.bias``, ``fpn_convs.{i}.conv.weight`` / ``.bias``), Xavier-uniform weights and zero biases as
    mmdet's ``init_cfg`` gives them.  ``num_outs`` None: one output per input.  ``trainable`` False: a forward that would need a gradient
    is refused (inference only).  ``trainable`` True: such a forward goes through ``NeckFunction``; under ``torch.no_grad()`` nothing
    differs.  Inside a ``dense.step_images()`` scope (a captured training step) both weight packs are derived once per scope by the step's
    own pack calls into fresh tensors and the ``_version``-keyed caches are left alone; a trainable forward may then be captured.  Not
    built, and refused where asked for: a trainable forward under a graph capture outside such a scope, ``add_extra_convs``, NCHW inputs, an fp16 hi + lo
    mode of the gradient operands."""

    def __init__(self, in_channels, out_channels=256, num_outs=None, trainable=False, add_extra_convs=False, grad_mode='f16'):
        super().__init__()
        if add_extra_convs:
            raise ValueError('FPNNeck: add_extra_convs=%r is not built (extra levels are stride-2 slices of the last output)' % (add_extra_convs,))
        if grad_mode != 'f16':
            raise ValueError("FPNNeck: grad_mode=%r is not built (the gradient operands are single fp16 values in the scaled domain: 'f16'; "
                             'there is no fp16 hi + lo mode)' % (grad_mode,))
        self.trainable = bool(trainable)
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
        # the fp16 weight image and the backward's (flipped / transposed), each at a fixed address per device, keyed on the weights' versions
        self._image = dense.WeightImage('fpn_pack', 'FPNNeck.forward under a capture with weights that are not packed: run one forward '
                                        '(or pack()) before the capture')
        self._image_bwd = dense.WeightImage('fpn_pack_bwd', 'FPNNeck backward under a capture with weights that are not packed')
        self._workspaces = {}           # (device index, n, planes) -> fp16 workspace at a fixed address
        self._bwd_workspaces = {}       # (device index, n, planes, input gradients) -> byte workspace of the backward

    # ---- weights
    def _weights(self):
        return [m.conv.weight for m in self.lateral_convs], [m.conv.weight for m in self.fpn_convs]

    def _biases(self):
        return [m.conv.bias for m in self.lateral_convs], [m.conv.bias for m in self.fpn_convs]

    def _checked_weights(self):
        """(lateral weights, output weights), all fp32 or all fp16 on one device"""
        lat, out = self._weights()
        ws = lat + out
        dev = ws[0].device
        if dev.type != 'cuda':
            raise RuntimeError('FPNNeck needs its parameters on the device (no CPU fallback)')
        if any(w.device != dev or w.dtype != ws[0].dtype for w in ws) or ws[0].dtype not in _DTYPES:
            raise TypeError('FPNNeck: the convolution weights must be all fp32 or all fp16, on one device')
        return lat, out

    def pack(self, stream=None):
        """Pack the weights now if they changed since the last pack (forward does this itself).  Returns the fp16 image."""
        lat, out = self._checked_weights()
        return self._image.get(lat + out, lambda dest: self._pack_launch(False, lat, out, dest, stream))

    def _pack_launch(self, bwd, lat, out, dest, stream):
        """sbev_fpn_pack_weights (``bwd``: sbev_fpn_pack_weights_bwd) on checked weights into ``dest`` (None: a fresh tensor)"""
        ws = lat + out
        dev = ws[0].device
        if any(not w.is_contiguous() for w in ws):
            raise ValueError('FPNNeck: the convolution weights must be contiguous')
        chw = [(c, 1, 1) for c in self.in_channels]
        name = 'sbev_fpn_pack_weights_bwd' if bwd else 'sbev_fpn_pack_weights'
        with torch.cuda.device(dev):
            if dest is None:
                nbytes = (backward_plan if bwd else plan)(chw, 0, len(chw))['pack_bytes']
                dest = torch.empty(nbytes // 2, dtype=torch.float16, device=dev)
            flat = (ctypes.c_int32 * (3 * len(chw)))(*[v for level in chw for v in level])
            s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if stream is None else stream
            _lib.check(getattr(_lib.load(), name)(len(chw), flat, dense.ptr_array(lat), dense.ptr_array(out),
                                                  _DTYPES[ws[0].dtype], ctypes.c_void_p(dest.data_ptr()), s), name)
        return dest

    def pack_bwd(self, stream=None):
        """The backward's weight image (sbev_fpn_pack_weights_bwd), packed now if the weights changed since its last pack."""
        lat, out = self._checked_weights()
        return self._image_bwd.get(lat + out, lambda dest: self._pack_launch(True, lat, out, dest, stream))

    def _backward_workspace(self, chw, n, input_grads, dev):
        key = (dev.index, n, tuple(chw), bool(input_grads))
        ws = self._bwd_workspaces.get(key)
        if ws is None:
            nbytes = backward_plan(chw, n, self.num_outs, input_grads)['workspace_bytes']
            ws = self._bwd_workspaces[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        return ws

    def _launch(self, inputs, chw, ws, out, out_dtype):
        """sbev_fpn_forward on checked arguments: the merged laterals into ``ws``, the outputs into ``out``"""
        L, dev, n = len(chw), inputs[0].device, inputs[0].shape[0]
        lat_b, out_b = self._biases()
        flat = (ctypes.c_int32 * (3 * L))(*[int(v) for level in chw for v in level])
        with torch.cuda.device(dev):
            wpack = self.pack()
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.load().sbev_fpn_forward(
                L, flat, n, self.num_outs, dense.ptr_array(inputs), _DTYPES[inputs[0].dtype], ctypes.c_void_p(wpack.data_ptr()),
                dense.ptr_array(lat_b), dense.ptr_array(out_b), ctypes.c_void_p(ws.data_ptr()),
                dense.ptr_array(out), _DTYPES[out_dtype], stream), 'sbev_fpn_forward')

    def _merged_views(self, ws, chw, n):
        views, at = [], 0
        for _, h, w in chw:
            views.append(ws[at:at + n * h * w * 256].view(n, h, w, 256).permute(0, 3, 1, 2))
            at += n * h * w * 256
        return views

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
        wants_grad = torch.is_grad_enabled() and (any(x.requires_grad for x in inputs) or any(p.requires_grad for p in self.parameters()))
        if wants_grad and not self.trainable:
            raise RuntimeError('FPNNeck is inference only unless built with trainable=True: call it under torch.no_grad()')
        if not all(x.is_cuda for x in inputs):
            raise RuntimeError('FPNNeck needs device tensors (no CPU fallback)')
        if any(b.dtype != torch.float32 or b.device != dev or not b.is_contiguous() for b in lat_b + out_b):
            raise TypeError('FPNNeck: the biases must be contiguous fp32 tensors on the inputs\' device')
        shapes = self.out_shapes(inputs)
        if wants_grad:
            if out is not None:
                raise ValueError('FPNNeck: out= is not taken by a forward that needs a gradient (autograd owns its outputs)')
            if out_dtype not in _DTYPES:
                raise TypeError('FPNNeck: out_dtype must be torch.float16 or torch.float32')
            if torch.cuda.is_current_stream_capturing() and not dense.in_step_images():
                raise RuntimeError('FPNNeck: a trainable forward under a graph capture (the neck inside CapturedHeadTrainStep) is not built: '
                                   'the weight packs would have to move into the graph')
            chw = tuple((c, int(x.shape[2]), int(x.shape[3])) for c, x in zip(self.in_channels, inputs))
            lat_w, out_w = self._weights()
            return list(NeckFunction.apply(self, chw, out_dtype, *inputs, *lat_w, *lat_b, *out_w, *out_b))
        if out is None:
            if out_dtype not in _DTYPES:
                raise TypeError('FPNNeck: out_dtype must be torch.float16 or torch.float32')
            out = [torch.empty((s[0], s[2], s[3], s[1]), dtype=out_dtype, device=dev).permute(0, 3, 1, 2) for s in shapes]
        else:
            out, out_dtype = dense.channels_last_out('FPNNeck', out, shapes, dev)
        chw = [(c, x.shape[2], x.shape[3]) for c, x in zip(self.in_channels, inputs)]
        with torch.cuda.device(dev):
            key = (dev.index, n, tuple(chw))
            ws = self._workspaces.get(key)
            if ws is None:
                p = plan(chw, n, self.num_outs)
                ws = self._workspaces[key] = torch.empty(max(p['workspace_bytes'] // 2, 8), dtype=torch.float16, device=dev)
        self._launch(inputs, chw, ws, out, out_dtype)
        self.merged = self._merged_views(ws, chw, n)
        return out
