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
in-place write, ``load_state_dict`` or ``.to()`` repacks at the next call).  By default inference only: the parameters are created with
``requires_grad=False`` and a forward that would need a gradient raises.  ``ResNetBackbone(..., trainable=True, frozen_stages=f)`` also
trains stages f + 1 .. (configs/r50_nuimg_704x256.py:31-40 with ``norm_eval=True``): a forward under grad goes through
``BackboneFunction`` and its backward is csrc/resnet_bwd.hip (sbev_resnet_backward).  There is no CPU path and no silent copy.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib, dense

MAX_LAYERS, PLAN_HEAD, LAYER_WORDS = 160, 18, 12        # SBEV_RESNET_MAX_LAYERS, SBEV_RESNET_PLAN_HEAD, SBEV_RESNET_LAYER_WORDS
PLAN_WORDS = PLAN_HEAD + LAYER_WORDS * MAX_LAYERS
STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
KINDS = ('stem', 'pool', 'conv')
EPILOGUES = {'bias': 0, 'relu': 1, 'residual_relu': 2}
_DTYPES = {torch.float32: 0, torch.float16: 2}          # SBEV_F32, SBEV_F16


def _i32(values):
    values = [int(v) for v in values]
    return (ctypes.c_int32 * max(len(values), 1))(*values)


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
        cols = [dense.ptr_array([l[j] for l in layers]) for j in range(5)]
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


BWD_PLAN_HEAD, BWD_LAYER_WORDS, GRAD_WINDOW_LOG2 = 16, 6, 3      # SBEV_RESNET_BWD_PLAN_HEAD, .._LAYER_WORDS, SBEV_RESNET_GRAD_WINDOW_LOG2
BWD_PLAN_WORDS = BWD_PLAN_HEAD + BWD_LAYER_WORDS * MAX_LAYERS
REPACK_HEAD, REPACK_LAYER_WORDS = 8, 12                          # SBEV_RESNET_REPACK_HEAD, SBEV_RESNET_REPACK_LAYER_WORDS
REPACK_WORDS = REPACK_HEAD + REPACK_LAYER_WORDS * MAX_LAYERS


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def wgrad_slabs(pixels):
    """(slabs, slab_len) of a weight gradient's reduction over ``pixels`` output pixels: slab_len = max(512, ceil(pixels / 16) rounded up
    to a multiple of 256) -- part of the backward's definition (include/sbev_hip.h: sbev_resnet_backward)"""
    slab_len = max(512, -(-(-(-pixels // 16)) // 256) * 256)
    return -(-pixels // slab_len), slab_len


def backward_plan(depth, n, H, W, out_indices=(0, 1, 2, 3), num_stages=4, base_channels=64, stage_blocks=None, first_trainable_stage=2):
    """sbev_resnet_backward_plan, a pure host function: a dict of launches, workspace_bytes, pack_bytes (the backward's image),
    acts_bytes (the activation buffer of a trainable forward), forward_workspace_bytes, forward_pack_bytes, first_kept, the byte offsets
    g3_offsets / g2_offset / g1_offset / part_offset inside the workspace, and layers: per launch slabs, slab_len, kept (a byte offset
    in acts, -(2 + k): outs[k], -1: not kept), pack_offset (-1: no image), trainable, dgrad.  Raises SbevError where the plan refuses."""
    out = (ctypes.c_int64 * BWD_PLAN_WORDS)()
    blocks = None if stage_blocks is None else _i32(stage_blocks)
    if stage_blocks is not None and len(stage_blocks) != num_stages:
        raise ValueError('stage_blocks must list num_stages=%d block counts' % num_stages)
    _lib.check(_lib.load().sbev_resnet_backward_plan(int(depth), blocks, int(num_stages), int(base_channels), int(n), int(H), int(W),
                                                     len(out_indices), _i32(out_indices), int(first_trainable_stage), out),
               'sbev_resnet_backward_plan')
    v = [int(x) for x in out]
    names = ('slabs', 'slab_len', 'kept', 'pack_offset', 'trainable', 'dgrad')
    layers = [dict(zip(names, v[BWD_PLAN_HEAD + BWD_LAYER_WORDS * i:BWD_PLAN_HEAD + BWD_LAYER_WORDS * (i + 1)])) for i in range(v[5])]
    return dict(launches=v[0], workspace_bytes=v[1], pack_bytes=v[2], acts_bytes=v[3], forward_workspace_bytes=v[4], first_kept=v[6],
                g3_offsets=(v[7], v[8]), g2_offset=v[9], g1_offset=v[10], part_offset=v[11], forward_pack_bytes=v[12], layers=layers)


def pack_layers_bwd(layers, eps=1e-5, pack=None):
    """sbev_resnet_pack_weights_bwd on a list of ``(weight, gamma, var)`` device tensors: the transposed (3 x 3: and flipped) fragment
    images of w', layer after layer.  Returns (the uint8 pack tensor, the byte offset of every layer's image)."""
    ws = [l[0] for l in layers]
    dev = ws[0].device
    desc, at, offs = [], 0, []
    for w in ws:
        cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        desc += [cin, cout, k * k]
        offs.append(at)
        at += k * k * cin * cout * 2
    with torch.cuda.device(dev):
        if pack is None:
            pack = torch.empty(max(at, 16), dtype=torch.uint8, device=dev)
        cols = [dense.ptr_array([l[j] for l in layers]) for j in range(3)]
        _lib.check(_lib.load().sbev_resnet_pack_weights_bwd(len(layers), _i32(desc), *cols, float(eps), _DTYPES[ws[0].dtype], _ptr(pack),
                                                            _stream(dev)), 'sbev_resnet_pack_weights_bwd')
    return pack, offs


def repack_plan(depth, pointers, w_dtype=torch.float32, num_stages=4, base_channels=64, stage_blocks=None, first_trainable_stage=2):
    """sbev_resnet_repack_plan, a pure host function.  ``pointers``: one (w, gamma, beta, mean, var) tuple of device ADDRESSES per
    convolution in launch order (0 the stem).  Returns a dict of table (the int64 words to upload), items (the work items: the grid of a
    launch with one workgroup each), pack_bytes / pack_bwd_bytes (the two images), and layers: per convolution w, gamma, beta, mean, var,
    cin, cout, taps, offset, bias_offset, bwd_offset (-1: no backward image), first_item.  ``first_trainable_stage`` = num_stages + 1:
    nothing trains, the backward image is empty.  Raises SbevError where the plan refuses."""
    if stage_blocks is not None and len(stage_blocks) != num_stages:
        raise ValueError('stage_blocks must list num_stages=%d block counts' % num_stages)
    blocks = None if stage_blocks is None else _i32(stage_blocks)
    cols = [(ctypes.c_void_p * max(len(pointers), 1))(*[p[j] for p in pointers]) for j in range(5)]
    table, out = (ctypes.c_int64 * REPACK_WORDS)(), (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().sbev_resnet_repack_plan(int(depth), blocks, int(num_stages), int(base_channels), int(first_trainable_stage), *cols,
                                                   _DTYPES[w_dtype], table, out), 'sbev_resnet_repack_plan')
    words = [int(v) for v in table[:int(out[0])]]
    names = ('w', 'gamma', 'beta', 'mean', 'var', 'cin', 'cout', 'taps', 'offset', 'bias_offset', 'bwd_offset', 'first_item')
    layers = [dict(zip(names, words[REPACK_HEAD + REPACK_LAYER_WORDS * i:REPACK_HEAD + REPACK_LAYER_WORDS * (i + 1)])) for i in range(words[0])]
    return dict(table=words, items=int(out[1]), pack_bytes=int(out[2]), pack_bwd_bytes=int(out[3]), layers=layers)


def repack(table_dev, pack, pack_bwd, eps=1e-5):
    """sbev_resnet_repack: ONE launch on the current stream that writes both images of the net ``table_dev`` (the uploaded table of
    ``repack_plan``) describes into the uint8 tensors ``pack`` and ``pack_bwd`` (None where the backward image is empty)."""
    dev = pack.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sbev_resnet_repack(_ptr(table_dev), _ptr(pack), _ptr(pack_bwd), float(eps), _stream(dev)), 'sbev_resnet_repack')
    return pack, pack_bwd


def conv_dgrad_f16(gy, pack, gx, taps, stride, gy2=None, stride2=1, mask=None, res=None, gp=None, scale=None, col_tile=0):
    """sbev_conv_dgrad_f16 on tensors, nothing allocated: ``gy`` [n, h, w, Cout] and ``gx`` [n, H, W, Cin] contiguous fp16, ``pack`` the
    image(s) of ``pack_layers_bwd``, ``gy2`` the optional second K segment (a 1 x 1 of ``stride2``), ``mask`` / ``res`` as gx, ``gp`` as gx
    in fp16 or fp32 with ``scale`` the fp32 pair (2^e, 2^-e)."""
    n, H, W, cin = (int(v) for v in gx.shape)
    dev = gx.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sbev_conv_dgrad_f16(
            _ptr(gy), _ptr(gy2), _ptr(pack), _ptr(mask), _ptr(res), _ptr(gp), _DTYPES[gp.dtype] if gp is not None else 0, _ptr(scale), _ptr(gx),
            n, H, W, cin, int(gy.shape[3]), int(taps), int(stride), 0 if gy2 is None else int(gy2.shape[3]), int(stride2), int(col_tile),
            _stream(dev)), 'sbev_conv_dgrad_f16')
    return gx


def conv_wgrad_f16(gy, x, part, taps, stride, slab_len=0):
    """sbev_conv_wgrad_f16 on tensors: the unscaled slab partials of one convolution's weight gradient and column sums into ``part``
    [slabs, taps * Cout * Cin + Cout] fp32; ``gy`` [n, h, w, Cout], ``x`` [n, H, W, Cin] contiguous fp16."""
    n, H, W, cin = (int(v) for v in x.shape)
    dev = x.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sbev_conv_wgrad_f16(_ptr(gy), _ptr(x), _ptr(part), n, H, W, cin, int(gy.shape[3]), int(taps), int(stride),
                                                   int(slab_len), _stream(dev)), 'sbev_conv_wgrad_f16')
    return part


def bn_fold_backward(part, w, gamma, mean, var, eps, grad_w, grad_gamma, grad_beta, scale=None):
    """sbev_bn_fold_backward on tensors: ``part`` [slabs, taps * Cout * Cin + Cout] fp32 -> grad_w (as w, fp32), grad_gamma, grad_beta
    (None: skipped); ``scale`` the fp32 pair (2^e, 2^-e) or None (1)."""
    cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    dev = w.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sbev_bn_fold_backward(_ptr(part), int(part.shape[0]), _ptr(scale), _ptr(w), _DTYPES[w.dtype], _ptr(gamma),
                                                     _ptr(mean), _ptr(var), float(eps), cin, cout, k * k, _ptr(grad_w), _ptr(grad_gamma),
                                                     _ptr(grad_beta), _stream(dev)), 'sbev_bn_fold_backward')


def backward_raw(net, n, H, W, first_trainable_stage, acts, outs, grad_outs, pack_bwd, workspace, grad_w, grad_gamma, grad_beta):
    """sbev_resnet_backward on tensors, nothing allocated and nothing checked beyond what the C entry checks: ``net`` a ResNetBackbone
    (its shape and its parameters), ``acts`` / ``outs`` as the trainable forward left them, ``grad_outs`` channels-last tensors of one
    dtype, the three gradient lists one entry per convolution in launch order (None: not wanted / frozen)."""
    pairs = net.conv_bn_pairs()
    dev = workspace.device
    to_nhwc = lambda t: t.permute(0, 2, 3, 1)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sbev_resnet_backward(
            net.depth, _i32(net.stage_blocks), net.num_stages, net.base_channels, int(n), int(H), int(W), len(net.out_indices),
            _i32(net.out_indices), int(first_trainable_stage), _ptr(acts), dense.ptr_array([to_nhwc(o) for o in outs]),
            dense.ptr_array([to_nhwc(g) for g in grad_outs]), _DTYPES[grad_outs[0].dtype], _ptr(pack_bwd), _ptr(workspace),
            dense.ptr_array([c.weight for c, _ in pairs]), _DTYPES[pairs[0][0].weight.dtype], dense.ptr_array([b.weight for _, b in pairs]),
            dense.ptr_array([b.running_mean for _, b in pairs]), dense.ptr_array([b.running_var for _, b in pairs]), float(net.eps), dense.ptr_array(grad_w),
            dense.ptr_array(grad_gamma), dense.ptr_array(grad_beta), _stream(dev)), 'sbev_resnet_backward')


class BackboneFunction(torch.autograd.Function):
    """A trainable backbone's forward under grad.  The node owns the buffer of the activations its backward reads (every launch's output
    from the last frozen stage's onward), so several forwards may precede their backwards; the parameters are kept by reference
    (``save_for_backward``: an in-place write between forward and backward is an error).  backward: the output gradients arrive
    materialised (zeros for an unused map), all fp16 or all fp32; one that is not channels-last in memory is converted by ONE torch copy;
    the parameter gradients are fresh fp32 tensors from ``autograd``'s parameter-gradient sink; the image gets None."""

    @staticmethod
    def forward(ctx, net, x, *params):
        dev = x.device
        n, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        fts = net.frozen_stages + 1
        with torch.cuda.device(dev):
            wpack = net.pack()
            net.pack_bwd()
            bp = net.backward_plan(n, H, W)
            acts = torch.empty(max(bp['acts_bytes'], 256), dtype=torch.uint8, device=dev)
            p, ws = net._workspace(dev, n, H, W, False)
            out = [torch.empty((n, h, w, c), dtype=torch.float16, device=dev).permute(0, 3, 1, 2) for c, h, w in p['outs']]
            _lib.check(_lib.load().sbev_resnet_forward_train(
                net.depth, _i32(net.stage_blocks), net.num_stages, net.base_channels, n, H, W, len(net.out_indices), _i32(net.out_indices), fts,
                _ptr(x), _DTYPES[x.dtype], _ptr(wpack), _ptr(ws), _ptr(acts), dense.ptr_array(out), _stream(dev)), 'sbev_resnet_forward_train')
        ctx.net, ctx.acts, ctx.shape, ctx.fts = net, acts, (n, H, W), fts
        ctx.save_for_backward(*out, *params)
        return tuple(out)

    @staticmethod
    def backward(ctx, *grad_outs):
        from . import autograd as A
        net, (n, H, W) = ctx.net, ctx.shape
        saved = ctx.saved_tensors
        k = len(net.out_indices)
        outs, params = saved[:k], saved[k:]
        gs = [g if g.permute(0, 2, 3, 1).is_contiguous() else g.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for g in grad_outs]
        if any(g.dtype != gs[0].dtype for g in gs) or gs[0].dtype not in _DTYPES:
            raise TypeError('ResNetBackbone backward: the output gradients must be all fp16 or all fp32')
        dev = outs[0].device
        need = ctx.needs_input_grad[2:]
        index = net._trainable_conv_index(ctx.fts)           # convolution number (launch order) of every (w, gamma, beta) triple in params
        nconv = len(net.conv_bn_pairs())
        gw, gg, gb = [None] * nconv, [None] * nconv, [None] * nconv
        with torch.cuda.device(dev):
            sink = lambda p: A._NO_TAP.sink(False, id(p), p, tuple(p.shape))[0]
            grads = [sink(p) if want else None for p, want in zip(params, need)]
            for t, j in enumerate(index):
                gw[j], gg[j], gb[j] = grads[3 * t], grads[3 * t + 1], grads[3 * t + 2]
                if gw[j] is None:      # the C entry always stores a weight gradient
                    gw[j] = torch.empty(params[3 * t].shape, dtype=torch.float32, device=dev)
            if n == 0:
                for g in grads:
                    if g is not None:
                        g.zero_()
            ws = net._backward_workspace(dev, n, H, W)
            backward_raw(net, n, H, W, ctx.fts, ctx.acts, outs, gs, net.pack_bwd(), ws, gw, gg, gb)
        return (None, None, *[A._NO_TAP.commit(False, id(p), g) if want else None for p, g, want in zip(params, grads, need)])


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
    ``deep_stem``, ``avg_down``, dilations, ``norm_eval=False``, other strides, an ``out_dtype`` other than fp16.

    ``trainable=False`` (the default) behaves exactly so.  ``trainable=True``: ``frozen_stages=f`` (0 .. num_stages) takes effect -- the
    stem and stages 1 .. f stay frozen, the convolution weights of the later stages get ``requires_grad=True`` and, unless
    ``norm_cfg['requires_grad']`` is False, so do their BatchNorm gamma / beta; ``norm_eval=True`` stays mandatory (running statistics
    always).  A forward under grad then goes through ``BackboneFunction``; under ``torch.no_grad()`` nothing differs, bit for bit.
    ``with_cp`` stays accepted without effect: nothing is recomputed, the activations are kept.  Refused by name: ``frozen_stages=-1``
    with ``trainable=True`` (a trainable stem: the 7 x 7 weight gradient and the max-pool backward are not built), an image that requires
    a gradient, a trainable forward under a graph capture outside a ``dense.step_images()`` scope.  Inside such a scope (a captured
    training step: ``train_graph.CapturedDetectorTrainStep``) ``pack()`` / ``pack_bwd()`` derive both images once per scope by ONE launch
    of the step itself (``sbev_resnet_repack``, through a device table of the parameters' addresses that a warm-up step uploads) and leave
    the ``_version``-keyed caches alone, so a replay folds the weights as they are then."""

    def __init__(self, depth=50, num_stages=4, out_indices=(0, 1, 2, 3), style='pytorch', base_channels=64, norm_cfg=None,
                 out_dtype=torch.float16, stage_blocks=None, in_channels=3, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1), frozen_stages=-1,
                 norm_eval=True, with_cp=False, zero_init_residual=True, dcn=None, stage_with_dcn=(False, False, False, False),
                 deep_stem=False, avg_down=False, conv_cfg=None, plugins=None, init_cfg=None, pretrained=None, trainable=False):
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
        self.trainable = bool(trainable)
        self.frozen_stages = int(frozen_stages)
        if self.trainable and self.frozen_stages < 0:
            raise ValueError('ResNetBackbone: frozen_stages=%r with trainable=True is not built (a trainable stem needs the 7 x 7 weight '
                             'gradient and the max-pool backward): freeze at least the stem, frozen_stages >= 0' % (frozen_stages,))
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
        if self.trainable:
            norms_learn = norm_cfg.get('requires_grad', True) is not False
            for s in range(self.frozen_stages, num_stages):
                for block in getattr(self, 'layer%d' % (s + 1)):
                    for conv, bn in block.pairs():
                        conv.weight.requires_grad_(True)
                        bn.weight.requires_grad_(norms_learn)
                        bn.bias.requires_grad_(norms_learn)
        self.eval()
        # the folded weight image and the backward's (transposed / flipped w'), each at a fixed address per device, keyed on the versions
        # of every parameter and buffer (the backward's also on frozen_stages); inside step_images() both come from _step_images()
        self._image = dense.WeightImage('resnet_pack', 'ResNetBackbone.forward under a capture with weights that are not packed: run one '
                                        'forward (or pack()) before the capture')
        self._image_bwd = dense.WeightImage('resnet_pack_bwd', 'ResNetBackbone backward under a capture with weights that are not packed')
        self._workspaces = {}           # (device index, n, H, W, keep) -> (plan, uint8 workspace at a fixed address)
        self._bwd_workspaces = {}       # (device index, n, H, W) -> uint8 workspace of the backward
        self._repack_tables = {}        # repack_key() -> (device table of sbev_resnet_repack, its plan), the latest key only: step_images() scopes

    # ---- weights
    def conv_bn_pairs(self):
        """(conv, bn) of every convolution in launch order: the stem, then per block conv1, conv2, [downsample], conv3"""
        pairs = [(self.conv1, self.bn1)]
        for s in range(self.num_stages):
            for block in getattr(self, 'layer%d' % (s + 1)):
                pairs += block.pairs()
        return pairs

    def _checked_layers(self):
        """(weight, gamma, beta, mean, var) of every convolution in launch order: the weights all fp32 or all fp16, the rest fp32, on
        one device"""
        layers = [(c.weight, b.weight, b.bias, b.running_mean, b.running_var) for c, b in self.conv_bn_pairs()]
        ws = [l[0] for l in layers]
        stats = [t for l in layers for t in l[1:]]
        dev = ws[0].device
        if dev.type != 'cuda':
            raise RuntimeError('ResNetBackbone needs its parameters on the device (no CPU fallback)')
        if any(w.device != dev or w.dtype != ws[0].dtype for w in ws) or ws[0].dtype not in _DTYPES:
            raise TypeError('ResNetBackbone: the convolution weights must be all fp32 or all fp16, on one device')
        if any(t.device != dev or t.dtype != torch.float32 for t in stats):
            raise TypeError('ResNetBackbone: the BatchNorm weights and statistics must be fp32, on the weights\' device')
        return layers

    def pack(self):
        """Fold and pack now if any parameter or buffer changed since the last pack (forward does this itself).  Returns the image.
        Inside step_images(): the scope's, both images by the step's own single launch."""
        layers = self._checked_layers()

        def make(dest):
            if any(not t.is_contiguous() for l in layers for t in l):
                raise ValueError('ResNetBackbone: parameters and buffers must be contiguous')
            return pack_layers(layers, self.eps, dest)[0]

        return self._image.get([t for l in layers for t in l], make, in_step=lambda: self._step_images(layers)[0])

    def _trainable_conv_index(self, first_trainable_stage):
        """convolution numbers (launch order, 0 the stem) of the stages from first_trainable_stage on"""
        at, index = 1, []
        for s in range(self.num_stages):
            for block in getattr(self, 'layer%d' % (s + 1)):
                k = len(block.pairs())
                if s >= first_trainable_stage - 1:
                    index += list(range(at, at + k))
                at += k
        return index

    def pack_bwd(self):
        """The backward's weight image (sbev_resnet_pack_weights_bwd), packed now if a parameter or a statistic changed since its last
        pack.  Returns the image."""
        layers = [(c.weight, b.weight, b.bias, b.running_mean, b.running_var) for c, b in self.conv_bn_pairs()]

        def make(dest):
            self.pack()           # its checks of devices, dtypes and contiguity hold for this image too
            bp = self.backward_plan(1, 32, 32)
            order = sorted((l['pack_offset'], i) for i, l in enumerate(bp['layers']) if l['pack_offset'] >= 0)
            todo = [(layers[i - 1][0], layers[i - 1][1], layers[i - 1][4]) for _, i in order]          # launch i is convolution i - 1
            if dest is not None and dest.numel() < bp['pack_bytes']:
                dest = None
            image, offs = pack_layers_bwd(todo, self.eps, dest)
            assert offs == [o for o, _ in order]
            return image

        def in_step():
            self.pack()           # its checks; the same scope entry
            return self._step_images(layers)[1]

        return self._image_bwd.get([t for l in layers for t in l], make, extra=(self.frozen_stages,), in_step=in_step)

    # ---- the two images inside a training step's scope (dense.step_images): one sbev_resnet_repack launch per step
    def repack_key(self):
        """what the device table of sbev_resnet_repack bakes in: device, dtype, first trainable stage, every tensor's address"""
        pairs = self.conv_bn_pairs()
        w = pairs[0][0].weight
        fts = self.frozen_stages + 1 if self.trainable else self.num_stages + 1
        return (w.device.index, w.dtype, min(fts, self.num_stages + 1)) + tuple(
            t.data_ptr() for c, b in pairs for t in (c.weight, b.weight, b.bias, b.running_mean, b.running_var))

    def repack_table(self, key):
        """the (device table, plan) built for ``key``, or None: a captured step keeps it alive beside its graph"""
        return self._repack_tables.get(key)

    def check_repack_table(self, key):
        """A captured step's replay-time check: the graph's repack launch reads the table built for ``key`` (``repack_key()`` at
        capture); a parameter or buffer that has moved since (``.to()``, ``p.data = ...``, ``load_state_dict(assign=True)``) would be
        folded from its OLD address."""
        now = self.repack_key()
        if now != key:
            moved = sum(a != b for a, b in zip(now[3:], key[3:]))
            raise RuntimeError('ResNetBackbone: %d parameter / buffer tensor(s) have another address, dtype or device than the captured '
                               "step's weight-repack table holds: capture a new step" % max(moved, 1))

    def _repack_table(self, layers):
        key = self.repack_key()
        hit = self._repack_tables.get(key)
        if hit is not None:
            return hit
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ResNetBackbone under a capture inside step_images(): no weight-repack table for the current parameter '
                               'addresses (the table is uploaded outside a capture): run a warm-up step first')
        if any(not t.is_contiguous() for l in layers for t in l):
            raise ValueError('ResNetBackbone: parameters and buffers must be contiguous')
        dev = layers[0][0].device
        p = repack_plan(self.depth, [tuple(t.data_ptr() for t in l) for l in layers], layers[0][0].dtype, self.num_stages, self.base_channels,
                        self.stage_blocks, key[2])
        table = torch.tensor(p['table'], dtype=torch.int64).to(dev)
        self._repack_tables = {key: (table, p)}         # the latest only: a captured step holds the table its graph reads (repack_table)
        return self._repack_tables[key]

    def _step_images(self, layers):
        """(forward image, backward image) of the current step_images() scope: derived at the first call by ONE launch on the current
        stream into fresh tensors (under a capture: from the capture's pool), returned by the later ones"""
        def make():
            table, p = self._repack_table(layers)
            dev = table.device
            with torch.cuda.device(dev):
                fwd = torch.empty(max(p['pack_bytes'], 16), dtype=torch.uint8, device=dev)
                bwd = torch.empty(p['pack_bwd_bytes'], dtype=torch.uint8, device=dev) if p['pack_bwd_bytes'] else None
            return repack(table, fwd, bwd, self.eps)

        return dense.step_image('resnet_repack', tuple(t for l in layers for t in l), make)

    def backward_plan(self, n, H, W):
        return backward_plan(self.depth, n, H, W, self.out_indices, self.num_stages, self.base_channels, self.stage_blocks,
                             self.frozen_stages + 1)

    def _workspace(self, dev, n, H, W, keep):
        key = (dev.index, n, H, W, keep)
        if key not in self._workspaces:
            p = self.plan(n, H, W, keep)
            self._workspaces[key] = (p, torch.empty(max(p['workspace_bytes'], 256), dtype=torch.uint8, device=dev))
        return self._workspaces[key]

    def _backward_workspace(self, dev, n, H, W):
        key = (dev.index, n, H, W)
        ws = self._bwd_workspaces.get(key)
        if ws is None:
            ws = self._bwd_workspaces[key] = torch.empty(max(self.backward_plan(n, H, W)['workspace_bytes'], 256), dtype=torch.uint8, device=dev)
        return ws

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
        wants_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if wants_grad and not self.trainable:
            raise RuntimeError('ResNetBackbone is inference only (its backward is not built): call it under torch.no_grad() and keep the '
                               'parameters frozen')
        if wants_grad:
            return self._forward_train(x, out, keep)
        dev = x.device
        n, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        if H < 1 or W < 1:
            raise ValueError('ResNetBackbone: an empty image (%d x %d)' % (H, W))
        if self.conv1.weight.device != dev:
            raise ValueError('ResNetBackbone: x is on %s, the parameters on %s' % (dev, self.conv1.weight.device))
        with torch.cuda.device(dev):
            wpack = self.pack()
            p, ws = self._workspace(dev, n, H, W, keep is not None)
            shapes = [(n, c, h, w) for c, h, w in p['outs']]
            if out is None:
                out = [torch.empty((n, h, w, c), dtype=torch.float16, device=dev).permute(0, 3, 1, 2) for _, c, h, w in shapes]
            else:
                out = dense.channels_last_out('ResNetBackbone', out, shapes, dev, torch.float16)[0]
            blocks = _i32(self.stage_blocks)
            _lib.check(_lib.load().sbev_resnet_forward(
                self.depth, blocks, self.num_stages, self.base_channels, n, H, W, len(self.out_indices), _i32(self.out_indices),
                int(keep is not None), ctypes.c_void_p(x.data_ptr()), _DTYPES[x.dtype], ctypes.c_void_p(wpack.data_ptr()),
                ctypes.c_void_p(ws.data_ptr()), dense.ptr_array(out), _stream(dev)), 'sbev_resnet_forward')
        if keep is not None:
            for l in p['layers']:
                if l['where'] < 0:
                    keep.append(out[-1 - l['where']])
                else:
                    nbytes = n * l['h'] * l['w'] * l['cout'] * 2
                    keep.append(ws[l['where']:l['where'] + nbytes].view(torch.float16).view(n, l['h'], l['w'], l['cout']).permute(0, 3, 1, 2))
        return out

    def _forward_train(self, x, out, keep):
        """a forward that needs a gradient, on checked x: through BackboneFunction"""
        if x.requires_grad:
            raise ValueError('ResNetBackbone: the image requires a gradient; no image gradient is ever produced (the stem is frozen): detach it')
        if out is not None or keep is not None:
            raise ValueError('ResNetBackbone: out= / keep= are not taken by a forward that needs a gradient (autograd owns its outputs)')
        if torch.cuda.is_current_stream_capturing() and not dense.in_step_images():
            raise RuntimeError('ResNetBackbone: a trainable forward under a graph capture (the backbone inside CapturedHeadTrainStep) is not '
                               'built: the weight packs would have to move into the graph')
        if x.device != self.conv1.weight.device:
            raise ValueError('ResNetBackbone: x is on %s, the parameters on %s' % (x.device, self.conv1.weight.device))
        if x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError('ResNetBackbone: an empty image (%d x %d)' % (x.shape[2], x.shape[3]))
        fts = self.frozen_stages + 1
        if fts > self.num_stages:
            raise RuntimeError('ResNetBackbone: frozen_stages=%d freezes every stage but a parameter requires a gradient' % self.frozen_stages)
        pairs = self.conv_bn_pairs()
        index = self._trainable_conv_index(fts)
        allowed = {id(t) for j in index for t in (pairs[j][0].weight, pairs[j][1].weight, pairs[j][1].bias)}
        for name, p in self.named_parameters():
            if p.requires_grad and id(p) not in allowed:
                raise RuntimeError('ResNetBackbone: %s requires a gradient but lies in the frozen part (frozen_stages=%d)' % (name, self.frozen_stages))
        params = [t for j in index for t in (pairs[j][0].weight, pairs[j][1].weight, pairs[j][1].bias)]
        return list(BackboneFunction.apply(self, x, *params))
