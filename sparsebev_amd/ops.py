"""Python operator layer over the C ABI -- mirrors the reference's operator interface
(models/csrc/wrapper.py:87-93 ``msmv_sampling``; models/sparsebev_sampling.py ``make_sample_points`` /
``sampling_4d``) with the same names, argument meaning and error behaviour, but every byte of work is
done by hand-written gfx950 kernels in libsbev_hip.so.  Tensors must live on a HIP device; there is no
CPU path (calling these with CPU tensors raises).
"""
import ctypes
import os

import torch

from . import _lib
from .utils import FrameSource

N_VIEWS = 6           # models/sparsebev_sampling.py:45
OUT_REF, OUT_MIX = 0, 1
_F32, _BF16, _F16 = 0, 1, 2


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _need_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('sparsebev_amd ops need device tensors (no CPU fallback); got a %s tensor' % t.device)


def _check_sampling_args(feats, sampling_locations, scale_weights, Bp, what):
    """The argument checks of msmv_sampling.cpp:106-125 shared by every sampler entry point: the kernel reinterprets
    loc / weights as fp32 rows of 3 / L floats, so anything else must be refused here."""
    if not 1 <= len(feats) <= 5:
        raise RuntimeError('%s supports 1..5 feature levels, got %d' % (what, len(feats)))
    if sampling_locations.dtype != torch.float32 or scale_weights.dtype != torch.float32:
        raise RuntimeError('sampling_loc / attn_weight must be float32')
    if sampling_locations.dim() != 4 or sampling_locations.shape[-1] != 3 or sampling_locations.shape[0] != Bp:
        raise RuntimeError('sampling_loc must be [B, Q, P, 3]')
    _, Q, P, _ = sampling_locations.shape
    if tuple(scale_weights.shape) != (Bp, Q, P, len(feats)):
        raise RuntimeError('attn_weight must be [B, Q, P, %d]' % len(feats))
    if P > 32:
        raise RuntimeError('num_point exceed limits')
    return Q, P


def _no_grad_only(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError('sparsebev_amd: this entry point is forward-only; the differentiable forms are '
                                  'ops.msmv_sampling (reference layout) and the decoder module in train() mode')


def _level_ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _pyramid(feats, N, G=None):
    """The C ABI's description of a feature pyramid (include/sbev_hip.h: sbev_msmv_fwd) for channels-last levels [..., H_l, W_l, row]:
    ``(c_feats, c_hw, L), (gdiv, c_stride_bo, stride_g, c_stride_v, stride_px)`` -- the two runs of positional arguments every sampler
    entry point takes, strides in elements.  G None: the reference's [B', N, H, W, C] (one group per sample batch); else the grouped
    [B*T*N or B*n_slots*N, H, W, G*C], group g = channel slice [g*C, (g+1)*C)."""
    L = len(feats)
    row = feats[0].shape[-1]
    pixels = [f.shape[-3] * f.shape[-2] for f in feats]
    c_hw = (ctypes.c_int32 * (2 * L))(*[v for f in feats for v in f.shape[-3:-1]])
    c_sbo = (ctypes.c_int64 * L)(*[N * n * row for n in pixels])
    c_sv = (ctypes.c_int64 * L)(*[n * row for n in pixels])
    gdiv, stride_g = (1, 0) if G is None else (G, row // G)
    return (_level_ptrs(feats), c_hw, L), (gdiv, c_sbo, stride_g, c_sv, row)


def _msmv_launch(feats, Bp, N, C, G, loc, weights, out, out_layout, T, Gout):
    levels, strides = _pyramid(feats, N, G)
    Q, P = loc.shape[1:3]
    st = _lib.load().sbev_msmv_fwd(*levels, _feat_dtype(feats), Bp, N, C, Q, P, *strides,
                                   _ptr(loc), _ptr(weights), _ptr(out), out_layout, T, Gout, _stream())
    _lib.check(st, 'sbev_msmv_fwd')


def _feat_dtype(feats):
    dt = feats[0].dtype
    if any(f.dtype != dt for f in feats):
        raise RuntimeError('all feature levels must share one dtype')
    if dt == torch.float32:
        return _F32
    if dt == torch.bfloat16:
        return _BF16
    if dt == torch.float16:
        return _F16
    raise RuntimeError('feature dtype must be float32, bfloat16 or float16, got %s' % dt)


def _msmv_forward(feats, sampling_locations, scale_weights, out_layout, T, G):
    Bp, N, _, _, C = feats[0].shape
    _, Q, P, _ = sampling_locations.shape
    if out_layout == OUT_REF:
        out = torch.empty(Bp, Q, C, P, device=feats[0].device, dtype=torch.float32)
    else:
        out = torch.empty(Bp // (T * G), Q, G, T * P, C, device=feats[0].device, dtype=torch.float32)
    _msmv_launch(feats, Bp, N, C, None, sampling_locations, scale_weights, out, out_layout, T, G)
    return out


_DET_FEAT_GRAD = os.environ.get('SBEV_DET_FEAT_GRAD', '0') == '1'


def deterministic_feature_grad(enable=None):
    """Process-wide switch of the sampler's feature gradient: off (default) = float atomics (sbev_msmv_bwd[_ex]), on = the atomics-free,
    bit-reproducible sum over a sorted tap list (sbev_msmv_bwd_taps / torch.sort / sbev_msmv_bwd_sum_sorted).  ``SBEV_DET_FEAT_GRAD=1``
    in the environment starts with it on.  ``enable`` None: query only.  Returns the previous setting.  The mode a backward runs in is
    ``deterministic_feature_grad_active()``, read when the backward runs."""
    global _DET_FEAT_GRAD
    prev = _DET_FEAT_GRAD
    if enable is not None:
        _DET_FEAT_GRAD = bool(enable)
    return prev


def deterministic_feature_grad_active():
    """The switch, or torch.use_deterministic_algorithms(True)."""
    return _DET_FEAT_GRAD or torch.are_deterministic_algorithms_enabled()


def _msmv_backward(feats, N, G, Bp, C, loc, weights, grad_out, grad_feats, grad_layout, T, Gout, deterministic):
    """Every sampler backward of this package: (grad_loc, grad_weights) of ``feats`` as _pyramid(feats, N, G) describes them, the feature
    gradient ACCUMULATED into ``grad_feats`` (None: frozen features, no feature gradient).  ``deterministic`` None: the switch."""
    lib = _lib.load()
    Q, P = loc.shape[1:3]
    loc, weights, grad_out = loc.contiguous(), weights.contiguous(), grad_out.contiguous()
    gloc = torch.empty_like(loc)
    gw = torch.empty_like(weights)
    (c_feats, c_hw, L), strides = _pyramid(feats, N, G)
    if deterministic is None:
        deterministic = deterministic_feature_grad_active()
    det = bool(deterministic) and grad_feats is not None
    c_gfeats = _level_ptrs(grad_feats) if grad_feats is not None else None
    st = lib.sbev_msmv_bwd_ex(c_feats, None if det else c_gfeats, c_hw, L, Bp, N, C, Q, P, *strides, _ptr(loc), _ptr(weights), _ptr(grad_out),
                              grad_layout, T, Gout, _ptr(gloc), _ptr(gw), _stream())
    _lib.check(st, 'sbev_msmv_bwd_ex')
    if det:
        n = lib.sbev_msmv_bwd_tap_count(Bp, Q, P, L)
        if n < 0:
            raise RuntimeError("deterministic feature gradient: B'*Q*P*L*4 is too large")
        if n > 0:
            keys = torch.empty(n, device=loc.device, dtype=torch.int64)
            coefs = torch.empty(n, device=loc.device, dtype=torch.float32)
            st = lib.sbev_msmv_bwd_taps(c_feats, c_hw, L, Bp, N, C, Q, P, *strides, _ptr(loc), _ptr(weights), _ptr(keys), _ptr(coefs), _stream())
            _lib.check(st, 'sbev_msmv_bwd_taps')
            # THE index: a stable ascending sort -- integer work (no execution order in its result), ties keep ascending tap index
            sorted_keys, order = torch.sort(keys, stable=True)
            st = lib.sbev_msmv_bwd_sum_sorted(c_gfeats, L, _ptr(sorted_keys), _ptr(order), _ptr(coefs), n, _ptr(grad_out), grad_layout,
                                              Bp, C, Q, P, T, Gout, _stream())
            _lib.check(st, 'sbev_msmv_bwd_sum_sorted')
    return gloc, gw


class MSMVSampling(torch.autograd.Function):
    """Autograd wrapper, the counterpart of MSMVSamplingC2345 / C23456 (models/csrc/wrapper.py:41-84): forward and
    backward are both HIP kernels (sbev_msmv_fwd / sbev_msmv_bwd_ex, see _msmv_backward); fp32 features, reference layout."""

    @staticmethod
    def forward(ctx, sampling_locations, scale_weights, *feats):
        ctx.save_for_backward(sampling_locations, scale_weights, *feats)
        return _msmv_forward(list(feats), sampling_locations, scale_weights, OUT_REF, 1, 1)

    @staticmethod
    def backward(ctx, grad_output):
        loc, weights, *feats = ctx.saved_tensors
        if feats[0].dtype != torch.float32:
            raise NotImplementedError('msmv_sampling backward needs fp32 features')
        grad_output = grad_output.contiguous().float()
        Bp, N, _, _, C = feats[0].shape
        _, Q, P, _ = loc.shape
        gfeats = [torch.zeros_like(f) for f in feats]              # the op accumulates (atomics, or one addition per row)
        gloc, gw = _msmv_backward(feats, N, None, Bp, C, loc, weights, grad_output, gfeats, OUT_REF, 1, 1, None)
        return (gloc, gw, *gfeats)


def msmv_sampling(mlvl_feats, sampling_locations, scale_weights, out_layout=OUT_REF, T=1, G=1):
    """Drop-in for the reference operator ``msmv_sampling`` (models/csrc/wrapper.py:87-93).

    mlvl_feats: list (1..5 levels) of contiguous channel-last ``[B', N, H_l, W_l, C]`` device tensors
    (fp32, or bf16 storage with fp32 accumulation); sampling_locations ``[B', Q, P, 3]``;
    scale_weights ``[B', Q, P, L]``.  Returns ``[B', Q, C, P]`` fp32 (or, with ``out_layout=OUT_MIX``,
    ``[B'/(T*G), Q, G, T*P, C]``).  Same preconditions as msmv_sampling.cpp:106-125 (contiguity, device,
    P <= 32); violations raise RuntimeError.  Differentiable (reference layout, fp32 features) like the
    reference's autograd Functions."""
    feats = list(mlvl_feats)
    _need_device(sampling_locations, scale_weights, *feats)
    for f in feats:
        if not f.is_contiguous():
            raise RuntimeError('value tensor has to be contiguous')
        if f.dim() != 5:
            raise RuntimeError('value tensor must be [B, N, H, W, C]')
    if not sampling_locations.is_contiguous():
        raise RuntimeError('sampling_loc tensor has to be contiguous')
    if not scale_weights.is_contiguous():
        raise RuntimeError('attn_weight tensor has to be contiguous')
    Bp = feats[0].shape[0] if feats else 0
    _check_sampling_args(feats, sampling_locations, scale_weights, Bp, 'msmv_sampling')
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (sampling_locations, scale_weights, *feats))
    if needs_grad:
        if out_layout != OUT_REF:
            raise NotImplementedError('autograd is wired for the reference output layout only')
        return MSMVSampling.apply(sampling_locations, scale_weights, *feats)
    return _msmv_forward(feats, sampling_locations, scale_weights, out_layout, T, G)


def _msmv_resident(word, levels, B, T, G, sampling_locations, scale_weights, out_layout, frame_slots=None, slot_table=None, n_slots=0):
    """msmv_sampling_nhwc / _ring / _pool: the grouped sampler over resident channels-last levels, ``word`` the entry point's own in
    the messages.  Frame t of sample b is image run b*T + t of a level, or slot frame_slots[t] / slot_table[b, t] of b's n_slots."""
    what = 'msmv_sampling_' + word
    feats = list(levels)
    _need_device(sampling_locations, scale_weights, *feats)
    _no_grad_only(sampling_locations, scale_weights, *feats)
    N = N_VIEWS
    Bp = B * T * G
    Q, P = _check_sampling_args(feats, sampling_locations, scale_weights, Bp, what)
    GC = feats[0].shape[-1]
    if GC % G != 0 or (GC // G) % 4 != 0:
        raise RuntimeError('%s feature channels %d must split into G=%d groups of a multiple of 4 channels' % (word, GC, G))
    C = GC // G
    src = FrameSource.of(frame_slots, slot_table, n_slots, (B, T), what, plain=None if word == 'pool' else 'dense')
    frames, dims = (B * src.n_slots, 'B*n_slots*6') if src.resident else (B * T, 'B*T*6')
    for f in feats:
        if not f.is_contiguous() or f.dim() != 4 or f.shape[0] != frames * N or f.shape[-1] != GC:
            raise RuntimeError('%s feature level must be contiguous [%s, H, W, G*C]' % (word, dims))
    if src.kind == 'ring' and len(src.frame_slots) != T:
        raise RuntimeError('frame_slots must name one slot per frame (T=%d)' % T)
    if out_layout == OUT_REF:
        out = torch.empty(Bp, Q, C, P, device=feats[0].device, dtype=torch.float32)
    else:
        out = torch.empty(B, Q, G, T * P, C, device=feats[0].device, dtype=torch.float32)
    pyramid, strides = _pyramid(feats, N, G)         # (stride_bo: one image run of a frame, or one slot)
    lib = _lib.load()
    fn, name, tail = {'dense': (lib.sbev_msmv_fwd, 'sbev_msmv_fwd', ()),
                      'ring': (lib.sbev_msmv_fwd_ring, 'sbev_msmv_fwd_ring', ((ctypes.c_int32 * len(src.frame_slots))(*src.frame_slots), n_slots)),
                      'pool': (lib.sbev_msmv_fwd_pool, 'sbev_msmv_fwd_pool', (_ptr(slot_table), n_slots))}[src.kind]
    st = fn(*pyramid, _feat_dtype(feats), Bp, N, C, Q, P, *strides, _ptr(sampling_locations.contiguous()), _ptr(scale_weights.contiguous()),
            _ptr(out), out_layout, T, G, *tail, _stream())
    _lib.check(st, name)
    return out


def msmv_sampling_nhwc(feats_nhwc, B, T, G, sampling_locations, scale_weights, out_layout=OUT_MIX):
    """Zero-copy variant: feats_nhwc is a list of ``[B*T*N, H_l, W_l, G*C]``
    channels-last pyramids straight from an NHWC neck; group g of sample batch b' = (b*T+t)*G+g is the
    channel slice [g*C, (g+1)*C) -- the reference's regroup copy (models/sparsebev_transformer.py:73-85,
    2x the feature bytes per call) never happens."""
    return _msmv_resident('nhwc', feats_nhwc, B, T, G, sampling_locations, scale_weights, out_layout)


def msmv_sampling_nhwc_backward(feats_nhwc, B, T, G, sampling_locations, scale_weights, grad_out, grad_feats=None,
                                grad_layout=OUT_MIX, deterministic=None):
    """Backward of msmv_sampling_nhwc (sbev_msmv_bwd_ex): grad_out in the forward's output layout ->
    (grad_loc [B',Q,P,3], grad_weights [B',Q,P,L]); grad wrt the features is ACCUMULATED into ``grad_feats`` (list of fp32 buffers
    shaped like feats_nhwc) or skipped entirely when it is None (frozen features).  How it is accumulated: ``deterministic`` False =
    float atomics (the sum's order changes from run to run); True = the bit-reproducible sorted-tap sum (four launches: the kernel
    above without feature buffers, sbev_msmv_bwd_taps, torch.sort, sbev_msmv_bwd_sum_sorted); None = deterministic_feature_grad_active()."""
    feats = list(feats_nhwc)
    _need_device(sampling_locations, scale_weights, grad_out, *feats)
    if _feat_dtype(feats) != _F32:
        raise NotImplementedError('the sampling backward needs fp32 feature maps (bf16 storage is an inference format)')
    N = N_VIEWS
    Bp = B * T * G
    _check_sampling_args(feats, sampling_locations, scale_weights, Bp, 'msmv_sampling_nhwc_backward')
    GC = feats[0].shape[-1]
    C = GC // G
    return _msmv_backward(feats, N, G, Bp, C, sampling_locations, scale_weights, grad_out, grad_feats, grad_layout, T, G, deterministic)


def msmv_sampling_ring(levels, B, T, G, frame_slots, n_slots, sampling_locations, scale_weights, out_layout=OUT_MIX):
    """Sampler over the online frame ring (cache.FrameFeatureCache): levels[l] = [B*n_slots*6, H, W, G*C]; logical frame
    t of a sample is read from physical slot frame_slots[t] (sbev_msmv_fwd_ring)."""
    return _msmv_resident('ring', levels, B, T, G, sampling_locations, scale_weights, out_layout, frame_slots=list(frame_slots), n_slots=n_slots)


def msmv_sampling_pool(levels, B, T, G, slot_table, n_slots, sampling_locations, scale_weights, out_layout=OUT_MIX):
    """Sampler over the keyed frame pool (cache.FramePool): levels[l] = [B*n_slots*6, H, W, G*C]; logical frame t of sample b is
    read from physical slot slot_table[b, t] -- a DEVICE int32 [B, T] the kernel reads (sbev_msmv_fwd_pool; entries are clamped to
    [0, n_slots) there, the caller keeps them in range).  n_slots may be below T: two frames of a window may share a slot."""
    return _msmv_resident('pool', levels, B, T, G, sampling_locations, scale_weights, out_layout, slot_table=slot_table, n_slots=n_slots)


def sample_mix_supported(L, C, P, T, G):
    return bool(_lib.load().sbev_sample_mix_supported(L, C, P, T, G, G))


def query_order(query_bbox, pc_range):
    """Launch order of the fused gather + mixing items (sbev_query_order): int32 [B*Q], sample b's rows b*Q + q sorted by the
    direction of the box centre around the ego origin.  query_bbox [B, Q, >= 2] fp32 (columns 0, 1 = normalised centre)."""
    _need_device(query_bbox)
    if query_bbox.dim() != 3 or query_bbox.dtype != torch.float32 or query_bbox.shape[-1] < 2:
        raise RuntimeError('query_order: query_bbox must be fp32 [B, Q, >= 2]')
    qb = query_bbox.contiguous()
    B, Q = qb.shape[:2]
    order = torch.empty(B * Q, device=qb.device, dtype=torch.int32)
    pcr = (ctypes.c_double * 6)(*[float(v) for v in pc_range])
    _lib.check(_lib.load().sbev_query_order(_ptr(qb), qb.shape[-1], pcr, B, Q, _ptr(order), _stream()), 'sbev_query_order')
    return order


def sample_mix(levels, B, T, G, sampling_locations, scale_weights, params, out_points, frame_slots=None, n_slots=0, order=None, up_log2=None,
               slot_table=None):
    """Gather + adaptive mixing in one launch (sbev_sample_mix_f32): levels as for msmv_sampling_nhwc (or the ring's
    buffers with frame_slots / n_slots, or the frame pool's with slot_table / n_slots: a device int32 [B, T], see
    msmv_sampling_pool -- sbev_sample_mix_pool), params [B,Q,G*(C*C + out_points*T*P)] -> mixed [B,Q,G*out_points*C].
    Bit-identical to msmv_sampling_nhwc(..., OUT_MIX) followed by the mixing kernel.  order (query_order(); any permutation of
    the B*Q rows as int32): the workgroups' launch order -- a placement hint, the result does not depend on it.
    up_log2 (an int; None: fp32): the same launch writing the operand format of the fp16 out-projection (sbev_sample_mix_pairs_f16,
    with an order sbev_sample_mix_pairs_f16_ordered) -- int32 of the same geometry, each word the (fp16 hi, fp16 lo) pair of
    y 2^up_log2 with hi in the low half: dense.f16s_pairs(sample_mix(...), up_log2) bit for bit."""
    if up_log2 is not None and (isinstance(up_log2, bool) or not isinstance(up_log2, int)):
        raise RuntimeError('sample_mix: up_log2 must be an int (the power of two of the pair format) or None')
    feats = list(levels)
    _need_device(sampling_locations, scale_weights, params, *feats)
    _no_grad_only(sampling_locations, scale_weights, params, *feats)
    N = N_VIEWS
    Q, P = _check_sampling_args(feats, sampling_locations, scale_weights, B * T * G, 'sample_mix')
    GC = feats[0].shape[-1]
    C = GC // G
    L = len(feats)
    if not sample_mix_supported(L, C, P, T, G):
        raise RuntimeError('sample_mix: shape not covered by the fused kernel (L=%d C=%d P=%d T=%d)' % (L, C, P, T))
    params = params.contiguous()
    if params.dtype != torch.float32 or params.numel() != B * Q * G * (C * C + out_points * T * P):
        raise RuntimeError('sample_mix: params must be fp32 [B, Q, G*(C*C + out_points*T*P)]')
    y = torch.empty(B, Q, G * out_points * C, device=params.device, dtype=torch.float32 if up_log2 is None else torch.int32)
    if order is not None:
        _need_device(order)
        if order.dtype != torch.int32 or order.numel() != B * Q or not order.is_contiguous():
            raise RuntimeError('sample_mix: order must be a contiguous int32 permutation of the B*Q rows')
    loc, weights = sampling_locations.contiguous(), scale_weights.contiguous()
    src = FrameSource.of(frame_slots, slot_table, n_slots, (B, T), 'sample_mix')
    if src.kind == 'pool' and any(f.shape[0] != B * n_slots * N for f in feats):
        raise RuntimeError('sample_mix: pool feature levels must be [B*n_slots*6, H, W, G*C]')
    pyramid, strides = _pyramid(feats, N, G)
    c_slots = (ctypes.c_int32 * T)(*src.frame_slots) if src.kind == 'ring' else None
    head = (*pyramid, _feat_dtype(feats), B, N, Q, T, G, P, C, *strides[1:], _ptr(loc), _ptr(weights), c_slots)
    tail = (n_slots, _ptr(params), _ptr(y), out_points, 1e-5)
    lib = _lib.load()
    if src.kind == 'pool':
        name = 'sbev_sample_mix_pool'
        st = lib.sbev_sample_mix_pool(*head, _ptr(slot_table), *tail, 0 if up_log2 is None else 1, up_log2 or 0, _ptr(order), _stream())
    elif up_log2 is None:
        name, st = 'sbev_sample_mix_f32', lib.sbev_sample_mix_f32_ordered(*head, *tail, _ptr(order), _stream())
    elif order is None:
        name, st = 'sbev_sample_mix_pairs_f16', lib.sbev_sample_mix_pairs_f16(*head, *tail, up_log2, _stream())
    else:
        name, st = 'sbev_sample_mix_pairs_f16', lib.sbev_sample_mix_pairs_f16_ordered(*head, *tail, up_log2, _ptr(order), _stream())
    _lib.check(st, name)
    return y


def project_select(sample_points, lidar2img, image_h, image_w, G, P, eps=1e-5, dump=False):
    """Front half of sampling_4d (models/sparsebev_sampling.py:49-114) on device, bit-exact camera-hit
    mask.  sample_points ``[B,Q,T,G*P,3]``, lidar2img ``[B,T*6,4,4]`` -> loc ``[B*T*G,Q,P,3]`` and, with
    dump=True, the DUMP-tap tensors (uvh ``[B,T,6,Q,GP,3]``, valid uint8 ``[B,T,6,Q,GP]``, i_view int32
    ``[B,T,Q,GP]``)."""
    _need_device(sample_points, lidar2img)
    sample_points = sample_points.contiguous().float()
    lidar2img = lidar2img.contiguous().float()
    B, Q, T, GP, _ = sample_points.shape
    assert GP == G * P and lidar2img.shape[1] == T * N_VIEWS
    dev = sample_points.device
    loc = torch.empty(B * T * G, Q, P, 3, device=dev, dtype=torch.float32)
    uvh = valid = iview = None
    if dump:
        uvh = torch.empty(B, T, N_VIEWS, Q, GP, 3, device=dev, dtype=torch.float32)
        valid = torch.empty(B, T, N_VIEWS, Q, GP, device=dev, dtype=torch.uint8)
        iview = torch.empty(B, T, Q, GP, device=dev, dtype=torch.int32)
    st = _lib.load().sbev_project_select(_ptr(sample_points), _ptr(lidar2img), B, Q, T, N_VIEWS, G, P,
                                         float(image_h), float(image_w), float(eps),
                                         _ptr(loc), _ptr(uvh), _ptr(valid), _ptr(iview), _stream())
    _lib.check(st, 'sbev_project_select')
    return (loc, uvh, valid, iview) if dump else loc


def sampling_front(query_bbox, offset, scale_logits, time_diff, pc_range, T, G, P, L,
                   want_points=True, want_weights=True):
    """make_sample_points + velocity warp + level softmax + weight reorder (see sbev_sampling_front in
    include/sbev_hip.h).  offset [B,Q,>=G*P*3] and scale_logits [B,Q,>=G*P*L] may be column slices of one packed
    GEMM output (only their last-dim stride must be 1).
    Returns (sample_points [B,Q,T,G*P,3] | None, weights_bp [B*G*T,Q,P,L] | None)."""
    _need_device(query_bbox, offset, scale_logits, time_diff)
    B, Q = query_bbox.shape[:2]
    dev = query_bbox.device
    query_bbox = query_bbox.contiguous().float()

    def rows(t):
        if t is None:
            return None, 0
        if t.stride(-1) != 1 or t.stride(0) != Q * t.stride(1):
            t = t.contiguous()
        return t, t.stride(1)

    offset, ld_off = rows(offset if want_points else None)
    scale_logits, ld_lg = rows(scale_logits if want_weights else None)
    td = time_diff.contiguous().float() if want_points else None
    pts = torch.empty(B, Q, T, G * P, 3, device=dev, dtype=torch.float32) if want_points else None
    wbp = torch.empty(B * G * T, Q, P, L, device=dev, dtype=torch.float32) if want_weights else None
    pc = (ctypes.c_double * 6)(*[float(v) for v in pc_range])
    st = _lib.load().sbev_sampling_front(_ptr(query_bbox), _ptr(offset), ld_off, _ptr(scale_logits), ld_lg, _ptr(td), pc,
                                         B, Q, T, G, P, L, _ptr(pts), _ptr(wbp), _stream())
    _lib.check(st, 'sbev_sampling_front')
    return pts, wbp
