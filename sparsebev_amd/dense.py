"""Dense half of the decoder layer (linears, LayerNorms, scale-adaptive self attention, adaptive mixing,
box refinement, NCHW->NHWC relayout) on the device.

Every op here is a hand-written gfx950 kernel in libsbev_hip.so (``NATIVE`` names the kernel behind each);
nothing runs through rocBLAS / ATen, and every function requires device tensors -- there is no CPU path.
"""
import contextlib
import ctypes

import torch

from . import _lib

# op -> kernel(s) it launches
NATIVE = {
    'linear': 'hip: gemm_nt_f32_kernel (v_mfma_f32_32x32x2_f32), split-K + fused bias/ReLU/residual/LayerNorm reducer',
    'linear_group': 'hip: gemm_group_small_kernel (cls / reg branch levels side by side)',
    'layer_norm': 'hip: splitk_reduce_kernel (1 slab)',
    'ln_linear': 'hip: gemm_group_small_kernel with the LayerNorm prologue (row statistics exchanged through LDS)',
    'linear_ln_relu': 'hip: gemm + LayerNorm/ReLU reducer; Linear(3->D): linear3_ln_relu_kernel',
    'self_attention': 'hip: gemm (q|k|v|tau) + sasa_kernel (flash-style, v_mfma_f32_16x16x4_f32) + gemm (out-proj, fused residual)',
    'adaptive_mixing': 'hip: gemm (generator) + adaptive_mixing_kernel (v_mfma_f32_16x16x4_f32) + split-K gemm (out-proj, fused residual + LayerNorm)',
    'linear_bf16s': 'hip: gemm_bf16s_gen_kernel / gemm_bf16s_out_kernel (v_mfma_f32_32x32x16_bf16 on hi + mid + lo bf16 images, fp32 accumulate)',
    'refine_bbox': 'hip: refine_kernel',
    'to_channels_last': 'hip: transpose_tiles_kernel',
}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('sparsebev_amd.dense needs device tensors (no CPU fallback)')


def _rows(x, width=None):
    """x as contiguous rows [-1, width] (width: its last dimension unless given)"""
    return x.reshape(-1, x.shape[-1] if width is None else width).contiguous()


def _ws(nbytes, device):
    """Reusable split-K workspace (one per device; grown on demand, stream-ordered reuse).  Under a torch graph capture the workspace
    is the capture's own, from its memory pool: a captured launch keeps its pointer, while the shared buffer is replaced -- freed -- as
    soon as a larger call comes along (a second captured step at a larger shape), and the next capture's empty_cache() unmaps it."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
    key = str(device)
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
        _WORKSPACES[key] = buf
    return buf


_WORKSPACES = {}
SPLITK_MIN_K = 2048          # reductions at least this long with few output tiles go split-K


def _splits_for(M, N, K):
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if K < SPLITK_MIN_K or tiles >= 128 or N % 4 or N > 1024:
        return 1
    return int(_lib.load().sbev_linear_splitk_plan(M, N, K))


def linear(x, w, b, relu=False, residual=None, ln=None, ln_relu=False):
    """y = act(x @ w.T + b) (+ residual), optionally followed by LayerNorm(ln=(gamma, beta)) (+ ReLU): the
    fp32 MFMA GEMM of csrc/gemm.hip (split-K with the fused epilogue when the reduction is long)."""
    _dev(x, w)
    K, N = x.shape[-1], w.shape[0]
    lead = x.shape[:-1]
    x2 = _rows(x)
    M = x2.shape[0]
    if K % 4 != 0:                                   # only the 3-wide position-encoder input; see position_encode()
        raise RuntimeError('sbev linear needs K %% 4 == 0 (got K=%d)' % K)
    w = w.contiguous()
    res2 = residual.reshape(-1, N).contiguous() if residual is not None else None
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    splits = _splits_for(M, N, K)
    if splits > 1 or (ln is not None and N % 4 == 0 and N <= 1024 and K >= 1024):
        if ln is not None and ln_relu:      # the fused epilogue's ReLU is the Linear's activation (before the residual), not the LayerNorm's
            raise RuntimeError('ln_relu with split-K: use layer_norm(relu=True) separately')
        wsb = lib.sbev_linear_splitk_workspace(M, N, splits)
        ws = _ws(wsb, x.device)
        st = lib.sbev_linear_splitk_f32(_p(x2), _p(w), _p(b), _p(res2), _p(ln[0] if ln else None), _p(ln[1] if ln else None),
                                        1e-5, _p(y), M, N, K, K, K, int(relu or (ln_relu and ln is None)), splits, _p(ws), _stream())
        _lib.check(st, 'sbev_linear_splitk_f32')
        return y.reshape(*lead, N)
    st = lib.sbev_linear_f32(_p(x2), _p(w), _p(b), _p(res2), _p(y), M, N, K, K, K, N, int(relu), _stream())
    _lib.check(st, 'sbev_linear_f32')
    y = y.reshape(*lead, N)
    if ln is not None:
        y = layer_norm(y, ln[0], ln[1], relu=ln_relu)
    return y


# ---- split-bf16 Linears (csrc/gemm_bf16s.hip): nimg = 3 "bf16x6" (fp32-class), nimg = 2 "bf16x3" ------------------------------
def split_bf16s_rows(x, nimg=3):
    """fp32 [rows, K] -> int16 [nimg, rows, K]: the row-major bf16 planes hi (, mid), lo with x == sum of the planes exactly
    (nimg = 3) / to 2^-17 relative (nimg = 2).  Operand format of linear_bf16s_gen."""
    _dev(x)
    x2 = _rows(x)
    rows, K = x2.shape
    out = torch.empty(nimg, rows, K, device=x.device, dtype=torch.int16)
    st = _lib.load().sbev_split_bf16s_rows(_p(x2), K, _p(out), rows, K, nimg, _stream())
    _lib.check(st, 'sbev_split_bf16s_rows')
    return out


def pack_bf16s_frags(w, nimg=3):
    """fp32 [N, K] -> int16 [ceil(N/32), K/16, nimg, 64, 8]: the bf16 images of W in v_mfma_f32_32x32x16_bf16 operand order
    (a ragged last 32-row block repeats row N - 1) -- the operand format of linear_bf16s_gen and linear_splitk_bf16s."""
    _dev(w)
    w = w.reshape(-1, w.shape[-1]).contiguous()
    N, K = w.shape
    out = torch.empty((N + 31) // 32, K // 16, nimg, 64, 8, device=w.device, dtype=torch.int16)
    st = _lib.load().sbev_pack_bf16s_frags(_p(w), K, _p(out), N, K, nimg, _stream())
    _lib.check(st, 'sbev_pack_bf16s_frags')
    return out


def linear_bf16s_gen(x, w_frags, b, nimg=3, relu=False):
    """y = act(x @ W.T + b) with W given as pack_bf16s_frags [N/32, K/16, nimg, 64, 8]; x fp32 [.., K] is split and packed
    here (one small launch).  N % 256 == 0, K % 32 == 0 (the parameter generator's shape)."""
    _dev(x, w_frags)
    K, N = x.shape[-1], w_frags.shape[0] * 32
    xs = pack_bf16s_frags(x, nimg)
    M = x.numel() // K
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    st = _lib.load().sbev_linear_bf16s_gen(_p(xs), _p(w_frags), _p(b), _p(y), M, N, K, N, int(relu), nimg, _stream())
    _lib.check(st, 'sbev_linear_bf16s_gen')
    return y.reshape(*x.shape[:-1], N)


def _splitk_out_proj(who, x, w_frags, b, residual, ln, relu, mode, call):
    """What the split-image out-projections share: rows of x, the slab workspace for the kernels' plan (raises where they do not cover
    the shape), residual and output, and the argument tail every one of their C calls ends with (bias ... stream; mode = nimg /
    nprod).  call(lib, x2, N, tail) makes the C call(s) while all of these are alive."""
    _dev(x, w_frags)
    K, N = x.shape[-1], w_frags.shape[0] * 32
    x2 = _rows(x)
    M = x2.shape[0]
    lib = _lib.load()
    plan = lib.sbev_linear_bf16s_out_plan(M, N, K)
    if plan <= 0:
        raise RuntimeError('%s does not cover M=%d N=%d K=%d' % (who, M, N, K))
    ws = _ws(plan * M * N * 4, x.device)
    res2 = _rows(residual, N) if residual is not None else None
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    lnw, lnb = ln if ln else (None, None)
    call(lib, x2, N, (_p(b), _p(res2), _p(lnw), _p(lnb), 1e-5, _p(y), M, N, K, K, int(relu), mode, _p(ws), _stream()))
    return y.reshape(*x.shape[:-1], N)


def linear_splitk_bf16s(x, w_frags, b, nimg=3, residual=None, ln=None, relu=False):
    """y = LayerNorm?(act(x @ W.T + b) + residual) with W given as pack_bf16s_frags [N/32, K/16, nimg, 64, 8], N == 256
    (the out-projection's shape); x stays fp32 and is split inside the kernel."""
    def call(lib, x2, N, tail):
        _lib.check(lib.sbev_linear_splitk_bf16s(_p(x2), _p(w_frags), *tail), 'sbev_linear_splitk_bf16s')

    return _splitk_out_proj('sbev_linear_splitk_bf16s', x, w_frags, b, residual, ln, relu, nimg, call)


# ---- fp16 hi + lo Linears (csrc/gemm_bf16s.hip, MODE 2 / 3): x 2^e = hi + lo (two fp16 images), 3 or 4 image products --------------
def pack_f16s_frags(w, per_tensor=False):
    """fp32 [N, K] -> (int16 [ceil(N/32), K/16, 2, 64, 8] fp16 hi / lo images of W * 2^e in MFMA operand order, scales): e per row
    (scales = [2, N]: 2^e, 2^-e) or one for the matrix (per_tensor: scales = [2]), chosen so that the scaled maximum is in [2^14, 2^15)."""
    _dev(w)
    w = w.reshape(-1, w.shape[-1]).contiguous()
    N, K = w.shape
    out = torch.empty((N + 31) // 32, K // 16, 2, 64, 8, device=w.device, dtype=torch.int16)
    scales = torch.empty(2 if per_tensor else 2 * N, device=w.device, dtype=torch.float32)
    st = _lib.load().sbev_pack_f16s_frags(_p(w), K, _p(out), _p(scales), N, K, int(per_tensor), _stream())
    _lib.check(st, 'sbev_pack_f16s_frags')
    return out, (scales if per_tensor else scales.reshape(2, N))


def linear_f16s_gen(x, w_frags, w_scales, b, nprod=3, relu=False, return_scale=False):
    """y = act(x @ W.T + b) with (w_frags, w_scales) = pack_f16s_frags(W); x fp32 [.., K] is scaled (per tensor), split and packed
    here.  N % 256 == 0, K % 32 == 0 (the parameter generator's shape).  return_scale: also x's {2^e, 2^-e} (device, [2])."""
    _dev(x, w_frags)
    K, N = x.shape[-1], w_frags.shape[0] * 32
    xs, xsc = pack_f16s_frags(x, per_tensor=True)
    M = x.numel() // K
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    st = _lib.load().sbev_linear_f16s_gen(_p(xs), _p(xsc), _p(w_frags), _p(w_scales[1]), _p(b), _p(y), M, N, K, N, int(relu), nprod, _stream())
    _lib.check(st, 'sbev_linear_f16s_gen')
    y = y.reshape(*x.shape[:-1], N)
    return (y, xsc) if return_scale else y


def f16s_tensor_scale(x):
    """{2^e, 2^-e} (device fp32 [2]) with max |x| 2^e in [2^14, 2^15): the operand scale gemm_tn_f16s takes.  x: fp32, contiguous,
    numel % 4 == 0."""
    _dev(x)
    x = x.contiguous()
    n = x.numel()
    K = x.shape[-1] if x.dim() >= 2 and x.shape[-1] % 4 == 0 else n
    out = torch.empty(2, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().sbev_f16s_tensor_scale(_p(x), K, n // K, K, _p(out), _stream()), 'sbev_f16s_tensor_scale')
    return out


def gemm_tn_f16s(A, lda, a_scale, B, ldb, b_scale, M, N, K, out=None, ldc=None, accumulate=False):
    """C[M,N] (+)= sum_k A[k*lda + m] B[k*ldb + n] (grad_W = grad_y^T . x) on the fp16 hi + lo kernels; a_scale / b_scale: device
    {2^e, 2^-e} of the operands (f16s_tensor_scale or a bound).  See sbev_gemm_tn_f16s."""
    _dev(A, B)
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
        ldc = N
    st = _lib.load().sbev_gemm_tn_f16s(_p(A), lda, _p(a_scale), _p(B), ldb, _p(b_scale), _p(out), ldc, M, N, K, int(accumulate), _stream())
    _lib.check(st, 'sbev_gemm_tn_f16s')
    return out


def f16s_pairs(x, up_log2):
    """fp32 -> int32 of the same shape: (fp16 hi, fp16 lo) of x * 2^up_log2 packed in one 32-bit slot (hi in the low half)"""
    _dev(x)
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().sbev_f16s_pairs(_p(x), _p(out), x.numel(), int(up_log2), _stream()), 'sbev_f16s_pairs')
    return out


def linear_splitk_f16s(x, w_frags, w_scales, b, nprod=3, residual=None, ln=None, relu=False, x_up_log2=None, x_is_pairs=False, x_scale=None):
    """y = LayerNorm?(act(x @ W.T + b) + residual), N == 256, with (w_frags, w_scales) = pack_f16s_frags(W); x stays fp32 and is
    multiplied by 2^x_up_log2 and split inside the kernel (default: from max |x|, one host sync -- the decoder passes its bound);
    x_is_pairs: x is f16s_pairs(x_fp32, x_up_log2) (int32), only de-interleaved inside the kernel;
    x_scale: device {2^e, 2^-e} of x (f16s_tensor_scale) instead of a host-side exponent -- no sync, no bound."""
    def call(lib, x2, N, tail):
        if x_scale is not None:
            st = lib.sbev_linear_splitk_f16s_xdev(_p(x2), _p(x_scale), _p(w_frags), _p(w_scales[1]), *tail)
            return _lib.check(st, 'sbev_linear_splitk_f16s_xdev')
        up = x_up_log2
        if up is None:
            import math
            mx = float(x2.abs().max())
            up = 15 - math.frexp(mx)[1] if mx > 0 and math.isfinite(mx) else 0
        nscale = torch.empty(N, device=x.device, dtype=torch.float32)
        _lib.check(lib.sbev_f16s_out_scale(_p(w_scales[1]), int(up), _p(nscale), N, _stream()), 'sbev_f16s_out_scale')
        st = lib.sbev_linear_splitk_f16s(_p(x2), int(x_is_pairs), int(up), _p(w_frags), _p(nscale), *tail)
        _lib.check(st, 'sbev_linear_splitk_f16s')

    return _splitk_out_proj('sbev_linear_splitk_f16s', x, w_frags, b, residual, ln, relu, nprod, call)


class _LinearProblem(ctypes.Structure):
    """struct sbev_linear_problem (include/sbev_hip.h)"""
    _fields_ = [('X', ctypes.c_void_p), ('W', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('residual', ctypes.c_void_p),
                ('Y', ctypes.c_void_p), ('M', ctypes.c_int64), ('N', ctypes.c_int32), ('K', ctypes.c_int32),
                ('ldx', ctypes.c_int64), ('ldw', ctypes.c_int64), ('ldy', ctypes.c_int64), ('relu', ctypes.c_int32)]


def linear_group(problems):
    """Up to 3 independent small linears [(x, w, b, relu), ...] (same K = 256 / 512) in one launch; returns the list
    of outputs.  Same arithmetic per output tile as linear() on each -- used for the cls / reg branches."""
    n = len(problems)
    arr = (_LinearProblem * n)()
    keep, outs = [], []
    for i, (x, w, b, relu) in enumerate(problems):
        _dev(x, w)
        K, N = x.shape[-1], w.shape[0]
        x2 = _rows(x)
        w = w.contiguous()
        y = torch.empty(x2.shape[0], N, device=x.device, dtype=torch.float32)
        keep += [x2, w]
        outs.append(y.reshape(*x.shape[:-1], N))
        arr[i] = _LinearProblem(x2.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, None, y.data_ptr(),
                                x2.shape[0], N, K, K, K, N, int(relu))
    st = _lib.load().sbev_linear_group_f32(ctypes.cast(arr, ctypes.c_void_p), n, _stream())
    _lib.check(st, 'sbev_linear_group_f32')
    return outs


def ln_linear(x, ln_w, ln_b, w, b, eps=1e-5, ln_relu=False, add_after=None, relu=False, residual=None):
    """xn = relu?(LayerNorm(x)) (+ add_after);  y = act(xn @ w.T + b) (+ residual).  Returns (xn, y).  One launch:
    the LayerNorm is the prologue of the Linear's small-tile kernel (csrc/gemm.hip), the way the decoder runtime runs
    the position encoder's last norm + attention in_proj, norm1 + the sampling Linear and norm3 + the branch heads."""
    _dev(x, ln_w, ln_b, w)
    K, N = x.shape[-1], w.shape[0]
    lead = x.shape[:-1]
    x2 = _rows(x)
    M = x2.shape[0]
    w = w.contiguous()
    aa = add_after.reshape(-1, K).contiguous() if add_after is not None else None
    rr = residual.reshape(-1, N).contiguous() if residual is not None else None
    xn = torch.empty_like(x2)
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    st = _lib.load().sbev_ln_linear_f32(_p(x2), _p(ln_w), _p(ln_b), eps, int(ln_relu), _p(aa), _p(xn), _p(w), _p(b), _p(rr), _p(y),
                                        M, N, K, K, N, int(relu), _stream())
    _lib.check(st, 'sbev_ln_linear_f32')
    return xn.reshape(x.shape), y.reshape(*lead, N)


def layer_norm(x, w, b, eps=1e-5, relu=False, add_after=None):
    """relu?(LayerNorm(x)) (+ add_after)"""
    _dev(x, w, b)
    N = x.shape[-1]
    x2 = _rows(x)
    y = torch.empty_like(x2)
    aa = add_after.reshape(-1, N).contiguous() if add_after is not None else None
    st = _lib.load().sbev_layer_norm_f32(_p(x2), _p(w), _p(b), eps, _p(aa), _p(y), x2.shape[0], N, int(relu), _stream())
    _lib.check(st, 'sbev_layer_norm_f32')
    return y.reshape(x.shape)


def linear_ln_relu(x, w, b, lnw, lnb):
    """relu(LayerNorm(x @ w.T + b)).  K == 3 (position encoder, input = the first 3 columns of query_bbox) has
    its own kernel: 3 FMAs per output are not a GEMM."""
    if w.shape[1] == 3:
        _dev(x, w)
        N = w.shape[0]
        ldx = x.shape[-1]
        x2 = _rows(x)
        y = torch.empty(x2.shape[0], N, device=x.device, dtype=torch.float32)
        st = _lib.load().sbev_linear3_ln_relu_f32(_p(x2), ldx, _p(w.contiguous()), _p(b), _p(lnw), _p(lnb), 1e-5, _p(y),
                                                  x2.shape[0], N, _stream())
        _lib.check(st, 'sbev_linear3_ln_relu_f32')
        return y.reshape(*x.shape[:-1], N)
    return linear(x, w, b, ln=(lnw, lnb), ln_relu=True)


_CAT_CACHE = {}
_STEP_IMAGES = None     # inside step_images(): key -> (source tensors, derived image); otherwise None


@contextlib.contextmanager
def step_images():
    """The scope of ONE training step in which every derived weight image (autograd._transposed, autograd._f16_frags, _cat_rows) is
    derived once, by launches of the step itself, and shared by the step's layers -- instead of coming from the process-wide caches
    keyed on the parameters' ``_version``.  The captured steps (train_graph) run warm-up, capture and therefore every replay under it:
    a graph captured on warm caches would record no transpose and no pack, and go on reading the images of the weights as they were at
    capture after an optimizer has moved them.  Under a capture the images come from the capture's memory pool.  Nests: an inner scope
    shares the outer one's images."""
    global _STEP_IMAGES
    outer = _STEP_IMAGES
    if outer is None:
        _STEP_IMAGES = {}
    try:
        yield
    finally:
        _STEP_IMAGES = outer


def in_step_images():
    """True inside a step_images() scope (the backbone's and the neck's weight packs then belong to the step: resnet.py, fpn.py)"""
    return _STEP_IMAGES is not None


def step_image(kind, tensors, make):
    """Inside a step_images() scope: the scope's one derived image ``kind`` of ``tensors``, by ``make()`` at the first call"""
    scope = _STEP_IMAGES
    key = (kind,) + tuple(id(t) for t in tensors)
    hit = scope.get(key)
    if hit is not None and all(a is b for a, b in zip(hit[0], tensors)):
        return hit[1]
    out = make()
    scope[key] = (tensors, out)       # keeps the sources alive for the step: a recycled id cannot match
    return out


def derived_image(cache_ok, kind, tensors, make, lookup, store):
    """One derived image of ``tensors`` by ``make()``: from the step's scope inside step_images(); from the process-wide cache
    (``lookup()`` -> image or None, ``store(image)``) in eager code; and while the current stream is capturing outside a scope the caches
    are neither read nor filled -- an image cached at capture would be read by every replay, whatever the weights have become."""
    if _STEP_IMAGES is not None:
        return step_image(kind, tensors, make)
    if not cache_ok or (tensors[0].is_cuda and torch.cuda.is_current_stream_capturing()):
        return make()
    out = lookup()
    if out is None:
        out = make()
        store(out)
    return out


class WeightImage:
    """A module's packed weight image at a fixed address (FPNNeck's and ResNetBackbone's forward and backward packs).  ``key`` is
    ``(data_ptr, _version)`` of every source tensor at the last pack (after ``extra``), None before the first; ``image`` the tensor.
    ``kind`` names the image in a step_images() scope, ``refusal`` is the message of a stale key under a capture."""

    def __init__(self, kind, refusal):
        self.kind, self.refusal = kind, refusal
        self.key = self.image = None

    def get(self, tensors, make, extra=(), in_step=None):
        """The image of ``tensors``.  Inside step_images(): the scope's own (``in_step()``, else ``make(None)`` once per scope), the
        cache neither read nor filled.  Otherwise the SAME tensor object while the key stands; under a capture a stale key is refused;
        else ``make(dest)`` repacks -- into the old image (``make`` may decline a ``dest`` it cannot use), so the image keeps its
        address and an already captured forward reads the new weights; ``dest`` is None at first and after a change of device."""
        if _STEP_IMAGES is not None:
            return in_step() if in_step is not None else step_image(self.kind, tuple(tensors), lambda: make(None))
        key = tuple(extra) + tuple((t.data_ptr(), t._version) for t in tensors)
        if key == self.key:
            return self.image
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(self.refusal)
        if self.image is not None and self.image.device != tensors[0].device:
            self.image = None
        self.image = make(self.image)
        self.key = key
        return self.image


def ptr_array(tensors):
    """void* [max(len, 1)] of the tensors' addresses for a C entry's pointer list; None: a null entry"""
    return (ctypes.c_void_p * max(len(tensors), 1))(*[None if t is None else t.data_ptr() for t in tensors])


def channels_last_out(who, out, shapes, dev, dtype=None):
    """``out=`` of a dense module's forward, checked: a list of len(shapes) tensors [n, C, h, w] of ``shapes`` in channels-last memory
    on ``dev``, all of ``dtype`` (None: of the first one's, fp16 or fp32).  Returns (the list, the dtype)."""
    out = list(out)
    if len(out) != len(shapes):
        raise ValueError('%s: out must list %d tensors' % (who, len(shapes)))
    if dtype is None:
        dtype = out[0].dtype
        if dtype not in (torch.float16, torch.float32):
            raise TypeError('%s: out must be fp16 or fp32' % who)
    for o, s in zip(out, shapes):
        if tuple(o.shape) != s or o.dtype != dtype or o.device != dev or (o.numel() and not o.permute(0, 2, 3, 1).is_contiguous()):
            raise ValueError('%s: out must be %s tensors of shape %s in channels-last memory on %s' % (who, dtype, s, dev))
    return out, dtype


def _cat_rows(*tensors):
    """torch.cat(tensors, 0), cached until any source is modified in place (parameters are static at inference).
    The entry keeps its source tensors alive and is matched by object identity, so a recycled device address can
    never alias a stale entry.  Inside step_images() / under a capture: see derived_image()."""
    return derived_image(True, 'cat', tensors, lambda: torch.cat([t.detach() for t in tensors], 0).contiguous(),
                         lambda: _cat_lookup(tensors), lambda out: _cat_store(tensors, out))


def _cat_lookup(tensors):
    hit = _CAT_CACHE.get(tuple(id(t) for t in tensors))
    if hit is not None and all(a is b and a._version == v for a, b, v in zip(hit[0], tensors, hit[1])):
        return hit[2]
    return None


def _cat_store(tensors, out):
    if len(_CAT_CACHE) > 64:
        _CAT_CACHE.clear()
    _CAT_CACHE[tuple(id(t) for t in tensors)] = (tensors, tuple(t._version for t in tensors), out)


def scale_adaptive_self_attention(query_bbox, x, pc_range, num_heads, in_w, in_b, out_w, out_b, tau_w, tau_b,
                                  pre_attn_mask=None, ln=None, qkvt=None):
    """models/sparsebev_transformer.py:210-228,236-248 + mmcv MultiheadAttention(batch_first) = x + MHA(x),
    optionally followed by LayerNorm (ln = norm1 of the decoder layer).

    Launches: ONE in-projection GEMM (q | k | v | tau, N = 3D + H) -> flash-style attention with the distance bias
    computed on the fly from the boxes -> out-projection GEMM with the residual (and LayerNorm) fused."""
    _dev(query_bbox, x)
    B, Q, D = x.shape
    hd = D // num_heads
    lib = _lib.load()
    query_bbox = query_bbox.contiguous()
    pc = (ctypes.c_double * 6)(*[float(v) for v in pc_range])
    if (3 * D + num_heads) % 4 != 0:
        raise RuntimeError('3*embed_dims + num_heads must be a multiple of 4')
    if qkvt is None:                                         # else: produced by ln_linear() together with x
        qkvt = linear(x, _cat_rows(in_w, tau_w), _cat_rows(in_b, tau_b))   # [B,Q,3D+H(+pad)]
    mask = None
    if pre_attn_mask is not None:
        mask = pre_attn_mask.to(device=x.device, dtype=torch.uint8).contiguous()
    att = torch.empty(B, Q, D, device=x.device, dtype=torch.float32)
    _lib.check(lib.sbev_sasa_f32(_p(qkvt), qkvt.shape[-1], _p(query_bbox), pc, _p(mask), _p(att), B, Q, num_heads, hd, _stream()),
               'sbev_sasa_f32')
    return linear(att, out_w, out_b, residual=x, ln=ln)


def adaptive_mixing(x, query, pg_w, pg_b, op_w, op_b, out_points, ln=None):
    """models/sparsebev_transformer.py:351-381.  x [B,Q,G,Pin,C], query [B,Q,D] -> [B,Q,D]
    (= LayerNorm(query + out_proj(mix)) when ln=(gamma, beta) is given: the norm2 of the decoder layer, fused).

    Three launches: parameter-generator GEMM -> per-(query, group) mixing kernel -> split-K out-projection whose
    slab reducer also applies bias, the `query +` residual and the LayerNorm."""
    _dev(x, query)
    B, Q, G, Pin, C = x.shape
    D = query.shape[-1]
    x = x.contiguous()
    params = linear(query, pg_w, pg_b)                                     # [B,Q,G*(C*C+Pout*Pin)]
    mixed = torch.empty(B, Q, G * out_points * C, device=x.device, dtype=torch.float32)
    st = _lib.load().sbev_adaptive_mixing_f32(_p(x), _p(params), _p(mixed), B * Q, G, Pin, C, out_points, 1e-5, _stream())
    _lib.check(st, 'sbev_adaptive_mixing_f32')
    return linear(mixed, op_w, op_b, residual=query, ln=ln)


def refine_bbox(query_bbox, reg, vel_div):
    """refine_bbox + velocity / time_diff (models/sparsebev_transformer.py:155-160,179-183; inverse_sigmoid
    models/utils.py:87-102)."""
    _dev(query_bbox, reg)
    B, Q, code = reg.shape
    if code != 10 or query_bbox.shape[-1] != 10:
        raise RuntimeError('refine_bbox: the box kernels are built for the 10-wide box code (got code_size=%d)' % code)
    out = torch.empty_like(reg)
    st = _lib.load().sbev_refine_bbox(_p(query_bbox.contiguous()), _p(reg.contiguous()), _p(vel_div), _p(out), B, Q, code, _stream())
    _lib.check(st, 'sbev_refine_bbox')
    return out


def to_channels_last(f):
    """[B,TN,GC,H,W] -> contiguous [B,TN,H,W,GC] (one tiled-transpose launch per level)."""
    _dev(f)
    if f.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return f.permute(0, 1, 3, 4, 2).contiguous()
    B, TN, GC, H, W = f.shape
    f = f.contiguous()
    out = torch.empty(B, TN, H, W, GC, device=f.device, dtype=f.dtype)
    if f.dtype == torch.float32:
        st = _lib.load().sbev_nchw_to_nhwc_f32(_p(f), _p(out), B * TN, GC, H * W, _stream())
        _lib.check(st, 'sbev_nchw_to_nhwc_f32')
    else:                                                    # bf16 / fp16 storage: the 2-byte relayout (bytes are moved, not interpreted)
        st = _lib.load().sbev_nchw_to_nhwc_b16(_p(f), _p(out), B * TN, GC, H * W, _stream())
        _lib.check(st, 'sbev_nchw_to_nhwc_b16')
    return out
