"""Differentiable forms of the decoder-layer ops: torch.autograd.Function wrappers whose forward AND backward are the
hand-written gfx950 kernels of libsbev_hip.so.

The reference trains through the decoder with plain autograd and recomputes the sampling / mixing / attention
``inner_forward`` under ``torch.utils.checkpoint`` (models/sparsebev_transformer.py:231-234,313-317,383-387).  Here every
op of ``SparseBEVTransformerDecoderLayer.forward`` (:162-193) has an explicit backward kernel behind the C ABI
(include/sbev_hip.h, "Training" block), and the three checkpointed blocks keep the same policy by construction: their
Functions save only their small inputs and re-run the forward kernels inside ``backward`` (the 118 MB dynamic-parameter and
mixed-activation tensors of adaptive mixing are never kept across the forward pass).

PyTorch is used for what it is here for -- device memory, streams, and the autograd graph between the Functions; no ATen
math kernel computes anything on this path except the parameter ``cat`` / output ``stack`` / ``nan_to_num`` plumbing.
"""
import ctypes
import os

import torch

from . import _lib, dense, ops

_EPS = 1e-5


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ---- the two GEMMs of every Linear backward (csrc/gemm_any.hip) -----------------------------------------------------
def gemm(A, a_kmajor, lda, B, b_kmajor, ldb, M, N, K, out=None, ldc=None, accumulate=False):
    """C[M,N] (+)= sum_k A(m,k) B(k,n) with either operand row-major (k contiguous) or k-major; see sbev_gemm_f32."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
        ldc = N
    need = lib.sbev_gemm_f32_workspace(M, N, K)
    ws = torch.empty(need // 4, device=A.device, dtype=torch.float32) if need > 0 else None
    st = lib.sbev_gemm_f32(_p(A), int(a_kmajor), lda, _p(B), int(b_kmajor), ldb, _p(out), ldc, M, N, K, int(accumulate), _p(ws), _stream())
    _lib.check(st, 'sbev_gemm_f32')
    return out


import weakref

# (id(parameter), kind) -> (weak reference to it, version, device, image); kind 'wt': W^T, 'f16' / 'f16t': pack_f16s_frags of W / W^T.
# A dead or recycled id never matches (`ref() is w`).
_WEIGHT_IMAGES = {}


def invalidate_caches():
    """Drop every cached W^T and fragment image.  Needed after writes that do not bump a tensor's ``_version`` -- ``p.data.copy_(...)``
    as mmcv's Fp16OptimizerHook / EMA hooks do -- before the next backward; ordinary optimizers (in-place ops on the parameter) are
    detected through ``_version`` and need nothing.  ``SparseBEVTransformerDecoder.invalidate_caches()`` calls this and
    re-binds the inference runtime's packed weight images."""
    _WEIGHT_IMAGES.clear()


def _weight_image(cache_ok, kind, w, make):
    """One derived image (``kind``) of the weight ``w`` by ``make()``, cached until the weight is modified in place."""
    # keyed by id() with a weak reference to the tensor OBJECT beside it (a WeakKeyDictionary would compare tensors with ==): the
    # cache never keeps a tensor alive, a recycled id never matches.  Parameters live across steps; the packed q | k | v | tau and
    # sampling weights are one tensor per decoder call shared by its layers (layer.packed_train_weights) and hit here from the second
    # layer's backward on.  Writes through ``.data`` do not bump ``_version``: see invalidate_caches().
    # Inside step_images() (the captured steps) the image belongs to the step instead, and a capture never touches this cache.
    key = (id(w), kind)

    def lookup():
        hit = _WEIGHT_IMAGES.get(key)
        if hit is not None and hit[0]() is w and hit[1] == w._version and hit[2] == w.device:
            return hit[3]
        return None

    def store(image):
        if len(_WEIGHT_IMAGES) >= 64:               # drop the entries of parameters that are gone
            for k in [k for k, v in _WEIGHT_IMAGES.items() if v[0]() is None]:
                del _WEIGHT_IMAGES[k]
        _WEIGHT_IMAGES[key] = (weakref.ref(w), w._version, w.device, image)

    return dense.derived_image(cache_ok, kind, (w,), make, lookup, store)


def _transposed(w):
    """W^T [K, N] of a Linear weight [N, K], made by the tiled-transpose kernel (layout.hip) and cached until the weight is
    modified in place (an optimizer step bumps ``_version``): with it grad_x = grad_y . W is the FORWARD product
    ``linear(grad_y, W^T)`` and runs on the tuned forward kernels -- the small-tile kernel for the 256-wide layers (6.6 us
    instead of a 128 x 128-tile split-K launch + slab sum: 33 us), the strip kernel for grad_mixed (K = 256 -> 32 768 columns),
    the register-tile split-K kernel for the generator's input gradient (K = 32 768).  Costs one 2 x 33.5 MB transpose per
    big weight and optimizer step (12 us each)."""
    def make():
        N, K = w.shape
        wt = torch.empty(K, N, device=w.device, dtype=torch.float32)
        st = _lib.load().sbev_nchw_to_nhwc_f32(_p(_c(w.detach())), _p(wt), 1, N, K, _stream())      # [1, R = N, S = K] -> [1, S, R]
        _lib.check(st, 'sbev_nchw_to_nhwc_f32 (weight transpose)')
        return wt

    return _weight_image(True, 'wt', w, make)


def _f16_frags(w, transposed=False):
    """The fp16 hi + lo fragment image (dense.pack_f16s_frags) of a Linear weight [N, K] -- or of W^T, the operand of grad_x = grad_y . W
    as a generator-shaped GEMM -- cached until the weight is modified in place (like _transposed: one pack per weight update)."""
    return _weight_image(w.is_leaf, 'f16t' if transposed else 'f16', w,
                         lambda: dense.pack_f16s_frags(_transposed(w) if transposed else _c(w.detach())))


step_images = dense.step_images


class Tap:
    """Gradient collector of the parameters a decoder call's layers SHARE (the reference stacks ONE layer six times,
    models/sparsebev_transformer.py:47-50): every backward node ADDS its parameter gradient to the parameter's one buffer in the
    epilogue of the kernel that computes it (sbev_gemm_f32 accumulate, sbev_bias_relu_bwd_acc, sbev_layer_norm_bwd_acc) and returns
    None to autograd; ``ParamTap`` -- one node per call, which autograd runs after every node holding its token -- hands the buffers
    over.  Replaces 5 torch `add` launches per parameter and step (48 parameters: 240 of a step's launches), and
    an ``AccumulateGrad`` hook (DDP) sees each parameter once, complete.  Like FeatureTap there is no forward-time counter: partial
    losses and repeated backward passes work.  The buffers are reached through ``sink`` (before a launch) and ``commit`` (after it)."""

    def __init__(self, params):
        self.ids = {id(p) for p in params if p.requires_grad}
        self.bufs = {}
        self.deferred = {}          # id(weight) -> [(grad_y [M, N], x [M, K]), ...]: small weight gradients, reduced in one launch at the end
        self.deferred_bias = {}     # id(bias) -> [grad_y [M, N], ...]: the bias's OWN recorded matrices (their column sums, at the end) -- not
                                    # the weight's list: a node that adds its bias gradient directly still records for the weight
        self.deferred_ln = {}       # (id(gamma), id(beta)) -> [gamma, beta, relu, [(grad_y, x, row statistics), ...]]
        self.token = ParamTap.apply(self, *params) if self.ids else None
        self._empty = None
        self._seen = {}             # id(backward node) -> (weak reference to it, graph task id of the execution that recorded)

    def fresh_pass(self):
        """Called by every recording node.  Segments left behind by a backward pass that RAISED before ParamTap ran must not leak into
        a retry over the same graph (retain_graph) -- but a different graph-task id alone does not mean the earlier pass is dead: a
        NESTED pass (``torch.utils.checkpoint(use_reentrant=True)`` around decoder layers, any Function that runs a backward inside
        the outer one) has its own id while the outer pass is merely suspended, and its records belong to the same ParamTap (round 4
        discarded on every id change: silently too-small parameter gradients under reentrant checkpointing -- ADVICE r4).  What does
        identify a dead pass: a backward NODE that already contributed to the pending sums executes AGAIN under another task id while
        ParamTap has not run in between -- a node runs once per pass, nested passes run other node objects (the recomputed graph's),
        so this is a new pass over the same graph and the pending sums are an aborted pass's.  (Not covered: an aborted pass whose
        every tapped node sat inside a reentrant checkpoint, retried -- the recomputed nodes are new objects; build a new forward.)"""
        if self.token is None:              # nothing to collect (no tap, or no parameter needs a gradient): nothing is ever recorded
            return
        get_node = getattr(torch._C, '_current_autograd_node', None)
        node = get_node() if get_node is not None else None
        if node is None:
            return
        task = torch._C._current_graph_task_id() if hasattr(torch._C, '_current_graph_task_id') else None
        hit = self._seen.get(id(node))
        if hit is not None and hit[0]() is node:
            if hit[1] == task:
                return                      # the same execution asking again (a node asks once per parameter)
            # re-executed with its earlier contribution still pending: the earlier pass never reached ParamTap
            self.deferred, self.deferred_bias, self.deferred_ln, self.bufs, self._seen = {}, {}, {}, {}, {}
        try:
            self._seen[id(node)] = (weakref.ref(node), task)
        except TypeError:                   # (a node type without weak references: no dead-pass detection for it)
            pass

    def has(self, pid):
        if self.token is None:
            return False
        self.fresh_pass()                   # (every tapped backward node asks this first)
        return pid in self.ids

    def filled(self, pid):
        """does the parameter already have a buffer in this pass (the next launch for it accumulates)"""
        return pid in self.bufs

    def sink(self, tapped, pid, like, shape=None):
        """Where a backward launch writes the gradient of parameter ``pid``, and its accumulate flag: the parameter's buffer and 1 when a
        tapped one has a buffer already; else a fresh fp32 tensor (``shape`` on ``like``'s device, or like ``like``) and 0."""
        buf = self.bufs.get(pid) if tapped else None
        if buf is not None:
            return buf, 1
        return (torch.empty_like(like) if shape is None else torch.empty(shape, device=like.device, dtype=torch.float32)), 0

    def commit(self, tapped, pid, buf):
        """After the launch's status check: a tapped parameter's buffer is registered for ParamTap's hand-over; returns what the node
        returns to autograd for the parameter -- None then, the fresh gradient itself when it is not tapped."""
        if not tapped:
            return buf
        self.bufs[pid] = buf
        return None

    def token_grad(self):
        """the token's (empty) gradient a tapped node returns; None for a node that took no token"""
        if self.token is None:
            return None
        if self._empty is None:
            self._empty = self.token.new_empty(0)
        return self._empty


_NO_TAP = Tap(())       # what a node without a tap holds instead: has() is False, sink() / commit() hand a fresh tensor through


def token_args(tap):
    """the ``(tap, token)`` tail of a tapped Function's ``apply``; empty without a tap or when none of its parameters needs a gradient"""
    return (tap, tap.token) if (tap is not None and tap.token is not None) else ()


def _pc6(pc_range):
    return (ctypes.c_double * 6)(*[float(v) for v in pc_range])


class ParamTap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tap, *params):
        ctx.tap, ctx.pids = tap, [id(p) for p in params]
        return params[0].new_empty(0)

    @staticmethod
    def backward(ctx, gtoken):
        tap = ctx.tap
        try:
            _group_bias_grads(tap)
            _group_ln_grads(tap)
            for pid, segs in tap.deferred.items():
                _multi_wgrad(tap, pid, segs)
            bufs = tap.bufs
            return (None, *[bufs.pop(pid, None) for pid in ctx.pids])
        finally:                        # whatever happened: the next backward pass starts from empty lists
            tap.deferred, tap.deferred_bias, tap.deferred_ln, tap._seen = {}, {}, {}, {}


def _plan_launches(jobs, max_jobs, max_segs=8):
    """The grouped reductions' launches.  ``jobs``: one ``(key, rows, number of segments, already has a buffer)`` per parameter in
    recording order; returns ``[(rows, [(key, seg_start, seg_stop, accumulate), ...]), ...]``: at most ``max_segs`` segments per entry,
    at most ``max_jobs`` entries and one row count per launch.  The second chunk of a parameter (more than ``max_segs`` layers) adds to
    what the first one wrote, so it goes into a LATER launch.  Plain values in and out: no tensor, no library."""
    rounds = {}                         # (chunk start, rows) -> entries, in recording order
    for key, rows, nseg, filled in jobs:
        for s0 in range(0, nseg, max_segs):
            rounds.setdefault((s0, rows), []).append((key, s0, min(s0 + max_segs, nseg), s0 > 0 or bool(filled)))
    return [(rows, part[j0:j0 + max_jobs]) for (_, rows), part in sorted(rounds.items()) for j0 in range(0, len(part), max_jobs)]


def _group_bias_grads(tap):
    """the recorded biases' gradients: column sums over all layers' grad_y matrices, <= 16 biases per sbev_colsum_group launch"""
    rec = tap.deferred_bias
    jobs = [(b_id, gs[0].shape[0], len(gs), tap.filled(b_id)) for b_id, gs in rec.items() if gs]
    for M, part in _plan_launches(jobs, 16):
        ng = len(part)
        segs = (ctypes.c_void_p * (ng * 8))()
        outs = (ctypes.c_void_p * ng)()
        Ns, nsegs, accs = (ctypes.c_int32 * ng)(), (ctypes.c_int32 * ng)(), (ctypes.c_int32 * ng)()
        bufs = []
        for i, (b_id, s0, s1, acc) in enumerate(part):
            gs = rec[b_id][s0:s1]
            N = gs[0].shape[1]
            bufs.append(tap.sink(True, b_id, gs[0], (N,))[0])
            for k, g in enumerate(gs):
                segs[i * 8 + k] = g.data_ptr()
            outs[i], Ns[i], nsegs[i], accs[i] = bufs[i].data_ptr(), N, len(gs), int(acc)
        _lib.check(_lib.load().sbev_colsum_group(segs, outs, Ns, nsegs, accs, ng, M, _stream()), 'sbev_colsum_group')
        for (b_id, _, _, _), buf in zip(part, bufs):
            tap.commit(True, b_id, buf)


_LN_GROUP = os.environ.get('SBEV_NO_LN_GROUP', '0') != '1'   # A/B switch: LayerNorm parameter gradients per layer (1) or grouped per call


def _group_ln_grads(tap):
    """the recorded LayerNorms' dgamma / dbeta: sums over all layers' (grad_y, x, statistics), <= 8 LayerNorms per launch"""
    rec = tap.deferred_ln
    jobs = [(ids, v[3][0][0].shape[0], len(v[3]), tap.filled(ids[0])) for ids, v in rec.items() if v[3]]
    VP = ctypes.c_void_p
    for M, part in _plan_launches(jobs, 8):
        ng = len(part)
        dYs, Xs, Ss = (VP * (ng * 8))(), (VP * (ng * 8))(), (VP * (ng * 8))()
        gam, bet, dgs, dbs = (VP * ng)(), (VP * ng)(), (VP * ng)(), (VP * ng)()
        Ns, nsegs, relus, accs = [(ctypes.c_int32 * ng)() for _ in range(4)]
        bufs = []
        for i, ((g_id, b_id), s0, s1, acc) in enumerate(part):
            g, b, relu, segs = rec[(g_id, b_id)]
            dg, dbeta = tap.sink(True, g_id, g)[0], tap.sink(True, b_id, b)[0]
            bufs.append((dg, dbeta))
            for k, (gy, x, st) in enumerate(segs[s0:s1]):
                dYs[i * 8 + k], Xs[i * 8 + k], Ss[i * 8 + k] = gy.data_ptr(), x.data_ptr(), st.data_ptr()
            gam[i], bet[i], dgs[i], dbs[i] = g.data_ptr(), b.data_ptr(), dg.data_ptr(), dbeta.data_ptr()
            Ns[i], nsegs[i], relus[i], accs[i] = g.shape[0], s1 - s0, int(relu), int(acc)
        _lib.check(_lib.load().sbev_layer_norm_param_group(dYs, Xs, Ss, gam, bet, dgs, dbs, Ns, nsegs, relus, accs, ng, M, _stream()),
                   'sbev_layer_norm_param_group')
        for ((g_id, b_id), _, _, _), (dg, dbeta) in zip(part, bufs):
            tap.commit(True, g_id, dg)
            tap.commit(True, b_id, dbeta)


def _multi_wgrad(tap, pid, segs):
    """grad_W [N, K] = sum over the layers' (grad_y, x) pairs of grad_y^T . x -- one sbev_gemm_f32_multi launch per <= 8 pairs"""
    lib = _lib.load()
    gy0, x0 = segs[0]
    M, N = gy0.shape
    K = x0.shape[1]
    for s0 in range(0, len(segs), 8):
        part = segs[s0:s0 + 8]
        n = len(part)
        buf, acc = tap.sink(True, pid, gy0, (N, K))
        A = (ctypes.c_void_p * n)(*[g.data_ptr() for g, _ in part])
        Bp = (ctypes.c_void_p * n)(*[x.data_ptr() for _, x in part])
        ws = torch.empty(max(lib.sbev_gemm_f32_multi_workspace(N, K, M, n) // 4, 1), device=gy0.device, dtype=torch.float32)
        st = lib.sbev_gemm_f32_multi(A, 1, N, Bp, 1, K, n, _p(buf), K, N, K, M, acc, _p(ws), _stream())
        _lib.check(st, 'sbev_gemm_f32_multi')
        tap.commit(True, pid, buf)


_DEFER_MAX = 1 << 18      # weight gradients up to 512 x 512 wait for the end of the call (their operands are < 2 MB per layer)
_BIAS_DEFER_MAX = 1 << 21 # recorded (masked) grad_y matrices of a bias: rows x columns per layer (8 MB at most)


def _defers(tap, pid, A, a_km, lda, b_km, ldb, M, N, K):
    return bool(a_km and b_km and M * N <= _DEFER_MAX and lda == M and ldb == N and K % 4 == 0 and K == A.shape[0] and A.is_contiguous()
                and (not tap.deferred.get(pid) or tap.deferred[pid][0][0].shape == A.shape))


def _wgrad(tap, pid, tapped, gz, x2, ld, K=None):
    """grad_W [N, K] = grad_z^T . x of a Linear from grad_z [M, N] and x [M, ld] (K = ld unless the Linear reads only x's first K columns).
    Tapped: (+)= into the parameter's buffer, None returned -- small gradients (both operands k-major, see _defers) are only recorded
    here: ParamTap reduces all layers' pairs in one launch.  Not tapped: returned as a new tensor."""
    M, N = gz.shape
    K = ld if K is None else K
    if not tapped:
        return gemm(gz, True, N, x2, True, ld, N, K, M)                     # grad_z^T . x
    tap.fresh_pass()
    if _defers(tap, pid, gz, True, N, True, ld, N, K, M):
        tap.deferred.setdefault(pid, []).append((gz, x2))
        return None
    buf, acc = tap.sink(True, pid, gz, (N, K))
    gemm(gz, True, N, x2, True, ld, N, K, M, out=buf, ldc=K, accumulate=acc)
    return tap.commit(True, pid, buf)


def _mixed_up_log2(n):
    """largest e with sqrt(n) 2^e < 65504: the fp16 scale of relu(LayerNorm over n elements, no affine) (csrc: sbev_decoder_mixed_up_log2)"""
    import math
    e = 0
    while math.sqrt(n) * 2.0 ** (e + 1) < 65504.0 and e < 15:
        e += 1
    return e


_SCALE_CONST = {}    # (device, e) -> fp32 [2] {2^e, 2^-e}


def _const_scale(device, e):
    """a caller-side bound as the device scale pair the fp16 GEMMs take"""
    key = (str(device), int(e))
    t = _SCALE_CONST.get(key)
    if t is None:
        t = _SCALE_CONST[key] = torch.tensor([2.0 ** e, 2.0 ** -e], device=device, dtype=torch.float32)
    return t


_WGRAD_F16 = os.environ.get('SBEV_NO_WGRAD_F16', '0') != '1'    # A/B switch: the two big grad_W GEMMs on the fp16 kernel (gemm_tn_f16s.hip)


_GQ_F16 = os.environ.get('SBEV_NO_GQ_F16', '0') != '1'          # A/B switch: grad_query = grad_params . W_pg on the fp16 split-K kernel


def _wgrad_tn_f16(tap, pid, tapped, A, lda, a_scale, B, ldb, b_scale, M, N, K):
    """grad_W [M, N] = A^T B on the fp16 hi + lo kernel: into the tapped parameter's buffer (returns None) or as a new tensor"""
    buf, acc = tap.sink(tapped, pid, A, (M, N))
    dense.gemm_tn_f16s(A, lda, a_scale, B, ldb, b_scale, M, N, K, out=buf, ldc=N, accumulate=acc)
    return tap.commit(tapped, pid, buf)


def _linear_grads(gz, w):
    """grad_x [M, K] = grad_z . W from grad_z [M, N] and w [N, K] (the weight's own gradient: _wgrad)"""
    M, N = gz.shape
    K = w.shape[1]
    if N % 4 == 0 and K % 4 == 0:
        return dense.linear(gz, _transposed(w), None)                           # grad_y . W as a forward Linear with W^T
    return gemm(gz, False, N, w, True, K, M, K, N)                              # 10-wide heads: the layout-generic kernel


def _bias_relu_bwd(gy2, y2, want_db, tap=_NO_TAP, pid=None):
    """(masked grad, bias grad): gy * (y > 0) when y2 is the ReLU output (else gy itself) and its column sums.  With a Tap holding the
    bias (pid) the sums are added to its buffer and None is returned for them."""
    M, N = gy2.shape
    if y2 is None and not want_db:
        return gy2, None
    gz = torch.empty_like(gy2) if y2 is not None else None
    tapped = want_db and tap.has(pid)
    db, acc = tap.sink(tapped, pid, gy2, (N,)) if want_db else (None, 0)
    lib = _lib.load()
    ws = torch.empty(max(lib.sbev_colsum_workspace(M, N) // 4, 1), device=gy2.device, dtype=torch.float32) if want_db else None
    st = lib.sbev_bias_relu_bwd_acc(_p(gy2), _p(y2), _p(gz), _p(db), M, N, N, _p(ws), acc, _stream())
    _lib.check(st, 'sbev_bias_relu_bwd')
    return (gz if gz is not None else gy2), tap.commit(tapped, pid, db)


def _linear_member_bwd(tap, w_id, b_id, gy, x, y, w, relu, need_w, want_db):
    """One Linear's backward up to grad_x: -> (grad_z [M, N], grad_W | None, grad_b | None) from the cotangent, the input, the ReLU
    output (None without ReLU) and the weight.  grad_z is the (masked) cotangent grad_x is made of; a tapped parameter's gradient goes
    into the tap and comes back as None."""
    N, K = w.shape
    gy2 = _c(gy).reshape(-1, N)
    x2 = _c(x).reshape(-1, K)
    y2 = y.reshape(-1, N) if relu else None
    w_tapped = need_w and tap.has(w_id)
    tap.fresh_pass()
    recorded = tap.deferred_bias.get(b_id)
    if (w_tapped and want_db and tap.has(b_id) and gy2.shape[0] * N <= _BIAS_DEFER_MAX and gy2.is_contiguous()
            and (not recorded or recorded[0].shape == gy2.shape)):
        # the bias gradient = column sums of this node's (masked) grad_y, recorded in the bias's own list and summed over all layers
        # at the end (a ReLU Linear: only the mask now -- a fully parallel elementwise launch; the one-launch mask + column sum has
        # N / 64 workgroups, 4 for a 256-wide layer, and took 10 us on the layer's critical path)
        gz, db = (_bias_relu_bwd(gy2, y2, False)[0] if relu else gy2), None
        tap.deferred_bias.setdefault(b_id, []).append(gz)
    else:
        gz, db = _bias_relu_bwd(gy2, y2, want_db, tap, b_id)
    return gz, (_wgrad(tap, w_id, w_tapped, gz, x2, K) if need_w else None), db


class Linear(torch.autograd.Function):
    """y = act(x W^T + b) (+ residual): forward = dense.linear (gemm.hip), backward = gemm_any.hip + bias_relu_bwd."""

    @staticmethod
    def forward(ctx, x, w, b, relu, residual, tap=None, token=None):
        # the ReLU mask is read off the output, which a residual would shift; the decoder layer never combines the two
        if relu and residual is not None:
            raise RuntimeError('autograd.Linear: relu together with a residual is not supported')
        y = dense.linear(x, w, b, relu=relu, residual=residual)
        ctx.relu = bool(relu)
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.has_b = b is not None
        ctx.tap, ctx.w_id, ctx.b_id = tap or _NO_TAP, id(w), id(b)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gz, gw, db = _linear_member_bwd(ctx.tap, ctx.w_id, ctx.b_id, gy, x, y, w, ctx.relu, ctx.needs_input_grad[1],
                                        ctx.has_b and ctx.needs_input_grad[2])
        gx = _linear_grads(gz, _c(w)).reshape(x.shape) if ctx.needs_input_grad[0] else None
        return gx, gw, db, None, gy if ctx.has_res and ctx.needs_input_grad[4] else None, None, ctx.tap.token_grad()


def linear(x, w, b, relu=False, residual=None, tap=None):
    return Linear.apply(x, w, b, relu, residual, *token_args(tap))


class LinearPair(torch.autograd.Function):
    """Two INDEPENDENT Linears in one launch each way (round 6): (ya, yb) = (act_a(xa Wa^T + ba), act_b(xb Wb^T + bb)) through
    dense.linear_group (gemm_group_small_kernel: the grouped launch the inference runtime uses for the two branch heads), and in backward
    both grad_x products as one grouped launch of Linears with W^T.  The decoder layer's classification and regression branches are two
    such chains side by side (models/sparsebev_transformer.py:174-183): 18 small-tile launches per layer and step were 6.4 % of the
    captured training step at 6.3 us each for ~1 us of arithmetic.  Same arithmetic per output tile as two Linear nodes; weight / bias
    gradients go through the same Tap deferral."""

    @staticmethod
    def forward(ctx, xa, wa, ba, relu_a, xb, wb, bb, relu_b, tap=None, token=None):
        ya, yb = dense.linear_group([(xa, wa, ba, relu_a), (xb, wb, bb, relu_b)])
        ctx.relu = (bool(relu_a), bool(relu_b))
        ctx.save_for_backward(xa, wa, ya if relu_a else None, xb, wb, yb if relu_b else None)
        ctx.has_b = (ba is not None, bb is not None)
        ctx.tap, ctx.w_id, ctx.b_id = tap or _NO_TAP, (id(wa), id(wb)), (id(ba), id(bb))
        return ya, yb

    @staticmethod
    def backward(ctx, gya, gyb):
        xa, wa, ya, xb, wb, yb = ctx.saved_tensors
        xs, ws, ys, gys = (xa, xb), (wa, wb), (ya, yb), (gya, gyb)
        need_x = (ctx.needs_input_grad[0], ctx.needs_input_grad[4])
        need_w = (ctx.needs_input_grad[1], ctx.needs_input_grad[5])
        need_b = (ctx.needs_input_grad[2], ctx.needs_input_grad[6])
        gz, gw, db = [None, None], [None, None], [None, None]
        for i in range(2):
            if gys[i] is not None:
                gz[i], gw[i], db[i] = _linear_member_bwd(ctx.tap, ctx.w_id[i], ctx.b_id[i], gys[i], xs[i], ys[i], ws[i], ctx.relu[i],
                                                         need_w[i], ctx.has_b[i] and need_b[i])
        # grad_x = grad_y . W of both members: one grouped launch when both are small-tile shapes (N, K multiples of 4), else one by one
        gx = [None, None]
        both = all(need_x[i] and gz[i] is not None and ws[i].shape[0] % 4 == 0 and ws[i].shape[1] % 4 == 0 for i in range(2)) \
            and ws[0].shape[0] == ws[1].shape[0]
        if both:
            gx = dense.linear_group([(gz[0], _transposed(ws[0]), None, False), (gz[1], _transposed(ws[1]), None, False)])
        else:
            for i in range(2):
                if need_x[i] and gz[i] is not None:
                    gx[i] = _linear_grads(gz[i], _c(ws[i]))
        gxa = gx[0].reshape(xa.shape) if gx[0] is not None else None
        gxb = gx[1].reshape(xb.shape) if gx[1] is not None else None
        return gxa, gw[0], db[0], None, gxb, gw[1], db[1], None, None, ctx.tap.token_grad()


def linear_pair(xa, wa, ba, relu_a, xb, wb, bb, relu_b, tap=None):
    return LinearPair.apply(xa, wa, ba, relu_a, xb, wb, bb, relu_b, *token_args(tap))


def _layer_norm_bwd_acc(tap, tapped, g_id, b_id, gy2, x2, g, b, relu):
    """relu?(LayerNorm) backward in one launch (sbev_layer_norm_bwd_acc): -> (grad_x, dgamma, dbeta) from grad_y [M, N] and the input
    x [M, N]; tapped: dgamma / dbeta are added to the parameters' buffers and come back as None."""
    M, N = x2.shape
    gx = torch.empty_like(x2)
    (dg, acc), (dbeta, acc_b) = tap.sink(tapped, g_id, g), tap.sink(tapped, b_id, b)
    lib = _lib.load()
    stats = torch.empty(max(lib.sbev_layer_norm_bwd_workspace(M, N) // 4, 1), device=x2.device, dtype=torch.float32)
    st = lib.sbev_layer_norm_bwd_acc(_p(gy2), _p(x2), _p(_c(g)), _p(_c(b)), _EPS, int(relu), _p(gx), _p(dg), _p(dbeta), _p(stats),
                                     M, N, acc & acc_b, _stream())
    _lib.check(st, 'sbev_layer_norm_bwd')
    return gx, tap.commit(tapped, g_id, dg), tap.commit(tapped, b_id, dbeta)


class LayerNorm(torch.autograd.Function):
    """relu?(LayerNorm(x)) (+ add_after): forward = dense.layer_norm, backward = sbev_layer_norm_bwd."""

    @staticmethod
    def forward(ctx, x, g, b, relu, add_after, tap=None, token=None):
        y = dense.layer_norm(x, g, b, relu=relu, add_after=add_after)
        ctx.relu = bool(relu)
        ctx.has_add = add_after is not None
        ctx.save_for_backward(x, g, b)
        ctx.tap, ctx.g_id, ctx.b_id = tap or _NO_TAP, id(g), id(b)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g, b = ctx.saved_tensors
        N = x.shape[-1]
        gy2, x2 = _c(gy).reshape(-1, N), _c(x).reshape(-1, N)
        M = x2.shape[0]
        tap = ctx.tap
        tapped = tap.has(ctx.g_id) and tap.has(ctx.b_id)
        if tapped:
            tap.fresh_pass()
        rec = tap.deferred_ln.get((ctx.g_id, ctx.b_id)) if tapped else None
        if (tapped and _LN_GROUP and not tap.filled(ctx.g_id) and g.is_contiguous() and b.is_contiguous()
                and (rec is None or not rec[3] or rec[3][0][0].shape == gy2.shape)):
            # shared LayerNorm: dX and the row statistics now, dgamma / dbeta of all layers in one grouped launch at the end of the call
            gx = torch.empty_like(x2)
            stats = torch.empty(2 * M, device=x.device, dtype=torch.float32)
            st = _lib.load().sbev_layer_norm_bwd_rows(_p(gy2), _p(x2), _p(g), _p(b), _EPS, int(ctx.relu), _p(gx), _p(stats), M, N, _stream())
            _lib.check(st, 'sbev_layer_norm_bwd_rows')
            tap.deferred_ln.setdefault((ctx.g_id, ctx.b_id), [g, b, ctx.relu, []])[3].append((gy2, x2, stats))
            dg = dbeta = None
        else:
            gx, dg, dbeta = _layer_norm_bwd_acc(tap, tapped, ctx.g_id, ctx.b_id, gy2, x2, g, b, ctx.relu)
        return gx.reshape(x.shape), dg, dbeta, None, gy if ctx.has_add and ctx.needs_input_grad[4] else None, None, tap.token_grad()


def layer_norm(x, g, b, relu=False, add_after=None, tap=None):
    return LayerNorm.apply(x, g, b, relu, add_after, *token_args(tap))


class Linear3LnRelu(torch.autograd.Function):
    """relu(LayerNorm(bbox[..., :3] W^T + b)) -- position_encoder[0..2] (models/sparsebev_transformer.py:116-119)."""

    @staticmethod
    def forward(ctx, bbox, w, b, lnw, lnb, tap=None, token=None):
        ctx.tap, ctx.pids = tap or _NO_TAP, (id(w), id(b), id(lnw), id(lnb))
        N = w.shape[0]
        ld = bbox.shape[-1]
        x2 = _c(bbox).reshape(-1, ld)
        M = x2.shape[0]
        y = torch.empty(M, N, device=bbox.device, dtype=torch.float32)
        pre = torch.empty(M, N, device=bbox.device, dtype=torch.float32)
        st = _lib.load().sbev_linear3_ln_relu_ex_f32(_p(x2), ld, _p(_c(w)), _p(b), _p(lnw), _p(lnb), _EPS, _p(y), _p(pre), M, N, _stream())
        _lib.check(st, 'sbev_linear3_ln_relu_ex_f32')
        ctx.save_for_backward(x2, w, lnw, lnb, pre)
        ctx.bshape = bbox.shape
        return y.reshape(*bbox.shape[:-1], N)

    @staticmethod
    def backward(ctx, gy):
        x2, w, lnw, lnb, pre = ctx.saved_tensors
        N = w.shape[0]
        M, ld = x2.shape
        gy2 = _c(gy).reshape(-1, N)
        tap = ctx.tap
        w_id, b_id, g_id, be_id = ctx.pids
        gpre, dg, dbeta = _layer_norm_bwd_acc(tap, tap.has(g_id) and tap.has(be_id), g_id, be_id, gy2, pre, lnw, lnb, True)
        _, db = _bias_relu_bwd(gpre, None, True, tap, b_id)
        gw = _wgrad(tap, w_id, tap.has(w_id), gpre, x2, ld, 3)              # grad_pre^T [N,M] . bbox[:, :3]
        gb = None
        if ctx.needs_input_grad[0]:
            gb = torch.zeros(M, ld, device=gy.device, dtype=torch.float32)
            gemm(gpre, False, N, _c(w), True, 3, M, 3, N, out=gb, ldc=ld)  # grad_pre . W -> columns 0..2 of the box grad
            gb = gb.reshape(ctx.bshape)
        return gb, gw, db, dg, dbeta, None, tap.token_grad()


# Dropout under graph capture: a captured training step freezes the host seeds of its dropout sites; with a device seed installed
# (train_graph.CapturedTrainStep does it around its warm-up and capture) every dropout launch also adds the int64 word behind this
# tensor, which the owner changes between replays.  None: the host seed alone (eager training, the reference-parity tests).
_DEVICE_SEED = [None]


class device_seed:
    """``with device_seed(t):`` -- dropout launches issued inside hash ``seed + t[0]`` (t: one int64 element on the device, kept alive
    by the autograd nodes that use it)."""

    def __init__(self, t):
        assert t is None or (t.is_cuda and t.dtype == torch.int64 and t.numel() == 1)
        self.t = t

    def __enter__(self):
        self.prev, _DEVICE_SEED[0] = _DEVICE_SEED[0], self.t
        return self.t

    def __exit__(self, *exc):
        _DEVICE_SEED[0] = self.prev
        return False


class SasaCore(torch.autograd.Function):
    """softmax(q k^T / sqrt(d) - dist * tau (+ DN mask)) v on the packed q | k | v | tau rows (attention.hip /
    attention_bwd.hip).  query_bbox only feeds the no-grad distance term (calc_bbox_dists is @torch.no_grad)."""

    @staticmethod
    def forward(ctx, qkvt, query_bbox, mask, pc_range, num_heads, attn_drop, seed):
        B, Q, ld = qkvt.shape
        qkvt = _c(qkvt)
        bbox = _c(query_bbox.detach())
        hd = 32
        Dm = num_heads * hd
        att = torch.empty(B, Q, Dm, device=qkvt.device, dtype=torch.float32)
        pc = _pc6(pc_range)
        lib = _lib.load()
        ds = _DEVICE_SEED[0] if attn_drop > 0.0 else None
        if attn_drop > 0.0:
            st = lib.sbev_sasa_train_fwd_f32_ds(_p(qkvt), ld, _p(bbox), pc, _p(mask), _p(att), B, Q, num_heads, hd, float(attn_drop), int(seed),
                                                _p(ds), _stream())
            _lib.check(st, 'sbev_sasa_train_fwd_f32')
        else:
            _lib.check(lib.sbev_sasa_f32(_p(qkvt), ld, _p(bbox), pc, _p(mask), _p(att), B, Q, num_heads, hd, _stream()), 'sbev_sasa_f32')
        ctx.save_for_backward(qkvt, bbox, mask, att)
        ctx.cfg = (pc_range, num_heads, float(attn_drop), int(seed), ds)
        return att

    @staticmethod
    def backward(ctx, gatt):
        qkvt, bbox, mask, att = ctx.saved_tensors
        pc_range, H, p, seed, ds = ctx.cfg
        B, Q, ld = qkvt.shape
        gq = torch.empty_like(qkvt)
        ws = torch.empty(2 * B * H * Q, device=qkvt.device, dtype=torch.float32)
        pc = _pc6(pc_range)
        st = _lib.load().sbev_sasa_bwd_f32_ds(_p(qkvt), ld, _p(bbox), pc, _p(mask), _p(att), _p(_c(gatt)), _p(gq), _p(ws), B, Q, H, 32,
                                              p, seed, _p(ds), _stream())
        _lib.check(st, 'sbev_sasa_bwd_f32')
        return gq, None, None, None, None, None, None


class AdaptiveMixing(torch.autograd.Function):
    """AdaptiveMixing.inner_forward (models/sparsebev_transformer.py:351-381) as ONE autograd node.

    ``recompute=True`` keeps only the node's inputs and re-runs the generator GEMM and the mixing kernel in backward -- the
    reference's activation-checkpoint policy (:383-387): 29.5 MB instead of 265 MB alive per layer at config 2.
    ``recompute=False`` (the decoder's default on this hardware: 6 layers x 236 MB = 1.4 GB of 288 GB) also keeps the dynamic
    parameters [B*Q, 32768] and the mixed activations [B*Q, 32768] and saves the two re-runs (183 us per layer)."""

    @staticmethod
    def forward(ctx, x, query, pg_w, pg_b, op_w, op_b, out_points, recompute, gemm_f16=False, tap=None, token=None):
        ctx.tap, ctx.pids = tap or _NO_TAP, (id(pg_w), id(pg_b), id(op_w), id(op_b))
        B, Q, G, Pin, C = x.shape
        D = query.shape[-1]
        BQ = B * Q
        ctx.out_points, ctx.recompute = out_points, bool(recompute)
        lib = _lib.load()
        # gemm_f16 (the decoder's default GEMM mode): generator, out-projection and grad_mixed on the fp16 hi + lo kernels --
        # three of the six 15-GFLOP GEMMs of a layer's forward + backward; the two grad_W GEMMs (reduced over the rows) run on
        # gemm_tn_f16s.hip's in-kernel split and grad_params . W_pg on the split-K kernel with a device-side scale: all six
        ctx.f16 = bool(gemm_f16) and not recompute and bool(lib.sbev_linear_bf16s_gen_ok(BQ, pg_w.shape[0], pg_w.shape[1])) and \
            bool(lib.sbev_linear_bf16s_out_ok(BQ, op_w.shape[0], op_w.shape[1])) and bool(lib.sbev_linear_bf16s_gen_ok(BQ, op_w.shape[1], op_w.shape[0]))
        if ctx.f16:
            x = _c(x)
            params, ctx.q_scale = dense.linear_f16s_gen(_c(query).reshape(BQ, D), *_f16_frags(pg_w), pg_b, return_scale=True)
            mixed = torch.empty(BQ, G * out_points * C, device=x.device, dtype=torch.float32)
            _lib.check(lib.sbev_adaptive_mixing_f32(_p(x), _p(params), _p(mixed), BQ, G, Pin, C, out_points, _EPS, _stream()),
                       'sbev_adaptive_mixing_f32')
            y = dense.linear_splitk_f16s(mixed, *_f16_frags(op_w), op_b, residual=_c(query).reshape(BQ, D),
                                         x_up_log2=_mixed_up_log2(out_points * C)).reshape(query.shape)
            ctx.save_for_backward(x, query, pg_w, pg_b, op_w, op_b, params, mixed)
            return y
        if recompute:
            y = dense.adaptive_mixing(x, query, pg_w, pg_b, op_w, op_b, out_points)       # = query + out_proj(mix)
            ctx.save_for_backward(x, query, pg_w, pg_b, op_w, op_b)
            return y
        x = _c(x)
        params = dense.linear(_c(query).reshape(BQ, D), pg_w, pg_b)
        mixed = torch.empty(BQ, G * out_points * C, device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().sbev_adaptive_mixing_f32(_p(x), _p(params), _p(mixed), BQ, G, Pin, C, out_points, _EPS, _stream()),
                   'sbev_adaptive_mixing_f32')
        y = dense.linear(mixed, op_w, op_b, residual=query).reshape(query.shape)
        ctx.save_for_backward(x, query, pg_w, pg_b, op_w, op_b, params, mixed)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.recompute:
            x, query, pg_w, pg_b, op_w, op_b = ctx.saved_tensors
            params = mixed = None
        else:
            x, query, pg_w, pg_b, op_w, op_b, params, mixed = ctx.saved_tensors
        B, Q, G, Pin, C = x.shape
        D = query.shape[-1]
        BQ = B * Q
        lib = _lib.load()
        x = _c(x)
        q2 = _c(query).reshape(BQ, D)
        gy2 = _c(gy).reshape(BQ, D)
        if params is None:        # recompute: dynamic parameters and mixed activations (the two forward launches)
            params = dense.linear(q2, pg_w, pg_b)                                        # [BQ, G*(C*C + Pout*Pin)]
            mixed = torch.empty(BQ, G * ctx.out_points * C, device=x.device, dtype=torch.float32)
            _lib.check(lib.sbev_adaptive_mixing_f32(_p(x), _p(params), _p(mixed), BQ, G, Pin, C, ctx.out_points, _EPS, _stream()),
                       'sbev_adaptive_mixing_f32')
        tap = ctx.tap
        pgw_id, pgb_id, opw_id, opb_id = ctx.pids
        opw_tapped, pgw_tapped = tap.has(opw_id), tap.has(pgw_id)
        # out-projection backward
        _, gb_op = _bias_relu_bwd(gy2, None, True, tap, opb_id)
        NM, NP = mixed.shape[1], params.shape[1]
        # the two big grad_W products (15 GFLOP each) on the fp16 hi + lo kernel: operand scales from what the fp16 forward / backward
        # GEMMs computed anyway (grad_y, query), the LayerNorm bound (mixed) and the mixing backward's per-item maxima (grad_params)
        wg_f16 = ctx.f16 and _WGRAD_F16 and bool(lib.sbev_gemm_tn_f16s_ok(D, NM, BQ)) and bool(lib.sbev_gemm_tn_f16s_ok(NP, D, BQ))
        if ctx.f16:      # grad_mixed = grad_y . W_op: generator-shaped (K = 256 -> 32768 columns) with the fragments of W_op^T
            gmixed, gy_scale = dense.linear_f16s_gen(gy2, *_f16_frags(op_w, transposed=True), None, return_scale=True)
        else:
            gmixed = _linear_grads(gy2, _c(op_w))
        if wg_f16:
            gw_op = _wgrad_tn_f16(tap, opw_id, opw_tapped, gy2, D, gy_scale, mixed, NM, _const_scale(x.device, _mixed_up_log2(ctx.out_points * C)), D, NM, BQ)
        else:
            gw_op = _wgrad(tap, opw_id, opw_tapped, gy2, mixed, NM)
        del mixed
        # mixing core backward
        gx = torch.empty_like(x)
        gparams = torch.empty_like(params)
        if wg_f16:
            item_max = torch.empty(BQ * G * 4, device=x.device, dtype=torch.float32)     # four partial maxima per item
            _lib.check(lib.sbev_adaptive_mixing_bwd_max_f32(_p(x), _p(params), _p(gmixed), _p(gx), _p(gparams), _p(item_max), BQ, G, Pin, C,
                                                            ctx.out_points, _EPS, _stream()), 'sbev_adaptive_mixing_bwd_max_f32')
        else:
            _lib.check(lib.sbev_adaptive_mixing_bwd_f32(_p(x), _p(params), _p(gmixed), _p(gx), _p(gparams), BQ, G, Pin, C, ctx.out_points,
                                                        _EPS, _stream()), 'sbev_adaptive_mixing_bwd_f32')
        del gmixed, params
        # parameter generator backward
        _, gb_pg = _bias_relu_bwd(gparams, None, True, tap, pgb_id)
        if wg_f16:
            gp_scale = dense.f16s_tensor_scale(item_max)
            gw_pg = _wgrad_tn_f16(tap, pgw_id, pgw_tapped, gparams, NP, gp_scale, q2, D, ctx.q_scale, NP, D, BQ)
        else:
            gw_pg = _wgrad(tap, pgw_id, pgw_tapped, gparams, q2, D)
        # grad_query = grad_y (the `query +` residual) + grad_params . W_pg: the forward split-K Linear with W_pg^T, residual fused
        if wg_f16 and _GQ_F16 and bool(lib.sbev_linear_bf16s_out_ok(BQ, D, NP)):       # the same product on the fp16 split-K kernel, scale from the maxima
            gq = dense.linear_splitk_f16s(gparams, *_f16_frags(pg_w, transposed=True), None, residual=gy2, x_scale=gp_scale).reshape(query.shape)
        else:
            gq = dense.linear(gparams, _transposed(pg_w), None, residual=gy2).reshape(query.shape)
        return gx, gq, gw_pg, gb_pg, gw_op, gb_op, None, None, None, None, tap.token_grad()


class FeatureTap(torch.autograd.Function):
    """Where the feature-map gradient of a decoder call is handed to autograd -- ONCE.  The sampler backward of every layer
    accumulates (atomics) into one channels-last buffer per level owned by the pyramid; six per-layer 735 MB gradient tensors
    and their summation never exist.  This node turns the caller's feature tensors into a 1-element token that every
    ``Sampling`` node of the call takes as an input: autograd's own dependency count then runs this node's backward after
    exactly those Sampling backwards that the current backward pass reaches -- a loss on some layers only, a second pass
    under ``retain_graph``, or a pass that reaches none of them all work, with no forward-time counter to go stale
    (ADVICE r2, medium)."""

    @staticmethod
    def forward(ctx, pyramid, *orig_feats):
        ctx.pyramid, ctx.n_feats = pyramid, len(orig_feats)
        return orig_feats[0].new_zeros(1, dtype=torch.float32)

    @staticmethod
    def backward(ctx, gtoken):
        pyr = ctx.pyramid
        if getattr(pyr, '_grads', None) is None:           # no Sampling backward accumulated anything in this pass
            return (None,) + (None,) * ctx.n_feats
        return (None, *pyr.take_feature_grads())


def feature_token(pyramid, orig_feats):
    """The token Sampling nodes take when the caller's feature maps need a gradient (else None)."""
    if not any(torch.is_tensor(f) and f.requires_grad for f in orig_feats):
        return None
    return FeatureTap.apply(pyramid, *orig_feats)


class Sampling(torch.autograd.Function):
    """SparseBEVSampling.inner_forward after its two Linears (models/sparsebev_transformer.py:270-311): sample points,
    velocity warp, level softmax, projection + view selection (sampling_4d front half), multi-scale gather.  Saves only
    (query_bbox, packed offsets | logits); points, locations and weights are recomputed in backward.

    Feature gradients are accumulated by atomics into ONE buffer per level shared by all layers of a decoder call and handed
    to autograd by the call's ``FeatureTap`` node (``feat_token``; None when the features need no gradient)."""

    @staticmethod
    def forward(ctx, query_bbox, both, pyramid, dctx, cfg, feat_token=None):
        T, G, P, L, pc_range = cfg
        n_off = G * P * 3
        bbox = _c(query_bbox)
        both = _c(both)
        offset, logits = both[..., :n_off], both[..., n_off:]
        pts, w_bp = ops.sampling_front(bbox, offset, logits, dctx.time_diff, pc_range, T, G, P, L)
        loc = ops.project_select(pts, dctx.lidar2img, dctx.image_h, dctx.image_w, G, P)
        out = pyramid.sample(loc, w_bp, T, G)
        ctx.save_for_backward(bbox, both)
        ctx.pyramid, ctx.dctx, ctx.cfg = pyramid, dctx, cfg
        ctx.feat_grad = feat_token is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        bbox, both = ctx.saved_tensors
        pyr, dctx = ctx.pyramid, ctx.dctx
        T, G, P, L, pc_range = ctx.cfg
        B, Q = bbox.shape[:2]
        n_off = G * P * 3
        offset, logits = both[..., :n_off], both[..., n_off:]
        pts, w_bp = ops.sampling_front(bbox, offset, logits, dctx.time_diff, pc_range, T, G, P, L)
        loc = ops.project_select(pts, dctx.lidar2img, dctx.image_h, dctx.image_w, G, P)
        gfeat_levels = pyr.grad_buffers() if ctx.feat_grad else None
        gloc, gw = pyr.sample_backward(loc, w_bp, _c(gout), T, G, gfeat_levels)
        lib = _lib.load()
        gpts = torch.empty_like(pts)
        _lib.check(lib.sbev_project_select_bwd(_p(pts), _p(_c(dctx.lidar2img)), _p(gloc), B, Q, T, ops.N_VIEWS, G, P,
                                               float(dctx.image_h), float(dctx.image_w), 1e-5, _p(gpts), _stream()), 'sbev_project_select_bwd')
        gboth = torch.empty(B, Q, both.shape[-1], device=bbox.device, dtype=torch.float32)     # offsets | logits, packed like `both`
        gbbox = torch.empty(B, Q, 10, device=bbox.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        pc = _pc6(pc_range)
        ld = both.shape[-1]
        st = lib.sbev_sampling_front_bwd(_p(bbox), _p(both), ld, ctypes.c_void_p(both.data_ptr() + 4 * n_off), ld, pc, B, Q, T, G, P, L,
                                         _p(gpts), _p(gw), _p(gboth), ctypes.c_void_p(gboth.data_ptr() + 4 * n_off), ld, _p(gbbox), _stream())
        _lib.check(st, 'sbev_sampling_front_bwd')
        # the feature gradient went into the shared buffers; the token's own gradient is a formal zero that orders FeatureTap
        # behind this node
        gtoken = torch.zeros(1, device=bbox.device, dtype=torch.float32) if ctx.feat_grad else None
        return gbbox, gboth, None, None, None, gtoken


class RefineBbox(torch.autograd.Function):
    """refine_bbox + velocity / time_diff (models/sparsebev_transformer.py:155-160,179-183)."""

    @staticmethod
    def forward(ctx, query_bbox, reg, vel_div):
        out = dense.refine_bbox(query_bbox, reg, vel_div)
        ctx.save_for_backward(_c(query_bbox), out, vel_div)
        return out

    @staticmethod
    def backward(ctx, gout):
        bbox, out, vel_div = ctx.saved_tensors
        B, Q, _ = out.shape
        greg = torch.empty_like(out)
        gb = torch.empty_like(out) if ctx.needs_input_grad[0] else None
        st = _lib.load().sbev_refine_bbox_bwd(_p(_c(gout)), _p(out), _p(bbox), _p(vel_div), _p(greg), _p(gb), B, Q, _stream())
        _lib.check(st, 'sbev_refine_bbox_bwd')
        return gb, greg, None


class Dropout(torch.autograd.Function):
    """x * keep / (1 - p) with a counter-based mask (sbev_dropout_f32); the backward re-generates the mask from the seed."""

    @staticmethod
    def forward(ctx, x, p, seed):
        x = _c(x)
        y = torch.empty_like(x)
        ds = _DEVICE_SEED[0]
        _lib.check(_lib.load().sbev_dropout_f32_ds(_p(x), _p(y), x.numel(), int(seed), _p(ds), float(p), _stream()), 'sbev_dropout_f32')
        ctx.cfg = (float(p), int(seed), ds)
        return y

    @staticmethod
    def backward(ctx, gy):
        p, seed, ds = ctx.cfg
        gy = _c(gy)
        gx = torch.empty_like(gy)
        _lib.check(_lib.load().sbev_dropout_f32_ds(_p(gy), _p(gx), gy.numel(), seed, _p(ds), p, _stream()), 'sbev_dropout_f32')
        return gx, None, None


def dropout(x, p, seed):
    return Dropout.apply(x, p, seed) if p > 0.0 else x
