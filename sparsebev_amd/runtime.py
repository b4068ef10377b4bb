"""Python face of the C++ decoder runtime (csrc/decoder.hip): one ctypes call enqueues the whole 6-layer
forward.  Mirrors include/sbev_hip.h's sbev_decoder_config / sbev_decoder_weights field for field."""
import ctypes
import math
import os
import warnings
import weakref
from collections import namedtuple

import torch

from . import _lib
from .utils import frame_source

MAX_LEVELS = 5
GEMM_F32, GEMM_BF16X3, GEMM_BF16X6, GEMM_BF16X3S, GEMM_F16X3, GEMM_F16X4 = 0, 1, 2, 3, 4, 5      # sbev_gemm_mode
# fp16 modes: how many binades a typical (4 sigma, median |gamma|) generator input may sit below the a-priori scale bound before the
# runtime refuses the split (lo stays a normal fp16 number down to 2^-17 of the bound; 2^-12 leaves 5 binades for the values' own spread)
F16_MAX_HEADROOM_LOG2 = 12
GEMM_MODES = {'f32': GEMM_F32, 'bf16x3': GEMM_BF16X3, 'bf16x6': GEMM_BF16X6, 'bf16x3s': GEMM_BF16X3S, 'f16x3': GEMM_F16X3, 'f16x4': GEMM_F16X4}
_f = ctypes.c_void_p


class DecoderConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('B', 'Q', 'T', 'N', 'G', 'P', 'L', 'D', 'H', 'ffn', 'num_classes',
                                              'code_size', 'num_layers', 'out_points', 'attn_in_rows', 'feat_dtype')] + \
               [('hw', (ctypes.c_int32 * 2) * MAX_LEVELS), ('image_h', ctypes.c_float), ('image_w', ctypes.c_float),
                ('eps_homo', ctypes.c_float), ('gemm_mode', ctypes.c_int32), ('n_slots', ctypes.c_int32),
                ('frame_slots', ctypes.c_int32 * 16), ('overlap', ctypes.c_int32),
                ('pc_range', ctypes.c_double * 6), ('slot_table', ctypes.c_void_p)]


_WEIGHT_FIELDS = ['pe0_w', 'pe0_b', 'pe1_g', 'pe1_b', 'pe3_w', 'pe3_b', 'pe4_g', 'pe4_b',
                  'attn_in_w', 'attn_in_b', 'attn_out_w', 'attn_out_b', 'samp_w', 'samp_b',
                  'pg_w', 'pg_b', 'op_w', 'op_b', 'pg_w2', 'op_w2', 'ffn0_w', 'ffn0_b', 'ffn1_w', 'ffn1_b',
                  'norm1_g', 'norm1_b', 'norm2_g', 'norm2_b', 'norm3_g', 'norm3_b',
                  'cls0_w', 'cls0_b', 'cls1_g', 'cls1_b', 'cls3_w', 'cls3_b', 'cls4_g', 'cls4_b', 'cls6_w', 'cls6_b',
                  'reg0_w', 'reg0_b', 'reg2_w', 'reg2_b', 'reg4_w', 'reg4_b', 'chain_pack', 'pg_ws', 'op_wp', 'pg_wdown', 'op_nscale', 'pg_xscale']


class DecoderWeights(ctypes.Structure):
    _fields_ = [(n, _f) for n in _WEIGHT_FIELDS]


class LazyFeats(ctypes.Structure):
    """sbev_lazy_feats: the NCHW sources of the on-demand relayout (a device pointer table + indices, or direct pointers)"""
    _fields_ = [('table', _f), ('index', ctypes.c_int32 * MAX_LEVELS), ('src', _f * MAX_LEVELS)]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _forward_cached(args, lazy, stream, prefix):
    """sbev_decoder_forward_cached of a prepared step -> status.  ``lazy``: None, or the NCHW sources of the on-demand relayout as (values,
    table): the levels' direct pointers (table None) or their indices into that device pointer table -- the one place that fills a LazyFeats (the
    library takes it right after the feature pointers); ``prefix``: the step's PrefixCache or None"""
    lz = None
    if lazy is not None:
        lz = LazyFeats(table=lazy[1])
        (lz.src if lazy[1] is None else lz.index)[:len(lazy[0])] = lazy[0]
    pfx = (ctypes.c_void_p(prefix.ptr), prefix.nbytes) if prefix is not None else (None, 0)
    return _lib.load().sbev_decoder_forward_cached(*args[:_AFTER_FEATS], ctypes.byref(lz) if lz is not None else None, *args[_AFTER_FEATS:], stream, *pfx)


class PrefixCache:
    """The device block of sbev_decoder_forward_cached (include/sbev_hip.h): layer 0's position encoder + in-projection, self attention
    and generated parameters read the queries and the weights only, and the reference builds the queries from two weight tensors on
    every call (models/sparsebev_head.py:126-127, 217-218) -- so a step whose queries repeat bit for bit skips those three launches and
    reads what the step that stored them left here.  Header words: 0 ``armed``, 1 ``force``, 2 ``hits``, 3 ``misses``.  One per captured
    step (dies with it) and one per DecoderRuntime for the eager path (header zeroed whenever anything but queries and frame changes)."""

    _live = None      # weak set of every cache alive: runtime.prefix_cache() writes their force words

    def __init__(self, nbytes, dev):
        self.nbytes, self.device = nbytes, dev
        self.buf = torch.empty(nbytes + 256, device=dev, dtype=torch.uint8)
        off = (-self.buf.data_ptr()) % 256
        self.ptr = self.buf.data_ptr() + off
        self.hdr = self.buf[off:off + 16].view(torch.int32)
        self.reset()
        if PrefixCache._live is None:
            PrefixCache._live = weakref.WeakSet()
        PrefixCache._live.add(self)

    def reset(self):
        """disarm: the next step recomputes whatever the rest of the block holds (stream-ordered on the current stream)"""
        self.hdr.zero_()
        self.force(_STATE['prefix_off'])

    def force(self, on):
        self.hdr[1:2].fill_(1 if on else 0)

    def counters(self):
        """(hits, misses) since the last reset; synchronises"""
        h = self.hdr.cpu()
        return int(h[2]), int(h[3])


def _prefix_cache_for(cfg, weights, mask, lazy, dev):
    """Bytes of the prefix cache a step of this config would use, or 0: the library's plan says it would not (op-by-op path, exact GEMM
    mode, a mask, launch profiling), or the block is above ``SBEV_PREFIX_CACHE_MAX_MB`` (default 1024)."""
    lib = _lib.load()
    if _STATE['profile'] or lib.sbev_decoder_prefix_planned(ctypes.byref(cfg), ctypes.byref(weights), 1, int(mask is not None), int(bool(lazy))) != 1:
        return 0
    need = int(lib.sbev_prefix_cache_bytes(ctypes.byref(cfg)))
    limit = float(os.environ.get('SBEV_PREFIX_CACHE_MAX_MB', '1024')) * 2 ** 20
    return need if 0 < need <= limit else 0


class DecoderRuntime:
    """Binds a SparseBEVTransformerDecoder's parameters (by pointer) to the C++ runtime and owns the workspace.
    Re-binds automatically when a parameter is replaced or modified in place (``_version`` / ``data_ptr`` change)."""

    def __init__(self, decoder, gemm_mode=0, overlap=False):
        if os.environ.get('SBEV_NO_SAMPLE_MIX') == '1':
            fuse_sample_mix(False)
        if os.environ.get('SBEV_NO_ROW_CHAIN') == '1':
            row_chain(False)
        self.decoder = decoder
        self.gemm_mode = gemm_mode
        self.overlap = overlap
        self._sig = None
        self._keep = None          # tensors whose storage the weight struct points into
        self._weights = None
        self._ws = None
        self._ws_key = None
        self._params = None        # cached parameter SLOTS (module._parameters dict, name); re-collected every 64 signature checks
        self._graph_ws = {}        # (device, size, stream) -> [workspace of the captured step graphs of that size replayed on that stream, graphs using it]
        self._sig_calls = 0
        self.mode_eff = gemm_mode
        self.f16_headroom_log2 = 0.0
        self.step_graphs = StepGraphs(self)
        self._prefix = None        # the eager path's PrefixCache ...
        self._prefix_key = None    # ... and what its contents were computed under (None: disarm before the next use)

    # -- weights -----------------------------------------------------------------------------------------
    def _signature(self):
        """((data_ptr, _version) of every parameter).  Walking the module tree costs ~0.15 ms per call, so the (module._parameters
        dict, name) SLOTS are cached and each call only looks the current Parameter object of every slot up -- a replaced
        Parameter (``load_state_dict(assign=True)``, ``lin.weight = nn.Parameter(...)``, pruning / parametrize) is a different
        object with its own (data_ptr, _version) and re-binds at once; the slot list itself (modules added or removed) is
        re-collected every 64th call."""
        self._sig_calls += 1
        if self._params is None or (self._sig_calls & 63) == 0:
            self._params = [(m._parameters, n) for m in self.decoder.modules() for n, p in m._parameters.items() if p is not None]
        try:
            ps = [d[n] for d, n in self._params]
            return tuple((p.data_ptr(), p._version) for p in ps)
        except (KeyError, AttributeError):          # a slot vanished or became None: re-collect now
            self._params = [(m._parameters, n) for m in self.decoder.modules() for n, p in m._parameters.items() if p is not None]
            return tuple((d[n].data_ptr(), d[n]._version) for d, n in self._params)

    def _ensure_bound(self):
        """(Re-)bind when a parameter was replaced or modified in place; returns the current signature."""
        sig = self._signature()
        if sig != self._sig:
            rebind = self._sig is not None            # (() = invalidated by hand: also a re-bind)
            self._bind()
            self._sig = sig
            if rebind:
                self.step_graphs.clear()    # graphs of the previous weight images can never be hit again: free them now
        return sig

    def _bind(self):
        layer = self.decoder.decoder_layer
        for p in layer.parameters():
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError('sparsebev_amd runtime needs fp32 parameters on the device (call .to("cuda"))')
        pe, sa, smp, mix = layer.position_encoder, layer.self_attn, layer.sampling, layer.mixing
        att = sa.attention.attn
        D = layer.embed_dims
        with torch.no_grad():               # the padded q | k | v | tau rows and the two sampling generators' rows: the layer's one recipe
            attn_in_w, attn_in_b, samp_w, samp_b = layer.packed_train_weights()
        self._attn_in_rows = attn_in_w.shape[0]
        cb, rb, ffn = layer.cls_branch, layer.reg_branch, layer.ffn.layers
        t = dict(
            pe0_w=pe[0].weight, pe0_b=pe[0].bias, pe1_g=pe[1].weight, pe1_b=pe[1].bias,
            pe3_w=pe[3].weight, pe3_b=pe[3].bias, pe4_g=pe[4].weight, pe4_b=pe[4].bias,
            attn_in_w=attn_in_w, attn_in_b=attn_in_b, attn_out_w=att.out_proj.weight, attn_out_b=att.out_proj.bias,
            samp_w=samp_w, samp_b=samp_b,
            pg_w=mix.parameter_generator.weight, pg_b=mix.parameter_generator.bias,
            op_w=mix.out_proj.weight, op_b=mix.out_proj.bias,
            ffn0_w=ffn[0][0].weight, ffn0_b=ffn[0][0].bias, ffn1_w=ffn[1].weight, ffn1_b=ffn[1].bias,
            norm1_g=layer.norm1.weight, norm1_b=layer.norm1.bias, norm2_g=layer.norm2.weight, norm2_b=layer.norm2.bias,
            norm3_g=layer.norm3.weight, norm3_b=layer.norm3.bias,
            cls0_w=cb[0].weight, cls0_b=cb[0].bias, cls1_g=cb[1].weight, cls1_b=cb[1].bias,
            cls3_w=cb[3].weight, cls3_b=cb[3].bias, cls4_g=cb[4].weight, cls4_b=cb[4].bias,
            cls6_w=cb[6].weight, cls6_b=cb[6].bias,
            reg0_w=rb[0].weight, reg0_b=rb[0].bias, reg2_w=rb[2].weight, reg2_b=rb[2].bias,
            reg4_w=rb[4].weight, reg4_b=rb[4].bias)
        keep = {k: v.detach().contiguous() for k, v in t.items()}
        self.mode_eff = self.gemm_mode      # what the launches run in: an fp16 mode falls back to the exact kernels when norm1 is unfit (below)
        if self.gemm_mode in (GEMM_F16X3, GEMM_F16X4):
            # The generator's input is norm1's output; its fp16 scale is fixed per bind from |LayerNorm(x) g + b| <= sqrt(D - 1) max|g| +
            # max|b| (no pass over the activations).  ONE power of two serves the whole tensor, so a channel whose |g| sits far below the
            # largest one lives that many binades under the fp16 range's top: hi stays normal down to 2^-29 of the bound, lo down to 2^-17.
            # A checkpoint with an outlier in norm1 (max|g| or max|b| thousands of times the typical |g|) would push the bulk of the
            # channels below that and quietly lose their lo image: refuse the split then and run the exact f32 kernels.
            g_abs = keep['norm1_g'].abs().float()
            gmax, gmed, bmax = float(g_abs.max()), float(g_abs.median()), float(keep['norm1_b'].abs().max())
            bound = math.sqrt(D - 1) * gmax + bmax
            typical = 4.0 * gmed             # a 4-sigma element of a typical channel
            self.f16_headroom_log2 = math.log2(bound / typical) if (typical > 0 and math.isfinite(bound) and bound > 0) else float('inf')
            if not (self.f16_headroom_log2 <= F16_MAX_HEADROOM_LOG2):
                self.mode_eff = GEMM_F32
                if not getattr(DecoderRuntime, '_warned_f16_bound', False):
                    warnings.warn('sparsebev_amd: norm1 puts typical generator inputs %.1f binades below the a-priori fp16 scale bound '
                                  '(max|gamma| %.3g, median|gamma| %.3g, max|beta| %.3g; limit %d): the two mixing GEMMs run on the exact f32 '
                                  'kernels instead of %s' % (self.f16_headroom_log2, gmax, gmed, bmax, F16_MAX_HEADROOM_LOG2,
                                                              'f16x3' if self.gemm_mode == GEMM_F16X3 else 'f16x4'))
                    DecoderRuntime._warned_f16_bound = True
        if self.gemm_mode == GEMM_BF16X3:      # one-off (hi, lo) bf16 images of the two big weight matrices
            lib = _lib.load()
            for name in ('pg_w', 'op_w'):
                src = keep[name]
                img = torch.empty(src.shape[0], src.shape[1] * 2, device=src.device, dtype=torch.int16)
                _lib.check(lib.sbev_split_bf16x3_weights(_ptr(src), _ptr(img), src.shape[0], src.shape[1],
                                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                           'sbev_split_bf16x3_weights')
                keep[name + '2'] = img
        if self.gemm_mode in (GEMM_BF16X6, GEMM_BF16X3S):      # split-bf16 images for csrc/gemm_bf16s.hip (3 or 2 images)
            from . import dense
            nimg = 3 if self.gemm_mode == GEMM_BF16X6 else 2
            keep['pg_ws'] = dense.pack_bf16s_frags(keep['pg_w'], nimg)
            keep['op_wp'] = dense.pack_bf16s_frags(keep['op_w'], nimg)
        if self.mode_eff in (GEMM_F16X3, GEMM_F16X4):          # scaled fp16 hi + lo images (csrc/gemm_bf16s.hip), one power of two per weight row
            from . import dense
            lib = _lib.load()
            keep['pg_ws'], pg_sc = dense.pack_f16s_frags(keep['pg_w'])
            keep['op_wp'], op_sc = dense.pack_f16s_frags(keep['op_w'])
            keep['pg_wdown'] = pg_sc[1].contiguous()
            c0 = DecoderConfig()
            c0.G, c0.D, c0.out_points = smp.num_groups, D, mix.out_points
            # the generator's input scale: the power of two of the bound computed above, fixed per bind
            e = 0 if not (bound > 0 and math.isfinite(bound)) else max(-100, min(100, math.floor(math.log2(65504.0 / bound) - 1e-9)))
            keep['pg_xscale'] = torch.tensor([2.0 ** e, 2.0 ** -e], device=pg_sc.device, dtype=torch.float32)
            keep['op_nscale'] = torch.empty(D, device=pg_sc.device, dtype=torch.float32)
            _lib.check(lib.sbev_f16s_out_scale(_ptr(op_sc[1].contiguous()), lib.sbev_decoder_mixed_up_log2(ctypes.byref(c0)), _ptr(keep['op_nscale']), D,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sbev_f16s_out_scale')
        w = DecoderWeights()
        for k in _WEIGHT_FIELDS:
            setattr(w, k, keep[k].data_ptr() if k in keep else None)
        # lane-ordered image of the small Linears' weights for the row-chain kernels (csrc/row_chain.hip), where they cover
        # the layer's shape; re-made with every re-bind
        lib = _lib.load()
        cfg = self._config(1, 1)            # (the pack depends on the layer's sizes only, not on the rows of a call)
        n_pack = lib.sbev_decoder_chain_pack_floats(ctypes.byref(cfg))
        if n_pack > 0:
            pack = torch.empty(n_pack, device=attn_in_w.device, dtype=torch.float32)
            st = lib.sbev_decoder_chain_pack(ctypes.byref(cfg), ctypes.byref(w), _ptr(pack),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            if st == 0:
                keep['chain_pack'] = pack
                w.chain_pack = pack.data_ptr()
            elif not getattr(DecoderRuntime, '_warned_chain', False):
                # e.g. a device without 160 KB of LDS per workgroup: the op-by-op launches compute the same layer
                warnings.warn('sparsebev_amd: row-chain weight image unavailable (%s): running the op-by-op launches'
                              % lib.sbev_last_error().decode('utf-8', 'replace'))
                DecoderRuntime._warned_chain = True
        self._keep, self._weights = keep, w
        self._prefix_key = None             # (also a re-bind asked for by hand under an unchanged signature: invalidate_caches)

    def _config(self, B, Q, pyramid=None, ctx=None):
        """The sbev_decoder_config of a [B, Q] call with the bound weights; with ``pyramid`` and ``ctx`` also what a forward reads of
        them (feature dtype and sizes, the frame ring's slots or the frame pool's device table, image size, pc_range)."""
        dec, layer = self.decoder, self.decoder.decoder_layer
        smp = layer.sampling
        cfg = DecoderConfig()
        cfg.B, cfg.Q, cfg.T, cfg.N, cfg.G, cfg.P, cfg.L = B, Q, smp.num_frames, 6, smp.num_groups, smp.num_points, smp.num_levels
        cfg.D, cfg.H, cfg.ffn = layer.embed_dims, layer.self_attn.num_heads, layer.ffn.layers[0][0].weight.shape[0]
        cfg.num_classes, cfg.code_size, cfg.num_layers = layer.num_classes, layer.code_size, dec.num_layers
        cfg.out_points, cfg.attn_in_rows = layer.mixing.out_points, self._attn_in_rows
        cfg.gemm_mode, cfg.overlap = self.mode_eff, int(self.overlap)
        if pyramid is None:
            return cfg
        cfg.feat_dtype = {torch.bfloat16: 1, torch.float16: 2}.get(pyramid.levels[0].dtype, 0)
        src = frame_source(pyramid, (B, cfg.T))
        cfg.n_slots = src.n_slots
        for t, sl in enumerate(src.frame_slots):
            cfg.frame_slots[t] = sl
        if src.kind == 'pool':                    # the kernels read (b, t) -> slot from this device table
            cfg.slot_table = src.slot_table.data_ptr()
        if len(pyramid.levels) != cfg.L or pyramid.T != cfg.T or pyramid.B != B:
            raise RuntimeError('feature pyramid (L=%d, T=%d, B=%d) does not match the decoder config (L=%d, T=%d, B=%d)'
                               % (len(pyramid.levels), pyramid.T, pyramid.B, cfg.L, cfg.T, B))
        for l, f in enumerate(pyramid.levels):
            cfg.hw[l][0], cfg.hw[l][1] = f.shape[1], f.shape[2]
        cfg.image_h, cfg.image_w, cfg.eps_homo = float(ctx.image_h), float(ctx.image_w), 1e-5
        for i, v in enumerate(dec.pc_range):
            cfg.pc_range[i] = float(v)
        return cfg

    def _finished(self, cls, box, stream):
        """(cls, box) nan_to_num'ed into new tensors by one more launch (sbev_finish_outputs)"""
        cls_o, box_o = torch.empty_like(cls), torch.empty_like(box)
        _lib.check(_lib.load().sbev_finish_outputs(_ptr(cls), _ptr(box), _ptr(cls_o), _ptr(box_o), cls.numel(), box.numel(), stream), 'sbev_finish_outputs')
        return cls_o, box_o

    # -- forward -----------------------------------------------------------------------------------------
    def _prepare(self, query_bbox, query_feat, pyramid, ctx, attn_mask, own_workspace=False):
        """(StepArgs, StepKeep, cls, box) on the runtime's workspace; ``own_workspace``: on a graph workspace whose reference the caller
        now holds (``keep.ws_key``)."""
        sig = self._ensure_bound()
        B, Q, D = query_feat.shape
        dev = query_feat.device
        cfg = self._config(B, Q, pyramid, ctx)
        cfg.D = D                           # the queries' own width: the library refuses one that does not fit the layer
        lib = _lib.load()
        need = lib.sbev_decoder_workspace_bytes(ctypes.byref(cfg))
        if need < 0:
            raise _lib.SbevError('sbev_decoder_workspace_bytes: ' + lib.sbev_last_error().decode())
        key = (str(dev), need)
        if own_workspace:                   # captured graphs keep a workspace of their own (eager calls use the runtime's)
            key = key + (torch.cuda.current_stream(dev).cuda_stream,)
            ws = self._take_graph_ws(key, need, dev)
        else:
            if self._ws is None or self._ws_key != key:
                self._ws = torch.zeros(need + 256, device=dev, dtype=torch.uint8)
                self._ws_key = key
            ws = self._ws
        ws_ptr = (ws.data_ptr() + 255) // 256 * 256
        cls = torch.empty(cfg.num_layers, B, Q, cfg.num_classes, device=dev, dtype=torch.float32)
        box = torch.empty(cfg.num_layers, B, Q, cfg.code_size, device=dev, dtype=torch.float32)
        feats = (ctypes.c_void_p * cfg.L)(*[f.data_ptr() for f in pyramid.levels])
        mask = attn_mask.to(device=dev, dtype=torch.uint8).contiguous() if attn_mask is not None else None
        qb, qf = query_bbox.contiguous(), query_feat.contiguous()
        args = StepArgs(ctypes.byref(cfg), ctypes.byref(self._weights), feats, _ptr(qb), _ptr(qf),
                        _ptr(ctx.time_diff), _ptr(ctx.lidar2img), _ptr(ctx.vel_div), _ptr(mask),
                        _ptr(cls), _ptr(box), ctypes.c_void_p(ws_ptr), need)
        return args, StepKeep(cfg, feats, qb, qf, mask, pyramid, ctx, ws, self._keep, key if own_workspace else None), cls, box

    def _take_graph_ws(self, key, need, dev):
        """One more graph on the workspace of its (device, size, stream): ONE per size AND per stream -- graphs replayed on one stream
        run one after the other and may share the pair counters / exchange rows / order buffer carved from it; two streams
        (multi-stream serving) would race on them."""
        slot = self._graph_ws.get(key)
        if slot is None:
            slot = self._graph_ws[key] = [torch.zeros(need + 256, device=dev, dtype=torch.uint8), 0]      # (zeroed once: the on-demand relayout's flag words start clean)
        slot[1] += 1
        return slot[0]

    def _release_graph_ws(self, key):
        """one graph less on its workspace; the last one frees it"""
        slot = self._graph_ws.get(key)
        if slot is not None:
            slot[1] -= 1
            if slot[1] <= 0:
                del self._graph_ws[key]

    def launches_per_layer(self, B, Q):
        """What sbev_decoder_forward would enqueue per layer for a [B, Q] call with the bound weights (asks the library)."""
        self._ensure_bound()
        cfg = self._config(B, Q)
        return int(_lib.load().sbev_decoder_launches_per_layer(ctypes.byref(cfg), ctypes.byref(self._weights)))

    def _eager_prefix(self, cfg, sig, mask, lazy, dev):
        """The eager path's prefix cache for this call, or None.  Its header is zeroed when the weight signature,
        the shapes, the gemm mode, the switches, pc_range, the layer count, the device or the stream are not what its contents were
        computed under, and after a forward that raised."""
        need = _prefix_cache_for(cfg, self._weights, mask, lazy, dev)
        if need == 0:
            return None
        key = (sig, cfg.B, cfg.Q, cfg.D, cfg.T, cfg.P, cfg.G, cfg.out_points, self.mode_eff, _switch_key(), tuple(self.decoder.pc_range),
               cfg.num_layers, str(dev), torch.cuda.current_stream(dev).cuda_stream, need)
        if self._prefix is None or self._prefix.nbytes != need or self._prefix.device != dev:
            self._prefix, self._prefix_key = None, None      # (free the old block first)
            self._prefix = PrefixCache(need, dev)
        elif key != self._prefix_key:
            self._prefix.reset()
        self._prefix_key = key
        return self._prefix

    def _eager(self, query_bbox, query_feat, pyramid, ctx, attn_mask, finish, lazy_from=None):
        """The eager step of ``forward`` and ``forward_lazy`` (after their pair-fault check) -> (cls, box).  ``lazy_from``: the NCHW levels
        that ``pyramid``'s channels-last buffers are filled from on demand, else ``pyramid`` is read as it is."""
        args, keep, cls, box = self._prepare(query_bbox, query_feat, pyramid, ctx, attn_mask)
        lazy = None
        if lazy_from is not None:
            if not _lib.load().sbev_decoder_lazy_supported(args.config):
                raise _lib.SbevError('sbev_decoder_forward_lazy does not cover this pyramid (4 groups x 64 channels; no frame ring)')
            if not all(f.is_cuda and f.is_contiguous() and f.data_ptr() % 16 == 0 and f.dtype == pyramid.levels[l].dtype for l, f in enumerate(lazy_from)):
                raise RuntimeError('forward_lazy needs contiguous, 16-byte aligned device NCHW levels of the buffers\' dtype')
            lazy = ([f.data_ptr() for f in lazy_from], None)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = _forward_cached(args, lazy, stream, self._eager_prefix(keep.cfg, self._sig, attn_mask, lazy is not None, query_feat.device))
        if st != 0:
            self._prefix_key = None      # whatever the failed step left: disarm before the next use
        _lib.check(st, 'sbev_decoder_forward' if lazy is None else 'sbev_decoder_forward_lazy')
        return self._finished(cls, box, stream) if finish else (cls, box)

    def prefix_counters(self):
        """(hits, misses) summed over this runtime's live prefix caches -- the eager one and every captured step's; synchronises"""
        caches = [self._prefix] + [e.prefix for e in self.step_graphs.entries.values() if isinstance(e, CapturedStep)]
        pairs = [c.counters() for c in caches if c is not None]
        return sum(h for h, _ in pairs), sum(m for _, m in pairs)

    def forward(self, query_bbox, query_feat, pyramid, ctx, attn_mask=None, finish=False):
        """pyramid: transformer.FeaturePyramid, cache.RingPyramid or cache.PoolPyramid (told apart by utils.frame_source, which also
        validates the pool's table); ctx: transformer.DecoderContext.  Returns (cls, bbox) stacked over
        layers -- raw, or with ``finish`` nan_to_num'ed by one more launch of this library (sbev_finish_outputs: what
        SparseBEVTransformer.forward applies, models/sparsebev_transformer.py:35-36)."""
        check_pair_faults()                 # an earlier step lost a pair hand-off: raise before anything is enqueued on top of it
        return self._eager(query_bbox, query_feat, pyramid, ctx, attn_mask, finish)

    def lazy_ok(self, mlvl_feats, src=None):
        """whether a feature LIST qualifies for the on-demand relayout of the eager step: the switch is on, every level is a contiguous,
        16-byte aligned NCHW device tensor [B, T*6, 256, H, W] of one dtype (what StepGraphs stages), 4 groups of 64 channels"""
        if not _STATE['lazy'] or (src or frame_source(mlvl_feats)).kind != 'list' or len(mlvl_feats) == 0:
            return False
        f0 = mlvl_feats[0]
        return all(torch.is_tensor(f) and f.is_cuda and StepGraphs._relayout_ok(f) and f.dtype == f0.dtype and f.shape[2] == 256 for f in mlvl_feats) \
            and self.decoder.decoder_layer.sampling.num_groups == 4

    def forward_lazy(self, query_bbox, query_feat, mlvl_feats, ctx, attn_mask=None, buffers=None, finish=False):
        """The eager step on the reference's NCHW feature list ``[B, T*6, 256, H_l, W_l]`` WITHOUT a dense relayout
        (sbev_decoder_forward_lazy): channels-last buffers (``buffers``, or new uninitialised ones) receive only the units the sample
        points read.  Bit-identical to ``forward`` on ``FeaturePyramid(mlvl_feats)``.  Returns (cls, box, pyramid-of-buffers)."""
        from . import transformer as TR
        check_pair_faults()
        pyramid = buffers if buffers is not None else TR.FeaturePyramid.empty_like_nchw(mlvl_feats)
        return (*self._eager(query_bbox, query_feat, pyramid, ctx, attn_mask, finish, lazy_from=mlvl_feats), pyramid)

    def capture(self, query_bbox, query_feat, pyramid, ctx, attn_mask=None):
        """Record one decoder step into a hipGraph (sbev_decoder_capture) and return a DecoderGraph.  The graph reads
        its inputs through the captured pointers: refresh ``query_bbox`` / ``query_feat`` / the pyramid levels /
        ``ctx`` tensors IN PLACE (``.copy_()``), call ``replay()``, read ``graph.cls`` / ``graph.box``.  The runtime's
        workspace belongs to the graph while it is alive: use another DecoderRuntime for un-captured calls."""
        if not (query_bbox.is_contiguous() and query_feat.is_contiguous()):
            raise RuntimeError('capture needs contiguous query tensors (they are read in place on every replay)')
        args, keep, cls, box = self._prepare(query_bbox, query_feat, pyramid, ctx, attn_mask)
        side = torch.cuda.Stream(device=query_feat.device)
        side.wait_stream(torch.cuda.current_stream())
        handle = ctypes.c_void_p()
        st = _lib.load().sbev_decoder_capture(*args, ctypes.c_void_p(side.cuda_stream), ctypes.byref(handle))
        _lib.check(st, 'sbev_decoder_capture')
        return DecoderGraph(handle, keep, cls, box)


# What a captured step is keyed on (see StepGraphs): the queries' shapes, StepGraphs._feat_key (shapes of staged levels; addresses and the
# slot mapping of levels read in place; the shapes of a frame-pool step's new frames, the address of their insert rows, their count per sample and layout), the mask's shape or None, DecoderRuntime._signature() of the bound weights, the device,
# _switch_key(), layer count and box range, the stream (a graph's workspace belongs to the stream it replays on) and ``finish``
StepKey = namedtuple('StepKey', 'bbox feat feats mask weights device switches num_layers pc_range stream finish')
# The tensors of one call whose addresses travel in the step's pointer table (outs: with ``finish`` the call's own (cls, bbox), else None;
# frames: the new frames of a frame-pool step (FrameSource.insert.frames), else None)
StepInputs = namedtuple('StepInputs', 'bbox feat feats mask outs frames', defaults=(None,))
# A prepared step (_prepare).  StepArgs: the leading arguments of sbev_decoder_forward / _capture in include/sbev_hip.h's order (``*args`` is the
# call).  StepKeep: what they point into; ``ws_key``: the key of a graph workspace the caller now holds a reference of (_release_graph_ws), else None
StepArgs = namedtuple('StepArgs', 'config weights feats query_bbox query_feat time_diff lidar2img vel_div mask cls box workspace workspace_bytes')
StepKeep = namedtuple('StepKeep', 'cfg feats query_bbox query_feat mask pyramid ctx workspace weights ws_key')
_AFTER_FEATS = StepArgs._fields.index('feats') + 1


class CapturedStep:
    """One captured step.  ``replays`` counts launches AFTER the capturing call's own; ``pinned``: keyed on addresses of buffers a caller
    may not bring back (the online ring's and the frame pool's buffers are persistent by construction and are not)."""

    def __init__(self, graph, pinned, staged=False, ctx_buf=None, n_packed=0, layout=None, image=None, ws_key=None, prefix=None):
        self.graph, self.pinned, self.staged, self.ctx_buf = graph, pinned, staged, ctx_buf
        self.n_packed, self.layout, self.image, self.ws_key = n_packed, layout, image, ws_key
        self.prefix = prefix       # the step's own PrefixCache (or None): workspaces are shared between steps, this is not
        self.replays = -1


EAGER, SIGHTED, CAPTURE, REPLAY = 'eager', 'sighted', 'capture', 'replay'


class StepBook:
    """StepGraphs' admission policy and bookkeeping, host only (no tensor of its own, no library call; as cache.SlotBook is to
    FramePool): which keys were seen once, which are captured, which graph goes when ``MAX`` are kept, and when a caller that never
    brings its buffers back gets no further address-keyed graph.  Graphs are whatever the entries hold as ``graph`` (``replay()`` /
    ``destroy()``); ``weights()`` is the current weight signature, ``release(step)`` gives a dropped step's workspace back."""

    MAX = 8
    MAX_WASTED = 3
    RETRY_EVERY = 64

    def __init__(self, weights, release):
        self._weights, self._release = weights, release
        self.entries = {}          # StepKey -> CapturedStep or _FirstSighting (seen once, not captured yet), least recently used first
        self.replays = 0
        self.captures = 0
        self.wasted = 0            # address-keyed graphs evicted without a single replay (forgiven by a replay of one, or slowly by time)
        self._refused = 0          # calls refused a capture because of them
        self._warned = False

    def clear(self):
        for e in self.entries.values():
            if isinstance(e, CapturedStep):
                self._destroy(e)
        self.entries.clear()

    def _destroy(self, e):
        e.graph.destroy()
        self._release(e)

    def _drop(self, key):
        e = self.entries.pop(key)
        if isinstance(e, CapturedStep):
            # "captured and never replayed" only counts against the caller when the graph could still have been hit: an entry of a
            # PREVIOUS weight signature (every optimizer step makes one) was orphaned by the weight update, not by the caller
            # bringing new buffers (evaluate-between-optimizer-steps loops switched replay off for good)
            if e.pinned and e.replays == 0 and key.weights == self._weights():
                self.wasted += 1
            self._destroy(e)

    def _never_replayed(self):
        """keys of the live address-keyed graphs of the CURRENT weight signature (as in _drop: ADVICE r5) that were captured and never replayed"""
        sig = self._weights()
        return [k for k, e in self.entries.items() if isinstance(e, CapturedStep) and e.pinned and e.replays == 0 and k.weights == sig]

    def _unproven(self):
        """address-keyed graphs (alive or already evicted) that were captured and never replayed afterwards"""
        return max(self.wasted, 0) + len(self._never_replayed())

    def admit(self, key, ident, pinned):
        """What this call does, and the key's entry: (EAGER, None) -- refused; (SIGHTED, None) -- eager this time, remembered (with
        ``ident``, the tensors an address-keyed entry depends on), captured if it comes again; (CAPTURE, its first sighting);
        (REPLAY, the captured step)."""
        e = self.entries.get(key)
        sighted = isinstance(e, _FirstSighting)
        if e is None or (sighted and not e.same(ident)):       # new (a recycled address of a dead tensor is not "the same input")
            if pinned and self._unproven() >= self.MAX_WASTED:
                self._refuse()
                return EAGER, None
            if e is None and len(self.entries) >= self.MAX:
                self._drop(next(iter(self.entries)))
            self.entries[key] = _FirstSighting(ident)
            return SIGHTED, None
        return (CAPTURE if sighted else REPLAY), e

    def _refuse(self):
        """Not for the life of the runtime: every RETRY_EVERY-th refused call forgives one never-replayed capture, so a caller that
        starts re-using its buffers later gets its graph after all (one probe capture per RETRY_EVERY calls otherwise)."""
        self._refused += 1
        if self._refused % self.RETRY_EVERY == 0:
            if self.wasted > 0:
                self.wasted -= 1
            else:
                stale = next(iter(self._never_replayed()), None)
                if stale is not None:
                    self._drop(stale)         # (counts it as wasted ...)
                    self.wasted = max(self.wasted - 1, 0)      # ... which this probe forgives: net zero, never negative
        if not self._warned:
            warnings.warn('sparsebev_amd: %d step graphs keyed on input addresses were captured and never replayed (the caller '
                          'passes new channels-last / pyramid buffers every call): no further address-keyed graphs; pass fp32 '
                          'NCHW feature lists or reuse the buffers' % self._unproven())
            self._warned = True

    def captured(self, key, step):
        self.entries[key] = step             # (in its first sighting's place)
        self.captures += 1

    def launch(self, key, step):
        self.entries[key] = self.entries.pop(key)            # most recently used last
        step.graph.replay()
        step.replays += 1
        self.replays += 1
        if step.pinned and step.replays > 0:
            self.wasted = 0                  # the caller DOES bring its buffers back: earlier never-replayed captures are forgiven


class StepGraphs(StepBook):
    """hipGraph replay of the whole per-call step: staging of the inputs, feature relayout and all decoder launches are ONE captured
    graph from the second call of a kind on; per call the host packs the per-sample constants (time_diff, lidar2img) and the
    input POINTERS into one small array, refreshes the graph's device copy of it through the pinned upload ring and launches.
    Results are bit-identical to the eager path (same kernels, same order).

    What a graph is keyed on -- round 4: shapes, not addresses.  The reference's loops hand ``model(...)`` freshly allocated
    tensors every step (timing.py:77-96, val.py; mmdet's eval loop: new backbone outputs, new query tensors out of
    ``SparseBEVHead.forward``), so:
      * queries and the attention mask are always STAGED: one in-graph copy launch reads their addresses from the refreshed
        table (sbev_copy_indirect) into buffers the graph owns;
      * fp32 NCHW feature lists (the reference's layout) go through the in-graph relayout, whose source address also comes from
        the table (sbev_nchw_to_nhwc_f32_indirect) -- any tensors of the same shapes replay the same graph, and the graph pins
        none of the caller's tensors;
      * the frame pool's streaming step (cache.FramePool.stream) brings K new frames per sample, NCHW or channels-last, 2-byte ones
        widened: one in-graph launch moves them into their slots (sbev_pool_insert_frames), K * L sources from the table, destinations
        from [K, B] device rows the pool refreshes with its slot table -- one graph per offered shape, whichever tensors the backbone
        hands over: typically one for K = 1 and one for a scene's first window.  FramePool.step is the K = 1 NCHW case and shares that
        graph;
      * inputs that are read IN PLACE by the decoder kernels -- channels-last lists, FeaturePyramid / the online ring's buffers --
        keep their addresses in the key.  A tensor list is only captured when the SAME tensor objects come back (weak
        references from the first sighting: a recycled address of a dead tensor is not "the same input"), and while
        ``MAX_WASTED`` address-keyed graphs stand captured but never replayed no further one is captured (the ring's own
        buffers are persistent by construction and exempt).
    A weight update, other switches, another layer count or box convention miss the cache.  At most ``MAX`` graphs are kept (least
    recently used first out); the graphs of one workspace size replayed on one stream share one workspace (DecoderRuntime._graph_ws),
    freed with the last of them.
    Replaces per-call Python + launch overhead of the reference's eager module chain (models/sparsebev_transformer.py:86-97)."""

    def __init__(self, runtime):
        super().__init__(lambda: runtime._sig, lambda step: runtime._release_graph_ws(step.ws_key))
        self.rt = runtime

    @staticmethod
    def _relayout_ok(f):
        return f.dim() == 5 and f.dtype in (torch.float32, torch.bfloat16, torch.float16) and f.is_contiguous() and f.data_ptr() % 16 == 0 and \
            not f.permute(0, 1, 3, 4, 2).is_contiguous()

    def _feat_key(self, feats, src):
        """(key part, the tensors whose identity an address-keyed entry depends on, staged?)"""
        if src.kind != 'list':              # FeaturePyramid / RingPyramid / PoolPyramid: resident channels-last buffers;
            # their level tensors are views made per call, so there is no object identity to remember: MAX_WASTED bounds a caller
            # that builds a new pyramid over new buffers every step.  The ring's slot order is a by-value kernel argument: its VALUES
            # are part of the key (one graph per ring phase).  The pool's table is device memory the captured step reads on replay:
            # its ADDRESS is, never its contents (one graph per shape).  A pool step's pending insert (FramePool.step / stream) adds a
            # launch to the step: the new frames' shapes and dtype, the ADDRESS of the insert rows, K and the layout -- all the launch
            # depends on; never the frames' addresses (they travel in the pointer table) nor the rows' contents
            table = src.slot_table
            fi = src.insert
            ins = None if fi is None else (tuple((tuple(f.shape), f.dtype) for f in fi.frames), fi.rows.data_ptr(), fi.K, fi.nhwc)
            return ('pyr', tuple((f.data_ptr(), tuple(f.shape), f.dtype) for f in feats.levels), src.frame_slots, src.n_slots,
                    None if table is None else (table.data_ptr(), tuple(table.shape)), ins), [], False
        if all(self._relayout_ok(f) for f in feats):
            return ('nchw', tuple((tuple(f.shape), f.dtype) for f in feats)), [], True
        return ('list', tuple((f.data_ptr(), tuple(f.shape), tuple(f.stride()), f.dtype) for f in feats)), list(feats), False

    def run(self, query_bbox, query_feat, mlvl_feats, attn_mask, img_metas, finish=False, src=None):
        """(cls, box) of the graph's own output buffers (the caller clones or post-processes out of place), or None when this
        call has to take the eager path.  ``finish``: the graph's last node (sbev_finish_outputs_indirect) writes the nan_to_num'ed
        outputs into tensors allocated for THIS call, whose addresses travel in the pointer table -- nothing runs after the replay,
        and what is returned belongs to the caller.  ``src``: the caller's frame_source(mlvl_feats), where it has read it already."""
        rt = self.rt
        if _STATE['profile'] or not (query_bbox.is_cuda and query_bbox.is_contiguous() and query_feat.is_contiguous()):
            return None                      # (bracketing launches with HIP events needs the eager enqueue)
        if query_bbox.data_ptr() % 16 or query_feat.data_ptr() % 16:
            return None
        if attn_mask is not None and not (attn_mask.is_cuda and attn_mask.dtype == torch.uint8 and attn_mask.is_contiguous() and attn_mask.data_ptr() % 16 == 0):
            return None                      # the runtime would convert it into a temporary: nothing stable to stage from
        src = src or frame_source(mlvl_feats)
        if src.kind == 'list' and not all(torch.is_tensor(f) and f.is_cuda for f in mlvl_feats):
            return None
        from . import transformer as TR
        check_pair_faults()                 # (before a capture or replay is built on an invalid step; one host-memory read)
        sig = rt._ensure_bound()
        fkey, ident, staged = self._feat_key(mlvl_feats, src)
        key = StepKey(tuple(query_bbox.shape), tuple(query_feat.shape), fkey, None if attn_mask is None else tuple(attn_mask.shape), sig,
                      torch.cuda.current_device(), _switch_key(), rt.decoder.num_layers, tuple(rt.decoder.pc_range),
                      torch.cuda.current_stream(query_bbox.device).cuda_stream, bool(finish))
        verdict, e = self.admit(key, ident, pinned=not staged and not src.resident)
        if e is None:
            return None
        B, Q = query_bbox.shape[:2]
        packed, layout, ih, iw = consts = TR.DecoderContext.pack(img_metas, B)
        outs = None
        if finish:                           # this call's own output tensors (the graph's last node writes them through the table)
            nl, nc, cs = rt.decoder.num_layers, rt.decoder.decoder_layer.num_classes, rt.decoder.decoder_layer.code_size
            outs = (torch.empty(nl, B, Q, nc, device=query_bbox.device, dtype=torch.float32),
                    torch.empty(nl, B, Q, cs, device=query_bbox.device, dtype=torch.float32))
        call = StepInputs(query_bbox, query_feat, mlvl_feats, attn_mask, outs, None if src.insert is None else src.insert.frames)
        if verdict == CAPTURE:
            e = self._capture(key, call, consts, staged, src)
            if e is None:
                return None
        else:
            if layout != e.layout or (ih, iw) != e.image:
                return None                  # other camera count / image size: not this graph's step
            TR._upload(self._with_table(packed, e.n_packed, e.staged, call), query_bbox.device, out=e.ctx_buf)
        self.launch(key, e)
        return outs if outs is not None else (e.graph.cls, e.graph.box)

    @staticmethod
    def _with_table(packed, n_packed, staged, call):
        """packed per-sample constants + the pointer table of this call (int64 words viewed as fp32 pairs) in ONE upload.
        Table: 0 query_bbox, 1 query_feat, 2 mask, [3 .. 3 + L) the NCHW levels (staged entries) or the new frames of a frame-pool
        step (never both: the pool is read in place; FramePool.stream brings K * L of them, set k's levels at [3 + k * L, 3 + (k + 1) * L)),
        then -- ``finish`` entries -- the call's output tensors cls, bbox.  The table is as long as the call needs: a step's buffer is
        allocated at capture for its own K."""
        import numpy as np
        ptrs = [call.bbox.data_ptr(), call.feat.data_ptr(), call.mask.data_ptr() if call.mask is not None else 0]
        if staged:
            ptrs += [f.data_ptr() for f in call.feats]
        elif call.frames is not None:
            ptrs += [f.data_ptr() for f in call.frames]
        if call.outs is not None:
            ptrs += [call.outs[0].data_ptr(), call.outs[1].data_ptr()]
        full = np.empty(n_packed + 2 * len(ptrs), dtype=np.float32)
        full[:packed.size] = packed
        full[packed.size:n_packed] = 0.0
        full[n_packed:].view(np.int64)[:] = ptrs
        return full

    def _capture(self, key, call, consts, staged, src):
        """Capture this call's step and book it; None: a feature layout neither read in place nor taken by the in-graph relayout
        (eager path).  Any exception between taking the workspace reference and a successful capture gives it back."""
        from . import transformer as TR
        rt, dev = self.rt, call.bbox.device
        packed, layout, ih, iw = consts
        # graph-owned staging buffers of the queries / mask (the decoder kernels read these)
        qb, qf = torch.empty_like(call.bbox), torch.empty_like(call.feat)
        mask = torch.empty_like(call.mask) if call.mask is not None else None
        pyramid = TR.FeaturePyramid.for_graph(call.feats, staged) if src.kind == 'list' else call.feats
        if pyramid is None:
            return None
        insert = None
        if src.insert is not None:           # a frame-pool step: the graph holds the pool's buffers and tables, none of the caller's frames
            pyramid = pyramid.resident()
            insert = (list(range(3, 3 + len(call.frames))), src.insert, pyramid)
        n_packed = (packed.size + 3) // 4 * 4                 # the table behind the constants, 16-byte aligned
        ctx = TR.DecoderContext.from_packed(self._with_table(packed, n_packed, staged, call), layout, ih, iw, dev)     # the graph reads constants AND table from this tensor on every replay
        args, keep, cls, box = rt._prepare(qb, qf, pyramid, ctx, mask, own_workspace=True)
        try:
            segs = [(0, qb), (1, qf)] + ([(2, mask)] if mask is not None else [])
            relayout = [(3 + l, buf) for l, buf in enumerate(pyramid.levels)] if staged else []      # (table index, graph-owned NHWC buffer)
            # the step's own prefix cache, header zeroed here: the replays' watch launch compares the staged queries with its copy
            lazy = len(relayout) > 0 and _STATE['lazy'] and bool(_lib.load().sbev_decoder_lazy_supported(args.config))      # (decided once: _record is told)
            need = _prefix_cache_for(keep.cfg, rt._weights, mask, lazy, dev)
            prefix = PrefixCache(need, dev) if need else None
            handle = self._record(args, ctypes.c_void_p(ctx.buffer.data_ptr() + 4 * n_packed), segs, relayout, lazy,
                                  (cls, box) if call.outs is not None else None, insert, prefix)
        except BaseException:
            rt._release_graph_ws(keep.ws_key)
            raise
        # what the graph's launches read or write: its own buffers, and -- address-keyed entries only -- the caller's feature buffers
        graph = DecoderGraph(handle, (keep, qb, qf, mask, ctx, None if staged else (None if insert else call.feats, pyramid)), cls, box)
        e = CapturedStep(graph, not staged and not src.resident, staged, ctx.buffer, n_packed, layout, (ih, iw), keep.ws_key, prefix)
        self.captured(key, e)
        return e

    @staticmethod
    def _record(args, table, segs, relayout, lazy, finish, insert=None, prefix=None):
        """The step's launches under stream capture -> the instantiated graph's handle: the in-graph copies of ``segs`` (table index,
        graph-owned buffer), the relayout of the staged levels (``lazy``, _capture's decision: on demand inside the step; else all fp32
        levels in one launch, or one launch per level), -- ``insert``: (table indices, the pyramid's pending FrameInsert, pool pyramid) -- the frame pool's new frames
        into their slots (sbev_pool_insert_frames, sources from the table), the decoder step, and -- ``finish``: the graph's (cls, box) -- the
        nan_to_num into the call's own outputs.  All on the one capture stream, in this order.  ``prefix``: the step's PrefixCache or None.
        Raises when any of it fails, with the capture ended."""
        lib = _lib.load()
        side = torch.cuda.Stream(device=segs[0][1].device)
        side.wait_stream(torch.cuda.current_stream())
        sp = ctypes.c_void_p(side.cuda_stream)
        c_idx = (ctypes.c_int32 * len(segs))(*[i for i, _ in segs])
        c_dst = (ctypes.c_void_p * len(segs))(*[t.data_ptr() for _, t in segs])
        c_nb = (ctypes.c_int64 * len(segs))(*[t.numel() * t.element_size() for _, t in segs])
        n = len(relayout)
        n_img, ch = relayout[0][1].shape[::3] if n else (0, 0)      # levels are [B*T*6, H, W, G*C]
        hws = [buf.shape[1] * buf.shape[2] for _, buf in relayout]
        _lib.check(lib.sbev_capture_begin(sp), 'sbev_capture_begin')
        ok, st_fwd = True, 0
        try:
            ok = lib.sbev_copy_indirect(table, len(segs), c_idx, c_dst, c_nb, sp) == 0
            # ``lazy``, the on-demand relayout: no dense pass at all -- every layer moves the units its sample points marked (sbev_decoder_forward_lazy)
            multi = (not lazy and 1 < n <= MAX_LEVELS and ch % 4 == 0 and _STATE['relayout_multi']
                     and all(buf.dtype == torch.float32 and hw % 4 == 0 for (_, buf), hw in zip(relayout, hws)))
            if multi:                        # every fp32 level of the pyramid in ONE launch (the coarse levels ride in the finest one's tail)
                c_ix = (ctypes.c_int32 * n)(*[i for i, _ in relayout])
                c_out = (ctypes.c_void_p * n)(*[buf.data_ptr() for _, buf in relayout])
                ok = ok and lib.sbev_nchw_to_nhwc_f32_multi_indirect(table, n, c_ix, c_out, n_img, ch, (ctypes.c_int32 * n)(*hws), sp) == 0
            elif not lazy:
                for (idx, buf), hw in zip(relayout, hws):
                    fn = lib.sbev_nchw_to_nhwc_f32_indirect if buf.dtype == torch.float32 else lib.sbev_nchw_to_nhwc_b16_indirect
                    ok = ok and fn(table, idx, _ptr(buf), n_img, ch, hw, sp) == 0
            if insert is not None and ok:
                from . import cache
                idx, pending, pool_pyr = insert
                ok = cache.pool_insert_frames(pending.frames, pool_pyr.levels, pending.rows, pool_pyr.n_slots, sp, pending.nhwc, table, idx, check=False) == 0
            st_fwd = _forward_cached(args, ([idx for idx, _ in relayout], table) if lazy else None, sp, prefix) if ok else 0
            ok = ok and st_fwd == 0
            if finish is not None:
                cls, box = finish
                i_out = 3 + (n if insert is None else len(insert[0]))
                ok = ok and lib.sbev_finish_outputs_indirect(table, i_out, i_out + 1, _ptr(cls), _ptr(box), cls.numel(), box.numel(), sp) == 0
        finally:
            handle = ctypes.c_void_p()
            st = lib.sbev_capture_end(sp, ctypes.byref(handle) if ok else None)
        if st_fwd == _lib.EFAULT:            # an EARLIER step lost a pair hand-off: the caller sees PairFaultError (pair mode off, acknowledged), as on the eager path
            _lib.check(st_fwd, 'sbev_decoder_forward (capture)')
        if not ok:
            raise _lib.SbevError('graph capture of the decoder step failed: ' + lib.sbev_last_error().decode())
        _lib.check(st, 'sbev_capture_end')
        torch.cuda.current_stream().wait_stream(side)
        return handle


class _FirstSighting:
    """An input combination seen once.  Address-keyed entries remember WHAT MEMORY the tensors were (weakly): the second sighting only
    counts when the same live storages come back at the same offsets / shapes / strides -- a recycled address of a freed tensor is a
    different input, while a caller that re-creates its views over persistent channels-last buffers every call (``permute`` /
    ``reshape`` per forward: new tensor OBJECTS, same storage) still matches (round 4 compared object identity and left that caller
    eager for good, without a word -- ADVICE r4).  A storage's Python object lives exactly as long as some tensor uses it."""

    def __init__(self, tensors):
        self.refs = [(weakref.ref(t.untyped_storage()), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype) for t in tensors]

    def same(self, tensors):
        return len(tensors) == len(self.refs) and all(
            r[0]() is not None and r[0]() is t.untyped_storage() and r[1:] == (t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)
            for r, t in zip(self.refs, tensors))


class DecoderGraph:
    """An instantiated hipGraph of one decoder step (see DecoderRuntime.capture)."""

    def __init__(self, handle, keep, cls, box):
        self._h, self._keep, self.cls, self.box = handle, keep, cls, box
        self.num_nodes = int(_lib.load().sbev_graph_num_nodes(handle))

    def replay(self):
        if self._h is None:
            raise RuntimeError('DecoderGraph was destroyed')
        st = _lib.load().sbev_graph_launch(self._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(st, 'sbev_graph_launch')
        return self.cls, self.box

    def destroy(self):
        if self._h is not None:
            _lib.load().sbev_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# The process-wide switches live in the LIBRARY (sbev_decoder_switches reports them, however each was set); Python owns only these:
class _State(dict):
    def __missing__(self, key):
        if key != 'order':
            raise KeyError(key)
        return _switch_key()[4]        # until query_order() is called: the library's own start value (SBEV_QUERY_ORDER)


# ('order' is kept for reports only -- query_order() writes it, nothing here decides by it)
_STATE = _State(profile=0,
                prefix_off=os.environ.get('SBEV_NO_PREFIX_CACHE') == '1',        # prefix caches are created with their force word set
                lazy=not os.environ.get('SBEV_NO_SPARSE_RELAYOUT'),      # staged NCHW pyramids: on-demand relayout of the units the sample points read
                relayout_multi=not os.environ.get('SBEV_NO_RELAYOUT_MULTI'))      # staged fp32 NCHW pyramids: all levels in one launch (A/B switch)


def _switch_key():
    """Everything process-wide that changes what a step enqueues: the library's switches as it holds them NOW (sbev_decoder_switches:
    the struct sbev_decoder_forward plans a step from, in include/sbev_hip.h's order) + the two Python-side ones.  A captured step is
    only replayed under the key it was recorded with."""
    buf = (ctypes.c_int32 * 32)()
    n = _lib.load().sbev_decoder_switches(buf, 32)
    assert 0 < n <= 32
    return tuple(buf[:n]) + (bool(_STATE['lazy']), bool(_STATE['relayout_multi']))


def out_fold(enable):
    """The out-projection GEMM folds its split-K slabs inside its launch (the chunk-workgroups of a row tile meet at a counter; fp16 GEMM
    modes, row chains, <= ~1000 rows; follows ``chain_pair``) so that the tail chain reads one row block instead of 32 slabs.  Bit-identical
    results either way.  OFF by default -- at config 2 it costs the out-projection 12.6 us and saves the tail 4;
    ``SBEV_OUT_FOLD=1`` starts with it on.  Returns the previous setting."""
    return bool(_lib.load().sbev_decoder_out_fold(int(bool(enable))))


def prefix_cache(enable):
    """Steps whose queries repeat bit for bit skip layer 0's three query-only launches (PrefixCache; default on, ``SBEV_NO_PREFIX_CACHE=1``
    starts with it off).  Off writes the ``force`` word of every live cache, stream-ordered on the current stream: the same captured
    steps then recompute everything on every replay -- no re-capture, no new key, bit-identical results.  Returns the previous setting."""
    prev = not _STATE['prefix_off']
    _STATE['prefix_off'] = not enable
    for c in list(PrefixCache._live or ()):
        with torch.cuda.device(c.device):
            c.force(not enable)
    return prev


def lazy_relayout(enable):
    """Replayable steps on NCHW feature lists move only the feature units the sample points read (on-demand relayout, default on;
    ``SBEV_NO_SPARSE_RELAYOUT=1`` starts with the dense relayout).  Bit-identical results either way.  Returns the previous setting."""
    prev = _STATE['lazy']
    _STATE['lazy'] = bool(enable)
    return prev


def query_order(enable):
    """The fused gather + mixing launch walks its items in sbev_query_order's order (one group and one arc of the camera ring per
    XCD: 20 % fewer fabric reads at config 2, not faster -- DESIGN_HISTORY.md section 10.8; off by default).  Bit-identical results either
    way.  Returns the previous setting."""
    mode = 2 if enable == 2 and enable is not True else int(bool(enable))      # 2: sorted once per step (from the input boxes) instead of every layer
    prev = int(_lib.load().sbev_decoder_query_order(mode))
    _STATE['order'] = mode
    return prev


def fuse_sample_mix(enable):
    """Gather + adaptive mixing as one launch inside sbev_decoder_forward where the fused kernel covers the shape (default on;
    results are bit-identical either way).  ``SBEV_NO_SAMPLE_MIX=1`` in the environment switches it off for A/B runs."""
    _lib.check(_lib.load().sbev_decoder_fuse_sample_mix(int(bool(enable))), 'sbev_decoder_fuse_sample_mix')


def row_chain(enable):
    """The row-local op chains of a layer (position encoder, attention projections, norms, ffn, branches, refine_bbox) as three
    launches with the rows in LDS instead of one launch per op (default on where the kernels cover the layer's shape; results
    agree to fp32 round-off, not bit for bit).  ``SBEV_NO_ROW_CHAIN=1`` in the environment switches it off for A/B runs."""
    _lib.check(_lib.load().sbev_decoder_row_chain(int(bool(enable))), 'sbev_decoder_row_chain')


def chain_pair(enable):
    """The tail chain on PAIRS of workgroups per row block (half the weight stream per CU, two in-launch hand-offs; default on
    where both members of every pair fit the device in one round: <= ~2000 rows on 256 CUs; results agree with the
    single-workgroup tail to fp32 round-off).  ``SBEV_NO_CHAIN_PAIR=1`` in the environment starts with it off.  Returns the
    previous setting."""
    return bool(_lib.load().sbev_decoder_chain_pair(int(bool(enable))))


def chain_fixed(enable):
    """The row-chain kernels with config 2's unit tables compiled in (csrc/row_chain.hip, "fixed plans"; default on, ``SBEV_CHAIN_FIXED=0``
    starts with them off).  Bit-identical results either way.  Not part of the step-graph key: a captured step keeps the kernels it was
    recorded with.  Returns the previous setting."""
    return bool(_lib.load().sbev_decoder_chain_fixed(int(bool(enable))))


def chain_fixed_launches():
    """Row-chain launches since the library was loaded that took a fixed-plan kernel (a captured launch counts once, at its capture)."""
    return int(_lib.load().sbev_decoder_chain_fixed_launches())


def _on_pair_fault():
    """SBEV_EFAULT came back (``_lib.check``): pair mode off (the library did that already; captured pair-mode steps are keyed on
    the switch and are not hit again) and acknowledge, so that the caller's repeated step runs on the single-workgroup tail."""
    lib = _lib.load()
    lib.sbev_decoder_chain_pair(0)
    lib.sbev_decoder_chain_pair_faults_ack()
    warnings.warn('sparsebev_amd: a pair-mode tail hand-off timed out (GPU shared / preempted?); pair mode is off for the rest of the process')


def check_pair_faults():
    """For callers that synchronise themselves: right AFTER ``torch.cuda.synchronize()`` (or an event / ``.item()`` on the step's
    outputs) this tells whether the step just finished -- or any since the last check -- lost a pair hand-off; raises
    ``_lib.PairFaultError`` (pair mode off, acknowledged) if so.  Costs one read of pinned host memory; never synchronises.  Without
    it a fault surfaces at the NEXT decoder call instead (``sbev_decoder_forward`` / graph replay refuse with SBEV_EFAULT)."""
    n = int(_lib.load().sbev_decoder_chain_pair_faults())
    if n > 0:
        _on_pair_fault()
        raise _lib.PairFaultError('%d pair-mode hand-off(s) timed out since the last check: the step(s) since then hold invalid rows; '
                                  'pair mode is off now, repeat them' % n)


def chain_pair_timeouts():
    """Pair hand-offs whose partner did not arrive within the poll bound since the library was loaded (0 on a GPU of our own;
    synchronises the device)."""
    n = _lib.load().sbev_decoder_chain_pair_timeouts()
    if n < 0:
        raise RuntimeError('sbev_decoder_chain_pair_timeouts: HIP error')
    return int(n)


def profile_sampler(enable):
    """enable: False / True (sampler launches only) or an int mask (1 sampler | 2 generator GEMM | 4 out-projection GEMM |
    8 fused gather + mixing)."""
    _lib.load().sbev_profile_sampler(int(enable))
    _STATE['profile'] = int(enable)


def profile_stride(every_n_calls):
    """Bracket the launches of only every n-th decoder call (the event records themselves cost ~2 % of a step)."""
    _lib.check(_lib.load().sbev_profile_stride(int(every_n_calls)), 'sbev_profile_stride')


def read_kernel_ms(kind, max_n=4096):
    """Elapsed ms of the bracketed launches of one kind (0 sampler, 1 generator GEMM, 2 out-projection GEMM, 3 fused gather +
    mixing)."""
    buf = (ctypes.c_float * max_n)()
    n = _lib.load().sbev_profile_read(kind, buf, max_n)
    return [buf[i] for i in range(n)]


def read_sampler_ms(max_n=4096):
    return read_kernel_ms(0, max_n)
