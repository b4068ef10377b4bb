"""The backward kernels at the shapes the reference TRAINS at, against fp64 references on the host: its two trainval configs are
T = 15 frames with P = 4 (vov99) and P = 8 (eva02) points, 5 levels and 1600 queries -- in_points Pin = T * P = 60 / 120 of the
mixing core, up to 1600 keys of the attention.  Every mixing_bwd_kernel<RT, FAST> instantiation, every key-loop shape of the
attention backward (one 256-key step, several, a ragged last one; with and without the DN mask and dropout), AdaptiveMixing at
both trainval shapes, one trained decoder layer at both, and the fp16 grad_W products past their 32-bit buffer offsets.

Each test prints what it measured next to its bound (``pytest -s``)."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from sparsebev_amd import _lib, autograd as AG, synthetic as S
from test_gpu_backward import DEV, PREFIX, rel, build, _keep_mask, _sasa_ref

pytestmark = pytest.mark.gpu
G, C, POUT = 4, 64, 128
MIX_NAMES = ['mixing.parameter_generator.weight', 'mixing.parameter_generator.bias', 'mixing.out_proj.weight', 'mixing.out_proj.bias']


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _mixing_core_ref(x, prm, gy, Pin, near=2e-6):
    """fp64 autograd of the mixing core relu(LN(S . relu(LN(x . M)))) (LayerNorms over the whole item, no affine), and the items
    whose fp64 pre-ReLU LayerNorm outputs (either stage) come within `near` of zero."""
    BQ = x.shape[0]
    xd, pd = x.double().requires_grad_(True), prm.double().requires_grad_(True)
    pv = pd.reshape(BQ, G, -1)
    M = pv[..., :C * C].reshape(BQ, G, C, C)
    Sm = pv[..., C * C:].reshape(BQ, G, POUT, Pin)
    h1 = F.layer_norm(xd @ M, [Pin, C])
    h2 = F.layer_norm(Sm @ torch.relu(h1), [POUT, C])
    torch.relu(h2).backward(gy.double().reshape(BQ, G, POUT, C))
    close = (h1.detach().abs() < near).flatten(2).any(-1) | (h2.detach().abs() < near).flatten(2).any(-1)
    return xd.grad, pd.grad.reshape(BQ, G, -1), close


def _mixing_core_case(Pin, BQ, x_offset=False, chunk=200):
    """Run both C entries on random items (generated on the device) and compare with fp64 in chunks of queries (host memory)."""
    g = torch.Generator(device=DEV).manual_seed(1000 + Pin + BQ + x_offset)
    NP = C * C + POUT * Pin
    x = torch.randn(BQ, G, Pin, C, generator=g, device=DEV)
    prm = torch.randn(BQ, G * NP, generator=g, device=DEV) * 0.3
    # upstream gradients spread over 11 binades from query to query: the per-item maxima see different magnitudes
    gy = torch.randn(BQ, G * POUT * C, generator=g, device=DEV) * torch.exp2(torch.randint(-6, 6, (BQ, 1), generator=g, device=DEV).float())
    if x_offset:      # x at a one-float storage offset: not 16-byte aligned, so Pin = 32 takes the generic <2> instance
        store = torch.empty(x.numel() + 1, device=DEV)
        xd = store[1:].view(x.shape)
        xd.copy_(x)
        assert xd.data_ptr() % 16 != 0
    else:
        xd = x
    lib = _lib.load()
    gx0, gp0 = torch.empty(x.shape, device=DEV), torch.empty_like(prm)
    gx1, gp1 = torch.empty(x.shape, device=DEV), torch.empty_like(prm)
    imax = torch.empty(BQ * G * 4, device=DEV)
    assert lib.sbev_adaptive_mixing_bwd_f32(_p(xd), _p(prm), _p(gy), _p(gx0), _p(gp0), BQ, G, Pin, C, POUT, 1e-5, None) == 0
    assert lib.sbev_adaptive_mixing_bwd_max_f32(_p(xd), _p(prm), _p(gy), _p(gx1), _p(gp1), _p(imax), BQ, G, Pin, C, POUT, 1e-5, None) == 0
    torch.cuda.synchronize()
    # the _max variant runs the same arithmetic and adds the four partial maxima per item that set grad_params' fp16 scale
    assert torch.equal(gx0, gx1) and torch.equal(gp0, gp1)
    assert torch.equal(imax.reshape(BQ * G, 4).amax(dim=1), gp1.reshape(BQ * G, NP).abs().amax(dim=1))
    del gx1, gp1
    parts = {'grad_x': (0, None), 'grad_M': (0, C * C), 'grad_S': (C * C, None)}
    num = dict.fromkeys(parts, 0.0)
    den = dict.fromkeys(parts, 0.0)
    n_close = 0
    for q0 in range(0, BQ, chunk):
        q1 = min(q0 + chunk, BQ)
        rx, rp, close = _mixing_core_ref(x[q0:q1].cpu(), prm[q0:q1].cpu(), gy[q0:q1].cpu(), Pin)
        keep = ~close                                                          # [queries, G]
        n_close += int(close.sum())
        have = {'grad_x': gx0[q0:q1].cpu().double(), 'grad_M': gp0[q0:q1].cpu().double().reshape(q1 - q0, G, NP)}
        have['grad_S'] = have['grad_M']
        want = {'grad_x': rx, 'grad_M': rp, 'grad_S': rp}
        for k, (c0, c1) in parts.items():
            a, b = have[k], want[k]
            if k != 'grad_x':
                a, b = a[..., c0:c1], b[..., c0:c1]
            num[k] = max(num[k], (a[keep] - b[keep]).abs().max().item())
            den[k] = max(den[k], b[keep].abs().max().item())
    return {k: num[k] / den[k] for k in parts}, n_close, BQ * G


@torch.enable_grad()
@pytest.mark.parametrize('Pin', [4, 12, 20, 28, 32, 36, 48, 60, 64, 72, 80, 84, 96, 100, 116, 120])
def test_mixing_core_backward_vs_fp64_every_row_tile_count(Pin):
    """sbev_adaptive_mixing_bwd_f32 dispatches on RT = ceil(Pin / 16): <1> (Pin 4, 12), <2> (20, 28; 32 with unaligned x: the next
    test), <2, FAST> (32), <3> (36, 48), <4> (60, 64), <5> (72, 80), <6> (84, 96), <7> (100), <8> (116, 120; over 64 KiB of LDS) --
    with a partly filled and a full last row tile wherever the instance allows.  grad_x and grad_params (the M and S
    parts) against fp64 autograd, max-abs error over max-abs value per tensor, bound 5e-6 (measured worst 5.9e-7 over all
    instantiations); _bwd_max_f32 bit-identical, its maxima exact.

    Excluded: items (query x group) with a pre-ReLU LayerNorm output within 2e-6 of zero in fp64.  There the fp32 forward that the
    kernel recomputes may take the other ReLU decision (its h carries ~1e-7..1e-6 of rounding); the forward value is continuous
    there but the gradient is not, and the whole item moves through the LayerNorm statistics -- a flipped decision, not a kernel
    error.  With ~N(0, 1) LayerNorm outputs that is ~3e-6 of the Pin*64 + 128*64 elements per item: a few percent of the items."""
    e, n_close, n = _mixing_core_case(Pin, 37)
    print('mixing bwd Pin=%d: %s  excluded %d of %d items' % (Pin, ' '.join('%s %.2e' % kv for kv in e.items()), n_close, n))
    assert n_close <= 0.08 * n
    assert max(e.values()) < 5e-6, e


@torch.enable_grad()
def test_mixing_core_backward_generic_two_tile_instance_at_32_points():
    """Pin = 32 with x NOT 16-byte aligned (a one-float storage offset) is the only way to the generic <2> instance (the FAST one
    needs aligned x; the SBEV_MIX_BWD_GENERIC switch is read once per process).  Its x loads are scalar, so the offset is legal."""
    e, n_close, n = _mixing_core_case(32, 37, x_offset=True)
    print('mixing bwd Pin=32 generic: %s  excluded %d of %d items' % (' '.join('%s %.2e' % kv for kv in e.items()), n_close, n))
    assert n_close <= 0.08 * n
    assert max(e.values()) < 5e-6, e


@torch.enable_grad()
def test_mixing_core_backward_vs_fp64_at_1600_queries_and_120_points():
    """The eva02 trainval mixing core at full size: B*Q = 1600 queries x 4 groups at Pin = 120 (<8>, 6 400 workgroups).  Items whose
    fp64 pre-ReLU LayerNorm outputs come within 2e-6 of zero are excluded, as above (a flipped ReLU decision is not a kernel error);
    their count is reported and must stay small."""
    e, n_close, n = _mixing_core_case(120, 1600)
    print('mixing bwd Pin=120 BQ=1600: %s  excluded %d of %d items' % (' '.join('%s %.2e' % kv for kv in e.items()), n_close, n))
    assert n_close <= 0.08 * n
    assert max(e.values()) < 5e-6, e


def _dn_mask(Q):
    """The query-denoising attention mask (True = masked): the first Q // 3 queries form denoising groups that see their own group and
    the matching queries; the matching queries do not see them.  Every row keeps at least its own group or the matching part."""
    n_dn = Q // 3
    gs = max(2, n_dn // 4)
    m = torch.zeros(Q, Q, dtype=torch.bool)
    m[n_dn:, :n_dn] = True
    for s0 in range(0, n_dn, gs):
        s1 = min(s0 + gs, n_dn)
        m[s0:s1, :s0] = True
        m[s0:s1, s1:n_dn] = True
    assert not m.all(dim=1).any()
    return m


@torch.enable_grad()
@pytest.mark.parametrize('Q,use_mask,p', [(1, False, 0.0), (31, False, 0.0), (33, True, 0.0), (255, False, 0.1), (256, True, 0.0),
                                          (257, False, 0.0), (257, True, 0.1), (400, True, 0.0), (400, False, 0.1), (900, False, 0.0),
                                          (900, True, 0.1), (1600, False, 0.0), (1600, True, 0.1)])
def test_sasa_core_backward_vs_fp64_over_the_key_loop(Q, use_mask, p):
    """autograd.SasaCore against the fp64 dense restatement: a workgroup takes 32 query rows and walks the keys 256 at a time, so
    Q <= 256 is one step (Q = 1, 31, 33: partly filled query tiles), 257 / 400 / 900 / 1600 several with a ragged last step (1600 =
    6 x 256 + 64), 256 exactly one full step.  With the DN mask and with dropout (sbev_sasa_train_fwd_f32 then writes the output):
    the output and grad_qkvt, tau columns included (they carry the largest error: a sum over every key).  Bounds 1e-5 (measured
    worst 8.6e-7 on the output, 1.2e-6 on the gradient at Q = 1600; test_sasa_core_function_vs_fp64 allows 2e-5 / 5e-5)."""
    B, H = (2 if Q <= 400 else 1), 8
    D = H * 32
    g = torch.Generator().manual_seed(5000 + Q)
    qkvt = torch.randn(B, Q, 3 * D + H, generator=g) * 0.7
    qkvt[..., 3 * D:] = torch.rand(B, Q, H, generator=g) * 0.2
    bbox = torch.rand(B, Q, 10, generator=g)
    mask = _dn_mask(Q) if use_mask else None
    gy = torch.randn(B, Q, D, generator=g)
    seed = 123456789 + Q
    keep = _keep_mask(seed, p, (B, H, Q, Q)) if p > 0 else None
    qd = qkvt.to(DEV).requires_grad_(True)
    md = mask.to(DEV).to(torch.uint8) if use_mask else None
    y = AG.SasaCore.apply(qd, bbox.to(DEV), md, tuple(S.PC_RANGE), H, p, seed)
    y.backward(gy.to(DEV))
    qc = qkvt.double().requires_grad_(True)
    yc = _sasa_ref(qc, bbox, mask, H, keep, p)
    yc.backward(gy.double())
    e_y, e_g, e_tau = rel(y, yc), rel(qd.grad, qc.grad), rel(qd.grad[..., 3 * D:], qc.grad[..., 3 * D:])
    print('sasa bwd Q=%d B=%d mask=%d p=%.1f: out %.2e  grad_qkvt %.2e  grad_tau %.2e' % (Q, B, use_mask, p, e_y, e_g, e_tau))
    assert e_y < 1e-5 and e_g < 1e-5 and e_tau < 1e-5
    if Q > 1:
        assert qc.grad[..., 3 * D:].abs().max() > 0                    # tau really receives a gradient
    if p > 0:
        assert abs(1 - keep.float().mean().item() - p) < 0.02


@torch.enable_grad()
@pytest.mark.parametrize('T,P,recompute', [(15, 4, False), (15, 4, True), (15, 8, False), (15, 8, True)])
def test_adaptive_mixing_function_at_the_trainval_points_vs_oracle_autograd(T, P, recompute):
    """autograd.AdaptiveMixing at in_points 60 (vov99) and 120 (eva02), both activation policies, against the oracle's adaptive_mixing
    under fp64 autograd.  Bounds 2e-6 on the output and 1e-5 on every gradient (measured worst 2.3e-7 / 7.0e-7; the same node at
    Pin 8 / 32 is held to 2e-5 / 1e-4 by test_adaptive_mixing_function_vs_oracle_autograd)."""
    from oracle import sparsebev_oracle as O
    g = torch.Generator().manual_seed(T * 100 + P)
    B, Q = 1, 20
    params = S.make_params(31, embed_dims=256, num_frames=T, num_points=P, num_levels=5)
    x = torch.randn(B, Q, G, T * P, C, generator=g)
    query = torch.randn(B, Q, 256, generator=g)
    gy = torch.randn(B, Q, 256, generator=g)
    dv = [t.to(DEV).requires_grad_(True) for t in [x, query] + [params[n] for n in MIX_NAMES]]
    y = AG.AdaptiveMixing.apply(*dv, 128, recompute)
    y.backward(gy.to(DEV))
    pc = {n: params[n].double().requires_grad_(True) for n in MIX_NAMES}
    xc, qc = x.double().requires_grad_(True), query.double().requires_grad_(True)
    yc = O.adaptive_mixing(pc, xc, qc)
    yc.backward(gy.double())
    errs = [rel(d.grad, c.grad) for d, c in zip(dv, [xc, qc] + [pc[n] for n in MIX_NAMES])]
    print('AdaptiveMixing Pin=%d recompute=%d: out %.2e  grads %s' % (T * P, recompute, rel(y, yc), ' '.join('%.2e' % v for v in errs)))
    assert rel(y, yc) < 2e-6
    assert max(errs) < 1e-5, errs


def _f16_vs_exact(B, Q, T, P, mags, seed):
    """AdaptiveMixing with gemm_f16=True against the same node on the exact kernels (no tap): the metrics of
    test_adaptive_mixing_fp16_gemms_full_size_without_a_tap_match_the_exact_path, evaluated on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=P, num_levels=5)
    x = torch.randn(B, Q, G, T * P, C, generator=g, device=DEV)
    query = torch.randn(B, Q, 256, generator=g, device=DEV)
    report = []
    for mag in mags:
        gy = torch.randn(B, Q, 256, generator=g, device=DEV) * mag
        grads = []
        for f16 in (False, True):
            dv = [x.clone().requires_grad_(True), query.clone().requires_grad_(True)] + [params[n].to(DEV).requires_grad_(True) for n in MIX_NAMES]
            y = AG.AdaptiveMixing.apply(*dv, 128, False, f16)
            y.backward(gy)
            grads.append([y.detach()] + [d.grad for d in dv])
            del dv, y
        for k, (a, b) in enumerate(zip(*grads)):
            assert torch.isfinite(b).all()
            if k == 0:
                e = ((b.double() - a.double()).abs().max() / a.double().abs().max()).item()
                report.append(('out', e))
                assert e < 2e-5, (mag, e)
                continue
            # a handful of the mixing core's ReLU decisions flip between the two forwards (last-bit differences) and move their block
            # through its LayerNorm statistics: norm-wise agreement, and all but a small fraction element-wise (grad_x only)
            d = (b.double() - a.double()).abs()
            l2 = (d.pow(2).sum() / a.double().pow(2).sum()).sqrt().item()
            off = (d > 2e-5 * a.abs().max().double()).double().mean().item()
            report.append((k, l2, off))
            assert l2 < 2e-3 and (k != 1 or off < 1e-2), (mag, k, a.shape, l2, off)
        del grads
    return report


@torch.enable_grad()
def test_adaptive_mixing_fp16_gemms_at_eva02_full_size_match_the_exact_path():
    """gemm_f16=True at the eva02 trainval shape, B = 1 x 1600 queries, P = 8, T = 15 (Pin 120: NP = 77 824 generated parameters per
    query; the grad_W products take the fp16 kernel, B*Q * NP = 1.2e8 < 2^29), against the exact path, also with a tiny gradient."""
    lib = _lib.load()
    assert lib.sbev_gemm_tn_f16s_ok(G * (C * C + POUT * 120), 256, 1600) == 1
    rep = _f16_vs_exact(1, 1600, 15, 8, (1.0, 1e-9), 78)
    print('AdaptiveMixing f16 vs exact B=1 Q=1600 Pin=120:', rep)


@torch.enable_grad()
def test_adaptive_mixing_fp16_gemms_past_32bit_offsets_fall_back_to_the_exact_products():
    """B = 8 x 900 queries at P = 8, T = 15: grad_W_pg = grad_params^T . query has K * M = 7200 * 77 824 = 5.6e8 >= 2^29, past the
    32-bit buffer offsets of sbev_gemm_tn_f16s.  sbev_gemm_tn_f16s_ok must refuse it so that the backward falls back to the exact
    kernels (it used to accept it and the launch then raised in the middle of backward); the result matches the exact path."""
    lib = _lib.load()
    NP = G * (C * C + POUT * 120)
    assert 8 * 900 * NP >= 1 << 29 and lib.sbev_gemm_tn_f16s_ok(NP, 256, 8 * 900) == 0
    rep = _f16_vs_exact(8, 900, 15, 8, (1.0,), 79)
    print('AdaptiveMixing f16 vs exact B=8 Q=900 Pin=120:', rep)


def _relu_inputs_recorded(fn):
    """Run fn() with torch.relu recording its inputs (the oracle's ReLU sites, in call order)."""
    seen, relu = [], torch.relu

    def rec(t):
        seen.append(t.detach())
        return relu(t)
    torch.relu = rec
    try:
        out = fn()
    finally:
        torch.relu = relu
    return out, seen


class TrainedLayer:
    """One decoder layer in train() mode (dropouts at 0), forward + backward on the device and under fp64 autograd in the oracle, for
    cotangents (cc, cb) on (cls, box): ``device`` / ``oracle`` return (cls, box, [(name, gradient)]) over query_feat, the 48 parameters
    and the feature maps, in the same order.  The oracle's forward is evaluated once (``pre``: its ReLU inputs, in call order)."""

    def __init__(self, B, Q, T, pyr, P, mode, use_mask, seed, metas=None, num_classes=10, pc_range=S.PC_RANGE):
        from oracle import sparsebev_oracle as O
        self.O, self.B, self.Q, self.T, self.P, self.mode, self.use_mask = O, B, Q, T, P, mode, use_mask
        self.num_classes, self.pc_range = num_classes, pc_range
        ih, iw, sizes = S.PYRAMIDS[pyr]
        self.L = L = len(sizes)
        self.params = S.make_params(seed, embed_dims=256, num_frames=T, num_points=P, num_levels=L, num_classes=num_classes)
        self.model = model = build(T, L, seed, 1, num_points=P, num_classes=num_classes, pc_range=pc_range).train()
        model.decoder.decoder_layer.self_attn.attn_drop = 0.0
        model.decoder.decoder_layer.ffn_drop = 0.0
        model.decoder.gemm_mode = mode
        self.feats = S.make_features(B, T, sizes, seed=seed + 1)
        self.bbox, self.feat = S.make_queries(B, Q, seed=seed + 2)
        self.metas = S.make_img_metas(B, T, ih, iw) if metas is None else metas
        self.mask = _dn_mask(Q) if use_mask else None
        self.md = self.mask.to(DEV) if use_mask else None
        g = torch.Generator().manual_seed(seed + 3)
        self.cc, self.cb = torch.randn(1, B, Q, num_classes, generator=g), torch.randn(1, B, Q, 10, generator=g)
        self._oracle = None

    def camera_choices_differing(self):
        """the camera choices of the device's sample points vs the oracle's (fp32: the projection is bit-exact with the device's)"""
        import os
        import tempfile
        from sparsebev_amd.utils import DUMP
        taps = []
        with tempfile.TemporaryDirectory() as tmp:
            DUMP.enabled, DUMP.out_dir = True, tmp
            try:
                with torch.no_grad():
                    self.model.eval()(self.bbox.to(DEV), self.feat.to(DEV), [f.to(DEV) for f in self.feats], self.md, copy.deepcopy(self.metas))
            finally:
                DUMP.enabled = False
                self.model.train()
            valid = torch.load(os.path.join(tmp, 'sample_points_cam_valid_mask_stage0.pth'))
        with torch.no_grad():
            self.O.decoder(self.params, self.bbox, self.feat, self.feats, self.metas, self.pc_range, num_layers=1, num_points=self.P,
                           pre_attn_mask=self.mask, taps=taps)
        return (valid.cpu() != taps[0]['valid']).sum(dim=(1, 2, 3, 4)).tolist()           # per sample

    def device(self, cc, cb):
        model = self.model
        model.zero_grad(set_to_none=True)
        fd = self.feat.to(DEV).requires_grad_(True)
        fsd = [f.to(DEV).requires_grad_(True) for f in self.feats]
        cls, box = model(self.bbox.to(DEV), fd, list(fsd), self.md, copy.deepcopy(self.metas))
        ((cls * cc.to(DEV)).sum() + (box * cb.to(DEV)).sum()).backward()
        grads = [('query_feat', fd.grad)] + [(k_[len(PREFIX):], p.grad) for k_, p in model.named_parameters()]
        grads += [('feat%d' % i, a.grad) for i, a in enumerate(fsd)]
        return cls, box, [(k_, None if g_ is None else g_.detach().clone()) for k_, g_ in grads]

    def oracle(self, cc, cb):
        if self._oracle is None:
            fo = self.feat.double().requires_grad_(True)
            fso = [f.double().requires_grad_(True) for f in self.feats]
            po = {k_: v_.double().requires_grad_(True) for k_, v_ in self.params.items()}
            (c2, b2, _), self.pre = _relu_inputs_recorded(
                lambda: self.O.decoder(po, self.bbox.double(), fo, fso, self.metas, self.pc_range, num_layers=1, num_points=self.P,
                                       pre_attn_mask=self.mask))
            names = ['query_feat'] + [k_[len(PREFIX):] for k_, _ in self.model.named_parameters()] + ['feat%d' % i for i in range(self.L)]
            leaves = [fo] + [po[k_] for k_ in names[1:1 + len(po)]] + fso
            self._oracle = (c2, b2, names, leaves)
        c2, b2, names, leaves = self._oracle
        grads = torch.autograd.grad((c2 * cc.double()).sum() + (b2 * cb.double()).sum(), leaves, retain_graph=True, allow_unused=True)
        return c2, b2, list(zip(names, grads))


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _one_layer_trained_vs_oracle(case, label):
    """The recipe of test_one_layer_trained_at_the_trainval_shapes_vs_oracle_autograd (its docstring gives the reasons and the measured
    figures) on a TrainedLayer: camera-hit masks equal first; then the outputs and the tensors with no mixing / camera decision between
    them and the loss (norm3, both branches) to 1e-5, every tensor norm-wise to 5e-3, max-abs median 5e-3 and worst 5e-2 -- and, when no
    mixing ReLU input lies within fp32 reach of zero, every tensor to 1e-4.  Returns the number of such ReLU inputs."""
    n_cam = case.camera_choices_differing()
    assert sum(n_cam) == 0, 'camera choices differ, per sample: %s' % n_cam
    cls, box, got = case.device(case.cc, case.cb)
    c2, b2, want = case.oracle(case.cc, case.cb)
    assert len(case.pre) == 9                   # position encoder 2, mixing 2, FFN 1, cls branch 2, reg branch 2
    mix_near = sum(int(((t != 0) & (t.abs() < 1e-5)).sum()) for t in case.pre[2:4])
    out_err = max(rel(cls, c2), rel(box, b2))
    pairs = [(k_, a, b) for (k_, a), (k2, b) in zip(got, want)]
    assert [k_ for k_, _ in got] == [k_ for k_, _ in want]
    assert len(pairs) == 1 + 48 + case.L and all(a is not None and b is not None for _, a, b in pairs)
    l2 = {k_: rel_l2(a, b) for k_, a, b in pairs}
    mx = {k_: rel(a, b) for k_, a, b in pairs}
    down = {k_: v_ for k_, v_ in mx.items() if 'cls_branch' in k_ or 'reg_branch' in k_ or 'norm3' in k_}
    vals = sorted(mx.values())
    report = sorted(((k_, l2[k_], mx[k_]) for k_ in l2), key=lambda t: -t[1])[:4]
    print('train layer %s T=%d P=%d %s mask=%d: mixing ReLU inputs 0 < |h| < 1e-5: %d; out %.2e  downstream %.2e  worst l2 %.2e  '
          'median max-abs %.2e  worst max-abs %.2e  %s' % (label, case.T, case.P, case.mode, case.use_mask, mix_near, out_err, max(down.values()),
                                                           max(l2.values()), vals[len(vals) // 2], vals[-1], report))
    if mix_near == 0:
        assert vals[-1] < 1e-4 and out_err < 1e-4, report
    assert out_err < 1e-5 and max(down.values()) < 1e-5, report
    assert max(l2.values()) < 5e-3, report
    assert vals[len(vals) // 2] < 5e-3 and vals[-1] < 5e-2, report
    return mix_near


@torch.enable_grad()
@pytest.mark.parametrize('P,mode,use_mask', [(4, 'f16x3', False), (4, 'f32', True), (8, 'f16x3', True), (8, 'f32', False)])
def test_one_layer_trained_at_the_trainval_shapes_vs_oracle_autograd(P, mode, use_mask):
    """One decoder layer in train() mode (dropouts at 0) at the reference's two trainval shapes -- T = 15 frames, P = 4 (vov99) and
    P = 8 (eva02), 5 levels -- at B = 2 x 49 queries on a small 5-level pyramid, forward + backward in the default GEMM mode (f16x3)
    and the exact one (f32), with the DN mask in one variant of each shape, against the oracle's decoder under torch autograd in
    FP64 on the CPU: outputs, grad_query_feat, all 48 parameter gradients and the feature-map gradients.

    The gradient is discontinuous wherever the forward takes a decision, and the device's forward is fp32.  (1) The camera choice of
    the 23 520 / 47 040 sample points: the hit masks of the HIP path's DUMP tap equal the oracle's for these inputs (asserted).
    (2) The ReLUs of the mixing core: 392 items x (Pin * 64 + 128 * 64) = 4.7 M / 6.2 M decisions on ~N(0, 1) LayerNorm outputs, of
    which some dozens lie within fp32 reach of zero (0 < |h| < 1e-5 in fp64: counted below; items whose every sample point misses
    have h = 0 exactly and take the same decision everywhere).  A flipped decision moves its (query, group) item's grad_params
    through the LayerNorm statistics, and the generator weight's gradient sums only 98 query rows, so its max-abs error is ~1e-2;
    grad_x carries it on to the feature maps.  The oracle shows this itself: its fp32 evaluation at P = 4, seed 640 takes 7 mixing
    ReLU decisions differently from its fp64 one, all at |h| <= 1.3e-6, with no other decision different, and is 6.5e-2 (max-abs)
    from it on a feature-map gradient.  Hence, when such decisions exist (37..53 of them in these four cases), as in
    test_full_size_c2_one_layer_backward_vs_oracle_autograd: the outputs and the tensors with no mixing / camera decision between
    them and the loss (norm3, both branches) to 1e-5 (measured worst 1.4e-6), every tensor NORM-wise to 5e-3 (measured worst 9.8e-4),
    max-abs median tensor 5e-3 (measured 5.0e-4) and worst 5e-2 (measured 1.4e-2, the generator weight); when none exist, every
    tensor to G11's 1e-4."""
    seed = 600 + 10 * P + use_mask
    _one_layer_trained_vs_oracle(TrainedLayer(2, 49, 15, 'tiny5', P, mode, use_mask, seed), 'trainval')
