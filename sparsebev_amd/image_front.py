"""ImageFrontEnd: the detector's own GPU-side image stage -- what SparseBEV.extract_feat does between the loader's batch and the
backbone (models/sparsebev.py:61-100, 48-49) -- as ONE launch of csrc/image_front.hip for all B * N images: uint8 (or fp32) in,
photometric distortion, BGR -> RGB, mean / std, zero pad to a multiple of ``size_divisor``, GridMask, fp32 (or fp16) out.

Reference counterpart: ``data_aug=dict(img_color_aug=True, img_norm_cfg=..., img_pad_cfg=dict(size_divisor=32))`` of the configs with
``GpuPhotoMetricDistortion``, ``pad_multiple`` and ``GridMask(ratio=0.5, prob=0.7)`` of models/utils.py: a few dozen torch passes over
the fp32 image tensor on every training and inference step.

What a call reads:
  * the per-call constants (mean, std, to_rgb, size_divisor, "colour on"): by value in the launch;
  * what is random per step (the five "applied" flags, contrast mode, delta, alpha, saturation, hue, the channel permutation, the mask's
    d / l / st_h / st_w): one 64-byte row per image in a device table at a fixed address per (device, B * N), refreshed through a pinned
    staging slot and one asynchronous copy (``upload``).  A captured launch therefore serves every step: under a capture ``forward``
    records the launch only, and the caller runs ``front.upload(front.draw(...))`` in front of each ``replay()``.
``draw`` consumes random numbers in the reference's order from the same generator (numpy's global state by default), so under
``np.random.seed(s)`` the parameters are the ones the reference would have used.

Not covered: channels-last output; HWC input; ``stop_prev_grad > 0`` (the reference then calls GridMask once per sub-batch -- such
per-sub-call masks fit the per-image table, ``FrontParams.mask`` has one row per image, but ``draw`` does not draw them); the loader's
CPU-side transforms.  There is no CPU path: a CPU tensor raises.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib

ROW_BYTES = 64          # SBEV_FRONT_ROW_BYTES
BRIGHT, CONTRAST, SAT, HUE, SWAP = 1, 2, 4, 8, 16      # FrontParams.flags bits
_U8, _F32, _F16 = 3, 0, 2                               # enum sbev_dtype

# one table row (include/sbev_hip.h: sbev_image_front)
ROW_DTYPE = np.dtype([('flags', '<i4'), ('mode', '<i4'), ('delta', '<f4'), ('alpha', '<f4'), ('sat', '<f4'), ('hue', '<f4'),
                      ('perm', '<i4', (3,)), ('mask', '<i4', (5,)), ('pad', '<i4', (2,))])
assert ROW_DTYPE.itemsize == ROW_BYTES


def plan(n, H, W, div):
    """(Hp, Wp, output elements, table bytes, workgroups): sbev_image_front_plan, a pure host function."""
    out = (ctypes.c_int64 * 5)()
    _lib.check(_lib.load().sbev_image_front_plan(int(n), int(H), int(W), int(div), out), 'sbev_image_front_plan')
    return tuple(int(v) for v in out)


class FrontParams:
    """What is random in one step, as host arrays with one entry per image: ``flags`` (bits BRIGHT, CONTRAST, SAT, HUE, SWAP: the
    transform is applied), ``mode`` (contrast before / after the HSV round trip), ``delta``, ``alpha``, ``sat``, ``hue`` (fp32, as the
    device uses them), ``perm`` [n, 3] and ``mask`` [n, 5] = (applied, d, l, st_h, st_w).  A fresh object applies nothing."""

    def __init__(self, n):
        self.rows = np.zeros(int(n), dtype=ROW_DTYPE)
        self.rows['alpha'] = 1.0
        self.rows['sat'] = 1.0
        self.rows['perm'] = np.arange(3)

    def __getattr__(self, name):
        if name != 'rows' and name in ROW_DTYPE.names:
            return self.rows[name]
        raise AttributeError(name)

    def __len__(self):
        return len(self.rows)

    def table(self):
        """The packed bytes: uint8 [n * 64]."""
        return np.ascontiguousarray(self.rows).view(np.uint8).reshape(-1).copy()


def update_metas(img_metas, B, N, H, W, size_divisor):
    """The meta updates of extract_feat (models/sparsebev.py:88-100) and pad_multiple (models/utils.py:111-116) for [B * N, 3, H, W]
    images; ``size_divisor`` None: no img_pad_cfg.  Returns (Hp, Wp).  Quirks kept: pad_shape is set whenever there is an img_pad_cfg,
    padded or not; pad_multiple counts the views from ``ori_shape``; input_shape is a torch.Size."""
    shape = (H, W, 3)
    for b in range(B):
        img_metas[b]['img_shape'] = [shape for _ in range(N)]
        img_metas[b]['ori_shape'] = [shape for _ in range(N)]
    Hp, Wp = H, W
    if size_divisor is not None:
        d = int(size_divisor)
        Hp, Wp = -(-H // d) * d, -(-W // d) * d
        n_views = len(img_metas[0]['ori_shape'])
        for b in range(len(img_metas)):
            img_metas[b]['img_shape'] = [(Hp, Wp, 3) for _ in range(n_views)]
            img_metas[b]['pad_shape'] = [(Hp, Wp, 3) for _ in range(n_views)]
    input_shape = torch.Size([Hp, Wp])
    for meta in img_metas:
        meta.update(input_shape=input_shape)
    return Hp, Wp


class ImageFrontEnd(nn.Module):
    """``ImageFrontEnd(img_norm_cfg, img_pad_cfg=None, img_color_aug=False, grid_mask=dict(ratio=0.5, prob=0.7), use_grid_mask=True,
    out_dtype=torch.float32)`` -- the reference's ``data_aug`` vocabulary (``from_data_aug`` takes that dict as the configs write it).
    ``img_norm_cfg`` None: no normalisation (mean 0, std 1, no flip).  Colour augmentation and GridMask run in training mode only."""

    brightness_delta = 32
    contrast_range = (0.5, 1.5)
    saturation_range = (0.5, 1.5)
    hue_delta = 18

    def __init__(self, img_norm_cfg, img_pad_cfg=None, img_color_aug=False, grid_mask=None, use_grid_mask=True, out_dtype=torch.float32):
        super().__init__()
        cfg = img_norm_cfg or dict(mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], to_rgb=False)
        mean, std = [float(v) for v in cfg['mean']], [float(v) for v in cfg['std']]
        if len(mean) != 3 or len(std) != 3:
            raise ValueError('ImageFrontEnd: mean and std need three entries')
        if out_dtype not in (torch.float32, torch.float16):
            raise ValueError('ImageFrontEnd: out_dtype is torch.float32 or torch.float16 (got %s)' % out_dtype)
        self.mean, self.std, self.to_rgb = mean, std, bool(cfg.get('to_rgb', False))
        self._mean_c, self._std_c = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        self.size_divisor = None if img_pad_cfg is None else int(img_pad_cfg['size_divisor'])
        self.img_color_aug = bool(img_color_aug)
        grid_mask = dict(ratio=0.5, prob=0.7) if grid_mask is None else grid_mask
        self.ratio, self.prob = float(grid_mask.get('ratio', 0.5)), float(grid_mask.get('prob', 0.7))
        self.use_grid_mask = bool(use_grid_mask)
        self.out_dtype = out_dtype
        self._tables = {}               # (device index, n) -> uint8 [n * 64] at a fixed address

    @classmethod
    def from_data_aug(cls, data_aug, **kw):
        return cls(data_aug.get('img_norm_cfg'), data_aug.get('img_pad_cfg'), data_aug.get('img_color_aug', False), **kw)

    # ---- the random part
    def draw(self, n, Hp, training=None, rng=None):
        """One step's parameters for n images whose PADDED height is Hp, drawn from ``rng`` (None: numpy's global state, which the
        reference uses; else a RandomState) in the reference's order: all contrast modes; per image brightness [+ contrast if mode 0];
        per image saturation, hue; per image [contrast if mode 1 +] swap; then GridMask's rand() -- consumed in eval mode too whenever
        ``use_grid_mask`` -- and only if it passes in training mode d, st_h, st_w."""
        R = np.random if rng is None else rng
        training = self.training if training is None else bool(training)
        p = FrontParams(n)
        if training and self.img_color_aug:
            lo_c, hi_c = self.contrast_range
            lo_s, hi_s = self.saturation_range
            modes = [int(R.randint(2)) for _ in range(n)]
            p.mode[:] = modes
            for i in range(n):
                if R.randint(2):
                    p.delta[i] = R.uniform(-self.brightness_delta, self.brightness_delta)
                    p.flags[i] |= BRIGHT
                if modes[i] == 0 and R.randint(2):
                    p.alpha[i] = R.uniform(lo_c, hi_c)
                    p.flags[i] |= CONTRAST
            for i in range(n):
                if R.randint(2):
                    p.sat[i] = R.uniform(lo_s, hi_s)
                    p.flags[i] |= SAT
                if R.randint(2):
                    p.hue[i] = R.uniform(-self.hue_delta, self.hue_delta)
                    p.flags[i] |= HUE
            for i in range(n):
                if modes[i] == 1 and R.randint(2):
                    p.alpha[i] = R.uniform(lo_c, hi_c)
                    p.flags[i] |= CONTRAST
                if R.randint(2):
                    p.perm[i] = R.permutation(3)
                    p.flags[i] |= SWAP
        if self.use_grid_mask:
            if not (R.rand() > self.prob or not training):
                d = int(R.randint(2, Hp))
                l = min(max(int(d * self.ratio + 0.5), 1), d - 1)
                st_h = int(R.randint(d))
                st_w = int(R.randint(d))
                p.mask[:] = (1, d, l, st_h, st_w)
        return p

    # ---- the device table
    def upload(self, params, device=None):
        """Refresh the device table of (device, len(params)) from ``params``: one pinned asynchronous copy on the current stream.  Never
        under a capture: it belongs in front of the ``replay()``.  Returns the table (uint8, fixed address)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ImageFrontEnd.upload while the stream is capturing: the upload belongs in front of the capture / replay')
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('ImageFrontEnd needs device tensors (no CPU fallback)')
        index = torch.cuda.current_device() if device.index is None else device.index
        device = torch.device('cuda', index)
        key = (index, len(params))
        table = self._tables.get(key)
        if table is None:
            table = self._tables[key] = torch.zeros(len(params) * ROW_BYTES, dtype=torch.uint8, device=device)
            assert table.data_ptr() % 16 == 0
        from .transformer import _upload
        _upload(params.table(), device, out=table)
        return table

    # ---- the call
    def forward(self, img, img_metas, params=None, out=None):
        """img: [B, N, 3, H, W], [B * N, 3, H, W] or a list of [N, 3, H, W] (stacked), uint8 or fp32, contiguous, on the device.
        Returns [B * N, 3, Hp, Wp] in ``out_dtype`` and writes img_shape / ori_shape / pad_shape / input_shape into ``img_metas`` as
        the reference does.  ``params`` None: drawn here (``draw``) -- except under a stream capture, where only the launch is recorded
        and the table is whatever ``upload`` last put there.  ``out``: an existing contiguous [B * N, 3, Hp, Wp] tensor of ``out_dtype`` to
        write into (every element is stored, the padding included)."""
        if isinstance(img, (list, tuple)):
            img = torch.stack(list(img), dim=0)
        if not img.is_cuda:
            raise RuntimeError('ImageFrontEnd needs device tensors (no CPU fallback)')
        B = len(img_metas)
        if img.dim() == 5:
            if img.shape[0] != B:
                raise ValueError('ImageFrontEnd: %d samples but %d img_metas' % (img.shape[0], B))
            N = img.shape[1]
            img = img.reshape(B * N, *img.shape[2:]) if img.is_contiguous() else img
        elif img.dim() == 4:
            if B < 1 or img.shape[0] % B:
                raise ValueError('ImageFrontEnd: %d images do not divide into %d samples' % (img.shape[0], B))
            N = img.shape[0] // B
        else:
            raise ValueError('ImageFrontEnd: img must be [B, N, 3, H, W] or [B * N, 3, H, W]')
        if img.dim() != 4 or not img.is_contiguous():
            raise ValueError('ImageFrontEnd: img must be contiguous')
        if img.shape[1] != 3:
            raise ValueError('ImageFrontEnd: 3 channels expected (got %d)' % img.shape[1])
        if img.dtype not in (torch.uint8, torch.float32):
            raise TypeError('ImageFrontEnd: img must be uint8 or float32 (got %s)' % img.dtype)
        n, _, H, W = img.shape
        Hp, Wp = update_metas(img_metas, B, N, H, W, self.size_divisor)
        colour = self.training and self.img_color_aug
        use_table = colour or (self.training and self.use_grid_mask)
        capturing = torch.cuda.is_current_stream_capturing()
        table = None
        with torch.cuda.device(img.device):
            if capturing:
                if params is not None:
                    raise RuntimeError('ImageFrontEnd.forward under a capture takes no params: upload(params) in front of each replay()')
                if use_table:
                    table = self._tables.get((img.device.index, n))
                    if table is None:
                        raise RuntimeError('ImageFrontEnd.forward under a capture before the first upload() for %d images' % n)
            else:
                if params is None:
                    params = self.draw(n, Hp)
                elif len(params) != n:
                    raise ValueError('ImageFrontEnd: params for %d images, %d given' % (len(params), n))
                if use_table:
                    table = self.upload(params, img.device)
            if out is None:
                out = torch.empty((n, 3, Hp, Wp), dtype=self.out_dtype, device=img.device)
            elif tuple(out.shape) != (n, 3, Hp, Wp) or out.dtype != self.out_dtype or out.device != img.device or not out.is_contiguous():
                raise ValueError('ImageFrontEnd: out must be a contiguous %s tensor of shape %s on %s' % (self.out_dtype, (n, 3, Hp, Wp), img.device))
            stream = ctypes.c_void_p(torch.cuda.current_stream(img.device).cuda_stream)
            _lib.check(_lib.load().sbev_image_front(
                ctypes.c_void_p(img.data_ptr()), _U8 if img.dtype == torch.uint8 else _F32,
                ctypes.c_void_p(out.data_ptr()), _F32 if self.out_dtype == torch.float32 else _F16,
                n, H, W, self.size_divisor or 1, self._mean_c, self._std_c, int(self.to_rgb), int(colour),
                None if table is None else ctypes.c_void_p(table.data_ptr()), stream), 'sbev_image_front')
        return out
