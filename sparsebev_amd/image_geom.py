"""ImageGeometry: the loader's ``RandomTransformImage`` (loaders/pipelines/transforms.py:218-341) on the device -- decoded camera
frames in, the backbone front end's input and the matching ``lidar2img`` out -- as ONE launch of csrc/image_geom.hip for all B * N
images: uint8 [B * N, H, W, 3] (HWC, as ``mmcv.imread`` returns them, channel order untouched) -> uint8 [B * N, 3, fH, fW], which is what
``ImageFrontEnd.forward`` accepts.  ``front(geom(raw, metas), metas)`` is the detector's whole image path in two launches.

Reference counterpart: per image ``PIL.Image.resize`` (bicubic, antialiased), ``crop`` to ``final_dim`` (black outside), an optional
``FLIP_LEFT_RIGHT``, ``rotate(0)``, and ``lidar2img = ida_mat @ lidar2img``; then the format bundle's HWC -> CHW.  The pixels equal
Pillow's at every byte: its 8-bit resampler is integer arithmetic, restated in the kernel (see csrc/image_geom.hip).

What a call reads:
  * one transform per SAMPLE (the reference draws one ``sample_augmentation()`` per ``__call__``, so all images of a sample share it):
    a block of bounds and integer coefficients written by ``sbev_image_geom_plan`` (a pure host function, double arithmetic in
    Pillow's order), plus an int32 row that maps each image to its block;
  * both live in one device buffer at a fixed address per (device, images, transforms), refreshed through a pinned staging slot and one
    asynchronous copy (``upload``).  A captured launch therefore serves every step: under a capture ``forward`` records the launch
    only, and the caller runs ``geom.upload(geom.draw(B))`` in front of each ``replay()``.
``draw`` consumes random numbers in the reference's order from the same generator (numpy's global state by default).

Not covered: a rotation other than 0 (every config of the reference has ``rot_lim = (0, 0)`` and ``Image.rotate(0)`` is a copy; anything
else raises), a resize that shrinks an axis by more than 3.5 (more than ``KMAX`` = 16 filter taps: refused by the plan, never truncated),
``GlobalRotScaleTransImage``, JPEG decoding.  There is no CPU path: a CPU tensor raises.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib

KMAX = 16               # SBEV_GEOM_KMAX
HEADER_WORDS = 8

GeomParams = namedtuple('GeomParams', ['resize', 'resize_dims', 'crop', 'flip', 'rotate'], defaults=(0,))
GeomParams.__doc__ = """One sample's transform, as ``RandomTransformImage.sample_augmentation`` returns it: ``resize`` (the factor, which
only ``ida_mat`` uses), ``resize_dims`` = (newW, newH), ``crop`` = (x0, y0, x0 + fW, y0 + fH), ``flip``, ``rotate`` (must be 0)."""

Plan = namedtuple('Plan', ['block_bytes', 'workgroups', 'ksize_x', 'ksize_y', 'src_bytes', 'tile_w', 'tile_h', 'src_rows'])


def plan(H, W, fH, fW, resize_dims, crop_xy, flip=False, table=False):
    """sbev_image_geom_plan, a pure host function: the ``Plan`` and, with ``table``, the transform block (int32 numpy array)."""
    out = (ctypes.c_int64 * 8)()
    lib = _lib.load()
    args = (int(H), int(W), int(fH), int(fW), int(resize_dims[0]), int(resize_dims[1]), int(crop_xy[0]), int(crop_xy[1]), int(bool(flip)))
    _lib.check(lib.sbev_image_geom_plan(*args, None, out), 'sbev_image_geom_plan')
    if not table:
        return Plan(*[int(v) for v in out])
    block = np.zeros(int(out[0]) // 4, dtype=np.int32)
    _lib.check(lib.sbev_image_geom_plan(*args, block.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), out), 'sbev_image_geom_plan')
    return Plan(*[int(v) for v in out]), block


def split_block(block, fH, fW):
    """A transform block's parts: (header [8], column bounds [fW, 2], row bounds [fH, 2], column coefficients [fW, KMAX], row
    coefficients [fH, KMAX]) -- views, layout of include/sbev_hip.h."""
    xb = HEADER_WORDS
    yb = xb + 2 * fW
    xk = (yb + 2 * fH + 3) // 4 * 4
    yk = xk + KMAX * fW
    return (block[:HEADER_WORDS], block[xb:yb].reshape(fW, 2), block[yb:yb + 2 * fH].reshape(fH, 2), block[xk:yk].reshape(fW, KMAX),
            block[yk:yk + KMAX * fH].reshape(fH, KMAX))


class ImageGeometry(nn.Module):
    """``ImageGeometry(ida_aug_conf, training=True)`` -- the configs' own dict: ``H``, ``W``, ``final_dim`` = (fH, fW), ``resize_lim``,
    ``bot_pct_lim``, ``rot_lim``, ``rand_flip``.  ``training`` selects the random branch of ``draw`` (``.train()`` / ``.eval()`` switch it
    like any module)."""

    def __init__(self, ida_aug_conf, training=True):
        super().__init__()
        self.ida_aug_conf = dict(ida_aug_conf)
        self.H, self.W = int(ida_aug_conf['H']), int(ida_aug_conf['W'])
        self.fH, self.fW = (int(v) for v in ida_aug_conf['final_dim'])
        if min(self.H, self.W, self.fH, self.fW) < 1:
            raise ValueError('ImageGeometry: H, W and final_dim must be positive')
        self.train(bool(training))
        self.views = 1                  # images per sample of the last forward: upload's default
        self._tables = {}               # (device index, images, transforms) -> int32 buffer at a fixed address

    # ---- the random part
    def draw(self, B, rng=None):
        """One ``GeomParams`` per sample, drawn from ``rng`` (None: numpy's global state, which the reference uses; else a RandomState)
        in the reference's order: uniform(resize_lim), uniform(bot_pct_lim), uniform(0, max(0, newW - fW)), choice([0, 1]) only when
        ``rand_flip``, uniform(rot_lim).  Eval mode draws nothing."""
        R = np.random if rng is None else rng
        conf = self.ida_aug_conf
        H, W, fH, fW = self.H, self.W, self.fH, self.fW
        out = []
        for _ in range(int(B)):
            if self.training:
                resize = R.uniform(*conf['resize_lim'])
                resize_dims = (int(W * resize), int(H * resize))
                newW, newH = resize_dims
                crop_h = int((1 - R.uniform(*conf['bot_pct_lim'])) * newH) - fH
                crop_w = int(R.uniform(0, max(0, newW - fW)))
                crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
                flip = False
                if conf['rand_flip'] and R.choice([0, 1]):
                    flip = True
                rotate = R.uniform(*conf['rot_lim'])
            else:
                resize = max(fH / H, fW / W)
                resize_dims = (int(W * resize), int(H * resize))
                newW, newH = resize_dims
                crop_h = int((1 - np.mean(conf['bot_pct_lim'])) * newH) - fH
                crop_w = int(max(0, newW - fW) / 2)
                crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
                flip = False
                rotate = 0
            if rotate != 0:
                raise NotImplementedError('ImageGeometry: rotation by %r degrees is not built (every config has rot_lim = (0, 0))' % (rotate,))
            out.append(GeomParams(resize, resize_dims, crop, flip, rotate))
        return out

    def _check(self, p):
        if p.rotate != 0:
            raise NotImplementedError('ImageGeometry: rotation by %r degrees is not built (every config has rot_lim = (0, 0))' % (p.rotate,))
        if (p.crop[2] - p.crop[0], p.crop[3] - p.crop[1]) != (self.fW, self.fH):
            raise ValueError('ImageGeometry: crop %s is not final_dim %s' % (tuple(p.crop), (self.fH, self.fW)))

    def ida_mat(self, params):
        """The 4 x 4 fp32 matrix of ``img_transform`` by its float32 steps: scale, minus crop, the mirror A = [[-1, 0], [0, 1]] with
        b = (crop width, 0), and the rotation-by-0 block (which is not skipped: it is part of the rounding)."""
        self._check(params)
        crop = params.crop
        ida_rot = torch.eye(2)
        ida_tran = torch.zeros(2)
        ida_rot *= params.resize
        ida_tran -= torch.Tensor(crop[:2])
        if params.flip:
            A = torch.Tensor([[-1, 0], [0, 1]])
            b = torch.Tensor([crop[2] - crop[0], 0])
            ida_rot = A.matmul(ida_rot)
            ida_tran = A.matmul(ida_tran) + b
        h = params.rotate / 180 * np.pi
        A = torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
        b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
        b = A.matmul(-b) + b
        ida_rot = A.matmul(ida_rot)
        ida_tran = A.matmul(ida_tran) + b
        mat = torch.eye(4)
        mat[:2, :2] = ida_rot
        mat[:2, 2] = ida_tran
        return mat.numpy()

    def update_metas(self, img_metas, params, views=None):
        """What ``RandomTransformImage.__call__`` writes: ``lidar2img[i] = ida_mat @ lidar2img[i]`` for every view of the sample (numpy,
        on the host, the dtypes that expression yields) and img_shape / ori_shape / pad_shape = (fH, fW, 3) per image (``views`` of
        them; None: as many as the sample has ``lidar2img`` matrices)."""
        if len(img_metas) != len(params):
            raise ValueError('ImageGeometry: %d img_metas but %d transforms' % (len(img_metas), len(params)))
        shape = (self.fH, self.fW, 3)
        for meta, p in zip(img_metas, params):
            mat = self.ida_mat(p)
            lidar2img = meta.get('lidar2img', [])
            for i in range(len(lidar2img)):
                lidar2img[i] = mat @ lidar2img[i]
            count = len(lidar2img) if views is None else int(views)
            for key in ('ori_shape', 'img_shape', 'pad_shape'):
                meta[key] = [shape for _ in range(count)]

    # ---- the device table
    def table(self, params, n):
        """The host image of the device buffer for n images of len(params) samples: int32 [round up to 4 of n] image -> block, then the
        blocks.  Raises (SbevError) where the plan refuses a transform."""
        B = len(params)
        if B < 1 or n % B:
            raise ValueError('ImageGeometry: %d images do not divide into %d samples' % (n, B))
        blocks = []
        for p in params:
            self._check(p)
            blocks.append(plan(self.H, self.W, self.fH, self.fW, p.resize_dims, p.crop[:2], p.flip, table=True)[1])
        rows = np.zeros((n + 3) // 4 * 4, dtype=np.int32)
        rows[:n] = np.repeat(np.arange(B, dtype=np.int32), n // B)
        return np.concatenate([rows] + blocks)

    def upload(self, params, device=None, n=None):
        """Refresh the device table of (device, n images, len(params) transforms) from ``params``: one pinned asynchronous copy on the
        current stream.  ``n`` None: len(params) * ``self.views``, the images per sample of the last ``forward`` (1 before the first).
        Never under a capture: it belongs in front of the ``replay()``.  Returns the buffer (int32, fixed address)."""
        if device is not None and torch.device(device).type != 'cuda':
            raise RuntimeError('ImageGeometry needs device tensors (no CPU fallback)')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ImageGeometry.upload while the stream is capturing: the upload belongs in front of the capture / replay')
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        index = torch.cuda.current_device() if device.index is None else device.index
        device = torch.device('cuda', index)
        B = len(params)
        if n is None:
            n = B * self.views
        host = self.table(params, int(n))
        key = (index, int(n), B)
        table = self._tables.get(key)
        if table is None:
            table = self._tables[key] = torch.zeros(len(host), dtype=torch.int32, device=device)
            assert table.data_ptr() % 16 == 0
        from .transformer import _upload
        _upload(host.view(np.uint8), device, out=table.view(torch.uint8))
        return table

    # ---- the call
    def forward(self, img, img_metas, params=None, out=None):
        """img: [B, N, H, W, 3] or [B * N, H, W, 3], uint8, contiguous, on the device.  Returns uint8 [B * N, 3, fH, fW] and writes into
        ``img_metas`` what the reference's transform writes (``update_metas``).  ``params`` None: drawn here (``draw``) -- except under a
        stream capture, where only the launch is recorded, the table is whatever ``upload`` last put there, and ``img_metas`` is left to
        the caller (``update_metas`` with each replay's draw).  ``out``: an existing contiguous uint8 [B * N, 3, fH, fW] tensor."""
        if not isinstance(img, torch.Tensor):
            raise TypeError('ImageGeometry: img must be a tensor')
        if img.dtype != torch.uint8:
            raise TypeError('ImageGeometry: img must be uint8 decoded frames (got %s)' % img.dtype)
        B = len(img_metas)
        if img.dim() == 5:
            if img.shape[0] != B:
                raise ValueError('ImageGeometry: %d samples but %d img_metas' % (img.shape[0], B))
            img = img.reshape(-1, *img.shape[2:]) if img.is_contiguous() else img
        if img.dim() != 4:
            raise ValueError('ImageGeometry: img must be [B, N, H, W, 3] or [B * N, H, W, 3], contiguous')
        if tuple(img.shape[1:]) != (self.H, self.W, 3):
            raise ValueError('ImageGeometry: frames of %s expected (HWC, the conf\'s H and W), got %s' % ((self.H, self.W, 3), tuple(img.shape[1:])))
        if not img.is_contiguous():
            raise ValueError('ImageGeometry: img must be contiguous')
        if not img.is_cuda:
            raise RuntimeError('ImageGeometry needs device tensors (no CPU fallback)')
        n = img.shape[0]
        if B < 1 or n % B:
            raise ValueError('ImageGeometry: %d images do not divide into %d samples' % (n, B))
        index = img.device.index
        capturing = torch.cuda.is_current_stream_capturing()
        with torch.cuda.device(img.device):
            if capturing:
                if params is not None:
                    raise RuntimeError('ImageGeometry.forward under a capture takes no params: upload(params) in front of each replay()')
                table = self._tables.get((index, n, B))
                if table is None:
                    raise RuntimeError('ImageGeometry.forward under a capture before the first upload() for %d images of %d samples' % (n, B))
            else:
                if params is None:
                    params = self.draw(B)
                elif len(params) != B:
                    raise ValueError('ImageGeometry: params for %d samples, %d given' % (B, len(params)))
                table = self.upload(params, img.device, n=n)
                self.update_metas(img_metas, params, views=n // B)
            self.views = n // B
            shape = (n, 3, self.fH, self.fW)
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=img.device)
            elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != img.device or not out.is_contiguous():
                raise ValueError('ImageGeometry: out must be a contiguous uint8 tensor of shape %s on %s' % (shape, img.device))
            rows_bytes = (n + 3) // 4 * 16
            stream = ctypes.c_void_p(torch.cuda.current_stream(img.device).cuda_stream)
            _lib.check(_lib.load().sbev_image_geom(
                ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, self.H, self.W, self.fH, self.fW,
                ctypes.c_void_p(table.data_ptr() + rows_bytes), ctypes.c_void_p(table.data_ptr()), B, stream), 'sbev_image_geom')
        return out
