"""On-device generation of the stage 1-2 training pairs (reference: mmsr/data/contras_dataset.py).

The reference makes every sample on the host: a random four-corner homography, ``cv2.warpPerspective``, a float64
``[H, W, 3]`` grid of transformed coordinates and four ``PIL.Image.resize(..., BICUBIC)`` calls.  Here a batch of uint8
RGB crops is uploaded once and ``ContrasPairGenerator`` makes everything ``TeacherContrasModel`` and
``StudentContrasDistillationModel`` read on the GPU (c2m_amd.ops.warp_perspective_u8 / pil_bicubic_resize_u8,
csrc/contras_pairs.hip).  Only the random draws and the 3x3 matrices stay on the host.

The homography draws consume a ``numpy.random.RandomState`` in the reference's order, so a seed gives the reference's
matrices; the four-point perspective transform is solved here as an 8x8 linear system in float64.  The resampling is
Pillow's, bit for bit.  The warp is bilinear on a 1/32-pixel position grid with a constant zero border: parity with
OpenCV unpinned; image and coordinates describe the same map by construction.
"""
import random

import numpy as np
import torch


def _four_point_transform(src, dst):
    """The 3x3 H (H[2,2] = 1) with H.(x, y, 1) ~ (u, v, 1) for the four pairs src[i] = (x, y) -> dst[i] = (u, v)."""
    A = np.zeros((8, 8), dtype=np.float64)
    rhs = np.zeros(8, dtype=np.float64)
    for i in range(4):
        x, y = float(src[i, 0]), float(src[i, 1])
        u, v = float(dst[i, 0]), float(dst[i, 1])
        A[i] = (x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u)
        A[i + 4] = (0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v)
        rhs[i], rhs[i + 4] = u, v
    h = np.linalg.solve(A, rhs)
    return np.append(h, 1.0).reshape(3, 3)


def pair_corners(rng, size=(160, 160), perturb=(0, 10), window=160):
    """The 18 draws of one sample -> (rect1, rect2): float32 [4, 2] corners (x, y) in the order top-left, top-right,
    bottom-right, bottom-left of the window and of its perturbed copy."""
    h, w = size
    x = rng.randint(perturb[1], max(w, w - window - perturb[1]))
    y = rng.randint(perturb[1], max(h, h - window - perturb[1]))
    corners = {"tl": (x, y), "tr": (x + window, y), "bl": (x, y + window), "br": (x + window, y + window)}
    moved = {}
    for name in ("tl", "tr", "bl", "br"):     # the draw order: x then y of each corner
        cx, cy = corners[name]
        mx = cx + rng.randint(perturb[0], perturb[1]) * rng.choice([-1.0, 1.0])
        my = cy + rng.randint(perturb[0], perturb[1]) * rng.choice([-1.0, 1.0])
        moved[name] = (mx, my)
    order = ("tl", "tr", "br", "bl")
    return (np.array([corners[k] for k in order], dtype=np.float32), np.array([moved[k] for k in order], dtype=np.float32))


def sample_pair_homography(rng, size=(160, 160), perturb=(0, 10), window=160):
    """One random pair transform -> (H, H_inverse), float64 [3, 3].  `rng` is a numpy.random.RandomState; `size` is
    (height, width).  H maps the window's corners onto their perturbed positions; H_inverse = inv(H) is what the image
    is warped with and what the transformed coordinates are made from."""
    rect1, rect2 = pair_corners(rng, size, perturb, window)
    H = _four_point_transform(rect1, rect2)
    return H, np.linalg.inv(H)


def validation_pool(n, size=160):
    """The n fixed H_inverse matrices of the validation set: drawn from a private RandomState(0), perturbation (0, 10),
    window 160 -> float64 [n, 3, 3]."""
    rng = np.random.RandomState(0)
    return np.stack([sample_pair_homography(rng, (size, size), (0, 10), 160)[1] for _ in range(n)]) if n else np.zeros((0, 3, 3))


class ContrasPairGenerator:
    """uint8 RGB crops [B,3,H,W] on the GPU -> the dict both contrastive models' ``feed_data`` read.

    Per sample, in this order: horizontal flip / vertical flip / transpose (three ``random() < 0.5`` draws from the
    generator's own ``random.Random``; flips need use_flip / use_rot as in the reference's augment), the homography draws
    (its own ``RandomState``), the warp, then the /scale and xscale-back resampling of both images.
    Keys: img_in, img_in_up, img_ref, img_ref_up (float32 RGB in [0, 1], [B,3,H,W]), img_in_lq, img_ref_lq
    ([B,3,H/scale,W/scale]), transformed_coordinate (float64 [B,H,W,3])."""

    def __init__(self, scale=4, use_flip=True, use_rot=True, perturb=(0, 10), window=160, seed=None):
        self.scale = int(scale)
        self.use_flip, self.use_rot = bool(use_flip), bool(use_rot)
        self.perturb, self.window = tuple(perturb), int(window)
        self.flip_rng = random.Random(seed)
        self.rng = np.random.RandomState(seed)

    def _augment(self, img):
        out = None
        for b in range(img.shape[0]):
            hflip = self.use_flip and self.flip_rng.random() < 0.5
            vflip = self.use_rot and self.flip_rng.random() < 0.5
            rot90 = self.use_rot and self.flip_rng.random() < 0.5
            if not (hflip or vflip or rot90):
                continue
            if rot90 and img.shape[-1] != img.shape[-2]:
                raise ValueError("use_rot transposes samples: the batch must be square")
            s = img[b]
            dims = [d for d, on in ((2, hflip), (1, vflip)) if on]
            if dims:
                s = torch.flip(s, dims)
            if rot90:
                s = s.transpose(1, 2)
            if out is None:
                out = img.clone()
            out[b] = s
        return img if out is None else out

    def __call__(self, img_u8, matrices=None):
        """matrices: optional [B,3,3] H_inverse matrices to warp with instead of drawn ones (no homography draws then)."""
        from c2m_amd import ops
        if not isinstance(img_u8, torch.Tensor) or img_u8.dim() != 4 or img_u8.shape[1] != 3 or img_u8.dtype != torch.uint8:
            raise TypeError("img_u8 must be a uint8 [B,3,H,W] tensor")
        B, _, H, W = img_u8.shape
        if H % self.scale or W % self.scale:
            raise ValueError(f"H and W must be multiples of scale = {self.scale}")
        img = self._augment(img_u8)
        if matrices is None:
            matrices = np.stack([sample_pair_homography(self.rng, (H, W), self.perturb, self.window)[1] for _ in range(B)])
        ref_f32, ref_u8, coords = ops.warp_perspective_u8(img, matrices)
        both = torch.cat([img, ref_u8])                     # input and Ref share the four resampling launches
        lq_u8, lq = ops.pil_bicubic_resize_u8(both, H // self.scale, W // self.scale, as_float=True)
        _, up = ops.pil_bicubic_resize_u8(lq_u8, H, W, as_float=True)
        _, img_f32 = ops.pil_bicubic_resize_u8(img, H, W, as_float=True)   # no resize: the uint8 -> float32 / 255 pass
        return {"img_in": img_f32, "img_in_lq": lq[:B], "img_in_up": up[:B], "img_ref": ref_f32, "img_ref_lq": lq[B:],
                "img_ref_up": up[B:], "transformed_coordinate": coords}
