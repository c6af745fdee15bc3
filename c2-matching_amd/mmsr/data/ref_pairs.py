"""On-device generation of the stage-3 batches (reference: mmsr/data/ref_cufed_dataset.py).

The reference makes every sample on the host: the Ref is resized to the GT size (CUFED's refs differ in size), GT and Ref
are flipped / transposed together, and each is resized down by `scale` and back up, five ``PIL.Image.resize(...,
BICUBIC)`` calls per sample.  Here decoded uint8 RGB images are uploaded once and ``RefPairGenerator`` makes the dict
``RefRestorationModel.feed_data`` reads on the GPU (c2m_amd.ops.pil_bicubic_resize2d_u8, csrc/ref_pairs.hip: both
resampling passes in one launch, the orientation applied on read).  Only the random draws stay on the host.  Resampling
is per plane, so the reference's BGR <-> RGB round trips around Pillow drop out; the numbers are Pillow's, bit for bit.

Reading image files or LMDBs is not part of this: the caller decodes and uploads.
"""
import random

import torch

KEYS = ("img_in", "img_in_lq", "img_in_up", "img_ref", "img_ref_lq", "img_ref_up")


def draw_flags(rng, n, use_flip=True, use_rot=True):
    """The reference's augment draws for n samples -> list of flag bytes (bit 0 hflip, bit 1 vflip, bit 2 transpose).
    Per sample, in this order: hflip (drawn only with use_flip), vflip, transpose (drawn only with use_rot), each
    ``rng.random() < 0.5``."""
    flags = []
    for _ in range(n):
        h = use_flip and rng.random() < 0.5
        v = use_rot and rng.random() < 0.5
        t = use_rot and rng.random() < 0.5
        flags.append(int(h) | int(v) << 1 | int(t) << 2)
    return flags


def val_geometry(in_hw, ref_hw, scale):
    """Validation sizes -> (cropped in (h, w), cropped ref (h, w), padded (h, w), padding): both images are cut to
    multiples of scale; if the results differ in size both are zero-padded at the bottom / right to the larger height and
    the larger width."""
    crop = lambda hw: (hw[0] - hw[0] % scale, hw[1] - hw[1] % scale)   # noqa: E731
    cin, cref = crop(in_hw), crop(ref_hw)
    if min(cin + cref) <= 0:
        raise ValueError(f"images of {tuple(in_hw)} / {tuple(ref_hw)} are smaller than scale = {scale}")
    padded = (max(cin[0], cref[0]), max(cin[1], cref[1]))
    return cin, cref, padded, cin != cref


def _check_u8(t, dims, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != dims or t.shape[-3] != 3:
        raise TypeError(f"{name} must be a uint8 {'[B,3,H,W]' if dims == 4 else '[3,H,W]'} tensor")
    return t


class RefPairGenerator:
    """uint8 RGB images on the GPU -> the dict ``RefRestorationModel.feed_data`` (and its validation loop) read.

    phase='train': ``gen(img_in, img_ref)`` with img_in uint8 [B,3,gt_size,gt_size] and img_ref uint8 [B,3,Hr,Wr] or a list
    of B uint8 [3,Hr_b,Wr_b] tensors.  Each Ref is resized to gt_size x gt_size, then GT and Ref of a sample take the same
    flip / transpose (``draw_flags`` from the generator's own ``random.Random(seed)``), then both go down by `scale` and
    back up.  -> img_in, img_ref, img_in_up, img_ref_up [B,3,gt,gt] and img_in_lq, img_ref_lq [B,3,gt/scale,gt/scale],
    float32 RGB in [0, 1].

    phase='val': ``gen(img_in, img_ref)`` with one pair, uint8 [3,H,W] and [3,Hr,Wr] of any sizes (``val_geometry``).  The
    same six keys with a leading batch dimension of 1 (img_in is the cropped, UNPADDED GT; everything else has the padded
    size or its 1/scale), plus padding (bool) and original_size = (height, width) of the cropped GT.

    Nothing here waits for the device: the flag bytes of a batch are the only host -> device traffic."""

    def __init__(self, phase="train", gt_size=160, scale=4, use_flip=True, use_rot=True, seed=None):
        if phase not in ("train", "val"):
            raise ValueError("phase must be 'train' or 'val'")
        self.phase, self.gt_size, self.scale = phase, int(gt_size), int(scale)
        if self.scale <= 0 or (phase == "train" and (self.gt_size <= 0 or self.gt_size % self.scale)):
            raise ValueError(f"gt_size = {gt_size} must be a positive multiple of scale = {scale}")
        self.use_flip, self.use_rot = bool(use_flip), bool(use_rot)
        self.flip_rng = random.Random(seed)

    def __call__(self, img_in, img_ref):
        return self._train(img_in, img_ref) if self.phase == "train" else self._val(img_in, img_ref)

    def _down_up(self, both, flags):
        """both uint8 [2B,3,H,W] (inputs, then refs) -> the six images; flags one per image or None."""
        from c2m_amd import ops
        H, W = both.shape[-2:]
        lq_u8, lq, full = ops.pil_bicubic_resize2d_u8(both, H // self.scale, W // self.scale, flags=flags, as_float=True,
                                                      oriented_float=True)
        _, up = ops.pil_bicubic_resize2d_u8(lq_u8, H, W, as_float=True)
        B = both.shape[0] // 2
        return {"img_in": full[:B], "img_in_lq": lq[:B], "img_in_up": up[:B], "img_ref": full[B:], "img_ref_lq": lq[B:],
                "img_ref_up": up[B:]}

    def _train(self, img_in, img_ref):
        from c2m_amd import ops
        gt = self.gt_size
        img_in = _check_u8(img_in, 4, "img_in")
        B = img_in.shape[0]
        if tuple(img_in.shape[-2:]) != (gt, gt) or B == 0:
            raise ValueError(f"img_in must be [B,3,{gt},{gt}], got {tuple(img_in.shape)}")
        if isinstance(img_ref, torch.Tensor):
            refs = [_check_u8(img_ref, 4, "img_ref")]
            n_ref = img_ref.shape[0]
        else:
            refs = [_check_u8(r, 3, "img_ref[b]") for r in img_ref]
            n_ref = len(refs)
        if n_ref != B:
            raise ValueError(f"{B} inputs but {n_ref} refs")
        flags = draw_flags(self.flip_rng, B, self.use_flip, self.use_rot)
        # the Ref at the GT's size (one launch per list entry: their sizes differ), inputs and refs in one tensor
        refs = [r if tuple(r.shape[-2:]) == (gt, gt) else ops.pil_bicubic_resize2d_u8(r, gt, gt) for r in refs]
        both = torch.cat([img_in, refs[0]]) if len(refs) == 1 and refs[0].dim() == 4 else torch.cat([img_in, torch.stack(refs)])
        return self._down_up(both, flags + flags)

    def _val(self, img_in, img_ref):
        s = self.scale
        img_in, img_ref = _check_u8(img_in, 3, "img_in"), _check_u8(img_ref, 3, "img_ref")
        (h, w), (hr, wr), (hp, wp), padding = val_geometry(img_in.shape[-2:], img_ref.shape[-2:], s)
        both = torch.zeros((2, 3, hp, wp), dtype=torch.uint8, device=img_in.device) if padding else \
            torch.empty((2, 3, hp, wp), dtype=torch.uint8, device=img_in.device)
        both[0, :, :h, :w] = img_in[:, :h, :w]
        both[1, :, :hr, :wr] = img_ref[:, :hr, :wr]
        out = self._down_up(both, None)
        if padding:
            out["img_in"] = out["img_in"][..., :h, :w].contiguous()
        out["padding"] = padding
        out["original_size"] = (h, w)
        return out
