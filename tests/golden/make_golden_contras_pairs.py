#!/usr/bin/env python3
"""Generates tests/golden/contras_pairs_pillow.npz: Pillow's own bicubic resizes of seeded uint8 images, the expected
outputs for the on-device resampler of the stage 1-2 pair generator (csrc/contras_pairs.hip).

    python tests/golden/make_golden_contras_pairs.py

Per case (an RGB image [3, H, W] from `image(name)`): `<name>/lq` = resize to (H/4, W/4) and `<name>/up` = that resized
back to (H, W), each channel as an 8-bit PIL image with Image.BICUBIC; case c50 also stores `c50/odd` = 50x30 -> 17x11.
The inputs are not stored: the tests rebuild them from the seeds below.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"c52": dict(shape=(3, 52, 36), seed=8101), "c50": dict(shape=(3, 50, 30), seed=8102),
         "c160": dict(shape=(3, 160, 160), seed=8103)}
ODD = {"c50": (17, 11)}      # one non-integer ratio
OUT = os.path.join(HERE, "contras_pairs_pillow.npz")


def image(name, index=0):
    """uint8 [3, H, W]; index > 0 gives further images of the same shape (the batches of the GPU tests)."""
    c = CASES[name]
    return np.random.RandomState(c["seed"] + 1000 * index).randint(0, 256, size=c["shape"]).astype(np.uint8)


def pillow_resize(img, out_h, out_w):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(ch).resize((out_w, out_h), Image.BICUBIC)) for ch in img])


def expected():
    out = {}
    for name, c in CASES.items():
        img = image(name)
        H, W = c["shape"][1:]
        lq = pillow_resize(img, H // 4, W // 4)
        out[f"{name}/lq"] = lq
        out[f"{name}/up"] = pillow_resize(lq, H, W)
        if name in ODD:
            out[f"{name}/odd"] = pillow_resize(img, *ODD[name])
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **expected())
    print(OUT, os.path.getsize(OUT), "bytes")
