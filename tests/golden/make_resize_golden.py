"""Record tests/golden/resize_pillow.npz: random uint8 images and what Pillow's
`Image.resize((w, h), Image.BILINEAR)` makes of them, the bytes `ResizeCrop.reference` is
defined to give (tests/test_resize_host.py).  Needs Pillow; run from the repository root:

    python tests/golden/make_resize_golden.py
"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (in h, in w, out h, out w, channels)
CASES = [
    (37, 53, 64, 64, 3),
    (7, 5, 3, 2, 3),
    (1, 1, 4, 4, 3),
    (60, 80, 24, 32, 3),
    (48, 64, 3, 4, 3),    # factor 16
    (33, 47, 33, 47, 3),  # identity
    (40, 30, 20, 30, 3),  # one axis only
    (37, 53, 64, 64, 1),  # single channel (mode "L")
    (60, 80, 24, 32, 1),
]


def pillow_resize(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    pil = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
    out = np.asarray(pil.resize((ow, oh), Image.BILINEAR))
    return out.reshape(oh, ow, img.shape[2])


def main():
    rng = np.random.default_rng(2024)
    arrays = {"pillow_version": np.array(PIL.__version__), "cases": np.array(CASES, dtype=np.int32)}
    for i, (h, w, oh, ow, c) in enumerate(CASES):
        img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
        arrays[f"in{i}"] = img
        arrays[f"out{i}"] = pillow_resize(img, oh, ow)
    path = os.path.join(HERE, "resize_pillow.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
