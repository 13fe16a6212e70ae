#!/usr/bin/env python
"""Writes tests/golden/png_adaptive.png and png_adaptive.npy: a 100 x 104 RGB
image encoded by PIL (libpng chooses a filter per row adaptively) and its
pixels.  The image is banded so that the heuristic picks different filters:
flat rows, horizontal and vertical gradients, diagonal structure, noise.
tests/test_png_cases_cpu.py checks that the file's filter bytes show at least
three types with Paeth and Up among them.

    python tests/golden/make_golden_png.py
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def picture():
    h, w = 100, 104
    rng = np.random.default_rng(20)
    y, x = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3), dtype=np.int64)
    img[0:12] = (40, 90, 200)                                   # flat
    img[12:30] = np.stack([2 * x, 255 - 2 * x, x], 2)[12:30]    # along the row
    img[30:48] = np.stack([5 * y, 3 * y, 255 - 2 * y], 2)[30:48]  # down
    diag = (3 * x + 5 * y)
    img[48:68] = np.stack([diag, diag + 40, 2 * diag], 2)[48:68]
    img[68:84] = rng.integers(0, 256, (16, w, 3))               # noise
    smooth = (128 + 100 * np.sin(x / 9.0) * np.cos(y / 5.0)).astype(np.int64)
    img[84:] = np.stack([smooth, smooth // 2, 255 - smooth], 2)[84:]
    img[84:] += rng.integers(0, 3, (h - 84, w, 3))
    return (img & 255).astype(np.uint8)


def main():
    img = picture()
    Image.fromarray(img, "RGB").save(os.path.join(HERE, "png_adaptive.png"),
                                     optimize=False, compress_level=6)
    np.save(os.path.join(HERE, "png_adaptive.npy"), img)


if __name__ == "__main__":
    main()
