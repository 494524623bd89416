"""Records PIL's Image.resize(size, resample=BICUBIC) for the small shapes of the resize tests as tests/golden/resize_<shape>.npz.

Each file holds x uint8 [3,Hs,Ws,3] (seeded uniform noise; a 0/255 checkerboard of period 3, whose overshoot hits both clamps; a
constant 255 image), y uint8 [3,Hd,Wd,3] (Pillow's results) and pillow_version.  Recorded data: synth.resize_bicubic_np and the
HIP kernel are held against it without Pillow installed.  The 1024x1024 -> 256x256 shape is left out (3 MiB per input); the tests
cover it through the restatement.

    python tests/golden/make_resize_golden.py
"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# (Hs, Ws, Hd, Wd)
SHAPES = [
    (218, 178, 256, 256), (37, 53, 16, 16), (16, 16, 37, 53), (5, 7, 16, 12), (3, 3, 8, 8),   # up and down, both ways
    (300, 200, 131, 200),                                                                        # vertical pass only
    (256, 100, 256, 64),                                                                         # horizontal pass only
    (256, 256, 256, 256),                                                                        # copy
    (1, 1, 4, 4), (64, 64, 1, 1),                                                                # degenerate
    (512, 192, 8, 3),                                                                            # factor 64, ksize 257
    (300, 250, 131, 77),                                                                         # several ragged tiles
]


def inputs(hs: int, ws: int) -> np.ndarray:
    """uint8 [3,hs,ws,3]: noise seeded by the shape, checkerboard of period 3, constant 255."""
    noise = np.random.default_rng(hs * 100003 + ws).integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:hs, 0:ws]
    checker = np.repeat(((((yy // 3) + (xx // 3)) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return np.stack([noise, checker, np.full((hs, ws, 3), 255, np.uint8)])


def main():
    for hs, ws, hd, wd in SHAPES:
        x = inputs(hs, ws)
        y = np.stack([np.asarray(Image.fromarray(im).resize((wd, hd), resample=Image.Resampling.BICUBIC)) for im in x])
        path = os.path.join(HERE, f"resize_{hs}x{ws}_{hd}x{wd}.npz")
        np.savez_compressed(path, x=x, y=y, pillow_version=np.array(PIL.__version__))
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
