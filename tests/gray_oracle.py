"""The colour-to-grey arithmetic of the extractor's colour input formats, in numpy: OpenCV 3.1.0's portable 8-bit RGB2Gray
(modules/imgproc/src/color.cpp: R2Y = 4899, G2Y = 9617, B2Y = 1868, yuv_shift = 14), a fixed-point sum with no float:

    grey = (4899 R + 9617 G + 1868 B + 8192) >> 14,     alpha ignored

The coefficients sum to 2^14, so the result never exceeds 255."""
import numpy as np

FMT_GRAY8, FMT_BGR8, FMT_RGB8, FMT_BGRA8, FMT_RGBA8 = 0, 1, 2, 3, 4
CHANNELS = {FMT_GRAY8: 1, FMT_BGR8: 3, FMT_RGB8: 3, FMT_BGRA8: 4, FMT_RGBA8: 4}
R2Y, G2Y, B2Y, SHIFT = 4899, 9617, 1868, 14


def to_gray(img, fmt):
    """(..., H, W, cn) uint8 in format `fmt` -> (..., H, W) uint8; FMT_GRAY8 takes (..., H, W) and returns a copy."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if fmt == FMT_GRAY8:
        return img.copy()
    assert img.shape[-1] == CHANNELS[fmt], (img.shape, fmt)
    c = img.astype(np.uint32)
    r, b = (c[..., 0], c[..., 2]) if fmt in (FMT_RGB8, FMT_RGBA8) else (c[..., 2], c[..., 0])
    return ((R2Y * r + G2Y * c[..., 1] + B2Y * b + (1 << (SHIFT - 1))) >> SHIFT).astype(np.uint8)
