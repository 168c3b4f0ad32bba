"""A stand-in for the two cv2 calls of main/mono_depth/get_mono_depth.py, for make_golden_mono_depth.py only (there is no
OpenCV here): imread returns an image of the size the generator recorded for the path, and resize is the identity, which
INTER_NEAREST_EXACT is between equal sizes; it asserts that the sizes are equal."""
import numpy as np

INTER_NEAREST_EXACT = 6
SIZES = {}                                       # path -> (height, width), filled in by the generator


def imread(path):
    height, width = SIZES[path]
    return np.zeros((height, width, 3), np.uint8)


def resize(src, dsize, interpolation=None):
    assert interpolation == INTER_NEAREST_EXACT, interpolation
    assert (src.shape[1], src.shape[0]) == tuple(dsize), (src.shape, dsize)
    return src
