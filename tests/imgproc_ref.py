"""Pure-numpy restatement of the pg_preprocess_images contract (include/plangen_hip.h): target size, Pillow's 8-bit bicubic coefficients
(libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc), horizontal then vertical pass through a uint8 intermediate, pad to a
square, lookup table.  No Pillow import: tests/test_imgproc_cpu.py checks it against Pillow and against the stored fixture."""
import math

import numpy as np

PRECISION_BITS = 22
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)

# (H, W, S) of tests/golden/imgproc_cases.npz, min_size 14 (tools/make_imgproc_golden.py)
CASES = [(37, 53, 32), (53, 37, 32), (20, 20, 32), (64, 97, 48), (5, 200, 32), (200, 5, 32), (48, 31, 48), (31, 48, 48), (333, 500, 384),
         (640, 427, 384)]
MIN_SIZE = 14
# not in the fixture (checked against Pillow live on the CPU, against this module on the GPU): exactly ONE pass runs -- min_size clamps the
# short side to the size it already has.  (In 48x31 -> 48 and 31x48 -> 48 the short side comes out unchanged too: both passes are skipped.)
EXTRA_CASES = [(14, 100, 32), (100, 14, 32)]


def case_name(h, w, s):
    return f"{h}x{w}_{s}"


def case_input(idx):
    """Seeded uint8 [H, W, 3] input of CASES[idx]; 333x500 is 0 / 255 only (the negative lobes clip on every edge)."""
    h, w, _ = (CASES + EXTRA_CASES)[idx]
    rs = np.random.RandomState(1000 + idx)
    if (h, w) == (333, 500):
        return ((rs.rand(h, w, 3) > 0.5) * 255).astype(np.uint8)
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def target_size(h, w, S, min_size=MIN_SIZE):
    m = max(h, w)
    return max(int(h / m * S), min_size), max(int(w / m * S), min_size)


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """(bounds int [out, 2] = (xmin, n), k int64 [out, ksize]) of one axis."""
    scale = fs = in_size / out_size
    if fs < 1.0:
        fs = 1.0
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    K = np.zeros((out_size, ksize), np.int64)
    B = np.zeros((out_size, 2), np.int64)
    ss = 1.0 / fs
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - c + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            K[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        B[xx] = (xmin, n)
    return B, K


def _pass_axis1(a, out_size):
    H, W, C = a.shape
    if out_size == W:
        return a
    B, K = coeffs(W, out_size)
    o = np.empty((H, out_size, C), np.uint8)
    for xx in range(out_size):
        x0, n = B[xx]
        acc = (a[:, x0:x0 + n, :].astype(np.int64) * K[xx, :n][None, :, None]).sum(1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                          # the contract accumulates in int32
        o[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return o


def resize(a, oh, ow):
    """uint8 [H, W, 3] -> uint8 [oh, ow, 3]: horizontal pass, uint8, vertical pass."""
    t = _pass_axis1(a, ow)
    return _pass_axis1(t.transpose(1, 0, 2), oh).transpose(1, 0, 2)


def pad_square(a, S, background):
    """expand2square onto the S x S canvas: uint8 [S, S, 3]."""
    oh, ow = a.shape[:2]
    out = np.empty((S, S, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    px, py = ((S - ow) // 2, 0) if ow < oh else (0, (S - oh) // 2)
    out[py:py + oh, px:px + ow] = a
    return out


def make_lut(mean, std, rescale_factor=1.0 / 255.0, do_normalize=True):
    v = (np.arange(256).astype(np.uint8).astype(np.float64) * rescale_factor).astype(np.float32)
    lut = np.stack([v, v, v])
    if do_normalize:
        for c in range(3):
            lut[c] = (lut[c] - np.float32(mean[c])) / np.float32(std[c])
    return lut.astype(np.float32)


def background_of(mean):
    return tuple(int(x * 255) for x in mean)


def preprocess_u8(a, S, min_size=MIN_SIZE, background=(127, 127, 127)):
    """uint8 [H, W, 3] -> the resized and padded uint8 [S, S, 3]."""
    oh, ow = target_size(a.shape[0], a.shape[1], S, min_size)
    return pad_square(resize(a, oh, ow), S, background)


def preprocess(a, S, mean, std, min_size=MIN_SIZE, rescale_factor=1.0 / 255.0, do_normalize=True, background=None):
    """uint8 [H, W, 3] -> float32 [3, S, S]."""
    u = preprocess_u8(a, S, min_size, background_of(mean) if background is None else background)
    lut = make_lut(mean, std, rescale_factor, do_normalize)
    return np.stack([lut[c][u[:, :, c]] for c in range(3)])
