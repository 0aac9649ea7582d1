"""Writes tests/golden/imgproc_cases.npz: what the reference's image processor makes of seeded uint8 inputs.

The reference's own class (three_party/Janus/janus/models/image_processing_vlm.py, VLMImageProcessor) cannot be imported where this
runs because torchvision is absent.  This generator therefore applies the reference's STATEMENTS -- ``resize`` line 137-156 (target
size, resize, expand2square line 41-52, to_numpy_array, transpose) and ``preprocess`` line 167-189 (rescale, normalize) -- with
``PIL.Image.resize(size[::-1], BICUBIC)`` in place of ``torchvision.transforms.functional.resize(pil_img, size, BICUBIC,
antialias=True)``, which for a PIL image is exactly that call (torchvision/transforms/_functional_pil.py: ``img.resize(tuple(size[::-1]),
interpolation)``).  rescale / normalize are transformers.image_transforms' own functions, called as BaseImageProcessor.rescale /
.normalize call them.  Class defaults: CLIP mean / std, rescale 1 / 255, min_size 14, background int(mean * 255).

Per case (tests/imgproc_ref.py CASES; inputs from imgproc_ref.case_input, numpy's frozen RandomState streams):
    <name>/resized  uint8 [oh, ow, 3]   Pillow's output
    <name>/padded   uint8 [S, S, 3]     after expand2square
    <name>/final    float32 [3, S, S]   after rescale + normalize
    <name>/input    uint8 [H, W, 3]
Two 384 x 384 results of random pixels do not compress below the size a fixture may have (each resized image alone is ~295 KB), so for
cases with S >= 256 the arrays are replaced by ``<name>/sha256`` = hex SHA-256 of the C-order bytes of (input, resized, padded, final,
final.astype(bfloat16) as int16): equality of the digests is equality of every bit.

    python tools/make_imgproc_golden.py        (needs Pillow and transformers; no GPU)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIGEST_FROM = 256


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bf16_bits(x: np.ndarray) -> np.ndarray:
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy()


def reference_pipeline(a: np.ndarray, image_size: int, min_size: int, image_mean, image_std, rescale_factor=1.0 / 255.0):
    from PIL import Image
    from transformers.image_transforms import normalize, rescale
    background_color = tuple([int(x * 255) for x in image_mean])
    pil_img = Image.fromarray(a, "RGB")
    # resize, line 137-156
    width, height = pil_img.size
    max_size = max(width, height)
    size = [max(int(height / max_size * image_size), min_size), max(int(width / max_size * image_size), min_size)]
    pil_img = pil_img.resize(tuple(size[::-1]), Image.BICUBIC)
    resized = np.array(pil_img)
    # expand2square, line 41-52
    width, height = pil_img.size
    if width > height:
        result = Image.new(pil_img.mode, (width, width), background_color)
        result.paste(pil_img, (0, (width - height) // 2))
        pil_img = result
    elif width < height:
        result = Image.new(pil_img.mode, (height, height), background_color)
        result.paste(pil_img, ((height - width) // 2, 0))
        pil_img = result
    padded = np.array(pil_img)
    x = np.transpose(padded, (2, 0, 1))
    # preprocess, line 167-189
    x = rescale(image=x, scale=rescale_factor, input_data_format="channels_first")
    x = normalize(image=x, mean=image_mean, std=image_std, input_data_format="channels_first")
    return resized, padded, np.ascontiguousarray(x, dtype=np.float32)


def main():
    import imgproc_ref as IR
    out = {}
    for i, (h, w, s) in enumerate(IR.CASES):
        a = IR.case_input(i)
        resized, padded, final = reference_pipeline(a, s, IR.MIN_SIZE, IR.CLIP_MEAN, IR.CLIP_STD)
        assert padded.shape == (s, s, 3) and final.shape == (3, s, s) and final.dtype == np.float32
        n = IR.case_name(h, w, s)
        if s >= DIGEST_FROM:
            out[n + "/sha256"] = np.array([sha(a), sha(resized), sha(padded), sha(final), sha(bf16_bits(final))])
            out[n + "/shape"] = np.array(resized.shape[:2])
        else:
            out[n + "/input"], out[n + "/resized"], out[n + "/padded"], out[n + "/final"] = a, resized, padded, final
    path = os.path.join(ROOT, "tests", "golden", "imgproc_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
