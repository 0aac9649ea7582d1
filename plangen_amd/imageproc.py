"""The mmu path's image processor on the device: the reference's ``VLMImageProcessor``
(three_party/Janus/janus/models/image_processing_vlm.py:92-192) behind ``hack_image_proc`` (plangen_base.py:136-147).

Resize so that the longer side is ``image_size`` (Pillow's 8-bit bicubic), pad to a square with ``background_color``, rescale by
``rescale_factor``, normalise by mean / std.  The pixels are computed by ``pg_preprocess_images`` (include/plangen_hip.h); the rescale /
normalise arithmetic enters as a 3 x 256 table filled here with exactly transformers' statements, so the result equals the reference's bit
for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

IMAGENET_MEAN = (0.48145466, 0.4578275, 0.40821073)
IMAGENET_STD = (0.26862954, 0.26130258, 0.27577711)


def background_of(image_mean) -> tuple:
    """VLMImageProcessor.__init__ (image_processing_vlm.py:122-125)."""
    return (127, 127, 127) if image_mean is None else tuple(int(x * 255) for x in image_mean)


def make_lut(image_mean, image_std, rescale_factor: float = 1.0 / 255.0, do_normalize: bool = True) -> np.ndarray:
    """float32 [3, 256]: what the reference makes of uint8 value v in channel c -- transformers.image_transforms.rescale
    (``(v.astype(float64) * scale).astype(float32)``) followed, when ``do_normalize``, by normalize (``(x - float32(mean)) / float32(std)``
    in float32)."""
    v = (np.arange(256, dtype=np.uint8).astype(np.float64) * rescale_factor).astype(np.float32)
    lut = np.repeat(v[None], 3, 0)
    if do_normalize:
        mean = np.array(list(image_mean), dtype=np.float32)
        std = np.array(list(image_std), dtype=np.float32)
        lut = ((lut.T - mean) / std).T
    return np.ascontiguousarray(lut, dtype=np.float32)


class ImagesOutputs:
    """What ``hack_image_proc`` returns (plangen_base.py:138-141)."""

    def __init__(self, pixel_values):
        self.pixel_values = pixel_values


def _to_u8_hwc(image):
    if isinstance(image, (np.ndarray, torch.Tensor)):
        return image
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None and isinstance(image, Image.Image):
        return np.asarray(image.convert("RGB"))
    raise TypeError(f"VLMImageProcessor: unsupported image type {type(image).__name__} (uint8 [H, W, 3] array / tensor, or a PIL image)")


class VLMImageProcessor:
    """Constructor arguments and attributes of the reference class; ``engine`` is the ``plangen_amd.Engine`` whose GPU does the work."""

    model_input_names = ["pixel_values"]

    def __init__(self, image_size: int, min_size: int = 14, image_mean: Optional[Sequence[float]] = IMAGENET_MEAN,
                 image_std: Optional[Sequence[float]] = IMAGENET_STD, rescale_factor: float = 1.0 / 255.0, do_normalize: bool = True,
                 engine=None, **kwargs):
        self.image_size = image_size
        self.rescale_factor = rescale_factor
        self.image_mean = image_mean
        self.image_std = image_std
        self.min_size = min_size
        self.do_normalize = do_normalize
        self.background_color = background_of(image_mean)
        self.engine = engine

    @classmethod
    def from_config(cls, directory: str, engine=None, **overrides) -> "VLMImageProcessor":
        """The checkpoint directory's ``preprocessor_config.json`` (what VLChatProcessor.from_pretrained reads) when it has one;
        otherwise ``overrides`` alone (``image_size`` is then required)."""
        kw = {}
        path = os.path.join(str(directory), "preprocessor_config.json") if directory else ""
        if path and os.path.exists(path):
            cfg = json.load(open(path))
            kw = {k: cfg[k] for k in ("image_size", "min_size", "image_mean", "image_std", "rescale_factor", "do_normalize") if k in cfg}
        kw.update(overrides)
        return cls(engine=engine, **kw)

    @property
    def default_shape(self):
        return [3, self.image_size, self.image_size]

    def preprocess(self, images, return_tensors: str = "pt", dtype=torch.float32, **kwargs) -> ImagesOutputs:
        if self.engine is None:
            raise RuntimeError("VLMImageProcessor needs an engine (plangen_amd.Engine): the images are processed on the GPU, there is no CPU fallback")
        if not isinstance(images, (list, tuple)):
            images = [images]
        if self.do_normalize and (self.image_mean is None or self.image_std is None):
            raise ValueError("do_normalize=True needs image_mean and image_std")
        px = self.engine.preprocess_images([_to_u8_hwc(im) for im in images], self.image_size, self.min_size,
                                           mean=self.image_mean, std=self.image_std, rescale_factor=self.rescale_factor, dtype=dtype,
                                           background=self.background_color, do_normalize=self.do_normalize)
        if return_tensors == "np":
            px = px.float().cpu().numpy()
        return ImagesOutputs(px)

    def __call__(self, images, return_tensors: str = "pt", **kwargs) -> ImagesOutputs:
        if isinstance(images, torch.Tensor):        # hack_image_proc: an already processed tensor passes through untouched
            return ImagesOutputs(images)
        return self.preprocess(images, return_tensors=return_tensors, **kwargs)


def load_image_u8(path: str) -> np.ndarray:
    """An ``image_path`` row's file: a ``.npy`` holding uint8 [H, W, 3], or anything Pillow opens (converted to RGB)."""
    if str(path).endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{path}: expected uint8 [H, W, 3], got {a.dtype} {a.shape}")
        return a
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"{path}: reading image files other than .npy needs Pillow") from e
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))
