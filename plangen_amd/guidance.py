"""Sample plans for the image decode loop (``pg_request_sample_plan``, include/plangen_hip.h): per-image temperature, top-k,
top-p and RNG key, and a guidance weight per image AND step.  Host-side only: numpy arrays in, numpy arrays out; ``Engine.decode_image_tokens(plan=)``
hands them to the library, which validates them again.

    plan = SamplePlan(cfg_weight=np.stack([schedule("cosine", 7.0, 3.0, 576), schedule("constant", 5.0, 5.0, 576)]), image_key=[0, 0])
"""
from __future__ import annotations

import numpy as np

from . import textproc

KINDS = ("constant", "linear", "cosine")


def _host(a, dtype, name):
    """numpy or torch (host) -> contiguous numpy array of ``dtype``; None stays None."""
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype == object or a.size == 0:
        raise ValueError(f"SamplePlan: {name} must be a non-empty numeric array")
    if np.issubdtype(dtype, np.integer) and not np.issubdtype(a.dtype, np.integer):
        if a.dtype == bool or not (np.isfinite(a).all() and (a == np.rint(a)).all()):
            raise ValueError(f"SamplePlan: {name} must hold integers (got {a.tolist()})")
    return np.ascontiguousarray(a.astype(dtype))


class SamplePlan:
    """Per-image sampler parameters of one ``decode_image_tokens`` call; ``None`` stands for the call's scalar.

    cfg_weight  [B] or [B, T] float: the guidance weight of image b (at step t); [B] is broadcast over the steps when T is known.
    temperature [B] float: <= 0 makes that image greedy (its top_k / top_p are ignored).
    top_k       [B] int >= 0 (0: off);  top_p [B] float in (0, 1] (1: off).
    image_key   [B] int >= 0: the image index in the RNG stream key (default: the image's global index); equal keys draw equal noise.
    """

    FIELDS = ("cfg_weight", "temperature", "top_k", "top_p", "image_key")

    def __init__(self, cfg_weight=None, temperature=None, top_k=None, top_p=None, image_key=None):
        self.cfg_weight = _host(cfg_weight, np.float32, "cfg_weight")
        self.temperature = _host(temperature, np.float32, "temperature")
        self.top_k = _host(top_k, np.int64, "top_k")
        self.top_p = _host(top_p, np.float32, "top_p")
        self.image_key = _host(image_key, np.int64, "image_key")
        self.validate()

    @property
    def B(self):
        for f in self.FIELDS:
            a = getattr(self, f)
            if a is not None:
                return int(a.shape[0])
        return 0

    def validate(self):
        """The checks of pg_request_sample_plan, with the offending entry named."""
        if all(getattr(self, f) is None for f in self.FIELDS):
            raise ValueError("SamplePlan: every array is None -- nothing to plan")
        B = self.B
        for f in self.FIELDS:
            a = getattr(self, f)
            if a is None:
                continue
            if f == "cfg_weight":
                if a.ndim not in (1, 2) or a.shape[0] != B:
                    raise ValueError(f"SamplePlan: cfg_weight has shape {a.shape}, expected [{B}] or [{B}, T]")
            elif a.shape != (B,):
                raise ValueError(f"SamplePlan: {f} has shape {a.shape}, expected [{B}] (the first array given has {B} images)")
        if self.cfg_weight is not None and not np.isfinite(self.cfg_weight).all():
            raise ValueError(f"SamplePlan: cfg_weight is not finite at {tuple(np.argwhere(~np.isfinite(self.cfg_weight))[0])}")
        if self.temperature is not None and not np.isfinite(self.temperature).all():
            raise ValueError(f"SamplePlan: temperature[{int(np.argmax(~np.isfinite(self.temperature)))}] is not finite")
        if self.top_k is not None and ((self.top_k < 0) | (self.top_k >= 2 ** 31)).any():
            raise ValueError(f"SamplePlan: top_k must be >= 0 (got {self.top_k.tolist()})")
        if self.top_p is not None and not ((self.top_p > 0) & (self.top_p <= 1)).all():
            raise ValueError(f"SamplePlan: top_p must lie in (0, 1] (got {self.top_p.tolist()})")
        if self.image_key is not None and ((self.image_key < 0) | (self.image_key >= 2 ** 31 - 1)).any():
            raise ValueError(f"SamplePlan: image_key must lie in [0, 2^31 - 1) (got {self.image_key.tolist()})")

    def weights(self, T: int):
        """cfg_weight as fp32 [B, T] ([B] broadcast over the steps), or None."""
        w = self.cfg_weight
        if w is None:
            return None
        if w.ndim == 1:
            return np.ascontiguousarray(np.broadcast_to(w[:, None], (w.shape[0], T)))
        if w.shape[1] != T:
            raise ValueError(f"SamplePlan: cfg_weight holds {w.shape[1]} steps, the call has T = {T}")
        return w

    def arrays(self, T: int):
        """The five host arrays in the ABI's dtypes (fp32 [B, T], fp32 [B], int32 [B], fp32 [B], int32 [B]); None where not given."""
        i32 = lambda a: None if a is None else np.ascontiguousarray(a.astype(np.int32))
        return self.weights(T), self.temperature, i32(self.top_k), self.top_p, i32(self.image_key)


def schedule(kind: str, w_start: float, w_end: float, T: int):
    """fp32 [T]: the guidance weight at positions t = 0 .. T - 1, computed in float64 and rounded once.  With s = t / (T - 1) (s = 0 when T = 1):

        constant   w_start
        linear     w_start + (w_end - w_start) * s
        cosine     w_end + (w_start - w_end) * (1 + cos(pi * s)) / 2

    Every kind starts at w_start; linear and cosine end at w_end and are monotone in between."""
    if kind not in KINDS:
        raise ValueError(f"schedule: kind {kind!r} is none of {KINDS}")
    if T < 1:
        raise ValueError(f"schedule: T = {T} must be >= 1")
    a, b = float(w_start), float(w_end)
    s = np.arange(T, dtype=np.float64) / max(T - 1, 1)
    if kind == "constant":
        w = np.full(T, a, dtype=np.float64)
    elif kind == "linear":
        w = a + (b - a) * s
    else:
        w = b + (a - b) * (1.0 + np.cos(np.pi * s)) / 2.0
        w[0] = a
        if T > 1:
            w[-1] = b
    return w.astype(np.float32)


def box_weights(box_texts, grid: int, inside: float, outside: float, use_centerhw: bool = False):
    """fp32 [grid * grid] in the image tokens' raster order: ``inside`` at the cells whose centre lies in ANY of the boxes (``textproc.box_cells``),
    ``outside`` elsewhere.  No box, or boxes that hold no cell centre, give all ``outside``."""
    m = np.zeros((grid, grid), dtype=bool)
    for bt in box_texts:
        m |= textproc.box_cells(bt, grid, use_centerhw)
    return np.where(m.reshape(-1), np.float32(inside), np.float32(outside)).astype(np.float32)


def replicate(plan_per_prompt: SamplePlan, p: int, B0: int) -> SamplePlan:
    """The plan of a batch of ``p`` replicas of ``B0`` prompts in the replica layout (image t * B0 + i = replica t of prompt i): every array of the
    per-prompt plan ([B0, ...]) tiled p times along the image axis."""
    if plan_per_prompt.B != B0:
        raise ValueError(f"replicate: the plan holds {plan_per_prompt.B} images, B0 = {B0}")
    if p < 1:
        raise ValueError(f"replicate: p = {p} must be >= 1")
    tile = lambda a: None if a is None else np.concatenate([a] * p, axis=0)
    return SamplePlan(*(tile(getattr(plan_per_prompt, f)) for f in SamplePlan.FIELDS))
