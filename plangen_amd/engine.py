"""Python owner of one ``pg_handle`` (one per process / GPU).

PyTorch-ROCm provides device tensors and the current HIP stream; every compute call goes
through the C ABI of include/plangen_hip.h.  No torch math on the product path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import PG_BF16, PG_F32, PG_FP8_E4M3
from .config import PlanGenConfig


class PlanGenError(RuntimeError):
    pass


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return PG_F32
    if t.dtype == torch.bfloat16:
        return PG_BF16
    raise TypeError(f"unsupported dtype {t.dtype} (need float32 or bfloat16)")


def _torch_dt(code: int):
    return torch.bfloat16 if code == PG_BF16 else torch.float32


def _wants_stats(return_stats) -> bool:
    """``return_stats``: False / None is off; True is n_alt = 0; an int is n_alt (0 is still a request)."""
    return return_stats is not None and return_stats is not False


def _n_alt(return_stats) -> int:
    return 0 if return_stats is True else int(return_stats)


def replica_owner(row: int, R0: int, shared: bool) -> int:
    """Owner rule of ``pg_prefill_replicated``: the row whose cache holds the prompt K/V that ``row`` of a batch of ``replicas`` copies of ``R0``
    CFG-interleaved rows (row t * R0 + r = replica t of row r) reads.  ``shared``: the negative prompt is batch-constant and shared, so every odd
    row reads row 1's; otherwise a row reads its first replica's.  A row aliases another row's prompt iff ``replica_owner(row) != row``."""
    return 1 if (shared and row % 2 == 1) else row % R0


def score_index(L: int, pad_len: Sequence[int], score_from: Sequence[int], device=None) -> torch.Tensor:
    """Index builder of ``Engine.score_text``: the flat positions r * L + j of the scored columns of an [R, L] id tensor, row-major --
    column j of row r is scored iff j >= score_from[r].  The hidden state that scores it sits at flat position - 1 (column j - 1 of the
    same row), which must be a real token: score_from[r] >= pad_len[r] + 1, else ValueError (a pad slot carries no hidden state, and
    column pad_len[r] has no predecessor).  score_from[r] == L scores nothing in row r."""
    pad_len = [int(v) for v in pad_len]
    score_from = [int(v) for v in score_from]
    if len(pad_len) != len(score_from):
        raise ValueError(f"score_from has {len(score_from)} entries for {len(pad_len)} rows")
    for r, (p, f) in enumerate(zip(pad_len, score_from)):
        if f < p + 1 or f > L:
            raise ValueError(f"row {r}: score_from={f} must lie in [pad_len + 1, L] = [{p + 1}, {L}]")
    sf = torch.tensor(score_from, dtype=torch.int64, device=device).view(-1, 1)
    j = torch.arange(L, dtype=torch.int64, device=device).view(1, -1)
    flat = torch.arange(len(score_from) * L, dtype=torch.int64, device=device).view(-1, L)
    return flat[j >= sf]


def head_logprob_geometry(n: int, V: int, K: int) -> dict:
    """The fused scoring head's tiling (score_head.hip::head_logprob_geom, mirrored): 256-row x 256-column tiles, G column groups of ``cpt``
    consecutive column tiles each -- a function of (n, V, K) alone.  ``ws_bytes``: the partials workspace a bf16 handle allocates for it."""
    tile, target_blocks = 256, 256
    ntm, ntn = (n + tile - 1) // tile, (V + tile - 1) // tile
    best = None
    for cpt in range(ntn, 0, -1):
        G = (ntn + cpt - 1) // cpt
        cost = ((ntm * G + target_blocks - 1) // target_blocks) * (cpt + 1)
        if best is None or cost < best[0]:
            best = (cost, cpt, G)
    _, cpt, G = best
    return dict(tile_rows=tile, tile_cols=tile, k_step=64, ntm=ntm, ntn=ntn, cpt=cpt, G=G, ws_bytes=(2 * 4 * G * n + 255) // 256 * 256)


def image_score_index(L: int, T: int, R: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Index builder of ``Engine.score_image``: (cond, uncond) int64 [B * T], B = R // 2, image-major -- the rows of the [R, L + T - 1, hidden]
    hidden tensor of one teacher-forced prefill of [prompt (L columns) | image embeddings 0 .. T-2], viewed as [R * (L + T - 1), hidden], that
    score image token j of image b: column L - 1 + j (the last prompt column scores token 0, the embedding of token j - 1 scores token j) of
    row 2b (cond) and of row 2b + 1 (uncond).  R must be even and >= 2, L >= 1 and T >= 1, else ValueError."""
    L, T, R = int(L), int(T), int(R)
    if R < 2 or R % 2:
        raise ValueError(f"R={R} must be even and >= 2 (CFG-interleaved rows: 2b cond, 2b + 1 uncond)")
    if L < 1 or T < 1:
        raise ValueError(f"L={L} and T={T} must be >= 1")
    W = L + T - 1
    col = L - 1 + torch.arange(T, dtype=torch.int64, device=device).view(1, T)
    row = 2 * torch.arange(R // 2, dtype=torch.int64, device=device).view(-1, 1)
    cond = (row * W + col).reshape(-1)
    return cond, cond + W


class Engine:
    """MI355X engine for the layout->image path.

    dtype 'bf16' (production: bf16 weights / activations / KV, fp32 accumulate, fp32 residual
    stream) or 'f32' (parity mode, BASELINE config 1).

    kv_dtype 'bf16' (default: the KV cache holds the compute dtype) or 'fp8': the opt-in FP8 (e4m3fn codes + one power-of-two scale
    per 128-element row) KV cache of the decode loop -- about half the cache bytes; results differ from the default's.  Needs
    dtype 'bf16'.  Format: include/plangen_hip.h.
    """

    def __init__(self, cfg: PlanGenConfig, dtype: str = "bf16", max_rows: int = 16, max_prompt: int = 256,
                 max_new: Optional[int] = None, max_images: Optional[int] = None, with_lm_head: bool = False,
                 with_vq_encoder: bool = False, with_vision: bool = False, max_vision_images: Optional[int] = None,
                 device: int = 0, diag: bool = False, kv_dtype: str = "bf16"):
        if not torch.cuda.is_available():
            raise PlanGenError("plangen_amd.Engine needs an MI355X (no CPU fallback)")
        # diag=True (tools/, bench.py's instrumented pass, hazard-screen tests): the handle lives in libplangen_diag.so -- the same object
        # code plus pg_diag_set_option; the product path never passes it
        self.diag = bool(diag)
        self.lib = _lib.load_diag() if diag else _lib.load()
        self.cfg = cfg
        self.dtype = dtype
        self.code = PG_BF16 if dtype == "bf16" else PG_F32
        if kv_dtype not in ("bf16", "fp8"):
            raise PlanGenError(f"kv_dtype must be 'bf16' or 'fp8' (got {kv_dtype!r})")
        self.kv_dtype = kv_dtype
        self.tdtype = _torch_dt(self.code)
        self.device = torch.device("cuda", device)
        self.max_rows = max_rows
        self.max_prompt = max_prompt
        self.max_new = max_new if max_new is not None else cfg.img_tokens
        self.max_images = max_images if max_images is not None else max(1, max_rows // 2)
        c = _lib.pg_config()
        for k in ("hidden", "inter", "n_layers", "n_heads", "head_dim", "vocab", "img_vocab", "img_dim", "grid",
                  "gen_head_dim", "vq_ch", "vq_z", "vq_res_blocks"):
            setattr(c, k, int(getattr(cfg, k)))
        c.vq_levels = len(cfg.vq_ch_mult)
        for i, m in enumerate(cfg.vq_ch_mult):
            c.vq_ch_mult[i] = int(m)
        c.rms_eps = cfg.rms_eps
        c.rope_theta = cfg.rope_theta
        c.compute_dtype = self.code
        c.max_rows, c.max_prompt, c.max_new, c.max_images = max_rows, max_prompt, self.max_new, self.max_images
        c.with_lm_head = int(with_lm_head)
        c.with_vq_encoder = int(with_vq_encoder)
        c.with_vision = int(with_vision)
        for k in ("vit_width", "vit_layers", "vit_heads", "vit_mlp", "vit_patch", "vit_img"):
            setattr(c, k, int(getattr(cfg, k)))
        c.max_vision_images = max_vision_images if max_vision_images is not None else self.max_images
        c.kv_dtype = PG_FP8_E4M3 if kv_dtype == "fp8" else 0
        self._c = c
        h = C.c_void_p()
        rc = self.lib.pg_create(C.byref(h), C.byref(c), device)
        if rc != 0:
            raise PlanGenError(f"pg_create failed ({_lib.STATUS.get(rc, rc)}): {self.lib.pg_last_error(None).decode()}")
        self.h = h
        self.R = 0
        self.L = 0
        self._keep = []       # tensors the library may still be reading asynchronously

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int, what: str):
        if rc != 0:
            raise PlanGenError(f"{what} failed ({_lib.STATUS.get(rc, rc)}): {self.lib.pg_last_error(self.h).decode()}")

    @property
    def stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
        return C.c_void_p(0 if t is None else t.data_ptr())

    def _dev(self, t: torch.Tensor, dtype=None) -> torch.Tensor:
        t = t.to(self.device)
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.contiguous()

    def close(self):
        if getattr(self, "h", None):
            self.lib.pg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self) -> int:
        return int(self.lib.pg_device_bytes(self.h))

    def set_option(self, key: str, value: int):
        self._check(self.lib.pg_set_option(self.h, key.encode(), int(value)), "pg_set_option")

    def set_diag_option(self, key: str, value: int):
        """Measurement-only switches of libplangen_diag.so (skip_attn, attn_variant, ...): needs Engine(diag=True)."""
        if not self.diag:
            raise PlanGenError("set_diag_option needs an engine created with diag=True (libplangen_diag.so)")
        self._check(self.lib.pg_diag_set_option(self.h, key.encode(), int(value)), "pg_diag_set_option")

    def timing(self) -> dict:
        t = _lib.pg_timing()
        self._check(self.lib.pg_get_timing(self.h, C.byref(t)), "pg_get_timing")
        return {k: getattr(t, k) for k, _ in t._fields_}

    def class_timing(self) -> dict:
        """Per-kernel-class sums of the last instrumented decode loop (after ``timing()``)."""
        out = {}
        cls = 0
        while True:
            name, ms, n, by = C.c_char_p(), C.c_double(), C.c_int(), C.c_double()
            if self.lib.pg_get_class_timing(self.h, cls, C.byref(name), C.byref(ms), C.byref(n), C.byref(by)) != 0:
                break
            out[name.value.decode()] = {"ms_sum": ms.value, "launches": n.value, "bytes_sum": by.value}
            cls += 1
        return out

    # ------------------------------------------------------------------ weights
    def load_tensors(self, sd: Dict[str, torch.Tensor]) -> Tuple[int, list]:
        """Hand tensors to ``pg_load_tensor`` by their reference state_dict names (HF Janus-Pro-1B keys,
        optionally with PlanGen's ``vl_gpt.`` prefix) WITHOUT finalizing: callers streaming a checkpoint in
        groups call this per group and :meth:`finalize` once.  Returns (#loaded, names the engine does not own)."""
        loaded, skipped = 0, []
        for name, t in sd.items():
            t = t.detach()
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            t = t.cpu().contiguous()
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            rc = self.lib.pg_load_tensor(self.h, name.encode(), C.c_void_p(t.data_ptr()), _dt(t), shape, t.dim())
            if rc == -4:
                skipped.append(name)
                continue
            self._check(rc, f"pg_load_tensor({name})")
            loaded += 1
        return loaded, skipped

    def merge_lora(self, name: str, A: torch.Tensor, B: torch.Tensor, scale: float) -> None:
        """``pg_merge_lora``: W <- W + scale * B A on the device, for the loaded projection ``name`` (its base state_dict name).
        A = lora_A [r, in], B = lora_B [out, r], fp32 or bf16 (other types are converted to fp32).  Un-finalizes the engine:
        call :meth:`finalize` after the last merge."""
        if A.dim() != 2 or B.dim() != 2 or B.shape[1] != A.shape[0]:
            raise PlanGenError(f"merge_lora({name}): lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} are not [r, in] / [out, r]")

        def host(t):
            t = t.detach()
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            return t.cpu().contiguous()

        A, B = host(A), host(B)
        rc = self.lib.pg_merge_lora(self.h, name.encode(), C.c_void_p(A.data_ptr()), _dt(A), C.c_void_p(B.data_ptr()), _dt(B),
                                    B.shape[0], A.shape[1], A.shape[0], float(scale))
        self._check(rc, f"pg_merge_lora({name})")

    def load_lora(self, adapters: Dict[str, Tuple[torch.Tensor, torch.Tensor]], alpha: float) -> int:
        """Merge every (lora_A, lora_B) pair of ``adapters`` (base weight name -> pair) with peft's scale alpha / r, r = A's rows.
        Returns the number merged; :meth:`finalize` is the caller's."""
        for name, (A, B) in adapters.items():
            self.merge_lora(name, A, B, float(alpha) / A.shape[0])
        return len(adapters)

    def finalize(self, strict: bool = True) -> int:
        """``pg_finalize_weights``: derived tables + decode weight layouts, once per checkpoint.  strict: raise when a
        required tensor was never loaded; otherwise the engine is told to run with the missing ones reading as zeros
        (``load_state_dict(strict=False)`` semantics of base_system.py:153-155).  Returns the number missing."""
        if not strict:
            self.set_option("allow_partial_weights", 1)
        missing = C.c_int(0)
        self._check(self.lib.pg_finalize_weights(self.h, C.byref(missing), self.stream), "pg_finalize_weights")
        if strict and missing.value:
            raise PlanGenError(f"{missing.value} required tensors missing; first: {self.lib.pg_last_error(self.h).decode()}")
        return missing.value

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> Tuple[int, list]:
        """load_tensors + finalize.  Returns (#loaded, skipped names)."""
        loaded, skipped = self.load_tensors(sd)
        self.finalize(strict)
        return loaded, skipped

    def init_synthetic(self, seed: int = 0, std: float = 0.02):
        """Seeded random-init weights of the configured architecture (bench / smoke: there is
        no checkpoint offline).  N(0, std^2) linears, norm weights 1, L2-normalised codebook
        (SURVEY 8d).  Generated tensor by tensor on the GPU, handed over through the same
        pg_load_tensor path a real checkpoint uses."""
        import math
        cfg = self.cfg
        g = torch.Generator(device=self.device).manual_seed(seed)

        def load(name, t):
            t = t.float().cpu().contiguous()
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            rc = self.lib.pg_load_tensor(self.h, name.encode(), C.c_void_p(t.data_ptr()), PG_F32, shape, t.dim())
            if rc != -4:
                self._check(rc, f"pg_load_tensor({name})")

        def nrm(*shape, s=std):
            return torch.randn(*shape, generator=g, device=self.device) * s

        H, I, HD = cfg.hidden, cfg.inter, cfg.n_heads * cfg.head_dim
        LM = "language_model.model."
        load(LM + "embed_tokens.weight", nrm(cfg.vocab, H))
        for i in range(cfg.n_layers):
            p = f"{LM}layers.{i}."
            for nme, shp in (("self_attn.q_proj", (HD, H)), ("self_attn.k_proj", (HD, H)), ("self_attn.v_proj", (HD, H)),
                             ("self_attn.o_proj", (H, HD)), ("mlp.gate_proj", (I, H)), ("mlp.up_proj", (I, H)),
                             ("mlp.down_proj", (H, I))):
                load(p + nme + ".weight", nrm(*shp))
            load(p + "input_layernorm.weight", torch.ones(H))
            load(p + "post_attention_layernorm.weight", torch.ones(H))
        load(LM + "norm.weight", torch.ones(H))
        load("language_model.lm_head.weight", nrm(cfg.vocab, H))
        G = cfg.gen_head_dim
        load("gen_head.output_mlp_projector.weight", nrm(G, H))
        load("gen_head.output_mlp_projector.bias", nrm(G))
        load("gen_head.vision_head.weight", nrm(cfg.img_vocab, G))
        load("gen_head.vision_head.bias", nrm(cfg.img_vocab))
        load("gen_embed.weight", nrm(cfg.img_vocab, cfg.img_dim, s=1.0))
        load("gen_aligner.layers.0.weight", nrm(H, cfg.img_dim, s=0.3))
        load("gen_aligner.layers.0.bias", nrm(H))
        load("gen_aligner.layers.2.weight", nrm(H, H))
        load("gen_aligner.layers.2.bias", nrm(H))
        V = "gen_vision_model."
        cb = (torch.rand(cfg.img_vocab, cfg.img_dim, generator=g, device=self.device) * 2 - 1) / cfg.img_vocab
        load(V + "quantize.embedding.weight", torch.nn.functional.normalize(cb, dim=-1))
        load(V + "post_quant_conv.weight", nrm(cfg.vq_z, cfg.img_dim, 1, 1, s=0.3))
        load(V + "post_quant_conv.bias", nrm(cfg.vq_z))

        def conv(name, cout, cin, k):
            load(name + ".weight", nrm(cout, cin, k, k, s=1.0 / math.sqrt(cin * k * k)))
            load(name + ".bias", nrm(cout, s=0.02))

        def norm(name, c):
            load(name + ".weight", torch.ones(c))
            load(name + ".bias", torch.zeros(c))

        def res(name, cin, cout):
            norm(name + ".norm1", cin); conv(name + ".conv1", cout, cin, 3)
            norm(name + ".norm2", cout); conv(name + ".conv2", cout, cout, 3)
            if cin != cout:
                conv(name + ".nin_shortcut", cout, cin, 1)

        def attn(name, c):
            norm(name + ".norm", c)
            for t in ("q", "k", "v", "proj_out"):
                conv(name + "." + t, c, c, 1)

        D = V + "decoder."
        nres = len(cfg.vq_ch_mult)
        bin_ = cfg.vq_ch * cfg.vq_ch_mult[-1]
        conv(D + "conv_in", bin_, cfg.vq_z, 3)
        res(D + "mid.0", bin_, bin_); attn(D + "mid.1", bin_); res(D + "mid.2", bin_, bin_)
        for bi, lvl in enumerate(reversed(range(nres))):
            bout = cfg.vq_ch * cfg.vq_ch_mult[lvl]
            for j in range(cfg.vq_res_blocks + 1):
                res(f"{D}conv_blocks.{bi}.res.{j}", bin_, bout)
                bin_ = bout
                if lvl == nres - 1:
                    attn(f"{D}conv_blocks.{bi}.attn.{j}", bin_)
            if lvl != 0:
                conv(f"{D}conv_blocks.{bi}.upsample.conv", bin_, bin_, 3)
        norm(D + "norm_out", bin_)
        conv(D + "conv_out", 3, bin_, 3)
        if self._c.with_vq_encoder:
            E = V + "encoder."
            conv(E + "conv_in", cfg.vq_ch, 3, 3)
            in_mult = (1,) + tuple(cfg.vq_ch_mult)
            b_in = cfg.vq_ch
            for lvl in range(nres):
                b_in = cfg.vq_ch * in_mult[lvl]
                b_out = cfg.vq_ch * cfg.vq_ch_mult[lvl]
                for j in range(cfg.vq_res_blocks):
                    res(f"{E}conv_blocks.{lvl}.res.{j}", b_in, b_out)
                    b_in = b_out
                    if lvl == nres - 1:
                        attn(f"{E}conv_blocks.{lvl}.attn.{j}", b_in)
                if lvl != nres - 1:
                    conv(f"{E}conv_blocks.{lvl}.downsample.conv", b_in, b_in, 3)
            res(E + "mid.0", b_in, b_in); attn(E + "mid.1", b_in); res(E + "mid.2", b_in, b_in)
            norm(E + "norm_out", b_in)
            conv(E + "conv_out", cfg.vq_z, b_in, 3)
            conv(V + "quant_conv", cfg.img_dim, cfg.vq_z, 1)
        if self._c.with_vision:
            Cw, Mh, ps = cfg.vit_width, cfg.vit_mlp, cfg.vit_patch
            VT = "vision_model.vision_tower."

            def lin(name, o, i):
                load(name + ".weight", nrm(o, i)); load(name + ".bias", nrm(o))

            load(VT + "patch_embed.proj.weight", nrm(Cw, 3, ps, ps, s=1.0 / math.sqrt(3 * ps * ps)))
            load(VT + "patch_embed.proj.bias", nrm(Cw))
            load(VT + "pos_embed", nrm(1, cfg.vit_tokens, Cw))
            for i in range(cfg.vit_layers):
                b = f"{VT}blocks.{i}."
                norm(b + "norm1", Cw); lin(b + "attn.qkv", 3 * Cw, Cw); lin(b + "attn.proj", Cw, Cw)
                norm(b + "norm2", Cw); lin(b + "mlp.fc1", Mh, Cw); lin(b + "mlp.fc2", Cw, Mh)
            norm(VT + "norm", Cw)
            lin("aligner.layers.0", H, Cw); lin("aligner.layers.2", H, H)
        missing = C.c_int(0)
        self._check(self.lib.pg_finalize_weights(self.h, C.byref(missing), self.stream), "pg_finalize_weights")
        if missing.value:
            raise PlanGenError(f"{missing.value} tensors missing after init_synthetic: {self.lib.pg_last_error(self.h).decode()}")

    # ------------------------------------------------------------------ language model
    @staticmethod
    def pad_len_from_mask(mask: torch.Tensor, L: int) -> list:
        """Leading-zero count of each row of a LEFT-padded attention mask [R, >=L]."""
        m = mask[:, :L].to("cpu", torch.int64)
        if not bool(((m[:, 1:] - m[:, :-1]) >= 0).all()):
            raise PlanGenError("attention_mask is not left-padded (0...01...1)")
        return (L - m.sum(-1)).tolist()

    @staticmethod
    def uncond_rows_shared(ids: torch.Tensor, pad_len: Sequence[int]) -> bool:
        """Host-side form of the library's probe: every odd (uncond CFG) row carries row 1's padding and ids."""
        R = ids.shape[0]
        if R < 4 or R % 2:
            return False
        if any(int(pad_len[r]) != int(pad_len[1]) for r in range(3, R, 2)):
            return False
        return bool((ids[3::2, int(pad_len[1]):] == ids[1, int(pad_len[1]):]).all())

    def _request_attn_spans(self, attn_spans, R: int) -> torch.Tensor:
        """``pg_request_attn_spans`` for the next prefill: ``attn_spans`` = (lo, hi, q_col0, n_q, layers) with lo / hi int [R, S] span
        bounds in columns (S in 1..16), the reported query columns [q_col0, q_col0 + n_q) and ``layers`` an iterable of layer indices
        (None: all).  Returns the fp32 [len(layers), R, n_q, S] tensor that prefill fills (NaN where it writes nothing), layers ascending."""
        lo, hi, q_col0, n_q, layers = attn_spans
        lo = torch.as_tensor(lo).to("cpu", torch.int32).contiguous()
        hi = torch.as_tensor(hi).to("cpu", torch.int32).contiguous()
        if lo.dim() != 2 or lo.shape != hi.shape or lo.shape[0] != R:
            raise PlanGenError(f"attn_spans: lo / hi must both be [R, S] = [{R}, S] (got {tuple(lo.shape)} / {tuple(hi.shape)})")
        layers = sorted(set(int(l) for l in (range(self.cfg.n_layers) if layers is None else layers)))
        if not layers or layers[0] < 0 or layers[-1] >= self.cfg.n_layers:
            raise PlanGenError(f"attn_spans: layers must be a non-empty subset of 0 .. {self.cfg.n_layers - 1}")
        mask = 0
        for l in layers:
            mask |= 1 << l
        S = lo.shape[1]
        out = torch.full((len(layers), R, max(int(n_q), 0), S), float("nan"), dtype=torch.float32, device=self.device)
        req = _lib.pg_attn_spans(lo.data_ptr(), hi.data_ptr(), R, S, int(q_col0), int(n_q), mask, out.data_ptr(), out.numel())
        self._check(self.lib.pg_request_attn_spans(self.h, C.byref(req)), "pg_request_attn_spans")
        return out

    def prefill(self, ids: torch.Tensor, pad_len: Sequence[int], position_mode: int = 0,
                return_hidden: bool = False, hidden_dtype=torch.float32, uncond_shared: Optional[bool] = None, attn_spans=None):
        """uncond_shared: None -> decided here when ``ids`` is still a HOST tensor (the collate's output; exact comparison, no device
        sync inside pg_prefill), probed on the device otherwise; True / False -> the caller's own host-side answer (bench.py:
        rank 0 compares the collated ids once and broadcasts the flag with them).  attn_spans (see ``_request_attn_spans``): the call
        returns (hidden or None, fp32 [layers, R, n_q, S] attention mass on the spans) instead."""
        if uncond_shared is None and not ids.is_cuda and position_mode == 0 and not return_hidden:
            uncond_shared = self.uncond_rows_shared(ids, pad_len)
        self.set_option("uncond_shared_hint", -1 if uncond_shared is None else int(bool(uncond_shared)))    # always sent: never a stale hint
        ids = self._dev(ids, torch.int32)
        R, L = ids.shape
        pl = (C.c_int32 * R)(*[int(v) for v in pad_len])
        out = torch.empty((R, L, self.cfg.hidden), dtype=hidden_dtype, device=self.device) if return_hidden else None
        mass = self._request_attn_spans(attn_spans, R) if attn_spans is not None else None
        self._check(self.lib.pg_prefill(self.h, self._p(ids), pl, R, L, position_mode, self._p(out),
                                        _dt(out) if out is not None else PG_F32, self.stream), "pg_prefill")
        self.R, self.L = R, L
        self._keep = [ids, mass]
        return out if attn_spans is None else (out, mass)

    def prefill_replicated(self, ids: torch.Tensor, pad_len: Sequence[int], replicas: int, alias: bool = True,
                           uncond_shared: Optional[bool] = None) -> None:
        """``pg_prefill_replicated``: the state of ``prefill(torch.cat([ids] * replicas), list(pad_len) * replicas)`` with every distinct prompt
        prefilled once.  ``ids`` [R0, L] / ``pad_len`` [R0] are the un-replicated CFG batch; afterwards the engine holds R0 * replicas rows (row
        t * R0 + r = replica t of row r).  alias=True: the replicas' prompt slots alias their owner's in the decode attention; False: they are
        copied (the A/B fallback, same bits).  uncond_shared as in :meth:`prefill` (evaluated on the replicated rows)."""
        R0, L = ids.shape
        if uncond_shared is None and not ids.is_cuda and replicas >= 1:
            pl_all = [int(v) for v in pad_len] * int(replicas)
            rep = torch.cat([ids] * int(replicas)) if replicas > 1 else ids
            uncond_shared = self.uncond_rows_shared(rep, pl_all) if R0 % 2 == 0 else False
        self.set_option("uncond_shared_hint", -1 if uncond_shared is None else int(bool(uncond_shared)))    # always sent: never a stale hint
        ids = self._dev(ids, torch.int32)
        pl = (C.c_int32 * R0)(*[int(v) for v in pad_len])
        self._check(self.lib.pg_prefill_replicated(self.h, self._p(ids), pl, R0, L, int(replicas), int(alias), self.stream), "pg_prefill_replicated")
        self.R, self.L = R0 * int(replicas), L
        self._keep = [ids]

    def prefill_embeds(self, embeds: torch.Tensor, pad_len: Sequence[int], position_mode: int = 0,
                       return_hidden: bool = False, hidden_dtype=torch.float32, attn_spans=None):
        """attn_spans: as in :meth:`prefill` -- the call returns (hidden or None, attention mass) instead."""
        embeds = self._dev(embeds)
        R, L, _ = embeds.shape
        pl = (C.c_int32 * R)(*[int(v) for v in pad_len])
        out = torch.empty((R, L, self.cfg.hidden), dtype=hidden_dtype, device=self.device) if return_hidden else None
        mass = self._request_attn_spans(attn_spans, R) if attn_spans is not None else None
        self._check(self.lib.pg_prefill_embeds(self.h, self._p(embeds), _dt(embeds), pl, R, L, position_mode,
                                               self._p(out), _dt(out) if out is not None else PG_F32, self.stream),
                    "pg_prefill_embeds")
        self.R, self.L = R, L
        self._keep = [embeds, mass]
        return out if attn_spans is None else (out, mass)

    def extend(self, ids: Optional[torch.Tensor] = None, embeds: Optional[torch.Tensor] = None, n_new: Optional[Sequence[int]] = None,
               return_hidden: bool = False, hidden_dtype=torch.float32):
        """``pg_prefill_extend``: continue the cached rows with many tokens in one pass.  Exactly one of ``ids`` int [R, Lx] / ``embeds``
        [R, Lx, hidden]; the first ``n_new[r]`` columns of row r are its new tokens (default: all Lx).  New token i of row r takes slot
        ``cached_len()[r] + i``, the RoPE position the preceding prefill's rule gives that slot, and attends to everything the row holds.
        Afterwards every decode entry point continues as after a prefill of the longer rows.  return_hidden: the final-norm hidden states
        [R, Lx, hidden] of the new tokens (unused columns zero)."""
        if (ids is None) == (embeds is None):
            raise PlanGenError("extend: exactly one of ids / embeds must be given")
        src = self._dev(ids, torch.int32) if ids is not None else self._dev(embeds)
        if src.dim() != (2 if ids is not None else 3) or src.shape[0] != self.R:
            raise PlanGenError(f"extend: expected {self.R} rows of [R, Lx{'' if ids is not None else ', hidden'}] (got {tuple(src.shape)})")
        Lx = src.shape[1]
        nn = [Lx] * self.R if n_new is None else [int(v) for v in n_new]
        if len(nn) != self.R:
            raise PlanGenError(f"extend: n_new has {len(nn)} entries for {self.R} rows")
        out = torch.empty((self.R, Lx, self.cfg.hidden), dtype=hidden_dtype, device=self.device) if return_hidden else None
        self._check(self.lib.pg_prefill_extend(self.h, self._p(src) if ids is not None else None, self._p(src) if ids is None else None,
                                               _dt(src) if ids is None else PG_F32, (C.c_int32 * self.R)(*nn), Lx, self._p(out),
                                               _dt(out) if out is not None else PG_F32, self.stream), "pg_prefill_extend")
        self._keep = [src]
        return out

    def rewind(self, lens: Sequence[int]) -> None:
        """``pg_rewind``: row r keeps its first ``lens[r]`` cached slots (1 <= lens[r] <= cached_len()[r]).  An :meth:`extend` follows before
        anything samples: the hidden state the samplers read is not recomputed."""
        ln = [int(v) for v in lens]
        if len(ln) != self.R:
            raise PlanGenError(f"rewind: lens has {len(ln)} entries for {self.R} rows")
        self._check(self.lib.pg_rewind(self.h, (C.c_int32 * self.R)(*ln), self.stream), "pg_rewind")

    def cached_len(self) -> list:
        """K/V slots every row holds: its prompt plus the decode steps run since (the token a loop emitted last was never fed back and has no
        slot).  Reads two small device arrays: synchronises."""
        ln = self.debug_read("len", 0, self.R, torch.int32)
        nd = self.debug_read("n_dec", 0, 1, torch.int32)
        return (ln + nd).tolist()

    def step(self, embeds: torch.Tensor, hidden_dtype=torch.float32) -> torch.Tensor:
        embeds = self._dev(embeds).view(self.R, self.cfg.hidden)
        out = torch.empty((self.R, self.cfg.hidden), dtype=hidden_dtype, device=self.device)
        self._check(self.lib.pg_step(self.h, self._p(embeds), _dt(embeds), self._p(out), _dt(out), self.stream), "pg_step")
        self._keep = [embeds]
        return out

    def gen_head(self, h: torch.Tensor) -> torch.Tensor:
        h = self._dev(h)
        R = h.shape[0]
        out = torch.empty((R, self.cfg.img_vocab), dtype=torch.float32, device=self.device)
        self._check(self.lib.pg_gen_head(self.h, self._p(h), _dt(h), self._p(out), R, self.stream), "pg_gen_head")
        self._keep = [h]
        return out

    def gen_embed(self, tok: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        tok = self._dev(tok.reshape(-1), torch.int32)
        out = torch.empty((tok.numel(), self.cfg.hidden), dtype=dtype, device=self.device)
        self._check(self.lib.pg_gen_embed(self.h, self._p(tok), self._p(out), _dt(out), tok.numel(), self.stream), "pg_gen_embed")
        self._keep = [tok]
        return out

    def embed_tokens(self, ids: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        shape = tuple(ids.shape)
        flat = self._dev(ids.reshape(-1), torch.int32)
        out = torch.empty((flat.numel(), self.cfg.hidden), dtype=dtype, device=self.device)
        self._check(self.lib.pg_embed_tokens(self.h, self._p(flat), self._p(out), _dt(out), flat.numel(), self.stream), "pg_embed_tokens")
        self._keep = [flat]
        return out.view(*shape, self.cfg.hidden)

    def decode_image_tokens(self, T: Optional[int] = None, cfg_weight: float = 5.0, temperature: float = 0.0,
                            seed: int = 0, force_tokens: Optional[torch.Tensor] = None,
                            force_mask: Optional[torch.Tensor] = None, return_logits: bool = False,
                            top_k: int = 0, top_p: float = 1.0, return_logprobs: bool = False, return_stats=False, plan=None):
        """The fused CFG decode loop.  top_k / top_p filter the sampled draws (temperature > 0; HF order temperature ->
        top-k -> top-p); (0, 1.0) is the unfiltered sampler.  return_logprobs: also fp32 [B, T], the log-probability of every emitted
        token under softmax(mixed / temperature) before the filters (``pg_request_token_logprobs``); with ``force_mask = zeros`` it is the
        log-likelihood of ``force_tokens``.  return_stats (True, or an int n_alt in 1..8): also (last) the dict of ``_request_stats``
        over [B, T]: the emitted tokens' entropy, rank and top-n_alt alternatives (``pg_request_token_stats``).  plan (a
        ``guidance.SamplePlan``): per-image temperature / top_k / top_p / RNG key and a per-(image, step) guidance weight in place of the
        scalars (``pg_request_sample_plan``; an array the plan leaves out takes the scalar).  Semantics: include/plangen_hip.h."""
        T = self.cfg.img_tokens if T is None else T
        B = self.R // 2
        if plan is not None and plan.B != B:
            raise PlanGenError(f"decode_image_tokens: the plan holds {plan.B} images, the batch has {B}")
        out = torch.zeros((B, T), dtype=torch.int32, device=self.device)
        lp = self._request_logprobs((B, T)) if return_logprobs else None
        stt = self._request_stats((B, T), return_stats) if _wants_stats(return_stats) else None
        ft = self._dev(force_tokens, torch.int32) if force_tokens is not None else None
        fm = self._dev(force_mask, torch.uint8) if force_mask is not None else None
        lg = torch.zeros((T, B, self.cfg.img_vocab), dtype=torch.float32, device=self.device) if return_logits else None
        if plan is not None:      # last of the preparations: nothing between the request and the call that consumes it can raise
            self._request_sample_plan(plan, T)
        if int(top_k) == 0 and float(top_p) == 1.0:
            self._check(self.lib.pg_decode_image_tokens(self.h, T, float(cfg_weight), float(temperature), int(seed),
                                                        self._p(ft), self._p(fm), self._p(out), self._p(lg), self.stream),
                        "pg_decode_image_tokens")
        else:
            self._check(self.lib.pg_decode_image_tokens_filtered(self.h, T, float(cfg_weight), float(temperature), int(top_k),
                                                                 float(top_p), int(seed), self._p(ft), self._p(fm), self._p(out),
                                                                 self._p(lg), self.stream), "pg_decode_image_tokens_filtered")
        self._keep = [ft, fm, out, lg, lp, stt]
        res = (out,) + ((lg,) if return_logits else ()) + ((lp,) if return_logprobs else ()) + ((stt,) if stt is not None else ())
        return res if len(res) > 1 else res[0]

    def decode_image_tokens_dual(self, T: Optional[int] = None, w_caption: float = 5.0, w_layout: float = 5.0, temperature: float = 0.0,
                                 seed: int = 0, force_tokens: Optional[torch.Tensor] = None, force_mask: Optional[torch.Tensor] = None,
                                 return_logits: bool = False, top_k: int = 0, top_p: float = 1.0, return_logprobs: bool = False,
                                 return_stats=False):
        """The fused decode loop under dual guidance (``pg_decode_image_tokens_dual``), after a prefill of R = 3B rows with
        ``uncond_shared=False``: row 3b = caption + layout (f), 3b + 1 = caption only (p), 3b + 2 = negative (u);
        ``mixed = (u + w_caption (p - u)) + w_layout (f - p)``.  Everything else -- shapes of the results, forcing, top_k / top_p,
        return_logprobs, return_stats -- as :meth:`decode_image_tokens` with B = R / 3.  No sample plan."""
        T = self.cfg.img_tokens if T is None else T
        if self.R % 3:
            raise PlanGenError(f"decode_image_tokens_dual: the batch has {self.R} rows, not a multiple of three")
        B = self.R // 3
        out = torch.zeros((B, T), dtype=torch.int32, device=self.device)
        lp = self._request_logprobs((B, T)) if return_logprobs else None
        stt = self._request_stats((B, T), return_stats) if _wants_stats(return_stats) else None
        ft = self._dev(force_tokens, torch.int32) if force_tokens is not None else None
        fm = self._dev(force_mask, torch.uint8) if force_mask is not None else None
        lg = torch.zeros((T, B, self.cfg.img_vocab), dtype=torch.float32, device=self.device) if return_logits else None
        self._check(self.lib.pg_decode_image_tokens_dual(self.h, T, float(w_caption), float(w_layout), float(temperature), int(top_k), float(top_p),
                                                         int(seed), self._p(ft), self._p(fm), self._p(out), self._p(lg), self.stream),
                    "pg_decode_image_tokens_dual")
        self._keep = [ft, fm, out, lg, lp, stt]
        res = (out,) + ((lg,) if return_logits else ()) + ((lp,) if return_logprobs else ()) + ((stt,) if stt is not None else ())
        return res if len(res) > 1 else res[0]

    @staticmethod
    def cfg3_sample_op(partial, S, slab, bias, V, B, out_tok, logits_out, embed_table, x, H, w_caption, w_layout, temperature, seed, T, step,
                       top_k=0, top_p=1.0, img_off=0, b_off=0, B_total=None, force_tok=None, force_mask=None, filtered=False, stored=False,
                       mix_out=None, stream=None) -> int:
        """``pg_diag_op_cfg3_sample`` (diagnostics library): one dual-guidance step of the image sampler on caller-given device tensors -- the
        slabs ``partial`` (rows [3B, V] per slab: 3b = f, 3b + 1 = p, 3b + 2 = u), ``out_tok`` int32 [B_total, T], ``logits_out`` fp32
        [T, B_total, V] or None, ``x`` fp32 [3B, H], ``mix_out`` fp32 [B, V] or None (the stored rows; needs filtered or stored).  Returns the
        status code (0: PG_OK); the stream is synchronised."""
        d = _lib.load_diag()
        fn = d.pg_diag_op_cfg3_sample
        _P, _I, _F = C.c_void_p, C.c_int, C.c_float
        fn.restype = C.c_int
        fn.argtypes = [_I, _I, _P, _I, C.c_long, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _F, _F, _F, C.c_uint64, _I, _F, _I, _I, _I, _I, _I, _P]
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        B_total = b_off + B if B_total is None else B_total
        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        return fn(int(bool(filtered)), int(bool(stored)), ptr(partial), S, slab, ptr(bias), V, B, ptr(force_tok), ptr(force_mask), ptr(out_tok),
                  ptr(logits_out), ptr(mix_out), ptr(embed_table), ptr(x), H, float(w_caption), float(w_layout), float(temperature), int(seed),
                  int(top_k), float(top_p), T, step, img_off, b_off, B_total, stream)

    def _request_sample_plan(self, plan, T: int):
        """``pg_request_sample_plan`` for the next image decode (the library copies the host arrays before it returns)."""
        arrs = plan.arrays(T)
        ptr = lambda a: C.c_void_p(0 if a is None else a.ctypes.data)
        req = _lib.pg_sample_plan(*(ptr(a) for a in arrs), plan.B, T)
        self._check(self.lib.pg_request_sample_plan(self.h, C.byref(req), self.stream), "pg_request_sample_plan")

    @staticmethod
    def cfg_sample_plan_op(partial, S, slab, bias, V, B, out_tok, logits_out, embed_table, x, H, w, temperature, top_k, top_p, key, seed, T, step,
                           b_off=0, B_total=None, force_tok=None, force_mask=None, filtered=False, stored=False, stream=None) -> int:
        """``pg_diag_op_cfg_sample_plan`` (diagnostics library): one step of the image sampler under a sample plan, on caller-given device
        tensors -- the slabs ``partial``, ``out_tok`` int32 [B_total, T], ``logits_out`` fp32 [T, B_total, V] or None, and the plan's device
        arrays ``w`` fp32 [B_total, T], ``temperature`` fp32 / ``top_k`` int32 / ``top_p`` fp32 / ``key`` int32 [B_total].  Returns the
        status code (0: PG_OK); the stream is synchronised."""
        d = _lib.load_diag()
        fn = d.pg_diag_op_cfg_sample_plan
        _P, _I = C.c_void_p, C.c_int
        fn.restype = C.c_int
        fn.argtypes = [_I, _I, _P, _I, C.c_long, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, C.c_uint64, _I, _I, _I, _I, _P]
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        B_total = b_off + B if B_total is None else B_total
        stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
        return fn(int(bool(filtered)), int(bool(stored)), ptr(partial), S, slab, ptr(bias), V, B, ptr(force_tok), ptr(force_mask), ptr(out_tok),
                  ptr(logits_out), ptr(embed_table), ptr(x), H, ptr(w), ptr(temperature), ptr(top_k), ptr(top_p), ptr(key), int(seed), T, step,
                  b_off, B_total, stream)

    def _request_logprobs(self, shape) -> torch.Tensor:
        """``pg_request_token_logprobs`` for the next decode / generate call: the fp32 tensor that call fills (NaN where it writes nothing)."""
        lp = torch.full(shape, float("nan"), dtype=torch.float32, device=self.device)
        self._check(self.lib.pg_request_token_logprobs(self.h, self._p(lp), lp.numel()), "pg_request_token_logprobs")
        return lp

    def _stats_buffers(self, shape, n_alt: int):
        """(dict of result tensors, the pg_token_stats naming them): fp32 NaN / int32 -2 where a call writes nothing."""
        shape = tuple(shape)
        d = {"logprob": torch.full(shape, float("nan"), dtype=torch.float32, device=self.device),
             "entropy": torch.full(shape, float("nan"), dtype=torch.float32, device=self.device),
             "rank": torch.full(shape, -2, dtype=torch.int32, device=self.device)}
        if n_alt > 0:
            d["alt_tok"] = torch.full(shape + (n_alt,), -2, dtype=torch.int32, device=self.device)
            d["alt_logprob"] = torch.full(shape + (n_alt,), float("nan"), dtype=torch.float32, device=self.device)
        req = _lib.pg_token_stats(self._p(d["logprob"]), self._p(d["entropy"]), self._p(d["rank"]), self._p(d.get("alt_tok")),
                                  self._p(d.get("alt_logprob")), n_alt, d["rank"].numel())
        return d, req

    def _request_stats(self, shape, return_stats) -> dict:
        """``pg_request_token_stats`` for the next decode / generate call: the dict that call fills -- ``logprob`` fp32, ``entropy`` fp32
        (nats), ``rank`` int32 (0: the emitted token was the mode) over ``shape``, and with n_alt > 0 ``alt_tok`` int32 / ``alt_logprob``
        fp32 over ``shape + (n_alt,)`` (-1 / -inf where a row has fewer alternatives)."""
        d, req = self._stats_buffers(shape, _n_alt(return_stats))
        self._check(self.lib.pg_request_token_stats(self.h, C.byref(req)), "pg_request_token_stats")
        return d

    def token_stats(self, x: torch.Tensor, tok: torch.Tensor, temperature: float = 0.0, n_alt: int = 0) -> dict:
        """``pg_op_token_stats``: the loops' uncertainty reducer over fp32 rows ``x`` [B, V] and tokens ``tok`` [B] -> the dict of
        ``_request_stats`` over [B]; ``logprob`` has the bits of ``token_logprob``."""
        x = self._dev(x, torch.float32).reshape(-1, x.shape[-1]).contiguous()
        B, V = x.shape
        t = self._dev(torch.as_tensor(tok), torch.int32).reshape(-1).contiguous()
        if t.numel() != B:
            raise PlanGenError(f"token_stats: {t.numel()} tokens for {B} rows")
        d, req = self._stats_buffers((B,), int(n_alt))
        self._check(self.lib.pg_op_token_stats(self.h, self._p(x), B, V, self._p(t), float(temperature), C.byref(req), self.stream),
                    "pg_op_token_stats")
        self._keep = [x, t, d]
        return d

    def token_logprob(self, x: torch.Tensor, tok: torch.Tensor, temperature: float = 0.0) -> torch.Tensor:
        """``pg_op_token_logprob``: the loops' scoring kernel over fp32 rows ``x`` [B, V] and tokens ``tok`` [B] -> fp32 [B],
        log softmax(x / temperature)[tok] (temperature <= 0: of x itself); a token outside [0, V) gives -inf."""
        x = self._dev(x, torch.float32).reshape(-1, x.shape[-1]).contiguous()
        B, V = x.shape
        t = self._dev(torch.as_tensor(tok), torch.int32).reshape(-1).contiguous()
        if t.numel() != B:
            raise PlanGenError(f"token_logprob: {t.numel()} tokens for {B} rows")
        out = torch.full((B,), float("nan"), dtype=torch.float32, device=self.device)
        self._check(self.lib.pg_op_token_logprob(self.h, self._p(x), B, V, self._p(t), float(temperature), self._p(out), self.stream),
                    "pg_op_token_logprob")
        self._keep = [x, t, out]
        return out

    # ------------------------------------------------------------------ scoring given text
    def score_tokens(self, hidden: torch.Tensor, target: torch.Tensor, row_idx: Optional[torch.Tensor] = None,
                     temperature: float = 0.0) -> torch.Tensor:
        """``pg_score_tokens``: log softmax(lm_head(hidden[row_idx[i]]) / temperature)[target[i]] -> fp32 [n]; ``hidden`` [..., hidden] in
        the compute dtype (what ``prefill*(return_hidden=True, hidden_dtype=engine.tdtype)`` returns), logits never materialised."""
        if hidden.dtype != self.tdtype:
            raise PlanGenError(f"score_tokens: hidden must be {self.tdtype} (the compute dtype), got {hidden.dtype}")
        h = self._dev(hidden).reshape(-1, hidden.shape[-1])
        t = self._dev(torch.as_tensor(target), torch.int32).reshape(-1)
        ri = self._dev(torch.as_tensor(row_idx), torch.int32).reshape(-1) if row_idx is not None else None
        if ri is not None and ri.numel() != t.numel():
            raise PlanGenError(f"score_tokens: {ri.numel()} row indices for {t.numel()} targets")
        out = torch.full((t.numel(),), float("nan"), dtype=torch.float32, device=self.device)
        self._check(self.lib.pg_score_tokens(self.h, self._p(h), _dt(h), h.shape[0], self._p(ri), self._p(t), t.numel(), float(temperature),
                                             self._p(out), self.stream), "pg_score_tokens")
        self._keep = [h, t, ri, out]
        return out

    def head_logprob(self, x: torch.Tensor, w: torch.Tensor, target: torch.Tensor, row_idx: Optional[torch.Tensor] = None,
                     temperature: float = 0.0) -> torch.Tensor:
        """``pg_op_head_logprob``: the device code of ``score_tokens`` on caller-given weights: x [rows, K], w [V, K] (converted to the
        compute dtype), target [n], row_idx [n] or None (rows 0 .. n-1) -> fp32 [n]."""
        x = self._dev(x, self.tdtype)
        w = self._dev(w, self.tdtype)
        rows, K = x.shape
        V = w.shape[0]
        t = self._dev(torch.as_tensor(target), torch.int32).reshape(-1)
        ri = self._dev(torch.as_tensor(row_idx), torch.int32).reshape(-1) if row_idx is not None else None
        out = torch.full((t.numel(),), float("nan"), dtype=torch.float32, device=self.device)
        self._check(self.lib.pg_op_head_logprob(self.h, self._p(x), rows, self._p(w), V, K, self._p(ri), self._p(t), t.numel(),
                                                float(temperature), self._p(out), self.stream), "pg_op_head_logprob")
        self._keep = [x, w, t, ri, out]
        return out

    def _score_hidden(self, hidden: torch.Tensor, target_ids: torch.Tensor, pad_len, score_from, temperature: float) -> torch.Tensor:
        R, L = target_ids.shape
        sel = score_index(L, pad_len, score_from, device=self.device)
        out = torch.zeros((R, L), dtype=torch.float32, device=self.device)
        if sel.numel():
            tgt = target_ids.reshape(-1).index_select(0, sel)
            lp = self.score_tokens(hidden, tgt, sel - 1, temperature)
            out.view(-1).index_copy_(0, sel, lp)
        return out

    def score_text(self, ids: torch.Tensor, pad_len: Sequence[int], score_from: Sequence[int], position_mode: int = 1,
                   temperature: float = 0.0) -> torch.Tensor:
        """Teacher-forced log-probabilities of given text in one prefill.  ``ids`` [R, L] left-padded (``pad_len``); column j of row r is
        scored from the hidden state at column j - 1, only columns j >= score_from[r] are scored (score_from[r] >= pad_len[r] + 1, else
        ValueError).  Returns fp32 [R, L]: log softmax(lm_head(h[r, j-1]) / temperature)[ids[r, j]] at the scored columns and 0.0
        elsewhere, so a row's sum is the log-probability of its scored span (the text loop's convention for finished rows).  The engine
        is left prefilled with ``ids``."""
        score_index(ids.shape[1], pad_len, score_from)      # validate before anything is launched
        ids = self._dev(ids, torch.int32)
        hid = self.prefill(ids, pad_len, position_mode=position_mode, return_hidden=True, hidden_dtype=self.tdtype)
        return self._score_hidden(hid, ids, pad_len, score_from, temperature)

    def score_text_embeds(self, embeds: torch.Tensor, pad_len: Sequence[int], target_ids: torch.Tensor, score_from: Sequence[int],
                          position_mode: int = 1, temperature: float = 0.0) -> torch.Tensor:
        """``score_text`` through ``pg_prefill_embeds``: ``embeds`` [R, L, hidden] is the input sequence (text and image embeddings, the
        ``mmu`` prompt) and ``target_ids`` [R, L] the token at every column (only the scored columns are read)."""
        score_index(target_ids.shape[1], pad_len, score_from)
        tgt = self._dev(target_ids, torch.int32)
        hid = self.prefill_embeds(embeds, pad_len, position_mode=position_mode, return_hidden=True, hidden_dtype=self.tdtype)
        return self._score_hidden(hid, tgt, pad_len, score_from, temperature)

    # ------------------------------------------------------------------ scoring given images
    def _cfg_score_args(self, what, target, cond_idx, uncond_idx):
        t = self._dev(torch.as_tensor(target), torch.int32).reshape(-1)
        ci = self._dev(torch.as_tensor(cond_idx), torch.int32).reshape(-1)
        ui = self._dev(torch.as_tensor(uncond_idx), torch.int32).reshape(-1)
        if ci.numel() != t.numel() or ui.numel() != t.numel():
            raise PlanGenError(f"{what}: {ci.numel()} cond / {ui.numel()} uncond indices for {t.numel()} targets")
        return t, ci, ui, torch.full((t.numel(),), float("nan"), dtype=torch.float32, device=self.device)

    def cfg_head_logprob(self, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], target: torch.Tensor, cond_idx: torch.Tensor,
                         uncond_idx: torch.Tensor, cfg_weight: float = 5.0, temperature: float = 1.0) -> torch.Tensor:
        """``pg_op_cfg_head_logprob``: log softmax((yu + cfg_weight * (yc - yu)) / temperature)[target[i]] with yc / yu = x[cond_idx[i]] /
        x[uncond_idx[i]] . w^T + bias -> fp32 [n]; x [rows, K] and w [V, K] are converted to the compute dtype, bias fp32 [V] or None."""
        x = self._dev(x, self.tdtype)
        w = self._dev(w, self.tdtype)
        b = self._dev(bias, torch.float32).reshape(-1) if bias is not None else None
        rows, K = x.shape
        V = w.shape[0]
        if b is not None and b.numel() != V:
            raise PlanGenError(f"cfg_head_logprob: bias has {b.numel()} entries for V={V}")
        t, ci, ui, out = self._cfg_score_args("cfg_head_logprob", target, cond_idx, uncond_idx)
        self._check(self.lib.pg_op_cfg_head_logprob(self.h, self._p(x), rows, self._p(w), V, K, self._p(b), self._p(ci), self._p(ui), self._p(t),
                                                    t.numel(), float(cfg_weight), float(temperature), self._p(out), self.stream),
                    "pg_op_cfg_head_logprob")
        self._keep = [x, w, b, t, ci, ui, out]
        return out

    def score_image_tokens(self, hidden: torch.Tensor, target: torch.Tensor, cond_idx: torch.Tensor, uncond_idx: torch.Tensor,
                           cfg_weight: float = 5.0, temperature: float = 1.0) -> torch.Tensor:
        """``pg_score_image_tokens``: the guided log-probability of image token target[i] from the hidden rows cond_idx[i] / uncond_idx[i] of
        ``hidden`` [..., hidden] (compute dtype): gen_head on every row of ``hidden``, CFG mix, temperature, log-softmax -> fp32 [n]."""
        if hidden.dtype != self.tdtype:
            raise PlanGenError(f"score_image_tokens: hidden must be {self.tdtype} (the compute dtype), got {hidden.dtype}")
        h = self._dev(hidden).reshape(-1, hidden.shape[-1])
        t, ci, ui, out = self._cfg_score_args("score_image_tokens", target, cond_idx, uncond_idx)
        self._check(self.lib.pg_score_image_tokens(self.h, self._p(h), _dt(h), h.shape[0], self._p(ci), self._p(ui), self._p(t), t.numel(),
                                                   float(cfg_weight), float(temperature), self._p(out), self.stream), "pg_score_image_tokens")
        self._keep = [h, t, ci, ui, out]
        return out

    def score_image_max_tokens(self) -> int:
        """Largest number of packed tokens (rows x columns, pads excluded) ``score_image`` sends through one prefill: every per-token buffer of
        the prefill -- the widest is the fp32 gate|up tensor, 2 * inter floats per token -- stays below 2^31 BYTES, so no index of any kernel on
        the way can pass 2^31 whatever unit it counts in."""
        c = self.cfg
        widest = max(2 * int(c.inter), 3 * int(c.n_heads) * int(c.head_dim), int(c.hidden), int(c.gen_head_dim))
        return (2 ** 31 - 1) // (4 * widest)

    def score_image(self, ids: torch.Tensor, pad_len: Sequence[int], codes: torch.Tensor, cfg_weight: float = 5.0,
                    temperature: float = 1.0) -> torch.Tensor:
        """Teacher-forced log-probabilities of given image tokens under the guided distribution the image sampler draws from, in ONE
        prefill instead of the 576-step loop.  ``ids`` int [2B, L]: the CFG-interleaved left-padded prompts ``prefill`` takes (``pad_len``
        [2B]); ``codes`` int [B, T]: the image tokens.  Returns fp32 [B, T]: log softmax((u + cfg_weight * (c - u)) / temperature)[codes[b, j]]
        with c / u the gen_head logits of rows 2b / 2b + 1 after [prompt | codes[b, :j]] -- what ``decode_image_tokens(force_tokens=codes,
        force_mask=zeros, return_logprobs=True)`` returns.  Needs max_prompt >= L + T - 1 and at most ``score_image_max_tokens()`` packed
        tokens (PlanGenError otherwise).  The engine is left prefilled with the L + T - 1 columns."""
        codes, emb = self._image_prefix_embeds("score_image", ids, pad_len, codes)
        R, L = ids.shape
        B, T = codes.shape
        cond, uncond = image_score_index(L, T, R, device=self.device)
        hid = self.prefill_embeds(emb, pad_len, position_mode=0, return_hidden=True, hidden_dtype=self.tdtype)
        return self.score_image_tokens(hid, codes.reshape(-1), cond, uncond, cfg_weight, temperature).view(B, T)

    def _image_prefix_embeds(self, who: str, ids: torch.Tensor, pad_len: Sequence[int], codes: torch.Tensor):
        """What ``score_image`` and ``attribute_image`` send through their one prefill: the checks and limits they share, then (codes int32
        [B, T] on the device, fp32 [2B, L + T - 1, hidden] = [embed(prompt) | gen_embed(codes[:, :T-1]) on both rows of a pair])."""
        if ids.dim() != 2 or ids.shape[0] < 2 or ids.shape[0] % 2:
            raise PlanGenError(f"{who}: ids must be [2B, L] with CFG-interleaved rows (got {tuple(ids.shape)})")
        R, L = ids.shape
        B = R // 2
        if codes.dim() != 2 or codes.shape[0] != B or codes.shape[1] < 1:
            raise PlanGenError(f"{who}: codes must be [B, T] = [{B}, T >= 1] for {R} prompt rows (got {tuple(codes.shape)})")
        if len(pad_len) != R:
            raise PlanGenError(f"{who}: {len(pad_len)} pad lengths for {R} rows")
        T = codes.shape[1]
        W = L + T - 1
        longest = W - min(int(p) for p in pad_len)
        if longest > self.max_prompt:
            raise PlanGenError(f"{who}: [prompt | image tokens] is {longest} tokens long: the engine needs max_prompt >= {longest} (it has {self.max_prompt})")
        ntok = sum(W - int(p) for p in pad_len)
        if ntok > self.score_image_max_tokens():
            raise PlanGenError(f"{who}: {ntok} packed tokens in one prefill exceed the limit of {self.score_image_max_tokens()}: score fewer images per call")
        codes = self._dev(codes, torch.int32)
        emb = torch.empty((R, W, self.cfg.hidden), dtype=torch.float32, device=self.device)
        emb[:, :L] = self.embed_tokens(ids)
        if T > 1:
            emb[:, L:] = self.gen_embed(codes[:, :T - 1]).view(B, T - 1, -1).repeat_interleave(2, dim=0)      # the same tokens on both rows of a pair
        return codes, emb

    # ------------------------------------------------------------------ attention mass on prompt spans
    def attn_span_mass(self, q: torch.Tensor, k: torch.Tensor, row_off: Sequence[int], length: Sequence[int], pad_len: Sequence[int],
                       lo, hi, q_col0: int, n_q: int, scale: Optional[float] = None) -> torch.Tensor:
        """``pg_op_attn_span_mass``: the span kernel on caller-given tensors, one layer.  ``q`` bf16 [tokens, nh * 128] packed (row r's slot j
        at token row_off[r] + j), ``k`` bf16 [R, nh, slots, 128], ``row_off`` / ``length`` / ``pad_len`` [R], ``lo`` / ``hi`` int [R, S] span
        bounds in columns (column = slot + pad_len[r]) -> fp32 [R, n_q, S], the attention mass of query columns [q_col0, q_col0 + n_q) on
        every span, mean over heads (definition: include/plangen_hip.h).  scale defaults to 1 / sqrt(128)."""
        q = self._dev(q, torch.bfloat16)
        k = self._dev(k, torch.bfloat16)
        if k.dim() != 4 or k.shape[3] != 128 or q.dim() != 2 or q.shape[1] != k.shape[1] * 128:
            raise PlanGenError(f"attn_span_mass: q must be [tokens, nh * 128] and k [R, nh, slots, 128] (got {tuple(q.shape)} / {tuple(k.shape)})")
        R, nh, slots, _ = k.shape
        lo_t = torch.as_tensor(lo).to(torch.int32).reshape(R, -1)
        hi_t = torch.as_tensor(hi).to(torch.int32).reshape(R, -1)
        S = lo_t.shape[1]
        if hi_t.shape != lo_t.shape or len(row_off) != R or len(length) != R or len(pad_len) != R:
            raise PlanGenError("attn_span_mass: row_off / length / pad_len must have R entries and lo / hi the same [R, S] shape")
        for r in range(R):      # the kernel trusts these: check them where they are still host numbers
            if int(length[r]) < 0 or int(length[r]) > slots or (int(row_off[r]) >= 0 and int(row_off[r]) + int(length[r]) > q.shape[0]):
                raise PlanGenError(f"attn_span_mass: row {r}: length {int(length[r])} / row_off {int(row_off[r])} leave k's {slots} slots or q's {q.shape[0]} tokens")
        dv = [self._dev(torch.as_tensor([int(v) for v in x], dtype=torch.int32)) for x in (row_off, length, pad_len)]
        lo_d, hi_d = self._dev(lo_t), self._dev(hi_t)
        out = torch.full((R, max(int(n_q), 0), S), float("nan"), dtype=torch.float32, device=self.device)
        sc = float(scale) if scale is not None else 128.0 ** -0.5
        self._check(self.lib.pg_op_attn_span_mass(self.h, self._p(q), self._p(k), self._p(dv[0]), self._p(dv[1]), self._p(dv[2]), self._p(lo_d),
                                                  self._p(hi_d), R, nh, slots, S, int(q_col0), int(n_q), sc, self._p(out), self.stream),
                    "pg_op_attn_span_mass")
        self._keep = [q, k, dv, lo_d, hi_d, out]
        return out

    def attribute_image(self, ids: torch.Tensor, pad_len: Sequence[int], codes: torch.Tensor, lo, hi, layers=None) -> torch.Tensor:
        """Attention mass of the query positions that PREDICT the image tokens on prompt spans, in the one teacher-forced prefill
        ``score_image`` runs: ``ids`` int [2B, L] / ``pad_len`` [2B] / ``codes`` int [B, T] as there; ``lo`` / ``hi`` int [B, S] (S in
        1..16): span s of image b is the prompt columns [lo, hi) of its CONDITIONAL row 2b.  Returns fp32 [n_layers_sel, B, T, S]: entry
        [l, b, j, s] is the share of attention (mean over heads, layer layers[l], ascending; None: all) that column L - 1 + j of row 2b
        -- the query that produced image token j, the row ``image_score_index`` names -- puts on span s.  Same limits and errors as
        ``score_image``; the engine is left prefilled with the L + T - 1 columns."""
        codes, emb = self._image_prefix_embeds("attribute_image", ids, pad_len, codes)
        R, L = ids.shape
        B, T = codes.shape
        lo_t = torch.as_tensor(lo).to("cpu", torch.int32)
        hi_t = torch.as_tensor(hi).to("cpu", torch.int32)
        if lo_t.dim() != 2 or lo_t.shape[0] != B or lo_t.shape != hi_t.shape:
            raise PlanGenError(f"attribute_image: lo / hi must both be [B, S] = [{B}, S] (got {tuple(lo_t.shape)} / {tuple(hi_t.shape)})")
        S = lo_t.shape[1]
        lo_r = torch.zeros((R, S), dtype=torch.int32)      # unconditional rows: empty spans
        hi_r = torch.zeros((R, S), dtype=torch.int32)
        lo_r[0::2], hi_r[0::2] = lo_t, hi_t
        _, mass = self.prefill_embeds(emb, pad_len, position_mode=0, attn_spans=(lo_r, hi_r, L - 1, T, layers))
        return mass[:, 0::2].contiguous()

    def generate_text(self, max_new_tokens: int, eos_id: int, min_new_tokens: int = 0, temperature: float = 0.0, top_k: int = 0,
                      top_p: float = 1.0, seed: int = 0, return_logits: bool = False, return_logprobs: bool = False, return_stats=False):
        """The text decode loop after a ``prefill*(position_mode=1)``: new tokens only, int64 [R, n <= max_new_tokens], finished rows
        padded with eos.  temperature <= 0: greedy (``generate_text_greedy``, bit for bit).  temperature > 0: sampled in HF's order
        (min_new EOS suppression -> temperature -> top-k -> top-p -> draw), keyed on (seed, row + the ``rng_image_offset`` option, step):
        a row's tokens do not depend on the other rows, and two rows that carry the same prompt draw different texts.
        return_logits: also fp32 [n, R, vocab], the logits every emitted token was drawn from.  return_logprobs: also fp32 [R, n], every
        emitted token's log-probability (0.0 once a row has finished, so a row's sum is its sequence log-probability).  return_stats
        (True, or an int n_alt): also (last) the ``_request_stats`` dict over [R, n].  Semantics: include/plangen_hip.h."""
        out = torch.full((self.R, max_new_tokens), eos_id, dtype=torch.int64, device=self.device)
        lg = torch.zeros((max_new_tokens, self.R, self.cfg.vocab), dtype=torch.float32, device=self.device) if return_logits else None
        lp = self._request_logprobs((self.R, max_new_tokens)) if return_logprobs else None
        stt = self._request_stats((self.R, max_new_tokens), return_stats) if _wants_stats(return_stats) else None
        n = C.c_int(0)
        self._check(self.lib.pg_generate_text_sampled(self.h, max_new_tokens, min_new_tokens, eos_id, float(temperature), int(top_k),
                                                      float(top_p), int(seed), self._p(out), C.byref(n), self._p(lg), self.stream),
                    "pg_generate_text_sampled")
        self._keep = [out, lg, lp, stt]
        res = (out[:, :n.value],) + ((lg[:n.value],) if return_logits else ()) + ((lp[:, :n.value],) if return_logprobs else ()) \
            + (({k: v[:, :n.value] for k, v in stt.items()},) if stt is not None else ())
        return res if len(res) > 1 else res[0]

    def set_text_dfa(self, dfa) -> None:
        """pg_set_text_dfa: upload a token automaton (``grammar.TokenDFA`` or anything with ``token_class`` [vocab], ``next_state``
        [n_states, n_classes], ``dist`` [n_states], ``start_state``) for ``generate_text_constrained`` / ``text_constrain``; None forgets it.
        The tables are validated and copied inside the call.  ``uploaded_dfa`` remembers the object, so that callers which pass the same
        cached automaton again (``language_model.generate(dfa=)``) can skip the upload."""
        self.uploaded_dfa = None
        if dfa is None:
            self._check(self.lib.pg_set_text_dfa(self.h, None, self.stream), "pg_set_text_dfa")
            return
        import numpy as np
        cls = np.ascontiguousarray(dfa.token_class, dtype=np.int16).reshape(-1)
        nxt = np.ascontiguousarray(dfa.next_state, dtype=np.int16)
        dist = np.ascontiguousarray(dfa.dist, dtype=np.int32).reshape(-1)
        if cls.shape[0] != self.cfg.vocab or nxt.ndim != 2 or dist.shape[0] != nxt.shape[0]:
            raise PlanGenError(f"set_text_dfa: token_class {cls.shape} must be [vocab={self.cfg.vocab}], next_state {nxt.shape} "
                               f"[n_states, n_classes], dist {dist.shape} [n_states]")
        d = _lib.pg_text_dfa(cls.ctypes.data, nxt.ctypes.data, dist.ctypes.data, nxt.shape[0], nxt.shape[1], int(dfa.start_state))
        self._check(self.lib.pg_set_text_dfa(self.h, C.byref(d), self.stream), "pg_set_text_dfa")
        self.uploaded_dfa = dfa

    def generate_text_constrained(self, max_new_tokens: int, eos_id: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                                  seed: int = 0, return_logits: bool = False, return_state: bool = False, return_logprobs: bool = False,
                                  return_stats=False):
        """``generate_text`` under the automaton of ``set_text_dfa``: disallowed tokens are -inf before temperature / top-k / top-p, a row
        only moves to states it can still finish from, so every row ends with eos inside ``max_new_tokens`` (needs dist[start] <=
        max_new_tokens).  return_logits: also the masked rows fp32 [n, R, vocab]; return_state: also the final states int32 [R];
        return_logprobs: also (last) fp32 [R, n], every emitted token's log-probability over the ALLOWED tokens (0.0 once a row has
        finished); return_stats (True, or an int n_alt): also (after it) the ``_request_stats`` dict over [R, n], masked tokens never
        among the alternatives.  Semantics: include/plangen_hip.h."""
        out = torch.full((self.R, max_new_tokens), eos_id, dtype=torch.int64, device=self.device)
        lg = torch.zeros((max_new_tokens, self.R, self.cfg.vocab), dtype=torch.float32, device=self.device) if return_logits else None
        st = torch.full((self.R,), -1, dtype=torch.int32, device=self.device) if return_state else None
        lp = self._request_logprobs((self.R, max_new_tokens)) if return_logprobs else None
        stt = self._request_stats((self.R, max_new_tokens), return_stats) if _wants_stats(return_stats) else None
        n = C.c_int(0)
        self._check(self.lib.pg_generate_text_constrained(self.h, max_new_tokens, eos_id, float(temperature), int(top_k), float(top_p),
                                                          int(seed), self._p(out), C.byref(n), self._p(st), self._p(lg), self.stream),
                    "pg_generate_text_constrained")
        self._keep = [out, lg, st, lp, stt]
        res = (out[:, :n.value],) + ((lg[:n.value],) if return_logits else ()) + ((st,) if return_state else ()) \
            + ((lp[:, :n.value],) if return_logprobs else ()) + (({k: v[:, :n.value] for k, v in stt.items()},) if stt is not None else ())
        return res if len(res) > 1 else res[0]

    def generate_text_greedy(self, max_new_tokens: int, eos_id: int, min_new_tokens: int = 0) -> torch.Tensor:
        out = torch.full((self.R, max_new_tokens), eos_id, dtype=torch.int64, device=self.device)
        n = C.c_int(0)
        self._check(self.lib.pg_generate_text_greedy(self.h, max_new_tokens, min_new_tokens, eos_id, self._p(out),
                                                     C.byref(n), self.stream), "pg_generate_text_greedy")
        return out[:, :n.value]

    # ------------------------------------------------------------------ VQ
    def vq_decode(self, codes: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        codes = self._dev(codes, torch.int32)
        B = codes.shape[0]
        S = self.cfg.img_size
        out = torch.empty((B, 3, S, S), dtype=dtype, device=self.device)
        self._check(self.lib.pg_vq_decode(self.h, self._p(codes), self._p(out), _dt(out), B, self.stream), "pg_vq_decode")
        self._keep = [codes]
        return out

    def vq_encode(self, img: torch.Tensor) -> torch.Tensor:
        img = self._dev(img)
        B = img.shape[0]
        out = torch.empty((B * self.cfg.img_tokens,), dtype=torch.int64, device=self.device)
        self._check(self.lib.pg_vq_encode(self.h, self._p(img), _dt(img), self._p(out), B, self.stream), "pg_vq_encode")
        self._keep = [img]
        return out

    def vision_encode(self, images: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        """aligner(vision_model(images)): [B,3,S,S] -> [B, P, hidden] (modeling_vlm.py:243-250)."""
        images = self._dev(images)
        B = images.shape[0]
        out = torch.empty((B, self.cfg.vit_tokens, self.cfg.hidden), dtype=dtype, device=self.device)
        self._check(self.lib.pg_vision_encode(self.h, self._p(images), _dt(images), self._p(out), _dt(out), B, self.stream),
                    "pg_vision_encode")
        self._keep = [images]
        return out

    def preprocess_images(self, images, out_size: int, min_size: int = 14, mean=(0.48145466, 0.4578275, 0.40821073),
                          std=(0.26862954, 0.26130258, 0.27577711), rescale_factor: float = 1.0 / 255.0, dtype=torch.float32,
                          background=None, do_normalize: bool = True, lut=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``pg_preprocess_images``: the reference's VLMImageProcessor (image_processing_vlm.py:127-192) on the device.  ``images``: a list of
        uint8 [H, W, 3] tensors or arrays of any sizes (host ones are copied to the device; device tensors with non-contiguous ROWS are
        passed by their row stride, not copied) -> [B, 3, out_size, out_size] ``dtype`` (float32 / bfloat16).  ``background`` defaults to
        the reference's ``int(mean * 255)``; ``lut`` (float32 [3, 256]) replaces the rescale / normalise table and ``out`` the freshly allocated result (tests)."""
        from .imageproc import background_of, make_lut
        devs = []
        for im in images:
            t = im if isinstance(im, torch.Tensor) else torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise TypeError(f"preprocess_images needs uint8 [H, W, 3] images (got {t.dtype} {tuple(t.shape)})")
            t = t.to(self.device)
            if t.numel() and (t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 0):      # pixels must be packed RGB; only the rows may be strided
                t = t.contiguous()
            devs.append(t)
        B = len(devs)
        descs = (_lib.pg_image_u8 * max(1, B))()
        for d, t in zip(descs, devs):
            d.pix_dev, d.height, d.width, d.row_stride = t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else t.shape[1] * 3
        table = make_lut(mean, std, rescale_factor, do_normalize) if lut is None else lut
        table = torch.as_tensor(table, dtype=torch.float32).cpu().contiguous()
        if tuple(table.shape) != (3, 256):
            raise TypeError("lut must be float32 [3, 256]")
        bg = (C.c_uint8 * 3)(*[int(v) for v in (background_of(mean) if background is None else background)])
        if out is None:
            out = torch.empty((B, 3, out_size, out_size), dtype=dtype, device=self.device)
        elif tuple(out.shape) != (B, 3, out_size, out_size) or not out.is_contiguous() or out.device != self.device:
            raise TypeError(f"out must be a contiguous [{B}, 3, {out_size}, {out_size}] tensor on {self.device}")
        self._check(self.lib.pg_preprocess_images(self.h, descs, B, int(out_size), int(min_size), bg, C.cast(table.data_ptr(), C.POINTER(C.c_float)),
                                                  self._p(out), _dt(out), self.stream), "pg_preprocess_images")
        self._keep = devs
        return out

    # ------------------------------------------------------------------ test taps
    def debug_read(self, name: str, index: int, numel: int, dtype) -> torch.Tensor:
        """Debug taps (include/plangen_hip.h).  With kv_dtype 'fp8', "kcache" / "vcache" are the uint8 codes (pass dtype=torch.uint8) and
        "kscale" / "vscale" the fp32 scales [max_rows, heads, slots]."""
        out = torch.zeros((numel,), dtype=dtype, device=self.device)       # the library copies min(numel, buffer size): the rest stays zero
        self._check(self.lib.pg_debug_read(self.h, name.encode(), index, self._p(out), out.numel() * out.element_size(),
                                           self.stream), "pg_debug_read")
        return out

    def op_kv_quantize(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """pg_op_kv_quantize: the FP8 KV cache's quantiser over bf16 rows ``x`` [n, 128] -> (codes uint8 [n, 128], scale fp32 [n])."""
        x = self._dev(x, torch.bfloat16).reshape(-1, 128).contiguous()
        n = x.shape[0]
        codes = torch.zeros((n, 128), dtype=torch.uint8, device=self.device)
        scale = torch.zeros((n,), dtype=torch.float32, device=self.device)
        self._check(self.lib.pg_op_kv_quantize(self.h, self._p(x), self._p(codes), self._p(scale), n, self.stream), "pg_op_kv_quantize")
        torch.cuda.synchronize()
        return codes, scale

    def op_rmsnorm(self, x: torch.Tensor, w: torch.Tensor, eps: float, partial: Optional[torch.Tensor] = None):
        x = self._dev(x, torch.float32).clone()
        M, H = x.shape
        w = self._dev(w, self.tdtype)
        S = 0 if partial is None else partial.shape[0]
        part = self._dev(partial, torch.float32) if partial is not None else None
        out = torch.empty((M, H), dtype=self.tdtype, device=self.device)
        self._check(self.lib.pg_op_rmsnorm(self.h, self._p(x), self._p(part), S, self._p(w), self._p(out), M, H, eps, self.stream), "pg_op_rmsnorm")
        torch.cuda.synchronize()
        return x, out

    def op_gemm(self, a: torch.Tensor, w: torch.Tensor, kind: int = 0) -> torch.Tensor:
        a = self._dev(a, self.tdtype)
        w = self._dev(w, self.tdtype)
        M, K = a.shape
        N = w.shape[0]
        out = torch.zeros((64, M, N), dtype=torch.float32, device=self.device)
        S = C.c_int(0)
        self._check(self.lib.pg_op_gemm(self.h, self._p(a), self._p(w), self._p(out), M, N, K, kind, C.byref(S), self.stream), "pg_op_gemm")
        torch.cuda.synchronize()
        return out[:S.value].sum(0)

    def op_gemm_splits(self, a: torch.Tensor, w: torch.Tensor) -> int:
        """Split-K slab count the decode GEMM picks for this shape under THIS handle's tuning."""
        a = self._dev(a, self.tdtype); w = self._dev(w, self.tdtype)
        M, K = a.shape
        N = w.shape[0]
        out = torch.zeros((64, M, N), dtype=torch.float32, device=self.device)
        S = C.c_int(0)
        self._check(self.lib.pg_op_gemm(self.h, self._p(a), self._p(w), self._p(out), M, N, K, 1, C.byref(S), self.stream), "pg_op_gemm")
        torch.cuda.synchronize()
        return S.value

    def op_swiglu_gemm(self, a: torch.Tensor, w_gate: torch.Tensor, w_up: torch.Tensor) -> torch.Tensor:
        """down-proj input of LlamaMLP: silu(a @ w_gate^T) * (a @ w_up^T) through the decode kernel (tiled weights,
        SwiGLU epilogue).  The gate/up rows are interleaved in blocks of 8 here, like pg_load_tensor does."""
        a = self._dev(a, torch.bfloat16)
        I, K = w_gate.shape
        wgu = torch.stack([w_gate.reshape(I // 8, 8, K), w_up.reshape(I // 8, 8, K)], dim=1).reshape(2 * I, K)
        wgu = self._dev(wgu, torch.bfloat16)
        M = a.shape[0]
        out = torch.empty((M, I), dtype=torch.bfloat16, device=self.device)
        self._check(self.lib.pg_op_swiglu_gemm(self.h, self._p(a), self._p(wgu), self._p(out), M, I, K, self.stream), "pg_op_swiglu_gemm")
        torch.cuda.synchronize()
        return out

    def op_uniform(self, bits: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(u, gumbel) the sampler derives from raw 64-bit RNG outputs (int64 tensor = the bit patterns)."""
        b = self._dev(bits.reshape(-1), torch.int64)
        n = b.numel()
        out = torch.empty((2 * n,), dtype=torch.float32, device=self.device)
        self._check(self.lib.pg_op_uniform(self.h, self._p(b), self._p(out), n, self.stream), "pg_op_uniform")
        torch.cuda.synchronize()
        return out[:n], out[n:]

    def sample_filter(self, logits: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
        """pg_op_sample_filter: kept mask (bool [B, V]) of the top-k / top-p sampler over fp32 rows ``logits`` [B, V]."""
        x = self._dev(logits, torch.float32).reshape(-1, logits.shape[-1]).contiguous()
        B, V = x.shape
        keep = torch.zeros((B, V), dtype=torch.uint8, device=self.device)
        self._check(self.lib.pg_op_sample_filter(self.h, self._p(x), B, V, float(temperature), int(top_k), float(top_p),
                                                 self._p(keep), self.stream), "pg_op_sample_filter")
        self._keep = [x, keep]
        return keep.bool().reshape(logits.shape)

    def text_sample(self, logits: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                    row_offset: int = 0, step: int = 0):
        """pg_op_text_sample: the text sampler's selection and draw over fp32 rows ``logits`` [B, V], V <= vocab ->
        (kept mask bool [B, V], drawn token int32 [B]) for the keys (seed, row + row_offset, step)."""
        x = self._dev(logits, torch.float32).reshape(-1, logits.shape[-1]).contiguous()
        B, V = x.shape
        keep = torch.zeros((B, V), dtype=torch.uint8, device=self.device)
        tok = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        self._check(self.lib.pg_op_text_sample(self.h, self._p(x), B, V, float(temperature), int(top_k), float(top_p), int(seed),
                                               int(row_offset), int(step), self._p(keep), self._p(tok), self.stream), "pg_op_text_sample")
        self._keep = [x, keep, tok]
        return keep.bool(), tok

    def text_constrain(self, logits: torch.Tensor, state, remaining: int, eos_id: int, temperature: float = 0.0, top_k: int = 0,
                       top_p: float = 1.0, seed: int = 0, row_offset: int = 0, step: int = 0):
        """pg_op_text_constrain: one constrained step over fp32 rows ``logits`` [B, V], V <= vocab, in the states ``state`` [B] ->
        (kept mask bool [B, V], token int32 [B], next state int32 [B])."""
        x = self._dev(logits, torch.float32).reshape(-1, logits.shape[-1]).contiguous()
        B, V = x.shape
        st = self._dev(torch.as_tensor(state), torch.int32).reshape(-1).contiguous()
        keep = torch.zeros((B, V), dtype=torch.uint8, device=self.device)
        tok = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        nxt = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        self._check(self.lib.pg_op_text_constrain(self.h, self._p(x), B, V, self._p(st), int(remaining), int(eos_id), float(temperature),
                                                  int(top_k), float(top_p), int(seed), int(row_offset), int(step), self._p(keep),
                                                  self._p(tok), self._p(nxt), self.stream), "pg_op_text_constrain")
        self._keep = [x, st, keep, tok, nxt]
        return keep.bool(), tok, nxt

    def op_conv3x3(self, x_nhwc: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, residual=None, up: int = 0,
                   stride2: int = 0) -> torch.Tensor:
        x = self._dev(x_nhwc, self.tdtype)
        B, Hi, Wi, Cin = x.shape
        Cout = w_oihw.shape[0]
        w = self._dev(w_oihw.permute(0, 2, 3, 1).reshape(Cout, 9, Cin), self.tdtype)   # [Cout][tap][Cin]
        b = self._dev(bias, torch.float32)
        Ho, Wo = (Hi // 2, Wi // 2) if stride2 else (Hi << up, Wi << up)
        r = self._dev(residual, self.tdtype) if residual is not None else None
        out = torch.empty((B, Ho, Wo, Cout), dtype=self.tdtype, device=self.device)
        self._check(self.lib.pg_op_conv3x3(self.h, self._p(x), self._p(w), self._p(b), self._p(r), self._p(out), B, Hi, Wi,
                                           Cin, Cout, up, stride2, self.stream), "pg_op_conv3x3")
        torch.cuda.synchronize()
        return out

    def op_groupnorm(self, x_nhwc: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, swish: bool) -> torch.Tensor:
        x = self._dev(x_nhwc, torch.float32)          # the VQ skip stream is fp32 in both modes
        B, Hs, Ws, Cc = x.shape
        g = self._dev(gamma, torch.float32)
        b = self._dev(beta, torch.float32)
        out = torch.empty(x.shape, dtype=self.tdtype, device=self.device)
        self._check(self.lib.pg_op_groupnorm(self.h, self._p(x), self._p(g), self._p(b), self._p(out), B, Hs * Ws, Cc,
                                             int(swish), self.stream), "pg_op_groupnorm")
        torch.cuda.synchronize()
        return out
