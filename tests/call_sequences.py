"""Helpers of tests/test_gpu_call_sequences.py: private engines, seeded batches, calls as closures, and the veteran-against-fresh runner.

A *call* is a function ``call(engine) -> dict`` that sets every option it depends on, runs one complete operation (prefill + decode, a text
generation, a scoring call, ...) and returns everything the operation produced as named DEVICE tensors, the KV-cache slots it wrote included
(``read_cache``).  It fetches nothing itself, but it is not free of synchronisation: host inputs (ids, forcing tensors) are uploaded from
pageable memory, which waits for the stream, and the text loop synchronises by design.  Only ``chain_call`` stages everything first and then
issues its calls with no host synchronisation at all.  ``run_sequence`` plays a list of calls on one long-lived handle (the veteran) and,
for every checked step, the same call (or the step's ``fresh`` one) alone on a handle created for it; the two dicts must be equal bit for bit."""
import warnings
from collections import namedtuple

import pytest
import torch

from plangen_amd.engine import Engine, PlanGenError, replica_owner

MAX_ROWS, MAX_PROMPT = 8, 96
DEFAULT_OPTS = dict(use_graph=0, share_uncond=1, lanes=-1)
CFG_WEIGHT = 5.0
_OPEN = []

Step = namedtuple("Step", "name call check fresh", defaults=(True, None))
Batch = namedtuple("Batch", "ids pad lens")


# ----------------------------------------------------------------------------------------------------------------- handles
def make_engine(cfg, weights, dtype, kv_dtype="bf16", diag=False):
    """A handle of this file's own, built like conftest.get_engine's (without the VQ encoder and SigLIP, which no call here runs)."""
    e = Engine(cfg, dtype=dtype, max_rows=MAX_ROWS, max_prompt=MAX_PROMPT, max_new=cfg.img_tokens, max_images=4, with_lm_head=True,
               kv_dtype=kv_dtype, diag=diag)
    _OPEN.append(e)
    e.load_state_dict({k: v for k, v in weights.items()
                       if not k.startswith(("vision_model.", "aligner.", "gen_vision_model.encoder", "gen_vision_model.quant_conv"))})
    return e


def close_all():
    while _OPEN:
        _OPEN.pop().close()


def apply_opts(e, opts):
    """Every option a call's result may depend on, set explicitly: a call never inherits one from the call before it."""
    o = {**DEFAULT_OPTS, **(opts or {})}
    fused = o.pop("fuse_rope", 1)
    for k, v in o.items():
        e.set_option(k, v)
    if e.diag:
        e.set_diag_option("fuse_rope", fused)
    return o, bool(fused)


def bump_tune_epoch(e):
    """Moves tune_epoch twice and leaves every knob at its default (split_target_big only acts at 96 rows and more)."""
    e.set_option("split_target_big", 256)
    e.set_option("split_target_big", 128)
    return {}


# ----------------------------------------------------------------------------------------------------------------- inputs
def batch(cfg, lens, seed, L=None, shared_neg=False):
    """Left-padded ids [R, L] with ``lens[r]`` random real tokens in row r.  shared_neg: every odd row carries row 1's prompt."""
    g = torch.Generator().manual_seed(seed)
    R, L = len(lens), max(lens) if L is None else L
    ids = torch.full((R, L), cfg.pad_id, dtype=torch.int32)
    for r, n in enumerate(lens):
        ids[r, L - n:] = torch.randint(8, cfg.vocab, (n,), generator=g, dtype=torch.int32)
    if shared_neg:
        for r in range(3, R, 2):
            assert lens[r] == lens[1]
            ids[r] = ids[1]
    return Batch(ids, [L - n for n in lens], list(lens))


def codes(cfg, B, T, seed):
    return torch.randint(0, cfg.img_vocab, (B, T), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


# ----------------------------------------------------------------------------------------------------------------- KV cache
def kv_spans(lens, new, R0=None, shared=False):
    """Per row, the slots [lo, hi) the call wrote: the prompt (unless the row aliases another row's: replica_owner) and ``new`` appended
    tokens.  R0: the distinct rows of an alias = 1 replicated batch; None: every row owns its prompt unless the negative one is shared."""
    R = len(lens)
    return [(0 if replica_owner(r, R0 or R, shared) == r else lens[r], lens[r] + new) for r in range(R)]


def read_cache(e, spans):
    """K and V of every layer (FP8: codes and scales) over ``spans``, as flat device tensors."""
    cfg, out = e.cfg, {}
    nh, slots = cfg.n_heads, MAX_PROMPT + cfg.img_tokens
    n = MAX_ROWS * nh * slots
    fp8 = e.kv_dtype == "fp8"
    planes = [("kcache", 128, torch.uint8 if fp8 else e.tdtype), ("vcache", 128, torch.uint8 if fp8 else e.tdtype)]
    if fp8:
        planes += [("kscale", 1, torch.float32), ("vscale", 1, torch.float32)]
    for li in range(cfg.n_layers):
        for name, w, dt in planes:
            buf = e.debug_read(name, li, n * w, dt).view(MAX_ROWS, nh, slots, w)
            out[f"{name}[{li}]"] = torch.cat([buf[r, :, lo:hi].reshape(-1) for r, (lo, hi) in enumerate(spans)])
    return out


# ----------------------------------------------------------------------------------------------------------------- calls
def _prefill(e, b, o, fused, kind, replicas, alias, on_device, uncond_shared):
    """Runs the prefill; returns (row lengths of the batch the engine now holds, R0 for kv_spans, whether the negative prompt is shared)."""
    ids = b.ids.to(e.device) if on_device else b.ids
    lens, pad = b.lens * replicas, b.pad * replicas
    shared = False
    if kind in ("ids", "replicated", "raw"):
        shared = bool(o["share_uncond"]) and fused and len(b.lens) % 2 == 0 and Engine.uncond_rows_shared(torch.cat([b.ids] * replicas), pad)
        shared = shared and uncond_shared is not False            # the caller's "not shared" is taken at its word
    if kind == "ids":
        e.prefill(ids, b.pad, uncond_shared=uncond_shared)
    elif kind == "raw":
        # pg_prefill as a C caller issues it: no "uncond_shared_hint" option is sent, so whatever hint the handle still holds is the one it
        # uses.  Engine has no public entry point that skips the option (it always sends one, on purpose), hence the reach into its
        # plumbing (_check, _p, lib) and the book-keeping Engine.prefill does after the call (R, L, _keep), mirrored line for line.
        import ctypes as C
        dev = b.ids.to(e.device)
        R, L = dev.shape
        e._check(e.lib.pg_prefill(e.h, e._p(dev), (C.c_int32 * R)(*b.pad), R, L, 0, None, 0, e.stream), "pg_prefill")
        e.R, e.L, e._keep = R, L, [dev]
    elif kind == "replicated":
        e.prefill_replicated(ids, b.pad, replicas, alias=alias, uncond_shared=uncond_shared)
    elif kind == "embeds":
        e.prefill_embeds(e.embed_tokens(b.ids), b.pad)
    else:
        raise ValueError(kind)
    return lens, (len(b.lens) if kind == "replicated" and alias and replicas > 1 else None), shared


def prefill_only(b, opts=None, kind="ids", replicas=1, alias=True, on_device=False, uncond_shared=None):
    """A prefill whose results nobody fetches: no output, no synchronisation (history for the call that follows)."""
    def call(e):
        o, fused = apply_opts(e, opts)
        _prefill(e, b, o, fused, kind, replicas, alias, on_device, uncond_shared)
        return {}
    return call


def prefill_hidden(b, opts=None, position_mode=0):
    """pg_prefill_embeds with hidden_out: the hidden states and the prompt K/V."""
    def call(e):
        apply_opts(e, opts)
        hid = e.prefill_embeds(e.embed_tokens(b.ids), b.pad, position_mode=position_mode, return_hidden=True)
        return {"hidden": hid, **read_cache(e, kv_spans(b.lens, 0))}
    return call


def image_call(b, T, opts=None, kind="ids", replicas=1, alias=True, on_device=False, uncond_shared=None, **dk):
    """prefill (``kind``) + pg_decode_image_tokens(T, **dk): tokens, logits / log-probs / stats where asked for, and the cache."""
    def call(e):
        o, fused = apply_opts(e, opts)
        lens, R0, shared = _prefill(e, b, o, fused, kind, replicas, alias, on_device, uncond_shared)
        out = _image_outputs(e.decode_image_tokens(T=T, cfg_weight=CFG_WEIGHT, **dk), dk)
        out.update(read_cache(e, kv_spans(lens, T - 1, R0, shared)))
        return out
    return call


def _image_outputs(res, dk):
    res = list(res) if isinstance(res, tuple) else [res]
    out = {"tokens": res.pop(0)}
    if dk.get("return_logits"):
        out["logits"] = res.pop(0)
    if dk.get("return_logprobs"):
        out["logprobs"] = res.pop(0)
    if res:
        out.update({f"stats.{k}": v for k, v in res.pop(0).items()})
    return out


def chain_call(batches, T, embeds_at=None, **dk):
    """Prefills of every batch of ``batches`` issued back to back, then a decode of the last: what the call returns is the last batch's.
    Everything is put on the device first -- ids, the embeddings of batch ``embeds_at`` (which goes through pg_prefill_embeds with
    hidden_out), and the caller's own answer to "is the negative prompt shared" (so neither the host comparison nor the device probe
    runs) -- and from the first prefill to the end of the decode nothing synchronises the host with the stream: no upload, no probe, no
    fetch.  torch's sync debug mode turns any synchronising torch call in that span into an error.  ``dk`` must not hold host tensors."""
    assert embeds_at is None or embeds_at < len(batches) - 1
    def call(e):
        apply_opts(e, None)
        staged = []
        for i, b in enumerate(batches):
            dev = b.ids.to(e.device)
            staged.append((b, dev, e.embed_tokens(dev) if i == embeds_at else None, Engine.uncond_rows_shared(b.ids, b.pad)))
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)          # "prototype feature": it does catch the blocking copies this is about
            torch.cuda.set_sync_debug_mode("error")
        try:
            for b, dev, emb, sh in staged:
                if emb is not None:
                    e.prefill_embeds(emb, b.pad, return_hidden=True)
                else:
                    e.prefill(dev, b.pad, uncond_shared=sh)
            res = e.decode_image_tokens(T=T, cfg_weight=CFG_WEIGHT, **dk)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        out = _image_outputs(res, dk)
        b, _, _, sh = staged[-1]
        out.update(read_cache(e, kv_spans(b.lens, T - 1, None, sh)))
        return out
    return call


def text_call(b, n, opts=None, dfa=None, **gk):
    """prefill(position_mode 1) + pg_generate_text_sampled, or pg_set_text_dfa + pg_generate_text_constrained when ``dfa`` is given."""
    def call(e):
        apply_opts(e, opts)
        e.prefill(b.ids, b.pad, position_mode=1)
        if dfa is not None:
            e.set_text_dfa(dfa)
            res = e.generate_text_constrained(n, e.cfg.eos_id, return_state=True, **gk)
        else:
            res = e.generate_text(n, e.cfg.eos_id, **gk)
        res = list(res) if isinstance(res, tuple) else [res]
        out = {"text": res.pop(0)}
        if gk.get("return_logits"):
            out["logits"] = res.pop(0)
        if dfa is not None:
            out["state"] = res.pop(0)
        if gk.get("return_logprobs"):
            out["logprobs"] = res.pop(0)
        if res:
            out.update({f"stats.{k}": v for k, v in res.pop(0).items()})
        out.update(read_cache(e, kv_spans(b.lens, out["text"].shape[1] - 1)))
        return out
    return call


def _then_decode(e, out, T):
    """What the engine defines for a decode right after a scoring call: its tokens, or its refusal."""
    try:
        out["tokens"] = e.decode_image_tokens(T=T, cfg_weight=CFG_WEIGHT, temperature=0.0)
    except PlanGenError as ex:
        out["refusal"] = str(ex)
    return out


def score_text_call(b, score_from, opts=None, then_decode=0, temperature=0.0):
    def call(e):
        apply_opts(e, opts)
        out = {"scores": e.score_text(b.ids, b.pad, score_from, temperature=temperature)}
        out.update(read_cache(e, kv_spans(b.lens, 0)))
        return _then_decode(e, out, then_decode) if then_decode else out
    return call


def score_image_call(b, img, opts=None, then_decode=0):
    def call(e):
        apply_opts(e, opts)
        out = {"scores": e.score_image(b.ids, b.pad, img)}
        out.update(read_cache(e, kv_spans([n + img.shape[1] - 1 for n in b.lens], 0)))
        return _then_decode(e, out, then_decode) if then_decode else out
    return call


def rejected(call, why):
    """``call`` must be refused by a host-side argument check (nothing is launched); ``why``: a regular expression over "<status>): <the
    library's message>" that names the check, not only its status.  History for the call that follows."""
    def wrapped(e):
        with pytest.raises(PlanGenError, match=why):
            call(e)
        return {}
    return wrapped


def forget_dfa(e):
    e.set_text_dfa(None)
    return {}


# ----------------------------------------------------------------------------------------------------------------- comparison
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


def to_host(d):
    torch.cuda.synchronize()
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def differences(got, want):
    """Names (with a count) of the entries of two result dicts that are not bit-equal."""
    bad = []
    if sorted(got) != sorted(want):
        return [f"outputs {sorted(got)} != {sorted(want)}"]
    for k, a in got.items():
        b = want[k]
        if not isinstance(a, torch.Tensor):
            if a != b:
                bad.append(f"{k}: {a!r} != {b!r}")
            continue
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f"{k}: {tuple(a.shape)} {a.dtype} != {tuple(b.shape)} {b.dtype}")
            continue
        ai, bi = (a.view(_BITS[a.dtype]), b.view(_BITS[b.dtype])) if a.dtype in _BITS else (a, b)
        if not torch.equal(ai, bi):
            ne = ai != bi
            bad.append(f"{k}: {int(ne.sum())} of {ne.numel()} differ, first at flat index {int(ne.reshape(-1).nonzero()[0])}")
    return bad


def assert_same(got, want, what):
    bad = differences(got, want)
    assert not bad, f"{what}: the veteran handle and a fresh handle disagree -- " + "; ".join(bad)


def fresh_result(make, call):
    e = make()
    try:
        return to_host(call(e))
    finally:
        e.close()
        _OPEN.remove(e)


def run_sequence(make, steps):
    """Plays ``steps`` on one veteran handle; every checked step must equal the same call (``fresh``, where the step names one: the part of
    the veteran's call that a handle without history runs) alone on a fresh handle."""
    vet = make()
    try:
        for i, st in enumerate(steps):
            got = st.call(vet)
            if st.check:
                assert got, st.name
                assert_same(to_host(got), fresh_result(make, st.fresh or st.call), f"step {i} ({st.name})")
    finally:
        torch.cuda.synchronize()
        vet.close()
        _OPEN.remove(vet)
