"""GPU: pg_prefill_replicated (Engine.prefill_replicated, System.t2i with share_replicas = 1) -- parallel_size replicas of one CFG batch with every
prompt prefilled once.  alias = 1 (replicas read their owner's prompt K/V in the grouped decode attention) against alias = 0 (the prompt K/V
copied into every replica's row, today's decode kernels) bit for bit; both against the plain path (pg_prefill of torch.cat([ids] * p)) within the
bound the project uses for share_uncond 1 vs 0; sampling, errors, replicas = 1, and t2i against the oracle."""
import numpy as np
import pytest
import torch

from conftest import get_engine
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

ENGINES = [("f32", {}), ("bf16", {}), ("bf16", {"kv_dtype": "fp8"})]
IDS = ["f32", "bf16", "bf16-fp8"]
T = 24


def _engine(tiny_cfg, tiny_weights, dtype, kw):
    return get_engine(tiny_cfg, tiny_weights, dtype, max_rows=12, max_prompt=192, **kw)


def _batch(cfg, cond_lens, neg_lens, seed=7):
    """CFG-interleaved un-replicated batch: one shared negative prompt (neg_lens an int) or one per sample (a tuple)."""
    from plangen_amd.engine import Engine
    from plangen_amd.system import t2i_infer_collate_batch
    g = torch.Generator().manual_seed(seed)
    cond = [torch.randint(8, cfg.vocab, (n,), generator=g).tolist() for n in cond_lens]
    if isinstance(neg_lens, int):
        neg = torch.randint(8, cfg.vocab, (neg_lens,), generator=g).tolist()
    else:
        neg = [torch.randint(8, cfg.vocab, (n,), generator=g).tolist() for n in neg_lens]
    ids, mask = t2i_infer_collate_batch(cond, neg, cfg.pad_id, cfg.img_tokens)
    return ids, Engine.pad_len_from_mask(mask, ids.shape[1]), mask


def _modes(cfg, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    force = torch.randint(0, cfg.img_vocab, (B, T), generator=g, dtype=torch.int32)
    return [("greedy", dict(temperature=0.0)), ("forced", dict(temperature=0.0, force_tokens=force)),
            ("sampled", dict(temperature=1.0, top_k=20, top_p=0.9, seed=11))]


def _dirty(e, ids, pad, p):
    """Fill every row's prompt slots with ANOTHER batch's K/V (a plain prefill of other ids of the same shape), so that an alias = 1 run that read a
    replica's own (never written) prompt slots could not find the right values left there by an earlier run."""
    g = torch.Generator().manual_seed(1234)
    other = torch.randint(8, 500, ids.shape, generator=g, dtype=ids.dtype)          # pad slots are skipped by pad_len
    e.prefill(torch.cat([other] * p), pad * p, uncond_shared=False)


def _decode(e, **kw):
    toks, lg = e.decode_image_tokens(T=T, cfg_weight=5.0, return_logits=True, **kw)
    torch.cuda.synchronize()
    return toks.cpu(), lg.cpu()


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("neg", [5, (5, 12)], ids=["shared-neg", "two-negs"])
@pytest.mark.parametrize("dtype,kw", ENGINES, ids=IDS)
def test_alias_equals_copy_bit_for_bit(tiny_cfg, tiny_weights, dtype, kw, neg, use_graph):
    """R0 = 4, p = 3, cond prompts of 9 and 170 tokens: tokens and per-step logits of alias = 1 and alias = 0 are equal for greedy,
    teacher-forced and sampled (temperature 1, top_k 20, top_p 0.9) loops of 24 steps."""
    e = _engine(tiny_cfg, tiny_weights, dtype, kw)
    ids, pad, _ = _batch(tiny_cfg, (9, 170), neg)
    e.set_option("use_graph", use_graph)
    try:
        for name, m in _modes(tiny_cfg, 6):
            out = []
            for alias in (True, False):
                if alias:
                    _dirty(e, ids, pad, 3)
                e.prefill_replicated(ids, pad, 3, alias=alias)
                out.append(_decode(e, **m))
            assert torch.equal(out[0][0], out[1][0]), (name, "tokens")
            assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32)), (name, "logits")
            assert not torch.isnan(out[0][1]).any()
    finally:
        e.set_option("use_graph", 0)


@pytest.mark.parametrize("dtype,kw", ENGINES, ids=IDS)
def test_alias_equals_copy_two_rows_two_replicas(tiny_cfg, tiny_weights, dtype, kw):
    """R0 = 2, p = 2: the replicated batch has 4 rows, so the negative prompt is shared (row 3 aliases row 1) although R0 < 4."""
    e = _engine(tiny_cfg, tiny_weights, dtype, kw)
    ids, pad, _ = _batch(tiny_cfg, (33,), 6)
    for name, m in _modes(tiny_cfg, 2):
        out = []
        for alias in (True, False):
            e.prefill_replicated(ids, pad, 2, alias=alias)
            out.append(_decode(e, **m))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32)), name
    # the aliased attention byte accounting counts the prompts once: fewer algorithmic bytes than the copy
    by = []
    e.set_option("time_attn", 1)
    try:
        for alias in (True, False):
            e.prefill_replicated(ids, pad, 2, alias=alias)
            e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0)
            by.append(e.timing()["attn_bytes_sum"])
    finally:
        e.set_option("time_attn", 0)
    assert 0 < by[0] < by[1], by


@pytest.mark.parametrize("neg", [5, (5, 12)], ids=["shared-neg", "two-negs"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_replicated_equals_plain_path(tiny_cfg, tiny_weights, dtype, neg):
    """prefill_replicated(ids, pad, p) against prefill(torch.cat([ids] * p), pad * p): f32 greedy tokens equal; teacher-forced logits within the
    share_uncond 1-vs-0 bound of tests/test_gpu_path.py (1e-4 f32, 5e-2 bf16): the plain path prefills p times as many packed tokens, so its
    prefill GEMMs may split K differently."""
    e = _engine(tiny_cfg, tiny_weights, dtype, {})
    p = 3
    ids, pad, _ = _batch(tiny_cfg, (9, 170), neg)
    modes = dict(_modes(tiny_cfg, 6))
    tol = 1e-4 if dtype == "f32" else 5e-2
    for alias in (True, False):
        for name in ("greedy", "forced"):
            e.prefill(torch.cat([ids] * p), pad * p)
            ref = _decode(e, **modes[name])
            e.prefill_replicated(ids, pad, p, alias=alias)
            got = _decode(e, **modes[name])
            if dtype == "f32":
                assert torch.equal(got[0], ref[0]), (name, alias)
            if name == "forced":
                err = (got[1] - ref[1]).abs().max().item()
                print(f"replicated vs plain [{dtype}, alias={alias}]: max |dlogit| = {err:.3e}")
                assert err < tol, (alias, err)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_owner_prompt_kv_equals_plain_rows(tiny_cfg, tiny_weights, dtype):
    """Batch invariance of the prefill, asserted on its own: the prompt-slot K/V of the owner rows after prefill_replicated equal the plain
    run's rows 0 .. R0-1 bit for bit (rows that alias the shared negative prompt hold no prompt in either run); with alias = 0 the
    replicas' rows equal them too."""
    e = _engine(tiny_cfg, tiny_weights, dtype, {})
    cfg = tiny_cfg
    p, slots, nh = 3, 192 + cfg.img_tokens, cfg.n_heads
    ids, pad, _ = _batch(cfg, (9, 170), 5)
    L, R0 = ids.shape[1], ids.shape[0]
    n_el = 12 * nh * slots * 128

    def caches():
        torch.cuda.synchronize()
        return [e.debug_read(nm, li, n_el, e.tdtype).cpu().view(12, nh, slots, 128) for li in range(cfg.n_layers) for nm in ("kcache", "vcache")]
    e.prefill(torch.cat([ids] * p), pad * p)
    plain = caches()
    e.prefill_replicated(ids, pad, p, alias=False)
    rep = caches()
    bt = torch.int32 if dtype == "f32" else torch.int16
    for a, b in zip(plain, rep):
        for r in range(R0 * p):
            if r % 2 == 1 and r != 1:
                continue                                   # aliases the shared negative prompt: never written
            n = L - pad[r % R0]
            assert torch.equal(a[r, :, :n].view(bt), b[r, :, :n].view(bt)), r


@pytest.mark.parametrize("dtype,kw", ENGINES, ids=IDS)
def test_sampled_replicas_differ_and_reproduce(tiny_cfg, tiny_weights, dtype, kw):
    """Replicas of one prompt draw different images (the RNG is keyed on the global image index); the same seed reproduces, seed + 1 does
    not; f32 equals the plain path's draws; rng_image_offset shards the replicated batch like any other."""
    e = _engine(tiny_cfg, tiny_weights, dtype, kw)
    ids, pad, _ = _batch(tiny_cfg, (9, 170), 5)
    p = 3

    def run(seed, replicated=True, off=0):
        e.set_option("rng_image_offset", off)
        i, pl = ids, pad
        if replicated:
            e.prefill_replicated(i, pl, p)
        else:
            e.prefill(torch.cat([i] * p), pl * p)
        t = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=1.0, seed=seed).cpu()
        e.set_option("rng_image_offset", 0)
        return t
    a, b, c = run(5), run(5), run(6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a[0], a[2]) and not torch.equal(a[0], a[4]) and not torch.equal(a[1], a[3])      # image k, k + 2, k + 4: one prompt
    if dtype == "f32":
        assert torch.equal(a, run(5, replicated=False))
    # keyed on the GLOBAL image index (row t * R0 + r -> image t * B0 + r // 2, plus rng_image_offset): a second handle's worth of offset
    # draws other images, reproducibly, and (f32, exact) the un-replicated batch at offset t * B0 draws exactly replica t's images
    shifted = run(5, off=6)
    assert not torch.equal(a, shifted) and torch.equal(run(5, off=6), shifted)
    if dtype == "f32":
        for t in range(p):
            e.set_option("rng_image_offset", 2 * t)
            e.prefill(ids, pad)
            one = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=1.0, seed=5).cpu()
            e.set_option("rng_image_offset", 0)
            assert torch.equal(one, a[2 * t:2 * t + 2]), t


@pytest.mark.parametrize("dtype,kw", ENGINES, ids=IDS)
def test_one_replica_is_pg_prefill(tiny_cfg, tiny_weights, dtype, kw):
    e = _engine(tiny_cfg, tiny_weights, dtype, kw)
    ids, pad, _ = _batch(tiny_cfg, (9, 170), 5)
    e.prefill(ids, pad)
    ref = _decode(e, temperature=0.0)
    for alias in (True, False):
        e.prefill_replicated(ids, pad, 1, alias=alias)
        got = _decode(e, temperature=0.0)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def test_errors(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    e = _engine(tiny_cfg, tiny_weights, "bf16", {})
    ids, pad, _ = _batch(tiny_cfg, (9, 30), 5)
    with pytest.raises(PlanGenError, match="PG_ERR_CAPACITY"):
        e.prefill_replicated(ids, pad, 4)                       # 16 rows > max_rows 12
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.prefill_replicated(ids, pad, 2, alias=2)
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.prefill_replicated(ids, pad, 0)
    e.prefill_replicated(ids, pad, 2, alias=True)
    e.set_option("lanes", 2)
    try:
        with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
            e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0)
    finally:
        e.set_option("lanes", 1)
    with pytest.raises(PlanGenError, match="PG_ERR_STATE"):
        e.generate_text_greedy(4, tiny_cfg.eos_id)
    # the handle is still usable
    e.prefill_replicated(ids, pad, 2, alias=True)
    assert e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0).shape == (4, 4)


def test_t2i_share_replicas_equals_oracle(tiny_cfg, tiny_weights, ocfg):
    """System.t2i with share_replicas = 1, parallel_size = 2, f32 greedy: both replicas equal the oracle's tokens (the assertion of
    tests/test_gpu_cli.py::test_parallel_size_replica_layout_and_file_names through the new path); under teacher forcing only replica 0 is forced."""
    from plangen_amd.system import System, t2i_infer_collate_batch
    e = _engine(tiny_cfg, tiny_weights, "f32", {})
    sysm = System(tiny_cfg, e)
    sysm.args.temperature, sysm.args.parallel_size, sysm.args.share_replicas = 0.0, 2, 1
    g = torch.Generator().manual_seed(5)
    cond = [torch.randint(8, tiny_cfg.vocab, (n,), generator=g).tolist() for n in (7, 5)]
    neg = torch.randint(8, tiny_cfg.vocab, (4,), generator=g).tolist()
    ids, mask = t2i_infer_collate_batch(cond, neg, tiny_cfg.pad_id, tiny_cfg.img_tokens)
    dec, _ = sysm.t2i(ids, mask)
    ref_tok, ref_img = R.t2i(tiny_weights, ocfg, ids, mask, 5.0)
    toks = sysm.last_generated_tokens.cpu()
    assert dec.shape[0] == 4 and toks.shape[0] == 4 and e.R == 8
    assert torch.equal(toks[:2], ref_tok) and torch.equal(toks[2:], ref_tok)
    assert ((dec[:2].cpu() - ref_img) ** 2).mean().item() <= 1e-4 and torch.equal(dec[:2], dec[2:])
    free = toks.clone()
    gt = torch.rand(2, 3, tiny_cfg.img_size, tiny_cfg.img_size, generator=g) * 2 - 1
    region = (torch.rand(2, tiny_cfg.img_tokens, generator=g) > 0.5).int()
    sysm.args.use_teacher_forcing = True
    dec, mask_image = sysm.t2i(ids, mask, gt_image=gt, edit_region=region)
    toks = sysm.last_generated_tokens.cpu()
    labels = e.vq_encode(gt).reshape(2, -1).cpu().int()
    assert dec.shape[0] == 4 and mask_image.shape[0] == 2
    assert torch.equal(toks[:2][region == 0], labels[region == 0]) and torch.equal(toks[2:], free[2:])
    # the default (share_replicas absent / 0) keeps replicating the ids: same tokens
    sysm.args.use_teacher_forcing, sysm.args.share_replicas = False, 0
    sysm.t2i(ids, mask)
    assert torch.equal(sysm.last_generated_tokens.cpu(), free)


def test_facade_model_call_with_replicas(tiny_cfg, tiny_weights):
    """language_model.model(input_ids=, attention_mask=, replicas=p): the stepwise facade on a replicated prefill equals the fused loop."""
    from plangen_amd.janus import MultiModalityCausalLM
    e = _engine(tiny_cfg, tiny_weights, "f32", {})
    ids, pad, mask = _batch(tiny_cfg, (9, 30), 5)
    e.prefill_replicated(ids, pad, 2)
    ref = e.decode_image_tokens(T=6, cfg_weight=5.0, temperature=0.0).cpu()
    vl = MultiModalityCausalLM(e)
    out = vl.language_model.model(input_ids=ids, attention_mask=mask, replicas=2)
    got = []
    for i in range(6):
        lg = vl.gen_head(out.last_hidden_state[:, -1, :])
        mix = lg[1::2] + 5.0 * (lg[0::2] - lg[1::2])
        nt = mix.argmax(-1)
        got.append(nt.cpu())
        if i < 5:
            emb = vl.prepare_gen_img_embeds(torch.stack([nt, nt], 1).view(-1)).unsqueeze(1)
            out = vl.language_model.model(inputs_embeds=emb, attention_mask=None, past_key_values=out.past_key_values)
    assert torch.equal(torch.stack(got, 1).int(), ref)


def test_full_width_128_rows():
    """Full-width 2-layer engine, bf16, R0 = 32 x p = 4 = 128 rows (the 4-wave grouped form at 16 heads), L = 256, 12 teacher-forced steps:
    alias 1 == alias 0 bit for bit, and both within 5e-2 of the plain 128-row run."""
    from test_gpu_smallbatch import _engine as fw_engine
    from test_gpu_fullwidth import _setup
    from plangen_amd.system import t2i_infer_collate_batch
    cfg = _setup()["cfg"]
    e = fw_engine("bf16", 128)
    g = torch.Generator().manual_seed(9)
    lens = [int(v) for v in torch.randint(40, 257, (16,), generator=g)]
    lens[0], lens[1] = 256, 97
    cond = [torch.randint(8, cfg.vocab, (n,), generator=g).tolist() for n in lens]
    neg = torch.randint(8, cfg.vocab, (37,), generator=g).tolist()
    ids, mask = t2i_infer_collate_batch(cond, neg, cfg.pad_id, cfg.img_tokens)
    from plangen_amd.engine import Engine
    pad = Engine.pad_len_from_mask(mask, ids.shape[1])
    assert ids.shape == (32, 256)
    Tn = 12
    force = torch.randint(0, cfg.img_vocab, (64, Tn), generator=g, dtype=torch.int32)

    def dec():
        t, lg = e.decode_image_tokens(T=Tn, cfg_weight=5.0, temperature=0.0, force_tokens=force, return_logits=True)
        torch.cuda.synchronize()
        return t.cpu(), lg.cpu()
    _dirty(e, ids, pad, 4)
    e.prefill_replicated(ids, pad, 4, alias=True)
    a = dec()
    e.prefill_replicated(ids, pad, 4, alias=False)
    b = dec()
    e.prefill(torch.cat([ids] * 4), pad * 4)
    c = dec()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    err = (a[1] - c[1]).abs().max().item()
    print(f"full width 128 rows: replicated vs plain max |dlogit| = {err:.3e}")
    assert err < 5e-2, err


@pytest.mark.parametrize("cond,neg,p,shared", [((33,), 6, 2, True), ((9, 170), 5, 3, True), ((9, 170), (5, 12), 3, False), ((9, 170), (7, 7), 3, False)],
                         ids=["R0=2", "R0=4-shared", "R0=4-pads-differ", "R0=4-ids-differ"])
def test_device_ids_take_the_device_probe(tiny_cfg, tiny_weights, cond, neg, p, shared):
    """ids already on the GPU and uncond_shared=None: no host-side hint, the sharing decision is the library's own device probe on the distinct
    odd rows (R0 = 2: nothing to compare, every odd virtual row is row 1).  Decided exactly as pg_prefill decides it on the replicated ids: the
    attention byte accounting (which counts a shared prompt once) and the tokens equal those of the host-ids call, and equal the plain path's."""
    e = _engine(tiny_cfg, tiny_weights, "f32", {})
    ids, pad, _ = _batch(tiny_cfg, cond, neg)
    from plangen_amd.engine import Engine
    assert Engine.uncond_rows_shared(torch.cat([ids] * p), pad * p) == shared
    out = {}
    e.set_option("time_attn", 1)
    try:
        for name in ("dev", "host", "plain"):
            for alias in (True, False):
                if name == "plain":
                    e.prefill(torch.cat([ids] * p).cuda(), pad * p)
                else:
                    e.prefill_replicated(ids.cuda() if name == "dev" else ids, pad, p, alias=alias)
                t = e.decode_image_tokens(T=6, cfg_weight=5.0, temperature=0.0).cpu()
                out[name, alias] = (t, e.timing()["attn_bytes_sum"])
    finally:
        e.set_option("time_attn", 0)
    for alias in (True, False):
        assert torch.equal(out["dev", alias][0], out["host", alias][0]) and torch.equal(out["dev", alias][0], out["plain", alias][0])
        assert out["dev", alias][1] == out["host", alias][1]
    assert out["dev", False][1] == out["plain", False][1]                  # alias = 0 decodes exactly what the plain path decodes
    assert out["dev", True][1] < out["dev", False][1]


@pytest.mark.parametrize("dtype,kw", ENGINES, ids=IDS)
def test_copy_kernel_and_owner_rows_cache_contents(tiny_cfg, tiny_weights, dtype, kw):
    """Cache contents after prefill_replicated against the plain prefill of the replicated ids, bit for bit, every layer, K and V (FP8: codes and
    both scale planes): alias = 0 -- every row that holds a prompt, replicas included (the copy kernel; its 8-byte path moves the FP8 scale
    pairs: prompts of 9 and 170 slots, odd and even); alias = 1 -- the owner rows (replicas' prompt slots are unspecified by contract)."""
    e = _engine(tiny_cfg, tiny_weights, dtype, kw)
    cfg = tiny_cfg
    fp8 = kw.get("kv_dtype") == "fp8"
    p, slots, nh = 3, 192 + cfg.img_tokens, cfg.n_heads
    ids, pad, _ = _batch(cfg, (9, 170), (5, 12))                        # two negative prompts: all 12 rows hold a prompt
    L, R0 = ids.shape[1], ids.shape[0]
    n_slots = 12 * nh * slots
    cdt = torch.uint8 if fp8 else e.tdtype
    bt = {torch.uint8: torch.uint8, torch.float32: torch.int32, torch.bfloat16: torch.int16}

    def caches():
        torch.cuda.synchronize()
        out = []
        for li in range(cfg.n_layers):
            for nm in ("kcache", "vcache"):
                out.append(e.debug_read(nm, li, n_slots * 128, cdt).cpu().view(12, nh, slots, 128))
            if fp8:
                for nm in ("kscale", "vscale"):
                    out.append(e.debug_read(nm, li, n_slots, torch.float32).cpu().view(12, nh, slots, 1))
        return out
    e.prefill(torch.cat([ids] * p), pad * p)
    plain = caches()
    for alias, rows in ((False, range(R0 * p)), (True, range(R0))):
        _dirty(e, ids, pad, p)
        e.prefill_replicated(ids, pad, p, alias=alias)
        for a, b in zip(plain, caches()):
            for r in rows:
                n = L - pad[r % R0]
                assert torch.equal(a[r, :, :n].view(bt[a.dtype]), b[r, :, :n].view(bt[b.dtype])), (alias, r)
