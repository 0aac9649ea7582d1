"""The path a checkpoint takes into an engine, at the tiny config: pg_load_tensor from bf16 and from fp32 sources into fp32 and bf16 engines, every slot and
every buffer pg_finalize_weights derives read back in its device layout (pg_diag_read_weight) against the host models of tests/load_ref.py, the derived
tables against fp64, a reload after finalize, and the loader's refusals.

W16 = the tiny weights rounded to bf16.  Each engine type is loaded from W16 held as fp32 tensors and from W16 held as bf16 tensors (what a Janus-Pro checkpoint
is); the bf16 engine also from a source that alternates the type tensor by tensor and from one with the vl_gpt. prefix on every name.  Every conversion
involved is exact, so all sources must leave the same bytes and give the same outputs.

Which test reaches a converter from which source: convert_kernel<float> (K_F32 slots of both engines, K_T of the fp32 engine), convert_kernel<bf16> and
convert_il16_kernel / convert_conv_kernel (K_T / K_IL16 / K_CONV slots) from both sources in test_slots; convert_f32_bf16_vec_kernel from the fp32 source only
(bf16 engine, K_T slots of >= 65536 elements: the projections and heads) in test_slots[bf16].  Row movers: test_same_results_from_either_source
(embed_gather, rows_to_f32, copy_rows, t_to_rows).

The measured maxima of the derived tables against their bounds are printed by test_derived_tables_against_fp64 and recorded in its docstring."""
import ctypes as C

import pytest
import torch

import load_ops as O
import load_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ENGINE_ARGS = dict(max_rows=8, max_prompt=96, max_images=4, with_lm_head=True, with_vq_encoder=True, with_vision=True, diag=True)
SOURCES = {"f32": ("f32", "bf16"), "bf16": ("f32", "bf16", "mixed", "prefixed")}
# a capacity that reaches the fused prefill epilogue: HD = 256 -> 3 column tiles of 256; ceil(8 x 2113 / 256) = 67 row tiles; 67 x 3 = 201 >= 200
FUSE_ROWS, FUSE_PROMPT = 8, 2113


@pytest.fixture(scope="module")
def W16(tiny_weights):
    return {k: v.to(BF) for k, v in tiny_weights.items()}


@pytest.fixture(scope="module")
def W32(W16):
    return {k: v.float() for k, v in W16.items()}


def source_of(W16, how):
    if how == "f32":
        return {k: v.float() for k, v in W16.items()}
    if how == "bf16":
        return dict(W16)
    if how == "mixed":
        return {k: (v.float() if i % 2 else v) for i, (k, v) in enumerate(W16.items())}
    return {"vl_gpt." + k: v for k, v in W16.items()}


@pytest.fixture(scope="module")
def engines(tiny_cfg, W16):
    from plangen_amd.engine import Engine
    out = {}
    for dtype, hows in SOURCES.items():
        for how in hows:
            e = Engine(tiny_cfg, dtype=dtype, max_new=tiny_cfg.img_tokens, **ENGINE_ARGS)
            src = source_of(W16, how)
            loaded, skipped = e.load_state_dict(src)
            assert loaded == len(src) and not skipped, (dtype, how, skipped[:3])
            out[(dtype, how)] = e
    yield out
    for e in out.values():
        e.close()


def _read(e, name):
    rc, t, info = O.read_weight(e, name)
    assert rc == O.PG_OK, (name, rc)
    return t, info


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(R.bits(a), R.bits(b))


# ------------------------------------------------------------------------------------------------------------------------------ slots
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_slots(engines, W16, dtype):
    """Every name the engine accepts holds the host model's bytes, whatever the source's type."""
    first = None
    for how in SOURCES[dtype]:
        e = engines[(dtype, how)]
        got = {}
        for name in W16:
            t, (n, es, kind) = _read(e, name)
            want, wkind = R.slot_ref(W16, name, dtype)
            assert kind == wkind and n == want.numel() and es == want.element_size(), (name, how, kind, wkind, n, es)
            res = R.same_bits(t, want)
            assert res["ok"], (name, how, res)
            got[name] = t
        if first is None:
            first = got
        else:
            assert all(_same(got[k], first[k]) for k in W16), how              # the sources give byte-identical buffers
    kinds = {R.expected_kind(k, tuple(v.shape)) for k, v in W16.items()}
    assert kinds == {R.K_T, R.K_F32, R.K_IL16_G, R.K_IL16_U, R.K_CONV}
    if dtype == "bf16":                                                        # the fp32 source reached the vector converter
        assert any(v.numel() >= 65536 and v.numel() % 8 == 0 and R.expected_kind(k, tuple(v.shape)) == R.K_T for k, v in W16.items())


def test_derived_copies(engines, tiny_cfg, W16):
    """Every decode-tiled copy equals the tiled model of its source; an fp32 handle has none, and tiny never reaches the fused prefill epilogue."""
    want = R.derived_refs(W16, tiny_cfg)
    assert len(want) == 4 * tiny_cfg.n_layers + 3 and all(v is not None for v in want.values())
    for how in SOURCES["bf16"]:
        e = engines[("bf16", how)]
        for name, w in want.items():
            t, (n, es, kind) = _read(e, name)
            assert kind == R.K_DERIVED and es == 2 and n == w.numel()
            res = R.same_bits(t, w)
            assert res["ok"], (name, how, res)
        for i in range(tiny_cfg.n_layers):
            rc, t, info = O.read_weight(e, f"layers.{i}.wqkv_p")
            assert rc == O.PG_ERR_STATE and t is None and info[0] == 3 * 256 * tiny_cfg.hidden, (rc, info)
    assert not R.can_fuse(ENGINE_ARGS["max_rows"], ENGINE_ARGS["max_prompt"], tiny_cfg.n_heads * 128)
    e = engines[("f32", "bf16")]
    for name in list(want) + ["layers.0.wqkv_p"]:
        rc, t, _ = O.read_weight(e, name)
        assert rc == O.PG_ERR_STATE and t is None, (name, rc)
    for name in ("layers.2.wqkv_t", "layers.-1.wo_t", "layers.0.wq_t", "layers.x.wd_t", "gh_w3_t", "", "vl_gpt.gen_embed.weight"):
        rc, t, _ = O.read_weight(e, name)
        assert rc == O.PG_ERR_NAME and t is None, (name, rc)


def test_wqkv_p_on_a_capacity_that_fuses(tiny_cfg, W16):
    """max_rows = 8, max_prompt = 2113: ceil(16904 / 256) x ceil(768 / 256) = 67 x 3 = 201 >= 200 tiles, so finalize builds wqkv_p (2112 gives 198: not)."""
    from plangen_amd.engine import Engine
    HD = tiny_cfg.n_heads * 128
    assert R.can_fuse(FUSE_ROWS, FUSE_PROMPT, HD) and not R.can_fuse(FUSE_ROWS, FUSE_PROMPT - 1, HD)
    e = Engine(tiny_cfg, dtype="bf16", max_rows=FUSE_ROWS, max_prompt=FUSE_PROMPT, max_new=8, max_images=1, diag=True)
    part = {k: v for k, v in W16.items() if any(p in k for p in ("q_proj", "k_proj", "v_proj"))}
    loaded, skipped = e.load_tensors(part)
    assert loaded == 3 * tiny_cfg.n_layers and not skipped
    assert e.finalize(strict=False) > 0
    for i in range(tiny_cfg.n_layers):
        wqkv = R.layer_matrices(W16, tiny_cfg, i)["wqkv"]
        t, (n, es, kind) = _read(e, f"layers.{i}.wqkv_p")
        assert kind == R.K_DERIVED and es == 2 and n == wqkv.numel()
        res = R.same_bits(t, R.interleave_qk_ref(wqkv, tiny_cfg.n_heads).reshape(-1))
        assert res["ok"], (i, res)
        assert not R.same_bits(t, wqkv.reshape(-1))["ok"]                      # it is a re-ordering, not a copy
        t, _ = _read(e, f"layers.{i}.wqkv_t")
        assert R.same_bits(t, R.tile_ref(wqkv))["ok"]
    e.close()


# ------------------------------------------------------------------------------------------------------------------------------ results
def _calls(e, cfg):
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(8, cfg.vocab, (2, 12), generator=g).to(torch.int32)
    pad = [0, 3]
    hid = e.prefill(ids, pad, return_hidden=True, hidden_dtype=torch.float32)
    out = {"prefill_hidden": torch.cat([hid[0].reshape(-1), hid[1, pad[1]:].reshape(-1)])}      # pad columns are never written
    out["gen_head"] = e.gen_head(torch.randn(1, cfg.hidden, generator=g))
    out["gen_embed"] = e.gen_embed(torch.tensor([cfg.img_vocab - 1], dtype=torch.int32))
    out["gen_embed_bf16"] = e.gen_embed(torch.tensor([3], dtype=torch.int32), dtype=BF)
    out["embed_tokens"] = e.embed_tokens(torch.tensor([cfg.vocab - 1], dtype=torch.int32))
    out["vq_decode"] = e.vq_decode(torch.randint(0, cfg.img_vocab, (1, cfg.img_tokens), generator=g).to(torch.int32))
    out["vq_encode"] = e.vq_encode(torch.rand(1, 3, cfg.img_size, cfg.img_size, generator=g) * 2 - 1)
    out["vision_encode"] = e.vision_encode(torch.randn(1, 3, cfg.vit_img, cfg.vit_img, generator=g))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_same_results_from_either_source(engines, tiny_cfg, dtype):
    """One call each of prefill (hidden out), gen_head, gen_embed, embed_tokens, vq_decode, vq_encode and vision_encode: a bf16 checkpoint and its fp32 copy give
    byte-identical outputs."""
    ref = _calls(engines[(dtype, "f32")], tiny_cfg)
    assert all(bool(torch.isfinite(v.double()).all()) for v in ref.values())
    assert float(ref["prefill_hidden"].abs().max()) > 0.1 and float(ref["vq_decode"].abs().max()) > 1e-3
    for how in SOURCES[dtype][1:]:
        got = _calls(engines[(dtype, how)], tiny_cfg)
        for k in ref:
            assert got[k].dtype == ref[k].dtype and torch.equal(got[k].view(torch.uint8), ref[k].view(torch.uint8)), (dtype, how, k)


# ------------------------------------------------------------------------------------------------------------------------------ derived tables
def _tables(e, cfg):
    V, H = cfg.img_vocab, cfg.hidden
    gt = e.debug_read("gen_table", 0, V * H, torch.float32).reshape(V, H)
    pq = e.debug_read("pq_table", 0, V * cfg.vq_z, e.tdtype).reshape(V, cfg.vq_z)
    torch.cuda.synchronize()
    return gt.cpu(), pq.cpu()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_derived_tables_against_fp64(engines, tiny_cfg, W32, dtype):
    """gen_table, pq_table and the RoPE tables against fp64, inside the bounds load_ref derives (max error / bound, <= 1 passes; all 320 table rows).
    Measured on an MI355X: gen_table at 0.017 of its bound (max error 7.8e-7) on both engines; pq_table at 0.174 (fp32 engine, max error 1.4e-7) and 0.987
    (bf16 engine, max error 3.5e-3: the one bf16 rounding of the stored value is nearly the whole bound there, and reaches it at the low end of a binade);
    cos_t at 0.474 (max error 2.09e-5), sin_t at 0.478 (2.14e-5) of 4 u phi + 2 u over all 320 positions."""
    e = engines[(dtype, "bf16")]
    gt, pq = _tables(e, tiny_cfg)
    ref, bound = R.gen_table_ref(W32)
    r_gt, e_gt = R.within(gt, ref, bound)
    ref, bound = R.pq_table_ref(W32, dtype)
    r_pq, e_pq = R.within(pq, ref, bound)
    max_pos = 2 * ENGINE_ARGS["max_prompt"] + tiny_cfg.img_tokens + 64
    cos_t, (n, es, _) = _read(e, "cos_t")
    sin_t, _ = _read(e, "sin_t")
    assert n == max_pos * 64 and es == 4
    cos, sin, bound = R.rope_ref(max_pos, tiny_cfg.rope_theta)
    r_cos, e_cos = R.within(cos_t.reshape(max_pos, 64), cos, bound)
    r_sin, e_sin = R.within(sin_t.reshape(max_pos, 64), sin, bound)
    print(f"derived tables [{dtype} engine] max error / bound (max error): gen_table {r_gt:.3f} ({e_gt:.3g}), pq_table {r_pq:.3f} ({e_pq:.3g}), "
          f"cos_t {r_cos:.3f} ({e_cos:.3g}), sin_t {r_sin:.3f} ({e_sin:.3g}) over {max_pos} positions")
    assert r_gt <= 1.0 and r_pq <= 1.0 and r_cos <= 1.0 and r_sin <= 1.0, (r_gt, r_pq, r_cos, r_sin)
    other = _tables(engines[(dtype, "f32")], tiny_cfg)
    assert _same(gt, other[0]) and _same(pq, other[1])                         # and the same bytes from either source


# ------------------------------------------------------------------------------------------------------------------------------ reload
def _snapshot(e, cfg, W, dtype):
    snap = {name: _read(e, name)[0] for name in W}
    if dtype == "bf16":
        snap.update({name: _read(e, name)[0] for name in R.derived_refs(W, cfg)})
    snap["cos_t"], snap["sin_t"] = _read(e, "cos_t")[0], _read(e, "sin_t")[0]
    snap["gen_table"], snap["pq_table"] = _tables(e, cfg)
    return snap


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reload_after_finalize(tiny_cfg, W16, dtype):
    """Three tensors loaded again after finalize: the engine refuses to run until finalize is called again; then the derived copies follow the new tensors and
    every other buffer keeps its bytes."""
    from plangen_amd.engine import Engine, PlanGenError
    e = Engine(tiny_cfg, dtype=dtype, max_new=tiny_cfg.img_tokens, **ENGINE_ARGS)
    e.load_state_dict(W16)
    before = _snapshot(e, tiny_cfg, W16, dtype)
    g = torch.Generator().manual_seed(99)
    q1 = "language_model.model.layers.1.self_attn.q_proj.weight"
    pqw = "gen_vision_model.post_quant_conv.weight"
    new = dict(W16)
    for name, src_dtype in (("gen_embed.weight", BF), (q1, torch.float32), (pqw, BF)):
        new[name] = (W16[name].float() + torch.randn(W16[name].shape, generator=g) * W16[name].float().std()).to(BF)
        loaded, skipped = e.load_tensors({name: new[name].to(src_dtype)})
        assert loaded == 1 and not skipped
    ids = torch.tensor([[9, 10], [9, 11]], dtype=torch.int32)
    for call in (lambda: e.prefill(ids, [0, 0]), lambda: e.gen_embed(torch.tensor([1], dtype=torch.int32)),
                 lambda: e.gen_head(torch.zeros(1, tiny_cfg.hidden)), lambda: e.vq_decode(torch.zeros(1, tiny_cfg.img_tokens, dtype=torch.int32))):
        with pytest.raises(PlanGenError, match="PG_ERR_STATE"):
            call()
    assert e.finalize() == 0
    e.prefill(ids, [0, 0])
    after = _snapshot(e, tiny_cfg, new, dtype)
    changed = {"gen_embed.weight", q1, pqw, "gen_table", "pq_table"} | ({"layers.1.wqkv_t"} if dtype == "bf16" else set())
    for name in before:
        if name in changed:
            assert not _same(after[name], before[name]), name
        else:
            assert _same(after[name], before[name]), name
    for name in ("gen_embed.weight", q1, pqw):
        assert R.same_bits(after[name], R.slot_ref(new, name, dtype)[0])["ok"], name
    k1 = q1.replace("q_proj", "k_proj")
    assert R.same_bits(after[k1], R.slot_ref(new, k1, dtype)[0])["ok"]        # the neighbouring third of wqkv kept its bytes
    if dtype == "bf16":
        assert R.same_bits(after["layers.1.wqkv_t"], R.tile_ref(R.layer_matrices(new, tiny_cfg, 1)["wqkv"]))["ok"]
    new32 = {k: v.float() for k, v in new.items()}
    ref, bound = R.gen_table_ref(new32)
    assert R.within(after["gen_table"], ref, bound)[0] <= 1.0
    assert R.within(before["gen_table"], ref, bound)[0] > 100                   # the old table is not the new tensors'
    ref, bound = R.pq_table_ref(new32, dtype)
    assert R.within(after["pq_table"], ref, bound)[0] <= 1.0
    assert R.within(before["pq_table"], ref, bound)[0] > 100
    e.close()


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_load_refusals(tiny_cfg, W16):
    from plangen_amd import _lib
    from plangen_amd.engine import Engine, PlanGenError
    e = Engine(tiny_cfg, dtype="bf16", max_rows=2, max_prompt=8, max_images=1, diag=True)
    down = "language_model.model.layers.0.mlp.down_proj.weight"
    e.load_tensors({down: W16[down]})
    kept, _ = _read(e, down)

    def load(name, t, dtype_code=None, shape=None):
        t = t.contiguous()
        shape = tuple(t.shape) if shape is None else shape
        arr = (C.c_int64 * max(1, len(shape)))(*shape)
        code = (_lib.PG_BF16 if t.dtype == BF else _lib.PG_F32) if dtype_code is None else dtype_code
        return e.lib.pg_load_tensor(e.h, name.encode(), C.c_void_p(t.data_ptr()), code, arr, len(shape))

    other = (W16[down].float() * 2 + 1).to(BF)
    assert load(down, other[:-1]) == O.PG_ERR_ARG                              # one row short
    assert "elements" in e.lib.pg_last_error(e.h).decode()
    assert load(down, other, shape=(other.numel() + 1,)) == O.PG_ERR_ARG
    assert load(down, other.t().contiguous()) == O.PG_ERR_ARG                  # transposed: the right count, the wrong shape
    assert "shape" in e.lib.pg_last_error(e.h).decode()
    q = "language_model.model.layers.0.self_attn.q_proj.weight"                # 256 x 256: square, so only a 3-D view of it can be told apart
    assert load(q, W16[q], shape=(1, 256, 256)) == O.PG_ERR_ARG
    conv = "gen_vision_model.decoder.conv_in.weight"
    assert load(conv, W16[conv], shape=tuple(W16[conv].permute(0, 2, 3, 1).shape)) == O.PG_ERR_ARG      # a channels-last conv weight
    for code in (_lib.PG_I32, _lib.PG_I64, _lib.PG_FP8_E4M3, 7, -1):
        assert load(down, other, dtype_code=code) == O.PG_ERR_ARG, code        # neither fp32 nor bf16
        assert "dtype" in e.lib.pg_last_error(e.h).decode()
    for name in ("language_model.model.layers.2.mlp.down_proj.weight", "down_proj.weight", "", "vl_gpt.", "vl_gpt.vl_gpt." + down, down + " "):
        assert load(name, other) == O.PG_ERR_NAME, name
    assert e.lib.pg_load_tensor(e.h, None, C.c_void_p(other.data_ptr()), _lib.PG_BF16, (C.c_int64 * 2)(*other.shape), 2) == O.PG_ERR_ARG
    assert e.lib.pg_load_tensor(e.h, down.encode(), None, _lib.PG_BF16, (C.c_int64 * 2)(*other.shape), 2) == O.PG_ERR_ARG
    after, _ = _read(e, down)
    assert _same(after, kept)                                                  # no refusal wrote anything
    assert load("vl_gpt." + down, other) == O.PG_OK                            # and the prefixed name is the same slot
    after, _ = _read(e, down)
    assert R.same_bits(after, other.reshape(-1))["ok"]
    with pytest.raises(PlanGenError, match="missing"):
        e.finalize(strict=True)
    e.close()
