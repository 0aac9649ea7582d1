"""Layout attribution through the engine (pg_request_attn_spans, Engine.prefill*(attn_spans=), Engine.attribute_image, System.attribute_layout,
--opt layout_attribution) on the tiny fixture engine: against the fp64 reference of tests/span_ref.py computed from the Q and K the same
prefill left behind, the bits across layer selections and KV dtypes, the one-shot rule, every refusal, and the host-side products."""
import ctypes as C
import dataclasses
import glob
import json
import os

import numpy as np
import pytest
import torch

import span_ref as SP
from conftest import get_engine
from plangen_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = [0, 3, 3, 7, 7, 0]
L0 = 20


def _case(e, cfg):
    g = torch.Generator().manual_seed(43)
    R, T = len(PAD), cfg.img_tokens
    ids = torch.randint(8, cfg.vocab, (R, L0), generator=g).int()
    for r, p in enumerate(PAD):
        ids[r, :p] = cfg.pad_id
    codes = torch.randint(0, cfg.img_vocab, (R // 2, T), generator=g).int()
    emb = torch.cat([e.embed_tokens(ids), e.gen_embed(codes[:, :T - 1]).view(R // 2, T - 1, -1).repeat_interleave(2, dim=0)], 1)
    W = L0 + T - 1
    lo = np.array([[p + 1, L0 - 4, 0, L0, 9] for p in PAD], dtype=np.int32)
    hi = np.array([[p + 5, L0, W, L0 + 10, 9] for p in PAD], dtype=np.int32)        # prompt head, prompt tail, everything, image columns, empty
    return ids, codes, emb, W, lo, hi


def _partition(W, S=4):
    edges = np.linspace(0, W, S + 1).round().astype(np.int32)
    return np.tile(edges[:-1], (len(PAD), 1)), np.tile(edges[1:], (len(PAD), 1))


def _ref_case(e, cfg, W, lo, hi, q_col0, n_q):
    """The span_ref case of the LAST layer, from the Q and K the last prefill left in the engine."""
    R, nh = len(PAD), cfg.n_heads
    slots = e.max_prompt + e.max_new
    length = np.array([W - p for p in PAD], dtype=np.int32)
    ntok = int(length.sum())
    q = e.debug_read("qbuf", 0, ntok * nh * 128, torch.bfloat16).float().cpu().numpy().reshape(ntok, nh, 128)
    k = e.debug_read("kcache", cfg.n_layers - 1, e.max_rows * nh * slots * 128, torch.bfloat16).float().cpu().numpy().reshape(e.max_rows, nh, slots, 128)[:R]
    return dict(family="prefill", q=q, k=k, row_off=np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int32), length=length,
                pad=np.array(PAD, dtype=np.int32), lo=lo, hi=hi, q_col0=q_col0, n_q=n_q, nh=nh, slots=slots, scale=SP.SCALE)


def test_last_layer_against_reference_and_layer_selection(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    ids, codes, emb, W, lo, hi = _case(e, tiny_cfg)
    T, nl = tiny_cfg.img_tokens, tiny_cfg.n_layers
    plain = e.prefill_embeds(emb, PAD, return_hidden=True, hidden_dtype=e.tdtype)
    hid, last = e.prefill_embeds(emb, PAD, return_hidden=True, hidden_dtype=e.tdtype, attn_spans=(lo, hi, L0 - 1, T, [nl - 1]))
    c = _ref_case(e, tiny_cfg, W, lo, hi, L0 - 1, T)
    A, bound = SP.span_mass_ref(c)
    got = last.cpu().numpy()
    assert got.shape == (1, len(PAD), T, lo.shape[1]) and np.isfinite(got).all()
    err, frac, exact = SP.worst(got[0], A, bound)
    print(f"last layer: max |A - A64| = {err:.3e}, error / bound = {frac:.3f}, bound <= {bound.max():.3e}")
    assert frac <= 1.0 and exact
    assert np.abs(got[0, :, :, 2] - 1.0).max() <= bound.max() and (got[0, :, :, 4] == 0).all()      # the whole frame, the empty span
    assert torch.equal(hid.view(torch.int16), plain.view(torch.int16))                                # the request changes nothing else
    # all layers: the last one's bits are the same; a second call repeats every bit
    _, every = e.prefill_embeds(emb, PAD, attn_spans=(lo, hi, L0 - 1, T, None))
    _, again = e.prefill_embeds(emb, PAD, attn_spans=(lo, hi, L0 - 1, T, range(nl)))
    assert every.shape[0] == nl and torch.equal(every[-1].view(torch.int32), last[0].view(torch.int32))
    assert torch.equal(every.view(torch.int32), again.view(torch.int32))
    assert not torch.equal(every[0], every[-1])
    # pg_prefill (ids) serves it too: the prompt columns alone
    _, from_ids = e.prefill(ids, PAD, attn_spans=(np.minimum(lo, L0), np.minimum(hi, L0), 0, L0, [0]))
    assert from_ids.shape == (1, len(PAD), L0, lo.shape[1]) and torch.isfinite(from_ids).all()
    for r, p in enumerate(PAD):
        assert (from_ids[0, r, :p] == 0).all() and (from_ids[0, r, p:, 2] - 1).abs().max() < 1e-4


def test_partition_sums_to_one_on_every_layer(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    _, _, emb, W, _, _ = _case(e, tiny_cfg)
    lo, hi = _partition(W)
    _, mass = e.prefill_embeds(emb, PAD, attn_spans=(lo, hi, 0, W, None))
    got = mass.cpu().numpy().astype(np.float64)
    S = lo.shape[1]
    for r, p in enumerate(PAD):
        assert (got[:, r, :p] == 0).all()                                       # pad queries: exactly zero on every layer
        nk = np.arange(p, W) - p + 1
        tol = S * SP.partition_bound(nk, tiny_cfg.n_heads)                      # the score error cancels in a partition: the rest of the bound
        dev = np.abs(got[:, r, p:].sum(-1) - 1.0)
        assert (dev <= tol[None, :]).all(), (r, float(dev.max()), float(tol.min()))


def test_request_is_one_shot(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    _, _, emb, W, lo, hi = _case(e, tiny_cfg)
    _, mass = e.prefill_embeds(emb, PAD, attn_spans=(lo, hi, 0, W, None))
    torch.cuda.synchronize()
    mass.fill_(-7.5)
    e.prefill_embeds(emb, PAD)
    torch.cuda.synchronize()
    assert (mass == -7.5).all()


def test_fp8_cache_gives_the_bf16_bits(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    f = get_engine(tiny_cfg, tiny_weights, "bf16", kv_dtype="fp8")
    _, _, emb, W, lo, hi = _case(e, tiny_cfg)
    _, a = e.prefill_embeds(emb, PAD, attn_spans=(lo, hi, L0 - 1, tiny_cfg.img_tokens, None))
    _, b = f.prefill_embeds(emb.to(f.device), PAD, attn_spans=(lo, hi, L0 - 1, tiny_cfg.img_tokens, None))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _raw_request(e, lo, hi, rows, n_spans, q_col0, n_q, mask, out, cap=None):
    lo = np.ascontiguousarray(lo, dtype=np.int32); hi = np.ascontiguousarray(hi, dtype=np.int32)
    req = _lib.pg_attn_spans(lo.ctypes.data, hi.ctypes.data, rows, n_spans, q_col0, n_q, mask, out.data_ptr(), out.numel() if cap is None else cap)
    return e.lib.pg_request_attn_spans(e.h, C.byref(req))


def test_refusals_leave_no_request_pending(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    ids, _, emb, W, lo, hi = _case(e, tiny_cfg)
    R, S, nl = len(PAD), lo.shape[1], tiny_cfg.n_layers
    out = torch.full((nl * R * W * 16,), -7.5, dtype=torch.float32, device=e.device)
    full = (1 << nl) - 1

    def nothing_pending(eng=e, x=emb):
        eng.prefill_embeds(x, PAD)
        torch.cuda.synchronize()
        assert (out == -7.5).all()

    # refused where the request is made
    lo17 = np.zeros((R, 17), dtype=np.int32)
    for args in ((lo17, lo17, R, 17, 0, 1, full), (lo, hi, R, 0, 0, 1, full), (lo, hi, R, S, 0, 1, 0), (lo, hi, R, S, 0, 1, 1 << nl),
                 (lo, hi, 0, S, 0, 1, full), (lo, hi, e.max_rows + 1, S, 0, 1, full), (lo, hi, R, S, -1, 1, full), (lo, hi, R, S, 0, 0, full)):
        assert _raw_request(e, *args, out) == -1, args[2:]
        nothing_pending()
    assert _raw_request(e, lo, hi, R, S, 0, 1, full, out, cap=0) == -1
    nothing_pending()
    # a valid request, then NULL: forgotten
    assert _raw_request(e, lo, hi, R, S, 0, W, full, out) == 0 and e.lib.pg_request_attn_spans(e.h, None) == 0
    nothing_pending()
    # refused by the prefill that would serve it, and consumed all the same
    big = lo.copy(); big[2, 1] = W + 1
    for args, code, cap in (((lo[:4], hi[:4], 4, S, 0, W, full), "PG_ERR_ARG", None),            # rows != R
                            ((lo, hi, R, S, W - 3, 4, full), "PG_ERR_ARG", None),               # q_col0 + n_q > L
                            ((lo, big, R, S, 0, W, full), "PG_ERR_ARG", None),                  # a span bound past L
                            ((lo, hi, R, S, 0, W, full), "PG_ERR_CAPACITY", nl * R * W * S - 1)):
        assert _raw_request(e, *args, out, cap=cap) == 0
        with pytest.raises(PlanGenError, match=code):
            e.prefill_embeds(emb, PAD)
        nothing_pending()
    assert _raw_request(e, lo[:, :1], hi[:, :1], R, 1, 0, L0, 1, out) == 0
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.prefill_replicated(ids, PAD, 1)
    nothing_pending()
    # a PG_F32 handle refuses at the prefill
    f = get_engine(tiny_cfg, tiny_weights, "f32")
    assert _raw_request(f, lo, hi, R, S, 0, W, full, out) == 0
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        f.prefill_embeds(emb, PAD)
    nothing_pending(f)
    # the Python front end: shapes and layers
    for bad in ((lo[:4], hi[:4], 0, W, None), (lo, hi[:, :2], 0, W, None), (lo, hi, 0, W, [nl]), (lo, hi, 0, W, [])):
        with pytest.raises(PlanGenError):
            e.prefill_embeds(emb, PAD, attn_spans=bad)
    nothing_pending()


def test_attribute_image_is_the_hand_built_call(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    ids, codes, emb, W, lo, hi = _case(e, tiny_cfg)
    T = tiny_cfg.img_tokens
    lo_p, hi_p = np.minimum(lo, L0)[0::2], np.minimum(hi, L0)[0::2]                  # spans of the conditional rows, inside the prompt
    got = e.attribute_image(ids, PAD, codes, lo_p, hi_p, layers=[1])
    lo_r = np.zeros_like(lo); hi_r = np.zeros_like(hi)
    lo_r[0::2], hi_r[0::2] = lo_p, hi_p
    _, want = e.prefill_embeds(emb, PAD, attn_spans=(lo_r, hi_r, L0 - 1, T, [1]))
    assert got.shape == (1, len(PAD) // 2, T, lo.shape[1]) and torch.equal(got.view(torch.int32), want[:, 0::2].contiguous().view(torch.int32))
    assert (want[:, 1::2] == 0).all()
    assert e.attribute_image(ids, PAD, codes, lo_p, hi_p).shape[0] == tiny_cfg.n_layers
    # score_image's limits and errors
    small = get_engine(tiny_cfg, tiny_weights, "bf16", max_rows=4, max_prompt=32)
    with pytest.raises(PlanGenError, match="max_prompt >= "):
        small.attribute_image(ids[:2], PAD[:2], codes[:1], lo_p[:1], hi_p[:1])
    with pytest.raises(PlanGenError, match="codes must be"):
        e.attribute_image(ids, PAD, codes[:2], lo_p, hi_p)
    with pytest.raises(PlanGenError, match="lo / hi"):
        e.attribute_image(ids, PAD, codes, lo_p[:2], hi_p[:2])


def test_attribute_layout(tiny_cfg, tiny_weights, tmp_path):
    """System.attribute_layout on a two-entity prompt through the checkpoint-shaped tokenizer fixture (layout tags added as single tokens)."""
    import tok_fixtures as TF
    from plangen_amd.system import System
    from plangen_amd.textproc import HFCodec, box_cells
    codec = HFCodec(TF.plain_hf_tokenizer_dir(tmp_path), special_tokens=True)
    cfg = dataclasses.replace(tiny_cfg, eos_id=codec.eos_token_id, pad_id=codec.pad_id)
    e = get_engine(tiny_cfg, tiny_weights, "bf16", max_rows=4, max_prompt=192)
    sysm = System(cfg, e, codec=codec)
    caps = ["a red cat on the table", "two dogs"]
    gts = ["<grounding><ref>a cat</ref><box>[0,0,500,250]</box><ref>the table</ref><box>[100,500,900,1000]</box></grounding>",
           "<grounding><ref>a red dog</ref><box>[70,70,100,100]</box></grounding>"]
    T, g = cfg.img_tokens, cfg.grid
    ids, m = sysm.pad_input_ids([sysm.wrap_uni_prompt(c, gr)[1].tolist() for c, gr in zip(caps, gts)])
    batch = dict(base_caption=caps, gt_grounding=gts, uni_inputs_ids=ids, uni_attention_mask=torch.cat([m, torch.ones((2, T), dtype=m.dtype)], -1))
    codes = torch.randint(0, cfg.img_vocab, (2, T), generator=torch.Generator().manual_seed(3)).int()
    out = sysm.attribute_layout(batch, codes=codes)
    assert [o["phrases"] for o in out] == [["a cat", "the table"], ["a red dog"]]
    boxes = [["[0,0,500,250]", "[100,500,900,1000]"], ["[70,70,100,100]"]]
    for o, bx in zip(out, boxes):
        E = len(bx)
        assert o["maps"].shape == (E, g, g) and o["maps"].dtype == torch.float32 and len(o["inside"]) == E
        assert (o["maps"] > 0).all() and (o["maps"].sum(0) < 1).all()              # disjoint spans of one softmax
        for i, t in enumerate(bx):
            cells = torch.from_numpy(box_cells(t, g))
            if cells.any():
                np.testing.assert_allclose(o["inside"][i], float(o["maps"][i][cells].double().sum() / o["maps"][i].double().sum()), rtol=1e-6)
            else:
                assert np.isnan(o["inside"][i])
    assert np.isnan(out[1]["inside"][0]) and 0 < out[0]["inside"][0] < 1
    # 'phrase' spans lie inside 'entity' spans: less mass everywhere; one layer instead of the mean of all
    ph = sysm.attribute_layout(batch, codes=codes, kind="phrase", layers=[0])
    assert (ph[0]["maps"] > 0).all() and ph[0]["maps"].shape == (2, g, g)
    en0 = sysm.attribute_layout(batch, codes=codes, layers=[0])
    assert (ph[0]["maps"] < en0[0]["maps"]).all()


def test_cli_option_writes_the_files(tmp_path):
    """--opt layout_attribution=True: the per-batch output of uni gains <batch_idx>_attribution.npy and the layout_attribution record; off by
    default (the record's keys are pinned by tests/test_gpu_image_score_path.py)."""
    import train
    from project.plangen.plangen_base import System
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='bf16'", "temperature=0.0", f"out_path={str(tmp_path)!r}",
            "test_data.task_type='uni'", "test_data.data_name='synthetic'", "max_prompt=256", "layout_attribution=True"]
    a = train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
    m = System(a, None)
    m.setup_data(None)
    m.resume(None)
    m.validation(0)
    g = m.cfg.grid
    m.engine.close()
    files = glob.glob(os.path.join(str(tmp_path), "test", "*", "0_batch", "0_layout.json"))
    assert len(files) == 1, files
    rec = json.load(open(files[0]))
    assert set(rec) == {"base_caption", "gt_grounding", "pr_grounding", "layout_attribution"}
    att = rec["layout_attribution"]
    arr = np.load(os.path.join(os.path.dirname(files[0]), "0_attribution.npy"))
    assert len(att) == 2 and arr.dtype == np.float32 and arr.shape == (2, max(len(x) for x in att), g, g)
    for b, items in enumerate(att):
        assert len(items) == rec["gt_grounding"][b].count("<ref>") >= 1
        assert all(set(it) == {"phrase", "inside"} and (it["inside"] is None or 0 <= it["inside"] <= 1) for it in items)
        assert np.isfinite(arr[b, :len(items)]).all() and (arr[b, :len(items)] > 0).all() and np.isnan(arr[b, len(items):]).all()
