"""Scoring given text through the engine (pg_score_tokens, Engine.score_text / score_text_embeds, System.score_layouts) on the tiny fixture
engine with lm_head, bf16 and f32: against the fp64 reference of tests/score_ref.py applied to the hidden states the same prefill
returns, against the text loop's own log-probabilities (f32), and the error paths."""
import numpy as np
import pytest
import torch

import logprob_ref as LR
import score_ref as SR
from conftest import get_engine, load_golden

pytestmark = pytest.mark.gpu

LM_HEAD = "language_model.lm_head.weight"


def _case(cfg):
    g = torch.Generator().manual_seed(31)
    R, L = 4, 20
    pad = [0, 3, 7, 11]
    score_from = [1, 8, 12, 20]                 # pad + 1, later starts, and a row that scores nothing
    ids = torch.randint(8, cfg.vocab, (R, L), generator=g).int()
    for r, p in enumerate(pad):
        ids[r, :p] = cfg.pad_id
    return ids, pad, score_from


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_score_text_against_reference(tiny_cfg, tiny_weights, dtype, temperature):
    from plangen_amd.engine import score_index
    e = get_engine(tiny_cfg, tiny_weights, dtype)
    ids, pad, score_from = _case(tiny_cfg)
    R, L = ids.shape
    lp = e.score_text(ids, pad, score_from, temperature=temperature).cpu()
    hid = e.prefill(ids, pad, position_mode=1, return_hidden=True, hidden_dtype=e.tdtype)
    torch.cuda.synchronize()
    assert lp.shape == (R, L) and lp.dtype == torch.float32
    sel = score_index(L, pad, score_from)
    scored = torch.zeros(R * L, dtype=torch.bool)
    scored[sel] = True
    assert (lp.reshape(-1)[~scored] == 0).all() and not np.signbit(lp.reshape(-1)[~scored].numpy()).any()      # exactly 0.0
    hidden = hid.float().cpu().reshape(R * L, -1)
    operand = "bf16" if dtype == "bf16" else "f32"
    target = ids.reshape(-1)[sel]
    lp64, bound = SR.head_logprob_ref(hidden, tiny_weights[LM_HEAD], target, sel - 1, temperature, operand=operand)
    got = lp.reshape(-1)[sel].numpy()
    err, frac = SR.worst(got, lp64, bound)
    print(f"score_text {dtype} T={temperature}: {len(sel)} scored, max |lp - lp64| = {err:.3e}, error / bound = {frac:.3f}")
    assert SR.within(got, lp64, bound).all()
    # using hidden[j] instead of hidden[j - 1] does not pass on these rows
    wrong, _ = SR.head_logprob_ref(hidden, tiny_weights[LM_HEAD], target, sel.clamp(max=R * L - 1), temperature, operand=operand)
    assert not SR.within(wrong, lp64, bound).all()
    # the same through pg_prefill_embeds: bit for bit
    emb = e.embed_tokens(ids, dtype=torch.float32)
    lp2 = e.score_text_embeds(emb, pad, ids, score_from, temperature=temperature).cpu()
    assert torch.equal(lp2.view(torch.int32), lp.view(torch.int32))


def _oracle_tolerance(W, ocfg, ids, mask, gen, eos):
    """Largest difference the CPU oracle shows between its whole-sequence and its step-by-step fp32 evaluation of the same tokens'
    log-probabilities (columns up to and including a row's first EOS)."""
    from oracle import ref_cpu as R
    B, n = gen.shape
    _, step_logits = R.generate_text_greedy(W, ocfg, R.embed_tokens(W, ids), mask, n, eos, force_tokens=gen, return_logits=True)
    step_lp = torch.log_softmax(step_logits.float(), -1).gather(2, gen.T[:, :, None])[:, :, 0].T           # [B, n]
    full_ids = torch.cat([ids.long(), gen], 1)
    full_mask = torch.cat([mask.long(), torch.ones_like(gen)], 1)
    pos = (full_mask.cumsum(-1) - 1).clamp(min=0)
    hidden, _ = R.llama_forward(W, ocfg, R.embed_tokens(W, full_ids), full_mask, pos)
    L = ids.shape[1]
    whole_lp = torch.log_softmax(R.lm_head(W, hidden[:, L - 1:L - 1 + n]).float(), -1).gather(2, gen[:, :, None])[:, :, 0]
    live = ((gen == eos).int().cumsum(1) - (gen == eos).int()) == 0
    return float((step_lp - whole_lp).abs()[live].max()), live


def test_f32_matches_the_text_loop(tiny_cfg, tiny_weights, ocfg):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    ids, mask, eos = torch.tensor(g["ids"]), torch.tensor(g["mask"]), int(g["eos"])
    L, T = ids.shape[1], 12
    pad = e.pad_len_from_mask(mask, L)
    e.prefill(ids, pad, position_mode=1)
    gen, loop_lp = e.generate_text(T, eos, return_logprobs=True)
    gen, loop_lp = gen.cpu(), loop_lp.cpu()
    n = gen.shape[1]
    full = torch.cat([ids, gen.int()], 1)
    lp = e.score_text(full, pad, [L] * ids.shape[0]).cpu()[:, L:]
    measured, live = _oracle_tolerance(tiny_weights, ocfg, ids, mask, gen, eos)
    tol = 4 * measured + LR.ATOL
    diff = float((lp - loop_lp).abs()[live].max())
    print(f"oracle whole-sequence vs step-by-step: {measured:.3e}; allowed {tol:.3e}; score_text vs the loop: {diff:.3e} over {int(live.sum())} tokens")
    assert diff <= tol
    # decode after a scoring call on the same handle: the tokens the fixture holds, as before it
    e.prefill(ids, pad, position_mode=1)
    again = e.generate_text_greedy(T, eos).cpu()
    assert torch.equal(again, gen) and np.array_equal(again[:, :g["out"].shape[1]].numpy(), g["out"][:, :again.shape[1]])


def test_error_paths(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    ids, pad, score_from = _case(tiny_cfg)
    nohead = get_engine(tiny_cfg, tiny_weights, "bf16", with_lm_head=False, max_rows=4)
    with pytest.raises(PlanGenError, match="PG_ERR_STATE"):
        nohead.score_text(ids, pad, score_from)
    assert b"lm_head" in nohead.lib.pg_last_error(nohead.h)
    assert nohead.prefill(ids, pad, position_mode=1, return_hidden=True).shape == (4, 20, tiny_cfg.hidden)       # still usable
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    with pytest.raises(ValueError):
        e.score_text(ids, pad, [1, 3, 12, 20])           # score_from == pad_len
    hid = e.prefill(ids, pad, position_mode=1, return_hidden=True, hidden_dtype=torch.bfloat16)
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.score_tokens(hid, torch.zeros(0, dtype=torch.int32))
    with pytest.raises(PlanGenError, match="compute dtype"):
        e.score_tokens(hid.float(), torch.zeros(3, dtype=torch.int32))
    assert torch.isfinite(e.score_text(ids, pad, score_from)).all()


@pytest.mark.parametrize("given", ["caption", "image"])
def test_score_layouts(tiny_cfg, tiny_weights, given):
    from plangen_amd.system import System
    from plangen_amd.textproc import TagWordCodec
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    codec = TagWordCodec(tiny_cfg.vocab, eos_id=tiny_cfg.eos_id, pad_id=tiny_cfg.pad_id)
    sysm = System(tiny_cfg, e, codec=codec)
    gts = ["<grounding><ref>a cat</ref><box>[12,40,500,620]</box></grounding>", "<grounding><ref>dog</ref><box>[1,2,3,4]</box></grounding>"]
    batch = dict(base_caption=["a cat on a mat", "one dog"], gt_grounding=gts)
    if given == "image":
        P = tiny_cfg.vit_tokens
        g = torch.Generator().manual_seed(3)
        q = [[1, 20, 21], [1, 22]]
        Lp = max(len(x) for x in q) + P
        ids = torch.full((2, Lp), tiny_cfg.pad_id, dtype=torch.long)
        seq = torch.zeros((2, Lp), dtype=torch.bool); attn = torch.zeros((2, Lp), dtype=torch.int32)
        for i, x in enumerate(q):
            row = [x[0]] + [0] * P + x[1:]
            ids[i, Lp - len(row):] = torch.tensor(row)
            seq[i, Lp - len(row) + 1:Lp - len(row) + 1 + P] = True
            attn[i, Lp - len(row):] = 1
        batch["prepare_inputs_infer"] = dict(input_ids=ids, pixel_values=torch.rand(2, 1, 3, tiny_cfg.vit_img, tiny_cfg.vit_img, generator=g) * 2 - 1,
                                             images_seq_mask=seq, images_emb_mask=torch.ones((2, 1, P), dtype=torch.bool), attention_mask=attn)
    out = sysm.score_layouts(batch, given=given)
    opn = len(codec.encode("<grounding>")) - 1
    want = [len(codec.encode(t)) - 1 - (opn if given == "caption" else 0) + 1 for t in gts]      # the layout's tokens + EOS
    assert out["n_tokens"] == want
    lp = out["logprobs"].cpu()
    assert [int(v) for v in (lp != 0).sum(-1)] == want and (lp <= 0).all()
    np.testing.assert_allclose(out["sum"], lp.sum(-1).numpy(), rtol=1e-6)
    np.testing.assert_allclose(out["mean"], [s / n for s, n in zip(out["sum"], want)], rtol=1e-6)


@pytest.mark.parametrize("task", ["plan", "uni_2stage", "mmu"])
def test_score_gt_layout_key_adds_the_record(tmp_path, task):
    """--opt score_gt_layout=True: the per-batch JSON of plan / uni_2stage / mmu gains gt_layout_logprob = {sum, mean, n_tokens}, one entry
    per row (without the key the record's keys are the three the CLI tests pin)."""
    import json
    import os
    import train
    from conftest import ROOT
    from project.plangen.plangen_base import System
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='f32'", "temperature=0.0", f"out_path={str(tmp_path)!r}",
            f"test_data.task_type={task!r}", "max_new_tokens=8", "max_prompt=384", "score_gt_layout=True"]
    a = train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
    m = System(a, None)
    m.setup_data(None)
    m.resume(None)
    m.validation(0)
    rec = json.load(open(os.path.join(str(tmp_path), "test", f"synthetic_{task}_1", "0_batch", "0_layout.json")))
    assert set(rec) == {"base_caption", "gt_grounding", "pr_grounding", "gt_layout_logprob"}
    sc = rec["gt_layout_logprob"]
    assert set(sc) == {"sum", "mean", "n_tokens"} and all(len(sc[k]) == 2 for k in sc)
    strip = 0 if task == "mmu" else len(m.codec.encode("<grounding>")) - 1
    assert sc["n_tokens"] == [len(m.codec.encode(g)) - 1 - strip + 1 for g in rec["gt_grounding"]]
    assert all(np.isfinite(s) and s < 0 and abs(s / n - mu) <= 1e-6 * abs(mu) for s, n, mu in zip(sc["sum"], sc["n_tokens"], sc["mean"]))
    m.engine.close()
