"""Scoring given images through the engine (pg_score_image_tokens, Engine.score_image, System.score_images) on the tiny fixture engine, bf16
and f32: against the fp64 reference of tests/cfg_score_ref.py applied to the layer-1 output and the hidden states of the same prefill,
against the teacher-forced decode loop's own log-probabilities (f32), the state it leaves behind, and the error paths."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import cfg_score_ref as CR
import logprob_ref as LR
import score_ref as SR
from conftest import get_engine

pytestmark = pytest.mark.gpu

W1, B1 = "gen_head.output_mlp_projector.weight", "gen_head.output_mlp_projector.bias"
W2, B2 = "gen_head.vision_head.weight", "gen_head.vision_head.bias"
CFG_W = 5.0


def _case(cfg):
    g = torch.Generator().manual_seed(41)
    R, L, T = 6, 20, cfg.img_tokens
    pad = [0, 3, 3, 7, 7, 0]
    ids = torch.randint(8, cfg.vocab, (R, L), generator=g).int()
    for r, p in enumerate(pad):
        ids[r, :p] = cfg.pad_id
    codes = torch.randint(0, cfg.img_vocab, (R // 2, T), generator=g).int()
    return ids, pad, codes


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_score_image_against_reference(tiny_cfg, tiny_weights, dtype, temperature):
    from plangen_amd.engine import image_score_index
    e = get_engine(tiny_cfg, tiny_weights, dtype)
    ids, pad, codes = _case(tiny_cfg)
    (R, L), T, G = ids.shape, codes.shape[1], tiny_cfg.gen_head_dim
    Wd = L + T - 1
    lp = e.score_image(ids, pad, codes, CFG_W, temperature).cpu()
    mid = e.debug_read("score_mid", 0, R * Wd * G, e.tdtype).float().cpu().view(R * Wd, G)       # the layer-1 output the head read
    assert lp.shape == (R // 2, T) and lp.dtype == torch.float32 and torch.isfinite(lp).all() and (lp <= 0).all()
    # the same prefill again, for its hidden states
    emb = torch.cat([e.embed_tokens(ids), e.gen_embed(codes[:, :T - 1]).view(R // 2, T - 1, -1).repeat_interleave(2, dim=0)], 1)
    hid = e.prefill_embeds(emb, pad, position_mode=0, return_hidden=True, hidden_dtype=e.tdtype).float().cpu().view(R * Wd, -1)
    operand = "bf16" if dtype == "bf16" else "f32"
    # layer 1: GELU_erf(hidden . W1^T + b1) in fp64 on the rounded operands.  Allowed: the accumulation (A * S, S = |h| . |W1|^T) and the bias
    # addition's rounding through GELU's slope (<= 1.13), 8 fp32 roundings' worth for the erf / products, and bf16's unit roundoff 2^-8 (8 significant bits) for the store
    h64, w64 = SR.round_operand(hid, operand).double(), SR.round_operand(tiny_weights[W1], operand).double()
    pre = h64 @ w64.T + tiny_weights[B1].double()
    g64 = torch.nn.functional.gelu(pre)
    K1 = hid.shape[1]
    A = K1 * SR.U if operand == "bf16" else K1 * SR.U / (1 - K1 * SR.U)
    tol1 = 1.13 * (A * (h64.abs() @ w64.abs().T) + SR.U * pre.abs()) + 8 * SR.U * (g64.abs() + pre.abs()) + (2.0 ** -8 * g64.abs() if operand == "bf16" else 0)
    real = torch.ones(R, Wd, dtype=torch.bool)
    for r, p in enumerate(pad):
        real[r, :p] = False
    d1 = (mid.double() - g64).abs()[real.view(-1)]
    print(f"layer 1 {dtype}: max |mid - g64| = {float(d1.max()):.3e}, max error / allowance = {float((d1 / tol1[real.view(-1)]).max()):.3f}")
    assert (d1 <= tol1[real.view(-1)]).all()
    # layer 2 + mix + log-softmax on the device's own layer-1 output
    cond, uncond = image_score_index(L, T, R)
    target = codes.reshape(-1)
    lp64, bound = CR.cfg_head_logprob_ref(mid, tiny_weights[W2], tiny_weights[B2], target, cond, uncond, CFG_W, temperature, operand)
    got = lp.reshape(-1).numpy()
    err, frac = SR.worst(got, lp64, bound)
    print(f"score_image {dtype} T={temperature}: {len(target)} scored, max |lp - lp64| = {err:.3e}, error / bound = {frac:.3f}")
    assert SR.within(got, lp64, bound).all()
    # column L + j instead of L - 1 + j does not pass on these rows
    wrong, _ = CR.cfg_head_logprob_ref(mid, tiny_weights[W2], tiny_weights[B2], target, (cond + 1).clamp(max=R * Wd - 1),
                                       (uncond + 1).clamp(max=R * Wd - 1), CFG_W, temperature, operand)
    assert not SR.within(wrong, lp64, bound).all()


def _oracle_tolerance(W, ocfg, ids, pad, codes, temperature):
    """Largest difference the CPU oracle shows between its whole-sequence and its step-by-step fp32 evaluation of the same image tokens'
    guided log-probabilities."""
    from oracle import ref_cpu as R
    (R2, L), T = ids.shape, codes.shape[1]
    mask = torch.ones((R2, L + T), dtype=torch.int32)
    for r, p in enumerate(pad):
        mask[r, :p] = 0
    inv = float(np.float32(1.0) / np.float32(temperature))

    def lp_of(mixed):                                                     # [B, T, V] -> [B, T]
        return torch.log_softmax(mixed.float() * inv, -1).gather(2, codes.long()[:, :, None])[:, :, 0]
    _, step = R.sample_image(W, ocfg, R.embed_tokens(W, ids), mask, CFG_W, n_tokens=T, force_tokens=codes, return_logits=True)
    step_lp = lp_of(step.transpose(0, 1))
    img = R.prepare_gen_img_embeds(W, codes[:, :T - 1].reshape(-1)).view(R2 // 2, T - 1, -1).repeat_interleave(2, dim=0)
    x = torch.cat([R.embed_tokens(W, ids), img], 1)
    pos = torch.arange(L + T - 1)[None].expand(R2, L + T - 1)
    hidden, _ = R.llama_forward(W, ocfg, x, mask, pos)
    logits = R.gen_head(W, hidden[:, L - 1:])
    whole_lp = lp_of(logits[1::2] + CFG_W * (logits[0::2] - logits[1::2]))
    return float((step_lp - whole_lp).abs().max())


def test_f32_matches_the_decode_loop(tiny_cfg, tiny_weights, ocfg):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, codes = _case(tiny_cfg)
    B, T = codes.shape
    temperature = 1.0
    # greedy tokens of this prompt before any scoring call
    e.prefill(ids, pad, position_mode=0)
    before = e.decode_image_tokens(T, CFG_W, 0.0).cpu()
    # the teacher-forced loop's own log-probabilities of the codes
    e.prefill(ids, pad, position_mode=0)
    toks, loop_lp = e.decode_image_tokens(T, CFG_W, temperature, force_tokens=codes, force_mask=torch.zeros((B, T), dtype=torch.uint8),
                                          return_logprobs=True)
    assert torch.equal(toks.cpu(), codes)
    lp = e.score_image(ids, pad, codes, CFG_W, temperature).cpu()
    measured = _oracle_tolerance(tiny_weights, ocfg, ids, pad, codes, temperature)
    tol = 4 * measured + LR.ATOL
    diff = float((lp - loop_lp.cpu()).abs().max())
    print(f"oracle whole-sequence vs step-by-step: {measured:.3e}; allowed {tol:.3e}; score_image vs the loop: {diff:.3e} over {B * T} tokens")
    assert diff <= tol
    # decode after a scoring call on the same handle: the tokens it yielded before
    e.prefill(ids, pad, position_mode=0)
    again = e.decode_image_tokens(T, CFG_W, 0.0).cpu()
    assert torch.equal(again, before)


def test_error_paths(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    from plangen_amd.system import System
    ids, pad, codes = _case(tiny_cfg)
    small = get_engine(tiny_cfg, tiny_weights, "bf16", max_prompt=64, max_rows=6, with_vq_encoder=False)
    with pytest.raises(PlanGenError, match="max_prompt >= 83"):
        small.score_image(ids, pad, codes)
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    with pytest.raises(PlanGenError, match="CFG-interleaved"):
        e.score_image(ids[:5], pad[:5], codes)                              # odd rows
    with pytest.raises(PlanGenError, match="codes must be"):
        e.score_image(ids, pad, codes[:2])                                  # 2 images' codes for 3 pairs
    with pytest.raises(PlanGenError, match="codes must be"):
        e.score_image(ids, pad, codes.reshape(-1))
    hid = torch.zeros((4, tiny_cfg.hidden), dtype=torch.float32, device=e.device)
    with pytest.raises(PlanGenError, match="compute dtype"):
        e.score_image_tokens(hid, [0, 1], [0, 2], [1, 3])
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.score_image_tokens(hid.bfloat16(), [], [], [])
    with pytest.raises(PlanGenError, match="with_vq_encoder"):
        System(tiny_cfg, small).score_images(dict(image=torch.zeros(1, 3, tiny_cfg.img_size, tiny_cfg.img_size)))
    assert torch.isfinite(e.score_image(ids, pad, codes)).all()              # still usable


def test_score_images(tiny_cfg, tiny_weights):
    """System.score_images on 3 images with an engine that holds 2 pairs: two chunks; the per-row numbers follow the scored mask."""
    from plangen_amd.system import System
    from plangen_amd.textproc import TagWordCodec
    e = get_engine(tiny_cfg, tiny_weights, "bf16", max_rows=4, max_prompt=192)      # room for a worded prompt + 63 image columns
    codec = TagWordCodec(tiny_cfg.vocab, eos_id=tiny_cfg.eos_id, pad_id=tiny_cfg.pad_id)
    sysm = System(tiny_cfg, e, codec=codec)
    caps = ["a cat on a mat", "one dog", "two birds over a lake"]
    gts = ["<grounding><ref>a cat</ref><box>[12,40,500,620]</box></grounding>", "<grounding><ref>dog</ref><box>[1,2,3,4]</box></grounding>",
           "<grounding><ref>birds</ref><box>[5,6,70,80]</box></grounding>"]
    T = tiny_cfg.img_tokens
    ids, m = sysm.pad_input_ids([sysm.wrap_uni_prompt(c, g)[1].tolist() for c, g in zip(caps, gts)])
    g = torch.Generator().manual_seed(5)
    batch = dict(base_caption=caps, gt_grounding=gts, uni_inputs_ids=ids, uni_attention_mask=torch.cat([m, torch.ones((3, T), dtype=m.dtype)], -1),
                 image=torch.rand(3, 3, tiny_cfg.img_size, tiny_cfg.img_size, generator=g) * 2 - 1)
    out = sysm.score_images(batch)
    lp = out["logprobs"].cpu()
    assert lp.shape == (3, T) and (lp <= 0).all() and torch.isfinite(lp).all() and out["n_tokens"] == [T] * 3
    np.testing.assert_allclose(out["sum"], lp.sum(-1).numpy(), rtol=1e-6)
    np.testing.assert_allclose(out["mean"], [s / T for s in out["sum"]], rtol=1e-6)
    scored = torch.zeros((3, T), dtype=torch.bool)
    scored[0, :5] = True
    scored[2, 10:] = True
    part = sysm.score_images(batch, scored=scored)
    assert part["n_tokens"] == [5, 0, T - 10] and part["mean"][1] == 0.0 and part["sum"][1] == 0.0
    np.testing.assert_allclose(part["sum"][0], float(lp[0, :5].sum()), rtol=1e-6)
    np.testing.assert_allclose(part["sum"][2], float(lp[2, 10:].sum()), rtol=1e-6)


def _run_cli(tmp_path, task, extra):
    import train
    from conftest import ROOT
    from project.plangen.plangen_base import System
    from plangen_amd.config import PlanGenConfig
    S = PlanGenConfig.tiny().img_size
    g = torch.Generator().manual_seed(9)
    rows = []
    for i in range(2):
        pt = os.path.join(str(tmp_path), f"img{i}.pt")
        torch.save(torch.rand(3, S, S, generator=g) * 2 - 1, pt)
        rows.append(dict(base_caption=f"a red cup {i}", gt_grounding=f"<grounding><ref>cup</ref><box>[1,2,30,4{i}]</box></grounding>", image_id=str(i),
                         image_pt=pt))
    data = os.path.join(str(tmp_path), "rows.jsonl")
    with open(data, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows))
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='f32'", "temperature=0.0", f"out_path={str(tmp_path)!r}",
            f"test_data.task_type={task!r}", f"test_data.data_file={data!r}", "max_new_tokens=8", "max_prompt=384"] + extra
    a = train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
    m = System(a, None)
    m.setup_data(None)
    m.resume(None)
    m.validation(0)
    files = glob.glob(os.path.join(str(tmp_path), "test", "*", "0_batch", "0_layout.json"))
    assert len(files) == 1, files
    rec = json.load(open(files[0]))
    m.engine.close()
    return rec, m


@pytest.mark.parametrize("task", ["uni", "uni_2stage"])
def test_score_gt_image_key_adds_the_record(tmp_path, task):
    """--opt score_gt_image=True: the per-batch JSON of uni / uni_2stage gains gt_image_logprob = {sum, mean, n_tokens}, one entry per row;
    without the key the record's keys are the three the CLI tests pin."""
    rec, m = _run_cli(tmp_path, task, ["score_gt_image=True"])
    assert set(rec) == {"base_caption", "gt_grounding", "pr_grounding", "gt_image_logprob"}
    sc = rec["gt_image_logprob"]
    T = m.cfg.img_tokens
    assert set(sc) == {"sum", "mean", "n_tokens"} and all(len(sc[k]) == 2 for k in sc) and sc["n_tokens"] == [T, T]
    assert all(np.isfinite(s) and s < 0 and abs(s / n - mu) <= 1e-6 * abs(mu) for s, n, mu in zip(sc["sum"], sc["n_tokens"], sc["mean"]))


def test_default_leaves_the_record_as_it_is(tmp_path):
    rec, _ = _run_cli(tmp_path, "uni", [])
    assert set(rec) == {"base_caption", "gt_grounding", "pr_grounding"}
