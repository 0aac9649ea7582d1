"""CPU: the fp64 reference of the token log-probability (logprob_ref.py) on its special cases, the power of the comparison the GPU tests
use (it must reject each wrong version of the definition by a wide margin), the ABI surface, and the select_best / layout_best_of host
logic of System on a stub engine."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
import logprob_ref as LR

NEG_INF = float("-inf")


# ----------------------------------------------------------------------------------------------------------------- reference
def test_reference_special_cases():
    y = np.array([[0.0, 1.0, 2.0, -1.0]], np.float32)
    z = np.log(np.exp(np.array([0.0, 1.0, 2.0, -1.0])).sum())
    assert abs(LR.token_logprob_ref(y, [2])[0] - (2.0 - z)) < 1e-12
    assert LR.token_logprob_ref(y, [2], 0.0)[0] == LR.token_logprob_ref(y, [2], -1.0)[0]         # temperature <= 0: x = y
    half = LR.token_logprob_ref(y, [2], 0.5)[0]
    assert abs(half - (4.0 - np.log(np.exp(2 * np.array([0.0, 1.0, 2.0, -1.0])).sum()))) < 1e-12
    # NaN counts as -inf: in the normaliser and as the token's own entry
    yn = np.array([[0.0, np.nan, 2.0, -1.0]], np.float32)
    assert abs(LR.token_logprob_ref(yn, [2])[0] - (2.0 - np.log(np.exp(np.array([0.0, 2.0, -1.0])).sum()))) < 1e-12
    assert LR.token_logprob_ref(yn, [1])[0] == NEG_INF
    # -inf token, token out of range, empty rows
    ym = np.array([[0.0, NEG_INF, 2.0, -1.0]], np.float32)
    assert LR.token_logprob_ref(ym, [1])[0] == NEG_INF
    assert LR.token_logprob_ref(y, [4])[0] == NEG_INF and LR.token_logprob_ref(y, [-1])[0] == NEG_INF
    assert LR.token_logprob_ref(np.full((1, 5), NEG_INF, np.float32), [0])[0] == NEG_INF
    assert LR.token_logprob_ref(np.full((1, 5), np.nan, np.float32), [3])[0] == NEG_INF
    # +inf: the mass lies evenly on the +inf entries
    yp = np.array([[0.0, np.inf, 2.0, np.inf]], np.float32)
    assert abs(LR.token_logprob_ref(yp, [1])[0] + np.log(2.0)) < 1e-12 and LR.token_logprob_ref(yp, [0])[0] == NEG_INF
    # a single entry is certain; a huge dynamic range needs the max-subtraction
    assert LR.token_logprob_ref(np.array([[3.5]], np.float32), [0])[0] == 0.0
    big = np.array([[4000.0, 3999.0, -4000.0]], np.float32)
    assert abs(LR.token_logprob_ref(big, [0])[0] + np.log1p(np.exp(-1.0))) < 1e-9


def test_reference_finished_rows_score_zero():
    g = np.random.default_rng(0)
    n, B, V, eos = 5, 3, 11, 4
    lg = g.standard_normal((n, B, V)).astype(np.float32)
    tok = np.array([[1, 2, 4, 4, 4], [4, 4, 4, 4, 4], [1, 2, 3, 5, 6]])
    lp = LR.text_logprobs_ref(lg, tok, eos)
    assert (lp[0, 3:] == 0).all() and lp[0, 2] < 0                       # the step that emits the EOS is scored, the ones after it are not
    assert (lp[1, 1:] == 0).all() and lp[1, 0] < 0 and (lp[2] < 0).all()
    assert abs(lp[0].sum() - sum(LR.token_logprob_ref(lg[t, 0], [tok[0, t]])[0] for t in range(3))) < 1e-12


def test_comparison_semantics():
    assert LR.close([NEG_INF, -1.0], [NEG_INF, -1.0]).all()
    assert not LR.close([-1e30], [NEG_INF])[0] and not LR.close([NEG_INF], [-5.0])[0] and not LR.close([np.nan], [-5.0])[0]
    assert LR.close([-5.0 - 0.9e-4], [-5.0])[0] and not LR.close([-5.0 - 1.2e-4], [-5.0])[0]
    assert (LR.ATOL, LR.RTOL) == (1e-4, 1e-6)


# ----------------------------------------------------------------------------------------------------------------- checker power
def _peaked_rows(seed=1, B=6, V=257):
    """Rows with one clear maximum (margin >= 3) and emitted tokens that are NOT the maximum."""
    g = np.random.default_rng(seed)
    y = (g.standard_normal((B, V)) * 2.4).astype(np.float32)
    top = g.integers(0, V, B)
    y[np.arange(B), top] = y.max(1) + 3.0
    tok = (top + 1 + g.integers(0, V - 1, B)) % V
    assert (tok != top).all()
    return y, tok


def _rejected(mut, true):
    """every entry differs by more than 100x the tolerance, so the comparison fails everywhere"""
    mut, true = np.asarray(mut), np.asarray(true)
    margin = np.abs(mut - true) / (LR.ATOL + LR.RTOL * np.abs(true))
    assert (margin > 100).all(), margin.min()
    assert not LR.close(mut, true).any()


def test_the_comparison_rejects_every_mutant():
    y, tok = _peaked_rows()
    T = 0.5
    true = LR.token_logprob_ref(y, tok, T)
    assert LR.close(true.astype(np.float32), true).all()                # ... and accepts the truth rounded to fp32
    _rejected(LR.mutant_no_temperature(y, tok, T), true)
    _rejected(LR.mutant_argmax_token(y, tok, T), true)
    # top-k: the emitted token inside the kept set (else the mutant is -inf against a finite value, rejected by the infinity rule)
    # -- on flat rows (no planted peak, temperature 3), where the 5 kept entries hold a small share of the mass
    k = 5
    flat = (np.random.default_rng(3).standard_normal(y.shape) * 2.4).astype(np.float32)
    tk = np.argsort(flat, axis=1)[:, -k]
    _rejected(LR.mutant_topk_renormalised(flat, tk, 3.0, k), LR.token_logprob_ref(flat, tk, 3.0))
    # mask / EOS ban: half of the vocabulary disallowed, the emitted token allowed
    g = np.random.default_rng(2)
    allowed = g.random(y.shape) < 0.5
    allowed[np.arange(len(tok)), tok] = True
    allowed[np.arange(len(tok)), np.argmax(y, 1)] = False               # the peak is masked: ignoring the mask moves the normaliser by ~3
    masked = np.where(allowed, y, np.float32(NEG_INF))
    _rejected(LR.mutant_mask_ignored(y, allowed, tok, T), LR.token_logprob_ref(masked, tok, T))
    # finished rows: compare on the columns after the EOS
    n, B, V, eos = 6, 4, 64, 9
    lg = (g.standard_normal((n, B, V)) * 2.4).astype(np.float32)
    toks = np.full((B, n), eos)
    toks[:, 0] = 3
    after = np.zeros((B, n), bool)
    after[:, 2:] = True
    _rejected(LR.mutant_finished_scored(lg, toks, eos, T)[after], LR.text_logprobs_ref(lg, toks, eos, T)[after])


# ----------------------------------------------------------------------------------------------------------------- ABI surface
def test_header_map_and_binding_declare_the_entry_points():
    from plangen_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    mp = open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    sym = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    m = re.search(r"int\s+pg_request_token_logprobs\s*\(([^;]*)\)\s*;", hdr)
    assert m and [p.split()[-1] for p in m.group(1).split(",")] == ["h", "out_dev", "capacity_floats"]
    m = re.search(r"int\s+pg_op_token_logprob\s*\(([^;]*)\)\s*;", hdr)
    assert m and [p.split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")] == \
        ["h", "x_dev", "B", "V", "tok_dev", "temperature", "logprob_dev", "s"]
    for name in ("pg_request_token_logprobs", "pg_op_token_logprob"):
        assert re.search(rf"\b{name};", mp), name
    assert sym["pg_request_token_logprobs"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64])
    assert sym["pg_op_token_logprob"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p])
    api = open(os.path.join(ROOT, "plangen_amd", "csrc", "engine_api.hip")).read()
    opts = api[api.index("int pg_set_option"):api.index("int64_t pg_device_bytes")]
    assert "logprob" not in opts                                         # a one-shot request, not an option: the key table does not grow
    ns = {}
    exec(open(os.path.join(ROOT, "project", "plangen", "cfg", "base.py")).read(), ns)
    assert ns["select_best"] is False and ns["layout_best_of"] == 1


# ----------------------------------------------------------------------------------------------------------------- host logic
def test_select_best_replicas_rule():
    from plangen_amd.system import System
    p, B0, T = 3, 4, 5
    lp = torch.full((p * B0, T), -1.0)
    lp[1 * B0 + 0] = -0.5                                                # prompt 0: replica 1 is best
    lp[2 * B0 + 1] = -0.25; lp[1 * B0 + 1] = -0.25                       # prompt 1: replicas 1 and 2 tie -> the lowest t
    lp[0 * B0 + 2, 3] = NEG_INF; lp[1 * B0 + 2] = -7.0; lp[2 * B0 + 2, 0] = NEG_INF     # prompt 2: a -inf token loses to any finite score
    lp[:, :][torch.tensor([3, 7, 11])] = NEG_INF                         # prompt 3: every replica -inf -> replica 0
    rows, replica, scores = System.select_best_replicas(lp, p)
    assert replica.tolist() == [1, 1, 1, 0] and rows.tolist() == [1 * B0 + 0, 1 * B0 + 1, 1 * B0 + 2, 3]
    assert scores.shape == (p, B0) and scores[1, 0].item() == pytest.approx(-0.5) and scores[0, 2].item() == NEG_INF
    # teacher forcing: only the positions that were not forced count, for every replica
    lp = torch.full((2 * 2, 4), -1.0)
    lp[0, 0] = NEG_INF                                                   # replica 0 of prompt 0: a forced token on an impossible entry, at an excluded position
    lp[2, 0] = -100.0; lp[2, 1:] = -2.0                                  # replica 1 of prompt 0 is worse on the scored positions
    scored = torch.tensor([[0, 1, 1, 1], [0, 0, 0, 0]]).bool()           # prompt 1: nothing scored -> 0.0 for every replica -> replica 0
    rows, replica, scores = System.select_best_replicas(lp, 2, scored)
    assert replica.tolist() == [0, 0] and scores[:, 0].tolist() == [-1.0, -2.0] and scores[:, 1].tolist() == [0.0, 0.0]


def test_select_best_layouts_rule():
    from plangen_amd.system import System
    eos, n, B = 9, 2, 3
    tok = torch.tensor([[1, 2, eos, eos], [1, eos, eos, eos], [1, 2, 3, 4],            # draw 0 of rows 0..2
                        [1, 2, 3, eos], [5, eos, eos, eos], [1, 2, 3, 4]])             # draw 1
    lp = torch.tensor([[-1.0, -1.0, -1.0, 0.0], [-2.0, -2.0, 0.0, 0.0], [-1.0, -1.0, -1.0, -1.0],
                       [-0.5, -0.5, -0.5, -0.5], [-2.0, -2.0, 0.0, 0.0], [-1.0, -1.0, NEG_INF, -1.0]])
    rows, replica, score = System.select_best_layouts(tok, lp, n, eos)
    # row 0: -3/3 against -2/4; row 1: a tie (-4/2 both) -> draw 0; row 2: no EOS -> 4 columns, the -inf draw loses
    assert replica.tolist() == [1, 0, 0] and rows.tolist() == [3, 1, 2]
    assert score.tolist() == pytest.approx([-0.5, -2.0, -1.0])


class _StubEngine:
    """Records the calls System makes; returns seeded tokens / scores."""
    device = torch.device("cpu")
    dtype = "f32"

    def __init__(self, cfg, max_rows=8):
        self.cfg, self.max_rows, self.calls, self.R = cfg, max_rows, [], 0
        self.lp = None
        self.uploaded_dfa = None

    def prefill(self, ids, pad, position_mode=0, **kw):
        self.calls.append(("prefill", tuple(ids.shape), kw)); self.R = ids.shape[0]

    def prefill_replicated(self, ids, pad, replicas, alias=True, **kw):
        self.calls.append(("prefill_replicated", tuple(ids.shape), replicas)); self.R = ids.shape[0] * replicas

    def decode_image_tokens(self, T, cfg_weight, temperature, seed, ft, fm, return_logits, **kw):
        self.calls.append(("decode_image_tokens", self.R, dict(kw)))
        T = self.cfg.img_tokens if T is None else T
        B = self.R // 2
        toks = (torch.arange(B * T).view(B, T) % self.cfg.img_vocab).int() + torch.arange(B).view(B, 1).int()
        if kw.get("return_logprobs"):
            return toks, self.lp(B, T)
        return toks

    def vq_decode(self, codes, dtype=torch.float32):
        self.calls.append(("vq_decode", tuple(codes.shape)))
        return codes.float().mean(1).view(-1, 1, 1, 1).expand(-1, 3, 2, 2).clone()

    def embed_tokens(self, ids, dtype=torch.float32):
        return torch.zeros(tuple(ids.shape) + (4,))

    def prefill_embeds(self, emb, pad, position_mode=0, **kw):
        self.calls.append(("prefill_embeds", tuple(emb.shape))); self.R = emb.shape[0]

    def _text(self, name, max_new, kw):
        self.calls.append((name, self.R, dict(kw)))
        eos = self.cfg.eos_id
        out = torch.full((self.R, 4), eos, dtype=torch.int64)
        out[:, 0] = 20 + torch.arange(self.R)
        if kw.get("return_logprobs"):
            return out, self.lp(self.R, 4)
        return out

    def generate_text(self, max_new, eos, min_new=0, **kw):
        return self._text("generate_text", max_new, kw)

    def generate_text_greedy(self, max_new, eos, min_new=0):
        return self._text("generate_text_greedy", max_new, {})

    def generate_text_constrained(self, max_new, eos, **kw):
        return self._text("generate_text_constrained", max_new, kw)


def _args(**kw):
    base = dict(seed=0, parallel_size=1, cfg_weight=5.0, temperature=1.0, top_k=0, top_p=1.0, use_teacher_forcing=False,
                debug_max_seq_len=None, janus_hw=32, neg_prompt="", use_neg_box=False)
    base.update(kw)
    return SimpleNamespace(**base)


def _cfg_batch(cfg, B0):
    from plangen_amd.system import t2i_infer_collate_batch
    return t2i_infer_collate_batch([[10 + i, 11, 12] for i in range(B0)], [9, 9], cfg.pad_id, cfg.img_tokens)


@pytest.mark.parametrize("share", [0, 1])
def test_t2i_select_best_rows_and_calls(tiny_cfg, share):
    from plangen_amd.system import System
    B0, p, T = 2, 3, tiny_cfg.img_tokens
    e = _StubEngine(tiny_cfg, max_rows=2 * B0 * p)
    # replica t of prompt i sits in row t * B0 + i with or without share_replicas: prompt 0 -> replica 2, prompt 1 -> replica 1
    want = {0: 2, 1: 1}

    def lp(B, T_):
        out = torch.full((B, T_), -3.0)
        for i, t in want.items():
            out[t * B0 + i] = -1.0
        return out
    e.lp = lp
    s = System(tiny_cfg, e, _args(parallel_size=p, select_best=True, share_replicas=share))
    ids, mask = _cfg_batch(tiny_cfg, B0)
    dec, _ = s.t2i(ids, mask)
    names = [c[0] for c in e.calls]
    assert names == (["prefill_replicated"] if share else ["prefill"]) + ["decode_image_tokens", "vq_decode"]
    assert e.calls[1][1] == 2 * B0 * p and e.calls[1][2].get("return_logprobs") is True
    assert e.calls[2][1] == (B0, T)                                      # only the kept rows reach the VQ decoder
    full = _StubEngine(tiny_cfg); full.R = 2 * B0 * p
    all_toks = full.decode_image_tokens(None, 5.0, 1.0, 0, None, None, False)
    assert dec.shape[0] == B0 and torch.equal(s.last_generated_tokens, all_toks[[2 * B0 + 0, 1 * B0 + 1]])
    assert s.last_selection["replica"].tolist() == [2, 1] and s.last_selection["score"].tolist() == [-1.0, -1.0]
    assert s.last_selection["scores"].shape == (p, B0)


def test_t2i_without_select_best_makes_todays_calls(tiny_cfg):
    from plangen_amd.system import System
    ids, mask = _cfg_batch(tiny_cfg, 2)
    for kw in (dict(parallel_size=1, select_best=True), dict(parallel_size=2), dict(parallel_size=2, select_best=False)):
        e = _StubEngine(tiny_cfg, max_rows=8)
        s = System(tiny_cfg, e, _args(**kw))
        dec, _ = s.t2i(ids, mask)
        p = kw["parallel_size"]
        assert [c[0] for c in e.calls] == ["prefill", "decode_image_tokens", "vq_decode"]
        assert e.calls[1][2] == dict(top_k=0, top_p=1.0)                 # no return_logprobs keyword at all
        assert e.calls[2][1][0] == 2 * p and dec.shape[0] == 2 * p and s.last_selection is None


def test_t2i_select_best_excludes_forced_positions(tiny_cfg):
    from plangen_amd.system import System
    B0, p, T = 2, 2, tiny_cfg.img_tokens
    e = _StubEngine(tiny_cfg, max_rows=2 * B0 * p)
    e.vq_encode = lambda img: torch.zeros(img.shape[0] * T, dtype=torch.int64)
    region = torch.ones(B0, T, dtype=torch.int32)
    region[:, :T // 2] = 0                                               # first half forced (mask == 0), second half free

    def lp(B, T_):
        out = torch.full((B, T_), -1.0)
        out[0, :T // 2] = NEG_INF                                        # replica 0, prompt 0: impossible forced tokens -- excluded, so it still wins on the free half
        out[0, T // 2:] = -0.5
        out[1 * B0 + 1, T // 2:] = -0.25                                 # prompt 1: replica 1 better on the free half
        out[1, :T // 2] = -0.01                                          # ... although replica 0 looks better on the forced half
        return out
    e.lp = lp
    s = System(tiny_cfg, e, _args(parallel_size=p, select_best=True, use_teacher_forcing=True))
    ids, mask = _cfg_batch(tiny_cfg, B0)
    s.t2i(ids, mask, gt_image=torch.zeros(B0, 3, 4, 4), edit_region=region)
    assert s.last_selection["replica"].tolist() == [0, 1]
    assert s.last_selection["score"].tolist() == pytest.approx([-0.5, -0.25])


def _stage1(tiny_cfg, e, B, **kw):
    from plangen_amd.system import System
    s = System(tiny_cfg, e, _args(**kw))
    ids = torch.arange(B * 3).view(B, 3).int() + 8
    batch = dict(uni_stage1_inputs_ids=ids, uni_stage1_attention_mask=torch.ones(B, 3, dtype=torch.int32))
    return s.uni_generate(batch, pred_layout=True, pred_image=False, max_new_tokens=4)


def test_layout_best_of_keeps_the_best_draw_and_reports_it(tiny_cfg):
    B, N = 2, 3
    e = _StubEngine(tiny_cfg, max_rows=8)

    def lp(R, n):
        out = torch.zeros(R, n)
        out[:, :2] = -2.0                                                # two scored columns (token, EOS)
        out[1 * B + 0, :2] = -0.5                                        # row 0: draw 1 is best
        out[2 * B + 1, :2] = -1.0                                        # row 1: draw 2 is best
        return out
    e.lp = lp
    out = _stage1(tiny_cfg, e, B, text_temperature=1.0, layout_best_of=N)
    assert [c[0] for c in e.calls] == ["prefill_embeds", "generate_text"]
    assert e.calls[0][1][0] == N * B and e.calls[1][2].get("return_logprobs") is True
    assert out["pr_layout_replica"].tolist() == [1, 2] and out["pr_layout_score"].tolist() == pytest.approx([-0.5, -1.0])
    assert out["pr_layout_ids"][:, 0].tolist() == [20 + 1 * B + 0, 20 + 2 * B + 1]      # the kept rows' tokens go on


def test_layout_best_of_errors_and_the_off_path(tiny_cfg):
    from plangen_amd.engine import PlanGenError
    e = _StubEngine(tiny_cfg, max_rows=8)
    with pytest.raises(PlanGenError, match="greedy"):
        _stage1(tiny_cfg, e, 2, layout_best_of=2)                        # text_temperature absent: greedy
    with pytest.raises(PlanGenError, match=r"(?s)12.*8|8.*12"):
        _stage1(tiny_cfg, e, 3, text_temperature=1.0, layout_best_of=4)  # 4 x 3 = 12 rows > max_rows 8
    assert e.calls == []                                                 # refused before anything ran
    for kw in (dict(text_temperature=1.0, layout_best_of=1), dict(text_temperature=1.0), dict()):
        e = _StubEngine(tiny_cfg, max_rows=8)
        out = _stage1(tiny_cfg, e, 2, **kw)
        assert [c[0] for c in e.calls] == ["prefill_embeds", "generate_text" if kw.get("text_temperature") else "generate_text_greedy"]
        assert e.calls[0][1][0] == 2 and "return_logprobs" not in e.calls[1][2]
        assert "pr_layout_replica" not in out and "pr_layout_score" not in out
