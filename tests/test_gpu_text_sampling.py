"""GPU: sampled text decode (pg_generate_text_sampled, pg_op_text_sample): temperature, top-k and top-p at vocabularies up to 102 400.
The kept sets are checked against the fp64 references of sampling_filter_ref.py (the header's rule and the transformers warpers)
outside the entries where fp32 and fp64 may legitimately decide differently; the loop is checked against the operator on its own tapped
logits and those against the oracle's forward over prompt + emitted prefix."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, get_engine, load_golden
from oracle import ref_cpu as R
from sampling_filter_ref import ambiguous, hf_keep, rule_keep

pytestmark = pytest.mark.gpu

V_FULL = 102400
LOGIT_STD = 2.4                 # measured std of the lm_head logits
AMBIGUOUS_CAP = 1e-3            # share of a non-crafted row family that may fall inside ambiguous(...)
# A k-th-value tie can only decide top_k = 1 when two logits collapse into one fp32 x = logit * (1 / T): that needs a margin of a few
# ulps of |logit| <= 32, i.e. < 2e-5.  The fixtures' own top-1 margins are asserted to be far above that.
MIN_TOP1_MARGIN = 1e-4

_S = {}


def _full(dtype="f32"):
    """The generate_fullvocab fixture's model (Janus width, 2 layers, vocab 102 400) on one engine per dtype."""
    from fullwidth_cfg import FULLV
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    if "W" not in _S:
        g = load_golden("generate_fullvocab.npz")
        ocfg = R.OracleCfg(**FULLV)
        W = R.make_weights(ocfg, seed=11)
        ws = float(sum(v.double().abs().sum() for v in W.values()))
        assert abs(ws - float(g["wsum"])) < 1e-6 * ws
        _S.update(W=W, g=g, cfg=PlanGenConfig(**FULLV), ocfg=ocfg)
    if dtype not in _S:
        e = Engine(_S["cfg"], dtype=dtype, max_rows=16, max_prompt=96, max_new=16, max_images=1, with_lm_head=True)
        e.load_state_dict(_S["W"])
        _S[dtype] = e
    return _S[dtype], _S


def _fixture(name, tiny_cfg, tiny_weights, ocfg):
    """(engine, cfg, weights, oracle cfg, golden, engine factory for a second handle)"""
    if name == "generate_tiny":
        return (get_engine(tiny_cfg, tiny_weights, "f32"), tiny_cfg, tiny_weights, ocfg, load_golden("generate_tiny.npz"),
                lambda: get_engine(tiny_cfg, tiny_weights, "f32", max_images=2))
    if name == "generate_fullvocab":
        e, s = _full("f32")
        return e, s["cfg"], s["W"], s["ocfg"], s["g"], None
    from fullwidth_cfg import FULLW
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    cfg, oc = PlanGenConfig(**FULLW), R.OracleCfg(**FULLW)
    W = R.make_weights(oc, seed=3)
    e = Engine(cfg, dtype="f32", max_rows=32, max_prompt=128, max_new=40, max_images=1, with_lm_head=True)
    e.load_state_dict(W)
    return e, cfg, W, oc, load_golden("generate_fullwidth.npz"), None


def _prefill(e, g, rows=None):
    from plangen_amd.engine import Engine
    ids, mask = torch.from_numpy(g["ids"].astype(np.int32)), torch.from_numpy(g["mask"].astype(np.int32))
    if rows is not None:
        ids, mask = ids[rows], mask[rows]
    emb = e.embed_tokens(ids.to(e.device))
    e.prefill_embeds(emb, Engine.pad_len_from_mask(mask, ids.shape[1]), position_mode=1)
    return ids, mask


def _gen(e, g, n, eos, rows=None, **kw):
    _prefill(e, g, rows)
    out = e.generate_text(n, eos, **kw)
    return (out[0].cpu(), out[1].cpu()) if isinstance(out, tuple) else out.cpu()


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["generate_tiny", "generate_fullwidth", "generate_fullvocab"])
def test_greedy_is_untouched_and_top_k_1_is_the_argmax(name, tiny_cfg, tiny_weights, ocfg):
    e, cfg, W, oc, g, _ = _fixture(name, tiny_cfg, tiny_weights, ocfg)
    eos, ref = int(g["eos"]), torch.from_numpy(g["out"].astype(np.int64))
    n = ref.shape[1]
    try:
        _prefill(e, g)
        old = e.generate_text_greedy(n, eos).cpu()
        new, lg = _gen(e, g, n, eos, temperature=0.0, return_logits=True)
        assert torch.equal(old, ref[:, :old.shape[1]]) and (ref[:, old.shape[1]:] == eos).all()
        assert torch.equal(new, old)
        assert torch.equal(_gen(e, g, n, eos, temperature=0.0, top_k=5, top_p=0.5, seed=9), old)       # greedy ignores the filters
        # the top-1 margin, from the fixture (the oracle's own logits where it stores none) and on the engine's tapped logits
        if "top_v" in g.files:
            margin = float((g["top_v"][..., 0] - g["top_v"][..., 1]).min())
        else:
            ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
            _, ol = R.generate_text_greedy(W, oc, R.embed_tokens(W, ids), mask, n, eos, return_logits=True)
            t2 = ol.topk(2, dim=-1).values
            margin = float((t2[..., 0] - t2[..., 1]).min())
        t2 = lg.topk(2, dim=-1).values
        print(f"{name}: fixture top-1 margin {margin:.3e}, engine {float((t2[..., 0] - t2[..., 1]).min()):.3e}")
        assert margin > MIN_TOP1_MARGIN and float((t2[..., 0] - t2[..., 1]).min()) > MIN_TOP1_MARGIN
        assert torch.equal(_gen(e, g, n, eos, temperature=0.7, top_k=1, seed=3), old)
        assert torch.equal(_gen(e, g, n, eos, temperature=0.7, top_k=0, top_p=1e-6, seed=4), old)
    finally:
        if name == "generate_fullwidth":
            e.close()


# ----------------------------------------------------------------------------------------------------------------- 2
def _families(V, gen):
    gauss = torch.randn(3, V, generator=gen) * LOGIT_STD
    peaked = torch.randn(3, V, generator=gen) * LOGIT_STD
    for r in range(3):
        idx = torch.randint(0, V, (min(V, 12),), generator=gen)
        peaked[r, idx] += torch.linspace(14, 8, len(idx))
    flat = torch.randn(3, V, generator=gen) * 1e-3
    return {"gaussian": gauss, "peaked": peaked, "flat": flat}


KTP = [(1.0, 50, 1.0), (1.0, 0, 0.9), (1.0, 50, 0.9), (0.7, 1000, 0.95), (1.3, 0, 0.5), (1.0, 1, 1.0), (1.0, 0, 1e-6)]
# More candidates than the select kernel's LDS holds (its walks then run over global memory).  At top_p = 0.999 the tail entries carry
# ~1e-8 of the mass each, so the reference's own +-1e-4 band around top_p spans thousands of them (2.3 % of a Gaussian row at V = 16 384 in
# fp64, independent of the device): equality outside the band is asserted, the cap on the band's size is not.
KTP_WIDE = [(0.7, 20000, 0.999)]


def _check_keep(e, rows, temp, k, p, cap=None, tag=""):
    got, _ = e.text_sample(rows, temp, k, p)
    got = got.cpu()
    amb = ambiguous(rows, temp, k, p)
    share = amb.float().mean(-1).max().item()
    ref = rule_keep(rows, temp, k, p)
    assert torch.equal(got[~amb], ref[~amb]), (tag, temp, k, p, torch.nonzero((got != ref) & ~amb)[:8].tolist())
    assert torch.equal(got[~amb], hf_keep(rows, temp, k, p)[~amb]), (tag, temp, k, p)
    if cap is not None:
        assert share <= cap, (tag, temp, k, p, share)
    return got, share


@pytest.mark.parametrize("V", [V_FULL, 16384, 16385, 7, 1])
def test_kept_sets_match_the_rule_and_the_warpers(V):
    e, _ = _full("f32")
    gen = torch.Generator().manual_seed(1000 + V)
    worst = 0.0
    for fam, rows in _families(V, gen).items():
        for temp, k, p in KTP:
            _, share = _check_keep(e, rows, temp, k, p, AMBIGUOUS_CAP if V >= 16384 else None, fam)
            worst = max(worst, share)
        for temp, k, p in KTP_WIDE:
            _check_keep(e, rows, temp, k, p, None, fam)
    print(f"V={V}: worst ambiguous share {worst:.2e}")


def test_kept_sets_on_crafted_rows():
    """The families of test_operator_on_crafted_rows at V = 102 400 (and the LDS-overflow fallback: top_p just below 1 on a flat row)."""
    e, _ = _full("f32")
    V = V_FULL
    inf, nan = float("inf"), float("nan")

    def check(rows, temp, k, p, expect=None):
        rows = torch.as_tensor(rows, dtype=torch.float32)
        got = e.text_sample(rows, temp, k, p)[0].cpu()
        ref = rule_keep(rows, temp, k, p)
        assert torch.equal(got, ref), (k, p, temp, torch.nonzero(got != ref)[:8].tolist())
        if expect is not None:
            assert torch.equal(got, torch.as_tensor(expect, dtype=torch.bool).reshape(got.shape)), (k, p)
        return got

    check(torch.full((2, V), 0.25), 1.0, 5, 1.0, torch.ones(2, V))                      # all equal: ties keep everything
    check(torch.full((1, V), -3.0), 1.0, 0, 0.1, torch.ones(1, V))
    row = torch.arange(V, dtype=torch.float32) * -1e-3
    row[10:14] = -2e-3                                                                   # copies of the third value across the k-th rank
    check(row[None], 1.0, 4, 1.0, row[None] >= -2e-3)
    check(row[None], 1.0, 3, 1.0, row[None] >= -2e-3)
    big = torch.arange(V, dtype=torch.float32) * -1e-3
    big[70000:90000] = -5.0                                                              # a 20 000-way tie across the k-th rank: more than LDS holds
    check(big[None], 1.0, 10000, 1.0, big[None] >= -5.0)
    x = torch.full((V,), -inf)
    pos = torch.arange(12) * 8191 + 5                                                    # spread over the row
    x[pos] = torch.log(torch.tensor([2.0 ** -(i + 1) for i in range(12)], dtype=torch.float64)).float()
    for p, nk in ((0.5 - 2 ** -10, 1), (0.5 + 2 ** -10, 2), (0.75 + 2 ** -10, 3), (0.875 + 2 ** -10, 4), (1e-6, 1)):
        exp = torch.zeros(V, dtype=torch.bool); exp[pos[:nk]] = True
        check(x[None], 1.0, 0, p, exp[None])
    exp = torch.zeros(V, dtype=torch.bool); exp[pos[:2]] = True
    check(x[None], 1.0, 2, 0.9, exp[None])                                               # top-k first, then top-p over the survivors
    y = torch.randn(V, generator=torch.Generator().manual_seed(5)) * LOGIT_STD
    y[3], y[7], y[99999] = -inf, nan, nan
    got = check(y[None], 1.0, 0, 0.5)
    assert not got[0, 3] and not got[0, 7] and not got[0, 99999]
    assert check(y[None], 1.0, V, 1.0).sum() == V - 3
    z = y.clone(); z[20], z[90000] = inf, inf
    check(z[None], 1.0, 0, 0.9, torch.isinf(z[None]) & (z[None] > 0))
    check(z[None], 1.0, 1, 1.0, torch.isinf(z[None]) & (z[None] > 0))
    check(y[None], 1.0, 10 * V, 1.0, torch.isfinite(y[None]))                            # top_k > V
    none = torch.full((2, V), -inf); none[1, 5] = nan
    got, tok = e.text_sample(none, 1.0, 5, 0.9)
    assert not got.any() and tok.cpu().tolist() == [0, 0]                                # nothing kept: token 0
    # top_p just below 1 on a flat row: ~all of the row is a candidate, the walks run over global memory
    flat = torch.randn(2, V, generator=torch.Generator().manual_seed(6)) * 1e-3
    for p in (0.999, 0.99999):
        amb = ambiguous(flat, 1.0, 0, p)
        got = e.text_sample(flat, 1.0, 0, p)[0].cpu()
        assert got.sum(-1).min() > 0.99 * V
        assert torch.equal(got[~amb], rule_keep(flat, 1.0, 0, p)[~amb]) and torch.equal(got[~amb], hf_keep(flat, 1.0, 0, p)[~amb])


# ----------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("temp,k,p", [(1.0, 0, 1.0), (1.0, 50, 0.9), (0.8, 0, 0.95)])
def test_draws_follow_the_filtered_softmax_chi_square(temp, k, p):
    from scipy import stats
    e, _ = _full("f32")
    gen = torch.Generator().manual_seed(77)
    row = torch.randn(V_FULL, generator=gen) * LOGIT_STD
    row[torch.randint(0, V_FULL, (40,), generator=gen)] += torch.linspace(9, 7, 40)          # top_k 50 + top_p 0.9 keeps 16 tokens of it
    B, calls = 256, 80                                                                   # 20 480 (seed, global row, step) keys
    rows = row[None].expand(B, -1).contiguous().to(e.device)
    draws = []
    for c in range(calls):
        keep, tok = e.text_sample(rows, temp, k, p, seed=1 + c % 5, row_offset=1000 * (c // 5), step=c)
        draws.append(tok.cpu())
    draws = torch.cat(draws).long()
    N = len(draws)
    keep = rule_keep(row[None], temp, k, p)[0]
    x = (row * torch.tensor(1.0 / temp, dtype=torch.float32)).double()
    prob = torch.softmax(torch.where(keep, x, torch.full_like(x, float("-inf"))), dim=-1)
    obs = torch.bincount(draws, minlength=V_FULL).double()
    amb = ambiguous(row[None], temp, k, p)[0]
    assert (obs[~keep & ~amb] == 0).all()                                                # filtered-out tokens are never drawn
    exp = prob * N
    single = exp >= 5
    o = torch.cat([obs[single], obs[~single].sum()[None]])
    xx = torch.cat([exp[single], exp[~single].sum()[None]])
    if xx[-1] < 5:                                                                       # pooled rest too small: fold it into the smallest bin
        o, xx = torch.cat([o[:-2], (o[-2] + o[-1])[None]]), torch.cat([xx[:-2], (xx[-2] + xx[-1])[None]])
    assert len(o) >= 5, len(o)
    chi2 = ((o - xx) ** 2 / xx).sum().item()
    pval = 1 - stats.chi2.cdf(chi2, df=len(o) - 1)
    print(f"T={temp} top_k={k} top_p={p}: {N} draws, {len(o)} bins, chi2 {chi2:.1f}, p-value {pval:.3g}")
    assert pval > 1e-4, (chi2, pval)
    # a draw that survives the filter equals the unfiltered draw for the same key
    if k or p < 1.0:
        _, t_off = e.text_sample(rows, temp, 0, 1.0, seed=3, row_offset=17, step=5)
        _, t_on = e.text_sample(rows, temp, k, p, seed=3, row_offset=17, step=5)
        surv = keep[t_off.cpu().long()]
        assert surv.any() and torch.equal(t_on.cpu()[surv], t_off.cpu()[surv])


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["generate_tiny", "generate_fullvocab"])
def test_loop_equals_operator_equals_model(name, tiny_cfg, tiny_weights, ocfg):
    from test_gpu_fullwidth import LOGIT_TOL_F32 as TOL_FULL            # the teacher-forced fp32 logit bounds of the existing text / image tests
    from test_gpu_path import LOGIT_TOL_F32 as TOL_TINY
    e, cfg, W, oc, g, _ = _fixture(name, tiny_cfg, tiny_weights, ocfg)
    tol = TOL_TINY if name == "generate_tiny" else TOL_FULL
    n, seed, temp, k, p = 10, 23, 1.0, 50, 0.9
    ids, mask = torch.from_numpy(g["ids"].astype(np.int32)), torch.from_numpy(g["mask"].astype(np.int32))
    B, V = ids.shape[0], cfg.vocab
    for eos, min_new in ((int(g["eos"]), 3), (None, 0)):
        if eos is None:                  # an EOS that is certain to be drawn: what row 0 emitted at step 2 of the first run (same keys)
            eos = int(out_prev[0, 2])
        out, lg = _gen(e, g, n, eos, min_new_tokens=min_new, temperature=temp, top_k=k, top_p=p, seed=seed, return_logits=True)
        out_prev = out
        L = out.shape[1]
        assert lg.shape == (L, B, V)
        unf = torch.ones(B, dtype=torch.bool)
        for t in range(L):
            assert torch.isinf(lg[t, :, eos]).all() == (t < min_new)                     # EOS suppressed before the filters, only while t < min_new
            keep, tok = e.text_sample(lg[t], temp, k, p, seed=seed, row_offset=0, step=t)
            tok = tok.cpu().long()
            assert torch.equal(out[unf, t], tok[unf]), (t, out[:, t], tok)
            assert keep.cpu()[torch.arange(B), tok].all()
            assert (out[~unf, t] == eos).all()                                           # finished rows emit eos
            if t < min_new:
                assert (out[:, t] != eos).all()
            unf &= out[:, t] != eos
            if not unf.any():
                assert L == t + 1                                                        # out_len = the first all-finished column
        assert L == n or not unf.any()
        if min_new == 0:
            assert not unf[0] and (out[0, 3:] == eos).all()                                  # row 0 drew EOS at step 2 at the latest
        # tapped logits == the oracle's forward over prompt + the emitted prefix
        _, ol = R.generate_text_greedy(W, oc, R.embed_tokens(W, ids), mask, L, eos, min_new_tokens=min_new, force_tokens=out, return_logits=True)
        fin = torch.isfinite(ol)
        assert torch.equal(fin, torch.isfinite(lg[:ol.shape[0]]))
        err = (lg[:ol.shape[0]][fin] - ol[fin]).abs().max().item()
        print(f"{name} eos={eos} min_new={min_new}: {L} steps, tapped-logit error vs the oracle {err:.2e} (bound {tol})")
        assert err < tol, err


# ----------------------------------------------------------------------------------------------------------------- 5
def test_execution_forms_agree_and_graph_replays_new_parameters(tiny_cfg, tiny_weights, ocfg):
    e, cfg, W, oc, g, second = _fixture("generate_tiny", tiny_cfg, tiny_weights, ocfg)
    n, eos = 12, cfg.eos_id
    P = [dict(temperature=1.0, top_k=30, top_p=0.9, seed=41), dict(temperature=0.7, top_k=5, top_p=1.0, seed=42),
         dict(temperature=1.2, top_k=0, top_p=1.0, seed=43), dict(temperature=1.0, top_k=0, top_p=0.8, seed=41)]
    run = lambda eng, kw, rows=None: _gen(eng, g, n, eos, rows=rows, min_new_tokens=n, **kw)
    base = [run(e, kw) for kw in P]
    assert len({tuple(b.reshape(-1).tolist()) for b in base}) == len(P)
    assert torch.equal(run(e, P[0]), base[0])                                            # same seed -> same ids
    assert not torch.equal(run(e, dict(P[0], seed=99)), base[0])
    e2 = second()
    e.set_option("use_graph", 1)
    try:
        for i in (0, 3, 1, 2, 0):        # filtered graph captured by the first call, replayed with new values; then the unfiltered structure
            assert torch.equal(run(e, P[i]), base[i]), i
            assert torch.equal(run(e2, P[i]), base[i]), i                                # stream launches on another handle
    finally:
        e.set_option("use_graph", 0)
    # a row's ids do not depend on its neighbours; two shards with rng_image_offset == one batch
    for i in (0, 2):
        e2.set_option("rng_image_offset", 1)
        try:
            tail = run(e2, P[i], rows=slice(1, 3))
        finally:
            e2.set_option("rng_image_offset", 0)
        assert torch.equal(tail, base[i][1:3]), i
        assert torch.equal(run(e2, P[i], rows=slice(0, 1)), base[i][0:1]), i
    # two rows with the same prompt draw different texts
    ids = torch.from_numpy(g["ids"])
    same = torch.stack([ids[0], ids[0]])
    from plangen_amd.engine import Engine
    msk = torch.from_numpy(g["mask"])[[0, 0]]
    e.prefill_embeds(e.embed_tokens(same.to(e.device)), Engine.pad_len_from_mask(msk, same.shape[1]), position_mode=1)
    two = e.generate_text(n, eos, min_new_tokens=n, **P[0]).cpu()
    assert torch.equal(two[0], base[0][0]) and not torch.equal(two[0], two[1])


# ----------------------------------------------------------------------------------------------------------------- 6
def test_bf16_fullvocab_runs_deterministic_and_in_the_kept_set():
    e, s = _full("bf16")
    g = s["g"]
    n, eos, kw = 8, s["cfg"].eos_id, dict(temperature=1.0, top_k=50, top_p=0.9, seed=5)
    out, lg = _gen(e, g, n, eos, min_new_tokens=n, return_logits=True, **kw)
    assert torch.equal(_gen(e, g, n, eos, min_new_tokens=n, **kw), out)
    B = out.shape[0]
    checked = 0
    for t in range(n):
        tok = out[:, t]
        amb = ambiguous(lg[t], 1.0, 50, 0.9)[torch.arange(B), tok]
        ok = hf_keep(lg[t], 1.0, 50, 0.9)[torch.arange(B), tok] & rule_keep(lg[t], 1.0, 50, 0.9)[torch.arange(B), tok]
        assert (ok | amb).all(), t
        checked += int((~amb).sum())
    assert checked >= 0.99 * B * n


# ----------------------------------------------------------------------------------------------------------------- 7
def test_argument_errors_leave_the_handle_usable(tiny_cfg, tiny_weights):
    from plangen_amd.engine import Engine, PlanGenError
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    eos = int(g["eos"])
    for k, p in ((-1, 1.0), (0, 0.0), (0, 1.5), (0, float("nan"))):
        _prefill(e, g)
        with pytest.raises(PlanGenError):
            e.generate_text(4, eos, temperature=1.0, top_k=k, top_p=p)
        with pytest.raises(PlanGenError):
            e.text_sample(torch.zeros(1, 8), 1.0, k, p)
    with pytest.raises(PlanGenError):
        e.text_sample(torch.zeros(1, tiny_cfg.vocab + 1), 1.0, 5, 1.0)
    with pytest.raises(PlanGenError):
        e.text_sample(torch.zeros(1, 8), 0.0, 5, 1.0)
    nohead = Engine(tiny_cfg, dtype="f32", max_rows=4, max_prompt=16, max_images=2)
    nohead.load_state_dict(tiny_weights)
    ids = torch.from_numpy(g["ids"].astype(np.int32))
    nohead.prefill(ids, [0] * ids.shape[0], position_mode=1)
    with pytest.raises(PlanGenError):
        nohead.generate_text(4, eos, temperature=1.0, top_k=5)
    nohead.close()
    _prefill(e, g)
    assert np.array_equal(e.generate_text_greedy(10, eos).cpu().numpy(), g["out"])


# ----------------------------------------------------------------------------------------------------------------- 8
def test_through_uni_generate(tiny_cfg, tiny_weights, ocfg):
    from types import SimpleNamespace
    from plangen_amd.system import System, pad_input_ids
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    gen = torch.Generator().manual_seed(51)
    prompt = torch.randint(8, tiny_cfg.vocab, (7,), generator=gen).tolist()
    other = torch.randint(8, tiny_cfg.vocab, (4,), generator=gen).tolist()
    neg = torch.randint(8, tiny_cfg.vocab, (5,), generator=gen).tolist()
    stage1 = [prompt, prompt, other]                                   # two rows carry the same prompt
    ids1, mask1 = pad_input_ids(stage1, tiny_cfg.pad_id)
    l2p = lambda i, new_ids: stage1[i] + [t for t in new_ids if t != tiny_cfg.eos_id][:6] + [9]
    batch = dict(uni_stage1_inputs_ids=ids1, uni_stage1_attention_mask=mask1, neg_inputs_ids=neg)
    base = dict(seed=3, parallel_size=1, cfg_weight=5.0, temperature=0.0, use_teacher_forcing=False, debug_max_seq_len=None,
                janus_hw=tiny_cfg.img_size, neg_prompt="", use_neg_box=False)
    ref_layout = R.generate_text_greedy(tiny_weights, ocfg, R.embed_tokens(tiny_weights, ids1), mask1, 8, tiny_cfg.eos_id)
    # keys absent: the greedy layouts of today (the oracle's)
    out = System(tiny_cfg, e, SimpleNamespace(**base)).uni_generate(batch, pred_layout=True, pred_image=False, max_new_tokens=8)
    assert np.array_equal(out["pr_layout_ids"].cpu().numpy(), ref_layout.numpy())
    s = System(tiny_cfg, e, SimpleNamespace(text_temperature=1.0, text_top_k=50, text_top_p=0.9, **base))
    runs = []
    for _ in range(2):
        plan = s.uni_generate(batch, pred_layout=True, pred_image=False, max_new_tokens=8, min_new_tokens=8)       # task 'plan'
        two = s.uni_generate(batch, pred_layout=True, layout_to_prompt=l2p, max_new_tokens=8, min_new_tokens=8)    # task 'uni_2stage'
        runs.append((plan["pr_layout_ids"].cpu(), two["pr_layout_ids"].cpu(), two["pr_tokens"].cpu(), two["pr_image"].cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                        # same seed: the whole output repeats
    lay = runs[0][1]
    assert torch.equal(runs[0][0], lay) and not torch.equal(lay[0], lay[1])          # same prompt, different rows: different layouts
    assert lay.shape == (3, 8) and runs[0][2].shape == (3, tiny_cfg.img_tokens)
    _prefill_ids = e.embed_tokens(ids1.to(e.device))
    from plangen_amd.engine import Engine
    e.prefill_embeds(_prefill_ids, Engine.pad_len_from_mask(mask1, ids1.shape[1]), position_mode=1)
    direct = e.generate_text(8, tiny_cfg.eos_id, min_new_tokens=8, temperature=1.0, top_k=50, top_p=0.9, seed=3).cpu()
    assert torch.equal(direct, lay)


@pytest.mark.parametrize("task", ["uni_2stage", "plan"])
def test_through_the_cli(tmp_path, task):
    import json
    import train
    from project.plangen.plangen_base import System as CliSystem

    def run(sub, *extra):
        opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='f32'", "temperature=0.0", f"out_path={str(tmp_path / sub)!r}",
                f"test_data.task_type={task!r}", "max_new_tokens=12", "max_prompt=160", *extra]
        a = train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
        m = CliSystem(a, None)
        seen, ids = [], []
        orig, orig_greedy = m.engine.generate_text, m.engine.generate_text_greedy

        def spy(*args, **kw):
            seen.append(kw)
            ids.append(orig(*args, **kw))
            return ids[-1]

        def spy_greedy(*args, **kw):
            ids.append(orig_greedy(*args, **kw))
            return ids[-1]
        m.engine.generate_text, m.engine.generate_text_greedy = spy, spy_greedy
        m.setup_data(None)
        m.resume(None)
        r = m.validation(0)
        m.engine.close()
        base = os.path.join(str(tmp_path / sub), "test", f"synthetic_{task}_1")
        assert r["out_dir"] == os.path.join(base, "0")
        for d in ("gt_image", "pr_image", "image_ids", "gt_image_ids"):
            assert os.path.isdir(os.path.join(base, "0", d))
        lay = json.load(open(os.path.join(base, "0_batch", "0_layout.json")))
        pngs = {f: open(os.path.join(base, "0", "pr_image", f), "rb").read() for f in sorted(os.listdir(os.path.join(base, "0", "pr_image")))}
        return lay, pngs, seen, [t.cpu() for t in ids]

    keys = ("text_temperature=1.0", "text_top_k=50", "text_top_p=0.9")
    lay_a, png_a, seen, ids_a = run("a", *keys)
    assert seen and all(kw["temperature"] == 1.0 and kw["top_k"] == 50 and kw["top_p"] == 0.9 and kw["seed"] == 0 for kw in seen)
    lay_b, png_b, _, ids_b = run("b", *keys)
    assert lay_a == lay_b and png_a == png_b and all(torch.equal(x, y) for x, y in zip(ids_a, ids_b))                            # same seed: identical output tree
    assert len(png_a) == (2 if task == "uni_2stage" else 0)
    lay_g, png_g, seen_g, ids_g = run("g")
    assert not seen_g and len(ids_g) == len(ids_a) == 1                 # keys absent: the greedy entry point, as before
    assert ids_g[0].shape[0] == ids_a[0].shape[0] and not torch.equal(ids_g[0][:, :4], ids_a[0][:, :4])
