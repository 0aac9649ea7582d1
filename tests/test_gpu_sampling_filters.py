"""GPU: top-k / top-p (nucleus) filtering of the image-token sampler (pg_decode_image_tokens_filtered, pg_op_sample_filter).
Teacher-forced tokens without a mask fix the context, so logits_out is known and every emitted token can be checked against the
kept set of the transformers warpers applied in float64 (sampling_filter_ref.py).  Rows where fp32 and fp64 may legitimately
decide differently are skipped and counted."""
import pytest
import torch

from conftest import get_engine
from sampling_filter_ref import ambiguous, hf_keep, rule_keep

pytestmark = pytest.mark.gpu

MEMBER_KP = [(1, 1.0), (50, 1.0), (0, 0.9), (200, 0.7), ("V", 1.0), (0, 1e-6)]
TEMPS = [0.7, 1.0, 1.3]


def _prompt(cfg, nimg, seed, lens=(9, 6, 11, 7, 5, 8, 10, 4)):
    from plangen_amd.system import t2i_infer_collate_batch
    g = torch.Generator().manual_seed(seed)
    cond = [torch.randint(8, cfg.vocab, (lens[i % len(lens)],), generator=g).tolist() for i in range(nimg)]
    neg = torch.randint(8, cfg.vocab, (4,), generator=g).tolist()
    ids, mask = t2i_infer_collate_batch(cond, neg, cfg.pad_id, cfg.img_tokens)
    pad = (ids.shape[1] - mask[:, :ids.shape[1]].sum(-1)).tolist()
    _MASKS[id(ids)] = mask
    return ids, pad, g


_MASKS = {}


def _decode_filtered_raw(e, T, cfgw, temp, k, p, seed, force=None):
    """The new entry point called directly (the Python wrapper routes (0, 1.0) to pg_decode_image_tokens)."""
    B = e.R // 2
    out = torch.zeros((B, T), dtype=torch.int32, device=e.device)
    ft = e._dev(force, torch.int32) if force is not None else None
    e._check(e.lib.pg_decode_image_tokens_filtered(e.h, T, float(cfgw), float(temp), int(k), float(p), int(seed), e._p(ft), None,
                                                   e._p(out), None, e.stream), "pg_decode_image_tokens_filtered")
    return out.cpu()


def _check_membership(toks, logits, temp, k, p, V):
    """toks [B, T], logits [T, B, V]: every emitted token in the HF kept set (ambiguous rows skipped); returns (checked, skipped)."""
    k = V if k == "V" else k
    rows = logits.permute(1, 0, 2).reshape(-1, V).cpu()          # [B*T, V] in toks' order
    t = toks.reshape(-1).long()
    n = torch.arange(len(t))
    amb = ambiguous(rows, temp, k, p)[n, t]
    keep = hf_keep(rows, temp, k, p)
    ok = keep[n, t]
    bad = (~ok) & (~amb)
    assert not bad.any(), (k, p, temp, torch.nonzero(bad).flatten()[:8].tolist())
    return int((~amb).sum()), int(amb.sum())


@pytest.fixture(scope="module")
def forced(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, g = _prompt(tiny_cfg, 2, 81)
    T = 12
    force = torch.randint(0, tiny_cfg.img_vocab, (2, T), generator=g).int()
    return e, ids, pad, force, T


def test_filters_off_equal_today_tiny(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 82)
    T = 16
    for temp, seed in ((1.0, 5), (1.3, 6)):
        e.prefill(ids, pad)
        ref = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=temp, seed=seed).cpu()
        e.prefill(ids, pad)
        assert torch.equal(_decode_filtered_raw(e, T, 5.0, temp, 0, 1.0, seed), ref)
    e.prefill(ids, pad)
    greedy = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=0.0).cpu()
    for k, p in ((1, 1.0), (7, 0.3), (0, 0.5)):
        e.prefill(ids, pad)
        assert torch.equal(e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=0.0, top_k=k, top_p=p).cpu(), greedy)


def test_filters_off_equal_today_fullwidth_and_filtered_membership():
    """img_vocab 16 384 (the production sampler width), 8 images: off == today; (1000, 0.95) draws stay in the kept set."""
    from fullwidth_cfg import FULLW
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    cfg = PlanGenConfig(**FULLW)
    e = Engine(cfg, dtype="bf16", max_rows=16, max_prompt=32, max_new=16, max_images=8)
    e.init_synthetic(seed=3)
    ids, pad, g = _prompt(cfg, 8, 83)
    T = 8
    e.prefill(ids, pad)
    ref = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=1.0, seed=11).cpu()
    e.prefill(ids, pad)
    assert torch.equal(_decode_filtered_raw(e, T, 5.0, 1.0, 0, 1.0, 11), ref)
    force = torch.randint(0, cfg.img_vocab, (8, T), generator=g).int()
    checked = skipped = 0
    for k, p, temp in ((1000, 0.95, 1.0), (0, 0.8, 1.3), (20, 1.0, 0.7)):
        e.prefill(ids, pad)
        toks, lg = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=temp, seed=12, force_tokens=force, return_logits=True,
                                         top_k=k, top_p=p)
        c, s = _check_membership(toks.cpu(), lg, temp, k, p, cfg.img_vocab)
        checked, skipped = checked + c, skipped + s
    assert skipped < 0.01 * (checked + skipped), (checked, skipped)
    e.close()


def test_kept_set_membership_and_subset_property(tiny_cfg, forced):
    e, ids, pad, force, T = forced
    V = tiny_cfg.img_vocab
    checked = skipped = qualify = total = 0
    for temp in TEMPS:
        e.prefill(ids, pad)
        off, lg = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=temp, seed=31, force_tokens=force, return_logits=True)
        off = off.cpu()
        for k, p in MEMBER_KP:
            kk = V if k == "V" else k
            e.prefill(ids, pad)
            on, lg2 = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=temp, seed=31, force_tokens=force, return_logits=True,
                                            top_k=kk, top_p=p)
            on = on.cpu()
            assert torch.equal(lg2, lg)                              # forced context: the logits do not depend on the draws
            c, s = _check_membership(on, lg, temp, kk, p, V)
            checked, skipped = checked + c, skipped + s
            rows = lg.permute(1, 0, 2).reshape(-1, V).cpu()
            if kk == 1 or p == 1e-6:                                 # these keep only the argmax of mixed
                top2 = torch.topk(rows, 2, dim=-1).values
                assert (top2[:, 0] > top2[:, 1]).all()
                assert torch.equal(on.reshape(-1).long(), rows.argmax(-1))
            # subset property: where the unfiltered draw survives the filter, the filtered draw equals it
            keep = rule_keep(rows, temp, kk, p)
            t_off = off.reshape(-1).long()
            surv = keep[torch.arange(len(t_off)), t_off]
            assert torch.equal(on.reshape(-1)[surv], off.reshape(-1)[surv]), (k, p, temp)
            if k != "V":
                qualify += int(surv.sum()); total += len(t_off)
    assert skipped < 0.01 * (checked + skipped), (checked, skipped)
    assert qualify >= 0.2 * total, (qualify, total)


def test_sampled_frequencies_follow_filtered_softmax_chi_square(tiny_cfg, tiny_weights, ocfg):
    """test_gpu_edges.py's chi-square protocol (600 seeds, bins of expected count >= 20) against HF-warped softmax at
    top_k=40, top_p=0.9, T=1.3; filtered-out tokens are never drawn."""
    from scipy import stats
    from oracle import ref_cpu as R
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, g = _prompt(tiny_cfg, 2, 84)
    mask = _MASKS[id(ids)]
    T, N, temp, k, p = 3, 600, 1.3, 40, 0.9
    force = torch.randint(0, tiny_cfg.img_vocab, (2, T), generator=g).int()
    _, logits = R.sample_image(tiny_weights, ocfg, R.embed_tokens(tiny_weights, ids), mask, 2.0, n_tokens=T,
                               force_tokens=force, return_logits=True)           # [T, B, V]
    draws = []
    for seed in range(N):
        e.prefill(ids, pad)
        draws.append(e.decode_image_tokens(T=T, cfg_weight=2.0, temperature=temp, seed=seed, force_tokens=force, top_k=k, top_p=p).cpu())
    draws = torch.stack(draws)                                                   # [N, B, T]
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    for t in range(T):
        for b in range(2):
            x = TopPLogitsWarper(p)(None, TopKLogitsWarper(k)(None, TemperatureLogitsWarper(temp)(None, logits[t, b:b + 1].double())))
            exp = torch.softmax(x, dim=-1)[0] * N
            obs = torch.bincount(draws[:, b, t].long(), minlength=tiny_cfg.img_vocab).double()
            assert (obs[exp == 0] == 0).all(), (t, b)
            order = torch.argsort(exp, descending=True)
            o, xx, co, cx = [], [], 0.0, 0.0
            for v in order.tolist():
                if exp[v] == 0:
                    break
                co += obs[v].item(); cx += exp[v].item()
                if cx >= 20:
                    o.append(co); xx.append(cx); co = cx = 0.0
            if cx > 0:
                o[-1] += co; xx[-1] += cx
            o, xx = torch.tensor(o), torch.tensor(xx)
            assert len(o) >= 5, len(o)
            chi2 = ((o - xx) ** 2 / xx).sum().item()
            pval = 1 - stats.chi2.cdf(chi2, df=len(o) - 1)
            assert pval > 1e-4, (t, b, chi2, pval)


def test_operator_on_crafted_rows(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    V = tiny_cfg.img_vocab
    inf, nan = float("inf"), float("nan")

    def check(rows, temp, k, p, expect=None):
        rows = torch.as_tensor(rows, dtype=torch.float32)
        got = e.sample_filter(rows, temp, k, p).cpu()
        ref = rule_keep(rows, temp, k, p)
        assert torch.equal(got, ref), (k, p, temp, torch.nonzero(got != ref)[:8].tolist())
        if expect is not None:
            assert torch.equal(got, torch.as_tensor(expect, dtype=torch.bool).reshape(got.shape)), (k, p, got)
        return got

    # all-equal rows: every filter keeps everything (ties)
    check(torch.full((2, V), 0.25), 1.0, 5, 1.0, torch.ones(2, V))
    check(torch.full((1, V), -3.0), 1.0, 0, 0.1, torch.ones(1, V))
    # ties exactly at the k-th value: all tied entries kept
    row = torch.arange(V, dtype=torch.float32) * -1.0
    row[10:14] = -2.0                                   # ranks 3.. hold four copies of -2
    check(row[None], 1.0, 4, 1.0, row[None] >= -2.0)
    check(row[None], 1.0, 3, 1.0, row[None] >= -2.0)
    # top-p boundary from binary fractions: probabilities 1/2, 1/4, 1/8, ... (masses above: 0, 1/2, 3/4, 7/8, ...)
    x = torch.full((V,), -inf)
    x[:12] = torch.log(torch.tensor([2.0 ** -(i + 1) for i in range(12)], dtype=torch.float64)).float()
    for p, nk in ((0.5 - 2 ** -10, 1), (0.5 + 2 ** -10, 2), (0.75 + 2 ** -10, 3), (0.875 + 2 ** -10, 4), (1e-6, 1)):
        check(x[None], 1.0, 0, p, torch.arange(V)[None] < nk)
    check(x[None], 1.0, 2, 0.9, torch.arange(V)[None] < 2)            # top-k first, then top-p over the survivors
    # +-inf and NaN: -inf / NaN never kept; +inf entries hold all the mass
    y = torch.randn(V, generator=torch.Generator().manual_seed(5))
    y[3], y[7], y[9] = -inf, nan, nan
    got = check(y[None], 1.0, 0, 0.5)
    assert not got[0, 3] and not got[0, 7] and not got[0, 9]
    got = check(y[None], 1.0, V, 1.0)
    assert got.sum() == V - 3
    z = y.clone(); z[20], z[30] = inf, inf
    check(z[None], 1.0, 0, 0.9, torch.isinf(z[None]) & (z[None] > 0))
    check(z[None], 1.0, 1, 1.0, torch.isinf(z[None]) & (z[None] > 0))
    # k > V keeps everything finite
    check(y[None], 1.0, 10 * V, 1.0, torch.isfinite(y[None]))
    # random rows at V = 256 and 16 384 (the 16 384-wide case on a full-vocabulary handle)
    g = torch.Generator().manual_seed(6)
    rows = torch.randn(16, V, generator=g) * 3
    for temp, k, p in ((1.0, 17, 1.0), (0.7, 0, 0.8), (1.3, 100, 0.6), (1.0, 3, 0.3)):
        amb = ambiguous(rows, temp, k, p, margin=1e-6)
        assert amb.sum() <= 0.01 * rows.numel()
        got = e.sample_filter(rows, temp, k, p).cpu()
        assert torch.equal(got[~amb], rule_keep(rows, temp, k, p)[~amb])
        assert torch.equal(got[~amb], hf_keep(rows, temp, k, p)[~amb])
    from fullwidth_cfg import FULLW
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    ew = Engine(PlanGenConfig(**dict(FULLW, n_layers=1)), dtype="bf16", max_rows=2, max_prompt=8, max_new=2, max_images=1)
    rows = torch.randn(8, 16384, generator=g) * 4
    for temp, k, p in ((1.0, 1000, 0.95), (1.0, 0, 0.9), (0.8, 50, 1.0)):
        amb = ambiguous(rows, temp, k, p, margin=1e-6)
        got = ew.sample_filter(rows, temp, k, p).cpu()
        assert amb.sum() <= 0.01 * rows.numel()
        assert torch.equal(got[~amb], hf_keep(rows, temp, k, p)[~amb])
    ew.close()


@pytest.fixture(scope="module")
def wide_engine(tiny_cfg):
    """A handle whose text AND image vocabularies admit rows up to SEL_MAXV = 16 384 (operators only: no weights loaded)."""
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    e = Engine(PlanGenConfig(**dict(tiny_cfg.model_dict(), vocab=16384, img_vocab=16384)), dtype="f32", max_rows=2, max_prompt=8, max_new=2,
               max_images=1)
    yield e
    e.close()


@pytest.mark.parametrize("V", [17, 1000, 4100, 16384])
def test_image_select_and_text_select_keep_the_same_set(V, wide_engine):
    """cfg_select_kernel (pg_op_sample_filter) and text_select_kernel (pg_op_text_sample) promise one rule -- the same integer keys, the same
    64-bit fixed-point masses -- so their kept masks are equal bit for bit, ties at the k-th value and at the top-p boundary and
    non-finite entries included; on Gaussian rows both are the rule of sampling_filter_ref outside ambiguous(...).
    V = 16 384 is the largest row of the image kernel and the fullest LDS candidate list of the text kernel."""
    e = wide_engine
    inf, nan = float("inf"), float("nan")
    gauss = torch.randn(3, V, generator=torch.Generator().manual_seed(900 + V)) * 2.4
    special = torch.randn(3, V, generator=torch.Generator().manual_seed(901 + V)) * 2.4
    special[0, 1], special[0, 5], special[0, V - 1], special[0, V // 2], special[0, 11] = -inf, inf, nan, inf, nan
    special[1] = -inf
    special[2] = 0.375
    for name, rows in (("gauss", gauss), ("quantised", torch.round(gauss / 0.25) * 0.25), ("special", special)):
        for temp, k, p in ((1.0, 0, 0.9), (0.7, 50, 1.0), (1.0, 50, 0.9), (1.3, 1000, 0.95), (1.0, V, 0.5), (1.0, 1, 1.0)):
            img = e.sample_filter(rows, temp, k, p).cpu()
            txt = e.text_sample(rows, temp, k, p)[0].cpu()
            assert torch.equal(img, txt), (name, V, temp, k, p, torch.nonzero(img != txt)[:8].tolist())
            if name == "gauss":
                amb = ambiguous(rows, temp, k, p)
                ref = rule_keep(rows, temp, k, p)
                assert torch.equal(img[~amb], ref[~amb]), (V, temp, k, p, torch.nonzero((img != ref) & ~amb)[:8].tolist())


def test_execution_forms_agree_and_graph_replays_new_parameters(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 85)
    T = 12

    def run(eng, k, p, seed=41, i=ids, pd=pad):
        eng.prefill(i, pd)
        return eng.decode_image_tokens(T=T, cfg_weight=5.0, temperature=1.0, seed=seed, top_k=k, top_p=p).cpu()

    base = {kp: run(e, *kp) for kp in ((30, 0.9), (5, 1.0))}
    assert not torch.equal(base[(30, 0.9)], base[(5, 1.0)])
    for opt, val in (("use_graph", 1), ("lanes", 2)):
        e.set_option(opt, val)
        try:
            for kp in ((30, 0.9), (5, 1.0), (30, 0.9)):      # one captured graph replayed with different (top_k, top_p)
                assert torch.equal(run(e, *kp), base[kp]), (opt, kp)
        finally:
            e.set_option(opt, 0 if opt == "use_graph" else 1)
    # two handles split by rng_image_offset: image 1 alone on a second handle draws what the batch drew
    e2 = get_engine(tiny_cfg, tiny_weights, "f32", max_images=2)
    e2.set_option("rng_image_offset", 1)
    try:
        one = run(e2, 30, 0.9, i=ids[2:4], pd=pad[2:4])
    finally:
        e2.set_option("rng_image_offset", 0)
    assert torch.equal(one[0], base[(30, 0.9)][1])


def test_argument_errors_leave_the_handle_usable(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 86)
    for k, p in ((-1, 1.0), (0, 0.0), (0, -0.5), (0, 1.5), (0, float("nan"))):
        e.prefill(ids, pad)
        with pytest.raises(PlanGenError):
            e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=1.0, top_k=k, top_p=p)
        with pytest.raises(PlanGenError):
            e.sample_filter(torch.zeros(1, 8), 1.0, k, p)
    with pytest.raises(PlanGenError):
        e.sample_filter(torch.zeros(1, tiny_cfg.img_vocab + 1), 1.0, 5, 1.0)
    e.prefill(ids, pad)
    ref = e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0).cpu()
    e.prefill(ids, pad)
    assert torch.equal(e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0).cpu(), ref)


def test_through_system_t2i_and_the_cli(tmp_path, tiny_cfg, tiny_weights):
    from types import SimpleNamespace
    from plangen_amd.system import System
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 87)
    mask = _MASKS[id(ids)]
    args = SimpleNamespace(seed=3, parallel_size=1, cfg_weight=5.0, temperature=1.0, top_k=9, top_p=0.8, use_teacher_forcing=False,
                           debug_max_seq_len=None, janus_hw=tiny_cfg.img_size, neg_prompt="", use_neg_box=False)
    s = System(tiny_cfg, e, args)
    s.t2i(ids, mask)
    toks = s.last_generated_tokens.cpu()
    e.prefill(ids, pad)
    direct, lg = e.decode_image_tokens(T=tiny_cfg.img_tokens, cfg_weight=5.0, temperature=1.0, seed=3, return_logits=True, top_k=9, top_p=0.8)
    assert torch.equal(toks, direct.cpu())
    c, sk = _check_membership(toks, lg, 1.0, 9, 0.8, tiny_cfg.img_vocab)
    assert sk < 0.01 * (c + sk)
    # train.py --opt top_k=... top_p=...: the values reach the engine call
    import os
    import train
    from conftest import ROOT
    from project.plangen.plangen_base import System as CliSystem
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='f32'", "temperature=1.0", f"out_path={str(tmp_path)!r}",
            "test_data.task_type='uni'", "max_new_tokens=12", "max_prompt=160", "top_k=5", "top_p=0.7"]
    a = train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
    m = CliSystem(a, None)
    assert m.args.top_k == 5 and m.args.top_p == 0.7
    seen = []
    orig = m.engine.decode_image_tokens

    def spy(T, cfg_weight, temperature, seed, ft, fm, return_logits=False, **kw):
        out, lg = orig(T, cfg_weight, temperature, seed, ft, fm, True, **kw)
        seen.append((out.cpu(), lg, kw.get("top_k"), kw.get("top_p")))
        return out
    m.engine.decode_image_tokens = spy
    m.setup_data(None)
    m.resume(None)
    m.validation(0)
    assert seen and all(k == 5 and p == 0.7 for _, _, k, p in seen)
    for out, lg, _, _ in seen:
        c, sk = _check_membership(out, lg, 1.0, 5, 0.7, m.cfg.img_vocab)
        assert sk < 0.01 * (c + sk)
    m.engine.close()
