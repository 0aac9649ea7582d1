"""GPU: sample plans through the C ABI (pg_request_sample_plan + pg_decode_image_tokens[_filtered]) on the tiny config, B = 3, T = 8.  Everything is compared
bit for bit against scalar calls on the SAME batch shape (same GEMM splits): a constant plan is the scalar call; image b of a planned call is image b of the
scalar call with b's parameters; step t of a per-step plan on a forced trajectory is step t of the scalar call at that weight."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import get_engine
from plangen_amd import _lib
from plangen_amd.engine import PlanGenError
from plangen_amd.guidance import SamplePlan, replicate
from test_gpu_sampling_filters import _prompt

pytestmark = pytest.mark.gpu
B, T = 3, 8
SEED = 17
# per image: (cfg_weight, temperature, top_k, top_p)
IMG = ((1.0, 0.0, 4, 0.5), (5.0, 0.9, 0, 1.0), (3.0, 1.2, 9, 0.8))


def _eq(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def _run(e, prefill, **kw):
    prefill()
    res = e.decode_image_tokens(T=T, return_logits=True, **kw)
    torch.cuda.synchronize()
    out = dict(tokens=res[0].cpu(), logits=res[1].cpu())
    i = 2
    if kw.get("return_logprobs"):
        out["logprobs"] = res[i].cpu(); i += 1
    if kw.get("return_stats"):
        out.update({f"stats.{k}": v.cpu() for k, v in res[i].items()})
    return out


def _same(a, b, what, rows=None):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if rows is not None:
            x, y = (x[:, rows], y[:, rows]) if k == "logits" else (x[rows], y[rows])
        assert _eq(x, y), (what, k)


def _full_plan(n=B):
    return SamplePlan(cfg_weight=[IMG[b % 3][0] for b in range(n)], temperature=[IMG[b % 3][1] for b in range(n)], top_k=[IMG[b % 3][2] for b in range(n)],
                      top_p=[IMG[b % 3][3] for b in range(n)])


@pytest.fixture(scope="module")
def eng(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, B, 131)
    return e, (lambda: e.prefill(ids, pad))


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=0.8), dict(temperature=0.8, top_k=9, top_p=0.8)], ids=["greedy", "sampled", "filtered"])
def test_constant_plan_is_the_scalar_call(eng, kw):
    e, pf = eng
    kw = dict(kw, cfg_weight=5.0, seed=SEED, return_logprobs=True, return_stats=2)
    ref = _run(e, pf, **kw)
    full = SamplePlan(cfg_weight=np.full((B, T), 5.0), temperature=[kw["temperature"]] * B, top_k=[kw.get("top_k", 0)] * B, top_p=[kw.get("top_p", 1.0)] * B,
                      image_key=list(range(B)))
    _same(_run(e, pf, plan=full, **kw), ref, "all five arrays")
    _same(_run(e, pf, plan=SamplePlan(temperature=[kw["temperature"]] * B), **kw), ref, "one array, the rest from the scalars")
    # the plan's values win over the scalars it replaces
    other = dict(kw, cfg_weight=2.0, temperature=0.3 if kw["temperature"] > 0 else 1.0, top_k=3, top_p=0.4)
    _same(_run(e, pf, plan=full, **other), ref, "scalars overridden")


def test_every_image_equals_the_scalar_call_with_its_parameters(eng):
    e, pf = eng
    planned = _run(e, pf, plan=_full_plan(), cfg_weight=9.0, temperature=0.5, seed=SEED, return_logprobs=True, return_stats=2)
    assert len({tuple(planned["tokens"][b].tolist()) for b in range(B)}) == B
    for b, (w, t, k, p) in enumerate(IMG):
        ref = _run(e, pf, cfg_weight=w, temperature=t, top_k=k, top_p=p, seed=SEED, return_logprobs=True, return_stats=2)
        _same(planned, ref, f"image {b}", rows=b)
    # no active filter anywhere: the unfiltered planned route, greedy and sampled images side by side
    p2 = SamplePlan(cfg_weight=[i[0] for i in IMG], temperature=[i[1] for i in IMG])
    planned = _run(e, pf, plan=p2, cfg_weight=9.0, temperature=0.5, seed=SEED, return_logprobs=True)
    for b, (w, t, _, _) in enumerate(IMG):
        _same(planned, _run(e, pf, cfg_weight=w, temperature=t, seed=SEED, return_logprobs=True), f"unfiltered image {b}", rows=b)


def test_per_step_weights_on_a_forced_trajectory(eng, tiny_cfg):
    e, pf = eng
    g = torch.Generator().manual_seed(5)
    force = torch.randint(0, tiny_cfg.img_vocab, (B, T), generator=g, dtype=torch.int32)
    w = (1.0 + 0.5 * np.arange(B * T, dtype=np.float32)).reshape(B, T)               # a different weight at every (image, step)
    planned = _run(e, pf, plan=SamplePlan(cfg_weight=w), temperature=0.0, force_tokens=force)
    for val in np.unique(w):
        ref = _run(e, pf, cfg_weight=float(val), temperature=0.0, force_tokens=force)
        for b, t in np.argwhere(w == val):
            assert _eq(planned["logits"][t, b], ref["logits"][t, b]) and planned["tokens"][b, t] == ref["tokens"][b, t], (b, t, val)


def test_same_noise(eng):
    e, pf = eng
    ids, pad, _ = _prompt(e.cfg, 1, 77)
    pr = lambda: e.prefill(torch.cat([ids] * 2), list(pad) * 2)                      # two copies of one prompt
    kw = dict(cfg_weight=5.0, temperature=1.0, seed=SEED)
    a = _run(e, pr, plan=SamplePlan(image_key=[4, 4]), **kw)
    assert _eq(a["tokens"][0], a["tokens"][1]) and _eq(a["logits"][:, 0], a["logits"][:, 1])
    d = _run(e, pr, **kw)
    assert not _eq(d["tokens"][0], d["tokens"][1])                                   # default keys: different noise
    w = np.full((2, T), 5.0, dtype=np.float32)
    w[1, 3] = 0.0
    c = _run(e, pr, plan=SamplePlan(cfg_weight=w, image_key=[4, 4]), **kw)
    assert _eq(c["tokens"][0, :3], c["tokens"][1, :3]) and _eq(c["logits"][:3, 0], c["logits"][:3, 1]) and not _eq(c["logits"][3, 0], c["logits"][3, 1])
    _same(c, a, "image 0 is untouched by image 1's weight", rows=0)


def test_replicated_prefill_and_fp8_cache(tiny_cfg, tiny_weights):
    ids, pad, _ = _prompt(tiny_cfg, B, 131)
    plan = replicate(_full_plan(), 2, B)
    kw = dict(cfg_weight=9.0, temperature=0.5, seed=SEED, return_logprobs=True)
    er = get_engine(tiny_cfg, tiny_weights, "bf16", max_rows=12, max_prompt=192)
    a = _run(er, lambda: er.prefill_replicated(ids, pad, 2, alias=True), plan=plan, **kw)
    b = _run(er, lambda: er.prefill(torch.cat([ids] * 2), list(pad) * 2), plan=plan, **kw)
    _same(a, b, "aliased replicas vs a plain prefill of the replicated ids")
    assert not _eq(a["tokens"][1], a["tokens"][B + 1])                               # replicas of a sampled prompt differ (different default keys)
    e8 = get_engine(tiny_cfg, tiny_weights, "bf16", kv_dtype="fp8")
    pf8 = lambda: e8.prefill(ids, pad)
    planned = _run(e8, pf8, plan=_full_plan(), **kw)
    for i, (w, t, k, p) in enumerate(IMG):
        _same(planned, _run(e8, pf8, cfg_weight=w, temperature=t, top_k=k, top_p=p, seed=SEED, return_logprobs=True), f"fp8 image {i}", rows=i)


def test_graph_replays_with_a_new_plan_and_the_request_is_one_shot(eng):
    e, pf = eng
    kw = dict(cfg_weight=9.0, temperature=0.5, seed=SEED)
    p1 = _full_plan()
    p2 = SamplePlan(cfg_weight=[2.0, 4.0, 6.0], temperature=[0.7, 0.0, 1.1], top_k=[0, 0, 5], top_p=[1.0, 1.0, 0.9], image_key=[9, 8, 7])
    eager = [_run(e, pf, plan=p1, **kw), _run(e, pf, plan=p2, **kw), _run(e, pf, **kw)]
    e.set_option("use_graph", 1)
    try:
        got = [_run(e, pf, plan=p1, **kw), _run(e, pf, plan=p2, **kw), _run(e, pf, **kw)]
    finally:
        e.set_option("use_graph", 0)
    for i, what in enumerate(("captured", "replayed with another plan", "no request: unplanned")):
        _same(got[i], eager[i], what)
    assert not _eq(eager[0]["tokens"], eager[2]["tokens"]) and not _eq(eager[0]["tokens"], eager[1]["tokens"])


def test_refusals_leave_the_handle_usable(eng):
    e, pf = eng
    kw = dict(cfg_weight=5.0, temperature=0.8, seed=SEED)
    ref = _run(e, pf, **kw)

    def request(B_=B, T_=T, **arrs):
        keep = {k: np.ascontiguousarray(v) for k, v in arrs.items()}
        ptr = lambda k: C.c_void_p(keep[k].ctypes.data) if k in keep else None
        req = _lib.pg_sample_plan(ptr("w"), ptr("temperature"), ptr("top_k"), ptr("top_p"), ptr("key"), B_, T_)
        return e.lib.pg_request_sample_plan(e.h, C.byref(req), e.stream)

    f32, i32 = np.float32, np.int32
    ones = np.ones(B, dtype=f32)
    # refused at the request: nothing is pending afterwards, the next call is the unplanned one
    bad_w = np.ones((B, T), dtype=f32); bad_w[1, 2] = np.nan
    for rc, args in ((-1, dict(w=bad_w)), (-1, dict(temperature=np.array([1, np.inf, 1], dtype=f32))), (-1, dict(top_p=np.array([1, 0, 1], dtype=f32))),
                     (-1, dict(top_p=np.array([1, np.nan, 1], dtype=f32))), (-1, dict(top_k=np.array([0, -1, 0], dtype=i32))), (-1, dict(key=np.array([0, -1, 0], dtype=i32))),
                     (-1, dict()), (-1, dict(B_=0, temperature=ones)), (-1, dict(T_=0, temperature=ones)), (-5, dict(B_=5, temperature=np.ones(5, dtype=f32))),
                     (-5, dict(T_=e.cfg.img_tokens + 1, temperature=ones))):
        assert request(temperature=0.1 * ones) == 0                                  # a pending plan is dropped by a refused request
        assert request(**args) == rc, args
        _same(_run(e, pf, **kw), ref, f"after a refused request {sorted(args)}")
    # refused at the consuming call: wrong B / T, lanes = 2; nothing launched, the prefill is still good, the plan is consumed
    for args in (dict(B_=2, temperature=np.ones(2, dtype=f32)), dict(T_=T + 1, temperature=ones)):
        pf()
        assert request(**args) == 0
        with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
            e.decode_image_tokens(T=T, **kw)
        res = e.decode_image_tokens(T=T, return_logits=True, **kw)
        torch.cuda.synchronize()
        assert _eq(res[0].cpu(), ref["tokens"]) and _eq(res[1].cpu(), ref["logits"])
    e.set_option("lanes", 2)
    try:
        pf()
        assert request(temperature=0.1 * ones) == 0
        with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
            e.decode_image_tokens(T=T, **kw)
    finally:
        e.set_option("lanes", 1)
    _same(_run(e, pf, **kw), ref, "after the lanes = 2 refusal")
    # NULL forgets; the text loop neither consumes nor sees a plan
    assert request(temperature=0.1 * ones) == 0 and e.lib.pg_request_sample_plan(e.h, None, e.stream) == 0
    _same(_run(e, pf, **kw), ref, "after NULL")


def test_the_plan_buffer_is_counted_by_device_bytes(tiny_cfg):
    from plangen_amd.engine import Engine
    e = Engine(tiny_cfg, dtype="f32", max_rows=8, max_prompt=96, max_new=tiny_cfg.img_tokens, max_images=4)
    try:
        before = e.lib.pg_device_bytes(e.h)
        t = np.ones(2, dtype=np.float32)
        req = _lib.pg_sample_plan(None, C.c_void_p(t.ctypes.data), None, None, None, 2, 4)
        assert e.lib.pg_request_sample_plan(e.h, C.byref(req), e.stream) == 0
        first = e.lib.pg_device_bytes(e.h)
        assert e.lib.pg_request_sample_plan(e.h, C.byref(req), e.stream) == 0
        Bm = 4
        assert first - before >= (Bm * tiny_cfg.img_tokens + 4 * Bm) * 4 and e.lib.pg_device_bytes(e.h) == first      # allocated once
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------------- System.t2i and the CLI
def _args(cfg, **kw):
    from types import SimpleNamespace
    base = dict(seed=SEED, parallel_size=1, cfg_weight=5.0, temperature=1.0, top_k=0, top_p=1.0, use_teacher_forcing=False, debug_max_seq_len=None,
                janus_hw=cfg.img_size, neg_prompt="", use_neg_box=False)
    base.update(kw)
    return SimpleNamespace(**base)


def test_t2i_replicas_at_different_weights_with_the_same_noise(tiny_cfg, tiny_weights):
    """parallel_size = 2, cfg_weights = [1, 5], same_noise, share_replicas: replica t is the image a plain t2i at cfg_weights[t] draws for the same prompt
    with the same noise -- its replica 0 (RNG key = the prompt's index), run on the same replicated shape."""
    from plangen_amd.system import System, t2i_infer_collate_batch
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = torch.Generator().manual_seed(41)
    cond = [torch.randint(8, tiny_cfg.vocab, (n,), generator=g).tolist() for n in (9, 6)]
    neg = torch.randint(8, tiny_cfg.vocab, (4,), generator=g).tolist()
    ids, mask = t2i_infer_collate_batch(cond, neg, tiny_cfg.pad_id, tiny_cfg.img_tokens)
    B0 = 2

    def run(**kw):
        s = System(tiny_cfg, e, _args(tiny_cfg, parallel_size=2, share_replicas=1, **kw))
        dec, _ = s.t2i(ids, mask)
        torch.cuda.synchronize()
        return s, s.last_generated_tokens.cpu(), dec.cpu()

    sp, toks, dec = run(cfg_weights=[1.0, 5.0], same_noise=True)
    assert toks.shape[0] == 2 * B0 and sp.last_sample_plan["weight_start"] == [1.0, 5.0] and sp.last_sample_plan["same_noise"] is True
    for t, w in enumerate((1.0, 5.0)):
        s0, ptoks, pdec = run(cfg_weight=w)
        assert s0.last_sample_plan is None
        assert _eq(toks[t * B0:(t + 1) * B0], ptoks[:B0]) and _eq(dec[t * B0:(t + 1) * B0], pdec[:B0]), w
    assert not _eq(toks[:B0], toks[B0:])
    # without share_replicas: the same tokens
    s2 = System(tiny_cfg, e, _args(tiny_cfg, parallel_size=2, share_replicas=0, cfg_weights=[1.0, 5.0], same_noise=True))
    s2.t2i(ids, mask)
    assert _eq(s2.last_generated_tokens.cpu(), toks)
    # per-replica lists of the wrong length are refused before anything runs
    with pytest.raises(PlanGenError, match="parallel_size"):
        System(tiny_cfg, e, _args(tiny_cfg, parallel_size=2, temperatures=[1.0])).t2i(ids, mask)


def test_in_box_weight_changes_only_in_box_rows_and_score_images_refuses(tiny_cfg, tiny_weights, tmp_path):
    import dataclasses
    import tok_fixtures as TF
    from plangen_amd.system import System
    from plangen_amd.textproc import HFCodec, box_cells
    codec = HFCodec(TF.plain_hf_tokenizer_dir(tmp_path), special_tokens=True)
    cfg = dataclasses.replace(tiny_cfg, eos_id=codec.eos_token_id, pad_id=codec.pad_id)
    e = get_engine(tiny_cfg, tiny_weights, "bf16", max_rows=4, max_prompt=192)
    caps = ["a red cat on the table", "two dogs"]
    gts = ["<grounding><ref>a cat</ref><box>[0,0,500,250]</box><ref>the table</ref><box>[100,500,900,1000]</box></grounding>",
           "<grounding><ref>a red dog</ref><box>[70,70,100,100]</box></grounding>"]
    Tn, g = cfg.img_tokens, cfg.grid
    s = System(cfg, e, _args(cfg, cfg_weight_in_box=9.0), codec=codec)
    ids, m = s.pad_input_ids([s.wrap_uni_prompt(c, gr)[1].tolist() for c, gr in zip(caps, gts)])
    batch = dict(base_caption=caps, gt_grounding=gts, uni_inputs_ids=ids, uni_attention_mask=torch.cat([m, torch.ones((2, Tn), dtype=m.dtype)], -1))
    cfg_ids, cfg_mask = s._cfg_prompt(batch)
    L = cfg_ids.shape[1]
    cond_rows = [cfg_ids[2 * i][cfg_mask[2 * i, :L].bool()].tolist() for i in range(2)]
    plan, rec = s.build_sample_plan(cond_rows, 1, 5.0, Tn)
    cells = [(box_cells("[0,0,500,250]", g) | box_cells("[100,500,900,1000]", g)).reshape(-1), box_cells("[70,70,100,100]", g).reshape(-1)]
    assert cells[0].any() and not cells[1].any()                                     # the second prompt's box holds no cell centre
    assert rec["in_box_share"] == [float(c.mean()) for c in cells] and rec["weight_in_box"] == 9.0
    codes = torch.randint(0, cfg.img_vocab, (2, Tn), generator=torch.Generator().manual_seed(3)).int()
    _, lg_plan = s.sample_image(cfg_ids, cfg_mask, 5.0, 0.0, force_tokens=codes, return_logits=True, plan=plan)
    _, lg_ref = s.sample_image(cfg_ids, cfg_mask, 5.0, 0.0, force_tokens=codes, return_logits=True)
    torch.cuda.synchronize()
    lg_plan, lg_ref = lg_plan.cpu(), lg_ref.cpu()
    for b in range(2):
        inside = torch.from_numpy(cells[b])
        assert _eq(lg_plan[~inside, b], lg_ref[~inside, b])
        assert all(not _eq(lg_plan[t, b], lg_ref[t, b]) for t in torch.nonzero(inside).flatten().tolist())
    with pytest.raises(PlanGenError, match="decode_image_tokens"):
        s.score_images(dict(batch, image=torch.zeros(2, 3, cfg.img_size, cfg.img_size)))


def test_cli_writes_the_sample_plan_record(tmp_path):
    import glob
    import json
    import os
    import train
    from project.plangen.plangen_base import System
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='bf16'", "temperature=1.0", f"out_path={str(tmp_path)!r}",
            "test_data.task_type='uni'", "test_data.data_name='synthetic'", "max_prompt=256", "parallel_size=2", "share_replicas=1", "cfg_weights=[1.0,5.0]",
            "same_noise=True", "cfg_schedule='linear'", "cfg_weight_end=2.0"]
    a = train.parse_args(["--cfg", os.path.join(root, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
    m = System(a, None)
    m.setup_data(None)
    m.resume(None)
    m.validation(0)
    m.engine.close()
    files = glob.glob(os.path.join(str(tmp_path), "test", "*", "0_batch", "0_layout.json"))
    assert len(files) == 1, files
    rec = json.load(open(files[0]))["sample_plan"]
    assert rec["schedule"] == "linear" and rec["weight_start"] == [1.0, 5.0] and rec["weight_end"] == [2.0, 2.0] and rec["same_noise"] is True
    assert len(rec["in_box_share"]) == 4 and rec["weight_in_box"] is None
