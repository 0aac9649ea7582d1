"""GPU: one step of the image sampler under dual guidance (pg_diag_op_cfg3_sample -> launch_cfg_step at three rows per image: cfg_scan_kernel<3>, the
cfg_select_kernel of the pair route, cfg_pick_kernel<3>) against the host model of tests/dual_ref.py.  The tapped row is compared with == on dyadic slabs and weights; greedy tokens bind always; a
sampled draw binds where the model's fp64 lead exceeds the device's arithmetic (draw_ref.decided with the E_g that tests/test_gpu_draws.py measures), at most
draw_ref.UNDECIDED_CAP of a parametrisation's draws may be open.  The degenerate cases are compared bit for bit with the pair operator on the same slabs."""
import numpy as np
import pytest
import torch

import draw_ops as O
import draw_ref as D
import dual_ref as U
from plangen_amd.engine import Engine
from test_gpu_draws import Tally, _e_g

pytestmark = pytest.mark.gpu
T = U.DUAL_T


@pytest.fixture(scope="module")
def E_g(tiny_cfg, tiny_weights):
    return _e_g(tiny_cfg, tiny_weights)[0]


def run(flat, S, slab, bias, V, B, wc, wl, temperature, seed, step, b_off=0, img_off=0, B_total=None, top_k=0, top_p=1.0, filtered=False, stored=False,
        tap=None, force=None, mask=None, T_=T, want_mix=False):
    """One dual step on guarded outputs.  Returns rc, tok [B_total, T], x [3B, H], tap [B, V] or None, mix [B, V] or None, ok (canaries and every other tap row
    intact; on a refusal every output untouched)."""
    B_total = b_off + B if B_total is None else B_total
    tap = (step < O.TAP_STEPS) if tap is None else tap
    out = O.Guarded(B_total, T_, torch.int32, O.UNSET)
    x = O.Guarded(3 * B, O.H, torch.float32, float("nan"))
    lg = O.Guarded(O.TAP_STEPS * B_total, V, torch.float32, O.CANARY) if tap else None
    mx = O.Guarded(B, V, torch.float32, O.CANARY) if want_mix else None
    ft = torch.as_tensor(force, dtype=torch.int32).cuda().contiguous() if force is not None else None
    fm = torch.as_tensor(mask, dtype=torch.uint8).cuda().contiguous() if mask is not None else None
    rc = Engine.cfg3_sample_op(flat, S, slab, bias, V, B, out.ptr, lg.ptr if tap else None, O.table(V), x.ptr, O.H, wc, wl, temperature, seed, T_, step,
                               top_k=top_k, top_p=top_p, img_off=img_off, b_off=b_off, B_total=B_total, force_tok=ft, force_mask=fm, filtered=filtered,
                               stored=stored, mix_out=mx.ptr if want_mix else None)
    torch.cuda.synchronize()
    ok = out.guards_intact() and x.guards_intact() and (mx is None or mx.guards_intact())
    rows = None
    if rc != O.PG_OK:
        ok = ok and bool((out.valid() == O.UNSET).all()) and bool(torch.isnan(x.valid()).all()) and (lg is None or bool((lg.t == O.CANARY).all()))
        ok = ok and (mx is None or bool((mx.t == O.CANARY).all()))
    elif tap:
        v = lg.valid().view(O.TAP_STEPS, B_total, V)
        rows = v[step, b_off:b_off + B].cpu()
        other = torch.ones(O.TAP_STEPS, B_total, dtype=torch.bool, device="cuda")
        other[step, b_off:b_off + B] = False
        ok = ok and lg.guards_intact() and bool((v[other] == O.CANARY).all())
    return dict(rc=rc, tok=out.valid().cpu(), x=x.valid().cpu(), tap=rows, mix=mx.valid().cpu() if want_mix else None, ok=ok)


def check_outputs(r, B, b_off, step, emits, feeds):
    """out_tok holds emits at [b_off + b][step] and nothing else; rows 3b .. 3b + 2 of x hold table[feed]."""
    want = torch.full_like(r["tok"], O.UNSET)
    for b in range(B):
        if emits[b] is not None:
            want[b_off + b, step] = emits[b]
        for j in range(3):
            assert torch.equal(r["x"][3 * b + j], O.table_row(feeds[b])), (b, j, feeds[b], r["x"][3 * b:3 * b + 3])
    assert torch.equal(r["tok"], want), (r["tok"][:, step].tolist(), emits)


def _family(V, S, with_bias, E_g, tag):
    tally = Tally(tag)
    B = U.DUAL_B
    for c in U.dual_cases(V, S, with_bias):
        flat, slab = O.slabs_dev(c["slabs"], 3 * B * V + 3 * V)                 # a slab stride beyond the rows: NaN between the slabs
        bias = torch.from_numpy(c["bias"]).cuda() if c["bias"] is not None else None
        flt = c["T"] > 0 and (c["top_k"] > 0 or c["top_p"] < 1.0)
        for step in c["steps"]:
            tap = step < O.TAP_STEPS
            r = run(flat, S, slab, bias, V, B, c["w_caption"], c["w_layout"], c["T"], c["seed"], step, c["b_off"], c["img_off"], c["B_total"], c["top_k"],
                    c["top_p"], filtered=flt, tap=tap, want_mix=flt)
            assert r["rc"] == O.PG_OK and r["ok"], (r["rc"], step)
            mixed, tok, gap, scale, ru, keep = U.case_model(c, step)
            if tap:
                assert torch.equal(r["tap"].double(), torch.from_numpy(mixed)), (step, c["w_caption"], c["w_layout"])
            if flt:
                assert torch.equal(r["mix"].double(), torch.from_numpy(mixed))
            got = r["tok"][c["b_off"]:c["b_off"] + B, step].numpy()
            check_outputs(r, B, c["b_off"], step, got.tolist(), [D.clamp(int(t), V) for t in got])
            if c["T"] <= 0:
                assert (got == tok).all(), ("greedy", step, got, tok)
                continue
            if keep is not None:
                assert keep[np.arange(B), got].all(), ("a token outside the keep set", step, got)
            tally.check(got, mixed, c["T"], c["seed"], D.image_key(np.arange(B), c["b_off"], c["img_off"], step), E_g, keep=keep,
                        none_token=-1 if keep is None else 0, ctx=(step, c["b_off"]))
    tally.close()


@pytest.mark.parametrize("S", U.DUAL_S)
@pytest.mark.parametrize("V", U.DUAL_V)
def test_dual_operator_draws_the_models_token(V, S, E_g):
    """Every weight pair, greedy and sampled, b_off > 0 and B_total > b_off + B, steps 0..3 and 574, 575 of T = 576; V = 17 and 1000 end in a ragged chunk."""
    _family(V, S, False, E_g, f"dual V={V} S={S}")


@pytest.mark.parametrize("V,S", [(17, 2), (1000, 5)])
def test_dual_operator_with_bias(V, S, E_g):
    _family(V, S, True, E_g, f"dual bias V={V} S={S}")


@pytest.mark.parametrize("V,S", [(1000, 2), (16384, 5), (17, 1)])
def test_degenerate_cases_equal_the_pair_operator_bit_for_bit(V, S):
    """p == f gives the pair result at w_caption, p == u the pair result at w_layout: tap, token and x, greedy and sampled, on slabs that are NOT dyadic (the
    fp32 roundings of the slab sum and of the mix must be the pair scan's)."""
    B, wc, wl, seed = 3, 5.0, 1.75, D.IMG_SEED + 7
    rng = np.random.default_rng(900 + V + S)
    fu = (rng.standard_normal((S, 2 * B, V)) * (2.4 / np.sqrt(S))).astype(np.float32)
    bias = torch.from_numpy((rng.standard_normal(V) * 0.5).astype(np.float32)).cuda()
    pair_flat, pair_slab = O.slabs_dev(fu)
    for which, w_pair in (("p==f", wc), ("p==u", wl)):
        tri = np.empty((S, 3 * B, V), dtype=np.float32)
        tri[:, 0::3] = fu[:, 0::2]; tri[:, 2::3] = fu[:, 1::2]
        tri[:, 1::3] = fu[:, 0::2] if which == "p==f" else fu[:, 1::2]
        flat, slab = O.slabs_dev(tri)
        for temperature in (0.0, 1.0):
            for step in (0, 3):
                for bs in (None, bias):
                    r = run(flat, S, slab, bs, V, B, wc, wl, temperature, seed, step, b_off=1, img_off=3, B_total=5)
                    q = O.cfg_sample(pair_flat, S, pair_slab, bs, V, B, w_pair, temperature, seed, step, img_off=3, b_off=1, B_total=5)
                    assert r["rc"] == O.PG_OK and r["ok"] and q["rc"] == O.PG_OK and q["ok"]
                    assert torch.equal(r["tap"], q["tap"]), (which, temperature, step, (r["tap"] - q["tap"]).abs().max())
                    assert torch.equal(r["tok"], q["tok"]), (which, temperature, step)
                    assert torch.equal(r["x"][0::3], q["x"][0::2]) and torch.equal(r["x"][2::3], q["x"][1::2])


def test_forcing_with_and_without_mask():
    V, B, S, step = 1000, 3, 2, 2
    rng = np.random.default_rng(21)
    slabs = D.dyadic_slabs(rng, S, 3 * B, V, 1.5)
    flat, slab = O.slabs_dev(slabs)
    b_off, B_total = 1, 5
    force = rng.integers(0, V, size=(B_total, T)).astype(np.int32)
    force[b_off, step] = V + 5                                   # out of range: emitted as given under a mask, clamped for the embedding row
    mask = np.ones((B_total, T), dtype=np.uint8)
    mask[b_off, step] = 0; mask[b_off + 2, step] = 0
    mixed, tok, *_ = U.step_model(slabs, None, 5.0, 1.0, 0.0, 0, 1.0, b_off, 0, step, 1)
    r = run(flat, S, slab, None, V, B, 5.0, 1.0, 0.0, 1, step, b_off, 0, B_total, force=force)
    assert r["rc"] == O.PG_OK and r["ok"]
    picks = [D.cfg_pick(int(tok[b]), V, T, step, force[b_off + b]) for b in range(B)]
    check_outputs(r, B, b_off, step, [p[0] for p in picks], [p[1] for p in picks])
    assert [p[0] for p in picks] == tok.tolist()                 # without a mask the emitted token stays the model's
    r = run(flat, S, slab, None, V, B, 5.0, 1.0, 0.0, 1, step, b_off, 0, B_total, force=force, mask=mask)
    assert r["rc"] == O.PG_OK and r["ok"]
    picks = [D.cfg_pick(int(tok[b]), V, T, step, force[b_off + b], mask[b_off + b]) for b in range(B)]
    check_outputs(r, B, b_off, step, [p[0] for p in picks], [p[1] for p in picks])
    assert picks[0][0] == V + 5 and picks[0][1] == V - 1 and picks[1][0] == int(tok[1])
    # a step past T: nothing is emitted, the model's token is fed back
    r = run(flat, S, slab, None, V, B, 5.0, 1.0, 0.0, 1, 3, b_off, 0, B_total, force=force[:, :3].copy(), T_=3, tap=False)
    assert r["rc"] == O.PG_OK and r["ok"]
    tok3 = U.step_model(slabs, None, 5.0, 1.0, 0.0, 0, 1.0, b_off, 0, 3, 1)[1]
    check_outputs(r, B, b_off, 3, [None] * B, tok3.tolist())


def test_stored_form_leaves_the_tapped_row_and_changes_nothing_else(E_g):
    V, B, S, seed = 16384, 3, 2, D.IMG_SEED + 3
    rng = np.random.default_rng(22)
    flat, slab = O.slabs_dev(D.dyadic_slabs(rng, S, 3 * B, V, 1.5))
    for temperature in (0.0, 1.0):
        a = run(flat, S, slab, None, V, B, 2.5, 7.0, temperature, seed, 1)
        b = run(flat, S, slab, None, V, B, 2.5, 7.0, temperature, seed, 1, stored=True, want_mix=True)
        assert a["rc"] == O.PG_OK and a["ok"] and b["rc"] == O.PG_OK and b["ok"]
        assert torch.equal(b["mix"], b["tap"]) and torch.equal(a["tap"], b["tap"]) and torch.equal(a["tok"], b["tok"]) and torch.equal(a["x"], b["x"])
    # the filtered form with a filter that keeps everything draws the unfiltered token
    f = run(flat, S, slab, None, V, B, 2.5, 7.0, 1.0, seed, 1, top_k=V, top_p=1.0, filtered=True, want_mix=True)
    assert f["rc"] == O.PG_OK and f["ok"] and torch.equal(f["tok"], a["tok"]) and torch.equal(f["mix"], a["tap"])


def test_argument_errors_launch_nothing():
    V, B, S = 17, 3, 1
    rng = np.random.default_rng(3)
    flat, slab = O.slabs_dev(D.dyadic_slabs(rng, S, 3 * B, V, 1.5))
    bad = (dict(b_off=2, B_total=B),                              # b_off + B > B_total
           dict(step=3, T_=3, tap=True),                          # a tap at step >= T
           dict(slab=3 * B * V - 1),                              # slabs that overlap
           dict(wc=float("nan")), dict(wl=float("nan")),
           dict(filtered=True, temperature=0.0), dict(filtered=True, temperature=1.0, top_p=0.0), dict(filtered=True, temperature=1.0, top_k=-1),
           dict(want_mix=True))                                   # mix_out without a store scan
    for kw in bad:
        a = dict(slab=slab, wc=5.0, wl=1.0, temperature=0.0, step=0)
        a.update(kw)
        r = run(flat, S, a.pop("slab"), None, V, B, a.pop("wc"), a.pop("wl"), a.pop("temperature"), 1, a.pop("step"), **a)
        assert r["rc"] == O.PG_ERR_ARG and r["ok"], kw
    r = run(flat, S, slab, None, V, B, 5.0, 1.0, 0.0, 1, 0)
    assert r["rc"] == O.PG_OK and r["ok"]
