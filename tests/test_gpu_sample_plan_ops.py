"""GPU: one step of the image sampler under a sample plan (pg_diag_op_cfg_sample_plan -> launch_cfg_step with a plan: the planned instantiations of cfg_scan_kernel
and cfg_select_kernel, then cfg_pick_kernel) against the host model of tests/plan_ref.py.  The tapped row is compared with == on dyadic slabs; a sampled draw binds
where the model's fp64 lead exceeds the device's arithmetic (draw_ref.decided with the E_g that tests/test_gpu_draws.py measures), at most
draw_ref.UNDECIDED_CAP of a parametrisation's draws may be open; greedy images bind always."""
import numpy as np
import pytest
import torch

import draw_ops as O
import draw_ref as D
import plan_ref as P
from plangen_amd.engine import Engine
from test_gpu_draws import Tally, _e_g

pytestmark = pytest.mark.gpu
T = P.PLAN_T


@pytest.fixture(scope="module")
def E_g(tiny_cfg, tiny_weights):
    return _e_g(tiny_cfg, tiny_weights)[0]


def plan_dev(plan):
    return dict(w=torch.from_numpy(np.ascontiguousarray(plan["w"], dtype=np.float32)).cuda(), temperature=torch.from_numpy(plan["temperature"].astype(np.float32)).cuda(),
                top_k=torch.from_numpy(plan["top_k"].astype(np.int32)).cuda(), top_p=torch.from_numpy(plan["top_p"].astype(np.float32)).cuda(),
                key=torch.from_numpy(plan["key"].astype(np.int32)).cuda())


def run(flat, S, slab, V, B, pd, seed, step, b_off, B_total, filtered, stored=False, tap=True, drop=None, T_=T):
    """One planned step on guarded outputs.  Returns rc, tok [B_total, T], tap [B, V] or None, ok (canaries and every other tap row intact)."""
    out = O.Guarded(B_total, T_, torch.int32, O.UNSET)
    x = O.Guarded(2 * B, O.H, torch.float32, float("nan"))
    lg = O.Guarded(O.TAP_STEPS * B_total, V, torch.float32, O.CANARY) if tap else None
    a = dict(pd)
    if drop:
        a[drop] = None
    rc = Engine.cfg_sample_plan_op(flat, S, slab, None, V, B, out.ptr, lg.ptr if tap else None, O.table(min(V, 16384)), x.ptr, O.H, a["w"], a["temperature"], a["top_k"],
                                   a["top_p"], a["key"], seed, T_, step, b_off, B_total, filtered=filtered, stored=stored)
    torch.cuda.synchronize()
    ok = out.guards_intact() and x.guards_intact()
    rows = None
    if rc != O.PG_OK:
        ok = ok and bool((out.valid() == O.UNSET).all()) and bool(torch.isnan(x.valid()).all()) and (lg is None or bool((lg.t == O.CANARY).all()))
    elif tap:
        v = lg.valid().view(O.TAP_STEPS, B_total, V)
        rows = v[step, b_off:b_off + B].cpu()
        other = torch.ones(O.TAP_STEPS, B_total, dtype=torch.bool, device="cuda")
        other[step, b_off:b_off + B] = False
        ok = ok and lg.guards_intact() and bool((v[other] == O.CANARY).all())
    return dict(rc=rc, tok=out.valid().cpu(), x=x.valid().cpu(), tap=rows, ok=ok)


@pytest.mark.parametrize("S", P.PLAN_S)
@pytest.mark.parametrize("V", P.PLAN_V)
def test_planned_operator_draws_the_models_token(V, S, E_g):
    """Every image's token is the model's, with the plan indexed by the global image (b_off > 0, B_total > b_off + B) at steps 0..3 and 574, 575 of T = 576."""
    tally = Tally(f"plan V={V} S={S}")
    B = P.PLAN_B
    for c in P.plan_cases(V, S):
        b_off, B_total, plan = c["b_off"], c["B_total"], c["plan"]
        flat, slab = O.slabs_dev(c["slabs"], 2 * B * V + 3 * V)
        pd = plan_dev(plan)
        cond, unc = P.cond_uncond(c)
        flt = P.filtered(plan)
        for step in c["steps"]:
            tap = step < O.TAP_STEPS
            r = run(flat, S, slab, V, B, pd, c["seed"], step, b_off, B_total, flt, tap=tap)
            assert r["rc"] == O.PG_OK and r["ok"], (r["rc"], step)
            mixed, tok, gap, scale, ru, smp = P.step_model(cond, unc, plan, b_off, step, c["seed"])
            if tap:
                assert torch.equal(r["tap"].double(), torch.from_numpy(mixed)), (step, b_off)
            got = r["tok"][b_off:b_off + B, step].numpy()
            want = torch.full_like(r["tok"], O.UNSET)
            want[b_off:b_off + B, step] = torch.from_numpy(got)
            assert torch.equal(r["tok"], want)                              # nothing else written
            for b in range(B):
                bg = b_off + b
                assert torch.equal(r["x"][2 * b], O.table_row(D.clamp(int(got[b]), V))) and torch.equal(r["x"][2 * b + 1], r["x"][2 * b])
                if not smp[b]:
                    assert got[b] == tok[b], ("greedy", step, bg, got[b], tok[b])
                    continue
                k, p = int(plan["top_k"][bg]), float(plan["top_p"][bg])
                keep = P.keep_set(mixed[b], float(plan["temperature"][bg]), k, p)
                tally.check(got[b:b + 1], mixed[b:b + 1], float(plan["temperature"][bg]), c["seed"], P.stream_key(int(plan["key"][bg]), step), E_g,
                            keep=None if keep is None else keep[None], none_token=-1 if keep is None else 0, ctx=(step, bg))
    tally.close()


def test_mixed_batch_equals_the_unplanned_operators():
    """Image 0 greedy, image 1 sampled unfiltered, image 2 sampled with (50, 0.9), one call at V = 16384: image 0 is the first-index argmax, images 1 and 2 are
    bit-equal to the unplanned unfiltered / filtered operator (default keys: the image index), and the tapped rows are the unplanned rows."""
    V, B, S, w, temp, seed = 16384, 3, 2, 5.0, 1.0, D.IMG_SEED + 99
    rng = np.random.default_rng(11)
    slabs = D.dyadic_slabs(rng, S, 2 * B, V, 1.5)
    flat, slab = O.slabs_dev(slabs)
    plan = dict(w=np.full((B, T), w, dtype=np.float32), temperature=np.array([0.0, temp, temp], dtype=np.float32), top_k=np.array([7, 0, 50], dtype=np.int32),
                top_p=np.array([0.5, 1.0, 0.9], dtype=np.float32), key=np.arange(B, dtype=np.int32))
    pd = plan_dev(plan)
    mixed = D.image_mixed(dict(slabs=slabs, bias=None, w=w))
    for step in (0, 3, 575):
        r = run(flat, S, slab, V, B, pd, seed, step, 0, B, True, tap=step < O.TAP_STEPS)
        assert r["rc"] == O.PG_OK and r["ok"]
        g = O.cfg_sample(flat, S, slab, None, V, B, w, 0.0, seed, step)
        u = O.cfg_sample(flat, S, slab, None, V, B, w, temp, seed, step)
        f = O.cfg_sample(flat, S, slab, None, V, B, w, temp, seed, step, filtered=1, top_k=50, top_p=0.9)
        got = r["tok"][:, step].tolist()
        assert got[0] == int(D.greedy(mixed)[0]) == int(g["tok"][0, step])      # its (7, 0.5) is ignored
        assert got[1] == int(u["tok"][1, step]) and got[2] == int(f["tok"][2, step]), (step, got)
        if r["tap"] is not None:
            assert torch.equal(r["tap"], u["tap"]) and torch.equal(r["tap"].double(), torch.from_numpy(mixed))
        assert torch.equal(r["x"][2:4], u["x"][2:4]) and torch.equal(r["x"][4:6], f["x"][4:6]) and torch.equal(r["x"][0:2], g["x"][0:2])
        # the same batch on the unfiltered planned route (no active filter anywhere): image 1 keeps its token, the store scan changes nothing
        p2 = dict(plan, top_k=np.zeros(B, dtype=np.int32), top_p=np.ones(B, dtype=np.float32))
        for stored in (False, True):
            r2 = run(flat, S, slab, V, B, plan_dev(p2), seed, step, 0, B, False, stored=stored, tap=step < O.TAP_STEPS)
            assert r2["rc"] == O.PG_OK and r2["ok"] and r2["tok"][:2, step].tolist() == got[:2] and int(r2["tok"][2, step]) == int(u["tok"][2, step])


def test_equal_keys_draw_equal_noise_and_distinct_keys_do_not(E_g):
    """The SAME row and parameters for every image: images that share a key emit the same token at every step drawn (both ends of T = 576 and a stride through it), on both routes; with distinct keys the tokens are
    the model's and the model's differ across images and steps (the decorrelation check of the unplanned operator)."""
    V, B, S = 1000, 3, 2
    rng = np.random.default_rng(7)
    slabs = np.tile(D.dyadic_slabs(rng, S, 2, V, 1.5), (1, B, 1))
    flat, slab = O.slabs_dev(slabs)
    mixed = D.image_mixed(dict(slabs=slabs, bias=None, w=1.0))
    tally = Tally("plan keys")
    seen = {}
    for flt in (False, True):
        base = dict(w=np.ones((B, T), dtype=np.float32), temperature=np.ones(B, dtype=np.float32), top_k=np.full(B, 200 if flt else 0, dtype=np.int32),
                    top_p=np.ones(B, dtype=np.float32))
        keep = np.stack([P.keep_set(mixed[b], 1.0, 200, 1.0) for b in range(B)]) if flt else None
        for keys in ((41, 41, 41), (41, 977, 5)):
            pd = plan_dev(dict(base, key=np.array(keys, dtype=np.int32)))
            for step in sorted(set(D.IMG_STEPS) | set(D.IMG_CASE_STEPS)) + list(range(4, 574, 57)):
                r = run(flat, S, slab, V, B, pd, D.IMG_SEED, step, 0, B, flt, tap=False)
                assert r["rc"] == O.PG_OK and r["ok"]
                got = r["tok"][:, step].numpy()
                want = tally.check(got, mixed, 1.0, D.IMG_SEED, P.stream_key(np.array(keys), step), E_g, keep=keep, ctx=(flt, keys, step))
                if len(set(keys)) == 1:
                    assert len(set(got.tolist())) == 1, (keys, step, got)
                elif not flt:
                    for b in range(B):
                        seen[(keys[b], step)] = int(want[b])
    tally.close()
    assert tally.open == 0
    assert len({v for (k, s), v in seen.items() if s == 0}) > 1                                      # across images
    for k in (41, 977, 5):
        assert len({seen[(k, s)] for s in D.IMG_STEPS}) > 1, k                                       # across steps of one image


def test_argument_errors_launch_nothing():
    V, B, S = 17, 3, 1
    rng = np.random.default_rng(3)
    flat, slab = O.slabs_dev(D.dyadic_slabs(rng, S, 2 * B, V, 1.5))
    pd = plan_dev(dict(w=np.ones((B, T), dtype=np.float32), temperature=np.ones(B, dtype=np.float32), top_k=np.zeros(B, dtype=np.int32),
                       top_p=np.ones(B, dtype=np.float32), key=np.arange(B, dtype=np.int32)))
    for drop in ("w", "temperature", "top_k", "top_p", "key"):
        r = run(flat, S, slab, V, B, pd, 1, 0, 0, B, False, drop=drop)
        assert r["rc"] == O.PG_ERR_ARG and r["ok"], drop
    r = run(flat, S, slab, V, B, pd, 1, 0, 2, B, False)                    # b_off + B > B_total
    assert r["rc"] == O.PG_ERR_ARG and r["ok"]
    r = run(flat, S, slab, V, B, pd, 1, 3, 0, B, False, T_=3)              # a tap at step >= T
    assert r["rc"] == O.PG_ERR_ARG and r["ok"]
    r = run(flat, S, 2 * B * V - 1, V, B, pd, 1, 0, 0, B, False)           # slabs that overlap
    assert r["rc"] == O.PG_ERR_ARG and r["ok"]
    r = run(flat, S, slab, V, B, pd, 1, 0, 0, B, False)
    assert r["rc"] == O.PG_OK and r["ok"]
