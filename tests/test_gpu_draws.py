"""GPU: the draw of both samplers -- the kernels that turn a row of logits into the emitted token -- against the host model of tests/draw_ref.py: the RNG
in integer-exact arithmetic, the stream keys, the fp64 Gumbel term and the first-index argmax.  A draw binds the device only where the model's fp64 lead over
the runner-up exceeds what the device's fp32 arithmetic and fast logarithms can move (draw_ref.decided, with E_g MEASURED here over all 2^23 values of u); at
most 1 % of a parametrisation's draws may be open, and an open draw must still be one of the model's top two.  The operators run the production launchers on
crafted slabs (pg_diag_op_cfg_sample / pg_diag_op_text_draw, tests/draw_ops.py) whose fp32 sums are exact, so the tapped row is compared with ==."""
import numpy as np
import pytest
import torch

import draw_ops as O
import draw_ref as D
from conftest import get_engine, load_golden

pytestmark = pytest.mark.gpu

# Measured on gfx950 (deterministic): max |device Gumbel term - fp64| over all 2^23 u.  The test asserts the next power of two above it.
E_G_BOUND = 2.0 ** -19         # measured 1.875019e-06 = 2^-19.025, at u = 0.999987781

_S = {}


def _e_g(tiny_cfg, tiny_weights):
    """(E_g, gumbel fp32 [2^23] on the CPU, fp64 reference, u): one sweep for the module."""
    if "eg" not in _S:
        e = get_engine(tiny_cfg, tiny_weights, "f32")
        bits = torch.arange(1 << 23, dtype=torch.int64) << 41
        u, g = e.op_uniform(bits)
        u, g = u.cpu().double().numpy(), g.cpu().double().numpy()
        ref = D.gumbel(D.uniform(bits.numpy().astype(np.uint64)))
        with np.errstate(invalid="ignore"):
            err = np.abs(g - ref)
        _S["eg"] = (float(np.nanmax(err)) if np.isfinite(g).all() else float("inf"), g, ref, u, err)
    return _S["eg"]


@pytest.fixture(scope="module")
def E_g(tiny_cfg, tiny_weights):
    return _e_g(tiny_cfg, tiny_weights)[0]


class Tally:
    """Decided / open draws of one parametrisation."""

    def __init__(self, tag):
        self.tag, self.n, self.open = tag, 0, 0

    def check(self, got, rows, temperature, seed, keys, E_g, keep=None, none_token=0, ctx=()):
        """got [n] device tokens against the model's draw on rows [n, V]."""
        got = np.asarray(got, dtype=np.int64)
        tok, gap, scale, ru = D.draw_top2(rows, temperature, seed, keys, keep)
        V = np.atleast_2d(rows).shape[1]
        want = np.where(tok == D.NONE, none_token if none_token >= 0 else V + none_token, tok)
        dec = D.decided(gap, scale, E_g)
        bad = dec & (got != want)
        assert not bad.any(), (self.tag, ctx, "decided draws differ", np.nonzero(bad)[0][:8].tolist(), got[bad][:8].tolist(), want[bad][:8].tolist())
        top2 = (got == want) | (got == ru)
        assert top2[~dec].all(), (self.tag, ctx, "an open draw outside the model's top two")
        self.n += dec.size
        self.open += int((~dec).sum())
        return want

    def close(self):
        print(f"{self.tag}: {self.open} of {self.n} draws open")
        assert self.open <= D.UNDECIDED_CAP * self.n, (self.tag, self.open, self.n)


def _same(a, b):
    """Bitwise-as-values equality of two float tensors, NaN == NaN."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _check_image_outputs(r, c_B, b_off, step, T, emits, feeds):
    """out_tok holds emits at [b_off + b][step] and nothing else; both CFG rows of x hold table[feed]; canaries intact."""
    assert r["rc"] == O.PG_OK and r["ok"]
    want = torch.full_like(r["tok"], O.UNSET)
    for b in range(c_B):
        if emits[b] is not None:
            want[b_off + b, step] = emits[b]
        assert torch.equal(r["x"][2 * b], O.table_row(feeds[b])) and torch.equal(r["x"][2 * b + 1], O.table_row(feeds[b])), (b, feeds[b], r["x"][2 * b:2 * b + 2])
    assert torch.equal(r["tok"], want), (r["tok"][:, step].tolist(), emits)


# ------------------------------------------------------------------------------------------------------------------------------------------------------- (a)
def test_gumbel_term_over_all_u(tiny_cfg, tiny_weights):
    """-__logf(-__logf(u)) for every one of the 2^23 values of u: finite, non-decreasing in u (a non-monotone transform reorders draws), and its maximum
    absolute error against fp64 -- E_g, the figure every decided / open decision below uses.  Measured on gfx950: see E_G_BOUND."""
    E, g, ref, u, err = _e_g(tiny_cfg, tiny_weights)
    assert (u == D.uniform(np.arange(1 << 23, dtype=np.uint64) << np.uint64(41))).all()
    assert np.isfinite(g).all()
    print(f"E_g = {E:.6e} = 2^{np.log2(E):.3f} at u = {u[np.argmax(err)]!r}; mean |error| {err.mean():.3e}")
    for name, sl in (("smallest", slice(0, 16)), ("largest", slice(-16, None))):
        print(f"  16 {name} u: errors " + " ".join(f"{x:.2e}" for x in err[sl]))
    edges = [0, 1 << 8, 1 << 12, 1 << 16, 1 << 20, 1 << 22, (1 << 23) - (1 << 20), (1 << 23) - (1 << 16), (1 << 23) - (1 << 12), (1 << 23) - (1 << 8), 1 << 23]
    print("  max error by range of u: " + "; ".join(f"[{u[a]:.3g}, {u[b - 1]:.9g}] {err[a:b].max():.2e}" for a, b in zip(edges[:-1], edges[1:])))
    d = np.diff(g)
    assert (d >= 0).all(), ("the Gumbel term decreases somewhere", int((d < 0).sum()), np.nonzero(d < 0)[0][:8].tolist())
    assert E <= E_G_BOUND, E


# ------------------------------------------------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("S", D.IMG_S)
@pytest.mark.parametrize("V", D.IMG_V)
def test_image_operator_draws_the_models_token(V, S, with_bias, E_g):
    """cfg_scan_kernel + cfg_pick_kernel on crafted slabs: every (cfg_weight, temperature, B) at six steps, offsets rotating, a seed >= 2^63; S > 4 takes the
    sum_slabs tail, V = 1 / 17 / 1000 leave chunks short or empty, the slab stride exceeds the rows (NaN between the slabs)."""
    tally = Tally(f"image V={V} S={S} bias={with_bias}")
    T = 576
    for c in D.image_cases(V, S, with_bias):
        B, b_off, img_off = c["B"], c["b_off"], c["img_off"]
        flat, slab = O.slabs_dev(c["slabs"], 2 * B * V + 3 * V)
        bias = torch.from_numpy(c["bias"]).cuda() if with_bias else None
        mixed = D.image_mixed(c)
        for step in c["steps"]:
            r = O.cfg_sample(flat, S, slab, bias, V, B, c["w"], c["T"], c["seed"], step, T, img_off, b_off, c["B_total"])
            if r["tap"] is not None:
                assert torch.equal(r["tap"].double(), torch.from_numpy(mixed)), (c["w"], c["T"], B, step)
            got = r["tok"][b_off:b_off + B, step].numpy()
            ctx = (c["w"], c["T"], B, step, b_off, img_off)
            if c["T"] > 0:
                want = tally.check(got, mixed, c["T"], c["seed"], D.image_key(np.arange(B), b_off, img_off, step), E_g, ctx=ctx)
                feeds = [D.clamp(int(t), V) for t in got]
                _check_image_outputs(r, B, b_off, step, T, [int(t) for t in got], feeds)
            else:
                want = D.greedy(mixed)
                assert (got == want).all(), (ctx, got, want)
                _check_image_outputs(r, B, b_off, step, T, want.tolist(), want.tolist())
    tally.close()


def test_image_draws_are_decorrelated_across_images_and_steps(E_g):
    """The SAME row for every image, at steps 0, 1 and 575, with nonzero offsets: the tokens are the model's, and the model's are not all equal -- a key
    that dropped step, the image index, b_off or img_off would repeat draws."""
    V, B, S, T = 1000, 3, 2, 576
    rng = np.random.default_rng(7)
    one = D.dyadic_slabs(rng, S, 2, V, 1.5)
    slabs = np.tile(one, (1, B, 1))
    flat, slab = O.slabs_dev(slabs)
    mixed = D.image_mixed(dict(slabs=slabs, bias=None, w=1.0))       # cfg_weight 1: a flat softmax (std 1.5), so that equal rows can draw different tokens
    assert (mixed == mixed[0]).all()
    tally = Tally("image decorrelation")
    seen = {}
    for b_off, img_off in ((0, 0), (2, 5), (2, 9), (3, 5)):
        for step in D.IMG_STEPS:
            r = O.cfg_sample(flat, S, slab, None, V, B, 1.0, 1.0, D.IMG_SEED, step, T, img_off, b_off, b_off + B)
            got = r["tok"][b_off:b_off + B, step].numpy()
            want = tally.check(got, mixed, 1.0, D.IMG_SEED, D.image_key(np.arange(B), b_off, img_off, step), E_g, ctx=(b_off, img_off, step))
            for b in range(B):
                seen[(b + b_off + img_off, step)] = int(want[b])
    tally.close()
    assert tally.open == 0
    g0 = {k: v for k, v in seen.items() if k[1] == 0}
    assert len(set(g0.values())) > len(g0) // 2, g0                      # across images
    for gi in {k[0] for k in seen}:
        assert len({seen[(gi, s)] for s in D.IMG_STEPS}) > 1, gi         # across steps of one image
    # (b_off, img_off) = (2, 5) and (3, 5) overlap in the global images 8 and 9: same key, same token (checked against the model above)


def test_image_greedy_ties_go_to_the_first_index():
    V, B, S = 1000, 3, 5
    slabs = np.zeros((S, 2 * B, V), dtype=np.float32)
    slabs[:, 0::2, :] = 0.25                                            # image 0: the whole row ties -> token 0
    slabs[0, 2, [999, 700, 701, 63, 64]] += 1.0                         # image 1: five-way tie across threads, waves and chunks -> 63
    slabs[4, 4, [999, 998]] += 2.0                                      # image 2: a tie inside the last (short) chunk, added by the LAST slab -> 998
    flat, slab = O.slabs_dev(slabs)
    for w in (1.0, 5.0):
        r = O.cfg_sample(flat, S, slab, None, V, B, w, 0.0, 3, 0)
        assert r["rc"] == O.PG_OK and r["ok"]
        assert r["tok"][:, 0].tolist() == [0, 63, 998], r["tok"][:, 0].tolist()
    # -0.0 and +0.0 tie as well
    z = np.full((1, 2, 17), -1.0, dtype=np.float32)
    z[0, :, 5], z[0, :, 11] = -0.0, 0.0
    flat, slab = O.slabs_dev(z)
    assert O.cfg_sample(flat, 1, slab, None, 17, 1, 1.0, 0.0, 3, 0)["tok"][0, 0].item() == 5


def test_image_force_and_mask_rules():
    """Every combination of has_force, has_mask and the mask bit; forced tokens outside [0, V) are emitted as given and fed clamped; step == T writes nothing."""
    V, B, S, T, b_off, B_total = 17, 3, 2, 5, 1, 5
    rng = np.random.default_rng(8)
    slabs = D.dyadic_slabs(rng, S, 2 * B, V, 1.5)
    flat, slab = O.slabs_dev(slabs)
    mixed = D.image_mixed(dict(slabs=slabs, bias=None, w=5.0))
    drawn = D.greedy(mixed)
    force = np.full((B_total, T), 3, dtype=np.int32)
    force[1:4, 2] = [V + 5, -3, 9]
    force[1:4, 4] = [0, V - 1, V]
    for step in (2, 4, T, T + 3):
        for has_force, mask_bit in ((False, None), (True, None), (True, 0), (True, 1)):
            mask = None if mask_bit is None else np.full((B_total, T), mask_bit, dtype=np.uint8)
            r = O.cfg_sample(flat, S, slab, None, V, B, 5.0, 0.0, 1, step, T, 0, b_off, B_total, force=force if has_force else None, mask=mask, tap=False)
            emits, feeds = zip(*[D.cfg_pick(int(drawn[b]), V, T, step, force[b_off + b] if has_force else None, None if mask is None else mask[b_off + b])
                                 for b in range(B)])
            if step >= T:
                assert all(e is None for e in emits) and list(feeds) == drawn.tolist()
            _check_image_outputs(r, B, b_off, min(step, T - 1), T, list(emits), list(feeds))
    # a mixed mask: bit per image
    mask = np.ones((B_total, T), dtype=np.uint8)
    mask[2, 2] = 0
    r = O.cfg_sample(flat, S, slab, None, V, B, 5.0, 0.0, 1, 2, T, 0, b_off, B_total, force=force, mask=mask, tap=False)
    emits, feeds = zip(*[D.cfg_pick(int(drawn[b]), V, T, 2, force[b_off + b], mask[b_off + b]) for b in range(B)])
    assert emits[1] == -3 and feeds[1] == 0 and emits[0] == drawn[0]
    _check_image_outputs(r, B, b_off, 2, T, list(emits), list(feeds))


def _special_rows(V, rng):
    """[6, V] float64: -inf entries, +inf entry, NaN entries, all -inf, all NaN, a mixture with nothing drawable."""
    inf, nan = np.inf, np.nan
    x = np.rint(rng.standard_normal((6, V)) * 2.4 * D.Q) / D.Q
    x[0, rng.random(V) < 0.5] = -inf
    x[0, 0] = 1.0
    x[1, V // 3], x[1, V - 1] = inf, inf                                # two +inf: the first
    x[2, rng.random(V) < 0.5] = nan
    x[2, V - 1] = 0.5
    x[3] = -inf
    x[4] = nan
    x[5, 0::2], x[5, 1::2] = nan, -inf
    return x


@pytest.mark.parametrize("V", [17, 1000, 16384])
def test_image_special_values(V, E_g):
    """-inf and NaN entries are never drawn, +inf always (the first one); a row with nothing to draw emits the pinned token, inside [0, V), and gathers an
    in-bounds embedding row (the NaN guard rows behind the table and the slabs stay out of every result).  cfg_weight 1 carries the cond row's value through."""
    rng = np.random.default_rng(9 + V)
    rows = _special_rows(V, rng)
    B = len(rows)
    slabs = np.zeros((1, 2 * B, V), dtype=np.float32)
    slabs[0, 0::2] = rows
    flat, slab = O.slabs_dev(slabs)
    tally = Tally(f"image special V={V}")
    for temperature, filtered in ((0.0, 0), (0.7, 0), (1.3, 0), (0.7, 1)):
        for step in (0, 1, 2):
            r = O.cfg_sample(flat, 1, slab, None, V, B, 1.0, temperature, D.IMG_SEED, step, filtered=filtered, top_k=0, top_p=1.0)
            assert r["rc"] == O.PG_OK and r["ok"]
            assert _same(r["tap"], torch.from_numpy(rows).float())
            got = r["tok"][:, step].numpy()
            none = 0 if filtered else V - 1
            if temperature > 0:
                tally.check(got, rows, temperature, D.IMG_SEED, D.image_key(np.arange(B), 0, 0, step), E_g, none_token=none, ctx=(temperature, filtered, step))
            else:
                want = D.greedy(rows)
                assert (got == np.where(want == D.NONE, none, want)).all()
            assert np.isfinite(rows[0, got[0]]) and got[1] == V // 3 and np.isfinite(rows[2, got[2]])
            assert got[3:].tolist() == [none] * 3                                   # pinned: DESIGN.md section 2
            _check_image_outputs(r, B, 0, step, 576, got.tolist(), got.tolist())    # x rows are finite table rows: nothing read behind the table
    tally.close()


@pytest.mark.parametrize("V", [17, 1000, 16384])
def test_image_filtered_draw_is_the_models_draw_over_the_kept_set(V, E_g, tiny_cfg):
    """The filtered route of launch_cfg_step: the token is the model's draw restricted to the kept mask pg_op_sample_filter returns for the same row, and it is the
    unfiltered operator's token whenever that one is kept."""
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    if "fe" not in _S:
        _S["fe"] = Engine(PlanGenConfig(**dict(tiny_cfg.model_dict(), img_vocab=16384)), dtype="f32", max_rows=4, max_prompt=16, max_new=8, max_images=2)
    e = _S["fe"]
    B, S = 3, 2
    tally = Tally(f"image filtered V={V}")
    rng = np.random.default_rng(10 + V)
    n_kept = n_not = 0
    for i, (temperature, k, p) in enumerate(((1.0, 5, 1.0), (0.7, 0, 0.8), (1.3, 50, 0.9), (1.0, 0, 1.0), (1.0, 1, 1.0))):
        slabs = D.dyadic_slabs(rng, S, 2 * B, V, 1.5)
        flat, slab = O.slabs_dev(slabs)
        mixed = D.image_mixed(dict(slabs=slabs, bias=None, w=1.0))   # cfg_weight 1: flat enough that unfiltered draws fall outside small kept sets
        keep = e.sample_filter(torch.from_numpy(mixed).float(), temperature, k, p).cpu().numpy()
        assert keep.any(-1).all()
        for step in (0, 1, 2, 3, 574, 575):
            keys = D.image_key(np.arange(B), 1, 7, step)
            a = dict(T=576, img_off=7, b_off=1, B_total=B + 2)
            rf = O.cfg_sample(flat, S, slab, None, V, B, 1.0, temperature, D.IMG_SEED + i, step, filtered=1, top_k=k, top_p=p, **a)
            ru = O.cfg_sample(flat, S, slab, None, V, B, 1.0, temperature, D.IMG_SEED + i, step, **a)
            assert rf["rc"] == O.PG_OK and rf["ok"] and ru["ok"]
            if rf["tap"] is not None:
                assert torch.equal(rf["tap"].double(), torch.from_numpy(mixed))
            gf, gu = rf["tok"][1:1 + B, step].numpy(), ru["tok"][1:1 + B, step].numpy()
            tally.check(gf, mixed, temperature, D.IMG_SEED + i, keys, E_g, keep=keep, ctx=(temperature, k, p, step))
            kept = keep[np.arange(B), gu]
            assert (gf[kept] == gu[kept]).all() and keep[np.arange(B), gf].all()
            n_kept, n_not = n_kept + int(kept.sum()), n_not + int((~kept).sum())
            _check_image_outputs(rf, B, 1, step, 576, gf.tolist(), gf.tolist())
    tally.close()
    assert n_kept > 0 and n_not > 0


def test_operator_argument_errors_launch_nothing():
    V, B, S = 17, 1, 1
    slabs = np.zeros((S, 2 * B, V), dtype=np.float32)
    flat, slab = O.slabs_dev(slabs)
    base = dict(flat=flat, S=S, slab=slab, bias=None, V=V, B=B, w=1.0, temperature=0.0, seed=0, step=0)
    bad = [dict(S=0), dict(V=0), dict(B=0), dict(slab=2 * B * V - 1), dict(step=-1), dict(step=576, tap=True), dict(T=0), dict(b_off=1, B_total=1),
           dict(img_off=-1), dict(mask=np.zeros((1, 576), dtype=np.uint8)), dict(filtered=1), dict(filtered=1, temperature=1.0, top_p=0.0),
           dict(filtered=1, temperature=1.0, top_k=-1), dict(temperature=float("nan"))]
    for kw in bad:
        r = O.cfg_sample(**dict(base, **kw))
        assert r["rc"] == O.PG_ERR_ARG, kw
        assert r["ok"] and (r["tok"] == O.UNSET).all() and torch.isnan(r["x"]).all(), kw
    big = np.zeros((1, 2, 16385), dtype=np.float32)
    f2, s2 = O.slabs_dev(big)
    assert O.cfg_sample(f2, 1, s2, None, 16385, 1, 1.0, 1.0, 0, 0, filtered=1)["rc"] == O.PG_ERR_ARG            # more than the select kernel's LDS row
    assert O.cfg_sample(**base)["rc"] == O.PG_OK
    tflat, tslab = O.slabs_dev(np.zeros((1, 2, V), dtype=np.float32))
    tbase = dict(flat=tflat, S=1, slab=tslab, V=V, B=2, mode=0, temperature=0.0, seed=0, step=0, eos=2)
    for kw in (dict(mode=2), dict(mode=1), dict(mode=1, temperature=-1.0), dict(S=0), dict(V=0), dict(B=0), dict(slab=2 * V - 1), dict(step=-1),
               dict(step=4096, tap=True), dict(max_new=0), dict(min_new=-1), dict(row_off=-1)):
        r = O.text_draw(**dict(tbase, **kw))
        assert r["rc"] == O.PG_ERR_ARG, kw
        assert r["ok"] and (r["out"] == O.UNSET).all() and torch.isnan(r["x"]).all() and r["unfinished"].tolist() == [1] * kw.get("B", 2), kw
    assert O.text_draw(**tbase)["rc"] == O.PG_OK


# ------------------------------------------------------------------------------------------------------------------------------------------------------- (c)
def _check_text_outputs(r, B, step, max_new, toks, unf_in, eos, V):
    assert r["rc"] == O.PG_OK and r["ok"]
    want = torch.full_like(r["out"], O.UNSET)
    for b in range(B):
        tok, still, row = D.text_pick(int(toks[b]), unf_in[b], eos, V)
        if step < max_new:
            want[b, step] = tok
        assert torch.equal(r["x"][b], O.table_row(row)), (b, tok, r["x"][b])
        assert int(r["unfinished"][b]) == still, (b, tok)
    assert torch.equal(r["out"], want)


@pytest.mark.parametrize("S", D.TXT_S)
@pytest.mark.parametrize("V", D.TXT_V_SCALAR + D.TXT_V_VECTOR)
def test_text_operator_draws_the_models_token(V, S, E_g):
    """text_scan_kernel (greedy and the in-scan Gumbel draw) + text_argmax_kernel: V = 1 / 3 / 255 with an odd slab stride take the scalar branch of the
    scan body, V = 4 / 4100 / 102400 with a stride that is a multiple of 4 the 16-byte one; the EOS ban below min_new, row_off, steps up to 4095, seeds >= 2^63,
    finished rows."""
    tally = Tally(f"text V={V} S={S}")
    B = D.TXT_B
    vector = V in D.TXT_V_VECTOR
    unf_in = [1, 1, 0, 1, 1, 1]
    for c in D.text_cases(V, S):
        flat, slab = O.slabs_dev(c["slabs"], B * V + (8 if vector else (1 if (B * V) % 2 == 0 else 2)))
        assert (slab % 4 == 0 and V % 4 == 0) == vector
        for step in c["steps"]:
            rows = D.text_rows(c, step)
            r = O.text_draw(flat, S, slab, V, B, 1 if c["T"] > 0 else 0, c["T"], c["seed"], step, c["eos"], c["min_new"], c["max_new"], c["row_off"], unf_in)
            if r["tap"] is not None:
                assert torch.equal(r["tap"].double(), torch.from_numpy(rows)), (c["T"], step)
            got = r["out"][:, step].numpy()
            live = np.array(unf_in, dtype=bool)
            assert (got[~live] == c["eos"]).all()
            if c["T"] > 0:
                want = tally.check(got[live], rows[live], c["T"], c["seed"], D.text_key(np.arange(B), c["row_off"], step)[live], E_g,
                                   ctx=(c["T"], step, c["row_off"], c["min_new"]))
                drawn = np.where(live, 0, 0)
                drawn[live] = got[live]
            else:
                g = D.greedy(rows)
                drawn = np.where(g == D.NONE, 0, g)
                assert (got[live] == drawn[live]).all()
            if step < c["min_new"] and V > 1:
                assert (got[live] != c["eos"]).all()                    # the ban
            _check_text_outputs(r, B, step, c["max_new"], drawn, unf_in, c["eos"], V)
    tally.close()


@pytest.mark.parametrize("V,slab_pad", [(255, 1), (4100, 0), (4100, 1), (102400, 4)])
def test_text_special_values_and_the_select_kernel(V, slab_pad, E_g):
    """Special values through both scan branches, and pg_op_text_sample (text_select_kernel) on the same rows: its token is the model's draw over its own
    returned mask; with the filters off it is the in-scan token."""
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    if "te" not in _S:
        _S["te"] = Engine(PlanGenConfig(**dict(PlanGenConfig.tiny().model_dict(), vocab=102400, eos_id=7, pad_id=3)), dtype="f32", max_rows=8, max_prompt=16,
                          max_new=8, max_images=1, with_lm_head=True)
    e = _S["te"]
    rng = np.random.default_rng(11 + V)
    rows = _special_rows(V, rng)
    B = len(rows)
    slabs = rows[None].astype(np.float32)
    flat, slab = O.slabs_dev(slabs, B * V + slab_pad)
    tally, tsel = Tally(f"text special V={V}"), Tally(f"text select V={V}")
    eos = V - 2
    for temperature, step, row_off in ((0.0, 0, 0), (0.7, 1, 0), (1.3, 3, 9)):
        r = O.text_draw(flat, 1, slab, V, B, 1 if temperature > 0 else 0, temperature, D.TXT_SEED, step, eos, 0, 4096, row_off)
        assert _same(r["tap"], torch.from_numpy(rows).float())
        got = r["out"][:, step].numpy()
        keys = D.text_key(np.arange(B), row_off, step)
        if temperature > 0:
            tally.check(got, rows, temperature, D.TXT_SEED, keys, E_g, none_token=0, ctx=(temperature, step))
        else:
            g = D.greedy(rows)
            assert (got == np.where(g == D.NONE, 0, g)).all()
        assert np.isfinite(rows[0, got[0]]) and got[1] == V // 3 and np.isfinite(rows[2, got[2]])
        assert got[3:].tolist() == [0, 0, 0]                                         # pinned: DESIGN.md section 2
        _check_text_outputs(r, B, step, 4096, got, [1] * B, eos, V)
        if temperature > 0:
            for k, p in ((0, 1.0), (5, 1.0), (0, 0.7)):
                keep, tok = e.text_sample(torch.from_numpy(rows).float(), temperature, k, p, seed=D.TXT_SEED, row_offset=row_off, step=step)
                keep, tok = keep.cpu().numpy(), tok.cpu().numpy()
                tsel.check(tok, rows, temperature, D.TXT_SEED, keys, E_g, keep=keep, none_token=0, ctx=(temperature, k, p))
                if (k, p) == (0, 1.0):
                    assert (tok == got).all()
    # ordinary rows: the select kernel with the filters off equals the in-scan draw, and the model
    c = D.text_cases(V, 1)[1]
    full = c["slabs"].astype(np.float64).sum(0)
    flat, slab = O.slabs_dev(c["slabs"], D.TXT_B * V + slab_pad)
    for step in c["steps"]:
        r = O.text_draw(flat, 1, slab, V, D.TXT_B, 1, c["T"], c["seed"], step, c["eos"], 0, 4096, 5)
        keys = D.text_key(np.arange(D.TXT_B), 5, step)
        got = r["out"][:, step].numpy()
        tally.check(got, full, c["T"], c["seed"], keys, E_g)
        for k, p in ((0, 1.0), (20, 0.9)):
            keep, tok = e.text_sample(torch.from_numpy(full).float(), c["T"], k, p, seed=c["seed"], row_offset=5, step=step)
            tsel.check(tok.cpu().numpy(), full, c["T"], c["seed"], keys, E_g, keep=keep.cpu().numpy())
            if (k, p) == (0, 1.0):
                assert (tok.cpu().numpy() == got).all()
    tally.close()
    tsel.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------------- (d)
def _image_prompt(cfg, nimg, seed):
    from plangen_amd.system import t2i_infer_collate_batch
    g = torch.Generator().manual_seed(seed)
    cond = [torch.randint(8, cfg.vocab, (n,), generator=g).tolist() for n in (9, 6, 11, 7)[:nimg]]
    neg = torch.randint(8, cfg.vocab, (4,), generator=g).tolist()
    ids, mask = t2i_infer_collate_batch(cond, neg, cfg.pad_id, cfg.img_tokens)
    return ids, (ids.shape[1] - mask[:, :ids.shape[1]].sum(-1)).tolist(), g


def _check_image_loop(tally, toks, lg, temperature, seed, E_g, img_off=0):
    """toks [B, T], lg [T, B, V]: every emitted token is the model's draw on the tapped row with the loop's key (image b + img_off, step t)."""
    T, B, V = lg.shape
    rows = lg.cpu().double().numpy().reshape(T * B, V)
    t, b = np.divmod(np.arange(T * B), B)
    tally.check(toks.cpu().numpy().T.reshape(-1), rows, temperature, seed, D.image_key(b, 0, img_off, t), E_g)


def test_image_loop_emits_the_models_draws(tiny_cfg, tiny_weights, E_g):
    """decode_image_tokens on the tiny model, fp32: free-running and teacher-forced (no mask: the emitted tokens are still the draws), two temperatures, one
    and two decode lanes, a shifted rng_image_offset."""
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, g = _image_prompt(tiny_cfg, 4, 91)
    T = 24
    force = torch.randint(0, tiny_cfg.img_vocab, (4, T), generator=g).int()
    tally = Tally("image loop tiny")
    seed = (1 << 63) + 77
    try:
        for lanes in (1, 2):
            e.set_option("lanes", lanes)
            for temperature in (0.7, 1.3):
                for ft in (None, force):
                    e.prefill(ids, pad)
                    toks, lg = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=temperature, seed=seed, force_tokens=ft, return_logits=True)
                    _check_image_loop(tally, toks, lg, temperature, seed, E_g)
        e.set_option("lanes", -1)
        e.set_option("rng_image_offset", 4000)
        e.prefill(ids, pad)
        toks, lg = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=1.0, seed=5, return_logits=True)
        _check_image_loop(tally, toks, lg, 1.0, 5, E_g, img_off=4000)
    finally:
        e.set_option("lanes", -1)
        e.set_option("rng_image_offset", 0)
    tally.close()


def test_text_loop_emits_the_models_draws(tiny_cfg, tiny_weights, E_g):
    """generate_text sampled on the generate_tiny fixture's prompts: every token an unfinished row emits is the model's draw on the tapped row with the key
    (row, step)."""
    from plangen_amd.engine import Engine
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    gf = load_golden("generate_tiny.npz")
    ids, mask = torch.from_numpy(gf["ids"].astype(np.int32)), torch.from_numpy(gf["mask"].astype(np.int32))
    eos = int(gf["eos"])
    tally = Tally("text loop tiny")
    for temperature, seed, min_new in ((0.7, 3, 0), (1.3, (1 << 63) + 5, 6)):
        e.prefill_embeds(e.embed_tokens(ids.to(e.device)), Engine.pad_len_from_mask(mask, ids.shape[1]), position_mode=1)
        out, lg = e.generate_text(12, eos, min_new_tokens=min_new, temperature=temperature, seed=seed, return_logits=True)
        out, lg = out.cpu().numpy(), lg.cpu().double().numpy()
        n, R, V = lg.shape
        live = np.ones(R, dtype=bool)
        for t in range(n):
            if live.any():
                tally.check(out[live, t], lg[t][live], temperature, seed, D.text_key(np.arange(R), 0, t)[live], E_g, ctx=(temperature, t))
            assert (out[~live, t] == eos).all()
            if t < min_new:
                assert (out[:, t] != eos).all() and np.isneginf(lg[t][:, eos]).all()
            live &= out[:, t] != eos
    tally.close()
    assert tally.n >= 20


def test_image_loop_at_the_full_width_vocabulary(E_g):
    """Six steps of the loop at img_vocab 16 384 and Janus width: the draw over the real head GEMM's slabs."""
    from fullwidth_cfg import FULLW
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    cfg = PlanGenConfig(**FULLW)
    e = Engine(cfg, dtype="f32", max_rows=8, max_prompt=32, max_new=8, max_images=4)
    try:
        e.init_synthetic(seed=3)
        ids, pad, _ = _image_prompt(cfg, 4, 92)
        tally = Tally("image loop full width")
        for temperature, seed in ((1.0, 11), (0.7, (1 << 63) + 12)):
            e.prefill(ids, pad)
            toks, lg = e.decode_image_tokens(T=6, cfg_weight=5.0, temperature=temperature, seed=seed, return_logits=True)
            _check_image_loop(tally, toks, lg, temperature, seed, E_g)
        tally.close()
    finally:
        e.close()
