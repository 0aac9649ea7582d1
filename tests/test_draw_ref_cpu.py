"""CPU: the host model of the samplers' draw (tests/draw_ref.py) against independent arithmetic, its stream keys' distinctness over the production ranges,
its draws against softmax, and -- for every input family tests/test_gpu_draws.py uses -- the share of draws that the decided / undecided rule leaves
open, with the conservative Gumbel-term error E_g = 2^-16 (the GPU tests use the measured one, which must not exceed it for this to carry over)."""
import math

import numpy as np
import pytest

import draw_ref as D

M64 = (1 << 64) - 1


def _rng_bits_int(seed, a, b):
    """csrc/common.h rng_bits with Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (a + 1) + 0xBF58476D1CE4E5B9 * (b + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_rng_bits_equals_python_integer_arithmetic():
    rng = np.random.default_rng(1)
    seeds = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 12345, (1 << 63) - 1, 1 << 63, (1 << 63) + 0x1234567, M64] + \
        [int(x) for x in rng.integers(0, 1 << 63, 8)] + [int(x) + (1 << 63) for x in rng.integers(0, 1 << 63, 8)]
    a_s = [0, 1, 575, 1000003, 127 * 1000003 + 575, (4096 + 127) * 1000003 + 575, M64, M64 - 1] + [int(x) for x in rng.integers(0, 1 << 40, 12)]
    b_s = [0, 1, 255, 16383, 102399, M64] + [int(x) for x in rng.integers(0, 102400, 10)]
    n = 0
    for seed in seeds:
        got = D.rng_bits(seed, np.array(a_s, dtype=object)[:, None], np.array(b_s, dtype=np.uint64)[None, :])
        assert got.dtype == np.uint64 and got.shape == (len(a_s), len(b_s))
        for i, a in enumerate(a_s):
            for j, b in enumerate(b_s):
                assert int(got[i, j]) == _rng_bits_int(seed, a, b), (seed, a, b)
                n += 1
    assert n >= 4000
    # scalar form, and a seed given as a numpy integer
    assert int(D.rng_bits(np.uint64(1 << 63), 5, 7)) == _rng_bits_int(1 << 63, 5, 7)


def test_uniform_is_the_formula_the_device_test_asserts():
    """tests/test_gpu_ops.py::test_sampler_uniform_strictly_inside_unit_interval: ((bits >> 41) + 0.5) / 2^23, extremes 2^-24 and 1 - 2^-24, every value
    an fp32 number."""
    rng = np.random.default_rng(2)
    bits = np.concatenate([np.array([0, 1, (1 << 41) - 1, 1 << 41, M64, M64 - (1 << 41) + 1, M64 - (1 << 41)], dtype=np.uint64),
                           rng.integers(0, 1 << 63, 5000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 5000, dtype=np.uint64)])
    u = D.uniform(bits)
    want = np.array([((int(b) >> 41) + 0.5) / 2 ** 23 for b in bits])
    assert (u == want).all()
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    g = D.gumbel(u)
    assert np.isfinite(g).all() and (np.diff(D.gumbel(np.sort(u))) >= 0).all()
    assert D.gumbel(0.5) == -math.log(math.log(2.0))


def test_stream_keys_are_the_stated_integers_and_pairwise_distinct():
    assert int(D.image_key(2, 3, 4, 5)) == (2 + 3 + 4) * 1000003 + 5
    assert int(D.text_key(6, 7, 8)) == (6 + 7) * 1000003 + 8
    assert int(D.image_key(0, 0, 0, 0)) == 0 and int(D.text_key(0, 0, 4095)) == 4095
    # the image loop: 128 images x 576 steps, img_off up to 4096 -- the key depends on the global image index b + b_off + img_off alone
    gi = np.arange(128 + 4096 + 1, dtype=np.uint64)
    k = D.image_key(gi[:, None], 0, 0, np.arange(576, dtype=np.uint64)[None, :]).ravel()
    assert len(np.unique(k)) == k.size
    for b, b_off, img_off in ((127, 0, 4096), (0, 64, 4032), (5, 100, 7)):
        assert (D.image_key(b, b_off, img_off, np.arange(576)) == k.reshape(len(gi), 576)[b + b_off + img_off]).all()
    # each of step, b, b_off, img_off moves the key
    base = int(D.image_key(3, 2, 5, 7))
    assert len({base, int(D.image_key(3, 2, 5, 8)), int(D.image_key(4, 2, 5, 7)), int(D.image_key(3, 3, 5, 8)), int(D.image_key(3, 2, 7, 7))}) == 5
    # the text loop: rows (with row_off) x 4096 steps
    rows = np.arange(1024, dtype=np.uint64)
    kt = D.text_key(rows[:, None], 0, np.arange(4096, dtype=np.uint64)[None, :]).ravel()
    assert len(np.unique(kt)) == kt.size
    assert int(D.text_key(3, 4000, 4095)) == int(kt.reshape(1024, 4096)[3, 4095]) + 4000 * 1000003


def test_greedy_draw_and_pick_rules():
    inf, nan = np.inf, np.nan
    assert D.greedy([[1.0, 3.0, 3.0, 2.0]]).tolist() == [1]                         # first index of the maximum
    assert D.greedy([[nan, -inf, nan]]).tolist() == [D.NONE]
    assert D.greedy([[nan, -1.0, nan, -1.0]]).tolist() == [1]
    assert D.greedy([[5.0, 4.0, 9.0]], keep=[[True, True, False]]).tolist() == [0]
    x = np.array([[0.0, -inf, nan, 1.0], [-inf, -inf, nan, -inf], [0.0, inf, 0.0, inf]])
    tok, gap, scale = D.draw(x, 1.0, 9, D.text_key(np.arange(3), 0, 0))
    assert tok[0] in (0, 3) and tok[1] == D.NONE and tok[2] == 1 and gap[2] == inf and gap[1] == inf
    tok1, gap1, _ = D.draw([[2.5]], 0.7, 1, [0])
    assert tok1.tolist() == [0] and gap1[0] == inf
    # keep restricts the draw; the unrestricted winner, when kept, is the restricted winner
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((64, 50)) * 2.4
    keys = D.text_key(np.arange(64), 11, 2)
    t_all, _, _, ru = D.draw_top2(rows, 1.3, 77, keys)
    keep = rng.random((64, 50)) < 0.5
    keep[np.arange(64), ru] = True
    t_k = D.draw(rows, 1.3, 77, keys, keep)[0]
    kept = keep[np.arange(64), t_all]
    assert (t_k[kept] == t_all[kept]).all() and (t_k[~kept] == ru[~kept]).all() and kept.any() and (~kept).any()
    # the feedback rules
    V, T = 10, 4
    force, m0, m1 = [7, 12, -3, 5], [0, 0, 0, 0], [1, 1, 1, 1]
    assert D.cfg_pick(4, V, T, 1) == (4, 4)
    assert D.cfg_pick(4, V, T, 0, force) == (4, 7)                                  # no mask: feed = forced only
    assert D.cfg_pick(4, V, T, 0, force, m0) == (7, 7)                              # mask 0: emit = feed = forced
    assert D.cfg_pick(4, V, T, 0, force, m1) == (4, 4)
    assert D.cfg_pick(4, V, T, 1, force, m0) == (12, 9) and D.cfg_pick(4, V, T, 2, force, m0) == (-3, 0)     # feed clamped, emit as forced
    assert D.cfg_pick(4, V, T, 4, force, m0) == (None, 4)                           # step >= T: nothing written, nothing forced
    assert D.cfg_pick(D.NONE, V, T, 0, none_token=V - 1) == (9, 9) and D.cfg_pick(D.NONE, V, T, 0, none_token=0) == (0, 0)
    assert D.text_pick(D.NONE, 1, 2, V) == (0, 1, 0) and D.text_pick(5, 0, 2, V) == (2, 0, 2) and D.text_pick(2, 1, 2, V) == (2, 0, 2)
    assert D.text_pick(5, 0, 100001, V) == (100001, 0, 9)


def test_decided_rule():
    assert not D.decided(0.0, 1.0, 0.0) and D.decided(np.inf, 1e9, 1.0)
    e = 2.0 ** -16
    thr = 2 * (e + 3 * 2.0 ** -24 * 8.0)
    assert D.decided(thr * 1.0001, 8.0, e) and not D.decided(thr, 8.0, e)


def test_model_draws_follow_softmax_chi_square():
    from scipy import stats
    V, N = 256, 60000
    rng = np.random.default_rng(4)
    row = rng.standard_normal(V) * 2.4
    for T, seed, row_off in ((1.0, 5, 0), (0.7, (1 << 63) + 9, 3)):
        p = np.exp(row / np.float32(T) - (row / np.float32(T)).max())
        p /= p.sum()
        tok = np.concatenate([D.draw(np.broadcast_to(row, (2000, V)), T, seed, D.image_key(np.arange(i, i + 2000) // 576, row_off, 0, np.arange(i, i + 2000) % 576))[0]
                              for i in range(0, N, 2000)])
        obs = np.bincount(tok, minlength=V).astype(np.float64)
        order = np.argsort(-p)
        bins_o, bins_e, o, e = [], [], 0.0, 0.0
        for v in order:                                                         # pool from the most probable down until a bin expects >= 20
            o, e = o + obs[v], e + N * p[v]
            if e >= 20:
                bins_o.append(o); bins_e.append(e); o = e = 0.0
        bins_o[-1] += o; bins_e[-1] += e
        bo, be = np.array(bins_o), np.array(bins_e)
        assert be.min() >= 20 and len(be) > 20
        chi2 = ((bo - be) ** 2 / be).sum()
        pval = 1 - stats.chi2.cdf(chi2, df=len(be) - 1)
        print(f"T={T}: {len(be)} bins, chi2 {chi2:.1f}, p {pval:.3f}")
        assert pval > 1e-4, (T, chi2, pval)


def _share(rows, T, seed, keys):
    _, gap, scale = D.draw(rows, T, seed, keys)
    und = ~D.decided(gap, scale, D.E_G_CPU)
    return int(und.sum()), und.size


@pytest.mark.parametrize("V", D.IMG_V)
def test_image_families_leave_under_one_percent_undecided(V):
    tot_u = tot_n = 0
    for S in D.IMG_S:
        for bias in (False, True):
            u = n = 0
            for c in D.image_cases(V, S, bias):
                if c["T"] <= 0:
                    continue
                mixed = D.image_mixed(c)
                assert (mixed.astype(np.float32).astype(np.float64) == mixed).all()            # the fp32 row is this row, exactly
                for step in c["steps"]:
                    du, dn = _share(mixed, c["T"], c["seed"], D.image_key(np.arange(c["B"]), c["b_off"], c["img_off"], step))
                    u, n = u + du, n + dn
            assert n >= 100 and u <= D.UNDECIDED_CAP * n, (V, S, bias, u, n)
            tot_u, tot_n = tot_u + u, tot_n + n
    print(f"image V={V}: {tot_u} of {tot_n} draws undecided at E_g = 2^-16")


@pytest.mark.parametrize("V", D.TXT_V_SCALAR + D.TXT_V_VECTOR)
def test_text_families_leave_under_one_percent_undecided(V):
    tot_u = tot_n = 0
    for S in D.TXT_S:
        u = n = 0
        for c in D.text_cases(V, S):
            if c["T"] <= 0:
                continue
            for step in c["steps"]:
                rows = D.text_rows(c, step)
                du, dn = _share(rows, c["T"], c["seed"], D.text_key(np.arange(D.TXT_B), c["row_off"], step))
                u, n = u + du, n + dn
        assert n >= 100 and u <= D.UNDECIDED_CAP * n, (V, S, u, n)
        tot_u, tot_n = tot_u + u, tot_n + n
    print(f"text V={V}: {tot_u} of {tot_n} draws undecided at E_g = 2^-16")


def test_loop_like_rows_leave_under_one_percent_undecided():
    """The loops' rows are the model's own logits (not dyadic): Gaussian rows of the measured spread at the tiny and the full-width vocabularies."""
    rng = np.random.default_rng(6)
    for V, n_rows, std in ((256, 512, 2.4), (256, 512, 9.6), (512, 512, 2.4), (16384, 64, 9.6)):
        rows = (rng.standard_normal((n_rows, V)) * std).astype(np.float32)
        for T in (0.7, 1.3):
            u, n = _share(rows, T, 12345, D.image_key(np.arange(n_rows) % 4, 0, 0, np.arange(n_rows) // 4))
            print(f"V={V} std={std} T={T}: {u} of {n} undecided")
            assert u <= D.UNDECIDED_CAP * n, (V, std, T, u, n)
