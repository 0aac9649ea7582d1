"""CPU: the reference, cases and mutants of tests/prefill_lin_ref.py, checked without a GPU -- what tests/test_gpu_prefill_lin_ops.py relies on:
the tile arithmetic of the cases (every one is admitted by gemm256_try's rule, the edges are where they claim to be), every mutant reference lies OUTSIDE
the bound on the chosen inputs, and the reference's own fp32 re-evaluation in another summation order stays under HALF the bound on every case, so a
ratio <= 1.0 measured on the GPU leaves no room for a mutant."""
import pytest
import torch

import prefill_lin_ref as P

NCU = P.NOMINAL_CUS


@pytest.fixture(scope="module")
def k128():
    rows = P.group_rows("k128", NCU)
    return rows, P.core("k128", rows)


def test_case_arithmetic():
    assert P.smallest_m(2048) == 6145 and P.smallest_m(256) == 50945
    assert not P.gemm256_takes(6144, 2048, 128, 1) and not P.gemm256_takes(6145, 2048, 64, 1) and not P.gemm256_takes(6145, 2048, 96, 1)
    ms = P.edge_ms(2048)
    for h in (256, 224, 192):
        k = -(-6146 // h)
        assert {k * h - 1, k * h, k * h + 1} <= set(ms), (h, sorted(ms))
    assert 6145 % 256 == 1 and 6399 % 256 == 255 and 6399 in ms and 6273 % 224 == 1
    assert all(6273 % h for h in (256, 224, 192))                               # the epilogue matrix's M: ragged at every height
    cs = P.cases256(NCU)
    assert len({c["id"] for c in cs}) == len(cs)
    assert {c["epi"] for c in cs if c["M"] == 6273} == set(P.EPIS)
    assert {c["K"] for c in cs} == {128, 192, 2048, 5632} and {c["N"] for c in cs} == {2048, 1800, 1802, 256}
    for ncu in (64, 104, 256, 304):
        wm = P.wrap_m(ncu)
        assert P.gemm256_takes(wm, 2048, 128, 1)
        assert 0 < P.tiles(wm, 2048, 256) - ncu <= 8 or (ncu < 200 and P.tiles(wm, 2048, 256) == 200)
        assert all(P.tiles(wm, 2048, h) > ncu for h in (256, 224, 192))
        assert len(P.second_pass_tiles(wm, 2048, 256, ncu)) == min(ncu, P.tiles(wm, 2048, 256) - ncu)
    # the rounds' tiles together are the tiles of the matrix, each once
    wm = P.wrap_m(NCU)
    for h in (256, 224, 192):
        ntm, ntn = -(-wm // h), 8
        allt = [t for r in range(-(-ntm * ntn // NCU)) for t in P.round_tiles(wm, 2048, h, NCU, r)]
        assert sorted(allt) == [(i, j) for i in range(ntm) for j in range(ntn)], h
    assert P.auto_height(13285, 2048, 256) in (256, 224, 192)
    assert P.is_pow2(0.125) and P.is_pow2(1.0) and not P.is_pow2(0.37)


@pytest.mark.parametrize("mutant", list(P.MUTANTS))
def test_every_mutant_lies_outside_the_bound(k128, mutant):
    rows, cr = k128
    M = P.wrap_m(NCU) if mutant == "wrap_skip" else 6273
    c = P.make_case("k128", M, 2048, P.MUTANTS[mutant])
    ref, mag = P.lin_ref(c, cr, rows)
    bound = P.lin_bound(c, ref, mag)
    for h in ((256, 224, 192) if mutant == "wrap_skip" else (256,)):
        bad, _ = P.lin_ref(c, cr, rows, mutant, height=h, G=NCU)
        wrong = ((bad - ref).abs() > bound) | torch.isnan(bad)
        print(f"{mutant} (height {h}): {int(wrong.sum())} of {wrong.numel()} elements outside the bound")
        assert P.ratio(bad, ref, bound) > 1.0
        if mutant == "wrap_skip":
            assert int(wrong.sum()) > 0.9 * sum(min(h, M - tm * h) * 256 for tm, _ in P.second_pass_tiles(M, 2048, h, NCU))
        if mutant == "clip16":
            assert M % 16 and int(wrong.sum()) > 0.9 * (M % 16) * 2048
    # and the checker takes the reference's own rounding to the output type
    assert P.ratio(P.rnd(ref.float(), c["out"]), ref, bound) <= 1.0


def test_clip16_and_wrap_leave_nan_where_the_output_is_not_the_residual(k128):
    rows, cr = k128
    c = P.make_case("k128", 6273, 2048, "bare")
    bad, _ = P.lin_ref(c, cr, rows, "clip16")
    assert bool(torch.isnan(bad[6272:]).all()) and not bool(torch.isnan(bad[:6272]).any())
    assert P.ratio(bad, *_rb(c, cr, rows)) == float("inf")
    M = P.wrap_m(NCU)
    c = P.make_case("k128", M, 2048, "bare")
    bad, _ = P.lin_ref(c, cr, rows, "wrap_skip", height=224, G=NCU)
    assert int(torch.isnan(bad).sum()) == sum(min(224, M - tm * 224) * 256 for tm, _ in P.second_pass_tiles(M, 2048, 224, NCU)) > 0


def _rb(c, cr, rows):
    ref, mag = P.lin_ref(c, cr, rows)
    return ref, P.lin_bound(c, ref, mag)


def _margin(c, cr, rows, row_idx=None):
    """max |fp32 re-evaluation - ref| / (bound without the store term); the store itself is checked separately: the rounded re-evaluation is within the full bound."""
    ref, mag = P.lin_ref(c, cr, rows, row_idx=row_idx)
    v = P.lin_emul32(c, rows, row_idx)
    r = P.ratio(v, ref, P.lin_bound(c, ref, mag, store=False))
    assert P.ratio(P.rnd(v, c["out"]), ref, P.lin_bound(c, ref, mag)) <= 1.0
    return r


def test_fp32_reevaluation_stays_under_half_the_bound_k128(k128):
    """Cases of one (group, N, epilogue) are row prefixes of the largest one: its elements are theirs."""
    rows, cr = k128
    largest = {}
    for c in P.cases256(NCU):
        if c["group"] == "k128":
            largest[(c["N"], c["epi"])] = max(largest.get((c["N"], c["epi"]), 0), c["M"])
    for (N, epi), M in largest.items():
        r = _margin(P.make_case("k128", M, N, epi), cr, rows)
        print(f"k128 M<={M} N={N} {epi}: fp32 re-evaluation / bound = {r:.3f}")
        assert r <= 0.5, (N, epi, r)


@pytest.mark.parametrize("group", ["k192", "n256", "k2048", "k5632"])
def test_fp32_reevaluation_stays_under_half_the_bound(group):
    """The deep cases on every 16th row and the last 33 (the float64 product of all 6145 rows at K = 5632 is the GPU test's, on the device)."""
    rows = P.group_rows(group, NCU)
    cs = [c for c in P.cases256(NCU) if c["group"] == group]
    assert len(cs) == 1 and cs[0]["M"] == rows
    idx = None
    if P.GROUPS[group][1] >= 2048:
        idx = torch.unique(torch.cat([torch.arange(0, rows, 16), torch.arange(rows - 33, rows)]))
    r = _margin(cs[0], P.core(group, rows, row_idx=idx), rows, idx)
    print(f"{cs[0]['id']}: fp32 re-evaluation / bound = {r:.3f}")
    assert r <= 0.5, r


def test_fp32_engine_cases():
    rows = P.group_rows("f32")
    cr = P.core("f32", rows)
    for c in P.cases_f32():
        r = _margin(c, cr, rows)
        assert r <= 0.5, (c["id"], r)
    c = P.make_case("f32", 130, 200, "inplace")
    ref, bound = _rb(c, cr, rows)
    for mutant in ("res_twice", "res_row_xor32", "clip16"):
        assert P.ratio(P.lin_ref(c, cr, rows, mutant)[0], ref, bound) > 1.0, mutant
    c = P.make_case("f32", 130, 200, "bias_m")
    assert P.ratio(P.lin_ref(c, cr, rows, "bias_m_col")[0], *_rb(c, cr, rows)) > 1.0
    c = P.make_case("f32", 130, 200, "res_sep")
    assert P.ratio(P.lin_ref(c, cr, rows, "res_ldc")[0], *_rb(c, cr, rows)) > 1.0
