"""CPU: the references and comparators of tests/skinny_ref.py (used by tests/test_gpu_skinny_ops.py): the slab references sum to the whole float64
product, de-interleaving inverts the [8 gate | 8 up] layout, the comparators accept the reference rounded to the kernels' output formats with room
(so the bounds have room before a kernel is involved) and reject a missing element and each planted error."""
import pytest
import torch

import skinny_ref as R

F64 = torch.float64
SHAPES = [(47, 208, 2048), (47, 4096, 2048), (47, 208, 2816)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda c: "M%d-N%d-K%d" % c)
def case(request):
    M, N, K = request.param
    x, W = R.make_x(M, K), R.make_w(N, K)
    return dict(M=M, N=N, K=K, x=x, W=W, full=R.full_ref(x, W))


def test_inputs_are_asymmetric():
    x13, x47 = R.make_x(13, 2048).to(F64), R.make_x(47, 2048).to(F64)
    rms = x47.pow(2).mean(-1).sqrt()
    assert rms[-4:].min() / rms[:4].max() > 1.5                                 # the row scale 1 + m / M grows along the rows
    assert (x13[-1] - x47[12]).abs().max() > 0.1                               # ... and depends on M: row M - 1 is not a row of another case
    W = R.make_w(208, 2048).to(F64)
    r = W.pow(2).mean(-1).sqrt()
    assert 3.0 < r[-16:].mean() / r[:16].mean() < 5.0                          # linspace(0.5, 2) over the output columns
    assert torch.equal(R.make_x(13, 2048), R.make_x(13, 2048)) and R.make_w(208, 2048) is R.make_w(208, 2048)


@pytest.mark.parametrize("S", [1, 2, 4, 8, 16])
def test_slab_references_sum_to_the_whole_product(case, S):
    if (case["K"] // R.SK_BK) % S:
        S = 2                                                                   # K = 2816: 22 chunks
    slabs = R.slab_refs(case["x"], case["W"], S)
    assert slabs.shape == (S, case["M"], case["N"])
    torch.testing.assert_close(slabs.sum(0), case["full"], rtol=0, atol=1e-12 * float(case["full"].abs().max()))
    if S > 1:                                                                   # the slabs are different things: no two alike
        assert (slabs[0] - slabs[1]).abs().max() > 0.1 * slabs[0].abs().max()


def test_deinterleave_inverts_the_gate_up_layout():
    g = torch.Generator().manual_seed(1)
    I, K = 40, 16
    wg, wu = torch.randn(I, K, generator=g), torch.randn(I, K, generator=g)
    W = R.interleave_rows(wg, wu)
    assert torch.equal(W[:8], wg[:8]) and torch.equal(W[8:16], wu[:8]) and torch.equal(W[16:24], wg[8:16])
    x = torch.randn(5, K, generator=g)
    gg, uu = R.deinterleave_cols(R.full_ref(x, W))
    torch.testing.assert_close(gg, x.to(F64) @ wg.to(F64).t(), rtol=0, atol=1e-13)
    torch.testing.assert_close(uu, x.to(F64) @ wu.to(F64).t(), rtol=0, atol=1e-13)
    want = torch.nn.functional.silu(x.to(F64) @ wg.to(F64).t()) * (x.to(F64) @ wu.to(F64).t())
    torch.testing.assert_close(R.swiglu_ref(x, W), want, rtol=1e-13, atol=1e-13)
    swapped = R.swiglu_ref(x, R.interleave_rows(wu, wg))
    assert (swapped - want).abs().max() > 0.1 * want.abs().max()


@pytest.mark.parametrize("S", [1, 2, 16])
def test_slab_comparator_accepts_the_rounded_reference_with_room(case, S):
    """The float64 reference rounded to fp32 (what a kernel with exact accumulation would store) and torch's own fp32 matmul of the same operands
    (an fp32 accumulation in another order than the kernels') both sit far inside the bound."""
    if (case["K"] // R.SK_BK) % S:
        S = 2
    ref = R.slab_refs(case["x"], case["W"], S)
    res = R.check_slabs(ref.float(), ref)
    kc = case["K"] // S
    xf, Wf = case["x"].float(), case["W"].float()
    f32 = torch.stack([xf[:, s * kc:(s + 1) * kc] @ Wf[:, s * kc:(s + 1) * kc].t() for s in range(S)])
    res32 = R.check_slabs(f32, ref)
    print(f"slab comparator M={case['M']} N={case['N']} K={case['K']} S={S}: fp32-rounded reference at {res['worst']:.3g} of the bound, "
          f"fp32 matmul at {res32['worst']:.3g}")
    assert res["ok"] and res["worst"] < 0.01, res
    assert res32["ok"] and res32["worst"] < 0.1, res32


@pytest.mark.parametrize("N2", [512, 4096])
def test_swiglu_comparator_accepts_the_rounded_reference_with_room(N2):
    M, K = 47, 2048
    x, W = R.make_x(M, K), R.make_w(N2, K, R.SWIGLU_GAIN)
    ref = R.swiglu_ref(x, W)
    g, _ = R.deinterleave_cols(R.full_ref(x, W))
    assert 0.5 < float(g.abs().median()) < 5.0                                  # the SiLU works in its curved range
    res = R.check_swiglu(ref.to(torch.bfloat16), ref)
    g32, u32 = R.deinterleave_cols(x.float() @ W.float().t())
    h32 = g32 / (1 + torch.exp(-g32)) * u32                                     # the epilogue's own formula in fp32
    res32 = R.check_swiglu(h32.to(torch.bfloat16), ref)                         # ... and its one rounding to bf16
    acc = float((h32.to(F64) - ref).abs().max()) / (R.SWIGLU_ATOL * float(ref.abs().max()))
    print(f"SwiGLU comparator 2I={N2}: bf16-rounded reference at {res['worst']:.3g} of the bound, fp32 arithmetic rounded to bf16 at {res32['worst']:.3g}, "
          f"fp32 arithmetic before the rounding at {acc:.3g} of the absolute term")
    assert res["ok"] and res["worst"] < 0.9, res
    assert res32["ok"] and res32["worst"] < 0.9, res32
    assert acc < 0.05, acc


def test_comparators_reject_missing_and_misplaced_elements(case):
    ref = R.slab_refs(case["x"], case["W"], 2)
    out = ref.float()
    out[1, 46, case["N"] - 1] = float("nan")                                    # an element never written
    res = R.check_slabs(out, ref)
    assert not res["ok"] and res["worst"] == float("inf") and res["where"]["rows"] == [46] and res["where"]["n_tiles"] == [case["N"] // 16 - 1]
    out = ref.float()
    out[0, 12:16, 32:48] = 0.0                                                  # an m-tile's last four rows of one n-tile
    res = R.check_slabs(out, ref)
    assert not res["ok"] and res["where"]["rows"] == [12, 13, 14, 15] and res["where"]["n_tiles"] == [2] and res["where"]["part"] == "slab 0"
    dup = ref.float()
    dup[:, 46] = dup[:, 45]                                                     # row M - 1 a copy of its neighbour
    assert not R.check_slabs(dup, ref)["ok"]
    if case["N"] == 208:
        x, W = case["x"], R.make_w(512, case["K"], R.SWIGLU_GAIN)
        href = R.swiglu_ref(x, W)
        h = href.to(torch.bfloat16)
        assert R.check_swiglu(h, href)["ok"]
        bad = h.clone(); bad[3, 8:16] = h[3, 0:8]
        assert not R.check_swiglu(bad, href)["ok"]
        bad = h.clone(); bad[46, 255] = float("nan")
        assert R.check_swiglu(bad, href)["worst"] == float("inf")
        assert R.agree(ref.float(), ref.float(), ref) == 0.0 and R.agree(ref.float(), dup, ref) > 1.0


@pytest.mark.parametrize("kind", R.MUTATIONS)
def test_slab_comparator_rejects_each_planted_error(case, kind):
    """On the rounded reference standing in for a kernel result: each mutant is outside the bound by a wide margin."""
    S = 2
    ref = R.slab_refs(case["x"], case["W"], S)
    res = R.check_slabs(ref.float(), R.mutate(ref, kind, case["x"], case["W"]))
    assert not res["ok"] and res["worst"] > 10.0, (kind, res)
    if kind == "slabs_exchanged":                                               # only the per-slab check can see it
        assert res["where"]["part"] == "slab 0"
        torch.testing.assert_close(R.mutate(ref, kind, case["x"], case["W"]).sum(0), ref.sum(0), rtol=0, atol=1e-12 * float(ref.abs().max()))
    if kind == "chunk_dropped":
        assert res["where"]["rows"] == [12, 13, 14, 15] and res["where"]["part"] == f"slab {S - 1}"
