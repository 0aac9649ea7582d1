"""CPU: the offset-causal attention reference of tests/extend_ref.py -- against a query-by-query evaluation, against attn_ref.prefill_ref
where the two must coincide (q0 = 0), and the mutants the checker has to reject before it is trusted with a kernel."""
import pytest
import torch

import attn_ref as A
import extend_ref as E

ROWS = [(0, 3), (1, 2), (5, 4), (63, 3), (64, 2), (65, 5), (0, 1)]


@pytest.mark.parametrize("needle", [False, True], ids=["random", "causal_needle"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_reference_matches_a_query_by_query_evaluation(dtype, needle):
    p = E.make_extend_case(11 + needle, dtype, 2, rows=ROWS, aliased_row=2, needle=needle)
    ref = E.extend_ref(p, dtype, flash=False)
    scale = torch.tensor(p["scale"], dtype=torch.float32).item()
    for r, (off, a, b) in enumerate(zip(p["row_off"], p["q0"], p["n_new"])):
        if off < 0:
            continue
        for i in range(b):
            assert p["tok_row"][off + i] == r and p["tok_j"][off + i] == a + i
            for h in range(p["nh"]):
                qv = A.f32(p["q"][off + i, h].to(A.F64) * scale)
                K = p["kc"][r, h, :a + i + 1].to(A.F64)
                V = p["vc"][r, h, :a + i + 1].to(A.F64)
                o = torch.softmax(K @ qv, dim=0) @ V
                assert torch.allclose(o, ref["out"][off + i, h], rtol=1e-12, atol=1e-12), (r, i, h)
    # rows without packed tokens contribute nothing, and the poison sits exactly behind each row's last new token
    assert ref["out"].shape[0] == p["Ntok"] == sum(b for r, (_, b) in enumerate(zip(p["q0"], p["n_new"])) if p["row_off"][r] >= 0)
    for r, L in enumerate(p["len"]):
        lo = 0 if p["row_off"][r] < 0 else L
        assert bool((p["vc"][r, :, lo:, 0].float() == A.POISON_V).all())


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_q0_zero_rows_are_a_prefill(dtype):
    """With q0 = 0 the extension is the causal prefill of the same tokens: the two references must agree to the last bit."""
    p = E.make_extend_case(5, dtype, 2, rows=ROWS, aliased_row=2)
    ext = E.extend_ref(p, dtype, flash=dtype == "bf16")
    pre = A.prefill_ref(E.as_prefill_case(p), dtype, flash=dtype == "bf16")
    n = 0
    for off, a, b in zip(p["row_off"], p["q0"], p["n_new"]):
        if off >= 0 and a == 0:
            n += 1
            for k in ("out", "pv_abs", "qterm"):
                assert torch.equal(ext[k][off:off + b], pre[k][off:off + b]), k
    assert n == 2


@pytest.mark.parametrize("needle", [False, True], ids=["random", "causal_needle"])
@pytest.mark.parametrize("dtype,flash", [("bf16", True), ("bf16", False), ("f32", False)], ids=["bf16-flash", "bf16-mode1", "f32-mode1"])
def test_checker_accepts_the_rounded_reference_and_rejects_every_mutant(dtype, flash, needle):
    p =E.make_extend_case(23 + needle, dtype, 2, rows=ROWS, aliased_row=2, needle=needle)
    ref = E.extend_ref(p, dtype, flash)
    bound = A.prefill_bound(ref, dtype, flash)
    ok, mx, _ = A.check(ref["out"].to(A.TORCH_T[dtype]), ref["out"], bound)
    assert ok, mx
    for mut in E.MUTANTS:
        got = E.extend_ref(p, dtype, flash, mut=mut)["out"].to(A.TORCH_T[dtype])
        ok, mx, worst = A.check(got, ref["out"], bound)
        print(f"{dtype} flash={flash} needle={needle} mutant {mut}: max |err| / bound = {mx:.3g}")
        assert not ok and mx > 10.0, f"mutant {mut} passes the checker ({mx:.3g} x the bound)"


def test_covering_subset_covers_both_axes():
    assert {a for a, _ in E.Q0_NNEW} == {0, 1, 63, 64, 65, 127, 128, 200, 831}
    assert {b for _, b in E.Q0_NNEW} == {1, 2, 31, 32, 33, 64, 127, 128, 129, 300}
