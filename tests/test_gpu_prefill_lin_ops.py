"""GPU: operator tests of the 256 x 256 GEMM's plain-operand epilogues (gemm256.hip on tile256.h, GemmA::kind == 0, the runtime epilogue of gemm_common.h) at
LLM prefill shapes, through pg_diag_op_gemm_epi (tests/vq_ops.py run_gemm_epi: form 2 = gemm256_try, form 1 = the 128 x 128 kernel), against the float64
reference and the derived bound of tests/prefill_lin_ref.py (cases, mutants and the reference's own margin are checked on the CPU by
tests/test_prefill_lin_ref_cpu.py).  The float64 products are taken on the device with torch (one per operand set, shared by its cases).

Every case: NaN pre-fill, guard bands and row gaps (ldc > N) intact; PG_OK from form 2 -- a shape gemm256_try sends back is an error here, never a silent
pass on the other kernel -- at every tile height and phase count (pg_tune->gemm256 = 1 auto, 4 / 5 / 6 = 256 / 224 / 192 rows, + 8 = four phases per K tile:
pg_diag_op_gemm_epi256); max |err| / bound <= 1 for both kernels, printed per case before it is asserted.

Bit identity between the two kernels is asserted for EVERY epilogue, not only the bare one: both accumulate K in the same order (the existing bare-epilogue
tests rely on that), and both run the same Epi arithmetic on the accumulator -- v scale, + bias_n, + bias_m, + residual, GELU, in that order, one element at a
time (store1_batch) or four (store4_batch).  The one freedom the compiler has is contracting v scale + bias into an fma in one kernel and not the other;
every scale used here is a power of two, whose product is exact, so the fma and the separate product round alike."""
import pytest
import torch

import prefill_lin_ref as P

pytestmark = pytest.mark.gpu

_CORE = {}


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cases():
    """The case list needs the device's CU count (the wrap case); collection must work without a device."""
    try:
        ncu = _ncu() if torch.cuda.is_available() else P.NOMINAL_CUS
    except Exception:
        ncu = P.NOMINAL_CUS
    return P.cases256(ncu)


CASES = _cases()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _group(group):
    """Operands, bias and residual of a group on the device and its float64 products; one group resident at a time."""
    if _CORE.get("group") != group:
        _CORE.clear()
        torch.cuda.empty_cache()
        rows = P.group_rows(group, _ncu())
        a, w, bn, bm, res = P.inputs(group, rows)
        T = torch.float32 if P.GROUPS[group][2] else torch.bfloat16
        _CORE.update(group=group, rows=rows, a=a.cuda().to(T), w=w.cuda().to(T), bn=bn.cuda(), bm=bm.cuda(), res=res.cuda(), core=P.core(group, rows, "cuda"))
    return _CORE


def _operands(c, g):
    """Keyword arguments of run_gemm_epi for case c: row / column prefixes of the group's device tensors."""
    M, N, K = c["M"], c["N"], c["K"]
    kw = dict(bias_n=g["bn"][:N] if c["bias_n"] else None, bias_m=g["bm"][:M] if c["bias_m"] else None, scale=c["scale"], act=c["act"], ldr=c["ldr"],
              inplace=c["inplace"], engine=c["engine"], dev_out=True)
    if c["res"] is not None:
        kw["res_kind"] = c["res"]
        if c["inplace"] or not c["ldr"] or c["ldr"] == N:
            kw["residual"] = g["res"][:M, :N].contiguous()
        else:
            if g.get("resbuf_id") != c["id"]:
                g.update(resbuf_id=c["id"], resbuf=P.residual_buffer(c, g["rows"]).cuda())          # its own layout, NaN between the rows
            kw["residual"] = g["resbuf"]
    return (g["a"][:M], g["w"][:N], c["out"], M, N, K, 1, K, 0, K, 0, c["ldc"], 0), kw


def _run(c, g, form, opt=None, **over):
    from vq_ops import run_gemm_epi
    args, kw = _operands(c, g)
    kw.update(over)
    return run_gemm_epi(*args, form=form, opt=opt, **kw)


def _ref_bound(c, g):
    ref, mag = P.lin_ref(c, g["core"], g["rows"])
    return ref, P.lin_bound(c, ref, mag)


# ------------------------------------------------------------------------------------------------------------------------------ the 256 tile
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["id"] for c in CASES])
def test_gemm256_plain_epilogues(i):
    c = CASES[i]
    g = _group(c["group"])
    ncu = _ncu()
    ref, bound = _ref_bound(c, g)
    o1 = _run(c, g, 1)
    assert o1["guards"] and o1["gaps"] and o1["nsplit"] == 0, "128 x 128 kernel: a guard band or a row gap was written"
    r1 = P.ratio(o1["out"][0], ref, bound)
    ratios = {}
    for opt in P.OPTS256:
        o2 = _run(c, g, 2, None if opt == 1 else opt)                          # expect = PG_OK: a shape sent back to the 128 x 128 kernel fails here
        assert o2["rc"] == 0 and o2["guards"] and o2["gaps"], f"gemm256 = {opt}: a guard band or a row gap was written"
        ratios[opt] = P.ratio(o2["out"][0], ref, bound)
        same = torch.equal(_bits(o2["out"]), _bits(o1["out"]))
        if not same:
            d = (_bits(o2["out"][0]) != _bits(o1["out"][0])).nonzero()
            print(f"{c['id']} gemm256 = {opt}: {d.shape[0]} elements differ from the 128 x 128 kernel, first at {d[0].tolist()}, err / bound {ratios[opt]:.3g}")
        assert same, (c["id"], opt)
        if c["inplace"] and opt == 1:                                          # the same launch again from identical inputs: equal bits
            again = _run(c, g, 2)
            assert torch.equal(_bits(again["out"]), _bits(o2["out"])), "the in-place launch is not repeatable"
    h = P.auto_height(c["M"], c["N"], ncu)
    print(f"{c['id']} ({c['why']}; {P.tiles(c['M'], c['N'], 256)} tiles of 256 rows on {ncu} CUs, auto height {h}): max |err| / bound = "
          f"{max(ratios.values()):.3g} (256 tile, all {len(ratios)} modes), {r1:.3g} (128 tile)")
    assert r1 <= 1.0 and max(ratios.values()) <= 1.0, (r1, ratios)


def test_wrap_case_runs_a_second_round_on_this_device():
    ncu = _ncu()
    wm = P.wrap_m(ncu)
    assert any(c["M"] == wm for c in CASES), "the case list was built for another CU count"
    over = P.tiles(wm, 2048, 256) - ncu
    assert (0 < over <= 8) or ncu < 200, (wm, ncu, over)
    assert all(P.tiles(wm, 2048, h) > ncu for h in P.HEIGHT.values())


def test_real_kernel_result_against_mutated_references_is_rejected():
    """A REAL result of the 256 tile: accepted against the reference, rejected against each mutant reference (a kernel with that bug differs from the true
    reference by what the mutant differs from it).  clip16 and wrap_skip at the height the launch ran."""
    ncu = _ncu()
    g = _group("k128")
    for mutant, epi in P.MUTANTS.items():
        M = P.wrap_m(ncu) if mutant == "wrap_skip" else 6273
        c = P.make_case("k128", M, 2048, epi)
        ref, bound = _ref_bound(c, g)
        for opt, h in P.HEIGHT.items() if mutant == "wrap_skip" else [(4, 256)]:
            got = _run(c, g, 2, opt)["out"][0]
            assert P.ratio(got, ref, bound) <= 1.0
            bad, _ = P.lin_ref(c, g["core"], g["rows"], mutant, height=h, G=ncu)
            r = P.ratio(got, bad, bound)
            print(f"{mutant} (height {h}): real result against the mutant reference: max |err| / bound = {r:.3g}")
            assert r > 1.0, (mutant, h, r)


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_alone_and_the_entry_point_usable():
    from vq_ops import PG_ERR_ARG, run_gemm_epi
    g = _group("k128")
    c = P.make_case("k128", 6273, 2048, "res_sep")
    args, kw = _operands(c, g)

    def refused(what, a=args, form=2, opt=None, **over):
        k = dict(kw)
        k.update(over)
        o = run_gemm_epi(*a, form=form, opt=opt, expect=PG_ERR_ARG, **k)
        assert o["untouched"] and o["guards"], what

    def with_(**ch):
        names = ("A", "W", "out_kind", "M", "N", "K", "batch", "lda", "strideA", "ldb", "strideB", "ldc", "strideC")
        d = dict(zip(names, args))
        d.update(ch)
        return tuple(d[n] for n in names)

    M, N, K = c["M"], c["N"], c["K"]
    a_flat, w_flat = g["a"].reshape(-1), g["w"].reshape(-1)
    for form in (2, 1):
        refused("K % 64", with_(A=g["a"][:M, :96].contiguous(), W=g["w"][:N, :96].contiguous(), K=96, lda=96, ldb=96), form)
        refused("misaligned A", with_(A=a_flat[1:1 + M * K]), form)
        refused("misaligned W", with_(W=w_flat[1:1 + N * K]), form)
        refused("misaligned bias_n", form=form, bias_n=torch.zeros(N + 4, device="cuda")[1:N + 1])
        refused("misaligned residual", form=form, residual=torch.zeros(M * c["ldr"] + 4, device="cuda")[1:])
        refused("overlapping batches", with_(batch=2, strideC=(M - 1) * c["ldc"] + N - 1), form, residual=None, ldr=0)
    refused("form 2 on the fp32 engine", with_(A=g["a"].float(), W=g["w"].float()), engine="f32")
    # what the admission rule sends back: one tile row short of 200 tiles, a single K tile, and an option that names no instantiation
    refused("192 tiles", with_(A=g["a"][:6144], M=6144), residual=None, ldr=0)
    refused("K = 64", with_(A=g["a"][:M, :64].contiguous(), W=g["w"][:N, :64].contiguous(), K=64, lda=64, ldb=64))
    for opt in (0, 2, 3, 7, 8, 9, 15, 16):
        refused(f"gemm256 = {opt}", opt=opt)
    ref, bound = _ref_bound(c, g)
    for form in (2, 1):
        o = run_gemm_epi(*args, form=form, **kw)
        assert o["guards"] and o["gaps"] and P.ratio(o["out"][0], ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------ the fp32 engine
@pytest.mark.parametrize("M", P.F32_M)
def test_gemm_f32_kernel_epilogues(M):
    """gemm_f32_kernel (form 0, fp32 engine) through the same epilogue matrix: N = 200, K = 72 (ragged 64 x 64 tiles, a K tail of 8)."""
    from vq_ops import PG_ERR_ARG
    g = _group("f32")
    worst = {}
    for c in (c for c in P.cases_f32() if c["M"] == M):
        ref, bound = _ref_bound(c, g)
        o = _run(c, g, 0)
        assert o["guards"] and o["gaps"], c["id"]
        worst[c["epi"]] = P.ratio(o["out"][0], ref, bound)
        if c["inplace"]:
            assert torch.equal(_bits(_run(c, g, 0)["out"]), _bits(o["out"])), "the in-place launch is not repeatable"
    print(f"gemm_f32_kernel M={M} N=200 K=72: max |err| / bound = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    # the fp32 engine stores fp32 and reads an fp32 residual: the two bf16 forms of the matrix are refused
    c = P.make_case("f32", M, 200, "bias_n")
    o = _run(dict(c, out="bf16"), g, 0, expect=PG_ERR_ARG)
    assert o["untouched"] and o["guards"]
    c = P.make_case("f32", M, 200, "res_sep")
    o = _run(c, g, 0, expect=PG_ERR_ARG, res_kind="bf16")
    assert o["untouched"] and o["guards"]
