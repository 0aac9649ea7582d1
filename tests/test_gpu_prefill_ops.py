"""GPU: operator tests of the prefill side of the LLM -- the 256 x 256 GEMM's two prefill epilogues (act 3: RoPE(q), RoPE(k) and the K/V cache write
from the accumulators, on the [8 | 8]-interleaved Wqkv; act 2: SwiGLU over [8 gate | 8 up] column blocks), rope_kv_kernel alone in both modes, and the
two weight interleavers -- against the fp64 references of tests/prefill_ref.py, through the diagnostics library's operator entry points
(plangen_amd/csrc/diag_ops.hip), which run the production launchers.

Shapes: the smallest gemm256_try takes (>= 200 tiles of 256 x 256, <= 25 % padding; tests/test_prefill_ref_cpu.py asserts the tile arithmetic), every
tile height (gemm256 = 4 / 5 / 6: 256 / 224 / 192 rows, 1: the automatic choice) in the two-phase and the four-phase schedule (+ 8).  Every M leaves a
partial last m-tile at all three heights; M = 16897 and 2305 leave a single row in the last 256-row tile.

Asserted for every launch (bounds derived in tests/prefill_ref.py, never fitted to a GPU run):
  (a) the fused epilogue is BIT-IDENTICAL to the unfused path (GEMM -> fp32 -> rope_kv_kernel / silu_mul_kernel; include/plangen_hip.h promises it);
  (b) both are within the derived bound of the fp64 reference on every element the token map owns;
  (c) every qbuf row and cache slot no token owns (over-capacity tokens, the row without tokens, slots past a row's length) and every guard row still
      holds the sentinel bit pattern, and every owned element was written.
The figures printed per launch (max |err| / bound) are for the reader; no tolerance is tuned from them."""
import pytest
import torch

import prefill_ref as P

pytestmark = pytest.mark.gpu

_CTX = {}


def _same_bits(a, b):
    return torch.equal(P.bits(a), P.bits(b))


def _ctx(kind, i, build):
    """One case at a time stays resident: its inputs, its reference (computed once per case) and the unfused results, on the device."""
    if _CTX.get("key") != (kind, i):
        _CTX.clear()
        torch.cuda.empty_cache()
        _CTX.update(build(), key=(kind, i))
    return _CTX


def _fmt(r):
    return " ".join(f"{k}={v:.3f}" for k, v in r.items())


# ------------------------------------------------------------------------------------------------------------------------------ QKV + RoPE + KV write
def _build_qkv(i):
    from prefill_ops import QkvDev
    nh, M, K = P.QKV_CASES[i]
    case = P.make_qkv_case(100 + i, nh, M, K)
    ref = P.qkv_rope_ref(case)
    dev = QkvDev(case, ref)
    # the unfused path twice: on the 128 x 128 GEMM (gemm256 = 0, a kernel that shares nothing with the fused one but the loaders) and as the engine
    # runs it (gemm256 = 1: the 256 x 256 kernel's plain epilogue)
    un0, un1 = dev.run(1, 0), dev.run(1, 1)
    return {"case": case, "ref": ref, "dev": dev, "un0": un0, "un1": un1}


@pytest.mark.parametrize("opt", P.OPTS256)
@pytest.mark.parametrize("i", range(len(P.QKV_CASES)), ids=lambda i: "nh%d-M%d-K%d" % P.QKV_CASES[i])
def test_qkv_rope_epilogue_equals_the_unfused_path_and_the_reference(i, opt):
    c = _ctx("qkv", i, lambda: _build_qkv(i))
    ref, tag = c["ref"], "qkv_rope nh=%d M=%d K=%d" % P.QKV_CASES[i]
    if "un_checked" not in c:
        r0, r1 = P.check_rope(*c["un0"], ref), P.check_rope(*c["un1"], ref)
        print(f"{tag} form 1 (gemm256 = 0): err / bound {_fmt(r0['ratio'])}; form 1 (gemm256 = 1): {_fmt(r1['ratio'])}")
        assert all(_same_bits(a, b) for a, b in zip(c["un0"], c["un1"])), "the unfused path differs between the 128 x 128 and the 256 x 256 GEMM"
        assert r0["sentinel"] and r1["sentinel"], "unfused path: a slot no token owns (or a guard row) was written, or an owned one was not"
        assert r0["ok"] and r1["ok"], (r0, r1)
        c["un_checked"] = True
    got = c["dev"].run(0, opt)
    res = P.check_rope(*got, ref)
    print(f"{tag} form 0 gemm256 = {opt}: err / bound {_fmt(res['ratio'])}")
    assert res["sentinel"], "a slot no token owns (or a guard row) was written, or an owned one was not"
    for name, a, b in zip("qkv", got, c["un0"]):
        assert _same_bits(a, b), (name, float((P.bits(a) != P.bits(b)).float().mean()))
    assert res["ok"], res


# ------------------------------------------------------------------------------------------------------------------------------ rope_kv_kernel alone
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("nh", [2, 5, 16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rope_kv_kernel_alone(dtype, mode, nh, S):
    """Decode map and prefill token map, slab sums, nh % 4 != 0 (the head >= nh return), rows that own nothing, over-capacity tokens, the clamp."""
    from prefill_ops import run_rope_kv
    case = P.make_rope_case(1000 + 10 * nh + S + 100 * mode, mode, nh, S, 300)
    ref = P.rope_kv_ref(case, dtype)
    res = P.check_rope(*[t.cpu() for t in run_rope_kv(case, ref, dtype)], ref)
    print(f"rope_kv {dtype} mode={mode} nh={nh} S={S}: err / bound {_fmt(res['ratio'])}")
    assert res["sentinel"], "a slot no token owns (or a guard row) was written, or an owned one was not"
    assert res["ok"], res


# ------------------------------------------------------------------------------------------------------------------------------ SwiGLU epilogue
def _build_swiglu(i):
    from prefill_ops import SwigluDev
    M, I, K = P.SWIGLU_CASES[i]
    case = P.make_swiglu_case(200 + i, M, I, K)
    ref = P.swiglu256_ref(case)
    ref = {k: v.cuda() for k, v in ref.items()}
    dev = SwigluDev(case)
    return {"case": case, "ref": ref, "dev": dev, "un0": dev.run(1, 0), "un1": dev.run(1, 1)}


@pytest.mark.parametrize("opt", P.OPTS256)
@pytest.mark.parametrize("i", range(len(P.SWIGLU_CASES)), ids=lambda i: "M%d-I%d-K%d" % P.SWIGLU_CASES[i])
def test_swiglu_epilogue_equals_the_unfused_path_and_the_reference(i, opt):
    """(g / (1 + expf(-g))) * u from bit-identical accumulators in both forms.  I = 360: N = 720 ends inside the last n-tile."""
    c = _ctx("swiglu", i, lambda: _build_swiglu(i))
    ref, tag = c["ref"], "swiglu256 M=%d I=%d K=%d" % P.SWIGLU_CASES[i]
    if "un_checked" not in c:
        (m0, g0), (m1, g1) = P.check_swiglu(c["un0"], ref), P.check_swiglu(c["un1"], ref)
        print(f"{tag} form 1 (gemm256 = 0): err / bound {m0:.3f}; form 1 (gemm256 = 1): {m1:.3f}")
        assert _same_bits(c["un0"], c["un1"]), "the unfused path differs between the 128 x 128 and the 256 x 256 GEMM"
        assert g0 and g1 and m0 <= 1.0 and m1 <= 1.0, (m0, g0, m1, g1)
        c["un_checked"] = True
    h = c["dev"].run(0, opt)
    mx, guard = P.check_swiglu(h, ref)
    print(f"{tag} form 0 gemm256 = {opt}: err / bound {mx:.3f}")
    assert guard, "rows behind row M - 1 of h were written"
    assert _same_bits(h, c["un0"]), float((P.bits(h) != P.bits(c["un0"])).float().mean())
    assert mx <= 1.0, mx


# ------------------------------------------------------------------------------------------------------------------------------ interleavers
@pytest.mark.parametrize("K", [64, 2048])
@pytest.mark.parametrize("nh", [1, 2, 16])
def test_interleave_qk_is_the_index_permutation(nh, K):
    from prefill_ops import run_interleave_qk
    W = torch.randn(3 * nh * 128, K, generator=torch.Generator().manual_seed(nh + K)).to(torch.bfloat16)
    got, guard = run_interleave_qk(W, nh)
    assert _same_bits(got, P.interleave_qk_ref(W, nh)) and guard


@pytest.mark.parametrize("I,H", [(8, 64), (360, 128), (5632, 2048)])
def test_convert_interleave16_is_the_index_permutation(I, H):
    from prefill_ops import run_interleave16
    g = torch.Generator().manual_seed(I + H)
    wg, wu = torch.randn(I, H, generator=g).to(torch.bfloat16), (3 + torch.randn(I, H, generator=g)).to(torch.bfloat16)
    got, guard = run_interleave16(wg, wu)
    assert _same_bits(got, P.interleave16_ref(wg, wu)) and guard


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_what_the_kernels_cannot_do_and_stay_usable():
    from prefill_ops import PG_ERR_ARG, PG_OK, QkvDev, SwigluDev, _i32, _ptr, _stream, lib, rope_kv_call, untouched
    nh, M, K = 2, 17000, 128
    case = P.make_qkv_case(300, nh, M, K)
    tm = case["tm"]
    ref = {"M": M, "R": tm["R"], "slots": tm["slots"], "nh": nh}              # the buffers' geometry is all the refusals need
    dev = QkvDev(case, ref)
    bufs = P.rope_buffers(ref, "bf16", "cuda")
    bad_row = _i32([tm["R"]] + tm["tok_row"][1:], "cuda")
    last = tm["tok_row"].index(tm["R"] - 1)
    over_last = list(tm["tok_j"])
    over_last[last] = tm["slots"]
    twice = list(tm["tok_j"])
    twice[tm["over"][0]] = 2 * tm["slots"]
    calls = {
        "gemm256_try declines M = 1000": dict(form=0, M=1000),
        "K = 96": dict(form=0, K=96), "K = 96, unfused": dict(form=1, K=96),
        "tok_row out of range": dict(form=0, tok_row=bad_row), "tok_row out of range, unfused": dict(form=1, tok_row=bad_row),
        "over capacity in the last row": dict(form=0, tok_j=_i32(over_last, "cuda")), "over capacity in the last row, unfused": dict(form=1, tok_j=_i32(over_last, "cuda")),
        "over capacity past the caches": dict(form=1, tok_j=_i32(twice, "cuda")),
        "misaligned qbuf": dict(form=0, qbuf_off=8), "misaligned qbuf, unfused": dict(form=1, qbuf_off=8),
    }
    for what, kw in calls.items():
        form = kw.pop("form")
        assert dev.call(form, 1, bufs, **kw) == PG_ERR_ARG and untouched(*bufs), what
    for opt in (0, 2, 3, 7, 8, 9, 15, 16):
        assert dev.call(0, opt, bufs) == PG_ERR_ARG and untouched(*bufs), opt
    # rope_kv alone
    rcase = P.make_rope_case(301, 1, 5, 3, 300)
    rref = P.rope_kv_ref(rcase, "bf16")
    def row_out(m): m.tok_row[7] = rcase["tm"]["R"]
    def neg_slot(m): m.tok_j[7] = -1
    def pos_out(m): m.pos_off[1] = rcase["tm"]["max_pos"]
    def over_in_last(m): m.tok_j[rcase["tm"]["tok_row"].index(rcase["tm"]["R"] - 1)] = rcase["tm"]["slots"]
    for edit in (row_out, neg_slot, pos_out, over_in_last):
        rc, rb = rope_kv_call(rcase, rref, "bf16", edit=edit)
        assert rc == PG_ERR_ARG and untouched(*rb), edit.__name__
    for over in (dict(S=0), dict(slab=300 * 3 * 5 * 128 - 1), dict(qbuf_off=4), dict(M=0)):
        rc, rb = rope_kv_call(rcase, rref, "bf16", **over)
        assert rc == PG_ERR_ARG and untouched(*rb), over
    dcase = P.make_rope_case(302, 0, 2, 1, 300)
    def past_the_caches(m): m.len[299] = 2 * dcase["tm"]["slots"]
    rc, rb = rope_kv_call(dcase, P.rope_kv_ref(dcase, "f32"), "f32", edit=past_the_caches)
    assert rc == PG_ERR_ARG and untouched(*rb)
    # SwiGLU
    scase = P.make_swiglu_case(303, 17000, 360, 128)
    sdev = SwigluDev(scase)
    h = sdev.buffer()
    for what, kw in {"I % 8": dict(I=356), "I % 8, unfused": dict(form=1, I=356), "gemm256_try declines M = 1000": dict(M=1000), "K = 96": dict(K=96),
                     "K = 96, unfused": dict(form=1, K=96), "misaligned h": dict(h_off=8), "misaligned h, unfused": dict(form=1, h_off=8)}.items():
        assert sdev.call(kw.pop("form", 0), 1, h, **kw) == PG_ERR_ARG and untouched(h), what
    assert sdev.call(0, 2, h) == PG_ERR_ARG and untouched(h)
    # interleavers
    src = torch.zeros(3 * 128 * 64 + 64, dtype=torch.bfloat16, device="cuda")
    dst = P.sentinel_like((3 * 128 + 1, 64), "bf16", "cuda")
    L = lib()
    assert L.pg_diag_op_interleave(0, _ptr(src, 2), None, _ptr(dst), 1, 64, _stream()) == PG_ERR_ARG       # misaligned source
    assert L.pg_diag_op_interleave(0, _ptr(src), None, _ptr(dst), 1, 60, _stream()) == PG_ERR_ARG          # K % 8
    assert L.pg_diag_op_interleave(1, _ptr(src), None, _ptr(dst), 8, 64, _stream()) == PG_ERR_ARG          # no up source
    assert L.pg_diag_op_interleave(1, _ptr(src), _ptr(src), _ptr(dst), 12, 64, _stream()) == PG_ERR_ARG    # I % 8
    assert L.pg_diag_op_interleave(2, _ptr(src), _ptr(src), _ptr(dst), 8, 64, _stream()) == PG_ERR_ARG
    assert untouched(dst)
    # the handle-free calls stay usable after the refusals
    assert dev.call(0, 1, bufs) == PG_OK and dev.call(1, 1, P.rope_buffers(ref, "bf16", "cuda")) == PG_OK
    assert not untouched(bufs[0]) and sdev.call(0, 1, h) == PG_OK and not untouched(h)
    rc, rb = rope_kv_call(rcase, rref, "bf16")
    assert rc == PG_OK and P.check_rope(*[t.cpu() for t in rb], rref)["ok"]


# ------------------------------------------------------------------------------------------------------------------------------ checker sensitivity
def test_real_kernel_result_against_mutated_references_is_rejected():
    """The checker on a REAL result of the fused kernel: accepted against the reference, rejected against each mutated reference (a kernel with that
    bug would differ from the true reference by what the mutant differs from it)."""
    c = _ctx("qkv", 2, lambda: _build_qkv(2))
    case = c["case"]
    got = [t.cpu() for t in c["dev"].run(0, 1)]
    assert P.check_rope(*got, c["ref"])["ok"]
    proj = P.project(case["xn"], case["W"])
    for mut in [("pos", 1), ("sin_sign",), ("swap_lo_hi",), ("head_xor",), ("no_clamp",), ("cols_plain_on_interleaved",), ("ragged_meta",)]:
        res = P.check_rope(*got, P.qkv_rope_ref(case, mut, proj=proj))
        assert not res["ok"], (mut, res)
    sc = _ctx("swiglu", 1, lambda: _build_swiglu(1))
    h = sc["dev"].run(0, 1)
    assert P.check_swiglu(h, sc["ref"])[0] <= 1.0
    sproj = P.project(sc["case"]["xn"], sc["case"]["W"])
    for mut in [("swap",), ("col_off4",), ("silu_u",)]:
        bad = {k: v.cuda() for k, v in P.swiglu256_ref(sc["case"], mut, proj=sproj).items()}
        assert P.check_swiglu(h, bad)[0] > 1.0, mut
