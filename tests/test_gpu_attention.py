"""GPU: operator tests of the attention kernels against the fp64 references of tests/attn_ref.py, through the diagnostics library's operator
entry points (plangen_amd/csrc/diag_ops.hip), which run the production launchers with one kernel form pinned.

Bounds (derivations in tests/attn_ref.py; never fitted to a GPU run), per output element, u = 2^-8 (bf16) / 2^-24 (f32):
  decode, fused and unfused, f32 and bf16:  u |ref| + RoPE evaluation-order spread + 2^-12 max|v|
  prefill attn_kernel mode 1:               u |ref| + 2^-12 max|v|
  prefill flash / flash2 (bf16):            u |ref| + u sum_i pi_i |v_i| (bf16 P) + |ref(bf16(q scale)) - ref(q scale)| + 2^-12 max|v|
  SigLIP tile / resident (bf16):            u |ref| + u sum_i pi_i |v_i| + 2^-12 max|v|
Every slot a kernel must not read holds a finite key whose score dominates and a distinctive V (attn_ref.POISON_*); the needle families put
one dominant key per (row, head) or per query where a wrong key index would move the output by a large fraction of |v|."""
import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu


def _report(tag, ok, mx, worst):
    print(f"{tag}: max |err| / bound = {mx:.3g} (worst flat index {worst})")
    assert ok, f"{tag}: error {mx:.3g} x the bound at flat index {worst}"


# ------------------------------------------------------------------------------------------------------------------------------ decode
def _check_decode(d, ref, tag, out, kc, vc):
    dtype = d["dtype"]
    _report(tag, *A.check(out.view(d["M"], d["nh"], 128), ref["out"], A.decode_bound(ref, dtype)))
    # the append: K within one unit in the last place of the reference RoPE, V bit-exact; nothing else in either cache changed
    r0, nh = d["r0"], d["nh"]
    kc_exp, vc_exp = d["kc"].clone(), d["vc"].clone()
    T = A.TORCH_T[dtype]
    for r in range(d["M"]):
        slot = d["len"][r] + d["n_dec"]
        got_k = kc[r0 + r, :, slot]
        ulps = A.ulp_distance(got_k, ref["k_new"][r].to(T))
        assert int(ulps.max()) <= 1, f"{tag}: appended K of row {r} off by {int(ulps.max())} ulp"
        assert torch.equal(vc[r0 + r, :, slot], ref["v_new"][r].to(T)), f"{tag}: appended V of row {r}"
        kc_exp[r0 + r, :, slot] = got_k
        vc_exp[r0 + r, :, slot] = ref["v_new"][r].to(T)
    assert torch.equal(kc, kc_exp), f"{tag}: K cache changed outside the append slots"
    assert torch.equal(vc, vc_exp), f"{tag}: V cache changed outside the append slots"


def _run_decode(d, forms=(0, 4, 8), unfused=True):
    from attn_ops import DecodeDev
    ref = A.decode_ref(d, d["dtype"])
    dev = DecodeDev(d)
    for form in forms:
        out, kc, vc = dev.run(form, 0)
        _check_decode(d, ref, f"fused form {form}", out, kc, vc)
    if unfused and d["shared_len"] == 0 and d["r0"] == 0:
        out, kc, vc = dev.run(0, 1)
        _check_decode(d, ref, "rope_kv + attn_kernel", out, kc, vc)


DECODE_S_ORDER = [(1, "none"), (2, "lpt"), (4, "perm"), (5, "none"), (8, "lpt")]


@pytest.mark.parametrize("needle", [False, True], ids=["random", "needle"])
@pytest.mark.parametrize("S,order", DECODE_S_ORDER)
@pytest.mark.parametrize("nh", [2, 16])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_ragged_key_counts(dtype, nh, S, order, needle):
    """One launch whose rows carry 0, 1, KPI +- 1, KPW +- 1, chunk +- 1 (both forms), 2 chunk + 1, 831 and 863 cached keys; the production
    choice, the big (4-wave) and the small (8-wave) form on the same inputs, and the unfused rope_kv + attn_kernel pair."""
    _run_decode(A.decode_counts_case(dtype, nh, S, order=order, needle=needle))


def _shared_params():
    out = []
    for dtype in ("f32", "bf16"):
        for gform in (4, 8):
            kpi, kpw, ch = A.decode_geometry(dtype, gform)
            pairs = [(1, 0), (kpi + 1, 1), (kpw, kpw - 1), (ch, ch + 1), (ch + 1, 575), (288, 575), (288, 0)]
            for i, (sl, nd) in enumerate(pairs):
                out.append(pytest.param(dtype, sl, nd, 4 if i % 2 else 0, id=f"{dtype}-g{gform}-shared{sl}-ndec{nd}-r0_{4 if i % 2 else 0}"))
    return out


@pytest.mark.parametrize("needle", [False, True], ids=["random", "needle"])
@pytest.mark.parametrize("dtype,shared_len,n_dec,r0", _shared_params())
def test_decode_shared_uncond_prompt(dtype, shared_len, n_dec, r0, needle):
    """Odd rows read [0, shared_len) from row 1 and a private tail of n_dec keys; r0 = 4: the second lane of the two-lane decode (caches,
    len and pos_off rebased, shared_row = 1 - r0 = -3)."""
    nh = 16 if (shared_len + n_dec) % 2 else 2
    S = [1, 2, 4, 5, 8][(shared_len + n_dec) % 5]
    _run_decode(A.decode_shared_case(dtype, nh, shared_len, n_dec, S, r0=r0, needle=needle, order="lpt" if r0 == 0 else "perm"))


# ------------------------------------------------------------------------------------------------------------------------------ prefill
@pytest.mark.parametrize("needle", [False, True], ids=["random", "causal_needle"])
@pytest.mark.parametrize("nh", [2, 16])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_prefill_packed_rows(dtype, nh, needle):
    """Rows of 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 288 tokens and one aliased row (row_off -1) in one packed launch; bf16:
    flash2, flash and attn_kernel mode 1; f32: attn_kernel mode 1.  obuf rows past the packed tokens and both caches stay untouched."""
    from attn_ops import run_prefill
    p = A.make_prefill_case(300 + nh + 2 * needle + (dtype == "bf16"), dtype, nh, needle=needle)
    flash_ref = A.prefill_ref(p, dtype, flash=dtype == "bf16")
    paths = [2, 1, 0] if dtype == "bf16" else [0]
    for path in paths:
        flash = path > 0
        out, tail, fill, kc, vc = run_prefill(p, path)
        _report(f"prefill path {path}", *A.check(out, flash_ref["out"], A.prefill_bound(flash_ref, dtype, flash)))
        assert torch.equal(tail, fill), f"path {path}: obuf rows of no packed token were written"
        assert torch.equal(kc, p["kc"]) and torch.equal(vc, p["vc"]), f"path {path}: the caches changed"
    if dtype == "bf16":
        b = A.prefill_bound(flash_ref, dtype, True)
        if not needle:
            assert float(b.max()) <= 0.01 * float(flash_ref["out"].abs().max())          # >= 5x tighter than 5 % of the maximum


# ------------------------------------------------------------------------------------------------------------------------------ SigLIP
@pytest.mark.parametrize("needle", [False, True], ids=["random", "needle"])
@pytest.mark.parametrize("C,NH", [(128, 2), (1024, 16)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [64, 192, 576, 640])
def test_vit_attention_forms(P, B, C, NH, needle):
    """The 64-key tile kernel (form 1) and the LDS-resident kernel with 4 / 8 / 12 / 16 waves; at P = 640 K / V^T of a head exceed the
    LDS budget and the launcher falls back to the tile kernel for every form."""
    from attn_ops import run_vit
    v = A.make_vit_case(500 + P + B + NH + needle, B, P, C, NH, needle=needle)
    ref = A.vit_ref(v["qk"], v["vt"], B, P, C, NH, v["scale"])
    bound = A.vit_bound(ref)
    for form in (1, 4, 8, 12, 16):
        _report(f"vit form {form}", *A.check(run_vit(v, form), ref["out"], bound))


# ------------------------------------------------------------------------------------------------------------------------------ arguments
def test_entry_points_refuse_unsupported_shapes():
    """PG_ERR_ARG, nothing launched: an append slot past the cache, a bad form, P % 64 != 0, heads that are not 64 wide."""
    from attn_ops import DecodeDev, lib, _ptr, _stream
    d = A.make_decode_case(1, "f32", 2, [5, 9], S=1)
    dev = DecodeDev(d)
    L = lib()
    args = lambda form, slots: (0, form, 0, _ptr(dev.qkv), 1, 2 * 3 * 256, _ptr(dev.obuf), _ptr(dev.kc), _ptr(dev.vc), _ptr(dev.cos),
                                _ptr(dev.sin), _ptr(dev.len), _ptr(dev.pos_off), _ptr(dev.n_dec), None, 0, 1, 2, 2, slots, d["max_pos"],
                                d["scale"], None, _stream())
    kc0 = dev.kc.clone()
    assert L.pg_diag_op_attn_decode(*args(0, 9)) == -1            # row 1 appends at slot 9 of 9
    assert L.pg_diag_op_attn_decode(*args(6, d["slots"])) == -1
    torch.cuda.synchronize()
    assert torch.equal(dev.kc, kc0)
    x = torch.zeros(4, dtype=torch.bfloat16, device="cuda")
    assert L.pg_diag_op_attn_vit(1, _ptr(x), _ptr(x), _ptr(x), 1, 96, 128, 2, 0.125, _stream()) == -1
    assert L.pg_diag_op_attn_vit(1, _ptr(x), _ptr(x), _ptr(x), 1, 128, 256, 2, 0.125, _stream()) == -1
    assert L.pg_diag_op_attn_vit(2, _ptr(x), _ptr(x), _ptr(x), 1, 128, 128, 2, 0.125, _stream()) == -1
