"""CPU: the fp64 references of tests/prefill_ref.py (used by tests/test_gpu_prefill_ops.py) are pinned to the Llama rotary embedding, accept what a
correct kernel produces (their own bf16 rounding, a plain fp32 emulation of the kernels' arithmetic) and reject every mutant -- the bug a kernel could
have -- through the same checker the GPU tests use; the case generators' invariants and the tile arithmetic of the GPU shapes are asserted here."""
import functools

import pytest
import torch

import attn_ref as A
import prefill_ref as P

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _qkv(nh=2, M=600, K=128):
    case = P.make_qkv_case(7 + nh, nh, M, K)
    proj = P.project(case["xn"], case["W"])
    return case, proj, P.qkv_rope_ref(case, proj=proj)


@functools.lru_cache(maxsize=None)
def _swiglu(M=70, I=64, K=128):
    case = P.make_swiglu_case(5, M, I, K)
    proj = P.project(case["xn"], case["W"])
    return case, proj, P.swiglu256_ref(case, proj=proj)


# ------------------------------------------------------------------------------------------------------------------------------ the reference itself
def test_rotate_half_reference_equals_llama_apply_rotary_pos_emb():
    case, proj, ref = _qkv()
    tm, nh, M = case["tm"], case["nh"], case["M"]
    pos = (torch.tensor(tm["pos_off"])[torch.tensor(tm["tok_row"])] + torch.tensor(tm["tok_j"])).clamp(max=tm["max_pos"] - 1)
    cos = torch.cat([case["cos"][pos], case["cos"][pos]], -1).to(F64)                # [M, 128]: emb = cat(freqs, freqs)
    sin = torch.cat([case["sin"][pos], case["sin"][pos]], -1).to(F64)
    y = proj[0]
    q, k = y[:, :nh * 128].view(M, nh, 128), y[:, nh * 128:2 * nh * 128].view(M, nh, 128)
    try:
        from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
        qe, ke = apply_rotary_pos_emb(q.transpose(0, 1)[None], k.transpose(0, 1)[None], cos[None], sin[None])
        qe, ke = qe[0].transpose(0, 1), ke[0].transpose(0, 1)
    except ImportError:
        from oracle.ref_cpu import apply_rope
        qe = apply_rope(q.transpose(0, 1)[None], cos[None], sin[None])[0].transpose(0, 1)
        ke = apply_rope(k.transpose(0, 1)[None], cos[None], sin[None])[0].transpose(0, 1)
    torch.testing.assert_close(ref["q"], qe, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(ref["k"], ke, rtol=1e-13, atol=1e-13)
    assert torch.equal(ref["v"], y[:, 2 * nh * 128:].view(M, nh, 128))
    # the tables are the oracle's: inv_freq = theta^(-2j/d), fp32
    from oracle.ref_cpu import rope_cos_sin
    oc, osn = rope_cos_sin(torch.arange(tm["max_pos"]), 128, 10000.0)
    torch.testing.assert_close(case["cos"], oc[:, :64], rtol=0, atol=2e-5)           # fp32 angles (oracle) against float64 angles rounded once
    torch.testing.assert_close(case["sin"], osn[:, :64], rtol=0, atol=2e-5)


def test_reference_rounded_to_bf16_passes_its_own_bound():
    case, proj, ref = _qkv()
    res = P.check_rope(*P.render_rope(ref, "bf16"), ref)
    assert res["ok"] and max(res["ratio"].values()) <= 1.0, res
    for dtype in ("bf16", "f32"):
        for mode in (0, 1):
            rc = P.make_rope_case(3, mode, 5, 3, 150)
            r = P.rope_kv_ref(rc, dtype)
            res = P.check_rope(*P.render_rope(r, dtype), r)
            assert res["ok"], (dtype, mode, res)
    _, _, sref = _swiglu()
    hb = P.sentinel_like((70 + P.GUARD, 64), "bf16")
    hb[:70] = sref["h"].to(torch.bfloat16)
    mx, guard = P.check_swiglu(hb, sref)
    assert mx <= 1.0 and guard, mx


def test_fp32_emulation_of_the_kernels_passes_the_bound():
    case, proj, ref = _qkv()
    y32 = case["xn"].float() @ case["W"].float().t()
    vals = P.emulate_rope_f32(y32, case["tm"], case["nh"], case["cos"], case["sin"])
    res = P.check_rope(*P.render_rope(ref, "bf16", vals), ref)
    assert res["ok"], res
    # K = 320, five K tiles, on the interleaved weights: the epilogue's column order undone by the permutation
    case2 = P.make_qkv_case(11, 2, 300, 320, pool=(1, 63, 64, 65))
    ref2 = P.qkv_rope_ref(case2)
    idx = P.interleave_qk_index(2)
    yp = case2["xn"].float() @ P.interleave_qk_ref(case2["W"], 2).float().t()
    y32 = torch.empty_like(yp)
    y32[:, idx] = yp
    res = P.check_rope(*P.render_rope(ref2, "bf16", P.emulate_rope_f32(y32, case2["tm"], 2, case2["cos"], case2["sin"])), ref2)
    assert res["ok"], res
    for dtype in ("bf16", "f32"):
        rc = P.make_rope_case(4, 1, 2, 3, 150)
        acc = torch.zeros_like(rc["qkv"][0])
        for s in range(3):
            acc = acc + rc["qkv"][s]
        r = P.rope_kv_ref(rc, dtype)
        res = P.check_rope(*P.render_rope(r, dtype, P.emulate_rope_f32(acc, rc["tm"], 2, rc["cos"], rc["sin"])), r)
        assert res["ok"], (dtype, res)
    scase, _, sref = _swiglu()
    h32 = P.emulate_swiglu_f32(scase["xn"].float() @ scase["W"].float().t(), 64)
    hb = P.sentinel_like((70 + P.GUARD, 64), "bf16")
    hb[:70] = h32.to(torch.bfloat16)
    mx, guard = P.check_swiglu(hb, sref)
    assert mx <= 1.0 and guard, mx


# ------------------------------------------------------------------------------------------------------------------------------ checker power
@pytest.mark.parametrize("mut", P.ROPE_MUTANTS, ids=lambda m: "_".join(str(x) for x in m))
def test_qkv_rope_checker_rejects_the_mutant(mut):
    """A kernel with this bug, rounded to bf16 into sentinel-filled buffers, fails the bound or the sentinel screen."""
    case, proj, ref = _qkv()
    bad = P.qkv_rope_ref(case, mut, proj=proj)
    res = P.check_rope(*P.render_rope(bad, "bf16"), ref)
    assert not res["ok"], (mut, res)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_rope_kv_checker_rejects_mutants_in_both_modes(dtype):
    for mode in (0, 1):
        rc = P.make_rope_case(9, mode, 5 if mode == 0 else 2, 3, 150)
        ref = P.rope_kv_ref(rc, dtype)
        for mut in [("sin_sign",), ("pos", 1), ("no_clamp",), ("k_slot", 1), ("v_rot",), ("drop_slab", 1), ("pos_off_row",)] + ([("head_xor",)] if mode else []):
            bad = P.rope_kv_ref(rc, dtype, mut)
            assert not P.check_rope(*P.render_rope(bad, dtype), ref)["ok"], (mode, mut)


def test_checker_sees_a_write_to_an_unowned_slot_and_a_missing_write():
    case, proj, ref = _qkv()
    qb, kc, vc = P.render_rope(ref, "bf16")
    tm = case["tm"]
    kc2 = kc.clone()
    kc2[tm["empty_row"], 0, 0, 5] = 0.0                                 # one element of a row that owns no token
    assert not P.check_rope(qb, kc2, vc, ref)["sentinel"]
    qb2 = qb.clone()
    qb2[tm["over"][0], 3] = 1.0                                         # the qbuf row of an over-capacity token
    assert not P.check_rope(qb2, kc, vc, ref)["sentinel"]
    vc2 = vc.clone()
    vc2[ref["R"], 1, 2, 3] = 0.0                                        # the guard row behind the cache
    assert not P.check_rope(qb, kc, vc2, ref)["sentinel"]
    vc3 = vc.clone()
    m = int(ref["q_owned"].nonzero()[10])
    vc3[ref["row"][m], 1, ref["slot"][m], 7] = P.sentinel_like((1,), "bf16")[0]      # an owned element never written
    assert not P.check_rope(qb, kc, vc3, ref)["ok"]


@pytest.mark.parametrize("mut", P.SWIGLU_MUTANTS, ids=lambda m: m[0])
def test_swiglu_checker_rejects_the_mutant(mut):
    case, proj, ref = _swiglu()
    bad = P.swiglu256_ref(case, mut, proj=proj)
    hb = P.sentinel_like((70 + P.GUARD, 64), "bf16")
    hb[:70] = bad["h"].to(torch.bfloat16)
    mx, _ = P.check_swiglu(hb, ref)
    assert mx > 1.0, (mut, mx)


def test_swiglu_reference_equals_the_plain_definition():
    case, proj, ref = _swiglu()
    g = case["xn"].to(F64) @ case["wg"].to(F64).t()
    u = case["xn"].to(F64) @ case["wu"].to(F64).t()
    torch.testing.assert_close(ref["h"], torch.nn.functional.silu(g) * u, rtol=1e-13, atol=1e-13)
    assert float(ref["bound"].max()) <= 0.01 * float(ref["h"].abs().max())


# ------------------------------------------------------------------------------------------------------------------------------ interleavers
def test_interleave_references_are_permutations_and_invert():
    import decode_ref as D
    for nh in (1, 2, 16):
        idx = P.interleave_qk_index(nh)
        assert torch.equal(idx.sort().values, torch.arange(3 * nh * 128))
        W = torch.arange(3 * nh * 128 * 8, dtype=torch.float32).view(-1, 8)
        Wp = P.interleave_qk_ref(W, nh)
        assert torch.equal(P.deinterleave_qk_ref(Wp, nh), W)
        assert torch.equal(Wp[2 * nh * 128:], W[2 * nh * 128:])          # v rows stay
        # n-tile t of a q / k head: rotary columns 8t .. 8t+7, then their partners 64+8t .. 64+8t+7
        head = idx[nh * 128:(nh + 1) * 128] - nh * 128
        assert head[:16].tolist() == list(range(8)) + list(range(64, 72)) and head[112:].tolist() == list(range(56, 64)) + list(range(120, 128))
    for I in (8, 360):
        wg, wu = torch.randn(I, 4), torch.randn(I, 4)
        W = P.interleave16_ref(wg, wu)
        assert torch.equal(W, D.interleave_gate_up(wg, wu))
        a, b = P.deinterleave16_ref(W)
        assert torch.equal(a, wg) and torch.equal(b, wu)


# ------------------------------------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("M", [1000, 2100, 16897])
def test_token_map_invariants(M):
    tm = P.make_token_map(M, M)
    assert P.token_map_ok(tm) and len(tm["tok_row"]) == M == len(tm["tok_j"])
    R, slots = tm["R"], tm["slots"]
    row, slot = torch.tensor(tm["tok_row"]), torch.tensor(tm["tok_j"])
    q_owned, c_owned = P.owned_masks(tm)
    assert int((~q_owned).sum()) == 2 and sorted((~q_owned).nonzero().flatten().tolist()) == sorted(tm["over"])
    assert all(tm["tok_row"][m] != R - 1 and slots <= tm["tok_j"][m] < 2 * slots for m in tm["over"])       # a missing guard stays inside the caches
    assert int(c_owned.sum()) == M - 2                                   # every other token owns exactly one slot
    assert not c_owned[tm["empty_row"]].any() and tm["lens"][tm["empty_row"]] == 0
    assert set(tm["lens"]) >= {1, 63, 64, 65, 255, 256, 257}
    assert (row[1:] < row[:-1]).any() and (slot[1:] < slot[:-1]).any() and (row[1:] > row[:-1]).any()       # not monotone
    assert sum(1 for p in tm["pos_off"] if p) >= R // 3 and 0 in tm["pos_off"]
    pos = torch.tensor(tm["pos_off"])[row] + slot
    crossing = (pos >= tm["max_pos"]) & q_owned
    assert int(crossing.sum()) >= 2 and set(row[crossing].tolist()) == {tm["clamped_row"]}
    dm = P.make_decode_map(M, 300)
    assert P.token_map_ok(dm) and dm["R"] == 302 and int((~P.owned_masks(dm)[0]).sum()) == 2
    assert (torch.tensor(dm["pos_off"])[:300] + torch.tensor(dm["tok_j"]) >= dm["max_pos"]).any()


def test_host_screen_restated_refuses_what_the_entry_points_refuse():
    tm = P.make_token_map(1, 600)
    bad = dict(tm, tok_row=[tm["R"]] + tm["tok_row"][1:])
    assert not P.token_map_ok(bad)
    last = tm["tok_row"].index(tm["R"] - 1)
    tj = list(tm["tok_j"])
    tj[last] = tm["slots"]
    assert not P.token_map_ok(dict(tm, tok_j=tj))                       # over capacity in the last row
    tj = list(tm["tok_j"])
    tj[tm["over"][0]] = 2 * tm["slots"]
    assert not P.token_map_ok(dict(tm, tok_j=tj))                       # so far over that a missing guard would leave the caches


def test_gpu_shapes_tile_arithmetic():
    """The table of the fused QKV cases: (m-tiles, n-tiles, tiles) as gemm256_try counts them, a partial last tile at all three tile heights."""
    want = {(2, 17000, 128): (67, 3, 201), (2, 16897, 320): (67, 3, 201), (16, 2100, 128): (9, 24, 216), (16, 2305, 192): (10, 24, 240)}
    assert set(want) == set(P.QKV_CASES)
    for (nh, M, K), counts in want.items():
        N = 3 * nh * 128
        assert P.tile_counts(M, N) == counts and P.gemm256_accepts(M, N, K), (nh, M, K)
        for h in (256, 224, 192):
            assert 0 < P.last_tile_rows(M, h) < h, (M, h)
    assert P.last_tile_rows(16897, 256) == 1 and P.last_tile_rows(2305, 256) == 1 and 320 // 64 == 5 and (192 // 64) % 2 == 1
    for M, I, K in P.SWIGLU_CASES:
        assert P.gemm256_accepts(M, 2 * I, K) and I % 8 == 0, (M, I, K)
    assert P.tile_counts(17000, 720) == (67, 3, 201) and 720 % 256 != 0 and (720 // 2) % 128 != 0      # N / 2 ends inside a tile
    assert not P.gemm256_accepts(1000, 768, 128) and not P.gemm256_accepts(17000, 768, 96)
