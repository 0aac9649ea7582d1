"""CPU: the host models and comparators of tests/load_ref.py (used by tests/test_gpu_load_ops.py and tests/test_gpu_load_path.py).  The two statements of the
bf16 rounding agree, each layout model agrees with an element-by-element transcription of its kernel's index arithmetic (and with tests/prefill_ref.py, which
models the two interleavers independently), the comparator accepts a model's own output and rejects each planted defect, and the derived tables' bounds have
room around an fp32 evaluation before a kernel is involved."""
import pytest
import torch

import load_ref as R
import prefill_ref as P

BF = torch.bfloat16
KINDS = ("f32", "bf16")


def test_the_two_bf16_roundings_agree_on_edges_and_random_bits():
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 2 ** 32, (200000,), generator=g, dtype=torch.int64)
    u = torch.where((u & 0x7FFFFFFF) > 0x7F800000, u & 0xBFFFFFFF, u)           # no NaNs: their payload is not part of the contract
    x = torch.cat([R.from_bits(u, "f32"), R.edge_block("f32")[:-1]])
    want = R.f32_to_bf16_bits(x)
    got = R.bits(x.to(BF)).to(torch.int64) & 0xFFFF
    assert torch.equal(got, want)
    e = dict(zip(R.EDGE_F32, (R.f32_to_bf16_bits(R.edge_block("f32")).tolist())))
    assert e[0x7F7FFFFF] == 0x7F80 and e[0x7F7F8000] == 0x7F80 and e[0x7F7F7FFF] == 0x7F7F      # up to infinity / the largest finite bf16
    assert e[0x3F808000] == 0x3F80 and e[0x3F818000] == 0x3F82 and e[0xBF808000] == 0xBF80 and e[0xBF818000] == 0xBF82      # ties go to even
    assert e[0x3F807FFF] == 0x3F80 and e[0x3F808001] == 0x3F81 and e[0x3F817FFF] == 0x3F81 and e[0x3F818001] == 0x3F82
    assert e[0x00000001] == 0 and e[0x00008000] == 0 and e[0x00018000] == 2 and e[0x007FFFFF] == 0x0080 and e[0x80000000] == 0x8000
    assert torch.isnan(R.edge_block("f32")[-1]) and torch.isnan(R.edge_block("bf16")[-1])
    assert int(torch.isnan(R.edge_block("f32")).sum()) == 1 and int(torch.isnan(R.edge_block("bf16")).sum()) == 1
    # bf16 -> fp32 appends 16 zero bits
    b = R.edge_block("bf16")
    assert torch.equal((R.bits(b.float()).to(torch.int64) & 0xFFFFFFFF)[:-1], ((R.bits(b).to(torch.int64) & 0xFFFF) << 16)[:-1])


@pytest.mark.parametrize("kind", KINDS)
def test_values_carry_the_edge_block_and_round_inexactly(kind):
    for n in (1, 7, 8, 65537):
        x = R.values(n, kind, seed=n)
        e = R.edge_block(kind)
        m = min(n, e.numel())
        assert R.same_bits(x[:m], e[:m])["ok"] and x.dtype == R.tdtype(kind)
        if n >= e.numel():
            assert R.same_bits(x[-e.numel():], e)["ok"]
    if kind == "f32":
        x = R.values(65537, kind, seed=1)
        inexact = (x.to(BF).float() != x) & torch.isfinite(x)
        assert float(inexact.float().mean()) > 0.9                              # the rounding is exercised by almost every element
    assert torch.equal(R.bits(R.values(100, kind, 5)), R.bits(R.values(100, kind, 5)))


def _conv_loop(w):
    co, ci, kk = w.shape
    dst = torch.empty(co * kk * ci, dtype=w.dtype)
    src = w.reshape(-1)
    for i in range(dst.numel()):                                                # convert_conv_kernel, line by line
        c, t = i % ci, i // ci
        tap, o = t % kk, t // kk
        dst[i] = src[(o * ci + c) * kk + tap]
    return dst.reshape(co, kk, ci)


def test_conv_layout_matches_the_kernel_index_arithmetic():
    for shape in [(1, 1, 9), (3, 5, 9), (4, 6, 1)]:
        w = torch.arange(shape[0] * shape[1] * shape[2], dtype=torch.float32).reshape(shape)
        assert torch.equal(R.conv_ref(w, "f32"), _conv_loop(w))
        w4 = w.reshape(shape[0], shape[1], *((3, 3) if shape[2] == 9 else (1, 1)))
        assert torch.equal(R.conv_ref(w4, "f32"), _conv_loop(w))
        assert torch.equal(R.conv_ref(w4, "f32"), w4.permute(0, 2, 3, 1).reshape(shape[0], shape[2], shape[1]))      # Engine.op_conv3x3's statement of it


def test_interleave16_matches_the_kernel_and_prefill_ref():
    for I, H in [(8, 8), (16, 24), (40, 16)]:
        g = torch.arange(I * H, dtype=torch.float32).reshape(I, H)
        u = g + 10000
        out = torch.full((2 * I, H), -1.0)
        for which, src in ((0, g), (1, u)):                                     # convert_il16_kernel, line by line
            for i in range(I * H):
                r, c = i // H, i % H
                out[(r >> 3) * 16 + which * 8 + (r & 7), c] = src.reshape(-1)[i]
        assert torch.equal(R.il16_ref(g, u, "f32"), out)
        assert torch.equal(R.il16_ref(g, u, "f32"), P.interleave16_ref(g, u))
        fill = R.sentinel_like((2 * I, H), "f32")
        half = R.il16_ref(g, None, "f32", fill=fill)                            # one launch writes its own rows only
        assert bool(R.is_sentinel(half[R.il16_rows(I, 1)]).all()) and torch.equal(half[R.il16_rows(I, 0)], g)
        assert sorted(torch.cat([R.il16_rows(I, 0), R.il16_rows(I, 1)]).tolist()) == list(range(2 * I))


def test_tiled_layout_matches_the_kernel_and_is_a_permutation():
    for N, K in [(16, 128), (48, 256), (32, 384)]:
        W = torch.arange(N * K, dtype=torch.float32).reshape(N, K)
        dst = torch.empty(N * K)
        nch = K // R.SK_BK
        for v in range(N * K // 8):                                             # tile_weights_kernel, line by line
            lane, i, t = v & 63, (v >> 6) & 3, v >> 8
            chunk, ntile = t % nch, t // nch
            n, k = ntile * 16 + (lane & 15), chunk * R.SK_BK + i * 32 + (lane >> 4) * 8
            dst[v * 8:v * 8 + 8] = W[n, k:k + 8]
        assert torch.equal(R.tile_ref(W), dst)
        assert sorted(R.tile_index(N, K).tolist()) == list(range(N * K // 8))
    assert R.can_tile(768, 256) and not R.can_tile(24, 128) and not R.can_tile(16, 192)


def test_rotary_interleave_matches_the_kernel_and_prefill_ref():
    for nh in (1, 2, 3):
        idx = R.interleave_qk_index(nh)
        HD = nh * 128
        for n in range(3 * HD):                                                 # interleave_qk_kernel, line by line
            sec = n // HD
            hc = n - sec * HD
            head, c = hc >> 7, hc & 127
            so = c
            if sec < 2:
                t, p = c >> 4, c & 15
                so = 8 * t + p if p < 8 else 64 + 8 * t + p - 8
            assert int(idx[n]) == sec * HD + head * 128 + so
        assert torch.equal(idx, P.interleave_qk_index(nh))
    assert R.can_fuse(8, 2113, 256) and not R.can_fuse(8, 2112, 256) and not R.can_fuse(8, 96, 256)


def test_row_mover_models():
    table = torch.arange(5 * 4, dtype=torch.float32).reshape(5, 4)
    ids = torch.tensor([-1, 0, 4, 5, R.INT32_MAX, 2, -2 ** 31], dtype=torch.int32)
    assert R.embed_gather_ref(table, ids, None)[:, 0].tolist() == [0, 0, 16, 16, 16, 8, 0]      # clamped to [0, vocab - 1]
    assert R.embed_gather_ref(table, ids, torch.tensor([5, 5, 2], dtype=torch.int32))[:, 0].tolist() == [8, 8, 16]
    src = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    dst = torch.full((5, 3), -1.0)
    out = R.copy_rows_ref(src, torch.tensor([3, 3, 0]), dst, torch.tensor([4, 0, 2]), 3)
    assert out[:, 0].tolist() == [9, -1, 0, -1, 9]
    assert R.copy_rows_ref(src, None, dst, None, 2)[:, 0].tolist() == [0, 3, -1, -1, -1]
    assert R.rows_to_f32_ref(src.to(BF), torch.tensor([2, 2]), 2).dtype == torch.float32
    out = R.t_to_rows_ref(torch.tensor([[1.00390625, 1.01171875]]), torch.zeros(2, 2, dtype=BF), torch.tensor([1]), 1)
    assert out[1].float().tolist() == [1.0, 1.015625] and out[0].float().tolist() == [0.0, 0.0]      # ties to even: 1 + 2^-8 down, 1 + 3 2^-8 up
    ids2 = torch.zeros(6, 10, dtype=torch.int32)
    assert R.rows_differ_ref(ids2, 3, 2, 1, 2, 4) == 0
    a = ids2.clone(); a[5, 3] = 1
    assert R.rows_differ_ref(a, 3, 2, 1, 2, 4) == 0                             # the difference sits at from - 1
    for col in (4, 9):
        a = ids2.clone(); a[5, col] = 1
        assert R.rows_differ_ref(a, 3, 2, 1, 2, 4) == 1
    a = ids2.clone(); a[1, 9] = 1                                               # in the reference row only: every probed row differs from it
    assert R.rows_differ_ref(a, 3, 2, 1, 2, 4) == 1
    a = ids2.clone(); a[4, 9] = 1                                               # a row the stride skips
    assert R.rows_differ_ref(a, 3, 2, 1, 2, 4) == 0
    iv = R.index_vectors(7, 9, 0)
    assert sorted(set(iv["permutation"].tolist())) == sorted(iv["permutation"].tolist()) and len(set(iv["repeats"].tolist())) < 7


@pytest.mark.parametrize("dst", KINDS)
@pytest.mark.parametrize("src", KINDS)
def test_comparator_accepts_the_models_and_rejects_each_planted_defect(src, dst):
    w = R.values(4 * 6 * 9, src, 11).reshape(4, 6, 3, 3)
    w[0, 0, 0, 0] = 1.5                                                         # keep the tensor free of the edge block's repeats where a defect is planted
    want = R.conv_ref(w, dst)
    assert R.same_bits(R.conv_ref(w, dst), want)["ok"]
    res = R.same_bits(R.defect_conv_swapped(w, dst), want)                      # tap and channel swapped
    assert not res["ok"] and res["n_bad"] > want.numel() // 2, res
    g, u = R.values(16 * 24, src, 12).reshape(16, 24), R.values(16 * 24, src, 13).reshape(16, 24)
    want = R.il16_ref(g, u, dst)
    assert R.same_bits(R.il16_ref(g, u, dst), want)["ok"]
    res = R.same_bits(R.defect_il16_halves(g, u, dst), want)                    # gate and up exchanged
    assert not res["ok"] and res["n_bad"] > want.numel() // 2, res
    for row in (0, 31):                                                         # one row dropped: the sentinel shows
        res = R.same_bits(R.defect_row_dropped(want, row), want)
        assert not res["ok"] and res["n_bad"] >= 24 - 2, res                    # (a NaN of the edge block in that row compares as NaN)
    x = torch.linspace(1.0, 2.0, 300).to(R.tdtype(dst))
    res = R.same_bits(R.defect_element_moved(x, 7, 150), x)                     # one element moved (exchanged with another)
    assert not res["ok"] and res["n_bad"] == 2 and res["first"][0] == 7, res
    nan_a, nan_b = R.from_bits(torch.tensor([0x7FC1]), "bf16"), R.from_bits(torch.tensor([0x7FC0]), "bf16")
    assert R.same_bits(nan_a, nan_b)["ok"] and not R.same_bits(torch.zeros(1, dtype=BF), nan_b)["ok"] and not R.same_bits(nan_a, torch.zeros(1, dtype=BF))["ok"]
    assert not R.same_bits(torch.zeros(1), -torch.zeros(1))["ok"]               # the sign of zero is a bit
    assert not R.same_bits(torch.zeros(2), torch.zeros(3))["ok"] and not R.same_bits(torch.zeros(2), torch.zeros(2, dtype=BF))["ok"]


def test_tiled_and_rotary_comparators_reject_a_moved_vector():
    W = R.values(32 * 256, "bf16", 21).reshape(32, 256)
    t = R.tile_ref(W)
    assert R.same_bits(R.tile_ref(W), t)["ok"]
    assert not R.same_bits(W.reshape(-1), t)["ok"]                              # row-major left in place
    assert not R.same_bits(R.defect_element_moved(t, 8 * 70, 8 * 71), t)["ok"]
    Wq = R.values(3 * 128 * 8, "bf16", 22).reshape(384, 8)
    p = R.interleave_qk_ref(Wq, 1)
    assert R.same_bits(p[256:], Wq[256:])["ok"] and not R.same_bits(p[:256], Wq[:256])["ok"]
    assert not R.same_bits(R.defect_row_dropped(p, 383), p)["ok"]


def test_slot_kinds_cover_every_name_of_the_reference_state_dict(ocfg, tiny_weights):
    kinds = {n: R.expected_kind(n, tuple(t.shape)) for n, t in tiny_weights.items()}
    assert set(kinds.values()) == {R.K_T, R.K_F32, R.K_IL16_G, R.K_IL16_U, R.K_CONV}
    assert kinds["gen_vision_model.decoder.conv_in.weight"] == R.K_CONV and kinds["gen_vision_model.encoder.conv_in.weight"] == R.K_F32
    assert kinds["gen_vision_model.decoder.mid.1.q.weight"] == R.K_T and kinds["gen_vision_model.post_quant_conv.weight"] == R.K_F32
    assert kinds["gen_vision_model.decoder.mid.1.norm.weight"] == R.K_F32 and kinds["language_model.model.norm.weight"] == R.K_T
    assert kinds["vision_model.vision_tower.patch_embed.proj.weight"] == R.K_T and kinds["vision_model.vision_tower.pos_embed"] == R.K_F32
    W16 = {k: v.to(BF) for k, v in tiny_weights.items()}
    W32 = {k: v.float() for k, v in W16.items()}
    for name in ("language_model.model.layers.1.mlp.up_proj.weight", "gen_vision_model.decoder.conv_out.weight", "gen_embed.weight",
                 "language_model.model.layers.0.self_attn.k_proj.weight"):
        for ek in KINDS:
            a, ka = R.slot_ref(W16, name, ek)
            b, kb = R.slot_ref(W32, name, ek)
            assert ka == kb == kinds[name] and R.same_bits(a, b)["ok"]          # a bf16 checkpoint and its fp32 copy load to the same bytes
            assert a.dtype == (torch.float32 if ka == R.K_F32 else R.tdtype(ek))
    d = R.derived_refs(W16, ocfg)
    assert all(v is not None for v in d.values()) and len(d) == 4 * ocfg.n_layers + 3
    assert d["layers.0.wqkv_t"].numel() == 3 * ocfg.n_heads * 128 * ocfg.hidden


def test_derived_table_bounds_have_room_and_reject_defects(tiny_weights):
    W = {k: v.to(BF).float() for k, v in tiny_weights.items()}
    ref, bound = R.gen_table_ref(W)
    e = torch.nn.functional.embedding(torch.arange(ref.shape[0]), W["gen_embed.weight"])
    f32 = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(e, W["gen_aligner.layers.0.weight"], W["gen_aligner.layers.0.bias"])),
                                     W["gen_aligner.layers.2.weight"], W["gen_aligner.layers.2.bias"])
    r, _ = R.within(f32, ref, bound)
    assert r < 0.5, r
    bad = f32.clone(); bad[3] = f32[4]
    assert R.within(bad, ref, bound)[0] > 100
    no_gelu = torch.nn.functional.linear(torch.nn.functional.linear(e, W["gen_aligner.layers.0.weight"], W["gen_aligner.layers.0.bias"]),
                                         W["gen_aligner.layers.2.weight"], W["gen_aligner.layers.2.bias"])
    assert R.within(no_gelu, ref, bound)[0] > 100
    assert float(bound.median()) < 1e-4 < float(ref.abs().median()) / 100       # an fp32 accumulation bound (K = 256: ~4e-5), far below the values
    for kind in KINDS:
        ref, bound = R.pq_table_ref(W, kind)
        cb = torch.nn.functional.normalize(W["gen_vision_model.quantize.embedding.weight"], dim=-1)
        f32 = torch.nn.functional.linear(cb, W["gen_vision_model.post_quant_conv.weight"].reshape(ref.shape[1], -1), W["gen_vision_model.post_quant_conv.bias"])
        got = f32.to(R.tdtype(kind))
        r, _ = R.within(got, ref, bound)
        assert r < (0.5 if kind == "f32" else 1.0), (kind, r)            # one bf16 rounding alone reaches 2^-8 |ref| at the low end of a binade
        unnorm = torch.nn.functional.linear(W["gen_vision_model.quantize.embedding.weight"] * 1.01,
                                            W["gen_vision_model.post_quant_conv.weight"].reshape(ref.shape[1], -1), W["gen_vision_model.post_quant_conv.bias"])
        assert R.within(unnorm.to(R.tdtype(kind)), ref, bound)[0] > 1.0
    cos, sin, bound = R.rope_ref(350, 10000.0)
    c32, s32 = R.rope_host_emul(350, 10000.0)
    rc, rs = R.within(c32, cos, bound)[0], R.within(s32, sin, bound)[0]
    print(f"RoPE tables, numpy fp32 evaluation over 350 positions: cos at {rc:.3f}, sin at {rs:.3f} of the bound")
    assert rc <= 1.0 and rs <= 1.0
    shifted = torch.cat([c32[1:], c32[:1]])
    assert R.within(shifted, cos, bound)[0] > 1000                              # a table one position off
    assert R.within(s32, cos, bound)[0] > 1000
    assert float(bound[349, 0]) < 1e-4 and float(bound[0].max()) < 2e-7         # 4 u phi + 2 u: 8.4e-5 at phi = 349, 1.2e-7 at phi = 0
