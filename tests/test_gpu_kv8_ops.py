"""GPU: operator tests of the FP8 KV cache -- the quantiser (pg_op_kv_quantize) bit for bit against tests/kv8_ref.py, and the fused decode
attention over an fp8 cache (pg_diag_op_attn_decode_kv8 -> the production launcher) against the fp64 reference of tests/attn_ref.py run on
the DEQUANTISED caches.  Given the codes the kernel is fp32 attention on exactly those values (the power-of-two scale multiplies are exact),
so the bound is attn_ref.decode_bound(ref, "bf16") unchanged."""
import ctypes as C
import itertools

import pytest
import torch

import attn_ref as A
import kv8_ref
from attn_ops import _i32, _ptr, _stream
from conftest import get_engine

pytestmark = pytest.mark.gpu

# block forms of launch_attn_decode_kv8 (plangen_amd/csrc/kernels.h: KV8_UN_BIG / KV8_UN_SMALL): form -> (UN, NW); 8 keys per wave load
KV8_FORMS = {4: (4, 4), 8: (5, 8)}
KV8_KPI = 8


def kv8_geometry(form):
    un, nw = KV8_FORMS[form]
    return KV8_KPI, KV8_KPI * un, nw * KV8_KPI * un


GEO = [kv8_geometry(f) for f in (4, 8)]


def kv8_counts():
    c = {0, 1, 831, 863}
    for kpi, kpw, ch in GEO:
        c |= {kpi - 1, kpi + 1, kpw - 1, kpw + 1, ch - 1, ch + 1, 2 * ch + 1}
    return sorted(c)


def counts_case(nh, S, order="none", needle=False, seed=0):
    """attn_ref.decode_counts_case's recipe with the kv8 forms' chunk boundaries."""
    counts = kv8_counts()
    counts = counts[1::2] + counts[0::2]
    return A.make_decode_case(1000 + seed + 7 * S + 3 * nh + 1, "bf16", nh, counts, S, n_dec=0, row_order=order, needle=needle,
                              geometry=GEO, pos_jitter=40 if S % 2 else 0)


def shared_case(nh, shared_len, n_dec, S, needle=False, order="none", seed=0):
    """attn_ref.decode_shared_case's recipe (r0 = 0: the two-lane decode is not supported by the fp8 cache) with the kv8 geometry."""
    evens = [shared_len + 37, 1, 290, 2 * shared_len + 3]
    lens = [shared_len if r & 1 else evens[(r // 2) % len(evens)] for r in range(6)]
    return A.make_decode_case(2000 + seed + shared_len + 5 * n_dec + S, "bf16", nh, [L + n_dec for L in lens], S, n_dec=n_dec,
                              shared_len=shared_len, r0=0, row_order=order, needle=needle, geometry=GEO)


_SIG = [C.c_int, C.c_void_p, C.c_int, C.c_long] + [C.c_void_p] * 10 + [C.c_int] * 6 + [C.c_float, C.c_void_p]


def _diag():
    from plangen_amd import _lib
    d = _lib.load_diag()
    d.pg_diag_op_attn_decode_kv8.restype, d.pg_diag_op_attn_decode_kv8.argtypes = C.c_int, _SIG
    return d


class Kv8Dev:
    """A decode case whose caches are quantised on the CPU: codes + interleaved (K, V) scales on the device, the dequantised caches for the
    reference."""

    def __init__(self, d, dev="cuda"):
        assert d["r0"] == 0 and d["dtype"] == "bf16"
        self.d = d
        self.kq, self.ks = kv8_ref.quantize(d["kc"])
        self.vq, self.vs = kv8_ref.quantize(d["vc"])
        self.kvs = torch.stack([self.ks, self.vs], -1).contiguous()
        self.ref_case = dict(d, kc=kv8_ref.dequantize(self.kq, self.ks), vc=kv8_ref.dequantize(self.vq, self.vs))
        self.qkv = d["qkv"].to(dev)
        self.cos, self.sin = d["cos"].to(dev), d["sin"].to(dev)
        self.len, self.pos_off, self.n_dec = _i32(d["len"], dev), _i32(d["pos_off"], dev), _i32([d["n_dec"]], dev)
        self.order = None if d["row_order"] is None else _i32(d["row_order"], dev)
        self.dev = dev

    def run(self, form):
        d = self.d
        kq, vq, kvs = self.kq.to(self.dev), self.vq.to(self.dev), self.kvs.to(self.dev)
        obuf = torch.full((d["M"], d["nh"] * 128), float("nan"), dtype=torch.bfloat16, device=self.dev)
        rc = _diag().pg_diag_op_attn_decode_kv8(form, _ptr(self.qkv), d["S"], d["M"] * 3 * d["nh"] * 128, _ptr(obuf), _ptr(kq), _ptr(vq), _ptr(kvs),
                                                _ptr(self.cos), _ptr(self.sin), _ptr(self.len), _ptr(self.pos_off), _ptr(self.n_dec),
                                                _ptr(self.order), d["shared_len"], d["shared_row_abs"], d["M"], d["nh"], d["slots"], d["max_pos"],
                                                d["scale"], _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return obuf.cpu(), kq.cpu(), vq.cpu(), kvs.cpu()


def check_append_and_poison(dv, kq, vq, kvs):
    """Every slot but the append slots is byte-identical; an append slot holds quantize() of the new key under one of the RoPE evaluation
    orders (per half: the compiler contracts the two rotation formulas independently) and of the new value, bit for bit."""
    d = dv.d
    M, nh = d["M"], d["nh"]
    touched = torch.zeros(kq.shape[:3], dtype=torch.bool)
    for r in range(M):
        slot = d["len"][r] + d["n_dec"]
        touched[r, :, slot] = True
        pos = min(d["pos_off"][r] + slot, d["max_pos"] - 1)
        _, ks, v_t = A.decode_qkv_new(d["qkv"], d["cos"], d["sin"], r, nh, pos, "bf16")
        vc, vsc = kv8_ref.quantize(v_t.float())
        assert torch.equal(vq[r, :, slot], vc) and torch.equal(kvs[r, :, slot, 1], vsc), ("v append", r)
        for h in range(nh):
            hit = False
            for a, b in itertools.product(range(3), range(3)):
                cand = torch.cat([ks[a][h, :64], ks[b][h, 64:]]).float()
                cc, cs = kv8_ref.quantize(cand)
                hit = hit or (torch.equal(kq[r, h, slot], cc) and bool(kvs[r, h, slot, 0] == cs))
            assert hit, ("k append", r, h)
    keep = ~touched
    assert torch.equal(kq[keep], dv.kq[keep]) and torch.equal(vq[keep], dv.vq[keep]), "a slot outside the append was written"
    assert torch.equal(kvs[keep].view(torch.int32), dv.kvs[keep].view(torch.int32)), "a scale outside the append was written"


CASES = [
    ("counts", dict(nh=2, S=1, order="none", needle=False)),
    ("counts", dict(nh=2, S=4, order="lpt", needle=True)),
    ("counts", dict(nh=3, S=8, order="random", needle=True)),
    ("shared", dict(nh=2, shared_len=37, n_dec=5, S=1, order="none", needle=True)),
    ("shared", dict(nh=3, shared_len=130, n_dec=0, S=4, order="lpt", needle=False)),
    ("shared", dict(nh=2, shared_len=41, n_dec=320, S=8, order="random", needle=True)),
]


@pytest.mark.parametrize("form", [4, 8])
@pytest.mark.parametrize("kind,kw", CASES)
def test_decode_attention_over_fp8_cache(kind, kw, form):
    d = counts_case(**kw) if kind == "counts" else shared_case(**kw)
    dv = Kv8Dev(d)
    ref = A.decode_ref(dv.ref_case, "bf16")
    bound = A.decode_bound(ref, "bf16")
    obuf, kq, vq, kvs = dv.run(form)
    ok, mx, worst = A.check(obuf.view(d["M"], d["nh"], 128), ref["out"], bound)
    print(f"kv8 decode {kind} {kw} form {form}: max |err| / bound = {mx:.3f}")
    assert ok, (mx, worst)
    check_append_and_poison(dv, kq, vq, kvs)


def test_reference_case_through_the_stock_helper_and_a_mutant_is_rejected():
    """attn_ref.decode_counts_case as it stands (bf16 geometry), and the checker's power: dropping a needle key from the reference fails."""
    d = A.decode_counts_case("bf16", 2, 4, order="lpt", needle=True)
    dv = Kv8Dev(d)
    ref = A.decode_ref(dv.ref_case, "bf16")
    obuf, kq, vq, kvs = dv.run(0)
    got = obuf.view(d["M"], d["nh"], 128)
    ok, mx, _ = A.check(got, ref["out"], A.decode_bound(ref, "bf16"))
    assert ok, mx
    check_append_and_poison(dv, kq, vq, kvs)
    (r, h), p = next(((rh, p) for rh, p in sorted(d["needles"].items()) if p < d["len"][rh[0]] + d["n_dec"] and p > 0))
    mut = A.decode_ref(dv.ref_case, "bf16", mut=("drop_key", p))
    ok_m, mx_m, _ = A.check(got, mut["out"], A.decode_bound(mut, "bf16"))
    print(f"mutant drop_key {p}: max |err| / bound = {mx_m:.1f}")
    assert not ok_m


@pytest.mark.parametrize("n", [1, 63, 64, 65, 10000])
def test_quantiser_bit_for_bit(tiny_cfg, tiny_weights, n):
    e = get_engine(tiny_cfg, tiny_weights, "bf16", kv_dtype="fp8")
    fam = kv8_ref.row_families(seed=n)
    x = fam[torch.arange(n) % fam.shape[0]].contiguous()
    codes, scale = e.op_kv_quantize(x)
    rc, rs = kv8_ref.quantize(x)
    assert torch.equal(scale.cpu().view(torch.int32), rs.view(torch.int32))
    bad = (codes.cpu() != rc)
    assert not bad.any(), (int(bad.sum()), x[bad][:8], codes.cpu()[bad][:8], rc[bad][:8])
