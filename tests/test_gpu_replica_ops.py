"""GPU: the grouped form of the fused decode attention (pg_diag_op_attn_decode_grouped / _grouped_kv8 -> the production launchers with
SeqState::group_rows > 0), the kernel behind pg_prefill_replicated(alias = 1).  A replica row (row >= R0) reads its prompt slots [0, len) from
its owner row (row % R0) with the key -> (wave, group, chunk) map and the arithmetic of a private row, so the grouped operator on an ALIASED
layout (replicas' prompt slots poisoned) must equal, bit for bit, the existing operator on a fully populated copy in which every replica's
prompt slots hold the owner's values: output rows and appended K/V (codes and scales for the FP8 cache).  Prompt lengths sit on the chunk
edges of both block shapes (keys per wave / per round: bf16 20 / 160 at 8 waves and 24 / 96 at 4 waves; FP8 40 / 320 and 32 / 128)."""
import ctypes as C

import pytest
import torch

from attn_ops import _i32, _ptr, _stream, lib as attn_lib

pytestmark = pytest.mark.gpu

_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
_SIG_GRP = [_I, _I, _P, _I, _L] + [_P] * 9 + [_I] * 7 + [_F, _P]
_SIG_GRP8 = [_I, _P, _I, _L] + [_P] * 10 + [_I] * 7 + [_F, _P]
_SIG_KV8 = [_I, _P, _I, _L] + [_P] * 10 + [_I] * 6 + [_F, _P]
TT = {"bf16": torch.bfloat16, "f32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}


def diag():
    d = attn_lib()
    d.pg_diag_op_attn_decode_grouped.restype, d.pg_diag_op_attn_decode_grouped.argtypes = C.c_int, _SIG_GRP
    d.pg_diag_op_attn_decode_grouped_kv8.restype, d.pg_diag_op_attn_decode_grouped_kv8.argtypes = C.c_int, _SIG_GRP8
    d.pg_diag_op_attn_decode_kv8.restype, d.pg_diag_op_attn_decode_kv8.argtypes = C.c_int, _SIG_KV8
    return d


def bits(t):
    return t.view(BITS[t.dtype])


class Case:
    """R0 owner rows x p replicas (row t * R0 + r = replica t of row r).  `full`: every row's cache fully populated (a replica's prompt slots
    hold its owner's values); `alias`: the same with the aliasing rows' prompt slots poisoned.  shared_len > 0: odd rows carry the shared
    uncond prompt of row 1 (poisoned in BOTH layouts for odd rows other than row 1 -- the existing alias) and only even rows are grouped."""

    def __init__(self, seed, kind, R0, p, nh, lens, n_dec, S=1, shared_len=0, order=False):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.kind, self.R0, self.p, self.nh, self.n_dec, self.S, self.shared_len = kind, R0, p, nh, n_dec, S, shared_len
        M = self.M = R0 * p
        assert len(lens) == R0
        self.lens = [lens[r % R0] for r in range(M)]
        slots = self.slots = max(self.lens) + n_dec + 3
        self.max_pos = slots + 5
        dev = "cuda"
        self.qkv = torch.randn(S, M, 3 * nh * 128, generator=g, device=dev) * (S ** -0.5)
        ang = torch.rand(self.max_pos, 64, generator=g, device=dev) * 6.28
        self.cos, self.sin = ang.cos().contiguous(), ang.sin().contiguous()
        self.len_d, self.pos_off, self.ndec_d = _i32(self.lens, dev), _i32([0] * M, dev), _i32([n_dec], dev)
        self.order = None
        if order:       # replicas of one owner adjacent, longest first: what the engine launches
            self.order = _i32(sorted(range(M), key=lambda r: (-self.lens[r], r % R0, r)), dev)
        shape = (M, nh, slots, 128)
        if kind == "fp8":
            def codes():
                c = torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.int32)
                return torch.where((c & 0x7F) == 0x7F, c - 9, c).to(torch.uint8)          # no NaN codes in the data
            self.k, self.v = codes(), codes()
            self.kvs = torch.pow(2.0, torch.randint(-4, 1, (M, nh, slots, 2), generator=g, device=dev).float()).contiguous()
            poison, spoison = 0x7F, float("nan")
        else:
            T = TT[kind]
            self.k = torch.randn(shape, generator=g, device=dev).to(T)
            self.v = torch.randn(shape, generator=g, device=dev).to(T)
            self.kvs = None
            poison = float("nan")
        rows = torch.arange(M, device=dev)
        slot_i = torch.arange(slots, device=dev)
        ln = torch.tensor(self.lens, device=dev)
        prompt = slot_i[None, :] < ln[:, None]                                         # [M, slots]
        sh_odd = (rows % 2 == 1) & (shared_len > 0)
        own = torch.where(sh_odd, torch.ones_like(rows), rows % R0)
        if shared_len > 0:
            assert all(self.lens[r] >= shared_len for r in range(1, M, 2))
        # prompt slots an aliasing row takes from its owner: [0, shared_len) for odd rows on the shared prompt, [0, len) for replicas
        ali_len = torch.where(sh_odd, torch.full_like(ln, shared_len), ln)
        aliased = (slot_i[None, :] < ali_len[:, None]) & (own != rows)[:, None]          # [M, slots]
        sel = aliased[:, None, :, None]
        for name in ("k", "v"):
            t = getattr(self, name)
            t = torch.where(sel, t[own], t)
            setattr(self, name, t.contiguous())
        if self.kvs is not None:
            self.kvs = torch.where(sel, self.kvs[own], self.kvs).contiguous()
        # the layout the reference run sees: rows on the shared uncond prompt are poisoned there too (the existing operator aliases them itself)
        sh_sel = (aliased & sh_odd[:, None])[:, None, :, None]
        grp_sel = (aliased & ~sh_odd[:, None])[:, None, :, None]
        self.sh_sel, self.grp_sel, self.prompt = sh_sel, grp_sel, prompt

        def poisoned(t, which, val):
            return torch.where(which.expand_as(t), torch.full_like(t, val), t)
        self.full = {n: poisoned(getattr(self, n), sh_sel, poison) for n in ("k", "v")}
        self.alias = {n: poisoned(self.full[n], grp_sel, poison) for n in ("k", "v")}
        if self.kvs is not None:
            self.full["s"] = poisoned(self.kvs, sh_sel, spoison)
            self.alias["s"] = poisoned(self.full["s"], grp_sel, spoison)

    def run(self, grouped, form=0):
        src = self.alias if grouped else self.full
        k, v = src["k"].clone(), src["v"].clone()
        s = src["s"].clone() if "s" in src else None
        odt = torch.float32 if self.kind == "f32" else torch.bfloat16
        obuf = torch.full((self.M, self.nh * 128), float("nan"), dtype=odt, device="cuda")
        slab = self.M * 3 * self.nh * 128
        scale = 128 ** -0.5
        common = (_ptr(self.cos), _ptr(self.sin), _ptr(self.len_d), _ptr(self.pos_off), _ptr(self.ndec_d), _ptr(self.order), self.shared_len, 1)
        tail = (self.M, self.nh, self.slots, self.max_pos, scale)
        d = diag()
        if self.kind == "fp8":
            if grouped:
                rc = d.pg_diag_op_attn_decode_grouped_kv8(form, _ptr(self.qkv), self.S, slab, _ptr(obuf), _ptr(k), _ptr(v), _ptr(s), *common, self.R0,
                                                          *tail, _stream())
            else:
                rc = d.pg_diag_op_attn_decode_kv8(form, _ptr(self.qkv), self.S, slab, _ptr(obuf), _ptr(k), _ptr(v), _ptr(s), *common, *tail, _stream())
        elif grouped:
            rc = d.pg_diag_op_attn_decode_grouped(int(self.kind == "bf16"), form, _ptr(self.qkv), self.S, slab, _ptr(obuf), _ptr(k), _ptr(v), *common,
                                                  self.R0, *tail, _stream())
        else:
            rc = d.pg_diag_op_attn_decode(int(self.kind == "bf16"), form, 0, _ptr(self.qkv), self.S, slab, _ptr(obuf), _ptr(k), _ptr(v), *common,
                                          *tail, None, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return obuf, k, v, s

    def check(self, form=0):
        og, kg, vg, sg = self.run(True, form)
        of, kf, vf, sf = self.run(False, form)
        assert not torch.isnan(of.float()).any(), "the reference run read a poisoned slot: the case is wrong"
        bad = (bits(og) != bits(of)).any(-1).nonzero().flatten().tolist()
        assert not bad, f"output rows differ: {bad[:8]} (lens {[self.lens[r] for r in bad[:8]]}, n_dec {self.n_dec})"
        # caches: outside the grouped rows' aliased prompt slots the two runs hold the same bytes (append slot included) ...
        keep = ~self.grp_sel
        for a, b, name in ((kg, kf, "k"), (vg, vf, "v")) + (((sg, sf, "scale"),) if sg is not None else ()):
            m = keep.expand_as(a)
            assert torch.equal(bits(a)[m], bits(b)[m]), f"{name} cache differs outside the aliased prompt slots"
            # ... and the grouped run has not written into them
            assert torch.equal(bits(a)[~m], bits(self.alias["s" if name == "scale" else name])[~m]), f"{name}: an aliased prompt slot was written"
        # the append slot really was written (not compared vacuously)
        for r in (0, self.M - 1):
            slot = self.lens[r] + self.n_dec
            assert not torch.equal(bits(kg[r, :, slot]), bits(self.alias["k"][r, :, slot]))


@pytest.mark.parametrize("n_dec", [0, 1, 19, 140])
def test_bf16_8wave_form(n_dec):
    """16 rows = R0 4 x p 4, 2 heads (M * nh <= 512: the 8-wave block, 20 keys per wave, 160 per round); lens 7 / 20 / 21 / 163."""
    Case(11 + n_dec, "bf16", 4, 4, 2, [7, 20, 21, 163], n_dec, S=1 + n_dec % 3, order=bool(n_dec % 2)).check()


@pytest.mark.parametrize("n_dec", [0, 23, 100])
def test_bf16_4wave_form(n_dec):
    """36 rows of 16 heads = R0 12 x p 3 (M * nh = 576 > 512: the 4-wave block, 24 keys per wave, 96 per round)."""
    lens = [23, 24, 25, 96, 97, 200, 24, 200, 97, 23, 96, 25]
    Case(50 + n_dec, "bf16", 12, 3, 16, lens, n_dec, S=2, order=n_dec == 23).check()


@pytest.mark.parametrize("n_dec", [0, 1, 39, 290])
def test_fp8_8wave_form(n_dec):
    """FP8 cache, 8-wave block (UN 5: 40 keys per wave, 320 per round): lengths at 8 * UN multiples +- 1."""
    Case(70 + n_dec, "fp8", 4, 4, 2, [7, 39, 41, 321], n_dec, S=1 + n_dec % 2, order=bool(n_dec % 2)).check()
    Case(71 + n_dec, "fp8", 2, 2, 3, [40, 319], n_dec).check()


@pytest.mark.parametrize("n_dec", [0, 31, 100])
def test_fp8_4wave_form(n_dec):
    """FP8 cache, 4-wave block (UN 4: 32 keys per wave, 128 per round), 36 rows of 16 heads."""
    lens = [31, 32, 33, 128, 129, 200, 32, 200, 129, 31, 128, 33]
    Case(90 + n_dec, "fp8", 12, 3, 16, lens, n_dec, S=2, order=n_dec == 31).check()


def test_f32():
    """PG_F32 (2 keys per wave load): 8-wave form 10 keys per wave / 80 per round, 4-wave form 12 / 48."""
    Case(5, "f32", 4, 3, 2, [9, 10, 11, 83], 7, S=2).check()
    Case(6, "f32", 4, 3, 2, [11, 12, 13, 49], 30, S=1, order=True).check(form=4)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("form", [4, 8])
def test_forced_forms_small_batch(kind, form):
    """Both block shapes at one small shape (the form argument overrides the launcher's choice), prompt shorter than / equal to / longer
    than a round."""
    Case(120 + form, kind, 4, 2, 2, [1, 96, 161, 330], 45, S=3).check(form=form)


@pytest.mark.parametrize("kind", ["bf16", "fp8", "f32"])
@pytest.mark.parametrize("n_dec", [0, 50])
def test_shared_uncond_and_grouping_together(kind, n_dec):
    """shared_len > 0 on odd rows (today's alias of row 1, untouched) with grouping on the even rows: R0 4 x p 3, odd rows carry the
    37-token shared prompt."""
    Case(200 + n_dec, kind, 4, 3, 2, [21, 37, 170, 37], n_dec, S=2, shared_len=37, order=True).check()


def test_argument_screen():
    c = Case(1, "bf16", 2, 2, 1, [5, 9], 0)
    d = diag()
    o = torch.zeros(c.M, 128, dtype=torch.bfloat16, device="cuda")
    k, v = c.alias["k"].clone(), c.alias["v"].clone()

    def call(group_rows, len_d=None):
        return d.pg_diag_op_attn_decode_grouped(1, 0, _ptr(c.qkv), c.S, c.M * 3 * 128, _ptr(o), _ptr(k), _ptr(v), _ptr(c.cos), _ptr(c.sin),
                                                _ptr(len_d if len_d is not None else c.len_d), _ptr(c.pos_off), _ptr(c.ndec_d), None, 0, 1,
                                                group_rows, c.M, 1, c.slots, c.max_pos, 0.1, _stream())
    assert call(0) == -1 and call(c.M + 1) == -1
    assert call(2, _i32([5, 9, 6, 9], "cuda")) == -1          # a replica whose length is not its owner's
    assert call(2) == 0
    torch.cuda.synchronize()
