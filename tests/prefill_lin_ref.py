"""Reference, cases, mutants and the fp32 re-evaluation of the operator tests of the 256 x 256 GEMM's plain-operand epilogues at LLM prefill shapes
(tests/test_gpu_prefill_lin_ops.py, tests/test_prefill_lin_ref_cpu.py): gemm256.hip on tile256.h with GemmA::kind == 0 and the runtime epilogue of
gemm_common.h -- v = acc scale + bias_n[col] + bias_m[row] + residual[row, col], the optional erf GELU, the store (fp32 or bf16) -- in the forms
pg_engine::gemm_residual (fp32 output aliasing the fp32 residual), gemm_f32out (bare) and the gen_head's first layer (bias_n + GELU, bf16) launch it.

Plain torch, any device (the GPU test keeps the float64 operands on the device; nothing here touches the package).  Notation as tests/vq_ref.py.

Bound.  vq_ref.gemm_bound(ref, mag, K, out_kind, act, scaled), unchanged: (K + 2) u32 x bracket [+ GELU terms] + u_out |ref|.  It lacks no term for these forms:
  * the residual's magnitude is part of the bracket ``mag`` as vq_ref.gemm_ref builds it (sum|a w| |scale| + |bias_n| + |bias_m| + |res|): one fp32 rounding of a
    partial result no larger than the bracket per epilogue addition -- bias_n, bias_m and the residual are three, and (K - 1) + 3 = K + 2 is what the bound
    already counts (a launch with all three has no GELU here, and the K - 1 of the accumulation is itself an over-count of one MFMA's internal order);
  * a bf16 residual is exact in fp32; an in-place residual is the same arithmetic on the same values (each element is read once, by the thread that then
    writes it);
  * scale = 0.125 is a power of two: the product is exact, so ``scaled`` (one more rounding) is NOT claimed for it.

Cases.  gemm256_try takes a plain launch when K % 64 == 0, K >= 128, the padded tile area is at most 5/4 of M N and there are at least 200 tiles of 256 x 256
(vision_ref.gemm256_takes restates it); pick_tile_height then chooses 256 / 224 / 192 rows (MT1 = 4 / 3 / 2) by a cost model over the device's CU count, or
pg_tune->gemm256 pins them (4 / 5 / 6; + 8 = four phases per K tile, PH = 4).  N = 2048 needs 25 tile rows: M = 6145 is the smallest M the rule admits (6144 =
192 tiles is refused), and K = 64 is refused at any size.  All cases of one (N, K) share one operand set: case rows / columns are PREFIXES of it, so one
float64 product serves them all."""
from __future__ import annotations

import functools
import math

import torch

from vision_ref import F64, U_F32, gemm256_takes, gemm_bound, rnd, u_of, worst      # noqa: F401  (re-exported for the tests)

OPTS256 = (1, 4, 5, 6, 12, 13, 14)                       # pg_tune->gemm256: auto | 256 / 224 / 192 rows pinned | + 8 = four phases per K tile
HEIGHT = {4: 256, 5: 224, 6: 192}
NOMINAL_CUS = 256                                        # MI355X; the GPU test passes the device's own count

# name: (N, K, fp32 engine).  k5632 = down_proj's depth, k2048 = o_proj's; n256 = the narrowest N (one tile column, 200 tile rows)
GROUPS = {"k128": (2048, 128, False), "k192": (2048, 192, False), "k2048": (2048, 2048, False), "k5632": (2048, 5632, False), "n256": (256, 128, False),
          "f32": (200, 72, True)}

# The epilogue matrix.  pad: ldc = N + pad; rpad: ldr = N + rpad (None: ldr = 0, "as the output"); inplace: out == residual.
EPIS = {
    "inplace":     dict(res="f32", inplace=True),                          # o_proj / down_proj: x += proj(h), ldc == N
    "inplace_gap": dict(res="f32", inplace=True, pad=8),                   # ldc > N, ldr = 0 (vector epilogue: ldc % 4 == 0)
    "inplace_odd": dict(res="f32", inplace=True, pad=3),                   # ldc % 4 != 0: vec_ok() false, the scalar epilogue
    "res_sep":     dict(res="f32", pad=8, rpad=16),                        # a separate residual, ldr != ldc
    "res_bf16":    dict(res="bf16", rpad=0),                               # bf16 residual, fp32 output
    "bias_n":      dict(bias_n=True),
    "bias_m":      dict(bias_m=True),
    "both_scaled": dict(bias_n=True, bias_m=True, scale=0.125),
    "gelu_bf16":   dict(bias_n=True, act=1, out="bf16"),                   # gen_head layer 1
    "bare":        dict(),                                                 # the slab form of gemm_f32out
}
F32_EPIS = {**{k: v for k, v in EPIS.items() if k not in ("res_bf16", "gelu_bf16")}, "gelu": dict(bias_n=True, act=1)}     # the fp32 engine stores fp32 and reads fp32
F32_M = (1, 37, 130)

MUTANTS = {"res_twice": "inplace", "res_row_xor32": "inplace", "res_ldc": "res_sep", "bias_m_col": "bias_m", "clip16": "inplace", "wrap_skip": "inplace"}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------------ tile arithmetic
def smallest_m(N):
    """The smallest M gemm256_try admits at this N (K >= 128): the first row of the tile row that completes 200 tiles."""
    ntn = -(-N // 256)
    M = (-(-200 // ntn) - 1) * 256 + 1
    assert gemm256_takes(M, N, 128, 1) and not gemm256_takes(M - 1, N, 128, 1)
    return M


def edge_ms(N):
    """{M: why}: one below, at and one above the first multiple of each tile height past the smallest admitted M; 6145 and 6399 leave 1 and 255 rows in the
    last 256-row tile."""
    lo = smallest_m(N)
    out = {lo: "smallest admitted; 1 row in the last 256-row tile"}
    for h in HEIGHT.values():
        k = -(-(lo + 1) // h)
        for d in (-1, 0, 1):
            out.setdefault(k * h + d, f"{k} x {h} {d:+d}")
    return out


def wrap_m(ncu, N=2048):
    """M whose 256-row tile count exceeds ncu by at most one tile row (1 .. N / 256 tiles): some persistent blocks run a second tile; ragged last tile."""
    ntn = -(-N // 256)
    return (max(-(-200 // ntn), ncu // ntn + 1) - 1) * 256 + 37


def tiles(M, N, height):
    return -(-M // height) * -(-N // 256)


def auto_height(M, N, ncu):
    """pick_tile_height for an unbatched launch, restated."""
    best, cost = None, None
    for h in (256, 224, 192):
        c = -(-tiles(M, N, h) // ncu) * (h + 16)
        if cost is None or c < cost:
            best, cost = h, c
    return best


def round_tiles(M, N, height, G, rnd):
    """(tile row, tile column) of the tiles round ``rnd`` of the persistent loop (base = rnd G) owns, in the kernel's order of tile indices: 4 tile rows x
    all tile columns per group.  (xcd_remap permutes positions inside a round; the set is what matters here.)"""
    ntm, ntn = -(-M // height), -(-N // 256)
    out = []
    for t in range(rnd * G, min((rnd + 1) * G, ntm * ntn)):
        mg, rem = divmod(t, 4 * ntn)
        gm = min(4, ntm - 4 * mg)
        out.append((mg * 4 + rem % gm, rem // gm))
    return out


def second_pass_tiles(M, N, height, G):
    return round_tiles(M, N, height, G, 1)


# ------------------------------------------------------------------------------------------------------------------------------ cases
def make_case(group, M, N, epi, why=""):
    Nf, K, f32 = GROUPS[group]
    e = (F32_EPIS if f32 else EPIS)[epi]
    ldc = N + e.get("pad", 0)
    ldr = 0 if e.get("rpad") is None else N + e["rpad"]
    return dict(group=group, M=M, N=N, K=K, epi=epi, ldc=ldc, ldr=ldr, out=e.get("out", "f32"), res=e.get("res"), inplace=bool(e.get("inplace")),
                bias_n=bool(e.get("bias_n")), bias_m=bool(e.get("bias_m")), scale=e.get("scale", 1.0), act=e.get("act", 0), why=why,
                engine="f32" if f32 else "bf16", id=f"{group}-M{M}-N{N}-{epi}")


def cases256(ncu=NOMINAL_CUS):
    """Every case meant for the 256 tile.  The whole epilogue matrix at M = 6273 (a ragged last tile at all three heights: 24 x 256 + 129, 28 x 224 + 1,
    32 x 192 + 129); the in-place residual at every M edge, at the wrap, at both N that end inside a tile column (1800: vector epilogue; 1802: scalar), at the
    narrowest N and at every K; the bf16 GELU form (8-byte stores) at the smallest M, the wrap and both ragged N."""
    lo, wm = smallest_m(2048), wrap_m(ncu)
    out = [make_case("k128", 6273, 2048, epi, "epilogue matrix") for epi in EPIS]
    for M, why in edge_ms(2048).items():
        if M != 6273:
            out.append(make_case("k128", M, 2048, "inplace", why))
    out.append(make_case("k128", lo, 2048, "gelu_bf16", "smallest admitted"))
    for epi in ("inplace", "gelu_bf16"):
        out.append(make_case("k128", wm, 2048, epi, "wrap: tiles > CUs"))
        out.append(make_case("k128", lo, 1800, epi, "N ends inside a tile column"))
        out.append(make_case("k128", lo, 1802, epi, "N % 4 != 0: scalar epilogue"))
    out.append(make_case("n256", smallest_m(256), 256, "inplace", "one tile column, 200 tile rows"))
    out.append(make_case("k192", lo, 2048, "inplace", "three K tiles"))
    out.append(make_case("k2048", lo, 2048, "inplace", "o_proj depth"))
    out.append(make_case("k5632", lo, 2048, "inplace", "down_proj depth"))
    for c in out:
        assert gemm256_takes(c["M"], c["N"], c["K"], 1), c["id"]
    return out


def cases_f32():
    return [make_case("f32", M, 200, epi) for M in F32_M for epi in F32_EPIS]


def group_rows(group, ncu=NOMINAL_CUS):
    """Rows of the group's operand set: the largest M any of its cases uses."""
    if group == "f32":
        return max(F32_M)
    return max(c["M"] for c in cases256(ncu) if c["group"] == group)


# ------------------------------------------------------------------------------------------------------------------------------ inputs and reference
@functools.lru_cache(maxsize=None)
def inputs(group, rows):
    """a [rows, K], w [N, K] (values of the engine's type), bias_n [N], bias_m [rows], res fp32 [rows, N].  Asymmetric as vision_ref.lin_inputs: a per-k ramp on a,
    a per-output ramp on w, a column ramp on bias_n and the residual -- and row ramps on a, bias_m and the residual, so rows cannot be exchanged either.
    Cached: callers must not modify the tensors."""
    N, K, f32 = GROUPS[group]
    g = _gen(sum(map(ord, group)) * 977 + rows)
    T = "f32" if f32 else "bf16"
    a = rnd(torch.randn(rows, K, generator=g) * torch.linspace(0.5, 1.5, K) * torch.linspace(1.2, 0.8, rows)[:, None], T)
    w = rnd(torch.randn(N, K, generator=g) * torch.linspace(0.6, 1.4, N)[:, None] / math.sqrt(K), T)
    bias_n = torch.linspace(-1.0, 1.0, N) + 0.01
    bias_m = torch.linspace(2.0, -2.0, rows) + 0.02
    res = torch.randn(rows, N, generator=g) * 2 + torch.linspace(3.0, -3.0, N) + torch.linspace(-1.0, 1.0, rows)[:, None]
    return a, w, bias_n, bias_m, res


def core(group, rows, device="cpu", row_idx=None):
    """(a w^T, |a| |w|^T) float64 [rows, N] on ``device``, computed once per group by the caller (row_idx: of those rows only)."""
    a, w = inputs(group, rows)[:2]
    if row_idx is not None:
        a = a[row_idx]
    a64, w64 = a.to(device, F64), w.to(device, F64)
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def residual_of(c, rows, device="cpu"):
    """The residual's VALUES [M, N] as the kernel receives them (fp32; the bf16 residual is its rounding), or None."""
    if c["res"] is None:
        return None
    r = inputs(c["group"], rows)[4][:c["M"], :c["N"]]
    return rnd(r, c["res"]).to(device)


def residual_buffer(c, rows):
    """A separate residual in its own layout: fp32 values [M, ldr] with NaN between the rows' ends (ldr > N), so a read past a row's N columns shows."""
    r = residual_of(c, rows)
    ld = c["ldr"] or c["N"]
    buf = torch.full((c["M"], ld), float("nan"))
    buf[:, :c["N"]] = r
    return buf


def lin_ref(c, cr, rows, mutant=None, height=256, G=NOMINAL_CUS, row_idx=None):
    """(ref, bracket) float64 [M, N] of case c from cr = core(..) (any device; row_idx: cr holds those rows of the case only, and so does the result).
    mutant (of MUTANTS, for the checker-power tests; the bracket is the true one):
      res_twice      the residual added twice
      res_row_xor32  the residual of row ^ 32, the lane-pair partner (rows whose partner lies past M keep their own)
      res_ldc        the residual read at row ldc + col of its buffer in place of row ldr + col (a case with ldr != ldc)
      bias_m_col     bias_m indexed by the column
      clip16         rows past the last multiple of 16 are never stored
      wrap_skip      the tiles of the persistent loop's second round (tile t + gridDim) are never stored
    What is never stored keeps the pre-fill: NaN, or the residual itself where the output aliases it."""
    M, N = c["M"], c["N"]
    dev = cr[0].device
    _, _, bn, bm, _ = inputs(c["group"], rows)
    if row_idx is None:
        dot, mag = cr[0][:M, :N] * c["scale"], cr[1][:M, :N] * abs(c["scale"])
    else:
        assert mutant is None and int(row_idx.max()) < M
        dot, mag = cr[0][:, :N] * c["scale"], cr[1][:, :N] * abs(c["scale"])
    if c["bias_n"]:
        b = bn[:N].to(dev, F64)
        dot, mag = dot + b, mag + b.abs()
    if c["bias_m"]:
        b = (bm[:M] if row_idx is None else bm[row_idx]).to(dev, F64)
        mag = mag + b.abs()[:, None]
        dot = dot + (bm.to(dev, F64)[torch.arange(N, device=dev) % bm.numel()][None, :] if mutant == "bias_m_col" else b[:, None])
    r = residual_of(c, rows, dev)
    if r is not None:
        r = (r if row_idx is None else r[row_idx.to(dev)]).to(F64)
        mag = mag + r.abs()
        add = r
        if mutant == "res_row_xor32":
            p = torch.arange(M, device=dev) ^ 32
            add = r[torch.where(p < M, p, torch.arange(M, device=dev))]
        elif mutant == "res_ldc":
            assert c["ldr"] and c["ldr"] != c["ldc"]
            flat = residual_buffer(c, rows).reshape(-1).to(dev, F64)
            idx = torch.arange(M, device=dev)[:, None] * c["ldc"] + torch.arange(N, device=dev)[None, :]
            add = flat[idx.clamp(max=flat.numel() - 1)]
        dot = dot + add * (2 if mutant == "res_twice" else 1)
    if c["act"] == 1:
        dot = 0.5 * dot * (1 + torch.erf(dot * 2.0 ** -0.5))
    if mutant in ("clip16", "wrap_skip"):
        kept = r if c["inplace"] else torch.full_like(dot, float("nan"))
        dot = dot.clone()
        if mutant == "clip16":
            dot[M // 16 * 16:] = kept[M // 16 * 16:]
        else:
            for tm, tn in second_pass_tiles(M, N, height, G):
                dot[tm * height:(tm + 1) * height, tn * 256:(tn + 1) * 256] = kept[tm * height:(tm + 1) * height, tn * 256:(tn + 1) * 256]
    return dot, mag


def is_pow2(x):
    return x > 0 and math.frexp(x)[0] == 0.5


def lin_bound(c, ref, mag, store=True):
    """vq_ref.gemm_bound for the case (module docstring).  store=False: without the output rounding term (the bound of the fp32 value before a bf16 store)."""
    return gemm_bound(ref, mag, c["K"], c["out"] if store else "f32", c["act"], scaled=not is_pow2(c["scale"]))


def ratio(got, ref, bound):
    return worst((got.to(F64) - ref).abs(), bound)[0]


def lin_emul32(c, rows, row_idx=None):
    """The operation in fp32 in ANOTHER order than any kernel's: K in chunks of 32 added from the last chunk to the first, the epilogue as
    (residual + bias_m) + (bias_n + acc scale), GELU in fp32; the value BEFORE the store's rounding (CPU)."""
    M, N = c["M"], c["N"]
    a, w, bn, bm, _ = inputs(c["group"], rows)
    a, w = (a[:M] if row_idx is None else a[row_idx]).float(), w[:N].float()
    acc = torch.zeros(a.shape[0], N)
    for k0 in reversed(range(0, c["K"], 32)):
        acc = acc + a[:, k0:k0 + 32] @ w[:, k0:k0 + 32].t()
    v = acc * torch.tensor(c["scale"], dtype=torch.float32)
    if c["bias_n"]:
        v = bn[:N] + v
    r = residual_of(c, rows)
    if r is not None and row_idx is not None:
        r = r[row_idx]
    bmv = (bm[:M] if row_idx is None else bm[row_idx])[:, None] if c["bias_m"] else None
    if r is not None and bmv is not None:
        v = (r + bmv) + v
    elif r is not None:
        v = r + v
    elif bmv is not None:
        v = bmv + v
    if c["act"] == 1:
        v = 0.5 * v * (1 + torch.erf(v * torch.tensor(2.0 ** -0.5, dtype=torch.float32)))
    return v
