"""fp64 reference and input families of offset-causal attention: what ``pg_prefill_extend`` asks of ``attn_extend_flash_kernel`` (bf16) and of
``attn_kernel`` mode 1 (bf16 / f32).  Row r of a launch already holds slots ``[0, q0[r])``; its ``n_new[r]`` packed queries sit in slots
``q0 .. q0 + n_new - 1`` and query i sees keys ``0 .. q0 + i`` of its own row.

Built on tests/attn_ref.py: the checker, the poison values, the cache generator and -- unchanged -- ``prefill_bound``: the extension kernels have
the rounding points of the prefill kernels (one output rounding; flash: bf16 P in the PV product and the bf16 ``q * scale``), so the reference
returns the same terms (``out``, ``pv_abs``, ``qterm``, ``vmax``) and the bound is the prefill bound of the same path, never a fitted one."""
from __future__ import annotations

import math

import torch

from attn_ref import F64, HD_LLM, POISON_SCORE, POISON_V, TORCH_T, _dominant_key, _scales, f32, make_kv_cache, round_t

# q0 crossed with n_new: every listed value of both axes appears, each tile-boundary q0 with a short, a boundary and a multi-block extension
Q0_NNEW = [(0, 1), (0, 128), (0, 300), (1, 2), (1, 129), (63, 1), (63, 33), (64, 64), (64, 31), (65, 32), (65, 127), (127, 1), (127, 129),
           (128, 128), (128, 2), (200, 300), (200, 33), (831, 1), (831, 64), (831, 129), (831, 31)]
MUTANTS = [("causal", -1), ("causal", +1), ("q0_ignored",), ("neighbour_row",), ("future_key", 2)]


def make_extend_case(seed, dtype, nh, rows=None, aliased_row=3, needle=False):
    """One packed extension launch.  rows: (q0, n_new) per row; row ``aliased_row`` is inserted with row_off = -1 (no packed token).  Slots
    >= q0 + n_new of every row and every slot of the aliased row hold the poison keys (attn_ref.POISON_*).  needle: q_i = h_i and
    k_{q0 + i + 1} = 3 h_i (h_i a random +-1 vector): the first key in every query's future dominates, so a mask that is off by one moves the
    output by a large fraction of |v|."""
    g = torch.Generator().manual_seed(seed)
    rows = list(rows or Q0_NNEW)
    if aliased_row is not None:
        rows.insert(aliased_row, (50, 7))
    R = len(rows)
    q0 = [a for a, _ in rows]
    n_new = [b for _, b in rows]
    lens = [a + b for a, b in rows]
    slots = max(lens) + 1 + 31
    row_off, tok_row, tok_j, n = [], [], [], 0
    for r, (a, b) in enumerate(rows):
        if r == aliased_row:
            row_off.append(-1)
            continue
        row_off.append(n)
        tok_row += [r] * b
        tok_j += list(range(a, a + b))
        n += b
    Ntok = n
    kc, vc = make_kv_cache(g, R, nh, slots, dtype)
    qs = _scales(g, (1, nh, HD_LLM), 0.3, 1.7).float()
    q = (torch.randn(Ntok, nh, HD_LLM, generator=g) * qs).to(TORCH_T[dtype])
    scale = 1.0 / math.sqrt(HD_LLM)
    if needle:
        for r, (off, (a, b)) in enumerate(zip(row_off, rows)):
            if off < 0:
                continue
            h = torch.randint(0, 2, (b, nh, HD_LLM), generator=g).float() * 2 - 1
            q[off:off + b] = h.to(TORCH_T[dtype])
            kc[r, :, a + 1:a + b + 1] = (3 * h).transpose(0, 1).to(TORCH_T[dtype])
    for r, (off, L) in enumerate(zip(row_off, lens)):
        lo = 0 if off < 0 else L
        qd = q[off + n_new[r] - 1].to(F64) if off >= 0 else q[0].to(F64)
        kc[r, :, lo:] = _dominant_key(qd, POISON_SCORE, scale, dtype)[:, None]
        vc[r, :, lo:] = POISON_V + torch.arange(HD_LLM, dtype=torch.float32)[None, None] / 8
    return {"q": q, "kc": kc, "vc": vc, "row_off": row_off, "q0": q0, "n_new": n_new, "len": lens, "tok_row": tok_row, "tok_j": tok_j, "R": R,
            "max_new": max(b for r, (_, b) in enumerate(rows) if r != aliased_row), "Ntok": Ntok, "nh": nh, "slots": slots, "scale": scale,
            "dtype": dtype}


def extend_ref(p, dtype, flash, mut=None):
    """Reference of one packed extension launch.  flash: the kernel rounds q * scale to bf16 (qterm).  mut (what a wrong kernel would do):
    ("causal", +-1) shifts the mask, ("q0_ignored",) masks as if the row were empty, ("neighbour_row",) takes key q0 from the next row,
    ("future_key", d) also sees key q0 + i + d.  Returns out [Ntok, nh, 128], pv_abs, qterm, vmax [Ntok, nh] -- the terms of
    attn_ref.prefill_bound."""
    mut = mut or (None,)
    q, kc, vc = p["q"].to(F64), p["kc"], p["vc"]
    Ntok, nh = q.shape[0], p["nh"]
    scale = torch.tensor(p["scale"], dtype=torch.float32).item()
    out = torch.zeros(Ntok, nh, HD_LLM, dtype=F64)
    pv_abs, qterm = torch.zeros_like(out), torch.zeros_like(out)
    vmax = torch.zeros(Ntok, nh, dtype=F64)
    for r, (off, a, b) in enumerate(zip(p["row_off"], p["q0"], p["n_new"])):
        if off < 0:
            continue
        reach = {"causal": max(mut[1], 0) if mut[0] == "causal" else 0, "future_key": mut[1] if mut[0] == "future_key" else 0}
        n = min(a + b + max(reach.values()), kc.shape[2])
        K = kc[r, :, :n].to(F64)
        V = vc[r, :, :n].to(F64)
        if mut[0] == "neighbour_row":
            K = K.clone(); V = V.clone()
            K[:, a] = kc[(r + 1) % p["R"], :, a].to(F64)
            V[:, a] = vc[(r + 1) % p["R"], :, a].to(F64)
        qr = q[off:off + b].transpose(0, 1)                          # [nh, n_new, 128]
        i = torch.arange(b)[:, None]
        t = torch.arange(n)[None, :]
        if mut[0] == "q0_ignored":
            mask = t <= i
        else:
            mask = t <= a + i + (mut[1] if mut[0] == "causal" else 0)
            mask[:, 0] = True                                        # ("causal", -1) at q0 = 0: query 0 still needs a key
        if mut[0] == "future_key":
            mask = mask | (t == a + i + mut[1])

        def attn(qq):
            s = torch.einsum("hld,hnd->hln", qq, K).masked_fill(~mask, float("-inf"))
            pi = torch.softmax(s, dim=-1)
            return torch.einsum("hln,hnd->hld", pi, V), pi
        qsc = f32(qr * scale)
        o, pi = attn(qsc)
        out[off:off + b] = o.transpose(0, 1)
        pv_abs[off:off + b] = torch.einsum("hln,hnd->hld", pi, V.abs()).transpose(0, 1)
        if flash:
            o2, _ = attn(round_t(qsc, "bf16"))
            qterm[off:off + b] = (o2 - o).abs().transpose(0, 1)
        vmax[off:off + b] = V.abs().amax(dim=(1, 2))[None, :]
    return {"out": out, "pv_abs": pv_abs, "qterm": qterm, "vmax": vmax}


def as_prefill_case(p):
    """The q0 = 0 rows of an extension case as a packed PREFILL launch on the same buffers (every other row gets row_off = -1): what
    attn_prefill_flash2_kernel must reproduce bit for bit."""
    keep = [off >= 0 and a == 0 for off, a in zip(p["row_off"], p["q0"])]
    d = dict(p)
    d["row_off"] = [off if k else -1 for off, k in zip(p["row_off"], keep)]
    d["len"] = [b if k else 0 for b, k in zip(p["n_new"], keep)]
    d["max_len"] = max(d["len"])
    return d
