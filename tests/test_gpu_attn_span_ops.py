"""pg_op_attn_span_mass (csrc/attn_span.hip) against the fp64 reference and bound of tests/span_ref.py: nh = 2, head_dim 128, rows of 1, 63,
64, 65, 130 and 200 tokens in one packed batch with a different pad_len each; every span kind, 1 and 16 spans, a single query in the middle
of a tile, every column and a run across tiles; flat, peaked and large-magnitude scores; canaries, repeatability, the partition sum."""
import numpy as np
import pytest
import torch

import span_ref as SP
from conftest import get_engine

pytestmark = pytest.mark.gpu

QUERY_SETS = [(100, 1), (0, SP.FRAME), (100, 70)]
_REF = {}


def _case(family, q_col0, n_q, n_spans, partition=False):
    key = (family, q_col0, n_q, n_spans, partition)
    if key not in _REF:
        c = SP.make_case(family, q_col0, n_q, n_spans, partition=partition)
        _REF[key] = (c,) + SP.span_mass_ref(c)
    return _REF[key]


def _run(e, c):
    q = torch.from_numpy(c["q"]).reshape(c["q"].shape[0], -1).bfloat16()
    k = torch.from_numpy(c["k"]).bfloat16()
    return e.attn_span_mass(q, k, c["row_off"], c["length"], c["pad"], c["lo"], c["hi"], c["q_col0"], c["n_q"], c["scale"])


@pytest.mark.parametrize("family", SP.FAMILIES)
@pytest.mark.parametrize("q_col0,n_q", QUERY_SETS)
@pytest.mark.parametrize("n_spans", [1, 16])
def test_against_reference(tiny_cfg, tiny_weights, family, q_col0, n_q, n_spans):
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    c, A, bound = _case(family, q_col0, n_q, n_spans)
    got = _run(e, c).cpu().numpy()
    assert got.shape == A.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err, frac, exact = SP.worst(got, A, bound)
    print(f"{family} q_col0={q_col0} n_q={n_q} S={n_spans}: max |A - A64| = {err:.3e}, error / bound = {frac:.3f}, bound <= {bound.max():.3e}")
    assert frac <= 1.0 and exact          # exact: pad queries are exactly 0


def test_large_family_needs_the_rescale(tiny_cfg, tiny_weights):
    """The large-magnitude family raises the running maximum in every later tile: the arithmetic model WITHOUT the rescale of the span sum
    misses the bound there by far, the kernel does not."""
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    c, A, bound = _case("large", 0, SP.FRAME, 16)
    _, frac_bad, _ = SP.worst(SP.span_mass_emulated(c, "no_rescale"), A, bound)
    _, frac, exact = SP.worst(_run(e, c).cpu().numpy(), A, bound)
    assert frac_bad >= 100.0 and frac <= 1.0 and exact


def test_output_between_canaries_and_repeatable(tiny_cfg, tiny_weights):
    import ctypes as C
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    c, A, bound = _case("peaked", 100, 70, 16)
    R, n_q, S = A.shape
    q = torch.from_numpy(c["q"]).reshape(c["q"].shape[0], -1).bfloat16().cuda()
    k = torch.from_numpy(c["k"]).bfloat16().cuda()
    dv = [torch.from_numpy(np.ascontiguousarray(c[n], dtype=np.int32)).cuda() for n in ("row_off", "length", "pad", "lo", "hi")]
    outs = []
    for _ in range(2):
        buf = torch.full((64 + R * n_q * S + 64,), -7.5, dtype=torch.float32, device="cuda")
        out = buf[64:64 + R * n_q * S]
        rc = e.lib.pg_op_attn_span_mass(e.h, e._p(q), e._p(k), *[e._p(t) for t in dv], R, c["nh"], c["slots"], S, c["q_col0"], n_q,
                                        C.c_float(c["scale"]), C.c_void_p(out.data_ptr()), e.stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert (buf[:64] == -7.5).all() and (buf[-64:] == -7.5).all()
        outs.append(out.clone().cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))          # two launches: the same bits
    _, frac, exact = SP.worst(outs[0].numpy().reshape(A.shape), A, bound)
    assert frac <= 1.0 and exact


@pytest.mark.parametrize("family", SP.FAMILIES)
def test_partition_sums_to_one(tiny_cfg, tiny_weights, family):
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    c, A, bound = _case(family, 0, SP.FRAME, 16, partition=True)
    got = _run(e, c).cpu().numpy().astype(np.float64)
    S = got.shape[-1]
    for r in range(got.shape[0]):
        p = int(c["pad"][r])
        assert (got[r, :p] == 0).all()                                              # pad queries: exactly zero
        dev = np.abs(got[r, p:].sum(-1) - 1.0)
        assert (dev <= S * bound[r, p:]).all(), (family, r, float(dev.max()))


def test_refusals(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    c, _, _ = _case("flat", 100, 1, 1)
    q = torch.from_numpy(c["q"]).reshape(c["q"].shape[0], -1).bfloat16()
    k = torch.from_numpy(c["k"]).bfloat16()
    lo17 = np.zeros((len(c["length"]), 17), dtype=np.int32)
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.attn_span_mass(q, k, c["row_off"], c["length"], c["pad"], lo17, lo17, 0, 1)
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.attn_span_mass(q, k, c["row_off"], c["length"], c["pad"], c["lo"], c["hi"], 0, 0)
    with pytest.raises(PlanGenError, match="slots"):
        e.attn_span_mass(q, k, c["row_off"], c["length"] + 100, c["pad"], c["lo"], c["hi"], 0, 1)
    f = get_engine(tiny_cfg, tiny_weights, "f32")
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        f.attn_span_mass(q, k, c["row_off"], c["length"], c["pad"], c["lo"], c["hi"], 0, 1)
