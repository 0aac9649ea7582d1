"""fp64 references for the top-k / top-p image-token sampler (pg_decode_image_tokens_filtered, pg_op_sample_filter): the
transformers warpers (TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper) and the rule the header states, plus the
test that flags rows where fp32 device arithmetic and an fp64 reference may legitimately disagree.  No GPU import here."""
import torch

TOPP_MARGIN = 1e-4


def hf_keep(logits: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    """bool [N, V]: entries the installed transformers warpers leave finite, applied in float64."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    x = TemperatureLogitsWarper(float(temperature))(None, logits.double().reshape(-1, logits.shape[-1]))
    if top_k > 0:
        x = TopKLogitsWarper(int(top_k))(None, x)
    if top_p < 1.0:
        x = TopPLogitsWarper(float(top_p))(None, x)
    return torch.isfinite(x)


def _x32(logits: torch.Tensor, temperature: float) -> torch.Tensor:
    """x = mixed * (1 / T) in fp32 as the device forms it; NaN -> -inf."""
    inv = torch.tensor(1.0 / temperature, dtype=torch.float32) if temperature > 0 else torch.tensor(1.0)
    x = logits.float().reshape(-1, logits.shape[-1]) * inv
    return torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)


def _topk_keep(x: torch.Tensor, top_k: int) -> torch.Tensor:
    V = x.shape[-1]
    if top_k <= 0 or top_k >= V:
        return torch.ones_like(x, dtype=torch.bool)
    kth = torch.sort(x, dim=-1, descending=True).values[:, top_k - 1:top_k]
    return x >= kth


def _weights(x: torch.Tensor, keep_k: torch.Tensor) -> torch.Tensor:
    xd = x.double()
    m = torch.where(keep_k, xd, torch.full_like(xd, float("-inf"))).max(dim=-1, keepdim=True).values
    w = torch.exp(xd - m)
    inf_max = torch.isinf(m) & (m > 0)
    w = torch.where(inf_max, (xd == float("inf")).double(), w)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return torch.where(keep_k, w, torch.zeros_like(w))


def _mass_above(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[N, V]: sum of w over entries with a strictly larger x (ties excluded)."""
    order = torch.sort(x, dim=-1, descending=True)
    xs, ws = order.values, torch.gather(w, 1, order.indices)
    cum = torch.cumsum(ws, dim=-1) - ws                         # mass before each sorted position
    # first position of each run of equal values: the mass strictly above that value
    first = torch.ones_like(xs, dtype=torch.bool)
    first[:, 1:] = xs[:, 1:] != xs[:, :-1]
    idx = torch.arange(xs.shape[1]).expand_as(xs)
    start = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), dim=-1).values
    above_sorted = torch.gather(cum, 1, start)
    out = torch.empty_like(above_sorted)
    out.scatter_(1, order.indices, above_sorted)
    return out


def rule_keep(logits: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    """bool [N, V]: the header's rule on the fp32 x the device uses (ties at either threshold kept, -inf / NaN never)."""
    x = _x32(logits, temperature)
    keep = _topk_keep(x, top_k)
    if top_p < 1.0:
        w = _weights(x, keep)
        Z = w.sum(-1, keepdim=True)
        keep = keep & (_mass_above(x, w) < top_p * Z)
    return keep & (x > float("-inf"))


def ambiguous(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, margin: float = TOPP_MARGIN) -> torch.Tensor:
    """bool [N, V]: entries whose membership fp32 device arithmetic and an fp64 reference may legitimately decide differently --
    within two ulps of a k-th value that has a distinct neighbour within two ulps (or is itself distinct from it), or a top-k
    survivor below the top value whose strictly-larger mass fraction is within ``margin`` of top_p."""
    x = _x32(logits, temperature)
    N, V = x.shape
    amb = torch.zeros(N, V, dtype=torch.bool)
    if 0 < top_k < V:
        xs = torch.sort(x, dim=-1, descending=True).values
        kth, nxt = xs[:, top_k - 1:top_k], xs[:, top_k:top_k + 1]
        ulp2 = 2 * (torch.nextafter(kth, torch.full_like(kth, float("inf"))) - kth)
        near = (x - kth).abs() <= ulp2
        amb |= near & ((x != kth) | ((kth != nxt) & ((kth - nxt) <= ulp2)))
    if top_p < 1.0:
        keep = _topk_keep(x, top_k)
        w = _weights(x, keep)
        frac = _mass_above(x, w) / w.sum(-1, keepdim=True)
        amb |= keep & (frac > 0) & ((frac - top_p).abs() < margin)          # frac 0: the top value, always kept
    return amb
