"""ops.moe_route on CPU tensors (reference.moe_route, the specification of
the fused prefill route) against reference.moe_gate followed by
ops.make_expert_subranges, field by field."""

import pytest
import torch

from moe_gate_cases import make_logits
from moe_gate_v3_cases import make_bias

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

# (N, E, n_group, topk_group, K, norm, scaling, max_tok, scoring, wt_bf16)
CASES = [
    (129, 64, 1, 1, 6, False, 1.0, 16, "softmax", False),
    (333, 160, 8, 3, 6, False, 16.0, 64, "softmax", True),
    (70, 256, 8, 4, 8, True, 2.5, 4, "sigmoid", False),
]


def gate_picks(logits, case, e_bias=None):
    """(weights, indices) of reference.moe_gate for the case."""
    N, E, n_group, topk_group, K, norm, scaling, max_tok, scoring, bf = case
    w, idx = ref.moe_gate(logits.float(), K, n_group, topk_group, scaling,
                          norm, scoring=scoring, e_bias=e_bias)
    return (w.to(torch.bfloat16).float() if bf else w), idx


def subranges_of(idx, w, E, max_tok):
    """The sort fields from make_expert_subranges + bincount; `order` last.
    make_expert_subranges leaves stale expert and offset values in its dead
    (cnt == 0) slots, the route zeroes them."""
    sub_e, sub_off, sub_cnt, sorted_tok, sorted_wt, order = \
        ops.make_expert_subranges(idx, w, E, max_tok)
    live = sub_cnt > 0
    counts = torch.bincount(idx.flatten().long(), minlength=E)
    starts = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    return (counts, starts, sub_e * live, sub_off * live, sub_cnt, sorted_tok,
            sorted_wt, order)


def check_sort_fields(r, idx, w, E):
    """Every field of route r behind indices / weights, for picks idx, w."""
    (counts, starts, sub_e, sub_off, sub_cnt, sorted_tok, sorted_wt,
     order) = subranges_of(idx, w, E, r.max_tok)
    P = idx.numel()
    assert torch.equal(r.counts.long(), counts)
    assert torch.equal(r.starts.long(), starts)
    assert r.max_count.tolist() == [int(counts.max())]
    assert torch.equal(r.sorted_tok, sorted_tok)
    assert torch.equal(r.sorted_e.long(), idx.flatten().long()[order])
    assert torch.equal(r.sorted_wt, sorted_wt)  # bit-equal: both fp32
    assert torch.equal(r.pair_pos.flatten().long()[order], torch.arange(P))
    assert torch.equal(r.sub_expert, sub_e)
    assert torch.equal(r.sub_off, sub_off)
    assert torch.equal(r.sub_cnt, sub_cnt)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-E%d-%s" % (
    c[0], c[1], c[8]))
def test_cpu_route_is_gate_plus_subranges(case):
    N, E, n_group, topk_group, K, norm, scaling, max_tok, scoring, bf = case
    logits = make_logits(N, E)
    e_bias = make_bias(E, 1) if scoring == "sigmoid" else None
    r = ops.moe_route(logits, K, n_group, topk_group, scaling, norm, max_tok,
                      scoring=scoring, e_bias=e_bias, wt_bf16=bf)
    w, idx = gate_picks(logits, case, e_bias)
    assert r.max_tok == max_tok
    assert torch.equal(r.indices.long(), idx)
    assert torch.equal(r.weights, w)
    check_sort_fields(r, idx, w, E)
