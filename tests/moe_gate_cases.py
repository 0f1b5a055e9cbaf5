"""Shared inputs for the fused MoE gating tests (CPU sanity + GPU).

Row t of the logits is a seeded random permutation of
(arange(E) - E//2) / 32.  For E <= 256 every value is exact in bf16
(|k| <= 128 fits the 8-bit significand), all values in a row are distinct
and neighbours differ by ~3% in probability, so there is no expert or
group tie and a correct gate must select exactly reference.moe_gate's set.
"""

import torch

# (N, E, n_group, topk_group, K, norm_topk, scaling, max_tok)
GRID = [
    (5, 64, 8, 3, 6, False, 1.0, 16),      # groups inside one register
    (33, 160, 8, 3, 6, False, 16.0, 16),   # V2 shape, E tail, 20-wide groups
    (7, 96, 8, 3, 4, False, 16.0, 4),      # debug-deepseek-grouped
    (9, 72, 4, 1, 8, True, 1.0, 16),       # one kept group, K limit, norm
    (128, 256, 8, 4, 8, True, 2.5, 16),    # every limit at once
    (3, 128, 1, 1, 6, False, 1.0, 4),      # ungrouped greedy, E > 64
    (16, 160, 16, 16, 6, False, 1.0, 16),  # all groups kept
]

GRID_IDS = ["N%d-E%d-g%d/%d-K%d" % c[:5] for c in GRID]


def make_logits(N: int, E: int, seed: int = 0) -> torch.Tensor:
    """[N, E] bf16 logits on the CPU; deterministic in (N, E, seed)."""
    g = torch.Generator().manual_seed(1000 * seed + E)
    base = (torch.arange(E, dtype=torch.float32) - E // 2) / 32.0
    rows = [base[torch.randperm(E, generator=g)] for _ in range(N)]
    out = torch.stack(rows).to(torch.bfloat16)
    assert torch.equal(out.float(), torch.stack(rows)), "not exact in bf16"
    return out
