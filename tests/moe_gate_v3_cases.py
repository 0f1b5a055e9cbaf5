"""Shared inputs for the sigmoid (DeepSeek-V3 noaux_tc) gate tests.

Logits come from moe_gate_cases.make_logits (exact in bf16, distinct per
row).  The per-expert selection bias is seeded fp32 in [-1.5, 0.5], so some
biased scores c = sigmoid(logit) + bias fall below -1 — the value the
softmax gate uses as its "masked" sentinel.

Every decision the gate takes must be clear of a near tie, so that a
fast-exp sigmoid (relative error ~1e-6) cannot legitimately change it and
the GPU test can demand the exact index sets.  For every row, in fp32
torch, each of these gaps is >= MIN_GAP:
  * the K-th vs the (K+1)-th biased score among the kept experts,
  * the topk_group-th vs the next group score,
  * the second vs the third biased score of every group that has three.
The seeds below were searched on the CPU (find_seeds) so that this holds;
the module asserts it at import.
"""

import torch

from moe_gate_cases import make_logits

MIN_GAP = 1e-4

# (N, E, n_group, topk_group, K, norm_topk, scaling, max_tok)
GRID = [
    (33, 256, 8, 4, 8, True, 2.5, 16),     # the V3 shape
    (128, 256, 8, 4, 8, True, 2.5, 16),    # every limit at once
    (7, 96, 8, 3, 4, True, 2.5, 4),        # E tail, 12-wide groups
    (5, 64, 32, 16, 8, False, 1.0, 16),    # groups of exactly 2
    (3, 128, 1, 1, 6, False, 1.0, 4),      # ungrouped
    (16, 160, 16, 16, 6, True, 1.0, 16),   # all groups kept
    (5, 64, 8, 3, 6, True, 2.5, 16),       # R = 1
]

GRID_IDS = ["N%d-E%d-g%d/%d-K%d" % c[:5] for c in GRID]

# (logits seed, bias seed) per grid entry, from find_seeds()
SEEDS = [(0, 2), (0, 2), (0, 0), (0, 0), (0, 0), (0, 1), (0, 0)]

# the grid entry that is also run with an all-zero bias
ZERO_BIAS_ENTRY = 0
ZERO_BIAS_LOGITS_SEED = 2


def make_bias(E: int, seed: int) -> torch.Tensor:
    """[E] fp32 selection bias in [-1.5, 0.5]; deterministic in (E, seed)."""
    g = torch.Generator().manual_seed(7000 * seed + E)
    return torch.rand(E, generator=g, dtype=torch.float32) * 2.0 - 1.5


def min_gap(case, logits: torch.Tensor, bias: torch.Tensor) -> float:
    """Smallest of the three decision gaps over all rows (fp32 torch)."""
    N, E, n_group, topk_group, K = case[:5]
    s = torch.sigmoid(logits.float())
    c = s + bias
    gaps = []
    if n_group > 1:
        gsz = E // n_group
        cg = c.reshape(N, n_group, gsz).sort(dim=-1, descending=True).values
        if gsz >= 3:
            gaps.append((cg[..., 1] - cg[..., 2]).min())
        gscore = (cg[..., 0] + cg[..., 1]).sort(dim=-1, descending=True)
        if topk_group < n_group:
            gaps.append((gscore.values[:, topk_group - 1]
                         - gscore.values[:, topk_group]).min())
        keep = torch.zeros(N, n_group, dtype=torch.bool)
        keep.scatter_(1, gscore.indices[:, :topk_group], True)
        mask = keep[:, :, None].expand(N, n_group, gsz).reshape(N, E)
        c = c.masked_fill(~mask, float("-inf"))
    cs = c.sort(dim=-1, descending=True).values
    gaps.append((cs[:, K - 1] - cs[:, K]).min())  # -inf next: gap = +inf
    return float(torch.stack(gaps).min())


def case_inputs(i: int, zero_bias: bool = False):
    """(case, logits [N, E] bf16, e_bias [E] fp32) for grid entry i."""
    case = GRID[i]
    N, E = case[:2]
    if zero_bias:
        return (case, make_logits(N, E, ZERO_BIAS_LOGITS_SEED),
                torch.zeros(E, dtype=torch.float32))
    ls, bs = SEEDS[i]
    return case, make_logits(N, E, ls), make_bias(E, bs)


def find_seeds(limit: int = 4000):
    """CPU search for SEEDS / ZERO_BIAS_LOGITS_SEED (run by hand when the
    grid changes)."""
    found = []
    for case in GRID:
        N, E = case[:2]
        hit = None
        for n in range(limit):
            ls, bs = n // 50, n % 50
            if min_gap(case, make_logits(N, E, ls), make_bias(E, bs)) >= MIN_GAP:
                hit = (ls, bs)
                break
        found.append(hit)
    case = GRID[ZERO_BIAS_ENTRY]
    zero = next((ls for ls in range(limit)
                 if min_gap(case, make_logits(case[0], case[1], ls),
                            torch.zeros(case[1])) >= MIN_GAP), None)
    return found, zero


ALL_INPUTS = [(i, False) for i in range(len(GRID))] + [(ZERO_BIAS_ENTRY, True)]
ALL_IDS = GRID_IDS + [GRID_IDS[ZERO_BIAS_ENTRY] + "-zero-bias"]

for _i, _zero in ALL_INPUTS:
    _case, _logits, _bias = case_inputs(_i, _zero)
    _gap = min_gap(_case, _logits, _bias)
    assert _gap >= MIN_GAP, (
        f"near tie in gate case {ALL_IDS[ALL_INPUTS.index((_i, _zero))]}: "
        f"min gap {_gap:.3e} < {MIN_GAP}")
