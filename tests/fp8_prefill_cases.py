"""Sub-range plans for the wide-tile FP8 MoE prefill kernels
(moe_fp8f16_gateup_wide, moe_fp8f16_down_wide), built from the kernels'
tile TM.  The weights, activations, budgets and references are those of
fp8_cases.py / quant_cases.py; CPU sanity in test_fp8_prefill_cpu.py, GPU
in test_fp8_prefill_gpu.py.

wide_a (N = 2 TM + 26 tokens, E = 3, expert 1 unused):
    expert 0: sub-ranges of TM and 1 tokens        (a full tile, a 1-token tail)
    a padded cnt = 0 slot, then 3 sorted rows outside every sub-range
    expert 2: sub-ranges of TM - 1, TM and 17 tokens
    a trailing padded slot
wide_b: the same sorted rows, expert 2 as ONE sub-range of 2 TM + 16 tokens
    that the kernel has to walk tile by tile (two full tiles and a 16-token
    tail).
Expert 0's tokens are the head of one seeded permutation of the first N - 2
tokens and expert 2's the head of another, so token order is not monotone,
most of expert 0's tokens go to both experts, and the last two tokens are
routed nowhere.

The fp32 exactness budget of fp8_cases.down_case is per output element
(at most two experts per token), so it does not depend on TM;
test_fp8_prefill_cpu.py asserts it for TM = 64 and 128 anyway.
"""

import torch

import fp8_cases as fc
import quant_cases as qc

TMS = (64, 128)
PLAN_NAMES = ("wide_a", "wide_b")
_plans = {}


def plans(TM: int):
    """{"wide_a": plan_d, "wide_b": plan_d} for tile TM."""
    if TM not in _plans:
        N = 2 * TM + 26
        e0 = torch.randperm(N - 2, generator=qc._gen(TM, 1)).tolist()[:TM + 1]
        e2 = torch.randperm(N - 2, generator=qc._gen(TM, 2)) \
            .tolist()[:2 * TM + 16]
        head = [(0, e0[:TM]), (0, e0[TM:]), (1, []), ("gap", 3)]
        a = head + [(2, e2[:TM - 1]), (2, e2[TM - 1:2 * TM - 1]),
                    (2, e2[2 * TM - 1:]), (0, [])]
        b = head + [(2, e2), (0, [])]
        _plans[TM] = {"wide_a": dict(N=N, plan=a), "wide_b": dict(N=N, plan=b)}
        assert [len(t) for e, t in a if e != "gap"] == \
            [TM, 1, 0, TM - 1, TM, 17, 0]
        assert len(set(e0) & set(e2)) > TM // 2
    return _plans[TM]


def subrange_rows(plan):
    """[(expert, [sorted rows], [tokens])] of the non-empty sub-ranges."""
    out, p = [], 0
    for e, toks in plan:
        if e == "gap":
            p += toks
            continue
        if toks:
            out.append((e, list(range(p, p + len(toks))), list(toks)))
        p += len(toks)
    return out


# --------------------------------------------------------------------------
# gate-up: the closed forms of quant_cases.gateup_expected for a whole
# offset sweep at once (that helper forms two [P, I, H] einsums per offset)
# --------------------------------------------------------------------------

def gateup_expected_sweep(kind, Wg64, Wu64, plan_d, H, offs, out_dtype):
    """h64 [len(offs), P, I]: live sorted rows per quant_cases constructions
    (a) / (b), other rows 0, with gateup_expected's exactness preconditions
    asserted on every offset."""
    pairs = qc.plan_pairs(plan_d["plan"])
    P = qc.build_subranges(plan_d["plan"])[1].numel()
    rows = torch.tensor([p for p, _, _ in pairs])
    es = torch.tensor([e for _, e, _ in pairs])
    ts = torch.tensor([t for _, _, t in pairs])
    h = torch.zeros(len(offs), P, Wg64.shape[1], dtype=torch.float64)
    for n, off in enumerate(offs):
        ks = qc.gateup_cols(plan_d["N"], H, off)[ts]
        assert int(ks.min()) >= 1  # x is 1 at column 0 and at ks, else 0
        gv = Wg64[es, :, 0] + Wg64[es, :, ks]
        uv = Wu64[es, :, 0] + Wu64[es, :, ks]
        if kind == "a":
            assert torch.all(gv == 32)
            live = 32.0 * uv
        else:
            assert torch.all(uv == 1) and gv.min() >= 17 and gv.max() < 2048
            assert torch.equal(gv, gv.round())
            live = gv
        true = gv / (1.0 + torch.exp(-gv)) * uv
        assert torch.equal(true.to(out_dtype), live.to(out_dtype))
        h[n, rows] = live
    assert qc._roundtrip(h, out_dtype), "h does not fit the output format"
    return h


def gateup_x_sweep(plan_d, H, offs, dead):
    """fp64 [len(offs), N, H] gate-up inputs, dead tokens' rows NaN."""
    return torch.stack([qc.poison_rows(qc.gateup_x(plan_d["N"], H, o), dead)
                        for o in offs])


# --------------------------------------------------------------------------
# down: emulation of the kernels' declared arithmetic over a plan, with the
# two slips a tiled walk can make
# --------------------------------------------------------------------------

def emulate_down(codes, s, h64, plan_d, TM: int, slip=None):
    """fp32 [N, H]: per sub-range fc.emulate_moe_linear on the fp16 rows,
    then out[tok] += wt * acc in fp32.

    slip="drop_row_tm": a walked sub-range loses its row TM (the first row
        of its second tile);
    slip="clamp_tail": the lanes of a tail tile past cnt, which load the
        clamped last row, scatter it too instead of being masked."""
    subs, _ = qc.build_subranges(plan_d["plan"])
    wt = subs[4]
    out = torch.zeros(plan_d["N"], codes.shape[1], dtype=torch.float32)
    for e, rows, toks in subrange_rows(plan_d["plan"]):
        acc = fc.emulate_moe_linear(h64[rows].to(torch.float16),
                                    fc.to_fp8(codes[e]), s[e])
        todo = list(range(len(rows)))
        if slip == "drop_row_tm" and len(rows) > TM:
            todo.remove(TM)
        if slip == "clamp_tail" and len(rows) % 16:
            todo += [len(rows) - 1] * (16 - len(rows) % 16)
        for i in todo:
            out[toks[i]] += wt[rows[i]] * acc[i]
    return out


# --------------------------------------------------------------------------
# random data on wide_a: the bounds of fp8_cases.random_gateup_ref /
# random_down_ref, re-evaluated for this plan
# --------------------------------------------------------------------------

def random_case(plan_d, seed: int = 0):
    mats = {n: fc.random_weight(fc.BUDGET_O, fc.BUDGET_K, fc.E, seed + i)
            for i, n in enumerate(("gate", "up", "down"))}
    g = torch.Generator().manual_seed(seed + 17)
    P = qc.build_subranges(plan_d["plan"])[1].numel()
    x = torch.randn(plan_d["N"], fc.BUDGET_K, generator=g).to(torch.float16)
    hh = torch.randn(P, fc.BUDGET_K, generator=g).to(torch.float16)
    return mats, x, hh


def random_down_ref(mats, hh, plan_d):
    """(ref64, bound) [N, O]; fp32 out."""
    W = mats["down"][2]
    wt = qc.build_subranges(plan_d["plan"])[0][4].double()
    ref64 = torch.zeros(plan_d["N"], W.shape[1], dtype=torch.float64)
    A = torch.zeros_like(ref64)
    for e, rows, toks in subrange_rows(plan_d["plan"]):
        h = hh[rows].double()
        w = wt[rows][:, None]
        ref64.index_add_(0, torch.tensor(toks), w * (h @ W[e].t()))
        A.index_add_(0, torch.tensor(toks), w * (h.abs() @ W[e].abs().t()))
    # one more rounding per pair for wt * acc and the atomic add
    return ref64, fc.acc_bound(A, fc.BUDGET_K) + 4 * fc.U_ACC * A


def random_gateup_ref(mats, x, plan_d):
    """(ref64, bound) [P, O]; fp16 out."""
    Wg, Wu = mats["gate"][2], mats["up"][2]
    P = qc.build_subranges(plan_d["plan"])[1].numel()
    ref64 = torch.zeros(P, Wg.shape[1], dtype=torch.float64)
    bound = torch.ones_like(ref64)
    for e, rows, toks in subrange_rows(plan_d["plan"]):
        xt = x[toks].double()
        g64, u64 = xt @ Wg[e].t(), xt @ Wu[e].t()
        Bg = fc.acc_bound(xt.abs() @ Wg[e].abs().t(), fc.BUDGET_K)
        Bu = fc.acc_bound(xt.abs() @ Wu[e].abs().t(), fc.BUDGET_K)
        silu = g64 / (1.0 + torch.exp(-g64))
        ref64[rows] = silu * u64
        bound[rows] = (fc.U_FP16 * ref64[rows].abs() + 2.0 ** -25
                       + 1.1 * Bg * u64.abs() + silu.abs() * Bu
                       + 1.1 * Bg * Bu)
    return ref64, bound
