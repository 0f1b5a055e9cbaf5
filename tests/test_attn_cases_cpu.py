"""CPU proof that the attention cases of test_attn_kernels_gpu.py can fail.

For every run of that module: the probe keys carry their share of the
softmax mass, an fp64 walk of the kernel's tiling with the kernel's
roundings stays within half the bound, every applicable defect misses the
bound by DEFECT_FACTOR, and each decode run launches in the regime its
case table entry states.
"""
import pytest
import torch

import attn_cases as ac
from mlx_sharding_amd.ops import reference as ref

DECODE_RUNS = ac.decode_runs()
DECODE_INPUTS = sorted({(c.name, lens) for c, _, lens, _, _ in DECODE_RUNS})
CASES = {c.name: c for c in ac.DECODE_CASES}
PREFILL = ac.PREFILL_CASES + ac.FALLBACK_CASES
# a dropped rescale shows where a later tile raises the running maximum by
# most of the GAP between the probe levels: exp(-0.5)
RESCALED = 0.61


def _run_id(r):
    return f"{r[0].name}-{r[1]}-{'_'.join(map(str, sorted(set(r[2]))))}" \
        f"{'r' if len(set(r[2])) > 1 else ''}"


def _missed(got, want, bound):
    """Worst err / bound of a defective result; rows the defect leaves
    without any key (NaN) do not count."""
    return ac.worst_ratio(torch.nan_to_num(got, nan=0.0) * ~got.isnan()
                          + want * got.isnan(), want, bound)


def _scale_visible(c):
    """A scale of Dv**-0.5 moves every score by the same factor: only the
    GAP between the probe levels changes, by 0.7 * |sqrt(Dk / Dv) - 1|.
    That reaches 4 x bound where the factor is 1.2 or more and no softcap
    flattens it again; the 6% of the 576/512 MLA rows is below what keys
    holding 1/16 of the mass each can show."""
    r = (c.Dk / c.Dv) ** 0.5
    return not c.softcap and max(r, 1 / r) >= 1.2


SEEN = set()


def _assert_defects(found, label):
    assert found, label
    for name, ratio in found.items():
        SEEN.add("drop_tile" if "drop_tile" in name else name)
        print(f"{label} {name}: {ratio:.1f} x bound")
        assert ratio >= ac.DEFECT_FACTOR, (label, name, ratio)


def test_reference_agrees_with_ops_reference():
    c = next(c for c in PREFILL if c.window and c.softcap)
    q, kbuf, vbuf, scale = ac.prefill_inputs(c)
    S = c.offset + c.T
    want, _, _ = ac.prefill_reference(c)
    got = ref.attention(q.float(), kbuf[:, :, :S].float(),
                        vbuf[:, :, :S].float(), scale, causal_offset=c.offset,
                        softcap=c.softcap, sliding_window=c.window)
    assert (got.double() - want).abs().max().item() < 1e-4


# --------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------

@pytest.mark.parametrize("run", DECODE_RUNS, ids=_run_id)
def test_decode_run_launches_in_its_regime(run):
    case, mode, lens, nsplit, tiles = run
    assert (mode == "host") <= (len(set(lens)) == 1)
    assert max(lens) <= case.cap
    got_ns, per = ac.run_launch(case, mode, lens)
    walked = max(len(t) for L in lens
                 for t in ac.decode_slices(L, case.window, got_ns, per))
    assert (got_ns, walked) == (nsplit, tiles)


def test_decode_runs_cover_the_multi_tile_modes():
    """Two or more tiles per block with nsplit == 1, under a host-length
    split and under a device-position split."""
    seen = {(ns == 1, mode == "host") for _, mode, _, ns, tiles in DECODE_RUNS
            if tiles >= 2}
    assert {(True, True), (True, False), (False, True), (False, False)} <= seen


@pytest.mark.parametrize("name,mode", [
    ("ns1_s513", "host"), ("s512_513_g2", "host"), ("s512_513_g2", "ragged"),
    ("cap4k_mla32", "ragged")])
def test_decode_multi_tile_runs_rescale(name, mode):
    """In each multi-tile mode some block really rescales its accumulator,
    so the no_alpha defect is checked there."""
    lens = next(l for c, m, l, _, _ in DECODE_RUNS
                if c.name == name and m == mode)
    alphas = []
    ac.decode_emulation(CASES[name], mode, lens, alphas=alphas)
    assert min(alphas) <= RESCALED


def test_decode_cases_cover_every_instantiation():
    shapes = {(c.Hq // c.Hkv, c.Dk, c.Dv, c.alias) for c in ac.DECODE_CASES}
    assert {g for g, _, dv, _ in shapes if dv <= 256} >= {1, 2, 4, 6, 7, 8, 16, 32}
    assert {g for g, _, dv, al in shapes if dv == 512 and al} >= {4, 16, 32}
    assert {dk for _, dk, _, _ in shapes} >= {64, 72, 80, 128, 192, 576}
    assert any(g == 4 and 256 < dv < 512 for g, _, dv, _ in shapes)


@pytest.mark.parametrize("name,lens", DECODE_INPUTS,
                         ids=[f"{n}-{'_'.join(map(str, l[:3]))}"
                              for n, l in DECODE_INPUTS])
def test_decode_probes_and_defects(name, lens):
    case = CASES[name]
    q, kbuf, vbuf, scale = ac.decode_inputs(name, lens)
    want, ps, bound = ac.decode_reference(case, lens)
    assert torch.isfinite(want).all()
    wider = ac.decode_reference(case, lens, window=case.window + 1)[1]
    for b, L in enumerate(lens):
        keys, outside = ac.decode_probes(case, L)
        assert ps[b][:, keys].min() >= ac.MASS, (b, L, ps[b][:, keys].min(0))
        if outside is not None:
            assert wider[b][:, outside].min() >= ac.MASS, (b, L)
        if case.softcap:  # raw scores on both sides of the cap
            raw = ac.scores(q[b:b + 1], kbuf[b:b + 1, :, keys], scale)
            assert raw.min() < case.softcap < raw.max() or len(keys) == 1

    modes = sorted({m for c, m, l, _, _ in DECODE_RUNS
                    if c.name == name and l == lens and m != "shared"})
    found = {}
    for mode in modes:
        alphas = []
        emu = ac.decode_emulation(case, mode, lens, alphas=alphas)
        ratio = ac.worst_ratio(emu.to(ac.BF16), want, bound)
        print(f"{name} {mode}: rounded walk at {ratio:.3f} x bound")
        assert ratio <= 0.5

        # the tiling defects, on the first row of each length
        nsplit, per = ac.run_launch(case, mode, lens)
        for b in {L: lens.index(L) for L in lens}.values():
            keys, _ = ac.decode_probes(case, lens[b])
            slices = ac.decode_slices(lens[b], case.window, nsplit, per)
            held = [[any(t0 <= j < t1 for j in keys) for t0, t1 in tiles]
                    for tiles in slices]
            row = [b]
            defects = {}
            if sum(map(sum, held)) >= 2:
                for si, tiles in enumerate(held):
                    for ti in [i for i, h in enumerate(tiles) if h]:
                        defects[f"drop_tile{si}.{ti}"] = {"drop_tile": (si, ti)}
            if min(alphas, default=1.0) <= RESCALED:
                defects["no_alpha"] = {"no_alpha": True}
            if sum(any(tiles) for tiles in held) >= 2:
                defects["no_factor"] = {"no_factor": True}
            for dname, kw in defects.items():
                got = ac.decode_emulation(case, mode, lens, rows=row, **kw)
                key = f"{mode} L={lens[b]} {dname}"
                found[key] = _missed(got, want[b:b + 1], bound[b:b + 1])
                if dname in ("no_alpha", "no_factor"):
                    # visible only where a later tile or another slice holds
                    # the larger maximum: one such row suffices
                    found[dname] = max(found.pop(key), found.get(dname, 0.0))

    multi = [L for L in lens if L >= 2 and case.window != 1]
    variants = {}
    if case.softcap:
        variants["no_softcap"] = dict(softcap=0.0)
    if case.window and any(L > case.window for L in lens):
        variants["window+1"] = dict(window=case.window + 1)
    if case.window > 1 and any(L >= case.window for L in lens):
        variants["window-1"] = dict(window=case.window - 1)
    if multi:
        variants["drop_last"] = dict(
            drop_key=lambda L: L - 1 if L in multi else None)
        variants["drop_first"] = dict(
            drop_key=lambda L: (max(0, L - case.window) if case.window else 0)
            if L in multi else None)
    if case.Hkv > 1 and case.Hq > case.Hkv:
        variants["gqa_mod"] = dict(gqa_mod=True)
    if _scale_visible(case) and multi:
        variants["scale_dv"] = dict(scale=case.Dv ** -0.5)
    for vname, kw in variants.items():
        found[vname] = _missed(ac.decode_reference(case, lens, **kw)[0], want,
                               bound)
    if found or max(lens) > 1:
        _assert_defects(found, name)


# --------------------------------------------------------------------------
# prefill
# --------------------------------------------------------------------------

def test_prefill_cases_cover_every_instantiation():
    assert {(c.Dk, c.Dv) for c in ac.PREFILL_CASES} == set(ac.PREFILL_PAIRS)
    assert len(ac.PREFILL_PAIRS) == 12
    grid = {(c.T, c.offset) for c in ac.PREFILL_CASES}
    assert grid >= {(T, o) for T in (1, 15, 16, 17, 64, 65, 130)
                    for o in (0, 1, 31, 32, 64)}
    assert {c.Hq // c.Hkv for c in ac.PREFILL_CASES} >= {1, 2, 8}
    for c in PREFILL:
        assert c.cap > c.offset + c.T
    # a window start past key 0: in a later block, and in the first block
    s_lo = lambda c, q0: max(0, c.offset + q0 - c.window + 1) & ~31
    assert any(c.window and s_lo(c, 0) == 0 and s_lo(c, 128) > 0
               for c in ac.PREFILL_CASES)
    assert any(c.window and s_lo(c, 0) > 0 for c in ac.PREFILL_CASES)


@pytest.mark.parametrize("case", PREFILL, ids=[c.name for c in PREFILL])
def test_prefill_probes_and_defects(case):
    c = case
    q, kbuf, vbuf, scale = ac.prefill_inputs(c)
    S, P = c.offset + c.T, ac._nfeat(c)
    want, p, bound = ac.prefill_reference(c)
    assert torch.isfinite(want).all()
    ok = ac.allowed_keys([c.offset], c.T, S, c.window)[0]          # [T, S]
    marked = torch.zeros(c.T, S, dtype=torch.bool)
    for t in range(c.T):
        for j in ac.prefill_marks(c, t):
            marked[t, j % P::P] = True
    probes = ok & marked
    assert probes[torch.arange(c.T), c.offset + torch.arange(c.T)].all()
    pmin = p.amin((0, 1)).masked_fill(~probes, 1.0)
    assert pmin.min() >= ac.MASS, pmin.min()
    # the keys just outside the mask would carry as much if admitted
    if c.T > 1:
        nxt = ac.prefill_reference(c, d_offset=1)[1].amin((0, 1))
        t = torch.arange(c.T - 1)
        assert nxt[t, c.offset + t + 1].min() >= ac.MASS
    if c.window and S > c.window:
        wider = ac.prefill_reference(c, window=c.window + 1)[1].amin((0, 1))
        t = torch.arange(max(0, c.window - c.offset), c.T)
        assert wider[t, c.offset + t - c.window].min() >= ac.MASS
    if c.softcap and (probes.sum(1) >= 2).any():
        raw = ac.scores(q, kbuf[:, :, :S], scale)                  # [B,k,g,T,S]
        raw = raw[..., probes]
        assert raw.min() < c.softcap < raw.max()

    alphas = []
    emu = ac.prefill_emulation(c, alphas=alphas)
    ratio = ac.worst_ratio(emu.to(ac.BF16), want, bound)
    print(f"{c.name}: rounded walk at {ratio:.3f} x bound")
    assert ratio <= 0.5

    found = {}
    tiles = ac.prefill_slices(S)[0]
    per_tile = torch.stack([probes[:, t0:t1].any(1) for t0, t1 in tiles], 1)
    for ti in range(len(tiles)):
        # visible in a row with a probe in this tile and one in another
        if (per_tile[:, ti] & (per_tile.sum(1) >= 2)).any():
            found[f"drop_tile{ti}"] = _missed(
                ac.prefill_emulation(c, drop_tile=(0, ti)), want, bound)
    if min(alphas, default=1.0) <= RESCALED:
        found["no_alpha"] = _missed(ac.prefill_emulation(c, no_alpha=True),
                                    want, bound)
    variants = {}
    if c.softcap and (probes.sum(1) >= 2).any():
        variants["no_softcap"] = dict(softcap=0.0)
    if c.window and S > c.window:
        variants["window+1"] = dict(window=c.window + 1)
    if c.window > 1 and S >= c.window:
        variants["window-1"] = dict(window=c.window - 1)
    if c.T > 1:
        variants["offset+1"] = dict(d_offset=1)
    if S > 1:
        variants["offset-1"] = dict(d_offset=-1)
    several = ok.sum(1) >= 2                                       # [T]
    if several.any():
        pos = c.offset + torch.arange(c.T)
        last = torch.zeros(c.T, S, dtype=torch.bool)
        last[torch.arange(c.T), pos] = several
        first = torch.zeros(c.T, S, dtype=torch.bool)
        lo = (pos - c.window + 1).clamp(min=0) if c.window else pos * 0
        first[torch.arange(c.T), lo] = several
        variants["drop_last"] = dict(drop=last[None])
        if c.window:
            variants["drop_first"] = dict(drop=first[None])
    if c.Hkv > 1 and c.Hq > c.Hkv:
        variants["gqa_mod"] = dict(gqa_mod=True)
    if _scale_visible(c) and several.any():
        variants["scale_dv"] = dict(scale=c.Dv ** -0.5)
    for vname, kw in variants.items():
        found[vname] = _missed(ac.prefill_reference(c, **kw)[0], want, bound)
    if found or S > 1:
        _assert_defects(found, c.name)


def test_every_defect_is_checked():
    """Each defect of attn_cases.DEFECTS applies to, and is caught in, at
    least one of a few named cases."""
    SEEN.clear()
    for name in ("s512_1025_g2_w600_cap50", "cap4k_g4_dv320"):
        for n, lens in DECODE_INPUTS:
            if n == name:
                test_decode_probes_and_defects(n, lens)
    for c in PREFILL:
        if c.name in ("pf_64x32_g2_T17_o31", "pf_128x128_g2_T130_o64_w40_cap30"):
            test_prefill_probes_and_defects(c)
    assert SEEN == set(ac.DEFECTS), set(ac.DEFECTS) ^ SEEN
