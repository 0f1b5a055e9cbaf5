"""attn_decode, attn_prefill and the composed prefill path against the fp64
reference on the probe cases of attn_cases.py, within 2**-7 * max|V| per
(batch row, kv head).  Cache rows at or beyond a row's length are NaN in K
and V.  test_attn_cases_cpu.py proves on the CPU that these cases fail for
a kernel with a wrong mask, softcap, tiling, GQA map or scale."""
import pytest
import torch

import attn_cases as ac
from mlx_sharding_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ext = ops.hip_ext


def _poisoned(buf, lens):
    """Device copy of a cache with NaN in every row past each length."""
    d = buf.to(DEV).clone()
    for b, L in enumerate(lens):
        d[b, :, L:] = float("nan")
    return d


def _check(label, got, want, bound):
    got = got.float().cpu()
    assert torch.isfinite(got).all(), label
    ratio = ac.worst_ratio(got, want, bound)
    print(f"{label}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, (label, ratio)


@pytest.mark.parametrize(
    "run", ac.decode_runs(),
    ids=[f"{c.name}-{mode}-{'_'.join(map(str, lens[:3]))}"
         for c, mode, lens, _, _ in ac.decode_runs()])
def test_attn_decode(run):
    c, mode, lens, _, _ = run
    assert ext().attn_decode_shape_ok(c.Hq // c.Hkv, c.Dv)
    q, kbuf, vbuf, scale = ac.decode_inputs(c.name, lens)
    want, _, bound = ac.decode_reference(c, lens)
    k = _poisoned(kbuf, lens)
    v = k[..., :c.Dv] if c.alias else _poisoned(vbuf, lens)
    pos = None
    if mode == "host":
        k, v = k[:, :, :lens[0]], v[:, :, :lens[0]]
    else:
        n = c.B if mode == "ragged" else 1
        pos = torch.tensor([L - 1 for L in lens[:n]], dtype=torch.int32,
                           device=DEV)
    got = ext().attn_decode(q.to(DEV), k, v, scale, c.softcap, c.window, pos)
    assert got.shape == (c.B, c.Hq, 1, c.Dv)
    got = got[:, :, 0]
    _check(f"attn_decode {c.name} {mode} {lens[:3]}", got, want, bound)
    for b, L in enumerate(lens):
        if L == 1 or c.window == 1:  # one key: that V row, bit for bit
            row = (kbuf[b, :, L - 1, :c.Dv] if c.alias else vbuf[b, :, L - 1])
            row = row.repeat_interleave(c.Hq // c.Hkv, 0)
            assert torch.equal(got[b].cpu(), row), (c.name, mode, b, L)


@pytest.mark.parametrize("case", ac.PREFILL_CASES,
                         ids=[c.name for c in ac.PREFILL_CASES])
def test_attn_prefill(case):
    c = case
    assert ext().attn_prefill_shape_ok(c.Dk, c.Dv)
    q, kbuf, vbuf, scale = ac.prefill_inputs(c)
    want, _, bound = ac.prefill_reference(c)
    S = c.offset + c.T
    k = _poisoned(kbuf, [S] * c.B)[:, :, :S]
    v = _poisoned(vbuf, [S] * c.B)[:, :, :S]
    got = ext().attn_prefill(q.to(DEV), k, v, scale, c.softcap, c.window,
                             c.offset)
    assert got.shape == (c.B, c.Hq, c.T, c.Dv)
    _check(f"attn_prefill {c.name}", got, want, bound)


@pytest.mark.parametrize("case", ac.FALLBACK_CASES,
                         ids=[c.name for c in ac.FALLBACK_CASES])
def test_composed_prefill(case):
    c = case
    assert not ext().attn_prefill_shape_ok(c.Dk, c.Dv)
    q, kbuf, vbuf, scale = ac.prefill_inputs(c)
    want, _, bound = ac.prefill_reference(c)
    S = c.offset + c.T
    k = _poisoned(kbuf, [S] * c.B)[:, :, :S]
    v = _poisoned(vbuf, [S] * c.B)[:, :, :S]
    got = ops.attention(q.to(DEV), k, v, scale, causal_offset=c.offset,
                        softcap=c.softcap, sliding_window=c.window)
    assert got.shape == (c.B, c.Hq, c.T, c.Dv)
    _check(f"composed prefill {c.name}", got, want, bound)


def test_attn_binding_limits():
    """Shapes without an instantiation are refused, not run."""
    def bf(*shape):
        return torch.zeros(*shape, device=DEV, dtype=torch.bfloat16)

    with pytest.raises(RuntimeError, match="unsupported GQA"):   # G = 3
        ext().attn_decode(bf(1, 3, 1, 64), bf(1, 1, 8, 64), bf(1, 1, 8, 64),
                          0.1, 0.0, 0, None)
    with pytest.raises(RuntimeError, match="unsupported GQA"):   # G = 8, DVT 2
        ext().attn_decode(bf(1, 8, 1, 64), bf(1, 1, 8, 64), bf(1, 1, 8, 320),
                          0.1, 0.0, 0, None)
    with pytest.raises(RuntimeError, match="no kernel instantiation"):
        ext().attn_prefill(bf(1, 1, 4, 96), bf(1, 1, 4, 96), bf(1, 1, 4, 96),
                           0.1, 0.0, 0, 0)
    torch.cuda.synchronize()
