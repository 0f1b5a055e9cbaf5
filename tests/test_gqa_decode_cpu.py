"""ops.gqa_decode_route's truth table, and ops.gqa_decode on CPU tensors."""
import types

import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref


@pytest.fixture
def stub_ext(monkeypatch):
    stub = types.SimpleNamespace(
        gqa_decode_shape_ok=lambda g, dk, dv: 1 <= g <= 16 and dk == dv
        and dk in (64, 128, 256))
    monkeypatch.setattr(ops, "hip_ext", lambda: stub)


# (G, Dk, Dv, batch, hkv, span, device_pos)
LLAMA70 = (8, 128, 128, 64, 8, 4096, False)


@pytest.mark.parametrize("env,shape,want", [
    ("0", LLAMA70, False),
    ("1", LLAMA70, True),
    ("1", (2, 256, 256, 1, 8, 512, True), True),
    ("1", (1, 128, 128, 64, 8, 4096, False), False),     # G = 1
    (None, (1, 128, 128, 64, 8, 4096, False), False),
    ("1", (8, 192, 128, 64, 8, 4096, False), False),     # no instantiation
    ("1", (17, 128, 128, 64, 8, 4096, False), False),
    (None, (8, 192, 128, 64, 8, 4096, False), False),
    # unset: the measured regions of PERFORMANCE.md and nothing else
    (None, LLAMA70, True),
    (None, (4, 128, 128, 1, 8, 512, False), True),
    (None, (4, 128, 128, 1, 8, 511, False), False),
    (None, (7, 128, 128, 16, 4, 2048, True), True),
    (None, (7, 128, 128, 16, 4, 2047, True), False),
    (None, (8, 64, 64, 64, 4, 8192, True), True),
    (None, (4, 64, 64, 64, 4, 8192, True), False),       # not measured
    (None, (2, 256, 256, 64, 8, 8192, True), False),     # within the spread
])
def test_route_truth_table(stub_ext, monkeypatch, env, shape, want):
    if env is None:
        monkeypatch.delenv("MLXS_AMD_GQA_MFMA", raising=False)
    else:
        monkeypatch.setenv("MLXS_AMD_GQA_MFMA", env)
    assert ops.gqa_decode_route(*shape) is want


def test_route_rejects_other_values(stub_ext, monkeypatch):
    monkeypatch.setenv("MLXS_AMD_GQA_MFMA", "yes")
    with pytest.raises(ValueError, match="MLXS_AMD_GQA_MFMA"):
        ops.gqa_decode_route(*LLAMA70)


@pytest.mark.parametrize("pos", (None, [0, 6, 3]), ids=("host", "ragged"))
def test_cpu_gqa_decode_is_reference_over_each_prefix(pos):
    B, Hq, Hkv, D, S = 3, 4, 2, 16, 7
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, Hq, 1, D, generator=g)
    k = torch.randn(B, Hkv, S, D, generator=g)
    v = torch.randn(B, Hkv, S, D, generator=g)
    p = None if pos is None else torch.tensor(pos, dtype=torch.int32)
    got = ops.gqa_decode(q, k, v, 0.25, 30.0, 4, p)
    assert got.shape == (B, Hq, 1, D)
    for b in range(B):
        L = S if pos is None else pos[b] + 1
        want = ref.attention(q[b:b + 1], k[b:b + 1, :, :L], v[b:b + 1, :, :L],
                             0.25, causal_offset=L - 1, softcap=30.0,
                             sliding_window=4)
        torch.testing.assert_close(got[b:b + 1], want)
