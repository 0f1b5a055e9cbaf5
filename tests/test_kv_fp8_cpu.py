"""The FP8 KV-cache storage format (ops.reference.kv_fp8_quantize) against a
plain fp64 computation, and KVCache / make_cache with the FP8 dtype."""
import bisect

import pytest
import torch

from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.ops import reference as ref
from mlx_sharding_amd.ops.kvcache import KVCache
from mlx_sharding_amd.utils.presets import get_preset

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
# the 127 non-negative finite e4m3 values; the index is the code
GRID = [(m / 8 * 2.0 ** -6) if ex == 0 else (1 + m / 8) * 2.0 ** (ex - 7)
        for ex in range(16) for m in range(8)][:127]


def fp64_quantize(row):
    amax = max(abs(x) for x in row)
    e = -100
    while amax > 448 * 2.0 ** e:      # exact in fp64; amax == 0 stays at -100
        e += 1
    codes = []
    for x in row:
        y = abs(x) / 2.0 ** e
        hi = min(bisect.bisect_left(GRID, y), 126)
        lo = max(hi - 1, 0)
        dl, dh = y - GRID[lo], GRID[hi] - y
        c = lo if dl < dh else hi if dh < dl else (lo if lo % 2 == 0 else hi)
        codes.append(c | (0x80 if x < 0 else 0))
    return codes, min(e, 120)


# amax exactly 448 * 2^e, and one bf16 ulp (2 * 2^e) below and above it
ROWS = [[a * 2.0 ** e, -3.0 * 2.0 ** e, 0.0, 2.0 ** e]
        for e in (-3, 0, 5) for a in (448.0, 446.0, 450.0)] + [
    [0.0, 0.0, 0.0, 0.0],
    # e = 0 and ties of e4m3: 17 -> 16, 19 -> 20, 2^-10 -> 0, 3 * 2^-10 -> 2^-8
    [448.0, 17.0, -19.0, 2.0 ** -10, 3 * 2.0 ** -10, -27.0, 288.0 + 16.0],
    [2.0 ** -120, -2.0 ** -125, 2.0 ** -130],          # e clamps at -100
    [1.5 * 2.0 ** 126, -2.0 ** 120, 1.0],
    [-255 / 128 * 2.0 ** 127, 2.0 ** 127, 2.0 ** 100],  # bf16 max: e = 120
]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"{r[0]:.4g}")
def test_quantize_designed_rows(row):
    x = torch.tensor(row, dtype=torch.float64).to(BF16)
    assert x.double().tolist() == row          # the rows are bf16 values
    codes, scale = ref.kv_fp8_quantize(x)
    want, e = fp64_quantize(row)
    assert scale.dtype == torch.float32 and scale.item() == 2.0 ** e
    assert codes.tolist() == want


def test_round_trip_within_half_an_ulp():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 128, generator=g)
         * torch.logspace(-12, 12, 64, base=2.0)[:, None]).to(BF16)
    codes, scale = ref.kv_fp8_quantize(x)
    deq = ref.kv_fp8_dequantize(codes, scale)
    y = x.double() / scale.double()[:, None]
    k = torch.frexp(y.abs())[1]                  # |y| in [2^(k-1), 2^k)
    half_ulp = 2.0 ** (torch.clamp(k - 1, min=-6) - 3).double() / 2
    assert ((deq.double() / scale.double()[:, None] - y).abs() <= half_ulp).all()


def _rows(B, H, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, T, D, generator=g) * 3).to(BF16)


def _check(cache, k, v, n):
    for buf, sc, x in ((cache._k, cache._ks, k), (cache._v, cache._vs, v)):
        codes, scale = ref.kv_fp8_quantize(x)
        assert torch.equal(buf[:, :, :n], codes)
        assert torch.equal(sc[:, :, :n], scale)


def test_cache_update_and_grow():
    c = KVCache(2, 64, 64, dtype=FP8, batch_size=2)
    k, v = _rows(2, 2, 1030, 64, 1), _rows(2, 2, 1030, 64, 2)
    c.update(k[:, :, :5], v[:, :, :5])
    kd, vd = c.update(k[:, :, 5:], v[:, :, 5:])   # grows past CHUNK
    assert c.capacity == 2 * KVCache.CHUNK and c.offset == 1030
    _check(c, k, v, 1030)
    assert torch.equal(kd, ref.kv_fp8_dequantize(*ref.kv_fp8_quantize(k)))
    assert torch.equal(c.dequant_views()[0], kd)


def test_cache_pool_slot_trim_and_device_positions():
    pool = KVCache(2, 64, 64, dtype=FP8, batch_size=3)
    pool.allocate(16, 3)
    k, v = _rows(1, 2, 6, 64, 3), _rows(1, 2, 6, 64, 4)
    s = pool.slot(1)
    s.update(k, v)
    s.trim(2)
    assert s.offset == 2 and pool._ks[1, :, 5].ne(0).all()
    _check(s, k, v, 6)                      # the slot is a view of the pool
    # ragged decode: row b lands at pos[b], bytes and scales in step
    pos = [7, 0, 15]
    pool.graph_pos = torch.tensor(pos, dtype=torch.int32)
    k1, v1 = _rows(3, 2, 1, 64, 6), _rows(3, 2, 1, 64, 7)
    kd, vd = pool.update(k1, v1)
    assert kd.shape == (3, 2, 16, 64) and kd.dtype == BF16
    for b, p in enumerate(pos):
        for buf, sc, x in ((pool._k, pool._ks, k1), (pool._v, pool._vs, v1)):
            codes, scale = ref.kv_fp8_quantize(x[b, :, 0])
            assert torch.equal(buf[b, :, p], codes)
            assert torch.equal(sc[b, :, p], scale)


def _model(name):
    return get_model_class(get_preset(name).model_type)(
        get_preset(name), get_preset(name).shard(0, 1))


def test_make_cache_reads_the_switch(monkeypatch):
    m = _model("debug-llama-gqa")
    monkeypatch.delenv("MLXS_AMD_KV_DTYPE", raising=False)
    assert m.make_cache()[0].dtype == BF16 and not m.make_cache()[0].fp8
    monkeypatch.setenv("MLXS_AMD_KV_DTYPE", "bf16")
    assert m.make_cache()[0].dtype == BF16
    monkeypatch.setenv("MLXS_AMD_KV_DTYPE", "fp8")
    assert m.make_cache()[0].fp8 and m.make_cache(dtype=BF16)[0].dtype == BF16
    monkeypatch.setenv("MLXS_AMD_KV_DTYPE", "int4")
    with pytest.raises(ValueError, match="bf16 or fp8"):
        m.make_cache()


@pytest.mark.parametrize("preset", ("debug-deepseek", "debug-gemma2",
                                    "debug-llama"))   # MLA; family; D = 32
def test_make_cache_refuses_fp8(preset, monkeypatch):
    monkeypatch.setenv("MLXS_AMD_KV_DTYPE", "fp8")
    with pytest.raises(ValueError, match="llama-family"):
        _model(preset).make_cache()
