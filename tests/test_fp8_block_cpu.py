"""FP8 block-quantized checkpoints end to end on the CPU: config parsing,
an HF-layout DeepSeek-V3 FP8 checkpoint directory against its dense twin,
the offline splitter, load-time quantization, the CLIs' --quantize fp8 and
FusedColumns over block-scaled weights."""

import json
import sys

import pytest
import torch
from safetensors.torch import load_file, save_file

from conftest import init_model
from mlx_sharding_amd.config import ModelConfig, QuantConfig
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.models.base import Linear
from mlx_sharding_amd.models.fuse import FusedColumns
from mlx_sharding_amd.ops import reference as ref
from mlx_sharding_amd.utils import loading
from mlx_sharding_amd.utils.presets import PRESETS, get_preset

F8 = torch.float8_e4m3fn
FP8_STANZA = {"quant_method": "fp8", "fmt": "e4m3",
              "activation_scheme": "dynamic", "weight_block_size": [128, 128]}


# --------------------------------------------------------------------------
# config
# --------------------------------------------------------------------------

def _cfg(**extra):
    return ModelConfig.from_dict(dict(PRESETS["debug-deepseek-v3"], **extra))


def test_fp8_stanza_parses():
    q = _cfg(quantization_config=FP8_STANZA).quantization
    assert (q.fmt, q.bits, q.group_size) == ("fp8_block", 8, 128)
    no_act = {k: v for k, v in FP8_STANZA.items() if k != "activation_scheme"}
    assert _cfg(quantization_config=no_act).quantization == q
    assert get_preset("debug-deepseek-v3", fp8=True).quantization == q


@pytest.mark.parametrize("field,value", [
    ("fmt", "e5m2"), ("weight_block_size", [64, 64]),
    ("activation_scheme", "static")])
def test_unsupported_fp8_stanza_names_the_field(field, value):
    with pytest.raises(ValueError, match=field):
        _cfg(quantization_config=dict(FP8_STANZA, **{field: value})).quantization


def test_quantization_stanza_wins_and_affine_defaults_unchanged():
    q = _cfg(quantization={"group_size": 32, "bits": 8},
             quantization_config=FP8_STANZA).quantization
    assert (q.fmt, q.bits, q.group_size) == ("affine", 8, 32)
    assert QuantConfig() == QuantConfig(group_size=64, bits=4, fmt="affine")
    assert QuantConfig.from_dict({}).fmt == "affine"
    assert _cfg().quantization is None
    # another quant_method is not ours to parse
    assert _cfg(quantization_config={"quant_method": "awq"}).quantization is None
    with pytest.raises(ValueError):
        QuantConfig(fmt="fp8_block", bits=4, group_size=128)


# --------------------------------------------------------------------------
# an HF-layout FP8 checkpoint and its dense twin
# --------------------------------------------------------------------------

N_LAYERS = 3
_FP8_SKIP = ("embed_tokens", "norm", "layernorm", "lm_head", "mlp.gate.")


def _raw_config():
    return dict(PRESETS["debug-deepseek-v3"], num_hidden_layers=N_LAYERS)


def _hf_state():
    """Per-expert HF keys of a random 3-layer V3, every decoder-layer
    nn.Linear FP8 block-quantized, one FP8 multi-token-prediction layer at
    index num_hidden_layers and a rotary inv_freq buffer.
    Returns (fp8 state, dense fp32 twin state)."""
    cfg = ModelConfig.from_dict(_raw_config())
    m = init_model(get_model_class("deepseek_v3"), cfg, cfg.shard(0, N_LAYERS),
                   seed=21)
    flat = {}
    for k, v in m.state_dict().items():
        if ".switch_mlp." in k:
            head, tail = k.split(".switch_mlp.")
            for e in range(v.shape[0]):
                flat[f"{head}.experts.{e}.{tail}"] = v[e].clone()
        else:
            flat[k] = v.clone()
    # an MTP layer: copies of layer 2 plus its own projections
    for k in [k for k in flat if k.startswith("model.layers.2.")]:
        flat[k.replace("model.layers.2.", f"model.layers.{N_LAYERS}.")] = flat[k]
    flat[f"model.layers.{N_LAYERS}.eh_proj.weight"] = \
        torch.randn(cfg.hidden_size, 2 * cfg.hidden_size).to(torch.bfloat16)
    fp8, dense = {}, {}
    for k, v in flat.items():
        if (k.startswith("model.layers.") and k.endswith(".weight")
                and v.dim() == 2 and not any(t in k for t in _FP8_SKIP)):
            w8, s = ref.quantize_fp8_block(v.float())
            fp8[k] = w8
            fp8[k[:-len("weight")] + "weight_scale_inv"] = s
            dense[k] = ref.dequantize_fp8_block(w8, s)
        else:
            fp8[k] = v
            dense[k] = v.float() if v.is_floating_point() else v
    inv = torch.arange(8, dtype=torch.float32)
    fp8["model.layers.0.self_attn.rotary_emb.inv_freq"] = inv
    dense["model.layers.0.self_attn.rotary_emb.inv_freq"] = inv
    return fp8, dense


def _write(dirpath, state, raw):
    dirpath.mkdir()
    keys = sorted(state)
    half = len(keys) // 2
    for i, part in enumerate((keys[:half], keys[half:])):
        save_file({k: state[k].clone() for k in part},
                  str(dirpath / f"model-{i + 1:05d}-of-00002.safetensors"))
    (dirpath / "config.json").write_text(json.dumps(raw))
    return dirpath


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = tmp_path_factory.mktemp("fp8ckpt")
    fp8, dense = _hf_state()
    return (_write(root / "fp8", fp8,
                   dict(_raw_config(), quantization_config=FP8_STANZA)),
            _write(root / "dense", dense, _raw_config()))


IDS = torch.randint(0, 512, (1, 7), generator=torch.Generator().manual_seed(4))


def _greedy(stages, steps=4):
    """Prefill + greedy steps through a chain of stage models.
    Returns (tokens, logits rows)."""
    caches = [m.make_cache(batch_size=1) for m in stages]
    toks, rows = [], []
    x = IDS
    with torch.no_grad():
        for _ in range(steps + 1):
            h = x
            for m, c in zip(stages, caches):
                h = m(h, c)
            rows.append(h[:, -1].float())
            toks.append(int(rows[-1].argmax(-1)))
            x = torch.tensor([[toks[-1]]])
    return toks, rows


def test_checkpoint_matches_dense_twin(ckpts):
    fp8_dir, dense_dir = ckpts
    m8, cfg8 = loading.load_model(fp8_dir, dtype=torch.float32)
    md, _ = loading.load_model(dense_dir, dtype=torch.float32)
    assert cfg8.quantization.fmt == "fp8_block"
    sd = m8.state_dict()
    # stacked experts: [E, O, K] fp8 and [E, RB, KB] fp32 scales
    w = sd["model.layers.1.mlp.switch_mlp.gate_proj.weight"]
    s = sd["model.layers.1.mlp.switch_mlp.gate_proj.weight_scale_inv"]
    assert w.dtype == F8 and w.shape == (96, 64, 128)
    assert s.dtype == torch.float32 and s.shape == (96, 1, 1)
    assert sd["model.layers.1.self_attn.kv_b_proj.weight"].dtype == F8
    assert sd["model.layers.1.mlp.gate.weight"].dtype == torch.float32
    assert not any(k.startswith(f"model.layers.{N_LAYERS}.") for k in sd)
    assert m8.fp_dtype == torch.float32
    t8, r8 = _greedy([m8])
    td, rd = _greedy([md])
    assert t8 == td
    for a, b in zip(r8, rd):
        d, top = float((a - b).abs().max()), float(b.abs().max())
        print("max|dlogit| %.3e of max|logit| %.3f" % (d, top))
        assert d <= 1e-5 * top


def test_bf16_load_keeps_fp8_and_fp32_scales(ckpts):
    m8, _ = loading.load_model(ckpts[0], dtype=torch.bfloat16)
    for k, v in m8.state_dict().items():
        if k.endswith("weight_scale_inv"):
            assert v.dtype == torch.float32, k
            assert m8.state_dict()[k[:-len("_scale_inv")]].dtype == F8, k
        elif k.endswith("e_score_correction_bias"):
            assert v.dtype == torch.float32
        elif v.is_floating_point() and v.element_size() > 1:
            assert v.dtype == torch.bfloat16, k
    assert m8.fp_dtype == torch.bfloat16
    toks, rows = _greedy([m8], steps=1)
    assert all(torch.isfinite(r).all() for r in rows)


def test_absorbed_weights_from_fp8_kv_b_proj(ckpts):
    m8, _ = loading.load_model(ckpts[0], dtype=torch.float32)
    md, _ = loading.load_model(ckpts[1], dtype=torch.float32)
    a8 = m8.model.layers["1"].self_attn
    ad = md.model.layers["1"].self_attn
    a8._ensure_absorb("cpu", torch.float32)
    ad._ensure_absorb("cpu", torch.float32)
    assert torch.equal(a8._w_uk, ad._w_uk) and torch.equal(a8._w_uv, ad._w_uv)
    sw8 = m8.model.layers["1"].mlp.switch_mlp
    swd = md.model.layers["1"].mlp.switch_mlp
    assert torch.equal(sw8.down_proj.dense(), swd.down_proj.dense())


def test_sharding_keeps_fp8_tensors(ckpts, tmp_path):
    fp8_dir = ckpts[0]
    f0 = loading.save_sharded_weights(fp8_dir, tmp_path / "s0", 0, 2)
    f1 = loading.save_sharded_weights(fp8_dir, tmp_path / "s1", 2, N_LAYERS)
    src = loading.load_weights(fp8_dir)
    for f, (lo, hi) in ((f0, (0, 2)), (f1, (2, N_LAYERS))):
        got = load_file(str(f))
        layers = {int(k.split(".")[2]) for k in got
                  if k.startswith("model.layers.")}
        assert layers == set(range(lo, hi))       # the MTP layer is dropped
        n8 = 0
        for k, v in got.items():
            assert v.dtype == src[k].dtype and torch.equal(
                v.view(torch.uint8) if v.dtype == F8 else v,
                src[k].view(torch.uint8) if v.dtype == F8 else src[k]), k
            if v.dtype == F8:
                n8 += 1
                assert got[k[:-len("weight")] + "weight_scale_inv"].dtype \
                    == torch.float32
        assert n8 > 0
        cfg = json.loads((f.parent / "config.json").read_text())
        assert cfg["quantization_config"] == FP8_STANZA
    whole, _ = loading.load_model(fp8_dir, dtype=torch.float32)
    s0, _ = loading.load_model(tmp_path / "s0", dtype=torch.float32)
    s1, _ = loading.load_model(tmp_path / "s1", dtype=torch.float32)
    assert _greedy([whole])[0] == _greedy([s0, s1])[0]


# --------------------------------------------------------------------------
# load-time quantization and the CLIs
# --------------------------------------------------------------------------

def test_quantize_weights_fp8(ckpts):
    w = loading.load_weights(ckpts[1])
    cfg = ModelConfig.load(ckpts[1])
    loading.quantize_weights(w, cfg, fmt="fp8")
    assert cfg.raw["quantization_config"] == FP8_STANZA
    assert cfg.quantization.fmt == "fp8_block"
    k = "model.layers.1.mlp.experts.3.down_proj.weight"
    assert w[k].dtype == F8
    assert w[k[:-len("weight")] + "weight_scale_inv"].shape == (1, 1)
    for k, v in w.items():       # the affine path's key filter
        if any(t in k for t in ("embed_tokens", "norm", "gate.weight")):
            assert v.dtype != F8, k
    with pytest.raises(ValueError, match="already FP8"):
        loading.quantize_weights(w, cfg, fmt="fp8")
    with pytest.raises(ValueError):
        loading.quantize_weights({}, ModelConfig.load(ckpts[1]), fmt="fp4")


def test_load_time_fp8_runs_and_already_fp8_raises(ckpts):
    m, cfg = loading.load_model(ckpts[1], dtype=torch.float32, quantize="fp8")
    assert cfg.quantization.fmt == "fp8_block"
    assert m.model.layers["0"].mlp.down_proj.weight.dtype == F8
    assert m.lm_head.weight.dtype == F8
    toks, rows = _greedy([m], steps=2)
    assert all(torch.isfinite(r).all() for r in rows)
    for q in ("fp8", (4, 64)):
        with pytest.raises(ValueError, match="already FP8"):
            loading.load_model(ckpts[0], quantize=q)


class _Stop(Exception):
    pass


def _capture(store):
    def fake(*args, **kwargs):
        store.append(kwargs.get("quantize"))
        raise _Stop
    return fake


def test_cli_quantize_fp8_parses(ckpts, monkeypatch):
    from mlx_sharding_amd import cli
    from mlx_sharding_amd.cli import generate, rccl_serve, server_main
    assert cli.quantize_request(cli.quantize_choice("fp8"), 32) == "fp8"
    assert cli.quantize_request(cli.quantize_choice("8"), 32) == (8, 32)
    assert cli.quantize_request(None, 64) is None
    model = str(ckpts[1])
    # server
    seen = []
    import mlx_sharding_amd.server.shard_server as ss
    monkeypatch.setattr(ss, "serve", _capture(seen))
    for q, want in (("fp8", "fp8"), ("4", (4, 64))):
        monkeypatch.setattr(sys, "argv", ["x", "--model", model, "--quantize", q,
                                          "--device", "cpu"])
        with pytest.raises(_Stop):
            server_main.main()
        assert seen[-1] == want
    # generate and rccl-serve load the model themselves
    import transformers
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained",
                        lambda *a, **k: object())
    monkeypatch.setattr(loading, "load_model", _capture(seen))
    import mlx_sharding_amd.parallel.rccl as rccl
    monkeypatch.setattr(rccl, "init_distributed",
                        lambda *a, **k: (0, 1, torch.device("cpu")))
    for main in (generate.main, rccl_serve.main):
        with pytest.raises(_Stop):
            main(["--model", model, "--quantize", "fp8",
                  "--quantize-group-size", "32"])
        assert seen[-1] == "fp8"
        with pytest.raises(SystemExit):
            main(["--model", model, "--quantize", "5"])


# --------------------------------------------------------------------------
# FusedColumns
# --------------------------------------------------------------------------

def _fp8_linear(K, O, seed):
    lin = Linear(K, O, QuantConfig(128, 8, "fp8_block"))
    g = torch.Generator().manual_seed(seed)
    w8, s = ref.quantize_fp8_block(torch.randn(O, K, generator=g) * 0.05)
    lin.weight.data, lin.weight_scale_inv.data = w8, s
    return lin


def test_fused_columns_fp8_on_block_edges():
    a, b, c = _fp8_linear(256, 128, 1), _fp8_linear(256, 256, 2), \
        _fp8_linear(256, 80, 3)
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(9))
    want = [l(x) for l in (a, b, c)]
    fused = FusedColumns([a, b, c])
    assert fused.weight.dtype == F8 and fused.weight.shape == (464, 256)
    assert fused.weight_scale_inv.shape == (4, 2)
    got = fused(x)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # the parts became views of the fused buffers and still work alone
    assert a.weight.data_ptr() == fused.weight.data_ptr()
    assert torch.equal(c(x), want[2])


def test_fused_columns_fp8_off_block_edge_mutates_nothing():
    a, b = _fp8_linear(256, 80, 1), _fp8_linear(256, 128, 2)
    before = [(p.data_ptr(), p.clone()) for l in (a, b)
              for p in (l.weight, l.weight_scale_inv)]
    with pytest.raises(AssertionError):
        FusedColumns([a, b])
    after = [p for l in (a, b) for p in (l.weight, l.weight_scale_inv)]
    for (ptr, old), p in zip(before, after):
        assert p.data_ptr() == ptr
        assert torch.equal(p.view(torch.uint8) if p.dtype == F8 else p,
                           old.view(torch.uint8) if p.dtype == F8 else old)
    dense = Linear(256, 128, None)
    with pytest.raises(AssertionError):
        FusedColumns([_fp8_linear(256, 128, 3), dense])
