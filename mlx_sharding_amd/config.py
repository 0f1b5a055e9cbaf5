"""Model/shard configuration.

The on-disk carrier is ``config.json`` exactly as in the reference
(/root/reference/shard/utils.py:33-39 injects ``start_layer``/``end_layer``
at load time; /root/reference/sharding_weight.py:48-60 bakes them into a
pre-sharded checkpoint).  We keep the raw dict around so arch-specific
model classes can pull their own fields.
"""

from __future__ import annotations

import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Optional


@dataclass
class ShardSpec:
    """Contiguous layer range [start, end) owned by one pipeline stage."""

    start_layer: int
    end_layer: int
    num_hidden_layers: int

    @property
    def is_first(self) -> bool:
        return self.start_layer == 0

    @property
    def is_last(self) -> bool:
        return self.end_layer == self.num_hidden_layers

    def owns(self, layer_idx: int) -> bool:
        return self.start_layer <= layer_idx < self.end_layer

    @property
    def n_layers(self) -> int:
        return self.end_layer - self.start_layer

    def __post_init__(self):
        if not (0 <= self.start_layer < self.end_layer <= self.num_hidden_layers):
            raise ValueError(
                f"invalid shard range [{self.start_layer}, {self.end_layer}) "
                f"for {self.num_hidden_layers} layers"
            )


@dataclass
class QuantConfig:
    """Quantization stanza from config.json.

    fmt "affine" (MLX-style): w = scales * q + biases, per group of
    `group_size` input elements; q packed little-endian into uint32
    (8 nibbles per word at bits=4).  Matches the checkpoint format the
    reference loads via /root/reference/shard/utils.py:54-65.

    fmt "fp8_block" (DeepSeek-V3/R1 originals): `weight` is
    float8_e4m3fn [O, K] and `weight_scale_inv` fp32
    [ceil(O/gs), ceil(K/gs)] holds one scale per gs x gs block,
    w[o, k] = float(weight[o, k]) * weight_scale_inv[o // gs, k // gs];
    bits=8 and group_size=128 (the block edge).
    """

    group_size: int = 64
    bits: int = 4
    fmt: str = "affine"

    def __post_init__(self):
        if self.fmt not in ("affine", "fp8_block"):
            raise ValueError(f"QuantConfig: unknown fmt {self.fmt!r}")
        if self.fmt == "fp8_block" and (self.bits != 8
                                        or self.group_size != 128):
            raise ValueError(
                "QuantConfig: fp8_block needs bits=8 and group_size=128 "
                f"(got bits={self.bits}, group_size={self.group_size})")

    @classmethod
    def from_dict(cls, d: dict) -> "QuantConfig":
        return cls(group_size=int(d.get("group_size", 64)), bits=int(d.get("bits", 4)))

    @classmethod
    def from_hf_fp8(cls, d: dict) -> "QuantConfig":
        """The `quantization_config` stanza of an FP8 checkpoint
        (quant_method == "fp8").  Only e4m3 weights in 128x128 blocks
        with dynamic (or unspecified) activation scaling are supported."""
        fmt = d.get("fmt", "e4m3")
        if fmt != "e4m3":
            raise ValueError(
                f"quantization_config: fmt {fmt!r} not supported (only 'e4m3')")
        wbs = d.get("weight_block_size")
        if wbs is None or list(wbs) != [128, 128]:
            raise ValueError(
                f"quantization_config: weight_block_size {wbs!r} not "
                f"supported (only [128, 128])")
        act = d.get("activation_scheme")
        if act not in (None, "dynamic"):
            raise ValueError(
                f"quantization_config: activation_scheme {act!r} not "
                f"supported (only 'dynamic')")
        return cls(group_size=128, bits=8, fmt="fp8_block")


FP8_QUANTIZATION_CONFIG = {"quant_method": "fp8", "fmt": "e4m3",
                           "activation_scheme": "dynamic",
                           "weight_block_size": [128, 128]}


@dataclass
class ModelConfig:
    model_type: str
    raw: dict = field(default_factory=dict)

    @property
    def num_hidden_layers(self) -> int:
        return int(self.raw["num_hidden_layers"])

    @property
    def hidden_size(self) -> int:
        return int(self.raw["hidden_size"])

    @property
    def vocab_size(self) -> int:
        return int(self.raw["vocab_size"])

    @property
    def quantization(self) -> Optional[QuantConfig]:
        q = self.raw.get("quantization")
        if q:
            return QuantConfig.from_dict(q)
        hf = self.raw.get("quantization_config")
        if hf and hf.get("quant_method") == "fp8":
            return QuantConfig.from_hf_fp8(hf)
        return None

    @property
    def start_layer(self) -> int:
        return int(self.raw.get("start_layer", 0))

    @property
    def end_layer(self) -> int:
        return int(self.raw.get("end_layer", self.num_hidden_layers))

    def shard(self, start_layer: Optional[int] = None, end_layer: Optional[int] = None) -> ShardSpec:
        s = self.start_layer if start_layer is None else start_layer
        e = self.end_layer if end_layer is None else end_layer
        return ShardSpec(s, e, self.num_hidden_layers)

    def get(self, key: str, default: Any = None) -> Any:
        return self.raw.get(key, default)

    def __getitem__(self, key: str) -> Any:
        return self.raw[key]

    @classmethod
    def from_dict(cls, d: dict) -> "ModelConfig":
        return cls(model_type=d["model_type"], raw=dict(d))

    @classmethod
    def load(cls, model_path: str | Path) -> "ModelConfig":
        p = Path(model_path) / "config.json"
        with open(p) as f:
            return cls.from_dict(json.load(f))
