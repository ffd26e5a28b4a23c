"""Engine weight layout and tensor-parallel sharding.

The decode kernels want, per rank (t = TP degree, r = rank):

* ``wqkv``  [(Hq/t + 2·Hkv/t)·128, H]  — q heads, then k heads, then v heads of this rank, each
  128-row head unit permuted by :func:`ops.reference.rotary_perm` so the fused RoPE epilogue finds
  the rotary partner 8 lanes away (column-parallel: Megatron split by heads).
* ``wo``    [H, Hq/t·128]              — row-parallel (input features split by heads).
* ``wgu``   [2·F/t, H]                 — gate/up rows interleaved in 8-row blocks (column-parallel),
  so the SiLU·mul epilogue pairs gate and up in one MFMA tile.
* ``wd``    [H, F/t]                   — row-parallel.
* ``lm_head`` [V/t, H]                 — vocab-parallel; the sampler merges per-rank candidates.
* ``embed`` [V, H] replicated (256 MiB; HBM is plentiful, and it avoids an all-reduce per step).

Every GEMM of the engine -- decode (gemm_skinny / gemm_stream / gemm_wide) and prefill (gemm_tiled) --
consumes the tiled layout of :func:`ops.reference.tile_weight` (``*_t`` fields, made by :func:`attach_tiled`):
every weight load instruction reads 1 KiB of contiguous HBM, and a (16-column, 32-deep) block is one MFMA B
fragment.  The row-major [out, in] matrices above are only the conversion input; :func:`attach_tiled` drops
them, so the model is resident once (round 1 kept both layouts for the library prefill GEMMs: 14.5 GB more for
Mistral-7B at TP=1, now KV cache).

``quantization="fp8"`` (TP = 1 only) quantises the five matrices once, at load, in the engine layout (so the scale
index is the engine row): ``*_q`` = e4m3 bytes in the byte tiled layout (:func:`ops.reference.tile_weight_f8`),
``*_scale`` = one fp32 power-of-two scale per row, and ``*_t`` = the tiled copy of ``bf16(q) * scale`` (exact), which
every kernel without an FP8 form keeps using.  Embedding, norms and rope are left alone.

``quantization="mxfp4"`` (TP = 1 only) does the same with OCP MXFP4: ``*_q`` = e2m1 nibble bytes and ``*_e`` = e8m0
scale bytes, one per 32 consecutive K of an engine row, both in the tiled layout
(:func:`ops.reference.tile_weight_mxfp4`), and ``*_t`` = the tiled copy of the exactly widened values.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from ..models.mistral import MistralConfig
from ..ops.reference import (gate_up_perm, quantize_weight_f8, quantize_weight_mxfp4, rotary_perm, tile_weight,
                             tile_weight_f8, tile_weight_mxfp4, untile_weight, widen_weight_f8, widen_weight_mxfp4)

# weight quantisation at load: none = bf16 only; fp8 = W8A16 e4m3, mxfp4 = W4A16 OCP MXFP4, each beside a widened copy
QUANTIZATIONS = ("none", "fp8", "mxfp4")


def parse_quantization(v) -> str:
    """None / "" / "none" -> "none"; "fp8" (or "fp8_e4m3") -> "fp8"; "mxfp4" -> "mxfp4"; anything else is an error
    naming the choices."""
    key = "none" if v is None else str(v).strip().lower()
    key = {"": "none", "fp8_e4m3": "fp8"}.get(key, key)
    if key not in QUANTIZATIONS:
        raise ValueError(f"quantization / QUANTIZATION must be one of {', '.join(QUANTIZATIONS)}; got {v!r}")
    return key


@dataclass
class LayerWeights:
    attn_norm: torch.Tensor
    wqkv: torch.Tensor   # row-major conversion inputs (None once attach_tiled has run)
    wo: torch.Tensor
    ffn_norm: torch.Tensor
    wgu: torch.Tensor
    wd: torch.Tensor
    # the engine's copies, in the tiled layout (attach_tiled)
    wqkv_t: torch.Tensor = None
    wo_t: torch.Tensor = None
    wgu_t: torch.Tensor = None
    wd_t: torch.Tensor = None
    # FP8 weights (quantization="fp8"): *_q = e4m3 bytes in the byte tiled layout (tile_weight_f8), *_scale = fp32
    # power-of-two scale per engine row; *_t is then the widened copy tile_weight(bf16(q) * scale)
    wqkv_q: torch.Tensor = None
    wqkv_scale: torch.Tensor = None
    wo_q: torch.Tensor = None
    wo_scale: torch.Tensor = None
    wgu_q: torch.Tensor = None
    wgu_scale: torch.Tensor = None
    wd_q: torch.Tensor = None
    wd_scale: torch.Tensor = None
    # MXFP4 weights (quantization="mxfp4"): *_q = e2m1 nibble bytes, *_e = e8m0 scale bytes per 32 K of an engine row,
    # both in the tiled layout (tile_weight_mxfp4); *_t is then the tiled widened copy
    wqkv_e: torch.Tensor = None
    wo_e: torch.Tensor = None
    wgu_e: torch.Tensor = None
    wd_e: torch.Tensor = None
    # per-layer dequantisation scales of an fp8 KV cache (stored = x / scale); 1.0 unless the checkpoint carries
    # vLLM's model.layers.N.self_attn.k_scale / .v_scale.  The same on every TP rank.  Unused with a bf16 cache.
    k_scale: float = 1.0
    v_scale: float = 1.0


@dataclass
class EngineWeights:
    cfg: MistralConfig
    tp_rank: int
    tp_size: int
    embed: torch.Tensor
    layers: list
    final_norm: torch.Tensor
    lm_head: torch.Tensor
    lm_head_t: torch.Tensor = None
    lm_head_q: torch.Tensor = None
    lm_head_scale: torch.Tensor = None
    lm_head_e: torch.Tensor = None
    quantization: str = "none"

    @property
    def nh(self) -> int:
        return self.cfg.num_heads // self.tp_size

    @property
    def nkv(self) -> int:
        return self.cfg.num_kv_heads // self.tp_size

    @property
    def ffn(self) -> int:
        return self.cfg.intermediate_size // self.tp_size

    @property
    def vocab_local(self) -> int:
        return self.cfg.vocab_size // self.tp_size

    @property
    def vocab_offset(self) -> int:
        return self.tp_rank * self.vocab_local

    def nbytes(self) -> int:
        """Bytes of the resident model: the bf16 copy (what a decode step streams, plus the embedding table) and,
        under quantization, the FP8 or MXFP4 copy beside it."""
        n = self.embed.numel() + self.final_norm.numel() + self.lm_head_t.numel()
        for L in self.layers:
            n += sum(t.numel() for t in (L.attn_norm, L.wqkv_t, L.wo_t, L.ffn_norm, L.wgu_t, L.wd_t))
        return 2 * n + self.nbytes_fp8() + self.nbytes_fp4()

    def nbytes_fp8(self) -> int:
        """Bytes of the FP8 copy (bytes and scales of every quantised matrix); 0 unless quantization is fp8."""
        if self.quantization != "fp8":
            return 0
        ts = [self.lm_head_q, self.lm_head_scale]
        for L in self.layers:
            ts += [L.wqkv_q, L.wqkv_scale, L.wo_q, L.wo_scale, L.wgu_q, L.wgu_scale, L.wd_q, L.wd_scale]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def nbytes_fp4(self) -> int:
        """Bytes of the MXFP4 copy (nibble and scale bytes of every quantised matrix); 0 unless quantization is mxfp4."""
        if self.quantization != "mxfp4":
            return 0
        ts = [self.lm_head_q, self.lm_head_e]
        for L in self.layers:
            ts += [L.wqkv_q, L.wqkv_e, L.wo_q, L.wo_e, L.wgu_q, L.wgu_e, L.wd_q, L.wd_e]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)


def _tile(m: torch.Tensor, quantization: str):
    """(tiled bf16, tiled quantised bytes, fp32 row scales, tiled e8m0 block scale bytes) of one engine-layout matrix.
    fp8: quantised per engine row (no block scales); mxfp4: per 32 K of an engine row (no row scales).  The bf16 copy
    is widened from the bytes, so both copies hold identical values.  (tile_weight(m), None, None, None) without
    quantization."""
    if quantization == "fp8":
        q, scale = quantize_weight_f8(m)
        return tile_weight(widen_weight_f8(q, scale).to(m.dtype)), tile_weight_f8(q), scale, None
    if quantization == "mxfp4":
        q, e = quantize_weight_mxfp4(m)
        qt, et = tile_weight_mxfp4(q, e)
        return tile_weight(widen_weight_mxfp4(q, e).to(m.dtype)), qt, None, et
    return tile_weight(m), None, None, None


def _tile_layer(L: LayerWeights, quantization: str) -> None:
    L.wqkv_t, L.wqkv_q, L.wqkv_scale, L.wqkv_e = _tile(L.wqkv, quantization)
    L.wo_t, L.wo_q, L.wo_scale, L.wo_e = _tile(L.wo, quantization)
    L.wgu_t, L.wgu_q, L.wgu_scale, L.wgu_e = _tile(L.wgu, quantization)
    L.wd_t, L.wd_q, L.wd_scale, L.wd_e = _tile(L.wd, quantization)
    L.wqkv = L.wo = L.wgu = L.wd = None


@torch.no_grad()
def attach_tiled(w: EngineWeights, quantization=None) -> EngineWeights:
    """Convert every GEMM weight to the tiled layout and drop the row-major input (idempotent).  quantization="fp8"
    or "mxfp4": the matrices (not the embedding, the norms or rope) are quantised here, once, in the engine layout."""
    w.quantization = parse_quantization(quantization) if w.quantization == "none" else w.quantization
    for L in w.layers:
        if L.wqkv_t is None:
            _tile_layer(L, w.quantization)
        L.wqkv = L.wo = L.wgu = L.wd = None
    if w.lm_head_t is None:
        w.lm_head_t, w.lm_head_q, w.lm_head_scale, w.lm_head_e = _tile(w.lm_head, w.quantization)
    w.lm_head = None
    return w


@torch.no_grad()
def quantize_engine_weights(w: EngineWeights, quantization="fp8") -> EngineWeights:
    """Quantise engine weights that were loaded without the option (idempotent): each matrix is taken back from its
    tiled bf16 copy, quantised in the engine layout, and both copies are stored as the loaders would have.  Weights
    already quantised in the other format are refused: their bf16 copy holds rounded values, and quantising those
    again would silently serve a model rounded twice."""
    q = _check_quantization(quantization, w.tp_size)
    if q == "none" or w.quantization == q:
        return w
    if w.quantization != "none":
        raise ValueError(f"the weights are already quantised as {w.quantization}: load them again with "
                         f"quantization={q} instead of quantising the rounded values a second time")
    attach_tiled(w)
    for L in w.layers:
        L.wqkv, L.wo, L.wgu, L.wd = (untile_weight(t) for t in (L.wqkv_t, L.wo_t, L.wgu_t, L.wd_t))
        _tile_layer(L, q)
    w.lm_head_t, w.lm_head_q, w.lm_head_scale, w.lm_head_e = _tile(untile_weight(w.lm_head_t), q)
    w.quantization = q
    return w


def _permute_units(w: torch.Tensor) -> torch.Tensor:
    """Permute the rows of each 128-row head unit by rotary_perm (works for q, k and v units)."""
    units = w.shape[0] // 128
    perm = rotary_perm().to(w.device)
    return w.view(units, 128, -1)[:, perm, :].reshape(w.shape)


def _kv_scale(t) -> float:
    """An optional checkpoint scale tensor (one element) as a positive finite float; absent = 1.0."""
    if t is None:
        return 1.0
    v = float(torch.as_tensor(t).float().reshape(-1)[0])
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"KV cache scale must be positive and finite, got {v}")
    return v


def _check_quantization(quantization, tp_size: int) -> str:
    q = parse_quantization(quantization)
    if q == "mxfp4" and tp_size > 1:
        raise ValueError("quantization=mxfp4 is not supported with tensor parallelism (tp > 1): the block scales are "
                         "not sharded; use --dp for more than one GPU")
    if q != "none" and tp_size > 1:
        raise ValueError("quantization=fp8 is not supported with tensor parallelism (tp > 1): the row scales are not "
                         "sharded; use --dp for more than one GPU")
    return q


def convert_standard(cfg: MistralConfig, std, tp_rank: int = 0, tp_size: int = 1, device="cpu",
                     quantization=None) -> EngineWeights:
    """Standard (HF-layout) weights -> this rank's engine weights (quantization="fp8" / "mxfp4": quantised once, here)."""
    quantization = _check_quantization(quantization, tp_size)
    cfg.validate(tp_size)
    D = cfg.head_dim
    nh, nkv, F = cfg.num_heads // tp_size, cfg.num_kv_heads // tp_size, cfg.intermediate_size // tp_size
    V = cfg.vocab_size // tp_size
    r = tp_rank
    layers = []
    for L in std["layers"]:
        q = L["q"][r * nh * D:(r + 1) * nh * D]
        k = L["k"][r * nkv * D:(r + 1) * nkv * D]
        v = L["v"][r * nkv * D:(r + 1) * nkv * D]
        wqkv = _permute_units(torch.cat([q, k, v]))
        wo = L["o"][:, r * nh * D:(r + 1) * nh * D]
        gate = L["gate"][r * F:(r + 1) * F]
        up = L["up"][r * F:(r + 1) * F]
        wgu = torch.cat([gate, up])[gate_up_perm(F)]
        wd = L["down"][:, r * F:(r + 1) * F]
        layers.append(LayerWeights(
            attn_norm=L["attn_norm"].contiguous().to(device), wqkv=wqkv.contiguous().to(device),
            wo=wo.contiguous().to(device), ffn_norm=L["ffn_norm"].contiguous().to(device),
            wgu=wgu.contiguous().to(device), wd=wd.contiguous().to(device),
            k_scale=_kv_scale(L.get("k_scale")), v_scale=_kv_scale(L.get("v_scale"))))
    return attach_tiled(EngineWeights(
        cfg=cfg, tp_rank=tp_rank, tp_size=tp_size, embed=std["embed"].contiguous().to(device), layers=layers,
        final_norm=std["final_norm"].contiguous().to(device), lm_head=std["lm_head"][r * V:(r + 1) * V].contiguous().to(device)),
        quantization)


@torch.no_grad()
def random_engine_weights(cfg: MistralConfig, tp_rank: int = 0, tp_size: int = 1, device="cuda",
                          seed: int = 0, dtype=torch.bfloat16, quantization=None) -> EngineWeights:
    """Random weights generated directly on the device in engine layout (the 7B bench path).

    Generating 14.5 GB through the standard layout on the host would take minutes; the engine layout
    is a fixed row permutation of the standard one, so the distribution is identical.  Each rank
    draws its own shard (seeded by (seed, rank)), i.e. the global model is a valid random model.
    """
    quantization = _check_quantization(quantization, tp_size)
    cfg.validate(tp_size)
    D, H = cfg.head_dim, cfg.hidden_size
    nh, nkv, F = cfg.num_heads // tp_size, cfg.num_kv_heads // tp_size, cfg.intermediate_size // tp_size
    V = cfg.vocab_size // tp_size
    gen = torch.Generator(device=device)
    gen.manual_seed(seed * 1000003 + tp_rank)

    def lin(out_f, in_f):
        t = torch.empty(out_f, in_f, device=device, dtype=dtype)
        t.normal_(0.0, 1.0 / math.sqrt(in_f), generator=gen)
        return t

    def norm(n):
        t = torch.empty(n, device=device, dtype=torch.float32).normal_(1.0, 0.1, generator=gen)
        return t.to(dtype)

    embed_gen = torch.Generator(device=device)
    embed_gen.manual_seed(seed * 1000003 + 999)  # replicated: identical on every rank
    embed = torch.empty(cfg.vocab_size, H, device=device, dtype=dtype).normal_(0.0, 1.0, generator=embed_gen)
    layers = []
    for _ in range(cfg.num_layers):
        L = LayerWeights(attn_norm=norm(H), wqkv=lin((nh + 2 * nkv) * D, H), wo=lin(H, nh * D),
                         ffn_norm=norm(H), wgu=lin(2 * F, H), wd=lin(H, F))
        _tile_layer(L, quantization)  # one layer's row-major copy at a time
        layers.append(L)
    return attach_tiled(EngineWeights(cfg=cfg, tp_rank=tp_rank, tp_size=tp_size, embed=embed, layers=layers,
                                      final_norm=norm(H), lm_head=lin(V, H)), quantization)


def load_safetensors(cfg: MistralConfig, path: str, tp_rank: int = 0, tp_size: int = 1, device="cpu",
                     quantization=None) -> EngineWeights:
    """Load an HF Mistral checkpoint directory (``*.safetensors``) into the engine layout."""
    from pathlib import Path

    from safetensors.torch import load_file

    tensors = {}
    for f in sorted(Path(path).glob("*.safetensors")):
        tensors.update(load_file(str(f)))
    std = {"embed": tensors["model.embed_tokens.weight"], "final_norm": tensors["model.norm.weight"],
           "lm_head": tensors.get("lm_head.weight", tensors["model.embed_tokens.weight"]), "layers": []}
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        std["layers"].append({
            "attn_norm": tensors[p + "input_layernorm.weight"],
            "q": tensors[p + "self_attn.q_proj.weight"], "k": tensors[p + "self_attn.k_proj.weight"],
            "v": tensors[p + "self_attn.v_proj.weight"], "o": tensors[p + "self_attn.o_proj.weight"],
            "ffn_norm": tensors[p + "post_attention_layernorm.weight"],
            "gate": tensors[p + "mlp.gate_proj.weight"], "up": tensors[p + "mlp.up_proj.weight"],
            "down": tensors[p + "mlp.down_proj.weight"],
            "k_scale": tensors.get(p + "self_attn.k_scale"), "v_scale": tensors.get(p + "self_attn.v_scale"),
        })
    return convert_standard(cfg, std, tp_rank, tp_size, device, quantization)
