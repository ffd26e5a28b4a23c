"""LoRA adapters: PEFT directories -> a device-resident pool in the engine's layout.

An adapter adds ``scale · B·A`` to some of the seven projections of every layer (``q_proj`` ... ``down_proj``).  The
engine never merges it: rows of different adapters share one step, so the low-rank products run beside the base GEMMs
(``ops.lora_shrink`` / ``ops.lora_expand_add``, csrc/kernels/lora.hip) and the delta is added to the projection's
output in the engine's row order, before RoPE and before SiLU.

Pool layout, per fused projection p in (qkv, o, gu, d) with S = (3, 1, 2, 1) slices and pool rank R:

* ``A[p]``  bf16 [layers, slots, S·R, K]  the A matrices of the slices stacked (q, k, v / gate, up), each zero-padded
  from its rank r to R rows: one shrink reads x once for all slices;
* ``B[p]``  bf16 [layers, slots, N, R]    B's rows in the order of the base weight's rows (``_permute_units`` for q / k /
  v, the 8-row gate / up interleave of ``wgu``), columns zero-padded to R; never scaled;
* ``slice_of_row[p]`` int32 [N]           which R columns of t output row n reads (no block-diagonal B);
* ``scale`` fp32 [slots]                  lora_alpha / r (rsLoRA: / sqrt(r)), applied to the fp32 sum by the expand kernel.

The tensors are allocated once and rewritten in place by :meth:`LoraPool.load`, so graphs captured over them see new
contents without recapture.  A module an adapter does not touch stays zero.
"""
from __future__ import annotations

import json
import math
import re
from dataclasses import dataclass, field
from pathlib import Path

import torch

from ..models.mistral import MistralConfig
from ..ops import LORA_MAX_SLOTS, LORA_RANKS
from ..ops.reference import gate_up_perm
from .weights import _permute_units

TARGET_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
PROJECTIONS = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",), "gu": ("gate_proj", "up_proj"),
               "d": ("down_proj",)}
_KEY = re.compile(r"layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)\.lora_([AB])(?:\.default)?\.weight$")


class LoraError(ValueError):
    """An adapter or a LoRA option the engine refuses; the message names the file and the reason."""


def module_shapes(cfg: MistralConfig) -> dict:
    """{module: (out features, in features)} of the base model."""
    H, F, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    q, kv = cfg.num_heads * D, cfg.num_kv_heads * D
    return {"q_proj": (q, H), "k_proj": (kv, H), "v_proj": (kv, H), "o_proj": (H, q), "gate_proj": (F, H),
            "up_proj": (F, H), "down_proj": (H, F)}


def parse_max_rank(v) -> int:
    r = int(v)
    if r not in LORA_RANKS:
        raise LoraError(f"max_lora_rank / MAX_LORA_RANK must be one of {', '.join(map(str, LORA_RANKS))}; got {v!r}")
    return r


def parse_max_loras(v) -> int:
    n = int(v)
    if not 1 <= n <= LORA_MAX_SLOTS:
        raise LoraError(f"max_loras / MAX_LORAS must be in [1, {LORA_MAX_SLOTS}]; got {v!r}")
    return n


def parse_lora_modules(items) -> dict:
    """["name=path", ...] (or one comma-separated string) -> {name: path}, in order."""
    if isinstance(items, str):
        items = [s for s in items.split(",") if s.strip()]
    out = {}
    for it in items or ():
        name, sep, path = str(it).strip().partition("=")
        if not sep or not name or not path:
            raise LoraError(f"lora_modules / LORA_MODULES entries are NAME=PATH; got {it!r}")
        if name in out:
            raise LoraError(f"lora_modules / LORA_MODULES names adapter {name!r} twice")
        out[name] = path
    return out


@dataclass
class LoraAdapter:
    name: str
    path: str
    r: int
    scale: float
    # layers[i] = {module: (A [r, in], B [out, r])} in the checkpoint's (HF) row order, bf16
    layers: list = field(default_factory=list)

    def delta(self, li: int, module: str):
        """scale · B·A of one module in fp32, HF order (None: the adapter does not touch it)."""
        ab = self.layers[li].get(module)
        return None if ab is None else self.scale * (ab[1].float() @ ab[0].float())


def load_adapter(path: str, cfg: MistralConfig, max_rank: int, name: str | None = None) -> LoraAdapter:
    """Read a PEFT directory (adapter_config.json + adapter_model.safetensors) and check it against the base model."""
    from safetensors.torch import load_file

    d = Path(path)
    cfg_file, w_file = d / "adapter_config.json", d / "adapter_model.safetensors"

    def refuse(f, why):
        raise LoraError(f"{f}: {why}")

    if not cfg_file.is_file():
        refuse(cfg_file, "not found")
    if not w_file.is_file():
        refuse(w_file, "not found")
    try:
        ac = json.loads(cfg_file.read_text())
    except ValueError as e:
        refuse(cfg_file, f"not JSON ({e})")
    if ac.get("bias", "none") != "none":
        refuse(cfg_file, f"bias = {ac['bias']!r} is not supported (only \"none\")")
    if ac.get("use_dora"):
        refuse(cfg_file, "use_dora (DoRA) is not supported")
    if ac.get("modules_to_save"):
        refuse(cfg_file, f"modules_to_save = {ac['modules_to_save']} is not supported")
    targets = ac.get("target_modules") or []
    targets = [targets] if isinstance(targets, str) else list(targets)
    other = sorted(set(targets) - set(TARGET_MODULES))
    if other:
        refuse(cfg_file, f"target module {other[0]!r} is not supported (only {', '.join(TARGET_MODULES)})")
    r = int(ac.get("r", 0))
    if r < 1:
        refuse(cfg_file, f"r = {ac.get('r')!r} is not a positive rank")
    if r > max_rank:
        refuse(cfg_file, f"rank r = {r} exceeds max_lora_rank = {max_rank}")
    if ac.get("rank_pattern") or ac.get("alpha_pattern"):
        refuse(cfg_file, "rank_pattern / alpha_pattern (per-module ranks or scales) are not supported")
    alpha = float(ac.get("lora_alpha", r))
    scale = alpha / math.sqrt(r) if ac.get("use_rslora") else alpha / r
    shapes = module_shapes(cfg)
    layers = [{} for _ in range(cfg.num_layers)]
    halves: dict = {}
    for key, t in load_file(str(w_file)).items():
        m = _KEY.search(key)
        if m is None or m.group(2) not in shapes:
            refuse(w_file, f"tensor {key!r} is not a lora_A / lora_B of a supported module "
                           f"({', '.join(TARGET_MODULES)})")
        li, mod, ab = int(m.group(1)), m.group(2), m.group(3)
        if li >= cfg.num_layers:
            refuse(w_file, f"tensor {key!r}: the base model has {cfg.num_layers} layers")
        out_f, in_f = shapes[mod]
        want = (r, in_f) if ab == "A" else (out_f, r)
        if tuple(t.shape) != want:
            refuse(w_file, f"tensor {key!r} has shape {tuple(t.shape)}, the base model needs {want}")
        halves[(li, mod, ab)] = t.to(torch.bfloat16)
    for (li, mod, ab), t in halves.items():
        if ab == "A":
            b = halves.get((li, mod, "B"))
            if b is None:
                refuse(w_file, f"layer {li} {mod} has lora_A without lora_B")
            layers[li][mod] = (t, b)
        elif (li, mod, "A") not in halves:
            refuse(w_file, f"layer {li} {mod} has lora_B without lora_A")
    return LoraAdapter(name=name or d.name, path=str(d), r=r, scale=scale, layers=layers)


def merge_into_standard(std: dict, adapter: LoraAdapter) -> dict:
    """Standard-layout weights with the adapter merged, W + scale · B·A in fp32 (what the engine's LoRA path must
    agree with; the engine itself never merges)."""
    names = {"q_proj": "q", "k_proj": "k", "v_proj": "v", "o_proj": "o", "gate_proj": "gate", "up_proj": "up",
             "down_proj": "down"}
    out = {k: v for k, v in std.items() if k != "layers"}
    out["layers"] = []
    for li, L in enumerate(std["layers"]):
        M = dict(L)
        for mod, k in names.items():
            dl = adapter.delta(li, mod)
            if dl is not None:
                M[k] = L[k].float() + dl
        out["layers"].append(M)
    return out


def _pad(t: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    out = torch.zeros(rows, cols, dtype=t.dtype)
    out[:t.shape[0], :t.shape[1]] = t
    return out


class LoraPool:
    """max_loras slots of pool rank R on `device` (TP = 1)."""

    def __init__(self, cfg: MistralConfig, max_loras: int = 4, max_rank: int = 16, device="cpu"):
        self.cfg, self.R, self.slots = cfg, parse_max_rank(max_rank), parse_max_loras(max_loras)
        self.device = torch.device(device)
        self.names: list = [None] * self.slots
        sh, L, R = module_shapes(cfg), cfg.num_layers, self.R
        F = cfg.intermediate_size
        bf = dict(dtype=torch.bfloat16, device=self.device)
        self.A, self.B, self.slice_of_row = {}, {}, {}
        for p, mods in PROJECTIONS.items():
            K, N = sh[mods[0]][1], sum(sh[m][0] for m in mods)
            self.A[p] = torch.zeros(L, self.slots, len(mods) * R, K, **bf)
            self.B[p] = torch.zeros(L, self.slots, N, R, **bf)
            sl = torch.cat([torch.full((sh[m][0],), s, dtype=torch.int32) for s, m in enumerate(mods)])
            if p == "gu":
                sl = sl[gate_up_perm(F)]
            # (q / k / v: the rotary permutation moves rows inside a 128-row head unit, so the slice ids stay put)
            self.slice_of_row[p] = sl.contiguous().to(self.device)
        self.scale = torch.zeros(self.slots, dtype=torch.float32, device=self.device)

    @staticmethod
    def bytes_for(cfg: MistralConfig, max_loras: int, max_rank: int) -> int:
        """Device bytes of a pool (counted before the KV page budget is sized)."""
        sh, n = module_shapes(cfg), 0
        for mods in PROJECTIONS.values():
            n += len(mods) * max_rank * sh[mods[0]][1] + sum(sh[m][0] for m in mods) * max_rank
        return 2 * n * cfg.num_layers * max_loras

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for d in (self.A, self.B) for t in d.values())

    def slot_of(self, name) -> int:
        """The slot of adapter `name` (-1 for None: the base model)."""
        if name is None:
            return -1
        try:
            return self.names.index(name)
        except ValueError:
            raise LoraError(f"LoRA adapter {name!r} is not loaded") from None

    def engine_layout(self, adapter: LoraAdapter, li: int) -> dict:
        """{projection: (A [S·R, K], B [N, R])} of layer li in the pool's layout (host tensors)."""
        sh, R, F = module_shapes(self.cfg), self.R, self.cfg.intermediate_size
        out = {}
        for p, mods in PROJECTIONS.items():
            As, Bs = [], []
            for m in mods:
                a, b = adapter.layers[li].get(m, (None, None))
                As.append(torch.zeros(R, sh[m][1], dtype=torch.bfloat16) if a is None else _pad(a, R, sh[m][1]))
                Bs.append(torch.zeros(sh[m][0], R, dtype=torch.bfloat16) if b is None else _pad(b, sh[m][0], R))
            B = torch.cat(Bs)
            if p == "qkv":
                B = _permute_units(B)
            elif p == "gu":
                B = B[gate_up_perm(F)]
            out[p] = (torch.cat(As).contiguous(), B.contiguous())
        return out

    @torch.no_grad()
    def load(self, slot: int, adapter: LoraAdapter) -> None:
        """Write `adapter` into `slot`, in place (stream-ordered copies into the tensors the graphs hold)."""
        if not 0 <= slot < self.slots:
            raise LoraError(f"LoRA slot {slot} outside the pool of {self.slots}")
        if adapter.r > self.R:
            raise LoraError(f"{adapter.path}: rank r = {adapter.r} exceeds max_lora_rank = {self.R}")
        if adapter.name in self.names and self.names.index(adapter.name) != slot:
            raise LoraError(f"LoRA adapter {adapter.name!r} is already loaded")
        for li in range(self.cfg.num_layers):
            for p, (A, B) in self.engine_layout(adapter, li).items():
                self.A[p][li, slot].copy_(A)
                self.B[p][li, slot].copy_(B)
        self.scale[slot] = adapter.scale
        self.names[slot] = adapter.name


def build_pool(cfg: MistralConfig, modules: dict, max_loras: int = 4, max_rank: int = 16, device="cpu") -> LoraPool:
    """Start-up: every NAME=PATH entry into its own slot (more entries than slots is an error)."""
    max_loras, max_rank = parse_max_loras(max_loras), parse_max_rank(max_rank)
    if len(modules) > max_loras:
        raise LoraError(f"{len(modules)} lora_modules for max_loras = {max_loras} slots (dynamic loading and eviction "
                        "are not supported: raise --max-loras, at most 8)")
    adapters = [load_adapter(path, cfg, max_rank, name=name) for name, path in modules.items()]  # refuse before allocating
    pool = LoraPool(cfg, max_loras, max_rank, device)
    for slot, a in enumerate(adapters):
        pool.load(slot, a)
    return pool
