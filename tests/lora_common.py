"""Synthetic PEFT adapters for the LoRA tests: generated from a seed, written with safetensors, never downloaded."""
import json
import math

import torch

from distributed_sse_for_llm_response_amd.engine.lora import TARGET_MODULES, module_shapes

_PART = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
         "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}


def adapter_tensors(cfg, seed, r=4, modules=TARGET_MODULES, b_std=0.05):
    """{PEFT key: bf16 tensor}: A ~ N(0, 1 / in), B ~ N(0, b_std^2) (a trained adapter's B is not zero)."""
    g = torch.Generator().manual_seed(seed)
    sh, out = module_shapes(cfg), {}
    for li in range(cfg.num_layers):
        for m in modules:
            o, i = sh[m]
            p = f"base_model.model.model.layers.{li}.{_PART[m]}.{m}."
            out[p + "lora_A.weight"] = (torch.randn(r, i, generator=g) / math.sqrt(i)).bfloat16()
            out[p + "lora_B.weight"] = (torch.randn(o, r, generator=g) * b_std).bfloat16()
    return out


def write_adapter(path, cfg, seed, r=4, alpha=None, modules=TARGET_MODULES, tensors=None, **config):
    """A PEFT directory at `path`; `config` overrides adapter_config.json fields.  Returns str(path)."""
    from safetensors.torch import save_file

    path.mkdir(parents=True, exist_ok=True)
    ac = {"peft_type": "LORA", "r": r, "lora_alpha": 2 * r if alpha is None else alpha, "bias": "none",
          "target_modules": list(modules), "use_rslora": False, "use_dora": False, "modules_to_save": None}
    ac.update(config)
    (path / "adapter_config.json").write_text(json.dumps(ac))
    save_file(adapter_tensors(cfg, seed, r, modules) if tensors is None else tensors,
              str(path / "adapter_model.safetensors"))
    return str(path)
