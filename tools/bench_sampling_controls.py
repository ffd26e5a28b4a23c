"""Cost of logit_bias / min_tokens / min_p when used (the numbers of profiles/r9/sampling_controls.md).

    python tools/bench_sampling_controls.py [--model mistral-7b] [--streams 64] [--ctx 512] [--reps 100]

1. The bias and ban pass alone at `--streams` rows x V = 32768: every row neutral, every row with 300 entries and a
   17-id ban in force; device events around `--reps` back-to-back launches after a warm-up.
2. The `--streams`-stream decode step of `--model` (random-init weights, garbage KV at `--ctx` tokens of context): the
   graphs captured at startup, then the lazily captured twins (their one-off capture time is printed) with every
   stream neutral and with every stream carrying 300 bias entries, a ban in force and min_p = 0.05 at temperature 1.
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()

    import torch

    from distributed_sse_for_llm_response_amd import ops
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
    from distributed_sse_for_llm_response_amd.engine.weights import random_engine_weights
    from distributed_sse_for_llm_response_amd.models.mistral import get_config

    ops.load_library(required=True)
    dev = torch.device("cuda", 0)

    def timed_us(fn, n=a.reps, warm=10):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) / n * 1e3, 1)

    def fill(meta, body, B, vocab, until):
        """Every slot: 300 distinct ids with small biases, 17 banned ids, the ban in force until `until`."""
        g = torch.Generator().manual_seed(0)
        for s in range(B):
            ids = torch.randperm(vocab, generator=g)[:ops.CTL_BIAS + ops.CTL_BAN].to(torch.int32)
            row = torch.zeros(ops.CTL_BODY, dtype=torch.int32)
            row[0:2 * ops.CTL_BIAS:2] = ids[:ops.CTL_BIAS]
            row[1:2 * ops.CTL_BIAS:2] = (torch.rand(ops.CTL_BIAS, generator=g) - 0.5).view(torch.int32)
            row[2 * ops.CTL_BIAS:2 * ops.CTL_BIAS + ops.CTL_BAN] = ids[ops.CTL_BIAS:]
            body[s].copy_(row)
        m = torch.zeros(4 * B, dtype=torch.int32)
        m[:B], m[B:2 * B], m[2 * B:3 * B] = ops.CTL_BIAS, ops.CTL_BAN, until
        m[3 * B:].view(torch.float32).fill_(0.05)
        meta.copy_(m)

    B, V = a.streams, 32768
    x = (torch.randn(B, V, device=dev) * 4).clamp_(-32, 32)
    meta = torch.zeros(4 * B, device=dev, dtype=torch.int32)
    body = torch.zeros(B, ops.CTL_BODY, device=dev, dtype=torch.int32)
    pos = torch.zeros(B, device=dev, dtype=torch.int32)
    neutral = timed_us(lambda: ops.sample_bias_ban(x, None, meta, body, pos, None, 0, V))
    fill(meta, body, B, V, 1 << 30)
    print(json.dumps({"what": "bias and ban pass alone", "rows": B, "V": V, "all_neutral_us": neutral,
                      "all_300_entries_17_bans_us": timed_us(
                          lambda: ops.sample_bias_ban(x, None, meta, body, pos, None, 0, V))}), flush=True)

    cfg = get_config(a.model)
    w = random_engine_weights(cfg, device=dev, seed=0)
    pages = a.ctx // 32 + 2
    r = ModelRunner(w, num_blocks=B * pages + 8, max_batch=B, max_model_len=a.ctx + 64, device=dev)
    for s in range(B):
        r.block_tables[s, :pages] = torch.arange(pages * s, pages * (s + 1), dtype=torch.int32)
    r.active.fill_(1)
    r.capture([B])

    def step_us():
        r.positions.fill_(a.ctx)  # (every replay advances the positions: keep the context fixed)
        return timed_us(lambda: r.decode(B), warm=5, n=min(a.reps, 50))

    out = {"what": "decode step", "model": cfg.name, "streams": B, "ctx": a.ctx, "V_local": w.vocab_local,
           "startup_graphs_us": step_us()}
    r.temperature.fill_(1.0)  # (the loaded case below samples: its baseline is the unfiltered sampling step)
    out["startup_graphs_temperature_1_us"] = step_us()
    r.temperature.zero_()
    r.enable_controls()
    out["twin_capture_s"] = round(r.twin_capture_s, 2)
    out["twins_all_neutral_us"] = step_us()
    fill(r.ctl_meta, r.ctl_body, B, cfg.vocab_size, 1 << 30)
    r.temperature.fill_(1.0)
    out["twins_all_300_bias_ban_min_p_us"] = step_us()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
