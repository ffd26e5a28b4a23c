"""Cost of logprobs / top_logprobs when used (the numbers of profiles/r8/logprobs.md).

    python tools/bench_logprobs.py [--model mistral-7b] [--streams 64] [--ctx 512] [--reps 100]

1. The three passes alone at `--streams` rows x V = 32768 with every row off, at N = 0 and at N = 20: device events
   around `--reps` back-to-back launches after a warm-up.
2. The `--streams`-stream decode step of `--model` (random-init weights, garbage KV at `--ctx` tokens of context): the
   graphs captured at startup, then the lazily captured twins with the logprob passes (their one-off capture time is
   printed) with every stream off and with every stream at N = 20, all replayed back to back in one process.
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

    B, V = a.streams, 32768
    x = (torch.randn(B, V, device=dev) * 4).clamp_(-32, 32)
    rec = torch.zeros(B, ops.LP_REC, device=dev)
    chosen = torch.zeros(B, device=dev)
    ring = torch.zeros(4, B, ops.LP_OUT, device=dev)
    ids = torch.randint(0, V, (B,), device=dev, dtype=torch.int32)
    for n in (-1, 0, 20):
        meta = torch.full((B,), n, device=dev, dtype=torch.int32)
        print(json.dumps({
            "what": "passes alone", "rows": B, "V": V, "N": n,
            "stats_us": timed_us(lambda: ops.logprob_stats(x, None, meta, None, rec, None, 0)),
            "chosen_us": timed_us(lambda: ops.logprob_chosen(x, ids, None, meta, None, chosen, 0)),
            "finish_us": timed_us(lambda: ops.logprob_finish(rec.unsqueeze(0), chosen.unsqueeze(0), None, meta, None,
                                                             ring, ring_row=0))}), flush=True)

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
    r.enable_logprobs()
    out["twin_capture_s"] = round(r.twin_capture_s, 2)
    out["twins_all_off_us"] = step_us()
    r.lp_meta.fill_(20)
    out["twins_all_N20_us"] = step_us()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
