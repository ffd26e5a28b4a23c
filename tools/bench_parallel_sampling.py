"""Parallel sampling: time to the first token of every choice of one n = 4 request, against four separate n = 1
requests of the same prompt submitted together (profiles/parallel_sampling.md).

One runner (captured graphs), one engine, prefix cache off.  Per iteration, with fresh random prompt tokens:

* ``fork``: ``add_request(prompt, n=4)``.  One prompt pass, then three siblings on forked pages, each prefilling its
  last prompt token alone (plus one page copy when the prompt does not end a page).
* ``separate``: four ``add_request(prompt)`` calls with seeds s .. s + 3, back to back before the first step: what a
  client has to do without ``n``.

The clock runs from the first add_request to the first token event of each choice on the host (engine steps
included).  Reported: the median over the iterations of the FIRST and of the LAST choice's first token, for both.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b-v0.3")
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--kv-dtype", default="auto")
    args = ap.parse_args()

    import numpy as np
    import torch

    from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
    from distributed_sse_for_llm_response_amd.engine.kv_cache import PAGE, blocks_needed
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
    from distributed_sse_for_llm_response_amd.engine.weights import random_engine_weights
    from distributed_sse_for_llm_response_amd.models.mistral import get_config

    n, L = args.n, args.prompt_len
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    cfg = get_config(args.model)
    w = random_engine_weights(cfg, device=device, seed=7)
    max_len = L + 4 * PAGE
    r = ModelRunner(w, num_blocks=(n + 1) * blocks_needed(max_len) + 4, max_batch=max(n, 4), max_model_len=max_len,
                    device=device, kv_cache_dtype=args.kv_dtype)
    r.capture()
    e = LLMEngine(r, eos_id=-1, prefill_budget=r.max_prefill_tokens)
    gen = torch.Generator().manual_seed(5)
    ids = iter(range(1 << 30))

    def run(prompt, fork: bool):
        torch.cuda.synchronize()
        base = f"r{next(ids)}"
        sp = lambda i: SamplingParams(temperature=1.0, max_tokens=2, seed=100 + i)  # noqa: E731
        t0 = time.perf_counter()
        if fork:
            e.add_request(base, prompt, sp(0), n=n)
        else:
            for i in range(n):
                e.add_request(f"{base}-s{i}", prompt, sp(i))
        first = {}
        while e.has_work():
            for ev in e.step():
                if not ev.done and ev.conversation_id not in first:
                    first[ev.conversation_id] = time.perf_counter() - t0
        assert len(first) == n, first
        t = sorted(first.values())
        return t[0], t[-1]

    rows = {"fork_first": [], "fork_last": [], "separate_first": [], "separate_last": []}
    before = dict(e.stats)
    for it in range(args.iters + 1):  # the first iteration warms up (allocator, first launches) and is dropped
        p = torch.randint(3, cfg.vocab_size, (L,), generator=gen).tolist()
        a = run(p, True)
        b = run(p, False)
        if it:
            for k, v in zip(rows, a + b):
                rows[k].append(v)
    med = {k: round(1000 * float(np.median(v)), 3) for k, v in rows.items()}
    print(json.dumps({
        "metric": "time to the first token of every choice (first add_request -> token event on the host)",
        "model": cfg.name, "prompt_len": L, "n": n, "iters": args.iters, "kv_dtype": args.kv_dtype,
        "fork_ms_first_choice": med["fork_first"], "fork_ms_last_choice": med["fork_last"],
        "separate_ms_first_request": med["separate_first"], "separate_ms_last_request": med["separate_last"],
        "fork_shared_tokens": e.stats["fork_shared_tokens"] - before["fork_shared_tokens"],
        "fork_tail_copies": e.stats["fork_tail_copies"] - before["fork_tail_copies"],
        "all_ms": {k: [round(1000 * x, 3) for x in v] for k, v in rows.items()},
        "data": "synthetic prompts, random-init weights"}), flush=True)


if __name__ == "__main__":
    main()
