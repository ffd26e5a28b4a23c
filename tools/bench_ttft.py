"""Time to first token for long prompts (BASELINE config 4: 8k-token prompts, TTFT + ITL, TP=1/2/4/8).

    python tools/bench_ttft.py [--prompt-len 8192] [--prompts 1] [--iters 3] [--decode-steps 16]
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 tools/bench_ttft.py ...   # config 4 at TP=8 (one rank per GPU, RCCL)

Per iteration: prefill `--prompts` fresh random prompts of `--prompt-len` tokens in chunks of
`--chunk` tokens (one engine prefill call per chunk; the tiled-layout GEMMs + the flash-prefill kernel +
paged KV writes), sample the first token, copy it to the host: that wall time is the TTFT.  Then
`--decode-steps` graph-captured decode steps give the ITL at that context length.  Rank 0 prints one
JSON line.  Random-init Mistral-7B-v0.3 weights (bf16), synthetic prompts.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cached_prefix_main(args):
    """TTFT of a prompt whose first N tokens are resident in the prefix cache, against the same engine without it.

    One runner, two engines over it, used one after the other: cache off and cache on.  Per iteration, with fresh
    random tokens: prompt 1 (`--prompt-len`) runs to its first token on both engines (a miss on the cache-on one: its
    TTFT is the cache's bookkeeping on top of a full prefill); prompt 2 = prompt 1's first N tokens + new ones runs
    on both: a full prefill with the cache off, N // 32 * 32 tokens skipped with it on.  TTFT = add_request to the
    first token event on the host (engine steps included, so it is the engine's TTFT, not the bare prefill call's)."""
    import numpy as np
    import torch

    from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
    from distributed_sse_for_llm_response_amd.engine.kv_cache import PAGE, blocks_needed
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
    from distributed_sse_for_llm_response_amd.engine.weights import random_engine_weights
    from distributed_sse_for_llm_response_amd.models.mistral import get_config

    n, keep = args.prompt_len, args.cached_prefix
    if not 0 <= keep < n:
        raise SystemExit("--cached-prefix must be in [0, --prompt-len)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    cfg = get_config(args.model)
    w = random_engine_weights(cfg, device=device, seed=7)
    max_len = n + 4 * PAGE
    r = ModelRunner(w, num_blocks=4 * blocks_needed(max_len) + 4, max_batch=2, max_model_len=max_len, device=device,
                    max_prefill_tokens=max(args.chunk, 8192), kv_cache_dtype=args.kv_dtype)
    r.capture()
    engines = {on: LLMEngine(r, eos_id=-1, prefill_budget=r.max_prefill_tokens, prefix_cache=on) for on in (False, True)}
    gen = torch.Generator().manual_seed(5)
    ids = iter(range(1 << 30))

    def ttft(e, prompt):
        torch.cuda.synchronize()
        e.ring_head = int(r.ring_counter.item())  # (the other engine advanced the runner's token ring meanwhile)
        t0 = time.perf_counter()
        e.add_request(f"r{next(ids)}", prompt, SamplingParams(temperature=0.0, max_tokens=2))
        dt, cached = None, -1
        while e.has_work():
            for ev in e.step():
                if dt is None and not ev.done:
                    dt = time.perf_counter() - t0
                if ev.done:
                    cached = ev.cached_tokens
        return dt, cached

    rows = {"off_first": [], "off_second": [], "on_miss": [], "on_hit": []}
    cached = 0
    for it in range(args.iters + 1):  # the first iteration warms up (allocator, first launches) and is dropped
        p1 = torch.randint(3, cfg.vocab_size, (n,), generator=gen).tolist()
        p2 = p1[:keep] + torch.randint(3, cfg.vocab_size, (n - keep,), generator=gen).tolist()
        a = ttft(engines[False], p1)[0]
        b = ttft(engines[False], p2)[0]
        c = ttft(engines[True], p1)[0]
        d, cached = ttft(engines[True], p2)
        if it:
            for k, v in zip(rows, (a, b, c, d)):
                rows[k].append(v)
    med = {k: round(1000 * float(np.median(v)), 3) for k, v in rows.items()}
    print(json.dumps({
        "metric": "TTFT with a cached prefix (engine add_request -> first token on the host)", "model": cfg.name,
        "prompt_len": n, "cached_prefix": keep, "cached_tokens": cached, "iters": args.iters,
        "ttft_ms_cache_off": med["off_second"], "ttft_ms_cache_on_hit": med["on_hit"],
        "ttft_ms_cache_off_first_prompt": med["off_first"], "ttft_ms_cache_on_miss": med["on_miss"],
        "all_ms": {k: [round(1000 * x, 3) for x in v] for k, v in rows.items()},
        "dtype": "bf16", "data": "synthetic prompts, random-init weights"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b-v0.3")
    ap.add_argument("--prompt-len", type=int, default=8192)
    ap.add_argument("--prompts", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--decode-steps", type=int, default=16)
    ap.add_argument("--kv-dtype", default="auto", choices=["auto", "bf16", "fp8", "fp8_e4m3"],
                    help="KV cache element type (fp8: prompts attend on the paged prefill kernel, not the flash kernel)")
    ap.add_argument("--profile-marker", action="store_true",
                    help="launch one bitwise_not kernel after the warm-up iteration: tools/trace_sum.py --after-kernel "
                         "bitwise_not then keeps only the timed iterations of a rocprofv3 kernel trace")
    ap.add_argument("--cached-prefix", type=int, default=None, metavar="N",
                    help="prefix caching: prefill one prompt, then time a second one that shares its first N tokens, "
                         "through the engine with the cache on, and the same second prompt with the cache off "
                         "(one GPU; both TTFTs in one JSON line)")
    args = ap.parse_args()
    if args.cached_prefix is not None:
        return cached_prefix_main(args)

    import numpy as np
    import torch
    import torch.distributed as dist

    from distributed_sse_for_llm_response_amd.engine.kv_cache import PAGE, blocks_needed
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
    from distributed_sse_for_llm_response_amd.engine.weights import random_engine_weights
    from distributed_sse_for_llm_response_amd.models.mistral import get_config
    from distributed_sse_for_llm_response_amd.parallel.comm import TPComm, init_distributed

    local = int(os.environ.get("LOCAL_RANK", "0"))
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    rank, local, world = init_distributed(device=device)
    comm = TPComm(rank=rank, size=world) if world > 1 else TPComm()
    cfg = get_config(args.model)
    w = random_engine_weights(cfg, tp_rank=comm.rank, tp_size=comm.size, device=device, seed=7)
    max_len = args.prompt_len + args.decode_steps + 2 * PAGE
    per = blocks_needed(max_len)
    B = max(1, args.prompts)
    r = ModelRunner(w, num_blocks=B * per + 4, max_batch=B, max_model_len=max_len, device=device, comm=comm,
                    max_prefill_tokens=max(args.chunk, 8192), kv_cache_dtype=args.kv_dtype)
    r.capture([B])
    gen = torch.Generator().manual_seed(5)

    # the slots' block tables and sampling parameters are set once, so a profiled iteration holds only the prefill
    # (and decode) kernels: no torch fill / copy kernels between the trace marker and the first prefill launch
    for s in range(B):
        r.block_tables[s, :per] = torch.tensor(list(range(s * per, (s + 1) * per)), dtype=torch.int32, device=device)
    r.temperature.fill_(1.0)
    r.top_p.fill_(1.0)
    r.active.zero_()

    def one_iter():
        seqs = []
        for s in range(B):
            blocks = list(range(s * per, (s + 1) * per))
            toks = torch.randint(3, cfg.vocab_size, (args.prompt_len,), generator=gen).tolist()
            seqs.append((s, toks, blocks))
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for start in range(0, args.prompt_len, args.chunk):
            n = min(args.chunk, args.prompt_len - start)
            last = start + n == args.prompt_len
            r.prefill([PrefillSeq(s, toks[start:start + n], start, blocks, last) for s, toks, blocks in seqs],
                      ring_row=0)
        first = r.ids[:B].cpu()  # D2H: the first token is on the host
        ttft = time.perf_counter() - t0
        if args.decode_steps:
            r.active[:B] = 1
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.decode_steps):
            r.decode(B)
        if args.decode_steps:
            r.active.zero_()
        torch.cuda.synchronize()
        itl = (time.perf_counter() - t1) / max(1, args.decode_steps)
        return ttft, itl, first

    one_iter()  # warm-up (allocator, first launches)
    if args.profile_marker:
        torch.ones(1, dtype=torch.int32, device=device).bitwise_not_()
        torch.cuda.synchronize()
    ttfts, itls = [], []
    for _ in range(args.iters):
        a, b, _ = one_iter()
        ttfts.append(a)
        itls.append(b)
    if world > 1:
        t = torch.tensor([max(ttfts), max(itls)], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        flops = 2 * 7.25e9 * args.prompt_len * B
        p50 = float(np.median(ttfts))
        print(json.dumps({
            "metric": "p50 TTFT for long prompts (+ ITL at that context)", "model": cfg.name, "tp": world,
            "prompt_len": args.prompt_len, "prompts": B, "chunk": args.chunk, "p50_ttft_ms": round(1000 * p50, 3),
            "ttfts_ms": [round(1000 * x, 3) for x in ttfts], "prefill_tokens_per_s": round(args.prompt_len * B / p50, 1),
            "dense_gemm_tflops_equiv": round(flops / p50 / 1e12, 1), "p50_itl_ms": round(1000 * float(np.median(itls)), 4),
            "dtype": "bf16", "data": "synthetic prompts, random-init weights"}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
