"""Step time of the decode step and of a prompt pass with and without LoRA (profiles/lora.md).

    python tools/bench_lora.py [--model mistral-7b-v0.3] [--streams 64] [--prompt-len 512] [--steps 100] [--rounds 3]

Cases, run alternately `rounds` times in one process over one set of random weights, each on a fresh runner with the
decode graph of `streams` rows captured:

  a  no LoRA pool (the default step: the code path of a server without --enable-lora)
  b  a pool of four rank-16 adapters, no request has named one (must replay the same start-up graph as a)
  c  every row on adapter 0
  d  the rows spread over the four adapters and the base model (-1, 0, 1, 2, 3, -1, ...)

and the prompt pass: one prompt of `prompt-len` tokens, eagerly replayed from its captured graph, with no pool and
under adapter 0.  Prints one JSON line: per case the median over the rounds and the spread (max - min), in ms.
The adapters are random (A ~ N(0, 1/K), B ~ N(0, 0.05^2), scale 2): the kernels' time does not depend on the values.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sse_for_llm_response_amd.engine.kv_cache import PAGE, blocks_needed  # noqa: E402
from distributed_sse_for_llm_response_amd.engine.lora import LoraPool  # noqa: E402
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq  # noqa: E402
from distributed_sse_for_llm_response_amd.engine.weights import random_engine_weights  # noqa: E402
from distributed_sse_for_llm_response_amd.models.mistral import get_config  # noqa: E402


def random_pool(cfg, dev, slots=4, rank=16):
    pool = LoraPool(cfg, slots, rank, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    for p in pool.A:
        pool.A[p].normal_(0.0, pool.A[p].shape[-1] ** -0.5, generator=g)
        pool.B[p].normal_(0.0, 0.05, generator=g)
    pool.scale.fill_(2.0)
    pool.names = [f"adapter{i}" for i in range(slots)]
    return pool


def build(w, cfg, dev, streams, prompt_len, steps, pool):
    max_len = prompt_len + steps + 2 * PAGE
    per = blocks_needed(max_len) + 1
    r = ModelRunner(w, num_blocks=streams * per + 4, max_batch=streams, max_model_len=max_len, device=dev, lora=pool,
                    max_prefill_tokens=max(2048, prompt_len))
    g = torch.Generator().manual_seed(1)
    seqs = []
    for s in range(streams):
        blocks = list(range(s * per, (s + 1) * per))
        r.block_tables[s, :per] = torch.tensor(blocks, dtype=torch.int32)
        toks = torch.randint(3, cfg.vocab_size, (prompt_len,), generator=g).tolist()
        seqs.append(PrefillSeq(slot=s, tokens=toks, start_pos=0, block_table=blocks, last_chunk=True))
    r.temperature.fill_(1.0)
    return r, seqs


def timed(fn, n, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n * 1e3


def run_case(w, cfg, dev, a, case):
    pool = None if case == "a" else random_pool(cfg, dev)
    r, seqs = build(w, cfg, dev, a.streams, a.prompt_len, a.steps + a.warmup, pool)
    adapters = {"c": [0] * a.streams, "d": [i % 5 - 1 for i in range(a.streams)]}.get(case, [-1] * a.streams)
    for s, ad in zip(seqs, adapters):
        s.adapter = ad
    r.capture([a.streams])
    if case in "cd":
        r.slot_adapter.copy_(torch.tensor(adapters, dtype=torch.int32))
        r.enable_lora()
    chunk = max(1, r.max_prefill_tokens // a.prompt_len)
    for i in range(0, a.streams, chunk):
        r.prefill(seqs[i:i + chunk], ring_row=0)
    r.active.fill_(1)
    graphs = r._graph_set()[0]
    assert (graphs is r.graphs) == (case in "ab"), "cases a and b must replay the start-up graphs, c and d the twins"
    timed(lambda: r.decode(a.streams), a.warmup, dev)
    ms = timed(lambda: r.decode(a.streams), a.steps, dev)
    out = {"step_ms": ms}
    if case in "ac":  # the prompt pass: slot 0's prompt again, from position 0 (its pages are rewritten in place)
        one = [PrefillSeq(0, seqs[0].tokens, 0, seqs[0].block_table, True, adapter=adapters[0])]
        timed(lambda: r.prefill(one, ring_row=0), 3, dev)
        out["prompt_ms"] = timed(lambda: r.prefill(one, ring_row=0), 10, dev)
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b-v0.3")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = get_config(a.model)
    w = random_engine_weights(cfg, device=dev, seed=1234)
    runs = {}
    for _ in range(a.rounds):
        for case in "abcd":
            for k, v in run_case(w, cfg, dev, a, case).items():
                runs.setdefault(f"{case}_{k}", []).append(v)
            print(json.dumps({k: [round(x, 4) for x in v] for k, v in runs.items()}), file=sys.stderr, flush=True)
    res = {k: {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4),
               "runs": [round(x, 4) for x in v]} for k, v in runs.items()}
    print(json.dumps({"model": cfg.name, "streams": a.streams, "prompt_len": a.prompt_len, "steps": a.steps,
                      "rounds": a.rounds, "cases": res}))


if __name__ == "__main__":
    main()
