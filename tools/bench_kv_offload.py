"""Host KV tier micro-benchmarks (profiles/kv_offload.md): the kv_pages_gather / kv_pages_scatter rate at 1, 16 and 256
pages for the full model's bf16 and fp8 page (32 layers, 8 KV heads: 4 MiB / 2 MiB), and the achieved rate of the
pinned D2H / H2D copies of the same records.

    python tools/bench_kv_offload.py [--iters 20] [--blocks 512]

Rates count each byte once per direction moved (a gather reads and writes every byte: bytes / time is what is
printed, to be compared with a read-only stream's rate at twice the traffic).  One JSON line per measurement."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from distributed_sse_for_llm_response_amd import ops  # noqa: E402


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=8)
    a = ap.parse_args()
    ops.load_library(required=True)
    dev = torch.device("cuda", 0)
    L, nb, hkv = a.layers, a.blocks, a.hkv
    for name, dtype in (("bf16", torch.bfloat16), ("fp8", torch.float8_e4m3fn)):
        k = torch.zeros(L, nb, hkv, 32, 128, device=dev, dtype=dtype)
        v = torch.zeros(L, nb, hkv, 128, 32, device=dev, dtype=dtype)
        per = 2 * L * hkv * 4096 * dtype.itemsize
        for n in (1, 16, 256):
            st = torch.zeros(n, per // dtype.itemsize, device=dev, dtype=dtype)
            g = torch.Generator().manual_seed(n)
            idx = torch.randperm(nb, generator=g)[:n].to(torch.int32).to(dev)
            for op, fn in (("gather", lambda: torch.ops.dsse.kv_pages_gather(k, v, idx, st)),
                           ("scatter", lambda: torch.ops.dsse.kv_pages_scatter(st, idx, k, v))):
                med, lo, hi = _time(fn, a.iters)
                print(json.dumps({"op": op, "dtype": name, "pages": n, "bytes": n * per, "ms_median": round(med, 4),
                                  "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                                  "GBps_median": round(n * per / med / 1e6, 1), "iters": a.iters}), flush=True)
            host = torch.empty(n, per, dtype=torch.uint8).pin_memory()
            su = st.view(torch.uint8)
            for op, fn in (("d2h", lambda: host.copy_(su, non_blocking=True)),
                           ("h2d", lambda: su.copy_(host, non_blocking=True)),
                           # as the engine issues them: one copy per page (host slots are not contiguous)
                           ("d2h_per_page", lambda: [host[i].copy_(su[i], non_blocking=True) for i in range(n)]),
                           ("h2d_per_page", lambda: [su[i].copy_(host[i], non_blocking=True) for i in range(n)])):
                med, lo, hi = _time(fn, max(3, a.iters // 4))
                print(json.dumps({"op": op, "dtype": name, "pages": n, "bytes": n * per, "ms_median": round(med, 4),
                                  "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                                  "GBps_median": round(n * per / med / 1e6, 1), "iters": max(3, a.iters // 4)}),
                      flush=True)
            del host, st
        del k, v


if __name__ == "__main__":
    main()
