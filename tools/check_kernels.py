"""Checked-kernel run (SURVEY.md §5.2 "HIP-side bounds-check debug build").

Run with the checked library: ``DSSE_KERNELS_VARIANT=checked python tools/check_kernels.py``
(``python -m distributed_sse_for_llm_response_amd._build kernels-checked`` builds it).

1. A clean pass: the tiny Mistral through prefill + graph-captured decode must record no violation.
2. Corrupted inputs (a block-table page past the cache, a token id past the vocabulary, a KV slot past
   the cache, a RoPE position past the table) must each be caught and attributed to the right kernel
   file — without a GPU fault, because the checked build substitutes a safe index after recording.

Prints ``CHECKS-OK`` on success; exits non-zero otherwise.
"""
from __future__ import annotations

import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sse_for_llm_response_amd import ops  # noqa: E402
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq  # noqa: E402
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard  # noqa: E402
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights  # noqa: E402


def expect(fn, file: str, what: str):
    ops.kernel_checks()  # clear
    fn()
    bad = ops.kernel_checks(raise_on_error=False)
    files = [b[0] for b in bad]
    if file not in files:
        raise SystemExit(f"{what}: expected a violation in {file}, got {bad}")
    print(f"caught {what}: {[b for b in bad if b[0] == file][0]}")


def check_w8(dev):
    """The FP8-weight GEMMs (gemm_w8.hip): every epilogue over the row counts and K ranges of tests/test_w8_gpu.py must
    record nothing; a KV slot past the cache in the unfused QKV epilogue must be caught in that file."""
    from distributed_sse_for_llm_response_amd.ops import reference as R

    g = torch.Generator().manual_seed(8)
    i32 = dict(dtype=torch.int32, device=dev)
    nh, nkv = 8, 2
    ops.kernel_checks()  # clear
    for K in (1536, 4096):
        ws = {}
        for N in (512, 1024, 2 * 704, (nh + 2 * nkv) * 128):
            q, s = R.quantize_weight_f8((torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16())
            ws[N] = (R.tile_weight_f8(q).to(dev), s.to(dev))
        for M in (1, 16, 17, 33, 64):
            x = torch.randn(M, K, generator=g).bfloat16().to(dev)
            part = torch.zeros(8 * M * 1536, device=dev)
            for dt in (torch.float32, torch.bfloat16):
                ops.gemm_out_w8(x, *ws[512], torch.zeros(M, 512, device=dev, dtype=dt))
            resid = torch.zeros(M, 1024, device=dev)
            ns = ops.gemm_resid_split_w8(x, *ws[1024], resid, part)
            ops.rmsnorm(resid, torch.ones(1024, dtype=torch.bfloat16, device=dev),
                        torch.zeros(M, 1024, dtype=torch.bfloat16, device=dev), 1e-5, part=part, nsplit=ns)
            ops.gemm_resid_w8(x, *ws[1024], resid)
            ops.gemm_silu_w8(x, *ws[2 * 704], torch.zeros(M, 704, dtype=torch.bfloat16, device=dev))
            kc = torch.zeros(2 * M, nkv, 32, 128, dtype=torch.bfloat16, device=dev)
            vc = torch.zeros(2 * M, nkv, 128, 32, dtype=torch.bfloat16, device=dev)
            ar = torch.arange(M, **i32)
            pos = (ar * 7) % 60
            bt = torch.arange(2 * M, **i32).view(M, 2)
            slots = bt[ar.long(), (pos // 32).long()] * 32 + pos % 32
            rope = torch.zeros(64, 64, 2, device=dev)
            qo, out = (torch.zeros(M, nh * 128, dtype=torch.bfloat16, device=dev) for _ in range(2))
            po, pml = torch.zeros(M * nkv * 16 * 128, device=dev), torch.zeros(M * nkv * 16 * 2, device=dev)
            ops.qkv_attention_decode_w8(x, *ws[1536], pos, slots, rope, qo, kc, vc, nh, nkv, part, bt, ar,
                                        torch.ones(M, **i32), pos + 1, ar, torch.zeros(M, **i32), out, po, pml, 128, 1)
            ops.gemm_qkv_rope_w8(x, *ws[1536], pos, slots, rope, qo, kc, vc, nh, nkv)
    clean = ops.kernel_checks(raise_on_error=False)
    if clean:
        raise SystemExit(f"false positive on valid FP8-weight GEMM launches: {clean}")
    print("gemm_w8.hip: clean over the epilogue shapes")
    bad_slots = slots.clone()
    bad_slots[0] = 2 * M * 32 + 5
    # unsplit, so that the kernel's own epilogue sees the slot (the split-K reduction is a template shared by the GEMM
    # files: which file's copy runs, and records, is the linker's choice)
    saved = os.environ.get("DSSE_KERNEL_CFG")
    os.environ["DSSE_KERNEL_CFG"] = ops.kernel_cfg_env(w8_split=1)
    ops.refresh_env()
    try:
        expect(lambda: ops.gemm_qkv_rope_w8(x, *ws[1536], pos, bad_slots, rope, qo, kc, vc, nh, nkv), "gemm_w8.hip",
               "FP8 QKV epilogue: slot past the cache")
    finally:
        if saved is None:
            del os.environ["DSSE_KERNEL_CFG"]
        else:
            os.environ["DSSE_KERNEL_CFG"] = saved
        ops.refresh_env()


def check_w4(dev):
    """The MXFP4-weight GEMMs (gemm_w4.hip): every epilogue over the row counts and K ranges of tests/test_w4_gpu.py must
    record nothing; a KV slot past the cache in the unfused QKV epilogue must be caught in that file."""
    from distributed_sse_for_llm_response_amd.ops import reference as R

    g = torch.Generator().manual_seed(4)
    i32 = dict(dtype=torch.int32, device=dev)
    nh, nkv = 8, 2
    ops.kernel_checks()  # clear
    for K in (1536, 4096):
        ws = {}
        for N in (512, 1024, 2 * 704, (nh + 2 * nkv) * 128):
            q, e = R.quantize_weight_mxfp4((torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16())
            ws[N] = tuple(t.to(dev) for t in R.tile_weight_mxfp4(q, e))
        for M in (1, 16, 17, 33, 64):
            x = torch.randn(M, K, generator=g).bfloat16().to(dev)
            part = torch.zeros(8 * M * 1536, device=dev)
            for dt in (torch.float32, torch.bfloat16):
                ops.gemm_out_w4(x, *ws[512], torch.zeros(M, 512, device=dev, dtype=dt))
            resid = torch.zeros(M, 1024, device=dev)
            ns = ops.gemm_resid_split_w4(x, *ws[1024], resid, part)
            ops.rmsnorm(resid, torch.ones(1024, dtype=torch.bfloat16, device=dev),
                        torch.zeros(M, 1024, dtype=torch.bfloat16, device=dev), 1e-5, part=part, nsplit=ns)
            ops.gemm_resid_w4(x, *ws[1024], resid)
            ops.gemm_silu_w4(x, *ws[2 * 704], torch.zeros(M, 704, dtype=torch.bfloat16, device=dev))
            kc = torch.zeros(2 * M, nkv, 32, 128, dtype=torch.bfloat16, device=dev)
            vc = torch.zeros(2 * M, nkv, 128, 32, dtype=torch.bfloat16, device=dev)
            ar = torch.arange(M, **i32)
            pos = (ar * 7) % 60
            bt = torch.arange(2 * M, **i32).view(M, 2)
            slots = bt[ar.long(), (pos // 32).long()] * 32 + pos % 32
            rope = torch.zeros(64, 64, 2, device=dev)
            qo, out = (torch.zeros(M, nh * 128, dtype=torch.bfloat16, device=dev) for _ in range(2))
            po, pml = torch.zeros(M * nkv * 16 * 128, device=dev), torch.zeros(M * nkv * 16 * 2, device=dev)
            ops.qkv_attention_decode_w4(x, *ws[1536], pos, slots, rope, qo, kc, vc, nh, nkv, part, bt, ar,
                                        torch.ones(M, **i32), pos + 1, ar, torch.zeros(M, **i32), out, po, pml, 128, 1)
            ops.gemm_qkv_rope_w4(x, *ws[1536], pos, slots, rope, qo, kc, vc, nh, nkv)
    clean = ops.kernel_checks(raise_on_error=False)
    if clean:
        raise SystemExit(f"false positive on valid MXFP4-weight GEMM launches: {clean}")
    print("gemm_w4.hip: clean over the epilogue shapes")
    bad_slots = slots.clone()
    bad_slots[0] = 2 * M * 32 + 5
    # unsplit, so that the kernel's own epilogue sees the slot (the split-K reduction is a template shared by the GEMM
    # files: which file's copy runs, and records, is the linker's choice)
    saved = os.environ.get("DSSE_KERNEL_CFG")
    os.environ["DSSE_KERNEL_CFG"] = ops.kernel_cfg_env(w4_split=1)
    ops.refresh_env()
    try:
        expect(lambda: ops.gemm_qkv_rope_w4(x, *ws[1536], pos, bad_slots, rope, qo, kc, vc, nh, nkv), "gemm_w4.hip",
               "MXFP4 QKV epilogue: slot past the cache")
    finally:
        if saved is None:
            del os.environ["DSSE_KERNEL_CFG"]
        else:
            os.environ["DSSE_KERNEL_CFG"] = saved
        ops.refresh_env()


def check_lora(dev):
    """The multi-LoRA products (lora.hip): the row counts and ranks of tests/test_lora_gpu.py must record nothing; an
    adapter slot past the pool must be caught in that file (the row is then treated as having no adapter)."""
    g = torch.Generator().manual_seed(9)
    K, N, slots = 1024, 1536, 2
    ops.kernel_checks()  # clear
    for R in (8, 16, 32, 64):
        for S in (1, 2, 3):
            A = (torch.randn(slots, S * R, K, generator=g) / 32).bfloat16().to(dev)
            B = torch.randn(slots, N, R, generator=g).bfloat16().to(dev)
            sl = (torch.arange(N) * S // N).int().to(dev)
            scale = torch.ones(slots, device=dev)
            for M in (1, 16, 17, 65, 300):
                x = torch.randn(M, K, generator=g).bfloat16().to(dev)
                ra = (torch.arange(M) % (slots + 1) - 1).int().to(dev)
                t = torch.empty(M, S * R, device=dev)
                ops.lora_shrink(x, A, ra, t)
                for dt in (torch.float32, torch.bfloat16):
                    ops.lora_expand_add(t, B, scale, ra, sl, torch.zeros(M, N, device=dev, dtype=dt))
    clean = ops.kernel_checks(raise_on_error=False)
    if clean:
        raise SystemExit(f"false positive on valid LoRA launches: {clean}")
    print("lora.hip: clean over the ranks, slice counts and row counts")
    bad = ra.clone()
    bad[0] = slots + 3
    expect(lambda: ops.lora_shrink(x, A, bad, t), "lora.hip", "LoRA shrink: adapter slot past the pool")


def main():
    dev = torch.device("cuda", 0)
    ops.load_library(required=True)
    if not torch.ops.dsse.kernels_checked():
        raise SystemExit("not the checked build: set DSSE_KERNELS_VARIANT=checked")
    if sys.argv[1:] == ["--only", "w8"]:
        check_w8(dev)
        torch.cuda.synchronize()
        print("CHECKS-OK")
        return

    if sys.argv[1:] == ["--only", "w4"]:
        check_w4(dev)
        torch.cuda.synchronize()
        print("CHECKS-OK")
        return
    if sys.argv[1:] == ["--only", "lora"]:
        check_lora(dev)
        torch.cuda.synchronize()
        print("CHECKS-OK")
        return

    # ---- 1. clean model run
    cfg = TINY
    w = convert_standard(cfg, init_standard_weights(cfg, seed=1), device=dev)
    r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device=dev, use_graphs=True)
    prompts = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 170)), [7] * 33]
    bts = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
    for i, bt in enumerate(bts):
        r.block_tables[i, : len(bt)] = torch.tensor(bt, dtype=torch.int32)
    r.prefill([PrefillSeq(i, p, 0, bts[i], True) for i, p in enumerate(prompts)], ring_row=0)
    r.active[:3] = 1
    r.capture([4])
    for _ in range(6):
        r.decode(4)
    clean = ops.kernel_checks(raise_on_error=False)
    if clean:
        raise SystemExit(f"false positive on a valid model run: {clean}")
    print("clean model run: no violations")

    # ---- 2. corrupted inputs
    g = torch.Generator().manual_seed(0)
    nblk, hkv, hq = 8, 8, 32
    kc = torch.randn(nblk, hkv, 32, 128, generator=g).bfloat16().to(dev)
    vc = torch.randn(nblk, hkv, 128, 32, generator=g).bfloat16().to(dev)
    q = torch.randn(1, hq, 128, generator=g).bfloat16().to(dev)
    bt = torch.tensor([[0, 1, nblk + 1000]], dtype=torch.int32, device=dev)  # third page is past the cache
    i32 = dict(dtype=torch.int32, device=dev)
    out = torch.zeros_like(q)
    po = torch.zeros(8 * 16 * 128 * 4, device=dev)
    pml = torch.zeros(8 * 16 * 2 * 4, device=dev)

    expect(lambda: ops.paged_attention(0, q, kc, vc, bt, torch.zeros(1, **i32), torch.ones(1, **i32),
                                       torch.tensor([90], **i32), torch.zeros(1, **i32), torch.zeros(1, **i32),
                                       out, po, pml, 128, 1), "attention.hip", "decode attention: bad page id")

    qp = torch.randn(90, hq, 128, generator=g).bfloat16().to(dev)
    outp = torch.zeros_like(qp)
    expect(lambda: ops.paged_attention(2, qp, kc, vc, bt, torch.zeros(1, **i32), torch.tensor([90], **i32),
                                       torch.tensor([90], **i32), torch.zeros(math.ceil(90 / 64), **i32),
                                       torch.arange(math.ceil(90 / 64), **i32), outp, po, pml, 96, 1),
           "attention_prefill.hip", "flash prefill: bad page id")

    H = 1024
    emb = torch.randn(100, H, generator=g).bfloat16().to(dev)
    resid = torch.zeros(2, H, device=dev)
    y = torch.zeros(2, H, dtype=torch.bfloat16, device=dev)
    nw = torch.ones(H, dtype=torch.bfloat16, device=dev)
    expect(lambda: ops.rmsnorm(resid, nw, y, 1e-5, embed=emb, ids=torch.tensor([3, 100 + 7], **i32)),
           "elementwise.hip", "embedding gather: token id past the vocabulary")

    nkv, nh = 8, 32
    qkv = torch.randn(1, (nh + 2 * nkv) * 128, generator=g).bfloat16().to(dev)
    rope = torch.zeros(64, 64, 2, device=dev)
    qo = torch.zeros(1, nh, 128, dtype=torch.bfloat16, device=dev)
    expect(lambda: ops.rope_kv_write(qkv, torch.tensor([3], **i32), torch.tensor([nblk * 32 + 5], **i32), rope, qo,
                                     kc, vc, nh, nkv), "elementwise.hip", "KV write: slot past the cache")
    expect(lambda: ops.rope_kv_write(qkv, torch.tensor([64 + 9], **i32), torch.tensor([4], **i32), rope, qo,
                                     kc, vc, nh, nkv), "elementwise.hip", "RoPE: position past the table")

    act = torch.ones(1, **i32)
    expect(lambda: ops.decode_prep(act, torch.tensor([70], **i32), bt, torch.zeros(1, **i32), torch.zeros(1, **i32),
                                   torch.zeros(1, **i32), nblk), "elementwise.hip", "decode_prep: bad page id")
    check_w8(dev)
    check_lora(dev)
    check_w4(dev)
    torch.cuda.synchronize()
    print("CHECKS-OK")


if __name__ == "__main__":
    main()
