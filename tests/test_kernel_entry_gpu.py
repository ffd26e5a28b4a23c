"""The decode-graph kernels with their reordered (preloaded) arguments compute what they computed before.

The default library (kernel arguments preloaded in SGPRs) and the `nopreload` variant (the same source, arguments
fetched from the kernarg segment) run the same seeded cases in two fresh child processes (DSSE_KERNELS_VARIANT picks
the library at import; it is never swapped inside a process).  Their outputs must agree bit for bit, and the default
library's must match ops/reference.py at the tolerances tests/test_kernels_gpu.py uses for the same ops.

Shapes: the smallest at which a misplaced argument shows.  Ring GEMM: 17 rows (two row tiles, the last one partly
empty) and 64, K = 256 (2 chunks: fewer than the ring is deep) and 4096, N = 256; K split 1 / 2 / 4 on 4 waves (grid 4 x S:
the host-computed XCD renumbering for S = 2, 4) and split 2 on 8 waves (grid 2 x 2, not a multiple of 8: the plain
numbering); slab, fp32-store, residual and SiLU·mul epilogues.  Folded QKV attention: 2 sequences, GQA group 4, newest
key closing a page (ctx 32), opening one (33) and opening the third (65).  RMSNorm: 3 rows, split-K slabs 1 and 4; the
embedding gather.  decode_prep + candidates + pick + ring_advance at B = 3.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from distributed_sse_for_llm_response_amd import ops  # noqa: E402
from distributed_sse_for_llm_response_amd.ops import reference as R  # noqa: E402

# (atol, rtol) per output kind: the values of tests/test_kernels_gpu.py for the same op against the same reference
TOL = {
    "gemm_f32": (1e-3, 1e-2),     # test_gemm_ring_lds_dma
    "resid": (1e-3, 1e-3),        # test_resid_split_ring_shapes
    "y": (2e-2, 1e-2),            # every rmsnorm test
    "silu": (2e-2, 2e-2),         # test_gemm_ring_lds_dma
    "norm_resid": (1e-4, 1e-5),   # test_rmsnorm_back_to_back_modes
    "qkv": (3e-2, 2e-2),          # test_gemm_qkv_rope_and_kv_write (k / v cache)
    # folded attention vs the reference = (folded vs two-op, 1.6e-2 / 1e-2: _folded_case) + (two-op decode attention vs
    # the reference, 1e-2 / 2e-2: test_paged_attention_decode)
    "attn": (2.6e-2, 3e-2),
    "exact": (0.0, 0.0),          # integers: sampler ids, decode_prep, ring
}
RING_CFGS = [("4", "1"), ("4", "2"), ("4", "4"), ("8", "2")]  # (waves, K split)


def _cfg(dev, **kv):
    """DSSE_KERNEL_CFG for the HIP library (the reference takes no configuration)."""
    if dev.type != "cuda":
        return
    os.environ["DSSE_KERNEL_CFG"] = ",".join(f"{k}={v}" for k, v in kv.items())
    ops.refresh_env()


def run_cases(dev):
    """Every case on `dev` (cpu: ops/reference.py through the same ops entry points).  {name: (kind, cpu tensor)};
    kind None = compared between the two libraries only."""
    out = {}
    hip = dev.type == "cuda"

    # ---- ring GEMM
    N = 256
    for M in (17, 64):
        for K in (256, 4096):
            g = torch.Generator().manual_seed(M * 7 + K)
            x = torch.randn(M, K, generator=g).bfloat16()
            w = R.tile_weight((torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16())
            r0 = torch.randn(M, N, generator=g)
            for nw, S in RING_CFGS:
                if K % (128 * int(S)):
                    continue  # K = 256 has two chunks
                _cfg(dev, gemm_impl=2, s_ring=1, ring2=0, s_nw=nw, s_split=S)
                tag = f"ring M{M} K{K} nw{nw} S{S}"
                xd, wd = x.to(dev), w.to(dev)
                o = torch.zeros(M, N, device=dev)
                ops.gemm_out(xd, wd, o)
                out[f"{tag} f32"] = ("gemm_f32", o.cpu())
                h = torch.zeros(M, N // 2, device=dev, dtype=torch.bfloat16)
                ops.gemm_silu(xd, wd, h)
                out[f"{tag} silu"] = ("silu", h.cpu())
                r = r0.clone().to(dev)
                part = torch.zeros(8 * 64 * N, device=dev)
                ns = ops.gemm_resid_split(xd, wd, r, part)
                if hip:
                    assert ns == (int(S) if int(S) > 1 else 0), (tag, ns)
                    out[f"{tag} slabs"] = (None, part[: max(ns, 1) * M * N].cpu())
                # the slabs' consumer (the RMSNorm) needs H % 1024 == 0: at N = 256 the test sums them itself
                if ns:
                    r += part[: ns * M * N].view(ns, M, N).sum(0)
                out[f"{tag} resid"] = ("resid", r.cpu())

    # ---- folded QKV attention (mode 3), the 2-wave key split of the 64-stream step
    nh, nkv, H = 32, 8, 1024
    for ctxs in ([32, 33], [33, 65], [65, 32]):
        _cfg(dev, gemm_impl=2, qkv_split=2, attn_kwv=2)
        g = torch.Generator().manual_seed(sum(ctxs) * 3 + ctxs[0])
        B = len(ctxs)
        nblk = [math.ceil(c / 32) for c in ctxs]
        total = sum(nblk) + 2
        perm = torch.randperm(total, generator=g).tolist()
        kc = torch.randn(total, nkv, 32, 128, generator=g).bfloat16()
        vc = torch.randn(total, nkv, 128, 32, generator=g).bfloat16()
        bt = torch.zeros(B, max(nblk) + 1, dtype=torch.int32)
        o = 0
        for b in range(B):
            bt[b, : nblk[b]] = torch.tensor(perm[o:o + nblk[b]], dtype=torch.int32)
            o += nblk[b]
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        slots = torch.tensor([int(bt[b, (c - 1) // 32]) * 32 + (c - 1) % 32 for b, c in enumerate(ctxs)],
                             dtype=torch.int32)
        x = torch.randn(B, H, generator=g).bfloat16().to(dev)
        w = R.tile_weight((torch.randn((nh + 2 * nkv) * 128, H, generator=g) / 32).bfloat16()).to(dev)
        rope = R.rope_table(1024, 1e6, dev)
        ar = torch.arange(B, dtype=torch.int32).to(dev)
        k_, v_ = kc.to(dev), vc.to(dev)
        q = torch.zeros(B, nh * 128, device=dev, dtype=torch.bfloat16)
        att = torch.zeros(B, nh * 128, device=dev, dtype=torch.bfloat16)
        slabs = torch.full((4 * B * (nh + 2 * nkv) * 128,), float("nan"), device=dev)
        po = torch.zeros(B * nkv * 16 * 128, device=dev)
        pml = torch.zeros(B * nkv * 16 * 2, device=dev)
        S = ops.qkv_attention_decode(x, w, (ctx - 1).to(dev), slots.to(dev), rope, q, k_, v_, nh, nkv, slabs, bt.to(dev),
                                     ar, torch.ones(B, dtype=torch.int32).to(dev), ctx.to(dev), ar,
                                     torch.zeros(B, dtype=torch.int32).to(dev), att, po, pml, 128, 1)
        if hip:
            assert S == 2, f"the folded path did not run (S = {S})"
        tag = f"attn ctx{ctxs}"
        out[f"{tag} out"] = ("attn", att.cpu())
        out[f"{tag} k"] = ("qkv", k_.cpu())
        out[f"{tag} v"] = ("qkv", v_.cpu())

    # ---- RMSNorm: split-K slabs (mode 3), embedding gather (mode 2)
    _cfg(dev)
    H = 4096
    g = torch.Generator().manual_seed(5)
    nwt = (1 + 0.1 * torch.randn(H, generator=g)).bfloat16().to(dev)
    for ns in (1, 4):
        r = torch.randn(3, H, generator=g).to(dev)
        part = torch.randn(ns, 3, H, generator=g).reshape(-1).to(dev)
        y = torch.zeros(3, H, device=dev, dtype=torch.bfloat16)
        ops.rmsnorm(r, nwt, y, 1e-5, part=part, nsplit=ns)
        out[f"norm3 S{ns} resid"] = ("norm_resid", r.cpu())
        out[f"norm3 S{ns} y"] = ("y", y.cpu())
    embed = torch.randn(64, H, generator=g).bfloat16().to(dev)
    ids = torch.tensor([63, 0, 17], dtype=torch.int32).to(dev)
    r = torch.zeros(3, H, device=dev)
    y = torch.zeros(3, H, device=dev, dtype=torch.bfloat16)
    ops.rmsnorm(r, nwt, y, 1e-5, embed=embed, ids=ids)
    out["norm2 resid"] = ("norm_resid", r.cpu())
    out["norm2 y"] = ("y", y.cpu())

    # ---- decode_prep, candidates + pick, ring_advance (B = 3)
    B, V = 3, 4096
    active = torch.tensor([1, 0, 1], dtype=torch.int32).to(dev)
    positions = torch.tensor([31, 5, 32], dtype=torch.int32)
    bt = (torch.arange(B * 4, dtype=torch.int32).view(B, 4) + 3).to(dev)
    prep = [torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    ops.decode_prep(active, positions.to(dev), bt, *prep)
    for n, t in zip(("slots", "ctx_len", "q_len"), prep):
        out[f"prep {n}"] = ("exact", t.cpu())
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(B, V, generator=g) * 3).to(dev)
    t = torch.tensor([0.0, 1.0, 0.7]).to(dev)
    k = torch.tensor([0, 0, 50], dtype=torch.int32).to(dev)
    p = torch.tensor([1.0, 1.0, 0.9]).to(dev)
    seeds = torch.randint(0, 2**31 - 1, (B, 2), generator=g, dtype=torch.int32).to(dev)
    pos = positions.clone().to(dev)
    ids = torch.full((B,), -1, dtype=torch.int32, device=dev)
    ring = torch.zeros(4, B, dtype=torch.int32, device=dev)
    ctr = torch.tensor([2], dtype=torch.int32).to(dev)
    ops.sample(logits, t, k, p, seeds, positions.to(dev), None, ids, ring, ctr, pos)
    ops.ring_advance(ctr)
    for n, t_ in (("ids", ids), ("ring", ring), ("positions", pos), ("counter", ctr)):
        out[f"sample {n}"] = ("exact", t_.cpu())
    return out


def _child(path):
    ops.load_library(required=True)
    want = os.environ.get("DSSE_KERNELS_VARIANT", "")
    assert ops.library_path().name == (f"libdsse_kernels_{want}.so" if want else "libdsse_kernels.so")
    res = run_cases(torch.device("cuda", 0))
    torch.cuda.synchronize()
    torch.save(res, path)


@pytest.fixture(scope="module")
def results(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("kernel_entry")
    res = {}
    for variant in ("", "nopreload"):
        path = d / f"out_{variant or 'default'}.pt"
        env = {**os.environ, "DSSE_KERNELS_VARIANT": variant, "DSSE_AUTOBUILD": "0"}
        env.pop("DSSE_KERNEL_CFG", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(path)], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, f"variant {variant or 'default'!r}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        res[variant] = torch.load(path)
    res["ref"] = run_cases(torch.device("cpu"))
    return res


@pytest.mark.gpu
def test_preloaded_and_plain_arguments_agree_bit_for_bit(results):
    a, b = results[""], results["nopreload"]
    assert a.keys() == b.keys() and len(a) == 78  # 64 reference-checked outputs + 14 slab sets
    for name in a:
        ta, tb = a[name][1], b[name][1]
        # compared as bytes: exact about -0.0 and NaN payloads too
        assert torch.equal(ta.contiguous().view(torch.uint8), tb.contiguous().view(torch.uint8)), name


@pytest.mark.gpu
def test_preloaded_arguments_match_the_reference(results):
    got, ref = results[""], results["ref"]
    checked = 0
    for name, (kind, t) in got.items():
        if kind is None:
            continue
        atol, rtol = TOL[kind]
        want = ref[name][1].float()
        err = (t.float() - want).abs()
        bad = int((err > atol + rtol * want.abs()).sum())
        assert bad == 0, f"{name}: {bad} / {t.numel()} elements off; max err {float(err.max()):.4g}"
        checked += 1
    assert checked == 64


if __name__ == "__main__":
    _child(sys.argv[1])
