"""MXFP4-weight decode GEMMs (csrc/kernels/gemm_w4.hip) on the GPU: the nibble, block, chunk and k-step order (exact),
every epilogue at the row counts and K ranges where the kernel changes path, block-scale placement, the real Mistral-7B
shapes against the bf16 kernels on the widened copy, the model runner under quantization="mxfp4" (graphs on and off,
the 64 / 65-row bucket boundary), and a clean pass of the checked build.  The weights are identical on both sides of every comparison, so the
tolerances are the project's own for the matching bf16 test: only the accumulation order differs."""
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights, reference_forward
from distributed_sse_for_llm_response_amd.ops import reference as R

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn

MS = [1, 16, 17, 33, 64]   # one, two and four 16-row MFMA tiles, full and ragged
KS = [1536, 4096]          # 12 and 32 chunks: split 4 or 8 ways 3 or 4 per workgroup (fewer than the ring holds);
                           # unsplit 12 and 32 (more than the ring's 5-8 slots)


def _close(a, b, atol, rtol, what=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{what}: {bad} / {a.numel()} elements off; max err {err.max().item():.4g}"


@pytest.fixture(autouse=True)
def _fresh_kernel_env():
    ops.refresh_env()
    yield
    ops.refresh_env()


def _cfg(monkeypatch, **kw):
    """DSSE_KERNEL_CFG = exactly these keys (None = leave the key out)."""
    monkeypatch.setenv("DSSE_KERNEL_CFG", ",".join(f"{k}={v}" for k, v in kw.items() if v is not None))
    ops.refresh_env()


_WEIGHTS = {}


def _weight(N, K, spread=0, block_spread=0):
    """(tiled nibbles, tiled scale bytes, row-major widened bf16, tiled widened bf16) of a seeded [N, K] weight, all on
    the host, made once per shape.  spread s > 0: row n is multiplied by 2^(s n mod 16); block_spread b > 0: the 32-block
    j of every row by 2^-(b j mod 16) -- neighbouring rows / blocks that many octaves apart, 16 octaves in all."""
    key = (N, K, spread, block_spread)
    if key not in _WEIGHTS:
        g = torch.Generator().manual_seed(N * 7 + K)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        if spread:
            w = w * torch.ldexp(torch.ones(N), (torch.arange(N) * spread % 16).int())[:, None]
        if block_spread:
            b = torch.ldexp(torch.ones(K // 32), -(torch.arange(K // 32) * block_spread % 16).int())
            w = w * b.repeat_interleave(32)[None, :]
        q, e = R.quantize_weight_mxfp4(w.bfloat16())
        wide = R.widen_weight_mxfp4(q, e)
        _WEIGHTS[key] = (*R.tile_weight_mxfp4(q, e), wide, R.tile_weight(wide))
    return _WEIGHTS[key]


def _x(M, K, seed=0):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(M * 13 + K + seed)).bfloat16()


# ---------------------------------------------------------------- byte order
@pytest.mark.parametrize("split", [0, 1])
def test_byte_order_is_exact(gpu, monkeypatch, split):
    """One-hot rows pick single weight columns: a swapped nibble, block scale, chunk or k-step changes a value.  Chunks
    0, 5 and the last; in each, one column in every 8-column piece (a lane group's k-step), odd and even nibbles; rows
    16 octaves apart and the 32-blocks of a row 16 octaves apart, so a scale byte on the wrong block shows."""
    _cfg(monkeypatch, w4_split=split or None)
    N, K = 512, 1536
    wq, ws, wide, _ = _weight(N, K, spread=1, block_spread=5)
    ks = [128 * c + 8 * grp + (3 * grp + c) % 8 for c in (0, 5, K // 128 - 1) for grp in range(16)]
    assert len(set(ks)) == 48 and {k % 2 for k in ks} == {0, 1}
    assert len(wide.float()[:, ks].abs().log2().floor().unique()) >= 24  # the picked values span the octaves
    x = torch.zeros(len(ks), K, dtype=torch.bfloat16)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    out = torch.full((len(ks), N), float("nan"), device=gpu)
    ops.gemm_out_w4(x.to(gpu), wq.to(gpu), ws.to(gpu), out)
    want = wide.float()[:, ks].t().contiguous()
    assert torch.equal(out.cpu(), want)
    nw, S = torch.ops.dsse.gemm_w4_plan(N, K)
    assert nw in (3, 4, 6, 7, 8) and (S == 1 if split else S > 1)


# ---------------------------------------------------------------- epilogues
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_store_epilogues(gpu, monkeypatch, M, K):
    N = 512
    wq, ws, _, wt = _weight(N, K)
    x = _x(M, K)
    ref = torch.zeros(M, N)
    R.gemm_out(x, wt, ref)
    for split in (None, 1):  # the dispatch's K split (slabs + reduction), then one unsplit launch (direct epilogue)
        _cfg(monkeypatch, w4_split=split)
        for dt, atol, rtol in ((torch.float32, 1e-3, 1e-3), (torch.bfloat16, 2e-2, 1e-2)):
            out = torch.full((M + 1, N), 7.0, device=gpu, dtype=dt)
            ops.gemm_out_w4(x.to(gpu), wq.to(gpu), ws.to(gpu), out[:M])
            _close(out[:M], ref, atol, rtol, f"gemm_out_w4 {dt} M={M} K={K} split={split}")
            assert bool((out[M] == 7.0).all())  # rows past M are not written


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_split_slabs_feed_the_fused_norm_and_the_unsplit_residual_add(gpu, monkeypatch, M, K):
    N = 1024
    wq, ws, _, wt = _weight(N, K)
    x = _x(M, K)
    g = torch.Generator().manual_seed(M + K)
    r0 = torch.randn(M, N, generator=g)
    nwt = (1 + 0.1 * torch.randn(N, generator=g)).bfloat16()
    ref_r, ref_y = r0.clone(), torch.zeros(M, N, dtype=torch.bfloat16)
    R.gemm_resid(x, wt, ref_r)
    R.rmsnorm(ref_r.clone(), nwt, ref_y, 1e-5)
    dq, ds = wq.to(gpu), ws.to(gpu)
    # slabs in the layout rmsnorm_kernel<3> consumes, already scaled
    r, y = r0.clone().to(gpu), torch.zeros(M, N, device=gpu, dtype=torch.bfloat16)
    part = torch.full((8 * M * N,), float("nan"), device=gpu)
    ns = ops.gemm_resid_split_w4(x.to(gpu), dq, ds, r, part)
    assert ns > 1  # 64 tiles: K is split to fill the chip, at every row count (the narrow ones included)
    ops.rmsnorm(r, nwt.to(gpu), y, 1e-5, part=part, nsplit=ns)
    _close(r, ref_r, 1e-3, 1e-3, f"resid via slabs M={M} K={K}")
    _close(y, ref_y, 2e-2, 1e-2, f"norm over slabs M={M} K={K}")
    # the unsplit residual add
    _cfg(monkeypatch, w4_split=1)
    r = r0.clone().to(gpu)
    assert ops.gemm_resid_split_w4(x.to(gpu), dq, ds, r, part) == 0
    _close(r, ref_r, 1e-3, 1e-3, f"resid add M={M} K={K}")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_silu_epilogue(gpu, monkeypatch, M, K):
    N = 2 * 704
    wq, ws, _, wt = _weight(N, K)
    x = _x(M, K)
    ref = torch.zeros(M, N // 2, dtype=torch.bfloat16)
    R.gemm_silu(x, wt, ref)
    for split in (None, 1):
        _cfg(monkeypatch, w4_split=split)
        out = torch.zeros(M, N // 2, device=gpu, dtype=torch.bfloat16)
        ops.gemm_silu_w4(x.to(gpu), wq.to(gpu), ws.to(gpu), out)
        _close(out, ref, 2e-2, 2e-2, f"gemm_silu_w4 M={M} K={K} split={split}")


def _decode_case(M, nh, nkv, seed):
    """M sequences of 1-60 keys on two private pages each: caches, block tables and this step's metadata."""
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randint(1, 61, (M,), generator=g).int()
    kc = torch.randn(2 * M + 1, nkv, 32, 128, generator=g).bfloat16()
    vc = torch.randn(2 * M + 1, nkv, 128, 32, generator=g).bfloat16()
    bt = torch.arange(2 * M, dtype=torch.int32).view(M, 2)
    pos = ctx - 1
    slots = (bt[torch.arange(M), (pos // 32).long()] * 32 + pos % 32).int()
    ar = torch.arange(M, dtype=torch.int32)
    return kc, vc, bt, pos, slots, ctx, ar


def _f8_codes(c):
    """e4m3 bytes as integers ordered like their values (+0 and -0 both 0): adjacent codes differ by 1."""
    b = c.cpu().view(torch.uint8).to(torch.int32)
    return torch.where(b >= 128, -(b - 128), b)


def _pages_close(got, want, what):
    """bf16 pages at the bf16 epilogue tolerance; FP8 pages by tests/test_kv_fp8_gpu.py's byte criterion (the two sides
    round sums that differ in accumulation order: at most one code apart, at most 1 % of the bytes)."""
    if got.dtype != FP8:
        return _close(got, want, 2e-2, 1e-2, what)
    d = (_f8_codes(got) - _f8_codes(want)).abs()
    assert int(d.max()) <= 1 and (d > 0).float().mean().item() <= 0.01, \
        f"{what}: largest code distance {int(d.max())}, {(d > 0).float().mean().item() * 100:.3f} % of bytes differ"
    assert not torch.isnan(got.cpu().float()).any(), what


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_qkv_slabs_into_the_folded_attention(gpu, monkeypatch, M, K, kv):
    """bf16 KV: the tolerances of the FP8-weight test.  FP8 KV (scales 0.5 / 0.25): pages by the byte criterion above,
    q and the attention output at the FP8-cache tolerances of tests/test_kv_fp8_gpu.py (3e-2 / 2e-2 and 1.6e-2 v_scale
    / 1e-2): both sides hold the same weight values, so nothing wider is needed."""
    nh, nkv = 8, 2
    f8 = kv == "fp8"
    scales = (0.5, 0.25) if f8 else (1.0, 1.0)
    q_tol, o_tol = ((3e-2, 2e-2), (1.6e-2 * scales[1], 1e-2)) if f8 else ((2e-2, 1e-2), (2e-2, 1e-2))
    N = (nh + 2 * nkv) * 128
    wq, ws, _, wt = _weight(N, K)
    x = _x(M, K).to(gpu)
    kc, vc, bt, pos, slots, ctx, ar = _decode_case(M, nh, nkv, M + K)
    if f8:
        kc, vc = (kc.float() / scales[0]).to(FP8), (vc.float() / scales[1]).to(FP8)
    rope = R.rope_table(128, 10000.0).to(gpu)
    meta = [t.to(gpu) for t in (bt, ar, torch.ones(M, dtype=torch.int32), ctx, ar, torch.zeros(M, dtype=torch.int32))]

    def run(w4, **cfg):
        _cfg(monkeypatch, **cfg)
        k_, v_ = kc.clone().to(gpu), vc.clone().to(gpu)
        q = torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16)
        out = torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16)
        slabs = torch.full((8 * M * N,), float("nan"), device=gpu)
        po, pml = torch.zeros(M * nkv * 16 * 128, device=gpu), torch.zeros(M * nkv * 16 * 2, device=gpu)
        if w4:
            ns = ops.qkv_attention_decode_w4(x, wq.to(gpu), ws.to(gpu), pos.to(gpu), slots.to(gpu), rope, q, k_, v_, nh,
                                             nkv, slabs, *meta, out, po, pml, 128, 1, *scales)
        else:
            ns = ops.qkv_attention_decode(x, wt.to(gpu), pos.to(gpu), slots.to(gpu), rope, q, k_, v_, nh, nkv, slabs,
                                          *meta, out, po, pml, 128, 1, *scales)
        return ns, q, k_, v_, out

    # the bf16 op on the widened weight: as the dispatch runs it, and unfused (which writes q_out)
    base = {True: run(False), False: run(False, fused_qkv_attn="0")}
    assert base[False][0] == 0 and base[False][1].abs().sum() > 0
    for what, cfg, folded in (("folded", {}, True), ("unfused, reduced slabs", dict(fused_qkv_attn="0"), False),
                              ("unfused, direct epilogue", dict(fused_qkv_attn="0", w4_split=1), False)):
        ns, q, k_, v_, o = run(True, **cfg)
        assert (ns >= 1) == folded, what
        _, q0, k0, v0, o0 = base[folded]
        if not folded:  # the folded kernel takes q from the slabs and leaves q_out alone
            _close(q, q0, *q_tol, f"q {what} M={M} K={K}")
        _pages_close(k_, k0, f"K pages {what} M={M} K={K}")
        _pages_close(v_, v0, f"V pages {what} M={M} K={K}")
        _close(o, o0, *o_tol, f"attention {what} M={M} K={K}")
        assert not torch.equal(k_.cpu().view(torch.uint8), kc.view(torch.uint8)) and o.abs().sum() > 0


# ---------------------------------------------------------------- scale placement
@pytest.mark.parametrize("split", [0, 1])
def test_block_scales_land_on_their_blocks(gpu, monkeypatch, split):
    """Neighbouring 32-blocks of every row 5 octaves apart, 16 octaves in all.  Against the full product only the
    largest blocks would count, so X is also masked to one block position (j mod 16) at a time: then every block that
    contributes has the same scale 2^-o, the sums are compared in that unit at the fp32 tolerance, and a scale byte
    applied to a neighbouring block, a whole row or a whole chunk is off by octaves."""
    _cfg(monkeypatch, w4_split=split or None)
    N, K, M = 512, 1536, 33
    wq, we, wide, wt = _weight(N, K, block_spread=5)
    eb = R.untile_weight_mxfp4(wq, we)[1]
    assert int(eb.max()) - int(eb.min()) >= 15 and all(len(row.unique()) >= 12 for row in eb[:4])
    x = _x(M, K, seed=5)
    dq, de = wq.to(gpu), we.to(gpu)
    ref = torch.zeros(M, N)
    R.gemm_out(x, wt, ref)
    out = torch.zeros(M, N, device=gpu)
    ops.gemm_out_w4(x.to(gpu), dq, de, out)
    _close(out, ref, 1e-3, 1e-3, "block scales")
    blk = torch.arange(K) // 32
    for o in range(16):
        xm = torch.where((blk * 5 % 16 == o)[None, :], x, torch.zeros_like(x))
        ref = torch.zeros(M, N)
        R.gemm_out(xm, wt, ref)
        out = torch.zeros(M, N, device=gpu)
        ops.gemm_out_w4(xm.to(gpu), dq, de, out)
        _close(out.cpu() * 2.0 ** o, ref * 2.0 ** o, 1e-3, 1e-3, f"blocks scaled by 2^-{o}")


# ---------------------------------------------------------------- full dimensions
def _gpu_weight(N, K, gpu, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    w = torch.empty(N, K, device=gpu, dtype=torch.bfloat16).normal_(0.0, 1.0 / math.sqrt(K), generator=g)
    q, e = R.quantize_weight_mxfp4(w)
    return *R.tile_weight_mxfp4(q, e), R.tile_weight(R.widen_weight_mxfp4(q, e))


def test_full_mistral_dimensions_against_the_bf16_kernels(gpu):
    """qkv, o, gate_up, down and the LM head at H 4096 / F 14336 / V 32768, 64 rows: the grid mapping (waves per
    workgroup, K split, XCD numbering) is shape-specific."""
    M, H, F, V, nh, nkv = 64, 4096, 14336, 32768, 32, 8
    plans = {n: tuple(torch.ops.dsse.gemm_w4_plan(*s)) for n, s in
             dict(qkv=(6144, H), o=(H, H), gate_up=(2 * F, H), down=(H, F), lm_head=(V, H)).items()}
    assert plans == dict(qkv=(6, 4), o=(8, 8), gate_up=(7, 1), down=(8, 8), lm_head=(8, 1)), plans  # 256 workgroups each
    gx = torch.Generator(device=gpu).manual_seed(1)
    xh = torch.empty(M, H, device=gpu, dtype=torch.bfloat16).normal_(generator=gx)
    xf = torch.empty(M, F, device=gpu, dtype=torch.bfloat16).normal_(generator=gx)
    # o and down: slabs into the fused norm
    for name, (N, K), x in (("o", (H, H), xh), ("down", (H, F), xf)):
        wq, ws, wt = _gpu_weight(N, K, gpu, 10 + K)
        nwt = torch.ones(N, device=gpu, dtype=torch.bfloat16)
        res = []
        for w4 in (True, False):
            r, y = torch.zeros(M, N, device=gpu), torch.zeros(M, N, device=gpu, dtype=torch.bfloat16)
            part = torch.zeros(8 * M * N, device=gpu)
            ns = ops.gemm_resid_split_w4(x, wq, ws, r, part) if w4 else ops.gemm_resid_split(x, wt, r, part)
            ops.rmsnorm(r, nwt, y, 1e-5, part=part, nsplit=ns)
            res.append((r, y))
        _close(res[0][0], res[1][0], 1e-3, 1e-3, name)
        _close(res[0][1], res[1][1], 2e-2, 1e-2, name + " norm")
        del wq, ws, wt
    wq, ws, wt = _gpu_weight(2 * F, H, gpu, 3)
    a, b = (torch.zeros(M, F, device=gpu, dtype=torch.bfloat16) for _ in range(2))
    ops.gemm_silu_w4(xh, wq, ws, a)
    ops.gemm_silu(xh, wt, b)
    _close(a, b, 2e-2, 2e-2, "gate_up")
    del wq, ws, wt
    wq, ws, wt = _gpu_weight(V, H, gpu, 4)
    a, b = (torch.zeros(M, V, device=gpu) for _ in range(2))
    ops.gemm_out_w4(xh, wq, ws, a)
    ops.gemm_out(xh, wt, b)
    _close(a, b, 1e-3, 1e-3, "lm_head")
    del wq, ws, wt
    wq, ws, wt = _gpu_weight(6144, H, gpu, 5)
    kc, vc, bt, pos, slots, ctx, ar = _decode_case(M, nh, nkv, 9)
    rope = R.rope_table(128, 10000.0).to(gpu)
    meta = [t.to(gpu) for t in (bt, ar, torch.ones(M, dtype=torch.int32), ctx, ar, torch.zeros(M, dtype=torch.int32))]
    res = []
    for w4 in (True, False):
        k_, v_ = kc.clone().to(gpu), vc.clone().to(gpu)
        q, out = (torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16) for _ in range(2))
        slabs = torch.zeros(8 * M * 6144, device=gpu)
        po, pml = torch.zeros(M * nkv * 16 * 128, device=gpu), torch.zeros(M * nkv * 16 * 2, device=gpu)
        args = (pos.to(gpu), slots.to(gpu), rope, q, k_, v_, nh, nkv, slabs, *meta, out, po, pml, 128, 1)
        ns = ops.qkv_attention_decode_w4(xh, wq, ws, *args) if w4 else ops.qkv_attention_decode(xh, wt, *args)
        assert ns == plans["qkv"][1] if w4 else ns >= 1
        res.append((k_, v_, out))
    for a, b, what in zip(res[0], res[1], ("qkv K pages", "qkv V pages", "qkv attention")):
        _close(a, b, 2e-2, 1e-2, what)


# ---------------------------------------------------------------- model runner
PAGES = 3
_MODEL = {}


def _widened_std(seed):
    """HF-layout weights whose matrices are already the widened MXFP4 values: quantisation per 32 K of a row commutes
    with the engine's row permutations, so the engine quantises them to the same values."""
    std = init_standard_weights(TINY, seed=seed)
    wide = lambda m: R.widen_weight_mxfp4(*R.quantize_weight_mxfp4(m))
    out = dict(std, lm_head=wide(std["lm_head"]), layers=[])
    for L in std["layers"]:
        out["layers"].append({k: (wide(v) if k in ("q", "k", "v", "o", "gate", "up", "down") else v)
                              for k, v in L.items()})
    return std, out


def _runner(gpu, graphs, max_batch=64):
    if "std" not in _MODEL:
        _MODEL["std"] = _widened_std(3)
    std, _ = _MODEL["std"]
    w = convert_standard(TINY, std, device=gpu, quantization="mxfp4")
    r = ModelRunner(w, num_blocks=max_batch * PAGES + 8, max_batch=max_batch, max_model_len=256, device=gpu,
                    use_graphs=graphs)
    assert r.quantization == "mxfp4" and r.w4
    return r


def _prefill(r, B):
    g = torch.Generator().manual_seed(B)
    prompts = [torch.randint(3, TINY.vocab_size, (int(torch.randint(3, 61, (1,), generator=g)),), generator=g).tolist()
               for _ in range(B)]
    tables = [list(range(i * PAGES, (i + 1) * PAGES)) for i in range(B)]
    for i, bt in enumerate(tables):
        r.block_tables[i, : len(bt)] = torch.tensor(bt, dtype=torch.int32)
    r.prefill([PrefillSeq(i, p, 0, tables[i], True) for i, p in enumerate(prompts)], ring_row=0)
    r.active.zero_()
    r.active[:B] = 1
    r.temperature.zero_()
    return prompts


def _steps(r, B, bucket, n=2):
    gen, logits = [[int(t)] for t in r.ids[:B].cpu()], []
    for _ in range(n):
        r.decode(bucket)
        torch.cuda.synchronize()
        logits.append(r.logits[:B].clone())
        for i, t in enumerate(r.ids[:B].cpu()):
            gen[i].append(int(t))
    return gen, logits


def _compare(ref_row, got_row, what):  # tests/test_model_full_dims_gpu.py's criterion
    ref_row, got_row = ref_row.float(), got_row.float()
    cos = torch.nn.functional.cosine_similarity(ref_row, got_row, dim=0).item()
    rel = ((ref_row - got_row).abs().max() / ref_row.abs().max()).item()
    assert cos > 0.998 and rel < 0.05, f"{what}: cosine {cos:.5f}, max-abs err / max {rel:.4f}"


def test_runner_decode_logits_graph_and_eager(gpu):
    B = 5
    runs = {}
    for graphs in (True, False):
        r = _runner(gpu, graphs, max_batch=8)
        if graphs:
            r.capture([8])  # before any prefill: the warm-up pass writes no KV (every slot inactive)
            assert 8 in r.graphs
        prompts = _prefill(r, B)
        runs[graphs] = _steps(r, B, 8, n=3)
    assert runs[True][0] == runs[False][0], "graph and eager tokens differ"
    _, wide = _MODEL["std"]
    gen, logits = runs[True]
    for i in range(B):
        ref, _ = reference_forward(TINY, wide, torch.tensor(prompts[i] + gen[i][:3]))
        for s in range(3):
            _compare(ref[len(prompts[i]) + s], logits[s][i].cpu(), f"seq {i} step {s}")
    # the bytes were used: the unquantised model's logits are further away than the tolerance allows somewhere
    plain, _ = _MODEL["std"]
    ref, _ = reference_forward(TINY, plain, torch.tensor(prompts[0] + gen[0][:1]))
    assert not torch.allclose(ref[len(prompts[0])], logits[0][0].cpu(), atol=1e-3, rtol=1e-3)


def test_64_and_65_row_buckets_agree(gpu):
    """The same 64 sequences through the 64-row bucket (MXFP4 kernels) and the 65-row bucket (the existing kernels over
    the widened copy): identical weight values, so the logits agree at the model tolerance."""
    B = 64
    res = {}
    for bucket in (64, 65):
        r = _runner(gpu, False, max_batch=65)
        _prefill(r, B)
        res[bucket] = _steps(r, B, bucket, n=1)
    for i in range(B):
        _compare(res[65][1][0][i], res[64][1][0][i], f"seq {i}")


# ---------------------------------------------------------------- checked build
def test_checked_build_is_clean_over_the_epilogue_shapes(gpu):
    from distributed_sse_for_llm_response_amd import _build

    _build.build_kernels(variant="checked")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_kernels.py"), "--only", "w4"],
                       capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DSSE_KERNELS_VARIANT": "checked", "DSSE_KERNEL_CFG": ""})
    assert r.returncode == 0 and "CHECKS-OK" in r.stdout and "gemm_w4.hip: clean" in r.stdout, \
        r.stdout[-3000:] + r.stderr[-3000:]
