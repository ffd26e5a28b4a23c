"""FP8-weight decode GEMMs (csrc/kernels/gemm_w8.hip) on the GPU: the byte order (exact), every epilogue at the row
counts and K ranges where the kernel changes path, scale placement, the real Mistral-7B shapes against the bf16
kernels on the widened copy, the model runner under quantization="fp8" (graphs on and off, the 64 / 65-row bucket
boundary), and a clean pass of the checked build.  The weights are identical on both sides of every comparison, so the
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

MS = [1, 16, 17, 33, 64]   # one, two and four 16-row MFMA tiles, full and ragged
KS = [1536, 4096]          # 12 and 32 chunks: split 4 ways 3 and 8 per workgroup; unsplit 12 and 32 (ring depths 5-8)


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


def _weight(N, K, spread=0):
    """(tiled bytes, scales, row-major widened bf16, tiled widened bf16) of a seeded [N, K] weight, all on the host,
    made once per shape.  spread s > 0: row n is multiplied by 2^(s n mod 16), so the row scales span 16 octaves (a
    N(0, 1/sqrt(K)) row of these K quantises with scale 2^-12: 2^-12 .. 2^3)."""
    key = (N, K, spread)
    if key not in _WEIGHTS:
        g = torch.Generator().manual_seed(N * 7 + K)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        if spread:
            w = w * torch.ldexp(torch.ones(N), (torch.arange(N) * spread % 16).int())[:, None]
        q, s = R.quantize_weight_f8(w.bfloat16())
        wide = R.widen_weight_f8(q, s)
        _WEIGHTS[key] = (R.tile_weight_f8(q), s, wide, R.tile_weight(wide))
    return _WEIGHTS[key]


def _x(M, K, seed=0):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(M * 13 + K + seed)).bfloat16()


# ---------------------------------------------------------------- byte order
@pytest.mark.parametrize("split", [0, 1])
def test_byte_order_is_exact(gpu, monkeypatch, split):
    """One-hot rows pick single weight columns: a dropped, doubled or permuted byte, chunk or k-step changes a value."""
    _cfg(monkeypatch, w8_split=split or None)
    N, K = 512, 1536
    wq, ws, wide, _ = _weight(N, K, spread=1)
    ks = [128 * c + 8 * grp + (3 * grp + c) % 8 for c in (0, 5, K // 128 - 1) for grp in range(16)]
    assert len(set(ks)) == 48
    x = torch.zeros(len(ks), K, dtype=torch.bfloat16)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    out = torch.full((len(ks), N), float("nan"), device=gpu)
    ops.gemm_out_w8(x.to(gpu), wq.to(gpu), ws.to(gpu), out)
    want = wide.float()[:, ks].t().contiguous()
    assert torch.equal(out.cpu(), want)
    nw, S = torch.ops.dsse.gemm_w8_plan(N, K)
    assert nw in (3, 4, 7, 8) and (S == 1 if split else S > 1)


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
        _cfg(monkeypatch, w8_split=split)
        for dt, atol, rtol in ((torch.float32, 1e-3, 1e-3), (torch.bfloat16, 2e-2, 1e-2)):
            out = torch.full((M + 1, N), 7.0, device=gpu, dtype=dt)
            ops.gemm_out_w8(x.to(gpu), wq.to(gpu), ws.to(gpu), out[:M])
            _close(out[:M], ref, atol, rtol, f"gemm_out_w8 {dt} M={M} K={K} split={split}")
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
    ns = ops.gemm_resid_split_w8(x.to(gpu), dq, ds, r, part)
    assert ns > 1  # 64 tiles: K is split to fill the chip, at every row count (the narrow ones included)
    ops.rmsnorm(r, nwt.to(gpu), y, 1e-5, part=part, nsplit=ns)
    _close(r, ref_r, 1e-3, 1e-3, f"resid via slabs M={M} K={K}")
    _close(y, ref_y, 2e-2, 1e-2, f"norm over slabs M={M} K={K}")
    # the unsplit residual add
    _cfg(monkeypatch, w8_split=1)
    r = r0.clone().to(gpu)
    assert ops.gemm_resid_split_w8(x.to(gpu), dq, ds, r, part) == 0
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
        _cfg(monkeypatch, w8_split=split)
        out = torch.zeros(M, N // 2, device=gpu, dtype=torch.bfloat16)
        ops.gemm_silu_w8(x.to(gpu), wq.to(gpu), ws.to(gpu), out)
        _close(out, ref, 2e-2, 2e-2, f"gemm_silu_w8 M={M} K={K} split={split}")


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


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_qkv_slabs_into_the_folded_attention(gpu, monkeypatch, M, K):
    nh, nkv = 8, 2
    N = (nh + 2 * nkv) * 128
    wq, ws, _, wt = _weight(N, K)
    x = _x(M, K).to(gpu)
    kc, vc, bt, pos, slots, ctx, ar = _decode_case(M, nh, nkv, M + K)
    rope = R.rope_table(128, 10000.0).to(gpu)
    meta = [t.to(gpu) for t in (bt, ar, torch.ones(M, dtype=torch.int32), ctx, ar, torch.zeros(M, dtype=torch.int32))]

    def run(w8, **cfg):
        _cfg(monkeypatch, **cfg)
        k_, v_ = kc.clone().to(gpu), vc.clone().to(gpu)
        q = torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16)
        out = torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16)
        slabs = torch.full((8 * M * N,), float("nan"), device=gpu)
        po, pml = torch.zeros(M * nkv * 16 * 128, device=gpu), torch.zeros(M * nkv * 16 * 2, device=gpu)
        if w8:
            ns = ops.qkv_attention_decode_w8(x, wq.to(gpu), ws.to(gpu), pos.to(gpu), slots.to(gpu), rope, q, k_, v_, nh,
                                             nkv, slabs, *meta, out, po, pml, 128, 1)
        else:
            ns = ops.qkv_attention_decode(x, wt.to(gpu), pos.to(gpu), slots.to(gpu), rope, q, k_, v_, nh, nkv, slabs,
                                          *meta, out, po, pml, 128, 1)
        return ns, q, k_, v_, out

    # the bf16 op on the widened weight: as the dispatch runs it, and unfused (which writes q_out)
    base = {True: run(False), False: run(False, fused_qkv_attn="0")}
    assert base[False][0] == 0 and base[False][1].abs().sum() > 0
    for what, cfg, folded in (("folded", {}, True), ("unfused, reduced slabs", dict(fused_qkv_attn="0"), False),
                              ("unfused, direct epilogue", dict(fused_qkv_attn="0", w8_split=1), False)):
        ns, q, k_, v_, o = run(True, **cfg)
        assert (ns >= 1) == folded, what
        _, q0, k0, v0, o0 = base[folded]
        if not folded:  # the folded kernel takes q from the slabs and leaves q_out alone
            _close(q, q0, 2e-2, 1e-2, f"q {what} M={M} K={K}")
        _close(k_, k0, 2e-2, 1e-2, f"K pages {what} M={M} K={K}")
        _close(v_, v0, 2e-2, 1e-2, f"V pages {what} M={M} K={K}")
        _close(o, o0, 2e-2, 1e-2, f"attention {what} M={M} K={K}")
        assert not torch.equal(k_.cpu(), kc) and o.abs().sum() > 0


# ---------------------------------------------------------------- scale placement
def test_row_scales_land_on_their_columns(gpu):
    N, K, M = 512, 1536, 33
    wq, ws, _, wt = _weight(N, K, spread=5)  # neighbouring rows 5 octaves apart
    assert float(ws.min()) <= 2.0 ** -12 and float(ws.max()) >= 2.0 ** 3 and len(ws.unique()) >= 16
    x = _x(M, K, seed=5)
    ref = torch.zeros(M, N)
    R.gemm_out(x, wt, ref)
    out = torch.zeros(M, N, device=gpu)
    ops.gemm_out_w8(x.to(gpu), wq.to(gpu), ws.to(gpu), out)
    _close(out, ref, 1e-3, 1e-3, "row scales")
    # and per column in units of its own scale, so the small-scale columns are held to the same bound
    unit = ws * 2.0 ** 12
    _close(out.cpu() / unit, ref / unit, 1e-3, 1e-3, "row scales, normalised")


# ---------------------------------------------------------------- full dimensions
def _gpu_weight(N, K, gpu, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    w = torch.empty(N, K, device=gpu, dtype=torch.bfloat16).normal_(0.0, 1.0 / math.sqrt(K), generator=g)
    q, s = R.quantize_weight_f8(w)
    return R.tile_weight_f8(q), s, R.tile_weight(R.widen_weight_f8(q, s))


def test_full_mistral_dimensions_against_the_bf16_kernels(gpu):
    """qkv, o, gate_up, down and the LM head at H 4096 / F 14336 / V 32768, 64 rows: the grid mapping (waves per
    workgroup, K split, XCD numbering) is shape-specific."""
    M, H, F, V, nh, nkv = 64, 4096, 14336, 32768, 32, 8
    plans = {n: tuple(torch.ops.dsse.gemm_w8_plan(*s)) for n, s in
             dict(qkv=(6144, H), o=(H, H), gate_up=(2 * F, H), down=(H, F), lm_head=(V, H)).items()}
    assert plans == dict(qkv=(3, 2), o=(4, 4), gate_up=(7, 1), down=(4, 4), lm_head=(8, 1)), plans  # 256 workgroups each
    gx = torch.Generator(device=gpu).manual_seed(1)
    xh = torch.empty(M, H, device=gpu, dtype=torch.bfloat16).normal_(generator=gx)
    xf = torch.empty(M, F, device=gpu, dtype=torch.bfloat16).normal_(generator=gx)
    # o and down: slabs into the fused norm
    for name, (N, K), x in (("o", (H, H), xh), ("down", (H, F), xf)):
        wq, ws, wt = _gpu_weight(N, K, gpu, 10 + K)
        nwt = torch.ones(N, device=gpu, dtype=torch.bfloat16)
        res = []
        for w8 in (True, False):
            r, y = torch.zeros(M, N, device=gpu), torch.zeros(M, N, device=gpu, dtype=torch.bfloat16)
            part = torch.zeros(8 * M * N, device=gpu)
            ns = ops.gemm_resid_split_w8(x, wq, ws, r, part) if w8 else ops.gemm_resid_split(x, wt, r, part)
            ops.rmsnorm(r, nwt, y, 1e-5, part=part, nsplit=ns)
            res.append((r, y))
        _close(res[0][0], res[1][0], 1e-3, 1e-3, name)
        _close(res[0][1], res[1][1], 2e-2, 1e-2, name + " norm")
        del wq, ws, wt
    wq, ws, wt = _gpu_weight(2 * F, H, gpu, 3)
    a, b = (torch.zeros(M, F, device=gpu, dtype=torch.bfloat16) for _ in range(2))
    ops.gemm_silu_w8(xh, wq, ws, a)
    ops.gemm_silu(xh, wt, b)
    _close(a, b, 2e-2, 2e-2, "gate_up")
    del wq, ws, wt
    wq, ws, wt = _gpu_weight(V, H, gpu, 4)
    a, b = (torch.zeros(M, V, device=gpu) for _ in range(2))
    ops.gemm_out_w8(xh, wq, ws, a)
    ops.gemm_out(xh, wt, b)
    _close(a, b, 1e-3, 1e-3, "lm_head")
    del wq, ws, wt
    wq, ws, wt = _gpu_weight(6144, H, gpu, 5)
    kc, vc, bt, pos, slots, ctx, ar = _decode_case(M, nh, nkv, 9)
    rope = R.rope_table(128, 10000.0).to(gpu)
    meta = [t.to(gpu) for t in (bt, ar, torch.ones(M, dtype=torch.int32), ctx, ar, torch.zeros(M, dtype=torch.int32))]
    res = []
    for w8 in (True, False):
        k_, v_ = kc.clone().to(gpu), vc.clone().to(gpu)
        q, out = (torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16) for _ in range(2))
        slabs = torch.zeros(8 * M * 6144, device=gpu)
        po, pml = torch.zeros(M * nkv * 16 * 128, device=gpu), torch.zeros(M * nkv * 16 * 2, device=gpu)
        args = (pos.to(gpu), slots.to(gpu), rope, q, k_, v_, nh, nkv, slabs, *meta, out, po, pml, 128, 1)
        ns = ops.qkv_attention_decode_w8(xh, wq, ws, *args) if w8 else ops.qkv_attention_decode(xh, wt, *args)
        assert ns == 2 if w8 else ns >= 1
        res.append((k_, v_, out))
    for a, b, what in zip(res[0], res[1], ("qkv K pages", "qkv V pages", "qkv attention")):
        _close(a, b, 2e-2, 1e-2, what)


# ---------------------------------------------------------------- model runner
PAGES = 3
_MODEL = {}


def _widened_std(seed):
    """HF-layout weights whose matrices are already the widened FP8 values: per-row quantisation commutes with the
    engine's row permutations, so the engine quantises them to the same bytes."""
    std = init_standard_weights(TINY, seed=seed)
    wide = lambda m: R.widen_weight_f8(*R.quantize_weight_f8(m))
    out = dict(std, lm_head=wide(std["lm_head"]), layers=[])
    for L in std["layers"]:
        out["layers"].append({k: (wide(v) if k in ("q", "k", "v", "o", "gate", "up", "down") else v)
                              for k, v in L.items()})
    return std, out


def _runner(gpu, graphs, max_batch=64):
    if "std" not in _MODEL:
        _MODEL["std"] = _widened_std(3)
    std, _ = _MODEL["std"]
    w = convert_standard(TINY, std, device=gpu, quantization="fp8")
    r = ModelRunner(w, num_blocks=max_batch * PAGES + 8, max_batch=max_batch, max_model_len=256, device=gpu,
                    use_graphs=graphs)
    assert r.quantization == "fp8_e4m3"
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
    """The same 64 sequences through the 64-row bucket (FP8 kernels) and the 65-row bucket (the existing kernels over
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
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_kernels.py"), "--only", "w8"],
                       capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DSSE_KERNELS_VARIANT": "checked", "DSSE_KERNEL_CFG": ""})
    assert r.returncode == 0 and "CHECKS-OK" in r.stdout and "gemm_w8.hip: clean" in r.stdout, \
        r.stdout[-3000:] + r.stderr[-3000:]
