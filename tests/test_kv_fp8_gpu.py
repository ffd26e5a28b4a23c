"""FP8 (e4m3) paged KV cache on gfx950: every HIP writer and reader against ops/reference.py run on the same fp8
cache, so the kernel error is the bf16 path's and the tolerances are those tests/test_kernels_gpu.py uses for the
same op (outputs: atol times v_scale).  Head configurations 32/8 and the TP shard 4/1, scale pairs (1, 1) and
(0.5, 2.0).

Cache bytes: V written from bf16 rows is bit-identical; K (RoPE: FMA contraction moves the rotated fp32 value by
about an ulp) and everything written from a GEMM's sums (accumulation order) may land on the adjacent e4m3 code, in
at most 1 % of the bytes.

Prompt attention: the flash kernel has no fp8 form -- the runner routes prompts through the paged prefill kernel
(mode 1) and the bindings refuse fp8 tensors on the flash ops; the flash cases assert exactly that.
"""
import math

import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.ops import reference as R

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
HEADS = [(32, 8), (4, 1)]
SCALES = [(1.0, 1.0), (0.5, 2.0)]


@pytest.fixture(autouse=True)
def _fresh_kernel_env():
    ops.refresh_env()
    yield
    ops.refresh_env()


def _close(a, b, atol, rtol, what=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = (err > atol + rtol * b.abs()).sum().item()
    print(f"{what}: max err {err.max().item():.4g} (atol {atol:.3g}, rtol {rtol:.3g})")
    assert bad == 0, f"{what}: {bad} / {a.numel()} elements off; max err {err.max().item():.4g}"


def _codes(c):
    """e4m3 bytes as integers ordered like their values (+0 and -0 both 0): adjacent codes differ by 1."""
    b = c.cpu().view(torch.uint8).to(torch.int32)
    return torch.where(b >= 128, -(b - 128), b)


def _bytes_close(got, want, what, cap=0.01):
    assert got.dtype == FP8 and want.dtype == FP8
    d = (_codes(got) - _codes(want)).abs()
    frac = (d > 0).float().mean().item()
    print(f"{what}: {frac * 100:.4f} % of bytes differ, largest code distance {int(d.max())}")
    assert int(d.max()) <= 1, f"{what}: a byte is {int(d.max())} codes away"
    assert frac <= cap, f"{what}: {frac * 100:.3f} % of the bytes differ"
    assert not torch.isnan(got.cpu().float()).any(), f"{what}: NaN byte"


def _bytes_equal(got, want, what):
    assert got.dtype == FP8 and torch.equal(got.cpu().view(torch.uint8), want.cpu().view(torch.uint8)), what


# ------------------------------------------------------------------------------------------------ writers
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("ks,vs", SCALES)
def test_rope_kv_write_fp8(gpu, nh, nkv, ks, vs):
    """70 rows: rows 0-31 fill page 2 in order (the 8-byte page-row V stores), rows 32-68 cross from page 4 into
    page 5 mid-page (per-element stores), row 69 is padding (slot -1).  Pages 0, 1, 3 are addressed by no slot."""
    T = 70
    g = torch.Generator().manual_seed(nh + int(ks * 10))
    qkv = (torch.randn(T, (nh + 2 * nkv) * 128, generator=g) * 1.5).bfloat16()
    pos = torch.arange(100, 100 + T, dtype=torch.int32)
    slots = torch.cat([torch.arange(64, 96), torch.arange(4 * 32 + 20, 4 * 32 + 20 + 37), torch.tensor([-1])]).to(torch.int32)
    rope = R.rope_table(1024, 1e6)
    q = torch.zeros(T, nh, 128, dtype=torch.bfloat16)
    kc, vc = torch.zeros(6, nkv, 32, 128, dtype=FP8), torch.zeros(6, nkv, 128, 32, dtype=FP8)
    qg, kg, vg = q.to(gpu), kc.to(gpu), vc.to(gpu)
    ops.rope_kv_write(qkv.to(gpu), pos.to(gpu), slots.to(gpu), rope.to(gpu), qg, kg, vg, nh, nkv, ks, vs)
    R.rope_kv_write(qkv, pos, slots, rope, q, kc, vc, nh, nkv, ks, vs)
    _close(qg, q, 2e-2, 1e-2, "q")
    _bytes_equal(vg, vc, "V bytes differ from the reference")
    _bytes_close(kg, kc, "K bytes")
    assert kc.view(torch.uint8)[2].any() and kc.view(torch.uint8)[5].any()
    for page in (0, 1, 3):
        assert not kg.view(torch.uint8)[page].any() and not vg.view(torch.uint8)[page].any(), "an unaddressed page"


GEMM_CONFIGS = {"auto": {}, "skinny-default": {"gemm_impl": "0"}, "tiled-default": {"gemm_impl": "4"}}


@pytest.mark.parametrize("cfg", sorted(GEMM_CONFIGS))
@pytest.mark.parametrize("M", [1, 9, 64, 200])
@pytest.mark.parametrize("nh,nkv,ks,vs", [(32, 8, 1.0, 1.0), (4, 1, 0.5, 2.0)])
def test_gemm_qkv_rope_fp8(gpu, monkeypatch, cfg, M, nh, nkv, ks, vs):
    monkeypatch.setenv("DSSE_KERNEL_CFG", ops.kernel_cfg_env(**GEMM_CONFIGS[cfg]))
    ops.refresh_env()
    K = 1024
    g = torch.Generator().manual_seed(M * 7 + nh)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = R.tile_weight((torch.randn((nh + 2 * nkv) * 128, K, generator=g) / 24).bfloat16())
    rope = R.rope_table(4096, 1e6)
    pos = torch.randint(0, 4000, (M,), generator=g, dtype=torch.int32)
    slots = torch.randperm(8 * 32, generator=g)[:M].to(torch.int32) + 32  # page 0 and page 9 stay unaddressed
    if M > 1:
        slots[-1] = -1
    q = torch.zeros(M, nh * 128, dtype=torch.bfloat16)
    kc, vc = torch.zeros(10, nkv, 32, 128, dtype=FP8), torch.zeros(10, nkv, 128, 32, dtype=FP8)
    qg, kg, vg = q.to(gpu), kc.to(gpu), vc.to(gpu)
    ops.gemm_qkv_rope(x.to(gpu), w.to(gpu), pos.to(gpu), slots.to(gpu), rope.to(gpu), qg, kg, vg, nh, nkv, ks, vs)
    R.gemm_qkv_rope(x, w, pos, slots, rope, q, kc, vc, nh, nkv, ks, vs)
    _close(qg, q, 3e-2, 2e-2, "q")
    _bytes_close(kg, kc, "K bytes")
    _bytes_close(vg, vc, "V bytes")
    for page in (0, 9):
        assert not kg.view(torch.uint8)[page].any() and not vg.view(torch.uint8)[page].any(), "an unaddressed page"


@pytest.mark.parametrize("op", ["rope_kv_write", "gemm_qkv_rope"])
def test_writers_saturate_at_448_without_nan(gpu, op):
    """Inputs beyond 448 x scale store +-448 (0x7e / 0xfe), never the NaN byte (0x7f / 0xff)."""
    nh, nkv, ks, vs = 4, 1, 0.5, 0.25
    rope = R.rope_table(64, 1e6)
    pos = torch.zeros(2, dtype=torch.int32)  # position 0: the rotation is the identity
    slots = torch.tensor([5, 40], dtype=torch.int32)
    kg, vg = torch.zeros(2, nkv, 32, 128, dtype=FP8, device=gpu), torch.zeros(2, nkv, 128, 32, dtype=FP8, device=gpu)
    qg = torch.zeros(2, nh * 128, dtype=torch.bfloat16, device=gpu)
    sign = torch.tensor([1.0, -1.0])[:, None]
    if op == "rope_kv_write":
        qkv = (sign * torch.full((2, (nh + 2 * nkv) * 128), 1000.0)).bfloat16()
        ops.rope_kv_write(qkv.to(gpu), pos.to(gpu), slots.to(gpu), rope.to(gpu), qg.view(2, nh, 128), kg, vg, nh, nkv,
                          ks, vs)
    else:
        x = (sign * torch.full((2, 128), 8.0)).bfloat16()
        w = R.tile_weight(torch.full(((nh + 2 * nkv) * 128, 128), 1.0).bfloat16())  # sums of +-1024
        ops.gemm_qkv_rope(x.to(gpu), w.to(gpu), pos.to(gpu), slots.to(gpu), rope.to(gpu), qg, kg, vg, nh, nkv, ks, vs)
    kb, vb = kg.cpu().view(torch.uint8), vg.cpu().view(torch.uint8)
    assert (kb[0, 0, 5] == 0x7E).all() and (kb[1, 0, 8] == 0xFE).all()
    vp0, vp1 = int(R.vperm(torch.tensor(5))), int(R.vperm(torch.tensor(8)))
    assert (vb[0, 0, :, vp0] == 0x7E).all() and (vb[1, 0, :, vp1] == 0xFE).all()
    assert not ((kb & 0x7F) == 0x7F).any() and not ((vb & 0x7F) == 0x7F).any()
    assert int((kb != 0).sum()) == 2 * 128 and int((vb != 0).sum()) == 2 * 128  # nothing else was written


# ------------------------------------------------------------------------------------------------ readers
def _attn_setup(ctxs, qlens, hq, hkv, gen):
    B = len(ctxs)
    nblk_seq = [math.ceil(c / 32) for c in ctxs]
    total = sum(nblk_seq) + 2
    perm = torch.randperm(total, generator=gen).tolist()
    kc = R.quantize_kv(torch.randn(total, hkv, 32, 128, generator=gen) * 2.0)
    vc = R.quantize_kv(torch.randn(total, hkv, 128, 32, generator=gen) * 2.0)
    bt = torch.zeros(B, max(nblk_seq) + 1, dtype=torch.int32)
    o = 0
    for b in range(B):
        bt[b, : nblk_seq[b]] = torch.tensor(perm[o:o + nblk_seq[b]], dtype=torch.int32)
        o += nblk_seq[b]
    q = torch.randn(sum(qlens), hq, 128, generator=gen).bfloat16()
    q_start = torch.tensor([sum(qlens[:b]) for b in range(B)], dtype=torch.int32)
    return kc, vc, bt, q, q_start


@pytest.mark.parametrize("hq,hkv", HEADS)
@pytest.mark.parametrize("ks,vs", SCALES)
@pytest.mark.parametrize("ctxs", [[1, 31, 32, 33, 300], [560] * 8])
@pytest.mark.parametrize("part,nparts,comb", [(128, None, "0"), (0, 4, "0"), (0, 4, "1")])
def test_decode_attention_fp8(gpu, monkeypatch, hq, hkv, ks, vs, ctxs, part, nparts, comb):
    """Mode 0 over an fp8 cache: fixed partitions of 128 keys and even partitions (part = 0, nparts = 4) merged by the
    combine kernel or the last arriver (three launches in a row: its tickets return to zero); one inactive slot."""
    monkeypatch.setenv("DSSE_KERNEL_CFG", ops.kernel_cfg_env(attn_comb=comb))
    ops.refresh_env()
    g = torch.Generator().manual_seed(sum(ctxs) + hq + part)
    B = len(ctxs)
    kc, vc, bt, q, q_start = _attn_setup(ctxs, [1] * B, hq, hkv, g)
    qlen = torch.ones(B, dtype=torch.int32)
    qlen[1] = 0  # an inactive slot: a short sequence, so the 300-key one (several pages and partitions) stays live
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    ws, wt = torch.arange(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    nparts = nparts or math.ceil(max(ctxs) / part)
    out = torch.zeros_like(q)
    R.paged_attention(0, q, kc, vc, bt, q_start, qlen, ctx, ws, wt, out, k_scale=ks, v_scale=vs)
    out_g = torch.zeros_like(q).to(gpu)
    po = torch.zeros(B * hkv * nparts * 16 * 128, device=gpu)
    pml = torch.zeros(B * hkv * nparts * 16 * 2, device=gpu)
    args = [t.to(gpu) for t in (q, kc, vc, bt, q_start, qlen, ctx, ws, wt)]
    live = qlen.bool()
    for _ in range(3 if comb == "1" else 1):
        out_g.zero_()
        ops.paged_attention(0, *args, out_g, po, pml, part, nparts, ks, vs)
        _close(out_g.cpu()[live], out[live], 1e-2 * vs, 2e-2, f"fp8 decode attention, attn_comb={comb}")


@pytest.mark.parametrize("nh,nkv,ks,vs", [(32, 8, 1.0, 1.0), (32, 8, 0.5, 2.0), (4, 1, 0.5, 2.0)])
@pytest.mark.parametrize("kwv", ["1", "2", "4"])
@pytest.mark.parametrize("M,nparts", [(9, 1), (9, 4), (64, 1), (64, 4)])
def test_folded_decode_fp8(gpu, monkeypatch, nh, nkv, ks, vs, kwv, M, nparts):
    """Mode 3 on an fp8 cache: cache bytes equal to the two-op path's (K: adjacent-code cap, FMA contraction; V from
    the same fp32 sums: bit-identical), output against the reference on the written cache, and a second step on
    the same cache whose reference reads the first step's key from the cache -- the newest key enters attention as
    its dequantised cache value."""
    # gemm_impl=2: the X-streaming GEMM leaves split-K slabs at every M here (the default dispatch takes the
    # register-streaming kernel up to 16 rows, which leaves none: mode 3 would not run at M = 9)
    monkeypatch.setenv("DSSE_KERNEL_CFG", ops.kernel_cfg_env(attn_kwv=kwv, gemm_impl="2"))
    H = 1024
    g = torch.Generator().manual_seed(M * 31 + nparts + nh)
    ctxs = torch.randint(1, 600, (M,), generator=g).tolist()
    ctxs[0] = 64  # the newest key is a page's last slot; the second step opens a new page
    kc, vc, bt, _, _ = _attn_setup([c + 1 for c in ctxs], [1] * M, nh, nkv, g)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    qlen = torch.ones(M, dtype=torch.int32)
    live = qlen.bool()
    rope = R.rope_table(1024, 1e6)
    w = R.tile_weight((torch.randn((nh + 2 * nkv) * 128, H, generator=g) / 32).bfloat16())
    part = 0 if nparts > 1 else math.ceil((max(ctxs) + 1) / 128) * 128
    qs, ws, wt = torch.arange(M, dtype=torch.int32), torch.arange(M, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    caches = {f: (kc.clone().to(gpu), vc.clone().to(gpu)) for f in (1, 0)}
    kref, vref = kc.clone(), vc.clone()
    for step in range(2):
        c = ctx + step
        pos = c - 1
        slots = torch.tensor([int(bt[b, (int(c[b]) - 1) // 32]) * 32 + (int(c[b]) - 1) % 32 for b in range(M)],
                             dtype=torch.int32)
        qlen_s, c_s, slots_s = qlen.clone(), c.clone(), slots.clone()
        qlen_s[-1], c_s[-1], slots_s[-1] = 0, 0, -1  # an inactive slot: no query, no key, no K/V write
        live = qlen_s.bool()
        x = torch.randn(M, H, generator=g).bfloat16()
        dev = [t.to(gpu) for t in (pos, slots_s, bt, qs, qlen_s, c_s, ws, wt)]
        res = {}
        for fused in (1, 0):
            monkeypatch.setenv("DSSE_KERNEL_CFG", ops.kernel_cfg_env(fused_qkv_attn=str(fused)))
            ops.refresh_env()
            k_, v_ = caches[fused]
            qg = torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16)
            out = torch.zeros(M, nh * 128, device=gpu, dtype=torch.bfloat16)
            slabs = torch.full((16 * M * (nh + 2 * nkv) * 128,), float("nan"), device=gpu)
            po = torch.zeros(M * nkv * nparts * 16 * 128, device=gpu)
            pml = torch.zeros(M * nkv * nparts * 16 * 2, device=gpu)
            S = ops.qkv_attention_decode(x.to(gpu), w.to(gpu), dev[0], dev[1], rope.to(gpu), qg, k_, v_, nh, nkv,
                                         slabs, dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], out, po, pml, part,
                                         nparts, ks, vs)
            res[fused] = (S, out.cpu().view(M, nh, 128), qg.cpu())
        assert res[0][0] == 0
        assert res[1][0] >= 1, "the folded path (mode 3) did not run"
        _bytes_close(caches[1][0], caches[0][0], f"step {step}: K bytes, folded vs two-op")
        _bytes_equal(caches[1][1], caches[0][1], f"step {step}: V bytes, folded vs two-op")
        # reference: this step's K / V written by the reference writer, then every key read from the cache
        qr = torch.zeros(M, nh * 128, dtype=torch.bfloat16)
        R.gemm_qkv_rope(x, w, pos, slots_s, rope, qr, kref, vref, nh, nkv, ks, vs)
        _bytes_close(caches[1][0], kref, f"step {step}: K bytes vs reference")
        _bytes_close(caches[1][1], vref, f"step {step}: V bytes vs reference")
        _close(res[0][2][live], qr[live], 3e-2, 2e-2, f"step {step}: q")
        # Reference attention over the kernels' own cache bytes (the reference's differ by the capped adjacent codes)
        # and the two-op path's q rows, every key -- this step's too -- read from the cache.  Two-op: the tolerance of
        # decode attention against the reference.  Folded against the two-op path: that of the bf16 folded test (the
        # newest key's score is an fp32 dot, not an MFMA column: one bf16 ulp); against the reference: the two together.
        want = torch.zeros(M, nh, 128, dtype=torch.bfloat16)
        R.paged_attention(0, res[0][2].view(M, nh, 128), caches[0][0].cpu(), caches[0][1].cpu(), bt, qs, qlen_s, c_s,
                          ws, wt, want, k_scale=ks, v_scale=vs)
        _close(res[0][1][live], want[live], 1e-2 * vs, 2e-2, f"step {step}: two-op attention out vs reference")
        _close(res[1][1][live], res[0][1][live], 1.6e-2 * vs, 1e-2, f"step {step}: folded vs two-op attention out")
        _close(res[1][1][live], want[live], 1.6e-2 * vs, 2e-2, f"step {step}: folded attention out vs reference")


def _prefill_case(gpu, hq, hkv, ctxs, qlens, ks, vs, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(ctxs)
    kc, vc, bt, q, q_start = _attn_setup(ctxs, qlens, hq, hkv, g)
    qlen, ctx = torch.tensor(qlens, dtype=torch.int32), torch.tensor(ctxs, dtype=torch.int32)
    tile = 64 // (hq // hkv)  # a mode-1 work item: 4 tiles of 16 / G queries
    ws, wt = [], []
    for b in range(B):
        for t in reversed(range(math.ceil(qlens[b] / tile))):
            ws.append(b)
            wt.append(t)
    ws, wt = torch.tensor(ws, dtype=torch.int32), torch.tensor(wt, dtype=torch.int32)
    part = math.ceil(max(ctxs) / 32) * 32
    out = torch.zeros_like(q)
    R.paged_attention(1, q, kc, vc, bt, q_start, qlen, ctx, ws, wt, out, k_scale=ks, v_scale=vs)
    return [t.to(gpu) for t in (q, kc, vc, bt, q_start, qlen, ctx, ws, wt)], part, out


@pytest.mark.parametrize("hq,hkv", HEADS)  # 4/1: one KV head (a TP = 8 rank), the group's 4 q heads in one tile
@pytest.mark.parametrize("ks,vs", SCALES)
@pytest.mark.parametrize("case", [([70, 33, 1], [70, 33, 1]),      # ragged chunks
                                  ([102], [70])])                   # ctx > q_len, the chunk starts at key 32: a page
#                                                                     boundary that is no 64-key boundary
def test_paged_prefill_fp8(gpu, hq, hkv, ks, vs, case):
    ctxs, qlens = case
    args, part, want = _prefill_case(gpu, hq, hkv, ctxs, qlens, ks, vs, sum(ctxs) + hq)
    out_g = torch.zeros_like(want).to(gpu)
    dummy = torch.zeros(1, device=gpu)
    ops.paged_attention(1, *args, out_g, dummy, dummy, part, 1, ks, vs)
    _close(out_g, want, 1e-2 * vs, 2e-2, "fp8 paged prefill attention")


@pytest.mark.parametrize("hq,hkv", HEADS)
def test_flash_ops_refuse_an_fp8_cache(gpu, hq, hkv):
    """The flash prefill kernels (mode 2 and the key split) read bf16 only: fp8 tensors are an error, not bytes read
    as bf16."""
    args, part, want = _prefill_case(gpu, hq, hkv, [70, 33, 1], [70, 33, 1], 1.0, 1.0, 9)
    out_g = torch.zeros_like(want).to(gpu)
    dummy = torch.zeros(1, device=gpu)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ops.paged_attention(2, *args, out_g, dummy, dummy, part, 1)
    q, kc, vc, bt, qs, ql, ctx, ws, wt = args
    work = torch.cat([ws[:1], wt[:1], torch.tensor([0, 1, -1], dtype=torch.int32, device=gpu)])
    comb = torch.zeros(0, dtype=torch.int32, device=gpu)
    po, pm = torch.zeros(hq * 64 * 128, device=gpu), torch.zeros(hq * 64 * 2, device=gpu)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ops.flash_prefill_split(q, kc, vc, bt, qs, ql, ctx, work, comb, out_g, po, pm, 1)
    assert not out_g.any()
    # mixed dtypes and scales on a bf16 cache are refused too
    with pytest.raises(RuntimeError, match="one dtype"):
        ops.paged_attention(1, q, kc, vc.view(torch.uint8).to(torch.bfloat16), bt, qs, ql, ctx, ws, wt, out_g, dummy,
                            dummy, part, 1)
    kb = torch.zeros(kc.shape, dtype=torch.bfloat16, device=gpu)
    vb = torch.zeros(vc.shape, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError, match="float8_e4m3fn KV cache only"):
        ops.paged_attention(1, q, kb, vb, bt, qs, ql, ctx, ws, wt, out_g, dummy, dummy, part, 1, 0.5, 2.0)


# ------------------------------------------------------------------------------------------------ runner
def _runner(device, dtype, graphs, scales=(0.5, 2.0)):
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
    from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
    from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights

    w = convert_standard(TINY, init_standard_weights(TINY, seed=1), device=device)
    for L in w.layers:
        L.k_scale, L.v_scale = scales if dtype == "fp8" else (1.0, 1.0)
    return ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device=device, use_graphs=graphs,
                       kv_cache_dtype=dtype)


PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 170)), [7] * 33]
BTS = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
LATE = (list(range(40, 77)), [30, 31, 32])  # a prompt absorbed by a mixed step (slot 3)


def _drive(r, force=None, steps=5, prompt_logits=None):
    """Prefill three prompts, decode, absorb a fourth prompt in ONE mixed step, decode on.  Returns the tokens of
    every step and, per step, the fp32 logits of the decode rows.  `force`: tokens to feed instead of the runner's
    own picks (teacher forcing: the CPU reference engine follows the GPU's stream).  `prompt_logits` (a dict, eager
    runners): receives slot -> the fp32 logits of the row that samples the prompt's first token."""
    from distributed_sse_for_llm_response_amd.engine.model_runner import PrefillSeq

    if prompt_logits is not None:
        orig = r._prefill_sample

        def spy(seqs, x, q_start, q_len, ring_row):
            for s, qs, ql in zip(seqs, q_start, q_len):
                if s.last_chunk:
                    lg = torch.zeros(1, r.w.vocab_local, dtype=torch.float32, device=x.device)
                    ops.gemm_out(x[qs + ql - 1: qs + ql].contiguous(), r.w.lm_head_t, lg)
                    prompt_logits[s.slot] = lg[0].float().cpu()
            return orig(seqs, x, q_start, q_len, ring_row)

        r._prefill_sample = spy

    for i, bt in enumerate(BTS + [LATE[1]]):
        r.block_tables[i, : len(bt)] = torch.tensor(bt, dtype=torch.int32)
    r.temperature[:4] = 0.0
    r.prefill([PrefillSeq(i, p, 0, BTS[i], True) for i, p in enumerate(PROMPTS)], ring_row=0)
    r.active[:3] = 1
    toks, logits = [], []

    def commit(n):
        ids = r.ids[:n].cpu().clone()
        toks.append(ids.tolist())
        if force is not None:
            r.ids[:n] = torch.tensor(force[len(toks) - 1][:n], dtype=torch.int32).to(r.ids.device)

    commit(3)
    for step in range(steps):
        if step == 2:
            r.mixed(4, [PrefillSeq(3, LATE[0], 0, LATE[1], True)], ring_row=int(r.ring_counter[0]))
            logits.append(r.logits[:3].float().cpu().clone())
            r.active[3] = 1
            commit(4)
        else:
            n = 3 if step < 2 else 4
            r.decode(4)
            logits.append(r.logits[:n].float().cpu().clone())
            commit(n)
    return toks, logits


@pytest.mark.parametrize("graphs", [True, False])
def test_runner_fp8_matches_the_cpu_reference_engine(gpu, monkeypatch, graphs):
    """A tiny-config ModelRunner with an fp8 cache (captured graphs: prefill, decode, one mixed step) against the CPU
    reference engine with an fp8 cache following the same tokens: at every decode row, and at the rows that sample
    the four prompts' first tokens (fp8 prefill; the mixed step's prompt), the GPU's token is within 0.1 of the
    reference's best logit (the method and GPU tolerance of tests/test_model_runner.py); pages of no block
    table stay zero.  A bf16 runner in the same process is unaffected."""
    before = _drive(_runner(gpu, "auto", graphs)) if graphs else None
    r = _runner(gpu, "fp8", graphs)
    assert r.kv.is_fp8 and r.attn_tile == 64 // (r.w.nh // r.w.nkv)
    # the dispatch itself: every attention launch of the fp8 runner (captured or eager) is the decode kernel or the
    # paged prefill kernel on fp8 tensors -- never a flash op
    modes = []
    real = ops.paged_attention
    monkeypatch.setattr(ops, "paged_attention", lambda mode, q, kc, *a, **kw: (modes.append((mode, kc.dtype)),
                                                                                real(mode, q, kc, *a, **kw))[1])
    monkeypatch.setattr(ops, "flash_prefill_split", lambda *a, **kw: pytest.fail("flash key split on an fp8 cache"))
    if graphs:
        r.capture([4])
        assert r.graphs and r.pf_graphs and r.mx_graphs, "decode, prefill and mixed graphs are captured under fp8"
    toks, _ = _drive(r)
    # (mode 1: the prompt passes; mode 0: the decode rows of the mixed step; decode steps fold it: qkv_attention_decode)
    assert {m for m, _ in modes} == {0, 1} and all(dt == FP8 for _, dt in modes), set(modes)
    monkeypatch.undo()
    c = _runner("cpu", "fp8", False)
    plog = {}
    ctoks, clogits = _drive(c, force=toks, prompt_logits=plog)
    # the prompts' first tokens: out of the fp8 prefill (slots 0-2) and of the prompt absorbed by the mixed step
    first = {0: toks[0][0], 1: toks[0][1], 2: toks[0][2], 3: toks[3][3]}
    assert sorted(plog) == [0, 1, 2, 3]
    pworst = max(float(plog[s].max() - plog[s][t]) for s, t in first.items())
    print(f"fp8 runner (graphs={graphs}): worst first-token logit gap to the CPU fp8 engine's pick {pworst:.4f}")
    assert pworst < 0.1
    worst = 0.0
    for step, rows in enumerate(clogits):
        for i in range(rows.shape[0]):
            worst = max(worst, float(rows[i].max() - rows[i][toks[step + 1][i]]))
    print(f"fp8 runner (graphs={graphs}): worst logit gap to the CPU fp8 engine's pick {worst:.4f}")
    assert worst < 0.1
    unused = [b for b in range(64) if b not in {x for bt in BTS + [LATE[1]] for x in bt}]
    assert r.kv.k.view(torch.uint8).any() and not r.kv.k.view(torch.uint8)[:, unused].any()
    assert not r.kv.v.view(torch.uint8)[:, unused].any()
    if graphs:  # the bf16 runner, again, after the fp8 runner ran in this process: the same tokens and logits
        after = _drive(_runner(gpu, "auto", graphs))
        assert after[0] == before[0] and all(torch.equal(a, b) for a, b in zip(after[1], before[1]))
