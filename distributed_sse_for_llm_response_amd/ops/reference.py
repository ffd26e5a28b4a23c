"""Plain-PyTorch fp32 reference implementations of every engine op.

These define the exact semantics (including the engine's permuted weight/cache layouts) that the
gfx950 HIP kernels in ``csrc/kernels`` implement.  They serve two purposes:

* numerics oracle: every GPU kernel test compares the HIP op against the function here;
* CPU execution: the engine, scheduler and server run end-to-end on CPU tensors for the
  plumbing tests (no GPU in the build container).  On a GPU tensor the HIP op always runs — there
  is no silent fallback (see ``ops/__init__.py``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

PAGE = 32  # KV-cache page size in tokens (kBS in csrc/kernels/api.h)
HEAD_DIM = 128


# ---------------------------------------------------------------- layouts
def rotary_perm() -> torch.Tensor:
    """perm[c] = head dim stored in permuted column c of a 128-wide head unit.

    Inside each 16-column tile j: columns 0..7 hold dims 8j..8j+7 and columns 8..15 hold dims
    64+8j..64+8j+7, so the rotary partners (d, d+64) are 8 lanes apart in the MFMA output tile.
    """
    c = torch.arange(HEAD_DIM)
    j, rr = c // 16, c % 16
    return torch.where(rr < 8, 8 * j + rr, 64 + 8 * j + (rr - 8))


def gate_up_perm(F: int) -> torch.Tensor:
    """Row order of the fused gate/up weight: tile t = [gate 8t..8t+7, up 8t..8t+7] (up at +F)."""
    c = torch.arange(2 * F)
    t, rr = c // 16, c % 16
    return torch.where(rr < 8, 8 * t + rr, F + 8 * t + (rr - 8))


def vperm(off: torch.Tensor) -> torch.Tensor:
    """Position of token `off` (0..31) inside a transposed V page row."""
    return ((off & 15) >> 2) * 8 + ((off >> 4) & 1) * 4 + (off & 3)


def tile_weight(w: torch.Tensor) -> torch.Tensor:
    """Row-major [N, K] weight -> the decode GEMMs' tiled layout (same shape, permuted storage).

    Blocks of (16-row tile T, 128-column chunk c) are stored contiguously in (T, c) order; inside a
    block, element [s][lane][j] with lane = r + 16 g holds W[16T + r][128c + 32g + 8s + j], i.e. the
    MFMA B fragment of k-step s (csrc/kernels/api.h kTileChunk), so every weight load instruction of
    the decode GEMM reads 1 KiB contiguous.
    """
    N, K = w.shape
    assert N % 16 == 0 and K % 128 == 0, (N, K)
    return w.reshape(N // 16, 16, K // 128, 4, 4, 8).permute(0, 2, 4, 3, 1, 5).contiguous().view(N, K)


def untile_weight(wt: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`tile_weight`."""
    N, K = wt.shape
    return wt.reshape(N // 16, K // 128, 4, 4, 16, 8).permute(0, 4, 1, 3, 2, 5).reshape(N, K)


def rope_table(max_pos: int, theta: float, device=None) -> torch.Tensor:
    """[max_pos, 64, 2] fp32 (cos, sin) for the rotate-half convention, head_dim 128."""
    inv = theta ** (-torch.arange(0, HEAD_DIM, 2, dtype=torch.float64) / HEAD_DIM)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).float().to(device)


def _unpermute_units(y: torch.Tensor, n_units: int) -> torch.Tensor:
    """[M, n_units*128] permuted columns -> [M, n_units, 128] in natural head-dim order."""
    perm = rotary_perm().to(y.device)
    yu = y.view(y.shape[0], n_units, HEAD_DIM)
    out = torch.empty_like(yu)
    out[:, :, perm] = yu
    return out


def _rope(x: torch.Tensor, positions: torch.Tensor, rope: torch.Tensor) -> torch.Tensor:
    """x [M, U, 128] natural order -> rotated (rotate-half)."""
    cs = rope[positions.long()]  # [M, 64, 2]
    cos, sin = cs[..., 0][:, None, :], cs[..., 1][:, None, :]
    x1, x2 = x[..., :64], x[..., 64:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


# ---- FP8 (e4m3fn) KV cache: the one definition of what a cache byte holds --------------------------------------
# Stored value = x / scale, per-layer fp32 scalars k_scale / v_scale; used value = stored * scale.  Quantisation is
# clamp(x * (1 / scale), -448, 448) in fp32, then ONE round-to-nearest-even to e4m3fn, taken from the fp32 value
# (the rotated K, the summed V) -- never from a bf16 copy of it.  The clamp is explicit: torch's own cast gives NaN
# above 464.  A key or value enters attention only as its dequantised cache value.
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def is_fp8(cache: torch.Tensor) -> bool:
    return cache.dtype == FP8


def quantize_kv(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """fp32 values -> e4m3fn cache elements (x / scale, clamped to +-448, rounded once)."""
    inv = torch.tensor(1.0 / float(scale), dtype=torch.float32, device=x.device)  # 1 / scale rounded to fp32, as the kernels get it
    return (x.float() * inv).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def dequantize_kv(c: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """Cache elements -> the fp32 values attention uses (bf16 cache: the values themselves)."""
    return c.float() * float(scale) if is_fp8(c) else c.float()


def _to_cache(x: torch.Tensor, cache: torch.Tensor, scale: float) -> torch.Tensor:
    return quantize_kv(x, scale) if is_fp8(cache) else x.to(cache.dtype)


def _write_kv(k: torch.Tensor, v: torch.Tensor, slots: torch.Tensor, k_cache, v_cache, k_scale=1.0, v_scale=1.0):
    """k, v: [M, Hkv, 128] (natural order) -> paged caches at `slots` (skip slot < 0)."""
    for m in range(k.shape[0]):
        s = int(slots[m])
        if s < 0:
            continue
        blk, off = s // PAGE, s % PAGE
        k_cache[blk, :, off, :] = _to_cache(k[m], k_cache, k_scale)
        v_cache[blk, :, :, int(vperm(torch.tensor(off)))] = _to_cache(v[m], v_cache, v_scale)


# ---------------------------------------------------------------- GEMMs
# The decode GEMMs take their weight in the tiled layout (tile_weight), like the HIP kernels.
def gemm_out(x, w, out):
    out.copy_((x.float() @ untile_weight(w).float().t()).to(out.dtype))


def gemm_resid(x, w, resid):
    resid.add_(x.float() @ untile_weight(w).float().t())


def gemm_silu(x, w, out):
    y = (x.float() @ untile_weight(w).float().t()).view(x.shape[0], -1, 2, 8)
    g, u = y[:, :, 0, :], y[:, :, 1, :]
    out.copy_((torch.nn.functional.silu(g) * u).reshape(x.shape[0], -1).to(out.dtype))


def gemm_qkv_rope(x, w, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0, v_scale=1.0):
    M = x.shape[0]
    y = x.float() @ untile_weight(w).float().t()
    qkv = _unpermute_units(y, nh + 2 * nkv)
    rot = _rope(qkv[:, : nh + nkv], positions[:M], rope)
    q_out.view(-1)[: M * nh * HEAD_DIM].copy_(rot[:, :nh].reshape(-1).to(q_out.dtype))
    _write_kv(rot[:, nh:], qkv[:, nh + nkv:], slots[:M], k_cache, v_cache, k_scale, v_scale)


# ---- FP8 (e4m3fn) weights, W8A16: the one definition of what a weight byte holds ---------------------------------
# value = bf16(byte) * scale[row].  One fp32 scale per output row, a power of two: the smallest 2^e with
# absmax(row) / 2^e <= 448 (a zero row: 1), so dividing by it is exact, the quotient never saturates, and the ONE
# rounding is torch's round-to-nearest-even cast to e4m3fn (v_cvt_pk_fp8_f32's).  Every e4m3 value is exact in bf16 and
# a power of two only moves the exponent, so widen_weight_f8 is exact in bf16 too: the FP8 kernels (bytes widened in
# registers, accumulator times scale) and the bf16 kernels over the widened copy multiply by identical weight values.
def quantize_weight_f8(w: torch.Tensor):
    """w [N, K] -> (q float8_e4m3fn [N, K] row-major, scale fp32 [N])."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    _, e = torch.frexp(amax / FP8_MAX)  # amax / 448 ~ m 2^e with m in [0.5, 1): 2^e is the scale unless m == 0.5
    s = torch.ldexp(torch.ones_like(amax), e)
    # settle the candidate against amax itself (the quotient above is rounded); products with 2^e are exact
    s = torch.where(FP8_MAX * (s * 0.5) >= amax, s * 0.5, s)
    s = torch.where(FP8_MAX * s < amax, s * 2.0, s)
    scale = torch.where(amax > 0, s, torch.ones_like(amax))
    return (wf / scale[:, None]).to(FP8), scale


def widen_weight_f8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The bf16 weight the FP8 bytes stand for (exact): bf16(q) * scale, row-major [N, K]."""
    return (q.view(FP8).float() * scale.float()[:, None]).to(torch.bfloat16)


def tile_weight_f8(q: torch.Tensor) -> torch.Tensor:
    """Row-major [N, K] e4m3 bytes -> the byte form of the tiled layout (same shape and dtype, permuted storage).

    The same (16-row tile T, 128-column chunk c) blocks as tile_weight, block-major (T, c), 2 KiB each; inside a block
    byte [h][lane][b] with lane = r + 16 g holds Wq[16T + r][128c + 32g + 16h + b]: a lane's 16 bytes are contiguous
    and widen to its MFMA B fragments of k-steps 2h and 2h + 1 (csrc/kernels/api.h kTileChunkF8).
    """
    N, K = q.shape
    assert N % 16 == 0 and K % 128 == 0, (N, K)
    b = q.view(torch.uint8).reshape(N // 16, 16, K // 128, 4, 2, 16).permute(0, 2, 4, 3, 1, 5).contiguous()
    return b.view(N, K).view(q.dtype)


def untile_weight_f8(qt: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`tile_weight_f8`."""
    N, K = qt.shape
    b = qt.view(torch.uint8).reshape(N // 16, K // 128, 2, 4, 16, 16).permute(0, 4, 1, 3, 2, 5).reshape(N, K)
    return b.contiguous().view(qt.dtype)


def _widened_tiled(wq, ws):
    """The tiled bf16 weight of tiled FP8 bytes + scales: what the bf16 reference GEMMs take."""
    return tile_weight(widen_weight_f8(untile_weight_f8(wq), ws))


def gemm_out_w8(x, wq, ws, out):
    gemm_out(x, _widened_tiled(wq, ws), out)


def gemm_resid_w8(x, wq, ws, resid):
    gemm_resid(x, _widened_tiled(wq, ws), resid)


def gemm_silu_w8(x, wq, ws, out):
    gemm_silu(x, _widened_tiled(wq, ws), out)


def gemm_qkv_rope_w8(x, wq, ws, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0, v_scale=1.0):
    gemm_qkv_rope(x, _widened_tiled(wq, ws), positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale)


# ---- MXFP4 weights (OCP e2m1 elements, one e8m0 scale per 32 consecutive K), W4A16: the one definition of what a
# stored nibble and scale byte mean.  value = e2m1(nibble) * 2^(scale byte - 127).  Nibble code: bit 3 sign, bits 2-1
# exponent, bit 0 mantissa, i.e. magnitudes FP4_GRID[code & 7]; a value that rounds to zero stores code 0, never 8.  The
# byte at [n, k / 2] holds element k (even) in its low nibble and element k + 1 in its high nibble.  The block scale is
# the smallest power of two s with 6 s >= amax(block), so the quotient never saturates and the ONE rounding is to the
# e2m1 grid, to nearest with ties to the even code.  Every e2m1 value has two significant bits and a power of two only
# moves the exponent, so widen_weight_mxfp4 is exact in bf16: the 4-bit kernels (v_cvt_scalef32_pk_bf16_fp4 in
# registers) and the bf16 kernels over the widened copy multiply by identical weight values.
FP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
FP4_MAX = 6.0
MX_BLOCK = 32
E8M0_BIAS, E8M0_MIN, E8M0_MAX = 127, 63, 191  # scale bytes are clamped to 2^-64 .. 2^64


def quantize_weight_mxfp4(w: torch.Tensor):
    """w [N, K] (K % 128 == 0, N % 16 == 0) -> (q uint8 [N, K / 2] row-major nibble pairs, e uint8 [N, K / 32])."""
    N, K = w.shape
    assert N % 16 == 0 and K % 128 == 0, (N, K)
    blk = w.float().reshape(N, K // MX_BLOCK, MX_BLOCK)
    amax = blk.abs().amax(dim=2)
    _, ex = torch.frexp(amax / FP4_MAX)  # amax / 6 ~ m 2^ex with m in [0.5, 1): 2^ex is the scale unless m == 0.5
    s = torch.ldexp(torch.ones_like(amax), ex)
    # settle the candidate against amax itself (the quotient above is rounded); products with 2^ex are exact
    s = torch.where(FP4_MAX * (s * 0.5) >= amax, s * 0.5, s)
    s = torch.where(FP4_MAX * s < amax, s * 2.0, s)
    _, es = torch.frexp(s)  # s = 0.5 * 2^es
    e = (es - 1 + E8M0_BIAS).clamp(E8M0_MIN, E8M0_MAX)
    e = torch.where(amax > 0, e, torch.full_like(e, E8M0_BIAS))
    v = blk / torch.ldexp(torch.ones_like(amax), e - E8M0_BIAS)[:, :, None]
    a = v.abs()
    grid = torch.tensor(FP4_GRID, device=w.device)
    mids = (grid[:-1] + grid[1:]) * 0.5
    lo = torch.bucketize(a, mids, right=False)  # a value on a midpoint goes down ...
    hi = torch.bucketize(a, mids, right=True)   # ... or up: take the even code of the two
    code = torch.where((lo != hi) & (lo % 2 == 1), hi, lo)
    code = torch.where((v < 0) & (code > 0), code + 8, code).to(torch.uint8).reshape(N, K)
    return code[:, 0::2] | (code[:, 1::2] << 4), e.to(torch.uint8)


def widen_weight_mxfp4(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """The bf16 weight the nibbles and scale bytes stand for (exact), row-major [N, K]."""
    N, K = q.shape[0], q.shape[1] * 2
    code = torch.stack((q & 15, q >> 4), dim=2).reshape(N, K).long()
    mag = torch.tensor(FP4_GRID, device=q.device)[code & 7]
    val = torch.where(code >= 8, -mag, mag).reshape(N, K // MX_BLOCK, MX_BLOCK)
    s = torch.ldexp(torch.ones(e.shape, device=q.device), e.int() - E8M0_BIAS)
    return (val * s[:, :, None]).reshape(N, K).to(torch.bfloat16)


def tile_weight_mxfp4(q: torch.Tensor, e: torch.Tensor):
    """Row-major (q [N, K / 2], e [N, K / 32]) -> the device layout (csrc/kernels/api.h kTileChunkF4 / kTileScaleF4):
    two tensors of the same shapes and dtype, permuted storage, over the (16-row tile T, 128-column chunk c) blocks of
    tile_weight, block-major (T, c).  Nibbles, 1 KiB per block: [lane = r + 16 g][16 bytes] = the bytes of
    W[16T + r][128c + 32g .. 32g + 31], one MX block.  Scales, 64 B per block: byte [lane] = that block's scale."""
    N, K = q.shape[0], q.shape[1] * 2
    assert N % 16 == 0 and K % 128 == 0 and e.shape == (N, K // MX_BLOCK), (q.shape, e.shape)
    qt = q.reshape(N // 16, 16, K // 128, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(N, K // 2)
    et = e.reshape(N // 16, 16, K // 128, 4).permute(0, 2, 3, 1).contiguous().view(N, K // MX_BLOCK)
    return qt, et


def untile_weight_mxfp4(qt: torch.Tensor, et: torch.Tensor):
    """Inverse of :func:`tile_weight_mxfp4`."""
    N, K = qt.shape[0], qt.shape[1] * 2
    q = qt.reshape(N // 16, K // 128, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K // 2)
    e = et.reshape(N // 16, K // 128, 4, 16).permute(0, 3, 1, 2).reshape(N, K // MX_BLOCK)
    return q.contiguous(), e.contiguous()


def _widened_tiled_f4(wq, we):
    """The tiled bf16 weight of tiled MXFP4 nibbles + scale bytes: what the bf16 reference GEMMs take."""
    return tile_weight(widen_weight_mxfp4(*untile_weight_mxfp4(wq, we)))


def gemm_out_w4(x, wq, we, out):
    gemm_out(x, _widened_tiled_f4(wq, we), out)


def gemm_resid_w4(x, wq, we, resid):
    gemm_resid(x, _widened_tiled_f4(wq, we), resid)


def gemm_silu_w4(x, wq, we, out):
    gemm_silu(x, _widened_tiled_f4(wq, we), out)


def gemm_qkv_rope_w4(x, wq, we, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0, v_scale=1.0):
    gemm_qkv_rope(x, _widened_tiled_f4(wq, we), positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale,
                  v_scale)


def rope_kv_write(qkv, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0, v_scale=1.0):
    T = qkv.shape[0]
    u = _unpermute_units(qkv.float(), nh + 2 * nkv)
    rot = _rope(u[:, : nh + nkv], positions[:T], rope)
    q_out.view(-1)[: T * nh * HEAD_DIM].copy_(rot[:, :nh].reshape(-1).to(q_out.dtype))
    _write_kv(rot[:, nh:], u[:, nh + nkv:], slots[:T], k_cache, v_cache, k_scale, v_scale)


def silu_mul(gu, h):
    y = gu.float().view(gu.shape[0], -1, 2, 8)
    h.copy_((torch.nn.functional.silu(y[:, :, 0]) * y[:, :, 1]).reshape(gu.shape[0], -1).to(h.dtype))


# ---------------------------------------------------------------- norms
def rmsnorm(resid, w, y, eps, delta=None, embed=None, ids=None, part=None, nsplit=0):
    M = y.shape[0]
    H = y.shape[1]
    if embed is not None:
        resid[:M] = embed[ids[:M].long()].float()
    elif delta is not None:
        resid[:M] += delta[:M].float()
    elif part is not None and nsplit > 0:
        resid[:M] += part.view(-1)[: nsplit * M * H].view(nsplit, M, H).sum(0)
    r = resid[:M]
    y.copy_((r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w.float()).to(y.dtype))


def decode_prep(active, positions, block_tables, slots, ctx_len, q_len, num_blocks: int = 2**31 - 1):
    B = active.numel()
    for b in range(B):
        if int(active[b]):
            pos = int(positions[b])
            slots[b] = int(block_tables[b, pos // PAGE]) * PAGE + pos % PAGE
            ctx_len[b] = pos + 1
            q_len[b] = 1
        else:
            slots[b] = -1
            ctx_len[b] = 0
            q_len[b] = 0


def ring_advance(counter):
    counter += 1


# ---------------------------------------------------------------- KV page movers (host tier of the prefix cache)
def _page_bytes(k_cache, v_cache, staging):
    """uint8 views: the caches as [L, blocks, seg] and staging as [records, 2 (K | V), L, seg] (bytes only, so one
    code path serves bf16 and fp8 caches)."""
    L, nb = k_cache.shape[:2]
    kb, vb = k_cache.view(torch.uint8).view(L, nb, -1), v_cache.view(torch.uint8).view(L, nb, -1)
    return kb, vb, staging.view(torch.uint8).view(staging.shape[0], 2, L, kb.shape[2])


def kv_pages_gather(k_cache, v_cache, blocks, staging):
    """staging[i] = [K layer 0 .. L-1 | V layer 0 .. L-1] of page blocks[i]."""
    kb, vb, sb = _page_bytes(k_cache, v_cache, staging)
    idx, n = blocks.long(), blocks.numel()
    if n:
        sb[:n, 0] = kb[:, idx].transpose(0, 1)
        sb[:n, 1] = vb[:, idx].transpose(0, 1)


def kv_pages_scatter(staging, blocks, k_cache, v_cache):
    """Page blocks[i] = staging[i] (the inverse of kv_pages_gather)."""
    kb, vb, sb = _page_bytes(k_cache, v_cache, staging)
    idx, n = blocks.long(), blocks.numel()
    if n:
        kb[:, idx] = sb[:n, 0].transpose(0, 1)
        vb[:, idx] = sb[:n, 1].transpose(0, 1)


def kv_pages_copy(k_cache, v_cache, pairs):
    """Page pairs[i][1] = page pairs[i][0], every layer, K and V (bytes only: bf16 and fp8 caches alike).  The sources
    are read before anything is written, as on the device, where no destination is a source."""
    if pairs.numel() == 0:
        return
    L, nb = k_cache.shape[:2]
    src, dst = pairs[:, 0].long(), pairs[:, 1].long()
    for c in (k_cache, v_cache):
        b = c.view(torch.uint8).view(L, nb, -1)
        b[:, dst] = b[:, src].clone()


# ---------------------------------------------------------------- attention
def gather_kv(k_cache, v_cache, block_table, n, k_scale=1.0, v_scale=1.0):
    """Keys/values 0..n-1 of one sequence in natural order: ([n, Hkv, 128], [n, Hkv, 128]); an fp8 cache is
    dequantised (stored * scale)."""
    ks, vs = [], []
    pos_of_tok = vperm(torch.arange(PAGE)).to(v_cache.device)  # natural token t lives at pos_of_tok[t]
    for p in range((n + PAGE - 1) // PAGE):
        blk = int(block_table[p])
        ks.append(k_cache[blk].permute(1, 0, 2).float())               # [32, Hkv, 128]
        vs.append(v_cache[blk][:, :, pos_of_tok].permute(2, 0, 1).float())  # [32, Hkv, 128]
    K, V = torch.cat(ks)[:n], torch.cat(vs)[:n]
    if is_fp8(k_cache):
        K, V = K * float(k_scale), V * float(v_scale)
    return K, V


def paged_attention(mode, q, k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work_seq, work_tile,
                    out, part_o=None, part_ml=None, part=0, nparts=1, k_scale=1.0, v_scale=1.0):
    """Causal GQA attention of each sequence's queries over its paged keys (all work items)."""
    hq, hkv = q.shape[1], k_cache.shape[1]
    G = hq // hkv
    seqs = sorted(set(int(b) for b in work_seq.tolist()))
    for b in seqs:
        ql, ctx = int(q_len[b]), int(ctx_len[b])
        if ql <= 0:
            continue
        qs = int(q_start[b])
        K, V = gather_kv(k_cache, v_cache, block_tables[b], ctx, k_scale, v_scale)
        K = K.repeat_interleave(G, dim=1)  # [ctx, hq, 128]
        V = V.repeat_interleave(G, dim=1)
        Q = q[qs: qs + ql].float()          # [ql, hq, 128]
        s = torch.einsum("qhd,khd->hqk", Q, K) / math.sqrt(HEAD_DIM)
        qpos = torch.arange(ctx - ql, ctx)[:, None]
        kpos = torch.arange(ctx)[None, :]
        s = s.masked_fill((kpos > qpos)[None].to(s.device), float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hqk,khd->qhd", p, V)
        out[qs: qs + ql] = o.to(out.dtype)


# ---------------------------------------------------------------- sampling
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 on uint64 numpy arrays holding uint32 values (matches common.h)."""
    c0, c1, c2, c3 = (np.asarray(a, dtype=np.uint64) & _U32 for a in (c0, c1, c2, c3))
    k0 = np.uint64(k0 & _U32)
    k1 = np.uint64(k1 & _U32)
    for _ in range(10):
        p0 = np.uint64(_M0) * c0
        p1 = np.uint64(_M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(_U32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(_U32)
        c0, c1, c2, c3 = (hi1 ^ c1 ^ k0) & np.uint64(_U32), lo1, (hi0 ^ c3 ^ k1) & np.uint64(_U32), lo0
        k0 = np.uint64((int(k0) + _W0) & _U32)
        k1 = np.uint64((int(k1) + _W1) & _U32)
    return c0, c1, c2, c3


def gumbel_noise(seed_lo: int, seed_hi: int, position: int, gidx: np.ndarray) -> np.ndarray:
    x, _, _, _ = philox4x32(gidx, np.full_like(gidx, position), np.full_like(gidx, 0x5353), np.zeros_like(gidx),
                            seed_lo, seed_hi)
    u = ((x >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    return -np.log(-np.log(u))


def _kept_mask(xb2: torch.Tensor, top_k: int, top_p: float, min_p: float = 0.0) -> torch.Tensor:
    """Elements kept by min_p, top-k, then top-p (ties at the boundary kept), on base-2 scaled logits.  min_p keeps
    x_i - max_j x_j >= log2(min_p); the three sets are top sets of one ordering, top-p's mass is the survivors'."""
    keep = torch.ones_like(xb2, dtype=torch.bool)
    if min_p > 0.0:
        keep &= xb2 >= xb2.max() + math.log2(min(min_p, 1.0))
    if 0 < top_k < xb2.numel():
        kth = torch.topk(xb2, top_k).values[-1]
        keep &= xb2 >= kth
    if top_p < 1.0:
        xmax = xb2.max()
        w = torch.where(keep, torch.exp2(xb2 - xmax), torch.zeros_like(xb2))
        z = w.sum()
        vals, order = torch.sort(torch.where(keep, xb2, torch.full_like(xb2, float("-inf"))), descending=True)
        cum = torch.cumsum(torch.exp2(vals - xmax).nan_to_num(0.0), 0)
        n_keep = int(torch.searchsorted(cum, top_p * z).clamp(max=vals.numel() - 1)) + 1
        thr = vals[n_keep - 1]
        keep &= xb2 >= thr
    return keep


def sample_row(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, seed: tuple, position: int,
               vocab_offset: int = 0, min_p: float = 0.0):
    """Returns (score, global index) exactly as the HIP sampler computes them."""
    x = logits.double()
    if not temperature > 0:
        i = int(torch.argmax(x))
        return float(x[i]), i + vocab_offset
    xb2 = (x / temperature) * (1.0 / math.log(2.0))
    keep = _kept_mask(xb2, top_k, top_p, min_p)
    gidx = np.arange(x.numel(), dtype=np.uint64) + np.uint64(vocab_offset)
    g = torch.from_numpy(gumbel_noise(seed[0], seed[1], position, gidx))
    sc = torch.where(keep, xb2 * math.log(2.0) + g, torch.full_like(xb2, float("-inf")))
    i = int(torch.argmax(sc))
    return float(sc[i]), i + vocab_offset


def sample_candidates(logits, temperature, top_k, top_p, seeds, positions, active, cand, vocab_offset=0,
                      ctl_meta=None, row_slot=None):
    """cand [B, C, 2]: the whole-row best goes to chunk 0, other chunks get -inf (same final pick).  With ctl_meta
    (sample_candidates_min_p): min_p of row b = ctl_meta's fourth column at slot row_slot[b] (else b)."""
    B = logits.shape[0]
    min_p = ctl_meta.view(-1)[3 * (ctl_meta.numel() // 4):].view(torch.float32) if ctl_meta is not None else None
    sd = seeds.reshape(-1).tolist()
    cand[..., 0] = float("-inf")
    cand[..., 1] = 0.0
    for b in range(B):
        if active is not None and not int(active[b]):
            continue
        seed = (sd[2 * b] & _U32, sd[2 * b + 1] & _U32)
        mp = float(min_p[int(row_slot[b]) if row_slot is not None else b]) if min_p is not None else 0.0
        sc, idx = sample_row(logits[b], float(temperature[b]), int(top_k[b]), float(top_p[b]), seed,
                             int(positions[b]), vocab_offset, mp)
        cand[b, 0, 0] = sc
        cand[b, 0, 1] = float(idx)  # CPU encoding: the index as a float value (GPU: its bit pattern)


def sample_pick(cand_all, active, next_ids, ring=None, ring_counter=None, positions_inc=None, vocab: int = 2**31 - 1):
    world, B, C, _ = cand_all.shape
    for b in range(B):
        if active is not None and not int(active[b]):
            continue
        best, bidx = float("-inf"), None
        for w in range(world):
            for c in range(C):
                s, i = float(cand_all[w, b, c, 0]), int(cand_all[w, b, c, 1])
                if s > best or (s == best and (bidx is None or i < bidx)):
                    best, bidx = s, i
        next_ids[b] = bidx
        if ring is not None:
            ring[int(ring_counter[0]) % ring.shape[0], b] = bidx
        if positions_inc is not None:
            positions_inc[b] += 1


def sample(logits, temperature, top_k, top_p, seeds, positions, active, next_ids, ring=None, ring_counter=None,
           positions_inc=None):
    cand = torch.empty(logits.shape[0], 1, 2)
    sample_candidates(logits, temperature, top_k, top_p, seeds, positions, active, cand)
    sample_pick(cand.unsqueeze(0), active, next_ids, ring, ring_counter, positions_inc)


def prefill_sample_gather(x, meta, slot_meta, xl, smeta):
    """CPU twin of sampler.hip prefill_sample_gather_kernel: meta = [rows | slots | last_pos (NS each) | n | ring_row],
    slot_meta = [active | temperature | top_k | top_p | seeds x 2] (Bm each) -> xl rows, smeta = [active | temperature |
    top_k | top_p | seeds x 2 | position] (NS each)."""
    NS, Bm = xl.shape[0], slot_meta.numel() // 6
    n = int(meta[3 * NS])
    xl.zero_()
    smeta.zero_()
    for i in range(NS):
        on = i < n
        slot = int(meta[NS + i]) if on else 0
        if on:
            xl[i] = x[int(meta[i])]
        smeta[i] = 1 if on else 0
        smeta[NS + i] = slot_meta[Bm + slot]
        smeta[2 * NS + i] = slot_meta[2 * Bm + slot]
        smeta[3 * NS + i] = slot_meta[3 * Bm + slot]
        smeta[4 * NS + 2 * i] = slot_meta[4 * Bm + 2 * slot]
        smeta[4 * NS + 2 * i + 1] = slot_meta[4 * Bm + 2 * slot + 1]
        smeta[6 * NS + i] = int(meta[2 * NS + i]) if on else 0


def prefill_sample_commit(meta, new_ids, ids, ring, positions):
    NS = new_ids.numel()
    n, row = int(meta[3 * NS]), int(meta[3 * NS + 1])
    for i in range(min(n, NS)):
        slot = int(meta[NS + i])
        ids[slot] = new_ids[i]
        ring[row, slot] = new_ids[i]
        positions[slot] = int(meta[2 * NS + i]) + 1


# ---- presence / frequency / repetition penalties (sampler.hip sample_penalty_kernel and the history append) ----
# Per-slot state: pen_meta int32 [4 Bm] = [presence | frequency | repetition (float32 bits) | n_prompt] and
# hist int32 [Bm, capacity + 1]: word 0 = tokens held, then the prompt followed by the generated tokens.
def _pen_params(pen_meta, slot: int):
    Bm = pen_meta.numel() // 4
    f = pen_meta.view(torch.float32)
    return float(f[slot]), float(f[Bm + slot]), float(f[2 * Bm + slot]), int(pen_meta[3 * Bm + slot])


def penalties_on(pen_meta, slot: int) -> bool:
    p, f, r, _ = _pen_params(pen_meta, slot)
    return p != 0.0 or f != 0.0 or r != 1.0


def sample_penalties(logits, active, pen_meta, hist, row_slot=None, vocab_offset=0, vocab: int = 2**31 - 1):
    """In place on logits [B, V] (row b = slot row_slot[b], else b), in the logits' own dtype; with c[v] = the
    occurrences of v among the generated tokens: every v in the prompt or generated gets x = x / r if x > 0 else
    x * r; then x -= f c[v]; then x -= p where c[v] > 0.  Inactive rows and rows whose parameters are neutral
    (p = f = 0, r = 1) are not touched; history tokens outside [vocab_offset, vocab_offset + V) are skipped."""
    B, V = logits.shape
    for b in range(B):
        if active is not None and not int(active[b]):
            continue
        slot = int(row_slot[b]) if row_slot is not None else b
        if not penalties_on(pen_meta, slot):
            continue
        p, f, r, n_prompt = _pen_params(pen_meta, slot)
        n = min(max(int(hist[slot, 0]), 0), hist.shape[1] - 1)
        toks = hist[slot, 1:1 + n].tolist()
        seen, cnt = set(), {}
        for j, t in enumerate(toks):
            v = t - vocab_offset
            if not 0 <= v < V:
                continue
            seen.add(v)
            if j >= n_prompt:
                cnt[v] = cnt.get(v, 0) + 1
        for v in seen:
            x = logits[b, v]
            if r != 1.0:
                x = x / r if x > 0 else x * r
            c = cnt.get(v, 0)
            x = x - f * c
            if c > 0:
                x = x - p
            logits[b, v] = x


# ---- logit_bias / min_tokens / stop_token_ids (sampler.hip sample_bias_ban_kernel) ----
# ctl_meta int32 [4 Bm] = [bias entries | banned ids | ban-until position | min_p (float32 bits)] per slot; ctl_body
# int32 [Bm, CTL_BODY]: CTL_BIAS x (global id, bias float32 bits), then CTL_BAN banned global ids.
CTL_BIAS, CTL_BAN = 300, 17
CTL_BODY = 2 * CTL_BIAS + CTL_BAN + 3


def sample_bias_ban(logits, active, ctl_meta, ctl_body, positions, row_slot=None, vocab_offset=0,
                    vocab: int = 2**31 - 1):
    """In place on logits [B, V] (row b = slot row_slot[b], else b), in fp32: x[id] += bias for the slot's entries,
    then, while positions[b] + 1 < ban_until, x[id] = -inf for its banned ids.  Inactive rows and rows whose slot
    has no entry and no ban in force are not touched; ids outside [vocab_offset, vocab_offset + V) are skipped."""
    B, V = logits.shape
    Bm = ctl_meta.numel() // 4
    for b in range(B):
        if active is not None and not int(active[b]):
            continue
        slot = int(row_slot[b]) if row_slot is not None else b
        nb = min(max(int(ctl_meta[slot]), 0), CTL_BIAS)
        nban = min(max(int(ctl_meta[Bm + slot]), 0), CTL_BAN)
        if int(positions[b]) + 1 >= int(ctl_meta[2 * Bm + slot]):
            nban = 0
        if nb == 0 and nban == 0:
            continue
        ids = ctl_body[slot, 0:2 * nb:2].tolist()
        bias = ctl_body[slot, 1:2 * nb:2].contiguous().view(torch.float32)
        for j, t in enumerate(ids):
            v = t - vocab_offset
            if 0 <= v < V and 0 <= t < vocab:
                logits[b, v] = logits[b, v] + bias[j]
        for t in ctl_body[slot, 2 * CTL_BIAS:2 * CTL_BIAS + nban].tolist():
            v = t - vocab_offset
            if 0 <= v < V and 0 <= t < vocab:
                logits[b, v] = float("-inf")


# ---- guided decoding (sampler.hip guide_live_kernel / sample_guide_mask_kernel / sample_guide_advance_kernel) ----
# tok_bytes uint8 [V_global, GUIDE_TOK_BYTES] / tok_len uint8 [V_global]: the pieces' UTF-8 bytes (length 0 = never
# allowed under a guide); guide_tab int16 (uint16 bits) [pool, GUIDE_STATES, 256], GUIDE_DEAD = dead; guide_flags int32
# [pool, GUIDE_STATES]: bit 0 accepting, bit 1 stuck; guide_meta int32 [2 slots] = pool index (-1 = off) | state.
GUIDE_STATES, GUIDE_POOL, GUIDE_TOK_BYTES, GUIDE_DEAD = 512, 32, 32, 0xFFFF
# The wide class (schema guides): guide_tab_wide int16 [pool <= GUIDE_WIDE_POOL, GUIDE_WIDE_STATES, 256] and
# guide_flags_wide int32 [pool, GUIDE_WIDE_STATES]; a guide_meta entry word in [GUIDE_POOL, GUIDE_POOL + pool) uses
# wide entry word - GUIDE_POOL, and its state is valid below GUIDE_WIDE_STATES.
GUIDE_WIDE_STATES, GUIDE_WIDE_POOL = 4096, 4


def guide_token_table(pieces, never=()):
    """(tok_bytes, tok_len) of a vocabulary: the UTF-8 bytes of piece(id).  Length 0 for the ids in `never`, the
    special pieces <unk> <s> </s>, and any piece that is empty or longer than GUIDE_TOK_BYTES bytes."""
    V = len(pieces)
    tb = np.zeros((V, GUIDE_TOK_BYTES), dtype=np.uint8)
    tl = np.zeros(V, dtype=np.uint8)
    for i, pc in enumerate(pieces):
        raw = pc.encode("utf-8") if isinstance(pc, str) else bytes(pc)
        if i in never or raw in (b"<unk>", b"<s>", b"</s>") or not 1 <= len(raw) <= GUIDE_TOK_BYTES:
            continue
        tb[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        tl[i] = len(raw)
    return torch.from_numpy(tb), torch.from_numpy(tl)


def _guide_np(t):
    return t.detach().cpu().contiguous().numpy()


def _guide_walk_all(tab, state: int, tok_bytes, tok_len, bound: int = GUIDE_STATES):
    """The state every token reaches from `state` (GUIDE_DEAD: none), vectorised over the vocabulary.  tab: uint16
    [bound, 256], bound = the states of the table's class."""
    st = np.full(tok_len.shape[0], state, dtype=np.int64)
    st[(tok_len < 1) | (tok_len > GUIDE_TOK_BYTES)] = GUIDE_DEAD
    if not 0 <= state < bound:
        st[:] = GUIDE_DEAD
    for j in range(GUIDE_TOK_BYTES):
        on = (tok_len > j) & (st != GUIDE_DEAD)
        if not on.any():
            break
        nxt = tab[st[on], tok_bytes[on, j]].astype(np.int64)
        nxt[nxt >= bound] = GUIDE_DEAD
        st[on] = nxt
    return st


def guide_walk(table, state: int, ids, tok_bytes, tok_len, eos: int = -1, bound: int = GUIDE_STATES) -> int:
    """Host walk: the DFA state after the tokens `ids` from `state` (EOS leaves it unchanged; a dead walk, an id
    outside the vocabulary or a token of length 0 makes it GUIDE_DEAD).  table: uint16 [n_states, 256]; bound = the
    states of its class (GUIDE_WIDE_STATES for a schema guide)."""
    table, tb, tl = np.asarray(table), _guide_np(tok_bytes), _guide_np(tok_len)
    for t in ids:
        t = int(t)
        if t == eos:
            continue
        if not (0 <= state < table.shape[0] and 0 <= t < tl.shape[0] and 1 <= tl[t] <= GUIDE_TOK_BYTES):
            return GUIDE_DEAD
        for byte in tb[t, :tl[t]]:
            state = int(table[state, byte])
            if state >= min(bound, table.shape[0]):
                return GUIDE_DEAD
    return state


def _guide_tab_np(guide_tab, entry: int):
    return _guide_np(guide_tab[entry]).view(np.uint16)


def _guide_class(guide_tab, guide_flags, entry: int, tab_wide, flags_wide):
    """(table pool, flags pool, index, state bound) of an entry word; None = outside both pools (guide off)."""
    if 0 <= entry < guide_tab.shape[0]:
        return guide_tab, guide_flags, entry, GUIDE_STATES
    if tab_wide is not None and 0 <= entry - GUIDE_POOL < tab_wide.shape[0]:
        return tab_wide, flags_wide, entry - GUIDE_POOL, GUIDE_WIDE_STATES
    return None


def guide_live(tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, entry: int, n_states: int, eos: int = -1,
               tab_wide=None, flags_wide=None):
    """Bit 1 of the flag of state s < n_states of the entry word `entry` (a narrow entry, or GUIDE_POOL + a wide
    one): no token of the vocabulary other than EOS survives from s."""
    guide_tab, guide_flags, entry, bound = _guide_class(guide_tab, guide_flags, entry, tab_wide, flags_wide)
    tab, tb, tl = _guide_tab_np(guide_tab, entry), _guide_np(tok_bytes), _guide_np(tok_len)
    for s in range(n_states):
        alive = _guide_walk_all(tab, s, tb, tl, bound) != GUIDE_DEAD
        if 0 <= eos < alive.shape[0]:
            alive[eos] = False
        guide_flags[entry, s] = (int(guide_flags[entry, s]) & 1) | (0 if alive.any() else 2)


def guide_mask(logits, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, row_slot=None, vocab_offset=0,
               eos: int = -1, json_tab=None, json_state=None, tab_wide=None, flags_wide=None):
    """In place on logits [B, V] (row b = slot row_slot[b], else b).  Inactive rows, slots with the guide off and
    slots in the dead state are not touched.  Otherwise column v (global id g = v + vocab_offset) becomes -inf unless
    g is allowed: EOS iff the state is accepting or stuck, another token iff its bytes walk from the state without
    meeting dead; at a stuck state EOS becomes 0.0.  Allowed columns keep their bits.  A JSON-mode slot (entry
    JSON_ENTRY; json_state given) walks the pushdown automaton from its (state, depth, stack) instead; EOS is 0.0 iff
    no other token of the global vocabulary survives (always so at JSON_DONE), else -inf.  A slot whose entry word is
    GUIDE_POOL + e uses wide entry e (tab_wide / flags_wide given) with states below GUIDE_WIDE_STATES."""
    B, V = logits.shape
    slots = guide_meta.numel() // 2
    tb, tl = _guide_np(tok_bytes), _guide_np(tok_len)
    Vg = tl.shape[0]
    for b in range(B):
        if active is not None and not int(active[b]):
            continue
        slot = int(row_slot[b]) if row_slot is not None else b
        entry, state = int(guide_meta[slot]), int(guide_meta[slots + slot])
        if entry == JSON_ENTRY and json_state is not None:
            js = _json_state_of(json_state, slot)
            if 0 <= js[0] < json_table()[0].shape[0] and 0 <= js[1] <= JSON_DEPTH:
                _json_mask_row(logits[b], js, tb, tl, vocab_offset, eos)
            continue
        cls = _guide_class(guide_tab, guide_flags, entry, tab_wide, flags_wide)
        if cls is None or not 0 <= state < cls[3]:
            continue
        tabs, flgs, entry, bound = cls
        flags = int(flgs[entry, state])
        ok = np.zeros(V, dtype=bool)
        n = max(0, min(V, Vg - vocab_offset))
        ok[:n] = _guide_walk_all(_guide_tab_np(tabs, entry), state, tb[vocab_offset:vocab_offset + n],
                                 tl[vocab_offset:vocab_offset + n], bound) != GUIDE_DEAD
        e = eos - vocab_offset
        if 0 <= e < n:
            ok[e] = bool(flags & 3)
        logits[b, torch.from_numpy(~ok)] = float("-inf")
        if 0 <= e < n and flags & 2:
            logits[b, e] = 0.0


def guide_advance(ids, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, row_slot=None, eos: int = -1,
                  json_tab=None, json_state=None, tab_wide=None, flags_wide=None):
    """guide_meta's state of row b's slot = walk(state, bytes(ids[b])); EOS leaves it, a dead walk or a token of
    length 0 makes it GUIDE_DEAD.  Inactive rows and slots with the guide off are skipped.  A JSON-mode slot moves
    its json_state words instead (a dead walk writes the state word only)."""
    slots = guide_meta.numel() // 2
    for b in range(ids.numel()):
        if active is not None and not int(active[b]):
            continue
        slot = int(row_slot[b]) if row_slot is not None else b
        entry = int(guide_meta[slot])
        if entry == JSON_ENTRY and json_state is not None and int(ids[b]) != eos:
            js = json_walk_ids(_json_state_of(json_state, slot), [int(ids[b])], tok_bytes, tok_len, eos)
            if js[0] == GUIDE_DEAD:
                json_state.view(4, -1)[0, slot] = GUIDE_DEAD
            else:
                json_state.view(4, -1)[:, slot] = torch.tensor(json_state_words(js), dtype=torch.int32)
            continue
        cls = _guide_class(guide_tab, guide_flags, entry, tab_wide, flags_wide)
        if cls is None or int(ids[b]) == eos:
            continue
        guide_meta[slots + slot] = guide_walk(_guide_tab_np(cls[0], cls[2]), int(guide_meta[slots + slot]),
                                              [int(ids[b])], tok_bytes, tok_len, eos, cls[3])


# ---- JSON mode (response_format json_object): the pushdown walk of the language J (docs/kernels.md, "Sampler") ----
# A slot whose guide_meta entry word is JSON_ENTRY uses no pool entry; json_state int32 [4, slots] = [lexical state |
# depth 0..JSON_DEPTH | stack bits 0..31 | stack bits 32..63] (state GUIDE_DEAD = dead; one stack bit per open
# container, 0 = object, 1 = array, innermost at bit 0).  json_table() uint16 [n, 256]: entry = next state | action <<
# 14, GUIDE_DEAD = no transition; action 1 / 2 pushes an object / array, 3 pops and the next state is what the pop
# uncovers (JSON_DONE at depth 0, else JSON_AFTER_OBJ / JSON_AFTER_ARR).  The device walks the same table (api.h).
JSON_ENTRY, JSON_DEPTH = -2, 64
JSON_START, JSON_DONE, JSON_AFTER_OBJ, JSON_AFTER_ARR = 0, 1, 2, 3
JSON_START_STATE, JSON_DEAD_STATE = (JSON_START, 0, 0), (GUIDE_DEAD, 0, 0)
_JSON_PUSH_OBJ, _JSON_PUSH_ARR, _JSON_POP = 1 << 14, 2 << 14, 3 << 14
_JSON_TABLE = None


def json_table():
    """The automaton, uint16 [n, 256], and (second value) the state numbers by name.  Lexical states are split by
    context ("o": the innermost container is an object, "a": an array, "k": an object key), so a closing byte always
    matches the stack's top bit and the byte after a number can be processed as the delimiter it is."""
    global _JSON_TABLE
    if _JSON_TABLE is not None:
        return _JSON_TABLE
    names = ["start", "done", "after_o", "after_a", "obj_open", "obj_key", "colon", "val_o", "arr_open", "val_a"]
    for c in "oa":
        names += [f"{n}_{c}" for n in ("minus", "zero", "int", "dot", "frac", "exp", "expsign", "expd",
                                       "t", "tr", "tru", "f", "fa", "fal", "fals", "n", "nu", "nul")]
    for c in "koa":
        names += [f"{n}_{c}" for n in ("str", "esc", "u1", "u2", "u3", "u4", "t1", "t2", "t2e0", "t2ed", "t3", "t3f0",
                                       "t3f4")]
    S = {n: i for i, n in enumerate(names)}
    assert (S["start"], S["done"], S["after_o"], S["after_a"]) == (JSON_START, JSON_DONE, JSON_AFTER_OBJ,
                                                                   JSON_AFTER_ARR)
    tab = np.full((len(names), 256), GUIDE_DEAD, dtype=np.uint16)

    def put(state, chars, to):
        for ch in chars:
            tab[S[state], ch if isinstance(ch, int) else ord(ch)] = to if isinstance(to, int) else S[to]

    ws, digits = " \t\n\r", "0123456789"
    put("start", "{", S["obj_open"] | _JSON_PUSH_OBJ)
    for st in ("after_o", "after_a", "obj_open", "obj_key", "colon", "val_o", "arr_open", "val_a"):
        put(st, ws, st)
    put("after_o", ",", "obj_key")
    put("after_o", "}", _JSON_POP)
    put("after_a", ",", "val_a")
    put("after_a", "]", _JSON_POP)
    put("obj_open", '"', "str_k")
    put("obj_open", "}", _JSON_POP)
    put("obj_key", '"', "str_k")
    put("colon", ":", "val_o")
    put("arr_open", "]", _JSON_POP)
    for st, c in (("val_o", "o"), ("val_a", "a"), ("arr_open", "a")):  # a value starts
        put(st, '"', f"str_{c}")
        put(st, "{", S["obj_open"] | _JSON_PUSH_OBJ)
        put(st, "[", S["arr_open"] | _JSON_PUSH_ARR)
        put(st, "-", f"minus_{c}")
        put(st, "0", f"zero_{c}")
        put(st, "123456789", f"int_{c}")
        for ch in "tfn":
            put(st, ch, f"{ch}_{c}")
    for c in "oa":
        after = f"after_{c}"
        put(f"minus_{c}", "0", f"zero_{c}")
        put(f"minus_{c}", "123456789", f"int_{c}")
        put(f"int_{c}", digits, f"int_{c}")
        for st in (f"zero_{c}", f"int_{c}"):
            put(st, ".", f"dot_{c}")
            put(st, "eE", f"exp_{c}")
        put(f"dot_{c}", digits, f"frac_{c}")
        put(f"frac_{c}", digits, f"frac_{c}")
        put(f"frac_{c}", "eE", f"exp_{c}")
        put(f"exp_{c}", "+-", f"expsign_{c}")
        put(f"exp_{c}", digits, f"expd_{c}")
        put(f"expsign_{c}", digits, f"expd_{c}")
        put(f"expd_{c}", digits, f"expd_{c}")
        for st in (f"zero_{c}", f"int_{c}", f"frac_{c}", f"expd_{c}"):  # one byte of lookahead: the delimiter
            for ch in ws + ",}]":
                tab[S[st], ord(ch)] = tab[S[after], ord(ch)]
        for word in ("true", "false", "null"):
            for i in range(1, len(word)):
                put(f"{word[:i]}_{c}", word[i], f"{word[:i + 1]}_{c}" if i + 1 < len(word) else after)
    for c, closed in (("k", "colon"), ("o", "after_o"), ("a", "after_a")):
        s = lambda n: f"{n}_{c}"  # noqa: E731
        put(s("str"), range(0x20, 0x80), s("str"))
        put(s("str"), '"', closed)
        put(s("str"), "\\", s("esc"))
        put(s("str"), range(0xC2, 0xE0), s("t1"))
        put(s("str"), range(0xE0, 0xF0), s("t2"))
        put(s("str"), [0xE0], s("t2e0"))  # no overlong three-byte forms
        put(s("str"), [0xED], s("t2ed"))  # no encoded surrogates
        put(s("str"), range(0xF1, 0xF4), s("t3"))
        put(s("str"), [0xF0], s("t3f0"))  # no overlong four-byte forms
        put(s("str"), [0xF4], s("t3f4"))  # nothing above U+10FFFF
        put(s("esc"), '"\\/bfnrt', s("str"))
        put(s("esc"), "u", s("u1"))
        for a, b in (("u1", "u2"), ("u2", "u3"), ("u3", "u4"), ("u4", "str")):
            put(s(a), digits + "abcdefABCDEF", s(b))
        put(s("t1"), range(0x80, 0xC0), s("str"))
        put(s("t2"), range(0x80, 0xC0), s("t1"))
        put(s("t2e0"), range(0xA0, 0xC0), s("t1"))
        put(s("t2ed"), range(0x80, 0xA0), s("t1"))
        put(s("t3"), range(0x80, 0xC0), s("t2"))
        put(s("t3f0"), range(0x90, 0xC0), s("t2"))
        put(s("t3f4"), range(0x80, 0x90), s("t2"))
    _JSON_TABLE = (tab, S)
    return _JSON_TABLE


def json_walk(data, state=JSON_START_STATE):
    """The byte walker: the (state, depth, stack) after the bytes `data` from `state`; JSON_DEAD_STATE where the walk
    dies (no transition, or a push at depth JSON_DEPTH).  The text so far is in J iff the state is JSON_DONE."""
    tab = json_table()[0]
    q, depth, stack = state
    if not (0 <= q < tab.shape[0] and 0 <= depth <= JSON_DEPTH):
        return JSON_DEAD_STATE
    for byte in bytes(data):
        e = int(tab[q, byte])
        if e == GUIDE_DEAD:
            return JSON_DEAD_STATE
        act, q = e >> 14, e & 0x3FFF
        if act == 3:
            if depth < 1:
                return JSON_DEAD_STATE
            depth, stack = depth - 1, stack >> 1
            q = JSON_DONE if depth == 0 else (JSON_AFTER_ARR if stack & 1 else JSON_AFTER_OBJ)
        elif act:
            if depth >= JSON_DEPTH:
                return JSON_DEAD_STATE
            depth, stack = depth + 1, ((stack << 1) | (act == 2)) & ((1 << 64) - 1)
    return (q, depth, stack)


def json_walk_all(state, tok_bytes, tok_len):
    """json_walk of every token from `state`, vectorised over the vocabulary: (q, depth, stack) arrays, q = GUIDE_DEAD
    where the token dies (length 0 or above GUIDE_TOK_BYTES included).  tok_bytes / tok_len: numpy uint8."""
    tab = json_table()[0]
    n = tok_len.shape[0]
    q0, d0, s0 = state
    q = np.full(n, q0, dtype=np.int64)
    depth = np.full(n, d0, dtype=np.int64)
    stack = np.full(n, s0, dtype=np.uint64)
    q[(tok_len < 1) | (tok_len > GUIDE_TOK_BYTES)] = GUIDE_DEAD
    if not (0 <= q0 < tab.shape[0] and 0 <= d0 <= JSON_DEPTH):
        q[:] = GUIDE_DEAD
    one = np.uint64(1)
    for j in range(GUIDE_TOK_BYTES):
        on = np.nonzero((tok_len > j) & (q != GUIDE_DEAD))[0]
        if on.size == 0:
            break
        e = tab[q[on], tok_bytes[on, j]].astype(np.int64)
        act, nq, d, s = e >> 14, e & 0x3FFF, depth[on], stack[on]
        dead = e == GUIDE_DEAD
        pop, push = (act == 3) & ~dead, ((act == 1) | (act == 2)) & ~dead
        dead |= (pop & (d < 1)) | (push & (d >= JSON_DEPTH))
        d = d - pop + push
        s = np.where(pop, s >> one, np.where(push, (s << one) | (act == 2).astype(np.uint64), s))
        nq = np.where(pop, np.where(d == 0, JSON_DONE, np.where((s & one) == one, JSON_AFTER_ARR, JSON_AFTER_OBJ)), nq)
        nq[dead] = GUIDE_DEAD
        q[on], depth[on], stack[on] = nq, d, s
    return q, depth, stack


def json_walk_ids(state, ids, tok_bytes, tok_len, eos: int = -1):
    """Host walk over token ids: the (state, depth, stack) after the tokens `ids` from `state` (EOS leaves it unchanged;
    a dead walk, an id outside the vocabulary or a token of length 0 makes it JSON_DEAD_STATE)."""
    tb, tl = _guide_np(tok_bytes), _guide_np(tok_len)
    for t in ids:
        t = int(t)
        if t == eos:
            continue
        if state[0] == GUIDE_DEAD or not (0 <= t < tl.shape[0] and 1 <= tl[t] <= GUIDE_TOK_BYTES):
            return JSON_DEAD_STATE
        state = json_walk(tb[t, :tl[t]].tobytes(), state)
    return state if state[0] != GUIDE_DEAD else JSON_DEAD_STATE


def json_state_words(state) -> list:
    """(state, depth, stack) as json_state's four int32 words."""
    q, depth, stack = state
    w = [q, depth, stack & 0xFFFFFFFF, (stack >> 32) & 0xFFFFFFFF]
    return [x - (1 << 32) if x >= (1 << 31) else x for x in w]


def _json_state_of(json_state, slot: int):
    w = [int(x) & 0xFFFFFFFF for x in json_state.view(4, -1)[:, slot].tolist()]
    q = w[0] if w[0] < (1 << 31) else w[0] - (1 << 32)
    d = w[1] if w[1] < (1 << 31) else w[1] - (1 << 32)
    return (q, d, w[2] | (w[3] << 32))


def _json_mask_row(row, state, tb, tl, vocab_offset: int, eos: int) -> None:
    """One JSON-mode row of guide_mask (row: the float32 logits of this shard's V columns, in place)."""
    V, Vg = row.shape[0], tl.shape[0]
    alive = json_walk_all(state, tb, tl)[0] != GUIDE_DEAD  # over the GLOBAL vocabulary: the stuck decision needs it
    if 0 <= eos < Vg:
        alive[eos] = False
    stuck = not alive.any()
    ok = np.zeros(V, dtype=bool)
    n = max(0, min(V, Vg - vocab_offset))
    ok[:n] = alive[vocab_offset:vocab_offset + n]
    row[torch.from_numpy(~ok)] = float("-inf")
    e = eos - vocab_offset
    if 0 <= eos < Vg and 0 <= e < n and stuck:
        row[e] = 0.0


def _hist_append(pen_meta, hist, slot: int, tok: int) -> None:
    if not penalties_on(pen_meta, slot):
        return
    n = int(hist[slot, 0])
    if 0 <= n < hist.shape[1] - 1:
        hist[slot, 1 + n] = tok
        hist[slot, 0] = n + 1


def sample_hist_append(new_ids, row_slot, active, pen_meta, hist):
    """hist[slot] += new_ids[i] for the active rows whose slot (row_slot[i], else i) has penalties on."""
    for i in range(new_ids.numel()):
        if active is not None and not int(active[i]):
            continue
        _hist_append(pen_meta, hist, int(row_slot[i]) if row_slot is not None else i, int(new_ids[i]))


def sample_pick_hist(cand_all, active, next_ids, ring, ring_counter, positions_inc, pen_meta, hist,
                     vocab: int = 2**31 - 1):
    """sample_pick, then the picked token of every active penalised row (row b = slot b) joins its history."""
    sample_pick(cand_all, active, next_ids, ring, ring_counter, positions_inc, vocab)
    sample_hist_append(next_ids[:cand_all.shape[1]], None, active, pen_meta, hist)


def prefill_sample_commit_hist(meta, new_ids, ids, ring, positions, pen_meta, hist):
    """prefill_sample_commit, then the first token of every finishing prompt whose slot has penalties on joins its
    history."""
    prefill_sample_commit(meta, new_ids, ids, ring, positions)
    NS = new_ids.numel()
    for i in range(min(int(meta[3 * NS]), NS)):
        _hist_append(pen_meta, hist, int(meta[NS + i]), int(new_ids[i]))


# ---- logprobs / top_logprobs (sampler.hip logprob_stats_kernel / logprob_chosen_kernel / logprob_finish_kernel) ----
# Raw logprobs: x[v] - logsumexp(x) over the full vocabulary of the fp32 logits as the LM head wrote them.  lp_meta
# int32 [slots]: -1 = off, 0..LP_TOP = N.  Order of the top-N: logit descending, equal logits by ascending global id.
LP_TOP = 20
LP_REC = 2 + 2 * LP_TOP
LP_OUT = 1 + 2 * LP_TOP
_LP_NONE = 0x7FFFFFFF
_NEG_INF = float("-inf")


def _lp_row(active, lp_meta, row_slot, b: int):
    """(N, slot) of row b; N < 0: the row is inactive or off."""
    if active is not None and not int(active[b]):
        return -1, -1
    slot = int(row_slot[b]) if row_slot is not None else b
    return min(int(lp_meta[slot]), LP_TOP), slot


def logprob_stats(logits, active, lp_meta, row_slot, rec, raw=None, vocab_offset=0):
    B, V = logits.shape
    rec_i = rec.view(torch.int32)
    for b in range(B):
        N, _ = _lp_row(active, lp_meta, row_slot, b)
        if N < 0:
            continue
        x = logits[b].to(torch.float32)
        if raw is not None:
            raw[b].copy_(x)
        m = x.max()
        rec[b, 0] = m
        rec[b, 1] = torch.exp(x - m).sum() if float(m) > _NEG_INF else 0.0
        rec[b, 2::2] = _NEG_INF
        rec_i[b, 3::2] = _LP_NONE
        n = min(N, V)
        if n > 0:
            vals, idx = torch.sort(x + 0.0, descending=True, stable=True)  # stable: equal logits by ascending id
            rec[b, 2:2 + 2 * n:2] = vals[:n]
            rec_i[b, 3:3 + 2 * n:2] = (idx[:n] + vocab_offset).to(torch.int32)


def logprob_chosen(logits, next_ids, active, lp_meta, row_slot, chosen, vocab_offset=0, vocab: int = 2**31 - 1):
    B, V = logits.shape
    for b in range(B):
        N, _ = _lp_row(active, lp_meta, row_slot, b)
        if N < 0:
            continue
        v = int(next_ids[b]) - vocab_offset
        chosen[b] = logits[b, v] if 0 <= v < V else _NEG_INF


def logprob_finish(rec_all, chosen_all, active, lp_meta, row_slot, lp_ring, ring_counter=None, ring_row_dev=None,
                   ring_row: int = -1, vocab: int = 2**31 - 1):
    world, B = rec_all.shape[0], rec_all.shape[1]
    R = lp_ring.shape[0]
    if ring_counter is not None:
        row = int(ring_counter[0]) % R
    elif ring_row_dev is not None:
        row = int(ring_row_dev[0])
    else:
        row = int(ring_row)
    rec_i = rec_all.view(torch.int32)
    ring_i = lp_ring.view(torch.int32)
    f32 = torch.float32
    for b in range(B):
        N, slot = _lp_row(active, lp_meta, row_slot, b)
        if N < 0:
            continue
        m = rec_all[:, b, 0]
        M = m.max()
        s = torch.zeros((), dtype=f32)
        for w in range(world):  # an empty / all -inf shard (s = 0, m = -inf) adds nothing: no inf - inf
            if float(m[w]) > _NEG_INF and float(rec_all[w, b, 1]) > 0.0:
                s = s + rec_all[w, b, 1] * torch.exp(m[w] - M)
        lse = M + torch.log(s) if float(s) > 0.0 else torch.tensor(_NEG_INF)
        c = chosen_all[:, b].max()
        lp_ring[row, slot, 0] = c - lse if float(c) > _NEG_INF else _NEG_INF
        cand = sorted(((-float(rec_all[w, b, 2 + 2 * j]), int(rec_i[w, b, 3 + 2 * j]), w * LP_TOP + j)
                       for w in range(world) for j in range(LP_TOP)))
        for rank in range(LP_TOP):
            neg, tid, k = cand[rank]
            used = rank < N and tid != _LP_NONE
            ring_i[row, slot, 1 + rank] = tid if used else -1
            val = rec_all[k // LP_TOP, b, 2 + 2 * (k % LP_TOP)]
            lp_ring[row, slot, 1 + LP_TOP + rank] = val - lse if used and float(val) > _NEG_INF else _NEG_INF


# ---------------------------------------------------------------- multi-LoRA (csrc/kernels/lora.hip)
def lora_shrink(x, A, row_adapter, t):
    """t[i] = A[row_adapter[i]] · x[i] in fp32 (A [slots, S·R, K]); rows with adapter -1 get zeros."""
    M = x.shape[0]
    ra = row_adapter[:M].long()
    t.zero_()
    for a in sorted(set(ra.tolist()) - {-1}):
        rows = (ra == a).nonzero().flatten()
        t[rows] = x[rows].float() @ A[a].float().t()


def lora_expand_add(t, B, scale, row_adapter, slice_of_row, out):
    """out[i, n] += scale[a] · Σ_j B[a][n, j] · t[i, slice_of_row[n]·R + j], a = row_adapter[i]; rows with adapter -1
    keep their bits.  The scale multiplies the fp32 sum; the result is rounded once to out's dtype."""
    M, R = out.shape[0], B.shape[2]
    ra = row_adapter[:M].long()
    cols = slice_of_row.long()[:, None] * R + torch.arange(R)[None, :]  # [N, R]: the columns of t row n reads
    for a in sorted(set(ra.tolist()) - {-1}):
        rows = (ra == a).nonzero().flatten()
        d = (t[rows].float()[:, cols] * B[a].float()[None]).sum(-1) * float(scale[a])
        out[rows] = (out[rows].float() + d).to(out.dtype)
