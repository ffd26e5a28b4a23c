"""Engine ops: gfx950 HIP kernels on GPU tensors, fp32 PyTorch references on CPU tensors.

The HIP library (``_lib/libdsse_kernels.so``, built by ``_build.build_kernels``) registers the
operators under ``torch.ops.dsse``.  Dispatch is by tensor device only:

* GPU tensor  -> the HIP kernel, always.  If the library is missing or failed to load, the call
  raises: there is no eager-PyTorch fallback on the GPU path.
* CPU tensor  -> the reference implementation in ``ops/reference.py`` (plumbing tests in the
  GPU-less build container).
"""
from __future__ import annotations

import os
from pathlib import Path

import torch

from . import reference as ref

_VARIANT = os.environ.get("DSSE_KERNELS_VARIANT", "")  # "checked" (device index checks) or "nt", see _build.py
_LIB = Path(__file__).resolve().parent.parent / "_lib" / (
    f"libdsse_kernels_{_VARIANT}.so" if _VARIANT else "libdsse_kernels.so")
_loaded = False
_load_error: str | None = None


def load_library(required: bool = False) -> bool:
    """Load the HIP kernel library once.  Returns True when torch.ops.dsse is available."""
    global _loaded, _load_error
    if _loaded:
        return True
    if not _LIB.exists() and os.environ.get("DSSE_AUTOBUILD", "1") == "1":
        try:
            from .._build import build_kernels

            build_kernels(variant=_VARIANT or None)
        except Exception as e:  # noqa: BLE001 - reported below
            _load_error = f"build failed: {e}"
    if _LIB.exists():
        try:
            torch.ops.load_library(str(_LIB))
            _loaded = True
        except Exception as e:  # noqa: BLE001
            _load_error = f"load failed: {e}"
    elif _load_error is None:
        _load_error = f"{_LIB} not built"
    if required and not _loaded:
        raise RuntimeError(f"dsse HIP kernels unavailable ({_load_error}); run `python -m "
                           "distributed_sse_for_llm_response_amd._build kernels`")
    return _loaded


def library_path() -> Path:
    return _LIB


def _hip(t: torch.Tensor) -> bool:
    if t.is_cuda:
        load_library(required=True)
        return True
    return False


def gemm_out(x, w, out):
    """out[M, N] = x[M, K] · w[N, K]ᵀ (bf16 or fp32 out)."""
    if _hip(x):
        torch.ops.dsse.gemm_out(x, w, out)
    else:
        ref.gemm_out(x, w, out)


def gemm_resid(x, w, resid):
    """resid[M, N] (fp32) += x · wᵀ."""
    if _hip(x):
        torch.ops.dsse.gemm_resid(x, w, resid)
    else:
        ref.gemm_resid(x, w, resid)


def gemm_silu(x, w, out):
    """out[M, N/2] = silu(gate) * up with the interleaved gate/up weight rows."""
    if _hip(x):
        torch.ops.dsse.gemm_silu(x, w, out)
    else:
        ref.gemm_silu(x, w, out)


def gemm_qkv_rope(x, w, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0, v_scale=1.0,
                  scratch=None):
    """Fused QKV projection + RoPE + paged KV write (decode).  The cache tensors' dtype selects the kernels: bf16, or
    float8_e4m3fn with the layer's k_scale / v_scale (stored = x / scale; ops/reference.py quantize_kv).  scratch
    (fp8 on the GPU only): an fp32 buffer of at least M x N floats for the projection's sums, else one is allocated."""
    if _hip(x):
        torch.ops.dsse.gemm_qkv_rope(x, w, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale,
                                     scratch)
    else:
        ref.gemm_qkv_rope(x, w, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale)


def gemm_resid_split(x, w, resid, part) -> int:
    """resid += x · wᵀ, or (when the X-in-LDS kernel splits K) write fp32 slabs [S, M, N] into `part`
    and return S so the following rmsnorm(part=..., nsplit=S) folds the reduction into the norm."""
    if _hip(x):
        return int(torch.ops.dsse.gemm_resid_split(x, w, resid, part))
    ref.gemm_resid(x, w, resid)
    return 0


def gemm_out_split(x, w, out, part) -> int:
    """out = x · wᵀ (bf16), or (when the chosen kernel splits K) fp32 slabs [S, M, N] into `part` and return S for a
    consumer that sums them (the TP decode step's IPC all-reduce, comm.all_reduce_rmsnorm(part=..., nsplit=S))."""
    if _hip(x):
        return int(torch.ops.dsse.gemm_out_split(x, w, out, part))
    ref.gemm_out(x, w, out)
    return 0


# ---- FP8 weights (W8A16; csrc/kernels/gemm_w8.hip): w_q = e4m3 bytes in the byte tiled layout (reference.py
# tile_weight_f8), w_scale = fp32 power-of-two row scales.  1-64 rows on the GPU; each op mirrors the bf16 op of the
# same name and equals it on the widened weight tile_weight(widen_weight_f8(...)) up to fp32 summation order.
W8_MAX_M = 64
quantize_weight_f8, widen_weight_f8 = ref.quantize_weight_f8, ref.widen_weight_f8
tile_weight_f8, untile_weight_f8 = ref.tile_weight_f8, ref.untile_weight_f8


def gemm_out_w8(x, w_q, w_scale, out):
    """out[M, N] = (x · w_qᵀ) * w_scale (bf16 or fp32 out)."""
    if _hip(x):
        torch.ops.dsse.gemm_out_w8(x, w_q, w_scale, out)
    else:
        ref.gemm_out_w8(x, w_q, w_scale, out)


def gemm_resid_w8(x, w_q, w_scale, resid):
    """resid[M, N] (fp32) += (x · w_qᵀ) * w_scale."""
    if _hip(x):
        torch.ops.dsse.gemm_resid_w8(x, w_q, w_scale, resid)
    else:
        ref.gemm_resid_w8(x, w_q, w_scale, resid)


def gemm_silu_w8(x, w_q, w_scale, out):
    """gemm_silu over an FP8 weight (interleaved gate/up rows)."""
    if _hip(x):
        torch.ops.dsse.gemm_silu_w8(x, w_q, w_scale, out)
    else:
        ref.gemm_silu_w8(x, w_q, w_scale, out)


def gemm_resid_split_w8(x, w_q, w_scale, resid, part) -> int:
    """gemm_resid_split over an FP8 weight: scaled fp32 slabs [S, M, N] in `part` and S, or the sum in resid and 0."""
    if _hip(x):
        return int(torch.ops.dsse.gemm_resid_split_w8(x, w_q, w_scale, resid, part))
    ref.gemm_resid_w8(x, w_q, w_scale, resid)
    return 0


def gemm_out_split_w8(x, w_q, w_scale, out, part) -> int:
    """gemm_out_split over an FP8 weight."""
    if _hip(x):
        return int(torch.ops.dsse.gemm_out_split_w8(x, w_q, w_scale, out, part))
    ref.gemm_out_w8(x, w_q, w_scale, out)
    return 0


def gemm_qkv_rope_w8(x, w_q, w_scale, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0,
                     v_scale=1.0, scratch=None):
    """gemm_qkv_rope over an FP8 weight (the unfused path of qkv_attention_decode_w8)."""
    if _hip(x):
        torch.ops.dsse.gemm_qkv_rope_w8(x, w_q, w_scale, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv,
                                        k_scale, v_scale, scratch)
    else:
        ref.gemm_qkv_rope_w8(x, w_q, w_scale, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale,
                             v_scale)


def qkv_attention_decode_w8(x, w_q, w_scale, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, slabs,
                            block_tables, q_start, q_len, ctx_len, work_seq, work_tile, out, part_o, part_ml, part,
                            nparts, k_scale=1.0, v_scale=1.0) -> int:
    """qkv_attention_decode over an FP8 weight: the projection leaves scaled fp32 slabs that the attention kernel
    folds in unchanged (returns the slab count; 0 = gemm_qkv_rope_w8 + paged_attention ran instead)."""
    if _hip(x):
        return int(torch.ops.dsse.qkv_attention_decode_w8(x, w_q, w_scale, positions, slots, rope, q_out, k_cache,
                                                          v_cache, nh, nkv, slabs, block_tables, q_start, q_len,
                                                          ctx_len, work_seq, work_tile, out, part_o, part_ml, part,
                                                          nparts, k_scale, v_scale))
    B = x.shape[0]
    ref.gemm_qkv_rope_w8(x, w_q, w_scale, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale)
    ref.paged_attention(0, q_out.view(B, nh, 128), k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work_seq,
                        work_tile, out.view(B, nh, 128), part_o, part_ml, part, nparts, k_scale, v_scale)
    return 0


# ---- MXFP4 weights (W4A16; csrc/kernels/gemm_w4.hip): w_q = e2m1 nibble bytes [N, K / 2], w_e = e8m0 block scale
# bytes [N, K / 32], both in the tiled layout (reference.py tile_weight_mxfp4).  1-64 rows on the GPU; each op mirrors
# the bf16 op of the same name and equals it on the widened weight tile_weight(widen_weight_mxfp4(...)) up to fp32
# summation order.
W4_MAX_M = 64
quantize_weight_mxfp4, widen_weight_mxfp4 = ref.quantize_weight_mxfp4, ref.widen_weight_mxfp4
tile_weight_mxfp4, untile_weight_mxfp4 = ref.tile_weight_mxfp4, ref.untile_weight_mxfp4


def gemm_out_w4(x, w_q, w_e, out):
    """out[M, N] = x · widen(w_q, w_e)ᵀ (bf16 or fp32 out)."""
    if _hip(x):
        torch.ops.dsse.gemm_out_w4(x, w_q, w_e, out)
    else:
        ref.gemm_out_w4(x, w_q, w_e, out)


def gemm_resid_w4(x, w_q, w_e, resid):
    """resid[M, N] (fp32) += x · widen(w_q, w_e)ᵀ."""
    if _hip(x):
        torch.ops.dsse.gemm_resid_w4(x, w_q, w_e, resid)
    else:
        ref.gemm_resid_w4(x, w_q, w_e, resid)


def gemm_silu_w4(x, w_q, w_e, out):
    """gemm_silu over an MXFP4 weight (interleaved gate/up rows)."""
    if _hip(x):
        torch.ops.dsse.gemm_silu_w4(x, w_q, w_e, out)
    else:
        ref.gemm_silu_w4(x, w_q, w_e, out)


def gemm_resid_split_w4(x, w_q, w_e, resid, part) -> int:
    """gemm_resid_split over an MXFP4 weight: fp32 slabs [S, M, N] in `part` and S, or the sum in resid and 0."""
    if _hip(x):
        return int(torch.ops.dsse.gemm_resid_split_w4(x, w_q, w_e, resid, part))
    ref.gemm_resid_w4(x, w_q, w_e, resid)
    return 0


def gemm_out_split_w4(x, w_q, w_e, out, part) -> int:
    """gemm_out_split over an MXFP4 weight."""
    if _hip(x):
        return int(torch.ops.dsse.gemm_out_split_w4(x, w_q, w_e, out, part))
    ref.gemm_out_w4(x, w_q, w_e, out)
    return 0


def gemm_qkv_rope_w4(x, w_q, w_e, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0,
                     v_scale=1.0, scratch=None):
    """gemm_qkv_rope over an MXFP4 weight (the unfused path of qkv_attention_decode_w4)."""
    if _hip(x):
        torch.ops.dsse.gemm_qkv_rope_w4(x, w_q, w_e, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv,
                                        k_scale, v_scale, scratch)
    else:
        ref.gemm_qkv_rope_w4(x, w_q, w_e, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale,
                             v_scale)


def qkv_attention_decode_w4(x, w_q, w_e, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, slabs,
                            block_tables, q_start, q_len, ctx_len, work_seq, work_tile, out, part_o, part_ml, part,
                            nparts, k_scale=1.0, v_scale=1.0) -> int:
    """qkv_attention_decode over an MXFP4 weight: the projection leaves fp32 slabs that the attention kernel
    folds in unchanged (returns the slab count; 0 = gemm_qkv_rope_w4 + paged_attention ran instead)."""
    if _hip(x):
        return int(torch.ops.dsse.qkv_attention_decode_w4(x, w_q, w_e, positions, slots, rope, q_out, k_cache,
                                                          v_cache, nh, nkv, slabs, block_tables, q_start, q_len,
                                                          ctx_len, work_seq, work_tile, out, part_o, part_ml, part,
                                                          nparts, k_scale, v_scale))
    B = x.shape[0]
    ref.gemm_qkv_rope_w4(x, w_q, w_e, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale)
    ref.paged_attention(0, q_out.view(B, nh, 128), k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work_seq,
                        work_tile, out.view(B, nh, 128), part_o, part_ml, part, nparts, k_scale, v_scale)
    return 0


# ---- multi-LoRA (csrc/kernels/lora.hip): every row names its adapter slot in row_adapter (int32, -1 = none)
LORA_RANKS = (8, 16, 32, 64)  # pool ranks the expand kernel is built for
LORA_MAX_SLOTS = 8


def lora_shrink(x, A, row_adapter, t):
    """t[M, S·R] (fp32) = A[row_adapter[i]] · x[i]: x [M, K] bf16, A [slots, S·R, K] bf16 (the stacked A matrices of a
    fused projection: one pass over x).  Rows with adapter -1 get zeros."""
    if _hip(x):
        torch.ops.dsse.lora_shrink(x, A, row_adapter, t)
    else:
        ref.lora_shrink(x, A, row_adapter, t)


def lora_expand_add(t, B, scale, row_adapter, slice_of_row, out):
    """out[i, n] += scale[a] · Σ_j B[a][n, j] · t[i, slice_of_row[n]·R + j] with a = row_adapter[i]: B [slots, N, R]
    bf16 in the engine's output-row order, scale [slots] fp32 (applied to the fp32 sum), out [M, N] fp32 or bf16.  Rows
    with adapter -1 keep their bits."""
    if _hip(out):
        torch.ops.dsse.lora_expand_add(t, B, scale, row_adapter, slice_of_row, out)
    else:
        ref.lora_expand_add(t, B, scale, row_adapter, slice_of_row, out)


def kernel_cfg_env(**overrides) -> str:
    """The DSSE_KERNEL_CFG string (the kernel library's one configuration override: "key=value,..."; keys in
    csrc/kernels/bindings.cpp env_int, e.g. gemm_impl, t_cfg, s_nw) with `overrides` merged into the current value.
    Set it in the environment, then call refresh_env()."""
    cur = {}
    for item in os.environ.get("DSSE_KERNEL_CFG", "").replace(";", ",").replace(" ", ",").split(","):
        if "=" in item:
            k, v = item.split("=", 1)
            cur[k.strip().lower()] = v.strip()
    for k, v in overrides.items():
        if v is None:
            cur.pop(k, None)
        else:
            cur[k] = str(v)
    return ",".join(f"{k}={v}" for k, v in cur.items())


def refresh_env() -> None:
    """Re-read the DSSE_* kernel tuning variables (cached by the library on first use)."""
    if load_library():
        torch.ops.dsse.refresh_env()


def rmsnorm(resid, w, y, eps, delta=None, embed=None, ids=None, part=None, nsplit=0):
    """resid (+= delta | sum of `nsplit` split-K slabs in `part` | = embed[ids]); y = rmsnorm(resid) * w."""
    if _hip(resid):
        torch.ops.dsse.rmsnorm(resid, w, y, eps, delta, embed, ids, part, nsplit)
    else:
        ref.rmsnorm(resid, w, y, eps, delta, embed, ids, part, nsplit)


def rope_kv_write(qkv, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale=1.0, v_scale=1.0):
    if _hip(qkv):
        torch.ops.dsse.rope_kv_write(qkv, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale)
    else:
        ref.rope_kv_write(qkv, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale)


def silu_mul(gu, h):
    if _hip(gu):
        torch.ops.dsse.silu_mul(gu, h)
    else:
        ref.silu_mul(gu, h)


def decode_prep(active, positions, block_tables, slots, ctx_len, q_len, num_blocks: int = 2**31 - 1):
    if _hip(active):
        torch.ops.dsse.decode_prep(active, positions, block_tables, slots, ctx_len, q_len, num_blocks)
    else:
        ref.decode_prep(active, positions, block_tables, slots, ctx_len, q_len)


def ring_advance(counter):
    if _hip(counter):
        torch.ops.dsse.ring_advance(counter)
    else:
        ref.ring_advance(counter)


def paged_attention(mode, q, k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work_seq, work_tile, out,
                    part_o, part_ml, part, nparts, k_scale=1.0, v_scale=1.0):
    """mode 0 = decode (flash-decoding partitions), 1 = prefill on 16-query tiles (decode-style kernel),
    2 = flash prefill on 64-query tiles (LDS-staged K/V, attention_prefill.hip).  A float8_e4m3fn cache (modes 0 and
    1; the flash kernel has no fp8 form and the HIP op refuses it) is read as stored * scale."""
    if _hip(q):
        torch.ops.dsse.paged_attention(mode, q, k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work_seq,
                                       work_tile, out, part_o, part_ml, part, nparts, k_scale, v_scale)
    else:
        ref.paged_attention(mode, q, k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work_seq, work_tile,
                            out, part_o, part_ml, part, nparts, k_scale, v_scale)


def flash_prefill_split(q, k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work, comb, out, part_o, part_ml,
                        nslots: int) -> None:
    """Flash prefill with long causal tiles split over key ranges (work = [seq | tile | (kb0, kb1) pairs | slot],
    comb = [(seq, tile, first slot, slots)]; ModelRunner._flash_split_plan): the parts leave partial O in slots that
    a combine kernel merges.  Same result as paged_attention mode 2 up to fp32 summation order."""
    if _hip(q):
        torch.ops.dsse.flash_prefill_split(q, k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work, comb, out,
                                           part_o, part_ml, nslots)
    else:  # the split is a schedule: the reference computes each tile whole (a split tile's items repeat it)
        if ref.is_fp8(k_cache):
            raise TypeError("flash_prefill_split has no float8_e4m3fn KV cache form: use paged_attention mode 1")
        nw = work.numel() // 5
        ref.paged_attention(2, q, k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work[:nw], work[nw:2 * nw],
                            out, part_o, part_ml, 32, 1)


def qkv_attention_decode(x, w, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, slabs, block_tables, q_start,
                         q_len, ctx_len, work_seq, work_tile, out, part_o, part_ml, part, nparts, k_scale=1.0,
                         v_scale=1.0) -> int:
    """Decode QKV projection + RoPE + KV write + attention.  HIP: the GEMM leaves fp32 split-K slabs in `slabs`
    and the attention kernel folds the reduction, RoPE and the K/V write in (returns the slab count; 0 = it ran
    gemm_qkv_rope + paged_attention instead).  Same result as those two ops."""
    if _hip(x):
        return int(torch.ops.dsse.qkv_attention_decode(x, w, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv,
                                                       slabs, block_tables, q_start, q_len, ctx_len, work_seq,
                                                       work_tile, out, part_o, part_ml, part, nparts, k_scale, v_scale))
    B = x.shape[0]
    ref.gemm_qkv_rope(x, w, positions, slots, rope, q_out, k_cache, v_cache, nh, nkv, k_scale, v_scale)
    ref.paged_attention(0, q_out.view(B, nh, 128), k_cache, v_cache, block_tables, q_start, q_len, ctx_len, work_seq,
                        work_tile, out.view(B, nh, 128), part_o, part_ml, part, nparts, k_scale, v_scale)
    return 0


def sample_candidates(logits, temperature, top_k, top_p, seeds, positions, active, cand, vocab_offset=0):
    """Per-rank pass: cand [B, C, 2] <- best (score, index) of each vocab chunk (Gumbel-max / argmax)."""
    if _hip(logits):
        torch.ops.dsse.sample_candidates(logits, temperature, top_k, top_p, seeds, positions, active, cand,
                                         vocab_offset)
    else:
        ref.sample_candidates(logits, temperature, top_k, top_p, seeds, positions, active, cand, vocab_offset)


def sample_pick(cand_all, active, next_ids, ring=None, ring_counter=None, positions_inc=None,
                vocab: int = 2**31 - 1):
    """Merge cand_all [world, B, C, 2] and commit: next_ids[b], ring[head][b], positions[b] += 1."""
    if _hip(cand_all):
        torch.ops.dsse.sample_pick(cand_all, active, next_ids, ring, ring_counter, positions_inc, vocab)
    else:
        ref.sample_pick(cand_all, active, next_ids, ring, ring_counter, positions_inc)


def prefill_sample_gather(x, meta, slot_meta, xl, smeta):
    """First-token sampling inside the prefill / mixed graphs: xl = the finishing prompts' last rows of x, smeta =
    their slots' sampling parameters (sampler.hip prefill_sample_gather_kernel has the layouts)."""
    if _hip(x):
        torch.ops.dsse.prefill_sample_gather(x, meta, slot_meta, xl, smeta)
    else:
        ref.prefill_sample_gather(x, meta, slot_meta, xl, smeta)


def prefill_sample_commit(meta, new_ids, ids, ring, positions):
    """ids[slot] = ring[ring_row][slot] = new_ids[i], positions[slot] = last_pos[i] + 1 for the n finishing prompts."""
    if _hip(new_ids):
        torch.ops.dsse.prefill_sample_commit(meta, new_ids, ids, ring, positions)
    else:
        ref.prefill_sample_commit(meta, new_ids, ids, ring, positions)


def sample_penalties(logits, active, pen_meta, hist, row_slot=None, vocab_offset=0, vocab: int = 2**31 - 1):
    """Presence / frequency / repetition penalties, in place on logits [B, V] (row stride >= V) before
    sample_candidates.  pen_meta int32 [4 Bm] = [presence | frequency | repetition (float32 bits) | n_prompt] per
    slot; hist int32 [Bm, capacity + 1] = [tokens held | prompt then generated tokens]; row b is slot row_slot[b]
    (else b).  Inactive rows and rows with neutral parameters keep their logits bit for bit."""
    if _hip(logits):
        torch.ops.dsse.sample_penalties(logits, active, pen_meta, hist, row_slot, vocab_offset, vocab)
    else:
        ref.sample_penalties(logits, active, pen_meta, hist, row_slot, vocab_offset, vocab)


CTL_BIAS, CTL_BAN, CTL_BODY = ref.CTL_BIAS, ref.CTL_BAN, ref.CTL_BODY  # logit_bias entries / banned ids / body words


def sample_bias_ban(logits, active, ctl_meta, ctl_body, positions, row_slot=None, vocab_offset=0,
                    vocab: int = 2**31 - 1):
    """logit_bias and the min_tokens ban, in place on logits [B, V] (row stride >= V): after logprob_stats, before
    sample_penalties.  ctl_meta int32 [4 Bm] = [bias entries | banned ids | ban-until position | min_p bits] per
    slot; ctl_body int32 [Bm, 620] = [300 x (global id, bias float32 bits) | 17 banned ids | pad]; row b is slot
    row_slot[b] (else b); positions[b] = the position of row b's predecessor token.  x[id] += bias, then x[id] = -inf
    for the banned ids while positions[b] + 1 < ban_until.  Inactive rows and rows with nothing to do keep their
    logits bit for bit."""
    if _hip(logits):
        torch.ops.dsse.sample_bias_ban(logits, active, ctl_meta, ctl_body, positions, row_slot, vocab_offset, vocab)
    else:
        ref.sample_bias_ban(logits, active, ctl_meta, ctl_body, positions, row_slot, vocab_offset, vocab)


def sample_candidates_min_p(logits, temperature, top_k, top_p, seeds, positions, active, cand, ctl_meta,
                            row_slot=None, vocab_offset=0):
    """sample_candidates with min_p (ctl_meta's fourth column, per slot; row b is slot row_slot[b], else b): after
    temperature a sampling row keeps x_i / T - max_j x_j / T >= ln(min_p), then top-k and top-p act on the survivors.
    0 = off; greedy rows are unaffected."""
    if _hip(logits):
        torch.ops.dsse.sample_candidates_min_p(logits, temperature, top_k, top_p, seeds, positions, active, cand,
                                               ctl_meta, row_slot, vocab_offset)
    else:
        ref.sample_candidates(logits, temperature, top_k, top_p, seeds, positions, active, cand, vocab_offset,
                              ctl_meta, row_slot)


# guided decoding: DFA states per pattern / resident patterns / bytes per piece / the dead state (api.h)
GUIDE_STATES, GUIDE_POOL, GUIDE_TOK_BYTES, GUIDE_DEAD = ref.GUIDE_STATES, ref.GUIDE_POOL, ref.GUIDE_TOK_BYTES, ref.GUIDE_DEAD
guide_token_table, guide_walk = ref.guide_token_table, ref.guide_walk
# the wide class of schema guides (guided_json / response_format json_schema): states per table / resident tables
GUIDE_WIDE_STATES, GUIDE_WIDE_POOL = ref.GUIDE_WIDE_STATES, ref.GUIDE_WIDE_POOL
# JSON mode (response_format json_object): the guide_meta entry word of a JSON slot, the depth cap, the pushdown
# automaton's table and its host walkers (bytes / the whole vocabulary / token ids); json_state int32 [4, slots]
JSON_ENTRY, JSON_DEPTH, JSON_START, JSON_DONE = ref.JSON_ENTRY, ref.JSON_DEPTH, ref.JSON_START, ref.JSON_DONE
JSON_START_STATE, JSON_DEAD_STATE = ref.JSON_START_STATE, ref.JSON_DEAD_STATE
json_table, json_walk, json_walk_all, json_walk_ids = ref.json_table, ref.json_walk, ref.json_walk_all, ref.json_walk_ids
json_state_words = ref.json_state_words


def guide_attach_json(guide_meta, json_tab, json_state):
    """JSON mode's two tensors travel with the guide_meta tensor they belong to (guide_mask / guide_advance keep their
    signatures): json_tab int16 [n, 256] (json_table's bits) and json_state int32 [4 slots], on guide_meta's device.
    Held as an attribute of this tensor object: a view or a copy of it does not carry them.  Returns guide_meta."""
    if json_state.numel() != 2 * guide_meta.numel() or json_state.device != guide_meta.device:
        raise ValueError("json_state must be [4 x slots] for guide_meta's slots, on its device")
    guide_meta.json_mode = (json_tab, json_state)
    return guide_meta


def _json_of(guide_meta):
    return getattr(guide_meta, "json_mode", (None, None))


def guide_attach_wide(guide_meta, tab_wide, flags_wide):
    """The wide pool of schema guides travels with guide_meta as JSON mode's tensors do: tab_wide int16 [pool <=
    GUIDE_WIDE_POOL, GUIDE_WIDE_STATES, 256] and flags_wide int32 [pool, GUIDE_WIDE_STATES], on guide_meta's device.
    A slot whose entry word is GUIDE_POOL + e then uses wide entry e; without them such a slot counts as off.
    Returns guide_meta."""
    if tab_wide.dim() != 3 or tuple(tab_wide.shape[1:]) != (GUIDE_WIDE_STATES, 256) or \
            not 1 <= tab_wide.shape[0] <= GUIDE_WIDE_POOL or tab_wide.dtype != torch.int16 or \
            tuple(flags_wide.shape) != (tab_wide.shape[0], GUIDE_WIDE_STATES) or flags_wide.dtype != torch.int32 or \
            tab_wide.device != guide_meta.device or flags_wide.device != guide_meta.device:
        raise ValueError("the wide pool must be int16 [pool <= 4, 4096, 256] and int32 [pool, 4096] on guide_meta's device")
    guide_meta.wide_pool = (tab_wide, flags_wide)
    return guide_meta


def _wide_of(guide_meta):
    return getattr(guide_meta, "wide_pool", (None, None))


def guide_live(tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, entry: int, n_states: int, eos: int = -1):
    """Once per table upload, stream-ordered before first use: bit 1 (stuck) of guide_flags[entry, s], s < n_states =
    no token of the global vocabulary other than EOS survives from state s.  entry >= GUIDE_POOL: wide entry entry -
    GUIDE_POOL of the pool attached to guide_meta (guide_attach_wide), n_states <= GUIDE_WIDE_STATES."""
    tab_wide, flags_wide = _wide_of(guide_meta)
    if entry >= GUIDE_POOL and (tab_wide is None or entry - GUIDE_POOL >= tab_wide.shape[0]):
        raise ValueError("guide_live: a wide entry needs the wide pool (guide_attach_wide)")
    if _hip(guide_tab):
        torch.ops.dsse.guide_live(tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, entry, n_states, eos,
                                  tab_wide, flags_wide)
    else:
        ref.guide_live(tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, entry, n_states, eos, tab_wide,
                       flags_wide)


def guide_mask(logits, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, row_slot=None, vocab_offset=0,
               eos: int = -1):
    """The guide's token mask, in place on logits [B, V] (row stride >= V): after sample_penalties, immediately before
    the candidates.  guide_meta int32 [2 slots] = pool index (-1 = off) | DFA state per slot; row b is slot
    row_slot[b] (else b).  Inactive rows, guide-off slots and dead states keep their logits bit for bit; otherwise a
    column stays iff its token's bytes walk from the state without meeting dead (EOS: iff accepting or stuck; 0.0 at a
    stuck state), else -inf.  Where guide_meta carries JSON mode's tensors (guide_attach_json), a slot whose pool index
    is JSON_ENTRY is masked by the pushdown walk of JSON mode, in the same launch; without them it counts as off.
    Likewise a slot whose pool index is GUIDE_POOL + e walks wide entry e of the pool attached with guide_attach_wide
    (states below GUIDE_WIDE_STATES)."""
    json_tab, json_state = _json_of(guide_meta)
    tab_wide, flags_wide = _wide_of(guide_meta)
    if _hip(logits):
        torch.ops.dsse.sample_guide_mask(logits, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta,
                                         row_slot, vocab_offset, eos, json_tab, json_state, tab_wide, flags_wide)
    else:
        ref.guide_mask(logits, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, row_slot, vocab_offset,
                       eos, json_tab, json_state, tab_wide, flags_wide)


def guide_advance(ids, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, row_slot=None, eos: int = -1):
    """After a commit: the guide state of row b's slot advances by the committed global id ids[b] (EOS: unchanged; a
    dead walk or a token of length 0: dead).  JSON-mode slots move their json_state words (see guide_mask)."""
    json_tab, json_state = _json_of(guide_meta)
    tab_wide, flags_wide = _wide_of(guide_meta)
    if _hip(guide_meta):
        torch.ops.dsse.sample_guide_advance(ids, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta,
                                            row_slot, eos, json_tab, json_state, tab_wide, flags_wide)
    else:
        ref.guide_advance(ids, active, tok_bytes, tok_len, guide_tab, guide_flags, guide_meta, row_slot, eos,
                          json_tab, json_state, tab_wide, flags_wide)


def sample_pick_hist(cand_all, active, next_ids, ring, ring_counter, positions_inc, pen_meta, hist,
                     vocab: int = 2**31 - 1):
    """sample_pick whose picked token also joins hist[b] (device-side, stream-ordered) where slot b has penalties."""
    if _hip(cand_all):
        torch.ops.dsse.sample_pick_hist(cand_all, active, next_ids, ring, ring_counter, positions_inc, pen_meta, hist,
                                        vocab)
    else:
        ref.sample_pick_hist(cand_all, active, next_ids, ring, ring_counter, positions_inc, pen_meta, hist, vocab)


def prefill_sample_commit_hist(meta, new_ids, ids, ring, positions, pen_meta, hist):
    """prefill_sample_commit whose first tokens also join the history of the slots that have penalties."""
    if _hip(new_ids):
        torch.ops.dsse.prefill_sample_commit_hist(meta, new_ids, ids, ring, positions, pen_meta, hist)
    else:
        ref.prefill_sample_commit_hist(meta, new_ids, ids, ring, positions, pen_meta, hist)


def sample_hist_append(new_ids, row_slot, active, pen_meta, hist):
    """hist[slot] += new_ids[i] (slot = row_slot[i], else i) for active rows whose slot has penalties."""
    if _hip(new_ids):
        torch.ops.dsse.sample_hist_append(new_ids, row_slot, active, pen_meta, hist)
    else:
        ref.sample_hist_append(new_ids, row_slot, active, pen_meta, hist)


LP_TOP = 20            # top_logprobs at most
LP_REC = 2 + 2 * LP_TOP   # per-(rank, row) record [max | sum exp(x - max) | LP_TOP x (logit, id bits)]
LP_OUT = 1 + 2 * LP_TOP   # per-token result [logprob of the sampled token | LP_TOP ids | LP_TOP logprobs]


def logprob_stats(logits, active, lp_meta, row_slot, rec, raw=None, vocab_offset=0):
    """Raw-logprob statistics of this rank's logits shard [B, V] (fp32, as the LM head wrote them: call it BEFORE
    sample_penalties).  lp_meta int32 [slots]: -1 = off, 0..20 = N; row b is slot row_slot[b] (else b).  Rows that
    are active and on get rec[b] = [max | sum exp(x - max) | 20 x (logit, global id bits)]: the shard's top-N by
    logit descending, equal logits by ascending id, unused entries (-inf, 0x7fffffff); `raw` [>= B, V] (optional)
    receives a copy of those rows.  Other rows leave rec / raw untouched."""
    if _hip(logits):
        torch.ops.dsse.logprob_stats(logits, active, lp_meta, row_slot, rec, raw, vocab_offset)
    else:
        ref.logprob_stats(logits, active, lp_meta, row_slot, rec, raw, vocab_offset)


def logprob_chosen(logits, next_ids, active, lp_meta, row_slot, chosen, vocab_offset=0, vocab: int = 2**31 - 1):
    """chosen[b] = logits[b, next_ids[b] - vocab_offset] when this shard holds the sampled id, else -inf (rows that
    are active and on).  `logits` must be the un-penalised values (logprob_stats' raw copy after a penalty pass)."""
    if _hip(logits):
        torch.ops.dsse.logprob_chosen(logits, next_ids, active, lp_meta, row_slot, chosen, vocab_offset, vocab)
    else:
        ref.logprob_chosen(logits, next_ids, active, lp_meta, row_slot, chosen, vocab_offset, vocab)


def logprob_finish(rec_all, chosen_all, active, lp_meta, row_slot, lp_ring, ring_counter=None, ring_row_dev=None,
                   ring_row: int = -1, vocab: int = 2**31 - 1):
    """Merge rec_all [world, B, 42] and chosen_all [world, B]: lse over all shards, the global top-N in the same
    order, and lp_ring[row, slot] = [logprob of the sampled token | 20 ids | 20 logprobs] (entries past min(N, vocab):
    id -1, -inf).  row = ring_counter[0] % R, else ring_row_dev[0], else ring_row: where the token itself went."""
    if _hip(rec_all):
        torch.ops.dsse.logprob_finish(rec_all, chosen_all, active, lp_meta, row_slot, lp_ring, ring_counter,
                                      ring_row_dev, ring_row, vocab)
    else:
        ref.logprob_finish(rec_all, chosen_all, active, lp_meta, row_slot, lp_ring, ring_counter, ring_row_dev,
                           ring_row, vocab)


def sample(logits, temperature, top_k, top_p, seeds, positions, active, next_ids, ring=None, ring_counter=None,
           positions_inc=None, nchunks: int = 16):
    """Single-rank convenience: candidates + pick."""
    B = logits.shape[0]
    cand = torch.empty(B, nchunks if logits.is_cuda else 1, 2, device=logits.device, dtype=torch.float32)
    sample_candidates(logits, temperature, top_k, top_p, seeds, positions, active, cand, 0)
    sample_pick(cand.unsqueeze(0), active, next_ids, ring, ring_counter, positions_inc)


def _kv_pages_args(k_cache, v_cache, blocks, staging, unique: bool):
    """Validate a page list ON THE HOST before anything is launched (a wild copy on the GPU is a fault): every index in
    [0, num_blocks), no duplicates for a scatter, no more pages than staging has records, and one element type for K,
    V and staging.  `blocks`: a list of ints or a CPU int32 tensor (pinned: its upload is then asynchronous).  Returns
    the list as an int32 tensor on the cache's device."""
    if isinstance(blocks, torch.Tensor):
        if blocks.is_cuda:
            raise ValueError("blocks must be a host list or CPU tensor: its indices are validated before the launch")
        if blocks.dtype != torch.int32 or blocks.dim() != 1:
            raise ValueError(f"blocks must be a 1-D int32 tensor, got {blocks.dtype} {tuple(blocks.shape)}")
        vals, host = blocks.tolist(), blocks
    else:
        vals = [int(b) for b in blocks]
        host = None
    if k_cache.dim() != 5 or v_cache.dim() != 5 or staging.dim() != 2:
        raise ValueError("k_cache / v_cache must be the 5-D paged caches and staging [records, bytes_per_block / itemsize]")
    if not (k_cache.dtype == v_cache.dtype == staging.dtype):
        raise ValueError(f"staging dtype {staging.dtype} and cache dtypes {k_cache.dtype} / {v_cache.dtype} must agree")
    num_blocks = k_cache.shape[1]
    bad = [b for b in vals if not 0 <= b < num_blocks]
    if bad:
        raise ValueError(f"blocks: index {bad[0]} outside [0, {num_blocks})")
    if unique and len(set(vals)) != len(vals):
        raise ValueError("blocks: a scatter may name each page once (duplicate index)")
    if len(vals) > staging.shape[0]:
        raise ValueError(f"blocks: n = {len(vals)} pages exceed the staging capacity of {staging.shape[0]} records")
    if host is None:
        host = torch.tensor(vals, dtype=torch.int32)
    return host.to(k_cache.device, non_blocking=True) if k_cache.is_cuda else host


def kv_pages_gather(k_cache, v_cache, blocks, staging):
    """staging[i] = page blocks[i] of the paged cache as one contiguous record [K layer 0 .. L-1 | V layer 0 .. L-1]
    (host tier of the prefix cache; csrc/kernels/kv_pages.hip).  `blocks` is a host list, validated here."""
    dev = _kv_pages_args(k_cache, v_cache, blocks, staging, unique=False)
    if _hip(k_cache):
        torch.ops.dsse.kv_pages_gather(k_cache, v_cache, dev, staging)
    else:
        ref.kv_pages_gather(k_cache, v_cache, dev, staging)


def kv_pages_scatter(staging, blocks, k_cache, v_cache):
    """The inverse of kv_pages_gather: page blocks[i] of the cache = staging[i]; every other page is untouched."""
    dev = _kv_pages_args(k_cache, v_cache, blocks, staging, unique=True)
    if _hip(k_cache):
        torch.ops.dsse.kv_pages_scatter(staging, dev, k_cache, v_cache)
    else:
        ref.kv_pages_scatter(staging, dev, k_cache, v_cache)


def kv_pages_copy(k_cache, v_cache, pairs):
    """Page dst = page src for every (src, dst) of `pairs`, all layers, K and V, inside the paged cache (parallel
    sampling: a sibling's private copy of its parent's partial last prompt page; csrc/kernels/kv_pages.hip).  `pairs` is
    a host list of (src_block, dst_block), validated HERE before anything is launched: every index in [0, num_blocks),
    each destination named once, and no destination also a source (one source may feed several destinations).  Every
    page that is not a destination is untouched."""
    if isinstance(pairs, torch.Tensor):
        if pairs.is_cuda:
            raise ValueError("pairs must be a host list or CPU tensor: its indices are validated before the launch")
        pairs = pairs.tolist()
    vals = []
    for p in pairs:
        if len(p) != 2:
            raise ValueError("pairs: every entry is (src_block, dst_block)")
        vals.append((int(p[0]), int(p[1])))
    if k_cache.dim() != 5 or v_cache.dim() != 5 or k_cache.shape[:3] != v_cache.shape[:3]:
        raise ValueError("k_cache / v_cache must be the 5-D paged caches of one shape")
    if k_cache.dtype != v_cache.dtype:
        raise ValueError(f"cache dtypes {k_cache.dtype} / {v_cache.dtype} must agree")
    num_blocks = k_cache.shape[1]
    bad = [b for p in vals for b in p if not 0 <= b < num_blocks]
    if bad:
        raise ValueError(f"pairs: index {bad[0]} outside [0, {num_blocks})")
    dsts = [d for _, d in vals]
    if len(set(dsts)) != len(dsts):
        raise ValueError("pairs: each destination page may be named once (duplicate destination)")
    both = set(dsts) & {s for s, _ in vals}
    if both:
        raise ValueError(f"pairs: page {min(both)} is both a destination and a source")
    if not vals:
        return  # nothing is launched
    host = torch.tensor(vals, dtype=torch.int32).view(-1, 2)
    if _hip(k_cache):
        dev = host.pin_memory().to(k_cache.device, non_blocking=True)
        torch.ops.dsse.kv_pages_copy(k_cache, v_cache, dev)
    else:
        ref.kv_pages_copy(k_cache, v_cache, host)


class KernelCheckError(RuntimeError):
    """An out-of-range device index caught by the checked kernel build."""


def kernel_checks(clear: bool = True, raise_on_error: bool = True) -> list:
    """Read the checked build's violation words (``_build.py kernels-checked``, DSSE_KERNELS_VARIANT=checked).

    Returns ``[(file, line, value, bound, count)]`` for every kernel file that recorded an out-of-range
    index since the last clear; raises KernelCheckError when ``raise_on_error`` and any were found.  The
    default build records nothing (empty list).  Synchronises the device.
    """
    load_library(required=True)
    if not torch.ops.dsse.kernels_checked():
        return []
    words = torch.ops.dsse.kernel_checks(clear).tolist()
    files = torch.ops.dsse.kernel_check_files().split(",")
    bad = [(f, *w) for f, w in zip(files, words) if w[3] > 0]
    if bad and raise_on_error:
        raise KernelCheckError("; ".join(f"{f}:{ln} index {v} not below {b} ({n} times)" for f, ln, v, b, n in bad))
    return bad

