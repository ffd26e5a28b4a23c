"""MXFP4 weights on the CPU: the quantiser (grid, ties, scale rule, error bound), the nibble order, the device layout
and its inverse, exact widening, the reference ops (equal to the bf16 reference ops on the widened weights), the engine
weights and the CPU runner under quantization="mxfp4", the option's parsing (--quantization / QUANTIZATION) and the
kernel's entry (metadata of a cross-compile only)."""
import argparse
import math
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from distributed_sse_for_llm_response_amd import _build, ops
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import (QUANTIZATIONS, convert_standard, parse_quantization,
                                                                 quantize_engine_weights, random_engine_weights)
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights, reference_forward
from distributed_sse_for_llm_response_amd.ops import reference as R
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _codes(q):
    """Row-major nibble codes [N, K] of packed bytes [N, K / 2]: element k (even) low, element k + 1 high."""
    return torch.stack((q & 15, q >> 4), dim=2).reshape(q.shape[0], -1)


def _block_weight(vals, fill=0.0):
    """A [16, 128] weight whose row 0, first 32-block starts with `vals` (the rest of the block is `fill`)."""
    w = torch.zeros(16, 128)
    w[0, :32] = fill
    w[0, : len(vals)] = torch.tensor(vals)
    return w


# ---------------------------------------------------------------- grid and ties
@pytest.mark.parametrize("e", [-9, -1, 0, 3, 11])
def test_grid_values_are_fixed_points(e):
    s = 2.0 ** e
    vals = [s * g for g in GRID] + [-s * g for g in GRID]  # amax = 6 s: the block scale is s
    w = _block_weight(vals)
    q, sc = R.quantize_weight_mxfp4(w)
    assert q.dtype == torch.uint8 and q.shape == (16, 64) and sc.dtype == torch.uint8 and sc.shape == (16, 4)
    assert int(sc[0, 0]) == 127 + e
    assert _codes(q)[0, :16].tolist() == list(range(8)) + [0] + list(range(9, 16))  # -0 stores code 0
    assert torch.equal(R.widen_weight_mxfp4(q, sc).float(), w)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_midpoints_round_to_the_even_code(sign):
    mids = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    s = 2.0 ** -3
    w = _block_weight([sign * s * m for m in mids] + [6.0 * s])  # the 6 pins the scale to s
    q, sc = R.quantize_weight_mxfp4(w)
    assert int(sc[0, 0]) == 124
    wide = R.widen_weight_mxfp4(q, sc).float()
    assert wide[0, :7].tolist() == [sign * s * v if v else 0.0 for v in want]
    assert _codes(q)[0, 0] == 0  # +-0.25 rounds to zero: code 0, never 8
    # just off a midpoint goes to the nearer neighbour
    w = _block_weight([sign * s * 2.5 * (1 + 2.0 ** -7), sign * s * 2.5 * (1 - 2.0 ** -7), 6.0 * s])
    wide = R.widen_weight_mxfp4(*R.quantize_weight_mxfp4(w)).float()
    assert wide[0, :2].tolist() == [sign * s * 3.0, sign * s * 2.0]


def test_negatives_that_round_to_zero_store_code_zero():
    w = _block_weight([-0.2, -0.25, -0.0, 6.0])
    q, _ = R.quantize_weight_mxfp4(w)
    assert _codes(q)[0, :3].tolist() == [0, 0, 0]
    assert not (_codes(R.quantize_weight_mxfp4(-torch.rand(16, 128) * 1e-3 + _block_weight([6.0]))[0]) == 8).any()


# ---------------------------------------------------------------- scale rule
def test_scale_rule():
    up = 1 + 2.0 ** -7  # the next bf16 above / below a power of two times 1.5
    cases = {6.0 * 2.0 ** -5: 122, 6.0 * 2.0 ** -5 * up: 123, 6.0 * 2.0 ** -5 * (1 - 2.0 ** -8): 122,
             6.0 * 2.0 ** 4: 131, 6.0 * 2.0 ** 4 * up: 132, 0.0: 127,
             2.0 ** -100: 63, 6.0 * 2.0 ** -64: 63, 6.0 * 2.0 ** -63: 64, 6.0 * 2.0 ** 64: 191}
    w = torch.zeros(16, 128 * 3)
    for i, amax in enumerate(cases):
        w[0, 32 * i + (5 * i) % 32] = -amax if i % 2 else amax
    q, sc = R.quantize_weight_mxfp4(w)
    assert sc[0, : len(cases)].tolist() == list(cases.values())
    assert bool((sc[1:] == 127).all()) and not q[1:].any()  # all-zero blocks
    wide = R.widen_weight_mxfp4(q, sc).float()
    exact = [a for a in cases if a in (6.0 * 2.0 ** -5, 6.0 * 2.0 ** 4, 6.0 * 2.0 ** -64, 6.0 * 2.0 ** -63, 6.0 * 2.0 ** 64)]
    for i, amax in enumerate(cases):
        if amax in exact:
            assert abs(float(wide[0, 32 * i + (5 * i) % 32])) == amax


def _spread_weight(N, K, seed):
    """N(0, 1/sqrt(K)) with row n scaled by 2^(n mod 16) and, inside a row, 32-block j by 2^(-(5 j) mod 16)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    w = w * torch.ldexp(torch.ones(N), (torch.arange(N) % 16).int())[:, None]
    blk = torch.ldexp(torch.ones(K // 32), -((torch.arange(K // 32) * 5) % 16).int())
    return (w * blk.repeat_interleave(32)[None, :]).bfloat16()


def test_no_saturation_and_error_bound_from_the_grid():
    N, K = 256, 1536
    w = _spread_weight(N, K, 3)
    q, sc = R.quantize_weight_mxfp4(w)
    s = torch.ldexp(torch.ones(sc.shape), sc.int() - 127).repeat_interleave(32, dim=1)
    wf = w.float()
    amax = wf.abs().view(N, K // 32, 32).amax(2)
    sb = torch.ldexp(torch.ones(sc.shape), sc.int() - 127)
    assert bool((6.0 * sb >= amax).all()) and bool((6.0 * (sb * 0.5) < amax)[amax > 0].all())  # the smallest such
    assert len(sc.unique()) >= 16
    wide = R.widen_weight_mxfp4(q, sc)
    assert wide.dtype == torch.bfloat16 and wide.shape == (N, K)
    v = wf.abs() / s
    mag = wide.float().abs() / s
    assert bool((mag <= 6.0).all()) and bool((v[mag == 6.0] >= 5.0).all()) and bool((mag == 6.0).any())
    # half the grid step at v: 0.5 up to 2, 1 up to 4, 2 up to 6
    bound = s * torch.where(v <= 2, 0.25, torch.where(v <= 4, 0.5, 1.0))
    assert bool(((wide.float() - wf).abs() <= bound).all())
    assert bool((torch.sign(wide.float()) * torch.sign(wf) >= 0).all())


# ---------------------------------------------------------------- layout and widening
@pytest.mark.parametrize("N", [16, 48, 512])
@pytest.mark.parametrize("K", [128, 384, 1536])
def test_layout_round_trip_and_documented_order(N, K):
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    e = torch.randint(63, 192, (N, K // 32), generator=g, dtype=torch.uint8)
    qt, et = R.tile_weight_mxfp4(q, e)
    assert qt.shape == q.shape and et.shape == e.shape and qt.dtype == et.dtype == torch.uint8
    q2, e2 = R.untile_weight_mxfp4(qt, et)
    assert torch.equal(q2, q) and torch.equal(e2, e)
    # positions: tile three byte planes of the linear index
    for src, width, tile_one in ((N * K // 2, K // 2, lambda p: R.tile_weight_mxfp4(p, e)[0]),
                                 (N * K // 32, K // 32, lambda p: R.tile_weight_mxfp4(q, p)[1])):
        idx = torch.arange(src).view(N, width)
        pos = sum(tile_one(((idx >> (8 * p)) & 255).to(torch.uint8)).to(torch.int64) << (8 * p) for p in range(3)).view(-1)
        assert torch.equal(pos.sort().values, torch.arange(src))
        T, c, lane = N // 16 - 1, K // 128 - 1, 37
        r, gq = lane & 15, lane >> 4
        if width == K // 2:  # block (T, c) of 1 KiB, [lane][b]: the bytes of W[16T + r][128c + 32g + 2b, + 2b + 1]
            b = 11
            assert int(pos[(T * (K // 128) + c) * 1024 + lane * 16 + b]) == (16 * T + r) * width + 64 * c + 16 * gq + b
        else:                # block (T, c) of 64 B, [lane]: the scale of W[16T + r][128c + 32g ..]
            assert int(pos[(T * (K // 128) + c) * 64 + lane]) == (16 * T + r) * width + 4 * c + gq


def test_nibble_order_and_exact_widening():
    N, K = 32, 256
    w = torch.zeros(N, K)
    cols = [(7 * n + 3) % K for n in range(N)]  # one non-zero element per row, odd and even columns
    for n, k in enumerate(cols):
        w[n, k] = (-1.0) ** n * 1.5 * 2.0 ** (n % 5)
    q, e = R.quantize_weight_mxfp4(w)
    for n, k in enumerate(cols):
        byte = int(q[n, k // 2])
        code = 7 | (8 if n % 2 else 0)  # the block's only value is its amax: 6 = exponent 11, mantissa 1
        assert byte == (code << 4 if k % 2 else code), (n, k, byte)
        assert int(q[n].count_nonzero()) == 1
        assert int(e[n, k // 32]) == 127 + n % 5 - 2  # amax = 1.5 * 2^j = 6 * 2^(j - 2)
    assert torch.equal(R.widen_weight_mxfp4(q, e).float(), w)
    # widening against an fp64 computation from the definition, every code and a range of scale bytes
    g = torch.Generator().manual_seed(1)
    q = torch.randint(0, 256, (64, 128), generator=g, dtype=torch.uint8)
    e = torch.randint(63, 192, (64, 8), generator=g, dtype=torch.uint8)
    code = _codes(q).long()
    man, ex, sg = code & 1, (code >> 1) & 3, code >> 3
    val = torch.where(ex == 0, 0.5 * man.double(), (1 + 0.5 * man.double()) * 2.0 ** (ex.double() - 1))
    want = (1 - 2 * sg).double() * val * 2.0 ** (e.double() - 127).repeat_interleave(32, dim=1)
    got = R.widen_weight_mxfp4(q, e)
    assert got.dtype == torch.bfloat16 and torch.equal(got.double(), want)


# ---------------------------------------------------------------- reference ops
def test_reference_ops_equal_the_bf16_ops_on_the_widened_weight():
    g = torch.Generator().manual_seed(5)
    M, K, nh, nkv = 5, 256, 2, 1
    x = torch.randn(M, K, generator=g).bfloat16()

    def quant(N):
        q, e = R.quantize_weight_mxfp4((torch.randn(N, K, generator=g) / 16).bfloat16())
        return *R.tile_weight_mxfp4(q, e), R.tile_weight(R.widen_weight_mxfp4(q, e))

    wq, we, wt = quant(64)
    for dt in (torch.bfloat16, torch.float32):
        a, b = torch.zeros(M, 64, dtype=dt), torch.zeros(M, 64, dtype=dt)
        ops.gemm_out_w4(x, wq, we, a)
        ops.gemm_out(x, wt, b)
        assert torch.equal(a, b) and a.abs().sum() > 0
    a, b = torch.ones(M, 64), torch.ones(M, 64)
    part = torch.zeros(8 * M * 64)
    assert ops.gemm_resid_split_w4(x, wq, we, a, part) == 0 and ops.gemm_resid_split(x, wt, b, part) == 0
    ops.gemm_resid_w4(x, wq, we, a)
    ops.gemm_resid(x, wt, b)
    assert torch.equal(a, b)
    a, b = torch.zeros(M, 32, dtype=torch.bfloat16), torch.zeros(M, 32, dtype=torch.bfloat16)
    ops.gemm_silu_w4(x, wq, we, a)
    ops.gemm_silu(x, wt, b)
    assert torch.equal(a, b)
    a, b = torch.zeros(M, 64, dtype=torch.bfloat16), torch.zeros(M, 64, dtype=torch.bfloat16)
    assert ops.gemm_out_split_w4(x, wq, we, a, part) == 0 and ops.gemm_out_split(x, wt, b, part) == 0
    assert torch.equal(a, b)
    assert ops.W4_MAX_M == 64

    wq, we, wt = quant((nh + 2 * nkv) * 128)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    pos, slots = i32(3, 4, 5, 6, 7), i32(3, 4, 5, 6, 7)
    rope = R.rope_table(64, 10000.0)
    bt = torch.zeros(M, 2, dtype=torch.int32)
    outs = []
    for w4 in (True, False, None):
        kc = torch.zeros(2, nkv, 32, 128, dtype=torch.bfloat16)
        vc = torch.zeros(2, nkv, 128, 32, dtype=torch.bfloat16)
        qo = torch.zeros(M, nh * 128, dtype=torch.bfloat16)
        o = torch.zeros(M, nh * 128, dtype=torch.bfloat16)
        meta = (bt, torch.arange(M, dtype=torch.int32), torch.ones(M, dtype=torch.int32), pos + 1,
                torch.arange(M, dtype=torch.int32), torch.zeros(M, dtype=torch.int32))
        if w4:
            ops.qkv_attention_decode_w4(x, wq, we, pos, slots, rope, qo, kc, vc, nh, nkv, part, *meta, o, part, part,
                                        32, 1)
        elif w4 is None:
            ops.gemm_qkv_rope_w4(x, wq, we, pos, slots, rope, qo, kc, vc, nh, nkv)
            o = outs[0][3]
        else:
            ops.qkv_attention_decode(x, wt, pos, slots, rope, qo, kc, vc, nh, nkv, part, *meta, o, part, part, 32, 1)
        outs.append((qo, kc, vc, o))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert outs[0][1].abs().sum() > 0 and outs[0][3].abs().sum() > 0


# ---------------------------------------------------------------- engine weights
MATS = ("wqkv", "wo", "wgu", "wd")


def _check_copies(w):
    """Every matrix: *_t is the tiling of the values widened from (*_q, *_e)."""
    for holder, names in [(w, ("lm_head",))] + [(L, MATS) for L in w.layers]:
        for f in names:
            q, e, t = (getattr(holder, f + s) for s in ("_q", "_e", "_t"))
            assert q.dtype == e.dtype == torch.uint8 and q.shape == (t.shape[0], t.shape[1] // 2)
            assert e.shape == (t.shape[0], t.shape[1] // 32) and getattr(holder, f + "_scale") is None
            assert torch.equal(t, R.tile_weight(R.widen_weight_mxfp4(*R.untile_weight_mxfp4(q, e))))


def test_engine_weights_under_mxfp4():
    std = init_standard_weights(TINY, seed=11)
    plain = convert_standard(TINY, std)
    w = convert_standard(TINY, std, quantization="mxfp4")
    assert w.quantization == "mxfp4" and plain.quantization == "none" and plain.nbytes_fp4() == 0
    _check_copies(w)
    # the matrices were quantised in the engine layout, from the values the unquantised load tiles
    q, e = R.quantize_weight_mxfp4(R.untile_weight(plain.layers[1].wd_t))
    assert torch.equal(w.layers[1].wd_q, R.tile_weight_mxfp4(q, e)[0])
    assert torch.equal(w.layers[1].wd_e, R.tile_weight_mxfp4(q, e)[1])
    assert not torch.equal(w.layers[1].wd_t, plain.layers[1].wd_t)
    # the embedding and the norms are left alone
    assert torch.equal(w.embed, plain.embed) and w.embed.dtype == torch.bfloat16
    assert torch.equal(w.final_norm, plain.final_norm) and torch.equal(w.layers[0].attn_norm, plain.layers[0].attn_norm)
    # both copies are counted: 4 bits per element and one byte per 32 of them
    mats = sum(t.numel() for L in w.layers for t in (L.wqkv_t, L.wo_t, L.wgu_t, L.wd_t)) + w.lm_head_t.numel()
    assert w.nbytes_fp4() == mats // 2 + mats // 32 and w.nbytes_fp8() == 0
    assert w.nbytes() == plain.nbytes() + w.nbytes_fp4()
    # weights loaded without the option are quantised to the same bytes, once
    r = ModelRunner(plain, num_blocks=8, max_batch=2, max_model_len=128, device="cpu", use_graphs=False,
                    quantization="mxfp4")
    assert r.quantization == "mxfp4" and r.w4 and not r.w8
    for a, b in zip(plain.layers, w.layers):
        for f in MATS:
            for s in ("_q", "_e", "_t"):
                assert torch.equal(getattr(a, f + s), getattr(b, f + s))
    assert torch.equal(plain.lm_head_q, w.lm_head_q) and torch.equal(plain.lm_head_t, w.lm_head_t)
    before = w.lm_head_q
    assert quantize_engine_weights(w, "mxfp4") is w and w.lm_head_q is before  # idempotent
    # FP8 weights are not quantised a second time, nor MXFP4 ones as FP8: an error, the weights as they were
    f8 = convert_standard(TINY, std, quantization="fp8")
    kept = f8.lm_head_q
    with pytest.raises(ValueError, match="already quantised as fp8"):
        quantize_engine_weights(f8, "mxfp4")
    assert f8.quantization == "fp8" and f8.lm_head_q is kept and f8.nbytes_fp4() == 0 and f8.nbytes_fp8() > 0
    with pytest.raises(ValueError, match="already quantised as mxfp4"):
        ModelRunner(w, num_blocks=8, max_batch=2, max_model_len=128, device="cpu", use_graphs=False,
                    quantization="fp8")


def test_random_engine_weights_under_mxfp4():
    w = random_engine_weights(TINY, device="cpu", seed=5, quantization="mxfp4")
    assert w.quantization == "mxfp4" and w.nbytes_fp4() > 0
    _check_copies(w)
    plain = random_engine_weights(TINY, device="cpu", seed=5)
    assert torch.equal(w.embed, plain.embed) and plain.lm_head_q is None and plain.lm_head_e is None


# ---------------------------------------------------------------- option parsing
def test_config_cli_environment_json_and_refusals(monkeypatch, capsys):
    assert QUANTIZATIONS == ("none", "fp8", "mxfp4")
    monkeypatch.delenv("QUANTIZATION", raising=False)
    assert ServeConfig().quantization == "none"
    monkeypatch.setenv("QUANTIZATION", "MXFP4")
    assert ServeConfig.from_env().quantization == "mxfp4"
    ap = argparse.ArgumentParser()
    ServeConfig.add_args(ap)
    monkeypatch.delenv("QUANTIZATION")
    cfg = ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "mxfp4"]))
    assert cfg.quantization == "mxfp4"
    assert ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "MXFP4"])).quantization == "mxfp4"
    assert ServeConfig.from_json(cfg.to_json()).quantization == "mxfp4"  # what every DP replica gets
    with pytest.raises(SystemExit):
        ap.parse_args(["--quantization", "int4"])
    assert "'none', 'fp8', 'mxfp4'" in capsys.readouterr().err
    with pytest.raises(ValueError, match="none, fp8, mxfp4"):
        ServeConfig.from_env().update_from_args(argparse.Namespace(quantization="int4"))
    ok = ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "mxfp4", "--dp", "2",
                                                                "--kv-cache-dtype", "fp8"]))
    assert ok.quantization == "mxfp4" and ok.dp == 2 and ok.kv_cache_dtype.startswith("fp8")
    with pytest.raises(ValueError, match="not supported with tensor parallelism"):
        ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "mxfp4", "--tp", "2"]))
    with pytest.raises(ValueError, match="not supported with --quantization mxfp4"):
        ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "mxfp4", "--enable-lora"]))
    with pytest.raises(ValueError, match="mxfp4 is not supported with tensor parallelism"):
        convert_standard(TINY, init_standard_weights(TINY, seed=1), tp_rank=0, tp_size=2, quantization="mxfp4")
    w = convert_standard(TINY, init_standard_weights(TINY, seed=1), tp_rank=0, tp_size=2)
    with pytest.raises(ValueError, match="mxfp4 is not supported with tensor parallelism"):
        ModelRunner(w, num_blocks=8, max_batch=2, max_model_len=128, device="cpu", use_graphs=False,
                    comm=TPComm(rank=0, size=2), quantization="mxfp4")
    assert parse_quantization("mxfp4") == "mxfp4" and parse_quantization(" MXFP4 ") == "mxfp4"
    for bad in ("int4", "int8", "awq", "fp4"):
        with pytest.raises(ValueError, match="none, fp8, mxfp4"):
            parse_quantization(bad)


def test_lora_is_refused_by_the_runner():
    w = convert_standard(TINY, init_standard_weights(TINY, seed=1), quantization="mxfp4")
    with pytest.raises(ValueError, match="LoRA is not supported with quantization=mxfp4"):
        ModelRunner(w, num_blocks=8, max_batch=2, max_model_len=128, device="cpu", use_graphs=False, lora=object())


def test_bench_harness_takes_the_option_from_the_environment(monkeypatch):
    from distributed_sse_for_llm_response_amd.engine import bench_harness

    monkeypatch.setenv("QUANTIZATION", "mxfp4")
    _, r = bench_harness._build_runner("mistral-tiny", torch.device("cpu"), 2, 16, 4, 1, False, 0, 1)
    assert r.quantization == "mxfp4" and r.w4 and r.w.layers[0].wqkv_e is not None and r.w.nbytes_fp4() > 0
    monkeypatch.delenv("QUANTIZATION")
    _, r = bench_harness._build_runner("mistral-tiny", torch.device("cpu"), 2, 16, 4, 1, False, 0, 1)
    assert r.quantization == "none" and not r.w4 and r.w.layers[0].wqkv_e is None and r.w.nbytes_fp4() == 0


# ---------------------------------------------------------------- CPU runner
def _widened_std(seed):
    """HF-layout weights whose matrices are already the widened MXFP4 values: blocks of 32 along K stay blocks under
    the engine's row permutations, and widened values quantise to themselves, so the engine stores the same values."""
    std = init_standard_weights(TINY, seed=seed)
    wide = lambda m: R.widen_weight_mxfp4(*R.quantize_weight_mxfp4(m))
    out = dict(std, lm_head=wide(std["lm_head"]), layers=[])
    for L in std["layers"]:
        out["layers"].append({k: (wide(v) if k in ("q", "k", "v", "o", "gate", "up", "down") else v)
                              for k, v in L.items()})
    return std, out


def test_cpu_runner_decode_logits_against_the_reference_on_widened_weights():
    std, wide = _widened_std(3)
    w = convert_standard(TINY, std, quantization="mxfp4")
    assert torch.equal(w.lm_head_t, convert_standard(TINY, wide).lm_head_t)  # the engine serves the widened values
    r = ModelRunner(w, num_blocks=16, max_batch=2, max_model_len=256, device="cpu", use_graphs=False)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(3, TINY.vocab_size, (n,), generator=g).tolist() for n in (9, 40)]
    tables = [[0, 1, 2], [3, 4, 5]]
    for i, bt in enumerate(tables):
        r.block_tables[i, : len(bt)] = torch.tensor(bt, dtype=torch.int32)
    r.prefill([PrefillSeq(i, p, 0, tables[i], True) for i, p in enumerate(prompts)], ring_row=0)
    r.active.zero_()
    r.active[:2] = 1
    r.temperature.zero_()
    first = [int(t) for t in r.ids[:2]]
    r.decode(2)  # a 2-row bucket: every projection and the LM head on the *_w4 ops
    for i in range(2):
        ref, _ = reference_forward(TINY, wide, torch.tensor(prompts[i] + [first[i]]))
        a, b = ref[len(prompts[i])].float(), r.logits[i].float()
        cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
        rel = ((a - b).abs().max() / a.abs().max()).item()
        assert cos > 0.998 and rel < 0.05, (i, cos, rel)  # the model tolerance of the GPU runner tests
    plain, _ = reference_forward(TINY, std, torch.tensor(prompts[0] + [first[0]]))
    assert not torch.allclose(plain[len(prompts[0])].float(), r.logits[0].float(), atol=1e-3, rtol=1e-3)


# ---------------------------------------------------------------- kernel entry
def test_kernel_entry_operands_are_preloaded_and_nothing_hidden_is_read(tmp_path):
    """docs/kernels.md "Kernel entry", from the descriptor metadata of a device-only compile: the 12 dwords the first
    DMA burst needs (X(2) ldx M W(2) E(2) K Kr gx xs) arrive preloaded, and no grid / block hidden argument is read."""
    hipcc = shutil.which("hipcc") or (_build.HIPCC if Path(_build.HIPCC).exists() else None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path / "gemm_w4.s"
    cmd = [hipcc, *_build.kernel_device_flags(None), "-w", "-S", "--cuda-device-only",
           str(_build.CSRC / "kernels" / "gemm_w4.hip"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    asm = out.read_text()
    preload = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        pl = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", m.group(2))
        preload[m.group(1)] = int(pl.group(1)) if pl else 0
    meta = asm[asm.index("amdhsa.kernels:"):]
    meta = meta[: meta.index(".end_amdgpu_metadata")]
    kinds = {}
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        kinds[re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)] = re.findall(r"\.value_kind:\s+(\S+)", entry)
    ring = [k for k in preload if k.startswith("_ZN4dsse14gemm_w4_kernel")]
    assert len(ring) >= 3 * 5 * 6 and set(ring) <= set(kinds)  # row tiles x wave counts x epilogue modes
    for k in ring:
        assert preload[k] >= 12, (k, preload[k])
        bad = [v for v in kinds[k] if v.startswith("hidden_block_count") or v.startswith("hidden_group_size")]
        assert not bad, (k, bad)
