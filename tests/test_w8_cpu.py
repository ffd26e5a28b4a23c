"""FP8 (e4m3) weights on the CPU: the quantiser and its error bound, the byte layout and its inverse, the reference ops
(equal to the bf16 reference ops on the widened weights), the CPU engine under quantization="fp8" and the option's
parsing (--quantization / QUANTIZATION)."""
import argparse
import math

import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
from distributed_sse_for_llm_response_amd.engine.weights import (convert_standard, parse_quantization,
                                                                 quantize_engine_weights)
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as R
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig

FP8 = torch.float8_e4m3fn


def _is_pow2(s: torch.Tensor) -> torch.Tensor:
    m, _ = torch.frexp(s)
    return m == 0.5


# ---------------------------------------------------------------- quantiser
@pytest.mark.parametrize("std", [1.0 / 32.0, None])  # N(0, 1/32) and N(0, 1/sqrt(K))
def test_quantiser_scales_and_error_bound(std):
    N, K = 256, 1536
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(N, K, generator=g) * (std or 1.0 / math.sqrt(K))).bfloat16()
    q, s = R.quantize_weight_f8(w)
    assert q.dtype == FP8 and q.shape == (N, K) and s.dtype == torch.float32 and s.shape == (N,)
    assert bool(_is_pow2(s).all())
    wf = w.float()
    amax = wf.abs().amax(1)
    assert bool((amax / s <= 448.0).all())            # no saturation
    assert bool((amax / (s * 0.5) > 448.0).all())     # and the smallest such power of two
    wide = R.widen_weight_f8(q, s)
    assert wide.dtype == torch.bfloat16
    # half an ulp of a 3-bit mantissa for normals, half the subnormal step 2^-9 s below 2^-6 s
    err = (wide.float() - wf).abs()
    assert bool((err <= 2.0 ** -4 * wf.abs() + 2.0 ** -10 * s[:, None]).all())
    # widening is exact in bf16: nothing is lost when the bytes become the bf16 copy
    assert torch.equal(wide.float(), q.float() * s[:, None])
    assert torch.equal(wide.float(), q.float().bfloat16().float() * s[:, None])


def test_quantiser_zero_row_and_single_extreme_value():
    w = torch.zeros(16, 128)
    w[1, 5] = 448.0 * 2.0 ** -7      # exactly 448 * 2^e: the scale is 2^e, the byte is +-448
    w[2, 9] = -448.0 * 2.0 ** 3
    w[3, 0] = 450.0                  # the next bf16 above 448: the next power of two
    q, s = R.quantize_weight_f8(w.bfloat16())
    assert s[0] == 1.0 and not q[0].view(torch.uint8).any()
    assert s[1] == 2.0 ** -7 and float(q[1, 5].float()) == 448.0
    assert s[2] == 2.0 ** 3 and float(q[2, 9].float()) == -448.0
    assert s[3] == 2.0
    wide = R.widen_weight_f8(q, s).float()
    assert torch.equal(wide[:3], w[:3]) and not torch.isnan(wide).any()


# ---------------------------------------------------------------- layout
@pytest.mark.parametrize("N", [16, 48, 512])
@pytest.mark.parametrize("K", [128, 384, 1536])
def test_byte_layout_round_trip(N, K):
    # every byte position distinct: three byte planes of the linear index
    idx = torch.arange(N * K).view(N, K)
    planes = [((idx >> (8 * p)) & 255).to(torch.uint8) for p in range(3)]
    tiled = [R.tile_weight_f8(p) for p in planes]
    assert all(t.shape == (N, K) and t.dtype == torch.uint8 for t in tiled)
    for p, t in zip(planes, tiled):
        assert torch.equal(R.untile_weight_f8(t), p)
    pos = sum(t.to(torch.int64) << (8 * i) for i, t in enumerate(tiled)).view(-1)
    assert torch.equal(pos.sort().values, torch.arange(N * K))  # a permutation of the positions
    # the documented order: block (T, c), then [h][lane = r + 16 g][b] = W[16T + r][128c + 32g + 16h + b]
    T, c, h, lane, b = (N // 16 - 1, K // 128 - 1, 1, 37, 11)
    r, g = lane & 15, lane >> 4
    off = ((T * (K // 128) + c) * 2 + h) * 1024 + lane * 16 + b
    assert int(pos[off]) == (16 * T + r) * K + 128 * c + 32 * g + 16 * h + b
    # float8 tensors go through the same permutation
    q = planes[0].view(FP8)
    assert torch.equal(R.tile_weight_f8(q).view(torch.uint8), tiled[0])


# ---------------------------------------------------------------- reference ops
def test_reference_ops_equal_the_bf16_ops_on_the_widened_weight():
    g = torch.Generator().manual_seed(5)
    M, K, nh, nkv = 5, 256, 2, 1
    x = torch.randn(M, K, generator=g).bfloat16()

    def quant(N):
        q, s = R.quantize_weight_f8((torch.randn(N, K, generator=g) / 16).bfloat16())
        return R.tile_weight_f8(q), s, R.tile_weight(R.widen_weight_f8(q, s))

    wq, ws, wt = quant(64)
    for dt in (torch.bfloat16, torch.float32):
        a, b = torch.zeros(M, 64, dtype=dt), torch.zeros(M, 64, dtype=dt)
        ops.gemm_out_w8(x, wq, ws, a)
        ops.gemm_out(x, wt, b)
        assert torch.equal(a, b) and a.abs().sum() > 0
    a, b = torch.ones(M, 64), torch.ones(M, 64)
    part = torch.zeros(8 * M * 64)
    assert ops.gemm_resid_split_w8(x, wq, ws, a, part) == 0 and ops.gemm_resid_split(x, wt, b, part) == 0
    ops.gemm_resid_w8(x, wq, ws, a)
    ops.gemm_resid(x, wt, b)
    assert torch.equal(a, b)
    a, b = torch.zeros(M, 32, dtype=torch.bfloat16), torch.zeros(M, 32, dtype=torch.bfloat16)
    ops.gemm_silu_w8(x, wq, ws, a)
    ops.gemm_silu(x, wt, b)
    assert torch.equal(a, b)
    a, b = torch.zeros(M, 64, dtype=torch.bfloat16), torch.zeros(M, 64, dtype=torch.bfloat16)
    assert ops.gemm_out_split_w8(x, wq, ws, a, part) == 0 and ops.gemm_out_split(x, wt, b, part) == 0
    assert torch.equal(a, b)

    wq, ws, wt = quant((nh + 2 * nkv) * 128)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    pos, slots = i32(3, 4, 5, 6, 7), i32(3, 4, 5, 6, 7)
    rope = R.rope_table(64, 10000.0)
    bt = torch.zeros(M, 2, dtype=torch.int32)
    outs = []
    for w8 in (True, False):
        kc = torch.zeros(2, nkv, 32, 128, dtype=torch.bfloat16)
        vc = torch.zeros(2, nkv, 128, 32, dtype=torch.bfloat16)
        qo = torch.zeros(M, nh * 128, dtype=torch.bfloat16)
        o = torch.zeros(M, nh * 128, dtype=torch.bfloat16)
        meta = (bt, torch.arange(M, dtype=torch.int32), torch.ones(M, dtype=torch.int32), pos + 1,
                torch.arange(M, dtype=torch.int32), torch.zeros(M, dtype=torch.int32))
        if w8:
            ops.qkv_attention_decode_w8(x, wq, ws, pos, slots, rope, qo, kc, vc, nh, nkv, part, *meta, o, part, part,
                                        32, 1)
        else:
            ops.qkv_attention_decode(x, wt, pos, slots, rope, qo, kc, vc, nh, nkv, part, *meta, o, part, part, 32, 1)
        outs.append((qo, kc, vc, o))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][1].abs().sum() > 0 and outs[0][3].abs().sum() > 0


# ---------------------------------------------------------------- CPU engine
_STD = {}


def _engine(seed, quantization):
    if seed not in _STD:
        _STD[seed] = init_standard_weights(TINY, seed=seed)
    w = convert_standard(TINY, _STD[seed], quantization=quantization)
    r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device="cpu", use_graphs=False)
    return LLMEngine(r, eos_id=-1, prefill_budget=256)


def _greedy(e, prompt, n):
    e.add_request("c", prompt, SamplingParams(temperature=0.0, max_tokens=n))
    toks = []
    for _ in range(4000):
        toks += [ev.token_id for ev in e.step() if ev.token_id >= 0 and not ev.done]
        if not e.has_work():
            break
    assert not e.has_work()
    return toks[:n]


def _prompt(i, n=24):
    g = torch.Generator().manual_seed(700 + i)
    return torch.randint(3, TINY.vocab_size, (n,), generator=g).tolist()


SEEDS = (11, 12, 13, 14)


def test_engine_decode_and_fresh_prefill_agree_and_differ_from_bf16():
    differs = 0
    for seed in SEEDS:
        e = _engine(seed, "fp8")
        assert e.quantization == "fp8_e4m3" and e.r.w.lm_head_q.dtype == FP8 and e.r.w.layers[0].wd_scale is not None
        p = _prompt(seed)
        toks = _greedy(e, p, 10)  # token 1 from the prefill (widened copy), 2.. from decode steps (the FP8 ops)
        assert len(toks) == 10
        for k in (4, 9):  # the same continuation recomputed by a fresh prefill of the longer prompt
            again = _greedy(_engine(seed, "fp8"), p + toks[:k], 1)
            assert again == toks[k:k + 1], (seed, k)
        bf = _engine(seed, None)
        assert bf.quantization == "none" and bf.r.w.lm_head_q is None
        differs += _greedy(bf, p, 10) != toks
    assert differs >= 1  # the option changes the weights


def test_runner_quantises_weights_loaded_without_the_option():
    w = convert_standard(TINY, init_standard_weights(TINY, seed=11))
    ref = convert_standard(TINY, init_standard_weights(TINY, seed=11), quantization="fp8")
    n0 = w.nbytes()
    r = ModelRunner(w, num_blocks=8, max_batch=2, max_model_len=128, device="cpu", use_graphs=False,
                    quantization="fp8")
    assert r.quantization == "fp8_e4m3" and r.w8
    for a, b in zip(w.layers, ref.layers):
        for f in ("wqkv", "wo", "wgu", "wd"):
            assert torch.equal(getattr(a, f + "_q").view(torch.uint8), getattr(b, f + "_q").view(torch.uint8))
            assert torch.equal(getattr(a, f + "_scale"), getattr(b, f + "_scale"))
            assert torch.equal(getattr(a, f + "_t"), getattr(b, f + "_t"))
    assert torch.equal(w.lm_head_t, ref.lm_head_t)
    # both copies are counted: the FP8 one is half the matrices' bf16 bytes plus the scales
    mats = sum(t.numel() for L in w.layers for t in (L.wqkv_t, L.wo_t, L.wgu_t, L.wd_t)) + w.lm_head_t.numel()
    rows = sum(t.numel() for L in w.layers for t in (L.wqkv_scale, L.wo_scale, L.wgu_scale, L.wd_scale))
    assert w.nbytes_fp8() == mats + 4 * (rows + w.lm_head_scale.numel()) and w.nbytes() == n0 + w.nbytes_fp8()
    assert quantize_engine_weights(w, "fp8") is w  # idempotent
    # the embedding and the norms are left alone
    assert torch.equal(w.embed, ref.embed) and w.embed.dtype == torch.bfloat16


# ---------------------------------------------------------------- option parsing
def test_config_cli_environment_json_and_tp_refusal(monkeypatch, capsys):
    monkeypatch.delenv("QUANTIZATION", raising=False)
    assert ServeConfig().quantization == "none" and ServeConfig.from_env().quantization == "none"
    monkeypatch.setenv("QUANTIZATION", "FP8")
    assert ServeConfig.from_env().quantization == "fp8"
    ap = argparse.ArgumentParser()
    ServeConfig.add_args(ap)
    monkeypatch.delenv("QUANTIZATION")
    cfg = ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "fp8"]))
    assert cfg.quantization == "fp8"
    assert ServeConfig.from_json(cfg.to_json()).quantization == "fp8"  # what every DP replica gets
    assert ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "none"])).quantization == "none"
    assert ServeConfig.from_env().update_from_args(ap.parse_args([])).quantization == "none"
    with pytest.raises(SystemExit):  # argparse: a usage error that lists the choices
        ap.parse_args(["--quantization", "int4"])
    assert "'none', 'fp8'" in capsys.readouterr().err
    with pytest.raises(ValueError, match="none, fp8"):
        ServeConfig.from_env().update_from_args(argparse.Namespace(quantization="int4"))
    monkeypatch.setenv("QUANTIZATION", "awq")
    with pytest.raises(ValueError, match="none, fp8"):
        ServeConfig.from_env()
    monkeypatch.delenv("QUANTIZATION")
    # --dp and an fp8 KV cache combine with it; --tp > 1 is refused at start-up
    ok = ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "fp8", "--dp", "2",
                                                                "--kv-cache-dtype", "fp8"]))
    assert ok.quantization == "fp8" and ok.dp == 2
    with pytest.raises(ValueError, match="not supported with tensor parallelism"):
        ServeConfig.from_env().update_from_args(ap.parse_args(["--quantization", "fp8", "--tp", "2"]))
    with pytest.raises(ValueError, match="tensor parallelism"):
        convert_standard(TINY, init_standard_weights(TINY, seed=1), tp_rank=0, tp_size=2, quantization="fp8")
    w = convert_standard(TINY, init_standard_weights(TINY, seed=1), tp_rank=0, tp_size=2)
    with pytest.raises(ValueError, match="tensor parallelism"):
        ModelRunner(w, num_blocks=8, max_batch=2, max_model_len=128, device="cpu", use_graphs=False,
                    comm=TPComm(rank=0, size=2), quantization="fp8")
    assert parse_quantization(None) == "none" and parse_quantization("fp8_e4m3") == "fp8"
    with pytest.raises(ValueError, match="none, fp8"):
        parse_quantization("int8")


def test_bench_harness_takes_the_option_from_the_environment(monkeypatch):
    from distributed_sse_for_llm_response_amd.engine import bench_harness

    monkeypatch.setenv("QUANTIZATION", "fp8")
    _, r = bench_harness._build_runner("mistral-tiny", torch.device("cpu"), 2, 16, 4, 1, False, 0, 1)
    assert r.quantization == "fp8_e4m3" and r.w.layers[0].wqkv_q is not None
    monkeypatch.delenv("QUANTIZATION")
    _, r = bench_harness._build_runner("mistral-tiny", torch.device("cpu"), 2, 16, 4, 1, False, 0, 1)
    assert r.quantization == "none" and r.w.layers[0].wqkv_q is None and r.w.nbytes_fp8() == 0
