"""Multi-LoRA on the GPU: lora_shrink / lora_expand_add (csrc/kernels/lora.hip) against float64 at the Mistral
shapes, their bit-exact independence of the rest of the batch, and the runner's LoRA layer body (eager and in graph
twins) against the fp32 reference model with the adapter merged.

Tolerances: the kernel outputs at the ones tests/test_kernels_gpu.py test_gemm_out_bf16_f32 uses (fp32 out: atol 1e-3,
rtol 1e-2; bf16 out: atol 2e-2, rtol 1e-2), the runner at tests/test_model_runner.py's GPU bound (0.1)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from lora_common import write_adapter
from test_lora_cpu import CFG, SEED, reference_gaps, run_runner

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.lora import (LoraAdapter, LoraPool, load_adapter, merge_into_standard,
                                                              module_shapes)
from distributed_sse_for_llm_response_amd.engine.weights import _permute_units, convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import init_standard_weights
from distributed_sse_for_llm_response_amd.ops.reference import gate_up_perm

pytestmark = pytest.mark.gpu


def test_new_ops_are_registered(gpu):
    ops.load_library(required=True)
    assert hasattr(torch.ops.dsse, "lora_shrink") and hasattr(torch.ops.dsse, "lora_expand_add")
    assert "lora.hip" in torch.ops.dsse.kernel_check_files().split(",")


# ---------------------------------------------------------------- one-hot: slot, row, slice map, permutation
@pytest.mark.parametrize("p,module", [("qkv", "q_proj"), ("qkv", "k_proj"), ("qkv", "v_proj"), ("gu", "gate_proj"),
                                      ("gu", "up_proj")])
def test_one_hot_delta_lands_in_one_element(gpu, p, module):
    """A selects input column 37, B writes checkpoint row 203 of `module`; x[2, 37] = 3 and scale = 0.5, so the delta
    is exactly 1.5, in row 2 and the engine column that holds that checkpoint row, and zero everywhere else."""
    sh = module_shapes(CFG)
    out_f, in_f = sh[module]
    A = torch.zeros(4, in_f, dtype=torch.bfloat16)
    B = torch.zeros(out_f, 4, dtype=torch.bfloat16)
    A[1, 37], B[203, 1] = 1.0, 1.0
    ad = LoraAdapter("hot", "hot", 4, 0.5, [{module: (A, B)} for _ in range(CFG.num_layers)])
    pool = LoraPool(CFG, 3, 8, device=gpu)
    pool.load(2, ad)
    mods = {"qkv": ("q_proj", "k_proj", "v_proj"), "gu": ("gate_proj", "up_proj")}[p]
    hf_row = sum(sh[m][0] for m in mods[:mods.index(module)]) + 203
    N = sum(sh[m][0] for m in mods)
    if p == "qkv":
        src = _permute_units(torch.arange(N, dtype=torch.float32)[:, None]).flatten().long()
    else:
        src = gate_up_perm(N // 2)
    col = int((src == hf_row).nonzero())
    x = torch.zeros(5, in_f, dtype=torch.bfloat16, device=gpu)
    x[2, 37], x[3, 37] = 3.0, 3.0
    ra = torch.tensor([2, 2, 2, 1, -1], dtype=torch.int32, device=gpu)  # row 3 names an empty slot: zero delta
    for dt in (torch.float32, torch.bfloat16):
        t = torch.full((5, pool.A[p].shape[2]), 7.0, device=gpu)
        out = torch.zeros(5, N, device=gpu, dtype=dt)
        ops.lora_shrink(x, pool.A[p][0], ra, t)
        ops.lora_expand_add(t, pool.B[p][0], pool.scale, ra, pool.slice_of_row[p], out)
        want = torch.zeros(5, N)
        want[2, col] = 1.5
        assert torch.equal(out.float().cpu(), want), (p, module, dt, out.float().cpu().nonzero().tolist())


# ---------------------------------------------------------------- against float64 at the Mistral shapes
def _case(K, N, S, R, r, slots, gen, dev):
    A = torch.zeros(slots, S * R, K)
    B = torch.zeros(slots, N, R)
    for s in range(S):  # rank r < R: the padding rows / columns stay zero
        A[:, s * R:s * R + r] = torch.randn(slots, r, K, generator=gen) / math.sqrt(K)
    B[:, :, :r] = torch.randn(slots, N, r, generator=gen) / math.sqrt(r)
    sl = (torch.arange(N) // 8 % S).int() if S == 2 else (torch.arange(N) * S // N).int()
    scale = torch.tensor([2.0, 0.5, 1.25][:slots])
    return A.bfloat16().to(dev), B.bfloat16().to(dev), sl.to(dev), scale.to(dev)


def _ref64(x, A, B, sl, scale, ra, out0):
    R = B.shape[2]
    out = out0.double().cpu().clone()
    x, A, B, sl, ra = x.double().cpu(), A.double().cpu(), B.double().cpu(), sl.long().cpu(), ra.long().cpu()
    for a in sorted(set(ra.tolist()) - {-1}):
        rows = (ra == a).nonzero().flatten()
        t = x[rows] @ A[a].t()
        d = torch.zeros(len(rows), B.shape[1], dtype=torch.float64)
        for s in range(int(sl.max()) + 1):
            cols = (sl == s).nonzero().flatten()
            d[:, cols] = t[:, s * R:(s + 1) * R] @ B[a][cols].t()
        out[rows] += float(scale[a]) * d
    return out


def _close(a, b, atol, rtol, what):
    err = (a.double().cpu() - b).abs()
    bad = int((err > atol + rtol * b.abs()).sum())
    assert bad == 0, f"{what}: {bad} / {a.numel()} elements off; max err {float(err.max()):.4g}"


@pytest.mark.parametrize("K,N,S", [(4096, 6144, 3), (4096, 4096, 1), (4096, 28672, 2), (14336, 4096, 1)])
def test_products_against_float64_at_mistral_shapes(gpu, K, N, S):
    g = torch.Generator().manual_seed(K + N)
    for R, r in ((8, 4), (16, 16), (64, 40)):
        A, B, sl, scale = _case(K, N, S, R, r, 3, g, gpu)
        for M in (1, 16, 17, 64, 65, 300):
            x = torch.randn(M, K, generator=g).bfloat16().to(gpu)
            ra = (torch.arange(M) % 4 - 1).int().to(gpu)  # -1, 0, 1, 2, ...
            for dt, atol in ((torch.float32, 1e-3), (torch.bfloat16, 2e-2)):
                out0 = torch.randn(M, N, generator=g).to(dt).to(gpu)
                out = out0.clone()
                t = torch.empty(M, S * R, device=gpu)
                ops.lora_shrink(x, A, ra, t)
                ops.lora_expand_add(t, B, scale, ra, sl, out)
                _close(out, _ref64(x, A, B, sl, scale, ra, out0), atol, 1e-2, f"K {K} N {N} R {R} M {M} {dt}")


# ---------------------------------------------------------------- adapter -1 and batch independence
def _apply(x, A, B, sl, scale, ra, out0):
    out = out0.clone()
    t = torch.empty(x.shape[0], A.shape[1], device=x.device)
    ops.lora_shrink(x, A, ra, t)
    ops.lora_expand_add(t, B, scale, ra, sl, out)
    return out, t


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rows_without_adapter_keep_their_bits_and_rows_do_not_see_each_other(gpu, dt):
    g = torch.Generator().manual_seed(3)
    K, N, S, R, M = 1024, 1536, 3, 16, 21
    A, B, sl, scale = _case(K, N, S, R, 16, 2, g, gpu)
    x = torch.randn(M, K, generator=g).bfloat16().to(gpu)
    out0 = torch.randn(M, N, generator=g).to(dt).to(gpu)
    ra = torch.tensor(([0, -1, 1, 1, -1, 0] * 4)[:M], dtype=torch.int32, device=gpu)
    out, t = _apply(x, A, B, sl, scale, ra, out0)
    none = ra.cpu() < 0
    assert torch.equal(out.cpu()[none], out0.cpu()[none]) and not t.cpu()[none].any()
    for a in (0, 1):  # every row bit-equal to the same row in a batch where all rows use that adapter
        solo, _ = _apply(x, A, B, sl, scale, torch.full((M,), a, dtype=torch.int32, device=gpu), out0)
        rows = ra.cpu() == a
        assert torch.equal(out.cpu()[rows], solo.cpu()[rows])
        assert not torch.equal(solo.cpu()[rows], out0.cpu()[rows])


def test_prompt_chunk_runs_with_unaligned_boundaries(gpu):
    """300 prompt rows of three sequences under adapters 0 / -1 / 1; the runs end at rows 101 and 187."""
    g = torch.Generator().manual_seed(4)
    K, N, S, R, M = 1024, 2 * 2816, 2, 8, 300
    A, B, sl, scale = _case(K, N, S, R, 8, 2, g, gpu)
    x = torch.randn(M, K, generator=g).bfloat16().to(gpu)
    out0 = torch.randn(M, N, generator=g).bfloat16().to(gpu)
    ra = torch.cat([torch.zeros(101), -torch.ones(86), torch.ones(113)]).int().to(gpu)
    out, _ = _apply(x, A, B, sl, scale, ra, out0)
    _close(out, _ref64(x, A, B, sl, scale, ra, out0), 2e-2, 1e-2, "runs")
    assert torch.equal(out[101:187].cpu(), out0[101:187].cpu())
    for a, rows in ((0, slice(0, 101)), (1, slice(187, 300))):
        solo, _ = _apply(x, A, B, sl, scale, torch.full((M,), a, dtype=torch.int32, device=gpu), out0)
        assert torch.equal(out[rows].cpu(), solo[rows].cpu())


# ---------------------------------------------------------------- runner
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapters")
    std = init_standard_weights(CFG, seed=SEED)
    a = load_adapter(write_adapter(d / "a", CFG, 60, r=4), CFG, 8, name="a")
    return std, a, merge_into_standard(std, a)


def _pool(a, dev):
    pool = LoraPool(CFG, 2, 8, device=dev)
    pool.load(1, a)
    return pool


@pytest.mark.parametrize("kv", ["auto", "fp8"])
def test_runner_with_adapter_matches_merged_reference(gpu, model, kv):
    """Eager and graph-replayed; bf16 and FP8 KV cache (tests/test_kv_fp8_gpu.py holds its runner to 0.1 as well)."""
    std, a, merged = model
    w = convert_standard(CFG, std, device=gpu)
    _, eager = run_runner(w, gpu, _pool(a, gpu), adapters=(1, 1, 1), kv=kv)
    r, graph = run_runner(w, gpu, _pool(a, gpu), adapters=(1, 1, 1), graphs=True, kv=kv)
    worst, _ = reference_gaps(merged, eager)
    print(f"kv {kv}: worst {worst:.4f}")
    assert worst < 0.1
    assert graph == eager
    key = (False, False, False, False, True)
    assert r._twin_key() == key and r._graph_set()[0] is r._twins[key][0] and set(r._twins[key][0]) == set(r.graphs)
    assert set(r._twins[key][1]) == set(r.pf_graphs)


def test_start_up_graphs_replay_until_the_first_adapter_request(gpu, model):
    std, a, _ = model
    w = convert_standard(CFG, std, device=gpu)
    r0, plain = run_runner(w, gpu, None, graphs=True)
    r1, base = run_runner(w, gpu, _pool(a, gpu), graphs=True, enable=False)
    assert not r1.lora_used and r1._graph_set()[0] is r1.graphs and not any(any(t) for t in r1._twins.values())
    assert base == plain  # a pool that no request has named changes nothing
    # after the first adapter request base rows ride in the LoRA body with adapter -1: the same tokens as that body
    # with no adapter anywhere (not the fused body, whose summation order differs)
    _, mixed = run_runner(w, gpu, _pool(a, gpu), adapters=(-1, 1, -1), graphs=True)
    _, none = run_runner(w, gpu, _pool(a, gpu), adapters=(-1, -1, -1), graphs=True)
    assert mixed[0] == none[0] and mixed[2] == none[2] and mixed[1] != none[1]
    worst, _ = reference_gaps(std, [none[0], none[1], none[2]])
    assert worst < 0.1


def test_checked_build_is_clean_over_the_lora_ops(gpu):
    from distributed_sse_for_llm_response_amd import _build

    _build.build_kernels(variant="checked")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_kernels.py"), "--only", "lora"],
                       capture_output=True, text=True, timeout=300,
                       env={**os.environ, "DSSE_KERNELS_VARIANT": "checked", "DSSE_KERNEL_CFG": ""})
    assert r.returncode == 0 and "CHECKS-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _worst(std, prompt, gen):
    from distributed_sse_for_llm_response_amd.models.mistral import reference_forward

    logits, _ = reference_forward(CFG, std, torch.tensor(prompt + gen))
    return max(float(logits[len(prompt) - 1 + j].max() - logits[len(prompt) - 1 + j][g]) for j, g in enumerate(gen))


def test_mixed_step_twin_replays_and_matches_eager(gpu, model):
    """A prompt under the adapter rides in a mixed step beside two decoding slots (adapter / base): the captured LoRA
    twin of the mixed graph gives the eager body's tokens, and both follow the merged / base reference."""
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq

    std, a, merged = model
    w = convert_standard(CFG, std, device=gpu)
    prompts = [[5, 17, 99, 3, 8, 1000, 42], [7] * 33, list(range(100, 170))]
    bts = [[0, 1, 2], [20, 21, 22], [10, 4, 5, 6]]
    adapters = (1, -1, 1)
    out = {}
    for graphs in (False, True):
        r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs,
                        lora=_pool(a, gpu))
        for i, bt in enumerate(bts):
            r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
        if graphs:
            r.capture([4])
        r.slot_adapter[:3] = torch.tensor(adapters, dtype=torch.int32)
        r.enable_lora()
        r.prefill([PrefillSeq(i, prompts[i], 0, bts[i], True, adapter=adapters[i]) for i in (0, 1)], ring_row=0)
        r.active[:2] = 1
        gen = [[int(r.ids[0])], [int(r.ids[1])], []]
        if graphs:
            assert r.mixed_graph_rows(4, len(prompts[2])) is not None and r._graph_set()[2] is not r.mx_graphs
        r.mixed(4, [PrefillSeq(2, prompts[2], 0, bts[2], True, adapter=1)], ring_row=int(r.ring_counter[0]))
        r.active[2] = 1
        ids = r.ids.cpu()
        for i in range(3):
            gen[i].append(int(ids[i]))
        for _ in range(3):
            r.decode(4)
            ids = r.ids.cpu()
            for i in range(3):
                gen[i].append(int(ids[i]))
        out[graphs] = gen
    assert out[True] == out[False]
    for i, ref in enumerate((merged, std, merged)):
        assert _worst(ref, prompts[i], out[False][i]) < 0.1, i


def test_wide_decode_bucket_under_the_lora_body(gpu, model):
    """192 decode rows (above the 128-row split of the fused step), adapters alternating with base rows: the LoRA
    body serves every bucket, and the LM head runs in its 256-row blocks."""
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq

    std, a, merged = model
    w = convert_standard(CFG, std, device=gpu)
    B = 192
    r = ModelRunner(w, num_blocks=B + 8, max_batch=B, max_model_len=64, device=gpu, use_graphs=False,
                    lora=_pool(a, gpu))
    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(3, CFG.vocab_size, (5 + i % 7,), generator=g).tolist() for i in range(B)]
    adapters = [1 if i % 2 else -1 for i in range(B)]
    r.block_tables[:, 0] = torch.arange(B, dtype=torch.int32)
    r.slot_adapter.copy_(torch.tensor(adapters, dtype=torch.int32))
    r.enable_lora()
    for i0 in range(0, B, 16):
        r.prefill([PrefillSeq(i, prompts[i], 0, [i], True, adapter=adapters[i]) for i in range(i0, i0 + 16)], ring_row=0)
    r.active.fill_(1)
    gen = [[t] for t in r.ids.cpu().tolist()]
    for _ in range(2):
        r.decode(B)
        for i, t in enumerate(r.ids.cpu().tolist()):
            gen[i].append(t)
    for i in (0, 1, 2, 127, 128, 129, 190, 191):
        assert _worst(merged if adapters[i] >= 0 else std, prompts[i], gen[i]) < 0.1, i
