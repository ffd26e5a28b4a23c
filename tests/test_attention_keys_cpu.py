"""The codeword attention problems of tests/attn_keys_common.py discriminate: requirements on the INPUTS of
tests/test_attention_keys_gpu.py, checked on the float64 reference alone (no kernel runs here).

For every problem the GPU file launches: the needles hold >= 0.99 of the softmax weight in every column, and every
mutant of the reference (a needle dropped, a needle counted twice, a mask one key too generous or too tight, a key
beyond ctx let in) moves some element of the column by >= 10 x the tolerance the GPU test applies to it.

The last test keeps the reason for these tests on record: on i.i.d. randn inputs, at the suite's tolerance, a
reference that loses or doubles one key is indistinguishable from the right one from 2000 keys up.
"""
import pytest
import torch

import attn_keys_common as A

MIN_WEIGHT, MIN_DISTANCE = 0.99, 10.0
SCALES = [(1.0, 1.0), (0.5, 2.0)]


def _require(mass, dist, sel, what):
    assert sel.any(), f"{what}: no column to check"
    assert mass[sel].min() >= MIN_WEIGHT, f"{what}: needle weight {mass[sel].min():.4f} < {MIN_WEIGHT}"
    assert dist[sel].min() >= MIN_DISTANCE, f"{what}: a mutant is {dist[sel].min():.2f} tolerances away, < {MIN_DISTANCE}"


def _decode_conditions(p, tol_vs=1.0, **cache):
    ref, mass = A.needle_expected(p, **cache)
    two = (p.J != p.JP) & ~p.ghost[:, None]
    for mutant in ("drop", "double"):
        out, _ = A.needle_expected(p, mutant, **cache)
        _require(mass, A.mutant_distance(ref, out, tol_vs), two, f"decode {mutant}")
    out, _ = A.needle_expected(p, "unmask", **cache)
    _require(mass, A.mutant_distance(ref, out, tol_vs), p.ghost[:, None].expand_as(p.J), "decode, a key beyond ctx")
    return ref


@pytest.mark.parametrize("hq,hkv", sorted(set(A.HEADS_DECODE + A.HEADS_GQA)))
def test_decode_sweep_inputs_discriminate(hq, hkv):
    p = A.decode_sweep(hq, hkv)
    # every boundary of every launch configuration is a needle of some column of its context
    for ctx, bl in A.decode_rows():
        have = set(p.J[(p.ctx == ctx) & ~p.ghost].flatten().tolist())
        for kwv in A.KWVS:
            for part, nparts in A.DECODE_PARTS:
                want = A.decode_boundaries(ctx, kwv, part, nparts or -(-max(A.DECODE_CTXS) // part))
                assert set(want) <= have, (ctx, kwv, part, nparts)
    ref = _decode_conditions(p)
    # the reference agrees with the closed form (V[j] + V[j']) / 2 up to the background term
    kv = torch.arange(hq) // (hq // hkv)
    vis = (p.JP < p.ctx[:, None])[..., None]
    vj, vjp = p.V[p.J, kv[None]], p.V[p.JP.clamp(max=p.nkeys - 1), kv[None]]
    assert (ref - (vj + torch.where(vis, vjp, vj)) / 2).abs().max() < 5e-3
    # heads of one GQA group hold different needle pairs
    if hq > hkv:
        g = p.J.view(p.J.shape[0], hkv, hq // hkv)[~p.ghost & (p.ctx > 64)]
        assert (g[..., 0] != g[..., 1]).all()


@pytest.mark.parametrize("hq,hkv", A.HEADS_DECODE)
@pytest.mark.parametrize("ks,vs", SCALES)
def test_decode_sweep_inputs_are_exact_in_fp8(hq, hkv, ks, vs):
    p = A.decode_sweep(hq, hkv)
    k8, v8 = A.to_fp8(p.kc, p.vc, ks, vs)  # asserts exactness
    _decode_conditions(p, vs, kc=k8, vc=v8, ks=ks, vs=vs)


def test_decode_long_context_inputs_discriminate():
    p = A.decode_long()
    assert int(p.ctx.max()) == 4096 and {127, 128, 4095, 4094, 2047, 2048} <= set(p.J.flatten().tolist())
    _decode_conditions(p)


def test_constant_v_expected_is_the_constant():
    p = A.decode_sweep(32, 8)
    kc, vc, q, c = A.const_v_problem(p, 7)
    Kc, Vc = A.cache_keys(p, kc, vc)
    for ctx in A.DECODE_CTXS:
        out, _ = A.attend64(q[:4], Kc, Vc, torch.full((4,), ctx))
        assert (out - c.repeat_interleave(4, 0)[None].double()).abs().max() < 1e-12


def _prefill_conditions(p, tol_vs=1.0, **cache):
    ref, mass = A.prefill_expected(p, "generous", **cache)
    out, _ = A.prefill_expected(p, "generous", "generous", **cache)
    every = torch.ones_like(p.J["generous"], dtype=torch.bool)
    _require(mass, A.mutant_distance(ref, out, tol_vs), every, "causal probe, mask one key too generous")
    ref, mass = A.prefill_expected(p, "tight", **cache)
    out, _ = A.prefill_expected(p, "tight", "tight", **cache)
    _require(mass, A.mutant_distance(ref, out, tol_vs), every & (p.qpos > 0)[:, None], "causal probe, mask one key too tight")
    ref, mass = A.prefill_expected(p, "edges", **cache)
    two = p.J["edges"] != p.JP["edges"]
    for mutant in ("drop", "double"):
        out, _ = A.prefill_expected(p, "edges", mutant, **cache)
        _require(mass, A.mutant_distance(ref, out, tol_vs), two, f"prefill edge needle {mutant}")
    assert mass.min() >= MIN_WEIGHT


@pytest.mark.parametrize("hq,hkv", A.HEADS_PREFILL)
def test_prefill_probe_inputs_discriminate(hq, hkv):
    p = A.prefill_sweep(hq, hkv)
    assert [(int(c), int(q)) for c, q in zip(p.ctx, p.qlen)] == list(A.PREFILL_CASES)
    _prefill_conditions(p)
    # every 64-key block edge below a long chunk's rows is some column's needle
    have = set(p.J["edges"].flatten().tolist())
    assert {64 * t - 1 for t in range(1, 20)} | {64 * t for t in range(1, 20)} <= have


@pytest.mark.parametrize("ks,vs", SCALES)
def test_prefill_probe_inputs_are_exact_in_fp8(ks, vs):
    p = A.prefill_sweep(4, 1)
    k8, v8 = A.to_fp8(p.kc, p.vc, ks, vs)
    _prefill_conditions(p, vs, kc=k8, vc=v8, ks=ks, vs=vs)


@pytest.mark.parametrize("i", range(len(A.SPLIT_CASES)))
def test_flash_split_inputs_discriminate(i):
    p, tiles, (work, comb, nslots) = A.split_sweep(i)
    assert len(comb) > 0
    _prefill_conditions(p)
    nw = work.size // 5
    have = {b: set(p.J["edges"][sum(q for _, q in p.cases[:b]): sum(q for _, q in p.cases[:b + 1])].flatten().tolist())
            for b in range(len(p.cases))}
    for k in range(nw):
        b, t = int(work[k]), int(work[nw + k])
        first_q = int(p.ctx[b] - p.qlen[b]) + 64 * t
        for kb in work[2 * nw + 2 * k: 2 * nw + 2 * k + 2].tolist():
            for e in (64 * kb - 1, 64 * kb):
                if 0 <= e < first_q:  # visible to the tile's rows
                    assert e in have[b], (b, t, kb, e)


@pytest.mark.parametrize("hq,hkv", A.HEADS_FOLDED)
def test_folded_decode_inputs_discriminate(hq, hkv):
    p = A.folded_sweep(hq, hkv)
    assert p.M > 17, "the folded path needs more than 16 rows to run under the default GEMM dispatch"
    live = p.ctx[:-1]
    # the newest key opens a page, follows its first key, closes a page: first page, a middle page, a partition's first
    assert {(int(c) - 1) % 32 for c in live} >= {0, 1, 31}
    assert {1, 2, 32, 65, 66, 96, 129, 130, 160} <= set(live.tolist())
    for c in set(live.tolist()):
        have = set(p.J[live == c].flatten().tolist())
        assert {c - 1, max(c - 2, 0)} <= have and set(A.folded_boundaries(c)) <= have
    ref, mass = A.folded_expected(p)
    two = p.J != p.JP
    for mutant in ("drop", "double"):
        out, _ = A.folded_expected(p, mutant)
        _require(mass, A.mutant_distance(ref, out), two, f"folded {mutant}")
        _require(mass, A.mutant_distance(ref, out, 2.0), two, f"folded {mutant}, v_scale 2")
    assert mass.min() >= MIN_WEIGHT
    # the GEMM reproduces the wanted rows exactly: q = the needle sums, k / v = the codewords of key ctx - 1
    from distributed_sse_for_llm_response_amd.ops import reference as R

    q = torch.zeros(p.M, hq * 128, dtype=torch.bfloat16)
    kc, vc = p.kc.clone(), p.vc.clone()
    R.gemm_qkv_rope(p.x, p.w, p.pos, p.slots, p.rope, q, kc, vc, hq, hkv)
    assert torch.equal(q.view(p.M, hq, 128)[:-1], p.q) and torch.equal(kc, p.full_kc) and torch.equal(vc, p.full_vc)
    assert not torch.equal(p.kc, p.full_kc)
    for ks, vs in SCALES:
        A.to_fp8(p.full_kc, p.full_vc, ks, vs)


def test_random_inputs_cannot_see_one_key():
    """The blind spot on record: 32 randn queries over ctx randn keys (4096 output elements), the float64 reference
    against itself with one key dropped or counted twice, at the suite's tolerance 1e-2 + 2e-2 |ref|."""
    def off(ctx, weight_of):
        g = torch.Generator().manual_seed(ctx)
        Q, K, V = (torch.randn(n, 1, 128, generator=g) for n in (32, ctx, ctx))
        lim = torch.full((32,), ctx)
        ref, _ = A.attend64(Q, K, V, lim)
        w = torch.ones(32, 1, ctx, dtype=torch.float64)
        weight_of(w)
        out, _ = A.attend64(Q, K, V, lim, w)
        return int(((out - ref).abs() > A.tolerance(ref)).sum()), float(ref.std())

    def drop(w):
        w[..., 128] = 0

    def double(w):
        w[..., 128] = 2

    def page(w):
        w[..., 128:160] = 0

    for ctx in (2000, 4096):
        assert off(ctx, drop)[0] == 0 and off(ctx, double)[0] == 0
        assert off(ctx, drop)[1] < 0.05  # the output's std shrinks like 1 / sqrt(ctx); the tolerance does not
    assert off(4096, page)[0] == 0, "at 4096 keys even a lost page passes"
    assert off(300, drop)[0] > 0 and off(300, page)[0] > 1000  # short contexts do see it
