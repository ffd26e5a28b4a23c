"""Key accounting of every attention kernel on gfx950: the codeword problems of tests/attn_keys_common.py (every key
matters: a dropped needle moves output elements by 1, a doubled one by 1/3, an unmasked one by 1/2) against their
float64 expected values at the suite's tolerance 1e-2 + 2e-2 |ref| (fp8: the absolute term times v_scale).
tests/test_attention_keys_cpu.py proves on the reference alone that these inputs discriminate.

Needles sit on every page, key-split-stride, partition, key-block and key-range edge of the launch configuration, on
the causal diagonal and just beyond ctx; the constant-V variant (V[k, d] = c_d) shows any disagreement between the
accumulated O and the accumulated l at every context.  The sweeps reach the instantiations the random-input tests
never run: the 2-page register ring (attn_pd=2), mode 0 with 1, 2 and 8 key-split waves, mode 0 at GQA groups 1, 2, 8
and 16, the folded decode at groups 1 and 2.
"""
import math

import pytest
import torch

import attn_keys_common as A
from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.ops import reference as R

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
SCALES = [(1.0, 1.0), (0.5, 2.0)]
KWV_PD = [(kwv, pd) for kwv in A.KWVS for pd in (1, 2)]
FOLDED_KWV_PD = [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (8, 1)]
SENTINEL = 7.0  # rows no kernel may write


@pytest.fixture(autouse=True)
def _fresh_kernel_env():
    ops.refresh_env()
    yield
    ops.refresh_env()


def _cfg(monkeypatch, **kw):
    monkeypatch.setenv("DSSE_KERNEL_CFG", ops.kernel_cfg_env(**{k: str(v) for k, v in kw.items()}))
    ops.refresh_env()


def _close(a, b, atol, rtol, what=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{what}: {bad} / {a.numel()} elements off; max err {err.max().item():.4g}"


_dev = {}


def _on(gpu, key, build):
    """Device copies and expected values of a problem, made once per module."""
    if key not in _dev:
        _dev[key] = build()
    return _dev[key]


# ------------------------------------------------------------------------------------------------ decode, mode 0
def _decode_state(gpu, p, key, ks=1.0, vs=1.0, fp8=False):
    """The needle sweep plus one inactive row, and the constant-V variant over the same block tables."""
    def build():
        B = p.q.shape[0] + 1
        kc, vc = A.to_fp8(p.kc, p.vc, ks, vs) if fp8 else (p.kc, p.vc)
        want, _ = A.needle_expected(p, kc=kc, vc=vc, ks=ks, vs=vs)
        ckc, cvc, cq, c = A.const_v_problem(p, 7)
        if fp8:  # V = c_d is exact in e4m3 at both scale pairs (asserted); K is randn: whatever it rounds to, O = c_d
            cvc_bf16 = cvc
            ckc, cvc = R.quantize_kv(ckc.float(), ks), R.quantize_kv(cvc.float(), vs)
            assert torch.equal(R.dequantize_kv(cvc, vs), cvc_bf16.float())
        G = p.hq // p.hkv
        qlen = torch.ones(B, dtype=torch.int32)
        qlen[-1] = 0  # an inactive row (it keeps a context and a query: neither may be used)
        meta = dict(bt=A.block_tables(p, B), qs=torch.arange(B, dtype=torch.int32), qlen=qlen,
                    ctx=torch.cat([p.ctx, p.ctx[-1:]]), ws=torch.arange(B, dtype=torch.int32),
                    wt=torch.zeros(B, dtype=torch.int32))
        return SimpleState(B=B, q=torch.cat([p.q, p.q[-1:]]).to(gpu), kc=kc.to(gpu), vc=vc.to(gpu), want=want,
                           cq=torch.cat([cq, cq[-1:]]).to(gpu), ckc=ckc.to(gpu), cvc=cvc.to(gpu),
                           cwant=c.repeat_interleave(G, 0)[None].expand(B - 1, -1, -1),
                           **{k: v.to(gpu) for k, v in meta.items()})
    return _on(gpu, key, build)


class SimpleState:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _decode_check(gpu, s, hkv, part, nparts, ks, vs, what, repeats=1):
    po = torch.zeros(s.B * hkv * nparts * 16 * 128, device=gpu)
    pml = torch.zeros(s.B * hkv * nparts * 16 * 2, device=gpu)
    for q, kc, vc, want, kind in ((s.q, s.kc, s.vc, s.want, "needles"), (s.cq, s.ckc, s.cvc, s.cwant, "constant V")):
        for _ in range(repeats):
            out = torch.full_like(q, SENTINEL)
            ops.paged_attention(0, q, kc, vc, s.bt, s.qs, s.qlen, s.ctx, s.ws, s.wt, out, po, pml, part, nparts, ks, vs)
            _close(out[:-1], want, A.ATOL * vs, A.RTOL, f"{what}, {kind}")
            assert (out[-1] == SENTINEL).all(), f"{what}, {kind}: the inactive row was written"


def _decode_sweep(gpu, monkeypatch, s, hkv, kwv, pd, ks, vs, what, parts=A.DECODE_PARTS, max_ctx=max(A.DECODE_CTXS)):
    for part, nparts in parts:
        nparts = nparts or math.ceil(max_ctx / part)
        for comb in (0, 1):
            _cfg(monkeypatch, attn_kwv=kwv, attn_pd=pd, attn_comb=comb)
            # attn_comb=1: three launches in a row, the last arriver's tickets must return to zero
            _decode_check(gpu, s, hkv, part, nparts, ks, vs, f"{what} kwv={kwv} pd={pd} part={part} nparts={nparts} "
                          f"attn_comb={comb}", repeats=3 if comb else 1)


@pytest.mark.parametrize("kwv,pd", KWV_PD)
def test_decode_needles_every_wave_count_and_ring(gpu, monkeypatch, kwv, pd):
    """Mode 0, bf16 cache, 32/8 heads: attn_kwv x attn_pd (the launcher honours pd = 2 for kwv <= 2; the rest run pd =
    1) x fixed partitions of 128 / 256 keys and even splits over 2 / 4 / 8, merged by the combine kernel and by the
    last arriver; contexts 33, 300, 545, 560 and 1100 over one shared cache."""
    p = A.decode_sweep(32, 8)
    s = _decode_state(gpu, p, ("decode", 32, 8))
    _decode_sweep(gpu, monkeypatch, s, 8, kwv, pd, 1.0, 1.0, "decode")


@pytest.mark.parametrize("kwv", A.KWVS)
def test_decode_needles_4096_keys_32_partitions(gpu, monkeypatch, kwv):
    p = A.decode_long()
    s = _decode_state(gpu, p, "decode4096")
    _decode_sweep(gpu, monkeypatch, s, 8, kwv, 2, 1.0, 1.0, "decode 4096", parts=((128, 32),))


@pytest.mark.parametrize("hq,hkv", A.HEADS_GQA)
@pytest.mark.parametrize("kwv", [1, 4])
def test_decode_needles_every_gqa_group(gpu, monkeypatch, hq, hkv, kwv):
    """Mode 0 at G = 1, 2, 4, 8, 16 (QT = 16 / G columns per query: a different column mapping each); every head of a
    group holds a different needle pair, so a column-to-(query, head) mix-up shows like a lost key.  The bindings
    admit every group that divides 16: none is refused."""
    p = A.decode_sweep(hq, hkv)
    s = _decode_state(gpu, p, ("decode", hq, hkv))
    _decode_sweep(gpu, monkeypatch, s, hkv, kwv, 1, 1.0, 1.0, f"decode G={hq // hkv}", parts=((128, None), (0, 4)))


@pytest.mark.parametrize("hq,hkv", A.HEADS_DECODE)
@pytest.mark.parametrize("ks,vs", SCALES)
@pytest.mark.parametrize("kwv,pd", [(k, d) for k in (1, 2, 4) for d in (1, 2)])
def test_decode_needles_fp8(gpu, monkeypatch, hq, hkv, ks, vs, kwv, pd):
    """The mode-0 sweep over an e4m3 cache (the codewords are exact in it: no looser tolerance)."""
    p = A.decode_sweep(hq, hkv)
    s = _decode_state(gpu, p, ("decode8", hq, hkv, ks), ks, vs, fp8=True)
    assert s.kc.dtype == FP8
    _decode_sweep(gpu, monkeypatch, s, hkv, kwv, pd, ks, vs, f"fp8 decode {hq}/{hkv} scales ({ks}, {vs})")


# ------------------------------------------------------------------------------------------------ folded decode
def _codes(c):
    b = c.cpu().view(torch.uint8).to(torch.int32)
    return torch.where(b >= 128, -(b - 128), b)


@pytest.mark.parametrize("hq,hkv", A.HEADS_FOLDED)
@pytest.mark.parametrize("kwv,pd", FOLDED_KWV_PD)
@pytest.mark.parametrize("dtype,ks,vs", [("bf16", 1.0, 1.0), ("fp8", 1.0, 1.0), ("fp8", 0.5, 2.0)])
def test_folded_decode_needles(gpu, monkeypatch, hq, hkv, kwv, pd, dtype, ks, vs):
    """Mode 3 at G = 1, 2, 4: q, k and v of the newest token come out of the QKV GEMM (one-hot x, identity rope) as
    exact codewords.  Needles at ctx - 1 (scored from the slabs, written by the kernel), ctx - 2 and the partition and
    stride edges; (ctx - 1) % 32 in {0, 1, 31} at the first page, a middle page and a partition's first page.  Against
    the float64 reference, against the two-op path as test_kernels_gpu._folded_case compares them, and the cache
    bytes against the codewords themselves."""
    p = A.folded_sweep(hq, hkv)

    def build():
        want, _ = A.folded_expected(p)
        dev = {k: getattr(p, k).to(gpu) for k in ("x", "w", "rope", "bt", "ctx", "qlen", "pos", "slots")}
        dev.update(qs=torch.arange(p.M, dtype=torch.int32, device=gpu), wt=torch.zeros(p.M, dtype=torch.int32, device=gpu))
        return want, dev
    want, d = _on(gpu, ("folded", hq, hkv), build)
    f8 = dtype == "fp8"
    kc0, vc0 = A.to_fp8(p.kc, p.vc, ks, vs) if f8 else (p.kc, p.vc)
    kfull, vfull = A.to_fp8(p.full_kc, p.full_vc, ks, vs) if f8 else (p.full_kc, p.full_vc)
    live = p.qlen.bool()
    for part, nparts in A.FOLDED_PARTS:
        nparts = nparts or math.ceil(int(p.ctx.max()) / part)
        res = {}
        for fused in (1, 0):
            _cfg(monkeypatch, attn_kwv=kwv, attn_pd=pd, fused_qkv_attn=fused)
            k_, v_ = kc0.clone().to(gpu), vc0.clone().to(gpu)
            q = torch.zeros(p.M, hq * 128, device=gpu, dtype=torch.bfloat16)
            out = torch.full((p.M, hq * 128), SENTINEL, device=gpu, dtype=torch.bfloat16)
            slabs = torch.full((16 * p.M * (hq + 2 * hkv) * 128,), float("nan"), device=gpu)
            po = torch.zeros(p.M * hkv * nparts * 16 * 128, device=gpu)
            pml = torch.zeros(p.M * hkv * nparts * 16 * 2, device=gpu)
            S = ops.qkv_attention_decode(d["x"], d["w"], d["pos"], d["slots"], d["rope"], q, k_, v_, hq, hkv, slabs,
                                         d["bt"], d["qs"], d["qlen"], d["ctx"], d["qs"], d["wt"], out, po, pml, part,
                                         nparts, ks, vs)
            res[fused] = (S, out.cpu().view(p.M, hq, 128), k_.cpu(), v_.cpu())
        what = f"folded {hq}/{hkv} {dtype} kwv={kwv} pd={pd} part={part} nparts={nparts}"
        assert res[0][0] == 0
        assert res[1][0] >= 1, f"{what}: the folded path did not run"
        for fused in (1, 0):
            _close(res[fused][1][live], want, A.ATOL * vs, A.RTOL, f"{what}, fused={fused}, against float64")
            assert (res[fused][1][~live] == SENTINEL).all(), f"{what}: the inactive row was written"
        _close(res[1][1][live], res[0][1][live], 1.6e-2 * vs, 1e-2, f"{what}: folded vs two-op attention out")
        if f8:
            dk = (_codes(res[1][2]) - _codes(res[0][2])).abs()
            assert int(dk.max()) <= 1 and (dk > 0).float().mean().item() <= 0.01, f"{what}: K bytes"
        else:
            _close(res[1][2], res[0][2], 1e-2, 1e-2, f"{what}: k cache")
        for fused in (1, 0):  # exact codewords: both paths leave the full cache, bit for bit, V and K alike
            assert torch.equal(res[fused][3].view(torch.uint8), vfull.view(torch.uint8)), f"{what}: V bytes, fused={fused}"
            assert torch.equal(res[fused][2].view(torch.uint8), kfull.view(torch.uint8)), f"{what}: K bytes, fused={fused}"


# ------------------------------------------------------------------------------------------------ prefill
def _prefill_state(gpu, p, key, ks=1.0, vs=1.0, fp8=False):
    def build():
        kc, vc = A.to_fp8(p.kc, p.vc, ks, vs) if fp8 else (p.kc, p.vc)
        want = {k: A.prefill_expected(p, k, kc=kc, vc=vc, ks=ks, vs=vs)[0] for k in p.q}
        B = len(p.cases)
        return SimpleState(kc=kc.to(gpu), vc=vc.to(gpu), want=want, q={k: v.to(gpu) for k, v in p.q.items()},
                           bt=A.block_tables(p, B).to(gpu), qs=p.q_start.to(gpu), qlen=p.qlen.to(gpu),
                           ctx=p.ctx.to(gpu))
    return _on(gpu, key, build)


def _prefill_check(gpu, p, s, mode, ks, vs, what):
    G = p.hq // p.hkv
    ws, wt = A.work_list(p, 64 if mode == 2 else 64 // G)
    part = math.ceil(int(p.ctx.max()) / 32) * 32
    dummy = torch.zeros(1, device=gpu)
    for kind in ("generous", "tight", "edges"):
        out = torch.full_like(s.q[kind], float("nan"))
        ops.paged_attention(mode, s.q[kind], s.kc, s.vc, s.bt, s.qs, s.qlen, s.ctx, ws.to(gpu), wt.to(gpu), out, dummy,
                            dummy, part, 1, ks, vs)
        assert not torch.isnan(out).any(), f"{what}, {kind}: a query row was never written"
        _close(out, s.want[kind], A.ATOL * vs, A.RTOL, f"{what}, {kind}")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("hq,hkv", A.HEADS_PREFILL)
def test_prefill_causal_probes(gpu, mode, hq, hkv):
    """Paged prefill (mode 1) and flash prefill (mode 2) at G = 1, 2, 4: for every query row, a needle on the diagonal
    key plus the masked key after it (a mask one key too generous halves the output), the diagonal key plus the one
    before it (a mask one key too tight), and needles over the 64-key block and page edges.  Ragged chunks whose
    first query sits mid-page and mid-block."""
    p = A.prefill_sweep(hq, hkv)
    _prefill_check(gpu, p, _prefill_state(gpu, p, ("prefill", hq, hkv)), mode, 1.0, 1.0, f"prefill mode {mode} {hq}/{hkv}")


@pytest.mark.parametrize("hg", ["auto", "1", "2", "4"])
def test_flash_prefill_causal_probes_head_split(gpu, monkeypatch, hg):
    """The one-kv-head shard (4/1) with the group's q heads split over 1 / 2 / 4 workgroups (flash_hg)."""
    if hg != "auto":
        _cfg(monkeypatch, flash_hg=hg)
    p = A.prefill_sweep(4, 1)
    _prefill_check(gpu, p, _prefill_state(gpu, p, ("prefill", 4, 1)), 2, 1.0, 1.0, f"flash prefill 4/1 flash_hg={hg}")


@pytest.mark.parametrize("hq,hkv", A.HEADS_DECODE)
@pytest.mark.parametrize("ks,vs", SCALES)
def test_paged_prefill_causal_probes_fp8(gpu, hq, hkv, ks, vs):
    p = A.prefill_sweep(hq, hkv)
    s = _prefill_state(gpu, p, ("prefill8", hq, hkv, ks), ks, vs, fp8=True)
    _prefill_check(gpu, p, s, 1, ks, vs, f"fp8 paged prefill {hq}/{hkv} scales ({ks}, {vs})")


@pytest.mark.parametrize("i", range(len(A.SPLIT_CASES)))
def test_flash_key_split_needles_on_every_range_edge(gpu, i):
    """Flash prefill with the tiles cut into key ranges by flash_split_plan(min_blocks=4, fill=1 << 20, min_target=5):
    needles at keys 64 kb - 1 and 64 kb of every range edge read out of the work list, plus the causal probes; twice
    in a row."""
    p, tiles, (work, comb, nslots) = A.split_sweep(i)
    assert len(comb) > 0 and nslots > len(comb) // 4
    s = _prefill_state(gpu, p, ("split", i))
    po = torch.zeros(nslots * p.hq * 64 * 128, device=gpu)
    pm = torch.zeros(nslots * p.hq * 64 * 2, device=gpu)
    wd, cd = torch.from_numpy(work).to(gpu), torch.from_numpy(comb).to(gpu)
    for kind in ("generous", "tight", "edges"):
        out = torch.full_like(s.q[kind], float("nan"))
        for rep in range(2):
            ops.flash_prefill_split(s.q[kind], s.kc, s.vc, s.bt, s.qs, s.qlen, s.ctx, wd, cd, out, po, pm, nslots)
            assert not torch.isnan(out).any(), "a query row was never written"
            _close(out, s.want[kind], A.ATOL, A.RTOL, f"flash key split {A.SPLIT_CASES[i]}, {kind}, launch {rep}")
