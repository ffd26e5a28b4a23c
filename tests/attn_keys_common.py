"""Shared by the key-accounting attention tests (CPU and GPU): "codeword" attention problems in which every key
matters, and their float64 expected values.  Plain torch, no GPU.

K[k] is a +-1.25 vector and V[k] a +-1 vector (exact in bf16 and in e4m3, also under the scale pair (0.5, 2)).  A
query is the sum of two "needle" keys, so the two needles score 200 / sqrt(128) = 17.7 against a background of
N(0, 2.2^2): the output is (V[j] + V[j']) / 2, and a kernel that drops j moves elements by 1, one that counts it twice
by 1/3.  Two choices keep the needle scores from falling below 17.7 (the cross term K[j] . K[j'] would otherwise move
both by N(0, 1.6^2) and the worst of ten thousand columns would sink into the background):

* consecutive keys are exactly orthogonal (K[k + 1] = K[k] * m with a balanced +-1 mask m), so the causal probes
  K[qpos] + K[qpos +- 1] score 17.68 on both keys;
* the fixed needle j' of a sweep is drawn among keys with K[j] . K[j'] >= 0.

All sequences of a decode or prefill problem share one set of cache pages (identical block-table rows): a sweep over
many key positions is one launch.  Expected values come from a float64 evaluation of the same attention over the keys
read back from the paged cache with ops/reference.py gather_kv.
"""
import math
from types import SimpleNamespace

import torch

from distributed_sse_for_llm_response_amd.ops import reference as R

PAGE, D = R.PAGE, R.HEAD_DIM
K_AMP, V_AMP = 1.25, 1.0
ATOL, RTOL = 1e-2, 2e-2          # the suite's attention tolerance (_close); fp8: ATOL times v_scale
KWVS = (1, 2, 4, 8)               # key-split waves per decode workgroup (attn_kwv)
# (part, nparts) of the decode sweeps: nparts None = by the longest context
DECODE_PARTS = ((128, None), (256, None), (0, 2), (0, 4), (0, 8))
DECODE_CTXS = (33, 300, 545, 560, 1100)
PREFILL_CASES = ((45, 45), (129, 65), (700, 100), (1333, 1333))
# folded decode: (ctx - 1) % 32 in {0, 1, 31} at the first page, a middle page and the first page of a partition
# (key 128 opens a partition of 128 keys and, at these contexts, of the even split over 4), plus the sweep's contexts
FOLDED_CTXS = (1, 2, 32, 65, 66, 96, 129, 130, 160, 385, 386, 416, 33, 300, 545, 560)
FOLDED_PARTS = ((128, None), (0, 4))
CONST_V = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)


def part_keys(part: int, nparts: int, kmax: int) -> int:
    """Keys per flash-decoding partition (attention.hip part_keys)."""
    if part > 0:
        return part
    per = -(-kmax // nparts)
    return max(PAGE, -(-per // PAGE) * PAGE)


def decode_boundaries(ctx: int, kwv: int, part: int, nparts) -> list:
    """Key positions at which a decode launch (page 32, kwv key-split waves, partitions of P keys) can lose or
    double a key: page and half-page edges, the stride edges 32 kwv i - 1 / 32 kwv i in the first, a middle and the
    last stride of the first, a middle and the last partition, the partition edges, the last two keys."""
    P = part_keys(part, nparts or 1, ctx)
    pos = {0, 1, 15, 16, 31, 32, 33, P - 1, P, P + 1, 2 * P - 1, 2 * P, ctx - 2, ctx - 1}
    stride = PAGE * kwv
    nz = -(-ctx // P)
    for z in {0, nz // 2, nz - 1}:
        k0, k1 = z * P, min((z + 1) * P, ctx)
        ns = -(-(k1 - k0) // stride)
        for i in {1, ns // 2, ns - 1}:
            e = k0 + stride * i
            if k0 < e < k1:
                pos |= {e - 1, e}
        pos |= {k0 - 1, k0}
    return sorted(p for p in pos if 0 <= p < ctx)


def decode_boundary_union(ctx: int, max_ctx: int) -> list:
    """Every boundary of `ctx` under all the (kwv, part, nparts) the sweeps run: one problem serves them all."""
    pos = set()
    for kwv in KWVS:
        for part, nparts in DECODE_PARTS:
            pos |= set(decode_boundaries(ctx, kwv, part, nparts or -(-max_ctx // part)))
    return sorted(pos)


def codewords(nkeys: int, hkv: int, gen) -> tuple:
    """K [nkeys, hkv, 128] in +-K_AMP with consecutive keys orthogonal, V [nkeys, hkv, 128] in +-V_AMP."""
    sign = lambda *s: torch.randint(0, 2, s, generator=gen).float() * 2 - 1  # noqa: E731
    k0 = sign(1, hkv, D)
    # balanced masks: 64 sign flips at random places
    order = torch.rand(nkeys - 1, hkv, D, generator=gen).argsort(-1)
    masks = torch.where(order < D // 2, -1.0, 1.0)
    K = torch.cat([k0, masks]).cumprod(0) * K_AMP
    return K, sign(nkeys, hkv, D) * V_AMP


def paged_cache(K, V, gen, extra_pages: int = 1):
    """Natural-order keys -> (k_cache [pages, hkv, 32, 128], v_cache [pages, hkv, 128, 32] (bf16), block-table row);
    the pages in a random order, `extra_pages` unaddressed pages of zeros mixed in."""
    n, hkv, _ = K.shape
    assert n % PAGE == 0
    npg = n // PAGE
    perm = torch.randperm(npg + extra_pages, generator=gen)[:npg]
    kc = torch.zeros(npg + extra_pages, hkv, PAGE, D)
    vc = torch.zeros(npg + extra_pages, hkv, D, PAGE)
    kc[perm] = K.view(npg, PAGE, hkv, D).permute(0, 2, 1, 3)
    vp = R.vperm(torch.arange(PAGE))
    vt = torch.zeros(npg, hkv, D, PAGE)
    vt[..., vp] = V.view(npg, PAGE, hkv, D).permute(0, 2, 3, 1)
    vc[perm] = vt
    return kc.bfloat16(), vc.bfloat16(), perm.to(torch.int32)


def to_fp8(kc, vc, ks: float, vs: float):
    """The bf16 codeword cache as an e4m3 cache under (k_scale, v_scale): exact, and asserted to be."""
    k8, v8 = R.quantize_kv(kc.float(), ks), R.quantize_kv(vc.float(), vs)
    assert torch.equal(R.dequantize_kv(k8, ks), kc.float()) and torch.equal(R.dequantize_kv(v8, vs), vc.float()), \
        "the codeword values are not exact in e4m3 under these scales"
    return k8, v8


def attend64(Q, K, V, limit, weight=None):
    """float64 attention of Q [n, hq, 128] over keys K / V [nk, hkv, 128]; column (i, h) sees keys < limit[i] (an int
    tensor [n] or [n, hq]); `weight` [n, hq, nk] multiplies the softmax numerators (the mutants: 0 drops a key, 2
    counts it twice).  Returns (out [n, hq, 128], p [n, hq, nk]), both float64."""
    n, hq, _ = Q.shape
    nk, hkv, _ = K.shape
    G = hq // hkv
    s = torch.einsum("nhgd,khd->nhgk", Q.double().view(n, hkv, G, D), K.double()) / math.sqrt(D)
    lim = limit if limit.dim() == 2 else limit[:, None].expand(n, hq)
    vis = torch.arange(nk)[None, None, :] < lim[:, :, None]
    s = s.reshape(n, hq, nk).masked_fill(~vis, float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values.clamp(min=-1e300))
    if weight is not None:
        e = e * weight
    p = e / e.sum(-1, keepdim=True).clamp(min=1e-300)
    out = torch.einsum("nhgk,khd->nhgd", p.reshape(n, hkv, G, nk), V.double()).reshape(n, hq, D)
    return out, p


def _anchor(K, j: int, kvh: int, ctx: int, avoid: set, gen) -> int:
    """The fixed second needle of column (j, kv head): a key below ctx away from every boundary (page offsets 5..11
    and 19..27), K[j] . K[j'] >= 0, preferring another page and, there, an odd page distance (another wave's stride
    for every kwv > 1).  j itself may lie at or beyond ctx (a ghost)."""
    offs = [5, 7, 9, 11, 19, 21, 23, 27]
    cand = [p * PAGE + o for p in range(-(-ctx // PAGE)) for o in offs]
    cand = [c for c in cand if c < ctx and c != j and not ({c - 1, c, c + 1} & avoid)]
    if not cand:
        cand = [c for c in range(ctx) if c != j] or [j]
    dots = (K[cand, kvh] * K[j, kvh]).sum(-1)
    ok = [c for c, d in zip(cand, dots.tolist()) if d >= 0] or cand
    for pref in (lambda c: (c // PAGE - j // PAGE) % 2 == 1, lambda c: c // PAGE != j // PAGE, lambda c: True):
        best = [c for c in ok if pref(c)]
        if best:
            return best[int(torch.randint(0, len(best), (1,), generator=gen))]


def needle_problem(rows, hq: int, hkv: int, seed: int, nkeys: int = None, ghosts: bool = True):
    """A decode-style needle sweep.  `rows` = [(ctx, boundary list)]: one sequence per boundary of each context; in
    sequence i head h takes needle j = list[(i + 5 h) % len], so every head of a GQA group holds a different needle
    pair and every boundary meets several heads.  With `ghosts`, two more sequences per context whose second needle is
    a key at or beyond ctx (it exists in the cache and must be ignored: expected V[j'] alone).  Returns a namespace:
    K, V natural keys; kc, vc, bt_row the shared paged cache; q [B, hq, 128] bf16; ctx [B]; J, JP [B, hq] the needles
    (JP's ghosts >= ctx); ghost [B] bool."""
    gen = torch.Generator().manual_seed(seed)
    G = hq // hkv
    max_ctx = max(c for c, _ in rows)
    nkeys = nkeys or (-(-max_ctx // PAGE) + 1) * PAGE  # a page of keys after the longest context: the tail mask
    K, V = codewords(nkeys, hkv, gen)
    kc, vc, bt_row = paged_cache(K, V, gen)
    ctxs, J, JP, ghost = [], [], [], []
    for ctx, bl in rows:
        assert bl and all(0 <= b < ctx for b in bl)
        avoid = set(bl)
        for i in range(len(bl)):
            js = [bl[(i + 5 * h) % len(bl)] for h in range(hq)]
            J.append(js)
            JP.append([_anchor(K, j, h // G, ctx, avoid, gen) for h, j in enumerate(js)])
            ctxs.append(ctx)
            ghost.append(False)
        if ghosts:
            beyond = sorted({ctx, ctx + 1, min(nkeys - 1, (ctx // PAGE + 1) * PAGE), min(nkeys - 1, ctx + 17)})
            for i in range(2):
                gs = [beyond[(i + h) % len(beyond)] for h in range(hq)]
                J.append([_anchor(K, g, h // G, ctx, avoid, gen) for h, g in enumerate(gs)])
                JP.append(gs)
                ctxs.append(ctx)
                ghost.append(True)
    J, JP = torch.tensor(J), torch.tensor(JP)
    kv = torch.arange(hq) // G
    q = (K[J, kv[None, :]] + K[JP, kv[None, :]]).bfloat16()
    return SimpleNamespace(K=K, V=V, kc=kc, vc=vc, bt_row=bt_row, q=q, ctx=torch.tensor(ctxs, dtype=torch.int32), J=J,
                           JP=JP, ghost=torch.tensor(ghost), hq=hq, hkv=hkv, nkeys=nkeys)


def decode_rows(ctxs=DECODE_CTXS) -> list:
    return [(c, decode_boundary_union(c, max(ctxs))) for c in ctxs]


def block_tables(p, B: int) -> torch.Tensor:
    return p.bt_row[None, :].expand(B, -1).contiguous()


def cache_keys(p, kc=None, vc=None, ks=1.0, vs=1.0):
    """The problem's keys read back through the paged cache (reference layout), float64."""
    Kc, Vc = R.gather_kv(p.kc if kc is None else kc, p.vc if vc is None else vc, p.bt_row, p.nkeys, ks, vs)
    return Kc.double(), Vc.double()


def needle_expected(p, mutant=None, kc=None, vc=None, ks=1.0, vs=1.0):
    """(out [B, hq, 128] float64, needle weight [B, hq]): the float64 reference over the cache; mutant "drop" /
    "double": needle J of every column weighted 0 / 2 (ghost columns: "unmask" lets the ghost key in)."""
    Kc, Vc = cache_keys(p, kc, vc, ks, vs)
    B = p.q.shape[0]
    out = torch.zeros(B, p.hq, D, dtype=torch.float64)
    mass = torch.zeros(B, p.hq, dtype=torch.float64)
    for ctx in sorted(set(p.ctx.tolist())):
        idx = (p.ctx == ctx).nonzero().flatten()
        n = idx.numel()
        nk = min(p.nkeys, ctx + 2 * PAGE)
        limit = torch.full((n, p.hq), ctx)
        w = torch.ones(n, p.hq, nk, dtype=torch.float64)
        g = p.ghost[idx]
        if mutant in ("drop", "double"):
            w[~g] = w[~g].scatter(-1, p.J[idx][~g][..., None], 0.0 if mutant == "drop" else 2.0)
        elif mutant == "unmask":
            limit[g] = p.JP[idx][g] + 1
        o, pr = attend64(p.q[idx], Kc[:nk], Vc[:nk], limit, w)
        out[idx] = o
        vis = p.JP[idx] < ctx
        m = pr.gather(-1, p.J[idx][..., None])[..., 0]
        m2 = pr.gather(-1, p.JP[idx].clamp(max=nk - 1)[..., None])[..., 0]
        mass[idx] = m + torch.where(vis & (p.JP[idx] != p.J[idx]), m2, torch.zeros_like(m2))
    return out, mass


def const_v_problem(p, seed: int):
    """The constant-V variant over p's contexts and block table: V[k, d] = c_d for every key, Q and K randn: the
    output must equal c_d at every context.  Returns (kc, vc, q, c [hkv, 128])."""
    gen = torch.Generator().manual_seed(seed)
    c = torch.tensor(CONST_V)[torch.randint(0, len(CONST_V), (p.hkv, D), generator=gen)]
    Kr = torch.randn(p.nkeys, p.hkv, D, generator=gen)
    npg = p.nkeys // PAGE
    kc, vc = torch.zeros_like(p.kc), torch.zeros_like(p.vc)  # p's page order: its block-table row serves both
    kc[p.bt_row.long()] = Kr.view(npg, PAGE, p.hkv, D).permute(0, 2, 1, 3).bfloat16()
    vc[p.bt_row.long()] = c[None, :, :, None].expand(npg, -1, -1, PAGE).bfloat16()
    q = torch.randn(p.q.shape, generator=gen).bfloat16()
    return kc, vc, q, c


# ------------------------------------------------------------------------------------------------ prefill probes
def prefill_problem(cases, hq: int, hkv: int, seed: int, edges_of=None):
    """Causal probes for the prefill kernels over one shared cache.  Sequence b = (ctx, qlen); query row i sits at
    qpos = ctx - qlen + i.  Three query sets ("kinds"), each [T, hq, 128]:
    generous: K[qpos] + K[qpos + 1] -- key qpos + 1 is in the cache but masked: expected V[qpos] alone;
    tight:    K[qpos] + K[qpos - 1] -- expected (V[qpos] + V[qpos - 1]) / 2;
    edges:    K[e] + K[qpos], e cycling (by row and head) over the 64-key block edges 64 t - 1, 64 t and the page
              edges between them below qpos (skipping an edge whose K[e] . K[qpos] < 0); with `edges_of`
              (sequence index -> key positions) over those positions instead."""
    gen = torch.Generator().manual_seed(seed)
    G = hq // hkv
    max_ctx = max(c for c, _ in cases)
    nkeys = (-(-max_ctx // PAGE) + 1) * PAGE
    K, V = codewords(nkeys, hkv, gen)
    kc, vc, bt_row = paged_cache(K, V, gen)
    kv = torch.arange(hq) // G
    qpos = torch.cat([torch.arange(c - ql, c) for c, ql in cases])
    T = qpos.numel()
    J = {"generous": qpos[:, None].expand(T, hq), "tight": qpos[:, None].expand(T, hq)}
    JP = {"generous": (qpos + 1)[:, None].expand(T, hq), "tight": (qpos - 1).clamp(min=0)[:, None].expand(T, hq)}
    edges = []
    seq = [b for b, (_, ql) in enumerate(cases) for _ in range(ql)]
    for i, qp in enumerate(qpos.tolist()):
        pool = edges_of(seq[i]) if edges_of else {e for t in range(qp // 64 + 2)
                                                  for e in (64 * t - 1, 64 * t, 64 * t + 31, 64 * t + 32)} | {0}
        el = sorted({e for e in pool if 0 <= e < qp}, reverse=True) or [qp]
        ok = ((K[el] * K[qp][None]).sum(-1) >= 0).tolist()  # [edges][hkv]: the needle pair's cross term
        row = []
        for h in range(hq):
            # odd columns stay among the newest edges: the diagonal key block and the one before it
            n = min(len(el), 9) if (i + h) % 2 else len(el)
            start = (i + 3 * h) % n
            pick = next((k for k in list(range(start, len(el))) + list(range(start)) if ok[k][h // G]), None)
            row.append(qp if pick is None else el[pick])
        edges.append(row)
    J["edges"] = torch.tensor(edges)
    JP["edges"] = qpos[:, None].expand(T, hq)
    q = {k: (K[J[k], kv[None, :]] + K[JP[k], kv[None, :]]).bfloat16() for k in J}
    return SimpleNamespace(K=K, V=V, kc=kc, vc=vc, bt_row=bt_row, q=q, J=J, JP=JP, qpos=qpos, cases=cases, hq=hq,
                           hkv=hkv, nkeys=nkeys, T=T,
                           ctx=torch.tensor([c for c, _ in cases], dtype=torch.int32),
                           qlen=torch.tensor([ql for _, ql in cases], dtype=torch.int32),
                           q_start=torch.tensor([sum(ql for _, ql in cases[:b]) for b in range(len(cases))],
                                                dtype=torch.int32))


def prefill_expected(p, kind: str, mutant=None, kc=None, vc=None, ks=1.0, vs=1.0, chunk: int = 256):
    """(out [T, hq, 128] float64, needle weight [T, hq]) of query set `kind`.  Mutants: "generous" = the mask one key
    too generous (keys <= qpos + 1), "tight" = one too tight (keys < qpos; row 0 of a cold prompt keeps key 0),
    "drop" / "double" = needle J weighted 0 / 2."""
    Kc, Vc = cache_keys(p, kc, vc, ks, vs)
    out = torch.zeros(p.T, p.hq, D, dtype=torch.float64)
    mass = torch.zeros(p.T, p.hq, dtype=torch.float64)
    for a in range(0, p.T, chunk):
        sl = slice(a, min(p.T, a + chunk))
        qp = p.qpos[sl]
        nk = min(p.nkeys, int(qp.max()) + 2)
        limit = qp + 1
        if mutant == "generous":
            limit = qp + 2
        elif mutant == "tight":
            limit = qp.clamp(min=1)
        w = None
        if mutant in ("drop", "double"):
            w = torch.ones(qp.numel(), p.hq, nk, dtype=torch.float64)
            w = w.scatter(-1, p.J[kind][sl][..., None], 0.0 if mutant == "drop" else 2.0)
        o, pr = attend64(p.q[kind][sl], Kc[:nk], Vc[:nk], limit, w)
        out[sl] = o
        j, jp = p.J[kind][sl], p.JP[kind][sl]
        m = pr.gather(-1, j[..., None])[..., 0]
        m2 = pr.gather(-1, jp.clamp(max=nk - 1)[..., None])[..., 0]
        vis = (jp < limit[:, None]) & (jp != j)
        mass[sl] = m + torch.where(vis, m2, torch.zeros_like(m2))
    return out, mass


def work_list(p, tile: int):
    """(work_seq, work_tile) of a prefill launch on `tile`-query work items, longest first."""
    ws, wt = [], []
    for b, (_, ql) in enumerate(p.cases):
        for t in reversed(range(-(-ql // tile))):
            ws.append(b)
            wt.append(t)
    return torch.tensor(ws, dtype=torch.int32), torch.tensor(wt, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ folded decode
def folded_boundaries(ctx: int) -> list:
    """Needles of a folded-decode sequence: ctx - 1 (scored from the slabs and written by the kernel), ctx - 2 (the
    last key read from the cache), then the partition and stride edges of every (kwv, part) the test runs."""
    pos = {ctx - 1, ctx - 2}
    for kwv in KWVS:
        for part, nparts in FOLDED_PARTS:
            pos |= set(decode_boundaries(ctx, kwv, part, nparts or -(-max(FOLDED_CTXS) // part)))
    first = [b for b in (ctx - 1, ctx - 2) if b >= 0]
    return first + sorted(b for b in pos if 0 <= b < ctx - 2)


def folded_problem(hq: int, hkv: int, seed: int, ctxs=FOLDED_CTXS, H: int = 1024):
    """Mode 3 (QKV GEMM folded into decode attention) on codewords.  Every sequence has its own pages (the kernel
    writes the newest key's slot) holding the same keys K / V; slot ctx - 1 starts as zeros and the GEMM produces
    q = the needle sums, k = K[ctx - 1], v = V[ctx - 1] exactly: x is one-hot (row m selects input feature m) and
    column m of the weight holds row m's QKV output in the engine's rotary-pair column order; the rope table is the
    identity.  Sequence rows: each context max(2, ceil(needles / hq)) times, row v head h takes needle
    list[(v hq + h) % len]; the last row is inactive.  Returns a namespace with the op's CPU inputs and `full_kc`,
    `full_vc`: the caches with every newest key in place."""
    gen = torch.Generator().manual_seed(seed)
    G = hq // hkv
    nkeys = (-(-max(ctxs) // PAGE) + 1) * PAGE
    K, V = codewords(nkeys, hkv, gen)
    rows = []
    for c in ctxs:
        bl = folded_boundaries(c)
        for v in range(max(2, -(-len(bl) // hq))):
            rows.append((c, [bl[(v * hq + h) % len(bl)] for h in range(hq)], set(bl)))
    M = len(rows) + 1
    assert M <= H
    npg_seq = [-(-c // PAGE) for c, _, _ in rows]
    total = sum(npg_seq) + 2
    perm = torch.randperm(total, generator=gen).tolist()
    bt = torch.zeros(M, max(npg_seq) + 1, dtype=torch.int32)
    full_kc = torch.zeros(total, hkv, PAGE, D)
    full_vc = torch.zeros(total, hkv, D, PAGE)
    vp = R.vperm(torch.arange(PAGE))
    J, JP, ctx, slots = [], [], [], []
    o = 0
    for m, (c, js, avoid) in enumerate(rows):
        pages = perm[o:o + npg_seq[m]]
        o += npg_seq[m]
        bt[m, : len(pages)] = torch.tensor(pages, dtype=torch.int32)
        nk = len(pages) * PAGE
        kk, vv = K[:nk].clone(), V[:nk].clone()
        kk[c:], vv[c:] = 0, 0  # nothing beyond the sequence's own keys
        full_kc[pages] = kk.view(-1, PAGE, hkv, D).permute(0, 2, 1, 3)
        vt = torch.zeros(len(pages), hkv, D, PAGE)
        vt[..., vp] = vv.view(-1, PAGE, hkv, D).permute(0, 2, 3, 1)
        full_vc[pages] = vt
        J.append(js)
        JP.append([_anchor(K, j, h // G, c, avoid, gen) for h, j in enumerate(js)])
        ctx.append(c)
        slots.append(pages[(c - 1) // PAGE] * PAGE + (c - 1) % PAGE)
    J, JP = torch.tensor(J), torch.tensor(JP)
    kvh = torch.arange(hq) // G
    qn = K[J, kvh[None, :]] + K[JP, kvh[None, :]]                     # [M - 1, hq, 128]
    newest = torch.tensor(ctx) - 1
    units = torch.cat([qn, K[newest], V[newest]], 1)                   # [M - 1, hq + 2 hkv, 128] natural order
    N = (hq + 2 * hkv) * D
    w = torch.zeros(N, H)
    w[:, : M - 1] = units[:, :, R.rotary_perm()].reshape(M - 1, N).t()
    x = torch.zeros(M, H)
    x[torch.arange(M - 1), torch.arange(M - 1)] = 1.0
    # initial caches: the newest key's slot still empty
    kc, vc = full_kc.clone(), full_vc.clone()
    for s in slots:
        kc[s // PAGE, :, s % PAGE, :] = 0
        vc[s // PAGE, :, :, int(vp[s % PAGE])] = 0
    rope = torch.zeros(max(ctxs) + 1, 64, 2)
    rope[..., 0] = 1.0
    ctx_t = torch.tensor(ctx + [0], dtype=torch.int32)
    return SimpleNamespace(K=K, V=V, kc=kc.bfloat16(), vc=vc.bfloat16(), full_kc=full_kc.bfloat16(),
                           full_vc=full_vc.bfloat16(), bt=bt, x=x.bfloat16(), w=R.tile_weight(w.bfloat16()),
                           rope=rope, ctx=ctx_t, qlen=torch.tensor([1] * (M - 1) + [0], dtype=torch.int32),
                           pos=(ctx_t - 1).clamp(min=0), slots=torch.tensor(slots + [-1], dtype=torch.int32),
                           q=qn.bfloat16(), J=J, JP=JP, hq=hq, hkv=hkv, M=M, H=H, nkeys=nkeys)


def folded_expected(p, mutant=None):
    """(out [M - 1, hq, 128] float64, needle weight) of the live rows over the natural keys."""
    n = p.M - 1
    out = torch.zeros(n, p.hq, D, dtype=torch.float64)
    mass = torch.zeros(n, p.hq, dtype=torch.float64)
    ctx = p.ctx[:n]
    for c in sorted(set(ctx.tolist())):
        idx = (ctx == c).nonzero().flatten()
        w = None
        if mutant in ("drop", "double"):
            w = torch.ones(idx.numel(), p.hq, c, dtype=torch.float64)
            w = w.scatter(-1, p.J[idx][..., None], 0.0 if mutant == "drop" else 2.0)
        o, pr = attend64(p.q[idx], p.K[:c].double(), p.V[:c].double(), torch.full((idx.numel(),), c), w)
        out[idx] = o
        m = pr.gather(-1, p.J[idx][..., None])[..., 0]
        m2 = pr.gather(-1, p.JP[idx][..., None])[..., 0]
        mass[idx] = m + torch.where(p.JP[idx] != p.J[idx], m2, torch.zeros_like(m2))
    return out, mass


# ------------------------------------------------------------------------------------------------ the problems
# One definition of every problem the GPU tests launch; the CPU test checks the same objects.
HEADS_DECODE = ((32, 8), (4, 1))                                   # the sweeps (bf16: 32/8; fp8: both)
HEADS_GQA = ((8, 8), (8, 4), (32, 8), (16, 2), (16, 1))             # G = 1, 2, 4, 8, 16
HEADS_FOLDED = ((8, 8), (8, 4), (32, 8), (4, 1))                    # G = 1, 2, 4, 4
HEADS_PREFILL = ((8, 8), (16, 8), (32, 8), (4, 1))                  # G = 1, 2, 4 and the one-kv-head shard
SPLIT_CASES = (((1, 4), ((2048, 2048),)), ((1, 4), ((1500, 1500), (700, 300))), ((2, 2), ((1333, 1333),)),
               ((2, 1), ((1100, 1100), (1030, 1030))))
_problems = {}


def _memo(key, build):
    if key not in _problems:
        _problems[key] = build()
    return _problems[key]


def decode_sweep(hq: int, hkv: int):
    return _memo(("decode", hq, hkv), lambda: needle_problem(decode_rows(), hq, hkv, seed=1000 + hq * 16 + hkv))


def decode_long():
    """One 4096-key context at part = 128: 32 partitions."""
    rows = [(4096, sorted({b for kwv in KWVS for b in decode_boundaries(4096, kwv, 128, 32)}))]
    return _memo("decode4096", lambda: needle_problem(rows, 32, 8, seed=4096))


def prefill_sweep(hq: int, hkv: int):
    return _memo(("prefill", hq, hkv), lambda: prefill_problem(PREFILL_CASES, hq, hkv, seed=2000 + hq * 16 + hkv))


def split_tiles(cases) -> list:
    """[(seq, tile, key blocks)] of a flash-prefill launch, heaviest first (ModelRunner's order)."""
    tiles = [(b, t, -(-(c - ql + min(ql, 64 * (t + 1))) // 64)) for b, (c, ql) in enumerate(cases)
             for t in range(-(-ql // 64))]
    return sorted(tiles, key=lambda x: -x[2])


def split_sweep(i: int):
    """SPLIT_CASES[i] cut by flash_split_plan as the engine would: (problem, tiles, plan); the 'edges' needles sit at
    keys 64 kb - 1 and 64 kb of every range edge kb0 / kb1 read out of the plan's work list."""
    def build():
        from distributed_sse_for_llm_response_amd.engine.model_runner import flash_split_plan

        (hkv, G), cases = SPLIT_CASES[i]
        tiles = split_tiles(cases)
        plan = flash_split_plan(tiles, hkv, min_blocks=4, fill=1 << 20, min_target=5)
        assert plan is not None
        work = plan[0]
        nw = work.size // 5
        edges = {}
        for k in range(nw):
            for kb in work[2 * nw + 2 * k: 2 * nw + 2 * k + 2].tolist():
                edges.setdefault(int(work[k]), set()).update({64 * kb - 1, 64 * kb})
        p = prefill_problem(cases, hkv * G, hkv, seed=3000 + i, edges_of=lambda b: edges[b])
        return p, tiles, plan
    return _memo(("split", i), build)


def folded_sweep(hq: int, hkv: int):
    return _memo(("folded", hq, hkv), lambda: folded_problem(hq, hkv, seed=5000 + hq * 16 + hkv))


def tolerance(ref, vs: float = 1.0):
    return ATOL * vs + RTOL * ref.abs()


def mutant_distance(ref, mut, vs: float = 1.0):
    """Per column, the largest |mutant - reference| in units of the GPU test's tolerance for that element."""
    return ((mut - ref).abs() / tolerance(ref, vs)).amax(-1)
