"""Paged KV cache (HBM) and its host-side block allocator.

Layout (one tensor per K and V for all layers, so a layer's cache is a contiguous view):

* K: [L, blocks, Hkv_local, 32, 128] bf16 — one key row = 256 contiguous bytes
* V: [L, blocks, Hkv_local, 128, 32] bf16 — transposed pages, tokens permuted by ``vperm``

Pages are 32 tokens.  At TP=1 Mistral-7B needs 128 KiB per token, so 100 GB of the 288 GB HBM holds
~780k tokens (about 190 sequences of 4k context per GPU).  The cache is zero-initialised so keys
past a sequence's end inside its last page are finite (they are masked, but 0·NaN would poison PV).

``dtype=torch.float8_e4m3fn`` (``kv_cache_dtype="fp8"``) stores one byte per element in the same shapes and element
order: a key row is 128 bytes, a token costs 64 KiB, and the same budget holds twice the pages.  Stored value =
x / scale with per-layer fp32 scalars ``k_scale`` / ``v_scale`` (default 1.0; ops/reference.py ``quantize_kv``).
Nothing above the cache -- allocator, block tables, slots, prefix-cache hashes -- knows the dtype.
"""
from __future__ import annotations

import hashlib
from array import array
from collections import OrderedDict

import torch

PAGE = 32

from ..serving.config import KV_CACHE_DTYPES  # ("auto", "bf16", "fp8", "fp8_e4m3"): auto = bf16; fp8 = fp8_e4m3


def kv_cache_torch_dtype(name) -> torch.dtype:
    """The cache element type of a ``kv_cache_dtype`` option (or a torch dtype, passed through)."""
    if isinstance(name, torch.dtype):
        if name not in (torch.bfloat16, torch.float8_e4m3fn):
            raise ValueError(f"KV cache dtype must be bfloat16 or float8_e4m3fn, got {name}")
        return name
    key = str(name or "auto").strip().lower()
    if key not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype must be one of {', '.join(KV_CACHE_DTYPES)}; got {name!r}")
    return torch.float8_e4m3fn if key.startswith("fp8") else torch.bfloat16


class KVCache:
    def __init__(self, num_layers: int, num_blocks: int, nkv: int, device, dtype=torch.bfloat16):
        dtype = kv_cache_torch_dtype(dtype)
        self.num_layers, self.num_blocks, self.nkv = num_layers, num_blocks, nkv
        self.dtype = dtype
        self.k = torch.zeros(num_layers, num_blocks, nkv, PAGE, 128, device=device, dtype=dtype)
        self.v = torch.zeros(num_layers, num_blocks, nkv, 128, PAGE, device=device, dtype=dtype)
        # per-layer dequantisation scales of an fp8 cache (host floats: constants of every captured graph)
        self.k_scale = [1.0] * num_layers
        self.v_scale = [1.0] * num_layers

    @property
    def is_fp8(self) -> bool:
        return self.dtype == torch.float8_e4m3fn

    @staticmethod
    def bytes_per_block(num_layers: int, nkv: int, dtype=torch.bfloat16) -> int:
        return 2 * num_layers * nkv * PAGE * 128 * kv_cache_torch_dtype(dtype).itemsize

    @classmethod
    def blocks_for_budget(cls, budget_bytes: int, num_layers: int, nkv: int, dtype=torch.bfloat16) -> int:
        return max(1, budget_bytes // cls.bytes_per_block(num_layers, nkv, dtype))


def page_hashes(tokens, prev: bytes = b"", first: int = 0) -> list:
    """Content hashes of the full pages of `tokens` from page `first` on: a chain, h_i = blake2b(h_{i-1} ||
    int32 bytes of tokens[32 i : 32 i + 32], 16-byte digest) with h_{-1} empty (`prev` = h_{first-1}), so a page's hash
    names the whole prefix up to and including it.  A 128-bit digest is treated as collision-free: two different
    prefixes with one hash would share KV pages, at odds of ~2^-128 per pair.  Nothing but the token ids feeds the KV
    (one model, no adapters), so there is no salt."""
    n = len(tokens) // PAGE
    raw = memoryview(array("i", tokens[PAGE * first:PAGE * n]).tobytes())  # (int32, native = little-endian here)
    out = []
    for i in range(n - first):
        prev = hashlib.blake2b(prev + raw[4 * PAGE * i:4 * PAGE * (i + 1)], digest_size=16).digest()
        out.append(prev)
    return out


class BlockAllocator:
    """Free-list allocator of KV pages (host side; the device only sees block tables).

    prefix_cache=True adds automatic prefix caching: per-page reference counts and a content index over full pages
    (``page_hashes``).  A page with a published hash whose last owner frees it stays indexed in an LRU pool of
    evictable pages, where a later ``lookup`` can revive it; ``allocate`` takes plain free pages first and evicts
    from the pool's least recently used end only when they run out.  Only full pages are shared, and a shared page
    is never written again.  With the flag off nothing below the free list is touched: the same pages in the same
    order as ever."""

    def __init__(self, num_blocks: int, prefix_cache: bool = False):
        self.num_blocks = num_blocks
        self._free = list(range(num_blocks - 1, -1, -1))
        self.prefix_cache = prefix_cache
        self.evictions = 0
        if prefix_cache:
            self._ref = [0] * num_blocks
            self._index: dict = {}      # page hash -> block
            self._hash_of: dict = {}    # block -> its published hash
            self._lru: OrderedDict = OrderedDict()  # evictable blocks (published, no owner), least recently used first

    @property
    def num_free(self) -> int:
        return len(self._free) + (len(self._lru) if self.prefix_cache else 0)

    def can_allocate(self, n: int) -> bool:
        return n <= self.num_free

    def allocate(self, n: int) -> list:
        if n > self.num_free:
            raise MemoryError(f"KV cache exhausted: need {n} blocks, {self.num_free} free")
        if not self.prefix_cache:
            return [self._free.pop() for _ in range(n)]
        out = []
        for _ in range(n):
            if self._free:
                b = self._free.pop()
            else:  # evict: the page leaves the index and is anybody's again
                b, _ = self._lru.popitem(last=False)
                del self._index[self._hash_of.pop(b)]
                self.evictions += 1
            self._ref[b] = 1
            out.append(b)
        return out

    def free(self, blocks) -> None:
        blocks = list(blocks)
        if not self.prefix_cache:
            self._free.extend(reversed(blocks))
            return
        plain = []
        # one reference less per block.  Tail first: a sequence's later pages enter the evictable pool before its
        # earlier ones, so they are evicted first and what survives of a prompt is still a usable (leading) prefix
        for b in reversed(blocks):
            self._ref[b] -= 1
            assert self._ref[b] >= 0, f"KV page {b} freed more often than it was taken"
            if self._ref[b] == 0:
                if b in self._hash_of:
                    self._lru[b] = None
                else:
                    plain.append(b)
        self._free.extend(plain)  # (already reversed: the first of `blocks` is the next one allocated, as ever)

    # ---- prefix cache -------------------------------------------------------------------------
    def lookup(self, hashes) -> list:
        """The longest leading run of `hashes` that is resident, as blocks; one reference is taken on each (a page
        that sat in the evictable pool leaves it).  The caller gives them back with ``free``."""
        out = []
        for h in hashes:
            b = self._index.get(h)
            if b is None:
                break
            out.append(b)
        for b in out:
            if self._ref[b] == 0:
                del self._lru[b]
            self._ref[b] += 1
        return out

    def publish(self, block: int, h: bytes) -> bool:
        """Record the content hash of a full page whose 32 writes are all enqueued.  A hash that is already indexed
        keeps its block: `block` then stays private (and goes back to the plain free list when freed)."""
        if h in self._index or block in self._hash_of:
            return False
        self._index[h] = block
        self._hash_of[block] = h
        return True

    def is_shared(self, block: int) -> bool:
        """More than one owner, or published (a later lookup may read it): it must never be written."""
        return self.prefix_cache and (self._ref[block] > 1 or block in self._hash_of)


def blocks_needed(num_tokens: int) -> int:
    return (num_tokens + PAGE - 1) // PAGE
