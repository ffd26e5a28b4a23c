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
    prefixes with one hash would share KV pages, at odds of ~2^-128 per pair.  Besides the token ids only a LoRA adapter feeds the KV: a
    sequence under an adapter starts its chain from a digest of the adapter's name as `prev` (LLMEngine._hash_salt), so
    its pages never serve another adapter or the base model; base-model chains start from the empty `prev`."""
    n = len(tokens) // PAGE
    raw = memoryview(array("i", tokens[PAGE * first:PAGE * n]).tobytes())  # (int32, native = little-endian here)
    out = []
    for i in range(n - first):
        prev = hashlib.blake2b(prev + raw[4 * PAGE * i:4 * PAGE * (i + 1)], digest_size=16).digest()
        out.append(prev)
    return out


class HostPageStore:
    """The prefix cache's second tier: evicted KV pages in host memory, indexed by the same content hashes.

    One allocation of `capacity_pages` records of `bytes_per_block` bytes (pinned for a GPU engine, so the copies to
    and from it are asynchronous; a plain tensor for the CPU engine), a hash -> slot index and an LRU order over the
    slots that may be recycled.  A slot is

    * ``free``     -- holds nothing;
    * ``filling``  -- reserved for a page whose device-to-host copy is in flight: its hash is known (a second spill
                      of the same content is refused) but ``find`` does not see it, so nothing reads half a page;
    * ``ready``    -- holds a whole page; visible to ``find`` and, least recently used first, recyclable;
    * ``reading``  -- ready, and the source of a host-to-device copy that has not completed (counted: several
                      restores may read one slot): visible, never recycled.

    The store only keeps books; the copies and their events belong to the runner (model_runner.KVOffload), which
    calls ``commit`` / ``release`` when they have completed."""

    FREE, FILLING, READY, READING = "free", "filling", "ready", "reading"

    def __init__(self, capacity_pages: int, bytes_per_block: int, pinned: bool = False):
        if capacity_pages < 1:
            raise ValueError("the host KV tier needs room for at least one page")
        self.capacity, self.bytes_per_block = int(capacity_pages), int(bytes_per_block)
        self.buf = torch.empty(self.capacity, self.bytes_per_block, dtype=torch.uint8, pin_memory=bool(pinned))
        self.state = [self.FREE] * self.capacity
        self._free = list(range(self.capacity - 1, -1, -1))
        self._slot_of: dict = {}   # hash -> slot (filling, ready or reading)
        self._hash_of: dict = {}   # slot -> hash
        self._readers = [0] * self.capacity
        self._lru: OrderedDict = OrderedDict()  # ready slots, least recently used first
        self.recycled = 0

    def __len__(self) -> int:
        return len(self._slot_of)

    def has(self, h: bytes) -> bool:
        """The hash holds a slot in any state (a page that is here, or on its way, is not spilled again)."""
        return h in self._slot_of

    def find(self, h: bytes):
        """The slot of a whole page with this hash (ready or reading), or None."""
        slot = self._slot_of.get(h)
        return None if slot is None or self.state[slot] == self.FILLING else slot

    def reserve(self, h: bytes):
        """A ``filling`` slot for a page about to be copied in: a free one, else the least recently used ready one
        (its content is dropped).  None when the hash already holds a slot or every slot is filling or being read."""
        if h in self._slot_of:
            return None
        if self._free:
            slot = self._free.pop()
        elif self._lru:
            slot, _ = self._lru.popitem(last=False)
            del self._slot_of[self._hash_of.pop(slot)]
            self.recycled += 1
        else:
            return None
        self.state[slot] = self.FILLING
        self._slot_of[h], self._hash_of[slot] = slot, h
        return slot

    def commit(self, slot: int) -> None:
        """The copy into a filling slot has completed: the page is visible from now on."""
        assert self.state[slot] == self.FILLING, (slot, self.state[slot])
        self.state[slot] = self.READY
        self._lru[slot] = None

    def cancel(self, slot: int) -> None:
        """A reserved slot whose copy was never issued goes back to the free list."""
        assert self.state[slot] == self.FILLING, (slot, self.state[slot])
        del self._slot_of[self._hash_of.pop(slot)]
        self.state[slot] = self.FREE
        self._free.append(slot)

    def acquire(self, slot: int) -> None:
        """A host-to-device copy will read this slot: it is not recycled until ``release``."""
        assert self.state[slot] in (self.READY, self.READING), (slot, self.state[slot])
        if self._readers[slot] == 0:
            del self._lru[slot]
            self.state[slot] = self.READING
        self._readers[slot] += 1

    def release(self, slot: int) -> None:
        """One reader's copy has completed (or was never issued); the last one makes the slot recyclable again, as the
        most recently used."""
        assert self.state[slot] == self.READING and self._readers[slot] > 0, (slot, self.state[slot])
        self._readers[slot] -= 1
        if self._readers[slot] == 0:
            self.state[slot] = self.READY
            self._lru[slot] = None


class BlockAllocator:
    """Free-list allocator of KV pages (host side; the device only sees block tables).

    prefix_cache=True adds automatic prefix caching: per-page reference counts and a content index over full pages
    (``page_hashes``).  A page with a published hash whose last owner frees it stays indexed in an LRU pool of
    evictable pages, where a later ``lookup`` can revive it; ``allocate`` takes plain free pages first and evicts
    from the pool's least recently used end only when they run out.  Only full pages are shared, and a shared page
    is never written again.  With the flag off nothing below the free list is touched: the same pages in the same
    order as ever.

    ``fork`` (parallel sampling: the choices of one request share their prompt's full pages) takes one more reference
    on blocks that already have an owner, in either mode.  With the prefix cache on that is the per-page count; with
    it off, a sparse table of the extra references, empty unless something was forked, so that ``free`` gives a block
    back only when its last owner lets go of it.

    host_store (a HostPageStore, with prefix_cache=True only) adds the host tier: an evicted page's (block, hash) goes
    on a spill list that the engine drains (``take_spills``) and copies out before the page's new owner writes it, and
    ``lookup_tiers`` continues a hash chain from the index into the store.  Which pages are handed out, and in which
    order, does not depend on the store."""

    def __init__(self, num_blocks: int, prefix_cache: bool = False, host_store: HostPageStore | None = None):
        if host_store is not None and not prefix_cache:
            raise ValueError("the host KV tier sits behind the prefix cache: it needs prefix_cache=True")
        self.num_blocks = num_blocks
        self._free = list(range(num_blocks - 1, -1, -1))
        self.prefix_cache = prefix_cache
        self.host_store = host_store
        self._spills: list = []  # (block, hash) of pages evicted since take_spills, least recently used first
        self.evictions = 0
        self._extra: dict = {}  # prefix_cache off: block -> references beyond the first (fork)
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
                h = self._hash_of.pop(b)
                del self._index[h]
                self.evictions += 1
                if self.host_store is not None:  # its bytes are still the page: the engine copies them out
                    self._spills.append((b, h))
            self._ref[b] = 1
            out.append(b)
        return out

    def free(self, blocks) -> None:
        blocks = list(blocks)
        if not self.prefix_cache:
            if self._extra:  # a forked block loses one reference and stays with its other owners
                kept = []
                for b in blocks:
                    n = self._extra.get(b)
                    if n is None:
                        kept.append(b)
                    elif n > 1:
                        self._extra[b] = n - 1
                    else:
                        del self._extra[b]
                blocks = kept
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

    def fork(self, blocks) -> list:
        """One more reference on each of `blocks`, which must have an owner already (parallel sampling: a sibling
        shares its parent's full prompt pages).  Returns them; the caller gives them back with ``free`` like any
        other block, and nobody writes them while they are shared (``is_shared``)."""
        blocks = list(blocks)
        if self.prefix_cache:
            for b in blocks:
                assert self._ref[b] > 0, f"KV page {b} forked without an owner"
                self._ref[b] += 1
        else:
            for b in blocks:
                self._extra[b] = self._extra.get(b, 0) + 1
        return blocks

    @property
    def has_forks(self) -> bool:
        """Prefix cache off: some block has more than one owner right now."""
        return bool(self._extra)

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

    def take_spills(self) -> list:
        """(block, hash) of the pages evicted since the last call, in eviction order (least recently used first).  The
        blocks already belong to their new owners: the caller must enqueue their copies before anything writes them."""
        out, self._spills = self._spills, []
        return out

    def lookup_tiers(self, hashes, max_host: int | None = None) -> tuple:
        """``lookup`` across both tiers: the longest leading run of `hashes` whose pages are resident in HBM or whole
        in the host store (HBM first; the run stops at the first hash in neither, and before host page number
        `max_host` + 1: the caller can restore only so many).  Returns (run, host): run[i] is the block of page i, or
        None for a page to restore; host = [(i, slot)] for those, in order.  A reference is taken on each block, and
        each host slot is acquired (``reading``): the caller gives them back with ``free`` / ``host_store.release``."""
        st = self.host_store
        run, host = [], []
        for i, h in enumerate(hashes):
            b = self._index.get(h)
            if b is None:
                slot = st.find(h) if st is not None else None
                if slot is None or (max_host is not None and len(host) >= max_host):
                    break
                host.append((i, slot))
            run.append(b)
        for b in run:
            if b is not None:
                if self._ref[b] == 0:
                    del self._lru[b]
                self._ref[b] += 1
        for _, slot in host:
            st.acquire(slot)
        return run, host

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
        if not self.prefix_cache:
            return block in self._extra
        return self._ref[block] > 1 or block in self._hash_of


def blocks_needed(num_tokens: int) -> int:
    return (num_tokens + PAGE - 1) // PAGE
