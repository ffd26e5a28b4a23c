"""The three sampling sites of the model runner (_sample_commit: decode and mixed steps; _graph_sample: the captured
first token; _prefill_sample: the eager first token) under all 16 combinations of (penalties, logprobs, bias / ban /
min_p, guides): every ops.* and comm.all_gather_into call they make, with its operands, equals the recorded list in
tests/golden/sampling_sites_parent.json, and the passes appear in the one documented order (docs/kernels.md,
ModelRunner._sample).  A tensor operand is recorded as (owner, storage offset, shape, stride, dtype), owner = the
runner / _PrefillStatic / weights attribute whose storage it shares ("fresh": none), so a captured graph built from
the same calls launches the same kernels on the same buffers.

The golden file was recorded by this code from the tree whose three sites were still written out by hand.  To record
it again (only when a sampling pass is added or an operand changes on purpose):

    DSSE_SAMPLING_SITES_REGEN=1 python -m pytest tests/test_sampling_sites_cpu.py

which rewrites the file and then compares against it; the switch is off by default.  The TP branch (comm.size > 1) is
covered by test_logprobs_cpu.py::test_tp2_logprobs_match_tp1 and test_tp_cpu.py, not here."""
import inspect
import itertools
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq, _PrefillStatic
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights

GOLDEN = Path(__file__).parent / "golden" / "sampling_sites_parent.json"
REGEN = os.environ.get("DSSE_SAMPLING_SITES_REGEN", "0") == "1"
FLAGS = list(itertools.product((False, True), repeat=4))  # (hist_used, lp_used, ctl_used, guide_used)
SITES = ("decode", "graph", "eager")
# the one pass order; ops outside it (the graph site's gather and both first-token sites' LM head) come first
PASS_ORDER = (("prefill_sample_gather", "gemm_out"), ("logprob_stats",), ("sample_bias_ban",), ("sample_penalties",),
              ("guide_mask",), ("sample_candidates", "sample_candidates_min_p"), ("all_gather_into",),
              ("sample_pick", "sample_pick_hist", "prefill_sample_commit_hist", "sample_hist_append"),
              ("guide_advance",), ("logprob_chosen", "logprob_finish"))
RANK = {name: i for i, names in enumerate(PASS_ORDER) for name in names}
_W = {}


def _key(flags) -> str:
    return "".join("1" if f else "0" for f in flags)


def _runner(flags):
    """A CPU runner with the features of `flags` on and non-neutral metadata in slots 0 and 1."""
    if "w" not in _W:
        _W["w"] = convert_standard(TINY, init_standard_weights(TINY, seed=11))
    r = ModelRunner(_W["w"], num_blocks=64, max_batch=4, max_model_len=512, device="cpu", use_graphs=False)
    hist, lp, ctl, guide = flags
    r.temperature[:2] = torch.tensor([0.0, 0.8])
    r.top_k[:2] = torch.tensor([0, 5], dtype=torch.int32)
    r.top_p[:2] = torch.tensor([1.0, 0.9])
    r.seeds[:2] = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32)
    r.positions[:2] = torch.tensor([7, 9], dtype=torch.int32)
    r.active[:2] = 1
    if hist:
        r.set_history(0, [5, 6, 7, 5], 3)
        r.set_history(1, [8, 9], 2)
        r.presence[:2] = torch.tensor([0.5, 0.0])
        r.frequency[:2] = torch.tensor([0.0, 0.25])
        r.repetition[:2] = torch.tensor([1.2, 1.0])
        r.n_prompt[:2] = torch.tensor([3, 2], dtype=torch.int32)
    if lp:
        r.enable_logprobs()
        r.lp_meta[:2] = torch.tensor([3, 0], dtype=torch.int32)
    if ctl:
        r.set_controls(0, {7: 1.5, 9: -2.0}, [2])
        r.set_controls(1, {}, [2, 11])
        m = r.ctl_meta.view(4, -1)
        m[0, :2], m[1, :2], m[2, :2] = torch.tensor([2, 0]), torch.tensor([1, 2]), torch.tensor([64, 64])
        r.min_p[:2] = torch.tensor([0.0, 0.05])
    if guide:
        r.set_guide_vocab(["a", "b", "c"], 2)  # ids 0 and 2 (EOS) belong to no guide: "b" is the language's alphabet
        tab = np.full((2, 256), ops.GUIDE_DEAD, dtype=np.uint16)
        tab[0, ord("b")] = tab[1, ord("b")] = 1  # b+
        r.upload_guide(1, tab, np.array([0, 1], dtype=np.uint8))
        r.set_guide(0, 1, 0)
        r.set_guide(1, 1, 1)
    return r


def _owners(r) -> dict:
    """storage address -> attribute name, first attribute in definition order (slot_meta before its views)."""
    out = {}

    def add(name, v):
        if isinstance(v, torch.Tensor):
            out.setdefault(v.untyped_storage().data_ptr(), name)
        elif isinstance(v, dict):
            for k, e in v.items():
                add(f"{name}[{k}]", e)

    for prefix, obj in (("", r), ("pf.", r.pf), ("w.", r.w), ("kv.", r.kv)):
        for name, v in (vars(obj) if obj is not None else {}).items():
            add(prefix + name, v)
    return out


def _enc(v, owners):
    if isinstance(v, torch.Tensor):
        return [owners.get(v.untyped_storage().data_ptr(), "fresh"), v.storage_offset(), list(v.shape),
                list(v.stride()), str(v.dtype).replace("torch.", "")]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"unrecorded operand type {type(v).__name__}")


class _Recorder:
    """Wraps every ops function and comm.all_gather_into for the length of a `with`; calls land in self.calls."""

    def __init__(self, r, mp):
        self.r, self.calls = r, []
        for name, fn in inspect.getmembers(ops, inspect.isfunction):
            if fn.__module__ == ops.__name__ and not name.startswith("_"):
                mp.setattr(ops, name, self._wrap(name, fn))
        mp.setattr(r.comm, "all_gather_into", self._wrap("all_gather_into", r.comm.all_gather_into))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def call(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            owners = _owners(self.r)
            self.calls.append([name, {k: _enc(v, owners) for k, v in bound.arguments.items()}])
            return fn(*a, **kw)
        return call

    def take(self) -> list:
        out, self.calls = self.calls, []
        return out


def _record(flags) -> dict:
    r = _runner(flags)
    g = torch.Generator().manual_seed(5)
    r.logits.copy_(torch.randn(r.logits.shape, generator=g))
    r.pf = _PrefillStatic(r, 256)
    r.pf.x.copy_(torch.randn(r.pf.x.shape, generator=g))
    bts = [list(range(8 * i, 8 * i + 8)) for i in range(2)]
    seqs = [PrefillSeq(0, [11, 12, 13, 14, 15], 0, bts[0], True), PrefillSeq(1, [21, 22, 23], 0, bts[1], True)]
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        rec = _Recorder(r, mp)
        r._sample_commit(4)
        out["decode"] = rec.take()
        q_start, q_len = r.pf.upload(seqs, 64, ring_row=3)
        r._graph_sample()
        out["graph"] = rec.take()
        r._prefill_sample(seqs, r.pf.x, q_start, q_len, 3)
        out["eager"] = rec.take()
    return out


@pytest.fixture(scope="module")
def golden():
    if REGEN:
        lines = [f'"{_key(f)}": ' + json.dumps(_record(f), separators=(",", ":")) for f in FLAGS]
        GOLDEN.write_text("{\n" + ",\n".join(lines) + "\n}\n")
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("flags", FLAGS, ids=_key)
def test_sites_make_the_recorded_calls_in_the_documented_order(flags, golden):
    got = json.loads(json.dumps(_record(flags)))
    for site in SITES:
        names = [c[0] for c in got[site]]
        ranks = [RANK[n] for n in names]  # (a KeyError: a new op at a sampling site needs its place in PASS_ORDER)
        assert ranks == sorted(ranks), (site, names)
        want = golden[_key(flags)][site]
        assert names == [c[0] for c in want], site
        for i, (a, b) in enumerate(zip(got[site], want)):
            assert a == b, (site, i, a[0])
    hist, lp, ctl, guide = flags
    for site in SITES:  # every pass that is on is there, at every site
        names = {c[0] for c in got[site]}
        assert ("logprob_stats" in names) == ("logprob_finish" in names) == lp
        assert ("sample_bias_ban" in names) == ("sample_candidates_min_p" in names) == ctl
        assert ("sample_penalties" in names) == hist
        assert ("guide_mask" in names) == ("guide_advance" in names) == guide


@pytest.mark.parametrize("flags", FLAGS, ids=_key)
def test_move_slots_swaps_every_per_slot_array(flags):
    r = _runner(flags)
    hist, lp, ctl, guide = flags
    arrays = [(r.ids, 0), (r.positions, 0)]
    arrays += [(r.hist_state, 0)] if hist else []
    arrays += [(r.lp_meta, 0)] if lp else []
    arrays += [(r.ctl_body, 0), (r.ctl_meta.view(4, -1), 1)] if ctl else []
    arrays += [(r.guide_meta.view(2, -1), 1)] if guide else []
    for n, (t, dim) in enumerate(arrays):  # distinct values everywhere: slot s of array n holds 1000 n + 100 s + j
        rows = t.movedim(dim, 0)
        rows.copy_((1000 * n + 100 * torch.arange(rows.shape[0]).view(-1, *[1] * (rows.dim() - 1)) +
                    torch.arange(rows[0].numel()).view(rows[0].shape) % 97).to(torch.int32))
    before = [t.clone() for t, _ in arrays]
    r.move_slots([0, 2], [2, 0])
    for (t, dim), b in zip(arrays, before):
        assert torch.equal(t.select(dim, 0), b.select(dim, 2)) and torch.equal(t.select(dim, 2), b.select(dim, 0))
        assert torch.equal(t.select(dim, 1), b.select(dim, 1)) and torch.equal(t.select(dim, 3), b.select(dim, 3))
