"""Kernel entry rule (docs/kernels.md, "Kernel entry"): every kernel of the 64-stream decode graph gets the operands of
its first loads preloaded in SGPRs and reads no hidden kernel argument.

Cross-compiles the device side of the four kernel files with the project's own flags (`hipcc -S --cuda-device-only`) and
reads two things per kernel, both metadata: the kernel descriptor's `.amdhsa_user_sgpr_kernarg_preload_length` and the
argument list of its `amdhsa.kernels` entry.  No instruction stream is searched.
"""
from __future__ import annotations

import concurrent.futures as cf
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from distributed_sse_for_llm_response_amd import _build

FILES = ["gemm_stream", "attention", "elementwise", "sampler"]

# (file, mangled-name prefix, dwords the entry needs preloaded).  The count is the kernarg dwords, padding included,
# up to the last argument that a first load's address depends on.
ENTRY = {
    # X(2) ldx M W(2) K N Kr gx xs S part(2): the first DMA burst's addresses and the split-K numbering
    "ring qkv <4,3,5,5>": ("gemm_stream", "_ZN4dsse16gemm_ring_kernelILi4ELi3ELi5ELi5ELb0EEEv", 14),
    "ring o/down <4,4,4,5>": ("gemm_stream", "_ZN4dsse16gemm_ring_kernelILi4ELi4ELi4ELi5ELb0EEEv", 14),
    "ring gate_up <4,7,3,3>": ("gemm_stream", "_ZN4dsse16gemm_ring_kernelILi4ELi7ELi3ELi3ELb0EEEv", 14),
    "ring lm_head <4,8,3,1>": ("gemm_stream", "_ZN4dsse16gemm_ring_kernelILi4ELi8ELi3ELi1ELb0EEEv", 14),
    # work_seq work_tile q_len ctx_len q_start block_tables (2 each) max_blocks nparts: the dependent-load chain
    "attention fold <1,2,1,4>": ("attention", "_ZN4dsse22paged_attention_kernelILi1ELi2ELi1ELi4EDF16bEEv", 14),
    # resid part w ids embed (2 each) nt nit nsplit M
    "rmsnorm<2>": ("elementwise", "_ZN4dsse14rmsnorm_kernelILi2EEEv", 14),
    "rmsnorm<3>": ("elementwise", "_ZN4dsse14rmsnorm_kernelILi3EEEv", 14),
    # B pad active positions block_tables (2 each) max_blocks num_blocks
    "decode_prep": ("elementwise", "_ZN4dsse18decode_prep_kernelE", 10),
    "ring_advance": ("elementwise", "_ZN4dsse19ring_advance_kernelE", 2),  # counter(2)
    # active temperature top_k top_p logits min_p (2 each) ld V
    "sample_chunk": ("sampler", "_ZN4dsse19sample_chunk_kernelE", 14),
    "sample_filtered": ("sampler", "_ZN4dsse22sample_filtered_kernelE", 14),
    # cand(2) world B nchunks pad active(2)
    "sample_pick": ("sampler", "_ZN4dsse18sample_pick_kernelE", 8),
}


def _compile(hipcc: str, src: Path, out: Path, variant):
    cmd = [hipcc, *_build.kernel_device_flags(variant), "-w", "-S", "--cuda-device-only", str(src), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, f"{' '.join(cmd)}\n{res.stderr[-4000:]}"
    return out.read_text()


def _parse(asm: str):
    """{kernel symbol: (preload length, [value_kind of every argument])} from the descriptors and the metadata."""
    preload = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        pl = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", m.group(2))
        preload[m.group(1)] = int(pl.group(1)) if pl else 0
    meta = asm[asm.index("amdhsa.kernels:"):]
    meta = meta[: meta.index(".end_amdgpu_metadata")]
    kinds = {}
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)
        kinds[name] = re.findall(r"\.value_kind:\s+(\S+)", entry)
    assert set(kinds) == set(preload) and preload, "descriptor and metadata kernel lists differ"
    return {k: (preload[k], kinds[k]) for k in preload}


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or (_build.HIPCC if Path(_build.HIPCC).exists() else None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("kernel_entry")
    kdir = _build.CSRC / "kernels"
    jobs = {(f, v): (kdir / f"{f}.hip", out / f"{f}_{v}.s", v) for f in FILES for v in (None,)}
    jobs[("elementwise", "nopreload")] = (kdir / "elementwise.hip", out / "elementwise_nopreload.s", "nopreload")
    with cf.ThreadPoolExecutor(len(jobs)) as ex:
        futs = {k: ex.submit(_compile, hipcc, *a) for k, a in jobs.items()}
        return {k: _parse(f.result()) for k, f in futs.items()}


def _find(parsed, prefix):
    hits = [k for k in parsed if k.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {len(hits)} kernels"
    return parsed[hits[0]]


@pytest.mark.parametrize("kernel", sorted(ENTRY))
def test_entry_operands_are_preloaded(device_asm, kernel):
    f, prefix, need = ENTRY[kernel]
    length, _ = _find(device_asm[(f, None)], prefix)
    assert length >= need, f"{kernel}: {length} dwords preloaded, its entry needs {need}"


@pytest.mark.parametrize("kernel", sorted(ENTRY))
def test_no_hidden_grid_or_block_argument(device_asm, kernel):
    f, prefix, _ = ENTRY[kernel]
    _, kinds = _find(device_asm[(f, None)], prefix)
    bad = [k for k in kinds if k.startswith("hidden_block_count") or k.startswith("hidden_group_size")]
    assert not bad, f"{kernel} reads {bad}: pass the value as a leading argument or make it a constant"


def test_nopreload_variant_preloads_nothing(device_asm):
    for sym, (length, _) in device_asm[("elementwise", "nopreload")].items():
        assert length == 0, sym
