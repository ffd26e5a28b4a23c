"""Cost of guided decoding when used (the numbers of profiles/r10/guided_decoding.md).

    python tools/bench_guided.py [--model mistral-7b] [--streams 64] [--ctx 512] [--reps 100]

1. The mask pass alone at `--streams` rows x V = 32768 over the synthetic vocabulary: every row off, every row at the
   start of a 512-state pattern that keeps most words alive (long walks), every row in a state that kills every token at
   its first byte; the live pass of that table; device events around `--reps` back-to-back launches after a warm-up.
2. The `--streams`-stream decode step of `--model` (random-init weights, garbage KV at `--ctx` tokens of context): the
   graphs captured at startup, then the lazily captured twins (their one-off capture time is printed) with every
   stream unguided and with every stream guided by the 512-state pattern (the advance pass moves the states as the
   step samples).
3. JSON mode (response_format json_object), in the same session: the mask pass alone with every row a JSON row at the
   start state, inside a string (the most permissive state) and at depth 64, over the synthetic vocabulary with 64 of
   its pieces replaced by JSON punctuation and fragments (the synthetic tokenizer has no braces); and the decode step
   with every stream in JSON mode on the runner's own (brace-less) table: inside a string, and stuck at the start state.
With --wide, instead of all that and without a model: the mask pass, the advance pass and the one-off live pass for a
4096-state table in the wide pool of schema guides (2 MiB, ops.guide_attach_wide) beside the same passes for the
512-state narrow pattern, at `--streams` rows x V = 32768, rows spread over the table's states (the numbers of
profiles/guided_json.md).
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERN = "[a-z ]{255}[a-z ]{255}[a-z ]"  # 512 states; every lower-case word of the vocabulary survives
DIGITS = "[0-9]{255}[0-9]{255}[0-9]"      # 512 states; all but ten tokens die at their first byte
# about 4050 states under the wide caps: 16 chains of 253 that do not merge (each ends in its own letter); inside a
# chain every lower-case word survives, as with PATTERN
WIDE_PATTERN = "|".join(c + "[a-z ]{251}" + c for c in "abcdefghijkmnprs")
JSON_PIECES = ["{", "}", "[", "]", '"', ":", ",", "\n", " ", "-", ".", "e", "E", "+", "true", "false", "null", '{"', '":',
               '",', '"}', "}}", "]}", "[[", '":"', '": "', '", "', "},{", "{}", "[]", "\\n", '\\"', "\\u00e9", "é",
               '":[', '":{', "}]", "]]", "],", "},", '"]', '"],', '":true', '":null', "\n  ", "\n    ", "1.5", "1e3", "-1",
               "0.", '{"a":', '{"id":', '"name":', '"value":', "[1,", ",2", "2]", '["', '"]}', "}}}", "]]}", " :", " ,",
               "\t"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--wide", action="store_true", help="time the guide passes for a 4096-state wide entry only")
    a = ap.parse_args()

    import numpy as np
    import torch

    from distributed_sse_for_llm_response_amd import ops, runtime
    from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
    from distributed_sse_for_llm_response_amd.engine.weights import random_engine_weights
    from distributed_sse_for_llm_response_amd.models.mistral import get_config
    from distributed_sse_for_llm_response_amd.models.tokenizer import SyntheticTokenizer

    ops.load_library(required=True)
    dev = torch.device("cuda", 0)

    def compiled(pattern):
        n, tab, acc = runtime.load().guide_compile(pattern)
        return np.frombuffer(tab, dtype=np.uint16).reshape(n, 256), np.frombuffer(acc, dtype=np.uint8)

    def timed_us(fn, n=a.reps, warm=10):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) / n * 1e3, 1)

    cfg = get_config(a.model)
    tok = SyntheticTokenizer(cfg.vocab_size)
    if a.wide:
        B, V = a.streams, cfg.vocab_size
        tb, tl = (t.to(dev) for t in ops.guide_token_table(tok.pieces(), never={0, tok.eos_id}))
        n, tab, acc = runtime.load().guide_compile_wide(WIDE_PATTERN)
        wide = (np.frombuffer(tab, dtype=np.uint16).reshape(n, 256), np.frombuffer(acc, dtype=np.uint8))
        gt = torch.full((1, ops.GUIDE_STATES, 256), -1, device=dev, dtype=torch.int16)
        gf = torch.zeros(1, ops.GUIDE_STATES, device=dev, dtype=torch.int32)
        wt = torch.full((1, ops.GUIDE_WIDE_STATES, 256), -1, device=dev, dtype=torch.int16)
        wf = torch.zeros(1, ops.GUIDE_WIDE_STATES, device=dev, dtype=torch.int32)
        meta = ops.guide_attach_wide(torch.zeros(2 * B, device=dev, dtype=torch.int32), wt, wf)
        res = {"what": "guide passes, narrow 512-state entry against wide 4096-state entry", "rows": B, "V": V}
        x = (torch.randn(B, V, device=dev) * 4).clamp_(-32, 32)
        ids = torch.full((B,), tok.encode("ba", add_bos=False)[0], device=dev, dtype=torch.int32)
        for name, (t, f), tabs, flgs, entry in (("narrow", compiled(PATTERN), gt, gf, 0),
                                                ("wide", wide, wt, wf, ops.GUIDE_POOL)):
            k = t.shape[0]
            tabs[0, :k] = torch.from_numpy(t.view(np.int16).copy()).to(dev)
            flgs[0, :k] = torch.from_numpy(f.astype(np.int32)).to(dev)
            res[f"{name}_states"] = k
            res[f"{name}_live_pass_us"] = timed_us(
                lambda: ops.guide_live(tb, tl, gt, gf, meta, entry, k, tok.eos_id), n=10, warm=2)
            m = torch.zeros(2 * B, dtype=torch.int32)
            m[:B] = entry
            for spread, states in (("start", torch.zeros(B)), ("spread", 1 + torch.arange(B) * ((k - 16) // B))):
                m[B:] = states.to(torch.int32)
                dm = m.to(dev)

                def mask():
                    meta.copy_(dm)
                    ops.guide_mask(x.copy_(x.clamp(min=-32)), None, tb, tl, gt, gf, meta, None, 0, tok.eos_id)

                def advance():
                    meta.copy_(dm)
                    ops.guide_advance(ids, None, tb, tl, gt, gf, meta, None, tok.eos_id)

                res[f"{name}_mask_{spread}_us"] = timed_us(mask)
                res[f"{name}_advance_{spread}_us"] = timed_us(advance)
        res["row_restore_and_meta_upload_alone_us"] = timed_us(lambda: (meta.copy_(dm), x.copy_(x.clamp(min=-32))))
        print(json.dumps(res), flush=True)
        return
    w = random_engine_weights(cfg, device=dev, seed=0)
    B = a.streams
    pages = a.ctx // 32 + 2
    r = ModelRunner(w, num_blocks=B * pages + 8, max_batch=B, max_model_len=a.ctx + 64, device=dev)
    r.set_guide_vocab(tok.pieces(), tok.eos_id)
    for s in range(B):
        r.block_tables[s, :pages] = torch.arange(pages * s, pages * (s + 1), dtype=torch.int32)
    r.active.fill_(1)
    r.capture([B])

    def step_us():
        r.positions.fill_(a.ctx)  # (every replay advances the positions: keep the context fixed)
        return timed_us(lambda: r.decode(B), warm=5, n=min(a.reps, 50))

    out = {"what": "decode step", "model": cfg.name, "streams": B, "ctx": a.ctx, "V_local": w.vocab_local,
           "startup_graphs_us": step_us()}
    r.temperature.fill_(1.0)  # (guided streams sample: their baseline is the sampling step)
    out["startup_graphs_temperature_1_us"] = step_us()
    r.enable_guides()
    out["twin_capture_s"] = round(r.twin_capture_s, 2)
    out["twins_all_unguided_us"] = step_us()
    r.upload_guide(0, *compiled(PATTERN))
    r.upload_guide(1, *compiled(DIGITS))

    def guide_all(entry, state=0):
        m = torch.zeros(2 * B, dtype=torch.int32)
        m[:B], m[B:] = entry, state
        r.guide_meta.copy_(m)

    # the mask pass alone, on the runner's own tables
    x = (torch.randn(B, cfg.vocab_size, device=dev) * 4).clamp_(-32, 32)
    alone = {"what": "mask pass alone", "rows": B, "V": cfg.vocab_size}
    guide_all(-1)
    alone["all_off_us"] = timed_us(lambda: r._guide_mask(x, None, None))
    guide_all(0)
    alone["all_words_survive_us"] = timed_us(lambda: r._guide_mask(x.copy_(x.clamp(min=-32)), None, None))
    alone["row_restore_alone_us"] = timed_us(lambda: x.copy_(x.clamp(min=-32)))
    guide_all(1)
    alone["all_die_at_first_byte_us"] = timed_us(lambda: r._guide_mask(x, None, None))
    alone["live_pass_512_states_us"] = timed_us(
        lambda: ops.guide_live(r.tok_bytes, r.tok_len, r.guide_tab, r.guide_flags, r.guide_meta, 0, 512, r.guide_eos),
        n=10, warm=2)
    print(json.dumps(alone), flush=True)

    def guided_step_us(entry):
        def fn():
            guide_all(entry)  # (back to the start state: the advance pass moved it)
            r.decode(B)
        r.positions.fill_(a.ctx)
        return timed_us(fn, warm=5, n=min(a.reps, 50))

    out["twins_all_guided_words_us"] = guided_step_us(0)
    out["twins_all_guided_digits_us"] = guided_step_us(1)
    guide_all(-1)
    out["twins_all_unguided_with_meta_upload_us"] = guided_step_us(-1)
    print(json.dumps(out), flush=True)

    # JSON mode: every row a pushdown row of the same two launches
    assert len(JSON_PIECES) == 64
    pieces = tok.pieces()
    pieces[3:3 + len(JSON_PIECES)] = JSON_PIECES
    jtb, jtl = (t.to(dev) for t in ops.guide_token_table(pieces, never={0, tok.eos_id}))
    states = {"start": ops.JSON_START_STATE, "in_string": ops.json_walk(b'{"k":"'),
              "depth_64": ops.json_walk(b'{"a":' * ops.JSON_DEPTH)}

    def json_all(state):
        m = torch.zeros(2 * B, dtype=torch.int32)
        m[:B] = ops.JSON_ENTRY
        r.guide_meta.copy_(m)
        r.json_state.copy_(torch.tensor(ops.json_state_words(state), dtype=torch.int32).repeat_interleave(B))

    def json_mask(tb, tl):
        ops.guide_mask(x.copy_(x.clamp(min=-32)), None, tb, tl, r.guide_tab, r.guide_flags, r.guide_meta, None, 0,
                       r.guide_eos)  # (r.guide_meta carries json_tab / json_state: ops.guide_attach_json)

    jm = {"what": "JSON mask pass alone (each figure includes the row restore)", "rows": B, "V": cfg.vocab_size,
          "json_pieces": len(JSON_PIECES), "row_restore_alone_us": timed_us(lambda: x.copy_(x.clamp(min=-32)))}
    for name, state in states.items():
        json_all(state)
        jm[f"{name}_us"] = timed_us(lambda: json_mask(jtb, jtl))
        jm[f"{name}_survivors"] = int((ops.json_walk_all(state, jtb.cpu().numpy(), jtl.cpu().numpy())[0]
                                       != ops.GUIDE_DEAD).sum())
    json_all(states["in_string"])
    jm["in_string_brace_less_vocabulary_us"] = timed_us(lambda: json_mask(r.tok_bytes, r.tok_len))
    print(json.dumps(jm), flush=True)

    def json_step_us(state):
        def fn():
            json_all(state)  # (back to the same state: the advance pass moved it)
            r.decode(B)
        r.positions.fill_(a.ctx)
        return timed_us(fn, warm=5, n=min(a.reps, 50))

    js = {"what": "decode step, every stream in JSON mode (the runner's brace-less table)", "model": cfg.name,
          "streams": B, "in_string_us": json_step_us(states["in_string"]),
          "stuck_at_start_us": json_step_us(states["start"])}
    guide_all(-1)
    js["all_unguided_with_meta_upload_us"] = guided_step_us(-1)
    print(json.dumps(js), flush=True)


if __name__ == "__main__":
    main()
