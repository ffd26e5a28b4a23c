"""Stop strings: the `stop` field of a request, matched on the decoded text of its completion.

The engine samples token ids; the text exists only where token events are published (the serving loop of a single
replica, a TP leader, each DP worker), so the matcher sits in that path: ``StopMatcher.filter`` takes the engine's
events of one publish call and returns the events to deliver.

* Matching runs on the concatenated pieces of the delivered and held tokens and may span token boundaries.  The
  delivered text ends just before the earliest match; the stream ends with a terminal frame (finish "stop") that takes
  the next sequence number, and the conversation is reported by ``pop_aborts`` so that the loop aborts the sequence in
  the engine (slot and KV pages freed).  Whatever the engine still publishes for it, its own terminal frame included,
  is dropped.
* Hold-back: a token frame is held only while a suffix of the text that starts inside it (or before it) is a proper
  prefix of some stop string, i.e. while a match could still begin there.  It goes out as soon as that is ruled out.
* On a match the token that straddles the match start is delivered with its text truncated (``TokenEvent.text``);
  tokens that start at or after the match are dropped together with their logprob entries.
* A stream that ends by itself (EOS, a stop token, length, an error) gets its held frames before the terminal frame.
* Nothing is matched while fewer than ``min_tokens`` tokens exist; those tokens are delivered at once and a match
  never starts inside them.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

from ..engine.engine import TokenEvent

MAX_STOP = 4  # stop strings per request (the HTTP server enforces it)


@dataclass
class _Stream:
    stops: tuple
    min_tokens: int
    prompt_tokens: int
    text: str = ""          # the completion so far: delivered + held
    open_at: int = 0        # a match may start at this offset at the earliest (end of the text that is final)
    held: list = field(default_factory=list)  # [(event, start offset of its piece in text)]
    tokens: int = 0
    last_seq: int = 0       # sequence number of the newest token frame seen


class StopMatcher:
    def __init__(self, piece):
        self.piece = piece            # token id -> text
        self.streams: dict = {}       # conversation id -> _Stream
        self.closed: set = set()      # ended here by a match; the engine's remaining events are dropped
        self._aborts: list = []

    def register(self, conversation_id: str, stops, min_tokens: int = 0, prompt_tokens: int = -1) -> None:
        stops = tuple(s for s in (stops or ()) if s)[:MAX_STOP]
        if stops:
            self.streams[conversation_id] = _Stream(stops, max(0, int(min_tokens)), int(prompt_tokens))

    def pop_aborts(self) -> list:
        out, self._aborts = self._aborts, []
        return out

    def filter(self, events: list) -> list:
        if not self.streams and not self.closed:
            return events
        out = []
        for e in events:
            if e.conversation_id in self.closed:
                if e.done:  # the engine's own terminal frame (the abort's): the conversation is gone
                    self.closed.discard(e.conversation_id)
                continue
            st = self.streams.get(e.conversation_id)
            if st is None:
                out.append(e)
            elif e.done:
                out += [h for h, _ in st.held]
                out.append(e)
                del self.streams[e.conversation_id]
            else:
                self._token(st, e, out)
        return out

    def _token(self, st: _Stream, e: TokenEvent, out: list) -> None:
        piece = e.text or self.piece(e.token_id)
        start = len(st.text)
        st.text += piece
        st.tokens += 1
        st.last_seq = e.sequence
        if st.tokens <= st.min_tokens:  # not matched yet: delivered, and no later match may reach into it
            out.append(e)
            st.open_at = len(st.text)
            return
        st.held.append((e, start))
        # the earliest match that ends inside the new piece (earlier text was searched when it arrived)
        at = -1
        for s in st.stops:
            i = st.text.find(s, max(st.open_at, start - len(s) + 1))
            if i >= 0 and (at < 0 or i < at):
                at = i
        if at >= 0:
            for h, h0 in st.held:
                if h0 >= at:
                    break
                if h0 + len(h.text or self.piece(h.token_id)) > at:  # straddles the match start: truncated
                    h.text = st.text[h0:at]
                out.append(h)
                st.last_seq = h.sequence
            else:
                st.last_seq = st.held[-1][0].sequence
            first_dropped = next((h.sequence for h, h0 in st.held if h0 >= at), st.last_seq + 1)
            out.append(TokenEvent(e.conversation_id, -1, first_dropped, True, text="[DONE]",
                                  timestamp_ns=time.time_ns(), finish="stop", prompt_tokens=st.prompt_tokens))
            del self.streams[e.conversation_id]
            self.closed.add(e.conversation_id)
            self._aborts.append(e.conversation_id)
            return
        # hold from the earliest offset at which a match could still begin; everything before it is final
        n, keep = len(st.text), len(st.text)
        longest = max(len(s) for s in st.stops)
        for i in range(max(st.open_at, n - longest + 1), n):
            tail = st.text[i:]
            if any(len(s) > len(tail) and s.startswith(tail) for s in st.stops):
                keep = i
                break
        while st.held and st.held[0][1] + len(st.held[0][0].text or self.piece(st.held[0][0].token_id)) <= keep:
            out.append(st.held.pop(0)[0])
        st.open_at = st.held[0][1] if st.held else n
