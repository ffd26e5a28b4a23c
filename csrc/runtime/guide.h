// Guided decoding: a byte-level regular expression compiled to a DFA table (guided_regex / guided_choice).
//
// One implementation serves both users: the HTTP routes validate a request's pattern with it (a bad pattern is a 400
// before the stream opens) and the engine process builds the device's transition table from it.
//
// Syntax (full-match semantics, bytes): literals (a non-ASCII UTF-8 literal is its byte sequence); `.` = any byte but
// \n; the escapes \d \D \w \W \s \S \n \t \r and escaped punctuation; classes [...] / [^...] with ranges (ASCII
// members only); groups (...) and (?:...); alternation |; the quantifiers * + ? {m} {m,} {m,n} with bounds <= 255.
// Everything else (anchors, back-references, look-around, lazy / possessive quantifiers, named groups, flags, other
// escapes) is rejected with a message that names the construct and its byte offset.  For ASCII subjects the language is
// that of Python's re.fullmatch on the same pattern (\s = [ \t\n\r\f\v]).
#pragma once

#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace guide {

constexpr int kGuideStates = 512;          // DFA states of a compiled pattern at most (what is returned)
constexpr int kGuidePatternBytes = 8192;   // pattern bytes at most, as carried
constexpr int kGuideNfaStates = 16384;     // NFA states at most (quantifiers are expanded)
constexpr long kGuideWork = 1L << 22;      // NFA-state visits of the subset construction at most
constexpr uint16_t kGuideDead = 0xFFFF;    // "no transition"

struct Dfa {
  int n_states = 0;
  std::vector<uint16_t> table;   // [n_states][256]; start state 0; kGuideDead = dead
  std::vector<uint8_t> accept;   // [n_states]: 1 = accepting
};

// Compile `pattern`.  On success: true and *out is trimmed (every state reaches an accepting state; transitions into
// states that do not are dead).  On failure: false and *err names the construct or limit and the offset.
bool compile(std::string_view pattern, Dfa* out, std::string* err);

// guided_choice lowered to one pattern: the alternation of the choices with every metacharacter escaped.
std::string choice_pattern(const std::vector<std::string>& choices);

}  // namespace guide
