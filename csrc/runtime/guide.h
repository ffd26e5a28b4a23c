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
// A schema guide (guided_json / response_format json_schema) compiles under caps of its own, eight times the above:
// bounded strings, bounded arrays and optional members multiply states.
constexpr int kGuideWideStates = 4096;
constexpr int kGuideWideNfaStates = 8 * kGuideNfaStates;
constexpr long kGuideWideWork = 8 * kGuideWork;
constexpr int kGuideSchemaBytes = 8192;    // schema text bytes at most

struct Dfa {
  int n_states = 0;
  std::vector<uint16_t> table;   // [n_states][256]; start state 0; kGuideDead = dead
  std::vector<uint8_t> accept;   // [n_states]: 1 = accepting
};

// Compile `pattern`.  On success: true and *out is trimmed (every state reaches an accepting state; transitions into
// states that do not are dead).  On failure: false and *err names the construct or limit and the offset.
bool compile(std::string_view pattern, Dfa* out, std::string* err);

// The schema guide's entry point: the same compiler under the wide caps (kGuideWideStates, kGuideWideNfaStates,
// kGuideWideWork).  It also reads one escape that compile() rejects, \xHH = the byte HH, alone or as a class member
// or range end: schema_pattern writes JSON's UTF-8 string body with it (a pattern travels as text, so it cannot hold
// the raw bytes).  Python's re reads \xHH as a code point, so the two still agree on ASCII subjects.
bool compile_wide(std::string_view pattern, Dfa* out, std::string* err);

// A JSON Schema lowered to a pattern for compile_wide.  The language is the COMPACT serialisation of the instances:
// no whitespace between tokens, object members in the order of `properties` (optional ones may be absent), strings
// as valid UTF-8 with one escape per code point.  Every string it accepts parses as JSON and validates against the
// schema; it is complete only for that compact form.  Subset (docs/kernels.md, "Sampler"): type (a list = an
// alternation); object with properties / required / additionalProperties false; array with items and minItems /
// maxItems <= 16; string with minLength / maxLength <= 64 (code points); integer / number; enum / const of scalars;
// anyOf, and oneOf over branches of pairwise different types; $ref to #/$defs/<name> or #/definitions/<name>,
// inlined.  title, description, default, examples, $schema, $id are ignored.  Anything else is an error that names
// the keyword and its JSON pointer; so are a recursive $ref, a schema above kGuideSchemaBytes and a pattern above
// kGuidePatternBytes.
bool schema_pattern(std::string_view schema_json, std::string* pattern, std::string* err);

// How schema_pattern's error ends when the schema itself (pointer #) is an object without `properties`: any JSON
// object, which is what response_format json_object gives and a schema guide does not.
constexpr char kSchemaFreeFormRoot[] =
    "'type' at # (an object without 'properties': free-form values belong to json_object)";

// guided_choice lowered to one pattern: the alternation of the choices with every metacharacter escaped.
std::string choice_pattern(const std::vector<std::string>& choices);

}  // namespace guide
