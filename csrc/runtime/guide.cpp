// Pattern compiler of guided decoding (guide.h): parse -> Thompson NFA (quantifiers expanded) -> subset construction
// over byte classes -> trim.  Every limit is an error, never a truncation; the NFA and work caps bound what a hostile
// pattern can cost.
#include "guide.h"

#include <algorithm>
#include <array>
#include <bitset>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <map>
#include <memory>

namespace guide {
namespace {

using Set = std::bitset<256>;

struct Fail {
  std::string msg;
};

[[noreturn]] void fail(const std::string& what, size_t at) {
  throw Fail{"guide pattern: " + what + " at offset " + std::to_string(at)};
}

struct Node {
  enum Kind { kSet, kCat, kAlt, kRep } kind = kCat;
  Set set;                                    // kSet
  std::vector<std::unique_ptr<Node>> kids;    // kCat / kAlt; kRep: one
  int lo = 0, hi = 0;                         // kRep: hi = -1 -> unbounded
  size_t at = 0;                              // kRep: offset of the quantifier
};
using NodeP = std::unique_ptr<Node>;

constexpr int kMaxNest = 100;

Set range_set(int lo, int hi) {
  Set s;
  for (int c = lo; c <= hi; ++c) s.set((size_t)c);
  return s;
}

// \d \w \s and their complements; false = `c` is none of them
bool shorthand(char c, Set* out) {
  Set s;
  switch (c | 0x20) {
    case 'd': s = range_set('0', '9'); break;
    case 'w': s = range_set('0', '9') | range_set('a', 'z') | range_set('A', 'Z'); s.set('_'); break;
    case 's': for (char k : {' ', '\t', '\n', '\r', '\f', '\v'}) s.set((size_t)k); break;
    default: return false;
  }
  if (c != 'd' && c != 'w' && c != 's' && c != 'D' && c != 'W' && c != 'S') return false;
  *out = (c & 0x20) ? s : ~s;
  return true;
}

bool is_punct(unsigned char c) { return c < 0x80 && c > ' ' && c != 0x7f && !isalnum(c); }

// What one compilation may cost and accept: compile() and compile_wide() differ in nothing else.
struct Limits {
  int max_states;     // states of the DFA returned at most
  int raw_states;     // states of the subset construction at most (above max_states only where `minimize`)
  int nfa_states;
  long work;
  bool minimize;      // merge equivalent states after the trim
  bool byte_escapes;  // \xHH = the byte HH (schema lowering writes UTF-8 ranges with it)
};
constexpr Limits kNarrow{kGuideStates, kGuideStates, kGuideNfaStates, kGuideWork, false, false};
constexpr Limits kWide{kGuideWideStates, 4 * kGuideWideStates, kGuideWideNfaStates, kGuideWideWork, true, true};

int hex_val(unsigned char c) {
  if (c >= '0' && c <= '9') return c - '0';
  c |= 0x20;
  return c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
}

struct Parser {
  std::string_view p;
  bool byte_escapes = false;
  size_t i = 0;
  int depth = 0;

  bool more() const { return i < p.size(); }
  unsigned char cur() const { return (unsigned char)p[i]; }

  // escape after the backslash at offset `at` (i is on the escaped byte): a single byte or a shorthand set
  Set escape(size_t at, bool* single, int* byte) {
    if (!more()) fail("trailing backslash", at);
    const unsigned char c = cur();
    ++i;
    Set s;
    *single = false;
    if (shorthand((char)c, &s)) return s;
    *single = true;
    if (c == 'n') *byte = '\n';
    else if (c == 't') *byte = '\t';
    else if (c == 'r') *byte = '\r';
    else if (is_punct(c)) *byte = c;
    else if (c == 'x' && byte_escapes) {
      if (i + 1 >= p.size() || hex_val((unsigned char)p[i]) < 0 || hex_val((unsigned char)p[i + 1]) < 0)
        fail("malformed byte escape \\x", at);
      *byte = hex_val((unsigned char)p[i]) * 16 + hex_val((unsigned char)p[i + 1]);
      i += 2;
    } else if (c >= '0' && c <= '9') fail(std::string("back-reference or octal escape \\") + (char)c, at);
    else if (c == 'b' || c == 'B' || c == 'A' || c == 'Z' || c == 'z' || c == 'G') fail(std::string("anchor \\") + (char)c, at);
    else if (c >= 0x80) fail("escaped non-ASCII byte", at);
    else fail(std::string("unsupported escape \\") + (char)c, at);
    s.set((size_t)*byte);
    return s;
  }

  NodeP leaf(const Set& s) {
    auto n = std::make_unique<Node>();
    n->kind = Node::kSet;
    n->set = s;
    return n;
  }

  NodeP klass() {  // i is just past '['
    const size_t at = i - 1;
    bool neg = false;
    if (more() && cur() == '^') { neg = true; ++i; }
    Set s;
    bool first = true;
    while (true) {
      if (!more()) fail("unterminated class [", at);
      unsigned char c = cur();
      if (c == ']' && !first) { ++i; break; }
      first = false;
      const size_t mat = i;
      ++i;
      bool single = true;
      int lo = c;
      if (c == '\\') {
        Set e = escape(mat, &single, &lo);
        if (!single) { s |= e; continue; }
      } else if (c >= 0x80) {
        fail("non-ASCII class member", mat);
      } else if (c == '[' && more() && cur() == ':') {
        fail("POSIX class [:", mat);
      }
      if (i + 1 < p.size() && p[i] == '-' && p[i + 1] != ']') {  // a range lo-hi
        ++i;
        const size_t hat = i;
        unsigned char h = cur();
        ++i;
        int hi = h;
        if (h == '\\') {
          bool hs = true;
          escape(hat, &hs, &hi);
          if (!hs) fail("class shorthand as a range end", hat);
        } else if (h >= 0x80) {
          fail("non-ASCII class member", hat);
        }
        if (hi < lo) fail("reversed class range", mat);
        s |= range_set(lo, hi);
      } else {
        s.set((size_t)lo);
      }
    }
    return leaf(neg ? ~s : s);
  }

  NodeP atom() {
    const size_t at = i;
    const unsigned char c = cur();
    ++i;
    switch (c) {
      case '(': {
        if (more() && cur() == '?') {
          if (i + 1 < p.size() && p[i + 1] == ':') {
            i += 2;
          } else {
            const char k = i + 1 < p.size() ? p[i + 1] : ' ';
            const char k2 = i + 2 < p.size() ? p[i + 2] : ' ';
            if (k == '=' || k == '!' || (k == '<' && (k2 == '=' || k2 == '!'))) fail("look-around (?" + std::string(1, k), at);
            if (k == 'P' || k == '<') fail("named group or named reference (?" + std::string(1, k), at);
            if (k == '#') fail("comment group (?#", at);
            fail("inline flag or extension group (?" + std::string(1, k), at);
          }
        }
        if (++depth > kMaxNest) fail("groups nested deeper than " + std::to_string(kMaxNest), at);
        NodeP n = alt();
        --depth;
        if (!more() || cur() != ')') fail("unterminated group (", at);
        ++i;
        return n;
      }
      case ')': fail("unbalanced )", at);
      case '[': return klass();
      case '.': { Set s; s.set(); s.reset('\n'); return leaf(s); }
      case '^': fail("anchor ^", at);
      case '$': fail("anchor $", at);
      case '*': case '+': case '?': fail(std::string("quantifier ") + (char)c + " with nothing to repeat", at);
      case '{': fail("unescaped {", at);
      case '\\': {
        bool single;
        int b;
        return leaf(escape(at, &single, &b));
      }
      default: {
        Set s;
        s.set(c);
        if (c < 0xC0 || !more() || (cur() & 0xC0) != 0x80) return leaf(s);
        // a non-ASCII UTF-8 literal: its byte sequence, as one atom (a quantifier repeats the whole character)
        auto n = std::make_unique<Node>();
        n->kind = Node::kCat;
        n->kids.push_back(leaf(s));
        while (more() && (cur() & 0xC0) == 0x80) {
          Set t;
          t.set(cur());
          n->kids.push_back(leaf(t));
          ++i;
        }
        return n;
      }
    }
  }

  // a quantifier at i, if any: wraps `n`
  NodeP quantified(NodeP n) {
    if (!more()) return n;
    const size_t at = i;
    const unsigned char c = cur();
    int lo, hi;
    if (c == '*') { lo = 0; hi = -1; ++i; }
    else if (c == '+') { lo = 1; hi = -1; ++i; }
    else if (c == '?') { lo = 0; hi = 1; ++i; }
    else if (c == '{') {
      size_t j = i + 1;
      auto number = [&](int* v) {
        size_t k = j;
        long x = 0;
        while (j < p.size() && p[j] >= '0' && p[j] <= '9' && j - k < 6) x = x * 10 + (p[j++] - '0');
        *v = (int)x;
        return j > k;
      };
      if (!number(&lo)) fail("quantifier { without a lower bound", at);
      hi = lo;
      if (j < p.size() && p[j] == ',') {
        ++j;
        if (!number(&hi)) hi = -1;
      }
      if (j >= p.size() || p[j] != '}') fail("malformed quantifier {", at);
      i = j + 1;
      if (lo > 255 || hi > 255) fail("quantifier bound above 255", at);
      if (hi >= 0 && hi < lo) fail("quantifier {m,n} with n < m", at);
    } else {
      return n;
    }
    if (more()) {
      if (cur() == '?') fail("lazy quantifier", i);
      if (cur() == '+') fail("possessive quantifier", i);
      if (cur() == '*' || cur() == '{') fail("quantifier on a quantifier", i);
    }
    auto r = std::make_unique<Node>();
    r->kind = Node::kRep;
    r->lo = lo;
    r->hi = hi;
    r->at = at;
    r->kids.push_back(std::move(n));
    return r;
  }

  NodeP cat() {
    auto n = std::make_unique<Node>();
    n->kind = Node::kCat;
    while (more() && cur() != '|' && cur() != ')') n->kids.push_back(quantified(atom()));
    return n;
  }

  NodeP alt() {
    NodeP first = cat();
    if (!more() || cur() != '|') return first;
    auto n = std::make_unique<Node>();
    n->kind = Node::kAlt;
    n->kids.push_back(std::move(first));
    while (more() && cur() == '|') {
      ++i;
      n->kids.push_back(cat());
    }
    return n;
  }
};

struct Nfa {
  struct State {
    int set = -1, out = -1;    // byte edge: sets[set] -> out
    std::vector<int> eps;
  };
  std::vector<State> st;
  std::vector<Set> sets;       // distinct byte sets
  size_t quant_at = 0;
  int cap = kGuideNfaStates;

  int add() {
    if ((int)st.size() >= cap)
      fail("pattern too large: more than " + std::to_string(cap) + " NFA states, expanding the quantifier", quant_at);
    st.emplace_back();
    return (int)st.size() - 1;
  }
  int set_id(const Set& s) {
    for (size_t k = 0; k < sets.size(); ++k)
      if (sets[k] == s) return (int)k;
    sets.push_back(s);
    return (int)sets.size() - 1;
  }

  // emits `n` between a fresh start and end state
  std::pair<int, int> emit(const Node& n) {
    switch (n.kind) {
      case Node::kSet: {
        const int s = add(), e = add();
        st[s].set = set_id(n.set);
        st[s].out = e;
        return {s, e};
      }
      case Node::kCat: {
        const int s = add();
        int e = s;
        for (auto& k : n.kids) {
          auto f = emit(*k);
          st[e].eps.push_back(f.first);
          e = f.second;
        }
        return {s, e};
      }
      case Node::kAlt: {
        const int s = add(), e = add();
        for (auto& k : n.kids) {
          auto f = emit(*k);
          st[s].eps.push_back(f.first);
          st[f.second].eps.push_back(e);
        }
        return {s, e};
      }
      case Node::kRep: {
        const size_t saved = quant_at;
        if (n.at >= quant_at) quant_at = n.at;  // (names the last quantifier in the pattern among those being expanded)
        const int s = add();
        int e = s;
        for (int k = 0; k < n.lo; ++k) {
          auto f = emit(*n.kids[0]);
          st[e].eps.push_back(f.first);
          e = f.second;
        }
        if (n.hi < 0) {  // e -> loop -> (child -> loop)* -> end
          const int loop = add(), end = add();
          auto f = emit(*n.kids[0]);
          st[e].eps.push_back(loop);
          st[loop].eps.push_back(f.first);
          st[f.second].eps.push_back(loop);
          st[loop].eps.push_back(end);
          e = end;
        } else if (n.hi > n.lo) {
          const int end = add();
          for (int k = n.lo; k < n.hi; ++k) {
            auto f = emit(*n.kids[0]);
            st[e].eps.push_back(f.first);
            st[e].eps.push_back(end);
            e = f.second;
          }
          st[e].eps.push_back(end);
          e = end;
        }
        quant_at = saved;
        return {s, e};
      }
    }
    return {0, 0};
  }
};

bool compile_with(std::string_view pattern, Dfa* out, std::string* err, const Limits& lim) {
  try {
    if (pattern.size() > (size_t)kGuidePatternBytes)
      throw Fail{"guide pattern: longer than " + std::to_string(kGuidePatternBytes) + " bytes"};
    Parser ps{pattern, lim.byte_escapes};
    NodeP root = ps.alt();
    if (ps.more()) fail("unbalanced )", ps.i);
    Nfa nfa;
    nfa.cap = lim.nfa_states;
    const auto se = nfa.emit(*root);
    const int final_state = se.second;
    const int N = (int)nfa.st.size();

    // byte classes: bytes that belong to the same byte sets behave alike
    std::array<int, 256> cls{};
    std::vector<int> rep;  // a representative byte per class
    {
      std::map<std::vector<bool>, int> seen;
      for (int b = 0; b < 256; ++b) {
        std::vector<bool> sig(nfa.sets.size());
        for (size_t k = 0; k < nfa.sets.size(); ++k) sig[k] = nfa.sets[k][(size_t)b];
        auto it = seen.find(sig);
        if (it == seen.end()) {
          it = seen.emplace(std::move(sig), (int)rep.size()).first;
          rep.push_back(b);
        }
        cls[(size_t)b] = it->second;
      }
    }
    const int C = (int)rep.size();

    long work = 0;
    auto spend = [&](long n) {
      work += n;
      if (work > lim.work)
        throw Fail{"guide pattern: too complex: the DFA construction exceeded its work cap of " +
                   std::to_string(lim.work) + " steps"};
    };
    std::vector<int> mark((size_t)N, -1);
    int stamp = 0;
    std::vector<int> stack;
    // epsilon closure of `seed`, reduced to the states that matter (a byte edge, or the final state), sorted
    auto closure = [&](const std::vector<int>& seed) {
      ++stamp;
      std::vector<int> key;
      stack.assign(seed.begin(), seed.end());
      for (int s : seed) mark[(size_t)s] = stamp;
      while (!stack.empty()) {
        const int s = stack.back();
        stack.pop_back();
        spend(1);
        if (nfa.st[(size_t)s].set >= 0 || s == final_state) key.push_back(s);
        for (int t : nfa.st[(size_t)s].eps)
          if (mark[(size_t)t] != stamp) {
            mark[(size_t)t] = stamp;
            stack.push_back(t);
          }
      }
      std::sort(key.begin(), key.end());
      return key;
    };

    std::map<std::vector<int>, int> index;
    std::vector<std::vector<int>> states;
    std::vector<std::vector<int>> trans;  // [state][class] -> state or -1
    auto intern = [&](std::vector<int> key) {
      auto it = index.find(key);
      if (it != index.end()) return it->second;
      if ((int)states.size() >= lim.raw_states)
        throw Fail{"guide pattern: needs more than " + std::to_string(lim.max_states) + " DFA states" +
                   (lim.raw_states > lim.max_states
                        ? " (more than " + std::to_string(lim.raw_states) + " before equivalent states are merged)" : "")};
      const int id = (int)states.size();
      index.emplace(key, id);
      states.push_back(std::move(key));
      trans.emplace_back((size_t)C, -1);
      return id;
    };
    intern(closure({se.first}));
    std::vector<int> moved;
    for (size_t d = 0; d < states.size(); ++d) {
      for (int c = 0; c < C; ++c) {
        moved.clear();
        const std::vector<int> cur = states[d];  // (a copy: intern may grow `states`)
        spend((long)cur.size());
        for (int s : cur) {
          const auto& q = nfa.st[(size_t)s];
          if (q.set >= 0 && nfa.sets[(size_t)q.set][(size_t)rep[(size_t)c]]) moved.push_back(q.out);
        }
        if (!moved.empty()) trans[d][(size_t)c] = intern(closure(moved));
      }
    }

    // trim: keep the states from which an accepting state is reachable
    const int D = (int)states.size();
    std::vector<uint8_t> acc((size_t)D, 0), live((size_t)D, 0);
    for (int d = 0; d < D; ++d)
      acc[(size_t)d] = std::binary_search(states[(size_t)d].begin(), states[(size_t)d].end(), final_state);
    live = acc;
    for (bool grew = true; grew;) {
      grew = false;
      for (int d = 0; d < D; ++d) {
        if (live[(size_t)d]) continue;
        for (int c = 0; c < C; ++c) {
          const int t = trans[(size_t)d][(size_t)c];
          if (t >= 0 && live[(size_t)t]) { live[(size_t)d] = 1; grew = true; break; }
        }
      }
    }
    if (!live[0]) throw Fail{"guide pattern: matches nothing"};
    std::vector<int> renum((size_t)D, -1);
    int n = 0;
    for (int d = 0; d < D; ++d)
      if (live[(size_t)d]) renum[(size_t)d] = n++;
    if (lim.minimize) {
      // Moore's refinement over the live states: two states stay together while they agree on acceptance and on the
      // block every byte class leads to (-1 = dead).  Blocks are numbered by their first state, so state 0 stays 0.
      std::vector<int> block((size_t)D, -1), next((size_t)D, -1);
      for (int d = 0; d < D; ++d)
        if (live[(size_t)d]) block[(size_t)d] = acc[(size_t)d];
      std::vector<int> sig((size_t)C + 1);
      for (int blocks = 0;;) {
        std::map<std::vector<int>, int> ids;
        for (int d = 0; d < D; ++d) {
          if (!live[(size_t)d]) continue;
          spend((long)C);
          sig[0] = block[(size_t)d];
          for (int c = 0; c < C; ++c) {
            const int t = trans[(size_t)d][(size_t)c];
            sig[(size_t)c + 1] = t >= 0 && live[(size_t)t] ? block[(size_t)t] : -1;
          }
          next[(size_t)d] = ids.emplace(sig, (int)ids.size()).first->second;
        }
        block.swap(next);
        if ((int)ids.size() == blocks) break;
        blocks = (int)ids.size();
      }
      n = 0;
      std::vector<int> first_of;
      for (int d = 0; d < D; ++d) {
        if (!live[(size_t)d]) continue;
        const int b = block[(size_t)d];
        if (b >= (int)first_of.size()) first_of.resize((size_t)b + 1, -1);
        if (first_of[(size_t)b] < 0) first_of[(size_t)b] = n++;
        renum[(size_t)d] = first_of[(size_t)b];
      }
    }
    if (n > lim.max_states)
      throw Fail{"guide pattern: needs more than " + std::to_string(lim.max_states) + " DFA states"};
    out->n_states = n;
    out->table.assign((size_t)n * 256, kGuideDead);
    out->accept.assign((size_t)n, 0);
    for (int d = 0; d < D; ++d) {
      if (!live[(size_t)d]) continue;
      const int r = renum[(size_t)d];
      out->accept[(size_t)r] = acc[(size_t)d];
      for (int b = 0; b < 256; ++b) {
        const int t = trans[(size_t)d][(size_t)cls[(size_t)b]];
        if (t >= 0 && live[(size_t)t]) out->table[(size_t)r * 256 + (size_t)b] = (uint16_t)renum[(size_t)t];
      }
    }
    return true;
  } catch (const Fail& f) {
    if (err) *err = f.msg;
    return false;
  }
}

// ---- JSON Schema -> pattern (guide.h schema_pattern) ---------------------------------------------------------------
[[noreturn]] void sfail(const std::string& what) { throw Fail{"json schema: " + what}; }

bool valid_utf8(std::string_view s) {
  for (size_t i = 0; i < s.size();) {
    const unsigned char c = (unsigned char)s[i];
    int n = c < 0x80 ? 0 : c >= 0xC2 && c <= 0xDF ? 1 : c >= 0xE0 && c <= 0xEF ? 2 : c >= 0xF0 && c <= 0xF4 ? 3 : -1;
    if (n < 0 || i + (size_t)n >= s.size() + (n ? 0 : 1)) return false;
    for (int k = 1; k <= n; ++k) {
      const unsigned char d = (unsigned char)s[i + (size_t)k];
      unsigned lo = 0x80, hi = 0xBF;
      if (k == 1) {
        if (c == 0xE0) lo = 0xA0;
        if (c == 0xED) hi = 0x9F;
        if (c == 0xF0) lo = 0x90;
        if (c == 0xF4) hi = 0x8F;
      }
      if (d < lo || d > hi) return false;
    }
    i += (size_t)n + 1;
  }
  return true;
}

// A JSON value with its members in document order (the order of `properties` is the order of the output).
struct Jv {
  enum Kind { kNull, kBool, kNumber, kString, kArray, kObject } kind = kNull;
  bool b = false;
  double num = 0;
  std::string str;                                // kString: the value (UTF-8)
  std::vector<Jv> arr;
  std::vector<std::pair<std::string, Jv>> obj;

  const Jv* get(std::string_view key) const {
    for (auto& kv : obj)
      if (kv.first == key) return &kv.second;
    return nullptr;
  }
};

struct JsonReader {
  std::string_view t;
  size_t i = 0;
  int depth = 0;

  [[noreturn]] void bad(const std::string& what) { sfail("malformed JSON: " + what + " at offset " + std::to_string(i)); }
  void ws() {
    while (i < t.size() && (t[i] == ' ' || t[i] == '\t' || t[i] == '\n' || t[i] == '\r')) ++i;
  }
  bool eat(char c) {
    ws();
    if (i < t.size() && t[i] == c) { ++i; return true; }
    return false;
  }
  static void put_utf8(std::string& out, unsigned cp) {
    if (cp < 0x80) out += (char)cp;
    else if (cp < 0x800) { out += (char)(0xC0 | cp >> 6); out += (char)(0x80 | (cp & 0x3F)); }
    else if (cp < 0x10000) {
      out += (char)(0xE0 | cp >> 12); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F));
    } else {
      out += (char)(0xF0 | cp >> 18); out += (char)(0x80 | ((cp >> 12) & 0x3F));
      out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F));
    }
  }
  unsigned hex4() {
    if (i + 4 > t.size()) bad("short \\u escape");
    unsigned v = 0;
    for (int k = 0; k < 4; ++k) {
      const int h = hex_val((unsigned char)t[i++]);
      if (h < 0) bad("bad \\u escape");
      v = v * 16 + (unsigned)h;
    }
    return v;
  }
  std::string string() {  // i is just past the opening quote
    std::string out;
    while (true) {
      if (i >= t.size()) bad("unterminated string");
      const unsigned char c = (unsigned char)t[i++];
      if (c == '"') return out;
      if (c < 0x20) bad("raw control byte in a string");
      if (c != '\\') { out += (char)c; continue; }
      if (i >= t.size()) bad("unterminated string");
      const char e = t[i++];
      switch (e) {
        case '"': case '\\': case '/': out += e; break;
        case 'b': out += '\b'; break;
        case 'f': out += '\f'; break;
        case 'n': out += '\n'; break;
        case 'r': out += '\r'; break;
        case 't': out += '\t'; break;
        case 'u': {
          unsigned cp = hex4();
          if (cp >= 0xDC00 && cp <= 0xDFFF) bad("lone surrogate");
          if (cp >= 0xD800 && cp <= 0xDBFF) {
            if (i + 2 > t.size() || t[i] != '\\' || t[i + 1] != 'u') bad("lone surrogate");
            i += 2;
            const unsigned lo = hex4();
            if (lo < 0xDC00 || lo > 0xDFFF) bad("lone surrogate");
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
          }
          put_utf8(out, cp);
          break;
        }
        default: bad("bad escape");
      }
    }
  }
  Jv value() {
    if (++depth > 64) bad("nested deeper than 64");
    ws();
    if (i >= t.size()) bad("unexpected end");
    Jv v;
    const char c = t[i];
    if (c == '{') {
      ++i;
      v.kind = Jv::kObject;
      if (!eat('}')) {
        do {
          if (!eat('"')) bad("expected a member name");
          std::string k = string();
          if (v.get(k)) bad("duplicate member \"" + k + "\"");
          if (!eat(':')) bad("expected :");
          v.obj.emplace_back(std::move(k), value());
        } while (eat(','));
        if (!eat('}')) bad("expected , or }");
      }
    } else if (c == '[') {
      ++i;
      v.kind = Jv::kArray;
      if (!eat(']')) {
        do v.arr.push_back(value());
        while (eat(','));
        if (!eat(']')) bad("expected , or ]");
      }
    } else if (c == '"') {
      ++i;
      v.kind = Jv::kString;
      v.str = string();
    } else if (t.substr(i, 4) == "true") { i += 4; v.kind = Jv::kBool; v.b = true; }
    else if (t.substr(i, 5) == "false") { i += 5; v.kind = Jv::kBool; }
    else if (t.substr(i, 4) == "null") { i += 4; }
    else {
      const size_t s = i;
      auto digits = [&] { size_t k = i; while (i < t.size() && t[i] >= '0' && t[i] <= '9') ++i; return i > k; };
      if (i < t.size() && t[i] == '-') ++i;
      if (i < t.size() && t[i] == '0') ++i;
      else if (!digits()) bad("unexpected character");
      if (i < t.size() && t[i] == '.') { ++i; if (!digits()) bad("bad number"); }
      if (i < t.size() && (t[i] == 'e' || t[i] == 'E')) {
        ++i;
        if (i < t.size() && (t[i] == '+' || t[i] == '-')) ++i;
        if (!digits()) bad("bad number");
      }
      v.kind = Jv::kNumber;
      v.num = strtod(std::string(t.substr(s, i - s)).c_str(), nullptr);
    }
    --depth;
    return v;
  }
  Jv document() {
    Jv v = value();
    ws();
    if (i != t.size()) bad("trailing text");
    return v;
  }
};

// the compact JSON text of a string, as json.dumps(ensure_ascii=False) writes it
std::string json_text(const std::string& s) {
  std::string out = "\"";
  for (unsigned char c : s) {
    switch (c) {
      case '"': out += "\\\""; break;
      case '\\': out += "\\\\"; break;
      case '\b': out += "\\b"; break;
      case '\f': out += "\\f"; break;
      case '\n': out += "\\n"; break;
      case '\r': out += "\\r"; break;
      case '\t': out += "\\t"; break;
      default:
        if (c < 0x20) {
          char buf[8];
          snprintf(buf, sizeof buf, "\\u%04x", c);
          out += buf;
        } else {
          out += (char)c;
        }
    }
  }
  return out + "\"";
}

// the compact JSON text of a number: an integral value below 2^53 as an integer, else the shortest round-trip form
std::string number_text(double v) {
  if (!std::isfinite(v)) sfail("a number out of range");
  char buf[40];
  if (v == std::floor(v) && std::fabs(v) < 9007199254740992.0) {
    snprintf(buf, sizeof buf, "%lld", (long long)v);
    return buf;
  }
  for (int p = 1; p <= 17; ++p) {
    snprintf(buf, sizeof buf, "%.*g", p, v);
    if (strtod(buf, nullptr) == v) break;
  }
  return buf;
}

std::string literal(const std::string& text) { return choice_pattern({text}); }

// One JSON string character = one code point: a UTF-8 sequence (no raw control byte, quote or backslash; no
// surrogate, no overlong form) or one escape (\uXXXX outside the surrogates, so never half a pair).
const char kStringChar[] =
    "(?:[^\"\\\\\\x00-\\x1f\\x80-\\xff]|[\\xc2-\\xdf][\\x80-\\xbf]|\\xe0[\\xa0-\\xbf][\\x80-\\xbf]|"
    "[\\xe1-\\xec\\xee\\xef][\\x80-\\xbf]{2}|\\xed[\\x80-\\x9f][\\x80-\\xbf]|\\xf0[\\x90-\\xbf][\\x80-\\xbf]{2}|"
    "[\\xf1-\\xf3][\\x80-\\xbf]{3}|\\xf4[\\x80-\\x8f][\\x80-\\xbf]{2}|"
    "\\\\(?:[\"\\\\/bfnrt]|u(?:[0-9a-cA-Ce-fE-F][0-9a-fA-F]{3}|[dD][0-7][0-9a-fA-F]{2})))";
const char kInteger[] = "-?(?:0|[1-9][0-9]*)";
const char kNumber[] = "-?(?:0|[1-9][0-9]*)(?:\\.[0-9]+)?(?:[eE][+\\-]?[0-9]+)?";

constexpr int kSchemaMaxLength = 64, kSchemaMaxItems = 16;

struct Lowering {
  const Jv& root;
  std::vector<std::string> refs;  // the $ref targets being inlined (a repeat is a cycle)
  int depth = 0;

  static bool annotation(const std::string& k) {
    return k == "title" || k == "description" || k == "default" || k == "examples" || k == "$schema" || k == "$id" ||
           k == "$defs" || k == "definitions";
  }
  [[noreturn]] static void unsupported(const std::string& k, const std::string& at, const std::string& why = "") {
    sfail("unsupported keyword '" + k + "' at " + at + (why.empty() ? "" : " (" + why + ")"));
  }
  // every member of `s` is one of `allowed` or an annotation
  static void only(const Jv& s, const std::string& at, std::initializer_list<const char*> allowed,
                   const std::string& why = "") {
    for (auto& kv : s.obj) {
      if (annotation(kv.first)) continue;
      bool ok = false;
      for (const char* a : allowed) ok = ok || kv.first == a;
      if (!ok) unsupported(kv.first, at, why);
    }
  }
  static int bound(const Jv& s, const char* key, int cap, int dflt, const std::string& at) {
    const Jv* v = s.get(key);
    if (!v) return dflt;
    if (v->kind != Jv::kNumber || v->num != std::floor(v->num) || v->num < 0 || v->num > cap)
      sfail(std::string("'") + key + "' at " + at + " must be an integer in [0, " + std::to_string(cap) + "]");
    return (int)v->num;
  }
  static std::string repeat(int lo, int hi) {  // hi < 0: unbounded
    if (hi < 0) return lo == 0 ? "*" : "{" + std::to_string(lo) + ",}";
    return lo == hi ? "{" + std::to_string(lo) + "}" : "{" + std::to_string(lo) + "," + std::to_string(hi) + "}";
  }
  static const char* type_of(const Jv& v) {
    switch (v.kind) {
      case Jv::kNull: return "null";
      case Jv::kBool: return "boolean";
      case Jv::kString: return "string";
      case Jv::kNumber: return v.num == std::floor(v.num) ? "integer" : "number";
      case Jv::kArray: return "array";
      default: return "object";
    }
  }
  static bool type_admits(const std::string& type, const Jv& v) {
    const std::string t = type_of(v);
    return t == type || (type == "number" && t == "integer");
  }
  static bool known_type(const std::string& t) {
    return t == "object" || t == "array" || t == "string" || t == "integer" || t == "number" || t == "boolean" ||
           t == "null";
  }
  static std::vector<std::string> types(const Jv& s, const std::string& at) {
    std::vector<std::string> out;
    const Jv* t = s.get("type");
    if (!t) return out;
    if (t->kind == Jv::kString) out.push_back(t->str);
    else if (t->kind == Jv::kArray && !t->arr.empty())
      for (auto& e : t->arr) {
        if (e.kind != Jv::kString) sfail("'type' at " + at + " must be a string or a list of strings");
        if (std::find(out.begin(), out.end(), e.str) == out.end()) out.push_back(e.str);
      }
    else sfail("'type' at " + at + " must be a string or a list of strings");
    for (auto& n : out)
      if (!known_type(n)) sfail("unknown type '" + n + "' at " + at);
    return out;
  }

  const Jv& resolve(const std::string& ref, const std::string& at) {
    for (const char* base : {"#/$defs/", "#/definitions/"}) {
      const std::string b = base;
      if (ref.compare(0, b.size(), b) != 0) continue;
      const std::string name = ref.substr(b.size());
      const Jv* defs = root.get(b.substr(2, b.size() - 3));
      const Jv* hit = defs && defs->kind == Jv::kObject && name.find_first_of("/~") == std::string::npos ? defs->get(name) : nullptr;
      if (!hit) sfail("$ref '" + ref + "' at " + at + " names no definition");
      return *hit;
    }
    unsupported("$ref", at, "only #/$defs/<name> and #/definitions/<name>: '" + ref + "'");
  }

  // the JSON types a oneOf branch can produce (integer and number count as one: their languages overlap)
  std::vector<std::string> branch_types(const Jv& s, const std::string& at, int hops = 0) {
    std::vector<std::string> out;
    if (s.kind != Jv::kObject) sfail("schema at " + at + " must be an object");
    if (const Jv* r = s.get("$ref")) {
      if (r->kind != Jv::kString || hops > 32) sfail("recursive $ref at " + at);
      return branch_types(resolve(r->str, at), at, hops + 1);
    }
    out = types(s, at);
    if (out.empty()) {
      if (const Jv* c = s.get("const")) out.push_back(type_of(*c));
      else if (const Jv* e = s.get("enum"); e && e->kind == Jv::kArray)
        for (auto& v : e->arr) out.push_back(type_of(v));
      else unsupported("oneOf", at, "a branch without 'type', 'const' or 'enum': exclusivity cannot be shown");
    }
    for (auto& t : out)
      if (t == "integer") t = "number";
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
  }

  std::string scalars(const Jv& s, const std::string& at) {
    only(s, at, {"enum", "const", "type"}, "beside enum / const");
    const Jv* e = s.get("enum");
    const Jv* c = s.get("const");
    if (e && c) unsupported("const", at, "together with enum");
    if (e && (e->kind != Jv::kArray || e->arr.empty())) sfail("'enum' at " + at + " must be a non-empty array");
    const std::vector<std::string> ts = types(s, at);
    std::vector<std::string> alts;
    auto add = [&](const Jv& v) {
      if (v.kind == Jv::kArray || v.kind == Jv::kObject)
        unsupported(e ? "enum" : "const", at, "only scalar values");
      bool ok = ts.empty();
      for (auto& t : ts) ok = ok || type_admits(t, v);
      if (!ok) return;  // (excluded by 'type': the instance must satisfy both)
      std::string text = v.kind == Jv::kNull ? "null" : v.kind == Jv::kBool ? (v.b ? "true" : "false")
                         : v.kind == Jv::kNumber ? number_text(v.num) : json_text(v.str);
      text = literal(text);
      if (std::find(alts.begin(), alts.end(), text) == alts.end()) alts.push_back(text);
    };
    if (c) add(*c);
    else for (auto& v : e->arr) add(v);
    if (alts.empty()) sfail("no value of the enum / const at " + at + " has its 'type'");
    std::string out = "(?:";
    for (size_t k = 0; k < alts.size(); ++k) out += (k ? "|" : "") + alts[k];
    return out + ")";
  }

  std::string object(const Jv& s, const std::string& at) {
    const Jv* props = s.get("properties");
    if (!props) unsupported("type", at, "an object without 'properties': free-form values belong to json_object");
    if (props->kind != Jv::kObject) sfail("'properties' at " + at + " must be an object");
    if (const Jv* ap = s.get("additionalProperties"))
      if (ap->kind != Jv::kBool || ap->b) unsupported("additionalProperties", at, "only false");
    std::vector<bool> req(props->obj.size(), false);
    if (const Jv* r = s.get("required")) {
      if (r->kind != Jv::kArray) sfail("'required' at " + at + " must be an array of strings");
      for (auto& n : r->arr) {
        size_t k = 0;
        while (n.kind == Jv::kString && k < props->obj.size() && props->obj[k].first != n.str) ++k;
        if (n.kind != Jv::kString) sfail("'required' at " + at + " must be an array of strings");
        if (k == props->obj.size()) sfail("'required' at " + at + " names '" + n.str + "', which 'properties' lacks");
        req[k] = true;
      }
    }
    // from the last member back: `after` = the members from k on once one has been written (each leads with a
    // comma), `first` = the same while none has been written yet
    std::string after, first;
    for (size_t k = props->obj.size(); k-- > 0;) {
      const std::string m = literal(json_text(props->obj[k].first)) + ":" +
                            schema(props->obj[k].second, at + "/properties/" + props->obj[k].first);
      if (req[k]) {
        first = m + after;
        after = "," + m + after;
      } else {
        first = "(?:" + m + after + "|" + first + ")";
        after = "(?:," + m + ")?" + after;
      }
      if (first.size() > 4 * (size_t)kGuidePatternBytes) sfail("the lowered pattern exceeds " + std::to_string(kGuidePatternBytes) + " bytes (kGuidePatternBytes) at " + at);
    }
    return "\\{" + first + "\\}";
  }

  std::string array(const Jv& s, const std::string& at) {
    const Jv* items = s.get("items");
    if (!items) unsupported("type", at, "an array without 'items': free-form values belong to json_object");
    if (items->kind != Jv::kObject) unsupported("items", at, "only a single schema");
    const int lo = bound(s, "minItems", kSchemaMaxItems, 0, at), hi = bound(s, "maxItems", kSchemaMaxItems, -1, at);
    if (hi >= 0 && hi < lo) sfail("'maxItems' below 'minItems' at " + at);
    if (hi == 0) return "\\[\\]";
    const std::string it = schema(*items, at + "/items");
    const std::string body = it + "(?:," + it + ")" + repeat(std::max(lo - 1, 0), hi < 0 ? -1 : hi - 1);
    return lo == 0 ? "\\[(?:" + body + ")?\\]" : "\\[" + body + "\\]";
  }

  std::string string(const Jv& s, const std::string& at) {
    const int lo = bound(s, "minLength", kSchemaMaxLength, 0, at), hi = bound(s, "maxLength", kSchemaMaxLength, -1, at);
    if (hi >= 0 && hi < lo) sfail("'maxLength' below 'minLength' at " + at);
    return std::string("\"") + kStringChar + repeat(lo, hi) + "\"";
  }

  std::string schema(const Jv& s, const std::string& at) {
    if (s.kind != Jv::kObject) sfail("schema at " + at + " must be an object (boolean schemas are not supported)");
    if (++depth > 32) sfail("schemas nested deeper than 32 at " + at);
    std::string out;
    if (const Jv* r = s.get("$ref")) {
      only(s, at, {"$ref"}, "beside $ref");
      if (r->kind != Jv::kString) sfail("'$ref' at " + at + " must be a string");
      const Jv& target = resolve(r->str, at);
      if (std::find(refs.begin(), refs.end(), r->str) != refs.end()) sfail("recursive $ref '" + r->str + "' at " + at);
      refs.push_back(r->str);
      out = schema(target, r->str);
      refs.pop_back();
    } else if (s.get("anyOf") || s.get("oneOf")) {
      const bool one = !s.get("anyOf");
      const char* key = one ? "oneOf" : "anyOf";
      only(s, at, {key}, std::string("beside ") + key);
      const Jv* br = s.get(key);
      if (br->kind != Jv::kArray || br->arr.empty()) sfail(std::string("'") + key + "' at " + at + " must be a non-empty array");
      std::vector<std::string> seen;
      out = "(?:";
      for (size_t k = 0; k < br->arr.size(); ++k) {
        const std::string bat = at + "/" + key + "/" + std::to_string(k);
        if (one)
          for (auto& t : branch_types(br->arr[k], bat)) {
            if (std::find(seen.begin(), seen.end(), t) != seen.end())
              unsupported("oneOf", at, "two branches admit the type '" + t + "': exclusivity is not enforced");
            seen.push_back(t);
          }
        out += (k ? "|" : "") + schema(br->arr[k], bat);
      }
      out += ")";
    } else if (s.get("enum") || s.get("const")) {
      out = scalars(s, at);
    } else {
      const std::vector<std::string> ts = types(s, at);
      if (ts.empty()) {
        only(s, at, {});
        unsupported("type", at, "a schema without 'type': free-form values belong to json_object");
      }
      auto has = [&](const char* t) { return std::find(ts.begin(), ts.end(), t) != ts.end(); };
      for (auto& kv : s.obj) {  // a keyword is read by the type it belongs to, and only where that type is listed
        const std::string& k = kv.first;
        if (annotation(k) || k == "type") continue;
        const bool ok = ((k == "properties" || k == "required" || k == "additionalProperties") && has("object")) ||
                        ((k == "items" || k == "minItems" || k == "maxItems") && has("array")) ||
                        ((k == "minLength" || k == "maxLength") && has("string"));
        if (!ok) unsupported(k, at);
      }
      out = ts.size() > 1 ? "(?:" : "";
      for (size_t k = 0; k < ts.size(); ++k) {
        const std::string& t = ts[k];
        out += k ? "|" : "";
        out += t == "object" ? object(s, at) : t == "array" ? array(s, at) : t == "string" ? string(s, at)
               : t == "integer" ? kInteger : t == "number" ? kNumber : t == "boolean" ? "(?:true|false)" : "null";
      }
      out += ts.size() > 1 ? ")" : "";
    }
    if (out.size() > 4 * (size_t)kGuidePatternBytes)
      sfail("the lowered pattern exceeds " + std::to_string(kGuidePatternBytes) + " bytes (kGuidePatternBytes) at " + at);
    --depth;
    return out;
  }
};

}  // namespace

bool compile(std::string_view pattern, Dfa* out, std::string* err) { return compile_with(pattern, out, err, kNarrow); }

bool compile_wide(std::string_view pattern, Dfa* out, std::string* err) {
  return compile_with(pattern, out, err, kWide);
}

bool schema_pattern(std::string_view schema_json, std::string* pattern, std::string* err) {
  try {
    if (schema_json.size() > (size_t)kGuideSchemaBytes)
      throw Fail{"json schema: longer than " + std::to_string(kGuideSchemaBytes) + " bytes"};
    if (!valid_utf8(schema_json)) throw Fail{"json schema: not valid UTF-8"};
    JsonReader rd{schema_json};
    Jv root = rd.document();
    Lowering lo{root};
    std::string out = lo.schema(root, "#");
    if (out.size() > (size_t)kGuidePatternBytes)
      throw Fail{"json schema: the lowered pattern has " + std::to_string(out.size()) + " bytes, more than " +
                 std::to_string(kGuidePatternBytes) + " (kGuidePatternBytes)"};
    *pattern = std::move(out);
    return true;
  } catch (const Fail& f) {
    if (err) *err = f.msg;
    return false;
  }
}

std::string choice_pattern(const std::vector<std::string>& choices) {
  std::string out;
  for (size_t k = 0; k < choices.size(); ++k) {
    if (k) out += '|';
    for (char c : choices[k]) {
      if (std::string_view("\\.^$*+?()[]{}|").find(c) != std::string_view::npos) out += '\\';
      out += c;
    }
  }
  return out;
}

}  // namespace guide
