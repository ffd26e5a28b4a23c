// Pattern compiler of guided decoding (guide.h): parse -> Thompson NFA (quantifiers expanded) -> subset construction
// over byte classes -> trim.  Every limit is an error, never a truncation; the NFA and work caps bound what a hostile
// pattern can cost.
#include "guide.h"

#include <algorithm>
#include <array>
#include <bitset>
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

struct Parser {
  std::string_view p;
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
    else if (c >= '0' && c <= '9') fail(std::string("back-reference or octal escape \\") + (char)c, at);
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

  int add() {
    if ((int)st.size() >= kGuideNfaStates)
      fail("pattern too large: more than " + std::to_string(kGuideNfaStates) + " NFA states, expanding the quantifier", quant_at);
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

}  // namespace

bool compile(std::string_view pattern, Dfa* out, std::string* err) {
  try {
    if (pattern.size() > (size_t)kGuidePatternBytes)
      throw Fail{"guide pattern: longer than " + std::to_string(kGuidePatternBytes) + " bytes"};
    Parser ps{pattern};
    NodeP root = ps.alt();
    if (ps.more()) fail("unbalanced )", ps.i);
    Nfa nfa;
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
      if (work > kGuideWork)
        throw Fail{"guide pattern: too complex: the DFA construction exceeded its work cap of " +
                   std::to_string(kGuideWork) + " steps"};
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
      if ((int)states.size() >= kGuideStates)
        throw Fail{"guide pattern: needs more than " + std::to_string(kGuideStates) + " DFA states"};
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
