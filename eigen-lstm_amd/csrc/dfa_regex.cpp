// Byte regular expressions to minimal byte automata (dfa_regex.h; include/lstm_hip.h).
//   pattern -> syntax tree (recursive descent) -> Thompson automaton (a bounded repeat is copies of its operand)
//           -> subset construction over byte classes (bytes no set of the pattern tells apart), under a fixed work limit
//           -> finish(): trim (reachable from 0, can reach an accepting state), Hopcroft's partition refinement, breadth-first
//              numbering from state 0 with bytes ascending
// lstm_hip_dfa_intersect walks the product of two tables and ends in the same finish().  Plain C++: no HIP, no device.
#include "dfa_regex.h"

#include <algorithm>
#include <bitset>
#include <cstdio>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace dfa {
namespace {

typedef std::bitset<256> Set;

struct Error { // thrown by the parser and the builders, caught by the entry points
    int pos;
    std::string msg;
};
[[noreturn]] void refuse(int pos, const char *fmt, int a = 0, int b = 0) {
    char buf[256];
    snprintf(buf, sizeof(buf), fmt, a, b);
    throw Error{pos, buf};
}

// ---- syntax tree
enum Kind { EMPTY, SET, CAT, ALT, REP };
struct Node {
    Kind kind;
    int set = -1;          // SET: index into sets
    std::vector<int> kids; // CAT, ALT; REP: one
    int lo = 0, hi = 0;    // REP: hi == -1 is unbounded
};

struct Parser {
    const uint8_t *p;
    int n, i = 0, depth = 0;
    std::vector<Node> nodes;
    std::vector<Set> sets;

    int node(Kind k) {
        nodes.push_back(Node{k});
        return (int)nodes.size() - 1;
    }
    int leaf(const Set &s) {
        const int id = node(SET);
        nodes[id].set = (int)sets.size();
        sets.push_back(s);
        return id;
    }
    static bool punct(int c) { return (c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E); }
    static int hex(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
    static Set range(int lo, int hi) {
        Set s;
        for (int b = lo; b <= hi; b++) s.set(b);
        return s;
    }
    // the escape at p[i] == '\\': a set; *single is its byte, or -1 for a class escape.  i moves past it.
    Set escape(int *single) {
        const int at = i;
        if (i + 1 >= n) refuse(at, "regex: the pattern ends in a backslash at byte %d", at);
        const int c = p[i + 1];
        i += 2;
        *single = -1;
        Set s;
        switch (c) {
        case 'n': *single = '\n'; break;
        case 'r': *single = '\r'; break;
        case 't': *single = '\t'; break;
        case 'f': *single = '\f'; break;
        case 'v': *single = '\v'; break;
        case 'x': {
            const int h1 = i < n ? hex(p[i]) : -1, h2 = i + 1 < n ? hex(p[i + 1]) : -1;
            if (h1 < 0 || h2 < 0) refuse(at, "regex: \\x needs two hex digits at byte %d", at);
            *single = h1 * 16 + h2;
            i += 2;
            break;
        }
        case 'd': case 'D': s = range('0', '9'); break;
        case 'w': case 'W': s = range('0', '9') | range('a', 'z') | range('A', 'Z'); s.set('_'); break;
        case 's': case 'S': s.set(' '); s.set('\t'); s.set('\n'); s.set('\r'); s.set('\f'); s.set('\v'); break;
        default:
            if (!punct(c)) refuse(at, "regex: unsupported escape at byte %d (a backslash goes before punctuation, n r t f v xHH d D w W s S)", at);
            *single = c;
        }
        if (*single >= 0) s.set(*single);
        else if (c == 'D' || c == 'W' || c == 'S') s = ~s;
        return s;
    }
    int parse_class() { // p[i] == '['
        const int open = i++;
        bool negate = false;
        if (i < n && p[i] == '^') negate = true, i++;
        Set s;
        bool first = true;
        for (;; first = false) {
            if (i >= n) refuse(open, "regex: the class opened at byte %d is not closed", open);
            int c = p[i];
            if (c == ']') {
                if (first) refuse(i, "regex: ] at byte %d must be escaped inside a class (an empty class matches nothing)", i);
                i++;
                break;
            }
            const int at = i;
            int lo;
            if (c == '\\') {
                const Set e = escape(&lo);
                if (lo < 0) { // a class escape: never a range end
                    if (i + 1 < n && p[i] == '-' && p[i + 1] != ']') refuse(at, "regex: the class escape at byte %d cannot start a range", at);
                    s |= e;
                    continue;
                }
            } else {
                if (c >= 0x80) refuse(at, "regex: raw byte 0x%02x inside a class at byte %d: write \\xHH", c, at);
                if (c == '[') refuse(at, "regex: [ at byte %d must be escaped inside a class", at);
                lo = c;
                i++;
            }
            if (i + 1 < n && p[i] == '-' && p[i + 1] != ']') { // a range (a '-' that comes last is a literal)
                i++;
                int hi;
                if (p[i] == '\\') {
                    const int eat = i;
                    escape(&hi);
                    if (hi < 0) refuse(eat, "regex: the class escape at byte %d cannot end a range", eat);
                } else {
                    hi = p[i];
                    if (hi >= 0x80) refuse(i, "regex: raw byte 0x%02x inside a class at byte %d: write \\xHH", hi, i);
                    if (hi == '[') refuse(i, "regex: [ at byte %d must be escaped inside a class", i);
                    i++;
                }
                if (hi < lo) refuse(at, "regex: the range at byte %d runs backwards", at);
                s |= range(lo, hi);
            } else
                s.set(lo);
        }
        return leaf(negate ? ~s : s);
    }
    // the quantifier at p[i], if there is one: true and lo / hi set
    bool quantifier(int *lo, int *hi) {
        if (i >= n) return false;
        const int c = p[i], at = i;
        if (c == '*') return *lo = 0, *hi = -1, i++, true;
        if (c == '+') return *lo = 1, *hi = -1, i++, true;
        if (c == '?') return *lo = 0, *hi = 1, i++, true;
        if (c != '{') return false;
        int j = i + 1, m = -1, k = -1;
        bool comma = false;
        auto number = [&](int *v) {
            if (j < n && p[j] >= '0' && p[j] <= '9') *v = 0;
            for (; j < n && p[j] >= '0' && p[j] <= '9'; j++) *v = std::min(*v * 10 + (p[j] - '0'), 1000000);
        };
        number(&m);
        if (j < n && p[j] == ',') comma = true, j++, number(&k);
        if (j >= n || p[j] != '}' || (m < 0 && k < 0)) refuse(at, "regex: { at byte %d does not start a quantifier {m}, {m,}, {m,n} or {,n}", at);
        if (!comma) k = m;
        if (m < 0) m = 0;
        if (m > MAX_REPEAT || k > MAX_REPEAT) refuse(at, "regex: the repeat count at byte %d is above %d", at, MAX_REPEAT);
        if (k >= 0 && k < m) refuse(at, "regex: the quantifier at byte %d has its minimum above its maximum", at);
        *lo = m, *hi = k;
        i = j + 1;
        return true;
    }
    int parse_atom() { // p[i] starts one
        const int c = p[i], at = i;
        int single;
        switch (c) {
        case '(': {
            if (++depth > MAX_DEPTH) refuse(at, "regex: groups nested deeper than %d at byte %d", MAX_DEPTH, at);
            i++;
            if (i < n && p[i] == '?') {
                if (i + 1 >= n || p[i + 1] != ':') refuse(at, "regex: unsupported group (?...) at byte %d: only ( ) and (?: ) group", at);
                i += 2;
            }
            const int inner = parse_alt();
            if (i >= n || p[i] != ')') refuse(at, "regex: the group opened at byte %d is not closed", at);
            i++;
            depth--;
            return inner;
        }
        case '[': return parse_class();
        case '.': {
            i++;
            Set s = ~Set();
            s.reset('\n');
            return leaf(s);
        }
        case '\\': {
            const Set s = escape(&single);
            return leaf(s);
        }
        case '*': case '+': case '?': case '{': refuse(at, "regex: nothing to repeat at byte %d", at);
        case '^': case '$': refuse(at, "regex: anchor at byte %d: a match is always a whole-string match", at);
        case ']': case '}': refuse(at, "regex: unescaped bracket at byte %d", at);
        default: {
            i++;
            Set s;
            s.set(c);
            return leaf(s);
        }
        }
    }
    int parse_cat() {
        const int cat = node(CAT);
        while (i < n && p[i] != '|' && p[i] != ')') {
            int atom = parse_atom(), lo, hi;
            if (quantifier(&lo, &hi)) {
                const int rep = node(REP);
                nodes[rep].kids.push_back(atom);
                nodes[rep].lo = lo, nodes[rep].hi = hi;
                atom = rep;
                if (i < n && (p[i] == '*' || p[i] == '+' || p[i] == '?' || p[i] == '{'))
                    refuse(i, "regex: a quantifier at byte %d follows a quantifier (no lazy, possessive or stacked forms: group first)", i);
            }
            nodes[cat].kids.push_back(atom);
        }
        return cat;
    }
    int parse_alt() {
        const int first = parse_cat();
        if (i >= n || p[i] != '|') return first;
        const int alt = node(ALT);
        nodes[alt].kids.push_back(first);
        while (i < n && p[i] == '|') {
            i++;
            const int next = parse_cat();
            nodes[alt].kids.push_back(next);
        }
        return alt;
    }
    int parse() {
        const int root = parse_alt();
        if (i < n) refuse(i, "regex: unmatched ) at byte %d", i); // (parse_alt stops at nothing else)
        return root;
    }
};

// ---- Thompson automaton: a node is a byte set with one way out, or up to two ways out that read nothing
struct Nfa {
    struct N {
        int set, out1, out2; // set >= 0: a byte of sets[set] leads to out1; set == -1: out1 / out2 (-1: none) read nothing
    };
    std::vector<N> nodes;
    int fresh() {
        if ((int)nodes.size() >= NFA_LIMIT) refuse(-1, "regex: too many states: the pattern unrolls to more than %d automaton nodes", NFA_LIMIT);
        nodes.push_back(N{-1, -1, -1});
        return (int)nodes.size() - 1;
    }
    void eps(int from, int to) {
        N &x = nodes[from];
        (x.out1 < 0 ? x.out1 : x.out2) = to;
    }
};
// the automaton of tree node `id` between fresh nodes *s and *e (e has no way out yet)
void build(const Parser &ps, int id, Nfa &nfa, int *s, int *e) {
    const Node &nd = ps.nodes[id];
    *s = nfa.fresh();
    switch (nd.kind) {
    case EMPTY: *e = *s; return;
    case SET:
        *e = nfa.fresh();
        nfa.nodes[*s].set = nd.set;
        nfa.nodes[*s].out1 = *e;
        return;
    case CAT: {
        int cur = *s;
        for (int kid : nd.kids) {
            int ks, ke;
            build(ps, kid, nfa, &ks, &ke);
            nfa.eps(cur, ks);
            cur = ke;
        }
        *e = nfa.fresh();
        nfa.eps(cur, *e);
        return;
    }
    case ALT: {
        // a chain of two-way splits
        *e = nfa.fresh();
        int split = *s;
        for (size_t k = 0; k < nd.kids.size(); k++) {
            int ks, ke;
            build(ps, nd.kids[k], nfa, &ks, &ke);
            nfa.eps(split, ks);
            nfa.eps(ke, *e);
            if (k + 2 < nd.kids.size()) {
                const int more = nfa.fresh();
                nfa.eps(split, more);
                split = more;
            } // (the last alternative hangs off the same split)
        }
        return;
    }
    case REP: {
        int cur = *s;
        for (int k = 0; k < nd.lo; k++) {
            int ks, ke;
            build(ps, nd.kids[0], nfa, &ks, &ke);
            nfa.eps(cur, ks);
            cur = ke;
        }
        *e = nfa.fresh();
        if (nd.hi < 0) { // x*: cur -> loop; loop -> x -> loop; loop -> e
            const int loop = nfa.fresh();
            int ks, ke;
            build(ps, nd.kids[0], nfa, &ks, &ke);
            nfa.eps(cur, loop);
            nfa.eps(loop, ks);
            nfa.eps(ke, loop);
            nfa.eps(loop, *e);
        } else {
            for (int k = nd.lo; k < nd.hi; k++) { // x? x? ...: each may skip to the end
                const int opt = nfa.fresh();
                int ks, ke;
                build(ps, nd.kids[0], nfa, &ks, &ke);
                nfa.eps(cur, opt);
                nfa.eps(opt, ks);
                nfa.eps(opt, *e);
                cur = ke;
            }
            nfa.eps(cur, *e);
        }
        return;
    }
    }
}

// ---- a table on its way out: trans[q * 256 + b] is a state or -1
struct Table {
    std::vector<int32_t> trans;
    std::vector<char> acc;
    int Q() const { return (int)acc.size(); }
};

// bytes whose columns are equal in every state fall into one class: cls[b] in 0..k-1, rep[c] one byte of class c
int byte_classes(const Table &t, int cls[256], std::vector<int> &rep) {
    std::map<std::vector<int32_t>, int> seen;
    std::vector<int32_t> col(t.Q());
    rep.clear();
    for (int b = 0; b < 256; b++) {
        for (int q = 0; q < t.Q(); q++) col[q] = t.trans[(size_t)q * 256 + b];
        auto it = seen.find(col);
        if (it == seen.end()) {
            it = seen.emplace(col, (int)rep.size()).first;
            rep.push_back(b);
        }
        cls[b] = it->second;
    }
    return (int)rep.size();
}

// trim, minimise, number breadth-first.  False: the language is empty.
bool finish(Table &t) {
    int Q = t.Q();
    // reachable from 0
    std::vector<char> fwd(Q, 0), bwd(Q, 0);
    std::vector<int> stack{0};
    fwd[0] = 1;
    while (!stack.empty()) {
        const int q = stack.back();
        stack.pop_back();
        for (int b = 0; b < 256; b++) {
            const int v = t.trans[(size_t)q * 256 + b];
            if (v >= 0 && !fwd[v]) fwd[v] = 1, stack.push_back(v);
        }
    }
    // can reach an accepting state: backwards over the reversed edges
    std::vector<std::vector<int>> pred(Q);
    for (int q = 0; q < Q; q++) {
        int last = -1;
        for (int b = 0; b < 256; b++) {
            const int v = t.trans[(size_t)q * 256 + b];
            if (v >= 0 && v != last) pred[v].push_back(q), last = v;
        }
    }
    for (int q = 0; q < Q; q++)
        if (t.acc[q]) bwd[q] = 1, stack.push_back(q);
    while (!stack.empty()) {
        const int q = stack.back();
        stack.pop_back();
        for (int v : pred[q])
            if (!bwd[v]) bwd[v] = 1, stack.push_back(v);
    }
    if (!bwd[0]) return false;
    for (int q = 0; q < Q; q++)
        for (int b = 0; b < 256; b++) {
            int32_t &v = t.trans[(size_t)q * 256 + b];
            if (!(fwd[q] && bwd[q]) || (v >= 0 && !(fwd[v] && bwd[v]))) v = -1;
        }
    // Hopcroft's partition refinement over byte classes (one byte of each class is looked at).  The states kept are 0..n-1,
    // and n is the sink every missing transition leads to; blocks start as {accepting, not} and are split by the
    // predecessors of a block taken from the worklist, the smaller half of every split going back onto it.
    int cls[256];
    std::vector<int> rep;
    const int k = byte_classes(t, cls, rep);
    std::vector<int> idx(Q, -1), live;
    for (int q = 0; q < Q; q++)
        if (fwd[q] && bwd[q]) idx[q] = (int)live.size(), live.push_back(q);
    const int n = (int)live.size(), S = n + 1;
    auto delta = [&](int u, int c) {
        if (u == n) return n;
        const int v = t.trans[(size_t)live[u] * 256 + rep[c]];
        return v < 0 ? n : idx[v];
    };
    std::vector<int> head((size_t)k * (S + 1), 0), inv((size_t)k * S); // per class: the predecessors of every state
    for (int c = 0; c < k; c++) {
        int *h = head.data() + (size_t)c * (S + 1), *list = inv.data() + (size_t)c * S;
        for (int u = 0; u < S; u++) h[delta(u, c) + 1]++;
        for (int v = 0; v < S; v++) h[v + 1] += h[v];
        std::vector<int> at(h, h + S);
        for (int u = 0; u < S; u++) list[at[delta(u, c)]++] = u;
    }
    std::vector<int> elems(S), loc(S), blk(S), first, size, marked, work, members, touched;
    {
        int at = 0;
        for (int pass = 0; pass < 2; pass++)
            for (int u = 0; u < S; u++)
                if ((u < n && t.acc[live[u]]) == (pass == 0)) elems[at] = u, loc[u] = at++, blk[u] = pass;
        int accepting = 0;
        for (int u = 0; u < n; u++) accepting += t.acc[live[u]] != 0;
        first = {0, accepting};
        size = {accepting, S - accepting};
        marked = {0, 0};
        work = {0, 1};
    }
    while (!work.empty()) {
        const int A = work.back();
        work.pop_back();
        members.assign(elems.begin() + first[A], elems.begin() + first[A] + size[A]);
        for (int c = 0; c < k; c++) {
            const int *h = head.data() + (size_t)c * (S + 1), *list = inv.data() + (size_t)c * S;
            touched.clear();
            for (int v : members)
                for (int e = h[v]; e < h[v + 1]; e++) { // move u to the front of its block: the marked part
                    const int u = list[e], b = blk[u], to = first[b] + marked[b];
                    if (loc[u] < to) continue; // (already marked: a state has one successor per class, so this cannot be)
                    const int other = elems[to];
                    elems[to] = u, elems[loc[u]] = other, loc[other] = loc[u], loc[u] = to;
                    if (marked[b]++ == 0) touched.push_back(b);
                }
            for (int b : touched) {
                const int mk = marked[b];
                marked[b] = 0;
                if (mk == size[b]) continue;
                const int nb = (int)first.size();
                if (mk <= size[b] - mk) { // the marked part leaves
                    first.push_back(first[b]), size.push_back(mk);
                    first[b] += mk, size[b] -= mk;
                } else {
                    first.push_back(first[b] + mk), size.push_back(size[b] - mk);
                    size[b] = mk;
                }
                marked.push_back(0);
                for (int e = first[nb]; e < first[nb] + size[nb]; e++) blk[elems[e]] = nb;
                // (b is on the worklist: both halves are; it is not: the smaller half, which nb is)
                work.push_back(nb);
            }
        }
    }
    std::vector<int> block(Q, -1), renum(first.size(), -1);
    int blocks = 0;
    for (int u = 0; u < n; u++) {
        if (renum[blk[u]] < 0) renum[blk[u]] = blocks++;
        block[live[u]] = renum[blk[u]];
    }
    // breadth-first from state 0's block, bytes ascending
    std::vector<int> member(blocks, -1), number(blocks, -1), order;
    for (int q : live)
        if (member[block[q]] < 0) member[block[q]] = q;
    number[block[0]] = 0;
    order.push_back(block[0]);
    for (size_t i = 0; i < order.size(); i++)
        for (int b = 0; b < 256; b++) {
            const int v = t.trans[(size_t)member[order[i]] * 256 + b];
            if (v >= 0 && number[block[v]] < 0) number[block[v]] = (int)order.size(), order.push_back(block[v]);
        }
    Table out;
    out.trans.assign(order.size() * 256, -1);
    out.acc.assign(order.size(), 0);
    for (size_t i = 0; i < order.size(); i++) {
        const int q = member[order[i]];
        out.acc[i] = t.acc[q];
        for (int b = 0; b < 256; b++) {
            const int v = t.trans[(size_t)q * 256 + b];
            if (v >= 0) out.trans[i * 256 + b] = number[block[v]];
        }
    }
    t = std::move(out);
    return true;
}

struct VecHash {
    size_t operator()(const std::vector<int> &v) const {
        size_t h = 1469598103934665603ull;
        for (int x : v) h = (h ^ (size_t)x) * 1099511628211ull;
        return h;
    }
};

// subset construction.  A state is the sorted set of byte nodes (and the final node) its closure holds.
Table determinise(const Nfa &nfa, const std::vector<Set> &sets, int start, int final_node) {
    // byte classes of the pattern's sets
    int cls[256] = {0}, k = 1;
    std::unordered_set<Set> seen; // (a long pattern repeats its sets: each distinct one refines the classes once)
    for (const Set &s : sets) {
        if (!seen.insert(s).second) continue;
        std::map<std::pair<int, bool>, int> ids;
        for (int b = 0; b < 256; b++) cls[b] = ids.emplace(std::make_pair(cls[b], s[b]), (int)ids.size()).first->second;
        k = (int)ids.size();
    }
    std::vector<int> rep(k, -1);
    for (int b = 255; b >= 0; b--) rep[cls[b]] = b;

    long long steps = 0;
    std::vector<int> stamp(nfa.nodes.size(), -1), stack;
    int round = 0;
    auto closure = [&](const std::vector<int> &from) { // the byte nodes and the final node reachable reading nothing
        std::vector<int> out;
        round++;
        for (int x : from)
            if (stamp[x] != round) stamp[x] = round, stack.push_back(x);
        while (!stack.empty()) {
            const int x = stack.back();
            stack.pop_back();
            if (++steps > WORK_STEPS) refuse(-1, "regex: too many states: the subset construction passed its work limit (2^%d node visits)", 27);
            const Nfa::N &nd = nfa.nodes[x];
            if (nd.set >= 0 || x == final_node) {
                out.push_back(x);
                if (nd.set >= 0) continue;
            }
            for (int v : {nd.out1, nd.out2})
                if (v >= 0 && stamp[v] != round) stamp[v] = round, stack.push_back(v);
        }
        std::sort(out.begin(), out.end());
        return out;
    };
    std::unordered_map<std::vector<int>, int, VecHash> ids;
    std::vector<std::vector<int>> states;
    Table t;
    auto intern = [&](std::vector<int> &&set) {
        auto it = ids.find(set);
        if (it != ids.end()) return it->second;
        if ((int)states.size() >= WORK_STATES)
            refuse(-1, "regex: too many states: the subset construction passed its work limit (%d states before minimisation)", WORK_STATES);
        const int id = (int)states.size();
        ids.emplace(set, id);
        t.acc.push_back(std::binary_search(set.begin(), set.end(), final_node));
        t.trans.resize(t.trans.size() + 256, -1);
        states.push_back(std::move(set));
        return id;
    };
    intern(closure({start}));
    std::vector<int> targets;
    for (size_t q = 0; q < states.size(); q++) {
        std::vector<int> to(k, -1);
        for (int c = 0; c < k; c++) {
            targets.clear();
            const std::vector<int> cur = states[q]; // (states may grow)
            for (int x : cur) {
                steps++;
                if (nfa.nodes[x].set >= 0 && sets[nfa.nodes[x].set][rep[c]]) targets.push_back(nfa.nodes[x].out1);
            }
            if (!targets.empty()) to[c] = intern(closure(targets));
        }
        for (int b = 0; b < 256; b++) t.trans[q * 256 + b] = to[cls[b]];
    }
    return t;
}

int32_t emit(const Table &t, uint16_t *next, uint8_t *accept, int32_t cap, const char *what, std::string &msg) {
    const int Q = t.Q();
    char buf[160];
    if (Q > MAX_STATES) {
        snprintf(buf, sizeof(buf), "%s: too many states: the minimal automaton has %d, above %d", what, Q, MAX_STATES);
        msg = buf;
        return -1;
    }
    if (!next && !accept) return Q;
    if (!next || !accept) {
        snprintf(buf, sizeof(buf), "%s: next and accept must both be given, or both be null to ask for the size", what);
        msg = buf;
        return -1;
    }
    if (cap < Q) {
        snprintf(buf, sizeof(buf), "%s: cap %d is below the %d states of the result", what, cap, Q);
        msg = buf;
        return -1;
    }
    for (size_t e = 0; e < (size_t)Q * 256; e++) next[e] = t.trans[e] < 0 ? (uint16_t)0xFFFF : (uint16_t)t.trans[e];
    for (int q = 0; q < Q; q++) accept[q] = t.acc[q] ? 1 : 0;
    return Q;
}

} // namespace

int32_t regex(const uint8_t *pattern, size_t len, int32_t stop_byte, uint16_t *next, uint8_t *accept, int32_t cap,
              int32_t *error_pos, std::string &msg) {
    if (error_pos) *error_pos = -1;
    char buf[160];
    if (!pattern && len > 0) return msg = "dfa_regex: null pattern", -1;
    if (len > (size_t)NFA_LIMIT) return msg = "dfa_regex: too many states: the pattern is longer than the automaton's node limit", -1;
    if (stop_byte < -1 || stop_byte > 255) {
        snprintf(buf, sizeof(buf), "dfa_regex: stop_byte must be -1 or in [0, 255] (got %d)", stop_byte);
        return msg = buf, -1;
    }
    try {
        Parser ps{pattern, (int)len};
        const int root = ps.parse();
        Nfa nfa;
        int s, e;
        build(ps, root, nfa, &s, &e);
        Table t = determinise(nfa, ps.sets, s, e);
        if (!finish(t)) return msg = "dfa_regex: empty language: the pattern matches no string", -1;
        if (stop_byte >= 0) {
            for (int q = 0; q < t.Q(); q++)
                if (t.trans[(size_t)q * 256 + stop_byte] >= 0) {
                    snprintf(buf, sizeof(buf), "dfa_regex: the pattern can match the stop byte 0x%02x: a stream ends at its first drawn stop byte", stop_byte);
                    return msg = buf, -1;
                }
            // L followed by the stop byte: one new final state, the only accepting one, looping on the stop byte alone
            const int fin = t.Q();
            for (int q = 0; q < fin; q++)
                if (t.acc[q]) t.trans[(size_t)q * 256 + stop_byte] = fin, t.acc[q] = 0;
            t.trans.resize(t.trans.size() + 256, -1);
            t.acc.push_back(1);
            t.trans[(size_t)fin * 256 + stop_byte] = fin;
            finish(t); // (already minimal: this numbers the new state)
        }
        return emit(t, next, accept, cap, "dfa_regex", msg);
    } catch (const Error &err) {
        if (error_pos) *error_pos = err.pos;
        msg = "dfa_" + err.msg;
        return -1;
    }
}

int32_t intersect(const uint16_t *a, int32_t qa, const uint8_t *acc_a, const uint16_t *b, int32_t qb, const uint8_t *acc_b,
                  uint16_t *next, uint8_t *accept, int32_t cap, std::string &msg) {
    char buf[200];
    const uint16_t *tabs[2] = {a, b};
    const int32_t qs[2] = {qa, qb};
    for (int k = 0; k < 2; k++) { // the checks of lstm_hip_dfa_restrict
        if (!tabs[k]) return msg = "dfa_intersect: null table", -1;
        if (qs[k] < 1 || qs[k] > MAX_STATES) {
            snprintf(buf, sizeof(buf), "dfa_intersect: states must be in [1, 4096] (got %d)", qs[k]);
            return msg = buf, -1;
        }
        for (size_t e = 0; e < (size_t)qs[k] * 256; e++)
            if (tabs[k][e] != 0xFFFF && tabs[k][e] >= qs[k]) {
                snprintf(buf, sizeof(buf), "dfa_intersect: entry next[%zu][%zu] = %u of table %c is neither a state below %d nor 0xFFFF", e / 256,
                         e % 256, (unsigned)tabs[k][e], k ? 'b' : 'a', qs[k]);
                return msg = buf, -1;
            }
    }
    std::unordered_map<uint32_t, int> ids; // (qa' << 12 | qb') -> product state
    std::vector<uint32_t> pairs;
    Table t;
    bool full = false;
    auto intern = [&](uint32_t pa, uint32_t pb) {
        const uint32_t key = pa << 12 | pb;
        auto it = ids.find(key);
        if (it != ids.end()) return it->second;
        if ((int)pairs.size() >= WORK_STATES) return full = true, 0;
        const int id = (int)pairs.size();
        ids.emplace(key, id);
        pairs.push_back(key);
        t.acc.push_back((!acc_a || acc_a[pa]) && (!acc_b || acc_b[pb]));
        t.trans.resize(t.trans.size() + 256, -1);
        return id;
    };
    intern(0, 0);
    for (size_t q = 0; q < pairs.size() && !full; q++) {
        const uint32_t pa = pairs[q] >> 12, pb = pairs[q] & 4095;
        for (int c = 0; c < 256; c++) {
            const uint16_t va = a[(size_t)pa * 256 + c], vb = b[(size_t)pb * 256 + c];
            if (va != 0xFFFF && vb != 0xFFFF) {
                const int id = intern(va, vb);
                t.trans[q * 256 + c] = id;
            }
        }
    }
    if (full) {
        snprintf(buf, sizeof(buf), "dfa_intersect: too many states: the product passed its work limit (%d states before minimisation)", WORK_STATES);
        return msg = buf, -1;
    }
    if (!finish(t)) return msg = "dfa_intersect: empty language: no string is accepted by both tables", -1;
    return emit(t, next, accept, cap, "dfa_intersect", msg);
}

} // namespace dfa
