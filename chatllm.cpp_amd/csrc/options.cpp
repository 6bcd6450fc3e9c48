// options.cpp -- the one place that reads the environment (options.h).  Plain C++: no HIP, no other file of the library; `g++ -c options.cpp` is all it needs.
#include "options.h"

#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>

extern char ** environ;

namespace {

enum { SCOPE_lib, SCOPE_host, SCOPE_python };
enum { KIND_presence = OPT_KIND_PRESENCE, KIND_int = OPT_KIND_INT, KIND_real = OPT_KIND_REAL, KIND_word = OPT_KIND_WORD };
enum { BAD_none, BAD_fallback, BAD_clamp, BAD_strict };
enum { WHEN_latched, WHEN_live };
enum { NUM_no, NUM_yes };
const char * const k_scope[] = { "lib", "host", "python" }, * const k_kind[] = { "presence", "int", "real", "word" }, * const k_bad[] = { "none", "fallback", "clamp", "strict" },
           * const k_when[] = { "latched", "live" }, * const k_num[] = { "no", "yes" };

struct row { const char * name; int scope, kind; const char * def, * accept; int bad, when, numerics; const char * desc; };
const row k_rows[OPT_COUNT] = {
#define CLLM_OPTION(name, scope, kind, def, accept, bad, when, numerics, desc) { #name, SCOPE_##scope, KIND_##kind, def, accept, BAD_##bad, WHEN_##when, NUM_##numerics, desc },
#include "options.def"
#undef CLLM_OPTION
};

struct value { bool set; int i; double r; const char * s; };
value g_val[OPT_COUNT];               // the first pass's result: what a latched switch is for the rest of the process
char  g_words[OPT_COUNT][32];         // a word switch's accept list, the bars replaced by 0: where opt_str's results live
std::once_flag g_once;

const char * word_match(int id, const char * s) {
    for (const char * p = g_words[id]; *p; p += strlen(p) + 1) if (!strcmp(p, s)) return p;
    return nullptr;
}
// accept: "" any, "lo..hi" (either end may be missing), "a|b|c"
bool int_accepted(const char * acc, long v, long & lo, long & hi) {
    lo = INT_MIN; hi = INT_MAX;
    if (!*acc) return true;
    if (const char * dd = strstr(acc, "..")) {
        if (dd != acc) lo = atol(acc);
        if (dd[2]) hi = atol(dd + 2);
        return v >= lo && v <= hi;
    }
    for (const char * p = acc; p; p = strchr(p, '|'), p = p ? p + 1 : p) if (atol(p) == v) return true;
    return false;
}

// THE rule: what `s` (the variable's text; null = unset) means for switch id.  The first pass and every live query go through it.  why (may be null): what a
// warning has to say about a value that is not taken as written, "" otherwise.
value parse(int id, const char * s, char * why, size_t why_len) {
    const row & o = k_rows[id];
    value v = { s != nullptr, 0, 0.0, o.def };
    if (why && why_len) why[0] = 0;
    auto say = [&](const char * fmt, ...) { if (why) { va_list ap; va_start(ap, fmt); vsnprintf(why, why_len, fmt, ap); va_end(ap); } };
    if (o.scope == SCOPE_python) return v;
    const char * t = s ? s : o.def;
    char * end = nullptr;
    switch (o.kind) {
    case KIND_int: {
        v.i = (int) strtol(t, &end, 10);                       // = atoi
        const bool number = end != t && !*end;
        const int def = atoi(o.def);
        long lo, hi;
        if (!s) break;
        if (!number && o.bad == BAD_strict) { v.i = def; say("is not a number: the default %d is used", def); }
        else if (!int_accepted(o.accept, v.i, lo, hi)) {
            const int use = o.bad == BAD_clamp ? (int)(v.i < lo ? lo : hi) : def;
            say("is not in %s: %d is used", o.accept, use);
            v.i = use;
        } else if (!number) say("is not a number: read as %d, the way atoi reads it", v.i);
        break;
    }
    case KIND_real:
        v.r = strtod(t, &end);                                 // = atof
        if (s && (end == t || *end)) say("is not a number: read as %g", v.r);
        break;
    case KIND_word:
        if (!s) break;
        if (const char * w = word_match(id, s)) v.s = w;
        else say("is not one of %s: %s%s is used", o.accept, *o.def ? "the default " : "the meaning of the unset switch", o.def);
        break;
    }
    return v;
}

void value_text(int id, const value & v, char * buf, size_t n) {
    const row & o = k_rows[id];
    if (o.scope == SCOPE_python) { const char * s = getenv(o.name); snprintf(buf, n, "%.60s", s ? s : ""); return; }
    switch (o.kind) {
    case KIND_presence: snprintf(buf, n, "%s", v.set ? "on" : "off"); break;
    case KIND_int:      snprintf(buf, n, "%d", v.i); break;
    case KIND_real:     snprintf(buf, n, "%g", v.r); break;
    default:            snprintf(buf, n, "%s", v.s); break;
    }
}

// Levenshtein distance of two names of at most 63 characters
int edit_distance(const char * a, size_t na, const char * b, size_t nb) {
    int prev[64], cur[64];
    for (size_t j = 0; j <= nb; j++) prev[j] = (int) j;
    for (size_t i = 1; i <= na; i++) {
        cur[0] = (int) i;
        for (size_t j = 1; j <= nb; j++) {
            const int sub = prev[j - 1] + (a[i - 1] != b[j - 1]), del = prev[j] + 1, ins = cur[j - 1] + 1;
            cur[j] = sub < del ? (sub < ins ? sub : ins) : (del < ins ? del : ins);
        }
        memcpy(prev, cur, (nb + 1) * sizeof(int));
    }
    return prev[nb];
}

int find_n(const char * name, size_t n) {
    for (int id = 0; id < OPT_COUNT; id++) if (strlen(k_rows[id].name) == n && !memcmp(k_rows[id].name, name, n)) return id;
    return -1;
}

void first_pass() {
    for (int id = 0; id < OPT_COUNT; id++) {
        if (k_rows[id].kind != KIND_word) continue;
        snprintf(g_words[id], sizeof(g_words[id]) - 1, "%s", k_rows[id].accept);       // (the last byte stays 0: the list ends with an empty word)
        for (char * p = g_words[id]; *p; p++) if (*p == '|') *p = 0;
    }
    char why[160], text[64];
    for (int id = 0; id < OPT_COUNT; id++) {
        const row & o = k_rows[id];
        const char * s = getenv(o.name);
        g_val[id] = parse(id, s, why, sizeof(why));
        if (!s || o.scope == SCOPE_python) continue;
        if (why[0]) fprintf(stderr, "[cllm] warning: %s=%.40s %s\n", o.name, s, why);
        if (o.kind == KIND_presence && (!*s || !strcmp(s, "0"))) fprintf(stderr, "[cllm] warning: %s=%s is a presence switch: any value, including 0, turns it on; unset it instead\n", o.name, s);
        if (o.numerics == NUM_yes) { value_text(id, g_val[id], text, sizeof(text)); fprintf(stderr, "[cllm] note: %s is set and changes numerics: %s is used\n", o.name, text); }
    }
    for (char ** e = environ; e && *e; e++) {
        if (strncmp(*e, "CLLM_", 5)) continue;
        const char * eq = strchr(*e, '=');
        const size_t n = eq ? (size_t)(eq - *e) : strlen(*e);
        if (find_n(*e, n) >= 0) continue;
        int best = -1, best_d = 3;
        if (n < 64) for (int id = 0; id < OPT_COUNT; id++) {
            const int d = edit_distance(*e, n, k_rows[id].name, strlen(k_rows[id].name));
            if (d < best_d) { best = id; best_d = d; }
        }
        if (best >= 0) fprintf(stderr, "[cllm] warning: %.*s is not a registered switch and is ignored: did you mean %s?\n", (int) n, *e, k_rows[best].name);
        else           fprintf(stderr, "[cllm] warning: %.*s is not a registered switch and is ignored\n", (int)(n < 64 ? n : 64), *e);
    }
}

value current(int id) {
    std::call_once(g_once, first_pass);
    return k_rows[id].when == WHEN_live ? parse(id, getenv(k_rows[id].name), nullptr, 0) : g_val[id];
}

}  // namespace

bool         opt_is_set(cllm_opt id) { return current(id).set; }
int          opt_int(cllm_opt id)    { return current(id).i; }
double       opt_real(cllm_opt id)   { return current(id).r; }
const char * opt_str(cllm_opt id)    { return current(id).s; }
int          opt_find(const char * name) { return name ? find_n(name, strlen(name)) : -1; }
int          opt_kind(cllm_opt id)   { return k_rows[id].kind; }

size_t opt_describe(char * buf, size_t size) {
    size_t need = 0;
    char line[1024], text[64];
    for (int id = 0; id < OPT_COUNT; id++) {
        const row & o = k_rows[id];
        const value v = current(id);
        value_text(id, v, text, sizeof(text));
        const int n = snprintf(line, sizeof(line), "%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%d\t%s\t%s\n", o.name, k_scope[o.scope], k_kind[o.kind], o.def, o.accept, k_bad[o.bad], k_when[o.when],
                               k_num[o.numerics], (int) v.set, text, o.desc);
        const size_t len = n < 0 ? 0 : (size_t) n < sizeof(line) ? (size_t) n : sizeof(line) - 1;
        if (buf && need < size) { const size_t room = size - need - 1, k = len < room ? len : room; memcpy(buf + need, line, k); buf[need + k] = 0; }
        need += len;
    }
    return need;
}
