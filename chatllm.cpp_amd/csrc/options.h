// options.h -- the CLLM_* environment switches, read through ONE validated table (options.def; parsed by options.cpp, plain C++ without HIP).
// The first query of any switch parses the whole environment once and says on stderr, each line once, what does not mean what its author may think: names that begin
// with CLLM_ and are not registered (with the nearest registered name), values a switch does not accept (with what is used instead), presence switches set to 0, and
// every set switch that changes numerics.  With nothing set nothing is printed.
// A `latched` switch keeps the value of that first pass; a `live` one is read from the environment again at every query, by the same rule (options.def says which).
#pragma once

#include <stddef.h>

enum cllm_opt {
#define CLLM_OPTION(name, scope, kind, def, accept, bad, when, numerics, desc) OPT_##name,
#include "options.def"
#undef CLLM_OPTION
    OPT_COUNT
};
enum { OPT_KIND_PRESENCE, OPT_KIND_INT, OPT_KIND_REAL, OPT_KIND_WORD };

bool         opt_is_set(cllm_opt id);      // any kind: the variable is in the environment
int          opt_int(cllm_opt id);         // int
double       opt_real(cllm_opt id);        // real
const char * opt_str(cllm_opt id);         // word: the accepted word, else the default; never null
// for the by-name C ABI (cllm_option_*): the switch of that name, -1 when it is not registered; its kind
int          opt_find(const char * name);
int          opt_kind(cllm_opt id);
// the table as text, one switch per line, tab-separated: name, scope, kind, default, accept, bad, when, numerics, set (0 / 1), the current value, description.
// Returns the length needed (without the terminating 0); writes at most size bytes.
size_t       opt_describe(char * buf, size_t size);
