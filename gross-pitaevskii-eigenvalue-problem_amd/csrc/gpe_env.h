// gpe_env.h -- how the GPE_* run-time switches are parsed.  Host only.  Every read of a switch in gpe_engine.hip and gpe_wide.hip is one
// call of a reader below, the switch's name a string literal at the call (tests/test_switch_table_cpu.py finds them that way).
// atoi / atoll throughout: text that is no number reads as 0.
#pragma once
#include <stdint.h>
#include <stdlib.h>

static inline bool env_set(const char* name) { return getenv(name) != nullptr; }                                  // present at all, whatever it holds
static inline bool env_on(const char* name) { const char* v = getenv(name); return !(v && atoi(v) == 0); }        // default on: only 0 turns it off
static inline bool env_opt_in(const char* name) { const char* v = getenv(name); return v && atoi(v) != 0; }       // default off: only non-zero turns it on
// unset: dflt; otherwise the value as it reads, unchecked
static inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static inline int64_t env_i64(const char* name, int64_t dflt) { const char* v = getenv(name); return v ? atoll(v) : dflt; }
// unset or outside [lo, hi]: dflt
static inline int env_int_in(const char* name, int dflt, int lo, int hi) { const int x = env_int(name, dflt); return (x < lo || x > hi) ? dflt : x; }
static inline int64_t env_i64_in(const char* name, int64_t dflt, int64_t lo, int64_t hi) { const int64_t x = env_i64(name, dflt); return (x < lo || x > hi) ? dflt : x; }
