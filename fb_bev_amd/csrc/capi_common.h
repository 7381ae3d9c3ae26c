// capi_common.h -- helpers shared by the translation units of the C ABI (capi.hip, capi_train.hip)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "rt.h"
#include "../../include/fbbev.h"

#define FBBEV_CHECK_LAUNCH()                      \
    do {                                          \
        int e_ = fbbev_rt_last_error();           \
        if (e_ != 0) return e_;                   \
    } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ------------------------------------------------------------------------------ environment knobs (docs/KNOBS.md)
// The library reads its environment here and nowhere else (tests/test_knobs_documented.py holds the names against docs/KNOBS.md).
// fbbev_env_int: the variable through atoi (text that is no number reads as 0), `dflt` when it is unset.
// fbbev_env_str: the variable's text, nullptr when it is unset.
static inline int fbbev_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline const char* fbbev_env_str(const char* name) { return getenv(name); }

// When a knob is read is part of its contract:
//   static const T v = <read>;          once per process in every build (a function-local static: thread-safe)
//   FBBEV_KNOB_ONCE(T, v, <read>);      once per process in the product; on every call in the CPU emulator build
//                                       (FBBEV_TEST_OVERRIDES), whose tests switch the knob inside one process
//   const T v = <read>;                 on every call in every build (docs/KNOBS.md lists these)
//   FBBEV_KNOB_EMU_INT(name, dflt)      the CPU emulator build reads it on every call; the product has no such knob: `dflt`
#ifdef FBBEV_TEST_OVERRIDES
#define FBBEV_KNOB_ONCE(type, var, read) const type var = (read)
#define FBBEV_KNOB_EMU_INT(name, dflt) fbbev_env_int(name, dflt)
#else
#define FBBEV_KNOB_ONCE(type, var, read) static const type var = (read)
#define FBBEV_KNOB_EMU_INT(name, dflt) (dflt)
#endif

// ------------------------------------------------------------------------------ row operands
// p: rows of `width` floats, *stride floats apart (0 = dense: becomes `width`), read or written 16 bytes at a time.
// FBBEV_E_BADARG when the rows would overlap, FBBEV_E_UNSUPPORTED when the 16-byte accesses cannot take them, else 0.  The caller
// has dealt with a null p (an optional operand that is absent is not checked and its stride is left alone).
static inline int row_operand(const void* p, long long* stride, long long width) {
    if (*stride == 0) *stride = width;
    if (*stride < width) return FBBEV_E_BADARG;
    if (*stride % 4 != 0 || !aligned16(p)) return FBBEV_E_UNSUPPORTED;
    return 0;
}
// Operands that an entry checks side by side (every stride is compared with its width before any alignment is looked at):
// FBBEV_E_BADARG of either one comes first.
static inline int row_worse(int a, int b) { return (a == FBBEV_E_BADARG || b == FBBEV_E_BADARG) ? FBBEV_E_BADARG : (a ? a : b); }

// ------------------------------------------------------------------------------ launches with dynamic LDS
// FBBEV_LAUNCH of `kern` with lds_bytes of dynamic LDS; more than 64 KiB must be opted into per kernel first (160 KiB per CU on
// gfx950), and a refusal is returned to the caller.  A kernel name with commas in its template arguments goes in parentheses.
#define FBBEV_LAUNCH_DYN_LDS(kern, grid, block, lds_bytes, stream, ...)                        \
    do {                                                                                       \
        if ((size_t)(lds_bytes) > 64 * 1024) {                                                 \
            const int e_lds_ = fbbev_rt_allow_dyn_lds((const void*)(kern), (lds_bytes));       \
            if (e_lds_) return e_lds_;                                                         \
        }                                                                                      \
        FBBEV_LAUNCH(kern, grid, block, lds_bytes, stream, __VA_ARGS__);                       \
    } while (0)
