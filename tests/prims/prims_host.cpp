// TEST-ONLY host build of the primitive dispatcher (prims_core.h), one record after another.  Built twice by tests/prims/build.py:
// g++ (libbppp_prims_gcc.so: the code path of the tests/emul emulation) and ROCm's clang++ (libbppp_prims_clang.so: the
// __builtin_addc / __builtin_subc carry chains of the device build).  Both carry the magnitude in every field element and assert it.
#include <assert.h>
#include <execinfo.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "prims_core.h"

#define PRIMS_API extern "C" __attribute__((visibility("default")))

PRIMS_API int prims_record_words(int which) { return which == 0 ? PRIM_IN_WORDS : PRIM_OUT_WORDS; }
// 1 when this library was compiled by clang (the addc/subc builtins path of field.h), 0 for g++
PRIMS_API int prims_is_clang(void) {
#if defined(__clang__)
    return 1;
#else
    return 0;
#endif
}
PRIMS_API int prims_run_host(const uint32_t* in, uint32_t* out, size_t n, const uint8_t* bytes, size_t nbytes) {
    for (size_t r = 0; r < n; r++) {
        const uint32_t* rin = in + r * PRIM_IN_WORDS;
        prims::prim_eval(rin[0], rin, out + r * PRIM_OUT_WORDS, bytes, nbytes);
    }
    return 0;
}
