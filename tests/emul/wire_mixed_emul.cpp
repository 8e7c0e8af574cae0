// TEST-ONLY host emulation of k_wire_expand_mixed (bp_pp_amd/csrc/wire_mixed_core.h): the exact __host__ __device__ lane function the
// kernel calls, compiled with g++ and run over every lane of a call, one "thread" after the other in ascending or descending order.
// The inputs are copied to the END of page-aligned mappings that are followed by an inaccessible page, and the outputs are written
// through such mappings too, so a lane that reads or writes behind a buffer's last byte faults instead of passing unseen.
#include <sys/mman.h>
#include <unistd.h>

#include <cstdlib>
#include <cstring>

#include "../../bp_pp_amd/csrc/plan_core.h"      // (before the device headers: field.h pulls <stdio.h> in inside its namespace in the host build)
#include "../../bp_pp_amd/csrc/wire_mixed_core.h"

using namespace bppp;

namespace {
// `bytes` bytes that end where a page begins that no access is allowed to
struct Guarded {
    uint8_t* map = nullptr;
    size_t map_bytes = 0;
    uint8_t* p = nullptr;
    bool take(size_t bytes) {
        const size_t page = (size_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
        map_bytes = body + page;
        void* m = mmap(nullptr, map_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) { map = nullptr; return false; }
        map = (uint8_t*)m;
        if (mprotect(map + body, page, PROT_NONE) != 0) return false;
        p = map + body - bytes;
        return true;
    }
    ~Guarded() { if (map) munmap(map, map_bytes); }
};
}  // namespace

extern "C" {

unsigned long long emul_wire_mixed_lanes(size_t n, int k_max, int rounds, int ns) {
    WireMixed m;
    memset(&m, 0, sizeof m);
    m.n = n; m.k_max = (u32)k_max; m.rounds = (u32)rounds; m.ns = (u32)ns;
    return wire_mixed_lanes(m);
}

// com33 [com33_bytes], proofs33 [proofs33_bytes]: the 33-byte slots of n instances, possibly cut short behind what the last instance
// uses.  com64 [n k_max 64], proofs64 [n (64 (4 + 2 rounds + k_max) + 32 ns)]: read as the pre-filled state, written with the result
// (a multiple of 4 bytes each, so the guarded copies keep the 4-byte alignment of the library's buffers).  0, or -1 without memory.
int emul_wire_expand_mixed(const uint8_t* com33, size_t com33_bytes, const uint8_t* proofs33, size_t proofs33_bytes, uint8_t* com64,
                           uint8_t* proofs64, const uint8_t* ks, size_t n, int k_max, int rounds, int ns, int descending) {
    const size_t c64 = n * (size_t)k_max * 64, p64 = n * (64 * (4 + 2 * (size_t)rounds + k_max) + 32 * (size_t)ns);
    Guarded gc33, gp33, gc64, gp64, gks;
    if (!gc33.take(com33_bytes) || !gp33.take(proofs33_bytes) || !gc64.take(c64) || !gp64.take(p64) || !gks.take(n)) return -1;
    memcpy(gc33.p, com33, com33_bytes);
    memcpy(gp33.p, proofs33, proofs33_bytes);
    memcpy(gc64.p, com64, c64);
    memcpy(gp64.p, proofs64, p64);
    memcpy(gks.p, ks, n);
    WireMixed m;
    m.com33 = gc33.p; m.proofs33 = gp33.p; m.com64 = gc64.p; m.proofs64 = gp64.p; m.ks = gks.p;
    m.n = n; m.k_max = (u32)k_max; m.rounds = (u32)rounds; m.ns = (u32)ns;
    const u64 lanes = wire_mixed_lanes(m);
    if (descending) for (u64 g = lanes; g-- > 0;) wire_mixed_expand_lane(m, g);
    else for (u64 g = 0; g < lanes; g++) wire_mixed_expand_lane(m, g);
    memcpy(com64, gc64.p, c64);
    memcpy(proofs64, gp64.p, p64);
    return 0;
}

}  // extern "C"
