// Which kernels a u64 verify / prove call of n proofs runs -- as ONE pure function of (n, SIMDs of the device, switches), with no HIP in
// it.  bppp_u64.hip's launch sequences take their decisions from the struct this returns and from nowhere else; the library exports the
// function (bppp_u64_plan, include/bppp.h) and remembers the plan of a context's last call ("last_verify_plan" / "last_prove_plan"
// of bppp_ctx_get_option), so tests can (a) check on the CPU that the plan is total and changes exactly at the documented sizes and
// (b) assert on the GPU that a batch of T-1, T, T+1 proofs really took the regime it was meant to exercise.
//
// The regimes exist because one lane per proof fills an MI355X (S = 1,024 SIMDs, 64 lanes each, two wavefronts per SIMD under the
// 256-register cap) only from 2^17 proofs up; below that a call's dependent chains are cut across lanes, and kernels whose data flow
// allows it share the SIMDs.  With S = 1,024:
//
//   verify  n <= S          (1,024)    "split4": a wavefront per fixed-base sum, 64 lanes per C0 sum, 16 per round, 4 table sets per proof
//           n <= 4 S        (4,096)    "split2": the same on 32 / 8 lanes, 2 table sets
//           n <= 16 S       (16,384)   lane groups of 4 for the variable-base sums; tables (a lane per point) on the helper stream
//           n <= 32 S       (32,768)   rounds on 2 lanes per proof; one-lane table kernel beside phase 1
//           n <= 64 S       (65,536)   one lane per proof in uncapped builds; tables beside phase 1; last round's sum beside the final sum
//           n <  128 S      (131,072)  the 256-register builds, 8 lanes per fixed-base sum
//           n >= 128 S                 one lane per fixed-base sum; up to 288 S (a chip filled once or twice) as TWO half-batch chains of
//                                      kernels that leapfrog on the SIMDs (twin), and up to 128 S with progress-paced wave priority (pace)
//   prove   n <= S: a wavefront per sum, wide round scalars | n <= 4 S: 16-lane stages and folds | n <= 16 S: 4-lane stages and folds |
//           n <= 32 S: next commitment from fixed-base sums | n <= 128 S: round scalars in four parts | n >= 128 S: one lane per sum;
//           the 256-register builds from more than 64 S values (one wavefront per SIMD) on
//
// The generic verifiers (WNLA, reciprocal, circuit: bppp_generic.hip) take theirs from plan_generic below in the same way; its code is
// "last_generic_form" of bppp_ctx_get_option (include/bppp.h has the bits).  n instances, blocks = ceil(n / 64):
//   all         n <= S           4 sets of round-point tables per instance, rounds on 16 lanes    | n <= 4 S: 2 sets, 8 lanes
//               n <= 8 S         a wavefront per fixed-base sum, 8 lanes beyond
//               n <= 16 S        rounds on 4 lanes per instance (4 blocks <= S)                    | n <= 32 S: 2 lanes | 1
//               n <= 32 S        final scalars on 8 lanes per instance (8 blocks <= 4 S)           | n <= 64 S: 4 | n <= 128 S: 2 | 1,
//                                and never more than 2^(rounds - 1)
//   reciprocal  n <= 8 S         phase 1 on 8 lanes per instance (2 G blocks <= S)                 | n <= 16 S: 4 | n <= 32 S: 2 | 1
//               n <= 32 S        round-point tables and C0's variable-base sum on the helper stream beside phase 1 (2 blocks <= S)
//               n >= 128 S       one lane per fixed-base sum
//   circuit     n <= 16 S        C0's variable-base sum on a lane per point (L blocks <= 2 S; L = 8 for up to 8 points)
//   aggregate   (the aggregated reciprocal range proof, agg_core.h) phase 1's lanes, `beside` and the one-lane fixed-base sums as for the
//               reciprocal verifier; C0's variable-base sum over its 4 + k points on one lane per instance, five points per pass
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace bppp_host {

static const unsigned PLAN_BLOCK = 64;          // BPPP_BLOCK: lanes of a one-lane-per-proof workgroup (checked against kernels.h in bppp_u64.hip)

struct PlanKnobs {
    int n_simds = 1024;
    bool no_small = false, no_lane_groups = false, no_split = false, timing = false;
    int tables_beside = -1, tail_beside = -1, fb_one_lane_mode = -1, next_overlap = -1;      // diagnostics: -1 = by size
    long next_msm_max = -1, lane_forms_max = -1, lane4_max = -1, scal_parts_max = -1;       // diagnostics: -1 = by n_simds
    int shared_inv = -1;         // diagnostics: proofs per shared inversion (0 none, 2 4 8 16) wherever the one-lane kernels run; -1 = by size
    int twin = -1;               // diagnostics: 1 = two half-batch sequences wherever the form allows it, 0 = never; -1 = by size
    int pace = -1;               // diagnostics: 1 = progress-paced wave priority in the one-lane sums always, 0 = never; -1 = by size
};

enum PlanTables { TABLES_INLINE = 0, TABLES_ASIDE, TABLES_BESIDE };        // on the main stream | lane-per-point kernel on the helper stream | one-lane kernel beside phase 1
enum PlanPhase1 { P1_FULL = 0, P1_SMALL, P1_WG4, P1_G16 };                 // 256-register build | uncapped | 256-thread workgroups (beside the tables) | 16 lanes per proof
enum PlanFb { FB_L8 = 0, FB_L1, FB_L64, FB_L4 };                           // lanes per fixed-base sum (FB_L1 also means: C0's two halves one after the other, not side by side)
enum PlanC0Var { C0V_FULL = 0, C0V_SMALL, C0V_G4, C0V_G32, C0V_G64 };
enum PlanRound { R_FULL = 0, R_SMALL, R_G2, R_G4, R_G8, R_G16 };

struct VerifyPlan {
    bool split = false;          // at most 4 proofs per SIMD: chains cut across lanes, `parts` table sets per proof
    int parts = 1;
    bool small = false;          // the grid is at most one wavefront per SIMD: uncapped register builds
    int tables = TABLES_INLINE, tparts = 1;
    int phase1 = P1_FULL, fb = FB_L8, c0var = C0V_FULL, round = R_FULL;
    bool tail_beside = false;    // round 4 as head + tail, final scalars and final sum on the helper stream
    bool final_scalars_g16 = false;
    size_t vtab_sets = 1;        // window-table sets per proof the call needs room for
    int shared_inv = 0;          // G = 2, 4, 8, 16: the field inversions of the table build and of the rounds are taken once per G proofs by
                                 // kernels of their own between the passes (straus_core.h: fe_batch_inv_lane); 0: every lane inverts for itself
    int twin = 1;                // 2: the batch runs as TWO half-batch launch sequences on two stream pairs (each half on the plan plan_verify_half
                                 // gives it); the other fields then describe a half.  1: one sequence
    int pace = 0;                // 1: the one-lane variable-base sums lower their wave priority as they advance (straus_core.h: straus_pace); 2: the one-lane fixed-base sums too (fb_core.h: fb_pace)
    uint32_t code() const {
        const uint32_t lg = shared_inv >= 16 ? 4 : shared_inv >= 8 ? 3 : shared_inv >= 4 ? 2 : shared_inv >= 2 ? 1 : 0;
        return (uint32_t)phase1 | (uint32_t)tables << 4 | (uint32_t)tparts << 8 | (uint32_t)fb << 12 | (uint32_t)c0var << 16 | (uint32_t)round << 20 |
               (uint32_t)(tail_beside ? 1 : 0) << 24 | (uint32_t)(small ? 1 : 0) << 25 | (uint32_t)(split ? 1 : 0) << 26 | lg << 27 |
               (uint32_t)(twin == 2 ? 1 : 0) << 30 | (uint32_t)(pace ? 1 : 0) << 31;        // (pace 2 is a diagnostic: described as pace=1)
    }
};

inline VerifyPlan plan_verify(size_t n, const PlanKnobs& k, bool rlc) {
    VerifyPlan p;
    const size_t S = (size_t)(k.n_simds > 0 ? k.n_simds : 1);
    const size_t blocks = (n + PLAN_BLOCK - 1) / PLAN_BLOCK;
    const bool lanes_ok = !k.no_small && !k.no_lane_groups && !k.no_split;
    p.split = lanes_ok && n <= 4 * S;
    // four parts per GLV stream up to one proof per SIMD, two beyond (the extra lanes start to queue: 4,096 proofs 4.3 ms in two parts, 5.1 in four)
    p.parts = p.split ? (n <= S ? 4 : 2) : 1;
    p.vtab_sets = (size_t)p.parts;
    p.small = !k.no_small && blocks <= S;
    // batches the lane groups serve (up to 16 proofs per SIMD) build their tables a lane per point on the helper stream while phase 1 runs
    const bool aside = p.split || (lanes_ok && 4 * blocks <= S);
    // ... the sizes above, while the one-lane kernels are a lone wavefront per SIMD, run the ONE-lane table kernel beside phase 1
    const bool beside = !aside && !k.timing && (k.tables_beside >= 0 ? k.tables_beside == 1 : (!k.no_split && !k.no_small && blocks <= S));
    p.tables = aside ? TABLES_ASIDE : beside ? TABLES_BESIDE : TABLES_INLINE;
    p.tparts = p.split ? p.parts : 1;
    p.phase1 = p.split ? P1_G16 : beside ? P1_WG4 : p.small ? P1_SMALL : P1_FULL;
    const bool fb_one_lane = k.fb_one_lane_mode >= 0 ? k.fb_one_lane_mode == 1 : n >= 128 * S;
    p.fb = p.split ? FB_L64 : fb_one_lane ? FB_L1 : FB_L8;
    const bool grouped = !k.no_lane_groups && 4 * blocks <= S;
    const bool pairs = !k.no_lane_groups && 2 * blocks <= S;
    p.c0var = p.split ? (p.parts == 4 ? C0V_G64 : C0V_G32) : grouped ? C0V_G4 : p.small ? C0V_SMALL : C0V_FULL;
    p.round = p.split ? (p.parts == 4 ? R_G16 : R_G8) : grouped ? R_G4 : pairs ? R_G2 : p.small ? R_SMALL : R_FULL;
    const bool one_lane_rounds = !p.split && !grouped && !pairs;
    p.tail_beside = !rlc && !k.timing && one_lane_rounds && (k.tail_beside >= 0 ? k.tail_beside == 1 : (p.small && !k.no_split));
    p.final_scalars_g16 = p.split;
    // Shared inversions: where the one-lane kernels run with four or more wavefronts per SIMD, a separate launch of n / G lanes that
    // inverts for G proofs each replaces 8 of the 9 field inversions a proof costs (4 in the table build, 4 in the rounds).  Such a
    // launch takes what ONE inversion takes (0.15 ms, a lone wavefront per SIMD) however many proofs there are, the inversions it
    // replaces 0.33 ms per 2^20 proofs: 2^20 proofs 147.6 -> 144.8 ms, 2^19 75.8 -> 74.8, 2^18 38.0 -> 37.6, nothing at 2^17
    // (profiles/r05/r05_q_ab_shared_inv.txt), so it starts at 256 S.
    const bool one_lane_all = p.round == R_FULL && p.tables == TABLES_INLINE && p.c0var == C0V_FULL;
    const int by_size = n >= 1024 * S ? 16 : n >= 256 * S ? 8 : 0;
    const int want = k.shared_inv >= 0 ? k.shared_inv : by_size;
    p.shared_inv = !one_lane_all ? 0 : want >= 16 ? 16 : want >= 8 ? 8 : want >= 4 ? 4 : want >= 2 ? 2 : 0;
    // A launch that fills the chip exactly once or twice ends in a long tail: the arbiter serves the older wavefront of a SIMD's pair
    // first, so one finishes early and its partner runs on alone at a lone wavefront's issue rate -- 41 % of the SIMD-time of the rounds
    // at 2^17 proofs (profiles/r06/r06_a_wave_timeline.txt), 9 % over the saturated rate for the whole call.  Two remedies, both plan fields:
    //   twin: the batch as two halves, each a launch sequence of its own on its own stream pair.  A SIMD then holds one wavefront of each
    //         half, of DIFFERENT kernels; when the older one ends, its sequence's next kernel moves in: the halves leapfrog and no SIMD
    //         is left with one wavefront except at the very end.  The halves run the 256-register one-lane kernels (plan_verify_half);
    //   pace: the sums lower their own wave priority as they advance, so that a pair ends together (straus_core.h: straus_pace).
    //   Where each pays (one box, child contexts timed in turns, profiles/r06/r06_j_twin_sizes.txt; g = wavefronts / wavefront slots):
    //   twin  g = 1 (2^17 proofs) -1.4 % on top of pace, 1.06 .. 1.25 -3 .. -6 %, 1.75 -11 %, 2 (2^18) -3.5 %, 2.25 -6 %; but +4 % at g = 1.5,
    //         +2 .. +4 % from 2.5 up (the halves' own part-filled generations collide): so up to g = 2.25, except a last generation that is
    //         30 .. 70 % full;
    //   pace  g <= 1 (one generation of pairs): -1.5 .. -2.3 %; +1.5 % beyond (a new wavefront must not outrank a half-done one).
    const size_t G = 2 * S, rem = blocks % G;
    const bool fills_once = blocks > S && blocks <= G;            // more than one wavefront per SIMD, at most two: ONE generation of pairs
    const bool twin_by_size = blocks >= G && 4 * blocks <= 9 * G && !(10 * rem > 3 * G && 10 * rem < 7 * G);
    const bool twin_ok = !rlc && !k.timing && one_lane_all && fb_one_lane && n >= 2 * PLAN_BLOCK;
    p.twin = twin_ok && (k.twin >= 0 ? k.twin == 1 : twin_by_size) ? 2 : 1;
    p.pace = !one_lane_all ? 0 : k.pace >= 0 ? k.pace : fills_once ? 1 : 0;
    return p;
}
// the plan of ONE half of a twin call (n_half proofs): the 256-register one-lane kernels and one lane per fixed-base sum whatever the
// half's size -- a half shares every SIMD with a wavefront of the other half
inline VerifyPlan plan_verify_half(size_t n_half, const PlanKnobs& k, int pace) {
    PlanKnobs h = k;
    h.no_small = true; h.fb_one_lane_mode = 1; h.tables_beside = 0; h.tail_beside = 0; h.twin = 0; h.pace = pace;
    VerifyPlan p = plan_verify(n_half, h, false);
    p.twin = 2;
    return p;
}
inline size_t twin_first_half(size_t n) { return (n / 2 + PLAN_BLOCK - 1) / PLAN_BLOCK * PLAN_BLOCK; }

enum PlanStage { ST_FULL = 0, ST_W2, ST_G4, ST_G4_W2, ST_G16, ST_G16_W2 };      // one lane (uncapped | 256 registers), 4 lanes, 16 lanes per value
enum PlanScalars { SC_ONE = 0, SC_PARTS, SC_WIDE };

struct ProvePlan {
    int fb = FB_L8;              // lanes per fixed-base sum of a single-job launch (FB_L4 is chosen per launch: fb4_from_jobs)
    int fb4_from_jobs = 0;       // a fused launch of at least this many jobs runs on 4 lanes per sum (0: never)
    bool next_by_msm = false;    // a level's commitment as E + R from fixed-base sums (else the variable-base kernel)
    bool w2 = false;             // 256-register builds of the one-lane stage / fold kernels
    int stage = ST_FULL, fold = ST_FULL;
    int scalars = SC_ONE;
    bool fold_leaves_scalars = false;      // the lane-form fold computes the next round's scalars itself
    bool overlap_next = false;   // the variable-base next commitment on the helper stream
    bool next_g4 = false;
    bool ct = false;
    uint32_t code() const {
        return (uint32_t)fb | (uint32_t)fb4_from_jobs << 4 | (uint32_t)stage << 8 | (uint32_t)fold << 12 | (uint32_t)scalars << 16 |
               (uint32_t)(next_by_msm ? 1 : 0) << 20 | (uint32_t)(w2 ? 1 : 0) << 21 | (uint32_t)(overlap_next ? 1 : 0) << 22 |
               (uint32_t)(next_g4 ? 1 : 0) << 23 | (uint32_t)(ct ? 1 : 0) << 24;
    }
};

inline ProvePlan plan_prove(size_t n, const PlanKnobs& k, bool ct) {
    ProvePlan p;
    p.ct = ct;
    const size_t S = (size_t)(k.n_simds > 0 ? k.n_simds : 1);
    const size_t blocks = (n + PLAN_BLOCK - 1) / PLAN_BLOCK;
    const bool fb_one_lane = k.fb_one_lane_mode >= 0 ? k.fb_one_lane_mode == 1 : n >= 128 * S;
    // a call of at most one value per SIMD: a wavefront per sum (6 additions per lane and a 6-step tree instead of 44 and 3)
    const bool fb_wave = !k.no_small && !k.no_split && n <= S;
    p.fb = fb_wave ? FB_L64 : fb_one_lane ? FB_L1 : FB_L8;
    // otherwise 8, 4 or 1 lanes: the fewest that still give every SIMD two wavefronts in the launch -- NJ * 4 n >= 128 S
    if (!fb_wave && !fb_one_lane) {
        for (int nj = 1; nj <= 4; nj++)
            if ((size_t)nj * 4 * n >= 128 * S) { p.fb4_from_jobs = nj; break; }
    }
    const size_t next_msm_max = k.next_msm_max >= 0 ? (size_t)k.next_msm_max : 32 * S;
    p.next_by_msm = fb_wave || (!k.no_split && !k.no_lane_groups && n <= next_msm_max);
    p.w2 = k.no_small || blocks > S;
    const size_t lane_forms_max = k.lane_forms_max >= 0 ? (size_t)k.lane_forms_max : 4 * S;
    const bool stage_lanes = !k.no_lane_groups && !k.no_split && !k.no_small && n <= lane_forms_max;
    const size_t g16_blocks = (16 * n + PLAN_BLOCK - 1) / PLAN_BLOCK, g4_blocks = (4 * n + PLAN_BLOCK - 1) / PLAN_BLOCK;
    const bool g16_w2 = g16_blocks > S;
    const bool stage_lanes4 = !stage_lanes && !k.no_lane_groups && !k.no_split && n <= (k.lane4_max >= 0 ? (size_t)k.lane4_max : 16 * S);
    const bool g4_w2 = k.no_small || g4_blocks > S;
    p.stage = stage_lanes ? (g16_w2 ? ST_G16_W2 : ST_G16) : stage_lanes4 ? (g4_w2 ? ST_G4_W2 : ST_G4) : p.w2 ? ST_W2 : ST_FULL;
    const bool fold_lanes = stage_lanes && p.next_by_msm, fold_lanes4 = stage_lanes4 && p.next_by_msm;
    p.fold = fold_lanes ? (g16_w2 ? ST_G16_W2 : ST_G16) : fold_lanes4 ? (g4_w2 ? ST_G4_W2 : ST_G4) : p.w2 ? ST_W2 : ST_FULL;
    p.fold_leaves_scalars = fold_lanes || fold_lanes4;
    const bool scal_parts = !fb_wave && !k.no_split && n <= (k.scal_parts_max >= 0 ? (size_t)k.scal_parts_max : 128 * S);
    p.scalars = fb_wave ? SC_WIDE : scal_parts ? SC_PARTS : SC_ONE;
    p.overlap_next = !k.timing && (k.next_overlap >= 0 ? k.next_overlap == 1 : 4 * blocks >= S);
    p.next_g4 = !k.no_lane_groups && 4 * blocks <= S;
    return p;
}

// ---- RLC mode: how the final checks of a batch are grouped, from what the previous RLC call on the context rejected.
// The stages (docs/design/09): bucket stage over superchunks of M proofs (Pippenger, ~ 4 ms per 2^20 proofs at M = 4096, more for
// smaller M) -> chunks of C proofs for the superchunks that failed (per proof a 64-doubling weighted commitment, ~ 7 ms per 2^20, plus
// the chunk's 49-base sum: 588 table additions shared by C proofs) -> the exact per-proof check for the chunks that failed.  A group
// passes only if every proof in it is valid: with a reject rate r a superchunk passes with probability e^(-r M), a chunk with
// e^(-r C).  Round 4 always took M = 4096 and C = 8: at r = 1/1024 every superchunk failed (its 4 ms wasted) and the chunks of 8 paid
// 74 table additions per proof where chunks of 32 pay 18.  With the rate of the previous call in hand:
//   M: the automatic size, halved while r M > 0.3 (down to 1,024: smaller bucket stages cost more than they save), no bucket stage at
//      all when even that one would fail more often than not (r M > 0.45);
//   C: 32 while a chunk of 32 still passes nine times in ten (r <= 1/256), else 8.
// rate < 0 = no history (first call, or the previous one still in flight): round 4's choice.
struct RlcPlan { unsigned super_m, chunk; };
inline RlcPlan plan_rlc(unsigned auto_super_m, bool super_is_auto, int chunk_option /* 0 auto, 8, 32 */, double rate) {
    RlcPlan p;
    p.super_m = auto_super_m;
    if (super_is_auto && auto_super_m && rate > 0) {
        unsigned m = auto_super_m;
        while (m > 1024 && rate * m > 0.3) m /= 2;
        p.super_m = rate * m > 0.45 ? 0u : m;
    }
    if (chunk_option == 8 || chunk_option == 32) p.chunk = (unsigned)chunk_option;
    else p.chunk = (rate >= 0 && rate * 256 <= 1.0) ? 32u : 8u;
    if (p.super_m % 32) p.chunk = 8;      // a superchunk is made of whole chunks (explicit sizes are multiples of 8)
    return p;
}

// "phase1=wg4 tables=beside/1 fb=l8 c0var=small round=small tail_beside=1 small=1 split=0" -- what tests assert on
inline int plan_describe(uint32_t code, bool prove, char* buf, size_t cap) {
    static const char* const P1[] = {"full", "small", "wg4", "g16"};
    static const char* const TB[] = {"inline", "aside", "beside"};
    static const char* const FB[] = {"l8", "l1", "l64", "l4"};
    static const char* const CV[] = {"full", "small", "g4", "g32", "g64"};
    static const char* const RD[] = {"full", "small", "g2", "g4", "g8", "g16"};
    static const char* const ST[] = {"full", "w2", "g4", "g4_w2", "g16", "g16_w2"};
    static const char* const SC[] = {"one", "parts", "wide"};
    auto pick = [](const char* const* t, size_t nt, uint32_t i) { return i < nt ? t[i] : "?"; };
    if (!prove)
        return std::snprintf(buf, cap, "phase1=%s tables=%s/%u fb=%s c0var=%s round=%s tail_beside=%u small=%u split=%u twin=%u pace=%u shared_inv=%u", pick(P1, 4, code & 15),
                             pick(TB, 3, (code >> 4) & 15), (code >> 8) & 15, pick(FB, 4, (code >> 12) & 15), pick(CV, 5, (code >> 16) & 15),
                             pick(RD, 6, (code >> 20) & 15), (code >> 24) & 1, (code >> 25) & 1, (code >> 26) & 1, ((code >> 30) & 1) + 1u, (code >> 31) & 1,
                             ((code >> 27) & 7) ? 1u << ((code >> 27) & 7) : 0u);
    return std::snprintf(buf, cap, "fb=%s fb4_from_jobs=%u stage=%s fold=%s scalars=%s next_by_msm=%u w2=%u overlap_next=%u next_g4=%u ct=%u",
                         pick(FB, 4, code & 15), (code >> 4) & 15, pick(ST, 6, (code >> 8) & 15), pick(ST, 6, (code >> 12) & 15), pick(SC, 3, (code >> 16) & 15),
                         (code >> 20) & 1, (code >> 21) & 1, (code >> 22) & 1, (code >> 23) & 1, (code >> 24) & 1);
}

// ---- The generic verifiers: WeightNormLinearArgument, ReciprocalRangeProofProtocol and ArithmeticCircuit for any generator-vector sizes
// (bppp_generic.hip).  All three end in the WNLA stage (tables of the round points, rounds, final scalars, final fixed-base sum); the
// reciprocal and the circuit verifier run a phase 1 and a C0 stage of their own in front of it.
struct GenericKnobs {
    int n_simds = 1024;
    bool no_lane_groups = false, no_split = false, timing = false;
    bool slow_rounds = false;          // BPPP_GENERIC_SLOW_ROUNDS: projective tables + complete additions in the rounds
    int lane_group = 0;                // BPPP_GENERIC_LANE_GROUP = 2 | 4: that many lanes per instance in the grouped kernels at any size (tests); 0 = by size
    long fb_wide_max = -1;             // diagnostic: the largest call (instances) whose fixed-base sums run a wavefront per instance; -1 = by size
    int fb_one_lane_mode = -1;         // diagnostic: the reciprocal verifier's fixed-base sums on one lane always (1) / never (0); -1 = by size
    int recip_beside = -1;             // diagnostic: the reciprocal verifier's one-lane kernels beside its fixed-base ones always (1) / never (0); -1 = by size
    int recip_p1_group = 0;            // diagnostic: 1 | 2 | 4 | 8 lanes per instance in the reciprocal verifier's phase 1; 0 = by size
};
enum { GENERIC_FORM_WNLA = 1, GENERIC_FORM_RECIPROCAL = 2, GENERIC_FORM_CIRCUIT = 3, GENERIC_FORM_AGGREGATE = 4 };
enum { GENERIC_FB_LANES8 = 0, GENERIC_FB_WAVEFRONT = 1, GENERIC_FB_ONE_LANE = 2 };

struct GenericPlan {
    int protocol = GENERIC_FORM_WNLA;
    bool fast = false;           // the rounds walk affine window tables of the round points (else: projective tables, complete additions)
    int tab_parts = 1;           // sets of round-point tables per instance: 1, or 2 / 4 with every 26-window stream cut in as many parts
    int round_group = 1;         // lanes per instance in the rounds
    int final_lg = 0;            // log2 of the lanes per instance in the final scalars
    int fb = GENERIC_FB_LANES8;  // lanes per fixed-base sum: GENERIC_FB_*
    int c0var_group = 0;         // reciprocal: lanes per instance in C0's variable-base sum (aggregate: always 1)
    int p1_group = 0;            // reciprocal, aggregate: lanes per instance in phase 1
    bool beside = false;         // reciprocal, aggregate: the round-point tables and C0's variable-base sum on the helper stream, beside phase 1
    int parts = 1;               // parts the call runs in (this is the plan of one of them)
    int c0_lanes = 0;            // circuit: lanes per instance of C0's variable-base sum on a lane per point (a power of two >= the points)
    bool per_point = false;      // circuit: C0's variable-base sum runs in that form
    int c0_chunks = 0;           // aggregate: shared-doubling passes of C0's variable-base sum, ceil((4 + k) / 5)
    // "last_generic_form" (include/bppp.h has the bit layout): each choice as the value its launch is given
    // (the protocol field has two bits: the aggregate verifier reads 0 there and sets bit 23)
    uint32_t code() const {
        return ((uint32_t)protocol & 3u) | (uint32_t)(protocol == GENERIC_FORM_AGGREGATE ? 1 : 0) << 23 | (uint32_t)tab_parts << 2 | (uint32_t)round_group << 5 | (uint32_t)final_lg << 10 | (uint32_t)fb << 12 |
               (uint32_t)p1_group << 14 | (uint32_t)(beside ? 1 : 0) << 18 | (uint32_t)parts << 19 | (uint32_t)(per_point ? 1 : 0) << 22;
    }
};

// the lanes one instance's final scalars are dealt to, as log2: what is wanted, cut to what the table of 2^rounds entries has room for
constexpr int final_scalars_lg_clip(int rounds, int want_lg) { return want_lg < rounds ? want_lg : (rounds > 0 ? rounds - 1 : 0); }
// the fast variable-base path of the rounds (window tables of the round points in the context's table buffer)
inline bool generic_fast(size_t rounds, const GenericKnobs& k) { return rounds != 0 && !k.slow_rounds; }

// Parts of a reciprocal verify call on device buffers (K chains on K streams, so that one part's fixed-base sums run under another
// part's one-lane kernels): one part with kernel timing on (the per-kernel times must add up), in RLC mode (its stages work on the
// whole batch) and for small calls; otherwise what the caller forces ("generic_parts": A/B runs, tests at small sizes), at most 4
inline int plan_generic_parts(size_t n, bool rlc, bool timing, int forced) {
    if (rlc || timing || n < 2 * PLAN_BLOCK) return 1;
    return forced > 4 ? 4 : forced > 0 ? forced : 1;
}

// n: instances of this call, or of this part of it; call_n: instances of the whole call (= n unless n_parts > 1) -- the lane-group
// choices go by the wavefronts of the WHOLE call, because the parts of a multi-part call share the chip; a part takes neither table
// parts nor the wavefront sums nor the helper stream (it is a chain on one stream).  c0_points: the 4 + k points of C0 (circuit, aggregate).
inline GenericPlan plan_generic(int protocol, size_t n, size_t rounds, const GenericKnobs& k, size_t call_n, int n_parts, size_t c0_points) {
    GenericPlan p;
    p.protocol = protocol;
    p.parts = n_parts;
    const bool part = n_parts > 1;
    const size_t S = (size_t)(k.n_simds > 0 ? k.n_simds : 1);
    const size_t blocks = (call_n + PLAN_BLOCK - 1) / PLAN_BLOCK;
    const bool groups = !k.no_lane_groups, split_ok = groups && !k.no_split;
    p.fast = generic_fast(rounds, k);
    // Sets of round-point tables: calls that leave the chip EMPTY -- at most four instances per SIMD -- cut every 26-window stream in 2
    // (4: at most one instance per SIMD) parts over tables of P and 2^65 P (P, 2^35 P, 2^70 P, 2^100 P), a lane per table, and walk a
    // round's sum on 8 (16) lanes: what such a call takes is the length of ONE instance's chain (round 6: one WNLA verify of the u64
    // size 4.1 -> ms).  The u64 verifier has done the same since round 3 (split, above).
    p.tab_parts = (part || !p.fast || !split_ok || k.lane_group) ? 1 : n <= S ? 4 : n <= 4 * S ? 2 : 1;
    // lanes per instance in the rounds: 16 / 8 over tables in 4 / 2 parts, else 4 or 2 while that still leaves wavefront slots free
    p.round_group = (!p.fast || !groups) ? 1 : p.tab_parts == 4 ? 16 : p.tab_parts == 2 ? 8 : k.lane_group ? k.lane_group :
                    4 * blocks <= S ? 4 : 2 * blocks <= S ? 2 : 1;
    // ... in the final scalars: up to 8 while the launch stays within four wavefronts per SIMD.  The work is independent per generator,
    // so unlike the rounds it divides by the full group size.  (lane_group, tests: 2 or 8 parts)
    int lg = 0;
    if (groups && k.lane_group) lg = k.lane_group == 2 ? 1 : 3;
    else if (groups) while (lg < 3 && (blocks << (lg + 1)) <= 4 * S) lg++;
    p.final_lg = final_scalars_lg_clip((int)rounds, lg);
    // The fixed-base sums.  One lane per instance from the size at which that fills the SIMDs twice over (the reciprocal verifier only).
    // A WAVEFRONT per instance instead of 8 lanes in calls of up to eight instances per SIMD, where 8 lanes per instance are at most one
    // wavefront per SIMD and the call waits for one lane's chain of (bases x windows) / 8 dependent table additions -- one instance of
    // configs[4]'s shape: k_wnla_msm 7.6 -> 0.86 ms, k_recip_c0_fixed 2.5 -> 0.32 ms; with phase 1 on lane groups the call 16.7 -> 6.1 ms
    // (round 6, profiles/r06/r06_p4_latency_recip256.txt).  By size, same shape on 16-bit tables: 2,048 instances 14.1 -> 8.4 ms, 4,096
    // 14.9 -> 11.2, 8,192 19.3 -> 18.6, 16,384 28.2 -> 28.7 (profiles/r06/r06_p5_fb_wide_sizes.txt): up to 8 S
    const bool recip_like = protocol == GENERIC_FORM_RECIPROCAL || protocol == GENERIC_FORM_AGGREGATE;
    const bool fb_one_lane = recip_like && (k.fb_one_lane_mode >= 0 ? k.fb_one_lane_mode == 1 : n >= 128 * S);
    const bool fb_wide = !part && (k.fb_wide_max >= 0 ? n <= (size_t)k.fb_wide_max : split_ok && n <= 8 * S);
    p.fb = fb_one_lane ? GENERIC_FB_ONE_LANE : fb_wide ? GENERIC_FB_WAVEFRONT : GENERIC_FB_LANES8;
    if (recip_like) {
        // (C0's sum: lane groups of 2 or 4; the aggregate verifier's 4 + k points go five per pass on one lane)
        p.c0var_group = protocol == GENERIC_FORM_AGGREGATE ? 1 : p.round_group > 4 ? 4 : p.round_group;
        if (protocol == GENERIC_FORM_AGGREGATE) p.c0_chunks = (int)((c0_points + 4) / 5);
        // What needs nothing but the proof bytes -- the round points' window tables -- and what needs only phase 1 -- the C0 points' tables
        // and C0's variable-base sum, one lane (or a lane group) per instance -- runs on the HELPER stream beside phase 1 and the fixed-base
        // half of C0 (8 lanes per instance: the kernel that fills the chip); round 6: 2^15 instances of configs[4]'s shape, where the
        // one-lane kernels are half a wavefront per SIMD, 46.6 -> 45.0 ms per batch.  With kernel timing on everything stays on one stream
        // so that the per-kernel times add up; the parts of a multi-part call are chains of their own.
        // (only while the one-lane kernels are at most half a wavefront per SIMD: beyond that the kernels fill the chip by themselves and
        // side by side they take LONGER than one after the other, as in the u64 verifier -- 2^16 instances 79.6 ms on two streams against
        // 79.2 on one, 2^17 154.2 / 153.0, 2^18 314.3 / 301.4: profiles/r06/r06_b1_recip_beside_sizes.txt)
        p.beside = p.fast && !k.timing && !part && (k.recip_beside >= 0 ? k.recip_beside == 1 : 2 * blocks <= S);
        // lanes per instance for phase 1's two loops over the digits: as many (up to 8) as keep the launch within ONE wavefront per SIMD --
        // the kernel is an uncapped build (one wavefront per SIMD fits), and a group's lanes each repeat the head (transcript, inversions:
        // a seventh of the one-lane kernel).  Round 6, configs[4]'s shape, the kernel alone: 2^15 instances 3.48 -> 2.10 ms on 2 lanes
        // (2.65 on 4, 3.8 on 8: two and four generations of wavefronts); the call 45.71 -> 45.30 ms, because the round-point tables
        // that ran beside the half-empty one-lane kernel now share its SIMDs (profiles/r06/r06_p2_recip_phase1_groups.txt)
        int G = 1;
        if (k.recip_p1_group) G = k.recip_p1_group;
        else if (groups && k.lane_group) G = k.lane_group == 2 ? 2 : 8;      // (tests: the smallest and the largest split at any size)
        else if (groups) while (G < 8 && 2 * (size_t)G * blocks <= S) G *= 2;
        p.p1_group = G;
    }
    if (protocol == GENERIC_FORM_CIRCUIT) {
        // C0's variable-base sum: a lane per point (c0_lanes per instance, tables and sum in one launch) while that stays within two
        // wavefronts per SIMD, else the one-lane kernels (five points per shared-doubling pass).  Round 6, `mixed_k2` (6 points): one
        // verify 4.74 -> 2.76 ms (this stage 3.0 -> 0.98), 8,192 instances 1.37 ms where 16,384 on the one-lane kernels take 2.64
        int L = 8;
        while ((size_t)L < c0_points && L < (1 << 30)) L *= 2;
        p.c0_lanes = L;
        p.per_point = p.fast && split_ok && L <= 64 && (size_t)L * ((n + PLAN_BLOCK - 1) / PLAN_BLOCK) <= 2 * S;
    }
    return p;
}

}  // namespace bppp_host
