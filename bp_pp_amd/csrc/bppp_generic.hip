// libbppp_hip.so, host side: generic WeightNormLinearArgument / ReciprocalRangeProofProtocol / ArithmeticCircuit verifiers and provers, and the
// generic fixed-base linear combination (the crate's commit functions).
#include "host.h"

// the launch choices of the three verifiers: one pure function of (protocol, instances, rounds, switches) in plan_core.h
using bppp_host::GenericPlan;
using bppp_host::plan_generic;
using bppp_host::GENERIC_FORM_WNLA; using bppp_host::GENERIC_FORM_RECIPROCAL; using bppp_host::GENERIC_FORM_CIRCUIT;
using bppp_host::GENERIC_FORM_AGGREGATE;
using bppp_host::GENERIC_FB_WAVEFRONT; using bppp_host::GENERIC_FB_ONE_LANE;

// one launch (or a short run of launches) on stream `st`, timed under KernelId `id` when kernel timing is on; a failure leaves the
// calling function with its code (an `int rc` and the context `c` are in scope wherever this is used)
#define GLAUNCH(st, id, ...)                                   \
    do {                                                       \
        rc = timed(c, id, st, [&]() { __VA_ARGS__; });         \
        if (rc != BPPP_OK) return rc;                          \
    } while (0)
static unsigned blocks_of(size_t n) { return (unsigned)((n + BPPP_BLOCK - 1) / BPPP_BLOCK); }
static unsigned fb_blocks_of(size_t n) { return (unsigned)((n * BPPP_FB_LANES + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }
static size_t take_bytes(size_t& off, size_t bytes) { const size_t o = off; off = align16(off + bytes); return o; }

// The WnlaWs of a WNLA stage that CONTINUES an outer protocol (r: the reciprocal verifier's RecipWs, 5 points per proof, or the circuit
// verifier's CircuitWs, 4): every instance's transcript goes on where the outer stage left it in r.tstate, the commitment and c, rho,
// mu are what the outer stage wrote to r.wn_*, and the proof fields are read in place out of the outer proof blob --
// 4 points | r | x | the points beyond 4 | l | n.  accept, ys, tab, msc: the stage's own buffers.
template <typename OuterWs>
static WnlaWs wnla_ws_continuing(const bppp_ctx* c, const OuterWs& r, size_t points, size_t nl, size_t nn, uint8_t* accept, u32* ys, u32* tab,
                                 u32* msc) {
    const size_t rounds = (size_t)r.rounds;
    WnlaWs w;
    std::memset(&w, 0, sizeof w);
    w.N = r.N; w.ng = c->ng; w.nh = c->nh; w.rounds = r.rounds; w.nl = (int)nl; w.nn = (int)nn;
    w.base = r.base; w.tio = r.tio; w.divergent_positions = r.tio.states && r.tio.n_states != 1;
    w.commitments = r.wn_commit; w.c = r.wn_c; w.rho = r.wn_rho; w.mu = r.wn_mu;
    w.proof_r = r.proofs + 256; w.proof_x = r.proofs + 256 + 64 * rounds; w.proof_l = r.proofs + 64 * points + 128 * rounds;
    w.proof_n = w.proof_l + 32 * nl;
    w.stride_r = w.stride_x = w.stride_l = w.stride_n = r.proof_bytes;
    w.transcript_preloaded = 1;
    w.accept = accept; w.status = r.status; w.tstate = r.tstate; w.acc = r.acc; w.pfix = r.pfix;
    w.ys = ys; w.tab = tab; w.msc = msc;
    w.straus = r.straus;
    w.fb = r.fb;
    return w;
}

extern "C" {

// caller transcripts of the generic verifiers (host pointers): n_states x 203 in, n x 203 out (optional)
struct HostTranscripts { const uint8_t* states; size_t n_states; uint8_t* states_out; };
static int check_host_transcripts(const HostTranscripts* tx, size_t n) {
    if (!tx) return BPPP_OK;
    if (!tx->states || (tx->n_states != 1 && tx->n_states != n)) return BPPP_ERR_INVALID_ARG;
    for (size_t i = 0; i < tx->n_states; i++)
        if (tx->states[203 * i + 200] >= BPPP_STROBE_R || tx->states[203 * i + 201] > BPPP_STROBE_R) return BPPP_ERR_INVALID_ARG;
    return BPPP_OK;
}
// device copies of a prover call's transcripts (host-buffer entry points): states in, advanced states out
struct TxDev {
    uint8_t *d_in = nullptr, *d_out = nullptr;      // carved out of the context's grow-only transcript staging
    int begin(bppp_ctx* c, const HostTranscripts* tx, size_t n, hipStream_t s, TranscriptIo& io, int& divergent) {
        io.states = nullptr; io.n_states = 0; io.states_out = nullptr; io.no_ops = 0;
        divergent = 0;
        if (!tx) return BPPP_OK;
        int rc = check_host_transcripts(tx, n);
        if (rc != BPPP_OK) return rc;
        const size_t b_in = align16(tx->n_states * 203);
        rc = ensure_buffer(c, c->d_txio, c->txio_bytes, b_in + (tx->states_out ? n * 203 : 0));
        if (rc != BPPP_OK) return rc;
        d_in = c->d_txio;
        if (tx->states_out) d_out = c->d_txio + b_in;
        HIP_TRY(hipMemcpyAsync(d_in, tx->states, tx->n_states * 203, hipMemcpyHostToDevice, s));
        io.states = d_in; io.n_states = tx->n_states; io.states_out = d_out;
        divergent = tx->n_states != 1;
        return BPPP_OK;
    }
    // after the last prover kernel: serialize every instance's transcript and queue the copy back
    // flagged_back (the provers from integers): every instance whose proof is zeroed -- any status -- gets its input state back
    int finish(const HostTranscripts* tx, const TranscriptIo& io, const strobe& base, const u32* tstate, size_t n, const int32_t* status, hipStream_t s,
               bool flagged_back = false) {
        if (!tx || !tx->states_out) return BPPP_OK;
        if (flagged_back) k_aprove_export_states<<<(unsigned)((n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, s>>>(io, base, tstate, n, status);
        else k_gprove_export_states<<<(unsigned)((n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, s>>>(io, base, tstate, n, status);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(tx->states_out, d_out, n * 203, hipMemcpyDeviceToHost, s));
        return BPPP_OK;
    }
};
// fast variable-base path of the generic verifiers' rounds: per instance 2 x rounds window tables (16 entries of 64 B per point), the
// running products of their build (BPPP_TSCR_PER_POINT per point) and the decoded round points -- 1.2 KB + 0.55 KB + 64 B per point, grow-only
// extra_points: tables of that many more points per instance behind the round points' (the reciprocal verifier's five C0 points)
static size_t wnla_fast_bytes(size_t n, size_t rounds, size_t extra_points, size_t parts = 1) {
    const size_t np = 2 * rounds * parts + extra_points;
    return align16(np * 16 * sizeof(apt_packed) * n) + align16((size_t)BPPP_TSCR_PER_POINT * np * 10 * sizeof(u32) * n) + align16(np * 16 * sizeof(u32) * n);
}
// The buffers of that path for the WnlaWs of a call (or part) on plan p, none where the plan has no fast rounds.
// base: where this call's (or this part's) share of the table buffer starts; null = the context's buffer, grown to what the call needs
// The extra points' tables (the outer protocol's C0 points) follow the p.tab_parts sets of round-point tables, at entry wnla_atab_first
static int wnla_fast_setup(bppp_ctx* c, WnlaWs& w, const GenericPlan& p, size_t extra_points, uint8_t* base = nullptr) {
    const size_t n = w.N, rounds = (size_t)w.rounds, parts = (size_t)p.tab_parts;
    w.atab = nullptr; w.tscr = nullptr; w.rpts = nullptr; w.tab_parts = p.tab_parts;
    if (!p.fast) return BPPP_OK;
    const size_t np = 2 * rounds * parts + extra_points;
    const size_t b_tab = align16(np * 16 * sizeof(apt_packed) * n), b_scr = align16((size_t)BPPP_TSCR_PER_POINT * np * 10 * sizeof(u32) * n);
    if (!base) {
        const int rc_t = ensure_buffer(c, c->d_gtab, c->gtab_bytes, wnla_fast_bytes(n, rounds, extra_points, parts));
        if (rc_t != BPPP_OK) return rc_t;
        base = c->d_gtab;
    }
    w.atab = (apt_packed*)base;
    w.tscr = (u32*)(base + b_tab);
    w.rpts = (u32*)(base + b_tab + b_scr);
    return BPPP_OK;
}
static int wnla_atab_first(const GenericPlan& p, size_t rounds) { return (int)(2 * rounds * 16 * (size_t)p.tab_parts); }
static unsigned fb64_blocks_of(size_t n) { return (unsigned)((n * 64 + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }
static unsigned fb1_blocks_of(size_t n) { return (unsigned)((n + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }
// the round points' window tables: a lane per instance, or a lane per (point, part) table in a call that leaves the chip empty
static void launch_wnla_tables(const WnlaWs& w, int tab_parts, size_t n, unsigned blocks, hipStream_t s) {
    if (tab_parts > 1) {
        int lp = 2;
        while (lp < 2 * w.rounds) lp *= 2;
        k_wnla_tables_split<<<(unsigned)(((size_t)lp * tab_parts * n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, s>>>(w, tab_parts, lp);
    }
    else k_wnla_tables<<<blocks, BPPP_BLOCK, 0, s>>>(w);
}
// the final scalars on 2^lg lanes per instance (GenericPlan::final_lg)
static void launch_wnla_final_scalars(const WnlaWs& w, int lg, unsigned blocks, hipStream_t s) {
    if (lg > 0) {
        k_wnla_final_scalars_grp<<<blocks << lg, BPPP_BLOCK, 0, s>>>(w, lg);
        k_wnla_final_scalars_join<<<blocks, BPPP_BLOCK, 0, s>>>(w, lg);
    } else k_wnla_final_scalars<<<blocks, BPPP_BLOCK, 0, s>>>(w);
}
// the device forms' optional counter of rejected instances: zeroed in front of the call (it reads zero after a call of no instances
// too), counted behind its last verdict; null = the caller did not ask
static int reset_reject_count(bppp_ctx* c, void* d_reject_count) {
    if (d_reject_count) HIP_TRY(hipMemsetAsync(d_reject_count, 0, sizeof(int), c->stream));
    return BPPP_OK;
}
static int launch_count_rejects(bppp_ctx* c, const void* d_accept, size_t n, void* d_reject_count) {
    if (!d_reject_count) return BPPP_OK;
    k_count_rejects<<<(unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), 256, 0, c->stream>>>((const uint8_t*)d_accept, n, (int*)d_reject_count);
    HIP_TRY(hipGetLastError());
    return BPPP_OK;
}
// "last_rlc_*" of an RLC call start at (0, 0), before its first allocation: a call that fails reports nothing stale
static void rlc_report_reset(bppp_ctx* c, const uint8_t* rlc_seed) {
    if (rlc_seed) { c->last_rlc_super_m = 0; c->last_rlc_chunk = 0; }
}
// one part of a multi-part call (recip_verify_device_entry): its stream and its shares of the context's buffers
// (started / stage: an event recorded behind the part's stage-th milestone -- 1 phase 1, 2 the C0 stage, 3 the rounds -- that the NEXT
// part's chain waits for, so that the chains run out of step: one part's fixed-base sums under another's one-lane kernels)
struct GenericPart { hipStream_t s; uint8_t* gtab; pt_slot* straus; size_t call_n; hipEvent_t started; int stage; int n_parts; };
static int part_milestone(const GenericPart* part, int stage, hipStream_t s) {
    if (part && part->started && part->stage == stage) HIP_TRY(hipEventRecord(part->started, s));
    return BPPP_OK;
}
// the wire form of the generic proofs (the *_sec1 entry points at the end of this file): conversion launches over a WireMap (wire_core.h)
static int wire_launch(WireMap m, bool expand, hipStream_t s) {
    const u64 lanes = wire_map_finish(m);
    if (lanes == 0) return BPPP_OK;
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    if (expand) k_wire_expand<<<blocks, 256, 0, s>>>(m);
    else k_wire_compress<<<blocks, 256, 0, s>>>(m);
    HIP_TRY(hipGetLastError());
    return BPPP_OK;
}
// one contiguous proof of P points and S scalars per instance: 33 P + 32 S bytes <-> 64 P + 32 S bytes, field order unchanged
static void wire_add_proof(WireMap& m, const uint8_t* src33, uint8_t* dst64, size_t P, size_t S) {
    const size_t b33 = 33 * P + 32 * S, b64 = 64 * P + 32 * S;
    wire_map_add(m, false, src33, b33, dst64, b64, P);
    wire_map_add(m, true, src33 + 33 * P, b33, dst64 + 64 * P, b64, S);
}
static size_t wire_proof_bytes(size_t P, size_t S) { return 33 * P + 32 * S; }
// THE EXPANSION of a wire-form verify call, stated once per protocol: n instances of k commitments and a proof of P points and S scalars
// become the 64-byte commitments | the 64-byte proofs (at o_proofs) in the wire buffer -- what the 64-byte verifier then reads
struct WireExp {
    size_t n, k, P, S;
    size_t com33_bytes() const { return n * k * 33; }
    size_t proofs33_bytes() const { return n * wire_proof_bytes(P, S); }
    size_t o_proofs() const { return align16(n * k * 64); }
    size_t bytes() const { return o_proofs() + n * (64 * P + 32 * S); }
    int launch(const uint8_t* d_com33, const uint8_t* d_proofs33, uint8_t* d_exp, hipStream_t s) const {
        WireMap m;
        wire_map_init(m, n);
        wire_map_add(m, false, d_com33, 33 * k, d_exp, 64 * k, k);
        wire_add_proof(m, d_proofs33, d_exp + o_proofs(), P, S);
        return wire_launch(m, true, s);
    }
};
static WireExp recip_wire_exp(size_t n, size_t rounds, size_t nl, size_t nn) { return {n, 1, 5 + 2 * rounds, nl + nn}; }
static WireExp agg_wire_exp(size_t n, size_t k, size_t rounds, size_t nl, size_t nn) { return {n, k, 4 + 2 * rounds + k, nl + nn}; }
static WireExp circuit_wire_exp(size_t n, size_t k, size_t rounds, size_t nl, size_t nn) { return {n, k, 4 + 2 * rounds, nl + nn}; }
// the WNLA call's: the commitment | proof.r | proof.x (c, rho, mu, proof.l and proof.n are scalars, read where they are)
struct WnlaWireExp {
    size_t n, rounds;
    size_t o_r() const { return align16(n * 64); }
    size_t o_x() const { return o_r() + align16(n * rounds * 64); }
    size_t bytes() const { return o_x() + align16(n * rounds * 64); }
    int launch(const uint8_t* d_com33, const uint8_t* d_r33, const uint8_t* d_x33, uint8_t* d_exp, hipStream_t s) const {
        WireMap m;
        wire_map_init(m, n);
        wire_map_add(m, false, d_com33, 33, d_exp, 64, 1);
        if (rounds) {
            wire_map_add(m, false, d_r33, 33 * rounds, d_exp + o_r(), 64 * rounds, rounds);
            wire_map_add(m, false, d_x33, 33 * rounds, d_exp + o_x(), 64 * rounds, rounds);
        }
        return wire_launch(m, true, s);
    }
};
// a prover's input points (k per instance) from the caller's host memory to d_dst in the 64-byte form: copied as they are, or (sec1)
// staged as 33 bytes at the head of the wire buffer, grown to wire_bytes for what the call will put behind them, and expanded on the device
static int prover_points_in(bppp_ctx* c, bool sec1, const uint8_t* src, uint8_t* d_dst, size_t n, size_t k, size_t wire_bytes, hipStream_t s) {
    if (!sec1) { HIP_TRY(hipMemcpyAsync(d_dst, src, n * k * 64, hipMemcpyHostToDevice, s)); return BPPP_OK; }
    const int rc = ensure_buffer(c, c->d_wire, c->wire_bytes, wire_bytes);
    if (rc != BPPP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_wire, src, n * k * 33, hipMemcpyHostToDevice, s));
    WireMap wm;
    wire_map_init(wm, n);
    wire_map_add(wm, false, c->d_wire, 33 * k, d_dst, 64 * k, k);
    return wire_launch(wm, true, s);
}

// ---- generic WeightNormLinearArgument entry points (host pointers; one device blob per call)
// (the context's grow-only buffer: no allocator round trip per call.  Whatever way the call ends, nothing of it is still running
// when the blob goes out of scope -- on the success path the stream has just been waited for and this costs nothing)
struct WnlaBlob {
    bppp_ctx* c = nullptr;
    uint8_t* d = nullptr;
    int take(bppp_ctx* ctx, size_t bytes) {
        c = ctx;
        int rc = ensure_blob(ctx, bytes);
        d = ctx->d_blob;
        return rc;
    }
    ~WnlaBlob() { if (c) quiesce(c); }
};
// THE HOST STAGING of a verify call over host buffers, in the blob or (the wire forms) in the wire buffer:
//     the inputs as given | accept n | status n x 4 | the caller's states in | their states out | `tail` bytes (workspace or expansion)
// begin() grows the buffer and queues the copies up on the context's stream; finish() takes the code of what ran between the two and,
// unless that failed, queues the copies back -- states out, accept, status where the caller asked for it -- and waits for the stream,
// the call's one sync.  Whatever way the call ends, nothing of it is
// still running when the staging goes out of scope (it is reused by the next call); behind finish() that costs nothing.
struct HostIn { const void* src; size_t bytes; };       // (null or empty: room is made, nothing is copied)
struct HostStage {
    bppp_ctx* c = nullptr;
    static constexpr size_t MAX_IN = 8;
    uint8_t *in[MAX_IN], *accept = nullptr, *tail = nullptr;
    int32_t* status = nullptr;
    TranscriptIo tio = {nullptr, 0, nullptr, 0};
    const TranscriptIo* dtio = nullptr;                 // &tio, or null without caller transcripts
    // gws_bytes: what the call needs of the device forms' workspace besides, grown behind the staging and in front of the first copy
    int begin(bppp_ctx* ctx, bool wire, std::initializer_list<HostIn> ins, size_t n, const HostTranscripts* tx, size_t tail_bytes,
              size_t gws_bytes = 0) {
        size_t off = 0, o_in[MAX_IN], k = 0;
        if (ins.size() > MAX_IN) return BPPP_ERR_INVALID_ARG;
        for (const HostIn& i : ins) o_in[k++] = take_bytes(off, i.bytes);
        const size_t o_acc = take_bytes(off, n), o_st = take_bytes(off, n * 4), o_ti = take_bytes(off, tx ? tx->n_states * 203 : 0),
                     o_to = take_bytes(off, tx && tx->states_out ? n * 203 : 0);
        if (!wire) c = ctx;      // (a blob call quiesces even where the blob fails to grow, as it always did)
        int rc = wire ? ensure_buffer(ctx, ctx->d_wire, ctx->wire_bytes, off + tail_bytes) : ensure_blob(ctx, off + tail_bytes);
        if (rc == BPPP_OK && gws_bytes) rc = ensure_buffer(ctx, ctx->d_gws, ctx->gws_bytes, gws_bytes);
        if (rc != BPPP_OK) return rc;
        c = ctx;                 // (a wire call quiesces from here on, its buffers grown, as it always did)
        uint8_t* d = wire ? c->d_wire : c->d_blob;
        k = 0;
        for (const HostIn& i : ins) {
            in[k] = d + o_in[k];
            if (i.src && i.bytes) HIP_TRY(hipMemcpyAsync(in[k], i.src, i.bytes, hipMemcpyHostToDevice, c->stream));
            k++;
        }
        accept = d + o_acc; status = (int32_t*)(d + o_st); tail = d + off;
        if (tx) {
            HIP_TRY(hipMemcpyAsync(d + o_ti, tx->states, tx->n_states * 203, hipMemcpyHostToDevice, c->stream));
            tio.states = d + o_ti; tio.n_states = tx->n_states; tio.states_out = tx->states_out ? d + o_to : nullptr;
            dtio = &tio;
        }
        return BPPP_OK;
    }
    int finish(int rc_run, size_t n, uint8_t* h_accept, int32_t* h_status, const HostTranscripts* tx) {
        if (rc_run != BPPP_OK) return rc_run;
        if (tio.states_out) HIP_TRY(hipMemcpyAsync(tx->states_out, tio.states_out, n * 203, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_accept, accept, n, hipMemcpyDeviceToHost, c->stream));
        if (h_status) HIP_TRY(hipMemcpyAsync(h_status, status, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return BPPP_OK;
    }
    ~HostStage() { if (c) quiesce(c); }
};

// ---- the random-linear-combination mode of the final sum (wnla_rlc_core.h), shared by the three generic verifiers: every one of them
//      ends in the WNLA stage, and this is that stage's last step.
// Where the RLC buffers sit in a call's workspace: taken behind `off`, the running end of the caller's own layout, whichever it is
struct WnlaRlcLayout { size_t lhs, sc, flag, list; };
static WnlaRlcLayout wnla_rlc_take(size_t& off, size_t n, size_t NB) {
    const size_t nchunks = (n + BPPP_RLC_CHUNK - 1) / BPPP_RLC_CHUNK;
    auto take = [&](size_t bytes) { size_t o = off; off = align16(off + bytes); return o; };
    WnlaRlcLayout o;
    o.lhs = take(30 * n * 4); o.sc = take(NB * 8 * n * 4); o.flag = take(nchunks); o.list = take((nchunks + 4) * 4);
    return o;
}
// RULE for the WNLA and circuit RLC entry points: a call with fewer than one complete chunk (n < 8) runs the exact final sum -- every
// instance of it would be re-checked by the exact kernels anyway (wnla_rlc_chunk_serial: an incomplete chunk is not usable), so the
// results are the same by construction and the chunk stage's six launches are saved; such a call reports "last_rlc_superchunk" =
// "last_rlc_chunk" = 0.  Every other call runs the chunk stage, at any launch form (per-part tables, lane-group rounds and the wide
// fixed-base sums of the stages before it are untouched; the flagged chunks' exact sums are a wavefront per instance themselves).
static bool wnla_rlc_applies(size_t n) { return n >= BPPP_RLC_CHUNK; }
// what such a call allocates besides its workspace, before its first launch: the bucket stage's buffers (launch_bucket_stage asks again)
static int wnla_rlc_prepare(bppp_ctx* c, size_t n) {
    return bucket_superchunk_for(c, n) ? ensure_bucket_capacity(c, n, (size_t)c->nbases) : BPPP_OK;
}
// The launches behind k_wnla_final_scalars in RLC mode: one MSM per chunk of 8 instances instead of one per instance; what does not
// pass is re-checked exactly (wnla_rlc_core.h).  d + o.*: the RLC buffers of this call; w.accept is written for every instance.
static int wnla_rlc_final_sum(bppp_ctx* c, const WnlaWs& w, const uint8_t* rlc_seed, uint8_t* d, const WnlaRlcLayout& o, hipStream_t s) {
    const size_t n = w.N, nchunks = (n + BPPP_RLC_CHUNK - 1) / BPPP_RLC_CHUNK;
    const int NB = c->nbases;
    const unsigned blocks = blocks_of(n), fb_blocks = fb_blocks_of(n);
    int rc;
    RlcWs rl;
    std::memset(&rl, 0, sizeof rl);
    for (int i = 0; i < 4; i++) {
        u64 v = 0;
        for (int k = 0; k < 8; k++) v |= (u64)rlc_seed[8 * i + k] << (8 * k);
        rl.seed[i] = v;
    }
    rl.lhs = (u32*)(d + o.lhs); rl.sc = (u32*)(d + o.sc); rl.flag = d + o.flag;
    rl.list = (u32*)(d + o.list); rl.count = (int*)(rl.list + nchunks + 1);
    const unsigned chunk_blocks = (unsigned)((nchunks * BPPP_RLC_CHUNK + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK);
    const unsigned check_blocks = (unsigned)(nchunks < 16384 ? nchunks : 16384);
    HIP_TRY(hipMemsetAsync(w.accept, 0, n, s));
    HIP_TRY(hipMemsetAsync(rl.count, 0, sizeof(int), s));
    const unsigned SM = bucket_superchunk_for(c, n);
    c->last_rlc_super_m = SM; c->last_rlc_chunk = BPPP_RLC_CHUNK;
    if (SM) {
        // bucket (Pippenger) stage first, as in the u64 verifier: superchunks of SM instances, the weighted commitments summed by
        // bucket accumulation and ONE 1 + ng + nh-base MSM per superchunk; the chunk-of-8 kernels only see what failed it
        BucketWs bw;
        rc = launch_bucket_stage(c, bw, n, SM, rl.seed, w.status, w.acc, w.msc, NB, w.accept, s,
                                 [&](int id, auto&& f) { return timed(c, id, s, f); });
        if (rc != BPPP_OK) return rc;
        rl.sflag = bw.sflag;
        rl.super_m = SM;
    }
    GLAUNCH(s, K_WNLA_RLC_LHS, k_wnla_rlc_lhs<<<blocks, BPPP_BLOCK, 0, s>>>(w, rl));
    GLAUNCH(s, K_WNLA_RLC_CHUNK, k_wnla_rlc_chunk<<<chunk_blocks, BPPP_FB_BLOCK, 0, s>>>(w, rl));
    GLAUNCH(s, K_WNLA_RLC_CHECK, k_wnla_rlc_check<<<check_blocks, 64, 0, s>>>(w, rl));
    GLAUNCH(s, K_WNLA_MSM, k_wnla_msm_flagged<<<1024, 64, 0, s>>>(w, rl));
    GLAUNCH(s, K_WNLA_MSM, k_wnla_msm_flagged_dense<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(w, rl));
    GLAUNCH(s, K_WNLA_ACCEPT, k_wnla_accept_flagged<<<blocks, BPPP_BLOCK, 0, s>>>(w, rl));
    return BPPP_OK;
}
// what the WNLA and circuit verifiers do in front of their workspace: whether the call's final sum runs in RLC mode (the rule above),
// "last_rlc_*" reset before the first allocation (a call that fails reports nothing stale), the projective tables, the bucket stage
static int wnla_call_prepare(bppp_ctx* c, size_t n, const uint8_t* rlc_seed, bool& rlc) {
    rlc = rlc_seed && wnla_rlc_applies(n);
    rlc_report_reset(c, rlc_seed);
    const int rc = ensure_straus_capacity(c, n);
    if (rc != BPPP_OK) return rc;
    return rlc ? wnla_rlc_prepare(c, n) : BPPP_OK;
}

// THE WNLA VERIFY STAGE, the tail of all three generic verifiers: on stream s over a prepared WnlaWs, in the form of the call's plan --
// the transcript's start, the round points' tables, the rounds, the final scalars, the final sum and the verdicts, the transcripts out.
// tables_done: the caller has launched the tables already (the reciprocal verifier, on its helper stream beside phase 1)
// rlc_seed: the final sum in RLC mode over the buffers d + o_rlc (wnla_rlc_final_sum); null = every instance's own sum
// part: the part of a multi-part call this is (its stage-3 milestone lies behind the rounds); null = the whole call
static int wnla_verify_stage(bppp_ctx* c, const WnlaWs& w, const GenericPlan& plan, hipStream_t s, bool tables_done = false,
                             const uint8_t* rlc_seed = nullptr, uint8_t* d = nullptr, const WnlaRlcLayout& o_rlc = {0, 0, 0, 0},
                             const GenericPart* part = nullptr) {
    const size_t n = w.N;
    const unsigned blocks = blocks_of(n);
    const int grp = plan.round_group;
    int rc;
    GLAUNCH(s, K_WNLA_BEGIN, k_wnla_begin<<<blocks, BPPP_BLOCK, 0, s>>>(w));
    if (plan.fast && !tables_done) GLAUNCH(s, K_WNLA_TABLES, launch_wnla_tables(w, plan.tab_parts, n, blocks, s));
    for (int k = 1; k <= w.rounds; k++) {
        if (grp > 1) GLAUNCH(s, K_WNLA_ROUND, k_wnla_round_grp<<<(unsigned)(((size_t)grp * n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, s>>>(w, k, grp));
        else GLAUNCH(s, K_WNLA_ROUND, k_wnla_round<<<blocks, BPPP_BLOCK, 0, s>>>(w, k));
    }
    rc = part_milestone(part, 3, s);
    if (rc != BPPP_OK) return rc;
    GLAUNCH(s, K_WNLA_FINAL_SCALARS, launch_wnla_final_scalars(w, plan.final_lg, blocks, s));
    if (rlc_seed) {
        rc = wnla_rlc_final_sum(c, w, rlc_seed, d, o_rlc, s);
        if (rc != BPPP_OK) return rc;
    } else {
        if (plan.fb == GENERIC_FB_ONE_LANE) GLAUNCH(s, K_WNLA_MSM, k_wnla_msm_l1<<<fb1_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(w));
        else if (plan.fb == GENERIC_FB_WAVEFRONT) GLAUNCH(s, K_WNLA_MSM, k_wnla_msm_l64<<<fb64_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(w));
        else GLAUNCH(s, K_WNLA_MSM, k_wnla_msm<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(w, 0));
        GLAUNCH(s, K_WNLA_ACCEPT, k_wnla_accept<<<blocks, BPPP_BLOCK, 0, s>>>(w));
    }
    if (w.tio.states_out) k_generic_export_states<<<blocks, BPPP_BLOCK, 0, s>>>(w);
    HIP_TRY(hipGetLastError());
    return BPPP_OK;
}

// what every WNLA verify entry point checks of its pointers (label: null with length 0 in the transcript form), and the sizes wnla_run
// takes -- checked by wnla_run itself, and by the wire-form entry points before they size their staging by them
static int wnla_verify_check(const bppp_ctx* c, const uint8_t* label, size_t label_len, const void* commitments, const void* cvec, const void* rho,
                             const void* mu, size_t rounds, const void* proof_r, const void* proof_x, const void* proof_l, size_t nl,
                             const void* proof_n, size_t nn, const void* accept) {
    if (!c || !label_ok(label, label_len) || !commitments || !cvec || !rho || !mu || (rounds && (!proof_r || !proof_x)) || (!proof_l && nl) ||
        (!proof_n && nn) || !accept)
        return BPPP_ERR_INVALID_ARG;
    return BPPP_OK;
}
static bool wnla_shape_ok(size_t rounds, size_t nl, size_t nn) { return rounds <= 12 && nl <= 4096 && nn <= 4096; }

static int wnla_run(bppp_ctx* c, bool commit, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments,
                    const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, size_t rounds, const uint8_t* proof_r,
                    const uint8_t* proof_x, const uint8_t* proof_l, size_t nl, const uint8_t* proof_n, size_t nn, uint8_t* out_points,
                    uint8_t* accept, int32_t* status, const HostTranscripts* tx = nullptr, bool device_io = false,
                    const uint8_t* rlc_seed = nullptr) {
    // device_io (bppp_wnla_verify_batch_device): every pointer above is DEVICE memory, read and written in place; the call is asynchronous
    // on the context's stream and only the workspace comes out of the context's buffer
    // rlc_seed (bppp_wnla_verify_batch_rlc[_device]): the final sum in RLC mode (wnla_rlc_final_sum, and the rule above it)
    HIP_TRY(hipSetDevice(c->device));
    if (!wnla_shape_ok(rounds, nl, nn)) return BPPP_ERR_INVALID_ARG;
    const GenericPlan plan = plan_generic(GENERIC_FORM_WNLA, n, rounds, generic_knobs_of(c), n, 1, 0);      // (of a verify call)
    int rc = check_host_transcripts(tx, n);
    if (rc != BPPP_OK) return rc;
    bool rlc;
    rc = wnla_call_prepare(c, n, rlc_seed, rlc);
    if (rc != BPPP_OK) return rc;
    const size_t NB = (size_t)c->nbases, T = (size_t)1 << rounds;
    // layout of the blob: inputs | outputs | workspace
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes); };
    const size_t o_com = take(n * 64), o_c = take(n * (size_t)c->nh * 32), o_rho = take(n * 32), o_mu = take(n * 32),
                 o_r = take(n * rounds * 64), o_x = take(n * rounds * 64), o_l = take(n * nl * 32), o_n = take(n * nn * 32),
                 o_out = take(n * 64), o_acc = take(n), o_st = take(n * 4), o_ts = take(52 * n * 4), o_a = take(30 * n * 4),
                 o_pf = take(30 * n * 4), o_ys = take((rounds ? rounds : 1) * 8 * n * 4), o_tab = take(2 * T * 8 * n * 4),
                 o_msc = take(NB * 8 * n * 4), o_ti = take(tx ? tx->n_states * 203 : 0), o_to = take(tx && tx->states_out ? n * 203 : 0);
    WnlaRlcLayout o_rlc = {0, 0, 0, 0};
    if (rlc) o_rlc = wnla_rlc_take(off, n, NB);
    WnlaBlob blob;
    if (device_io) { const int rc_b = ensure_blob(c, off + 16); if (rc_b != BPPP_OK) return rc_b; }       // (no sync when the call returns)
    else { const int rc_b = blob.take(c, off + 16); if (rc_b != BPPP_OK) return rc_b; }
    uint8_t* d = c->d_blob;
    hipStream_t s = c->stream;
    auto up = [&](size_t o, const uint8_t* src, size_t bytes) -> hipError_t {
        return (src && bytes && !device_io) ? hipMemcpyAsync(d + o, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    if (tx) HIP_TRY(up(o_ti, tx->states, tx->n_states * 203));
    HIP_TRY(up(o_com, commitments, n * 64));
    HIP_TRY(up(o_c, cvec, n * (size_t)c->nh * 32));
    HIP_TRY(up(o_rho, rho, n * 32));
    HIP_TRY(up(o_mu, mu, n * 32));
    HIP_TRY(up(o_r, proof_r, n * rounds * 64));
    HIP_TRY(up(o_x, proof_x, n * rounds * 64));
    HIP_TRY(up(o_l, proof_l, n * nl * 32));
    HIP_TRY(up(o_n, proof_n, n * nn * 32));
    auto in = [&](size_t o, const uint8_t* p) -> const uint8_t* { return device_io ? p : d + o; };
    WnlaWs w;
    std::memset(&w, 0, sizeof w);
    w.N = n; w.ng = c->ng; w.nh = c->nh; w.rounds = (int)rounds; w.nl = (int)nl; w.nn = (int)nn;
    w.commitments = in(o_com, commitments); w.c = in(o_c, cvec); w.rho = in(o_rho, rho); w.mu = in(o_mu, mu); w.proof_r = in(o_r, proof_r); w.proof_x = in(o_x, proof_x);
    w.proof_l = in(o_l, proof_l); w.proof_n = in(o_n, proof_n); w.out_points = d + o_out;
    w.accept = device_io ? accept : d + o_acc; w.status = (device_io && status) ? status : (int32_t*)(d + o_st);
    w.tstate = (u32*)(d + o_ts); w.acc = (u32*)(d + o_a); w.pfix = (u32*)(d + o_pf); w.ys = (u32*)(d + o_ys);
    w.tab = (u32*)(d + o_tab); w.msc = (u32*)(d + o_msc);
    w.stride_r = rounds * 64; w.stride_x = rounds * 64; w.stride_l = nl * 32; w.stride_n = nn * 32;
    w.straus = c->d_straus;
    w.fb = fb_table_of(c, n);
    if (!commit) t_new(w.base, label, (u32)label_len);
    if (tx) {
        w.tio.states = d + o_ti; w.tio.n_states = tx->n_states; w.tio.states_out = tx->states_out ? d + o_to : nullptr;
        w.tio.no_ops = rounds == 0;
        w.divergent_positions = tx->n_states != 1;
    }
    const unsigned blocks = blocks_of(n);
    if (commit) {
        k_wnla_commit_scalars<<<blocks, BPPP_BLOCK, 0, s>>>(w);
        k_wnla_msm<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(w, 1);
        k_wnla_commit_store<<<blocks, BPPP_BLOCK, 0, s>>>(w);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_points, d + o_out, n * 64, hipMemcpyDeviceToHost, s));
    } else {
        rc = wnla_fast_setup(c, w, plan, 0);
        if (rc != BPPP_OK) return rc;
        c->last_generic_form = plan.code();
        rc = wnla_verify_stage(c, w, plan, s, false, rlc ? rlc_seed : nullptr, d, o_rlc);
        if (rc != BPPP_OK) return rc;
        if (device_io) return BPPP_OK;
        HIP_TRY(hipMemcpyAsync(accept, d + o_acc, n, hipMemcpyDeviceToHost, s));
        if (w.tio.states_out) HIP_TRY(hipMemcpyAsync(tx->states_out, d + o_to, n * 203, hipMemcpyDeviceToHost, s));
    }
    if (status) HIP_TRY(hipMemcpyAsync(status, d + o_st, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BPPP_OK;
}

int bppp_wnla_commit_batch(bppp_ctx* c, size_t n, const uint8_t* cvec, const uint8_t* mu, const uint8_t* l, size_t nl,
                           const uint8_t* nvec, size_t nn, uint8_t* out, int32_t* status) {
    CtxLock lock_(c);
    if (!c || !cvec || !mu || (!l && nl) || (!nvec && nn) || !out) return BPPP_ERR_INVALID_ARG;
    if (n == 0) return BPPP_OK;
    return wnla_run(c, true, nullptr, 0, n, nullptr, cvec, nullptr, mu, 0, nullptr, nullptr, l, nl, nvec, nn, out, nullptr, status);
}

int bppp_wnla_verify_batch(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments,
                           const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, size_t rounds, const uint8_t* proof_r,
                           const uint8_t* proof_x, const uint8_t* proof_l, size_t nl, const uint8_t* proof_n, size_t nn,
                           uint8_t* accept, int32_t* status) {
    CtxLock lock_(c);
    const int rc = wnla_verify_check(c, label, label_len, commitments, cvec, rho, mu, rounds, proof_r, proof_x, proof_l, nl, proof_n, nn, accept);
    if (rc != BPPP_OK || n == 0) return rc;
    return wnla_run(c, false, label, label_len, n, commitments, cvec, rho, mu, rounds, proof_r, proof_x, proof_l, nl, proof_n, nn, nullptr,
                    accept, status);
}

int bppp_wnla_verify_batch_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const void* d_commitments, const void* d_c,
                                  const void* d_rho, const void* d_mu, size_t rounds, const void* d_proof_r, const void* d_proof_x,
                                  const void* d_proof_l, size_t nl, const void* d_proof_n, size_t nn, void* d_accept, void* d_status) {
    CtxLock lock_(c);
    const int rc = wnla_verify_check(c, label, label_len, d_commitments, d_c, d_rho, d_mu, rounds, d_proof_r, d_proof_x, d_proof_l, nl, d_proof_n, nn,
                                     d_accept);
    if (rc != BPPP_OK || n == 0) return rc;
    return wnla_run(c, false, label, label_len, n, (const uint8_t*)d_commitments, (const uint8_t*)d_c, (const uint8_t*)d_rho, (const uint8_t*)d_mu, rounds,
                    (const uint8_t*)d_proof_r, (const uint8_t*)d_proof_x, (const uint8_t*)d_proof_l, nl, (const uint8_t*)d_proof_n, nn, nullptr,
                    (uint8_t*)d_accept, (int32_t*)d_status, nullptr, true);
}

// the same two in RLC mode: the exact twins' argument checks, and a seed
int bppp_wnla_verify_batch_rlc(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments,
                               const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, size_t rounds, const uint8_t* proof_r,
                               const uint8_t* proof_x, const uint8_t* proof_l, size_t nl, const uint8_t* proof_n, size_t nn,
                               uint8_t* accept, int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    const int rc = wnla_verify_check(c, label, label_len, commitments, cvec, rho, mu, rounds, proof_r, proof_x, proof_l, nl, proof_n, nn, accept);
    if (rc != BPPP_OK || n == 0) return rc;
    return wnla_run(c, false, label, label_len, n, commitments, cvec, rho, mu, rounds, proof_r, proof_x, proof_l, nl, proof_n, nn, nullptr,
                    accept, status, nullptr, false, seed);
}
int bppp_wnla_verify_batch_rlc_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const void* d_commitments, const void* d_c,
                                      const void* d_rho, const void* d_mu, size_t rounds, const void* d_proof_r, const void* d_proof_x,
                                      const void* d_proof_l, size_t nl, const void* d_proof_n, size_t nn, void* d_accept, void* d_status,
                                      const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    const int rc = wnla_verify_check(c, label, label_len, d_commitments, d_c, d_rho, d_mu, rounds, d_proof_r, d_proof_x, d_proof_l, nl, d_proof_n, nn,
                                     d_accept);
    if (rc != BPPP_OK || n == 0) return rc;
    return wnla_run(c, false, label, label_len, n, (const uint8_t*)d_commitments, (const uint8_t*)d_c, (const uint8_t*)d_rho, (const uint8_t*)d_mu, rounds,
                    (const uint8_t*)d_proof_r, (const uint8_t*)d_proof_x, (const uint8_t*)d_proof_l, nl, (const uint8_t*)d_proof_n, nn, nullptr,
                    (uint8_t*)d_accept, (int32_t*)d_status, nullptr, true, seed);
}

int bppp_wnla_verify_batch_transcript(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, const uint8_t* commitments,
                                      const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, size_t rounds, const uint8_t* proof_r,
                                      const uint8_t* proof_x, const uint8_t* proof_l, size_t nl, const uint8_t* proof_n, size_t nn,
                                      uint8_t* accept, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    const int rc = wnla_verify_check(c, nullptr, 0, commitments, cvec, rho, mu, rounds, proof_r, proof_x, proof_l, nl, proof_n, nn, accept);
    if (rc != BPPP_OK || n == 0) return rc;
    HostTranscripts tx = {states, n_states, states_out};
    return wnla_run(c, false, nullptr, 0, n, commitments, cvec, rho, mu, rounds, proof_r, proof_x, proof_l, nl, proof_n, nn, nullptr, accept,
                    status, &tx);
}

// ---- generic ReciprocalRangeProofProtocol::verify (reciprocal.rs:98-107) on a context built by bppp_wnla_ctx_create over
//      g, g_vec || g_vec_, h_vec || h_vec_
// workspace (beyond the caller's commitments / proofs / accept / status) of one reciprocal verify call: where each buffer sits, and the total
struct RecipVerifyLayout { size_t ts, sc0, pts, a, pf, inv, wc, wcv, rho, mu, ys, tab, msc; WnlaRlcLayout rlc; size_t total; };
static RecipVerifyLayout recip_verify_layout(const bppp_ctx* c, size_t n, size_t dim_nd, size_t dim_np, size_t rounds, bool rlc) {
    const size_t NB = (size_t)c->nbases, T = (size_t)1 << rounds, NH = (size_t)c->nh;
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes); };
    RecipVerifyLayout o;
    o.ts = take(52 * n * 4); o.sc0 = take((dim_nd + 6) * 8 * n * 4); o.pts = take(5 * 16 * n * 4); o.a = take(30 * n * 4);
    o.pf = take(30 * n * 4); o.inv = take(dim_np * 8 * n * 4); o.wc = take(n * 64); o.wcv = take(n * NH * 32); o.rho = take(n * 32);
    o.mu = take(n * 32); o.ys = take((rounds ? rounds : 1) * 8 * n * 4); o.tab = take(2 * T * 8 * n * 4); o.msc = take(NB * 8 * n * 4);
    o.rlc = {0, 0, 0, 0};
    if (rlc) o.rlc = wnla_rlc_take(off, n, NB);
    o.total = off;
    return o;
}
static size_t recip_verify_ws_bytes(const bppp_ctx* c, size_t n, size_t dim_nd, size_t dim_np, size_t rounds, bool rlc = false) {
    return recip_verify_layout(c, n, dim_nd, dim_np, rounds, rlc).total;
}
// the launch sequence, every buffer in device memory; d_ws holds recip_verify_ws_bytes()
static int recip_verify_device_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                    const uint8_t* d_com, const uint8_t* d_proofs, size_t rounds, size_t nl, size_t nn, uint8_t* d_acc,
                                    int32_t* d_st, uint8_t* d_ws, const TranscriptIo* dtio = nullptr, const uint8_t* rlc_seed = nullptr,
                                    const GenericPart* part = nullptr) {
    // which kernels the call (or part) runs, on how many lanes per instance and on which stream: plan_core.h
    const GenericPlan plan = plan_generic(GENERIC_FORM_RECIPROCAL, n, rounds, generic_knobs_of(c), part ? part->call_n : n, part ? part->n_parts : 1, 0);
    const RecipVerifyLayout o = recip_verify_layout(c, n, dim_nd, dim_np, rounds, rlc_seed != nullptr);
    uint8_t* d = d_ws;
    hipStream_t s = part ? part->s : c->stream;
    RecipWs r;
    std::memset(&r, 0, sizeof r);
    r.N = n; r.nd = (int)dim_nd; r.np = (int)dim_np; r.rounds = (int)rounds; r.nl = (int)nl; r.nn = (int)nn;
    r.NG = c->ng; r.NH = c->nh; r.proof_bytes = 64 * (5 + 2 * rounds) + 32 * (nl + nn);
    r.commitments = d_com; r.proofs = d_proofs; r.status = d_st; r.tstate = (u32*)(d + o.ts);
    r.sc0 = (u32*)(d + o.sc0); r.pts = (u32*)(d + o.pts); r.acc = (u32*)(d + o.a); r.pfix = (u32*)(d + o.pf); r.inv = (u32*)(d + o.inv);
    r.straus = part ? part->straus : c->d_straus;
    r.wn_commit = d + o.wc; r.wn_c = d + o.wcv; r.wn_rho = d + o.rho; r.wn_mu = d + o.mu;
    r.fb = fb_table_of(c, n);
    t_new(r.base, label, (u32)label_len);
    if (dtio) r.tio = *dtio;
    WnlaWs w = wnla_ws_continuing(c, r, 5, nl, nn, d_acc, (u32*)(d + o.ys), (u32*)(d + o.tab), (u32*)(d + o.msc));
    const unsigned blocks = blocks_of(n);
    int rc;
    // the WNLA stage's table buffer with room for the five C0 points' tables behind the round points': the variable-base part of C0 on
    // affine window tables too (and on lane groups while one lane per instance leaves wavefront slots free)
    rc = wnla_fast_setup(c, w, plan, 5, part ? part->gtab : nullptr);
    if (rc != BPPP_OK) return rc;
    r.atab = w.atab; r.tscr = w.tscr; r.atab_first = wnla_atab_first(plan, rounds);
    const bool beside = plan.beside;      // the round points' tables, the C0 points' tables and C0's variable-base sum on the helper stream
    hipStream_t a = beside ? c->aux_stream : s;
    const int G = plan.p1_group;
    c->last_generic_form = plan.code();
    if (beside) {
        HIP_TRY(hipEventRecord(c->ev_tab, s));               // (the call's inputs are ready on s)
        HIP_TRY(hipStreamWaitEvent(a, c->ev_tab, 0));
        GLAUNCH(a, K_WNLA_TABLES, launch_wnla_tables(w, plan.tab_parts, n, blocks, a));
    }
    if (G > 1) GLAUNCH(s, K_RECIP_PHASE1, k_recip_phase1_grp<<<(unsigned)(((size_t)G * n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, s>>>(r, G));
    else GLAUNCH(s, K_RECIP_PHASE1, k_recip_phase1<<<blocks, BPPP_BLOCK, 0, s>>>(r));
    rc = part_milestone(part, 1, s);
    if (rc != BPPP_OK) return rc;
    if (beside) {
        HIP_TRY(hipEventRecord(c->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(a, c->ev_fork, 0));
    }
    if (plan.fb == GENERIC_FB_ONE_LANE) GLAUNCH(s, K_RECIP_C0_FIXED, k_recip_c0_fixed_l1<<<fb1_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    else if (plan.fb == GENERIC_FB_WAVEFRONT) GLAUNCH(s, K_RECIP_C0_FIXED, k_recip_c0_fixed_l64<<<fb64_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    else GLAUNCH(s, K_RECIP_C0_FIXED, k_recip_c0_fixed<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    if (plan.fast) {
        const int grp = plan.c0var_group;
        GLAUNCH(a, K_RECIP_C0_VAR, {
            k_recip_c0_tables<<<blocks, BPPP_BLOCK, 0, a>>>(r);
            if (grp > 1) k_recip_c0_var_grp<<<(unsigned)(((size_t)grp * n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, a>>>(r, grp);
            else k_recip_c0_var<<<blocks, BPPP_BLOCK, 0, a>>>(r);
        });
    } else GLAUNCH(s, K_RECIP_C0_VAR, k_recip_c0_var<<<blocks, BPPP_BLOCK, 0, s>>>(r));
    if (beside) {
        HIP_TRY(hipEventRecord(c->ev_join, a));
        HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
    }
    GLAUNCH(s, K_RECIP_C0_FINISH, k_recip_c0_finish<<<blocks, BPPP_BLOCK, 0, s>>>(r));
    rc = part_milestone(part, 2, s);
    if (rc != BPPP_OK) return rc;
    return wnla_verify_stage(c, w, plan, s, beside, rlc_seed, d, o.rlc, part);      // (the final sum in RLC mode whenever a seed is given, at any n)
}
static int recip_verify_check_args(const bppp_ctx* c, size_t dim_nd, size_t dim_np, size_t rounds, size_t nl, size_t nn) {
    if (dim_nd == 0 || dim_np == 0 || dim_nd > (size_t)c->ng || dim_nd + 10 > (size_t)c->nh || dim_np > dim_nd + 1 || rounds > 12 ||
        nl > 4096 || nn > 4096)
        return BPPP_ERR_INVALID_ARG;
    return BPPP_OK;
}
// ReciprocalRangeProofProtocol { dim_nd: 16, dim_np: 16 } over 16 + 32 generators with a standard-shape proof IS the u64 protocol
// (u64_proof.rs:42-54 builds exactly this and calls reciprocal verify), and its proof layout is the 928-byte u64 form: the specialised
// kernels (closed-form scalars, affine window tables, fixed-base tables shared with the generic path) take such calls -- an order of
// magnitude faster than the generic kernels, same verdicts and statuses.  BPPP_GENERIC_U64_SHAPE=1 keeps the generic kernels (A/B, tests).
static bool recip_is_u64_shape(const bppp_ctx* c, size_t dim_nd, size_t dim_np, size_t rounds, size_t nl, size_t nn) {
    return !c->generic_u64_shape && c->ng == 16 && c->nh == 32 && dim_nd == 16 && dim_np == 16 && rounds == 4 && nl == 2 && nn == 1;
}
int recip_verify_device_entry(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                              const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl, size_t nn, void* d_accept,
                              void* d_status, const uint8_t* rlc_seed, void* d_reject_count) {
    if (!c || !label_ok(label, label_len) || !d_commitments || !d_proofs || !d_accept || !d_status) return BPPP_ERR_INVALID_ARG;
    int rc = recip_verify_check_args(c, dim_nd, dim_np, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (recip_is_u64_shape(c, dim_nd, dim_np, rounds, nl, nn))
        return verify_device_impl(c, label, label_len, n, d_commitments, d_proofs, d_accept, d_status, nullptr, d_reject_count, rlc_seed, nullptr);
    HIP_TRY(hipSetDevice(c->device));
    rc = reset_reject_count(c, d_reject_count);
    if (rc != BPPP_OK || n == 0) return rc;
    rc = ensure_straus_capacity(c, n);
    if (rc != BPPP_OK) return rc;
    // A call that leaves the chip under-filled runs as K PARTS on K streams.  One lane per instance gives 2^15 instances of BASELINE
    // configs[4]'s shape 512 wavefronts on 1,024 SIMDs for phase 1, the C0 tables and sum, the round tables and the eight rounds -- a
    // third of the step waiting on lone wavefronts' dependent chains -- while the two fixed-base sums (8 lanes per instance: 769 and 263
    // bases) fill it.  Instances are independent, so the parts need no ordering among themselves: one part's fixed-base sums run under
    // another part's one-lane kernels, and the wavefront slots the chains leave idle do the sums' work.
    const int K = bppp_host::plan_generic_parts(n, rlc_seed != nullptr, c->timing, c->generic_parts);
    if (K > 1) {
        rc = bppp_ensure_twin_lanes(c);
        if (rc != BPPP_OK) return rc;
        size_t m[4], lo[4], ws_off[4], gt_off[4], ws_total = 0, gt_total = 0;
        const size_t per = ((n + (size_t)K - 1) / (size_t)K + BPPP_BLOCK - 1) / BPPP_BLOCK * BPPP_BLOCK;
        int parts = 0;
        for (size_t a = 0; a < n; a += per, parts++) {
            lo[parts] = a; m[parts] = n - a < per ? n - a : per;
            ws_off[parts] = ws_total; ws_total += align16(recip_verify_ws_bytes(c, m[parts], dim_nd, dim_np, rounds, false)) + 256;
            gt_off[parts] = gt_total; gt_total += wnla_fast_bytes(m[parts], rounds, 5) + 256;
        }
        rc = ensure_buffer(c, c->d_gws, c->gws_bytes, ws_total);
        if (rc != BPPP_OK) return rc;
        const bool fast = bppp_host::generic_fast(rounds, generic_knobs_of(c));
        if (fast) {
            rc = ensure_buffer(c, c->d_gtab, c->gtab_bytes, gt_total);
            if (rc != BPPP_OK) return rc;
        }
        hipStream_t streams[4] = {c->stream, c->twin_stream, c->aux_stream, c->twin_aux};
        hipEvent_t joins[4] = {nullptr, c->ev_twin_join, c->ev2_fork, c->ev2_join};
        hipEvent_t started[4] = {c->ev_tab, c->ev_fork, c->ev_join, nullptr};      // (free here: a part's kernels are one chain on one stream)
        const int stage = c->generic_stagger;
        const size_t proof_bytes = 64 * (5 + 2 * rounds) + 32 * (nl + nn);
        HIP_TRY(hipEventRecord(c->ev_twin_fork, c->stream));
        for (int i = 1; i < parts; i++) HIP_TRY(hipStreamWaitEvent(streams[i], c->ev_twin_fork, 0));
        int rc_parts = BPPP_OK;
        for (int i = 0; i < parts && rc_parts == BPPP_OK; i++) {
            const GenericPart gp = {streams[i], fast ? c->d_gtab + gt_off[i] : nullptr, c->d_straus + lo[i] * 5 * BPPP_STRAUS_ENTRIES, n,
                                    stage && i + 1 < parts ? started[i] : nullptr, stage, parts};
            if (stage && i > 0) HIP_TRY(hipStreamWaitEvent(streams[i], started[i - 1], 0));
            rc_parts = recip_verify_device_impl(c, label, label_len, m[i], dim_nd, dim_np, (const uint8_t*)d_commitments + 64 * lo[i],
                                                (const uint8_t*)d_proofs + proof_bytes * lo[i], rounds, nl, nn, (uint8_t*)d_accept + lo[i],
                                                (int32_t*)d_status + lo[i], c->d_gws + ws_off[i], nullptr, nullptr, &gp);
        }
        // (joined even after a failed launch: nothing of this call may outlive it on a stream the caller does not know)
        for (int i = 1; i < parts; i++) {
            HIP_TRY(hipEventRecord(joins[i], streams[i]));
            HIP_TRY(hipStreamWaitEvent(c->stream, joins[i], 0));
        }
        rc = rc_parts;
    } else {
        // persistent, grow-only workspace (the host-pointer entry point allocates per call instead)
        const size_t need = recip_verify_ws_bytes(c, n, dim_nd, dim_np, rounds, rlc_seed != nullptr);
        rc = ensure_buffer(c, c->d_gws, c->gws_bytes, need);
        if (rc != BPPP_OK) return rc;
        rc = recip_verify_device_impl(c, label, label_len, n, dim_nd, dim_np, (const uint8_t*)d_commitments, (const uint8_t*)d_proofs, rounds, nl,
                                      nn, (uint8_t*)d_accept, (int32_t*)d_status, c->d_gws, nullptr, rlc_seed);
    }
    return rc != BPPP_OK ? rc : launch_count_rejects(c, d_accept, n, d_reject_count);
}
int bppp_reciprocal_verify_batch_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                        const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl, size_t nn,
                                        void* d_accept, void* d_status) {
    CtxLock lock_(c);
    return recip_verify_device_entry(c, label, label_len, n, dim_nd, dim_np, d_commitments, d_proofs, rounds, nl, nn, d_accept, d_status, nullptr, nullptr);
}
int bppp_reciprocal_verify_batch_rlc_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                            const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl, size_t nn,
                                            void* d_accept, void* d_status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return recip_verify_device_entry(c, label, label_len, n, dim_nd, dim_np, d_commitments, d_proofs, rounds, nl, nn, d_accept, d_status, seed, nullptr);
}
static int recip_verify_host_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                  const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                  int32_t* status, const HostTranscripts* tx, const uint8_t* rlc_seed = nullptr);
int bppp_reciprocal_verify_batch_rlc(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                     const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                     int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return recip_verify_host_impl(c, label, label_len, n, dim_nd, dim_np, commitments, proofs, rounds, nl, nn, accept, status, nullptr, seed);
}
int bppp_reciprocal_verify_batch(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                 const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                 int32_t* status) {
    CtxLock lock_(c);
    return recip_verify_host_impl(c, label, label_len, n, dim_nd, dim_np, commitments, proofs, rounds, nl, nn, accept, status, nullptr);
}
int bppp_reciprocal_verify_batch_transcript(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, size_t dim_nd, size_t dim_np,
                                            const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn,
                                            uint8_t* accept, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    HostTranscripts tx = {states, n_states, states_out};
    return recip_verify_host_impl(c, nullptr, 0, n, dim_nd, dim_np, commitments, proofs, rounds, nl, nn, accept, status, &tx);
}
static int recip_verify_host_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                  const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                  int32_t* status, const HostTranscripts* tx, const uint8_t* rlc_seed) {
    if (!c || !label_ok(label, label_len) || !commitments || !proofs || !accept) return BPPP_ERR_INVALID_ARG;
    int rc = recip_verify_check_args(c, dim_nd, dim_np, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (n == 0) return BPPP_OK;
    rc = check_host_transcripts(tx, n);
    if (rc != BPPP_OK) return rc;
    if (recip_is_u64_shape(c, dim_nd, dim_np, rounds, nl, nn)) {      // the u64 protocol under its generic name: the specialised path
        if (tx) return bppp_u64_verify_batch_transcript(c, n, tx->states, tx->n_states, commitments, proofs, accept, status, tx->states_out);
        if (rlc_seed) return bppp_u64_verify_batch_rlc(c, label, label_len, n, commitments, proofs, accept, status, rlc_seed);
        return bppp_u64_verify_batch(c, label, label_len, n, commitments, proofs, accept, status);
    }
    HIP_TRY(hipSetDevice(c->device));
    rc = ensure_straus_capacity(c, n);
    if (rc != BPPP_OK) return rc;
    const size_t proof_bytes = 64 * (5 + 2 * rounds) + 32 * (nl + nn);
    HostStage hs;
    rc = hs.begin(c, false, {{commitments, n * 64}, {proofs, n * proof_bytes}}, n, tx,
                  recip_verify_ws_bytes(c, n, dim_nd, dim_np, rounds, rlc_seed != nullptr));
    if (rc != BPPP_OK) return rc;
    rc = recip_verify_device_impl(c, label, label_len, n, dim_nd, dim_np, hs.in[0], hs.in[1], rounds, nl, nn, hs.accept, hs.status, hs.tail,
                                  hs.dtio, rlc_seed);
    return hs.finish(rc, n, accept, status, tx);
}

// ---------------------------------------------------------------- aggregated reciprocal range proof: k values under one proof
// (agg_core.h has the protocol; tests/agg_cases.py states it on the oracle).  The verifier: phase 1 and the C0 stage of its own, then
// the WNLA stage, whose final sum runs exact or in RLC mode (a seed given).  k = 1 IS ReciprocalRangeProofProtocol and goes to that
// verifier's entry points.  The wire (SEC1) forms are with the other verifiers' at the end of this file.
struct AggVerifyLayout { size_t ts, sc0, pts, a, pf, inv, vs, wc, wcv, rho, mu, ys, tab, msc; WnlaRlcLayout rlc; size_t total; };
static AggVerifyLayout agg_verify_layout(const bppp_ctx* c, size_t n, size_t k, size_t dim_nd, size_t dim_np, size_t rounds, bool rlc = false) {
    const size_t NB = (size_t)c->nbases, T = (size_t)1 << rounds, NH = (size_t)c->nh, nm = k * dim_nd;
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes); };
    AggVerifyLayout o;
    o.ts = take(52 * n * 4); o.sc0 = take((nm + 5 + k) * 8 * n * 4); o.pts = take((4 + k) * 16 * n * 4); o.a = take(30 * n * 4);
    o.pf = take(30 * n * 4); o.inv = take(dim_np * 8 * n * 4); o.vs = take(k * 40 * n * 4); o.wc = take(n * 64); o.wcv = take(n * NH * 32);
    o.rho = take(n * 32); o.mu = take(n * 32); o.ys = take((rounds ? rounds : 1) * 8 * n * 4); o.tab = take(2 * T * 8 * n * 4);
    o.msc = take(NB * 8 * n * 4);
    o.rlc = {0, 0, 0, 0};
    if (rlc) o.rlc = wnla_rlc_take(off, n, NB);      // behind the aggregate's own buffers
    o.total = off;
    return o;
}
static size_t agg_proof_bytes(size_t k, size_t rounds, size_t nl, size_t nn) { return 64 * (4 + 2 * rounds + k) + 32 * (nl + nn); }
// 1 <= k <= 64, k dim_nd generators of g_vec and dim_nd + 10 of h_vec in the context, dim_np <= dim_nd + 1, the WNLA stage's bounds
static int agg_shape_check(size_t ng, size_t nh, size_t k, size_t dim_nd, size_t dim_np, size_t rounds, size_t nl, size_t nn) {
    if (k == 0 || k > 64 || dim_nd == 0 || dim_np == 0 || dim_nd > ng || k * dim_nd > ng || dim_nd + 10 > nh ||
        dim_np > dim_nd + 1 || rounds > 12 || nl > 4096 || nn > 4096)
        return BPPP_ERR_INVALID_ARG;
    return BPPP_OK;
}
// THE SHAPE OF AN AGGREGATE VERIFY CALL as its entry point was given it, handed down unchanged through the runs, the parts and the chain
// mixed: the call is one of MIXED value counts (agg_mixed_core.h) -- instance i has ks[i] values in slots laid out by k, its k_max
// rlc_seed: the final sum in RLC mode -- by the WNLA and circuit verifiers' rule (wnla_rlc_applies), so a part of fewer than 8
// instances runs the exact sum; everything before the final sum is the exact pipeline in the plan's launch form either way
struct AggCall { const uint8_t* label; size_t label_len, k; bool mixed; size_t dim_nd, dim_np, rounds, nl, nn; const uint8_t* rlc_seed; };
// the workspace of n instances of such a call over the buffers at d, laid out by o, and the caller's device buffers
static void agg_ws_fill(AggWs& r, const bppp_ctx* c, const AggCall& a, size_t n, uint8_t* d, const AggVerifyLayout& o, const uint8_t* d_com,
                        const uint8_t* d_proofs, int32_t* d_st) {
    r.N = n; r.k = (int)a.k; r.nd = (int)a.dim_nd; r.np = (int)a.dim_np; r.rounds = (int)a.rounds; r.nl = (int)a.nl; r.nn = (int)a.nn;
    r.NG = c->ng; r.NH = c->nh; r.proof_bytes = agg_proof_bytes(a.k, a.rounds, a.nl, a.nn);
    r.commitments = d_com; r.proofs = d_proofs; r.status = d_st; r.tstate = (u32*)(d + o.ts);
    r.sc0 = (u32*)(d + o.sc0); r.pts = (u32*)(d + o.pts); r.acc = (u32*)(d + o.a); r.pfix = (u32*)(d + o.pf); r.inv = (u32*)(d + o.inv);
    r.vsum = (u32*)(d + o.vs);
    r.straus = c->d_straus;
    r.wn_commit = d + o.wc; r.wn_c = d + o.wcv; r.wn_rho = d + o.rho; r.wn_mu = d + o.mu;
    r.fb = fb_table_of(c, n);
    t_new(r.base, a.label, (u32)a.label_len);
}
// the launch sequence of one call (or of one max_batch part of it), every buffer in device memory; d_ws holds agg_ws_bytes()
// d_ks (a mixed call): phase 1 and the variable-base half of C0 run on every instance's own count (k_agg_mixed.hip; k_i = 1 runs on
// these kernels too), phase 1 copies l | n behind the workspace and the WNLA stage reads them there.  No caller gives both d_ks and
// dtio: the _tx kernels are the uniform form's.  The RLC kernels read the final scalars, the commitments after the last round and the
// statuses out of the workspace, never the proof.
static int agg_verify_device_impl(bppp_ctx* c, const AggCall& call, size_t n, const uint8_t* d_ks, const uint8_t* d_com, const uint8_t* d_proofs,
                                  uint8_t* d_acc, int32_t* d_st, uint8_t* d_ws, const TranscriptIo* dtio) {
    const size_t k = call.k, rounds = call.rounds, nl = call.nl, nn = call.nn;
    const GenericPlan plan = plan_generic(GENERIC_FORM_AGGREGATE, n, rounds, generic_knobs_of(c), n, 1, 4 + k);
    const bool rlc = call.rlc_seed && wnla_rlc_applies(n);
    const AggVerifyLayout o = agg_verify_layout(c, n, k, call.dim_nd, call.dim_np, rounds, rlc);
    uint8_t* d = d_ws;
    hipStream_t s = c->stream;
    AggMixedWs m;                 // (the uniform kernels take its AggWs alone)
    std::memset(&m, 0, sizeof m);
    AggWs& r = m.w;
    agg_ws_fill(r, c, call, n, d, o, d_com, d_proofs, d_st);
    if (dtio) r.tio = *dtio;      // the caller's transcripts: phase 1 starts on them, the WNLA stage (tio, divergent_positions) exports them
    WnlaWs w = wnla_ws_continuing(c, r, 4 + k, nl, nn, d_acc, (u32*)(d + o.ys), (u32*)(d + o.tab), (u32*)(d + o.msc));
    if (d_ks) {
        m.ks = d_ks; m.ln = d + o.total;
        w.proof_l = m.ln; w.proof_n = m.ln + 32 * nl;       // (r and x sit at one offset for every k_i and are read in place)
        w.stride_l = w.stride_n = 32 * (nl + nn);
    }
    const unsigned blocks = blocks_of(n);
    int rc;
    // the WNLA stage's table buffer with room for the 4 + k points of C0's variable-base part behind the round points' tables
    rc = wnla_fast_setup(c, w, plan, 4 + k);
    if (rc != BPPP_OK) return rc;
    r.atab = w.atab; r.tscr = w.tscr; r.atab_first = wnla_atab_first(plan, rounds);
    // as the reciprocal verifier: what needs only the proof bytes (the round points' tables) and what needs only phase 1 (the C0
    // points' tables and sum) on the helper stream, beside phase 1 and the fixed-base half of C0
    const bool beside = plan.beside;
    hipStream_t a = beside ? c->aux_stream : s;
    const int G = plan.p1_group;
    c->last_generic_form = plan.code();
    if (beside) {
        HIP_TRY(hipEventRecord(c->ev_tab, s));               // (the call's inputs are ready on s)
        HIP_TRY(hipStreamWaitEvent(a, c->ev_tab, 0));
        GLAUNCH(a, K_WNLA_TABLES, launch_wnla_tables(w, plan.tab_parts, n, blocks, a));
    }
    const unsigned p1_blocks = G > 1 ? (unsigned)(((size_t)G * n + BPPP_BLOCK - 1) / BPPP_BLOCK) : blocks;
    if (d_ks) {
        if (G > 1) GLAUNCH(s, K_AGG_PHASE1, k_agg_mixed_phase1_grp<<<p1_blocks, BPPP_BLOCK, 0, s>>>(m, G));
        else GLAUNCH(s, K_AGG_PHASE1, k_agg_mixed_phase1<<<blocks, BPPP_BLOCK, 0, s>>>(m));
    } else if (r.tio.states) {      // the caller's transcripts: the _tx kernels, same launch form
        if (G > 1) GLAUNCH(s, K_AGG_PHASE1, k_agg_phase1_grp_tx<<<p1_blocks, BPPP_BLOCK, 0, s>>>(r, G));
        else GLAUNCH(s, K_AGG_PHASE1, k_agg_phase1_tx<<<p1_blocks, BPPP_BLOCK, 0, s>>>(r));
    } else if (G > 1) GLAUNCH(s, K_AGG_PHASE1, k_agg_phase1_grp<<<p1_blocks, BPPP_BLOCK, 0, s>>>(r, G));
    else GLAUNCH(s, K_AGG_PHASE1, k_agg_phase1<<<blocks, BPPP_BLOCK, 0, s>>>(r));
    if (beside) {
        HIP_TRY(hipEventRecord(c->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(a, c->ev_fork, 0));
    }
    if (plan.fb == GENERIC_FB_ONE_LANE) GLAUNCH(s, K_AGG_C0_FIXED, k_agg_c0_fixed_l1<<<fb1_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    else if (plan.fb == GENERIC_FB_WAVEFRONT) GLAUNCH(s, K_AGG_C0_FIXED, k_agg_c0_fixed_l64<<<fb64_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    else GLAUNCH(s, K_AGG_C0_FIXED, k_agg_c0_fixed<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    GLAUNCH(a, K_AGG_C0_VAR, {
        if (d_ks) {
            if (plan.fast) k_agg_mixed_c0_tables<<<blocks, BPPP_BLOCK, 0, a>>>(m);
            k_agg_mixed_c0_var<<<blocks, BPPP_BLOCK, 0, a>>>(m);
        } else {
            if (plan.fast) k_agg_c0_tables<<<blocks, BPPP_BLOCK, 0, a>>>(r);
            k_agg_c0_var<<<blocks, BPPP_BLOCK, 0, a>>>(r);
        }
    });
    if (beside) {
        HIP_TRY(hipEventRecord(c->ev_join, a));
        HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
    }
    GLAUNCH(s, K_AGG_C0_FINISH, k_agg_c0_finish<<<blocks, BPPP_BLOCK, 0, s>>>(r));
    return wnla_verify_stage(c, w, plan, s, beside, rlc ? call.rlc_seed : nullptr, d, o.rlc);
}
// a call of more than max_batch instances runs as consecutive parts on the context's stream over one workspace, as the u64 verifier's
// (instances are independent), each with its own slice of ks where the call is a mixed one; d_ws: agg_ws_bytes(min(n, max_batch))
static size_t agg_part_size(const bppp_ctx* c, size_t n) { return n < c->max_batch ? n : c->max_batch; }
static int agg_verify_parts(bppp_ctx* c, const AggCall& a, size_t n, const uint8_t* d_ks, const uint8_t* d_com, const uint8_t* d_proofs,
                            uint8_t* d_acc, int32_t* d_st, uint8_t* d_ws, const TranscriptIo* dtio) {
    const size_t per = agg_part_size(c, n), pb = agg_proof_bytes(a.k, a.rounds, a.nl, a.nn);
    unsigned first_super_m = 0, first_chunk = 0;
    for (size_t lo = 0; lo < n; lo += per) {
        const size_t m = n - lo < per ? n - lo : per;
        // a part's own slice of the caller's states (or the one shared state) and of states_out
        TranscriptIo pio = {nullptr, 0, nullptr, 0};
        if (dtio) {
            const bool shared = dtio->n_states == 1;
            pio.states = dtio->states + (shared ? 0 : 203 * lo); pio.n_states = shared ? 1 : m;
            pio.states_out = dtio->states_out ? dtio->states_out + 203 * lo : nullptr;
        }
        const int rc = agg_verify_device_impl(c, a, m, d_ks ? d_ks + lo : nullptr, d_com + 64 * a.k * lo, d_proofs + pb * lo, d_acc + lo, d_st + lo,
                                              d_ws, dtio ? &pio : nullptr);
        if (rc != BPPP_OK) return rc;
        if (lo == 0) { first_super_m = c->last_rlc_super_m; first_chunk = c->last_rlc_chunk; }
    }
    // "last_rlc_*": what the first part used (every part but the last has its size); (0, 0) where it ran the exact sum
    if (a.rlc_seed) { c->last_rlc_super_m = first_super_m; c->last_rlc_chunk = first_chunk; }
    return BPPP_OK;
}
// what a call allocates in front of its parts besides its workspace; "last_rlc_*" reset first, so that a failing call reports nothing stale
static int agg_verify_prepare(bppp_ctx* c, size_t per, const uint8_t* rlc_seed) {
    rlc_report_reset(c, rlc_seed);
    const int rc = ensure_straus_capacity(c, per);
    if (rc != BPPP_OK) return rc;
    return rlc_seed && wnla_rlc_applies(per) ? wnla_rlc_prepare(c, per) : BPPP_OK;
}
// the workspace of a call or part: the uniform one for k (k_max), its RLC buffers included, and behind it the l | n copies of a mixed call
static size_t agg_mixed_ws_bytes(const bppp_ctx* c, size_t n, size_t k_max, size_t dim_nd, size_t dim_np, size_t rounds, size_t nl, size_t nn,
                                 bool rlc) {
    return agg_verify_layout(c, n, k_max, dim_nd, dim_np, rounds, rlc).total + align16(n * 32 * (nl + nn));
}
static size_t agg_ws_bytes(const bppp_ctx* c, const AggCall& a, size_t n) {
    const bool rlc = a.rlc_seed != nullptr;
    return a.mixed ? agg_mixed_ws_bytes(c, n, a.k, a.dim_nd, a.dim_np, a.rounds, a.nl, a.nn, rlc)
                   : agg_verify_layout(c, n, a.k, a.dim_nd, a.dim_np, a.rounds, rlc).total;
}
// a call over device buffers, arguments checked (and k > 1 unless it is a mixed call, which forwards nothing): asynchronous on the
// context's stream, the workspace in the grow-only d_gws
static int agg_verify_device_run(bppp_ctx* c, const AggCall& a, size_t n, const void* d_ks, const void* d_commitments, const void* d_proofs,
                                 void* d_accept, void* d_status, void* d_reject_count, const TranscriptIo* dtio = nullptr) {
    HIP_TRY(hipSetDevice(c->device));
    int rc = reset_reject_count(c, d_reject_count);
    if (rc != BPPP_OK || n == 0) return rc;
    const size_t per = agg_part_size(c, n);
    rc = agg_verify_prepare(c, per, a.rlc_seed);
    if (rc != BPPP_OK) return rc;
    rc = ensure_buffer(c, c->d_gws, c->gws_bytes, agg_ws_bytes(c, a, per));
    if (rc != BPPP_OK) return rc;
    rc = agg_verify_parts(c, a, n, (const uint8_t*)d_ks, (const uint8_t*)d_commitments, (const uint8_t*)d_proofs, (uint8_t*)d_accept,
                          (int32_t*)d_status, c->d_gws, dtio);
    return rc != BPPP_OK ? rc : launch_count_rejects(c, d_accept, n, d_reject_count);
}
// what every aggregate entry point decides first: its buffers (ptrs_ok), the label, the shape and, of a mixed call, ks (host memory:
// every count in [1, k]; device memory: only that it is given -- an instance outside the range is flagged where it is read)
static int agg_call_check(const bppp_ctx* c, const AggCall& a, bool ptrs_ok, size_t n, const void* ks, int ks_on_device) {
    if (!c || !label_ok(a.label, a.label_len) || !ptrs_ok) return BPPP_ERR_INVALID_ARG;
    if (!a.mixed) return agg_shape_check((size_t)c->ng, (size_t)c->nh, a.k, a.dim_nd, a.dim_np, a.rounds, a.nl, a.nn);
    return bppp_reciprocal_agg_mixed_check_args((size_t)c->ng, (size_t)c->nh, n, a.k, (const uint8_t*)ks, ks_on_device, a.dim_nd, a.dim_np,
                                                a.rounds, a.nl, a.nn);
}
// device buffers: a uniform call of k = 1 IS the reciprocal verifier's; d_ks null unless the call is a mixed one
static int agg_verify_device_entry(bppp_ctx* c, const AggCall& a, size_t n, const void* d_ks, const void* d_commitments, const void* d_proofs,
                                   void* d_accept, void* d_status, void* d_reject_count) {
    const int rc = agg_call_check(c, a, d_commitments && d_proofs && d_accept && d_status, n, d_ks, 1);
    if (rc != BPPP_OK) return rc;
    if (!a.mixed && a.k == 1)
        return recip_verify_device_entry(c, a.label, a.label_len, n, a.dim_nd, a.dim_np, d_commitments, d_proofs, a.rounds, a.nl, a.nn, d_accept,
                                         d_status, a.rlc_seed, d_reject_count);
    return agg_verify_device_run(c, a, n, d_ks, d_commitments, d_proofs, d_accept, d_status, d_reject_count);
}
// host buffers, staged in the blob (ks, of a mixed call, behind the proofs -- the whole slots go up; the kernels read an instance's first
// k_i commitments and proof_bytes(k_i) bytes only).  tx (the _transcript form, uniform calls only): the callers' transcripts in (1 or n),
// each instance's advanced transcript out; label null
static int agg_verify_host_entry(bppp_ctx* c, const AggCall& a, size_t n, const uint8_t* ks, const uint8_t* commitments, const uint8_t* proofs,
                                 uint8_t* accept, int32_t* status, const HostTranscripts* tx = nullptr) {
    int rc = agg_call_check(c, a, commitments && proofs && accept, n, ks, 0);
    if (rc != BPPP_OK) return rc;
    if (tx && (!tx->states || (tx->n_states != 1 && tx->n_states != n))) return BPPP_ERR_INVALID_ARG;
    if (!a.mixed && a.k == 1)
        return recip_verify_host_impl(c, a.label, a.label_len, n, a.dim_nd, a.dim_np, commitments, proofs, a.rounds, a.nl, a.nn, accept, status, tx,
                                      a.rlc_seed);
    if (n == 0) return BPPP_OK;
    rc = check_host_transcripts(tx, n);
    if (rc != BPPP_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t per = agg_part_size(c, n);
    rc = agg_verify_prepare(c, per, a.rlc_seed);
    if (rc != BPPP_OK) return rc;
    HostStage hs;
    rc = hs.begin(c, false, {{commitments, n * a.k * 64}, {proofs, n * agg_proof_bytes(a.k, a.rounds, a.nl, a.nn)}, {ks, a.mixed ? n : 0}}, n, tx,
                  agg_ws_bytes(c, a, per));
    if (rc != BPPP_OK) return rc;
    rc = agg_verify_parts(c, a, n, a.mixed ? hs.in[2] : nullptr, hs.in[0], hs.in[1], hs.accept, hs.status, hs.tail, hs.dtio);
    return hs.finish(rc, n, accept, status, tx);
}
size_t bppp_reciprocal_agg_proof_bytes(size_t k, size_t rounds, size_t nl, size_t nn) { return agg_proof_bytes(k, rounds, nl, nn); }
int bppp_reciprocal_agg_verify_batch_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                            size_t dim_np, const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl,
                                            size_t nn, void* d_accept, void* d_status, void* d_reject_count) {
    CtxLock lock_(c);
    return agg_verify_device_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, nullptr, d_commitments, d_proofs,
                                   d_accept, d_status, d_reject_count);
}
int bppp_reciprocal_agg_verify_batch_rlc_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                size_t dim_np, const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl,
                                                size_t nn, void* d_accept, void* d_status, void* d_reject_count, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_verify_device_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, seed}, n, nullptr, d_commitments, d_proofs,
                                   d_accept, d_status, d_reject_count);
}
int bppp_reciprocal_agg_verify_batch(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd, size_t dim_np,
                                     const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                     int32_t* status) {
    CtxLock lock_(c);
    return agg_verify_host_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, nullptr, commitments, proofs,
                                 accept, status);
}
int bppp_reciprocal_agg_verify_batch_rlc(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd, size_t dim_np,
                                         const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                         int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_verify_host_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, seed}, n, nullptr, commitments, proofs,
                                 accept, status);
}
// ---- the aggregate on the CALLER'S transcripts (`t: &mut Transcript`): the states in (1 shared or n), every instance's advanced
//      transcript out; an instance flagged BPPP_ST_BAD_ENCODING gets its input state back.  No RLC form, as for the other protocols.
int bppp_reciprocal_agg_verify_batch_transcript(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, size_t k, size_t dim_nd,
                                                size_t dim_np, const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl,
                                                size_t nn, uint8_t* accept, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    const HostTranscripts tx = {states, n_states, states_out};
    return agg_verify_host_entry(c, {nullptr, 0, k, false, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, nullptr, commitments, proofs,
                                 accept, status, &tx);
}
// k = 1 over device buffers: the reciprocal verifier on the caller's device states (the u64 kernels for the u64 shape), one launch chain
// on the context's stream with the workspace in the grow-only buffer
static int recip_verify_transcript_device(bppp_ctx* c, size_t n, const void* d_states, size_t n_states, size_t dim_nd, size_t dim_np,
                                          const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl, size_t nn, void* d_accept,
                                          void* d_status, void* d_reject_count, void* d_states_out) {
    int rc = recip_verify_check_args(c, dim_nd, dim_np, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (recip_is_u64_shape(c, dim_nd, dim_np, rounds, nl, nn)) {
        const VerifyTranscripts tx = {d_states, n_states, d_states_out};
        return verify_device_impl(c, nullptr, 0, n, d_commitments, d_proofs, d_accept, d_status, nullptr, d_reject_count, nullptr, &tx);
    }
    HIP_TRY(hipSetDevice(c->device));
    rc = reset_reject_count(c, d_reject_count);
    if (rc != BPPP_OK || n == 0) return rc;
    rc = ensure_straus_capacity(c, n);
    if (rc != BPPP_OK) return rc;
    rc = ensure_buffer(c, c->d_gws, c->gws_bytes, recip_verify_ws_bytes(c, n, dim_nd, dim_np, rounds, false));
    if (rc != BPPP_OK) return rc;
    const TranscriptIo dtio = {(const uint8_t*)d_states, n_states, (uint8_t*)d_states_out, 0};
    rc = recip_verify_device_impl(c, nullptr, 0, n, dim_nd, dim_np, (const uint8_t*)d_commitments, (const uint8_t*)d_proofs, rounds, nl, nn,
                                  (uint8_t*)d_accept, (int32_t*)d_status, c->d_gws, &dtio, nullptr);
    return rc != BPPP_OK ? rc : launch_count_rejects(c, d_accept, n, d_reject_count);
}
// device buffers: the states cannot be read here, so a state merlin cannot be in flags its instance (BPPP_ST_BAD_ENCODING) on the device
int bppp_reciprocal_agg_verify_batch_transcript_device(bppp_ctx* c, size_t n, const void* d_states, size_t n_states, size_t k, size_t dim_nd,
                                                       size_t dim_np, const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl,
                                                       size_t nn, void* d_accept, void* d_status, void* d_reject_count, void* d_states_out) {
    CtxLock lock_(c);
    const AggCall a = {nullptr, 0, k, false, dim_nd, dim_np, rounds, nl, nn, nullptr};
    const int rc = agg_call_check(c, a, d_states && (n_states == 1 || n_states == n) && d_commitments && d_proofs && d_accept && d_status, n, nullptr, 1);
    if (rc != BPPP_OK) return rc;
    if (k == 1)
        return recip_verify_transcript_device(c, n, d_states, n_states, dim_nd, dim_np, d_commitments, d_proofs, rounds, nl, nn, d_accept, d_status,
                                              d_reject_count, d_states_out);
    const TranscriptIo dtio = {(const uint8_t*)d_states, n_states, (uint8_t*)d_states_out, 0};
    return agg_verify_device_run(c, a, n, nullptr, d_commitments, d_proofs, d_accept, d_status, d_reject_count, &dtio);
}
// ---- aggregates of MIXED value counts in one batch (agg_mixed_core.h): instance i has ks[i] values in slots laid out by k_max.  Label
//      transcripts; the final sum exact or in RLC mode (a seed given).  The launch chain, the parts and the runs are the uniform
//      aggregate's on an AggCall that says `mixed` (agg_verify_device_impl and what follows it); only the argument check is the
//      mixed calls' own, and nothing is forwarded.  The wire (SEC1) forms are with the other verifiers' at the end of this file.
// what the two mixed calls decide about their arguments besides the NULL checks of the buffers, on a context of ng | nh generators in
// g_vec || g_vec_ | h_vec || h_vec_; pure, so that it can be asked without a context or a device.  ks_on_device: ks is only checked
// for NULL (the device form: an instance outside [1, k_max] is flagged where it is read)
int bppp_reciprocal_agg_mixed_check_args(size_t ng, size_t nh, size_t n, size_t k_max, const uint8_t* ks, int ks_on_device, size_t dim_nd,
                                         size_t dim_np, size_t rounds, size_t nl, size_t nn) {
    if (!ks) return BPPP_ERR_INVALID_ARG;
    const int rc = agg_shape_check(ng, nh, k_max, dim_nd, dim_np, rounds, nl, nn);
    if (rc != BPPP_OK || ks_on_device) return rc;
    for (size_t i = 0; i < n; i++)
        if (ks[i] == 0 || ks[i] > k_max) return BPPP_ERR_INVALID_ARG;
    return BPPP_OK;
}
int bppp_reciprocal_agg_verify_batch_mixed_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max, const void* d_ks,
                                                  size_t dim_nd, size_t dim_np, const void* d_commitments, const void* d_proofs, size_t rounds,
                                                  size_t nl, size_t nn, void* d_accept, void* d_status, void* d_reject_count) {
    CtxLock lock_(c);
    return agg_verify_device_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, d_ks, d_commitments, d_proofs,
                                   d_accept, d_status, d_reject_count);
}
int bppp_reciprocal_agg_verify_batch_mixed_rlc_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max,
                                                      const void* d_ks, size_t dim_nd, size_t dim_np, const void* d_commitments,
                                                      const void* d_proofs, size_t rounds, size_t nl, size_t nn, void* d_accept, void* d_status,
                                                      void* d_reject_count, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_verify_device_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, seed}, n, d_ks, d_commitments, d_proofs,
                                   d_accept, d_status, d_reject_count);
}
int bppp_reciprocal_agg_verify_batch_mixed(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max, const uint8_t* ks,
                                           size_t dim_nd, size_t dim_np, const uint8_t* commitments, const uint8_t* proofs, size_t rounds,
                                           size_t nl, size_t nn, uint8_t* accept, int32_t* status) {
    CtxLock lock_(c);
    return agg_verify_host_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, ks, commitments, proofs,
                                 accept, status);
}
int bppp_reciprocal_agg_verify_batch_mixed_rlc(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max, const uint8_t* ks,
                                               size_t dim_nd, size_t dim_np, const uint8_t* commitments, const uint8_t* proofs, size_t rounds,
                                               size_t nl, size_t nn, uint8_t* accept, int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_verify_host_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, seed}, n, ks, commitments, proofs,
                                 accept, status);
}

// ---------------------------------------------------------------- generic ArithmeticCircuit (circuit.rs:95-256)
struct bppp_circuit {
    CircuitDev cd;
    const int* d_part = nullptr;     // [3 nv + nm]: LO | LL | LR | NO (the prover places w_o with it)
    uint8_t* d_blob = nullptr;
    size_t blob_bytes = 0;
};
int bppp_circuit_create(bppp_ctx* c, bppp_circuit** out, const size_t dims[6], int f_l, int f_m, const uint8_t* W_m, const uint8_t* W_l,
                        const uint8_t* a_m, const uint8_t* a_l, const int32_t* part_lo, const int32_t* part_ll, const int32_t* part_lr,
                        const int32_t* part_no) {
    CtxLock lock_(c);
    if (!c || !out || !dims || !W_m || !W_l || !a_m || !a_l || !part_lo || !part_ll || !part_lr || !part_no) return BPPP_ERR_INVALID_ARG;
    const size_t nm = dims[0], no = dims[1], k = dims[2], nl = dims[3], nv = dims[4], nw = dims[5];
    // the reference's own definitions (circuit.rs:100-106) and what the context's generators can serve
    if (nm == 0 || nv == 0 || k == 0 || nl != nv * k || nw != 2 * nm + no || nm > (size_t)c->ng || nv + 9 > (size_t)c->nh || k > 1024 ||
        nm > 65536 || nv > 65536 || no > 65536)
        return BPPP_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    CircuitHostData hd;
    if (!circuit_host_build(hd, dims, W_m, W_l, a_m, a_l, part_lo, part_ll, part_lr, part_no)) return BPPP_ERR_INVALID_ARG;
    std::vector<int>&cpl = hd.cpl, &rl = hd.rl, &cpm = hd.cpm, &rm = hd.rm, &colmap = hd.colmap;
    std::vector<u32>&vl = hd.vl, &vm = hd.vm, &al = hd.al, &am = hd.am;
    bppp_circuit* q = new (std::nothrow) bppp_circuit();
    if (!q) return BPPP_ERR_INVALID_ARG;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align16(off + bytes + 16); return o; };
    const size_t o_cpl = take(cpl.size() * 4), o_rl = take(rl.size() * 4), o_vl = take(vl.size() * 4), o_cpm = take(cpm.size() * 4),
                 o_rm = take(rm.size() * 4), o_vm = take(vm.size() * 4), o_cm = take(colmap.size() * 4), o_al = take(al.size() * 4),
                 o_am = take(am.size() * 4);
    std::vector<int> parts(3 * nv + nm);
    for (size_t j = 0; j < nv; j++) { parts[j] = part_lo[j]; parts[nv + j] = part_ll[j]; parts[2 * nv + j] = part_lr[j]; }
    for (size_t j = 0; j < nm; j++) parts[3 * nv + j] = part_no[j];
    const size_t o_part = take(parts.size() * 4);
    hipError_t e = ctx_malloc(c, (void**)&q->d_blob, off);
    if (e != hipSuccess) {
        delete q;
        g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? BPPP_ERR_NOMEM : BPPP_ERR_HIP;
    }
    q->blob_bytes = off;
    auto up = [&](size_t o, const void* src, size_t bytes) { return bytes ? hipMemcpy(q->d_blob + o, src, bytes, hipMemcpyHostToDevice) : hipSuccess; };
    if (up(o_cpl, cpl.data(), cpl.size() * 4) != hipSuccess || up(o_rl, rl.data(), rl.size() * 4) != hipSuccess ||
        up(o_vl, vl.data(), vl.size() * 4) != hipSuccess || up(o_cpm, cpm.data(), cpm.size() * 4) != hipSuccess ||
        up(o_rm, rm.data(), rm.size() * 4) != hipSuccess || up(o_vm, vm.data(), vm.size() * 4) != hipSuccess ||
        up(o_cm, colmap.data(), colmap.size() * 4) != hipSuccess || up(o_al, al.data(), al.size() * 4) != hipSuccess ||
        up(o_am, am.data(), am.size() * 4) != hipSuccess || up(o_part, parts.data(), parts.size() * 4) != hipSuccess) {
        (void)hipFree(q->d_blob);
        delete q;
        g_last_error = "circuit upload failed";
        return BPPP_ERR_HIP;
    }
    CircuitDev& cd = q->cd;
    cd.nm = (int)nm; cd.no = (int)no; cd.k = (int)k; cd.nl = (int)nl; cd.nv = (int)nv; cd.nw = (int)nw; cd.f_l = f_l ? 1 : 0; cd.f_m = f_m ? 1 : 0;
    cd.colptr_l = (const int*)(q->d_blob + o_cpl); cd.rows_l = (const int*)(q->d_blob + o_rl); cd.vals_l = (const u32*)(q->d_blob + o_vl);
    cd.colptr_m = (const int*)(q->d_blob + o_cpm); cd.rows_m = (const int*)(q->d_blob + o_rm); cd.vals_m = (const u32*)(q->d_blob + o_vm);
    cd.colmap = (const int*)(q->d_blob + o_cm); cd.a_l = (const u32*)(q->d_blob + o_al); cd.a_m = (const u32*)(q->d_blob + o_am);
    q->d_part = (const int*)(q->d_blob + o_part);
    *out = q;
    return BPPP_OK;
}
void bppp_circuit_destroy(bppp_circuit* q) {
    if (!q) return;
    if (q->d_blob) (void)hipFree(q->d_blob);
    delete q;
}
// what every circuit verify entry point checks of its arguments (label: null with length 0 in the transcript form)
static int circuit_verify_check(const bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, const void* commitments,
                              const void* proofs, const void* accept, size_t rounds, size_t nl, size_t nn) {
    if (!c || !q || !label_ok(label, label_len) || !commitments || !proofs || !accept) return BPPP_ERR_INVALID_ARG;
    const CircuitDev& cd = q->cd;
    if (cd.nm > c->ng || cd.nv + 9 > c->nh || rounds > 12 || nl > 4096 || nn > 4096) return BPPP_ERR_INVALID_ARG;
    return BPPP_OK;
}
static int circuit_verify_host_impl(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                    const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                    int32_t* status, const HostTranscripts* tx, bool device_io = false, const uint8_t* rlc_seed = nullptr);
// ArithmeticCircuit::verify over DEVICE buffers (commitments n x k x 64, proofs, accept n, status n or null), asynchronous on the
// context's stream: the resident form of bppp_circuit_verify_batch
int bppp_circuit_verify_batch_device(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n, const void* d_commitments,
                                     const void* d_proofs, size_t rounds, size_t nl, size_t nn, void* d_accept, void* d_status) {
    CtxLock lock_(c);
    return circuit_verify_host_impl(c, q, label, label_len, n, (const uint8_t*)d_commitments, (const uint8_t*)d_proofs, rounds, nl, nn,
                                    (uint8_t*)d_accept, (int32_t*)d_status, nullptr, true);
}
int bppp_circuit_verify_batch(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments,
                              const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept, int32_t* status) {
    CtxLock lock_(c);
    return circuit_verify_host_impl(c, q, label, label_len, n, commitments, proofs, rounds, nl, nn, accept, status, nullptr);
}
// the same two in RLC mode (wnla_rlc_final_sum): the exact twins' argument checks, and a seed
int bppp_circuit_verify_batch_rlc(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments,
                                  const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept, int32_t* status,
                                  const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return circuit_verify_host_impl(c, q, label, label_len, n, commitments, proofs, rounds, nl, nn, accept, status, nullptr, false, seed);
}
int bppp_circuit_verify_batch_rlc_device(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                         const void* d_commitments, const void* d_proofs, size_t rounds, size_t nl, size_t nn, void* d_accept,
                                         void* d_status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return circuit_verify_host_impl(c, q, label, label_len, n, (const uint8_t*)d_commitments, (const uint8_t*)d_proofs, rounds, nl, nn,
                                    (uint8_t*)d_accept, (int32_t*)d_status, nullptr, true, seed);
}
int bppp_circuit_verify_batch_transcript(bppp_ctx* c, const bppp_circuit* q, size_t n, const uint8_t* states, size_t n_states,
                                         const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn,
                                         uint8_t* accept, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    HostTranscripts tx = {states, n_states, states_out};
    return circuit_verify_host_impl(c, q, nullptr, 0, n, commitments, proofs, rounds, nl, nn, accept, status, &tx);
}
static int circuit_verify_host_impl(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                    const uint8_t* commitments, const uint8_t* proofs, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                    int32_t* status, const HostTranscripts* tx, bool device_io, const uint8_t* rlc_seed) {
    // rlc_seed (bppp_circuit_verify_batch_rlc[_device]): the final sum in RLC mode (wnla_rlc_final_sum, and the rule above it)
    int rc = circuit_verify_check(c, q, label, label_len, commitments, proofs, accept, rounds, nl, nn);
    if (rc != BPPP_OK || n == 0) return rc;
    const CircuitDev& cd = q->cd;
    const GenericPlan plan = plan_generic(GENERIC_FORM_CIRCUIT, n, rounds, generic_knobs_of(c), n, 1, 4 + (size_t)cd.k);
    rc = check_host_transcripts(tx, n);
    if (rc != BPPP_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    bool rlc;
    rc = wnla_call_prepare(c, n, rlc_seed, rlc);
    if (rc != BPPP_OK) return rc;
    const size_t NB = (size_t)c->nbases, T = (size_t)1 << rounds, NH = (size_t)c->nh, k = (size_t)cd.k, nm = (size_t)cd.nm, nv = (size_t)cd.nv;
    const size_t proof_bytes = 64 * (4 + 2 * rounds) + 32 * (nl + nn);
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes); };
    const size_t o_com = take(n * k * 64), o_pr = take(n * proof_bytes), o_acc = take(n), o_st = take(n * 4), o_ts = take(52 * n * 4),
                 o_lam = take((size_t)cd.nl * 8 * n * 4), o_muv = take(nm * 8 * n * 4), o_coef = take((3 * nm + 3 * nv) * 8 * n * 4),
                 o_sc0 = take((nm + 5 + k) * 8 * n * 4), o_pts = take((4 + k) * 16 * n * 4), o_a = take(30 * n * 4), o_pf = take(30 * n * 4),
                 o_wc = take(n * 64), o_wcv = take(n * NH * 32), o_rho = take(n * 32), o_mu = take(n * 32),
                 o_ys = take((rounds ? rounds : 1) * 8 * n * 4), o_tab = take(2 * T * 8 * n * 4), o_msc = take(NB * 8 * n * 4),
                 o_ti = take(tx ? tx->n_states * 203 : 0), o_to = take(tx && tx->states_out ? n * 203 : 0);
    WnlaRlcLayout o_rlc = {0, 0, 0, 0};
    if (rlc) o_rlc = wnla_rlc_take(off, n, NB);
    WnlaBlob blob;
    if (device_io) { const int rc_b = ensure_blob(c, off + 16); if (rc_b != BPPP_OK) return rc_b; }       // (no sync when the call returns)
    else { const int rc_b = blob.take(c, off + 16); if (rc_b != BPPP_OK) return rc_b; }
    uint8_t* d = c->d_blob;
    hipStream_t s = c->stream;
    if (tx) HIP_TRY(hipMemcpyAsync(d + o_ti, tx->states, tx->n_states * 203, hipMemcpyHostToDevice, s));
    if (!device_io) {
        HIP_TRY(hipMemcpyAsync(d + o_com, commitments, n * k * 64, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d + o_pr, proofs, n * proof_bytes, hipMemcpyHostToDevice, s));
    }
    CircuitWs r;
    std::memset(&r, 0, sizeof r);
    r.N = n; r.cd = cd; r.rounds = (int)rounds; r.NG = c->ng; r.NH = c->nh; r.proof_bytes = proof_bytes;
    r.commitments = device_io ? commitments : d + o_com; r.proofs = device_io ? proofs : d + o_pr;
    r.status = (device_io && status) ? status : (int32_t*)(d + o_st); r.tstate = (u32*)(d + o_ts);
    r.lamv = (u32*)(d + o_lam); r.muv = (u32*)(d + o_muv); r.coef = (u32*)(d + o_coef); r.sc0 = (u32*)(d + o_sc0); r.pts = (u32*)(d + o_pts);
    r.acc = (u32*)(d + o_a); r.pfix = (u32*)(d + o_pf);
    r.straus = c->d_straus;
    r.wn_commit = d + o_wc; r.wn_c = d + o_wcv; r.wn_rho = d + o_rho; r.wn_mu = d + o_mu;
    r.fb = fb_table_of(c, n);
    t_new(r.base, label, (u32)label_len);
    if (tx) { r.tio.states = d + o_ti; r.tio.n_states = tx->n_states; r.tio.states_out = tx->states_out ? d + o_to : nullptr; }
    WnlaWs w = wnla_ws_continuing(c, r, 4, nl, nn, device_io ? accept : d + o_acc, (u32*)(d + o_ys), (u32*)(d + o_tab), (u32*)(d + o_msc));
    const unsigned blocks = blocks_of(n);
    // the WNLA stage's table buffer with room for the 4 + k points of C0's variable-base part behind the round points' tables
    rc = wnla_fast_setup(c, w, plan, 4 + k);
    if (rc != BPPP_OK) return rc;
    r.atab = w.atab; r.tscr = w.tscr; r.atab_first = wnla_atab_first(plan, rounds);
    c->last_generic_form = plan.code();
    GLAUNCH(s, K_CIRCUIT_PHASE1, k_circuit_phase1<<<blocks, BPPP_BLOCK, 0, s>>>(r));
    if (plan.fb == GENERIC_FB_WAVEFRONT) GLAUNCH(s, K_CIRCUIT_C0_FIXED, k_circuit_c0_fixed_l64<<<fb64_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    else GLAUNCH(s, K_CIRCUIT_C0_FIXED, k_circuit_c0_fixed<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r));
    GLAUNCH(s, K_CIRCUIT_C0_VAR, {
        // (a lane per point: tables and sum in one launch)
        if (plan.per_point) k_circuit_c0_var_pts<<<(unsigned)(((size_t)plan.c0_lanes * n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, s>>>(r, plan.c0_lanes);
        else {
            if (plan.fast) k_circuit_c0_tables<<<blocks, BPPP_BLOCK, 0, s>>>(r);
            k_circuit_c0_var<<<blocks, BPPP_BLOCK, 0, s>>>(r);
        }
    });
    GLAUNCH(s, K_CIRCUIT_C0_FINISH, k_circuit_c0_finish<<<blocks, BPPP_BLOCK, 0, s>>>(r));
    rc = wnla_verify_stage(c, w, plan, s, false, rlc ? rlc_seed : nullptr, d, o_rlc);
    if (rc != BPPP_OK) return rc;
    if (device_io) return BPPP_OK;
    HIP_TRY(hipMemcpyAsync(accept, d + o_acc, n, hipMemcpyDeviceToHost, s));
    if (w.tio.states_out) HIP_TRY(hipMemcpyAsync(tx->states_out, d + o_to, n * 203, hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(hipMemcpyAsync(status, d + o_st, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BPPP_OK;
}

// sum_j scalars[i][j] * generator[base_index[j]] for n independent rows, through the context's fixed-base tables: the crate's
// commit functions (circuit.rs:146-151, reciprocal.rs:88-95, u64_proof.rs:37-39) are instances of this with fixed index lists.
int bppp_msm_batch(bppp_ctx* c, size_t n, size_t nterms, const int32_t* base_index, const uint8_t* scalars, uint8_t* out, int32_t* status) {
    CtxLock lock_(c);
    if (!c || !base_index || !scalars || !out || nterms == 0 || nterms > 65536) return BPPP_ERR_INVALID_ARG;
    for (size_t j = 0; j < nterms; j++) {
        if (base_index[j] < 0 || base_index[j] >= c->nbases) return BPPP_ERR_INVALID_ARG;
        if (j && base_index[j] <= base_index[j - 1]) return BPPP_ERR_INVALID_ARG;      // strictly increasing
    }
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int> runs;
    for (size_t j = 0; j < nterms;) {
        size_t e = j + 1;
        while (e < nterms && base_index[e] == base_index[e - 1] + 1) e++;
        runs.push_back((int)j); runs.push_back(base_index[j]); runs.push_back((int)(e - j));
        j = e;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align16(off + bytes); return o; };
    const size_t o_sc = take(n * nterms * 32), o_runs = take(runs.size() * 4), o_msc = take(nterms * 8 * n * 4), o_pf = take(30 * n * 4),
                 o_st = take(n * 4), o_out = take(n * 64);
    WnlaBlob blob;
    { const int rc_b = blob.take(c, off); if (rc_b != BPPP_OK) return rc_b; }
    uint8_t* d = blob.d;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_sc, scalars, n * nterms * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_runs, runs.data(), runs.size() * 4, hipMemcpyHostToDevice, s));
    MsmWs w;
    std::memset(&w, 0, sizeof w);
    w.N = n; w.nterms = (int)nterms; w.nruns = (int)(runs.size() / 3);
    w.scalars = d + o_sc; w.runs = (const int*)(d + o_runs); w.msc = (u32*)(d + o_msc); w.pfix = (u32*)(d + o_pf);
    w.status = (int32_t*)(d + o_st); w.out = d + o_out;
    w.fb = fb_table_of(c, n);
    const unsigned blocks = (unsigned)((n + BPPP_BLOCK - 1) / BPPP_BLOCK);
    const unsigned fb_blocks = (unsigned)((n * BPPP_FB_LANES + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK);
    k_msm_scalars<<<blocks, BPPP_BLOCK, 0, s>>>(w);
    k_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(w);
    k_msm_store<<<blocks, BPPP_BLOCK, 0, s>>>(w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d + o_out, n * 64, hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(hipMemcpyAsync(status, d + o_st, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BPPP_OK;
}

// WeightNormLinearArgument::prove (wnla.rs:125-190) for n instances sharing the context's generators.
void bppp_wnla_proof_shape(size_t nl, size_t nn, size_t* rounds, size_t* nl_out, size_t* nn_out) {
    size_t r, a, b;
    wnla_proof_shape(nl, nn, r, a, b);
    if (rounds) *rounds = r;
    if (nl_out) *nl_out = a;
    if (nn_out) *nn_out = b;
}
// "ct_prover" for the generic provers: the 4-bit table over THIS context's generators (built at the first use) for the sums over secret
// scalars -- every entry of every window read and selected by mask, complete additions (fb_core.h: fb_lookup_add_ct)
static int ct_setup(bppp_ctx* c, FbTable& fb_ct, int& ct, size_t n) {
    ct = 0;
    if (!c->ct_prover) return BPPP_OK;
    const int rc = ensure_ct_table(c);
    if (rc != BPPP_OK) return rc;
    fb_ct.table = c->d_table_ct; fb_ct.W = 4; fb_ct.N = n;
    ct = 1;
    return BPPP_OK;
}
// ---- the WNLA prove stage, the tail of all three generic provers
struct WnlaProveShape { size_t n, nl, nn, rounds, nl_f, nn_f; };      // instances | lengths of l and n | wnla_proof_shape of the two
struct WnlaProveBufs { size_t pr, px, pl, pn, vl, vn, vc, ch, cg, prm, cm; };
// The stage's buffers out of a caller's running layout, in two runs -- the proof fields it writes, then its state (the WNLA prover has
// its status and transcripts between the two).  pad: bytes of slack behind each buffer, as the caller's layout has always had them.
static void wnla_prove_take_proof(WnlaProveBufs& o, size_t& off, const WnlaProveShape& sh, size_t pad) {
    o.pr = take_bytes(off, sh.n * sh.rounds * 64 + pad); o.px = take_bytes(off, sh.n * sh.rounds * 64 + pad);
    o.pl = take_bytes(off, sh.n * sh.nl_f * 32 + pad); o.pn = take_bytes(off, sh.n * sh.nn_f * 32 + pad);
}
static void wnla_prove_take_state(WnlaProveBufs& o, size_t& off, const bppp_ctx* c, const WnlaProveShape& sh, size_t pad) {
    const size_t n = sh.n, ng = (size_t)c->ng, nh = (size_t)c->nh;
    o.vl = take_bytes(off, (sh.nl + 1) * 8 * n * 4 + pad); o.vn = take_bytes(off, (sh.nn + 1) * 8 * n * 4 + pad);
    o.vc = take_bytes(off, nh * 8 * n * 4 + pad); o.ch = take_bytes(off, nh * 8 * n * 4 + pad); o.cg = take_bytes(off, (ng + 1) * 8 * n * 4 + pad);
    o.prm = take_bytes(off, 3 * 8 * n * 4 + pad); o.cm = take_bytes(off, 16 * n * 4 + pad);
}
// The stage's WnlaProveWs over those buffers at d and the caller's inputs (device memory); grows the projective tables of X, R (the next
// commitment by the relation).  Left to the caller: the transcript (base, tio, or transcript_preloaded) and the "ct_prover" table.
static int wnla_prove_fill(bppp_ctx* c, WnlaProveWs& w, const WnlaProveShape& sh, uint8_t* d, const WnlaProveBufs& o, const uint8_t* commitments,
                           const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, const uint8_t* l_in, const uint8_t* n_in, int32_t* status,
                           u32* tstate, u32* msc, u32* pbuf) {
    std::memset(&w, 0, sizeof w);
    const int rc = ensure_straus_capacity(c, sh.n);
    if (rc != BPPP_OK) return rc;
    w.straus = c->d_straus;
    w.N = sh.n; w.ng = c->ng; w.nh = c->nh; w.nl = (int)sh.nl; w.nn = (int)sh.nn; w.rounds = (int)sh.rounds; w.nl_f = (int)sh.nl_f; w.nn_f = (int)sh.nn_f;
    w.commitments = commitments; w.c = cvec; w.rho = rho; w.mu = mu; w.l_in = l_in; w.n_in = n_in;
    w.proof_r = d + o.pr; w.proof_x = d + o.px; w.proof_l = d + o.pl; w.proof_n = d + o.pn;
    w.status = status; w.tstate = tstate; w.vl = (u32*)(d + o.vl); w.vn = (u32*)(d + o.vn); w.vc = (u32*)(d + o.vc);
    w.ch = (u32*)(d + o.ch); w.cg = (u32*)(d + o.cg); w.prm = (u32*)(d + o.prm); w.com = (u32*)(d + o.cm); w.msc = msc; w.pbuf = pbuf;
    w.fb = fb_table_of(c, sh.n);
    return BPPP_OK;
}
static void wnla_prove_launch(const WnlaProveWs& w, hipStream_t s) {
    const unsigned blocks = blocks_of(w.N), fb_blocks = fb_blocks_of(w.N);
    k_wprove_init<<<blocks, BPPP_BLOCK, 0, s>>>(w);
    for (int k = 0; k < w.rounds; k++) {
        k_wprove_round_scalars<<<blocks, BPPP_BLOCK, 0, s>>>(w, k);
        k_wprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(w, 0, -1);
        k_wprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(w, 1, k);
        k_wprove_round_fold<<<blocks, BPPP_BLOCK, 0, s>>>(w, k);
        if (k == 0 && w.rounds > 1) k_wprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(w, 2, -1);   // level 1's commitment; later levels by the relation
    }
    k_wprove_finish<<<blocks, BPPP_BLOCK, 0, s>>>(w);
}

// ---- the circuit prove stage, shared by the circuit prover and the reciprocal prover (whose circuit is built per call)
struct CircuitProveBufs { size_t r9, lv, nv, lam, muv, coef, misc, msc, pb, wc, wcv, rho, mu, wlv, wnv; };
// the stage's scalar vectors, scalar sets and what it hands to the WNLA stage, out of a caller's running layout (16 bytes of slack each)
static CircuitProveBufs circuit_prove_take(size_t& off, const bppp_ctx* c, size_t n, size_t nm, size_t nv, size_t nl) {
    const size_t NB = (size_t)c->nbases, NG = (size_t)c->ng, NH = (size_t)c->nh;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes + 16); };
    CircuitProveBufs o;
    o.r9 = take(4 * 9 * 8 * n * 4); o.lv = take(6 * nv * 8 * n * 4); o.nv = take(4 * nm * 8 * n * 4); o.lam = take(nl * 8 * n * 4);
    o.muv = take(nm * 8 * n * 4); o.coef = take((3 * nm + 3 * nv) * 8 * n * 4); o.misc = take(8 * 8 * n * 4); o.msc = take(3 * NB * 8 * n * 4);
    o.pb = take(3 * 30 * n * 4); o.wc = take(n * 64); o.wcv = take(n * NH * 32); o.rho = take(n * 32); o.mu = take(n * 32);
    o.wlv = take(n * NH * 32); o.wnv = take(n * NG * 32);
    return o;
}
// those buffers into a CircuitProveWs whose N and cd are set
static void circuit_prove_carve(CircuitProveWs& p, uint8_t* d, const CircuitProveBufs& o) {
    const size_t n = p.N, nm = (size_t)p.cd.nm, nv = (size_t)p.cd.nv;
    u32* r9 = (u32*)(d + o.r9);
    p.ro = r9; p.rl = r9 + 72 * n; p.rr = r9 + 144 * n; p.rs = r9 + 216 * n;
    u32* lv = (u32*)(d + o.lv);
    p.lo = lv; p.ll = lv + nv * 8 * n; p.lr = lv + 2 * nv * 8 * n; p.ls = lv + 3 * nv * 8 * n; p.v1 = lv + 4 * nv * 8 * n; p.cl0 = lv + 5 * nv * 8 * n;
    u32* nvv = (u32*)(d + o.nv);
    p.no = nvv; p.nl = nvv + nm * 8 * n; p.nr = nvv + 2 * nm * 8 * n; p.ns = nvv + 3 * nm * 8 * n;
    p.lamv = (u32*)(d + o.lam); p.muv = (u32*)(d + o.muv); p.coef = (u32*)(d + o.coef); p.misc = (u32*)(d + o.misc);
    p.msc = (u32*)(d + o.msc); p.pbuf = (u32*)(d + o.pb);
    p.wn_commit = d + o.wc; p.wn_c = d + o.wcv; p.wn_rho = d + o.rho; p.wn_mu = d + o.mu; p.wn_l = d + o.wlv; p.wn_n = d + o.wnv;
}
static int circuit_prove_launch(const bppp_ctx* c, const CircuitProveWs& p, hipStream_t s) {
    const unsigned blocks = blocks_of(p.N), fb_blocks = fb_blocks_of(p.N);
    HIP_TRY(hipMemsetAsync(p.msc, 0, 3 * (size_t)c->nbases * 8 * p.N * 4, s));     // the sets are written sparsely (slot = base index)
    k_cprove_stage_a<<<blocks, BPPP_BLOCK, 0, s>>>(p);
    for (int set = 0; set < 3; set++) k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, set, 0);
    k_cprove_stage_b<<<blocks, BPPP_BLOCK, 0, s>>>(p);
    k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, 0, 0);
    k_cprove_stage_c<<<blocks, BPPP_BLOCK, 0, s>>>(p);
    k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, 0, 1);
    k_cprove_stage_d<<<blocks, BPPP_BLOCK, 0, s>>>(p);
    return BPPP_OK;
}
// the WNLA stage behind it: the circuit stage's outputs in, its transcript continued
static int wnla_prove_fill_behind(bppp_ctx* c, WnlaProveWs& w, const WnlaProveShape& sh, uint8_t* d, const WnlaProveBufs& o, const CircuitProveWs& p) {
    const int rc = wnla_prove_fill(c, w, sh, d, o, p.wn_commit, p.wn_c, p.wn_rho, p.wn_mu, p.wn_l, p.wn_n, p.status, p.tstate, p.msc, p.pbuf);
    w.transcript_preloaded = 1;
    w.base = p.base; w.tio = p.tio; w.divergent_positions = p.divergent_positions;
    return rc;
}

// ---- the proofs of the circuit and reciprocal provers back to the caller: head (4 points) | r | x | [extra: one more point] | l | n per
//      instance out of the two stages' buffers, a flagged instance as zero bytes; then the transcripts, the draws wiped, the stream waited for
struct ProveReturn { uint8_t* proofs; int32_t* status; const HostTranscripts* tx; TxDev* txd; DrawWipe* wipe; };
static int prove_return_tail(const CircuitProveWs& p, const ProveReturn& r, hipStream_t s) {
    const int rc = r.txd->finish(r.tx, p.tio, p.base, p.tstate, p.N, p.status, s);
    if (rc != BPPP_OK) return rc;
    HIP_TRY(r.wipe->now());      // the draws cleared behind the last kernel that reads them
    HIP_TRY(hipStreamSynchronize(s));
    return BPPP_OK;
}
// the 33-byte form: assembled and compressed on the device into d_out (the wire buffer), one copy back
static int prove_return_sec1(const CircuitProveWs& p, const WnlaProveWs& w, const uint8_t* d_extra, uint8_t* d_out, const ProveReturn& r, hipStream_t s) {
    const size_t n = p.N, rounds = (size_t)w.rounds, nl_f = (size_t)w.nl_f, nn_f = (size_t)w.nn_f, wP = 4 + 2 * rounds + (d_extra ? 1 : 0);
    const size_t pb = wire_proof_bytes(wP, nl_f + nn_f);
    WireMap wm;
    wire_map_init(wm, n);
    wm.zero_if = p.status;
    wire_map_add(wm, false, p.proof_head, 256, d_out, pb, 4);
    wire_map_add(wm, false, w.proof_r, rounds * 64, d_out + 33 * 4, pb, rounds);
    wire_map_add(wm, false, w.proof_x, rounds * 64, d_out + 33 * (4 + rounds), pb, rounds);
    if (d_extra) wire_map_add(wm, false, d_extra, 64, d_out + 33 * (4 + 2 * rounds), pb, 1);
    wire_map_add(wm, true, w.proof_l, nl_f * 32, d_out + 33 * wP, pb, nl_f);
    wire_map_add(wm, true, w.proof_n, nn_f * 32, d_out + 33 * wP + 32 * nl_f, pb, nn_f);
    const int rc = wire_launch(wm, false, s);
    if (rc != BPPP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(r.proofs, d_out, n * pb, hipMemcpyDeviceToHost, s));
    if (r.status) HIP_TRY(hipMemcpyAsync(r.status, p.status, n * 4, hipMemcpyDeviceToHost, s));
    return prove_return_tail(p, r, s);
}
// the 64-byte form: assembled on the host side of the copy
static int prove_return_64(const CircuitProveWs& p, const WnlaProveWs& w, const uint8_t* d_extra, const ProveReturn& r, hipStream_t s) {
    const size_t n = p.N, b_rx = (size_t)w.rounds * 64, b_e = d_extra ? 64 : 0, b_l = (size_t)w.nl_f * 32, b_n = (size_t)w.nn_f * 32;
    const size_t proof_bytes = 256 + 2 * b_rx + b_e + b_l + b_n;
    std::vector<uint8_t> head(n * 256), pe(n * b_e), pr(n * b_rx), px(n * b_rx), pl(n * b_l), pn(n * b_n);
    std::vector<int32_t> st(n);
    HIP_TRY(hipMemcpyAsync(head.data(), p.proof_head, n * 256, hipMemcpyDeviceToHost, s));
    if (b_e) HIP_TRY(hipMemcpyAsync(pe.data(), d_extra, n * b_e, hipMemcpyDeviceToHost, s));
    if (b_rx) {
        HIP_TRY(hipMemcpyAsync(pr.data(), w.proof_r, n * b_rx, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(px.data(), w.proof_x, n * b_rx, hipMemcpyDeviceToHost, s));
    }
    if (b_l) HIP_TRY(hipMemcpyAsync(pl.data(), w.proof_l, n * b_l, hipMemcpyDeviceToHost, s));
    if (b_n) HIP_TRY(hipMemcpyAsync(pn.data(), w.proof_n, n * b_n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st.data(), p.status, n * 4, hipMemcpyDeviceToHost, s));
    const int rc = prove_return_tail(p, r, s);
    if (rc != BPPP_OK) return rc;
    for (size_t i = 0; i < n; i++) {
        uint8_t* o = r.proofs + i * proof_bytes;
        if (st[i] != 0) { std::memset(o, 0, proof_bytes); continue; }
        auto put = [&](const std::vector<uint8_t>& v, size_t bytes) { if (bytes) std::memcpy(o, v.data() + i * bytes, bytes); o += bytes; };
        put(head, 256); put(pr, b_rx); put(px, b_rx); put(pe, b_e); put(pl, b_l); put(pn, b_n);
    }
    if (r.status) std::memcpy(r.status, st.data(), n * 4);
    return BPPP_OK;
}

static int wnla_prove_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, const HostTranscripts* tx, size_t n, const uint8_t* commitments,
                           const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, const uint8_t* l, size_t nl, const uint8_t* nvec, size_t nn,
                           uint8_t* proof_r, uint8_t* proof_x, uint8_t* proof_l, uint8_t* proof_n, int32_t* status, bool sec1 = false) {
    // sec1 (bppp_wnla_prove_batch_sec1): commitments n x 33 in, proof_r / proof_x n x rounds x 33 out (SEC1, converted on the device)
    if (!c || !label_ok(label, label_len) || !commitments || !cvec || !rho || !mu || (!l && nl) || (!nvec && nn) || nl > 65536 || nn > 65536)
        return BPPP_ERR_INVALID_ARG;
    size_t rounds, nl_f, nn_f;
    wnla_proof_shape(nl, nn, rounds, nl_f, nn_f);
    if ((rounds && (!proof_r || !proof_x)) || (nl_f && !proof_l) || (nn_f && !proof_n)) return BPPP_ERR_INVALID_ARG;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t NB = (size_t)c->nbases, nh = (size_t)c->nh;
    const WnlaProveShape sh = {n, nl, nn, rounds, nl_f, nn_f};
    WnlaProveBufs o;
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes); };
    const size_t o_com = take(n * 64), o_c = take(n * nh * 32), o_rho = take(n * 32), o_mu = take(n * 32), o_l = take(n * nl * 32 + 16),
                 o_n = take(n * nn * 32 + 16);
    wnla_prove_take_proof(o, off, sh, 16);
    const size_t o_st = take(n * 4), o_ts = take(52 * n * 4);
    wnla_prove_take_state(o, off, c, sh, 0);
    const size_t o_msc = take(3 * NB * 8 * n * 4), o_pb = take(3 * 30 * n * 4);
    WnlaBlob blob;
    { const int rc_b = blob.take(c, off); if (rc_b != BPPP_OK) return rc_b; }
    uint8_t* d = blob.d;
    hipStream_t s = c->stream;
    const size_t o_wout = align16(n * 33), o_wout_x = o_wout + align16(n * rounds * 33);
    { const int rc_i = prover_points_in(c, sec1, commitments, d + o_com, n, 1, o_wout_x + n * rounds * 33 + 16, s); if (rc_i != BPPP_OK) return rc_i; }
    HIP_TRY(hipMemcpyAsync(d + o_c, cvec, n * nh * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_rho, rho, n * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_mu, mu, n * 32, hipMemcpyHostToDevice, s));
    if (nl) HIP_TRY(hipMemcpyAsync(d + o_l, l, n * nl * 32, hipMemcpyHostToDevice, s));
    if (nn) HIP_TRY(hipMemcpyAsync(d + o_n, nvec, n * nn * 32, hipMemcpyHostToDevice, s));
    WnlaProveWs w;
    int rc = wnla_prove_fill(c, w, sh, d, o, d + o_com, d + o_c, d + o_rho, d + o_mu, d + o_l, d + o_n, (int32_t*)(d + o_st), (u32*)(d + o_ts),
                             (u32*)(d + o_msc), (u32*)(d + o_pb));
    if (rc != BPPP_OK) return rc;
    { const int rc_ct = ct_setup(c, w.fb_ct, w.ct, n); if (rc_ct != BPPP_OK) return rc_ct; }      // l, n are the caller's secrets here (wnla.rs:152-160)
    t_new(w.base, label, (u32)label_len);
    TxDev txd;
    rc = txd.begin(c, tx, n, s, w.tio, w.divergent_positions);
    if (rc != BPPP_OK) return rc;
    w.tio.no_ops = rounds == 0;
    wnla_prove_launch(w, s);
    HIP_TRY(hipGetLastError());
    if (rounds && sec1) {
        WireMap wm;
        wire_map_init(wm, n);
        wire_map_add(wm, false, d + o.pr, rounds * 64, c->d_wire + o_wout, rounds * 33, rounds);
        wire_map_add(wm, false, d + o.px, rounds * 64, c->d_wire + o_wout_x, rounds * 33, rounds);
        rc = wire_launch(wm, false, s);
        if (rc != BPPP_OK) return rc;
        HIP_TRY(hipMemcpyAsync(proof_r, c->d_wire + o_wout, n * rounds * 33, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(proof_x, c->d_wire + o_wout_x, n * rounds * 33, hipMemcpyDeviceToHost, s));
    } else if (rounds) {
        HIP_TRY(hipMemcpyAsync(proof_r, d + o.pr, n * rounds * 64, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(proof_x, d + o.px, n * rounds * 64, hipMemcpyDeviceToHost, s));
    }
    if (nl_f) HIP_TRY(hipMemcpyAsync(proof_l, d + o.pl, n * nl_f * 32, hipMemcpyDeviceToHost, s));
    if (nn_f) HIP_TRY(hipMemcpyAsync(proof_n, d + o.pn, n * nn_f * 32, hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(hipMemcpyAsync(status, d + o_st, n * 4, hipMemcpyDeviceToHost, s));
    rc = txd.finish(tx, w.tio, w.base, w.tstate, n, w.status, s);
    if (rc != BPPP_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return BPPP_OK;
}
int bppp_wnla_prove_batch(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments, const uint8_t* cvec,
                          const uint8_t* rho, const uint8_t* mu, const uint8_t* l, size_t nl, const uint8_t* nvec, size_t nn,
                          uint8_t* proof_r, uint8_t* proof_x, uint8_t* proof_l, uint8_t* proof_n, int32_t* status) {
    CtxLock lock_(c);
    return wnla_prove_impl(c, label, label_len, nullptr, n, commitments, cvec, rho, mu, l, nl, nvec, nn, proof_r, proof_x, proof_l, proof_n, status);
}
int bppp_wnla_prove_batch_transcript(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, const uint8_t* commitments,
                                     const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, const uint8_t* l, size_t nl, const uint8_t* nvec,
                                     size_t nn, uint8_t* proof_r, uint8_t* proof_x, uint8_t* proof_l, uint8_t* proof_n, int32_t* status,
                                     uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    HostTranscripts tx = {states, n_states, states_out};
    return wnla_prove_impl(c, nullptr, 0, &tx, n, commitments, cvec, rho, mu, l, nl, nvec, nn, proof_r, proof_x, proof_l, proof_n, status);
}

// ArithmeticCircuit::prove (circuit.rs:260-556) for n instances of a shared circuit.
static int circuit_prove_impl(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, const HostTranscripts* tx, size_t n,
                              const uint8_t* v_commitments, const uint8_t* v, const uint8_t* s_v, const uint8_t* w_l, const uint8_t* w_r,
                              const uint8_t* w_o, const uint8_t* rnd, uint8_t* proofs, int32_t* status, bool sec1 = false,
                              const uint8_t* seed = nullptr, uint64_t stream_base = 0) {
    // sec1 (bppp_circuit_prove_batch_sec1): v_commitments n x k x 33 in, proofs in the 33-byte form out (converted on the device)
    if (!c || !q || !label_ok(label, label_len) || !v_commitments || !v || !s_v || !w_l || !w_r || (!rnd && !seed) || !proofs) return BPPP_ERR_INVALID_ARG;
    const CircuitDev& cd = q->cd;
    if ((cd.no && !w_o) || cd.nm > c->ng || cd.nv + 9 > c->nh) return BPPP_ERR_INVALID_ARG;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t NG = (size_t)c->ng, NH = (size_t)c->nh, k = (size_t)cd.k, nm = (size_t)cd.nm, nv = (size_t)cd.nv, no = (size_t)cd.no,
                 n_rnd = 18 + nv + nm;
    // seeded (bppp_*_prove_batch_seeded): the draws are made on the device below instead of uploaded
    if (seed && !draw_args_ok(seed, stream_base, n, n_rnd)) return BPPP_ERR_INVALID_ARG;
    WnlaProveShape sh = {n, NH, NG, 0, 0, 0};
    wnla_proof_shape(NH, NG, sh.rounds, sh.nl_f, sh.nn_f);
    const size_t proof_bytes = 64 * (4 + 2 * sh.rounds) + 32 * (sh.nl_f + sh.nn_f);
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes + 16); };
    const size_t o_vp = take(n * k * 64), o_v = take(n * k * nv * 32), o_sv = take(n * k * 32), o_wl = take(n * nm * 32), o_wr = take(n * nm * 32),
                 o_wo = take(n * no * 32), o_rnd = take(n * n_rnd * 32), o_head = take(n * 256), o_st = take(n * 4), o_ts = take(52 * n * 4);
    const CircuitProveBufs o_c = circuit_prove_take(off, c, n, nm, nv, (size_t)cd.nl);
    WnlaProveBufs o_w;
    wnla_prove_take_proof(o_w, off, sh, 16);
    wnla_prove_take_state(o_w, off, c, sh, 16);
    (void)take(n * proof_bytes);      // (unused room at the blob's end, kept: the blob's size decides which later call on the context reallocates)
    WnlaBlob blob;
    { const int rc_b = blob.take(c, off); if (rc_b != BPPP_OK) return rc_b; }
    uint8_t* d = blob.d;
    hipStream_t s = c->stream;
    const size_t o_wout = align16(n * k * 33);
    const size_t wire_bytes = o_wout + n * wire_proof_bytes(4 + 2 * sh.rounds, sh.nl_f + sh.nn_f) + 16;
    { const int rc_i = prover_points_in(c, sec1, v_commitments, d + o_vp, n, k, wire_bytes, s); if (rc_i != BPPP_OK) return rc_i; }
    HIP_TRY(hipMemcpyAsync(d + o_v, v, n * k * nv * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_sv, s_v, n * k * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_wl, w_l, n * nm * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_wr, w_r, n * nm * 32, hipMemcpyHostToDevice, s));
    if (no) HIP_TRY(hipMemcpyAsync(d + o_wo, w_o, n * no * 32, hipMemcpyHostToDevice, s));
    DrawWipe wipe = {seed ? d + o_rnd : nullptr, n * n_rnd * 32, s};
    if (seed) { const int rc_d = draw_enqueue(s, seed, stream_base, n, n_rnd, d + o_rnd); if (rc_d != BPPP_OK) return rc_d; }
    else HIP_TRY(hipMemcpyAsync(d + o_rnd, rnd, n * n_rnd * 32, hipMemcpyHostToDevice, s));
    CircuitProveWs p;
    std::memset(&p, 0, sizeof p);
    p.N = n; p.cd = cd; p.NG = c->ng; p.NH = c->nh; p.n_rnd = (int)n_rnd; p.rnd_stride = n_rnd * 32; p.part = q->d_part;
    p.v_pts = d + o_vp; p.v = d + o_v; p.s_v = d + o_sv; p.w_l = d + o_wl; p.w_r = d + o_wr; p.w_o = d + o_wo; p.rnd = d + o_rnd;
    p.proof_head = d + o_head; p.status = (int32_t*)(d + o_st); p.tstate = (u32*)(d + o_ts);
    circuit_prove_carve(p, d, o_c);
    p.fb = fb_table_of(c, n);
    { const int rc_ct = ct_setup(c, p.fb_ct, p.ct, n); if (rc_ct != BPPP_OK) return rc_ct; }      // c_l, c_r, c_o, c_s: witness and blindings (circuit.rs:336-345, 469-470)
    t_new(p.base, label, (u32)label_len);
    TxDev txd;
    int rc = txd.begin(c, tx, n, s, p.tio, p.divergent_positions);
    if (rc != BPPP_OK) return rc;
    WnlaProveWs w;
    rc = wnla_prove_fill_behind(c, w, sh, d, o_w, p);
    if (rc != BPPP_OK) return rc;
    rc = circuit_prove_launch(c, p, s);
    if (rc != BPPP_OK) return rc;
    wnla_prove_launch(w, s);
    HIP_TRY(hipGetLastError());
    const ProveReturn ret = {proofs, status, tx, &txd, &wipe};
    return sec1 ? prove_return_sec1(p, w, nullptr, c->d_wire + o_wout, ret, s) : prove_return_64(p, w, nullptr, ret, s);
}
int bppp_circuit_prove_batch(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n, const uint8_t* v_commitments,
                             const uint8_t* v, const uint8_t* s_v, const uint8_t* w_l, const uint8_t* w_r, const uint8_t* w_o,
                             const uint8_t* rnd, uint8_t* proofs, int32_t* status) {
    CtxLock lock_(c);
    return circuit_prove_impl(c, q, label, label_len, nullptr, n, v_commitments, v, s_v, w_l, w_r, w_o, rnd, proofs, status);
}
int bppp_circuit_prove_batch_transcript(bppp_ctx* c, const bppp_circuit* q, size_t n, const uint8_t* states, size_t n_states,
                                        const uint8_t* v_commitments, const uint8_t* v, const uint8_t* s_v, const uint8_t* w_l, const uint8_t* w_r,
                                        const uint8_t* w_o, const uint8_t* rnd, uint8_t* proofs, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    HostTranscripts tx = {states, n_states, states_out};
    return circuit_prove_impl(c, q, nullptr, 0, &tx, n, v_commitments, v, s_v, w_l, w_r, w_o, rnd, proofs, status);
}

// The reciprocal circuit's pattern for (dim_nd, dim_np) in device memory.  The first prove call of a shape on a context builds it on
// the host, allocates and uploads it (a synchronous copy: the host vectors live on this frame); every later call finds it here, so no
// prove call waits for its stream on account of the pattern, and the device-resident forms stay asynchronous.
static int recip_pattern_get(bppp_ctx* c, size_t nd, size_t np, RecipPatternDev& out) {
    for (const RecipPatternDev& rp : c->recip_patterns)
        if (rp.nd == nd && rp.np == np) { out = rp; return BPPP_OK; }
    RecipPattern P;
    recip_pattern_build(P, nd, np);
    const CircuitHostData& hd = P.hd;
    RecipPatternDev rp;
    std::memset(&rp, 0, sizeof rp);
    rp.nd = nd; rp.np = np; rp.nw = P.dims[5];
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes + 16); };
    rp.cpl = take(hd.cpl.size() * 4); rp.rl = take(hd.rl.size() * 4); rp.vl = take(hd.vl.size() * 4); rp.cpm = take(hd.cpm.size() * 4);
    rp.rm = take(hd.rm.size() * 4); rp.vm = take(hd.vm.size() * 4); rp.cmp = take(hd.colmap.size() * 4); rp.al = take(hd.al.size() * 4);
    rp.am = take(hd.am.size() * 4); rp.il = take(P.inst_l.size() * 4); rp.im = take(P.inst_m.size() * 4); rp.part = take(P.parts.size() * 4);
    std::vector<uint8_t> host(off, 0);
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) std::memcpy(host.data() + o, src, bytes); };
    put(rp.cpl, hd.cpl.data(), hd.cpl.size() * 4); put(rp.rl, hd.rl.data(), hd.rl.size() * 4); put(rp.vl, hd.vl.data(), hd.vl.size() * 4);
    put(rp.cpm, hd.cpm.data(), hd.cpm.size() * 4); put(rp.rm, hd.rm.data(), hd.rm.size() * 4); put(rp.vm, hd.vm.data(), hd.vm.size() * 4);
    put(rp.cmp, hd.colmap.data(), hd.colmap.size() * 4); put(rp.al, hd.al.data(), hd.al.size() * 4); put(rp.am, hd.am.data(), hd.am.size() * 4);
    put(rp.il, P.inst_l.data(), P.inst_l.size() * 4); put(rp.im, P.inst_m.data(), P.inst_m.size() * 4);
    put(rp.part, P.parts.data(), P.parts.size() * 4);
    HIP_TRY(ctx_malloc(c, (void**)&rp.d, off));
    const hipError_t e = hipMemcpy(rp.d, host.data(), off, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(rp.d); HIP_TRY(e); }
    c->recip_patterns.push_back(rp);
    out = rp;
    return BPPP_OK;
}

// The forms of the prover FROM INTEGERS (bppp_reciprocal_prove_values_batch*): digits, multiplicities and the value commitment are
// made on the device from x and s (recip_witness_core.h; recip_prove_core.h: RecipCommitWs), and the commitments go back to the caller.
// device: x, s, rnd, proofs, commitments_out and status are DEVICE memory, read and written in place, and the call is asynchronous on
// the context's stream.
// d_tx (the aggregate prover's k = 1 on the caller's transcripts, device buffers): the states where they are, in place of `tx`
struct RecipValues { bool device; uint8_t* commitments_out; const TranscriptIo* d_tx = nullptr; };

// ReciprocalRangeProofProtocol::prove (reciprocal.rs:110-146) for runtime dim_nd / dim_np: the inputs placed in the call's blob (uploaded;
// in the device-resident forms used where they are), then the launch chain, then the proofs back.
static int recip_prove_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, const HostTranscripts* tx, size_t n, size_t dim_nd, size_t dim_np,
                            const uint8_t* commitments, const uint8_t* x, const uint8_t* sblind, const uint8_t* digits, const uint8_t* m,
                            const uint8_t* rnd, uint8_t* proofs, int32_t* status, bool sec1 = false,
                            const uint8_t* seed = nullptr, uint64_t stream_base = 0, const RecipValues* values = nullptr) {
    // sec1 (bppp_reciprocal_prove_batch_sec1): commitments n x 33 in, proofs in the 33-byte form out (converted on the device)
    if (!c || !label_ok(label, label_len) || !x || !sblind || (!rnd && !seed) || !proofs) return BPPP_ERR_INVALID_ARG;
    if (values ? !values->commitments_out : (!commitments || !digits || !m)) return BPPP_ERR_INVALID_ARG;
    if (dim_nd == 0 || dim_np == 0 || dim_nd > (size_t)c->ng || dim_nd + 10 > (size_t)c->nh || dim_np > dim_nd + 1 || dim_nd > 4096)
        return BPPP_ERR_INVALID_ARG;
    // from integers: only the shapes whose digits x determines, dim_np^dim_nd <= n
    if (values && !recip_values_shape_ok(dim_nd, dim_np)) return BPPP_ERR_INVALID_ARG;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    const bool device_io = values && values->device;
    const size_t NG = (size_t)c->ng, NH = (size_t)c->nh, nd = dim_nd, np = dim_np, nm = nd, nv = nd + 1, nl = nv, n_rnd = 20 + 2 * nd;
    // seeded (bppp_*_prove_batch_seeded): the draws are made on the device below instead of uploaded
    if (seed && !draw_args_ok(seed, stream_base, n, n_rnd)) return BPPP_ERR_INVALID_ARG;
    RecipPatternDev pat;
    { const int rc_p = recip_pattern_get(c, nd, np, pat); if (rc_p != BPPP_OK) return rc_p; }
    WnlaProveShape sh = {n, NH, NG, 0, 0, 0};
    wnla_proof_shape(NH, NG, sh.rounds, sh.nl_f, sh.nn_f);
    const size_t proof_bytes = 64 * (5 + 2 * sh.rounds) + 32 * (sh.nl_f + sh.nn_f);
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes + 16); };
    // inputs (from integers: digits, m and the commitments are written here by the witness and commitment kernels)
    const size_t o_com = take(n * 64), o_x = take(n * 32), o_s = take(n * 32), o_dig = take(n * nd * 32), o_m = take(n * np * 32),
                 o_rnd = take(n * n_rnd * 32);
    // reciprocal stage
    const size_t o_st = take(n * 4), o_ts = take(52 * n * 4), o_inst = take((1 + np) * 8 * n * 4), o_scr = take((nd + np) * 8 * n * 4),
                 o_cpv = take(n * nv * 32), o_cpsv = take(n * 32), o_cpwr = take(n * nm * 32), o_cpvp = take(n * 64), o_prr = take(n * 64);
    // circuit prover, WNLA prover
    const size_t o_head = take(n * 256);
    const CircuitProveBufs o_c = circuit_prove_take(off, c, n, nm, nv, nl);
    WnlaProveBufs o_w;
    wnla_prove_take_proof(o_w, off, sh, 16);
    wnla_prove_take_state(o_w, off, c, sh, 16);
    // from integers: the witness kernel's status, and (host buffers) the proofs as they go back
    const size_t o_wst = values ? take(n * 4) : 0, o_pout = (values && !device_io) ? take(n * proof_bytes) : 0;
    WnlaBlob blob;
    if (device_io) { const int rc_b = ensure_blob(c, off); if (rc_b != BPPP_OK) return rc_b; }      // (no sync when the call returns)
    else { const int rc_b = blob.take(c, off); if (rc_b != BPPP_OK) return rc_b; }
    uint8_t* d = c->d_blob;
    hipStream_t s = c->stream;
    auto up = [&](size_t o, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(d + o, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess; };
    const size_t o_wout = align16(n * 33);
    const size_t wire_bytes = o_wout + n * wire_proof_bytes(5 + 2 * sh.rounds, sh.nl_f + sh.nn_f) + 16;
    if (!values) { const int rc_i = prover_points_in(c, sec1, commitments, d + o_com, n, 1, wire_bytes, s); if (rc_i != BPPP_OK) return rc_i; }
    if (!device_io) { HIP_TRY(up(o_x, x, n * 32)); HIP_TRY(up(o_s, sblind, n * 32)); }
    if (!values) { HIP_TRY(up(o_dig, digits, n * nd * 32)); HIP_TRY(up(o_m, m, n * np * 32)); }
    DrawWipe wipe = {seed ? d + o_rnd : nullptr, n * n_rnd * 32, s};
    if (seed) { const int rc_d = draw_enqueue(s, seed, stream_base, n, n_rnd, d + o_rnd); if (rc_d != BPPP_OK) return rc_d; }
    else if (!device_io) HIP_TRY(up(o_rnd, rnd, n * n_rnd * 32));
    RecipProveWs r;
    std::memset(&r, 0, sizeof r);
    r.N = n; r.nd = (int)nd; r.np = (int)np; r.NG = c->ng; r.NH = c->nh; r.n_rnd = (int)n_rnd;
    r.commitments = d + o_com; r.x = device_io ? x : d + o_x; r.s = device_io ? sblind : d + o_s; r.digits = d + o_dig; r.m = d + o_m;
    r.rnd = (device_io && !seed) ? rnd : d + o_rnd;
    r.status = (int32_t*)(d + o_st); r.tstate = (u32*)(d + o_ts); r.inst_vals = (u32*)(d + o_inst); r.scr = (u32*)(d + o_scr);
    r.msc = (u32*)(d + o_c.msc); r.pbuf = (u32*)(d + o_c.pb);      // (the circuit stage's: the two stages run one after the other)
    r.cp_v = d + o_cpv; r.cp_sv = d + o_cpsv; r.cp_wr = d + o_cpwr; r.cp_vpts = d + o_cpvp; r.proof_r = d + o_prr;
    r.fb = fb_table_of(c, n);
    { const int rc_ct = ct_setup(c, r.fb_ct, r.ct, n); if (rc_ct != BPPP_OK) return rc_ct; }      // the reciprocals 1 / (e + d_i) (reciprocal.rs:118)
    t_new(r.base, label, (u32)label_len);
    TxDev txd;
    int rc = txd.begin(c, tx, n, s, r.tio, r.divergent_positions);
    if (rc != BPPP_OK) return rc;
    if (values && values->d_tx) { r.tio = *values->d_tx; r.divergent_positions = r.tio.n_states != 1; }
    CircuitProveWs p;
    std::memset(&p, 0, sizeof p);
    p.base = r.base; p.tio = r.tio; p.divergent_positions = r.divergent_positions;
    CircuitDev& cd = p.cd;
    cd.nm = (int)nm; cd.no = (int)np; cd.k = 1; cd.nl = (int)nl; cd.nv = (int)nv; cd.nw = (int)pat.nw; cd.f_l = 1; cd.f_m = 0;
    cd.colptr_l = (const int*)(pat.d + pat.cpl); cd.rows_l = (const int*)(pat.d + pat.rl); cd.vals_l = (const u32*)(pat.d + pat.vl);
    cd.colptr_m = (const int*)(pat.d + pat.cpm); cd.rows_m = (const int*)(pat.d + pat.rm); cd.vals_m = (const u32*)(pat.d + pat.vm);
    cd.colmap = (const int*)(pat.d + pat.cmp); cd.a_l = (const u32*)(pat.d + pat.al); cd.a_m = (const u32*)(pat.d + pat.am);
    cd.inst_l = (const int*)(pat.d + pat.il); cd.inst_m = (const int*)(pat.d + pat.im); cd.inst_vals = r.inst_vals;
    p.N = n; p.NG = c->ng; p.NH = c->nh; p.n_rnd = (int)(18 + nv + nm); p.rnd_stride = n_rnd * 32; p.part = (const int*)(pat.d + pat.part);
    p.transcript_preloaded = 1;
    p.v_pts = r.cp_vpts; p.v = r.cp_v; p.s_v = r.cp_sv; p.w_l = r.digits; p.w_r = r.cp_wr; p.w_o = r.m; p.rnd = r.rnd + 32;
    p.proof_head = d + o_head; p.status = r.status; p.tstate = r.tstate;
    circuit_prove_carve(p, d, o_c);
    p.fb = r.fb; p.fb_ct = r.fb_ct; p.ct = r.ct;
    WnlaProveWs w;
    rc = wnla_prove_fill_behind(c, w, sh, d, o_w, p);
    if (rc != BPPP_OK) return rc;
    const unsigned blocks = blocks_of(n);
    if (values) {
        // the witness and the value commitment: x alone in, what stage r1 reads out (x and s are secrets: the "ct_prover" table as below)
        RecipWitnessWs ww;
        std::memset(&ww, 0, sizeof ww);
        recip_witness_shape(ww, nd, np);
        ww.N = n; ww.x = r.x; ww.digits = d + o_dig; ww.m = d + o_m; ww.status = (int32_t*)(d + o_wst);
        RecipCommitWs cw;
        std::memset(&cw, 0, sizeof cw);
        cw.N = n; cw.NG = c->ng; cw.x = r.x; cw.s = r.s; cw.status = ww.status; cw.msc = r.msc; cw.pbuf = r.pbuf; cw.out = d + o_com;
        cw.fb = r.fb; cw.fb_ct = r.fb_ct; cw.ct = r.ct;
        GLAUNCH(s, K_RPROVE_WITNESS, k_rprove_witness<<<blocks, BPPP_BLOCK, 0, s>>>(ww, cw));
        GLAUNCH(s, K_RPROVE_COMMIT, {
            k_rprove_commit<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(cw);
            k_rprove_commit_store<<<blocks, BPPP_BLOCK, 0, s>>>(cw);
        });
        r.witness_status = ww.status;
    }
    HIP_TRY(hipMemsetAsync(r.msc, 0, 3 * (size_t)c->nbases * 8 * n * 4, s));
    int rc_l = BPPP_OK;
    GLAUNCH(s, K_RPROVE_CHAIN, {
        k_rprove_stage_r1<<<blocks, BPPP_BLOCK, 0, s>>>(r);
        k_rprove_msm<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, s>>>(r);
        k_rprove_stage_r2<<<blocks, BPPP_BLOCK, 0, s>>>(r);
        rc_l = circuit_prove_launch(c, p, s);
        if (rc_l == BPPP_OK) wnla_prove_launch(w, s);
    });
    if (rc_l != BPPP_OK) return rc_l;
    HIP_TRY(hipGetLastError());
    if (values) {
        // the proofs put together on the device (a flagged instance as zero bytes): into the caller's buffer, or the blob and one copy back
        ProofAssembleWs a;
        std::memset(&a, 0, sizeof a);
        a.N = n; a.proof_bytes = proof_bytes; a.nseg = 6; a.status = p.status; a.out = device_io ? proofs : d + o_pout;
        a.src[0] = p.proof_head; a.bytes[0] = 256;
        a.src[1] = w.proof_r; a.bytes[1] = (u32)(sh.rounds * 64);
        a.src[2] = w.proof_x; a.bytes[2] = (u32)(sh.rounds * 64);
        a.src[3] = r.proof_r; a.bytes[3] = 64;
        a.src[4] = w.proof_l; a.bytes[4] = (u32)(sh.nl_f * 32);
        a.src[5] = w.proof_n; a.bytes[5] = (u32)(sh.nn_f * 32);
        const size_t words = n * (proof_bytes / 4);
        if ((words + 255) / 256 > 0xFFFFFFFFu) return BPPP_ERR_INVALID_ARG;
        k_gprove_assemble<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
        const hipMemcpyKind back = device_io ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (sec1 && !device_io) {
            // the aggregate's k = 1 wire form: the assembled proofs and the commitments compressed into the wire buffer, copied back from there
            const size_t wP = 5 + 2 * sh.rounds, wS = sh.nl_f + sh.nn_f, wire_pb = wire_proof_bytes(wP, wS), o_wc = align16(n * wire_pb);
            const int rc_w = ensure_buffer(c, c->d_wire, c->wire_bytes, o_wc + n * 33);
            if (rc_w != BPPP_OK) return rc_w;
            WireMap wm;
            wire_map_init(wm, n);
            wire_map_add(wm, false, d + o_pout, proof_bytes, c->d_wire, wire_pb, wP);
            wire_map_add(wm, true, d + o_pout + 64 * wP, proof_bytes, c->d_wire + 33 * wP, wire_pb, wS);
            wire_map_add(wm, false, d + o_com, 64, c->d_wire + o_wc, 33, 1);
            rc = wire_launch(wm, false, s);
            if (rc != BPPP_OK) return rc;
            HIP_TRY(hipMemcpyAsync(proofs, c->d_wire, n * wire_pb, back, s));
            HIP_TRY(hipMemcpyAsync(values->commitments_out, c->d_wire + o_wc, n * 33, back, s));
        } else {
            if (!device_io) HIP_TRY(hipMemcpyAsync(proofs, d + o_pout, n * proof_bytes, back, s));
            if (values->d_tx) {
                // device states can be invalid, which stage r1 finds behind the commitment kernels: the commitments through the
                // assembly kernel too, so that such an instance's is zeroed with its proof (as agg_prove_part's)
                ProofAssembleWs ac;
                std::memset(&ac, 0, sizeof ac);
                ac.N = n; ac.proof_bytes = 64; ac.nseg = 1; ac.status = p.status; ac.out = values->commitments_out;
                ac.src[0] = d + o_com; ac.bytes[0] = 64;
                k_gprove_assemble<<<(unsigned)((n * 16 + 255) / 256), 256, 0, s>>>(ac);
                HIP_TRY(hipGetLastError());
            } else HIP_TRY(hipMemcpyAsync(values->commitments_out, d + o_com, n * 64, back, s));
        }
        if (status) HIP_TRY(hipMemcpyAsync(status, p.status, n * 4, back, s));
        // the caller's transcripts (the aggregate's k = 1): a zeroed instance gets its input state back
        if (values->d_tx && p.tio.states_out) {
            k_aprove_export_states<<<blocks, BPPP_BLOCK, 0, s>>>(p.tio, p.base, p.tstate, n, p.status);
            HIP_TRY(hipGetLastError());
        } else {
            rc = txd.finish(tx, p.tio, p.base, p.tstate, n, p.status, s, true);
            if (rc != BPPP_OK) return rc;
        }
        HIP_TRY(wipe.now());      // the draws cleared behind the last kernel that reads them
        if (!device_io) HIP_TRY(hipStreamSynchronize(s));
        return BPPP_OK;
    }
    const ProveReturn ret = {proofs, status, tx, &txd, &wipe};
    return sec1 ? prove_return_sec1(p, w, r.proof_r, c->d_wire + o_wout, ret, s) : prove_return_64(p, w, r.proof_r, ret, s);
}
int bppp_reciprocal_prove_batch(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                const uint8_t* commitments, const uint8_t* x, const uint8_t* sblind, const uint8_t* digits, const uint8_t* m,
                                const uint8_t* rnd, uint8_t* proofs, int32_t* status) {
    CtxLock lock_(c);
    return recip_prove_impl(c, label, label_len, nullptr, n, dim_nd, dim_np, commitments, x, sblind, digits, m, rnd, proofs, status);
}
int bppp_reciprocal_prove_batch_transcript(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, size_t dim_nd, size_t dim_np,
                                           const uint8_t* commitments, const uint8_t* x, const uint8_t* sblind, const uint8_t* digits,
                                           const uint8_t* m, const uint8_t* rnd, uint8_t* proofs, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    HostTranscripts tx = {states, n_states, states_out};
    return recip_prove_impl(c, nullptr, 0, &tx, n, dim_nd, dim_np, commitments, x, sblind, digits, m, rnd, proofs, status);
}


// ---------------------------------------------------------------- the wire form of the generic proofs (SEC1, the crate's serialised types)
// reciprocal::SerializableProof, circuit::SerializableProof, wnla::SerializableProof (reciprocal.rs:37-41, circuit.rs:36-46, wnla.rs:33-38):
// the C-ABI layouts above with every point 33-byte SEC1-compressed in place and the scalars as they are.  The verifiers expand the
// inputs on the device (k_wire_expand, one lane per point) into the context's wire buffer and run the 64-byte path on it; an undecodable
// point becomes the off-curve (1, 0), which phase 1 flags BPPP_ST_BAD_ENCODING -- the status the 64-byte form gets for that point.  The
// provers decompress their input commitments the same way and compress their proofs on the device (k_wire_compress) before the copy
// back.  The host-buffer forms stage the 33-byte bytes in the same buffer, in front of the expanded form.
// ---- reciprocal
// arguments checked; d_exp: recip_wire_exp().bytes() in the wire buffer
static int recip_sec1_run(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np, const uint8_t* d_com33,
                          const uint8_t* d_proofs33, size_t rounds, size_t nl, size_t nn, void* d_accept, void* d_status, uint8_t* d_exp,
                          const uint8_t* rlc_seed, void* d_reject_count = nullptr) {
    const WireExp e = recip_wire_exp(n, rounds, nl, nn);
    // on c->stream: a call split into parts forks them from c->stream behind this (ev_twin_fork in recip_verify_device_entry)
    const int rc = e.launch(d_com33, d_proofs33, d_exp, c->stream);
    if (rc != BPPP_OK) return rc;
    return recip_verify_device_entry(c, label, label_len, n, dim_nd, dim_np, d_exp, d_exp + e.o_proofs(), rounds, nl, nn, d_accept, d_status,
                                     rlc_seed, d_reject_count);
}
// rlc_seed (the *_rlc_sec1 entry points of all three verifiers): the expansion is the same launch; what runs behind it is the 64-byte
// RLC twin's pipeline on the expanded bytes, so a flagged instance is kept out of the weighted sums exactly as there
// d_reject_count (the aggregate's k = 1 forward only): the number of rejected instances, as recip_verify_device_entry's
static int recip_sec1_device_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                  const void* d_commitments33, const void* d_proofs33, size_t rounds, size_t nl, size_t nn,
                                  void* d_accept, void* d_status, const uint8_t* rlc_seed, void* d_reject_count = nullptr) {
    if (!c || !label_ok(label, label_len) || !d_commitments33 || !d_proofs33 || !d_accept || !d_status) return BPPP_ERR_INVALID_ARG;
    int rc = recip_verify_check_args(c, dim_nd, dim_np, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (n == 0) {      // (nothing to verify at either shape; the counter, where one is given, reads zero as after any other call)
        if (!d_reject_count) return BPPP_OK;
        HIP_TRY(hipSetDevice(c->device));
        return reset_reject_count(c, d_reject_count);
    }
    if (recip_is_u64_shape(c, dim_nd, dim_np, rounds, nl, nn))      // the u64 wire form is the same 33 + 525 bytes: its own expand kernel
        return verify_sec1_device_impl(c, label, label_len, n, d_commitments33, d_proofs33, d_accept, d_status, nullptr, d_reject_count, rlc_seed);
    HIP_TRY(hipSetDevice(c->device));
    rc = ensure_buffer(c, c->d_wire, c->wire_bytes, recip_wire_exp(n, rounds, nl, nn).bytes());
    if (rc != BPPP_OK) return rc;
    return recip_sec1_run(c, label, label_len, n, dim_nd, dim_np, (const uint8_t*)d_commitments33, (const uint8_t*)d_proofs33, rounds, nl, nn,
                          d_accept, d_status, c->d_wire, rlc_seed, d_reject_count);
}
int bppp_reciprocal_verify_batch_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                             const void* d_commitments33, const void* d_proofs33, size_t rounds, size_t nl, size_t nn,
                                             void* d_accept, void* d_status) {
    CtxLock lock_(c);
    return recip_sec1_device_impl(c, label, label_len, n, dim_nd, dim_np, d_commitments33, d_proofs33, rounds, nl, nn, d_accept, d_status, nullptr);
}
int bppp_reciprocal_verify_batch_rlc_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                                 const void* d_commitments33, const void* d_proofs33, size_t rounds, size_t nl, size_t nn,
                                                 void* d_accept, void* d_status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return recip_sec1_device_impl(c, label, label_len, n, dim_nd, dim_np, d_commitments33, d_proofs33, rounds, nl, nn, d_accept, d_status, seed);
}
static int recip_sec1_host_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                int32_t* status, const uint8_t* rlc_seed) {
    if (!c || !label_ok(label, label_len) || !commitments33 || !proofs33 || !accept) return BPPP_ERR_INVALID_ARG;
    int rc = recip_verify_check_args(c, dim_nd, dim_np, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (n == 0) return BPPP_OK;
    if (recip_is_u64_shape(c, dim_nd, dim_np, rounds, nl, nn))
        return rlc_seed ? bppp_u64_verify_batch_rlc_sec1(c, label, label_len, n, commitments33, proofs33, accept, status, rlc_seed)
                        : bppp_u64_verify_batch_sec1(c, label, label_len, n, commitments33, proofs33, accept, status);
    HIP_TRY(hipSetDevice(c->device));
    const WireExp e = recip_wire_exp(n, rounds, nl, nn);
    HostStage hs;
    rc = hs.begin(c, true, {{commitments33, e.com33_bytes()}, {proofs33, e.proofs33_bytes()}}, n, nullptr, e.bytes());
    if (rc != BPPP_OK) return rc;
    rc = recip_sec1_run(c, label, label_len, n, dim_nd, dim_np, hs.in[0], hs.in[1], rounds, nl, nn, hs.accept, hs.status, hs.tail, rlc_seed);
    return hs.finish(rc, n, accept, status, nullptr);
}
int bppp_reciprocal_verify_batch_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                      const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                      int32_t* status) {
    CtxLock lock_(c);
    return recip_sec1_host_impl(c, label, label_len, n, dim_nd, dim_np, commitments33, proofs33, rounds, nl, nn, accept, status, nullptr);
}
int bppp_reciprocal_verify_batch_rlc_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                          const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn,
                                          uint8_t* accept, int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return recip_sec1_host_impl(c, label, label_len, n, dim_nd, dim_np, commitments33, proofs33, rounds, nl, nn, accept, status, seed);
}
// the single-proof front end's batched call over wire rows (bppp_coalesce.hip: bppp_reciprocal_verify_one_sec1): the callers' transcripts
// in (1 or n), each instance's advanced transcript out -- bppp_reciprocal_verify_batch_transcript over the wire form.  Staging and the
// expanded inputs in the wire buffer, the workspace in the device entry points' grow-only buffer: no allocation once a front end is warm
int recip_verify_sec1_transcript_host(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, size_t dim_nd, size_t dim_np,
                                      const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn,
                                      uint8_t* accept, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!c || !states || !commitments33 || !proofs33 || !accept) return BPPP_ERR_INVALID_ARG;
    int rc = recip_verify_check_args(c, dim_nd, dim_np, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (n == 0) return BPPP_OK;
    const HostTranscripts tx = {states, n_states, states_out};
    rc = check_host_transcripts(&tx, n);
    if (rc != BPPP_OK) return rc;
    if (recip_is_u64_shape(c, dim_nd, dim_np, rounds, nl, nn))
        return verify_sec1_transcript_host(c, n, states, n_states, commitments33, proofs33, accept, status, states_out);
    HIP_TRY(hipSetDevice(c->device));
    rc = ensure_straus_capacity(c, n);
    if (rc != BPPP_OK) return rc;
    const WireExp e = recip_wire_exp(n, rounds, nl, nn);
    HostStage hs;
    rc = hs.begin(c, true, {{commitments33, e.com33_bytes()}, {proofs33, e.proofs33_bytes()}}, n, &tx, e.bytes(),
                  recip_verify_ws_bytes(c, n, dim_nd, dim_np, rounds, false));
    if (rc != BPPP_OK) return rc;
    rc = e.launch(hs.in[0], hs.in[1], hs.tail, c->stream);
    if (rc != BPPP_OK) return rc;
    rc = recip_verify_device_impl(c, nullptr, 0, n, dim_nd, dim_np, hs.tail, hs.tail + e.o_proofs(), rounds, nl, nn, hs.accept, hs.status,
                                  c->d_gws, hs.dtio, nullptr);
    return hs.finish(rc, n, accept, status, &tx);
}

// ---- aggregate: n x k commitments and the proof c_l c_r c_o c_s | r | x | R_0 .. R_{k-1} | l | n, 4 + 2 rounds + k points in front of
//      the scalars.  One expansion over the whole call on the context's stream, in front of the max_batch parts; k = 1 is the
//      reciprocal wire form and goes to its entry points.
//      Aggregates of MIXED value counts (d_ks / ks given): 33-byte slots laid out by k_max, instance i in the uniform wire layout for
//      ks[i] in front of its slots, expanded by k_wire_expand_mixed (wire_mixed_core.h); the mixed chain then runs on the expanded
//      slots.  Nothing is forwarded: k_max = 1 runs here too
// arguments checked; d_exp: agg_wire_exp(n, k).bytes() in the wire buffer
static int agg_sec1_run(bppp_ctx* c, const AggCall& a, size_t n, const uint8_t* d_ks, const uint8_t* d_com33, const uint8_t* d_proofs33,
                        void* d_accept, void* d_status, void* d_reject_count, uint8_t* d_exp, const TranscriptIo* dtio = nullptr) {
    const WireExp e = agg_wire_exp(n, a.k, a.rounds, a.nl, a.nn);
    if (a.mixed) {
        WireMixed m;
        m.com33 = d_com33; m.proofs33 = d_proofs33; m.com64 = d_exp; m.proofs64 = d_exp + e.o_proofs(); m.ks = d_ks;
        m.n = n; m.k_max = (u32)a.k; m.rounds = (u32)a.rounds; m.ns = (u32)(a.nl + a.nn);
        k_wire_expand_mixed<<<(unsigned)((wire_mixed_lanes(m) + 255) / 256), 256, 0, c->stream>>>(m);
        HIP_TRY(hipGetLastError());
    } else {
        const int rc = e.launch(d_com33, d_proofs33, d_exp, c->stream);
        if (rc != BPPP_OK) return rc;
    }
    return agg_verify_device_run(c, a, n, d_ks, d_exp, d_exp + e.o_proofs(), d_accept, d_status, d_reject_count, dtio);
}
// device buffers.  "last_rlc_*" are reset here, in front of agg_verify_prepare's own reset: the wire buffer's growth comes first and can
// fail, and such a call reports (0, 0) too
static int agg_sec1_device_entry(bppp_ctx* c, const AggCall& a, size_t n, const void* d_ks, const void* d_commitments33, const void* d_proofs33,
                                 void* d_accept, void* d_status, void* d_reject_count) {
    int rc = agg_call_check(c, a, d_commitments33 && d_proofs33 && d_accept && d_status, n, d_ks, 1);
    if (rc != BPPP_OK) return rc;
    if (!a.mixed && a.k == 1)
        return recip_sec1_device_impl(c, a.label, a.label_len, n, a.dim_nd, a.dim_np, d_commitments33, d_proofs33, a.rounds, a.nl, a.nn, d_accept,
                                      d_status, a.rlc_seed, d_reject_count);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) return reset_reject_count(c, d_reject_count);
    rlc_report_reset(c, a.rlc_seed);
    rc = ensure_buffer(c, c->d_wire, c->wire_bytes, agg_wire_exp(n, a.k, a.rounds, a.nl, a.nn).bytes());
    if (rc != BPPP_OK) return rc;
    return agg_sec1_run(c, a, n, (const uint8_t*)d_ks, (const uint8_t*)d_commitments33, (const uint8_t*)d_proofs33, d_accept, d_status,
                        d_reject_count, c->d_wire);
}
int bppp_reciprocal_agg_verify_batch_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                 size_t dim_np, const void* d_commitments33, const void* d_proofs33, size_t rounds, size_t nl,
                                                 size_t nn, void* d_accept, void* d_status, void* d_reject_count) {
    CtxLock lock_(c);
    return agg_sec1_device_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, nullptr, d_commitments33, d_proofs33,
                                 d_accept, d_status, d_reject_count);
}
int bppp_reciprocal_agg_verify_batch_rlc_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                     size_t dim_np, const void* d_commitments33, const void* d_proofs33, size_t rounds,
                                                     size_t nl, size_t nn, void* d_accept, void* d_status, void* d_reject_count,
                                                     const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_sec1_device_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, seed}, n, nullptr, d_commitments33, d_proofs33,
                                 d_accept, d_status, d_reject_count);
}
int bppp_reciprocal_agg_verify_batch_mixed_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max,
                                                       const void* d_ks, size_t dim_nd, size_t dim_np, const void* d_commitments33,
                                                       const void* d_proofs33, size_t rounds, size_t nl, size_t nn, void* d_accept,
                                                       void* d_status, void* d_reject_count) {
    CtxLock lock_(c);
    return agg_sec1_device_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, d_ks, d_commitments33, d_proofs33,
                                 d_accept, d_status, d_reject_count);
}
int bppp_reciprocal_agg_verify_batch_mixed_rlc_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max,
                                                           const void* d_ks, size_t dim_nd, size_t dim_np, const void* d_commitments33,
                                                           const void* d_proofs33, size_t rounds, size_t nl, size_t nn, void* d_accept,
                                                           void* d_status, void* d_reject_count, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_sec1_device_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, seed}, n, d_ks, d_commitments33, d_proofs33,
                                 d_accept, d_status, d_reject_count);
}
// host buffers: the 33-byte input (ks too, of a mixed call, whose whole slots go up: the expansion reads an instance's first k_i
// commitments and S(k_i) bytes only) staged in the wire buffer, in front of accept, status, the states and the expanded form
// tx (the _transcript_sec1 form, uniform calls only): as agg_verify_host_entry's
static int agg_sec1_host_entry(bppp_ctx* c, const AggCall& a, size_t n, const uint8_t* ks, const uint8_t* commitments33, const uint8_t* proofs33,
                               uint8_t* accept, int32_t* status, const HostTranscripts* tx = nullptr) {
    int rc = agg_call_check(c, a, commitments33 && proofs33 && accept, n, ks, 0);
    if (rc != BPPP_OK) return rc;
    if (tx && (!tx->states || (tx->n_states != 1 && tx->n_states != n))) return BPPP_ERR_INVALID_ARG;
    if (!a.mixed && a.k == 1) {
        if (tx)
            return recip_verify_sec1_transcript_host(c, n, tx->states, tx->n_states, a.dim_nd, a.dim_np, commitments33, proofs33, a.rounds, a.nl, a.nn,
                                                     accept, status, tx->states_out);
        return recip_sec1_host_impl(c, a.label, a.label_len, n, a.dim_nd, a.dim_np, commitments33, proofs33, a.rounds, a.nl, a.nn, accept, status,
                                    a.rlc_seed);
    }
    if (n == 0) return BPPP_OK;
    rc = check_host_transcripts(tx, n);
    if (rc != BPPP_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rlc_report_reset(c, a.rlc_seed);      // (as agg_sec1_device_entry's)
    const WireExp e = agg_wire_exp(n, a.k, a.rounds, a.nl, a.nn);
    HostStage hs;
    rc = hs.begin(c, true, {{commitments33, e.com33_bytes()}, {proofs33, e.proofs33_bytes()}, {ks, a.mixed ? n : 0}}, n, tx, e.bytes());
    if (rc != BPPP_OK) return rc;
    rc = agg_sec1_run(c, a, n, a.mixed ? hs.in[2] : nullptr, hs.in[0], hs.in[1], hs.accept, hs.status, nullptr, hs.tail, hs.dtio);
    return hs.finish(rc, n, accept, status, tx);
}
size_t bppp_reciprocal_agg_proof_sec1_bytes(size_t k, size_t rounds, size_t nl, size_t nn) { return wire_proof_bytes(4 + 2 * rounds + k, nl + nn); }
int bppp_reciprocal_agg_verify_batch_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd, size_t dim_np,
                                          const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn,
                                          uint8_t* accept, int32_t* status) {
    CtxLock lock_(c);
    return agg_sec1_host_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, nullptr, commitments33, proofs33,
                               accept, status);
}
// the wire form on the caller's transcripts (host buffers): the expansion in front is the label form's
int bppp_reciprocal_agg_verify_batch_transcript_sec1(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, size_t k, size_t dim_nd,
                                                     size_t dim_np, const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds,
                                                     size_t nl, size_t nn, uint8_t* accept, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!states) return BPPP_ERR_INVALID_ARG;
    const HostTranscripts tx = {states, n_states, states_out};
    return agg_sec1_host_entry(c, {nullptr, 0, k, false, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, nullptr, commitments33, proofs33,
                               accept, status, &tx);
}
int bppp_reciprocal_agg_verify_batch_rlc_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                              size_t dim_np, const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl,
                                              size_t nn, uint8_t* accept, int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_sec1_host_entry(c, {label, label_len, k, false, dim_nd, dim_np, rounds, nl, nn, seed}, n, nullptr, commitments33, proofs33,
                               accept, status);
}
int bppp_reciprocal_agg_verify_batch_mixed_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max, const uint8_t* ks,
                                                size_t dim_nd, size_t dim_np, const uint8_t* commitments33, const uint8_t* proofs33,
                                                size_t rounds, size_t nl, size_t nn, uint8_t* accept, int32_t* status) {
    CtxLock lock_(c);
    return agg_sec1_host_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, nullptr}, n, ks, commitments33, proofs33,
                               accept, status);
}
int bppp_reciprocal_agg_verify_batch_mixed_rlc_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max,
                                                    const uint8_t* ks, size_t dim_nd, size_t dim_np, const uint8_t* commitments33,
                                                    const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                                    int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_sec1_host_entry(c, {label, label_len, k_max, true, dim_nd, dim_np, rounds, nl, nn, seed}, n, ks, commitments33, proofs33,
                               accept, status);
}

// ---- circuit
// arguments checked; d_exp: circuit_wire_exp().bytes() in the wire buffer
static int circuit_sec1_run(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n, const uint8_t* d_com33,
                            const uint8_t* d_proofs33, size_t rounds, size_t nl, size_t nn, uint8_t* d_accept, int32_t* d_status, uint8_t* d_exp,
                            const uint8_t* rlc_seed) {
    const WireExp e = circuit_wire_exp(n, (size_t)q->cd.k, rounds, nl, nn);
    const int rc = e.launch(d_com33, d_proofs33, d_exp, c->stream);
    if (rc != BPPP_OK) return rc;
    return circuit_verify_host_impl(c, q, label, label_len, n, d_exp, d_exp + e.o_proofs(), rounds, nl, nn, d_accept, d_status, nullptr, true,
                                    rlc_seed);
}
static int circuit_sec1_device_impl(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                    const void* d_commitments33, const void* d_proofs33, size_t rounds, size_t nl, size_t nn,
                                    void* d_accept, void* d_status, const uint8_t* rlc_seed) {
    int rc = circuit_verify_check(c, q, label, label_len, d_commitments33, d_proofs33, d_accept, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    rc = ensure_buffer(c, c->d_wire, c->wire_bytes, circuit_wire_exp(n, (size_t)q->cd.k, rounds, nl, nn).bytes());
    if (rc != BPPP_OK) return rc;
    return circuit_sec1_run(c, q, label, label_len, n, (const uint8_t*)d_commitments33, (const uint8_t*)d_proofs33, rounds, nl, nn,
                            (uint8_t*)d_accept, (int32_t*)d_status, c->d_wire, rlc_seed);
}
int bppp_circuit_verify_batch_sec1_device(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                          const void* d_commitments33, const void* d_proofs33, size_t rounds, size_t nl, size_t nn,
                                          void* d_accept, void* d_status) {
    CtxLock lock_(c);
    return circuit_sec1_device_impl(c, q, label, label_len, n, d_commitments33, d_proofs33, rounds, nl, nn, d_accept, d_status, nullptr);
}
int bppp_circuit_verify_batch_rlc_sec1_device(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                              const void* d_commitments33, const void* d_proofs33, size_t rounds, size_t nl, size_t nn,
                                              void* d_accept, void* d_status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return circuit_sec1_device_impl(c, q, label, label_len, n, d_commitments33, d_proofs33, rounds, nl, nn, d_accept, d_status, seed);
}
static int circuit_sec1_host_impl(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                  const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                  int32_t* status, const uint8_t* rlc_seed) {
    int rc = circuit_verify_check(c, q, label, label_len, commitments33, proofs33, accept, rounds, nl, nn);
    if (rc != BPPP_OK) return rc;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    const WireExp e = circuit_wire_exp(n, (size_t)q->cd.k, rounds, nl, nn);
    HostStage hs;
    rc = hs.begin(c, true, {{commitments33, e.com33_bytes()}, {proofs33, e.proofs33_bytes()}}, n, nullptr, e.bytes());
    if (rc != BPPP_OK) return rc;
    rc = circuit_sec1_run(c, q, label, label_len, n, hs.in[0], hs.in[1], rounds, nl, nn, hs.accept, hs.status, hs.tail, rlc_seed);
    return hs.finish(rc, n, accept, status, nullptr);
}
int bppp_circuit_verify_batch_sec1(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                   const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn, uint8_t* accept,
                                   int32_t* status) {
    CtxLock lock_(c);
    return circuit_sec1_host_impl(c, q, label, label_len, n, commitments33, proofs33, rounds, nl, nn, accept, status, nullptr);
}
int bppp_circuit_verify_batch_rlc_sec1(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                       const uint8_t* commitments33, const uint8_t* proofs33, size_t rounds, size_t nl, size_t nn,
                                       uint8_t* accept, int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return circuit_sec1_host_impl(c, q, label, label_len, n, commitments33, proofs33, rounds, nl, nn, accept, status, seed);
}

// ---- WeightNormLinearArgument (the commitment and proof.r / proof.x are points; proof.l / proof.n scalars, taken as they are)
// arguments checked; d_exp: WnlaWireExp::bytes() in the wire buffer
static int wnla_sec1_run(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* d_com33, const uint8_t* d_c,
                         const uint8_t* d_rho, const uint8_t* d_mu, size_t rounds, const uint8_t* d_r33, const uint8_t* d_x33, const uint8_t* d_l,
                         size_t nl, const uint8_t* d_n, size_t nn, uint8_t* d_accept, int32_t* d_status, uint8_t* d_exp,
                         const uint8_t* rlc_seed) {
    const WnlaWireExp e = {n, rounds};
    const int rc = e.launch(d_com33, d_r33, d_x33, d_exp, c->stream);
    if (rc != BPPP_OK) return rc;
    return wnla_run(c, false, label, label_len, n, d_exp, d_c, d_rho, d_mu, rounds, d_exp + e.o_r(), d_exp + e.o_x(), d_l, nl, d_n, nn, nullptr,
                    d_accept, d_status, nullptr, true, rlc_seed);
}
static int wnla_sec1_device_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const void* d_commitments33,
                                 const void* d_c, const void* d_rho, const void* d_mu, size_t rounds, const void* d_proof_r33,
                                 const void* d_proof_x33, const void* d_proof_l, size_t nl, const void* d_proof_n, size_t nn,
                                 void* d_accept, void* d_status, const uint8_t* rlc_seed) {
    int rc = wnla_verify_check(c, label, label_len, d_commitments33, d_c, d_rho, d_mu, rounds, d_proof_r33, d_proof_x33, d_proof_l, nl, d_proof_n,
                               nn, d_accept);
    if (rc != BPPP_OK) return rc;
    if (!wnla_shape_ok(rounds, nl, nn)) return BPPP_ERR_INVALID_ARG;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    rc = ensure_buffer(c, c->d_wire, c->wire_bytes, WnlaWireExp{n, rounds}.bytes());
    if (rc != BPPP_OK) return rc;
    return wnla_sec1_run(c, label, label_len, n, (const uint8_t*)d_commitments33, (const uint8_t*)d_c, (const uint8_t*)d_rho, (const uint8_t*)d_mu,
                         rounds, (const uint8_t*)d_proof_r33, (const uint8_t*)d_proof_x33, (const uint8_t*)d_proof_l, nl, (const uint8_t*)d_proof_n,
                         nn, (uint8_t*)d_accept, (int32_t*)d_status, c->d_wire, rlc_seed);
}
int bppp_wnla_verify_batch_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const void* d_commitments33,
                                       const void* d_c, const void* d_rho, const void* d_mu, size_t rounds, const void* d_proof_r33,
                                       const void* d_proof_x33, const void* d_proof_l, size_t nl, const void* d_proof_n, size_t nn,
                                       void* d_accept, void* d_status) {
    CtxLock lock_(c);
    return wnla_sec1_device_impl(c, label, label_len, n, d_commitments33, d_c, d_rho, d_mu, rounds, d_proof_r33, d_proof_x33, d_proof_l, nl,
                                 d_proof_n, nn, d_accept, d_status, nullptr);
}
int bppp_wnla_verify_batch_rlc_sec1_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const void* d_commitments33,
                                           const void* d_c, const void* d_rho, const void* d_mu, size_t rounds, const void* d_proof_r33,
                                           const void* d_proof_x33, const void* d_proof_l, size_t nl, const void* d_proof_n, size_t nn,
                                           void* d_accept, void* d_status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return wnla_sec1_device_impl(c, label, label_len, n, d_commitments33, d_c, d_rho, d_mu, rounds, d_proof_r33, d_proof_x33, d_proof_l, nl,
                                 d_proof_n, nn, d_accept, d_status, seed);
}
static int wnla_sec1_host_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments33,
                               const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, size_t rounds, const uint8_t* proof_r33,
                               const uint8_t* proof_x33, const uint8_t* proof_l, size_t nl, const uint8_t* proof_n, size_t nn,
                               uint8_t* accept, int32_t* status, const uint8_t* rlc_seed) {
    int rc = wnla_verify_check(c, label, label_len, commitments33, cvec, rho, mu, rounds, proof_r33, proof_x33, proof_l, nl, proof_n, nn, accept);
    if (rc != BPPP_OK) return rc;
    if (!wnla_shape_ok(rounds, nl, nn)) return BPPP_ERR_INVALID_ARG;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    HostStage hs;       // (proof.r / proof.x of no rounds and l / n of length 0 may be null: room of 0 bytes, no copy)
    rc = hs.begin(c, true, {{commitments33, n * 33}, {cvec, n * (size_t)c->nh * 32}, {rho, n * 32}, {mu, n * 32}, {proof_r33, n * rounds * 33},
                            {proof_x33, n * rounds * 33}, {proof_l, n * nl * 32}, {proof_n, n * nn * 32}}, n, nullptr, WnlaWireExp{n, rounds}.bytes());
    if (rc != BPPP_OK) return rc;
    uint8_t* const* in = hs.in;
    rc = wnla_sec1_run(c, label, label_len, n, in[0], in[1], in[2], in[3], rounds, in[4], in[5], in[6], nl, in[7], nn, hs.accept, hs.status, hs.tail,
                       rlc_seed);
    return hs.finish(rc, n, accept, status, nullptr);
}
int bppp_wnla_verify_batch_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments33,
                                const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, size_t rounds, const uint8_t* proof_r33,
                                const uint8_t* proof_x33, const uint8_t* proof_l, size_t nl, const uint8_t* proof_n, size_t nn,
                                uint8_t* accept, int32_t* status) {
    CtxLock lock_(c);
    return wnla_sec1_host_impl(c, label, label_len, n, commitments33, cvec, rho, mu, rounds, proof_r33, proof_x33, proof_l, nl, proof_n, nn,
                               accept, status, nullptr);
}
int bppp_wnla_verify_batch_rlc_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments33,
                                    const uint8_t* cvec, const uint8_t* rho, const uint8_t* mu, size_t rounds, const uint8_t* proof_r33,
                                    const uint8_t* proof_x33, const uint8_t* proof_l, size_t nl, const uint8_t* proof_n, size_t nn,
                                    uint8_t* accept, int32_t* status, const uint8_t seed[32]) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return wnla_sec1_host_impl(c, label, label_len, n, commitments33, cvec, rho, mu, rounds, proof_r33, proof_x33, proof_l, nl, proof_n, nn,
                               accept, status, seed);
}

// ---- provers: the 64-byte provers' impls with sec1 = true (33-byte commitments in, 33-byte proof points out)
int bppp_reciprocal_prove_batch_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                     const uint8_t* commitments33, const uint8_t* x, const uint8_t* sblind, const uint8_t* digits,
                                     const uint8_t* m, const uint8_t* rnd, uint8_t* proofs33, int32_t* status) {
    CtxLock lock_(c);
    return recip_prove_impl(c, label, label_len, nullptr, n, dim_nd, dim_np, commitments33, x, sblind, digits, m, rnd, proofs33, status, true);
}
int bppp_circuit_prove_batch_sec1(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                  const uint8_t* v_commitments33, const uint8_t* v, const uint8_t* s_v, const uint8_t* w_l, const uint8_t* w_r,
                                  const uint8_t* w_o, const uint8_t* rnd, uint8_t* proofs33, int32_t* status) {
    CtxLock lock_(c);
    return circuit_prove_impl(c, q, label, label_len, nullptr, n, v_commitments33, v, s_v, w_l, w_r, w_o, rnd, proofs33, status, true);
}
int bppp_wnla_prove_batch_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, const uint8_t* commitments33, const uint8_t* cvec,
                               const uint8_t* rho, const uint8_t* mu, const uint8_t* l, size_t nl, const uint8_t* nvec, size_t nn,
                               uint8_t* proof_r33, uint8_t* proof_x33, uint8_t* proof_l, uint8_t* proof_n, int32_t* status) {
    CtxLock lock_(c);
    return wnla_prove_impl(c, label, label_len, nullptr, n, commitments33, cvec, rho, mu, l, nl, nvec, nn, proof_r33, proof_x33, proof_l, proof_n,
                           status, true);
}


// ---- seeded provers (include/bppp.h: "Seeded provers"): the rnd twins with the draws made on the device into the rnd region of the
//      call's staging, which is cleared after the call
int bppp_reciprocal_prove_batch_seeded(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                       const uint8_t* commitments, const uint8_t* x, const uint8_t* sblind, const uint8_t* digits,
                                       const uint8_t* m, const uint8_t seed[32], uint64_t stream_base, uint8_t* proofs, int32_t* status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return recip_prove_impl(c, label, label_len, nullptr, n, dim_nd, dim_np, commitments, x, sblind, digits, m, nullptr, proofs, status, false,
                            seed, stream_base);
}
int bppp_circuit_prove_batch_seeded(bppp_ctx* c, const bppp_circuit* q, const uint8_t* label, size_t label_len, size_t n,
                                    const uint8_t* v_commitments, const uint8_t* v, const uint8_t* s_v, const uint8_t* w_l, const uint8_t* w_r,
                                    const uint8_t* w_o, const uint8_t seed[32], uint64_t stream_base, uint8_t* proofs, int32_t* status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return circuit_prove_impl(c, q, label, label_len, nullptr, n, v_commitments, v, s_v, w_l, w_r, w_o, nullptr, proofs, status, false,
                              seed, stream_base);
}

// ---- the reciprocal prover from integers: x and s in, commitments and proofs out (include/bppp.h: "Range proofs from integers")
int bppp_reciprocal_prove_values_batch(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                       const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd, uint8_t* proofs, uint8_t* commitments,
                                       int32_t* status) {
    CtxLock lock_(c);
    if (!rnd) return BPPP_ERR_INVALID_ARG;
    const RecipValues v = {false, commitments};
    return recip_prove_impl(c, label, label_len, nullptr, n, dim_nd, dim_np, nullptr, x, sblind, nullptr, nullptr, rnd, proofs, status, false,
                            nullptr, 0, &v);
}
int bppp_reciprocal_prove_values_batch_seeded(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                              const uint8_t* x, const uint8_t* sblind, const uint8_t seed[32], uint64_t stream_base,
                                              uint8_t* proofs, uint8_t* commitments, int32_t* status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    const RecipValues v = {false, commitments};
    return recip_prove_impl(c, label, label_len, nullptr, n, dim_nd, dim_np, nullptr, x, sblind, nullptr, nullptr, nullptr, proofs, status, false,
                            seed, stream_base, &v);
}
int bppp_reciprocal_prove_values_batch_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd, size_t dim_np,
                                              const void* d_x, const void* d_s, const void* d_rnd, void* d_proofs, void* d_commitments,
                                              void* d_status) {
    CtxLock lock_(c);
    if (!d_rnd) return BPPP_ERR_INVALID_ARG;
    const RecipValues v = {true, (uint8_t*)d_commitments};
    return recip_prove_impl(c, label, label_len, nullptr, n, dim_nd, dim_np, nullptr, (const uint8_t*)d_x, (const uint8_t*)d_s, nullptr, nullptr,
                            (const uint8_t*)d_rnd, (uint8_t*)d_proofs, (int32_t*)d_status, false, nullptr, 0, &v);
}
int bppp_reciprocal_prove_values_batch_seeded_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t dim_nd,
                                                     size_t dim_np, const void* d_x, const void* d_s, const uint8_t seed[32],
                                                     uint64_t stream_base, void* d_proofs, void* d_commitments, void* d_status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    const RecipValues v = {true, (uint8_t*)d_commitments};
    return recip_prove_impl(c, label, label_len, nullptr, n, dim_nd, dim_np, nullptr, (const uint8_t*)d_x, (const uint8_t*)d_s, nullptr, nullptr,
                            nullptr, (uint8_t*)d_proofs, (int32_t*)d_status, false, seed, stream_base, &v);
}

// ---------------------------------------------------------------- aggregated reciprocal range proof: the prover from integers
// (agg_prove_core.h has the stages; tests/agg_cases.py::prove states the protocol on the oracle).  k = 1 IS the reciprocal prover from
// integers and goes to its entry points.
static int agg_prove_shape_get(bppp_ctx* c, size_t k, size_t nd, size_t np, AggProveShapeDev& out) {
    for (const AggProveShapeDev& ap : c->agg_prove_shapes)
        if (ap.k == k && ap.nd == nd && ap.np == np) { out = ap; return BPPP_OK; }
    AggProveShape P;
    agg_prove_shape_build(P, k, nd, np);
    AggProveShapeDev ap;
    std::memset(&ap, 0, sizeof ap);
    ap.k = k; ap.nd = nd; ap.np = np;
    size_t off = 0;
    ap.part = take_bytes(off, P.parts.size() * 4 + 16); ap.al = take_bytes(off, P.al.size() * 4 + 16); ap.am = take_bytes(off, P.am.size() * 4 + 16);
    std::vector<uint8_t> host(off, 0);
    std::memcpy(host.data() + ap.part, P.parts.data(), P.parts.size() * 4);
    std::memcpy(host.data() + ap.al, P.al.data(), P.al.size() * 4);
    std::memcpy(host.data() + ap.am, P.am.data(), P.am.size() * 4);
    HIP_TRY(ctx_malloc(c, (void**)&ap.d, off));
    const hipError_t e = hipMemcpy(ap.d, host.data(), off, hipMemcpyHostToDevice);      // (synchronous: the host vector lives on this frame)
    if (e != hipSuccess) { (void)hipFree(ap.d); HIP_TRY(e); }
    c->agg_prove_shapes.push_back(ap);
    out = ap;
    return BPPP_OK;
}
// where one part's buffers sit in the context's blob
struct AggProveLayout {
    size_t x, s, rnd, com, dig, m, st, rst, vsc, vpb, ts, inst, scr, rsc, rpb, vsum, cpv, cpsv, cpwr, cpvp, prR, head, pout, cout;
    CircuitProveBufs c;
    WnlaProveBufs w;
    size_t total;
};
static AggProveLayout agg_prove_layout(const bppp_ctx* c, size_t n, size_t k, size_t nd, size_t np, const WnlaProveShape& sh, size_t proof_bytes) {
    const size_t nm = k * nd, nv = nd + 1, rows = n * k, n_rnd = agg_prove_draws(k, nd);
    size_t off = 0;
    auto take = [&](size_t bytes) { return take_bytes(off, bytes + 16); };
    AggProveLayout o;
    o.x = take(rows * 32); o.s = take(rows * 32); o.rnd = take(n * n_rnd * 32); o.com = take(rows * 64); o.dig = take(n * nm * 32);
    o.m = take(n * np * 32); o.st = take(n * 4); o.rst = take(rows * 4); o.vsc = take(2 * 8 * rows * 4); o.vpb = take(30 * rows * 4);
    o.ts = take(52 * n * 4); o.inst = take((2 + np) * 8 * n * 4); o.scr = take((nm + np) * 8 * n * 4); o.rsc = take(nv * 8 * rows * 4);
    o.rpb = take(30 * rows * 4); o.vsum = take(k * 50 * n * 4); o.cpv = take(rows * nv * 32); o.cpsv = take(rows * 32);
    o.cpwr = take(n * nm * 32); o.cpvp = take(rows * 64); o.prR = take(rows * 64); o.head = take(n * 256);
    o.c = circuit_prove_take(off, c, n, nm, nv, k * nv);
    WnlaProveShape shn = sh;
    shn.n = n;
    wnla_prove_take_proof(o.w, off, shn, 16);
    wnla_prove_take_state(o.w, off, c, shn, 16);
    o.pout = take(n * proof_bytes); o.cout = take(rows * 64);
    o.total = off;
    return o;
}
// Instances per part: "max_batch" bounds the multiplication gates (k dim_nd per instance) whose vectors a part holds -- the circuit
// prover keeps about two dozen scalar vectors of that length, three scalar sets over all generators and the WNLA prover's state,
// roughly 150-200 KB per instance at (16, 16, 16) -- so the default 2^21 gives 2^13 instances of that shape, about 1.6 GB.
static size_t agg_prove_part_size(const bppp_ctx* c, size_t n, size_t k, size_t nd) {
    size_t per = c->max_batch / (k * nd);
    if (per < 1) per = 1;
    return n < per ? n : per;
}
// one part of m instances: the launch chain on the context's stream.  Host forms: inputs uploaded into the blob, outputs copied back
// (queued; the caller waits).  Device forms: x, s, rnd, proofs, commitments, status used where they are.
// sec1 (host forms only): the assembled proofs and commitments compressed on the device into the wire buffer (the caller has grown it
// to agg_prove_wire_bytes of a part) and copied back from there, 33-byte points
static size_t agg_prove_wire_bytes(size_t n, size_t k, size_t wire_pb) { return align16(n * wire_pb) + n * k * 33; }
static int agg_prove_part(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t m, size_t k, size_t nd, size_t np, const AggProveShapeDev& shp,
                          const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd, const uint8_t* seed, uint64_t stream, uint8_t* proofs,
                          uint8_t* commitments, int32_t* status, bool device_io, const WnlaProveShape& sh0, size_t proof_bytes, bool sec1,
                          const HostTranscripts* tx = nullptr) {
    // tx: this part's slice of the caller's transcripts -- host pointers in the host forms, device pointers in the device form
    const size_t n = m, nm = k * nd, nv = nd + 1, rows = n * k, n_rnd = agg_prove_draws(k, nd);
    WnlaProveShape sh = sh0;
    sh.n = n;
    const AggProveLayout o = agg_prove_layout(c, n, k, nd, np, sh, proof_bytes);
    uint8_t* d = c->d_blob;
    hipStream_t s = c->stream;
    int rc = BPPP_OK;
    if (!device_io) {
        HIP_TRY(hipMemcpyAsync(d + o.x, x, rows * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d + o.s, sblind, rows * 32, hipMemcpyHostToDevice, s));
    }
    DrawWipe wipe = {seed ? d + o.rnd : nullptr, n * n_rnd * 32, s};
    if (seed) { const int rc_d = draw_enqueue(s, seed, stream, n, n_rnd, d + o.rnd); if (rc_d != BPPP_OK) return rc_d; }
    else if (!device_io) HIP_TRY(hipMemcpyAsync(d + o.rnd, rnd, n * n_rnd * 32, hipMemcpyHostToDevice, s));
    AggProveWs a;
    std::memset(&a, 0, sizeof a);
    a.N = n; a.k = (int)k; a.nd = (int)nd; a.np = (int)np; a.NG = c->ng; a.NH = c->nh; a.n_rnd = (int)n_rnd;
    recip_witness_shape(a.rw, nd, np);
    a.x = device_io ? x : d + o.x; a.s = device_io ? sblind : d + o.s; a.rnd = (device_io && !seed) ? rnd : d + o.rnd;
    a.digits = d + o.dig; a.m = d + o.m; a.status = (int32_t*)(d + o.st); a.row_status = (int32_t*)(d + o.rst); a.vsc = (u32*)(d + o.vsc);
    a.commitments = d + o.com; a.tstate = (u32*)(d + o.ts); a.inst_vals = (u32*)(d + o.inst); a.scr = (u32*)(d + o.scr);
    a.rsc = (u32*)(d + o.rsc); a.rpb = (u32*)(d + o.rpb); a.vsum = (u32*)(d + o.vsum);
    a.cp_v = d + o.cpv; a.cp_sv = d + o.cpsv; a.cp_wr = d + o.cpwr; a.cp_vpts = d + o.cpvp; a.proof_R = d + o.prR;
    a.fb = fb_table_of(c, rows);
    { const int rc_ct = ct_setup(c, a.fb_ct, a.ct, rows); if (rc_ct != BPPP_OK) return rc_ct; }      // x_i, s_i, rb_i and the reciprocals are secret
    t_new(a.base, label, (u32)label_len);
    TxDev txd;
    if (tx && device_io) {
        a.tio.states = tx->states; a.tio.n_states = tx->n_states; a.tio.states_out = tx->states_out;
        a.divergent_positions = tx->n_states != 1;
    } else {
        rc = txd.begin(c, tx, n, s, a.tio, a.divergent_positions);
        if (rc != BPPP_OK) return rc;
    }
    // the value commitments: the reciprocal prover's commitment kernels over N k rows
    RecipCommitWs cw;
    std::memset(&cw, 0, sizeof cw);
    cw.N = rows; cw.NG = c->ng; cw.x = a.x; cw.s = a.s; cw.status = a.row_status; cw.msc = a.vsc; cw.pbuf = (u32*)(d + o.vpb); cw.out = d + o.com;
    cw.fb = a.fb; cw.fb_ct = a.fb_ct; cw.ct = a.ct;
    // the circuit prover on the aggregate's circuit: closed-form collect, so no pattern
    CircuitProveWs p;
    std::memset(&p, 0, sizeof p);
    p.base = a.base; p.tio = a.tio; p.divergent_positions = a.divergent_positions;
    CircuitDev& cd = p.cd;
    cd.nm = (int)nm; cd.no = (int)np; cd.k = (int)k; cd.nl = (int)(k * nv); cd.nv = (int)nv; cd.nw = (int)(2 * nm + np); cd.f_l = 1; cd.f_m = 0;
    cd.a_l = (const u32*)(shp.d + shp.al); cd.a_m = (const u32*)(shp.d + shp.am); cd.inst_vals = a.inst_vals;
    p.N = n; p.NG = c->ng; p.NH = c->nh; p.n_rnd = (int)(18 + nv + nm); p.rnd_stride = n_rnd * 32; p.part = (const int*)(shp.d + shp.part);
    p.transcript_preloaded = 1;
    p.v_pts = a.cp_vpts; p.v = a.cp_v; p.s_v = a.cp_sv; p.w_l = a.digits; p.w_r = a.cp_wr; p.w_o = a.m; p.rnd = a.rnd + 32 * k;
    p.proof_head = d + o.head; p.status = a.status; p.tstate = a.tstate;
    circuit_prove_carve(p, d, o.c);
    p.fb = fb_table_of(c, n);
    { const int rc_ct = ct_setup(c, p.fb_ct, p.ct, n); if (rc_ct != BPPP_OK) return rc_ct; }
    WnlaProveWs w;
    rc = wnla_prove_fill_behind(c, w, sh, d, o.w, p);
    if (rc != BPPP_OK) return rc;
    const unsigned blocks = blocks_of(n), fb_blocks = fb_blocks_of(n), row_blocks = blocks_of(rows), row_fb_blocks = fb_blocks_of(rows);
    GLAUNCH(s, K_APROVE_WITNESS, k_aprove_witness<<<blocks, BPPP_BLOCK, 0, s>>>(a));
    GLAUNCH(s, K_APROVE_COMMIT, {
        k_rprove_commit<<<row_fb_blocks, BPPP_FB_BLOCK, 0, s>>>(cw);
        k_rprove_commit_store<<<row_blocks, BPPP_BLOCK, 0, s>>>(cw);
    });
    GLAUNCH(s, K_APROVE_POLES, {
        if (a.tio.states) k_aprove_stage_r1_tx<<<blocks, BPPP_BLOCK, 0, s>>>(a);
        else k_aprove_stage_r1<<<blocks, BPPP_BLOCK, 0, s>>>(a);
        k_aprove_msm<<<row_fb_blocks, BPPP_FB_BLOCK, 0, s>>>(a);
        k_aprove_stage_r2<<<blocks, BPPP_BLOCK, 0, s>>>(a);
    });
    HIP_TRY(hipMemsetAsync(p.msc, 0, 3 * (size_t)c->nbases * 8 * n * 4, s));     // the sets are written sparsely (slot = base index)
    GLAUNCH(s, K_APROVE_STAGE_A, {
        k_cprove_stage_a<<<blocks, BPPP_BLOCK, 0, s>>>(p);
        for (int set = 0; set < 3; set++) k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, set, 0);
    });
    if (p.tio.states) GLAUNCH(s, K_APROVE_STAGE_B, k_aprove_stage_b_tx<<<blocks, BPPP_BLOCK, 0, s>>>(p));
    else GLAUNCH(s, K_APROVE_STAGE_B, k_aprove_stage_b<<<blocks, BPPP_BLOCK, 0, s>>>(p));
    if (c->timing) GLAUNCH(s, K_APROVE_COLLECT, k_aprove_collect<<<blocks, BPPP_BLOCK, 0, s>>>(p));      // (same values again: its time alone)
    GLAUNCH(s, K_APROVE_TAIL, {
        k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, 0, 0);
        k_cprove_stage_c<<<blocks, BPPP_BLOCK, 0, s>>>(p);
        k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, 0, 1);
        k_cprove_stage_d<<<blocks, BPPP_BLOCK, 0, s>>>(p);
        wnla_prove_launch(w, s);
    });
    HIP_TRY(hipGetLastError());
    // the proofs put together on the device (a flagged instance as zero bytes); a flagged instance's commitments zeroed by the same kernel
    ProofAssembleWs as;
    std::memset(&as, 0, sizeof as);
    as.N = n; as.proof_bytes = proof_bytes; as.nseg = 6; as.status = p.status; as.out = device_io ? proofs : d + o.pout;
    as.src[0] = p.proof_head; as.bytes[0] = 256;
    as.src[1] = w.proof_r; as.bytes[1] = (u32)(sh.rounds * 64);
    as.src[2] = w.proof_x; as.bytes[2] = (u32)(sh.rounds * 64);
    as.src[3] = a.proof_R; as.bytes[3] = (u32)(k * 64);
    as.src[4] = w.proof_l; as.bytes[4] = (u32)(sh.nl_f * 32);
    as.src[5] = w.proof_n; as.bytes[5] = (u32)(sh.nn_f * 32);
    size_t words = n * (proof_bytes / 4);
    if ((words + 255) / 256 > 0xFFFFFFFFu) return BPPP_ERR_INVALID_ARG;
    k_gprove_assemble<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(as);
    // the commitments through the same kernel: one segment of k x 64 bytes, so that a status raised behind the witness stage zeroes them too
    ProofAssembleWs ac;
    std::memset(&ac, 0, sizeof ac);
    ac.N = n; ac.proof_bytes = k * 64; ac.nseg = 1; ac.status = p.status; ac.out = device_io ? commitments : d + o.cout;
    ac.src[0] = d + o.com; ac.bytes[0] = (u32)(k * 64);
    words = n * (k * 16);
    k_gprove_assemble<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(ac);
    HIP_TRY(hipGetLastError());
    if (sec1) {
        // (a flagged instance's zero bytes come out as the identity's zero bytes: a zeroed 33-byte-point proof and k x 33 zero bytes)
        const size_t wP = 4 + 2 * sh.rounds + k, wS = sh.nl_f + sh.nn_f, wire_pb = wire_proof_bytes(wP, wS), o_wc = align16(n * wire_pb);
        WireMap wm;
        wire_map_init(wm, n);
        wire_map_add(wm, false, d + o.pout, proof_bytes, c->d_wire, wire_pb, wP);
        wire_map_add(wm, true, d + o.pout + 64 * wP, proof_bytes, c->d_wire + 33 * wP, wire_pb, wS);
        wire_map_add(wm, false, d + o.cout, 64 * k, c->d_wire + o_wc, 33 * k, k);
        rc = wire_launch(wm, false, s);
        if (rc != BPPP_OK) return rc;
        HIP_TRY(hipMemcpyAsync(proofs, c->d_wire, n * wire_pb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(commitments, c->d_wire + o_wc, rows * 33, hipMemcpyDeviceToHost, s));
    } else if (!device_io) {
        HIP_TRY(hipMemcpyAsync(proofs, d + o.pout, n * proof_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(commitments, d + o.cout, rows * 64, hipMemcpyDeviceToHost, s));
    }
    if (status) HIP_TRY(hipMemcpyAsync(status, p.status, n * 4, device_io ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    // every instance's transcript as the prover left it; an instance whose proof is zeroed gets its input state back
    if (tx && device_io) {
        if (a.tio.states_out) {
            k_aprove_export_states<<<blocks, BPPP_BLOCK, 0, s>>>(a.tio, a.base, p.tstate, n, p.status);
            HIP_TRY(hipGetLastError());
        }
    } else {
        rc = txd.finish(tx, a.tio, a.base, p.tstate, n, p.status, s, true);
        if (rc != BPPP_OK) return rc;
    }
    HIP_TRY(wipe.now());      // the draws cleared behind the last kernel that reads them
    return BPPP_OK;
}
static int agg_prove_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t nd, size_t np, const uint8_t* x,
                          const uint8_t* sblind, const uint8_t* rnd, const uint8_t* seed, uint64_t stream_base, uint8_t* proofs,
                          uint8_t* commitments, int32_t* status, bool device_io, bool sec1 = false, const HostTranscripts* tx = nullptr) {
    // tx (the _transcript forms): the callers' transcripts in (1 or n) and out, pointers of the kind the call's other buffers are; the
    // host forms check the states here, the device form flags an invalid one per instance
    if (!c || !label_ok(label, label_len) || !x || !sblind || (!rnd && !seed) || !proofs || !commitments) return BPPP_ERR_INVALID_ARG;
    if (!agg_prove_shape_ok(k, nd, np, (size_t)c->ng, (size_t)c->nh)) return BPPP_ERR_INVALID_ARG;
    const size_t n_rnd = agg_prove_draws(k, nd);
    if (seed && !draw_args_ok(seed, stream_base, n, n_rnd)) return BPPP_ERR_INVALID_ARG;
    if (tx && (!tx->states || (tx->n_states != 1 && tx->n_states != n))) return BPPP_ERR_INVALID_ARG;
    if (tx && !device_io && n) { const int rc_t = check_host_transcripts(tx, n); if (rc_t != BPPP_OK) return rc_t; }
    if (k == 1) {
        const TranscriptIo d_tx = {tx ? tx->states : nullptr, tx ? tx->n_states : 0, tx ? tx->states_out : nullptr, 0};
        const RecipValues v = {device_io, commitments, tx && device_io ? &d_tx : nullptr};
        return recip_prove_impl(c, label, label_len, device_io ? nullptr : tx, n, nd, np, nullptr, x, sblind, nullptr, nullptr, rnd, proofs, status,
                                sec1, seed, stream_base, &v);
    }
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    AggProveShapeDev shp;
    { const int rc_s = agg_prove_shape_get(c, k, nd, np, shp); if (rc_s != BPPP_OK) return rc_s; }
    WnlaProveShape sh = {0, (size_t)c->nh, (size_t)c->ng, 0, 0, 0};
    wnla_proof_shape(sh.nl, sh.nn, sh.rounds, sh.nl_f, sh.nn_f);
    const size_t proof_bytes = agg_proof_bytes(k, sh.rounds, sh.nl_f, sh.nn_f);
    const size_t per = agg_prove_part_size(c, n, k, nd);
    sh.n = per;
    WnlaBlob blob;      // host forms: nothing of the call still runs when it returns, whichever way it leaves
    const size_t blob_bytes = agg_prove_layout(c, per, k, nd, np, sh, proof_bytes).total;
    if (device_io) { const int rc_b = ensure_blob(c, blob_bytes); if (rc_b != BPPP_OK) return rc_b; }
    else { const int rc_b = blob.take(c, blob_bytes); if (rc_b != BPPP_OK) return rc_b; }
    const size_t wire_pb = wire_proof_bytes(4 + 2 * sh.rounds + k, sh.nl_f + sh.nn_f);
    if (sec1) { const int rc_w = ensure_buffer(c, c->d_wire, c->wire_bytes, agg_prove_wire_bytes(per, k, wire_pb)); if (rc_w != BPPP_OK) return rc_w; }
    const size_t out_pb = sec1 ? wire_pb : proof_bytes, out_cb = sec1 ? 33 : 64;
    for (size_t lo = 0; lo < n; lo += per) {
        const size_t m = n - lo < per ? n - lo : per;
        // a part's own slice of the caller's states (or the one shared state) and of states_out
        HostTranscripts ptx = {nullptr, 0, nullptr};
        if (tx) {
            const bool shared = tx->n_states == 1;
            ptx.states = tx->states + (shared ? 0 : 203 * lo); ptx.n_states = shared ? 1 : m;
            ptx.states_out = tx->states_out ? tx->states_out + 203 * lo : nullptr;
        }
        const int rc = agg_prove_part(c, label, label_len, m, k, nd, np, shp, x + lo * k * 32, sblind + lo * k * 32,
                                      rnd ? rnd + lo * n_rnd * 32 : nullptr, seed, stream_base + lo, proofs + lo * out_pb,
                                      commitments + lo * k * out_cb, status ? status + lo : nullptr, device_io, sh, proof_bytes, sec1,
                                      tx ? &ptx : nullptr);
        if (rc != BPPP_OK) return rc;
    }
    if (!device_io) HIP_TRY(hipStreamSynchronize(c->stream));
    return BPPP_OK;
}
size_t bppp_reciprocal_agg_prove_draws(size_t k, size_t dim_nd) { return agg_prove_draws(k, dim_nd); }
int bppp_reciprocal_agg_prove_values_batch(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd, size_t dim_np,
                                           const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd, uint8_t* proofs, uint8_t* commitments,
                                           int32_t* status) {
    CtxLock lock_(c);
    if (!rnd) return BPPP_ERR_INVALID_ARG;
    return agg_prove_impl(c, label, label_len, n, k, dim_nd, dim_np, x, sblind, rnd, nullptr, 0, proofs, commitments, status, false);
}
int bppp_reciprocal_agg_prove_values_batch_seeded(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                  size_t dim_np, const uint8_t* x, const uint8_t* sblind, const uint8_t seed[32],
                                                  uint64_t stream_base, uint8_t* proofs, uint8_t* commitments, int32_t* status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_prove_impl(c, label, label_len, n, k, dim_nd, dim_np, x, sblind, nullptr, seed, stream_base, proofs, commitments, status, false);
}
// the wire form (host buffers only): the same calls with the proofs and the commitments compressed on the device before the copy back
int bppp_reciprocal_agg_prove_values_batch_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                size_t dim_np, const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd, uint8_t* proofs33,
                                                uint8_t* commitments33, int32_t* status) {
    CtxLock lock_(c);
    if (!rnd) return BPPP_ERR_INVALID_ARG;
    return agg_prove_impl(c, label, label_len, n, k, dim_nd, dim_np, x, sblind, rnd, nullptr, 0, proofs33, commitments33, status, false, true);
}
int bppp_reciprocal_agg_prove_values_batch_seeded_sec1(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                       size_t dim_np, const uint8_t* x, const uint8_t* sblind, const uint8_t seed[32],
                                                       uint64_t stream_base, uint8_t* proofs33, uint8_t* commitments33, int32_t* status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_prove_impl(c, label, label_len, n, k, dim_nd, dim_np, x, sblind, nullptr, seed, stream_base, proofs33, commitments33, status, false,
                          true);
}
int bppp_reciprocal_agg_prove_values_batch_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                  size_t dim_np, const void* d_x, const void* d_s, const void* d_rnd, void* d_proofs,
                                                  void* d_commitments, void* d_status) {
    CtxLock lock_(c);
    if (!d_rnd) return BPPP_ERR_INVALID_ARG;
    return agg_prove_impl(c, label, label_len, n, k, dim_nd, dim_np, (const uint8_t*)d_x, (const uint8_t*)d_s, (const uint8_t*)d_rnd, nullptr, 0,
                          (uint8_t*)d_proofs, (uint8_t*)d_commitments, (int32_t*)d_status, true);
}
int bppp_reciprocal_agg_prove_values_batch_seeded_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, size_t dim_nd,
                                                         size_t dim_np, const void* d_x, const void* d_s, const uint8_t seed[32],
                                                         uint64_t stream_base, void* d_proofs, void* d_commitments, void* d_status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_prove_impl(c, label, label_len, n, k, dim_nd, dim_np, (const uint8_t*)d_x, (const uint8_t*)d_s, nullptr, seed, stream_base,
                          (uint8_t*)d_proofs, (uint8_t*)d_commitments, (int32_t*)d_status, true);
}
// the same on the CALLER'S transcripts: states in (1 shared or n), every instance's transcript as the prover left it out; an instance
// whose proof is zeroed gets its input state back
int bppp_reciprocal_agg_prove_values_batch_transcript(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, size_t k, size_t dim_nd,
                                                      size_t dim_np, const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd, uint8_t* proofs,
                                                      uint8_t* commitments, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!rnd || !states) return BPPP_ERR_INVALID_ARG;
    const HostTranscripts tx = {states, n_states, states_out};
    return agg_prove_impl(c, nullptr, 0, n, k, dim_nd, dim_np, x, sblind, rnd, nullptr, 0, proofs, commitments, status, false, false, &tx);
}
int bppp_reciprocal_agg_prove_values_batch_transcript_seeded(bppp_ctx* c, size_t n, const uint8_t* states, size_t n_states, size_t k,
                                                             size_t dim_nd, size_t dim_np, const uint8_t* x, const uint8_t* sblind,
                                                             const uint8_t seed[32], uint64_t stream_base, uint8_t* proofs,
                                                             uint8_t* commitments, int32_t* status, uint8_t* states_out) {
    CtxLock lock_(c);
    if (!seed || !states) return BPPP_ERR_INVALID_ARG;
    const HostTranscripts tx = {states, n_states, states_out};
    return agg_prove_impl(c, nullptr, 0, n, k, dim_nd, dim_np, x, sblind, nullptr, seed, stream_base, proofs, commitments, status, false, false, &tx);
}
int bppp_reciprocal_agg_prove_values_batch_transcript_device(bppp_ctx* c, size_t n, const void* d_states, size_t n_states, size_t k,
                                                             size_t dim_nd, size_t dim_np, const void* d_x, const void* d_s, const void* d_rnd,
                                                             void* d_proofs, void* d_commitments, void* d_status, void* d_states_out) {
    CtxLock lock_(c);
    if (!d_rnd || !d_states) return BPPP_ERR_INVALID_ARG;
    const HostTranscripts tx = {(const uint8_t*)d_states, n_states, (uint8_t*)d_states_out};
    return agg_prove_impl(c, nullptr, 0, n, k, dim_nd, dim_np, (const uint8_t*)d_x, (const uint8_t*)d_s, (const uint8_t*)d_rnd, nullptr, 0,
                          (uint8_t*)d_proofs, (uint8_t*)d_commitments, (int32_t*)d_status, true, false, &tx);
}

// ---- the prover from integers for MIXED value counts (agg_prove_mixed_core.h): instance i has ks[i] values in slots laid out by k_max.
//      Label transcripts, 64-byte outputs.  The blob, the shape data and the parts are agg_prove_part's for k = k_max (agg_prove_layout,
//      agg_prove_shape_get, agg_prove_part_size) with a part's slice of ks behind them; the fixed-base sums, stage D and the WNLA prover
//      are the uniform launches; nothing is forwarded (k_max = 1 runs here too).
int bppp_reciprocal_agg_prove_mixed_check_args(size_t ng, size_t nh, size_t n, size_t k_max, const uint8_t* ks, int ks_on_device, size_t dim_nd,
                                               size_t dim_np) {
    return agg_prove_mixed_args_ok(ng, nh, n, k_max, ks, ks_on_device != 0, dim_nd, dim_np) ? BPPP_OK : BPPP_ERR_INVALID_ARG;
}
// one part of m instances.  ks: this part's slice -- a host pointer in the host forms (uploaded behind the part's layout), else a device one
static int agg_prove_mixed_part(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t m, size_t k, size_t nd, size_t np,
                                const AggProveShapeDev& shp, const uint8_t* ks, const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd,
                                const uint8_t* seed, uint64_t stream, uint8_t* proofs, uint8_t* commitments, int32_t* status, bool device_io,
                                const WnlaProveShape& sh0, size_t proof_bytes) {
    const size_t n = m, nm = k * nd, nv = nd + 1, rows = n * k, n_rnd = agg_prove_draws(k, nd);
    WnlaProveShape sh = sh0;
    sh.n = n;
    const AggProveLayout o = agg_prove_layout(c, n, k, nd, np, sh, proof_bytes);
    uint8_t* d = c->d_blob;
    hipStream_t s = c->stream;
    int rc = BPPP_OK;
    if (!device_io) {
        HIP_TRY(hipMemcpyAsync(d + o.total, ks, n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d + o.x, x, rows * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d + o.s, sblind, rows * 32, hipMemcpyHostToDevice, s));
    }
    DrawWipe wipe = {seed ? d + o.rnd : nullptr, n * n_rnd * 32, s};
    if (seed) { const int rc_d = draw_enqueue(s, seed, stream, n, n_rnd, d + o.rnd); if (rc_d != BPPP_OK) return rc_d; }
    else if (!device_io) HIP_TRY(hipMemcpyAsync(d + o.rnd, rnd, n * n_rnd * 32, hipMemcpyHostToDevice, s));
    AggProveMixedWs am;
    std::memset(&am, 0, sizeof am);
    am.ks = device_io ? ks : d + o.total;
    AggProveWs& a = am.a;
    a.N = n; a.k = (int)k; a.nd = (int)nd; a.np = (int)np; a.NG = c->ng; a.NH = c->nh; a.n_rnd = (int)n_rnd;
    recip_witness_shape(a.rw, nd, np);
    a.x = device_io ? x : d + o.x; a.s = device_io ? sblind : d + o.s; a.rnd = (device_io && !seed) ? rnd : d + o.rnd;
    a.digits = d + o.dig; a.m = d + o.m; a.status = (int32_t*)(d + o.st); a.row_status = (int32_t*)(d + o.rst); a.vsc = (u32*)(d + o.vsc);
    a.commitments = d + o.com; a.tstate = (u32*)(d + o.ts); a.inst_vals = (u32*)(d + o.inst); a.scr = (u32*)(d + o.scr);
    a.rsc = (u32*)(d + o.rsc); a.rpb = (u32*)(d + o.rpb); a.vsum = (u32*)(d + o.vsum);
    a.cp_v = d + o.cpv; a.cp_sv = d + o.cpsv; a.cp_wr = d + o.cpwr; a.cp_vpts = d + o.cpvp; a.proof_R = d + o.prR;
    a.fb = fb_table_of(c, rows);
    { const int rc_ct = ct_setup(c, a.fb_ct, a.ct, rows); if (rc_ct != BPPP_OK) return rc_ct; }
    t_new(a.base, label, (u32)label_len);
    // the value commitments over N k_max rows (the rows behind an instance's k_i carry zero scalars: the identity)
    RecipCommitWs cw;
    std::memset(&cw, 0, sizeof cw);
    cw.N = rows; cw.NG = c->ng; cw.x = a.x; cw.s = a.s; cw.status = a.row_status; cw.msc = a.vsc; cw.pbuf = (u32*)(d + o.vpb); cw.out = d + o.com;
    cw.fb = a.fb; cw.fb_ct = a.fb_ct; cw.ct = a.ct;
    CircuitProveMixedWs pm;
    std::memset(&pm, 0, sizeof pm);
    pm.ks = am.ks; pm.k_max = (int)k;
    CircuitProveWs& p = pm.p;
    p.base = a.base;
    CircuitDev& cd = p.cd;
    cd.nm = (int)nm; cd.no = (int)np; cd.k = (int)k; cd.nl = (int)(k * nv); cd.nv = (int)nv; cd.nw = (int)(2 * nm + np); cd.f_l = 1; cd.f_m = 0;
    cd.a_l = (const u32*)(shp.d + shp.al); cd.a_m = (const u32*)(shp.d + shp.am); cd.inst_vals = a.inst_vals;
    p.N = n; p.NG = c->ng; p.NH = c->nh; p.n_rnd = (int)(18 + nv + nm); p.rnd_stride = n_rnd * 32; p.part = (const int*)(shp.d + shp.part);
    p.transcript_preloaded = 1;
    p.v_pts = a.cp_vpts; p.v = a.cp_v; p.s_v = a.cp_sv; p.w_l = a.digits; p.w_r = a.cp_wr; p.w_o = a.m; p.rnd = a.rnd + 32 * k;
    p.proof_head = d + o.head; p.status = a.status; p.tstate = a.tstate;
    circuit_prove_carve(p, d, o.c);
    p.fb = fb_table_of(c, n);
    { const int rc_ct = ct_setup(c, p.fb_ct, p.ct, n); if (rc_ct != BPPP_OK) return rc_ct; }
    WnlaProveWs w;
    rc = wnla_prove_fill_behind(c, w, sh, d, o.w, p);
    if (rc != BPPP_OK) return rc;
    const unsigned blocks = blocks_of(n), fb_blocks = fb_blocks_of(n), row_blocks = blocks_of(rows), row_fb_blocks = fb_blocks_of(rows);
    GLAUNCH(s, K_APMIX_WITNESS, k_aprove_mixed_witness<<<blocks, BPPP_BLOCK, 0, s>>>(am));
    GLAUNCH(s, K_APMIX_COMMIT, {
        k_rprove_commit<<<row_fb_blocks, BPPP_FB_BLOCK, 0, s>>>(cw);
        k_rprove_commit_store<<<row_blocks, BPPP_BLOCK, 0, s>>>(cw);
    });
    GLAUNCH(s, K_APMIX_POLES, {
        k_aprove_mixed_stage_r1<<<blocks, BPPP_BLOCK, 0, s>>>(am);
        k_aprove_msm<<<row_fb_blocks, BPPP_FB_BLOCK, 0, s>>>(a);
        k_aprove_mixed_stage_r2<<<blocks, BPPP_BLOCK, 0, s>>>(am);
    });
    HIP_TRY(hipMemsetAsync(p.msc, 0, 3 * (size_t)c->nbases * 8 * n * 4, s));     // every fill writes k_i nd entries: zeros behind them
    GLAUNCH(s, K_APMIX_STAGE_A, {
        k_aprove_mixed_stage_a<<<blocks, BPPP_BLOCK, 0, s>>>(pm);
        for (int set = 0; set < 3; set++) k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, set, 0);
    });
    // stage B once per value count the call may hold (k_aggprove_mixed.hip: the lanes of that count run, the others leave at once)
    GLAUNCH(s, K_APMIX_STAGE_B, {
        for (int kk = 1; kk <= (int)k; kk++) k_aprove_mixed_stage_b<<<blocks, BPPP_BLOCK, 0, s>>>(pm, kk);
    });
    if (c->timing) GLAUNCH(s, K_APMIX_COLLECT, k_aprove_mixed_collect<<<blocks, BPPP_BLOCK, 0, s>>>(pm));      // (same values again: its time alone)
    GLAUNCH(s, K_APMIX_TAIL, {
        k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, 0, 0);
        k_aprove_mixed_stage_c<<<blocks, BPPP_BLOCK, 0, s>>>(pm);
        k_cprove_msm<<<fb_blocks, BPPP_FB_BLOCK, 0, s>>>(p, 0, 1);
        k_cprove_stage_d<<<blocks, BPPP_BLOCK, 0, s>>>(p);
        wnla_prove_launch(w, s);
    });
    HIP_TRY(hipGetLastError());
    // the proofs and the commitments put together on the device: an instance's k_i poles and commitments, zero bytes behind what it
    // uses and in every flagged instance
    ProofAssembleMixedWs as;
    std::memset(&as, 0, sizeof as);
    as.ks = am.ks; as.k_max = (int)k; as.vseg = 3;
    as.w.N = n; as.w.proof_bytes = proof_bytes; as.w.nseg = 6; as.w.status = p.status; as.w.out = device_io ? proofs : d + o.pout;
    as.w.src[0] = p.proof_head; as.w.bytes[0] = 256;
    as.w.src[1] = w.proof_r; as.w.bytes[1] = (u32)(sh.rounds * 64);
    as.w.src[2] = w.proof_x; as.w.bytes[2] = (u32)(sh.rounds * 64);
    as.w.src[3] = a.proof_R; as.w.bytes[3] = (u32)(k * 64);
    as.w.src[4] = w.proof_l; as.w.bytes[4] = (u32)(sh.nl_f * 32);
    as.w.src[5] = w.proof_n; as.w.bytes[5] = (u32)(sh.nn_f * 32);
    ProofAssembleMixedWs ac;
    std::memset(&ac, 0, sizeof ac);
    ac.ks = am.ks; ac.k_max = (int)k; ac.vseg = 0;
    ac.w.N = n; ac.w.proof_bytes = k * 64; ac.w.nseg = 1; ac.w.status = p.status; ac.w.out = device_io ? commitments : d + o.cout;
    ac.w.src[0] = d + o.com; ac.w.bytes[0] = (u32)(k * 64);
    const size_t words = n * (proof_bytes / 4), cwords = n * (k * 16);
    if ((words + 255) / 256 > 0xFFFFFFFFu) return BPPP_ERR_INVALID_ARG;
    GLAUNCH(s, K_APMIX_ASSEMBLE, {
        k_aprove_mixed_assemble<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(as);
        k_aprove_mixed_assemble<<<(unsigned)((cwords + 255) / 256), 256, 0, s>>>(ac);
    });
    HIP_TRY(hipGetLastError());
    if (!device_io) {
        HIP_TRY(hipMemcpyAsync(proofs, d + o.pout, n * proof_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(commitments, d + o.cout, rows * 64, hipMemcpyDeviceToHost, s));
    }
    if (status) HIP_TRY(hipMemcpyAsync(status, p.status, n * 4, device_io ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    HIP_TRY(wipe.now());      // the draws cleared behind the last kernel that reads them
    return BPPP_OK;
}
static int agg_prove_mixed_impl(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k, const uint8_t* ks, size_t nd, size_t np,
                                const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd, const uint8_t* seed, uint64_t stream_base,
                                uint8_t* proofs, uint8_t* commitments, int32_t* status, bool device_io) {
    if (!c || !label_ok(label, label_len) || !x || !sblind || (!rnd && !seed) || !proofs || !commitments) return BPPP_ERR_INVALID_ARG;
    if (!agg_prove_mixed_args_ok((size_t)c->ng, (size_t)c->nh, n, k, ks, device_io, nd, np)) return BPPP_ERR_INVALID_ARG;
    const size_t n_rnd = agg_prove_draws(k, nd);
    if (seed && !draw_args_ok(seed, stream_base, n, n_rnd)) return BPPP_ERR_INVALID_ARG;
    if (n == 0) return BPPP_OK;
    HIP_TRY(hipSetDevice(c->device));
    AggProveShapeDev shp;
    { const int rc_s = agg_prove_shape_get(c, k, nd, np, shp); if (rc_s != BPPP_OK) return rc_s; }
    WnlaProveShape sh = {0, (size_t)c->nh, (size_t)c->ng, 0, 0, 0};
    wnla_proof_shape(sh.nl, sh.nn, sh.rounds, sh.nl_f, sh.nn_f);
    const size_t proof_bytes = agg_proof_bytes(k, sh.rounds, sh.nl_f, sh.nn_f);
    const size_t per = agg_prove_part_size(c, n, k, nd);
    sh.n = per;
    WnlaBlob blob;      // host forms: nothing of the call still runs when it returns, whichever way it leaves
    const size_t blob_bytes = agg_prove_layout(c, per, k, nd, np, sh, proof_bytes).total + align16(per);      // (+ a part's ks)
    if (device_io) { const int rc_b = ensure_blob(c, blob_bytes); if (rc_b != BPPP_OK) return rc_b; }
    else { const int rc_b = blob.take(c, blob_bytes); if (rc_b != BPPP_OK) return rc_b; }
    for (size_t lo = 0; lo < n; lo += per) {
        const size_t m = n - lo < per ? n - lo : per;
        const int rc = agg_prove_mixed_part(c, label, label_len, m, k, nd, np, shp, ks + lo, x + lo * k * 32, sblind + lo * k * 32,
                                            rnd ? rnd + lo * n_rnd * 32 : nullptr, seed, stream_base + lo, proofs + lo * proof_bytes,
                                            commitments + lo * k * 64, status ? status + lo : nullptr, device_io, sh, proof_bytes);
        if (rc != BPPP_OK) return rc;
    }
    if (!device_io) HIP_TRY(hipStreamSynchronize(c->stream));
    return BPPP_OK;
}
int bppp_reciprocal_agg_prove_values_batch_mixed(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max, const uint8_t* ks,
                                                 size_t dim_nd, size_t dim_np, const uint8_t* x, const uint8_t* sblind, const uint8_t* rnd,
                                                 uint8_t* proofs, uint8_t* commitments, int32_t* status) {
    CtxLock lock_(c);
    if (!rnd) return BPPP_ERR_INVALID_ARG;
    return agg_prove_mixed_impl(c, label, label_len, n, k_max, ks, dim_nd, dim_np, x, sblind, rnd, nullptr, 0, proofs, commitments, status, false);
}
int bppp_reciprocal_agg_prove_values_batch_mixed_seeded(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max,
                                                        const uint8_t* ks, size_t dim_nd, size_t dim_np, const uint8_t* x, const uint8_t* sblind,
                                                        const uint8_t seed[32], uint64_t stream_base, uint8_t* proofs, uint8_t* commitments,
                                                        int32_t* status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_prove_mixed_impl(c, label, label_len, n, k_max, ks, dim_nd, dim_np, x, sblind, nullptr, seed, stream_base, proofs, commitments,
                                status, false);
}
int bppp_reciprocal_agg_prove_values_batch_mixed_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max,
                                                        const void* d_ks, size_t dim_nd, size_t dim_np, const void* d_x, const void* d_s,
                                                        const void* d_rnd, void* d_proofs, void* d_commitments, void* d_status) {
    CtxLock lock_(c);
    if (!d_rnd) return BPPP_ERR_INVALID_ARG;
    return agg_prove_mixed_impl(c, label, label_len, n, k_max, (const uint8_t*)d_ks, dim_nd, dim_np, (const uint8_t*)d_x, (const uint8_t*)d_s,
                                (const uint8_t*)d_rnd, nullptr, 0, (uint8_t*)d_proofs, (uint8_t*)d_commitments, (int32_t*)d_status, true);
}
int bppp_reciprocal_agg_prove_values_batch_mixed_seeded_device(bppp_ctx* c, const uint8_t* label, size_t label_len, size_t n, size_t k_max,
                                                               const void* d_ks, size_t dim_nd, size_t dim_np, const void* d_x, const void* d_s,
                                                               const uint8_t seed[32], uint64_t stream_base, void* d_proofs,
                                                               void* d_commitments, void* d_status) {
    CtxLock lock_(c);
    if (!seed) return BPPP_ERR_INVALID_ARG;
    return agg_prove_mixed_impl(c, label, label_len, n, k_max, (const uint8_t*)d_ks, dim_nd, dim_np, (const uint8_t*)d_x, (const uint8_t*)d_s,
                                nullptr, seed, stream_base, (uint8_t*)d_proofs, (uint8_t*)d_commitments, (int32_t*)d_status, true);
}

}  // extern "C"
#undef GLAUNCH
