"""GPU tier of the single-proof front end over WIRE rows: bppp_u64_verify_one_sec1[_transcript] and
bppp_reciprocal_verify_one_sec1[_transcript] (include/bppp.h) -- one proof per call from many host threads, 33-byte SEC1 points.
Wire callers and 64-byte callers share one context; every answer is the batched wire-form entry point's for that row and the
oracle's verdict, a pre-loaded transcript comes back advanced as the oracle advances it, and an undecodable row gets
BPPP_ST_BAD_ENCODING and its transcript back untouched."""
import threading

import numpy as np
import pytest

from bp_pp_amd import wire

pytestmark = pytest.mark.gpu

LABELS = [b"u64 range proof", b"another protocol"]
PER_LABEL = 28
BAD_ENCODING = 1


def _need_gpu():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")


def _run_threads(n, work):
    """n threads released together; work(i) per thread; any exception fails the test"""
    errs = []
    gate = threading.Barrier(n)

    def body(i):
        try:
            gate.wait()
            work(i)
        except Exception as e:                # noqa: BLE001
            errs.append((i, repr(e)))

    th = [threading.Thread(target=body, args=(i,)) for i in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a caller hangs"
    assert not errs, errs[:3]


@pytest.fixture(scope="module")
def requests_64(oracle_c):
    """64 requests as 64 callers hold them: 28 under each of two labels and 8 on pre-loaded transcripts; every other one a wire row;
    some wrong (a proof scalar changed), some undecodable (wire rows: a bad tag; 64-byte rows: a coordinate changed).  Expected
    verdicts, statuses and transcripts come from the oracle, request by request, on the expanded bytes."""
    import transcript_cases as TC
    import workload
    gens, dl = workload.generators(), workload.generator_dlogs()
    reqs = []
    for li, label in enumerate(LABELS):
        first = 9100 + 100 * li
        x, s, rnd = workload.values(PER_LABEL, first=first), workload.blindings(PER_LABEL, first=first), workload.prover_randomness(PER_LABEL, first=first)
        P, V = oracle_c.u64_prove_trapdoor_batch(dl, label, x, s, rnd, nthreads=4)
        P, V = P.copy(), V.copy()
        for j in range(PER_LABEL):
            sec1 = (j + li) % 2 == 0
            if j % 5 == 1:
                P[j, 870 + j] ^= 1 + (j % 7)                          # a scalar changed: well-formed, wrong
            v33, p33 = wire.compress_point(bytes(V[j])), bytearray(wire.abi_to_sec1(bytes(P[j])))
            if j % 7 == 3:
                if sec1:
                    p33[33 * (j % 13)] = 0x04                          # a tag k256 refuses
                else:
                    P[j, 64 * (j % 13) + 7] ^= 0x20                    # a coordinate changed: off the curve
            v64, p64 = (wire.expand(v33, 1)[0].tobytes(), wire.expand(bytes(p33), 13, 3)[0].tobytes()) if sec1 else (bytes(V[j]), bytes(P[j]))
            rc = oracle_c.u64_verify(gens, label, v64, p64)
            reqs.append(dict(label=label, sec1=sec1, V=v33 if sec1 else v64, P=bytes(p33) if sec1 else p64, V64=v64, P64=p64,
                             accept=1 if rc == 1 else 0, flagged=rc < 0))
    tc = TC.make(8)
    assert tc["gens"] == gens
    for j in range(8):
        sec1 = j % 2 == 0
        state, v64, p64 = bytes(tc["states_in"][j]), bytes(tc["V"][j]), bytearray(tc["P"][j])
        if j == 3 or j == 4:
            p64[900] ^= 8                                              # wrong: the transcript still advances
        v33, p33 = wire.compress_point(v64), bytearray(wire.abi_to_sec1(bytes(p64)))
        if j == 6:
            p33[33 * 9:33 * 10] = b"\x02" + bytes(32)                  # `02 || 0`: never entered, the transcript stays
            p64 = wire.expand(bytes(p33), 13, 3)[0].tobytes()
        if j in (3, 4):
            ok, after = TC.oracle_verify(tc, j, v64, bytes(p64), state)
            assert not ok
        elif j == 6:
            ok, after = False, state
        else:
            ok, after = True, bytes(tc["states_after"][j])
        reqs.append(dict(state=state, sec1=sec1, V=v33 if sec1 else v64, P=bytes(p33) if sec1 else bytes(p64), V64=v64, P64=bytes(p64),
                         accept=int(ok), flagged=j == 6, after=after))
    assert len(reqs) == 64 and sum(r["sec1"] for r in reqs) == 32
    assert sum(r["flagged"] for r in reqs) >= 8 and sum(1 for r in reqs if not r["accept"] and not r["flagged"]) >= 8
    return reqs


@pytest.fixture(scope="module")
def proto():
    _need_gpu()
    import workload
    from bp_pp_amd import U64RangeProofProtocol
    g, gv, hv = workload.split_generators(workload.generators())
    p = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=8)
    yield p
    p.close()


def test_64_threads_mix_wire_and_64_byte_callers_on_one_context(proto, requests_64):
    from bp_pp_amd.transcript import Transcript
    reqs = requests_64
    out = [None] * len(reqs)

    def work(i):
        r = reqs[i]
        call = proto.verify_one_sec1 if r["sec1"] else proto.verify_one
        if "state" in r:
            tr = Transcript(state=r["state"])
            acc, st = call(r["V"], r["P"], tr)
            out[i] = (acc, st, tr.state)
        else:
            out[i] = call(r["V"], r["P"], r["label"]) + (None,)

    before = proto.coalesce_stats("verify_sec1"), proto.coalesce_stats("verify")
    _run_threads(len(reqs), work)
    after = proto.coalesce_stats("verify_sec1"), proto.coalesce_stats("verify")
    for i, (r, (acc, st, state)) in enumerate(zip(reqs, out)):
        assert int(acc) == r["accept"] and (st != 0) == r["flagged"], (i, acc, st, r["sec1"])
        if r["flagged"]:
            assert st == BAD_ENCODING, (i, st)
        if "after" in r:
            assert state == r["after"], i
    assert after[0]["requests"] - before[0]["requests"] == 32 and after[1]["requests"] - before[1]["requests"] == 32
    assert after[0]["batches"] - before[0]["batches"] < 32           # the wire rows were gathered into batched launches
    # each wire row's answer is the batched wire-form entry point's for that row
    for label in LABELS:
        sel = [i for i, r in enumerate(reqs) if r["sec1"] and r.get("label") == label]
        V33 = np.frombuffer(b"".join(reqs[i]["V"] for i in sel), np.uint8).reshape(-1, 33)
        P33 = np.frombuffer(b"".join(reqs[i]["P"] for i in sel), np.uint8).reshape(-1, 525)
        acc, st = proto.verify_batch_sec1(V33, P33, label)
        assert [(bool(a), int(s)) for a, s in zip(acc, st)] == [out[i][:2] for i in sel], label
    # ... and for the rows on pre-loaded transcripts: the batched transcript entry point on the expanded bytes, states included
    sel = [i for i, r in enumerate(reqs) if r["sec1"] and "state" in r]
    V64 = np.frombuffer(b"".join(reqs[i]["V64"] for i in sel), np.uint8).reshape(-1, 64)
    P64 = np.frombuffer(b"".join(reqs[i]["P64"] for i in sel), np.uint8).reshape(-1, 928)
    acc, st, states = proto.verify_batch_transcript(V64, P64, [reqs[i]["state"] for i in sel])
    assert [(bool(a), int(s), bytes(t)) for a, s, t in zip(acc, st, states)] == [out[i] for i in sel]


def test_invalid_arguments_are_refused_without_touching_the_gpu(proto):
    import ctypes as C
    from bp_pp_amd import _capi
    L = _capi.lib()
    acc, st = C.c_uint8(9), C.c_int32(9)
    bad_state = bytearray(203)
    bad_state[200] = 166
    buf = C.create_string_buffer(bytes(bad_state), 203)
    assert L.bppp_u64_verify_one_sec1_transcript(proto._ctx, buf, bytes(33), bytes(525), C.byref(acc), C.byref(st)) == _capi.ERR_INVALID_ARG
    assert L.bppp_u64_verify_one_sec1(proto._ctx, b"l", 1, None, bytes(525), C.byref(acc), C.byref(st)) == _capi.ERR_INVALID_ARG
    assert L.bppp_u64_verify_one_sec1(None, b"l", 1, bytes(33), bytes(525), C.byref(acc), C.byref(st)) == _capi.ERR_INVALID_ARG
    assert L.bppp_u64_verify_one_sec1(proto._ctx, b"l", C.c_size_t(1 << 32), bytes(33), bytes(525), C.byref(acc), C.byref(st)) == _capi.ERR_INVALID_ARG
    assert acc.value == 9 and st.value == 9
    with pytest.raises(ValueError):
        proto.verify_one_sec1(bytes(64), bytes(525), b"label")
    with pytest.raises(ValueError):
        proto.verify_one_sec1(bytes(33), bytes(928), b"label")


def test_reciprocal_verify_one_sec1_from_many_threads():
    """One shape, (8, 4): wire rows and 64-byte rows of the same shape on one context (two of its four generic front ends), label and
    transcript forms; every verdict the oracle's, every wire answer the batched wire-form entry point's, every transcript what the
    batched transcript entry point leaves for the expanded row."""
    _need_gpu()
    import recip_cases
    from bp_pp_amd.transcript import Transcript
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    nd, npp, B = 8, 4, 10
    case = recip_cases.make(nd, npp, B)
    proto = ReciprocalRangeProofProtocol(nd, npp, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        rounds, nl, nn = shape = (case["rounds"], case["nl"], case["nn"])
        NP = 5 + 2 * rounds
        P, com = case["proofs"].copy(), case["commitments"].copy()
        P[0, -1] ^= 1                                                  # wrong
        com[2] = case["commitments"][3]                                # wrong
        com33, P33 = wire.pack(com, 1), wire.pack(P, NP, nl + nn)
        P33[1, 33 * (4 + rounds):33 * (5 + rounds)] = np.frombuffer(b"\x02" + bytes(32), np.uint8)      # x[0] = `02 || 0`
        com33[5, 0] = 0x07                                             # a bad tag on a commitment
        com64, P64 = wire.expand(com33, 1), wire.expand(P33, NP, nl + nn)
        exp = [recip_cases.oracle_verify(case, bytes(com64[b]), bytes(P64[b])) for b in range(B)]
        assert [b for b in range(B) if exp[b] != 1] == [0, 1, 2, 5] and [b for b in range(B) if exp[b] < 0] == [1, 5]
        acc_b, st_b = proto.verify_batch_sec1(case["label"], com33, P33, *shape)
        _, _, ref_states = proto.verify_batch(b"", com64, P64, *shape, transcripts=[Transcript(case["label"]) for _ in range(B)])
        S = [Transcript(case["label"]) for _ in range(2 * B)]
        out = [None] * (4 * B)

        def work(t):
            for i in range(t, 4 * B, 8):
                b, form = i % B, i // B                                # form 0, 1: wire rows (label, transcript); 2, 3: 64-byte rows
                if form == 0:
                    out[i] = proto.verify_one_sec1(bytes(com33[b]), bytes(P33[b]), *shape, case["label"])
                elif form == 1:
                    out[i] = proto.verify_one_sec1(bytes(com33[b]), bytes(P33[b]), *shape, S[b])
                elif form == 2:
                    out[i] = proto.verify_one(bytes(com64[b]), bytes(P64[b]), *shape, case["label"])
                else:
                    out[i] = proto.verify_one(bytes(com64[b]), bytes(P64[b]), *shape, S[B + b])

        _run_threads(8, work)
        for i in range(4 * B):
            b = i % B
            acc, st = out[i]
            assert int(acc) == (1 if exp[b] == 1 else 0) and (st != 0) == (exp[b] < 0), (i, out[i], exp[b])
            assert (int(acc), st) == (int(acc_b[b]), int(st_b[b])), (i, out[i])
        fresh = Transcript(case["label"]).state
        for b in range(B):
            assert S[b].state == S[B + b].state == bytes(ref_states[b]), b
            assert (S[b].state == fresh) == (exp[b] < 0), b            # untouched exactly where the row was undecodable
        with pytest.raises(ValueError):
            proto.verify_one_sec1(bytes(33), bytes(P33[0][:-1]), *shape, b"label")
    finally:
        proto.close()


def test_destroy_with_wire_callers_inside_drains(oracle_c):
    """bppp_ctx_destroy while wire-form and 64-byte callers are asleep inside their front ends (a deadline of 1 s keeps them there):
    those calls complete with their proper verdicts, woken by the drain; callers that keep calling while the context goes away get
    their verdict or BPPP_ERR_CLOSED, never anything else, and nobody hangs."""
    _need_gpu()
    import ctypes as C
    import time
    import workload
    from bp_pp_amd import U64RangeProofProtocol, _capi
    g, gv, hv = workload.split_generators(workload.generators())
    _, V, P, _ = workload.make_batch(8, first=9300)
    P = P.copy()
    P[3, 900] ^= 1
    V33, P33 = wire.pack(V, 1), wire.pack(P, 13, 3)
    P33[6, 0] = 0x09                                                   # undecodable
    want33 = [(0, 0, BAD_ENCODING) if t == 6 else (0, 0 if t == 3 else 1, 0) for t in range(8)]      # (return code, accept, status)
    want64 = [(0, 0 if t == 3 else 1, 0) for t in range(8)]
    L = _capi.lib()
    label = workload.LABEL

    def one(ctx, t, sec1):
        acc, st = C.c_uint8(7), C.c_int32(0)
        if sec1:
            rc = L.bppp_u64_verify_one_sec1(ctx, label, len(label), V33[t].tobytes(), P33[t].tobytes(), C.byref(acc), C.byref(st))
        else:
            rc = L.bppp_u64_verify_one(ctx, label, len(label), V[t].tobytes(), P[t].tobytes(), C.byref(acc), C.byref(st))
        return rc, acc.value, st.value

    # (1) callers asleep inside both front ends when the destroy comes
    p = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=4)
    ctx = p._ctx.value
    p.set_option("coalesce_us", 1_000_000)                             # (the callers below create the two front ends themselves)
    results = [None] * 16
    th = [threading.Thread(target=lambda t=t: results.__setitem__(t, one(ctx, t % 8, t < 8))) for t in range(16)]
    t0 = time.time()
    for t in th:
        t.start()
    # The one wait of this file, as in tests/test_gpu_coalesce.py: the destroy must find the sixteen INSIDE (a call started after it
    # returned would be the caller's error), and nothing outside the library tells when they are.
    time.sleep(0.25)
    assert results == [None] * 16                                      # asleep behind the 1 s deadline
    p.close()                                                          # destroy with callers inside: drains both front ends
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th), "a caller hangs"
    assert time.time() - t0 < 0.9                                      # woken by the drain, not by the deadline
    assert results[:8] == want33 and results[8:] == want64, results

    # (2) callers that keep calling while the context is destroyed
    p = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=4)
    ctx = p._ctx.value
    p.set_option("coalesce_us", 50)
    assert one(ctx, 0, True) == (0, 1, 0)
    gate = threading.Lock()
    state = {"stop": False}
    seen, bad = {"ok": 0, "closed": 0}, []

    def loop(t):
        k = t
        while True:
            with gate:                                                 # a call is only started while the context is certainly alive
                if state["stop"]:
                    return
            r = one(ctx, k % 8, t % 2 == 0)
            if r[0] == _capi.ERR_CLOSED:
                seen["closed"] += 1
                return                                                 # the context is gone: no further call
            if r != (want64 if t % 2 else want33)[k % 8]:
                bad.append((t, k, r))
                return
            seen["ok"] += 1
            k += 1

    th = [threading.Thread(target=loop, args=(t,)) for t in range(12)]
    for t in th:
        t.start()
    while seen["ok"] < 48 and not bad and any(t.is_alive() for t in th):
        threading.Event().wait(0.002)
    with gate:
        state["stop"] = True
    p.close()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th), "a caller hangs"
    assert not bad, bad[:5]
