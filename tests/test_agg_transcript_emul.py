"""The aggregate's caller-transcript device code on the host (tests/emul/agg_transcript_emul.cpp: agg_phase1<true>, the WNLA stage with
tio set, tio_export; agg_prove_stage_r1<true>, the circuit and WNLA provers, agg_prove_export) against the oracle on the same pre-loaded
transcripts (tests/agg_transcript_cases.py), at shapes (2, 4, 4) and (6, 2, 3), for each pre-loaded state of the golden pool -- the six
positions of the mixed batch and the shared state:
    verifier  every challenge and commitment of the oracle's trace (e through rho, mu, the c vector, ps_tau, pn_tau, C0), accept and
              status, and the exported 203 bytes; corrupted rows by class; a state merlin cannot be in
    prover    proofs and commitments byte-identical to the oracle's prove on the same transcript and draws, and the exported state"""
import json
import os

import numpy as np
import pytest

import agg_cases as A
import agg_golden
import agg_prove_cases as AP
import agg_transcript_cases as AT
import bppp_oracle as O
from emul.build import load as load_emul
from emul.build_agg_transcript import load as load_tx

SHAPES = [(2, 4, 4), (6, 2, 3)]
W = 4
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_transcript_cases.json")
_tables, _pool = {}, {}


def _table(case):
    key = (case["k"], case["nd"])
    if key not in _tables:
        L = load_emul()
        NB = 1 + case["NG"] + case["NH"]
        tab = np.zeros(L.emul_fb_table_entries(NB, W) * 64, dtype=np.uint8)
        assert L.emul_fb_build(agg_golden.generators(case), NB, W, tab.ctypes.data) == 0
        _tables[key] = tab
    return _tables[key]


def _u8(blobs, *shape):
    return np.frombuffer(b"".join(blobs), np.uint8).reshape(len(blobs), *shape).copy()


def pool(shape):
    """(case, b [P], C [P, k, 64], Q [P, pb], S_in [P, 203], S_out [P, 203], corrupted): the mixed entries, then the shared ones."""
    if shape not in _pool:
        with open(PATH) as f:
            g = json.load(f)["%d,%d,%d" % shape]
        case = A.setup(*shape)
        es = g["mixed"] + g["shared"]
        S = [AT.mixed_state(case, i) for i in range(len(g["mixed"]))] + [AT.shared_state(case)] * len(g["shared"])
        _pool[shape] = (case, [e["b"] for e in es], _u8([bytes.fromhex(e["commitments"]) for e in es], shape[0], 64),
                        _u8([bytes.fromhex(e["proof"]) for e in es], case["proof_bytes"]), _u8(S, 203),
                        _u8([bytes.fromhex(e["state_out"]) for e in es], 203), g["corrupted"])
    return _pool[shape]


def verify(case, S, C, Q, G=1):
    L = load_tx()
    n, k, nm, NH = C.shape[0], case["k"], case["nm"], case["NH"]
    S, C, Q = np.ascontiguousarray(S), np.ascontiguousarray(C), np.ascontiguousarray(Q)
    assert S.shape[0] in (1, n) and Q.shape == (n, case["proof_bytes"])
    out = dict(rho=np.zeros((n, 32), np.uint8), mu=np.zeros((n, 32), np.uint8), c=np.zeros((n, NH, 32), np.uint8),
               pn=np.zeros((n, nm + 1, 32), np.uint8), c0=np.zeros((n, 64), np.uint8), p1=np.zeros(n, np.int32),
               acc=np.zeros(n, np.uint8), st=np.full(n, 7, np.int32), states=np.full((n, 203), 0xEE, np.uint8))
    tab = _table(case)
    rc = L.emul_aggtx_verify(tab.ctypes.data, W, case["NG"], NH, k, case["nd"], case["np"], S.ctypes.data, S.shape[0], n, C.ctypes.data,
                             Q.ctypes.data, case["rounds"], case["nl"], case["nn"], G, 0, out["rho"].ctypes.data, out["mu"].ctypes.data,
                             out["c"].ctypes.data, out["pn"].ctypes.data, out["c0"].ctypes.data, out["p1"].ctypes.data, out["acc"].ctypes.data,
                             out["st"].ctypes.data, out["states"].ctypes.data)
    assert rc == 0
    return out


def _sc(row):
    return int.from_bytes(row.tobytes(), "big")


def _assert_trace(case, out, i, state, com, proof):
    """Row i against the oracle's verify on `state`: the trace, the verdict, the advanced state."""
    tr = []
    t = AT.unser(state)
    assert AT.verify_on(case, t, com, proof, tr) == 1
    d = {k: v for k, v in tr if not k.startswith("wnla")}
    assert _sc(out["rho"][i]) == d["rho"] and _sc(out["mu"][i]) == d["rho"] * d["rho"] % O.N
    assert [_sc(r) for r in out["c"][i]] == d["c"]
    assert _sc(out["pn"][i, 0]) == d["ps_tau"] and [_sc(r) for r in out["pn"][i, 1:]] == d["pn_tau"]
    assert out["c0"][i].tobytes() == O.pt_to_xy64(d["C0"])
    assert out["p1"][i] == 0 and out["acc"][i] == 1 and out["st"][i] == 0
    assert out["states"][i].tobytes() == AT.ser(t)


@pytest.mark.parametrize("shape", SHAPES)
def test_verifier_trace_verdict_and_state_equal_the_oracle_for_each_preloaded_state(shape):
    case, _, C, Q, S, So, _ = pool(shape)
    nmix = len(AT.mixed_positions(case["label"]))
    assert sorted(S[:nmix, 200].tolist()) == sorted(AT.mixed_positions(case["label"])) and S[nmix, 200] == AT.SHARED_POS
    out = verify(case, S, C, Q)
    for i in range(len(Q)):
        _assert_trace(case, out, i, S[i].tobytes(), C[i].tobytes(), Q[i].tobytes())
    assert out["states"].tobytes() == So.tobytes()               # (the state the oracle's prover left: the golden file's)
    # one shared state (n_states = 1), and the lane-group form of phase 1: the same results
    sh = verify(case, S[nmix:nmix + 1], C[nmix:], Q[nmix:])
    assert sh["acc"].all() and not sh["st"].any() and sh["states"].tobytes() == So[nmix:].tobytes()
    for G in (2, 8):
        g = verify(case, S, C, Q, G)
        for key in out:
            assert g[key].tobytes() == out[key].tobytes(), (G, key)


@pytest.mark.parametrize("shape", SHAPES)
def test_corrupted_rows_and_invalid_states_get_the_oracle_verdicts_and_states(shape):
    case, _, C, Q, S, So, corrupted = pool(shape)
    C, Q, S = C.copy(), Q.copy(), S.copy()
    exp = {i: (1, 0, So[i].tobytes()) for i in range(len(Q))}
    for entry, kind, acc, flagged, sout in corrupted:
        AT.corrupt(case, C[entry], Q[entry], kind)
        exp[entry] = (acc, AT.ST_BAD_ENCODING if flagged else 0, bytes.fromhex(sout))
        assert AT.verify_state(case, S[entry].tobytes(), C[entry].tobytes(), Q[entry].tobytes()) == (acc, bool(flagged), bytes.fromhex(sout))
    # states merlin cannot be in: pos >= 166, and pos_begin > 166 at the label state's own position -- flagged, returned unchanged
    label_pos = AT.ser(O.Transcript(case["label"]))[200]
    S[4, 200] = 166
    S[5, 200], S[5, 201] = label_pos, 167
    for i in (4, 5):
        exp[i] = (0, AT.ST_BAD_ENCODING, S[i].tobytes())
        assert load_tx().emul_aggtx_position_key(S.ctypes.data, len(S), i) == 0x100
    assert load_tx().emul_aggtx_position_key(S.ctypes.data, len(S), 1) == S[1, 200] == 165
    out = verify(case, S, C, Q)
    for i, (acc, st, sout) in exp.items():
        assert (int(out["acc"][i]), int(out["st"][i])) == (acc, st), i
        assert out["states"][i].tobytes() == sout, (i, "state")


def prove(case, S, x, s, rnd):
    L = load_tx()
    n, k = x.shape[0], case["k"]
    S, x, s, rnd = (np.ascontiguousarray(a) for a in (S, x, s, rnd))
    proofs, com = np.full((n, case["proof_bytes"]), 0xEE, np.uint8), np.full((n, k, 64), 0xEE, np.uint8)
    st, out = np.full(n, 7, np.int32), np.full((n, 203), 0xEE, np.uint8)
    tab = _table(case)
    rc = L.emul_aggtx_prove(tab.ctypes.data, W, case["NG"], case["NH"], k, case["nd"], case["np"], S.ctypes.data, S.shape[0], n, x.ctypes.data,
                            s.ctypes.data, rnd.ctypes.data, proofs.ctypes.data, com.ctypes.data, st.ctypes.data, out.ctypes.data)
    assert rc == case["proof_bytes"], rc
    return proofs, com, st, out


@pytest.mark.parametrize("shape", SHAPES)
def test_prover_bytes_and_states_equal_the_oracles_for_each_preloaded_state(shape):
    case, bs, C, Q, S, So, _ = pool(shape)
    nmix = len(AT.mixed_positions(case["label"]))
    x, s, rnd = AP.batch(case, bs, load_tx().emul_aggtx_draws(case["k"], case["nd"]))
    got, gcom, st, out = prove(case, S, x, s, rnd)
    assert not st.any(), st.tolist()
    for i in range(len(bs)):
        assert gcom[i].tobytes() == C[i].tobytes() and got[i].tobytes() == Q[i].tobytes(), (shape, i, "proof")
        assert out[i].tobytes() == So[i].tobytes(), (shape, i, "state")
    # one entry proved again by the oracle itself, not read from the file
    assert AT.prove_state(case, S[1].tobytes(), bs[1]) == (C[1].tobytes(), Q[1].tobytes(), out[1].tobytes())
    # the shared state as n_states = 1
    sh = prove(case, S[nmix:nmix + 1], x[nmix:], s[nmix:], rnd[nmix:])
    assert sh[0].tobytes() == Q[nmix:].tobytes() and sh[3].tobytes() == So[nmix:].tobytes() and not sh[2].any()


def test_prover_zeroed_instances_get_their_input_state_back():
    """An out-of-range value, and a state merlin cannot be in: zeroed proof and commitments, the status, the input state; the
    neighbours are the oracle's."""
    shape = (2, 4, 4)
    case, bs, C, Q, S, So, _ = pool(shape)
    x, s, rnd = AP.batch(case, bs, load_tx().emul_aggtx_draws(case["k"], case["nd"]))
    x, S = x.copy(), S.copy()
    x[2, 1] = np.frombuffer((4**4).to_bytes(32, "big"), np.uint8)
    S[3, 200] = 200
    got, gcom, st, out = prove(case, S, x, s, rnd)
    assert st.tolist() == [0, 0, AT.ST_OUT_OF_RANGE, AT.ST_BAD_ENCODING] + [0] * (len(bs) - 4)
    for i in (2, 3):
        assert not got[i].any() and not gcom[i].any() and out[i].tobytes() == S[i].tobytes()
    keep = [i for i in range(len(bs)) if i not in (2, 3)]
    assert got[keep].tobytes() == Q[keep].tobytes() and gcom[keep].tobytes() == C[keep].tobytes() and out[keep].tobytes() == So[keep].tobytes()
