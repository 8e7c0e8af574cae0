"""CPU tier for the generic ArithmeticCircuit::verify device code (circuit_core.h + wnla_core.h compiled for the host) against
the oracle: the reference's own `ac_works` statement (tests.rs:45-136), k = 2 with every partition type, the f_m path, and the
f_l + f_m shape whose intermediate values (C0, c) are compared with the big-integer oracle because neither side accepts it -- and the
shape family of circuit_cases.FAMILY (k up to 61: every chunk size and chunk count of circuit_c0_var; NH = 32; NG with and without
padding; no w_o; no flag; f_m with nv > 1; f_l + f_m at k = 5), every statement of it on its accept bits, on C0 and all NH entries of c,
and on the prover's bytes."""
import numpy as np
import pytest

import bppp_oracle as O
import circuit_cases
from emul.build import load


def _table(L, case, W=4):
    gens = case["g"] + b"".join(case["gv"]) + b"".join(case["gv_"]) + b"".join(case["hv"]) + b"".join(case["hv_"])
    NB = 1 + case["NG"] + case["NH"]
    tab = np.zeros(L.emul_fb_table_entries(NB, W) * 64, dtype=np.uint8)
    assert L.emul_fb_build(gens, NB, W, tab.ctypes.data) == 0
    return tab, W


def _run(L, case, tab, W, com, proofs, want_mid=False):
    B = com.shape[0]
    acc, st = np.zeros(B, np.uint8), np.zeros(B, np.int32)
    com, proofs = np.ascontiguousarray(com), np.ascontiguousarray(proofs)
    c0 = np.zeros((B, 64), np.uint8)
    cv = np.zeros((B, case["NH"], 32), np.uint8)
    p = case["parts"]
    rc = L.emul_circuit_verify(tab.ctypes.data, W, case["NG"], case["NH"], case["dims"], int(case["f_l"]), int(case["f_m"]),
                               case["Wm_bytes"], case["Wl_bytes"], case["am_bytes"], case["al_bytes"], p["LO"].ctypes.data,
                               p["LL"].ctypes.data, p["LR"].ctypes.data, p["NO"].ctypes.data, case["label"], len(case["label"]), B,
                               com.ctypes.data, proofs.ctypes.data, case["rounds"], case["pl"], case["pn"], acc.ctypes.data,
                               st.ctypes.data, c0.ctypes.data if want_mid else None, cv.ctypes.data if want_mid else None)
    assert rc == 0
    return (acc, st, c0, cv) if want_mid else (acc, st)


@pytest.mark.parametrize("name", ["ac_works", "mixed_k2", "fm_nv1"])
def test_generic_circuit_verify_vs_oracle(name):
    L = load()
    case = circuit_cases.make(name, B=3)
    tab, W = _table(L, case)
    acc, st = _run(L, case, tab, W, case["commitments"], case["proofs"])
    assert acc.tolist() == [1, 1, 1] and not st.any()
    # tampered: last scalar, a commitment swapped between instances, c_s replaced by c_l
    P = case["proofs"].copy()
    P[0, -1] ^= 1
    P[2, 192:256] = P[2, 0:64]
    com = case["commitments"].copy()
    com[1, 0] = case["commitments"][0, 0]
    acc, st = _run(L, case, tab, W, com, P)
    exp = [circuit_cases.oracle_verify(case, com[b].tobytes(), P[b].tobytes()) for b in range(3)]
    assert acc.tolist() == exp == [0, 0, 0] and not st.any()
    P = case["proofs"].copy()
    P[1, 70] ^= 1                                  # c_r off the curve
    acc, st = _run(L, case, tab, W, case["commitments"], P)
    assert st.tolist() == [0, 1, 0] and acc.tolist() == [1, 0, 1]


def _oracle_circuit(case):
    pts = lambda lst: [O.pt_from_xy64(b) for b in lst]
    part = lambda typ, j: (None if case["part"][typ][j] < 0 else case["part"][typ][j])
    return O.ArithmeticCircuit(dim_nm=case["nm"], dim_no=case["no"], k=case["k"], dim_nl=case["nl"], dim_nv=case["nv"], dim_nw=case["nw"],
                               g=O.pt_from_xy64(case["g"]), g_vec=pts(case["gv"]), h_vec=pts(case["hv"]), W_m=case["W_m"], W_l=case["W_l"],
                               a_m=case["a_m"], a_l=case["a_l"], f_l=case["f_l"], f_m=case["f_m"], g_vec_=pts(case["gv_"]),
                               h_vec_=pts(case["hv_"]), partition=part)


def test_complete_table_is_the_oracles_verdict():
    """circuit_cases.COMPLETE is the C oracle's verdict on its own prover's output, statement by statement; every launch form the family
    is there for has a statement the verifier ACCEPTS (a form reached by rejected proofs only would be compared on a verdict of 0), and at
    most four statements of the family are incomplete."""
    assert set(circuit_cases.COMPLETE) == set(circuit_cases.STATEMENTS)
    for name in circuit_cases.STATEMENTS:
        case = circuit_cases.make(name, B=2)
        got = [circuit_cases.oracle_verify(case, case["commitments"][b].tobytes(), case["proofs"][b].tobytes()) for b in range(2)]
        assert got == [int(circuit_cases.COMPLETE[name])] * 2, name
    required = {"k4", "k5", "k11", "k13", "k60", "k61", "nv8", "nm5", "nm8", "nm16", "nof", "fm_nv2", "fl_fm_k5"}
    assert required <= set(circuit_cases.FAMILY)
    assert set(circuit_cases.LAUNCH_FORMS) == {"L=8", "L=16", "L=32", "L=64", "one lane past 64 points", "NH=32", "NG padded", "NG exact", "no flag"}
    for form, names in circuit_cases.LAUNCH_FORMS.items():
        assert any(circuit_cases.COMPLETE[n] for n in names), form
    assert sum(1 for n in circuit_cases.FAMILY if not circuit_cases.COMPLETE[n]) <= 4
    assert all(circuit_cases.COMPLETE[n] for n in ("k5", "k11"))
    # the forms are what the statements' dimensions say they are
    for name, fn in circuit_cases.FAMILY.items():
        nm, no, nv, k = fn.dims
        st = fn()
        assert (st["nm"], st["no"], st["nv"], st["k"]) == (nm, no, nv, k)
    dims = lambda n: circuit_cases.FAMILY[n].dims
    assert [4 + dims(n)[3] for n in ("k4", "k5", "k11", "k13", "k60", "k61")] == [8, 9, 15, 17, 64, 65]
    assert [circuit_cases.c0_lanes(n) for n in ("k4", "k5", "k11", "k13", "k60", "k61", "fl_fm_k5")] == [8, 16, 16, 32, 64, 128, 16]
    assert dims("nv8")[2] + 9 > 16 and dims("k13")[1] == 0
    assert [dims(n)[0] for n in ("nm5", "nm7", "nm8", "nm16")] == [5, 7, 8, 16]


@pytest.mark.parametrize("name", list(circuit_cases.FAMILY))
def test_family_verify_vs_oracle(name):
    """Accept bits of the host build against the C oracle's at every family statement: honest instances (accepted exactly where
    COMPLETE says so), the three tampers of test_generic_circuit_verify_vs_oracle, and the status bit of an off-curve point."""
    L = load()
    B = 3
    case = circuit_cases.make(name, B=B)
    tab, W = _table(L, case)
    ov = lambda com, P: [circuit_cases.oracle_verify(case, com[b].tobytes(), P[b].tobytes()) for b in range(B)]
    acc, st = _run(L, case, tab, W, case["commitments"], case["proofs"])
    honest = ov(case["commitments"], case["proofs"])
    assert acc.tolist() == honest == [int(circuit_cases.COMPLETE[name])] * B and not st.any()
    P = case["proofs"].copy()
    P[0, -1] ^= 1
    P[2, 192:256] = P[2, 0:64]
    com = case["commitments"].copy()
    com[1, 0] = case["commitments"][0, 0]
    acc, st = _run(L, case, tab, W, com, P)
    assert acc.tolist() == ov(com, P) == [0, 0, 0] and not st.any()
    P = case["proofs"].copy()
    P[1, 70] ^= 1                                  # c_r off the curve
    acc, st = _run(L, case, tab, W, case["commitments"], P)
    assert st.tolist() == [0, 1, 0] and acc.tolist() == [honest[0], 0, honest[2]]


@pytest.mark.parametrize("name", ["fl_fm", "mixed_k2"] + list(circuit_cases.FAMILY))
def test_circuit_intermediates_vs_bigint_oracle(name):
    """C0 (circuit.rs:230-235) and the c vector (circuit.rs:208-229) of the device code against the Python big-integer
    restatement's trace -- the check that still bites where the accept bit is 0 on both sides."""
    L = load()
    case = circuit_cases.make(name, B=2)
    tab, W = _table(L, case)
    acc, st, c0, cv = _run(L, case, tab, W, case["commitments"], case["proofs"], want_mid=True)
    circ = _oracle_circuit(case)
    R = case["rounds"]
    for b in range(2):
        pr = case["proofs"][b].tobytes()
        P = lambda i: O.pt_from_xy64(pr[64 * i:64 * i + 64])
        sc_at = lambda o: int.from_bytes(pr[o:o + 32], "big")
        off = 64 * (4 + 2 * R)
        proof = O.CircuitProof(c_l=P(0), c_r=P(1), c_o=P(2), c_s=P(3), r=[P(4 + i) for i in range(R)], x=[P(4 + R + i) for i in range(R)],
                               l=[sc_at(off + 32 * i) for i in range(case["pl"])],
                               n=[sc_at(off + 32 * case["pl"] + 32 * i) for i in range(case["pn"])])
        v = [O.pt_from_xy64(case["commitments"][b, i].tobytes()) for i in range(case["k"])]
        trace = []
        ok = circ.verify(v, O.Transcript(case["label"]), proof, trace)
        tr = dict((k_, v_) for k_, v_ in trace if isinstance(k_, str))
        assert c0[b].tobytes() == O.pt_to_xy64(tr["C0"])
        exp_c = list(tr["c"]) + [0] * (case["NH"] - len(tr["c"]))
        assert [int.from_bytes(cv[b, i].tobytes(), "big") for i in range(case["NH"])] == exp_c
        assert int(acc[b]) == int(ok) == circuit_cases.oracle_verify(case, case["commitments"][b].tobytes(), pr)
    assert not st.any()


@pytest.mark.parametrize("name", ["ac_works", "mixed_k2", "fm_nv1", "fl_fm"] + list(circuit_cases.FAMILY))
def test_generic_circuit_prove_is_byte_identical_to_the_oracle(name):
    """circuit.rs:260-556 + wnla.rs:125-190 on the device code: for the same witness and the same sequence of prover scalars the
    proof bytes must equal the reference-shaped prover's (incl. the f_l + f_m shape, whose proofs neither side's verifier accepts)."""
    L = load()
    B = 2
    case = circuit_cases.make(name, B=B)
    tab, W = _table(L, case)
    p = case["parts"]
    proofs = np.zeros((B, case["proof_bytes"]), np.uint8)
    st = np.zeros(B, np.int32)
    c = {k_: np.ascontiguousarray(case[k_]) for k_ in ("commitments", "v_bytes", "s_v", "wl_bytes", "wr_bytes", "wo_bytes", "rnd")}
    rc = L.emul_circuit_prove(tab.ctypes.data, W, case["NG"], case["NH"], case["dims"], int(case["f_l"]), int(case["f_m"]), case["Wm_bytes"],
                              case["Wl_bytes"], case["am_bytes"], case["al_bytes"], p["LO"].ctypes.data, p["LL"].ctypes.data,
                              p["LR"].ctypes.data, p["NO"].ctypes.data, case["label"], len(case["label"]), B, c["commitments"].ctypes.data,
                              c["v_bytes"].ctypes.data, c["s_v"].ctypes.data, c["wl_bytes"].ctypes.data, c["wr_bytes"].ctypes.data,
                              c["wo_bytes"].ctypes.data if case["no"] else None, c["rnd"].ctypes.data, proofs.ctypes.data, st.ctypes.data)
    assert rc == case["proof_bytes"] and not st.any()
    for b in range(B):
        got, exp = proofs[b].tobytes(), case["proofs"][b].tobytes()
        assert got[:256] == exp[:256], "c_l, c_r, c_o, c_s"
        assert got == exp
