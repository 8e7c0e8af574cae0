"""GPU tests of the generic proofs' wire form (include/bppp.h: bppp_{reciprocal,circuit,wnla}_{verify,prove}_batch_sec1[_device]): the
33-byte SEC1 forms give exactly the accept bits and statuses of the 64-byte twins on the expanded input -- for clean and tampered
batches, undecodable points in every position, batch sizes that leave a ragged tail of the flat lane map, the reciprocal call split
into parts -- and the provers' wire output is the 64-byte provers' output compressed."""
import functools

import numpy as np
import pytest

from bp_pp_amd import wire

pytestmark = pytest.mark.gpu

OFF = bytes(31) + b"\x01" + bytes(32)      # what an undecodable point expands to: (1, 0), off the curve


def _need_gpu():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")


def _nonresidue_x() -> int:
    x = 1
    while pow((x ** 3 + 7) % wire.P, (wire.P - 1) // 2, wire.P) != wire.P - 1:
        x += 1
    return x


def bad_encodings(valid33: bytes):
    """(33-byte encoding, the 64-byte point it stands for) for every kind of damage the wire form can carry."""
    x = valid33[1:]
    return [(b"\x04" + x, OFF), (b"\x01" + x, OFF), (b"\x02" + wire.P.to_bytes(32, "big"), OFF),
            (b"\x03" + (2 ** 256 - 1).to_bytes(32, "big"), OFF), (b"\x02" + _nonresidue_x().to_bytes(32, "big"), OFF),
            (bytes(33), bytes(64))]


def pts33(a64: np.ndarray) -> np.ndarray:
    """[..., 64] points -> [..., 33]"""
    flat = a64.reshape(-1, 64)
    if flat.shape[0] == 0:
        return np.zeros((*a64.shape[:-1], 33), np.uint8)
    return np.stack([np.frombuffer(wire.compress_point(bytes(p)), np.uint8) for p in flat]).reshape(*a64.shape[:-1], 33)


def proofs33(p64: np.ndarray, n_points: int) -> np.ndarray:
    return np.stack([np.frombuffer(wire.generic_abi_to_sec1(bytes(p), n_points), np.uint8) for p in p64])


def tile(a: np.ndarray, B: int) -> np.ndarray:
    return a[np.arange(B) % a.shape[0]].copy()


def dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- reciprocal
@functools.lru_cache(maxsize=None)
def _recip_case(nd, npp):
    import recip_cases
    return recip_cases.make(nd, npp, 3 if nd > 64 else 4)


def _recip_proto(case, nd, npp):
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    return ReciprocalRangeProofProtocol(nd, npp, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0,
                                        fb_window_bits=8 if nd > 64 else 16)


def _generic_kernels(monkeypatch, on):
    if on:
        monkeypatch.setenv("BPPP_GENERIC_U64_SHAPE", "1")
    else:
        monkeypatch.delenv("BPPP_GENERIC_U64_SHAPE", raising=False)


def _recip_sec1_both(proto, label, com33, pr33, shape):
    """host form and device form of the SEC1 verifier -> (acc, st), asserting they agree"""
    acc, st = proto.verify_batch_sec1(label, com33, pr33, *shape)
    B = com33.shape[0]
    import torch
    dC, dP = dev(com33), dev(pr33)
    dA, dS = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.full((B,), 9, dtype=torch.int32, device="cuda")
    proto.verify_batch_sec1_device(label, B, dC.data_ptr(), dP.data_ptr(), *shape, dA.data_ptr(), dS.data_ptr())
    proto.synchronize()
    assert (dA.cpu().numpy() == acc).all() and (dS.cpu().numpy() == st).all()
    return acc, st


@pytest.mark.parametrize("nd,npp,generic", [(16, 16, False), (16, 16, True), (32, 16, True), (12, 10, True), (256, 16, True)])
def test_reciprocal_sec1_matches_64_byte_form_and_oracle(nd, npp, generic, monkeypatch):
    _need_gpu()
    import recip_cases
    case = _recip_case(nd, npp)
    _generic_kernels(monkeypatch, generic)
    proto = _recip_proto(case, nd, npp)
    try:
        shape = (case["rounds"], case["nl"], case["nn"])
        P = 5 + 2 * case["rounds"]
        oracle = [1 if recip_cases.oracle_verify(case, bytes(c), bytes(p)) == 1 else 0 for c, p in zip(case["commitments"], case["proofs"])]
        for B in (1, 63, 257):
            com, pr = tile(case["commitments"], B), tile(case["proofs"], B)
            for b in range(0, B, 5):
                pr[b, -1] ^= 1                                      # n0: a rejected proof
            acc64, st64 = proto.verify_batch(case["label"], com, pr, *shape)
            acc, st = _recip_sec1_both(proto, case["label"], pts33(com), proofs33(pr, P), shape)
            assert (acc == acc64).all() and (st == st64).all()
            clean = [b for b in range(B) if b % 5]
            assert [int(acc[b]) for b in clean] == [oracle[b % len(oracle)] for b in clean]
            assert not acc[::5].any()
    finally:
        proto.close()


@pytest.mark.parametrize("nd,npp,generic", [(32, 16, True), (16, 16, False)])
def test_reciprocal_sec1_undecodable_points(nd, npp, generic, monkeypatch):
    """Every kind of damage in the commitment, a head point, r[0], x[rounds-1] and the reciprocal r: the damaged instance gets the twin's
    status for (1, 0) (or the identity) in that place -- BPPP_ST_BAD_ENCODING for the undecodable ones -- and its neighbours are untouched."""
    _need_gpu()
    case = _recip_case(nd, npp)
    _generic_kernels(monkeypatch, generic)
    proto = _recip_proto(case, nd, npp)
    try:
        r = case["rounds"]
        shape = (r, case["nl"], case["nn"])
        P = 5 + 2 * r
        positions = [None, 2, 4, 4 + 2 * r - 1, 4 + 2 * r]          # commitment, c_o, r[0], x[rounds-1], reciprocal r
        damage = bad_encodings(wire.compress_point(bytes(case["commitments"][0])))
        B = 2 * len(positions) * len(damage) + 1
        com, pr = tile(case["commitments"], B), tile(case["proofs"], B)
        com33, pr33 = pts33(com), proofs33(pr, P)
        undecodable = []
        i = 1
        for pos in positions:
            for enc, pt in damage:                                  # instance i damaged, i + 1 clean
                if pos is None:
                    com33[i] = np.frombuffer(enc, np.uint8); com[i] = np.frombuffer(pt, np.uint8)
                else:
                    pr33[i, 33 * pos:33 * pos + 33] = np.frombuffer(enc, np.uint8); pr[i, 64 * pos:64 * pos + 64] = np.frombuffer(pt, np.uint8)
                if pt == OFF:
                    undecodable.append(i)
                i += 2
        acc64, st64 = proto.verify_batch(case["label"], com, pr, *shape)
        acc, st = _recip_sec1_both(proto, case["label"], com33, pr33, shape)
        assert (acc == acc64).all() and (st == st64).all()
        assert all(st[i] == 1 and acc[i] == 0 for i in undecodable)
        assert acc[0::2].all() and not st[0::2].any()
    finally:
        proto.close()


def test_reciprocal_sec1_in_parts_equals_one_part():
    """generic_parts = 2 on a batch of 2 x 256 and more: the parts fork from the context's stream behind the expand kernel."""
    _need_gpu()
    import torch
    case = _recip_case(32, 16)
    proto = _recip_proto(case, 32, 16)
    try:
        shape = (case["rounds"], case["nl"], case["nn"])
        B = 600
        com, pr = tile(case["commitments"], B), tile(case["proofs"], B)
        for b in (0, 255, 256, 299, 300, 301, B - 1):
            pr[b, -1] ^= 1
        com33, pr33 = pts33(com), proofs33(pr, 5 + 2 * case["rounds"])
        pr33[257, 33 * 4] = 0x04                                     # an undecodable r[0]
        dC, dP = dev(com33), dev(pr33)
        res = {}
        for k in (1, 2):
            proto.set_option("generic_parts", k)
            dA = torch.zeros(B, dtype=torch.uint8, device="cuda"); dS = torch.full((B,), 9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            proto.verify_batch_sec1_device(case["label"], B, dC.data_ptr(), dP.data_ptr(), *shape, dA.data_ptr(), dS.data_ptr())
            proto.synchronize()
            res[k] = (dA.cpu().numpy(), dS.cpu().numpy())
        assert (res[1][0] == res[2][0]).all() and (res[1][1] == res[2][1]).all()
        acc, st = res[2]
        assert acc.sum() == B - 8 and st[257] == 1 and st.sum() == 1
    finally:
        proto.close()


@pytest.mark.parametrize("nd,npp", [(32, 16), (16, 16)])
def test_reciprocal_prove_sec1(nd, npp):
    _need_gpu()
    case = _recip_case(nd, npp)
    proto = _recip_proto(case, nd, npp)
    try:
        args = (case["x"], case["s"], case["digits"], case["m"], case["rnd"])
        com = case["commitments"]
        proofs, st, shape = proto.prove_batch(case["label"], com, *args)
        assert not st.any()
        P = 5 + 2 * shape[0]
        com33 = pts33(com)
        p33, st33, shape33 = proto.prove_batch_sec1(case["label"], com33, *args)
        assert shape33 == shape and not st33.any()
        assert (p33 == proofs33(proofs, P)).all()
        acc, st = proto.verify_batch_sec1(case["label"], com33, p33, *shape)
        assert acc.all() and not st.any()
        # an undecodable commitment: the 64-byte prover's answer for (1, 0) there -- BPPP_ST_BAD_ENCODING, a zeroed proof
        bad, bad64 = com33.copy(), com.copy()
        bad[1, 0] = 0x04
        bad64[1] = np.frombuffer(OFF, np.uint8)
        p33b, st33b, _ = proto.prove_batch_sec1(case["label"], bad, *args)
        p64b, st64b, _ = proto.prove_batch(case["label"], bad64, *args)
        assert (st33b == st64b).all() and (p33b == proofs33(p64b, P)).all()
        assert st33b[1] == 1 and not p33b[1].any() and not np.delete(st33b, 1).any()
        assert (np.delete(p33b, 1, axis=0) == np.delete(p33, 1, axis=0)).all()
    finally:
        proto.close()


# ---------------------------------------------------------------------------------------------------------------- circuit
@functools.lru_cache(maxsize=None)
def _circuit_case(name):
    import circuit_cases
    return circuit_cases.make(name, 3)


def _circuit(case):
    from bp_pp_amd.wnla import ArithmeticCircuit
    part = lambda typ, j: (None if case["part"][typ][j] < 0 else int(case["part"][typ][j]))
    arr = lambda b: np.frombuffer(b, np.uint8).reshape(-1, 32)
    return ArithmeticCircuit(case["nm"], case["no"], case["k"], case["nv"], case["g"], case["gv"], case["hv"], arr(case["Wm_bytes"]),
                             arr(case["Wl_bytes"]), arr(case["am_bytes"]), arr(case["al_bytes"]), case["f_l"], case["f_m"], case["gv_"],
                             case["hv_"], part, device=0, fb_window_bits=16)


def _circuit_sec1_both(circ, label, com33, pr33, shape):
    acc, st = circ.verify_batch_sec1(label, com33, pr33, *shape)
    B = com33.shape[0]
    import torch
    dC, dP = dev(com33), dev(pr33)
    dA, dS = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.full((B,), 9, dtype=torch.int32, device="cuda")
    circ.verify_batch_sec1_device(label, B, dC.data_ptr(), dP.data_ptr(), *shape, dA.data_ptr(), dS.data_ptr())
    circ.synchronize()
    assert (dA.cpu().numpy() == acc).all() and (dS.cpu().numpy() == st).all()
    return acc, st


@pytest.mark.parametrize("name", ["ac_works", "mixed_k2", "fl_fm", "fm_nv1"])
def test_circuit_sec1_matches_64_byte_form_and_oracle(name):
    _need_gpu()
    import circuit_cases
    case = _circuit_case(name)
    circ = _circuit(case)
    try:
        shape = (case["rounds"], case["pl"], case["pn"])
        P = 4 + 2 * case["rounds"]
        oracle = [1 if circuit_cases.oracle_verify(case, bytes(c), bytes(p)) == 1 else 0 for c, p in zip(case["commitments"], case["proofs"])]
        for B in (1, 63, 257):
            com, pr = tile(case["commitments"], B), tile(case["proofs"], B)
            for b in range(0, B, 5):
                pr[b, -1] ^= 1
            acc64, st64 = circ.verify_batch(case["label"], com, pr, *shape)
            acc, st = _circuit_sec1_both(circ, case["label"], pts33(com), proofs33(pr, P), shape)
            assert (acc == acc64).all() and (st == st64).all()
            clean = [b for b in range(B) if b % 5]
            assert [int(acc[b]) for b in clean] == [oracle[b % len(oracle)] for b in clean]
    finally:
        circ.close()


def test_circuit_sec1_undecodable_points():
    _need_gpu()
    case = _circuit_case("mixed_k2")
    circ = _circuit(case)
    try:
        r, k = case["rounds"], case["k"]
        shape = (r, case["pl"], case["pn"])
        P = 4 + 2 * r
        positions = [None, 2, 4, 4 + 2 * r - 1]                      # commitment v[k-1], c_o, r[0], x[rounds-1]
        damage = bad_encodings(wire.compress_point(bytes(case["commitments"][0, 0])))
        B = 2 * len(positions) * len(damage) + 1
        com, pr = tile(case["commitments"], B), tile(case["proofs"], B)
        com33, pr33 = pts33(com), proofs33(pr, P)
        undecodable, i = [], 1
        for pos in positions:
            for enc, pt in damage:
                if pos is None:
                    com33[i, k - 1] = np.frombuffer(enc, np.uint8); com[i, k - 1] = np.frombuffer(pt, np.uint8)
                else:
                    pr33[i, 33 * pos:33 * pos + 33] = np.frombuffer(enc, np.uint8); pr[i, 64 * pos:64 * pos + 64] = np.frombuffer(pt, np.uint8)
                if pt == OFF:
                    undecodable.append(i)
                i += 2
        acc64, st64 = circ.verify_batch(case["label"], com, pr, *shape)
        acc, st = _circuit_sec1_both(circ, case["label"], com33, pr33, shape)
        assert (acc == acc64).all() and (st == st64).all()
        assert all(st[i] == 1 and acc[i] == 0 for i in undecodable)
        assert acc[0::2].all() and not st[0::2].any()
    finally:
        circ.close()


@pytest.mark.parametrize("name", ["ac_works", "mixed_k2"])
def test_circuit_prove_sec1(name):
    _need_gpu()
    case = _circuit_case(name)
    circ = _circuit(case)
    try:
        args = (case["v_bytes"], case["s_v"], case["wl_bytes"], case["wr_bytes"], case["wo_bytes"], case["rnd"])
        com = case["commitments"]
        proofs, st, shape = circ.prove_batch(case["label"], com, *args)
        assert not st.any()
        com33 = pts33(com)
        p33, st33, shape33 = circ.prove_batch_sec1(case["label"], com33, *args)
        assert shape33 == shape and not st33.any()
        assert (p33 == proofs33(proofs, 4 + 2 * shape[0])).all()
        acc, st = circ.verify_batch_sec1(case["label"], com33, p33, *shape)
        assert acc.all() and not st.any()
        bad, bad64 = com33.copy(), com.copy()
        bad[0, 0, 1:] = np.frombuffer(wire.P.to_bytes(32, "big"), np.uint8)      # x = p
        bad64[0, 0] = np.frombuffer(OFF, np.uint8)
        p33b, st33b, _ = circ.prove_batch_sec1(case["label"], bad, *args)
        p64b, st64b, _ = circ.prove_batch(case["label"], bad64, *args)
        assert (st33b == st64b).all() and (p33b == proofs33(p64b, 4 + 2 * shape[0])).all()
        assert st33b[0] == 1 and not p33b[0].any() and not st33b[1:].any() and (p33b[1:] == p33[1:]).all()
    finally:
        circ.close()


# ---------------------------------------------------------------------------------------------------------------- WNLA
@functools.lru_cache(maxsize=None)
def _wnla_case(ng, nh):
    import wnla_cases
    return wnla_cases.make(ng, nh, 3)


def _wnla(case):
    from bp_pp_amd.wnla import WeightNormLinearArgument
    return WeightNormLinearArgument(case["g"], case["gv"], case["hv"], device=0, fb_window_bits=8 if case["nh"] > 64 else 16)


def _wnla_sec1_both(w, case, B, com33, r33, x33, rest):
    c, rho, mu, pl, pn = rest
    acc, st = w.verify_batch_sec1(case["label"], com33, c, rho, mu, r33, x33, pl, pn)
    import torch
    d = [dev(a) for a in (com33, c, rho, mu, r33, x33, pl, pn)]
    dA, dS = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.full((B,), 9, dtype=torch.int32, device="cuda")
    w.verify_batch_sec1_device(case["label"], B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), r33.shape[1],
                               d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), pl.shape[1], d[7].data_ptr(), pn.shape[1], dA.data_ptr(),
                               dS.data_ptr())
    w.synchronize()
    assert (dA.cpu().numpy() == acc).all() and (dS.cpu().numpy() == st).all()
    return acc, st


@pytest.mark.parametrize("ng,nh", [(4, 4), (16, 32), (3, 5), (1, 2), (256, 512)])
def test_wnla_sec1_matches_64_byte_form_and_oracle(ng, nh):
    _need_gpu()
    import wnla_cases
    case = _wnla_case(ng, nh)
    w = _wnla(case)
    try:
        oracle = [1 if wnla_cases.oracle_verify(case, b) == 1 else 0 for b in range(3)]
        for B in (1, 63, 257):
            t = {k: tile(case[k], B) for k in ("commitments", "c", "rho", "mu", "proof_r", "proof_x", "proof_l", "proof_n")}
            for b in range(0, B, 5):
                t["proof_l"][b, 0, 31] ^= 1
            rest = (t["c"], t["rho"], t["mu"], t["proof_l"], t["proof_n"])
            acc64, st64 = w.verify_batch(case["label"], t["commitments"], t["c"], t["rho"], t["mu"], t["proof_r"], t["proof_x"],
                                         t["proof_l"], t["proof_n"])
            acc, st = _wnla_sec1_both(w, case, B, pts33(t["commitments"]), pts33(t["proof_r"]), pts33(t["proof_x"]), rest)
            assert (acc == acc64).all() and (st == st64).all()
            clean = [b for b in range(B) if b % 5]
            assert [int(acc[b]) for b in clean] == [oracle[b % 3] for b in clean]
    finally:
        w.close()


def test_wnla_sec1_undecodable_points():
    _need_gpu()
    case = _wnla_case(4, 4)
    w = _wnla(case)
    try:
        r = case["rounds"]
        assert r >= 1
        damage = bad_encodings(wire.compress_point(bytes(case["commitments"][0])))
        positions = [("commitments", None), ("proof_r", 0), ("proof_x", r - 1)]
        B = 2 * len(positions) * len(damage) + 1
        t = {k: tile(case[k], B) for k in ("commitments", "c", "rho", "mu", "proof_r", "proof_x", "proof_l", "proof_n")}
        s33 = {"commitments": pts33(t["commitments"]), "proof_r": pts33(t["proof_r"]), "proof_x": pts33(t["proof_x"])}
        undecodable, i = [], 1
        for key, j in positions:
            for enc, pt in damage:
                if j is None:
                    s33[key][i] = np.frombuffer(enc, np.uint8); t[key][i] = np.frombuffer(pt, np.uint8)
                else:
                    s33[key][i, j] = np.frombuffer(enc, np.uint8); t[key][i, j] = np.frombuffer(pt, np.uint8)
                if pt == OFF:
                    undecodable.append(i)
                i += 2
        rest = (t["c"], t["rho"], t["mu"], t["proof_l"], t["proof_n"])
        acc64, st64 = w.verify_batch(case["label"], t["commitments"], t["c"], t["rho"], t["mu"], t["proof_r"], t["proof_x"], t["proof_l"],
                                     t["proof_n"])
        acc, st = _wnla_sec1_both(w, case, B, s33["commitments"], s33["proof_r"], s33["proof_x"], rest)
        assert (acc == acc64).all() and (st == st64).all()
        assert all(st[i] == 1 and acc[i] == 0 for i in undecodable)
        assert acc[0::2].all() and not st[0::2].any()
    finally:
        w.close()


@pytest.mark.parametrize("ng,nh", [(4, 4), (3, 5)])
def test_wnla_prove_sec1(ng, nh):
    _need_gpu()
    case = _wnla_case(ng, nh)
    w = _wnla(case)
    try:
        args = (case["c"], case["rho"], case["mu"], case["l"], case["n"])
        pr, px, pl, pn, st = w.prove_batch(case["label"], case["commitments"], *args)
        assert not st.any()
        com33 = pts33(case["commitments"])
        r33, x33, pl33, pn33, st33 = w.prove_batch_sec1(case["label"], com33, *args)
        assert not st33.any()
        assert (r33 == pts33(pr)).all() and (x33 == pts33(px)).all() and (pl33 == pl).all() and (pn33 == pn).all()
        acc, st = w.verify_batch_sec1(case["label"], com33, case["c"], case["rho"], case["mu"], r33, x33, pl33, pn33)
        assert acc.all() and not st.any()
        bad = com33.copy()
        bad[2] = np.frombuffer(b"\x02" + _nonresidue_x().to_bytes(32, "big"), np.uint8)
        bad64 = case["commitments"].copy()
        bad64[2] = np.frombuffer(OFF, np.uint8)
        r33b, x33b, pl33b, pn33b, st33b = w.prove_batch_sec1(case["label"], bad, *args)
        prb, pxb, plb, pnb, stb = w.prove_batch(case["label"], bad64, *args)
        assert (st33b == stb).all() and (r33b == pts33(prb)).all() and (x33b == pts33(pxb)).all()
        assert (pl33b == plb).all() and (pn33b == pnb).all()
        assert st33b[2] == 1 and not st33b[:2].any() and not r33b[2].any() and not x33b[2].any()
        assert (r33b[:2] == r33[:2]).all() and (pl33b[:2] == pl33[:2]).all()
    finally:
        w.close()
