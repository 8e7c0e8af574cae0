"""CPU tier of the reduction-fused Jacobian formulas: csrc/point.h's ptj_dbl (six reductions: Y3 = -(E (X3 - D) + 8 B^2) as one fused
column sum, csrc/field.h's fe_mul_add_sqr) and ptj_madd against the COMPLETE projective law (pt_dbl, pt_madd_nonid) after conversion
to affine.  The emulation library exports whole sums only, so the formulas are driven by a stand-alone host program,
tests/emul/point_formulas.cpp: the device headers compiled by g++ with the magnitude bookkeeping on (BPPP_FE_DEBUG), where a formula
that outgrows a documented bound aborts.  Inputs: the OpenSSL vector points of tests/golden/openssl_secp256k1.json.

Groups (one line of the program's output each):
  helper       a b + 8 c^2 for operands 0, 1, p - 1 and vector coordinates, and with the largest limbs the bound sum = 64 admits
  vectors      every vector point as a canonical accumulator under many Z
  magnitudes   accumulators at the largest input magnitudes the callers produce, (6, 3, 2), and every combination below
  special      coordinates 1 and p - 1 (x = 1 is on the curve; Z = 1, Z = p - 1)
  chains       5 doublings then 4 additions, the round's window step, three windows in a row; magnitudes <= (6, 3, 2) after every step
  exceptional  H = 0, empty accumulator, skipped digit: Z becomes and stays 0, `empty` and `skip` propagate, limbs untouched on a skip"""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = ("helper", "vectors", "magnitudes", "special", "chains", "exceptional")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("point_formulas")
    exe, pts = str(d / "point_formulas"), str(d / "points.txt")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "emul", "point_formulas.cpp")])
    with open(os.path.join(HERE, "golden", "openssl_secp256k1.json")) as f:
        vec = json.load(f)
    with open(pts, "w") as f:
        f.write("".join(v["xy"] + "\n" for v in vec["mul_g"]) + "".join(v["peer_xy"] + "\n" for v in vec["ecdh"]))
    r = subprocess.run([exe, pts], capture_output=True, text=True, timeout=120)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-2000:])     # anything else: a magnitude assert fired (abort) or bad input
    lines = {}
    for ln in r.stdout.splitlines():
        verdict, name, rest = ln.split(" ", 2)
        lines[name] = (verdict, rest)
    return lines


@pytest.mark.parametrize("group", GROUPS)
def test_fused_formulas_match_the_complete_law(report, group):
    assert group in report, sorted(report)
    verdict, rest = report[group]
    assert verdict == "ok" and int(rest) > 0, (group, verdict, rest)
