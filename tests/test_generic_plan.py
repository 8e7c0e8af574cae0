"""The launch choices of the generic verifiers (WNLA, reciprocal, circuit) as the pure function they are taken from -- csrc/plan_core.h:
plan_generic, compiled here with g++ behind an extern "C" wrapper (nothing of the library is linked, nothing runs on a GPU): the hand-
written table of forms at every threshold (tests/generic_forms.py, the one the GPU tier asserts on recorded calls:
tests/test_gpu_generic_boundaries.py), the sizes at which the form changes, the diagnostic overrides, and that every field fits its bit
field of "last_generic_form" at any size.  The twin of tests/test_plan.py (the u64 plan)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from generic_forms import FORMS, expected_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOCOL = {"wnla": 1, "recip": 2, "circuit": 3}
# rounds and C0 points of the shapes the GPU sweep runs: WNLA over 16 + 32 generators, the reciprocal (32, 16) shape, the circuit `mixed_k2`
SHAPE = {"wnla": (4, 0), "recip": (5, 0), "circuit": (2, 6)}
KNOBS = ("n_simds", "no_lane_groups", "no_split", "timing", "slow_rounds", "lane_group", "fb_wide_max", "fb_one_lane_mode", "recip_beside",
         "recip_p1_group")
DEFAULTS = dict(n_simds=1024, no_lane_groups=0, no_split=0, timing=0, slow_rounds=0, lane_group=0, fb_wide_max=-1, fb_one_lane_mode=-1,
                recip_beside=-1, recip_p1_group=0)

HOST_TU = r'''
#include "plan_core.h"
using namespace bppp_host;
// knobs: n_simds, no_lane_groups, no_split, timing, slow_rounds, lane_group, fb_wide_max, fb_one_lane_mode, recip_beside, recip_p1_group
// out: code, fast, tab_parts, round_group, final_lg, fb, c0var_group, p1_group, beside, parts, c0_lanes, per_point
extern "C" void generic_plan(int protocol, unsigned long long n, unsigned long long rounds, const long long* kn, unsigned long long call_n,
                             int n_parts, unsigned long long c0_points, long long* out) {
    GenericKnobs k;
    k.n_simds = (int)kn[0]; k.no_lane_groups = kn[1]; k.no_split = kn[2]; k.timing = kn[3]; k.slow_rounds = kn[4]; k.lane_group = (int)kn[5];
    k.fb_wide_max = (long)kn[6]; k.fb_one_lane_mode = (int)kn[7]; k.recip_beside = (int)kn[8]; k.recip_p1_group = (int)kn[9];
    const GenericPlan p = plan_generic(protocol, n, rounds, k, call_n, n_parts, c0_points);
    const long long v[12] = {(long long)p.code(), p.fast, p.tab_parts, p.round_group, p.final_lg, p.fb, p.c0var_group, p.p1_group, p.beside,
                             p.parts, p.c0_lanes, p.per_point};
    for (int i = 0; i < 12; i++) out[i] = v[i];
}
extern "C" int generic_parts(unsigned long long n, int rlc, int timing, int forced) { return plan_generic_parts(n, rlc, timing, forced); }
'''
FIELDS = ("code", "fast", "tab_parts", "round_group", "final_lg", "fb", "c0var_group", "p1_group", "beside", "parts", "c0_lanes", "per_point")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the host build of csrc/plan_core.h")
    d = tmp_path_factory.mktemp("generic_plan")
    src, so = d / "generic_plan.cpp", d / "generic_plan.so"
    src.write_text(HOST_TU)
    subprocess.check_call([gxx, "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "bp_pp_amd", "csrc"), "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    L.generic_plan.argtypes = [C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.c_int, C.c_ulonglong, C.c_void_p]
    L.generic_plan.restype = None
    L.generic_parts.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int]
    out = (C.c_longlong * len(FIELDS))()

    def call(protocol, n, rounds=None, c0_points=None, call_n=None, n_parts=1, **knobs):
        assert set(knobs) <= set(KNOBS), knobs
        kn = (C.c_longlong * len(KNOBS))(*[dict(DEFAULTS, **knobs)[k] for k in KNOBS])
        L.generic_plan(PROTOCOL[protocol], n, SHAPE[protocol][0] if rounds is None else rounds, kn, n if call_n is None else call_n, n_parts,
                       SHAPE[protocol][1] if c0_points is None else c0_points, out)
        return dict(zip(FIELDS, out))
    call.parts = L.generic_parts
    return call


def decode(v):
    """WeightNormLinearArgument.generic_form()'s own reading of "last_generic_form" (include/bppp.h has the bits)."""
    from types import SimpleNamespace
    from bp_pp_amd.wnla import WeightNormLinearArgument
    return WeightNormLinearArgument.generic_form(SimpleNamespace(get_option=lambda name: v))


def test_every_row_of_the_form_table(plan):
    S = 1024
    for (protocol, T), row in FORMS.items():
        assert len(row) == 3
        for d in (-1, 0, 1):
            n = T * S + d
            assert decode(plan(protocol, n)["code"]) == expected_form(protocol, T, d), (protocol, T, d)
            # per-kernel timing on: everything on one stream
            assert decode(plan(protocol, n, timing=1)["code"]) == dict(expected_form(protocol, T, d), beside=0), (protocol, T, d)


def _changes(plan, protocol, S, upto):
    prev, out = None, []
    for n in range(1, upto + 1):
        code = plan(protocol, n, n_simds=S)["code"]
        if prev is not None and code != prev:
            out.append(n)
        prev = code
    return out


def test_the_form_changes_only_at_the_documented_sizes(plan):
    # S = 1,024: first size of 2 table sets, of one, of the 8-lane sums (and the reciprocal phase 1 on 4 lanes), of rounds on 2 lanes (the
    # circuit's C0 sum on one lane per instance; phase 1 on 2), of one-lane rounds with the final scalars on 4 lanes (phase 1 on one lane,
    # nothing beside it), of final scalars on 2 lanes, on one; the reciprocal verifier's one-lane sums from 128 S
    wnla = [1025, 4097, 8193, 16385, 32769, 65537, 131073]
    assert _changes(plan, "wnla", 1024, 140000) == wnla
    assert _changes(plan, "recip", 1024, 140000) == sorted(wnla + [131072])
    # (two rounds clip the final scalars' split to lg 1, which every size up to 128 S reaches: no change at 64 S + 1)
    assert _changes(plan, "circuit", 1024, 140000) == [1025, 4097, 8193, 16385, 32769, 131073]
    # the thresholds scale with the device
    assert _changes(plan, "wnla", 256, 40000) == [257, 1025, 2049, 4097, 8193, 16385, 32769]
    assert _changes(plan, "recip", 256, 40000) == [257, 1025, 2049, 4097, 8193, 16385, 32768, 32769]
    assert _changes(plan, "circuit", 256, 40000) == [257, 1025, 2049, 4097, 8193, 32769]


SIZES = [1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 4097, 8193, 16385, 32769, 65537, 131071, 131072, 131073, 1 << 20]


def test_lane_group_override_holds_at_every_size(plan):
    for protocol in PROTOCOL:
        rounds = SHAPE[protocol][0]
        for g, lg, p1 in ((2, 1, 2), (4, 3, 8)):
            for n in SIZES:
                p = plan(protocol, n, lane_group=g)
                assert (p["tab_parts"], p["round_group"], p["final_lg"]) == (1, g, min(lg, rounds - 1)), (protocol, g, n)
                assert p["p1_group"] == (p1 if protocol == "recip" else 0)
                if protocol == "recip":
                    assert p["c0var_group"] == g


def test_no_lane_groups_and_slow_rounds(plan):
    for protocol in PROTOCOL:
        for n in SIZES:
            p = plan(protocol, n, no_lane_groups=1)
            assert (p["tab_parts"], p["round_group"], p["final_lg"], p["per_point"]) == (1, 1, 0, 0) and p["fb"] != 1, (protocol, n)
            assert p["p1_group"] == (1 if protocol == "recip" else 0) and p["c0var_group"] <= 1
            for q in (plan(protocol, n, slow_rounds=1), plan(protocol, n, rounds=0)):
                assert (q["fast"], q["tab_parts"], q["round_group"], q["beside"], q["per_point"]) == (0, 1, 1, 0, 0), (protocol, n)
            assert plan(protocol, n, rounds=0)["final_lg"] == 0
            assert plan(protocol, n)["fast"] == 1
            # no_split: one table set, no wavefront sums, no per-point sum; the lane groups stay
            p = plan(protocol, n, no_split=1)
            assert p["tab_parts"] == 1 and p["fb"] != 1 and p["per_point"] == 0 and p["round_group"] in (4, 2, 1)


def test_diagnostic_overrides_win_over_size(plan):
    for n in SIZES:
        for g in (1, 2, 4, 8):
            assert plan("recip", n, recip_p1_group=g)["p1_group"] == g
            assert plan("recip", n, recip_p1_group=g, no_lane_groups=1)["p1_group"] == g
            assert plan("recip", n, recip_p1_group=g, lane_group=4)["p1_group"] == g
        assert plan("recip", n, recip_beside=1)["beside"] == 1 and plan("recip", n, recip_beside=0)["beside"] == 0
        # ... but not over what rules the helper stream out: kernel timing, no round-point tables
        assert plan("recip", n, recip_beside=1, timing=1)["beside"] == 0 and plan("recip", n, recip_beside=1, slow_rounds=1)["beside"] == 0
        assert plan("recip", n, fb_one_lane_mode=1)["fb"] == 2 and plan("recip", n, fb_one_lane_mode=0)["fb"] != 2
        assert plan("recip", n, fb_one_lane_mode=1, fb_wide_max=1 << 30)["fb"] == 2          # (one lane first, as the launch code reads it)
        for protocol in ("wnla", "circuit"):                                                  # (the reciprocal verifier's switch only)
            assert plan(protocol, n, fb_one_lane_mode=1)["fb"] == plan(protocol, n)["fb"] != 2
        for protocol in PROTOCOL:
            assert plan(protocol, n, fb_wide_max=1 << 30, fb_one_lane_mode=0)["fb"] == 1
            assert plan(protocol, n, fb_wide_max=1 << 30, fb_one_lane_mode=0, no_lane_groups=1, no_split=1)["fb"] == 1
            assert plan(protocol, n, fb_wide_max=0, fb_one_lane_mode=0)["fb"] == 0
            assert plan(protocol, n, fb_wide_max=n, fb_one_lane_mode=0)["fb"] == 1 and plan(protocol, n, fb_wide_max=n - 1, fb_one_lane_mode=0)["fb"] == 0


def test_a_part_of_a_call(plan):
    S = 1024
    for n, call_n in ((64, 128), (512, 1024), (4096, 8192), (8192, 16384), (8256, 16385), (16384, 32768), (16448, 32769), (40000, 80000)):
        p, whole = plan("recip", n, call_n=call_n, n_parts=2), plan("recip", call_n)
        assert (p["tab_parts"], p["beside"], p["parts"]) == (1, 0, 2) and p["fb"] != 1, (n, call_n)
        assert decode(p["code"])["parts"] == 2
        assert plan("recip", n, call_n=call_n, n_parts=2, recip_beside=1)["beside"] == 0
        assert plan("recip", n, call_n=call_n, n_parts=2, fb_wide_max=1 << 30)["fb"] == 0
        # the groups go by the wavefronts of the whole call, which are more than the part's own
        blocks = -(-call_n // 64)
        assert p["round_group"] == (4 if 4 * blocks <= S else 2 if 2 * blocks <= S else 1)
        assert p["p1_group"] == whole["p1_group"] and p["final_lg"] == whole["final_lg"]
        if whole["tab_parts"] == 1:
            assert p["round_group"] == whole["round_group"]
    assert plan("recip", 8192, call_n=16385, n_parts=2)["round_group"] == 2 and plan("recip", 8192)["round_group"] == 4
    # one lane per fixed-base sum goes by the part's own instances
    assert plan("recip", 128 * S, call_n=256 * S, n_parts=2)["fb"] == 2 and plan("recip", 128 * S - 1, call_n=256 * S, n_parts=2)["fb"] == 0
    # how many parts: one for small calls, in RLC mode and with kernel timing on; else what is forced, 4 at most
    assert [plan.parts(n, 0, 0, 0) for n in (1, 127, 128, 1 << 20)] == [1, 1, 1, 1]
    assert [plan.parts(n, 0, 0, 2) for n in (1, 127, 128, 1 << 20)] == [1, 1, 2, 2]
    assert [plan.parts(1000, 0, 0, f) for f in (-1, 0, 1, 2, 3, 4, 5, 9)] == [1, 1, 1, 2, 3, 4, 4, 4]
    assert plan.parts(1000, 1, 0, 4) == 1 and plan.parts(1000, 0, 1, 4) == 1


def test_plan_is_total(plan):
    """Every field within its bit field of the code at any size, device and round count; the code says what the fields say."""
    for S in (1, 4, 304, 1024, 4096):
        sizes = [0, 1, 2, 63, 64, 65] + [S * k + d for k in (1, 4, 8, 16, 32, 64, 128, 1000) for d in (-1, 0, 1)] + [2**31, 2**40]
        for n in sizes:
            for rounds in range(13):
                for protocol in PROTOCOL:
                    for knobs in ({}, {"lane_group": 4}, {"no_split": 1}, {"recip_p1_group": 8, "fb_one_lane_mode": 1}):
                        p = plan(protocol, n, rounds=rounds, c0_points=6, n_simds=S, **knobs)
                        assert p["tab_parts"] in (1, 2, 4) and p["round_group"] in (1, 2, 4, 8, 16) and p["fb"] in (0, 1, 2), (S, n, rounds)
                        assert 0 <= p["final_lg"] <= min(3, max(rounds - 1, 0)), (S, n, rounds)
                        assert p["p1_group"] in ((1, 2, 4, 8) if protocol == "recip" else (0,)) and p["parts"] == 1
                        assert p["c0var_group"] == (min(p["round_group"], 4) if protocol == "recip" else 0)
                        assert p["c0_lanes"] == (8 if protocol == "circuit" else 0)
                        assert p["fast"] == (rounds != 0)
                        assert 0 <= p["code"] < 1 << 23
                        assert decode(p["code"]) == {"protocol": {"wnla": "wnla", "recip": "reciprocal", "circuit": "circuit"}[protocol],
                                                     "tab_parts": p["tab_parts"], "round_group": p["round_group"], "final_scalars_lg": p["final_lg"],
                                                     "fixed_base": ("lanes8", "wavefront", "one_lane")[p["fb"]], "phase1_group": p["p1_group"],
                                                     "beside": p["beside"], "parts": 1, "per_point": p["per_point"]}
    # the circuit's lanes per instance: the smallest power of two that holds the points, 8 at least; a lane per point up to a wavefront
    assert [plan("circuit", 100, c0_points=c)["c0_lanes"] for c in (0, 5, 8, 9, 16, 17, 64, 65, 1028)] == [8, 8, 8, 16, 16, 32, 64, 128, 2048]
    assert [plan("circuit", 100, c0_points=c)["per_point"] for c in (5, 8, 9, 64, 65)] == [1, 1, 1, 1, 0]
    # ... while that stays within two wavefronts per SIMD: L ceil(n / 64) <= 2 S
    assert [plan("circuit", n, c0_points=33)["per_point"] for n in (2048, 2049)] == [1, 0]
