"""The launch form of a generic verify call at T - 1, T, T + 1 instances for every size threshold T (in units of S = "n_simds") of
csrc/plan_core.h: plan_generic, written by hand from the list below -- NOT computed from n.  Shared by
tests/test_generic_plan.py (the pure function, on the CPU) and tests/test_gpu_generic_boundaries.py (what a call on the GPU recorded
in "last_generic_form", with the verdicts against the oracle).

Sizes are in units of S = "n_simds" (1,024 on an MI355X), blocks = ceil(n / 64):
    tables in 4 | 2 | 1 parts, rounds on 16 | 8 lanes                 n <= S | n <= 4 S
    rounds on 4 | 2 | 1 lanes (one set of tables)                     4 blocks <= S | 2 blocks <= S         = n <= 16 S | 32 S
    final scalars on 8 | 4 | 2 | 1 lanes (lg 3 | 2 | 1 | 0)           blocks << (lg + 1) <= 4 S             = n <= 32 S | 64 S | 128 S,
                                                                      and lg <= rounds - 1
    fixed-base sums on a wavefront | 8 lanes per instance             n <= 8 S
    reciprocal: fixed-base sums on one lane                           n >= 128 S
    reciprocal: phase 1 on 8 | 4 | 2 | 1 lanes                        2 G blocks <= S                       = n <= 8 S | 16 S | 32 S
    reciprocal: tables and C0's sum beside phase 1                    2 blocks <= S (timing off)            = n <= 32 S
    circuit: C0's variable-base sum on a lane per point (L = 8)       L blocks <= 2 S                       = n <= 16 S"""

THRESHOLDS = [1, 4, 8, 16, 32, 64]          # x S
RECIP_ONLY = 128                            # x S: the one-lane fixed-base sums


def F(tab_parts, round_group, lg, fixed_base, phase1_group=0, beside=0, per_point=0):
    return dict(tab_parts=tab_parts, round_group=round_group, final_scalars_lg=lg, fixed_base=fixed_base, phase1_group=phase1_group,
                beside=beside, parts=1, per_point=per_point)


W, L8, L1 = "wavefront", "lanes8", "one_lane"
# (protocol, T in S) -> the form at T - 1, T, T + 1 instances.  Written by hand from the list above; NOT computed from n.
FORMS = {
    ("wnla", 1): (F(4, 16, 3, W), F(4, 16, 3, W), F(2, 8, 3, W)),
    ("wnla", 4): (F(2, 8, 3, W), F(2, 8, 3, W), F(1, 4, 3, W)),
    ("wnla", 8): (F(1, 4, 3, W), F(1, 4, 3, W), F(1, 4, 3, L8)),
    ("wnla", 16): (F(1, 4, 3, L8), F(1, 4, 3, L8), F(1, 2, 3, L8)),
    ("wnla", 32): (F(1, 2, 3, L8), F(1, 2, 3, L8), F(1, 1, 2, L8)),
    ("wnla", 64): (F(1, 1, 2, L8), F(1, 1, 2, L8), F(1, 1, 1, L8)),
    # two rounds: the final scalars split in two at most (lg 1) at every size of the sweep
    ("circuit", 1): (F(4, 16, 1, W, per_point=1), F(4, 16, 1, W, per_point=1), F(2, 8, 1, W, per_point=1)),
    ("circuit", 4): (F(2, 8, 1, W, per_point=1), F(2, 8, 1, W, per_point=1), F(1, 4, 1, W, per_point=1)),
    ("circuit", 8): (F(1, 4, 1, W, per_point=1), F(1, 4, 1, W, per_point=1), F(1, 4, 1, L8, per_point=1)),
    ("circuit", 16): (F(1, 4, 1, L8, per_point=1), F(1, 4, 1, L8, per_point=1), F(1, 2, 1, L8)),
    ("circuit", 32): (F(1, 2, 1, L8), F(1, 2, 1, L8), F(1, 1, 1, L8)),
    ("circuit", 64): (F(1, 1, 1, L8), F(1, 1, 1, L8), F(1, 1, 1, L8)),
    ("recip", 1): (F(4, 16, 3, W, 8, 1), F(4, 16, 3, W, 8, 1), F(2, 8, 3, W, 8, 1)),
    ("recip", 4): (F(2, 8, 3, W, 8, 1), F(2, 8, 3, W, 8, 1), F(1, 4, 3, W, 8, 1)),
    ("recip", 8): (F(1, 4, 3, W, 8, 1), F(1, 4, 3, W, 8, 1), F(1, 4, 3, L8, 4, 1)),
    ("recip", 16): (F(1, 4, 3, L8, 4, 1), F(1, 4, 3, L8, 4, 1), F(1, 2, 3, L8, 2, 1)),
    ("recip", 32): (F(1, 2, 3, L8, 2, 1), F(1, 2, 3, L8, 2, 1), F(1, 1, 2, L8, 1, 0)),
    ("recip", 64): (F(1, 1, 2, L8, 1, 0), F(1, 1, 2, L8, 1, 0), F(1, 1, 1, L8, 1, 0)),
    ("recip", 128): (F(1, 1, 1, L8, 1, 0), F(1, 1, 1, L1, 1, 0), F(1, 1, 0, L1, 1, 0)),
}
# distinct forms per sweep.  WNLA: {4 parts; 2 parts; group 4 + wavefront sum; group 4 + 8-lane sum; group 2; group 1 with the final
# scalars on 4 lanes; the same on 2 lanes} (final scalars on ONE lane start beyond 128 S: only the reciprocal sweep goes there).
# Circuit: the round count clips lg to 1, so the last two of those are one form, and both per_point values are among the six.
# Reciprocal: those seven, 128 S on the one-lane fixed-base sums, 128 S + 1 with one-lane final scalars as well; G = 8, 4, 2, 1 and
# both `beside` values among them.
N_FORMS = {"wnla": 7, "circuit": 6, "recip": 9}
PROTOCOL_NAME = {"wnla": "wnla", "circuit": "circuit", "recip": "reciprocal"}


def expected_form(protocol, T, d):
    return dict(FORMS[(protocol, T)][d + 1], protocol=PROTOCOL_NAME[protocol])
