// TEST-ONLY stand-alone host program (tests/test_point_formulas_fused.py builds and runs it): the incomplete Jacobian formulas of
// csrc/point.h (ptj_dbl, ptj_madd) and the fused column-sum helper of csrc/field.h against the COMPLETE projective law (pt_dbl,
// pt_madd_nonid), after conversion to affine.  The host build of the headers carries every field element's magnitude and asserts
// every bound (BPPP_FE_DEBUG), so a formula that outgrows its documented magnitudes aborts here.
//
//   point_formulas POINTS.txt      one affine point per line, 128 hex digits x || y
//
// prints one line per check group, "ok NAME CASES" or "FAIL NAME detail", and exits 0 only if every group passed.
#include <assert.h>
#include <execinfo.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bp_pp_amd/csrc/point.h"

using namespace bppp;

static int g_failed = 0;
static std::string g_detail;
static void fail(const char* what, size_t i) {
    if (g_detail.empty()) g_detail = std::string(what) + " case " + std::to_string(i);
}
static void report(const char* name, size_t cases) {
    if (g_detail.empty()) printf("ok %s %zu\n", name, cases);
    else { printf("FAIL %s %s\n", name, g_detail.c_str()); g_failed++; }
    g_detail.clear();
}

static fe fe_zero() { fe z; fe_set_u32(z, 0); return z; }
static fe fe_one() { fe o; fe_set_u32(o, 1); return o; }
static fe fe_pm1() { fe r; fe_neg_m<1>(r, fe_one()); fe_normalize(r); return r; }   // p - 1, canonical
// the same value at magnitude m: a + 2 (m - 1) p, every limb within one unit of 2^26 of the largest a magnitude-m limb may hold
static fe raise(const fe& a, int m) {
    fe r = a, z = fe_zero();
    switch (m) {
        case 1: break;
        case 2: fe_sub_m<0>(r, a, z); break;
        case 3: fe_sub_m<1>(r, a, z); break;
        case 4: fe_sub_m<2>(r, a, z); break;
        case 5: fe_sub_m<3>(r, a, z); break;
        case 6: fe_sub_m<4>(r, a, z); break;
        case 7: fe_sub_m<5>(r, a, z); break;
        case 8: fe_sub_m<6>(r, a, z); break;
        default: assert(0);
    }
    return r;
}
// the largest limbs magnitude m allows (some field value; used where only the arithmetic identity matters)
static fe fe_max_limbs(int m) {
    fe r;
    for (int i = 0; i < 9; i++) r.v[i] = 2u * m * BPPP_M26;
    r.v[9] = 2u * m * BPPP_M22;
    FE_SETMAG(r, m);
    return r;
}
// Jacobian coordinates (x z^2, y z^3, z) of an affine point, raised to magnitudes (mx, my, mz)
static ptj jac(const apt& p, const fe& z, int mx, int my, int mz) {
    ptj a;
    fe z2, z3;
    fe_sqr(z2, z);
    fe_mul(z3, z2, z);
    fe_mul(a.X, p.x, z2);
    fe_mul(a.Y, p.y, z3);
    a.X = raise(a.X, mx);
    a.Y = raise(a.Y, my);
    a.Z = raise(z, mz);
    return a;
}
struct xy64 { uint8_t b[64]; };
static xy64 affine_of(const pt& p) {
    apt r;
    xy64 o;
    pt_to_affine(r, p);
    apt_to_xy64(o.b, r);
    return o;
}
static xy64 affine_of(const ptj& a, bool empty) {
    pt p;
    ptj_to_pt(p, a, empty);
    return affine_of(p);
}
static bool same(const xy64& a, const xy64& b) { return memcmp(a.b, b.b, 64) == 0; }
static bool same_limbs(const fe& a, const fe& b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }
// what the callers rely on after every step (point.h: "Coordinate magnitudes stay <= (6, 3, 2)")
static bool mags_ok(const ptj& a) { return FE_MAG(a.X) <= 6 && FE_MAG(a.Y) <= 3 && FE_MAG(a.Z) <= 2; }

static bool check_dbl(const apt& p, const fe& z, int mx, int my, int mz) {
    ptj a = jac(p, z, mx, my, mz);
    ptj_dbl(a);
    pt P, D;
    pt_from_affine(P, p);
    pt_dbl(D, P);
    return mags_ok(a) && same(affine_of(a, false), affine_of(D));
}
static bool check_madd(const apt& p, const fe& z, int mx, int my, int mz, const apt& q) {
    ptj a = jac(p, z, mx, my, mz);
    bool empty = false;
    ptj_madd(a, empty, q, false);
    pt P, S;
    pt_from_affine(P, p);
    pt_madd_nonid(S, P, q);
    return !empty && mags_ok(a) && same(affine_of(a, false), affine_of(S));
}

// a vector point to add to pts[i]: the first from index `from` on with another x (the file holds k G and -k G, and +-q is "exceptional")
static const apt& other(const std::vector<apt>& pts, size_t i, size_t from) {
    for (size_t k = 0;; k++) {
        const apt& q = pts[(from + k) % pts.size()];
        if (!fe_eq(q.x, pts[i].x)) return q;
    }
}

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: point_formulas POINTS.txt\n"); return 2; }
    std::vector<apt> pts;
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char line[512];
    while (fgets(line, sizeof line, f)) {
        uint8_t b[64];
        int n = 0;
        for (; n < 64 && hexval(line[2 * n]) >= 0 && hexval(line[2 * n + 1]) >= 0; n++) b[n] = (uint8_t)(hexval(line[2 * n]) * 16 + hexval(line[2 * n + 1]));
        if (n == 0) continue;
        apt a;
        if (n != 64 || !apt_from_xy64(a, b) || apt_is_identity(a)) { fprintf(stderr, "bad point line: %s", line); return 2; }
        pts.push_back(a);
    }
    fclose(f);
    if (pts.size() < 8) { fprintf(stderr, "need at least 8 points\n"); return 2; }
    const size_t n = pts.size();
    const fe one = fe_one(), pm1 = fe_pm1();
    // Z values: 1, p - 1, 2, and the coordinates of the vector points themselves (arbitrary field elements)
    std::vector<fe> zs = {one, pm1};
    { fe two; fe_set_u32(two, 2); zs.push_back(two); }
    for (size_t i = 0; i < n; i++) zs.push_back(i & 1 ? pts[i].x : pts[i].y);

    // ---- the fused helper at its bounds: a b + 8 c^2 against fe_mul, fe_sqr, fe_mul_small
    {
        size_t cases = 0;
        std::vector<fe> ops = {fe_zero(), one, pm1, pts[0].x, pts[1].y};
        auto ref = [](const fe& a, const fe& b, const fe& c) {
            fe m, s, r;
            fe_mul(m, a, b);
            fe_sqr(s, c);
            fe_mul_small(s, s, 8);
            fe_add(r, m, s);
            return r;
        };
        for (const fe& a : ops) for (const fe& b : ops) for (const fe& c : ops) {
            fe r;
            fe_mul_add_sqr<3>(r, a, b, c);
            if (!(FE_MAG(r) <= 1 && fe_eq(r, ref(a, b, c)))) fail("canonical operands", cases);
            // the magnitudes of the doubling's call, 3 x 6 + 8 x 1, with the operands' limbs raised accordingly
            fe ar = raise(a, 3), br = raise(b, 6), r2;
            fe_mul_add_sqr<3>(r2, ar, br, c);
            if (!fe_eq(r2, ref(a, b, c))) fail("raised operands", cases);
            cases++;
        }
        // column sums at the bound: the largest limbs of magnitudes 8 x 7 + 8 x 1 x 1 = 64, and 7 x 8 the other way round
        const int mm[4][3] = {{8, 7, 1}, {7, 8, 1}, {6, 8, 1}, {4, 8, 2}};   // the last: 32 + 8 x 2 x 2, limbs shifted to bit 32
        for (auto& m : mm) {
            fe a = fe_max_limbs(m[0]), b = fe_max_limbs(m[1]), c = fe_max_limbs(m[2]), r;
            fe_mul_add_sqr<3>(r, a, b, c);
            if (!fe_eq(r, ref(a, b, c))) fail("largest limbs", cases);
            cases++;
        }
        report("helper", cases);
    }
    // ---- the OpenSSL vector points, canonical accumulators (magnitudes (1, 1, 1))
    {
        size_t cases = 0;
        for (size_t i = 0; i < n; i++) for (size_t j = 0; j < zs.size(); j += (i % 4 == 0 ? 1 : 7)) {
            if (!check_dbl(pts[i], zs[j], 1, 1, 1)) fail("dbl", cases);
            if (!check_madd(pts[i], zs[j], 1, 1, 1, other(pts, i, i + 1 + j))) fail("madd", cases);
            cases++;
        }
        report("vectors", cases);
    }
    // ---- the largest input magnitudes the callers produce, (6, 3, 2), and every smaller combination on a few points
    {
        size_t cases = 0;
        for (size_t i = 0; i < n; i++) {
            const fe& z = zs[(3 * i + 1) % zs.size()];
            if (!check_dbl(pts[i], z, 6, 3, 2)) fail("dbl (6, 3, 2)", cases);
            if (!check_madd(pts[i], z, 6, 3, 2, other(pts, i, i + 5))) fail("madd (6, 3, 2)", cases);
            cases++;
        }
        for (int mx = 1; mx <= 6; mx++) for (int my = 1; my <= 3; my++) for (int mz = 1; mz <= 2; mz++) for (size_t i = 0; i < 3; i++) {
            if (!check_dbl(pts[i], zs[i + 1], mx, my, mz)) fail("dbl magnitudes", cases);
            if (!check_madd(pts[i], zs[i + 1], mx, my, mz, other(pts, i, i + 3))) fail("madd magnitudes", cases);
            cases++;
        }
        report("magnitudes", cases);
    }
    // ---- coordinates 0, 1 and p - 1.  X = 0 and Y = 0 do not occur on the curve with Z != 0 (7 is no cube times a square there; the
    // group has odd order), so 0 is covered by Z = 0 below ("exceptional") and by the helper's operands above; x = 1 is on the curve
    // (y^2 = 8), x = p - 1 is (y^2 = 6) if 6 is a square; Z = 1 and Z = p - 1 turn those into X = 1 and X = p - 1, Y = +-y
    {
        size_t cases = 0;
        const fe xs[2] = {one, pm1};
        for (const fe& x : xs) {
            fe rhs, y, y2, seven;
            fe_sqr(rhs, x);
            fe_mul(rhs, rhs, x);
            fe_set_u32(seven, 7);
            fe_add(rhs, rhs, seven);
            fe_sqrt_candidate(y, rhs);
            fe_sqr(y2, y);
            if (!fe_eq(y2, rhs)) continue;
            fe_normalize(y);
            apt p;
            p.x = x;
            fe_normalize(p.x);
            p.y = y;
            const fe zz[2] = {one, pm1};
            for (const fe& z : zz) for (int big = 0; big < 2; big++) {
                if (!check_dbl(p, z, big ? 6 : 1, big ? 3 : 1, big ? 2 : 1)) fail("dbl", cases);
                if (!check_madd(p, z, big ? 6 : 1, big ? 3 : 1, big ? 2 : 1, pts[cases % n])) fail("madd onto", cases);
                if (!check_madd(pts[cases % n], zs[cases % zs.size()], big ? 6 : 1, big ? 3 : 1, big ? 2 : 1, p)) fail("madd of", cases);
                cases++;
            }
        }
        if (cases < 4) fail("x = 1 must be on the curve", cases);
        report("special", cases);
    }
    // ---- the round's window step: 5 doublings, then 4 additions, three windows in a row so that each formula sees the other's output
    {
        size_t cases = 0;
        for (size_t i = 0; i + 1 < n; i += 2) {
            ptj a = jac(pts[i], zs[(i + 2) % zs.size()], 1, 1, 1);
            bool empty = false;
            pt P;
            pt_from_affine(P, pts[i]);
            for (int w = 0; w < 3; w++) {
                for (int d = 0; d < 5; d++) {
                    ptj_dbl(a);
                    pt_dbl(P, P);
                    if (!mags_ok(a)) fail("magnitudes after a doubling", cases);
                }
                for (int k = 0; k < 4; k++) {
                    const apt& q = pts[(i + 1 + 4 * w + k) % n];
                    ptj_madd(a, empty, q, false);
                    pt S;
                    pt_madd_nonid(S, P, q);
                    P = S;
                    if (!mags_ok(a)) fail("magnitudes after an addition", cases);
                }
                if (!same(affine_of(a, empty), affine_of(P))) fail("window", cases);
            }
            cases++;
        }
        report("chains", cases);
    }
    // ---- today's contract for the exceptional inputs
    {
        size_t cases = 0;
        for (size_t i = 0; i < 6; i++) {
            const apt &p = pts[i], &q = pts[i + 1];
            // empty accumulator: doublings keep it (Z = 0), a skipped digit keeps it empty, the first real point IS the sum
            ptj a;
            ptj_init(a);
            bool empty = true;
            for (int d = 0; d < 5; d++) ptj_dbl(a);
            if (!fe_is_zero(a.Z)) fail("doubling an empty accumulator", cases);
            ptj_madd(a, empty, q, true);
            if (!empty || !fe_is_zero(a.Z)) fail("skip on empty", cases);
            ptj_madd(a, empty, p, false);
            if (empty || !same_limbs(a.X, p.x) || !same_limbs(a.Y, p.y) || !same_limbs(a.Z, one)) fail("first point", cases);
            pt P;
            pt_from_affine(P, p);
            if (!same(affine_of(a, empty), affine_of(P))) fail("first point, affine", cases);
            // a skipped digit leaves a non-empty accumulator untouched, limb for limb
            ptj b = jac(p, zs[i + 2], 6, 3, 2), b0 = b;
            empty = false;
            ptj_madd(b, empty, q, true);
            if (empty || !same_limbs(b.X, b0.X) || !same_limbs(b.Y, b0.Y) || !same_limbs(b.Z, b0.Z)) fail("skip", cases);
            // H = 0 (acc = +q and acc = -q): Z becomes 0 and stays 0 through doublings and additions; `empty` stays false
            for (int neg = 0; neg < 2; neg++) {
                apt pq = p;
                if (neg) { fe_neg_m<1>(pq.y, p.y); fe_normalize(pq.y); }
                ptj c = jac(p, zs[i + 3], neg ? 6 : 1, neg ? 3 : 1, neg ? 2 : 1);
                empty = false;
                ptj_madd(c, empty, pq, false);
                if (empty || !fe_is_zero(c.Z)) fail("H = 0", cases);
                ptj_dbl(c);
                if (!fe_is_zero(c.Z)) fail("doubling after H = 0", cases);
                ptj_madd(c, empty, q, false);
                if (empty || !fe_is_zero(c.Z)) fail("addition after H = 0", cases);
                ptj_madd(c, empty, q, true);
                for (int d = 0; d < 5; d++) ptj_dbl(c);
                if (empty || !fe_is_zero(c.Z) || !mags_ok(c)) fail("window after H = 0", cases);
            }
            cases++;
        }
        report("exceptional", cases);
    }
    return g_failed ? 1 : 0;
}
