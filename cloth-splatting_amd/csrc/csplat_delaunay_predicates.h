// csplat_delaunay_predicates.h -- the three exact decisions of the Delaunay walk (csplat_delaunay.hip; include/csplat.h "Delaunay
// triangulation" states the definitions).  Host code may include it as well as device code: tests/delaunay_predicates_main.cpp holds it to
// integer arithmetic.
//
// Every input is a float32 coordinate widened to double.  Each decision is taken in two stages:
//   filter   the expression in plain fp64 with a forward error bound; the sign is returned when the value clears the bound
//   exact    the expression as a sum of monomials of the INPUT coordinates (no differences), each monomial formed without error, summed
//            without error as a non-overlapping fp64 expansion (two-sum; two-product by explicit fma); the sign is that of the largest
//            component
// Why nothing rounds in the exact stage: a float32 has a 24-bit significand and exponents 2^-149 .. 2^127.  A product of two is 48 bits:
// exact in fp64.  A degree-4 monomial is the product of two such doubles: hi + lo by two-product, exact because every term is a multiple
// of 2^-596 and below 2^512 -- nothing over- or underflows in fp64, denormal float32 inputs and 60-binade gaps between them included.
//
// Nothing here may contract a multiply and an add into an fma: the two-sum and the error bounds assume one rounding per operation.  clang
// (hipcc, host and device) is told so below; another host compiler must be given -ffp-contract=off.
#pragma once
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define DP_FN __host__ __device__ static inline
#define DP_FN_COLD __host__ __device__ static __attribute__((noinline))
#else
#define DP_FN static inline
#define DP_FN_COLD static __attribute__((noinline))
#endif

struct dp_pt {
    double x, y;
};

#define DP_EPS 1.1102230246251565e-16 /* 2^-53 */
#define DP_UNSURE 2                   /* a filter's answer: the exact stage decides */

DP_FN double dp_abs(double v) { return v < 0.0 ? -v : v; }

DP_FN void dp_two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

DP_FN void dp_two_prod(double a, double b, double &p, double &e) {
    p = a * b;
    e = __builtin_fma(a, b, -p);
}

// e[0 .. n): a non-overlapping expansion, components of increasing magnitude, none zero.  Adds b in place; returns the new length (at most
// n + 1).  The result has the same properties (grow-expansion with zero elimination, Shewchuk 1997, theorem 10).
DP_FN int dp_grow(double *e, int n, double b) {
    double q = b;
    int m = 0;
    for (int i = 0; i < n; i++) {
        double s, h;
        dp_two_sum(q, e[i], s, h);
        if (h != 0.0) e[m++] = h;        // m <= i: e[i] has been read
        q = s;
    }
    if (q != 0.0) e[m++] = q;
    return m;
}

DP_FN int dp_expansion_sign(const double *e, int n) { return n == 0 ? 0 : (e[n - 1] > 0.0 ? 1 : -1); }

// ---- orientation: the sign of | ax ay 1 ; bx by 1 ; cx cy 1 |, positive when a, b, c turn counter-clockwise -------------------------------
DP_FN int dp_orient_filter(dp_pt a, dp_pt b, dp_pt c) {
    const double l = (a.x - c.x) * (b.y - c.y), r = (a.y - c.y) * (b.x - c.x);
    const double det = l - r;
    // each difference, each product and the last subtraction round once: |det - true| <= ((1 + eps)^4 - 1) (|l| + |r|) < 5 eps (|l| + |r|)
    const double bound = 8.0 * DP_EPS * (dp_abs(l) + dp_abs(r));
    return det > bound ? 1 : (-det > bound ? -1 : DP_UNSURE);
}

// the six monomials, each one double; e holds 6
DP_FN int dp_orient_expansion(dp_pt a, dp_pt b, dp_pt c, double *e) {
    int n = 0;
    n = dp_grow(e, n, a.x * b.y);
    n = dp_grow(e, n, -(a.y * b.x));
    n = dp_grow(e, n, b.x * c.y);
    n = dp_grow(e, n, -(b.y * c.x));
    n = dp_grow(e, n, c.x * a.y);
    n = dp_grow(e, n, -(c.y * a.x));
    return n;
}

DP_FN_COLD int dp_orient_exact(dp_pt a, dp_pt b, dp_pt c) {
    double e[6];
    return dp_expansion_sign(e, dp_orient_expansion(a, b, c, e));
}

DP_FN int dp_orient(dp_pt a, dp_pt b, dp_pt c, unsigned &exact) {
    const int s = dp_orient_filter(a, b, c);
    if (s != DP_UNSURE) return s;
    exact++;
    return dp_orient_exact(a, b, c);
}

// ---- distance: the sign of |a - o|^2 - |b - o|^2 ---------------------------------------------------------------------------------------------
DP_FN int dp_nearer_filter(dp_pt o, dp_pt a, dp_pt b) {
    const double ax = a.x - o.x, ay = a.y - o.y, bx = b.x - o.x, by = b.y - o.y;
    const double da = ax * ax + ay * ay, db = bx * bx + by * by;
    // a squared distance: (1 + eps)^2 per difference pair, one rounding per product, one for the sum: < 5 eps relative
    const double bound = 16.0 * DP_EPS * (da + db);
    const double d = da - db;
    return d > bound ? 1 : (-d > bound ? -1 : DP_UNSURE);
}

DP_FN_COLD int dp_nearer_exact(dp_pt o, dp_pt a, dp_pt b) {
    // |a|^2 - 2 o.a - |b|^2 + 2 o.b: eight monomials, each one double (a factor 2 is exact)
    double e[8];
    int n = 0;
    n = dp_grow(e, n, a.x * a.x);
    n = dp_grow(e, n, a.y * a.y);
    n = dp_grow(e, n, -2.0 * (o.x * a.x));
    n = dp_grow(e, n, -2.0 * (o.y * a.y));
    n = dp_grow(e, n, -(b.x * b.x));
    n = dp_grow(e, n, -(b.y * b.y));
    n = dp_grow(e, n, 2.0 * (o.x * b.x));
    n = dp_grow(e, n, 2.0 * (o.y * b.y));
    return dp_expansion_sign(e, n);
}

// -1: a is nearer to o than b;  +1: b is nearer;  0: equally far
DP_FN int dp_nearer(dp_pt o, dp_pt a, dp_pt b, unsigned &exact) {
    const int s = dp_nearer_filter(o, a, b);
    if (s != DP_UNSURE) return s;
    exact++;
    return dp_nearer_exact(o, a, b);
}

// ---- in-circle with the symbolic tie rule ------------------------------------------------------------------------------------------------------
// det = | ax ay ax^2+ay^2 1 ; b ; c ; d |: positive when d lies strictly inside the circle through the counter-clockwise a, b, c.
DP_FN int dp_incircle_filter(dp_pt a, dp_pt b, dp_pt c, dp_pt d) {
    const double adx = a.x - d.x, ady = a.y - d.y, bdx = b.x - d.x, bdy = b.y - d.y, cdx = c.x - d.x, cdy = c.y - d.y;
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy, alift = adx * adx + ady * ady;
    const double cdxady = cdx * ady, adxcdy = adx * cdy, blift = bdx * bdx + bdy * bdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady, clift = cdx * cdx + cdy * cdy;
    const double det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady);
    const double permanent = (dp_abs(bdxcdy) + dp_abs(cdxbdy)) * alift + (dp_abs(cdxady) + dp_abs(adxcdy)) * blift + (dp_abs(adxbdy) + dp_abs(bdxady)) * clift;
    // with exact differences the evaluation is within (10 + 96 eps) eps of the permanent (Shewchuk 1997, the A stage of incircle); every
    // monomial has four difference factors, each rounded once here: another (1 + eps)^4 - 1 < 5 eps.  24 eps leaves room.
    const double bound = 24.0 * DP_EPS * permanent;
    return det > bound ? 1 : (-det > bound ? -1 : DP_UNSURE);
}

// e += sign * o[0 .. no) * (p.x^2 + p.y^2), every partial product hi + lo
DP_FN int dp_add_lifted(double *e, int n, const double *o, int no, dp_pt p, double sign) {
    const double xx = p.x * p.x, yy = p.y * p.y;      // 48 bits each: exact
    for (int i = 0; i < no; i++) {
        double hi, lo;
        dp_two_prod(o[i], xx, hi, lo);
        n = dp_grow(e, n, sign * lo);
        n = dp_grow(e, n, sign * hi);
        dp_two_prod(o[i], yy, hi, lo);
        n = dp_grow(e, n, sign * lo);
        n = dp_grow(e, n, sign * hi);
    }
    return n;
}

// The exact determinant by its four cofactors +orient(b,c,d), -orient(a,c,d), +orient(a,b,d), -orient(a,b,c), each times its point's lifted
// height: 4 * 6 * 2 degree-4 monomials of two doubles each, at most 96 components.  When it is zero the lifted height of point p is raised
// by eps_p, eps_0 >> eps_1 >> ... > 0: the sign is that of the first non-zero cofactor in ascending point index (ia .. id are the indices).
DP_FN_COLD int dp_incircle_exact(dp_pt a, dp_pt b, dp_pt c, dp_pt d, int ia, int ib, int ic, int id) {
    double oa[6], ob[6], oc[6], od[6], e[96];
    const int na = dp_orient_expansion(b, c, d, oa), nb = dp_orient_expansion(a, c, d, ob);
    const int nc = dp_orient_expansion(a, b, d, oc), nd = dp_orient_expansion(a, b, c, od);
    int n = 0;
    n = dp_add_lifted(e, n, oa, na, a, 1.0);
    n = dp_add_lifted(e, n, ob, nb, b, -1.0);
    n = dp_add_lifted(e, n, oc, nc, c, 1.0);
    n = dp_add_lifted(e, n, od, nd, d, -1.0);
    int s = dp_expansion_sign(e, n);
    if (s != 0) return s;
    const int idx[4] = {ia, ib, ic, id};
    const int cof[4] = {dp_expansion_sign(oa, na), -dp_expansion_sign(ob, nb), dp_expansion_sign(oc, nc), -dp_expansion_sign(od, nd)};
    int first = 0x7fffffff;
    for (int q = 0; q < 4; q++)
        if (cof[q] != 0 && idx[q] < first) {
            first = idx[q];
            s = cof[q];
        }
    return s;
}

DP_FN int dp_incircle(dp_pt a, dp_pt b, dp_pt c, dp_pt d, int ia, int ib, int ic, int id, unsigned &exact) {
    const int s = dp_incircle_filter(a, b, c, d);
    if (s != DP_UNSURE) return s;
    exact++;
    return dp_incircle_exact(a, b, c, d, ia, ib, ic, id);
}
