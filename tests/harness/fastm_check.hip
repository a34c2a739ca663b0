// se3_math.h, namespace fastm: rcp, sqrt_rsqrt, sincos and atan_ratio -- the device forms behind every pose the engine, the batched LM
// and the pairs tracker compute -- called DIRECTLY, one lane per argument, and held on the host to long double (division, sqrtl, sinl,
// cosl, atanl) in ULPS OF THE CORRECTLY ROUNDED DOUBLE (section 1); then qlog<true>, qexp<true> and so3_exp on the device against the
// reference's formulas restated branch for branch in long double, measured by the header's host half (section 2).
//
//   fastm_check_bin           everything, the device included
//   fastm_check_bin --host    no HIP call is made.  Every input list is built; libm's sin, cos, atan(n / w), sqrt, 1 / sqrt and the IEEE
//                             1.0 / x go through the same ulp checker in the device forms' place (every single operation at or below 1 ulp,
//                             sqrt and the division correctly rounded, the two compositions at what follows from that, see
//                             BOUND_LIBM: this proves the checker and the long-double reference on the machine at hand); section 2 is evaluated with the host half alone (its 1e-13 condition and the branch
//                             counts).  This is the mode for the host sanitizers (the file also compiles as plain C++).
//
// Every bound below is derived from the forms as written and from the precision of the formats; none is taken from a device run.
// u = 2^-53 is the unit roundoff: one rounding to nearest changes a value by at most u of itself, which is between 1/2 and 1 ulp of the
// result, and a relative error e of a result is at most e / u of its ulps.  The long-double references are good to 2^-11 ulp of a double
// (64-bit significand, glibc's sinl / cosl / atanl are below 1 ulp of their own format); SLACK = 2^-10 ulp is added to every bound for
// them and for the second-order terms the derivations drop.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "se3_math.h"

namespace
{
    typedef unsigned long long u64;
    typedef long double ld;

    constexpr ld SLACK = 1.0L / 1024.0L;

    // ---- the derived bounds, in ulps ----------------------------------------------------------------------------------------------------
    // PREMISE: v_rcp_f64 and v_rsq_f64 return estimates with a relative error e0 <= 2^-20 (the header says 2^-23; the derivations need far
    // less).  The device run measures both estimates against this premise and fails if it does not hold.
    const ld EST_PREMISE = std::ldexp(1.0, -20);
    //
    // rcp.  r = (1 + e0) / x.  A step forms d = fma(-x, r, 1) = -e (one rounding of a value of size e) and fma(r, d, r) = (1 - e^2)(1 + u)
    // / x.  After the first step e1 <= e0^2 + u <= 2^-40 + 2^-53; the second step's value BEFORE its final rounding is (1 - e1^2 - e1 u) / x,
    // off by 2^-79 relative = 2^-26 ulp, and the final rounding adds 1/2 ulp: the correctly rounded reciprocal except next to a rounding
    // boundary.  A power of two: the residual d is 0 or the estimate's own error, the same steps end on 1 / x exactly (checked as equality).
    constexpr ld BOUND_RCP = 0.5L + SLACK;
    // sqrt_rsqrt, r.  y = (1 + e) / sqrt(x), h = x / 2 (exact).  A step forms t = fl(h y), d = fma(-t, y, 0.5) and fma(y, d, y): in real
    // numbers y (1.5 - h y^2) = (1 - 1.5 e^2 - ..) / sqrt(x); the rounding of t moves d by at most u / 2 (h y^2 is 1/2), d's own rounding is
    // of size u e.  e1 <= 1.5 e0^2 + 1.5 u <= 2^-39; the second step's value before its final rounding is off by u / 2 + 1.5 e1^2 relative
    // (at most 1/2 ulp), the final rounding by 1/2 ulp more.
    constexpr ld BOUND_RSQRT = 1.0L + SLACK;
    // sqrt_rsqrt, s.  y is now within 1.5 u, t = fl(x y) within e_t <= 2.5 u of the root.  The correction adds fma(-t, t, x) = -x (2 e_t +
    // e_t^2) (exact product, one rounding of a value of size u x) times y / 2 = (1 + e_y) / (2 sqrt(x)): the first-order error cancels, what
    // is left before the final rounding is e_t e_y + e_t^2 / 2 + e_t u <= 10 u^2 = 2^-49 ulp.  Correctly rounded except next to a boundary.
    constexpr ld BOUND_SQRT = 0.5L + SLACK;
    // sincos.  k = rint(x * 2/pi); r1 = fma(-k, c1, x) is exact for |x| < 2^21 (c1 has 33 bits, k c1 <= 54 bits and a multiple of 2^-32, the
    // difference is below |x| and a multiple of min(ulp(x), 2^-32)); r = fma(-k, c2, r1) rounds once.  The true reduced argument is
    // rho = x - k pi/2 = r1 - k c2 - k D with D = pi/2 - c1 - c2, so r = (rho + k D)(1 + u): an ABSOLUTE error |k| |D| in the argument, hence
    // (|sin'|, |cos'| <= 1) in both results, and a relative one of u in r (none where k = 0).  |r| <= pi/4 (1 + 2^-30).
    //   sine kernel  r + (z r)(S1 + z ps):  the argument's rounding, dr <= ulp(r) / 2, moves the result by dr cos(r) / sin(r) relative: at
    //     most u for |r| < 1/2 and 2^-54 / tan(1/2) = 0.915 u above.  The correction term c = (z r)(S1 + z ps) carries z (u), z r (2 u),
    //     S1 + z ps (1.1 u: ps is 1/20 of S1) and its product: 4.1 u of |c| <= r^3 / 6, which is 0.044 of sin(r) at r = 1/2 and 0.114 at pi/4:
    //     0.18 u and 0.47 u.  The polynomial itself is within 2^-58 (0.03 u).  With the final rounding:
    //       |r| < 1/2: 0.5 + 1.0 + 0.18 + 0.03 = 1.71 ulp;   |r| >= 1/2: 0.5 + 0.915 + 0.47 + 0.03 = 1.92 ulp
    //   cosine kernel  w + (((1 - w) - hz) + z pc), hz = z / 2, w = fl(1 - hz): (1 - w) - hz is w's rounding error exactly, so the value is
    //     1 - hz + z pc with the errors of z (u z / 2 <= 0.31 u absolute), of z pc (3 u of z^2 / 24 <= 0.016: 0.05 u) and of the inner sum
    //     (0.016 u); the argument's rounding moves it by dr sin(r) <= 0.36 u.  The result is in [0.707, 1] where 1 ulp is u:
    //       0.5 + 0.31 + 0.05 + 0.02 + 0.03 + 0.36 = 1.27 ulp
    //   Either output is either kernel, by quadrant.  FMA contraction of the polynomials removes roundings and adds none.
    constexpr ld BOUND_SINCOS = 1.93L + SLACK;
    // The absolute term |k| |D| (times 1 + 2^-20 for the u (k D) the relative part leaves out).  pi/2 = PIO2_HI + PIO2_LO to 128 bits;
    // (PIO2_HI - c1) - c2 is exact in long double (c1 reaches 2^-32, PIO2_HI 2^-63, c2 2^-86, the difference is below 2^-65).
    constexpr ld PIO2_HI = 0xc.90fdaa22168c235p-3L, PIO2_LO = -0xe.ce675d1fc8f8cbbp-69L;
    constexpr double SC_INVPIO2 = 6.36619772367581382433e-01, SC_C1 = 1.57079632673412561417e+00, SC_C2 = 6.07710050650619224932e-11;
    const ld SC_D = fabsl(((PIO2_HI - (ld)SC_C1) - (ld)SC_C2) + PIO2_LO); // 3.52e-27
    // atan_ratio, from three parts: the quotient, the reduced argument's rcp, fdlibm's kernel.
    //   quotient: x0 = fl(num * rcp(den)) = (num / den)(1 + e), |e| <= 2 u (rcp within 1/2 ulp, one product).  atan moves by e t / (1 + t^2),
    //     which is at most e of atan(t) itself and at most e / 2 absolute.
    //   reduced argument x = N * rcp(Dn): N (2 ax - 1, ax - 1, ax - 1.5) is exact (Sterbenz); Dn rounds once (1 + 1.5 ax: twice), rcp and the
    //     product once each: 3 u (4 u) of |x|;  -rcp(ax): u of |x|.
    //   kernel: x - x (s1 + s2) below 0.4375: 5 u of a term that is <= 0.068 of the result, and the final rounding; above,
    //     hi - ((x (s1 + s2) - lo) - x): the inner sum rounds at |x| < 1/4 (<= 2^-56 absolute, 2^-55 in the last range), then the final
    //     rounding; hi + lo is the breakpoint's arctangent to 2^-106; the polynomial is within 0.03 u.
    //   per range, in ulps of a result in the binade named (1 ulp = u / 2 below 1/2, u below 1, 2 u above):
    //     [0, 0.4375):       2 g(t) + 0.5 + 1.67 t^2 + 0.03, g = t / ((1 + t^2) atan t) <= 1 - 0.6 t^2           <= 2.65
    //     [0.4375, 0.6875):  result < 1/2 (t < 0.5463): (2 * 0.4208 + 3 * 0.0513 + 0.125) u * 2 + 0.5 + 0.03      = 2.77
    //                        result >= 1/2:              2 * 0.4669 + 3 * 0.1395 + 0.125 + 0.5 + 0.03              = 2.01
    //     [0.6875, 1.1875):  2 * 0.5 + 3 * 0.185 + 0.125 + 0.5 + 0.04                                             = 2.22
    //     [1.1875, 2.4375):  result < 1 (t < 1.5574): 2 * 0.4927 + 4 * 0.1124 + 0.125 + 0.5 + 0.04                = 2.10
    //                        result >= 1:            (2 * 0.4546 + 4 * 0.2013 + 0.125) / 2 + 0.5 + 0.04           = 1.46
    //     [2.4375, inf):     (2 * 0.351 + 0.35 + 0.09 + 0.25) / 2 + 0.5 + 0.03                                    = 1.23
    //   The largest is 2.77: more than the header's "one or two", under the issue's ceiling of 4.
    constexpr ld BOUND_ATAN = 2.8L + SLACK;
    // libm and IEEE in the forms' place (--host).  Every single operation is held to its own argument: a libm call (sin, cos, atan) within
    // 1 ulp, sqrt and the division correctly rounded.  The two COMPOSITIONS are then held to the true value at what follows from that:
    // the inner result's 1/2 ulp is a relative u, up to 1 ulp of the outer result, so 1 / sqrt(x) is within 1 + 1/2 and atan(n / w) within
    // 1 + 1 ulp of 1 / sqrt(x) and atan(n / w) in real numbers (1 ulp for either is NOT reachable: 1.47 is measured for both).
    constexpr ld BOUND_LIBM = 1.0L + SLACK, BOUND_EXACT = 0.5L + SLACK, BOUND_LIBM_RSQRT = 1.5L + SLACK, BOUND_LIBM_ATAN_RATIO = 2.0L + SLACK;

    struct Rng
    {
        u64 s;
        u64 next()
        { // splitmix64
            u64 z = (s += 0x9e3779b97f4a7c15ull);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
            return z ^ (z >> 31);
        }
        double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
        double uniform(double lo, double hi) { return lo + (hi - lo) * unit(); }
        double loguniform(double lo, double hi) { return std::exp(uniform(std::log(lo), std::log(hi))); }
        double binade(int elo, int ehi) { return std::ldexp(1.0 + unit(), elo + (int)(next() % (u64)(ehi - elo + 1))); }
        double sign() { return (next() & 1) ? -1.0 : 1.0; }
    };

    // v and the four doubles on each side
    void nine(std::vector<double> &out, double v)
    {
        const double inf = std::numeric_limits<double>::infinity();
        double lo = v;
        for (int i = 0; i < 4; ++i) lo = std::nextafter(lo, -inf);
        for (int i = 0; i < 9; ++i) { out.push_back(lo); lo = std::nextafter(lo, inf); }
    }

    // 1 ulp of the double c (the spacing of the doubles at and above |c|)
    ld ulp_of(double c)
    {
        if (c == 0.0) return std::ldexp(1.0, -1074);
        int e = std::ilogb(c);
        if (e < -1022) e = -1022;
        return ldexpl(1.0L, e - 52);
    }

    struct Span { std::string name; size_t lo, hi; }; // an input class: lanes [lo, hi) of its function's list

    struct Stat
    {
        std::string what;
        u64 n = 0, bad = 0;
        ld worst = 0, worst_abs = 0, worst_rel = 0, worst_share = 0; // ulps; |error|; |error| / |reference|; |error| / allowed
        double a0 = 0, a1 = 0;
        ld bound = 0;
        bool with_abs = false;
    };
    int g_notes = 0;

    // `got` against `ref` inside bound * ulp(correctly rounded ref) + abs_term; a0, a1 the arguments for the report
    void judge(Stat &s, double got, ld ref, ld bound, ld abs_term, double a0, double a1)
    {
        ++s.n;
        s.bound = bound;
        const double c = (double)ref;
        const ld inf = std::numeric_limits<ld>::infinity();
        ld e = fabsl((ld)got - ref);
        if (!(e == e)) e = inf;
        const ld u = ulp_of(c), eu = e / u, allowed = bound * u + abs_term;
        if (eu > s.worst || s.n == 1) { s.worst = eu; s.a0 = a0; s.a1 = a1; }
        if (e > s.worst_abs) s.worst_abs = e;
        if (ref != 0 && e / fabsl(ref) > s.worst_rel) s.worst_rel = e / fabsl(ref);
        if (allowed > 0 && e / allowed > s.worst_share) s.worst_share = e / allowed;
        if (!(e <= allowed))
        {
            ++s.bad;
            if (g_notes++ < 12)
                printf("  OUTSIDE %s: arguments %a (%.17g), %a (%.17g): got %a, reference %.21Lg, %.4Lg ulp (bound %.4Lg ulp + %.3Lg)\n", s.what.c_str(),
                       a0, a0, a1, a1, got, ref, eu, bound, abs_term);
        }
    }
    void fail_note(Stat &s, const char *why, double a0, double got)
    {
        ++s.bad;
        if (g_notes++ < 12) printf("  OUTSIDE %s: argument %a (%.17g): got %a: %s\n", s.what.c_str(), a0, a0, got, why);
    }
    void print_stat(const Stat &s)
    {
        printf("%-58s cases %8llu  worst %9.4Lg ulp (bound %.4Lg) at %a", s.what.c_str(), s.n, s.worst, s.bound, s.a0);
        if (s.a1 != 0) printf(", %a", s.a1);
        if (s.with_abs) printf("  worst absolute %.3Le, worst relative %.3Le, worst share of the allowed error %.3Lf", s.worst_abs, s.worst_rel, s.worst_share);
        printf("  outside %llu\n", s.bad);
    }

    // ---- section 1: inputs --------------------------------------------------------------------------------------------------------------
    struct Inputs
    {
        std::vector<double> rcp_x, sq_x, sc_x, at_n, at_d;
        std::vector<Span> rcp_c, sq_c, sc_c, at_c;
        size_t rcp_pow2_lo = 0, rcp_pow2_hi = 0, sc_nan_lo = 0, at_zero_lo = 0, at_zero_hi = 0;
    };
    void close_span(std::vector<Span> &spans, const char *name, size_t size)
    {
        spans.push_back(Span{name, spans.empty() ? 0 : spans.back().hi, size});
    }

    Inputs make_inputs()
    {
        Inputs in;
        const double inf = std::numeric_limits<double>::infinity(), pi = 3.14159265358979323846;
        { // rcp
            Rng r{11};
            for (int i = 0; i < (1 << 20); ++i) in.rcp_x.push_back(r.sign() * r.binade(-1022, 1021)); // x and 1 / x normal
            close_span(in.rcp_c, "log-uniform over every binade, both signs", in.rcp_x.size());
            in.rcp_pow2_lo = in.rcp_x.size();
            for (int e = -1022; e <= 1022; ++e) { in.rcp_x.push_back(std::ldexp(1.0, e)); in.rcp_x.push_back(-std::ldexp(1.0, e)); }
            in.rcp_pow2_hi = in.rcp_x.size();
            close_span(in.rcp_c, "powers of two (exact)", in.rcp_x.size());
            nine(in.rcp_x, 1.0); nine(in.rcp_x, 2.0);
            close_span(in.rcp_c, "neighbours of 1 and 2", in.rcp_x.size());
        }
        { // sqrt_rsqrt
            Rng r{12};
            for (int i = 0; i < (1 << 20); ++i) in.sq_x.push_back(r.loguniform(1e-20, 1e3));
            close_span(in.sq_c, "log-uniform [1e-20, 1e3]", in.sq_x.size());
            for (int i = 0; i < (1 << 18); ++i) in.sq_x.push_back(r.binade(-1000, 999));
            close_span(in.sq_c, "log-uniform [2^-1000, 2^1000]", in.sq_x.size());
            nine(in.sq_x, 1e-20); nine(in.sq_x, 1.0); nine(in.sq_x, 4.0);
            close_span(in.sq_c, "neighbours of 1e-20, 1 and 4", in.sq_x.size());
        }
        { // sincos
            Rng r{13};
            for (int i = 0; i < (1 << 20); ++i) { const double x = r.uniform(0.0, 0.5 * pi); in.sc_x.push_back(x); in.sc_x.push_back(-x); }
            close_span(in.sc_c, "half-angles: uniform [0, pi/2] and negatives", in.sc_x.size());
            for (int i = 0; i < (1 << 18); ++i) in.sc_x.push_back(r.uniform(-8.0, 8.0));
            close_span(in.sc_c, "uniform [-8, 8]", in.sc_x.size());
            for (int i = 0; i < (1 << 18); ++i) in.sc_x.push_back(r.sign() * r.loguniform(1e-300, 1e5));
            close_span(in.sc_c, "log-uniform [1e-300, 1e5], both signs", in.sc_x.size());
            std::vector<int> ks;
            for (int k = 0; k <= 64; ++k) ks.push_back(k);
            ks.push_back(1 << 10); ks.push_back(1 << 16); ks.push_back(63661);
            for (int k : ks) nine(in.sc_x, (double)((ld)k * (PIO2_HI + PIO2_LO)));
            close_span(in.sc_c, "neighbours of k pi/2", in.sc_x.size());
            for (int k : ks) nine(in.sc_x, (double)(((ld)k + 0.5L) * (PIO2_HI + PIO2_LO)));
            close_span(in.sc_c, "neighbours of (k + 1/2) pi/2", in.sc_x.size());
            in.sc_nan_lo = in.sc_x.size();
            in.sc_x.push_back(std::numeric_limits<double>::quiet_NaN()); in.sc_x.push_back(inf); in.sc_x.push_back(-inf);
            close_span(in.sc_c, "NaN, +inf, -inf (both results NaN)", in.sc_x.size());
        }
        { // atan_ratio
            Rng r{14};
            auto put = [&](double n, double d) { in.at_n.push_back(n); in.at_d.push_back(d); };
            for (int i = 0; i < (1 << 20); ++i)
            {
                const double a = r.uniform(0.0, 2.0 * pi);
                const double n = std::fabs(std::sin(0.5 * a)), w = std::cos(0.5 * a);
                if (a > 0.0 && std::fabs(w) >= 1e-10) put(n, w);
            }
            close_span(in.at_c, "(|sin(a/2)|, cos(a/2)), a uniform (0, 2 pi)", in.at_n.size());
            for (int i = 0; i < (1 << 18); ++i)
            {
                const double ratio = r.loguniform(1e-12, 1e12), d = r.loguniform(1e-10, 1e3), n = ratio * d;
                put(n, d); put(-n, d); put(n, -d); put(-n, -d);
            }
            close_span(in.at_c, "ratio log-uniform [1e-12, 1e12], four signs", in.at_n.size());
            for (double L : {0.4375, 0.6875, 1.1875, 2.4375})
                for (double d : {1.0, 3.0, 0.1})
                {
                    std::vector<double> ns;
                    nine(ns, L * d);
                    for (double n : ns) put(n, d);
                }
            close_span(in.at_c, "range limits: neighbours of L den", in.at_n.size());
            in.at_zero_lo = in.at_n.size();
            for (double d : {1.0, -1.0, 3.0, 1e-10, 1e3}) { put(0.0, d); put(-0.0, d); }
            in.at_zero_hi = in.at_n.size();
            for (double d : {1.0, -1.0, 3.0, 0.1, 1e-10, 1e3}) put(d, d);
            for (int i = 0; i < 1024; ++i) { const double d = r.sign() * r.loguniform(1e-10, 1e3); put(d, d); }
            close_span(in.at_c, "num = 0 and num = den", in.at_n.size());
            {
                std::vector<double> ns;
                nine(ns, 1e290);
                for (double n : {1e289, 0.5e290, 2e290, 1e291, 1e295, 1e300}) ns.push_back(n);
                for (double n : ns) { put(n, 1e-10); put(-n, 1e-10); }
            }
            close_span(in.at_c, "den = 1e-10, num round 1e290 (the 1e300 guard)", in.at_n.size());
        }
        return in;
    }

    // ---- section 1: results (the device's, or libm's and IEEE's in --host) and their check ------------------------------------------------
    struct Results
    {
        std::vector<double> rcp, rcp_est, sq_s, sq_r, sq_est, sn, cs, at;
        bool device = false;
    };

    void host_results(const Inputs &in, Results &o)
    {
        o.device = false;
        for (double x : in.rcp_x) o.rcp.push_back(1.0 / x);
        for (double x : in.sq_x) { o.sq_s.push_back(std::sqrt(x)); o.sq_r.push_back(1.0 / std::sqrt(x)); }
        for (double x : in.sc_x) { o.sn.push_back(std::sin(x)); o.cs.push_back(std::cos(x)); }
        for (size_t i = 0; i < in.at_n.size(); ++i) o.at.push_back(std::atan(in.at_n[i] / in.at_d[i]));
    }

    u64 check_forms(const Inputs &in, const Results &o)
    {
        const bool dev = o.device;
        const char *tag = dev ? "" : "libm / IEEE in place of ";
        std::vector<Stat> all;
        auto fresh = [&](const char *fn, const Span &c, bool with_abs = false) {
            Stat s;
            s.what = std::string(tag) + fn + ": " + c.name;
            s.with_abs = with_abs;
            return s;
        };
        // rcp
        for (const Span &c : in.rcp_c)
        {
            Stat s = fresh("rcp", c);
            for (size_t i = c.lo; i < c.hi; ++i)
            {
                const double x = in.rcp_x[i];
                judge(s, o.rcp[i], 1.0L / (ld)x, dev ? BOUND_RCP : BOUND_EXACT, 0, x, 0);
                if (i >= in.rcp_pow2_lo && i < in.rcp_pow2_hi && !(o.rcp[i] == 1.0 / x)) fail_note(s, "the reciprocal of a power of two must be exact", x, o.rcp[i]);
            }
            all.push_back(s);
        }
        // sqrt_rsqrt
        for (const Span &c : in.sq_c)
        {
            Stat ss = fresh("sqrt_rsqrt s", c), sr = fresh("sqrt_rsqrt r", c), sd = fresh("the division alone, 1.0 / s", c);
            for (size_t i = c.lo; i < c.hi; ++i)
            {
                const double x = in.sq_x[i];
                const ld root = sqrtl((ld)x);
                judge(ss, o.sq_s[i], root, dev ? BOUND_SQRT : BOUND_EXACT, 0, x, 0);
                judge(sr, o.sq_r[i], 1.0L / root, dev ? BOUND_RSQRT : BOUND_LIBM_RSQRT, 0, x, 0);
                if (!dev) judge(sd, o.sq_r[i], 1.0L / (ld)o.sq_s[i], BOUND_EXACT, 0, o.sq_s[i], 0);
            }
            all.push_back(ss); all.push_back(sr);
            if (!dev) all.push_back(sd);
        }
        // sincos
        for (const Span &c : in.sc_c)
        {
            const bool special = c.lo >= in.sc_nan_lo, by_k = c.name.find("neighbours") != std::string::npos;
            Stat s1 = fresh("sincos sin", c, by_k), s2 = fresh("sincos cos", c, by_k);
            for (size_t i = c.lo; i < c.hi; ++i)
            {
                const double x = in.sc_x[i];
                if (special)
                {
                    ++s1.n; ++s2.n;
                    if (!std::isnan(o.sn[i])) fail_note(s1, "want NaN", x, o.sn[i]);
                    if (!std::isnan(o.cs[i])) fail_note(s2, "want NaN", x, o.cs[i]);
                    continue;
                }
                const double k = std::rint(x * SC_INVPIO2); // the form's own k: one product, one rint, the same bits on the host
                const ld abs_term = dev ? fabsl((ld)k) * SC_D * (1.0L + 1.0L / 1048576.0L) : 0.0L;
                judge(s1, o.sn[i], sinl((ld)x), dev ? BOUND_SINCOS : BOUND_LIBM, abs_term, x, 0);
                judge(s2, o.cs[i], cosl((ld)x), dev ? BOUND_SINCOS : BOUND_LIBM, abs_term, x, 0);
            }
            all.push_back(s1); all.push_back(s2);
        }
        // atan_ratio
        for (const Span &c : in.at_c)
        {
            Stat s = fresh("atan_ratio", c), sa = fresh("atan alone, of the double n / w", c), sd = fresh("the division alone, n / w", c);
            for (size_t i = c.lo; i < c.hi; ++i)
            {
                const double n = in.at_n[i], d = in.at_d[i];
                judge(s, o.at[i], atanl((ld)n / (ld)d), dev ? BOUND_ATAN : BOUND_LIBM_ATAN_RATIO, 0, n, d);
                if (i >= in.at_zero_lo && i < in.at_zero_hi && !(o.at[i] == 0.0)) fail_note(s, "atan of a zero numerator must be a zero", n, o.at[i]);
                if (dev) continue;
                const double q = n / d;
                judge(sd, q, (ld)n / (ld)d, BOUND_EXACT, 0, n, d);
                if (std::isfinite(q)) judge(sa, o.at[i], atanl((ld)q), BOUND_LIBM, 0, q, 0);
            }
            all.push_back(s);
            if (!dev) { all.push_back(sa); all.push_back(sd); }
        }
        u64 bad = 0;
        for (const Stat &s : all) { print_stat(s); bad += s.bad; }
        if (dev)
        { // the premise of the derivations
            ld wr = 0, ws = 0;
            double ar = 0, as = 0;
            for (size_t i = 0; i < in.rcp_x.size(); ++i)
            {
                const ld t = 1.0L / (ld)in.rcp_x[i], e = fabsl(((ld)o.rcp_est[i] - t) / t);
                if (!(e <= wr)) { wr = e; ar = in.rcp_x[i]; }
            }
            for (size_t i = 0; i < in.sq_x.size(); ++i)
            {
                const ld t = 1.0L / sqrtl((ld)in.sq_x[i]), e = fabsl(((ld)o.sq_est[i] - t) / t);
                if (!(e <= ws)) { ws = e; as = in.sq_x[i]; }
            }
            printf("premise: v_rcp_f64 worst relative error %.3Le (2^%.1f) at %a, v_rsq_f64 %.3Le (2^%.1f) at %a; the derivations assume 2^-20\n", wr,
                   (double)log2l(wr), ar, ws, (double)log2l(ws), as);
            if (!(wr <= EST_PREMISE) || !(ws <= EST_PREMISE)) { printf("  OUTSIDE the premise of the derived bounds\n"); ++bad; }
        }
        return bad;
    }

    // ---- section 2: qlog<true>, qexp<true>, so3_exp ---------------------------------------------------------------------------------------
    // The reference's formulas (Quaternion.h: log, exp) branch for branch in long double, on the doubles the device gets.  M_PI is the
    // reference's double constant; the rational coefficients are those of the formulas (their rounding to double multiplies terms below
    // 1e-20 of the result).  Returns the branch.
    enum { LOG_SERIES = 0, LOG_PI = 1, LOG_GENERAL = 2, EXP_SERIES = 0, EXP_GENERAL = 1 };
    const char *const LOG_BRANCH[3] = {"sn < 1e-20", "|w| < 1e-10", "general"};
    const char *const EXP_BRANCH[2] = {"th2 < 1e-20", "general"};

    int ref_qlog(const double q[4], ld tg[3], ld J[12])
    {
        const ld x = q[0], y = q[1], z = q[2], w = q[3];
        const ld sn = x * x + y * y + z * z;
        ld lam, dx = 0, dy = 0, dz = 0, dw = 0;
        int branch;
        if (sn < 1e-20L)
        {
            branch = LOG_SERIES;
            const ld www = w * w * w;
            lam = 2.0L / w - 2.0L / 3.0L * sn / www;
            dx = 2.0L / w - 4.0L / 3.0L * x / www;
            dy = 2.0L / w - 4.0L / 3.0L * y / www;
            dz = 2.0L / w - 4.0L / 3.0L * z / www;
            dw = -2.0L / (w * w) + 2.0L * sn / (www * w);
        }
        else
        {
            const ld n = sqrtl(sn);
            if (fabsl(w) < 1e-10L)
            {
                branch = LOG_PI;
                const ld pi = (ld)3.14159265358979323846;
                lam = (w > 0 ? pi : -pi) / n;
                const ld s = (w > 0 ? -lam : lam) / sn;
                dx = s * x; dy = s * y; dz = s * z;
            }
            else
            {
                branch = LOG_GENERAL;
                lam = 2.0L * atanl(n / w) / n;
                const ld dn = (2.0L * w - lam) / n;
                dx = dn * x / n; dy = dn * y / n; dz = dn * z / n;
                dw = -2.0L;
            }
        }
        J[0] = dx * x + lam; J[1] = dy * x;       J[2] = dz * x;        J[3] = dw * x;
        J[4] = dx * y;       J[5] = dy * y + lam; J[6] = dz * y;        J[7] = dw * y;
        J[8] = dx * z;       J[9] = dy * z;       J[10] = dz * z + lam; J[11] = dw * z;
        tg[0] = lam * x; tg[1] = lam * y; tg[2] = lam * z;
        return branch;
    }

    int ref_qexp(const double t[3], ld q[4], ld J[12])
    {
        const ld x = t[0], y = t[1], z = t[2];
        const ld th2 = x * x + y * y + z * z;
        ld im, re;
        int branch;
        if (th2 < 1e-20L)
        {
            branch = EXP_SERIES;
            const ld th4 = th2 * th2;
            im = 0.5L - th2 / 48.0L + th4 / 3840.0L;
            re = 1.0L - th2 / 8.0L + th4 / 384.0L;
            for (int i = 0; i < 12; ++i) J[i] = 0;
            J[0] = J[4] = J[8] = 0.5L;
        }
        else
        {
            branch = EXP_GENERAL;
            const ld th = sqrtl(th2), hs = sinl(0.5L * th);
            im = hs / th;
            re = cosl(0.5L * th);
            const ld ux = x / th, uy = y / th, uz = z / th;
            const ld dim = 0.5L * re / th - im / th, dre = -0.5L * hs;
            const ld ax = dim * ux, ay = dim * uy, az = dim * uz;
            J[0] = ax * x + im; J[1] = ay * x;      J[2] = az * x;
            J[3] = ax * y;      J[4] = ay * y + im; J[5] = az * y;
            J[6] = ax * z;      J[7] = ay * z;      J[8] = az * z + im;
            J[9] = dre * ux;    J[10] = dre * uy;   J[11] = dre * uz;
        }
        q[0] = im * x; q[1] = im * y; q[2] = im * z; q[3] = re;
        return branch;
    }

    // largest element-wise error relative to the reference's largest element
    ld rel_err(const double *got, const ld *ref, int n)
    {
        ld m = 0, e = 0;
        for (int i = 0; i < n; ++i)
        {
            const ld d = fabsl((ld)got[i] - ref[i]);
            if (!(d == d)) return std::numeric_limits<ld>::infinity();
            if (d > e) e = d;
            if (fabsl(ref[i]) > m) m = fabsl(ref[i]);
        }
        return e / m;
    }

    struct Cases
    {
        std::vector<double> q, tg;       // 4 per logarithm case; 3 per exponential case (qexp and so3_exp)
        std::vector<double> qa, ta;      // the angle a case was made from (0: a threshold or branch case, outside the floor)
        std::vector<int> qx, tx;         // its axis
        u64 dropped = 0;                 // random cases closer than 1e-6 to a threshold
        size_t nq() const { return qa.size(); }
        size_t nt() const { return ta.size(); }
    };
    constexpr double MARGIN = 1e-6;
    bool near(double v, double threshold) { return std::fabs(v / threshold - 1.0) < MARGIN; }

    Cases make_cases()
    {
        Cases c;
        const double pi = 3.14159265358979323846;
        const double raw[3][3] = {{0.0, 0.0, 1.0}, {0.3, -0.5, 0.8}, {1e-8, -1e-8, 1.0}}; // coordinate, generic, two components 1e-8 of the third
        double axis[3][3];
        for (int a = 0; a < 3; ++a)
        {
            const double n = std::sqrt(raw[a][0] * raw[a][0] + raw[a][1] * raw[a][1] + raw[a][2] * raw[a][2]);
            for (int i = 0; i < 3; ++i) axis[a][i] = raw[a][i] / n;
        }
        auto put_q = [&](int a, double x, double y, double z, double w, double angle, bool fixed) {
            const double sn = x * x + y * y + z * z;
            if (!fixed && (near(sn, 1e-20) || near(std::fabs(w), 1e-10))) { ++c.dropped; return; }
            c.q.push_back(x); c.q.push_back(y); c.q.push_back(z); c.q.push_back(w);
            c.qa.push_back(angle); c.qx.push_back(a);
        };
        auto quat = [&](int a, double angle, double sign, double tag, bool fixed = false) {
            const double s = std::sin(0.5 * angle), w = std::cos(0.5 * angle);
            put_q(a, sign * s * axis[a][0], sign * s * axis[a][1], sign * s * axis[a][2], sign * w, tag, fixed);
        };
        auto put_t = [&](int a, double angle, double tag, bool fixed = false) {
            const double x = angle * axis[a][0], y = angle * axis[a][1], z = angle * axis[a][2];
            if (!fixed && near(x * x + y * y + z * z, 1e-20)) { ++c.dropped; return; }
            c.tg.push_back(x); c.tg.push_back(y); c.tg.push_back(z);
            c.ta.push_back(tag); c.tx.push_back(a);
        };
        // the angles of tests/pose_algebra_ref.py (its "pi", w == 0 exactly, is among the |w| < 1e-10 cases below)
        const double listed[18] = {1e-11, 0.99e-10, 1.01e-10, 1e-9, 1.5e-8, 3e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-2, 0.4, 1.1, 1.6, 2.2, 2.9, 3.1, pi - 1e-11};
        Rng r{21};
        for (int a = 0; a < 3; ++a)
        {
            for (double ang : listed) { quat(a, ang, 1.0, ang); put_t(a, ang, ang); }
            for (int i = 0; i < (1 << 16); ++i) { const double ang = r.loguniform(1e-12, pi); quat(a, ang, 1.0, ang); put_t(a, ang, ang); }
            for (int i = 0; i < (1 << 16); ++i)
            {
                const double ang = r.uniform(0.0, 2.0 * pi);
                if (!(ang > 0.0)) continue;
                quat(a, ang, 1.0, ang); put_t(a, ang, ang);
                if (ang > pi) { quat(a, ang, -1.0, ang); put_t(a, -ang, ang); } // the flip
            }
            // thresholds, at relative distances from 1e-6 (a hair more, so that the sums formed in double stay outside it) on both sides
            for (double dist : {1.0000001e-6, 2e-6, 1e-5, 1e-3})
                for (double side : {-1.0, 1.0})
                {
                    const double f = 1.0 + side * dist;
                    quat(a, 2.0 * std::asin(1e-10 * std::sqrt(f)), 1.0, 0.0, true);   // sn = 1e-20 f
                    put_t(a, 1e-10 * std::sqrt(f), 0.0, true);                          // th2 = 1e-20 f
                    for (double sg : {-1.0, 1.0})                                       // |w| = 1e-10 f
                        put_q(a, axis[a][0], axis[a][1], axis[a][2], sg * 1e-10 * f, 0.0, true);
                }
            // inside |w| < 1e-10: the branch no angle of a list reaches but pi itself
            put_q(a, axis[a][0], axis[a][1], axis[a][2], 0.0, 0.0, true);
            for (int i = 0; i < 64; ++i)
                for (double sg : {-1.0, 1.0}) put_q(a, axis[a][0], axis[a][1], axis[a][2], sg * r.loguniform(1e-18, 0.99e-10), 0.0, true);
        }
        // a fixed case must itself respect the margin (the sums as formed here, in double, without contraction)
        for (size_t i = 0; i < c.nq(); ++i)
        {
            const double *q = &c.q[4 * i];
            if (near(q[0] * q[0] + q[1] * q[1] + q[2] * q[2], 1e-20) || near(std::fabs(q[3]), 1e-10)) { printf("a logarithm case sits inside the margin\n"); exit(2); }
        }
        for (size_t i = 0; i < c.nt(); ++i)
        {
            const double *t = &c.tg[3 * i];
            if (near(t[0] * t[0] + t[1] * t[1] + t[2] * t[2], 1e-20)) { printf("an exponential case sits inside the margin\n"); exit(2); }
        }
        return c;
    }

    struct PoseOut
    {
        std::vector<double> log_tg, log_J, exp_q, exp_J, so3_q; // 3, 12 per logarithm case; 4, 12, 4 per exponential case
        void size(size_t nq, size_t nt) { log_tg.resize(3 * nq); log_J.resize(12 * nq); exp_q.resize(4 * nt); exp_J.resize(12 * nt); so3_q.resize(4 * nt); }
    };

    void host_half(const Cases &c, PoseOut &o)
    {
        o.size(c.nq(), c.nt());
        for (size_t i = 0; i < c.nq(); ++i)
        {
            mbavo::LogJac J;
            mbavo::qlog<true>(mbavo::load_quat(&c.q[4 * i]), &o.log_tg[3 * i], &J);
            memcpy(&o.log_J[12 * i], J.m, sizeof J.m);
        }
        for (size_t i = 0; i < c.nt(); ++i)
        {
            mbavo::ExpJac J;
            const mbavo::Quat q = mbavo::qexp<true>(&c.tg[3 * i], &J), s = mbavo::so3_exp(&c.tg[3 * i]);
            const double qv[4] = {q.x, q.y, q.z, q.w}, sv[4] = {s.x, s.y, s.z, s.w};
            memcpy(&o.exp_q[4 * i], qv, sizeof qv);
            memcpy(&o.exp_J[12 * i], J.m, sizeof J.m);
            memcpy(&o.so3_q[4 * i], sv, sizeof sv);
        }
    }

    // Per quantity and case: |device - ref| <= 4 max(host_err(case), floor), host_err = |host half - ref| on the case, floor the largest
    // host_err over the angles in [1e-2, 2.9] (the rule of tests/pose_algebra_ref.py), all relative to the case's largest entry.  No
    // case's bound may exceed CEILING: where the host half alone breaks that, the case is reported as a finding and the run fails.
    constexpr ld CEILING = 1e-13L;
    constexpr int NQUANT = 5;
    const char *const QUANT[NQUANT] = {"qlog tg", "qlog Jacobian", "qexp q", "qexp Jacobian", "so3_exp q"};

    u64 check_pose(const Cases &c, const PoseOut &host, const PoseOut *dev)
    {
        const size_t nq = c.nq(), nt = c.nt();
        std::vector<ld> herr[NQUANT], derr[NQUANT];
        std::vector<int> lbranch(nq), ebranch(nt);
        u64 log_count[3] = {0, 0, 0}, exp_count[2] = {0, 0};
        for (int k = 0; k < 2; ++k) { herr[k].resize(nq); derr[k].resize(nq); }
        for (int k = 2; k < NQUANT; ++k) { herr[k].resize(nt); derr[k].resize(nt); }
        for (size_t i = 0; i < nq; ++i)
        {
            ld tg[3], J[12];
            lbranch[i] = ref_qlog(&c.q[4 * i], tg, J);
            ++log_count[lbranch[i]];
            herr[0][i] = rel_err(&host.log_tg[3 * i], tg, 3);
            herr[1][i] = rel_err(&host.log_J[12 * i], J, 12);
            if (dev) { derr[0][i] = rel_err(&dev->log_tg[3 * i], tg, 3); derr[1][i] = rel_err(&dev->log_J[12 * i], J, 12); }
        }
        for (size_t i = 0; i < nt; ++i)
        {
            ld q[4], J[12];
            ebranch[i] = ref_qexp(&c.tg[3 * i], q, J);
            ++exp_count[ebranch[i]];
            herr[2][i] = rel_err(&host.exp_q[4 * i], q, 4);
            herr[3][i] = rel_err(&host.exp_J[12 * i], J, 12);
            herr[4][i] = rel_err(&host.so3_q[4 * i], q, 4); // (the same value: Sophus' series and closed form are the quaternion exponential's)
            if (dev) { derr[2][i] = rel_err(&dev->exp_q[4 * i], q, 4); derr[3][i] = rel_err(&dev->exp_J[12 * i], J, 12); derr[4][i] = rel_err(&dev->so3_q[4 * i], q, 4); }
        }
        u64 bad = 0;
        printf("section 2: %zu logarithm cases (%s %llu, %s %llu, %s %llu), %zu exponential cases (%s %llu, %s %llu); %llu random cases inside the "
               "1e-6 margin of a threshold left out\n", nq, LOG_BRANCH[0], log_count[0], LOG_BRANCH[1], log_count[1], LOG_BRANCH[2], log_count[2], nt,
               EXP_BRANCH[0], exp_count[0], EXP_BRANCH[1], exp_count[1], c.dropped);
        for (int b = 0; b < 3; ++b) if (log_count[b] < 100) { printf("  branch %s of qlog has fewer than 100 cases\n", LOG_BRANCH[b]); ++bad; }
        for (int b = 0; b < 2; ++b) if (exp_count[b] < 100) { printf("  branch %s of qexp has fewer than 100 cases\n", EXP_BRANCH[b]); ++bad; }
        for (int k = 0; k < NQUANT; ++k)
        {
            const bool is_log = k < 2;
            const size_t n = is_log ? nq : nt;
            const std::vector<double> &ang = is_log ? c.qa : c.ta;
            const std::vector<int> &br = is_log ? lbranch : ebranch;
            const int nb = is_log ? 3 : 2;
            ld floor_ = 0;
            for (size_t i = 0; i < n; ++i)
                if (ang[i] >= 1e-2 && ang[i] <= 2.9 && herr[k][i] > floor_) floor_ = herr[k][i];
            ld wh[3] = {0, 0, 0}, wd[3] = {0, 0, 0}, wshare = 0;
            u64 findings = 0, outside = 0;
            int notes = 0;
            for (size_t i = 0; i < n; ++i)
            {
                const int b = br[i];
                const ld h = herr[k][i], bound = 4.0L * (h > floor_ ? h : floor_);
                if (!(h <= wh[b])) wh[b] = h;
                const double *arg = is_log ? &c.q[4 * i] : &c.tg[3 * i];
                if (!(bound <= CEILING))
                {
                    ++findings;
                    if (notes++ < 4)
                        printf("  FINDING %s: the host half is %.3Le from the reference (bound %.3Le over the ceiling %.1Le): axis %d, arguments %a %a %a %a\n",
                               QUANT[k], h, bound, CEILING, (is_log ? c.qx : c.tx)[i], arg[0], arg[1], arg[2], is_log ? arg[3] : 0.0);
                }
                if (!dev) continue;
                const ld d = derr[k][i];
                if (!(d <= wd[b])) wd[b] = d;
                if (d / bound > wshare) wshare = d / bound;
                if (!(d <= bound))
                {
                    ++outside;
                    if (notes++ < 4)
                        printf("  OUTSIDE %s: device %.3Le, host half %.3Le, bound %.3Le: axis %d, branch %s, arguments %a %a %a %a\n", QUANT[k], d, h, bound,
                               (is_log ? c.qx : c.tx)[i], is_log ? LOG_BRANCH[b] : EXP_BRANCH[b], arg[0], arg[1], arg[2], is_log ? arg[3] : 0.0);
                }
            }
            printf("%-14s cases %7zu  floor %.3Le  worst per branch", QUANT[k], n, floor_);
            for (int b = 0; b < nb; ++b)
            {
                printf("  [%s] host %.3Le", is_log ? LOG_BRANCH[b] : EXP_BRANCH[b], wh[b]);
                if (dev) printf(" device %.3Le", wd[b]);
            }
            if (dev) printf("  worst device share of its bound %.3Lf", wshare);
            printf("  over the ceiling %llu  outside %llu\n", findings, outside);
            bad += findings + outside;
        }
        return bad;
    }

#if defined(__HIPCC__)
    // ---- the device side: pure arithmetic, lane i reads and writes element i (or its 3, 4, 12 elements) of its own arrays, i < n ----------
    __global__ void k_rcp(const double *x, double *out, double *est, unsigned n)
    {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
        out[i] = mbavo::fastm::rcp(x[i]);
        est[i] = __builtin_amdgcn_rcp(x[i]);
#endif
    }
    __global__ void k_sqrt_rsqrt(const double *x, double *s, double *r, double *est, unsigned n)
    {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
        double a, b;
        mbavo::fastm::sqrt_rsqrt(x[i], a, b);
        s[i] = a; r[i] = b;
        est[i] = __builtin_amdgcn_rsq(x[i]);
#endif
    }
    __global__ void k_sincos(const double *x, double *sn, double *cs, unsigned n)
    {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
        double a, b;
        mbavo::fastm::sincos(x[i], a, b);
        sn[i] = a; cs[i] = b;
#endif
    }
    __global__ void k_atan_ratio(const double *num, const double *den, double *out, unsigned n)
    {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
        out[i] = mbavo::fastm::atan_ratio(num[i], den[i]);
#endif
    }
    __global__ void k_qlog(const double *q, double *tg, double *J, unsigned n)
    {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        mbavo::LogJac lj;
        double t[3];
        mbavo::qlog<true>(mbavo::load_quat(q + 4 * (size_t)i), t, &lj);
        for (int a = 0; a < 3; ++a) tg[3 * (size_t)i + a] = t[a];
        for (int a = 0; a < 12; ++a) J[12 * (size_t)i + a] = lj.m[a];
    }
    __global__ void k_qexp(const double *tg, double *q, double *J, double *so3, unsigned n)
    {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        mbavo::ExpJac ej;
        const double t[3] = {tg[3 * (size_t)i], tg[3 * (size_t)i + 1], tg[3 * (size_t)i + 2]};
        const mbavo::Quat a = mbavo::qexp<true>(t, &ej), b = mbavo::so3_exp(t);
        q[4 * (size_t)i] = a.x; q[4 * (size_t)i + 1] = a.y; q[4 * (size_t)i + 2] = a.z; q[4 * (size_t)i + 3] = a.w;
        so3[4 * (size_t)i] = b.x; so3[4 * (size_t)i + 1] = b.y; so3[4 * (size_t)i + 2] = b.z; so3[4 * (size_t)i + 3] = b.w;
        for (int k = 0; k < 12; ++k) J[12 * (size_t)i + k] = ej.m[k];
    }

#define HIP_OK(call)                                                                                      \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); return false; }         \
    } while (0)

    bool upload(const std::vector<double> &v, double *&d)
    {
        HIP_OK(hipMalloc((void **)&d, v.size() * sizeof(double)));
        HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
        return true;
    }
    bool blank(size_t count, double *&d)
    {
        HIP_OK(hipMalloc((void **)&d, count * sizeof(double)));
        HIP_OK(hipMemset(d, 0xcd, count * sizeof(double))); // a lane that writes nothing is seen
        return true;
    }
    bool download(std::vector<double> &v, size_t count, double *d)
    {
        v.resize(count);
        HIP_OK(hipMemcpy(v.data(), d, count * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d));
        return true;
    }
    dim3 grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

    bool run_device(const Inputs &in, const Cases &c, Results &o, PoseOut &p)
    {
        o.device = true;
        double *x = nullptr, *y = nullptr, *a = nullptr, *b = nullptr, *e = nullptr, *f = nullptr;
        size_t n = in.rcp_x.size();
        if (!upload(in.rcp_x, x) || !blank(n, a) || !blank(n, e)) return false;
        hipLaunchKernelGGL(k_rcp, grid(n), dim3(256), 0, 0, x, a, e, (unsigned)n);
        HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
        if (!download(o.rcp, n, a) || !download(o.rcp_est, n, e)) return false;
        HIP_OK(hipFree(x));

        n = in.sq_x.size();
        if (!upload(in.sq_x, x) || !blank(n, a) || !blank(n, b) || !blank(n, e)) return false;
        hipLaunchKernelGGL(k_sqrt_rsqrt, grid(n), dim3(256), 0, 0, x, a, b, e, (unsigned)n);
        HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
        if (!download(o.sq_s, n, a) || !download(o.sq_r, n, b) || !download(o.sq_est, n, e)) return false;
        HIP_OK(hipFree(x));

        n = in.sc_x.size();
        if (!upload(in.sc_x, x) || !blank(n, a) || !blank(n, b)) return false;
        hipLaunchKernelGGL(k_sincos, grid(n), dim3(256), 0, 0, x, a, b, (unsigned)n);
        HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
        if (!download(o.sn, n, a) || !download(o.cs, n, b)) return false;
        HIP_OK(hipFree(x));

        n = in.at_n.size();
        if (!upload(in.at_n, x) || !upload(in.at_d, y) || !blank(n, a)) return false;
        hipLaunchKernelGGL(k_atan_ratio, grid(n), dim3(256), 0, 0, x, y, a, (unsigned)n);
        HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
        if (!download(o.at, n, a)) return false;
        HIP_OK(hipFree(x)); HIP_OK(hipFree(y));

        n = c.nq();
        if (!upload(c.q, x) || !blank(3 * n, a) || !blank(12 * n, b)) return false;
        hipLaunchKernelGGL(k_qlog, grid(n), dim3(256), 0, 0, x, a, b, (unsigned)n);
        HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
        if (!download(p.log_tg, 3 * n, a) || !download(p.log_J, 12 * n, b)) return false;
        HIP_OK(hipFree(x));

        n = c.nt();
        if (!upload(c.tg, x) || !blank(4 * n, a) || !blank(12 * n, b) || !blank(4 * n, f)) return false;
        hipLaunchKernelGGL(k_qexp, grid(n), dim3(256), 0, 0, x, a, b, f, (unsigned)n);
        HIP_OK(hipGetLastError()); HIP_OK(hipDeviceSynchronize());
        if (!download(p.exp_q, 4 * n, a) || !download(p.exp_J, 12 * n, b) || !download(p.so3_q, 4 * n, f)) return false;
        HIP_OK(hipFree(x));
        return true;
    }
#else
    bool run_device(const Inputs &, const Cases &, Results &, PoseOut &) { return false; }
#endif

    double seconds_since(std::chrono::steady_clock::time_point t0)
    {
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
} // namespace

int main(int argc, char **argv)
{
    bool host_mode = false;
    for (int i = 1; i < argc; ++i)
    {
        if (!strcmp(argv[i], "--host")) host_mode = true;
        else { printf("usage: %s [--host]\n", argv[0]); return 2; }
    }
#if !defined(__HIPCC__)
    if (!host_mode) { printf("built without the device side: only --host\n"); return 2; }
#endif
    const auto t_start = std::chrono::steady_clock::now();
    const Inputs in = make_inputs();
    const Cases cases = make_cases();
    printf("fastm_check (%s): rcp %zu, sqrt_rsqrt %zu, sincos %zu, atan_ratio %zu arguments; |pi/2 - (c1 + c2)| = %.6Le\n",
           host_mode ? "--host: no device, libm and IEEE in the forms' place" : "device", in.rcp_x.size(), in.sq_x.size(), in.sc_x.size(), in.at_n.size(), SC_D);
    if (!(SC_D > 3.5e-27L && SC_D < 3.54e-27L)) { printf("the reduction constants' error is not the 3.52e-27 the header's literals give\nFASTM CHECK FAILED\n"); return 1; }

    Results res;
    PoseOut host, dev;
    double t_device = 0;
    if (host_mode) host_results(in, res);
    else
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (!run_device(in, cases, res, dev)) { printf("FASTM CHECK FAILED (device run)\n"); return 3; }
        t_device = seconds_since(t0);
    }
    const auto t_verify = std::chrono::steady_clock::now();
    u64 bad = check_forms(in, res);
    host_half(cases, host);
    bad += check_pose(cases, host, host_mode ? nullptr : &dev);
    printf("total: %llu outside; device phase %.2f s, host references %.2f s, whole run %.2f s\n", bad, t_device, seconds_since(t_verify), seconds_since(t_start));
    if (bad) { printf("FASTM CHECK FAILED\n"); return 1; }
    printf("FASTM CHECK PASSED\n");
    return 0;
}
