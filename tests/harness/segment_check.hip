// se3_math.h: spline_segment_checked / spline_segment_index -- the one range gate between a caller's time stamps and the knot
// addresses knots_t + 3 * idx, knots_R + 4 * idx -- and pose_entries.h: pose_sample_segment<2> / <4>, which forms a blur sample's
// time and passes it through the gate, called DIRECTLY, one lane per case, on the device and (the gate) through its host half,
// against an exact reference on the host:
//   tn = (t - t0) / dt with the same two double operations, contraction off;
//   in range  iff  tn is finite and, with i = (long long)truncl(tn) (only formed where it fits), i >= 0 && i + KD <= N;
//   idx = i, u = the double tn - i;
//   the saturated index: i held to [INT_MIN, INT_MAX], INT_MIN for NaN.
// Asserted: the flag is the reference's; 0 <= idx <= N - KD for EVERY case, in range or not (what makes idx safe to index knots
// with); in range, idx and u are the reference's bits; the host half and the device give identical bits for every case (idx, u,
// flag, saturated index); the sample time of pose_sample_segment (cap - exp / 2 + s exp / (S - 1 + 1e-8)) is recomputed on the
// host with the same operations.  The kernel reads NO knots: it stores idx, u and the flag and cannot fault whatever the gate says.
//
// Cases, per (t0, dt) of {0, -3.5, 1.7e9} x {0.5, 1/30, 1e-3}, KD of {2, 4}, N of {KD, KD + 1, 7, 2^20}: targets tn*, each as
// t = t0 + tn* dt and the doubles on both sides of it -- the integers -2, -1, 0, 1, N-KD-1, N-KD, N-KD+1, N and the doubles on both
// sides of each; -0.0, +-the smallest denormal, +-the smallest normal; 2^31 - 5 .. 2^31 + 1; +-{2^32, 2^32 + 0.5, 2^53, 2^63, 2^64,
// 1e300, DBL_MAX}; +-inf, NaN of both signs --, 2^20 random times uniform over [-2, N + 2] segments, and for pose_sample_segment
// every target as the capture time with S of {1, 2, 8, 21}, every sample, and exposures {0, 0.1, NaN, inf, 1e300}.
//
//   segment_check_bin           everything, the device included
//   segment_check_bin --host    the host half against the reference (no HIP call is made): for the host sanitizers
#include <hip/hip_runtime.h>
#include <chrono>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "pose_entries.h"

namespace
{
    typedef unsigned long long u64;
    enum { C_INTEGER, C_ZERO, C_EDGE31, C_FAR, C_NONFINITE, C_RANDOM, C_POSE, NCLS };
    const char *const CLS_NAME[NCLS] = {"integers and the doubles beside them", "round zero", "round 2^31", "far", "inf and NaN",
                                        "random", "pose_sample_segment"};

    struct Combo { double t0, dt; int N, KD; };
    // S == 0: the gate itself at time t.  S > 0: pose_sample_segment, t the capture time, ex the exposure, sample smp of S.
    struct Case { double t, ex; unsigned short combo; unsigned char S, smp, cls, pad[3]; };
    struct Out { double u; int idx, sat, flag, pad; };
    static_assert(sizeof(Case) == 24 && sizeof(Out) == 24, "packed as the kernel reads them");

    u64 bits(double d) { u64 b; memcpy(&b, &d, 8); return b; }
    double from_bits(u64 b) { double d; memcpy(&d, &b, 8); return d; }

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
    };

    // ---- the exact reference ----------------------------------------------------------------------------------------------
    double ref_tn(double t, double t0, double dt)
    {
#pragma clang fp contract(off)
        const double d = t - t0;
        return d / dt;
    }
    double ref_sample_time(double cap, double ex, int S, int smp)
    {
#pragma clang fp contract(off)
        const double half = ex * 0.5, a = cap - half;
        const double num = (double)smp * ex, den = (double)(S - 1) + 1e-8;
        const double q = num / den;
        return a + q;
    }
    struct Ref { bool in; long long idx; double u; int sat; };
    Ref reference(double t, const Combo &c)
    {
#pragma clang fp contract(off)
        Ref r = {false, 0, 0.0, INT_MIN};
        const double tn = ref_tn(t, c.t0, c.dt);
        if (tn != tn) return r;
        const long double tr = truncl((long double)tn);
        if (!std::isfinite(tn) || fabsl(tr) >= 4611686018427387904.0L) // 2^62: beyond any int count, and (long long) must fit
        {
            r.sat = tn > 0 ? INT_MAX : INT_MIN;
            return r;
        }
        const long long i = (long long)tr;
        r.sat = i > (long long)INT_MAX ? INT_MAX : i < (long long)INT_MIN ? INT_MIN : (int)i;
        r.in = i >= 0 && i + (long long)c.KD <= (long long)c.N;
        r.idx = i;
        if (r.in) r.u = tn - (double)i;
        return r;
    }

    // ---- the header's host half -------------------------------------------------------------------------------------------
    Out host_half(double t, const Combo &c)
    {
        Out o = {0.0, 0, 0, 0, 0};
        o.flag = mbavo::spline_segment_checked(t, c.t0, c.dt, c.N, c.KD, o.idx, o.u) ? 1 : 0;
        o.sat = mbavo::spline_segment_index(t, c.t0, c.dt);
        return o;
    }

    // ---- the cases ----------------------------------------------------------------------------------------------------------
    struct Target { double tn; int cls; };
    std::vector<Target> targets(const Combo &c)
    {
        const double inf = std::numeric_limits<double>::infinity();
        std::vector<Target> v;
        for (int j : {-2, -1, 0, 1, c.N - c.KD - 1, c.N - c.KD, c.N - c.KD + 1, c.N})
            for (double d : {std::nextafter((double)j, -inf), (double)j, std::nextafter((double)j, inf)}) v.push_back({d, C_INTEGER});
        for (double d : {-0.0, DBL_TRUE_MIN, -DBL_TRUE_MIN, DBL_MIN, -DBL_MIN}) v.push_back({d, C_ZERO});
        for (int j = -5; j <= 1; ++j) v.push_back({2147483648.0 + j, C_EDGE31});
        for (double d : {4294967296.0, 4294967296.5, 9007199254740992.0, 9223372036854775808.0, 18446744073709551616.0, 1e300, DBL_MAX})
        {
            v.push_back({d, C_FAR});
            v.push_back({-d, C_FAR});
        }
        v.push_back({inf, C_NONFINITE});
        v.push_back({-inf, C_NONFINITE});
        v.push_back({from_bits(0x7ff8000000000000ull), C_NONFINITE});
        v.push_back({from_bits(0xfff8000000000000ull), C_NONFINITE});
        return v;
    }
    // target tn* as a time and the doubles on both sides of it (t0 == 0: the product alone, so that -0.0 keeps its sign)
    void times_of(double tn, const Combo &c, double t[3])
    {
        const double inf = std::numeric_limits<double>::infinity();
        t[1] = c.t0 == 0.0 ? tn * c.dt : c.t0 + tn * c.dt;
        t[0] = std::nextafter(t[1], -inf);
        t[2] = std::nextafter(t[1], inf);
    }

    const int SAMPLES[4] = {1, 2, 8, 21};

    void make_cases(const std::vector<Combo> &combos, int first, int count, u64 seed, std::vector<Case> &cases)
    {
        const double inf = std::numeric_limits<double>::infinity();
        const double exposures[5] = {0.0, 0.1, from_bits(0x7ff8000000000000ull), inf, 1e300};
        cases.clear();
        for (int ci = first; ci < first + count; ++ci)
        {
            const Combo &c = combos[ci];
            for (const Target &tg : targets(c))
            {
                double t[3];
                times_of(tg.tn, c, t);
                for (int k = 0; k < 3; ++k)
                {
                    cases.push_back(Case{t[k], 0.0, (unsigned short)ci, 0, 0, (unsigned char)tg.cls, {0, 0, 0}});
                    for (int S : SAMPLES)
                        for (int smp = 0; smp < S; ++smp)
                            for (double ex : exposures)
                                cases.push_back(Case{t[k], ex, (unsigned short)ci, (unsigned char)S, (unsigned char)smp, C_POSE, {0, 0, 0}});
                }
            }
        }
        Rng r{seed};
        for (int i = 0; i < (1 << 20); ++i)
        { // uniform over [-2, N + 2] segments of one of the (KD, N) of this (t0, dt)
            const int ci = first + (int)(r.next() % (u64)count);
            const Combo &c = combos[ci];
            const double x = -2.0 + r.unit() * (c.N + 4.0);
            cases.push_back(Case{c.t0 + x * c.dt, 0.0, (unsigned short)ci, 0, 0, C_RANDOM, {0, 0, 0}});
        }
    }

    // ---- the device side ----------------------------------------------------------------------------------------------------
    __global__ void k_segment(const Case *__restrict__ cases, const Combo *__restrict__ combos, unsigned n, Out *__restrict__ out)
    {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        const Case &cs = cases[i];
        const Combo c = combos[cs.combo];
        Out o = {0.0, 0, 0, 0, 0};
        if (cs.S == 0)
        {
            o.flag = mbavo::spline_segment_checked(cs.t, c.t0, c.dt, c.N, c.KD, o.idx, o.u) ? 1 : 0;
            o.sat = mbavo::spline_segment_index(cs.t, c.t0, c.dt);
        }
        else
        { // a descriptor whose cap and exp_t are valid one-element arrays; nothing else of it is read
            mbavo::ProblemDesc d;
            memset(&d, 0, sizeof d);
            d.cap = &cs.t; d.exp_t = &cs.ex; d.t0 = c.t0; d.dt = c.dt; d.S = cs.S; d.F = 1; d.N = c.N;
            bool oob;
            if (c.KD == 2) mbavo::pose_sample_segment<2>(d, 0, cs.smp, o.idx, o.u, oob);
            else mbavo::pose_sample_segment<4>(d, 0, cs.smp, o.idx, o.u, oob);
            o.flag = oob ? 0 : 1;
        }
        out[i] = o;
    }

#define HIP_OK(call)                                                                                      \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); return false; }         \
    } while (0)

    struct DeviceBuffers { Case *cases = nullptr; Combo *combos = nullptr; Out *out = nullptr; size_t room = 0; };

    bool run_device(DeviceBuffers &b, const std::vector<Combo> &combos, const std::vector<Case> &cases, std::vector<Out> &out)
    {
        const size_t n = cases.size();
        if (!b.combos)
        {
            HIP_OK(hipMalloc((void **)&b.combos, combos.size() * sizeof(Combo)));
            HIP_OK(hipMemcpy(b.combos, combos.data(), combos.size() * sizeof(Combo), hipMemcpyHostToDevice));
        }
        if (b.room < n)
        {
            if (b.cases) { HIP_OK(hipFree(b.cases)); HIP_OK(hipFree(b.out)); }
            HIP_OK(hipMalloc((void **)&b.cases, n * sizeof(Case)));
            HIP_OK(hipMalloc((void **)&b.out, n * sizeof(Out)));
            b.room = n;
        }
        HIP_OK(hipMemcpy(b.cases, cases.data(), n * sizeof(Case), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(b.out, 0xcd, n * sizeof(Out))); // a lane that writes nothing is seen: its flag is neither 0 nor 1
        hipLaunchKernelGGL(k_segment, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, b.cases, b.combos, (unsigned)n, b.out);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        out.resize(n);
        HIP_OK(hipMemcpy(out.data(), b.out, n * sizeof(Out), hipMemcpyDeviceToHost));
        return true;
    }
    bool release(DeviceBuffers &b)
    {
        if (b.cases) { HIP_OK(hipFree(b.cases)); HIP_OK(hipFree(b.out)); }
        if (b.combos) HIP_OK(hipFree(b.combos));
        return true;
    }

    // ---- verification -------------------------------------------------------------------------------------------------------
    struct Tally
    {
        u64 cases[NCLS] = {0}, in_range[NCLS] = {0}, bad[NCLS] = {0};
        u64 at_minus_one = 0, at_upper = 0, between = 0; // tn == -1 exactly, tn == N - KD + 1 exactly, tn in (-1, 0)
        std::vector<std::string> first;
        void note(const char *who, const char *what, const Case &cs, const Combo &c, double t, const Out &got, const Ref &want)
        {
            if (first.size() >= 8) return;
            char buf[512];
            snprintf(buf, sizeof buf, "  MISMATCH %s, %s: class %s, t = %a (cap %a, exp %a, S %d, sample %d), t0 = %a, dt = %a, N = %d, KD = %d: "
                     "got flag %d idx %d u %a index %d, reference in range %d idx %lld u %a index %d", who, what, CLS_NAME[cs.cls], t, cs.t, cs.ex,
                     cs.S, cs.smp, c.t0, c.dt, c.N, c.KD, got.flag, got.idx, got.u, got.sat, (int)want.in, want.idx, want.u, want.sat);
            first.push_back(buf);
        }
    };

    // `got` (the host half or the device) against the reference; false on any difference
    bool against_reference(Tally &ta, const char *who, const Case &cs, const Combo &c, double t, const Out &got, const Ref &want)
    {
        bool ok = true;
        if (got.flag != (want.in ? 1 : 0)) { ta.note(who, "the flag", cs, c, t, got, want); ok = false; }
        if (!(got.idx >= 0 && got.idx <= c.N - c.KD)) { ta.note(who, "idx outside [0, N - KD]", cs, c, t, got, want); ok = false; }
        if (want.in && ((long long)got.idx != want.idx || bits(got.u) != bits(want.u))) { ta.note(who, "idx or u in range", cs, c, t, got, want); ok = false; }
        if (cs.S == 0 && got.sat != want.sat) { ta.note(who, "the saturated index", cs, c, t, got, want); ok = false; }
        return ok;
    }

    void verify(const std::vector<Combo> &combos, const std::vector<Case> &cases, const std::vector<Out> *dev, Tally &ta)
    {
        for (size_t i = 0; i < cases.size(); ++i)
        {
            const Case &cs = cases[i];
            const Combo &c = combos[cs.combo];
            const double t = cs.S == 0 ? cs.t : ref_sample_time(cs.t, cs.ex, cs.S, cs.smp);
            const Ref want = reference(t, c);
            Out h = host_half(t, c);
            if (cs.S != 0) h.sat = 0; // (pose_sample_segment has no saturated index: the device lane leaves 0)
            bool ok = against_reference(ta, "host half", cs, c, t, h, want);
            if (dev)
            {
                const Out &d = (*dev)[i];
                ok = against_reference(ta, "device", cs, c, t, d, want) && ok;
                if (d.flag != h.flag || d.idx != h.idx || bits(d.u) != bits(h.u) || d.sat != h.sat)
                {
                    ta.note("device (got) against the host half", "bits", cs, c, t, d, Ref{h.flag == 1, h.idx, h.u, h.sat});
                    ok = false;
                }
            }
            ++ta.cases[cs.cls];
            ta.in_range[cs.cls] += want.in;
            ta.bad[cs.cls] += !ok;
            const double tn = ref_tn(t, c.t0, c.dt);
            ta.at_minus_one += tn == -1.0;
            ta.at_upper += tn == (double)(c.N - c.KD + 1);
            ta.between += tn > -1.0 && tn < 0.0;
        }
    }

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
    const auto t_start = std::chrono::steady_clock::now();
    const double t0s[3] = {0.0, -3.5, 1.7e9}, dts[3] = {0.5, 1.0 / 30.0, 1e-3};
    std::vector<Combo> combos; // 8 (KD, N) per (t0, dt), (t0, dt)-major
    for (double t0 : t0s)
        for (double dt : dts)
            for (int KD : {2, 4})
                for (int N : {KD, KD + 1, 7, 1 << 20}) combos.push_back(Combo{t0, dt, N, KD});
    printf("segment_check (%s): %zu (t0, dt, KD, N), %zu targets x 3 times each, 2^20 random times per (t0, dt)\n",
           host_mode ? "--host: no device" : "device and host", combos.size(), targets(combos[0]).size());

    Tally ta;
    DeviceBuffers buf;
    std::vector<Case> cases;
    std::vector<Out> dev;
    double t_device = 0;
    for (int g = 0; g < 9; ++g)
    {
        make_cases(combos, 8 * g, 8, 7000 + g, cases);
        if (!host_mode)
        {
            const auto t0 = std::chrono::steady_clock::now();
            if (!run_device(buf, combos, cases, dev)) { printf("SEGMENT CHECK FAILED (device run)\n"); return 3; }
            t_device += seconds_since(t0);
        }
        verify(combos, cases, host_mode ? nullptr : &dev, ta);
    }
    if (!host_mode && !release(buf)) { printf("SEGMENT CHECK FAILED (device run)\n"); return 3; }

    u64 failures = 0, total = 0, empty = 0;
    for (int k = 0; k < NCLS; ++k)
    {
        printf("class %-38s cases %9llu  in range %9llu  out of range %9llu  failures %llu\n", CLS_NAME[k], ta.cases[k], ta.in_range[k],
               ta.cases[k] - ta.in_range[k], ta.bad[k]);
        failures += ta.bad[k];
        total += ta.cases[k];
        empty += ta.cases[k] == 0;
    }
    printf("cases with tn == -1 exactly %llu, tn == N - KD + 1 exactly %llu, tn in (-1, 0) %llu\n", ta.at_minus_one, ta.at_upper, ta.between);
    for (const std::string &s : ta.first) printf("%s\n", s.c_str());
    printf("total: %llu cases, %llu failures; device phase %.2f s, whole run %.2f s\n", total, failures, t_device, seconds_since(t_start));
    if (empty || !ta.at_minus_one || !ta.at_upper || !ta.between)
    {
        printf("SEGMENT CHECK FAILED (an empty class of cases)\n");
        return 1;
    }
    if (failures) { printf("SEGMENT CHECK FAILED\n"); return 1; }
    printf("SEGMENT CHECK PASSED\n");
    return 0;
}
