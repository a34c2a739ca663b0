// pixel_math.h: tap_fetch / tap_blend -- the bilinear keyframe tap behind bilinear_tap, sample_eval, the engine's pixel body
// and the pairs depth evaluation -- called DIRECTLY, at exactly chosen coordinates, in its four variants (cost-only, float
// pairs, half pairs, packed keyframe words), on the device and through its host half, against
//   A  a plain host restatement of the reference's definition (compute_pixel_intensity.h:40-68: inclusive bounds test, float
//      weights, float accumulation in the order w11 I11 + w10 I10 + w01 I01 + w00 I00, no contraction) that decodes the
//      image formats from their documented bit layouts with its own code: BIT FOR BIT, every coordinate, no tolerance;
//   B  the real-number bilinear interpolant in long double, inside a bound derived from the operation count (below):
//      guards A against a misreading of the definition that A and the header would share;
//   the host half of the header (tap_fetch / tap_blend / bilinear_tap compiled for the host): the same bits as the device;
//   each other: val is the same bits in all four variants and gx, gy in the three gradient variants (the header's claim
//      that the packed word and the half pairs lose nothing).
// Images are the smallest at which each branch exists, sit at offsets that defeat natural alignment inside a larger buffer
// whose margins hold values unlike the edge pixels next to them, and carry 0/255 checkerboards, random bytes and gradient
// planes filled independently of the intensities; a sweep image holds every (kx, ky) in [-255, 255]^2 beside six intensities.
//
//   tap_check_bin           everything, the device included
//   tap_check_bin --host    everything that needs no GPU (no HIP call is made): A, B, the host half, the sweep for the host
//                           half; images are allocated at their exact size with malloc and no margin, so that a read outside
//                           an image is a heap overflow for the host sanitizers (the file also compiles as plain C++).
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
#include <thread>
#include <vector>
#include "pixel_math.h"

namespace
{
    typedef unsigned long long u64;
    constexpr int NV = 4; // variant v: 0 cost-only <false, 0>, 1 float pairs <true, 0>, 2 half pairs <true, 1>, 3 packed words <true, 2>
    const char *const VNAME[NV] = {"cost", "float", "half", "packed"};

    // Bound on |result - B|, u = 2^-24 the unit roundoff of fp32, M the largest pixel value (255; 127.5 for a gradient).
    // Weights (every rounded value is <= 1 in magnitude, so every rounding is <= u):
    //   dx = fl(x - xi), dy likewise: the difference is exact in double, its conversion adds              u   each
    //   dxdy = fl(dx dy): the errors of dx and dy and one rounding                                         3u
    //   w11 = dxdy                                                                                         3u
    //   w01 = fl(dx - dxdy), w10 = fl(dy - dxdy): u + 3u and one rounding                                  5u   each
    //   w00 = fl(fl(fl(1 - dx) - dy) + dxdy): (u + u) + (u + u) + (3u + u)                                 8u
    //   the four weight errors together, each multiplying a pixel value <= M                              21u M
    // Blend (the exact weighted sum of values <= M with weights that sum to 1 is <= M, and so is every partial sum, up
    // to the weight errors above): four products and three sums, each rounded once                         7u M
    // The packed variant blends the doubled differences (<= 255) and halves the result, which is exact: 28u 255 / 2, the
    // same.  The conversions to double are exact.  Second-order terms, products that round in the subnormal range (2^-149
    // each) and B's own long-double rounding (2^-63 relative) are covered by the factor 1 + 2^-10.
    //   bound = 28 * 2^-24 * M * (1 + 2^-10):   4.26e-4 for the intensity, 2.13e-4 for a gradient
    constexpr long double U32 = 1.0L / 16777216.0L;
    constexpr long double BOUND_VAL = 28.0L * U32 * 255.0L * (1.0L + 1.0L / 1024.0L);
    constexpr long double BOUND_GRAD = 28.0L * U32 * 127.5L * (1.0L + 1.0L / 1024.0L);
    // Where a blend weight is subnormal (a coordinate closer than 2^-126 to a pixel centre, the "tiny" coordinates below) the
    // formats cannot agree to the bit: each of the four products w * (0.5 k) of the float and half variants rounds at 2^-149
    // (error <= 2^-150) where the packed variant's w * k is exact or rounds once after the halving.  Their gradients agree
    // within 4 * 2^-150 there; everywhere else the bits are equal.
    const double TINY_CROSS = std::ldexp(1.0, -148);

    struct Pix { int I, kx, ky; }; // intensity and DOUBLED central differences, |k| <= 255

    struct Image
    {
        std::string name;
        int H = 0, W = 0;
        long off = 0, total = 0; // pixels of margin in front of the image, pixels allocated (host mode: 0, H * W)
        std::vector<Pix> px;     // the H * W logical pixels
        unsigned char *base[4] = {nullptr, nullptr, nullptr, nullptr}; // allocations: u8, float pairs, half pairs, packed words
        size_t bytes[4] = {0, 0, 0, 0};
        unsigned char *I = nullptr, *Gf = nullptr, *Gh = nullptr, *Gp = nullptr; // the image origins inside them (as bytes)
        unsigned char *dbase[4] = {nullptr, nullptr, nullptr, nullptr};           // device copies
        u64 word_mismatch = 0; // pack_keyframe_word against the documented layout
    };
    const size_t PIXBYTES[4] = {1, 8, 4, 4};

    int flip(int k) { return k > 0 ? k - 256 : k + 255; } // another value of [-255, 255], never k itself

    // pixel q of the allocation, q in [-off, total - off): the image, or a margin pixel unlike the edge pixel of its column
    Pix ext_pixel(const Image &im, long q)
    {
        const long n = (long)im.H * im.W;
        if (q >= 0 && q < n) return im.px[(size_t)q];
        const long col = ((q % im.W) + im.W) % im.W;
        const Pix e = im.px[(size_t)(q < 0 ? col : n - im.W + col)];
        return Pix{e.I ^ 0x80, flip(e.kx), flip(e.ky)};
    }

    unsigned short half_bits(float v)
    {
        const _Float16 h = (_Float16)v;
        unsigned short b;
        memcpy(&b, &h, 2);
        return b;
    }

    // the four formats of one pixel, from the documented layouts: u8; float pairs 0.5 k; half pairs of that; one word with
    // bits 0-7 I, bits 8-16 kx and bits 23-31 ky as 9-bit two's complement
    void store_pixel(Image &im, long q, const Pix &p)
    {
        im.I[q] = (unsigned char)p.I;
        const float g[2] = {0.5f * (float)p.kx, 0.5f * (float)p.ky};
        memcpy(im.Gf + q * 8, g, 8);
        const unsigned short h[2] = {half_bits(g[0]), half_bits(g[1])};
        memcpy(im.Gh + q * 4, h, 4);
        const unsigned fx = (unsigned)(p.kx < 0 ? p.kx + 512 : p.kx), fy = (unsigned)(p.ky < 0 ? p.ky + 512 : p.ky);
        const unsigned w = (unsigned)p.I + fx * 256u + fy * 8388608u;
        memcpy(im.Gp + q * 4, &w, 4);
        if (mbavo::pack_keyframe_word(p.I, p.kx, p.ky) != w) ++im.word_mismatch;
    }

    // Host mode: every format at its exact size from malloc.  Otherwise: inside a 256-byte aligned allocation (as hipMalloc
    // gives) at `off` pixels, off = 1 (mod 4) and >= W + 2: the u8 image starts 1 byte off a word, the half and packed images
    // 4 bytes off an 8-byte boundary, the float image 8 bytes off a 16-byte boundary; W + 2 pixels of margin or more follow.
    bool allocate(Image &im, bool host_mode)
    {
        const long n = (long)im.H * im.W;
        if (host_mode) { im.off = 0; im.total = n; }
        else
        {
            im.off = im.W + 2;
            while (im.off % 4 != 1) ++im.off;
            im.total = im.off + n + im.W + 2 + 3;
        }
        for (int f = 0; f < 4; ++f)
        {
            im.bytes[f] = (size_t)im.total * PIXBYTES[f];
            im.base[f] = (unsigned char *)(host_mode ? malloc(im.bytes[f]) : aligned_alloc(256, (im.bytes[f] + 255) / 256 * 256));
            if (!im.base[f]) return false;
        }
        im.I = im.base[0] + im.off;
        im.Gf = im.base[1] + im.off * 8;
        im.Gh = im.base[2] + im.off * 4;
        im.Gp = im.base[3] + im.off * 4;
        for (long q = -im.off; q < im.total - im.off; ++q) store_pixel(im, q, ext_pixel(im, q));
        return true;
    }

    void release(Image &im)
    {
        for (int f = 0; f < 4; ++f) { free(im.base[f]); im.base[f] = nullptr; }
    }

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
        int below(int n) { return (int)(next() % (u64)n); }
    };

    // central differences of the image, zero on the 1-pixel border, as the keyframe producers form them
    void central_differences(Image &im)
    {
        const int H = im.H, W = im.W;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
            {
                Pix &p = im.px[(size_t)y * W + x];
                p.kx = p.ky = 0;
                if (x > 0 && x < W - 1 && y > 0 && y < H - 1)
                {
                    p.kx = im.px[(size_t)y * W + x + 1].I - im.px[(size_t)y * W + x - 1].I;
                    p.ky = im.px[(size_t)(y + 1) * W + x].I - im.px[(size_t)(y - 1) * W + x].I;
                }
            }
    }

    // content 0: 0/255 checkerboard of 2 x 2 cells (central differences of exactly +-255 and 0 beside 0 and 255 intensities);
    // 1: random bytes and their central differences; 2: "free": intensities and both difference planes drawn independently
    void fill(Image &im, int content, u64 seed)
    {
        Rng r{seed};
        im.px.resize((size_t)im.H * im.W);
        for (int y = 0; y < im.H; ++y)
            for (int x = 0; x < im.W; ++x)
            {
                Pix &p = im.px[(size_t)y * im.W + x];
                if (content == 0) p = Pix{(((x >> 1) + (y >> 1)) & 1) ? 255 : 0, 0, 0};
                else if (content == 1) p = Pix{r.below(256), 0, 0};
                else
                {
                    const int ends[6] = {0, 1, 127, 128, 254, 255};
                    p.I = r.below(4) == 0 ? ends[r.below(6)] : r.below(256);
                    p.kx = r.below(4) == 0 ? (r.below(2) ? 255 : -255) : r.below(511) - 255;
                    p.ky = r.below(4) == 0 ? (r.below(2) ? 255 : -255) : r.below(511) - 255;
                }
            }
        if (content != 2) central_differences(im);
        else if (im.H > 8 && im.W > 8)
        { // the case TINY_CROSS is about, made certain: at x = y = 2^-149 the packed blend gives 0.5 (2^-149 + 2^-149), the others 0 + 0
            im.px[0].kx = im.px[0].ky = 0;
            im.px[1].kx = im.px[1].ky = 1;
            im.px[(size_t)im.W].kx = im.px[(size_t)im.W].ky = 1;
        }
    }

    struct Coords
    {
        std::vector<double> x, y;
        std::vector<unsigned char> tiny; // a subnormal blend weight: see TINY_CROSS
        size_t n() const { return x.size(); }
    };

    std::vector<double> axis_values(int n, std::vector<unsigned char> &tiny)
    {
        const double inf = std::numeric_limits<double>::infinity(), dmin = std::ldexp(1.0, -1074);
        std::vector<double> v = {-inf, -1e300, -2147483649.0, -1.0, -dmin, -0.0, 0.0, dmin, 0.5, 1.0 - std::ldexp(1.0, -53), 1.0};
        for (int e : {n - 2, n - 1})
        {
            v.push_back(std::nextafter((double)e, -inf));
            v.push_back((double)e);
            v.push_back(std::nextafter((double)e, inf));
        }
        for (double d : {(double)n, 2147483647.0, 2147483648.0, 4294967296.5, 1e300, inf, std::numeric_limits<double>::quiet_NaN()}) v.push_back(d);
        tiny.assign(v.size(), 0);
        // beyond the list of the issue: distances from a pixel centre that are subnormal (or the smallest normal) in fp32
        for (int e : {-149, -140, -127, -126}) { v.push_back(std::ldexp(1.0, e)); tiny.push_back(e < -126); }
        return v;
    }

    double snap(Rng &r, int n)
    {
        const double frac[4] = {0.0, std::ldexp(1.0, -24), 0.5, 1.0 - std::ldexp(1.0, -24)};
        const int k = r.below(n);
        return k == n - 1 ? (double)k : (double)k + frac[r.below(4)];
    }

    Coords make_coords(const Image &im, u64 seed)
    {
        Coords c;
        std::vector<unsigned char> tx, ty;
        const std::vector<double> ax = axis_values(im.W, tx), ay = axis_values(im.H, ty);
        for (size_t j = 0; j < ay.size(); ++j)
            for (size_t i = 0; i < ax.size(); ++i) { c.x.push_back(ax[i]); c.y.push_back(ay[j]); c.tiny.push_back(tx[i] | ty[j]); }
        Rng r{seed};
        for (int i = 0; i < 65536; ++i)
        {
            double x = r.unit() * (im.W - 1), y = r.unit() * (im.H - 1);
            if ((i & 3) == 0)
            { // a quarter snapped to k + {0, 2^-24, 0.5, 1 - 2^-24} on one or both axes
                const int axes = 1 + r.below(3);
                if (axes & 1) x = snap(r, im.W);
                if (axes & 2) y = snap(r, im.H);
            }
            c.x.push_back(x); c.y.push_back(y); c.tiny.push_back(0);
        }
        return c;
    }

    struct Res
    {
        bool ok;
        double val, gx, gy;
    };
    u64 bits(double d) { u64 b; memcpy(&b, &d, 8); return b; }

    // ---- reference A ----------------------------------------------------------------------------------------------------
    int field9(unsigned w, int lo)
    {
        const int f = (int)((w >> lo) & 0x1ffu);
        return f >= 256 ? f - 512 : f;
    }
    float half_value(const unsigned char *p)
    {
        _Float16 h;
        memcpy(&h, p, 2);
        return (float)h;
    }

    // intensity and the two gradient operands of pixel q as variant v stores them (packed: the doubled differences)
    void load_pixel(const Image &im, int v, long q, float &i, float &a, float &b)
    {
        if (q < 0 || q >= (long)im.H * im.W) { fprintf(stderr, "reference A indexed pixel %ld outside the image\n", q); abort(); }
        a = b = 0.0f;
        if (v == 3)
        {
            unsigned w;
            memcpy(&w, im.Gp + q * 4, 4);
            i = (float)(w & 0xffu);
            a = (float)field9(w, 8);
            b = (float)field9(w, 23);
            return;
        }
        i = (float)im.I[q];
        if (v == 1) { memcpy(&a, im.Gf + q * 8, 4); memcpy(&b, im.Gf + q * 8 + 4, 4); }
        if (v == 2) { a = half_value(im.Gh + q * 4); b = half_value(im.Gh + q * 4 + 2); }
    }

    Res ref_a(const Image &im, int v, double x, double y)
    {
#pragma clang fp contract(off)
        Res r = {false, 0.0, 0.0, 0.0};
        const int H = im.H, W = im.W;
        if (!(x >= 0 && x <= W - 1 && y >= 0 && y <= H - 1)) return r;
        r.ok = true;
        int xi = (int)x, yi = (int)y;
        if (xi > W - 2) xi = W - 2;
        if (yi > H - 2) yi = H - 2;
        const float dx = (float)(x - xi), dy = (float)(y - yi);
        const float dxdy = dx * dy;
        const float w00 = 1.0f - dx - dy + dxdy, w01 = dx - dxdy, w10 = dy - dxdy, w11 = dxdy;
        const long q = (long)yi * W + xi;
        float i00, i01, i10, i11, a00, a01, a10, a11, b00, b01, b10, b11;
        load_pixel(im, v, q, i00, a00, b00);
        load_pixel(im, v, q + 1, i01, a01, b01);
        load_pixel(im, v, q + W, i10, a10, b10);
        load_pixel(im, v, q + W + 1, i11, a11, b11);
        float s = w11 * i11;
        s = s + w10 * i10;
        s = s + w01 * i01;
        s = s + w00 * i00;
        r.val = (double)s;
        if (v == 0) return r;
        float a = w11 * a11;
        a = a + w10 * a10;
        a = a + w01 * a01;
        a = a + w00 * a00;
        float b = w11 * b11;
        b = b + w10 * b10;
        b = b + w01 * b01;
        b = b + w00 * b00;
        if (v == 3) { a = 0.5f * a; b = 0.5f * b; }
        r.gx = (double)a;
        r.gy = (double)b;
        return r;
    }

    // ---- reference B: the real-number interpolant of the logical pixels ---------------------------------------------------
    void ref_b(const Image &im, double x, double y, long double out[3])
    {
        int xi = (int)x, yi = (int)y;
        if (xi > im.W - 2) xi = im.W - 2;
        if (yi > im.H - 2) yi = im.H - 2;
        const long double fx = (long double)x - xi, fy = (long double)y - yi;
        const Pix &p00 = im.px[(size_t)yi * im.W + xi], &p01 = (&p00)[1], &p10 = (&p00)[im.W], &p11 = (&p00)[im.W + 1];
        const long double w00 = (1 - fx) * (1 - fy), w01 = fx * (1 - fy), w10 = (1 - fx) * fy, w11 = fx * fy;
        out[0] = w00 * p00.I + w01 * p01.I + w10 * p10.I + w11 * p11.I;
        out[1] = 0.5L * (w00 * p00.kx + w01 * p01.kx + w10 * p10.kx + w11 * p11.kx);
        out[2] = 0.5L * (w00 * p00.ky + w01 * p01.ky + w10 * p10.ky + w11 * p11.ky);
    }

    // ---- the header's host half --------------------------------------------------------------------------------------------
    template <bool WG, int G>
    Res twin(const Image &im, double x, double y)
    {
        const float *grad = (const float *)(G == 0 ? im.Gf : G == 1 ? im.Gh : im.Gp);
        mbavo::TapLoads t;
        mbavo::tap_fetch<WG, G>(im.I, grad, im.H, im.W, x, y, t);
        Res r = {t.ok, 0.0, 0.0, 0.0};
        if (t.ok) mbavo::tap_blend<WG, G>(t, r.val, r.gx, r.gy);
        return r;
    }
    Res twin_v(const Image &im, int v, double x, double y)
    {
        switch (v)
        {
        case 0: return twin<false, 0>(im, x, y);
        case 1: return twin<true, 0>(im, x, y);
        case 2: return twin<true, 1>(im, x, y);
        default: return twin<true, 2>(im, x, y);
        }
    }
    template <bool WG>
    Res twin_bilinear(const Image &im, double x, double y)
    {
        Res r = {false, 0.0, 0.0, 0.0};
        r.ok = mbavo::bilinear_tap<WG>(im.I, (const float *)im.Gf, im.H, im.W, x, y, r.val, r.gx, r.gy);
        return r;
    }

    // ---- device results: variant-major, n lanes per variant -----------------------------------------------------------------
    struct DevOut
    {
        size_t n = 0;
        std::vector<unsigned char> ok; // [4 n]
        std::vector<u64> b;            // [3][4 n]: val, gx, gy
        bool have = false;
        unsigned char okv(int v, size_t p) const { return ok[v * n + p]; }
        u64 get(int k, int v, size_t p) const { return b[((size_t)k * NV + v) * n + p]; }
    };

    struct Report
    {
        u64 lanes = 0, ok_count[NV] = {0, 0, 0, 0};
        u64 mism_a[NV] = {0, 0, 0, 0}, mism_twin[NV] = {0, 0, 0, 0}, mism_cross[NV] = {0, 0, 0, 0}, mism_b[NV] = {0, 0, 0, 0};
        u64 mism_twin_a[NV] = {0, 0, 0, 0};
        u64 tiny_differs = 0; // tiny coordinates at which the formats' gradient bits differ (inside TINY_CROSS)
        long double worst_val = 0, worst_grad = 0;
        std::vector<std::string> first;
        u64 total() const
        {
            u64 t = 0;
            for (int v = 0; v < NV; ++v) t += mism_a[v] + mism_twin[v] + mism_cross[v] + mism_b[v] + mism_twin_a[v];
            return t;
        }
        void note(const Image &im, const char *what, int v, double x, double y, const char *field, u64 got, u64 want)
        {
            if (first.size() >= 6) return;
            char buf[400];
            snprintf(buf, sizeof buf, "  MISMATCH %s: image %s, variant %s, x = %a, y = %a, %s: got %016llx want %016llx", what,
                     im.name.c_str(), VNAME[v], x, y, field, got, want);
            first.push_back(buf);
        }
    };

    // `got` against `want` in ok and, where ok, in the fields variant v has; returns the number of differing fields (0 or more)
    int compare(Report &rep, const Image &im, const char *what, int v, double x, double y, const Res &got, const Res &want)
    {
        if (got.ok != want.ok) { rep.note(im, what, v, x, y, "ok", got.ok, want.ok); return 1; }
        if (!want.ok) return 0;
        int bad = 0;
        if (bits(got.val) != bits(want.val)) { rep.note(im, what, v, x, y, "val", bits(got.val), bits(want.val)); ++bad; }
        if (v > 0 && bits(got.gx) != bits(want.gx)) { rep.note(im, what, v, x, y, "gx", bits(got.gx), bits(want.gx)); ++bad; }
        if (v > 0 && bits(got.gy) != bits(want.gy)) { rep.note(im, what, v, x, y, "gy", bits(got.gy), bits(want.gy)); ++bad; }
        return bad;
    }

    double as_double(u64 b) { double d; memcpy(&d, &b, 8); return d; }
    Res dev_res(const DevOut &d, int v, size_t p)
    {
        return Res{d.okv(v, p) == 1, as_double(d.get(0, v, p)), as_double(d.get(1, v, p)), as_double(d.get(2, v, p))};
    }

    void verify_image(const Image &im, const Coords &c, const DevOut &dev, Report &rep)
    {
        for (size_t p = 0; p < c.n(); ++p)
        {
            const double x = c.x[p], y = c.y[p];
            Res subject[NV]; // what the cross-format rule and B look at: the device's results, the host half's in host mode
            for (int v = 0; v < NV; ++v)
            {
                ++rep.lanes;
                const Res a = ref_a(im, v, x, y);
                const Res h = twin_v(im, v, x, y);
                if (dev.have)
                {
                    const Res d = dev_res(dev, v, p);
                    if (dev.okv(v, p) > 1) { rep.note(im, "device lane wrote nothing", v, x, y, "ok", dev.okv(v, p), a.ok); ++rep.mism_a[v]; }
                    else if (compare(rep, im, "device against A", v, x, y, d, a)) ++rep.mism_a[v];
                    if (compare(rep, im, "host half against device", v, x, y, h, d)) ++rep.mism_twin[v];
                    subject[v] = d;
                }
                else
                {
                    if (compare(rep, im, "host half against A", v, x, y, h, a)) ++rep.mism_twin_a[v];
                    subject[v] = h;
                }
                if (v < 2)
                { // bilinear_tap is the float instantiation: <false> is variant 0, <true> variant 1
                    const Res bt = v == 0 ? twin_bilinear<false>(im, x, y) : twin_bilinear<true>(im, x, y);
                    if (compare(rep, im, "host bilinear_tap against host tap_fetch + tap_blend", v, x, y, bt, h)) ++rep.mism_twin_a[v];
                }
                rep.ok_count[v] += subject[v].ok;
            }
            if (!subject[1].ok) continue;
            long double b[3];
            ref_b(im, x, y, b);
            for (int v = 0; v < NV; ++v)
            {
                if (!subject[v].ok) continue; // (a difference in ok is already counted above)
                const long double ev = fabsl((long double)subject[v].val - b[0]);
                if (ev > rep.worst_val) rep.worst_val = ev;
                bool bad = !(ev <= BOUND_VAL);
                if (bad) rep.note(im, "outside the bound of B", v, x, y, "val", bits(subject[v].val), bits((double)b[0]));
                if (v > 0)
                {
                    const long double ex = fabsl((long double)subject[v].gx - b[1]), ey = fabsl((long double)subject[v].gy - b[2]);
                    if (ex > rep.worst_grad) rep.worst_grad = ex;
                    if (ey > rep.worst_grad) rep.worst_grad = ey;
                    if (!(ex <= BOUND_GRAD)) { bad = true; rep.note(im, "outside the bound of B", v, x, y, "gx", bits(subject[v].gx), bits((double)b[1])); }
                    if (!(ey <= BOUND_GRAD)) { bad = true; rep.note(im, "outside the bound of B", v, x, y, "gy", bits(subject[v].gy), bits((double)b[2])); }
                }
                if (bad) ++rep.mism_b[v];
                // cross-format: val as variant 1 has it, gx and gy as variant 1 has them
                if (v == 1) continue;
                bool cross = false;
                if (bits(subject[v].val) != bits(subject[1].val))
                { cross = true; rep.note(im, "formats differ (want: float pairs)", v, x, y, "val", bits(subject[v].val), bits(subject[1].val)); }
                if (v > 1)
                {
                    const bool sx = bits(subject[v].gx) == bits(subject[1].gx), sy = bits(subject[v].gy) == bits(subject[1].gy);
                    if (c.tiny[p])
                    {
                        if (!sx || !sy) ++rep.tiny_differs;
                        if (!(fabs(subject[v].gx - subject[1].gx) <= TINY_CROSS))
                        { cross = true; rep.note(im, "formats differ by more than 2^-148 (want: float pairs)", v, x, y, "gx", bits(subject[v].gx), bits(subject[1].gx)); }
                        if (!(fabs(subject[v].gy - subject[1].gy) <= TINY_CROSS))
                        { cross = true; rep.note(im, "formats differ by more than 2^-148 (want: float pairs)", v, x, y, "gy", bits(subject[v].gy), bits(subject[1].gy)); }
                    }
                    else
                    {
                        if (!sx) { cross = true; rep.note(im, "formats differ (want: float pairs)", v, x, y, "gx", bits(subject[v].gx), bits(subject[1].gx)); }
                        if (!sy) { cross = true; rep.note(im, "formats differ (want: float pairs)", v, x, y, "gy", bits(subject[v].gy), bits(subject[1].gy)); }
                    }
                }
                if (cross) ++rep.mism_cross[v];
            }
        }
    }

    // ---- the field sweep -----------------------------------------------------------------------------------------------------
    // pixel (x, y), x < 511, y < 6 * 511, holds kx = x - 255, ky = y % 511 - 255 and the (y / 511)-th of six intensities; two
    // more columns (W odd: every second row starts off a word) and one more row hold other values.  An integer coordinate has
    // the weights (1, 0, 0, 0), so the tap returns the pixel's own fields.
    const int SWEEP_I[6] = {0, 1, 127, 128, 254, 255};
    constexpr int SWEEP_W = 513, SWEEP_H = 6 * 511 + 1;
    void fill_sweep(Image &im)
    {
        Rng r{99};
        im.H = SWEEP_H; im.W = SWEEP_W; im.name = "3067x513 sweep";
        im.px.resize((size_t)im.H * im.W);
        for (int y = 0; y < im.H; ++y)
            for (int x = 0; x < im.W; ++x)
                im.px[(size_t)y * im.W + x] = (x < 511 && y < 6 * 511) ? Pix{SWEEP_I[y / 511], x - 255, y % 511 - 255}
                                                                       : Pix{r.below(256), r.below(511) - 255, r.below(511) - 255};
    }
    Coords sweep_coords()
    {
        Coords c;
        c.x.reserve((size_t)6 * 511 * 511); c.y.reserve((size_t)6 * 511 * 511);
        for (int y = 0; y < 6 * 511; ++y)
            for (int x = 0; x < 511; ++x) { c.x.push_back((double)x); c.y.push_back((double)y); }
        c.tiny.assign(c.x.size(), 0);
        return c;
    }
    void verify_sweep_range(const Image &im, const Coords &c, const DevOut &dev, size_t lo, size_t hi, Report &rep)
    {
        for (size_t p = lo; p < hi; ++p)
        {
            const double x = c.x[p], y = c.y[p];
            const Pix &px = im.px[(size_t)y * im.W + (size_t)x];
            const Res want = {true, (double)px.I, 0.5 * px.kx, 0.5 * px.ky};
            for (int v = 0; v < NV; ++v)
            {
                ++rep.lanes;
                ++rep.ok_count[v];
                if (compare(rep, im, "host half against the pixel's fields", v, x, y, twin_v(im, v, x, y), want)) ++rep.mism_twin_a[v];
                if (!dev.have) continue;
                if (dev.okv(v, p) > 1) { rep.note(im, "device lane wrote nothing", v, x, y, "ok", dev.okv(v, p), 1); ++rep.mism_a[v]; }
                else if (compare(rep, im, "device against the pixel's fields", v, x, y, dev_res(dev, v, p), want)) ++rep.mism_a[v];
            }
        }
    }
    void merge(Report &into, const Report &r)
    {
        into.lanes += r.lanes;
        for (int v = 0; v < NV; ++v)
        {
            into.ok_count[v] += r.ok_count[v]; into.mism_a[v] += r.mism_a[v]; into.mism_twin[v] += r.mism_twin[v];
            into.mism_cross[v] += r.mism_cross[v]; into.mism_b[v] += r.mism_b[v]; into.mism_twin_a[v] += r.mism_twin_a[v];
        }
        for (const std::string &s : r.first) if (into.first.size() < 6) into.first.push_back(s);
    }

    void print_report(const Image &im, const Report &r, bool device, bool sweep)
    {
        printf("image %-22s lanes %8llu  ok", im.name.c_str(), r.lanes);
        for (int v = 0; v < NV; ++v) printf(" %s %llu", VNAME[v], r.ok_count[v]);
        printf("  mismatches per variant:");
        const char *sep = "";
        if (device)
        {
            printf(sweep ? " device/fields" : " device/A");
            for (int v = 0; v < NV; ++v) printf(" %llu", r.mism_a[v]);
            if (!sweep) { printf(", host/device"); for (int v = 0; v < NV; ++v) printf(" %llu", r.mism_twin[v]); }
            sep = ",";
        }
        printf("%s%s", sep, sweep ? " host/fields" : device ? " host bilinear_tap" : " host/A and bilinear_tap");
        for (int v = 0; v < NV; ++v) printf(" %llu", r.mism_twin_a[v]);
        if (!sweep)
        {
            printf(", formats"); for (int v = 0; v < NV; ++v) printf(" %llu", r.mism_cross[v]);
            printf(", B"); for (int v = 0; v < NV; ++v) printf(" %llu", r.mism_b[v]);
            printf("  worst |val - B| %.3Le (bound %.3Le)  worst |g - B| %.3Le (bound %.3Le)  tiny-weight taps whose formats differ inside 2^-148: %llu",
                   r.worst_val, BOUND_VAL, r.worst_grad, BOUND_GRAD, r.tiny_differs);
        }
        printf("  pack_keyframe_word mismatches %llu\n", im.word_mismatch);
        for (const std::string &s : r.first) printf("%s\n", s.c_str());
    }

#if defined(__HIPCC__)
    // ---- the device side -----------------------------------------------------------------------------------------------------
    struct Job
    {
        const unsigned char *I;
        const float *Gf, *Gh, *Gp;
        int H, W;
        const double *x, *y;
        unsigned n;
        unsigned char *ok;
        u64 *out;
    };

    template <bool WG, int G>
    __device__ void tap_lane(const Job &j, const float *grad, int v, unsigned p)
    {
        mbavo::TapLoads t;
        mbavo::tap_fetch<WG, G>(j.I, grad, j.H, j.W, j.x[p], j.y[p], t); // always, as the engine does: a dropped sample's loads stay inside
        const size_t lane = (size_t)v * j.n + p, stride = (size_t)NV * j.n;
        j.ok[lane] = t.ok ? 1 : 0;
        if (!t.ok) return;
        double val, gx = 0, gy = 0;
        mbavo::tap_blend<WG, G>(t, val, gx, gy);
        j.out[lane] = (u64)__double_as_longlong(val);
        j.out[stride + lane] = (u64)__double_as_longlong(gx);
        j.out[2 * stride + lane] = (u64)__double_as_longlong(gy);
    }

    __global__ void k_tap(Job j)
    {
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= (size_t)NV * j.n) return;
        const int v = (int)(i / j.n);
        const unsigned p = (unsigned)(i % j.n);
        switch (v)
        {
        case 0: tap_lane<false, 0>(j, j.Gf, v, p); break;
        case 1: tap_lane<true, 0>(j, j.Gf, v, p); break;
        case 2: tap_lane<true, 1>(j, j.Gh, v, p); break;
        default: tap_lane<true, 2>(j, j.Gp, v, p); break;
        }
    }

#define HIP_OK(call)                                                                                      \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); return false; }         \
    } while (0)

    bool run_device(Image &im, const Coords &c, DevOut &out)
    {
        const size_t n = c.n(), lanes = NV * n;
        for (int f = 0; f < 4; ++f)
        {
            HIP_OK(hipMalloc((void **)&im.dbase[f], im.bytes[f]));
            HIP_OK(hipMemcpy(im.dbase[f], im.base[f], im.bytes[f], hipMemcpyHostToDevice));
        }
        double *dx = nullptr, *dy = nullptr;
        unsigned char *dok = nullptr;
        u64 *dout = nullptr;
        HIP_OK(hipMalloc((void **)&dx, n * 8));
        HIP_OK(hipMalloc((void **)&dy, n * 8));
        HIP_OK(hipMalloc((void **)&dok, lanes));
        HIP_OK(hipMalloc((void **)&dout, 3 * lanes * 8));
        HIP_OK(hipMemcpy(dx, c.x.data(), n * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dy, c.y.data(), n * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dok, 0xcd, lanes)); // a lane that writes nothing is seen
        HIP_OK(hipMemset(dout, 0xcd, 3 * lanes * 8));
        Job j;
        j.I = im.dbase[0] + im.off;
        j.Gf = (const float *)(im.dbase[1] + im.off * 8);
        j.Gh = (const float *)(im.dbase[2] + im.off * 4);
        j.Gp = (const float *)(im.dbase[3] + im.off * 4);
        j.H = im.H; j.W = im.W; j.x = dx; j.y = dy; j.n = (unsigned)n; j.ok = dok; j.out = dout;
        hipLaunchKernelGGL(k_tap, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, 0, j);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        out.n = n; out.ok.resize(lanes); out.b.resize(3 * lanes); out.have = true;
        HIP_OK(hipMemcpy(out.ok.data(), dok, lanes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(out.b.data(), dout, 3 * lanes * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(dx)); HIP_OK(hipFree(dy)); HIP_OK(hipFree(dok)); HIP_OK(hipFree(dout));
        for (int f = 0; f < 4; ++f) { HIP_OK(hipFree(im.dbase[f])); im.dbase[f] = nullptr; }
        return true;
    }
#else
    struct Job {};
    bool run_device(Image &, const Coords &, DevOut &) { return false; }
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
    const int shapes[6][2] = {{2, 2}, {2, 3}, {3, 2}, {5, 7}, {3, 64}, {33, 65}}; // H x W
    const char *const content_name[3] = {"checker", "random", "free"};
    const int NI = 18;
    std::vector<Image> images(NI + 1);
    std::vector<Coords> coords(NI + 1);
    std::vector<DevOut> dev(NI + 1);
    std::vector<Report> reports(NI + 1);
    for (int s = 0; s < 6; ++s)
        for (int k = 0; k < 3; ++k)
        {
            Image &im = images[s * 3 + k];
            im.H = shapes[s][0]; im.W = shapes[s][1];
            im.name = std::to_string(im.H) + "x" + std::to_string(im.W) + " " + content_name[k];
            fill(im, k, 1000 + s * 3 + k);
            coords[s * 3 + k] = make_coords(im, 5000 + s * 3 + k);
        }
    fill_sweep(images[NI]);
    coords[NI] = sweep_coords();
    for (Image &im : images)
        if (!allocate(im, host_mode)) { printf("out of memory\n"); return 2; }
    printf("tap_check (%s): %d images and the sweep image, %zu coordinate pairs per image (%zu of them the cross product of the edge values), "
           "4 variants; margins %s\n", host_mode ? "--host: no device" : "device and host", NI, coords[0].n(), coords[0].n() - 65536,
           host_mode ? "none, exact-size allocations" : "W + 2 pixels or more, images off their natural alignment");

    double t_device = 0;
    if (!host_mode)
    {
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i <= NI; ++i)
            if (!run_device(images[i], coords[i], dev[i])) { printf("TAP CHECK FAILED (device run)\n"); return 3; }
        t_device = seconds_since(t0);
    }

    // verification on the host: the images on up to 8 threads, the sweep in 8 ranges
    const auto t_verify = std::chrono::steady_clock::now();
    {
        std::vector<std::thread> pool;
        for (int w = 0; w < 6; ++w)
            pool.emplace_back([&, w] { for (int i = w; i < NI; i += 6) verify_image(images[i], coords[i], dev[i], reports[i]); });
        for (std::thread &t : pool) t.join();
    }
    {
        const int parts = 8;
        std::vector<Report> part(parts);
        std::vector<std::thread> pool;
        const size_t n = coords[NI].n();
        for (int w = 0; w < parts; ++w)
            pool.emplace_back([&, w] { verify_sweep_range(images[NI], coords[NI], dev[NI], n * w / parts, n * (w + 1) / parts, part[w]); });
        for (std::thread &t : pool) t.join();
        for (const Report &r : part) merge(reports[NI], r);
    }
    const double t_host = seconds_since(t_verify);

    u64 failures = 0, lanes = 0;
    long double worst_val = 0, worst_grad = 0;
    for (int i = 0; i <= NI; ++i)
    {
        print_report(images[i], reports[i], !host_mode, i == NI);
        failures += reports[i].total() + images[i].word_mismatch;
        lanes += reports[i].lanes;
        if (reports[i].worst_val > worst_val) worst_val = reports[i].worst_val;
        if (reports[i].worst_grad > worst_grad) worst_grad = reports[i].worst_grad;
    }
    for (Image &im : images) release(im);
    printf("total: %llu lanes, %llu failures; worst |val - B| %.3Le of %.3Le, worst |g - B| %.3Le of %.3Le; device phase %.2f s, "
           "host verification %.2f s, whole run %.2f s\n", lanes, failures, worst_val, BOUND_VAL, worst_grad, BOUND_GRAD, t_device, t_host,
           seconds_since(t_start));
    if (failures) { printf("TAP CHECK FAILED\n"); return 1; }
    printf("TAP CHECK PASSED\n");
    return 0;
}
