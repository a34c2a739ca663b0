// pairs_photocal.hip -- the sensor's photometric calibration where a batch of keyframe pairs takes its images in (include/mbavo.h:
// mbavo_pairs_set_photometric, _clear_photometric, _photocal_stats) and its stand-alone siblings (mbavo_photometric_table,
// mbavo_photometric_u8_batch): the inverse response curve as a table of 256 floats and the inverse vignette as a float map in the
// geometry the images arrive in, applied inside the ONE launch that fills level 0 -- the calibrated remap in place of the plain
// one, or with undistort = 0 one launch over all images that changed in place of the strided copies and the scatter.  The value
// is rounded to a byte once, after the bilinear blend.
//
// The per-pixel bodies are photocal_math.h's; what is written here is the indexing, which follows pairs_prep.hip's remap kernels
// (grid row y < n_key: the keyframe of pair_of_row, else pair y - n_key's current frame), and two policies:
//
//   CAL   whose calibration (and, for raw images, whose map) a pair's images go through: the object's one, or with
//         mbavo_pairs_opts.num_cameras > 0 that of the pair's camera -- the same for a whole grid row, a scalar load
//   VIG   photocal_math.h: NoVignette (the call brought no vignette: no map is read) or Vignette
//
// and one switch, LDS: a grid row reads ONE table, so a workgroup stages its 1 KB in LDS (lane v loads entry v) and the taps look
// theirs up there; LDS = false reads the table through the vector cache instead (tools/pairs_photocal_bench.py times both).
// All streaming work, HBM-bound; vector stores only, nothing atomic.
#include "pairs_prep.h"
#include "pairs_desc.h"
#include "photocal_math.h"
#include "vo_frontend.h"
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <type_traits>

namespace mbavo
{
    namespace pairs
    {
        // the calibrations on the device: table g at luts + 256 g, inverse vignette g at inv + inv_floats g (VIG = false: not read)
        struct PhotoCalSet
        {
            const float *luts, *inv;
            long long inv_floats;
        };
        template <bool VIG>
        __device__ __forceinline__ auto vignette_of(const PhotoCalSet &set, int g)
        {
            if constexpr (VIG) return Vignette{set.inv + (size_t)g * (size_t)set.inv_floats};
            else return NoVignette{};
        }
        // the table of a workgroup's calibration: staged in LDS by all 256 lanes (call it before any lane leaves), or as it lies
        template <bool LDS>
        __device__ __forceinline__ const float *table_of(const float *lut)
        {
            if constexpr (LDS)
            {
                __shared__ float s_lut[256];
                s_lut[threadIdx.x] = lut[threadIdx.x];
                __syncthreads();
                return s_lut;
            }
            else return lut;
        }

        struct OneCalibration
        {
            const float *map; // undistort != 0: the object's one map
            __device__ __forceinline__ int of_pair(int) const { return 0; }
            __device__ __forceinline__ const float *map_of(int) const { return map; }
        };
        struct CameraCalibrations
        {
            const PairCamera *cams;
            const float *maps; // undistort != 0: G maps of map_floats each
            long long map_floats;
            __device__ __forceinline__ int of_pair(int pair) const { return cams[pair].cam; }
            __device__ __forceinline__ const float *map_of(int pair) const { return maps + (size_t)cams[pair].cam * (size_t)map_floats; }
        };

        // ---- (undistort = 0) level 0 of the images that changed, calibrated on their way into the object: 16 destination bytes
        // per lane as k_pairs_scatter_level0 (the destination is 256-byte aligned; a source image starts wherever y * npx falls)
        template <class CAL, bool VIG, bool LDS>
        __global__ __launch_bounds__(256) void k_pairs_photocal_level0(const PairLevelDesc *__restrict__ desc, int L, const int *__restrict__ key_pairs,
                                                                       int n_key, const unsigned char *__restrict__ src_key,
                                                                       const unsigned char *__restrict__ src_cur, int npx, const CAL cal,
                                                                       const PhotoCalSet set)
        {
            const int y = blockIdx.y;
            const bool key = y < n_key;
            const int pair = key ? pair_of_row(key_pairs, y) : y - n_key;
            const int g = cal.of_pair(pair);
            const float *lut = table_of<LDS>(set.luts + (size_t)g * 256);
            const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 16;
            if (i0 >= npx) return;
            const unsigned char *src = (key ? src_key : src_cur) + (size_t)(key ? y : y - n_key) * npx;
            const PairLevelDesc &d = desc[(size_t)pair * L];
            photocal_sixteen(src, lut, vignette_of<VIG>(set, g), key ? d.ref : d.cur, npx, i0);
        }

        // ---- (undistort != 0) k_pairs_remap_level0 and k_pairs_remap_level0_both of pairs_prep.hip under the calibrated tap
        template <class CAL, bool VIG, bool LDS>
        __global__ __launch_bounds__(256) void k_pairs_photocal_remap(const PairLevelDesc *__restrict__ desc, int L, const int *__restrict__ key_pairs,
                                                                      int n_key, const unsigned char *__restrict__ raw_key,
                                                                      const unsigned char *__restrict__ raw_cur, int Hs, int Ws, int npx, const CAL cal,
                                                                      const PhotoCalSet set)
        {
            const int y = blockIdx.y;
            const bool key = y < n_key;
            const int pair = key ? pair_of_row(key_pairs, y) : y - n_key;
            const int g = cal.of_pair(pair);
            const float *lut = table_of<LDS>(set.luts + (size_t)g * 256);
            const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
            if (i0 >= npx) return;
            const unsigned char *__restrict__ src = (key ? raw_key : raw_cur) + (size_t)(key ? y : y - n_key) * Hs * Ws;
            const PairLevelDesc &d = desc[(size_t)pair * L];
            remap_four_cal<1>({src}, Hs, Ws, cal.map_of(pair), lut, vignette_of<VIG>(set, g), {key ? d.ref : d.cur}, npx, i0);
        }
        template <bool VIG, bool LDS>
        __global__ __launch_bounds__(256) void k_pairs_photocal_remap_both(const PairLevelDesc *__restrict__ desc, int L,
                                                                           const unsigned char *__restrict__ raw_key,
                                                                           const unsigned char *__restrict__ raw_cur, int Hs, int Ws, int npx,
                                                                           const CameraCalibrations cal, const PhotoCalSet set)
        {
            const int pair = blockIdx.y;
            const int g = cal.of_pair(pair);
            const float *lut = table_of<LDS>(set.luts + (size_t)g * 256);
            const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
            if (i0 >= npx) return;
            const PairLevelDesc &d = desc[(size_t)pair * L];
            const size_t off = (size_t)pair * Hs * Ws;
            remap_four_cal<2>({raw_key + off, raw_cur + off}, Hs, Ws, cal.map_of(pair), lut, vignette_of<VIG>(set, g), {d.ref, d.cur}, npx, i0);
        }

        // ---- the inverse vignettes of all calibrations in one launch: a flat array of n floats, four per lane (the destination is
        // 256-byte aligned; a caller's vignette off a 16-byte boundary goes float by float)
        __global__ __launch_bounds__(256) void k_photocal_inverse_vignette(const float *__restrict__ V, float *__restrict__ inv, long long n, float v_min)
        {
            const long long i0 = ((long long)blockIdx.x * 256 + (long long)threadIdx.x) * 4;
            if (i0 >= n) return;
            if (i0 + 4 <= n && ((size_t)(V + i0) & 15) == 0)
            {
                const float4 v = *reinterpret_cast<const float4 *>(V + i0);
                *reinterpret_cast<float4 *>(inv + i0) = make_float4(inverse_vignette(v.x, v_min), inverse_vignette(v.y, v_min),
                                                                    inverse_vignette(v.z, v_min), inverse_vignette(v.w, v_min));
            }
            else
                for (int j = 0; j < 4 && i0 + j < n; ++j) inv[i0 + j] = inverse_vignette(V[i0 + j], v_min);
        }

        // ---- the stand-alone call: image y of a caller's packed array under calibration cal_of_image[y], the pinhole intake's
        // device function.  No __restrict__ on the images: d_dst == d_src is allowed (a lane reads its 16 bytes, then stores them).
        template <bool VIG, bool LDS>
        __global__ __launch_bounds__(256) void k_photometric_u8_batch(const unsigned char *src, int npx, const PhotoCalSet set,
                                                                      const int *__restrict__ cal_of_image, unsigned char *dst)
        {
            const size_t y = blockIdx.y;
            const int g = cal_of_image[y];
            const float *lut = table_of<LDS>(set.luts + (size_t)g * 256);
            const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 16;
            if (i0 >= npx) return;
            photocal_sixteen(src + y * npx, lut, vignette_of<VIG>(set, g), dst + y * npx, npx, i0);
        }

        // f(VIG, LDS) as compile-time booleans
        template <class F>
        static void with_variant(bool vig, bool lds, F &&f)
        {
            if (vig) { if (lds) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
            else { if (lds) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
        }
    } // namespace pairs

    using namespace pairs;

    // Pure host, IEEE double, operation by operation (no product feeds a sum here: nothing can be contracted).  The output is
    // written only once every entry has passed.
    int photometric_table(const double *h_G, double scale, float *h_lut)
    {
        if (!h_lut || !(scale > 0.0 && scale <= 1.0)) return MBAVO_E_ARG; // (a NaN fails)
        float lut[256];
        if (!h_G)
            for (int i = 0; i < 256; ++i) lut[i] = (float)(scale * (255.0 * ((double)i - 0.0) / (255.0 - 0.0))); // G[i] = i
        else
        {
            for (int i = 0; i < 256; ++i)
                if (!std::isfinite(h_G[i]) || (i > 0 && h_G[i] < h_G[i - 1])) return MBAVO_E_ARG;
            if (!(h_G[255] > h_G[0])) return MBAVO_E_ARG;
            for (int i = 0; i < 256; ++i) lut[i] = (float)(scale * (255.0 * (h_G[i] - h_G[0]) / (h_G[255] - h_G[0])));
        }
        memcpy(h_lut, lut, sizeof(lut));
        return 0;
    }

    int photometric_u8_batch(Engine &eng, int n_img, const unsigned char *d_src, int H, int W, int n_cal, const float *h_luts, const float *d_inv,
                             const int *h_cal_of_image, unsigned char *d_dst)
    {
        if (!d_src || !d_dst || !h_luts || n_img < 1 || n_img > kUndistortMaxBatch || n_cal < 1 || H < 1 || W < 1 ||
            (long long)H * W > kUndistortMaxPixels)
            return MBAVO_E_ARG;
        if (!h_cal_of_image && n_cal != 1 && n_cal != n_img) return MBAVO_E_ARG; // (no list: one calibration for all, or image i's own)
        // [tables n_cal x 256 floats | calibration of every image] in one copy
        const size_t lut_bytes = sizeof(float) * 256 * (size_t)n_cal, bytes = lut_bytes + sizeof(int) * (size_t)n_img;
        std::vector<char> up(bytes);
        memcpy(up.data(), h_luts, lut_bytes);
        int *cal = reinterpret_cast<int *>(up.data() + lut_bytes);
        for (int i = 0; i < n_img; ++i)
        {
            cal[i] = h_cal_of_image ? h_cal_of_image[i] : (n_cal == 1 ? 0 : i);
            if (cal[i] < 0 || cal[i] >= n_cal) return MBAVO_E_ARG;
        }
        char *dev = (char *)eng.named_scratch(kPhotocalSlot, bytes);
        if (!dev) return (int)hipErrorOutOfMemory;
        // (a pageable source: the copy is staged before the call returns)
        const hipError_t e = hipMemcpyAsync(dev, up.data(), bytes, hipMemcpyHostToDevice, eng.stream());
        if (e != hipSuccess) return (int)e;
        const int npx = H * W;
        const PhotoCalSet set{(const float *)dev, d_inv, (long long)npx};
        const bool lds = opt_flag(0, read_env_overrides().pairs_photocal_lds, true);
        with_variant(d_inv != nullptr, lds, [&](auto vig, auto in_lds) {
            hipLaunchKernelGGL((k_photometric_u8_batch<decltype(vig)::value, decltype(in_lds)::value>), dim3((npx + 4095) / 4096, n_img), dim3(256), 0,
                               eng.stream(), d_src, npx, set, (const int *)(dev + lut_bytes), d_dst);
        });
        return (int)hipGetLastError();
    }

    // Everything is checked (the tables into a scratch vector) before anything is copied, launched or changed -- the statistics of
    // the call before included; then one copy of the n tables from the pinned mirror and, with a vignette, one launch.  Nothing
    // is waited for, not even the copy of the call before out of the mirror: every reader of the tables is an intake, and every
    // intake ends in a stream synchronisation, so a copy that may still be under way when the mirror is refilled belongs to a call
    // no intake has followed, and the copy enqueued here overwrites whatever it left, in stream order.
    int PairBatch::set_photometric(int n, const double *h_G, const float *d_vignette, const mbavo_pairs_photocal_opts *o)
    {
        PhotoCal &pc = photocal_;
        if (!arena_ || n != cameras()) return MBAVO_E_ARG;
        const double scale = o && o->scale != 0.0 ? o->scale : 1.0;
        float v_min = o ? o->v_min : 0.0f;
        if (!std::isfinite(v_min) || v_min < 0.0f) return MBAVO_E_ARG;
        if (v_min == 0.0f) v_min = 0.0625f;
        if (camera_missing()) return MBAVO_E_ARG; // (the vignette's geometry is the raw camera's, a calibration belongs to a camera: none yet)
        std::vector<float> luts(256 * (size_t)n);
        for (int g = 0; g < n; ++g)
        {
            const int rc = photometric_table(h_G ? h_G + 256 * (size_t)g : nullptr, scale, &luts[256 * (size_t)g]);
            if (rc != 0) return rc;
        }
        // (the raw size cannot have changed since the maps were allocated: the camera calls reject that, PairBatch::raw_size_fixed)
        const int Hr = opts_.undistort != 0 ? raw_H_ : plan_.H[0], Wr = opts_.undistort != 0 ? raw_W_ : plan_.W[0];
        const size_t lut_bytes = sizeof(float) * luts.size(), map_px = (size_t)Hr * (size_t)Wr;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        if (!pc.luts && (e = pc.luts.alloc(lut_bytes)) != hipSuccess) return (int)e;
        if (!pc.mirror && (e = pc.mirror.alloc(lut_bytes)) != hipSuccess) return (int)e;
        if (d_vignette && !pc.inv)
        {
            if ((e = pc.inv.alloc(sizeof(float) * map_px * (size_t)n)) != hipSuccess) return (int)e;
            pc.Hr = Hr; pc.Wr = Wr;
        }
        pc.stats = CallStats{};
        memcpy(pc.mirror, luts.data(), lut_bytes);
        if ((e = hipMemcpyAsync(pc.luts, pc.mirror, lut_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if (d_vignette)
        {
            const long long total = (long long)map_px * n;
            hipLaunchKernelGGL(k_photocal_inverse_vignette, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, st, d_vignette, pc.inv.p, total, v_min);
            ++pc.stats.launches;
        }
        pc.vignette = d_vignette != nullptr;
        pc.lds = opt_flag(0, read_env_overrides().pairs_photocal_lds, true);
        pc.active = true;
        return (int)hipGetLastError();
    }

    int PairBatch::clear_photometric()
    {
        if (!arena_) return MBAVO_E_ARG;
        photocal_.active = false; // (the storage stays: a later set_photometric finds it)
        photocal_.stats = CallStats{};
        return 0;
    }

    int PairBatch::level0_calibrated(int n_key, const int *d_keys, const unsigned char *d_sharp, int n_cur, const unsigned char *d_blur, CallStats &s)
    {
        const PairsPlan &p = plan_;
        const PhotoCal &pc = photocal_;
        const int npx0 = p.H[0] * p.W[0], rows = n_key + n_cur, L = p.L;
        if (rows == 0) return 0;
        const bool raw = opts_.undistort != 0;
        hipStream_t st = eng_.stream();
        const PairLevelDesc *desc = lay_.desc(arena_);
        const PhotoCalSet set{pc.luts, pc.vignette ? pc.inv.p : nullptr, (long long)pc.Hr * pc.Wr};
        const float *maps = raw ? lay_.maps(arena_) : nullptr;
        const long long map_floats = 2ll * npx0;
        const int Hs = raw_H_, Ws = raw_W_;
        const dim3 grid(raw ? (npx0 + 1023) / 1024 : (npx0 + 4095) / 4096, rows);
        const bool both = raw && opts_.num_cameras > 0 && remap_both_ && !d_keys && n_key == p.B && n_cur == p.B; // (as PairBatch::level0)
        ++s.launches;
        with_variant(pc.vignette, pc.lds, [&](auto vig, auto in_lds) {
            constexpr bool V = decltype(vig)::value, S = decltype(in_lds)::value;
            auto launch = [&](const auto &cal) {
                using CAL = std::decay_t<decltype(cal)>;
                if (raw)
                    hipLaunchKernelGGL((k_pairs_photocal_remap<CAL, V, S>), grid, dim3(256), 0, st, desc, L, d_keys, n_key, d_sharp, d_blur, Hs, Ws, npx0,
                                       cal, set);
                else
                    hipLaunchKernelGGL((k_pairs_photocal_level0<CAL, V, S>), grid, dim3(256), 0, st, desc, L, d_keys, n_key, d_sharp, d_blur, npx0, cal,
                                       set);
            };
            if (opts_.num_cameras == 0) launch(OneCalibration{maps});
            else if (both)
                hipLaunchKernelGGL((k_pairs_photocal_remap_both<V, S>), dim3(grid.x, p.B), dim3(256), 0, st, desc, L, d_sharp, d_blur, Hs, Ws, npx0,
                                   CameraCalibrations{lay_.pair_cameras(arena_), maps, map_floats}, set);
            else launch(CameraCalibrations{lay_.pair_cameras(arena_), maps, map_floats});
        });
        return 0;
    }
} // namespace mbavo
