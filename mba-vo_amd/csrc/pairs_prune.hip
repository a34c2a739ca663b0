// pairs_prune.hip -- flagged keypoints removed from the object's own arrays on the device, their depths and the filter's state moved
// along (include/mbavo.h: mbavo_pairs_prune_keypoints): a stable, in-place stream compaction per (pair, level).
//
//   k_pairs_prune     the call's ONE launch: one workgroup of 256 per (listed pair, reported level).
//                count    the slice in tiles of 256, ascending: a lane reads its keypoint's flag byte, depth and filter state (what
//                         the enabled criteria need, nothing else) and gives the verdict; the four integer sums meet in LDS.  kept
//                         and min_keep decide, before anything moves, whether the (pair, level) is skipped.
//                move     the slice again: a lane loads its keypoint -- coordinates, depth, the four state entries -- into
//                         registers and waits for them, ranks itself among the tile's survivors by a ballot per wave and the four
//                         waves' totals in LDS (keyframe_math.h: block_rank_of_flag, whose barrier every lane passes with its tile
//                         loaded), and stores to place base + rank.  A destination never exceeds its source and lies below the
//                         next tile, which is loaded only from its own range: no staging, no atomics, the same bits for any B.
//                close    lane 0 writes the count, the count's copy behind the records and the record.
#include "keyframe_math.h"
#include "pairs_desc.h"
#include "pairs_prep.h"
#include <cstring>
#include <iterator>

namespace mbavo
{
    namespace pairs
    {
        enum PruneVerdict { kPruneKeep = 0, kPruneFlag = 1, kPruneDepth = 2, kPruneFilter = 3 };

        // what a lane reads of keypoint i for the verdict, and the verdict: the first criterion that holds (include/mbavo.h, step 1)
        struct PruneSlice
        {
            const unsigned char *flags; // the level's first flag byte, or null: no flag criterion
            const double *kp_z, *info;  // (info, n_obs, n_rej: the slot's first entries)
            const int *n_obs, *n_rej;
            __device__ __forceinline__ int verdict(const mbavo_pairs_prune_opts &o, int i) const
            {
                if (flags)
                {
                    const unsigned f = flags[i];
                    if (f < 32u && ((o.drop_mask >> f) & 1u)) return kPruneFlag;
                }
                if (o.check_depth == 1)
                {
                    const double D = kp_z[i];
                    if (!(__builtin_isfinite(D) && D >= o.z_min && (o.z_max == 0.0 || D <= o.z_max))) return kPruneDepth;
                }
                if (o.use_filter == 1)
                {
                    if (o.min_info > 0.0 && info[i] < o.min_info) return kPruneFilter;
                    if (o.min_obs > 0 && n_obs[i] < o.min_obs) return kPruneFilter;
                    if (o.rej_limit > 0 && n_rej[i] >= o.rej_limit) return kPruneFilter;
                }
                return kPruneKeep;
            }
        };

        __global__ __launch_bounds__(256) void k_pairs_prune(const PruneArgs a)
        {
            __shared__ int s_sum[4][4];  // [wave][verdict]
            __shared__ int s_rank[2][4]; // the waves' survivor counts of a tile, even and odd tiles apart
            const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
            const int ent = (int)blockIdx.x;
            const int at = ent / a.levels, li = ent - at * a.levels, l = a.level < 0 ? li : a.level;
            const int b = a.list[at];
            const size_t e = (size_t)b * a.L + l;
            const int K = a.counts[e];
            const PairLevelDesc &pd = a.desc[e];
            const mbavo_pairs_prune_opts o = *a.opts;
            const long long s0 = (long long)b * a.st_stride + a.st0[l], o0 = (long long)b * a.out_stride + a.out0[l];
            double2 *kp_xy = reinterpret_cast<double2 *>(pd.kp_xy);
            double *kp_z = pd.kp_z;
            const bool state = a.mu != nullptr; // (use_filter = 1 without it is rejected on the host)
            double *mu = state ? a.mu + s0 : nullptr, *info = state ? a.info + s0 : nullptr;
            int *n_obs = state ? a.n_obs + s0 : nullptr, *n_rej = state ? a.n_rej + s0 : nullptr;
            const PruneSlice sl{a.flags && o.drop_mask != 0u ? a.flags + o0 : nullptr, kp_z, info, n_obs, n_rej};

            // ---- count
            int n[4] = {0, 0, 0, 0};
            for (int t = 0; t < K; t += 256)
            {
                const int i = t + tid;
                if (i >= K) continue;
                const int v = sl.verdict(o, i);
#pragma unroll
                for (int j = 0; j < 4; ++j) n[j] += v == j;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) n[j] += __shfl_xor(n[j], off);
                if (lane == 0) s_sum[wave][j] = n[j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) n[j] = ((s_sum[0][j] + s_sum[1][j]) + s_sum[2][j]) + s_sum[3][j];
            const int kept = n[kPruneKeep];
            const bool skipped = kept < K && kept < o.min_keep;
            const bool move = o.apply == 1 && !skipped && kept < K;

            // ---- move (and the caller's keep bytes)
            if (move || a.keep)
            {
                unsigned char *keep_out = a.keep ? a.keep + o0 : nullptr;
                int base = 0;
                for (int t = 0, par = 0; t < K; t += 256, par ^= 1)
                {
                    const int i = t + tid;
                    const bool in = i < K;
                    const bool keep = in && (skipped || sl.verdict(o, i) == kPruneKeep);
                    double2 p = {0.0, 0.0};
                    double D = 0.0, m = 0.0, w = 0.0;
                    int no = 0, nr = 0;
                    if (move && keep)
                    {
                        p = kp_xy[i]; D = kp_z[i];
                        if (state)
                        {
                            m = mu[i]; w = info[i];
                            no = n_obs[i]; nr = n_rej[i];
                        }
                    }
                    // the tile is in registers before the barrier inside the rank, so before any lane's store
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    int total;
                    const int r = base + block_rank_of_flag(keep, s_rank[par], total);
                    base += total;
                    if (in && keep_out) keep_out[i] = keep ? 1 : 0;
                    if (move && keep && r != i)
                    { // (r < i, r < kept)
                        kp_xy[r] = p; kp_z[r] = D;
                        if (state)
                        {
                            mu[r] = m; info[r] = w;
                            n_obs[r] = no; n_rej[r] = nr;
                        }
                    }
                }
            }

            // ---- close
            if (tid != 0) return;
            const int after = move ? kept : K;
            if (move) a.counts[e] = kept;
            a.new_counts[e] = after;
            struct mbavo_pairs_prune *out = a.out + ent;
            out->status = 0; out->num_before = K; out->num_kept = skipped ? K : kept;
            out->by_flag = n[kPruneFlag]; out->by_depth = n[kPruneDepth]; out->by_filter = n[kPruneFilter];
            out->skipped = skipped ? 1 : 0; out->pad = 0;
        }
    } // namespace pairs

    using namespace pairs;

    int PairBatch::prune_keypoints(int n, const int *h_pairs, const mbavo_pairs_prune_opts *o, const unsigned char *d_flags, struct mbavo_pairs_prune *h_out,
                                   unsigned char *d_keep)
    {
        DepthCall &call = prune_call_;
        call.stats = CallStats{};
        if (!arena_ || !prepared_ || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        const bool every = n == 0 && !h_pairs;
        if (!every && carry_list(n, h_pairs) != 0) return MBAVO_E_ARG;
        if (o->level < -1 || o->level >= L || !flags01({o->apply, o->use_filter, o->check_depth})) return MBAVO_E_ARG;
        if (o->min_obs < 0 || o->rej_limit < 0 || o->min_keep < 0 || bad_limit(o->min_info)) return MBAVO_E_ARG;
        if (std::any_of(std::begin(o->reserved), std::end(o->reserved), [](int v) { return v != 0; })) return MBAVO_E_ARG;
        if ((o->drop_mask != 0u && !d_flags) || (o->use_filter == 1 && !filter_ready_)) return MBAVO_E_ARG;
        mbavo_pairs_prune_opts opt = *o;
        if (depth_limits(opt.z_min, opt.z_max) != 0) return MBAVO_E_ARG;
        const int np = every ? B : n, levels = o->level < 0 ? L : 1;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();

        // [records n x levels | B x L ints] move in ONE copy; the options and the list in one
        const size_t rec_bytes = sizeof(struct mbavo_pairs_prune) * (size_t)np * levels, cnt_bytes = sizeof(int) * (size_t)B * L;
        const size_t opt_bytes = sizeof(mbavo_pairs_prune_opts) + sizeof(int) * (size_t)B;
        if ((e = call.open(sizeof(struct mbavo_pairs_prune) * (size_t)B * L + cnt_bytes, 1, opt_bytes)) != hipSuccess) return (int)e;
        *(mbavo_pairs_prune_opts *)call.h_opts = opt;
        int *h_list = (int *)(call.h_opts + sizeof(opt));
        for (int i = 0; i < np; ++i) h_list[i] = every ? i : h_pairs[i];
        if ((e = call.upload(sizeof(opt) + sizeof(int) * (size_t)np)) != hipSuccess) return (int)e;

        PruneArgs a{};
        a.desc = lay_.desc(arena_); a.counts = lay_.counts(arena_);
        a.opts = (const mbavo_pairs_prune_opts *)call.d_opts; a.list = (const int *)(a.opts + 1);
        a.L = L; a.level = o->level; a.levels = levels;
        a.st_stride = slots_.outs(-1, a.st0);
        a.out_stride = slots_.outs(o->level, a.out0);
        if (filter_ready_)
        {
            const FilterArrays f = filter_arrays();
            a.mu = f.mu; a.info = f.info; a.n_obs = f.n_obs; a.n_rej = f.n_rej;
        }
        a.flags = d_flags; a.keep = d_keep;
        a.out = (struct mbavo_pairs_prune *)call.records; a.new_counts = (int *)(call.records + rec_bytes);
        hipLaunchKernelGGL(k_pairs_prune, dim3(np * levels), dim3(256), 0, st, a);
        call.stats.launches = 1;
        if (o->apply == 0) return call.finish(h_out, rec_bytes);

        // the ONE read-back: the host's K follows the device's counts, the serials say what the prune did to the keypoints
        const int rb = read_back(call.records, call.mirror, nullptr, rec_bytes + cnt_bytes, call.stats);
        if (rb != 0) return rb;
        if (h_out) memcpy(h_out, call.mirror, rec_bytes);
        const int *h_new = (const int *)(call.mirror + rec_bytes);
        for (int i = 0; i < np; ++i)
        {
            const int b = h_list[i];
            bool lost = false;
            for (int j = 0; j < levels; ++j)
            {
                const size_t at = (size_t)b * L + (o->level < 0 ? j : o->level);
                lost = lost || h_new[at] < probs_[at].K;
                h_counts_[at] = probs_[at].K = h_new[at];
            }
            if (!lost) continue;
            // (the indices of smoothing and hand-over are rebuilt at their next use; a filter state that was current stays so)
            const unsigned long long old = kp_serial_[b]++;
            for (int l = 0; l < L && !seeded_at_.empty(); ++l)
                if (seeded_at_[(size_t)b * L + l] == old) seeded_at_[(size_t)b * L + l] = kp_serial_[b];
        }
        return 0;
    }
} // namespace mbavo
