// pairs_smooth.hip -- every keypoint's inverse depth smoothed over its image neighbours (include/mbavo.h: mbavo_pairs_smooth_depths):
// a weighted mean over itself and the neighbours that agree with it, a fill from all neighbours where none agrees, a flag where
// neither can be done.  No pose is read.  At most TWO launches:
//
//   k_pairs_smooth_index   one workgroup per reported (pair, level) whose index is stale (a word per pair behind the options says
//                so; the others leave at once): a counting sort of the level's keypoints into bins of edge s, members ascending
//                within a bin (pairs_bin_index.h: bin_index, the body pairs_carry.hip's index shares).
//   k_pairs_smooth         the refinement's grid without its tiles' items: workgroup g of the G of a (pair, level) takes the
//                keypoints [256 t, 256 t + 256) for t = g, g + G, ..; a lane per keypoint merges the (up to) nine bins around it by
//                ascending keypoint index -- nine cursors, each resting on its bin's next member inside the window -- so that the
//                sums of step 3 are formed over ascending j.  New depths (and the filter's mu) go to a staging array; the
//                workgroup that takes the LAST ticket of the (pair, level) -- every read of an old depth is behind it then --
//                writes them into the object: a Jacobi sweep across workgroups.  The record's sums are closed as the refinement's (close_record).
#include "pairs_bin_index.h"
#include "pairs_depth_eval.h"

namespace mbavo
{
    namespace pairs
    {
        // the level's keypoints as the members of the index: every one of them, at the whole pixel the object stores
        struct SmoothKeypoints
        {
            static constexpr bool kEvery = true;
            const double2 *__restrict__ kp_xy;
            __device__ __forceinline__ bool at(int i, int &x, int &y) const
            {
                const double2 p = kp_xy[i];
                x = (int)p.x; y = (int)p.y;
                return true;
            }
        };

        __global__ __launch_bounds__(256) void k_pairs_smooth_index(const SmoothArgs a)
        {
            extern __shared__ int s_hist[]; // [kIndexWaves][nb]
            __shared__ int s_wave[4];
            const int ent = (int)blockIdx.x;
            const int b = ent / a.levels, li = ent - b * a.levels, l = a.level < 0 ? li : a.level;
            if (((a.rebuild[b] >> l) & 1) == 0) return;
            const size_t e = (size_t)b * a.L + l;
            const PairLevelDesc &pd = a.desc[e];
            const int K = a.counts[e], s = a.blob->s[l];
            const int nbx = (pd.W + s - 1) / s, nby = (pd.H + s - 1) / s; // nbx nby <= kSmoothBins (the host chose s so)
            const long long s0 = (long long)b * a.st_stride + a.st0[l];
            const SmoothKeypoints members{reinterpret_cast<const double2 *>(pd.kp_xy)};
            bin_index(members, K, s, nbx, nby, a.starts + e * kSmoothStarts, a.perm + s0, a.pxy + s0, s_hist, s_wave);
        }

        // one of the nine cursors of a keypoint's merge: p .. e of the permutation, h the keypoint index it rests on
        struct SmoothCursor
        {
            int p, e, h;
        };
        constexpr int kNoHead = 0x7fffffff;

        // the cursor moves on to its bin's next member inside the window that is not the keypoint itself
        __device__ __forceinline__ void smooth_rest(SmoothCursor &c, const int *__restrict__ perm, const SmoothXY *__restrict__ pxy, int i, int x, int y,
                                                    int r)
        {
            c.h = kNoHead;
            while (c.p < c.e)
            {
                const SmoothXY q = pxy[c.p];
                const int dx = q.x - x, dy = q.y - y;
                if (dx >= -r && dx <= r && dy >= -r && dy <= r)
                {
                    const int j = perm[c.p];
                    if (j != i)
                    {
                        c.h = j;
                        return;
                    }
                }
                ++c.p;
            }
        }

        __device__ __forceinline__ double smooth_weight(const SmoothArgs &a, int weights, long long si, long long oi)
        {
            if (weights == 0) return 1.0;
            const double w = weights == 1 ? a.info[si] : a.weight[oi];
            return w > 0.0 ? w : 0.0; // (NaN: 0)
        }

        __global__ __launch_bounds__(256) void k_pairs_smooth(const SmoothArgs a)
        {
#pragma clang fp contract(off)
            __shared__ double s_w[4];
            __shared__ int s_last;
            const int tid = threadIdx.x;
            const int ent = (int)blockIdx.y, grp = (int)blockIdx.x;
            const int b = ent / a.levels, li = ent - b * a.levels, l = a.level < 0 ? li : a.level;
            const int G = a.groups[l];
            if (grp >= G) return; // (the grid's width is the widest level's)
            const size_t e = (size_t)b * a.L + l;
            const PairLevelDesc &pd = a.desc[e];
            const mbavo_pairs_smooth_opts o = a.blob->o;
            const int K = a.counts[e], s = a.blob->s[l], r = o.radius, W = pd.W;
            const int nbx = (W + s - 1) / s, nby = (pd.H + s - 1) / s;
            const double2 *__restrict__ kp_xy = reinterpret_cast<const double2 *>(pd.kp_xy);
            double *kp_z = pd.kp_z;
            const unsigned char *__restrict__ img = pd.ref;
            const int *__restrict__ starts = a.starts + e * kSmoothStarts;
            const long long s0 = (long long)b * a.st_stride + a.st0[l], o0 = (long long)b * a.out_stride + a.out0[l];
            const int *__restrict__ perm = a.perm + s0;
            const SmoothXY *__restrict__ pxy = a.pxy + s0;

            double rel_sum = 0.0, n_support = 0.0; // (integers below 2^53: exact)
            int n_valid = 0, n_supported = 0, n_filled = 0, n_outliers = 0, n_moved = 0;
            for (int t0 = grp * 256; t0 < K; t0 += G * 256)
            {
                const int i = t0 + tid;
                if (i >= K) continue;
                const double Di = kp_z[i];
                const bool valid = __builtin_isfinite(Di) && Di > 0.0;
                double rho_bar = __builtin_nan(""), D_new = __builtin_nan(""), mu_new = __builtin_nan("");
                int cls = 0, nC = 0;
                if (valid)
                {
                    const double2 p = kp_xy[i];
                    const int x = (int)p.x, y = (int)p.y;
                    const int Ii = img[(long long)y * W + x];
                    const double rho_i = 1.0 / Di, wi = smooth_weight(a, o.weights, s0 + i, o0 + i);
                    const double tol = o.max_rel_diff * rho_i;
                    int bx = x / s, by = y / s;
                    bx = bx < 0 ? 0 : (bx >= nbx ? nbx - 1 : bx);
                    by = by < 0 ? 0 : (by >= nby ? nby - 1 : by);
                    SmoothCursor cur[9];
#pragma unroll
                    for (int q = 0; q < 9; ++q)
                    {
                        const int cx = bx + q % 3 - 1, cy = by + q / 3 - 1;
                        cur[q].p = cur[q].e = 0;
                        if (cx >= 0 && cx < nbx && cy >= 0 && cy < nby)
                        {
                            cur[q].p = starts[cy * nbx + cx];
                            cur[q].e = starts[cy * nbx + cx + 1];
                        }
                        smooth_rest(cur[q], perm, pxy, i, x, y, r);
                    }
                    double SWC = 0.0, SRC = 0.0, SWN = 0.0, SRN = 0.0;
                    int nN = 0;
                    for (;;)
                    {
                        int j = cur[0].h;
#pragma unroll
                        for (int q = 1; q < 9; ++q) j = cur[q].h < j ? cur[q].h : j;
                        if (j == kNoHead) break;
#pragma unroll
                        for (int q = 0; q < 9; ++q)
                            if (cur[q].h == j) // (a keypoint is in one bin: one cursor)
                            {
                                ++cur[q].p;
                                smooth_rest(cur[q], perm, pxy, i, x, y, r);
                            }
                        const double Dj = kp_z[j];
                        if (!(__builtin_isfinite(Dj) && Dj > 0.0)) continue;
                        const double wj = smooth_weight(a, o.weights, s0 + j, o0 + j);
                        if (!(wj > 0.0)) continue;
                        if (o.max_intensity_diff != 0)
                        {
                            const double2 pj = kp_xy[j];
                            const int Ij = img[(long long)(int)pj.y * W + (int)pj.x];
                            const int d = Ij - Ii;
                            if ((d < 0 ? -d : d) > o.max_intensity_diff) continue;
                        }
                        const double rho_j = 1.0 / Dj, wr = wj * rho_j;
                        ++nN;
                        SWN = SWN + wj;
                        SRN = SRN + wr;
                        if (fabs(rho_j - rho_i) <= tol)
                        {
                            ++nC;
                            SWC = SWC + wj;
                            SRC = SRC + wr;
                        }
                    }
                    bool proposed = true;
                    if (nC >= o.min_support)
                    {
                        cls = 1;
                        rho_bar = (wi * rho_i + o.strength * SRC) / (wi + o.strength * SWC);
                    }
                    else if (o.fill == 1 && nN >= o.min_support)
                    {
                        cls = 2;
                        rho_bar = SRN / SWN;
                    }
                    else
                    {
                        cls = 3;
                        proposed = false;
                    }
                    bool stands = false;
                    if (proposed)
                    {
                        D_new = 1.0 / rho_bar;
                        stands = __builtin_isfinite(D_new) && D_new >= o.z_min && (o.z_max == 0.0 || D_new <= o.z_max);
                    }
                    if (!stands)
                    {
                        rho_bar = rho_i;
                        D_new = __builtin_nan("");
                    }
                    const bool moved = stands && rho_bar != rho_i;
                    if (moved) mu_new = rho_bar;
                    const double rel = (rho_bar - rho_i) / rho_i;
                    rel_sum = rel_sum + rel * rel;
                    ++n_valid;
                    n_supported += cls == 1; n_filled += cls == 2; n_outliers += cls == 3; n_moved += moved;
                    n_support = n_support + (double)nC;
                }
                if (a.rho) a.rho[o0 + i] = rho_bar;
                if (a.flags) a.flags[o0 + i] = (unsigned char)cls;
                if (a.support) a.support[o0 + i] = nC;
                if (o.apply == 1)
                {
                    a.stage_D[s0 + i] = D_new;
                    if (o.sync_filter == 1) a.stage_rho[s0 + i] = mu_new;
                }
            }
            // ---- the record, and behind the last ticket the staged values into the object
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // (this lane's staged values, before the workgroup's ticket)
            const double mine[kSmoothSums] = {(double)n_valid, (double)n_supported, (double)n_filled, (double)n_outliers, (double)n_moved, n_support, rel_sum};
            double rs[kSmoothSums];
            const bool last = close_record<kSmoothSums>(mine, s_w, a.partials, a.tickets, ent, grp, G, rs);
            if (tid == 0)
            {
                if (last)
                {
                    struct mbavo_pairs_smooth *out = a.out + ent;
                    out->num_keypoints = K; out->num_valid = (int)rs[0]; out->num_supported = (int)rs[1]; out->num_filled = (int)rs[2];
                    out->num_outliers = (int)rs[3]; out->num_moved = (int)rs[4]; out->sum_support = (long long)rs[5]; out->sum_sq_rel = rs[6];
                }
                s_last = last ? 1 : 0;
            }
            __syncthreads();
            if (s_last == 0 || o.apply != 1) return;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            for (int i = tid; i < K; i += 256)
            {
                const double D = __hip_atomic_load(a.stage_D + s0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (D == D) kp_z[i] = D;
                if (o.sync_filter == 1)
                {
                    const double m = __hip_atomic_load(a.stage_rho + s0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (m == m) a.mu[s0 + i] = m;
                }
            }
        }
    } // namespace pairs

    using namespace pairs;

    int PairBatch::smooth_depths(const mbavo_pairs_smooth_opts *o, struct mbavo_pairs_smooth *h_out, const double *d_weight, double *d_rho,
                                 unsigned char *d_flags, int *d_support)
    {
        DepthCall &call = smooth_call_;
        call.stats = CallStats{};
        if (!arena_ || !prepared_ || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        if (o->level < -1 || o->level >= L || !flags01({o->apply, o->fill, o->sync_filter})) return MBAVO_E_ARG;
        if (o->weights < 0 || o->weights > 2 || ((o->weights == 1 || o->sync_filter == 1) && !filter_ready_)) return MBAVO_E_ARG;
        if ((o->weights == 2 && !d_weight) || (o->sync_filter == 1 && o->apply == 0)) return MBAVO_E_ARG;
        if (o->radius < 1 || o->radius > 16 || o->min_support < 1 || o->max_intensity_diff < 0 || o->max_intensity_diff > 255) return MBAVO_E_ARG;
        for (double v : {o->max_rel_diff, o->strength})
            if (!(v > 0.0 && v <= 1.0)) return MBAVO_E_ARG;
        mbavo_pairs_smooth_opts opt = *o;
        if (depth_limits(opt.z_min, opt.z_max) != 0) return MBAVO_E_ARG;
        const int levels = o->level < 0 ? L : 1;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();

        SmoothArgs a{};
        a.desc = lay_.desc(arena_); a.counts = lay_.counts(arena_);
        a.L = L; a.level = o->level; a.levels = levels;
        for (int l = 0; l < L; ++l) a.groups[l] = slots_.groups256[l];
        a.st_stride = slots_.outs(-1, a.st0);
        a.out_stride = slots_.outs(o->level, a.out0);
        const size_t n_slots = slots_.n_slots;
        // the first call: the index and the staging (include/mbavo.h)
        const IndexLayout ix = index_layout(p, n_slots);
        if (!smooth_index_)
        {
            if ((e = smooth_index_.alloc((size_t)ix.o_tail + 2 * sizeof(double) * n_slots + 16)) != hipSuccess) return (int)e;
            index_serial_.assign((size_t)B * L, 0);
            index_s_.assign((size_t)B * L, 0);
        }
        const size_t rec = sizeof(struct mbavo_pairs_smooth) * (size_t)B;
        const size_t opt_bytes = sizeof(SmoothBlob) + sizeof(int) * (size_t)B; // the options, the bin edges and the B words: ONE copy
        if ((e = call.open(rec * L, kSmoothSums, opt_bytes)) != hipSuccess) return (int)e;
        SmoothBlob *h_blob = (SmoothBlob *)call.h_opts;
        int *h_rebuild = (int *)(h_blob + 1);
        h_blob->o = opt;
        for (int l = 0; l < 8; ++l) h_blob->s[l] = l < L ? bin_edge(o->radius, p.W[l], p.H[l]) : 0;
        bool any = false;
        for (int b = 0; b < B; ++b)
        { // bit l: level l of pair b is reported and its index was built from other keypoints or with another bin edge
            int word = 0;
            for (int i = 0; i < levels; ++i)
            {
                const int l = o->level < 0 ? i : o->level;
                const size_t at = (size_t)b * L + l;
                if (index_serial_[at] != kp_serial_[b] || index_s_[at] != h_blob->s[l]) word |= 1 << l;
            }
            h_rebuild[b] = word;
            any = any || word != 0;
        }
        if ((e = call.upload(opt_bytes)) != hipSuccess) return (int)e;
        a.blob = (const SmoothBlob *)call.d_opts; a.rebuild = (const int *)(a.blob + 1);
        a.starts = ix.starts(smooth_index_); a.perm = ix.perm(smooth_index_); a.pxy = ix.pxy(smooth_index_);
        a.stage_D = (double *)(smooth_index_.p + ix.o_tail); a.stage_rho = a.stage_D + n_slots;
        if (filter_ready_)
        {
            const FilterArrays f = filter_arrays();
            a.mu = f.mu; a.info = f.info;
        }
        a.weight = d_weight; a.rho = d_rho; a.flags = d_flags; a.support = d_support;
        a.partials = call.partials; a.tickets = call.tickets;
        a.out = (struct mbavo_pairs_smooth *)call.records;
        if (any)
        {
            const size_t lds = index_lds(p, o->radius, o->level);
            if ((e = eng_.ensure_lds((const void *)k_pairs_smooth_index, lds)) != hipSuccess) return (int)e;
            hipLaunchKernelGGL(k_pairs_smooth_index, dim3(B * levels), dim3(256), lds, st, a);
            ++call.stats.launches;
            for (int b = 0; b < B; ++b)
                for (int l = 0; l < L; ++l)
                    if ((h_rebuild[b] >> l) & 1)
                    {
                        index_serial_[(size_t)b * L + l] = kp_serial_[b];
                        index_s_[(size_t)b * L + l] = h_blob->s[l];
                    }
        }
        hipLaunchKernelGGL(k_pairs_smooth, dim3(DepthSlots::width(o->level, a.groups), B * levels), dim3(256), 0, st, a);
        ++call.stats.launches;
        return call.finish(h_out, rec * levels);
    }
} // namespace mbavo
