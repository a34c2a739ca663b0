// pairs_carry.hip -- a keyframe's keypoint depths and filter state handed to the pair's next keyframe (include/mbavo.h:
// mbavo_pairs_carry_save, mbavo_pairs_carry_adopt) without a depth map: the old keyframe's keypoints are warped once into a per-pair
// set of carried points, and after the update every new keypoint gathers from that set.
//
//   k_pairs_carry_warp     the save's first launch, on the smoothing's grid: workgroup g of the G of a (listed pair, level) takes
//                the keypoints [256 t, 256 t + 256) for t = g, g + G, ..; a lane per keypoint warps it into the new keyframe and
//                STAGES the outcome by source index -- its pixel (x < 0: not carried), rho' and w'.  The record's sums are closed
//                as the refinement's.  Nothing after this kernel evaluates the warp or its predicate again.
//   k_pairs_carry_index    the save's second launch: one workgroup per (listed pair, level), the counting sort of the staged pixels
//                into bins (pairs_bin_index.h: bin_index, the body k_pairs_smooth_index runs), members the staged entries with
//                x >= 0.  Count and scatter read the same staged word, so a place is below the count.
//   k_pairs_carry_adopt    the adopt's ONE launch, on the same grid: a lane per new keypoint walks the (up to) nine bins around it
//                for rho_max, then merges them by ascending source index -- nine cursors, each resting on its bin's next member
//                inside the window and in the foreground -- so that SW and SR are formed over ascending j.  The depth, the filter's
//                state and the caller's arrays are written by the keypoint's own lane; carried points are read from the save's
//                buffers alone.
#include "pairs_bin_index.h"
#include "pairs_depth_eval.h"

namespace mbavo
{
    namespace pairs
    {
        // the (listed pair, level) of a workgroup row
        struct CarrySlot
        {
            int b, l, K;
            size_t e;
            long long s0;
        };
        __device__ __forceinline__ CarrySlot carry_slot(const CarryArgs &a, int ent, const CarryPair &cp)
        {
            CarrySlot c;
            c.b = cp.pair; c.l = ent - (ent / a.L) * a.L;
            c.e = (size_t)c.b * a.L + c.l;
            c.K = a.counts[c.e];
            c.s0 = (long long)c.b * a.st_stride + a.st0[c.l];
            return c;
        }

        __global__ __launch_bounds__(256) void k_pairs_carry_warp(const CarryArgs a)
        {
#pragma clang fp contract(off)
            __shared__ double s_w[4];
            const int tid = threadIdx.x;
            const int ent = (int)blockIdx.y, grp = (int)blockIdx.x;
            const CarryPair &cp = a.list[ent / a.L];
            const CarrySlot c = carry_slot(a, ent, cp);
            const int G = a.groups[c.l];
            if (grp >= G) return; // (the grid's width is the widest level's)
            const PairLevelDesc &pd = a.desc[c.e];
            const mbavo_pairs_carry_save_opts o = *(const mbavo_pairs_carry_save_opts *)a.opts;
            const double sc = (double)(1 << c.l);
            const double *k0 = a.of_pair ? &a.of_pair[c.b].fx : a.intr;
            const double fx = k0[0] / sc, fy = k0[1] / sc, cx = k0[2] / sc, cy = k0[3] / sc;
            const double W = (double)pd.W, H = (double)pd.H;
            const double t0 = cp.t[0], t1 = cp.t[1], t2 = cp.t[2];
            const double R00 = cp.R[0], R01 = cp.R[1], R02 = cp.R[2], R10 = cp.R[3], R11 = cp.R[4], R12 = cp.R[5], R20 = cp.R[6], R21 = cp.R[7],
                         R22 = cp.R[8];
            const double2 *__restrict__ kp_xy = reinterpret_cast<const double2 *>(pd.kp_xy);
            const double *__restrict__ kp_z = pd.kp_z;

            double w_sum = 0.0;
            int n_valid = 0, n_carried = 0;
            for (int t = grp * 256; t < c.K; t += G * 256)
            {
                const int i = t + tid;
                if (i >= c.K) continue;
                const double D = kp_z[i];
                SmoothXY at{-1, -1};
                double rho_c = 0.0, w_c = 0.0;
                if (__builtin_isfinite(D) && D > 0.0)
                {
                    ++n_valid;
                    const double2 p = kp_xy[i];
                    const double rx = (p.x - cx) / fx, ry = (p.y - cy) / fy;
                    const double d0 = D * rx - t0, d1 = D * ry - t1, d2 = D - t2;
                    const double X = (R00 * d0 + R10 * d1) + R20 * d2;
                    const double Y = (R01 * d0 + R11 * d1) + R21 * d2;
                    const double Dn = (R02 * d0 + R12 * d1) + R22 * d2;
                    if (__builtin_isfinite(Dn) && Dn >= o.z_min && (o.z_max == 0.0 || Dn <= o.z_max))
                    {
                        const double u = fx * (X / Dn) + cx, v = fy * (Y / Dn) + cy;
                        const double xf = floor(u + 0.5), yf = floor(v + 0.5);
                        if (xf >= 0.0 && xf < W && yf >= 0.0 && yf < H)
                        {
                            const double cc = (R02 * rx + R12 * ry) + R22;
                            const double s = (cc * (D * D)) / (Dn * Dn);
                            const double w = o.weights == 1 ? a.info_in[c.s0 + i] : 1.0;
                            const double wn = (w / (s * s)) * o.deflate;
                            if (wn > 0.0 && __builtin_isfinite(wn))
                            {
                                at = SmoothXY{(int)xf, (int)yf};
                                rho_c = 1.0 / Dn;
                                w_c = wn;
                                ++n_carried;
                                w_sum = w_sum + wn;
                            }
                        }
                    }
                }
                a.sxy[c.s0 + i] = at;
                a.c_rho[c.s0 + i] = rho_c;
                a.c_w[c.s0 + i] = w_c;
            }
            const double mine[kCarrySaveSums] = {(double)n_valid, (double)n_carried, w_sum}; // (integers below 2^53: exact)
            double r[kCarrySaveSums];
            if (!close_record<kCarrySaveSums>(mine, s_w, a.partials, a.tickets, ent, grp, G, r)) return;
            struct mbavo_pairs_carry_save *out = (struct mbavo_pairs_carry_save *)a.out + ent;
            out->num_keypoints = c.K; out->num_valid = (int)r[0]; out->num_carried = (int)r[1]; out->reserved = 0;
            out->sum_w = r[2];
        }

        // the staged outcomes of a level's warp as the members of the index: the carried ones, at their pixel in the new keyframe
        struct CarriedPoints
        {
            static constexpr bool kEvery = false;
            const SmoothXY *__restrict__ sxy;
            __device__ __forceinline__ bool at(int i, int &x, int &y) const
            {
                const SmoothXY p = sxy[i];
                x = p.x; y = p.y;
                return p.x >= 0;
            }
        };

        __global__ __launch_bounds__(256) void k_pairs_carry_index(const CarryArgs a)
        {
            extern __shared__ int s_hist[]; // [kIndexWaves][nb]
            __shared__ int s_wave[4];
            const int ent = (int)blockIdx.x;
            const CarryPair &cp = a.list[ent / a.L];
            const CarrySlot c = carry_slot(a, ent, cp);
            const PairLevelDesc &pd = a.desc[c.e];
            const int s = bin_edge(cp.radius, pd.W, pd.H);
            const int nbx = (pd.W + s - 1) / s, nby = (pd.H + s - 1) / s; // nbx nby <= kSmoothBins
            const CarriedPoints members{a.sxy + c.s0};
            bin_index(members, c.K, s, nbx, nby, a.starts + c.e * kSmoothStarts, a.perm + c.s0, a.pxy + c.s0, s_hist, s_wave);
        }

        // one of the nine cursors of a keypoint's merge: p .. e of the carried set, h the source index it rests on
        struct CarryCursor
        {
            int p, e, h;
        };
        constexpr int kCarryNoHead = 0x7fffffff;

        // the cursor moves on to its bin's next member inside the window whose rho' is at least `floor_rho`
        __device__ __forceinline__ void carry_rest(CarryCursor &c, const int *__restrict__ perm, const SmoothXY *__restrict__ pxy,
                                                   const double *__restrict__ c_rho, int x, int y, int r, double floor_rho)
        {
            c.h = kCarryNoHead;
            while (c.p < c.e)
            {
                const SmoothXY q = pxy[c.p];
                const int dx = q.x - x, dy = q.y - y;
                if (dx >= -r && dx <= r && dy >= -r && dy <= r)
                {
                    const int j = perm[c.p];
                    if (c_rho[j] >= floor_rho)
                    {
                        c.h = j;
                        return;
                    }
                }
                ++c.p;
            }
        }

        __global__ __launch_bounds__(256) void k_pairs_carry_adopt(const CarryArgs a)
        {
#pragma clang fp contract(off)
            __shared__ double s_w[4];
            const int tid = threadIdx.x;
            const int ent = (int)blockIdx.y, grp = (int)blockIdx.x;
            const CarryPair &cp = a.list[ent / a.L];
            const CarrySlot c = carry_slot(a, ent, cp);
            const int G = a.groups[c.l];
            if (grp >= G) return; // (the grid's width is the widest level's)
            const PairLevelDesc &pd = a.desc[c.e];
            const mbavo_pairs_carry_adopt_opts o = *(const mbavo_pairs_carry_adopt_opts *)a.opts;
            const int r = cp.radius, s = bin_edge(r, pd.W, pd.H);
            const int nbx = (pd.W + s - 1) / s, nby = (pd.H + s - 1) / s;
            const double2 *__restrict__ kp_xy = reinterpret_cast<const double2 *>(pd.kp_xy);
            double *kp_z = pd.kp_z;
            const int *__restrict__ starts = a.starts + c.e * kSmoothStarts;
            const int *__restrict__ perm = a.perm + c.s0;
            const SmoothXY *__restrict__ pxy = a.pxy + c.s0;
            const double *__restrict__ c_rho = a.c_rho + c.s0, *__restrict__ c_w = a.c_w + c.s0;

            double info_sum = 0.0, rel_sum = 0.0;
            int n_adopted = 0, n_empty = 0;
            for (int t = grp * 256; t < c.K; t += G * 256)
            {
                const int i = t + tid;
                if (i >= c.K) continue;
                const double2 p = kp_xy[i];
                const int x = (int)p.x, y = (int)p.y;
                const double Di = kp_z[i];
                int bx = x / s, by = y / s;
                bx = bx < 0 ? 0 : (bx >= nbx ? nbx - 1 : bx);
                by = by < 0 ? 0 : (by >= nby ? nby - 1 : by);
                // ---- rho_max over the window (a maximum: any order)
                int p0[9], p1[9], nN = 0;
                double rho_max = 0.0; // (a carried rho' is > 0)
#pragma unroll
                for (int q = 0; q < 9; ++q)
                {
                    const int bcx = bx + q % 3 - 1, bcy = by + q / 3 - 1;
                    p0[q] = p1[q] = 0;
                    if (bcx >= 0 && bcx < nbx && bcy >= 0 && bcy < nby)
                    {
                        p0[q] = starts[bcy * nbx + bcx];
                        p1[q] = starts[bcy * nbx + bcx + 1];
                    }
                    for (int at = p0[q]; at < p1[q]; ++at)
                    {
                        const SmoothXY m = pxy[at];
                        const int dx = m.x - x, dy = m.y - y;
                        if (dx >= -r && dx <= r && dy >= -r && dy <= r)
                        {
                            const double rj = c_rho[perm[at]];
                            ++nN;
                            rho_max = rj > rho_max ? rj : rho_max;
                        }
                    }
                }
                // ---- the foreground's sums over ascending source index
                int nC = 0, flag = 0;
                double SW = 0.0, SR = 0.0, rho_n = __builtin_nan(""), D_n = __builtin_nan("");
                if (nN > 0)
                {
                    const double floor_rho = (1.0 - o.max_rel_diff) * rho_max;
                    CarryCursor cur[9];
#pragma unroll
                    for (int q = 0; q < 9; ++q)
                    {
                        cur[q].p = p0[q]; cur[q].e = p1[q];
                        carry_rest(cur[q], perm, pxy, c_rho, x, y, r, floor_rho);
                    }
                    for (;;)
                    {
                        int j = cur[0].h;
#pragma unroll
                        for (int q = 1; q < 9; ++q) j = cur[q].h < j ? cur[q].h : j;
                        if (j == kCarryNoHead) break;
#pragma unroll
                        for (int q = 0; q < 9; ++q)
                            if (cur[q].h == j) // (a carried point is in one bin: one cursor)
                            {
                                ++cur[q].p;
                                carry_rest(cur[q], perm, pxy, c_rho, x, y, r, floor_rho);
                            }
                        const double wj = c_w[j], wr = wj * c_rho[j];
                        ++nC;
                        SW = SW + wj;
                        SR = SR + wr;
                    }
                    flag = 2;
                    if (nC >= o.min_support)
                    {
                        rho_n = SR / SW;
                        D_n = 1.0 / rho_n;
                        flag = __builtin_isfinite(D_n) && D_n >= o.z_min && (o.z_max == 0.0 || D_n <= o.z_max) ? 1 : 3;
                    }
                }
                const bool adopted = flag == 1;
                if (adopted)
                {
                    ++n_adopted;
                    info_sum = info_sum + SW;
                    if (__builtin_isfinite(Di) && Di > 0.0)
                    {
                        const double rho_i = 1.0 / Di, rel = (rho_n - rho_i) / rho_i;
                        rel_sum = rel_sum + rel * rel;
                    }
                }
                n_empty += flag == 0;
                const long long si = c.s0 + i;
                if (a.rho) a.rho[si] = adopted ? rho_n : __builtin_nan("");
                if (a.info_out) a.info_out[si] = adopted ? SW : 0.0;
                if (a.count) a.count[si] = nC;
                if (a.flags) a.flags[si] = (unsigned char)flag;
                if (o.apply == 1 && adopted) kp_z[i] = D_n;
                if (o.seed_filter == 1)
                {
                    double mu, info;
                    if (adopted)
                    {
                        mu = rho_n;
                        info = (o.max_info == 0.0 || SW <= o.max_info) ? SW : o.max_info;
                    }
                    else
                    {
                        mu = 1.0 / Di;
                        info = o.prior_rel_sigma == 0.0 ? 0.0 : 1.0 / ((o.prior_rel_sigma * mu) * (o.prior_rel_sigma * mu));
                    }
                    a.mu[si] = mu; a.info[si] = info;
                    a.n_obs[si] = 0; a.n_rej[si] = 0;
                }
            }
            const double mine[kCarryAdoptSums] = {(double)n_adopted, (double)n_empty, info_sum, rel_sum}; // (integers below 2^53: exact)
            double rs[kCarryAdoptSums];
            if (!close_record<kCarryAdoptSums>(mine, s_w, a.partials, a.tickets, ent, grp, G, rs)) return;
            struct mbavo_pairs_carry_adopt *out = (struct mbavo_pairs_carry_adopt *)a.out + ent;
            out->num_keypoints = c.K; out->num_adopted = (int)rs[0]; out->num_empty = (int)rs[1]; out->reserved = 0;
            out->sum_info = rs[2]; out->sum_sq_rel = rs[3];
        }
    } // namespace pairs

    using namespace pairs;

    int PairBatch::carry_list(int n, const int *h_pairs) const
    {
        if (!arena_ || !prepared_ || !h_pairs || n < 1 || n > plan_.B) return MBAVO_E_ARG;
        for (int i = 0; i < n; ++i)
            if (h_pairs[i] < 0 || h_pairs[i] >= plan_.B || (i > 0 && h_pairs[i] <= h_pairs[i - 1])) return MBAVO_E_ARG;
        return 0;
    }

    int PairBatch::carry_args(CarryArgs &a, size_t opts_size)
    {
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        a = CarryArgs{};
        a.desc = lay_.desc(arena_); a.counts = lay_.counts(arena_);
        a.of_pair = opts_.num_cameras > 0 ? lay_.pair_cameras(arena_) : nullptr;
        for (int i = 0; i < 4; ++i) a.intr[i] = opts_.intrinsics[i];
        a.L = L;
        for (int l = 0; l < L; ++l) a.groups[l] = slots_.groups256[l];
        a.st_stride = slots_.outs(-1, a.st0);
        const size_t n_slots = slots_.n_slots;
        // the first carry call: the carried sets (include/mbavo.h)
        const IndexLayout ix = index_layout(p, n_slots);
        const long long o_rho = ix.o_tail + align_up((long long)sizeof(SmoothXY) * (long long)n_slots, kAlign);
        if (!carry_set_)
        {
            if ((e = carry_set_.alloc((size_t)o_rho + 2 * sizeof(double) * n_slots + 16)) != hipSuccess) return (int)e;
            armed_.assign((size_t)B, 0);
        }
        a.starts = ix.starts(carry_set_); a.perm = ix.perm(carry_set_); a.pxy = ix.pxy(carry_set_);
        a.sxy = (SmoothXY *)(carry_set_.p + ix.o_tail); a.c_rho = (double *)(carry_set_.p + o_rho); a.c_w = a.c_rho + n_slots;
        if (filter_ready_)
        {
            const FilterArrays f = filter_arrays();
            a.mu = f.mu; a.info = f.info; a.n_obs = f.n_obs; a.n_rej = f.n_rej;
            a.info_in = a.info;
        }
        // (both calls share one scratch: the larger record, the larger options, four sums)
        const size_t rec_bytes_max = sizeof(struct mbavo_pairs_carry_adopt) * (size_t)B * L;
        const size_t opt_bytes_max = sizeof(mbavo_pairs_carry_adopt_opts) + sizeof(CarryPair) * (size_t)B;
        if ((e = carry_call_.open(rec_bytes_max, kCarryAdoptSums, opt_bytes_max)) != hipSuccess) return (int)e;
        const DepthCall &c = carry_call_;
        a.opts = c.d_opts; a.list = (const CarryPair *)(c.d_opts + opts_size);
        a.partials = c.partials; a.tickets = c.tickets; a.out = c.records;
        return 0;
    }

    int PairBatch::carry_save(int n, const int *h_pairs, const double *h_T, const mbavo_pairs_carry_save_opts *o, struct mbavo_pairs_carry_save *h_out)
    {
        csv_stats_ = CallStats{};
        if (!o || !h_T || carry_list(n, h_pairs) != 0) return MBAVO_E_ARG;
        const int L = plan_.L;
        for (int i = 0; i < n; ++i)
        {
            const double *T = h_T + 7 * i;
            for (int j = 0; j < 7; ++j)
                if (!std::isfinite(T[j])) return MBAVO_E_ARG;
            const double qq = T[3] * T[3] + T[4] * T[4] + T[5] * T[5] + T[6] * T[6];
            if (!(qq >= 1.0 - 1e-9 && qq <= 1.0 + 1e-9)) return MBAVO_E_ARG;
        }
        if (o->radius < 1 || o->radius > 16 || !(o->deflate > 0.0 && o->deflate <= 1.0)) return MBAVO_E_ARG;
        if (!flags01({o->weights}) || (o->weights == 1 && !filter_ready_)) return MBAVO_E_ARG;
        mbavo_pairs_carry_save_opts opt = *o;
        if (depth_limits(opt.z_min, opt.z_max) != 0) return MBAVO_E_ARG;

        CarryArgs a;
        const int rc = carry_args(a, sizeof(opt));
        if (rc != 0) return rc;
        hipStream_t st = eng_.stream();
        char *h_opts = carry_call_.h_opts;
        *(mbavo_pairs_carry_save_opts *)h_opts = opt;
        CarryPair *h_list = (CarryPair *)(h_opts + sizeof(opt));
        for (int i = 0; i < n; ++i)
        {
            const double *T = h_T + 7 * i;
            h_list[i].pair = h_pairs[i]; h_list[i].radius = o->radius;
            for (int j = 0; j < 3; ++j) h_list[i].t[j] = T[j];
            rotation_entries(T + 3, h_list[i].R);
        }
        hipError_t e;
        if ((e = carry_call_.upload(sizeof(opt) + sizeof(CarryPair) * (size_t)n)) != hipSuccess) return (int)e;
        const size_t lds = index_lds(plan_, o->radius, -1);
        if ((e = eng_.ensure_lds((const void *)k_pairs_carry_index, lds)) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_pairs_carry_warp, dim3(DepthSlots::width(-1, a.groups), n * L), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_pairs_carry_index, dim3(n * L), dim3(256), lds, st, a);
        csv_stats_.launches = 2;
        for (int i = 0; i < n; ++i) armed_[h_pairs[i]] = o->radius;
        return carry_call_.finish(h_out, sizeof(struct mbavo_pairs_carry_save) * (size_t)n * L, &csv_stats_);
    }

    int PairBatch::carry_adopt(int n, const int *h_pairs, const mbavo_pairs_carry_adopt_opts *o, struct mbavo_pairs_carry_adopt *h_out, double *d_rho,
                               double *d_info, int *d_count, unsigned char *d_flags)
    {
        cad_stats_ = CallStats{};
        if (!o || carry_list(n, h_pairs) != 0) return MBAVO_E_ARG;
        const int L = plan_.L;
        if (!flags01({o->apply, o->seed_filter})) return MBAVO_E_ARG;
        if (o->seed_filter == 1 && (o->apply == 0 || !filter_ready_)) return MBAVO_E_ARG;
        if (o->min_support < 1 || !(o->max_rel_diff > 0.0 && o->max_rel_diff <= 1.0)) return MBAVO_E_ARG;
        if (bad_limit(o->prior_rel_sigma) || bad_limit(o->max_info)) return MBAVO_E_ARG;
        mbavo_pairs_carry_adopt_opts opt = *o;
        if (depth_limits(opt.z_min, opt.z_max) != 0) return MBAVO_E_ARG;
        if (armed_.empty()) return MBAVO_E_ARG;
        for (int i = 0; i < n; ++i)
            if (armed_[h_pairs[i]] == 0) return MBAVO_E_ARG;

        CarryArgs a;
        const int rc = carry_args(a, sizeof(opt));
        if (rc != 0) return rc;
        hipStream_t st = eng_.stream();
        char *h_opts = carry_call_.h_opts;
        *(mbavo_pairs_carry_adopt_opts *)h_opts = opt;
        CarryPair *h_list = (CarryPair *)(h_opts + sizeof(opt));
        for (int i = 0; i < n; ++i)
        {
            h_list[i] = CarryPair{};
            h_list[i].pair = h_pairs[i]; h_list[i].radius = armed_[h_pairs[i]];
        }
        hipError_t e;
        if ((e = carry_call_.upload(sizeof(opt) + sizeof(CarryPair) * (size_t)n)) != hipSuccess) return (int)e;
        a.rho = d_rho; a.info_out = d_info; a.count = d_count; a.flags = d_flags;
        hipLaunchKernelGGL(k_pairs_carry_adopt, dim3(DepthSlots::width(-1, a.groups), n * L), dim3(256), 0, st, a);
        cad_stats_.launches = 1;
        for (int i = 0; i < n; ++i)
        {
            armed_[h_pairs[i]] = 0;
            if (o->seed_filter == 1)
                for (int l = 0; l < L; ++l) seeded_at_[(size_t)h_pairs[i] * L + l] = kp_serial_[h_pairs[i]];
        }
        return carry_call_.finish(h_out, sizeof(struct mbavo_pairs_carry_adopt) * (size_t)n * L, &cad_stats_);
    }
} // namespace mbavo
